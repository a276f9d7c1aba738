"""The fixtures of the mate search tests (tests/test_cpu_mate_model.py, tests/test_gpu_mate_search.py, tests/test_gpu_mate_frontends.py):
tests/golden/mate_cases.json, found by tests/golden/make_mate_cases.py. A fixture is a placement, the side to move, the halfmove clock
and an optional move history (UCI) played from the placement; the root searched is the position after the history. ``budgets``: the
node budgets (besides the large one) the fixture is to be searched with. No expected number is stored: the tests take them from
tests/mate_model.py, and tests/test_cpu_mate_model.py checks that the set still holds what each category needs."""
from __future__ import annotations

import json
import os

import numpy as np

from golden_cases import _place

MATE_IN_TWO = _place({"d0": 7, "i7": 3, "g7": 1, "e9": 15})     # tests/solver_cases.py "mate_in_two": i7i8, Kf9 forced, i8i9
BIG = 16384                                                      # the large budget: every fixture finishes below it at 15 plies or is state 3 there too
PLIES = (1, 3, 7, 15)
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mate_cases.json")


def load():
    with open(_PATH) as f:
        return json.load(f)


def squares(fx) -> np.ndarray:
    return _place(fx["placement"])


def move_id(uci: str) -> int:
    from oracle import lib
    return int(lib().xq_move_id((ord(uci[0]) - 97) + 9 * int(uci[1]), (ord(uci[2]) - 97) + 9 * int(uci[3])))


def uci(move: int) -> str:
    from oracle import lib
    return lib().xq_move_uci(int(move)).decode()


def board(fx, history: bool = True, halfmove=None):
    """The root of a fixture as an OracleBoard that carries its history."""
    from oracle import OracleBoard
    o = OracleBoard.from_array(squares(fx), fx["turn"], fx["halfmove"] if halfmove is None else halfmove)
    for mv in fx["history"]:
        o.push(mv)
    if not history:
        o = OracleBoard.from_array(o.squares(), int(o.turn), o.halfmove)
    return o


def checkers(after, king_side: int) -> set:
    """The squares of the pieces that attack the king of ``king_side`` on the position ``after`` (that side to move): the from-squares
    of the other side's legal moves onto the king's square, were it to move. A pinned checker is missed; the tags only ever need one
    example."""
    from oracle import OracleBoard, lib
    L = lib()
    sq = after.squares()
    ksq = int(np.flatnonzero(sq == (7 if king_side else 15))[0])
    other = OracleBoard.from_array(sq, king_side ^ 1)
    return {int(L.xq_move_from(i)) for i in other.legal_ids() if L.xq_move_to(i) == ksq}


def tags_of(root, state: int, dist: int, move: int) -> set:
    """What a state-1 fixture shows besides its distance: ``discovered`` / ``double`` (a one-ply mate whose moved piece is not among
    the checkers / with two checkers), ``late`` (the mating move's index in the root's list is >= 64), ``capture`` (dist >= 3: the
    defender's only reply to the first move captures the piece that moved)."""
    from oracle import lib
    L = lib()
    tags = set()
    if state != 1:
        return tags
    ids = root.legal_ids()
    if ids.index(move) >= 64:
        tags.add("late")
    a = root.copy()
    a.push_id(move)
    if dist == 1:
        ch = checkers(a, int(a.turn))
        if ch and int(L.xq_move_to(move)) not in ch:
            tags.add("discovered")
        if len(ch) >= 2:
            tags.add("double")
    else:
        rep = a.legal_ids()
        if len(rep) == 1 and L.xq_move_to(rep[0]) == L.xq_move_to(move):
            tags.add("capture")
    return tags
