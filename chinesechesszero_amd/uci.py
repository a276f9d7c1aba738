"""UCI-style stdin/stdout front-end on the single-board path.

The reference's README (README.md:3) advertises "standard UCI protocol" but ships no loop; what it does
use everywhere are UCI coordinate strings ("a0a1", tools.py:172-269). This is that missing loop:
``uci``, ``isready``, ``ucinewgame``, ``position startpos|fen <fen> [moves ...]``, ``go [nodes N]``,
``setoption name Playouts|MultiPV value N``, ``setoption name Solver value true|false`` (MCTS-solver: ``score mate N``), ``setoption name LCB value true|false`` (``bestmove`` is the
lower-confidence-bound move; ``LCBStdevs`` / ``LCBMinVisitRatio``: its numbers; the ``info`` lines stay as they are),
``setoption name MateSearch value PLIES`` / ``MateNodes value N`` (before the search, look for a forced mate by consecutive checks --
``ccz_mate_search``, no evaluator call --: ``info depth D score mate N nodes <nodes> pv <move>`` and ``bestmove``; 0 = off), ``go mate N``
(that search at 2N - 1 plies for this one command, falling back to the normal search), ``d``, ``quit``. ``go`` reports one ``info depth .. multipv .. score cp .. nodes .. pv ..``
line per principal variation (``SelfPlayEngine.principal_variations``); ``cp`` is a display mapping of the first move's Q
(``analyse.cp_of``). The search is ``MCTS_AI`` on the HIP engine (no CPU fallback).
"""
from __future__ import annotations

import sys

import numpy as np

from .game import RED, Board, Move, _SYMBOL
from .options import MATE_MAX_NODES, MATE_MAX_PLIES, MATE_NODES, SearchOptions
from .parameters import C_PUCT, PLAYOUT

ENGINE_NAME = "cczero-mi355x"


def board_from_fen(fen: str) -> Board:
    parts = fen.split()
    if not parts:
        raise ValueError("empty FEN")
    rows = parts[0].split("/")
    if len(rows) != 10:
        raise ValueError("FEN needs 10 ranks")
    sq = np.zeros(90, np.uint8)
    for i, row in enumerate(rows):
        r, f = 9 - i, 0
        for ch in row:
            if ch.isdigit():
                f += int(ch)
            else:
                if ch.lower() not in _SYMBOL or f > 8:
                    raise ValueError(f"bad FEN row {row!r}")
                sq[f + 9 * r] = _SYMBOL[ch.lower()] + (0 if ch.isupper() else 8)
                f += 1
        if f != 9:
            raise ValueError(f"bad FEN row {row!r}")
    turn = RED if len(parts) < 2 or parts[1] in ("w", "r") else not RED
    halfmove = int(parts[4]) if len(parts) > 4 and parts[4].isdigit() else 0
    return Board(sq, turn, halfmove)


def parse_position(tokens: list[str], validate: bool = True) -> Board:
    """tokens after 'position'. ``validate=False`` pushes the moves without asking the rules (no GPU call per move): the batched
    analysis lets the device check them where they are played (``SelfPlayEngine.set_positions``)."""
    if not tokens:
        raise ValueError("position needs startpos or fen")
    if tokens[0] == "startpos":
        board = Board()
        rest = tokens[1:]
    elif tokens[0] == "fen":
        end = tokens.index("moves") if "moves" in tokens else len(tokens)
        board = board_from_fen(" ".join(tokens[1:end]))
        rest = tokens[end:]
    else:
        raise ValueError("position needs startpos or fen")
    if rest and rest[0] == "moves":
        for u in rest[1:]:
            m = Move.from_uci(u)
            if validate and m.id not in board.legal_ids():
                raise ValueError(f"illegal move {u}")
            board.push(m)
    return board


def go_mate_plies(tok):
    """``go ... mate N``: the plies of the mate search of this one command, 2N - 1 clamped to the cap; None without ``mate``.
    ValueError: N is missing, no integer, or < 1."""
    if "mate" not in tok:
        return None
    i = tok.index("mate")
    if i + 1 >= len(tok) or not tok[i + 1].lstrip("-").isdigit() or int(tok[i + 1]) < 1:
        raise ValueError("go mate needs a number of moves >= 1")
    return min(2 * int(tok[i + 1]) - 1, MATE_MAX_PLIES)


class UciLoop:
    def __init__(self, policy_value_fn=None, n_playout: int = PLAYOUT, device: int = 0, out=sys.stdout):
        self.policy_value_fn = policy_value_fn
        self.n_playout = n_playout
        self.device = device
        self.out = out
        self.board = None
        self.ai = None
        self.multipv = 1
        self.solver = False
        self.width = 1               # Width: leaves per evaluator call (1: the sequential, scouted search)
        self.lcb = False             # LCB: bestmove is the lower-confidence-bound move (LCBStdevs / LCBMinVisitRatio: its numbers)
        self.lcb_opts = {}
        self.mate_plies = 0          # MateSearch: plies of the mate search before every go (0: off); MateNodes: its budget (None: the default)
        self.mate_nodes = None
        self.search_opts = {}        # FpuReduction / FpuAbsolute / CpuctBase / CpuctFactor as set; empty: the reference's PUCT

    def _search(self):
        """The ``search`` dict of ``MCTS_AI`` for the options set so far (None: none was set)."""
        from .searchcfg import make_search
        o = self.search_opts
        return make_search(o.get("fpureduction"), o.get("fpuabsolute"), None, None, o.get("cpuctbase"), o.get("cpuctfactor"))

    def _lcb(self):
        """The ``lcb`` dict of ``MCTS_AI`` for the options set so far (None: off)."""
        from .options import make_lcb
        return make_lcb(self.lcb_opts.get("lcbstdevs", True), self.lcb_opts.get("lcbminvisitratio")) if self.lcb else None

    def _mate(self, plies=None):
        """The ``mate_search`` dict for the options set so far (None: off); ``plies``: of this one command (``go mate N``)."""
        from .options import make_mate_search
        return make_mate_search(self.mate_plies if plies is None else plies, self.mate_nodes if (plies or self.mate_plies) else None)

    def _set(self, **new) -> bool:
        """Set ``solver`` / ``width`` / ``search_opts`` if they still go together (``SearchOptions``); else say why not and leave all as it was."""
        old = {k: getattr(self, k) for k in new}
        vars(self).update(new)
        try:
            self.width = int(self.width)
            if not 1 <= self.width <= 64:
                raise ValueError(f"Width {self.width} must be in 1..64")
            SearchOptions(self.n_playout, width=self.width, solver=self.solver, search=self._search(), lcb=self._lcb(), mate_search=self._mate())
        except ValueError as e:
            vars(self).update(old)
            self._say(f"info string error {e}")
            return False
        return True

    def _say(self, s: str):
        print(s, file=self.out, flush=True)

    def _player(self, nodes: int):
        from .mcts import MCTS_AI
        if self.policy_value_fn is None:
            from .net import PolicyValueNet
            self.policy_value_fn = PolicyValueNet(device=f"cuda:{self.device}").policy_value_fn
        search, lcb = self._search(), self._lcb()
        if self.ai is None or self.ai.mcts.lcb != lcb or self.ai.mcts.n_playout != nodes or self.ai.mcts.solver != self.solver or self.ai.mcts.search_cfg != search \
                or self.ai.mcts.width != self.width:
            self.ai = MCTS_AI(self.policy_value_fn, c_puct=C_PUCT, n_playout=nodes, is_selfplay=False, device=self.device, solver=self.solver,
                              search=search, width=self.width, lcb=lcb)
        return self.ai

    def _say_pvs(self, ai):
        """One ``info depth <len> multipv <i> score cp <cp> nodes <root visits> pv <m1 m2 ...>`` line per principal variation of the
        search just finished (the tree is still on the engine: ``get_action`` only marks it for discarding)."""
        from .analyse import cp_of
        from .engine import mate_score
        pv = ai.mcts._engine.principal_variations(multipv=self.multipv, max_len=32)
        # Solver on: a line whose first move leads to a proven child says `score mate N` (N in moves, negative: the side to move is
        # mated); the move a proven root asks for (bestmove follows it) leads line 1 when the most visited move is another one
        mates, proven = {}, None
        if self.solver:
            rp, rc = ai.mcts.root_proof(), ai.mcts.root_children()
            mates = {int(a): mate_score(rp["child_state"][i], rp["child_dist"][i]) for i, a in enumerate(rc["acts"])}
            proven = ai.mcts.proof_move()
        for r in range(self.multipv):
            ln = int(pv["len"][0, r])
            if ln:
                ids = [int(i) for i in pv["moves"][0, r, :ln]]
                if r == 0 and proven is not None and ids[0] != proven:
                    ids = [proven]
                mate = mates.get(ids[0])
                score = f"mate {mate}" if mate is not None else f"cp {cp_of(pv['q'][0, r], pv['visits'][0, r, 0])}"
                line = " ".join(Move.from_id(i).uci() for i in ids)
                self._say(f"info depth {len(ids)} multipv {r + 1} score {score} nodes {int(pv['root_visits'][0])} pv {line}")

    def handle(self, line: str) -> bool:
        """Process one command line; returns False on quit."""
        tok = line.split()
        if not tok:
            return True
        cmd = tok[0]
        if cmd == "uci":
            self._say(f"id name {ENGINE_NAME}")
            self._say("id author cczero-mi355x builders")
            self._say(f"option name Playouts type spin default {self.n_playout} min 1 max 1000000")
            self._say("option name MultiPV type spin default 1 min 1 max 128")
            self._say("option name Solver type check default false")
            self._say("option name Width type spin default 1 min 1 max 64")
            self._say("option name LCB type check default false")
            self._say("option name LCBStdevs type string default 5")
            self._say("option name LCBMinVisitRatio type string default 0.15")
            self._say(f"option name MateSearch type spin default 0 min 0 max {MATE_MAX_PLIES}")
            self._say(f"option name MateNodes type spin default {MATE_NODES} min 1 max {MATE_MAX_NODES}")
            self._say("option name FpuReduction type string default <empty>")
            self._say("option name FpuAbsolute type string default <empty>")
            self._say("option name CpuctBase type string default <empty>")
            self._say("option name CpuctFactor type string default <empty>")
            self._say("uciok")
        elif cmd == "isready":
            self._say("readyok")
        elif cmd == "setoption" and len(tok) >= 5 and tok[1] == "name" and tok[2].lower() == "playouts":
            self.n_playout = int(tok[4])
        elif cmd == "setoption" and len(tok) >= 5 and tok[1] == "name" and tok[2].lower() == "multipv":
            self.multipv = max(1, min(128, int(tok[4])))
        elif cmd == "setoption" and len(tok) >= 5 and tok[1] == "name" and tok[2].lower() == "solver":
            self._set(solver=tok[4].lower() == "true")
        elif cmd == "setoption" and len(tok) >= 5 and tok[1] == "name" and tok[2].lower() == "lcb":
            self._set(lcb=tok[4].lower() == "true")
        elif cmd == "setoption" and len(tok) >= 5 and tok[1] == "name" and tok[2].lower() in ("lcbstdevs", "lcbminvisitratio"):
            try:
                self._set(lcb_opts=dict(self.lcb_opts, **{tok[2].lower(): float(tok[4])}))
            except ValueError as e:
                self._say(f"info string error {e}")
        elif cmd == "setoption" and len(tok) >= 5 and tok[1] == "name" and tok[2].lower() in ("matesearch", "matenodes"):
            try:
                self._set(**{"mate_plies" if tok[2].lower() == "matesearch" else "mate_nodes": int(tok[4])})
            except ValueError as e:
                self._say(f"info string error {e}")
        elif cmd == "setoption" and len(tok) >= 5 and tok[1] == "name" and tok[2].lower() == "width":
            self._set(width=tok[4])
        elif cmd == "setoption" and len(tok) >= 5 and tok[1] == "name" and tok[2].lower() in ("fpureduction", "fpuabsolute", "cpuctbase", "cpuctfactor"):
            name = tok[2].lower()
            opts = dict(self.search_opts)
            try:
                opts[name] = float(tok[4])
            except ValueError as e:
                self._say(f"info string error {e}")
                return True
            if name in ("fpureduction", "fpuabsolute"):      # the later of the two forms stands
                opts.pop("fpuabsolute" if name == "fpureduction" else "fpureduction", None)
            if self._set(search_opts=opts):
                self._say("info string search parameters set: scout slots are off for this session")
        elif cmd == "ucinewgame":
            self.board = Board()
            self.ai = None
        elif cmd == "position":
            try:
                self.board = parse_position(tok[1:])
            except (ValueError, KeyError) as e:
                self._say(f"info string error {e}")
        elif cmd == "go":
            if self.board is None:
                self.board = Board()
            nodes = self.n_playout
            if "nodes" in tok:
                nodes = int(tok[tok.index("nodes") + 1])
            if self.board.is_game_over():
                self._say("bestmove (none)")
                return True
            ai = self._player(nodes)
            try:
                mate = self._mate(go_mate_plies(tok))
            except ValueError as e:
                self._say(f"info string error {e}")
                return True
            move, probs = ai.get_action(self.board, temp=1e-3, return_prob=True, mate_search=mate)
            if ai.last_mate is not None:     # a forced mate by checks: no playout ran, the tree holds nothing to report
                _, dist, mate_nodes = ai.last_mate
                self._say(f"info depth {dist} score mate {(dist + 1) // 2} nodes {mate_nodes} pv {Move.from_id(move).uci()}")
                self._say(f"bestmove {Move.from_id(move).uci()}")
                return True
            self._say_pvs(ai)
            rc = ai.mcts.root_children()
            self._say(f"info nodes {int(rc['root_visits'])} string visits {int(rc['visits'].max())}/{int(rc['visits'].sum())}")
            self._say(f"bestmove {Move.from_id(move).uci()}")
        elif cmd == "d":
            self._say(str(self.board if self.board is not None else Board()))
        elif cmd == "quit":
            return False
        return True

    def run(self, inp=sys.stdin):
        for line in inp:
            if not self.handle(line.strip()):
                break


if __name__ == "__main__":
    UciLoop().run()
