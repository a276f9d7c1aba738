"""CPU: the sequential model of the mate search (tests/mate_model.py) and its fixtures (tests/mate_cases.py), without a GPU.

The fixture set must hold what every category of the GPU test needs (counted here on the model alone); the model is certified two
ways -- the exhaustive ``solver_model.negamax`` on the short mates, and an independent AND/OR replay under the oracle's exact game rules
on every mate --; three mis-stated models each give another answer on some fixture; and the option parsing, the UCI option lines and
``go mate N`` (with a fake player) behave as the front ends document.

Two things the fixtures pin that are worth knowing when reading a failure:
  * ``mate_in_two`` of tests/solver_cases.py is a forced mate in three plies whose FIRST move (i7i8) is quiet: the checking-sequence search
    does not find it by definition (include/cczero.h: it "never looks at a quiet first move"), the model says state 2 at every depth, and
    negamax says WIN in 3 by a move that gives no check.
  * the two ``history`` fixtures are forced wins under the game's rules (negamax: WIN in 3 by a checking move) that the search misses
    on purpose: any repeat of a history position blocks, not only the fourth."""
import io
import os
import re

import numpy as np
import pytest

import mate_cases as mc
import mate_model as mm
import solver_model as sm

FIXTURES = mc.load()
NAMES = [f["name"] for f in FIXTURES]
# the dist-5 fixtures of the fewest positions within three plies: an exhaustive five-ply negamax of each ends within seconds
NEGAMAX5 = ("h26_dist5", "h27_dist5", "h29_small", "h32_small")


def _fx(name):
    return FIXTURES[NAMES.index(name)]


_CACHE = {}


def result(fx, plies=7, budget=mc.BIG, **kw):
    """The model's (state, dist, move, nodes), computed once per setting and shared by the tests."""
    key = (fx["name"], plies, budget, tuple(sorted(kw.items())))
    if key not in _CACHE:
        o = mc.board(fx, **{k: v for k, v in kw.items() if k in ("history", "halfmove")})
        _CACHE[key] = mm.mate_search(o, plies, budget, wrong=kw.get("wrong"))
    return _CACHE[key]


def _gives_check(board, mv):
    c = board.copy()
    c.push_id(mv)
    return c.in_check()


# ---------------------------------------------------------------------------------------------------------------- the fixture set
def test_the_constants_are_the_headers():
    from chinesechesszero_amd import _lib, options
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    with open(os.path.join(root, "include", "cczero.h")) as f:
        text = f.read()
    plies = int(re.search(r"#define CCZ_MATE_MAX_PLIES (\d+)", text).group(1))
    nodes = int(re.search(r"#define CCZ_MATE_MAX_NODES (\d+)", text).group(1))
    assert (plies, nodes) == (mm.MAX_PLIES, mm.MAX_NODES) == (_lib.MATE_MAX_PLIES, _lib.MATE_MAX_NODES) == (options.MATE_MAX_PLIES, options.MATE_MAX_NODES)
    assert (_lib.MATE_NONE, _lib.MATE_FOUND, _lib.MATE_NO_MATE, _lib.MATE_BUDGET) == (mm.NONE, mm.FOUND, mm.NO_MATE, mm.BUDGET) == (0, 1, 2, 3)
    assert mc.BIG <= nodes and max(mc.PLIES) <= plies and _lib.ABI_VERSION == 9
    assert re.search(r"#define CCZ_ABI_VERSION 9\b", text)


def test_the_seed_fixtures():
    assert len(FIXTURES) <= 80 and len(set(NAMES)) == len(NAMES)
    st, dist, mv, nodes = result(_fx("two_rooks"))
    assert (st, dist, mc.uci(mv), nodes) == (mm.FOUND, 1, "a7a9", 2)
    wide = _fx("wide_late_mate")
    ids = mc.board(wide).legal_ids()
    st, dist, mv, _ = result(wide)
    assert (st, dist, mc.uci(mv)) == (mm.FOUND, 1, "a5a9") and len(ids) == 105 and ids.index(mv) == 67
    assert sum(_gives_check(mc.board(wide), i) and not _after(mc.board(wide), i).legal_ids() for i in ids) == 1      # the only mating move
    # mate_in_two: a mate in three plies that begins with a quiet move -- out of the search's scope, and the model says so at every depth
    two = _fx("mate_in_two")
    board = mc.board(two)
    assert sm.negamax(board, 3) == sm.pack(sm.WIN, 3) and not _gives_check(board, mc.move_id("i7i8"))
    assert sm.state_of(sm.negamax(_after(board, mc.move_id("i7i8")), 2)) == sm.LOSS
    for plies in mc.PLIES:
        assert result(two, plies)[:3] == (mm.NO_MATE, 0, -1)


def _after(board, mv):
    c = board.copy()
    c.push_id(mv)
    return c


def test_the_fixtures_hold_what_every_category_needs():
    by_dist = {d: set() for d in (1, 3, 5, 7)}
    tags, with_check, small, hist, clock = set(), 0, 0, 0, 0
    for fx in FIXTURES:
        st, dist, mv, nodes = r = result(fx)
        board = mc.board(fx)
        if st == mm.FOUND:
            assert dist in by_dist and mv in board.legal_ids() and _gives_check(board, mv), fx["name"]
            by_dist[dist].add((fx["name"], fx["turn"]))
            tags |= mc.tags_of(board, st, dist, mv)
            for b in fx["budgets"]:
                got = result(fx, budget=b)
                small += got == (mm.BUDGET, 0, -1, b)
        elif st == mm.NO_MATE:
            with_check += any(_gives_check(board, i) for i in board.legal_ids())
        if fx["history"]:
            bare = result(fx, history=False)
            hist += bare[0] == mm.FOUND and (st != mm.FOUND or dist > bare[1])
        if fx["halfmove"] >= 100:
            assert board.halfmove == fx["halfmove"]
            clock += st != mm.FOUND and result(fx, halfmove=0)[0] == mm.FOUND
        assert r[0] != mm.BUDGET and result(fx, 15)[0] != mm.BUDGET, fx["name"]     # the large budget is large for every fixture
    for d, got in by_dist.items():
        assert len(got) >= 4 and {t for _, t in got} == {0, 1}, (d, got)
    assert with_check >= 8 and small >= 2 and hist >= 2 and clock >= 1, (with_check, small, hist, clock)
    assert {"discovered", "double", "late", "capture"} <= tags, tags


def test_budgets_stop_at_the_count():
    fx = _fx("h18_dist7")
    full = result(fx)
    assert full[0] == mm.FOUND and result(fx, budget=1) == (mm.BUDGET, 0, -1, 1)
    assert result(fx, budget=full[3]) == (mm.BUDGET, 0, -1, full[3])           # the node that would complete the proof reaches the budget
    assert result(fx, budget=full[3] + 1) == full
    with pytest.raises(AssertionError):
        mm.MateSearch(4, 10)


# ---------------------------------------------------------------------------------------------------------------- certification
@pytest.mark.parametrize("name", [f["name"] for f in FIXTURES if result(f)[0] == mm.FOUND and result(f)[1] <= 3] + list(NEGAMAX5))
def test_negamax_agrees_on_the_short_mates(name):
    fx = _fx(name)
    st, dist, mv, _ = result(fx)
    assert st == mm.FOUND and (dist <= 3 or dist == 5)
    board = mc.board(fx)
    got = sm.negamax(board, dist)
    assert sm.state_of(got) == sm.WIN and sm.dist_of(got) <= dist, (name, got)
    assert sm.state_of(sm.negamax(_after(board, mv), dist - 1)) == sm.LOSS          # ... and the model's move is a winning one


def test_negamax_finds_no_checking_mate_where_the_model_finds_none():
    seen = quiet = 0
    for fx in FIXTURES:
        if result(fx, 3)[0] != mm.NO_MATE or fx["history"] or fx["halfmove"]:
            continue
        board = mc.board(fx)
        if len(board.legal_ids()) > 60:
            continue
        seen += 1
        if sm.state_of(sm.negamax(board, 3)) == sm.WIN:
            # a win within three plies that the search does not see: every winning first move is quiet, or -- where it gives check --
            # some reply to it is answered only by a STALEMATING move (mate_in_two: i7i9+ Ke8, g7f7), which is out of scope too
            winners = [i for i in board.legal_ids() if sm.state_of(sm.negamax(_after(board, i), 2)) == sm.LOSS]
            assert winners and not mm.forced_win(board, 3, quiet_plies=0), fx["name"]
            for i in winners:
                a = _after(board, i)
                if a.in_check():
                    assert any(not any(_after(_after(a, r), m).in_check() and not _after(_after(a, r), m).legal_ids()
                                       for m in _after(a, r).legal_ids()) for r in a.legal_ids()), (fx["name"], mc.uci(i))
            quiet += 1
    assert seen >= 8 and quiet >= 1                # (mate_in_two is one of the latter)


def test_the_history_fixtures_are_wins_the_search_misses_on_purpose():
    n = 0
    for fx in FIXTURES:
        if fx["history"]:
            board = mc.board(fx)
            assert result(fx, 3)[0] == mm.NO_MATE and sm.negamax(board, 3) == sm.pack(sm.WIN, 3), fx["name"]
            assert result(fx, 3, wrong="repeats_ok")[:2] == (mm.FOUND, 3) == result(fx, 3, history=False)[:2]
            n += 1
    assert n >= 2


def test_every_mate_is_a_forced_win_under_the_games_own_rules():
    n = 0
    for fx in FIXTURES:
        for plies in (7, 15):
            st, dist, mv, _ = result(fx, plies)
            if st == mm.FOUND and (plies == 7 or result(fx)[0] != mm.FOUND):
                board = mc.board(fx)
                assert mm.forced_win(board, dist), (fx["name"], dist)
                assert mm._defender_lost(_after(board, mv), dist - 1, 3), fx["name"]       # by the move the search names
                assert dist == 1 or not mm.forced_win(board, dist - 2, quiet_plies=0), fx["name"]   # (no shorter mate by checks alone)
                n += 1
    assert n >= 20


# ---------------------------------------------------------------------------------------------------------------- mis-stated models
@pytest.mark.parametrize("wrong", mm.WRONG)
def test_a_mis_stated_model_gives_another_answer(wrong):
    differ = []
    for fx in FIXTURES:
        for budget in [mc.BIG] + fx["budgets"]:
            if result(fx, budget=budget, wrong=wrong) != result(fx, budget=budget):
                differ.append((fx["name"], budget))
    assert differ, wrong


# ---------------------------------------------------------------------------------------------------------------- options, UCI
def test_make_mate_search_and_its_refusals():
    import argparse
    from chinesechesszero_amd import options as O
    assert O.make_mate_search(None) is None and O.make_mate_search(0) is None and O.make_mate_search(False) is None
    assert O.make_mate_search(7) == {"max_plies": 7, "node_budget": O.MATE_NODES}
    assert O.make_mate_search(31, 1) == {"max_plies": 31, "node_budget": 1}
    for bad in ((4,), (-1,), (33,), (7, 0), (7, O.MATE_MAX_NODES + 1), (None, 5)):
        with pytest.raises(ValueError):
            O.make_mate_search(*bad)
    assert O.mate_search_of({"plies": 5, "nodes": 64}) == {"max_plies": 5, "node_budget": 64} == O.mate_search_of({"max_plies": 5, "node_budget": 64})
    with pytest.raises(ValueError):
        O.mate_search_of({"plies": 5, "depth": 3})

    def parse(argv):
        ap = argparse.ArgumentParser()
        O.add_mate_search_args(ap)
        return O.mate_search_from_args(ap, ap.parse_args(argv))
    assert parse([]) is None and parse(["--mate-search", "7"]) == {"max_plies": 7, "node_budget": O.MATE_NODES}
    assert parse(["--mate-search", "15", "--mate-nodes", "256"]) == {"max_plies": 15, "node_budget": 256}
    for argv in (["--mate-nodes", "256"], ["--mate-search", "8"], ["--mate-search", "7", "--mate-nodes", "0"]):
        with pytest.raises(SystemExit):
            parse(argv)


def test_search_options_carry_it_beside_the_tables():
    from chinesechesszero_amd import options as O
    off = O.SearchOptions(solver=False, search=None)
    assert off.mate_search is None and off.keywords() == {"solver": False, "search": None} and off.log_line(None) == "" and off.report(None) == {}
    on = O.SearchOptions(solver=False, mate_search=7)
    assert on.mate_search == {"max_plies": 7, "node_budget": O.MATE_NODES} and on.keywords() == {"solver": False} and on.on == {}
    assert "mate_search" not in O.ALL_OPTIONS
    assert on.report(None) == {"mate_search": {"max_plies": 7, "node_budget": O.MATE_NODES, "boards": 0, "mates": 0, "mean_nodes": None}}
    on.mate_counts.update(boards=4, mates=1, nodes=10)
    assert on.log_line(None) == ", mate search boards 4, mates 1, mean nodes 2.5" and on.report(None)["mate_search"]["mean_nodes"] == 2.5
    with pytest.raises(ValueError):
        O.SearchOptions(mate_search=6)


class _FakeEngine:
    """What ``options.mate_moves`` asks of an engine."""
    B, solver = 4, True

    def mate_search(self, plies, nodes):
        self.asked = (plies, nodes)
        return {"state": np.array([1, 1, 2, 0], np.int32), "dist": np.array([3, 5, 0, 0], np.int32),
                "move": np.array([11, 22, -1, -1], np.int32), "nodes": np.array([9, 40, 7, 0], np.int32)}

    def game_status(self):
        return {"over": np.array([0, 0, 0, 1], np.uint8)}

    def root_proof(self):
        return {"state": np.array([1, 1, 0, 0], np.uint8), "dist": np.array([5, 3, 0, 0], np.uint8)}


def test_mate_moves_fills_forced_and_yields_to_a_quicker_proof():
    from chinesechesszero_amd.options import mate_moves
    e, counts = _FakeEngine(), {"boards": 0, "mates": 0, "nodes": 0}
    forced, n = mate_moves(e, None, None)
    assert forced is None and n == 0 and not hasattr(e, "asked")                      # off: no call
    cfg = {"max_plies": 7, "node_budget": 100}
    forced, n = mate_moves(e, cfg, np.array([5, 6, 7, -1], np.int32), counts=counts)
    # board 0: the tree's WIN proof takes 5 plies, the mate 3 -> the mate; board 1: the proof is quicker (3 <= 5) -> it stays
    assert forced.tolist() == [11, 6, 7, -1] and n == 1 and e.asked == (7, 100)
    assert counts == {"boards": 3, "mates": 2, "nodes": 56}
    forced, n = mate_moves(e, cfg, None)
    assert forced.tolist() == [11, 22, -1, -1] and n == 2                            # (nothing proven was forced: both mates are written)


class _FakePlayer:
    """Stands in for ``MCTS_AI`` under ``UciLoop``: finds the mate only when asked for at least three plies."""
    def __init__(self):
        self.calls = []
        self.last_mate = None
        self.mcts = self

    def get_action(self, board, temp=1e-3, return_prob=False, mate_search=None):
        self.calls.append(mate_search)
        self.last_mate = (mc.move_id("i7i8"), 3, 17) if mate_search and mate_search["max_plies"] >= 3 else None
        return (mc.move_id("a0a1") if self.last_mate is None else self.last_mate[0]), np.zeros(2086)

    def root_children(self):
        return {"root_visits": np.int32(5), "visits": np.array([5])}


def test_uci_options_and_go_mate_with_a_fake_player():
    from chinesechesszero_amd import options as O
    from chinesechesszero_amd.uci import UciLoop, go_mate_plies
    assert go_mate_plies(["go"]) is None and go_mate_plies(["go", "mate", "2"]) == 3 and go_mate_plies("go nodes 5 mate 1".split()) == 1
    assert go_mate_plies(["go", "mate", "99"]) == O.MATE_MAX_PLIES
    for bad in (["go", "mate"], ["go", "mate", "x"], ["go", "mate", "0"]):
        with pytest.raises(ValueError):
            go_mate_plies(bad)
    out = io.StringIO()
    loop = UciLoop(policy_value_fn=lambda b: None, n_playout=8, out=out)
    fake = _FakePlayer()
    loop._player = lambda nodes: fake
    loop._say_pvs = lambda ai: None
    loop.handle("uci")
    lines = out.getvalue().splitlines()
    assert f"option name MateSearch type spin default 0 min 0 max {O.MATE_MAX_PLIES}" in lines
    assert f"option name MateNodes type spin default {O.MATE_NODES} min 1 max {O.MATE_MAX_NODES}" in lines
    loop.board = type("RunningGame", (), {"is_game_over": lambda self: False})()      # (the product's Board asks the GPU for its rules)
    loop.handle("go")                                     # off: the player is asked for no mate search
    loop.handle("go mate 2")                              # this one command: three plies, the default budget
    loop.handle("go")
    loop.handle("go mate 0")                              # refused: an error line, no search
    loop.handle("setoption name MateSearch value 4")      # refused: even
    loop.handle("setoption name MateNodes value 64")
    loop.handle("setoption name MateSearch value 1")
    loop.handle("go")                                     # one ply with 64 nodes: nothing found, the normal search answers
    loop.handle("go mate 2")                              # ... and three plies for this command, with the budget that was set
    loop.handle("setoption name MateSearch value 0")
    loop.handle("go")
    assert fake.calls == [None, {"max_plies": 3, "node_budget": O.MATE_NODES}, None, {"max_plies": 1, "node_budget": 64},
                          {"max_plies": 3, "node_budget": 64}, None]
    text = out.getvalue().splitlines()
    assert text.count("info depth 3 score mate 2 nodes 17 pv i7i8") == 2 and text.count("bestmove i7i8") == 2 and text.count("bestmove a0a1") == 4
    assert sum(l.startswith("info string error") for l in text) == 2
    assert (loop.mate_plies, loop.mate_nodes) == (0, 64)
