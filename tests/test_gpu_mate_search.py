"""GPU: ``ccz_mate_search`` against its sequential model (tests/mate_model.py) on the fixtures of tests/mate_cases.py: state, dist, move
and nodes are equal, exactly, at every depth and budget the fixtures name; the call changes nothing of the engine and writes nothing
but its four arrays; what it refuses it refuses with an error and no sticky bit."""
import functools

import numpy as np
import pytest
import torch

import mate_cases as mc
import mate_model as mm
from gpu_harness import make_evaluator, planes_to_squares

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = mc.load()
NAMES = [f["name"] for f in FIXTURES]
N = len(FIXTURES)
ALONE = ("wide_late_mate", "h18_dist7", "h22_history")          # each also searched in an engine of one board


def _load(e, fixtures, extra_park=0):
    B = e.B
    sq = np.zeros((B, 90), np.uint8)
    turn, half, moves = np.ones(B, np.uint8), np.zeros(B, np.int32), [[] for _ in range(B)]
    for b, fx in enumerate(fixtures):
        sq[b], turn[b], half[b] = mc.squares(fx), fx["turn"], fx["halfmove"]
        moves[b] = [mc.move_id(u) for u in fx["history"]]
    status = e.set_positions(sq, turn, half, moves, park=np.arange(B) >= len(fixtures))
    assert not status.any(), status
    return e


def _engine(fixtures=FIXTURES, n_boards=None, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    return _load(SelfPlayEngine(len(fixtures) if n_boards is None else n_boards, n_playout=32, seed=3, **kw), fixtures)


@functools.lru_cache(maxsize=None)
def model(name, plies, budget):
    """The model's answer, computed once and shared by the tests."""
    return mm.mate_search(mc.board(FIXTURES[NAMES.index(name)]), plies, budget)


def _settings():
    return [(p, mc.BIG) for p in mc.PLIES] + sorted({(7, b) for fx in FIXTURES for b in fx["budgets"]})


def _same(got, fixtures, plies, budget, rows=None):
    for b, fx in enumerate(fixtures):
        want = model(fx["name"], plies, budget)
        have = tuple(int(got[k][b if rows is None else rows[b]]) for k in ("state", "dist", "move", "nodes"))
        print(fx["name"], plies, budget, have, want)
        assert have == want, (fx["name"], plies, budget, have, want)


@pytest.fixture(scope="module")
def engine():
    return _engine()


def test_all_fixtures_equal_the_model_at_every_setting(engine):
    for plies, budget in _settings():
        _same(engine.mate_search(plies, budget), FIXTURES, plies, budget)
    states = {model(n, 7, mc.BIG)[0] for n in NAMES} | {model(fx["name"], 7, b)[0] for fx in FIXTURES for b in fx["budgets"]}
    assert states == {mm.FOUND, mm.NO_MATE, mm.BUDGET}


@pytest.mark.parametrize("name", ALONE)
def test_one_fixture_alone_at_one_board(name):
    fx = FIXTURES[NAMES.index(name)]
    e = _engine([fx])
    for plies, budget in [(p, mc.BIG) for p in mc.PLIES] + [(7, b) for b in fx["budgets"]]:
        _same(e.mate_search(plies, budget), [fx], plies, budget)


def test_budget_one_is_state_three_with_one_node(engine):
    got = engine.mate_search(7, 1)
    assert (got["state"] == mm.BUDGET).all() and (got["nodes"] == 1).all() and (got["dist"] == 0).all() and (got["move"] == -1).all()


def test_parked_finished_and_inactive_boards_are_not_searched():
    from chinesechesszero_amd.engine import SelfPlayEngine
    two = FIXTURES[NAMES.index("two_rooks")]
    e = SelfPlayEngine(4, n_playout=32, seed=3, eval_cache_log2=10)
    sq = np.stack([mc.squares(two)] * 4)
    moves = [[], [mc.move_id("a7a9")], [], []]                  # board 1: the mate is on the board, the game is over
    status = e.set_positions(sq, np.ones(4, np.uint8), np.zeros(4, np.int32), moves, park=np.array([0, 0, 1, 0], bool))
    assert not status.any() and e.game_status()["over"].tolist() == [0, 1, 1, 0]
    e.set_scouts(1)                                             # board 3 lies beyond the active boards
    got = e.mate_search(7, 64)
    assert got["state"].tolist() == [mm.FOUND, 0, 0, 0] and got["dist"].tolist() == [1, 0, 0, 0]
    assert got["move"].tolist() == [mc.move_id("a7a9"), -1, -1, -1] and got["nodes"].tolist() == [2, 0, 0, 0]
    e.set_scouts(0)
    assert e.mate_search(7, 64)["state"].tolist() == [mm.FOUND, 0, 0, mm.FOUND]
    assert e.stats()["error_flags"] == 0


def _snapshot(e):
    rc, st = e.root_children(), e.game_status()
    return ([rc[k].tobytes() for k in ("k", "acts", "visits", "q", "prior", "root_visits")], [st[k].tobytes() for k in ("over", "winner", "plies", "turn")],
            e.stats(), e.root_positions().tobytes())


def test_the_same_answers_on_grown_trees_and_nothing_of_the_engine_changes():
    e = _engine()
    ev = make_evaluator("hash", [7] * N)
    for _ in range(20):
        e.select_leaves()
        sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
        P, V = ev(sq, turn)
        e.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
    before = _snapshot(e)
    assert e.root_children()["root_visits"].max() == 20
    for plies, budget in ((7, mc.BIG), (15, mc.BIG), (7, 11)):
        _same(e.mate_search(plies, budget), FIXTURES, plies, budget)
    assert _snapshot(e) == before and before[2]["error_flags"] == 0
    # ... and the search goes on as if the call had not been made: the next leaves are those of an engine that was never asked
    f = _engine()
    for _ in range(20):
        f.select_leaves()
        sq, turn = planes_to_squares(f.leaf_input.float().cpu().numpy())
        P, V = ev(sq, turn)
        f.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
    assert torch.equal(e.select_leaves(), f.select_leaves()) and e.leaf_info()["ids"].tobytes() == f.leaf_info()["ids"].tobytes()


def test_the_outputs_sit_in_an_arena_that_comes_back_intact(engine):
    pad = 256
    arena = torch.full((pad + 16 * N + pad,), 0xFF, dtype=torch.uint8, device=DEV)
    out = arena[pad:pad + 16 * N].view(torch.int32).view(4, N)
    got = engine.mate_search(7, mc.BIG, out=out)
    _same(got, FIXTURES, 7, mc.BIG)
    host = arena.cpu().numpy()
    assert (host[:pad] == 0xFF).all() and (host[pad + 16 * N:] == 0xFF).all()
    assert np.array_equal(host[pad:pad + 16 * N].view(np.int32).reshape(4, N), np.stack([got[k] for k in ("state", "dist", "move", "nodes")]))


def test_refusals_return_an_error_and_set_no_flag(engine):
    from chinesechesszero_amd._lib import MATE_MAX_NODES, MATE_MAX_PLIES, CczError
    for plies, budget in ((2, 64), (0, 64), (-1, 64), (MATE_MAX_PLIES + 2, 64), (MATE_MAX_PLIES + 1, 64), (7, 0), (7, -5), (7, MATE_MAX_NODES + 1)):
        with pytest.raises(CczError, match="ccz_mate_search"):
            engine.mate_search(plies, budget)
    assert engine.stats()["error_flags"] == 0
    got = engine.mate_search(MATE_MAX_PLIES, MATE_MAX_NODES)       # the caps themselves are accepted, and the launch ends
    assert set(got["state"].tolist()) <= {mm.FOUND, mm.NO_MATE, mm.BUDGET} and (got["nodes"] <= MATE_MAX_NODES).all()
    with pytest.raises(ValueError):
        engine.mate_search(7, 64, out=torch.zeros((4, N + 1), dtype=torch.int32, device=DEV))


def test_the_move_follows_a_non_default_move_rank():
    """Descending ids: the first mating move in `legal_moves` order is another one where a position has several."""
    import oracle
    rank = (2085 - np.arange(2086)).astype(np.uint16)
    oracle.set_rules(move_rank=rank)
    try:
        want = [mm.mate_search(mc.board(fx), 7, mc.BIG) for fx in FIXTURES]
    finally:
        oracle.set_rules()
    moved = [fx["name"] for fx, w in zip(FIXTURES, want) if w[0] == mm.FOUND and w[2] != model(fx["name"], 7, mc.BIG)[2]]
    assert moved, "no fixture tells the two orders apart"
    got = _engine(move_rank=rank, type_rank=None).mate_search(7, mc.BIG)
    for b, fx in enumerate(FIXTURES):
        assert tuple(int(got[k][b]) for k in ("state", "dist", "move", "nodes")) == want[b], (fx["name"], want[b])
