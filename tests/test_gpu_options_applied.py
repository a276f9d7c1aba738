"""GPU: a front end built WITH its options (``options.SearchOptions.apply``) against the same front end built with none and the same
settings then made by hand with ``engine.set_*`` (the reference here: the setters themselves are pinned by their own tests). 8 boards
(4 pairs in the arena), 16 playouts, one move, the same seed: the settings as the kernels read them, ``engine.solver``, the root
children after the search (k, acts, visits) and the move played are equal, exactly, on every board -- parked ones included."""
import numpy as np
import pytest

from chinesechesszero_amd.searchcfg import make_search
from chinesechesszero_amd.stopcfg import StopPoll, make_early_stop

pytestmark = pytest.mark.gpu

B, N, SEED = 8, 16, 3
SEARCH = make_search(fpu_reduction=0.3, cpuct_factor=1.0)
STOP = make_early_stop(single_reply=True, gap=1.0)
RESIGN = {"threshold": -0.9, "consecutive": 2, "min_ply": 0}
LINES = ["startpos", "startpos moves h2e2", "startpos moves h2e2 h9g7", "startpos moves b0c2 b9c7 c2b0", "startpos moves b2e2",
         "startpos moves c3c4 c6c5"]          # 6 positions on 8 boards: the last two boards are parked


def _by_hand(front_end, engine, resign=None):
    """The reference: every setter called on the engine, and the attributes the front end's own move logic reads."""
    engine.set_early_stop(**STOP)
    engine.set_search(**SEARCH)
    engine.set_solver(True)
    if resign is not None:
        engine.set_resign(**resign)
        front_end.resign = dict(resign)
    front_end.solver, front_end.search_cfg, front_end.early_stop = True, dict(SEARCH), dict(STOP)
    if hasattr(front_end, "_poll"):
        front_end._poll = StopPoll(engine, STOP)


def _same(a, b):
    """``a`` / ``b``: (engine, root children after the search, moves played) of the two builds."""
    (ea, ra, ma), (eb, rb, mb) = a, b
    assert ea.search_settings() == eb.search_settings() == dict(SEARCH, enabled=True)
    assert ea.early_stop_settings() == eb.early_stop_settings() and ea.early_stop_settings()["enabled"]
    assert ea.solver is True and eb.solver is True
    for key in ("k", "acts", "visits"):
        assert np.array_equal(ra[key], rb[key]), key
    assert ra["visits"].sum() > 0 and np.array_equal(np.asarray(ma), np.asarray(mb))
    ea.check_healthy()
    eb.check_healthy()


def _resign_bytes(engine):
    return {k: v.tobytes() for k, v in engine.resign_status().items()}          # (bytes: an unknown last_value is NaN)


def test_batched_self_play():
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    from test_gpu_selfplay_all_options import HashLogits

    def run(by_hand):
        opts = {} if by_hand else dict(resign=RESIGN, solver=True, search=SEARCH, early_stop=STOP)
        sp = BatchedSelfPlay(HashLogits(), B, n_playout=N, seed=SEED, **opts)
        if by_hand:
            _by_hand(sp, sp.engine, RESIGN)
        sp.search()
        rc = sp.engine.root_children()
        return sp.engine, rc, sp.finish_move().cpu().numpy()
    a, b = run(False), run(True)
    _same(a, b)
    assert _resign_bytes(a[0]) == _resign_bytes(b[0])


def test_arena():
    from chinesechesszero_amd.arena import Arena
    from test_gpu_resign_arena import ValueStub

    def run(by_hand):
        opts = {} if by_hand else dict(resign=RESIGN, solver=True, search=SEARCH, early_stop=STOP)
        ar = Arena(ValueStub(0.95), ValueStub(0.95), B // 2, n_playout=N, opening_plies=4, seed=SEED, max_plies=10, eval_cache_log2=12, **opts)
        if by_hand:
            _by_hand(ar, ar.engine, dict(RESIGN, p_playon=0.0))
        ar.search()
        rc = ar.engine.root_children()
        return ar.engine, rc, ar.finish_move()
    a, b = run(False), run(True)
    _same(a, b)
    assert _resign_bytes(a[0]) == _resign_bytes(b[0])


def test_batched_match():
    from chinesechesszero_amd.match import BatchedMatch
    from chinesechesszero_amd.net import uniform_evaluator

    def run(by_hand):
        opts = {} if by_hand else dict(solver=True, search=SEARCH, early_stop=STOP)
        m = BatchedMatch(uniform_evaluator, uniform_evaluator, B, n_playout=N, seed=SEED, max_plies=10, **opts)
        if by_hand:
            _by_hand(m, m.engine)
        seen = []
        m.before_move = lambda mm: seen.append(mm.engine.root_children())
        moves = m.play_move(1)
        return m.engine, seen[0], moves
    _same(run(False), run(True))


def test_batched_analysis():
    from chinesechesszero_amd.analyse import BatchedAnalysis
    from test_gpu_selfplay_all_options import HashLogits

    def run(by_hand):
        opts = {} if by_hand else dict(solver=True, search=SEARCH, early_stop=STOP)
        an = BatchedAnalysis(HashLogits(), B, n_playout=N, multipv=1, max_len=4, seed=SEED, **opts)
        if by_hand:
            _by_hand(an.sp, an.engine)
            an.solver = True
        records = an.analyse(LINES)
        return (an.engine, an.engine.root_children(), [r["bestmove"] for r in records]), records
    (a, ra), (b, rb) = run(False), run(True)
    _same(a, b)
    assert ra == rb and all(r["status"] == "ok" for r in ra)
