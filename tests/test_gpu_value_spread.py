"""GPU: the value spread S per node and the LCB move (ccz_set_value_stats / ccz_root_value_stats / ccz_lcb_moves, include/cczero.h;
DESIGN.md section 8m) against the sequential model of tests/value_spread_model.py. Exact, no tolerance anywhere: after every
simulation N, Q bits and S bits of every root's children and N and S bits of the root (the root's Q has no accessor), on the stepping
sequences, across kept-tree re-roots; ccz_lcb_moves' moves, child indices and every bound's bits.

Boards (search_model.inputs): the start position, ``widest`` (108 moves: the second 64-lane pass of the expansion's S = 0 and of
ccz_lcb_moves) and ``mate_in_two`` (terminal leaves, whose value comes from the status). 48 simulations a move, three moves.

Every test here fails on the parent commit at its first call: the library has no ccz_set_value_stats."""
import numpy as np
import pytest
import torch

import search_model as sm
import selfplay_model as spm
import value_spread_model as vsm
from test_gpu_gumbel import _close, _lockstep
from test_gpu_search_params import _engine, _move

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WHICH = [sm.START, sm.WIDE, sm.MATE2]
SIMS, MOVES = 48, 3
LCB_SETTINGS = [(5.0, 0.15, 2), (0.0, 0.0, 0), (1.0, 1.0, 5), (2.5, 0.4, 3)]


def _case(evaluator="hash", which=WHICH, **kw):
    salts = tuple(sm.SALTS[j] for j in which)
    f = sm.EVALUATORS[evaluator](salts)
    cfg = dict(max_plies=MOVES)
    cfg.update(kw)
    m = vsm.SpreadModel(sm.boards(which), salts, sm.SEED, sm.BASE, evaluator=lambda b, board: f(b, board.squares(), int(board.turn)), **cfg)
    return m, f


def _positions(which=WHICH):
    return [sm.inputs()[j] for j in which]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same_spread(e, m, where, scouts=0):
    """N, Q, S of every live root's children and N, S of the root, bit for bit; zero rows past k, on finished boards and scout slots."""
    rc, vs = e.root_children(), e.root_value_stats()
    for b in range(e.B):
        if b >= m.B or m.over[b]:
            assert not vs["S"][b].view(np.uint32).any() and vs["root_S"][b].view(np.uint32) == 0, (where, b)
            continue
        _, N, Q, _ = m.root_children(b)
        S, root_s = m.root_spread(b)
        k = len(N)
        assert rc["k"][b] == k and np.array_equal(rc["visits"][b][:k], N), (where, b)
        assert np.array_equal(_bits(rc["q"][b][:k]), _bits(Q)), (where, b)
        assert np.array_equal(_bits(vs["S"][b][:k]), _bits(S)), (where, b, vs["S"][b][:k], S)
        assert not vs["S"][b][k:].view(np.uint32).any(), (where, b)
        assert rc["root_visits"][b] == m.roots[b].N and _bits(vs["root_S"][b:b + 1])[0] == _bits([root_s])[0], (where, b)


def _same_lcb(e, m, where, scouts=0):
    """ccz_lcb_moves at every setting: moves, child indices and the bits of every bound (-inf where there is none, 0 past k)."""
    departed = 0
    for z, ratio, mv in LCB_SETTINGS:
        got = e.lcb_moves(z, ratio, mv, with_bounds=True)
        moves, child, lcb = (got[k].cpu().numpy() for k in ("moves", "child", "lcb"))
        wm, wc, wl = vsm.lcb_moves(m, z, ratio, mv, scouts=scouts)
        assert np.array_equal(moves, wm) and np.array_equal(child, wc), (where, z, ratio, mv, moves, wm, child, wc)
        assert np.array_equal(lcb.view(np.uint64), wl.view(np.uint64)), (where, z, ratio, mv)
        assert np.array_equal(e.lcb_moves(z, ratio, mv).cpu().numpy(), wm)          # (without the optional outputs)
        for b in range(m.B):
            if wc[b] >= 0:
                departed += int(wc[b] != vsm.first_max_visits(m.root_children(b)[1]))
    return departed


# ---------------------------------------------------------------------------------------------------------------- 1. the sequences
@pytest.mark.parametrize("fused", [False, True], ids=["select_expand", "step"])
@pytest.mark.parametrize("evaluator", ["hash", "peaked"])
def test_engine_equals_the_model_after_every_simulation(evaluator, fused):
    m, f = _case(evaluator)
    e = _engine(_positions(), n_playout=SIMS, max_plies=MOVES)
    assert e.get_value_stats() is False
    e.set_value_stats(True)
    assert e.get_value_stats() is True
    departed, widest = 0, 0
    for mv in range(MOVES):
        _lockstep(e, m, f, SIMS, fused, (evaluator, mv), after_step=lambda i: _same_spread(e, m, (evaluator, mv, i)))
        widest = max(widest, max(len(m.root_children(b)[0]) for b in range(m.B) if not m.over[b]))
        departed += _same_lcb(e, m, (evaluator, mv))
        _move(e, m, (evaluator, mv))                  # a kept-tree re-root: S travels with the node, the pool half flips
        _same_spread(e, m, (evaluator, mv, "re-rooted"))
        _same_lcb(e, m, (evaluator, mv, "re-rooted"))
    assert widest > 64                                                # children 64.. exist: the second pass
    assert departed > 0                                               # at some setting the LCB move is not the most visited one
    assert any(float(s) > 0.0 for b in range(m.B) if not m.over[b] for s in m.root_spread(b)[0])
    _close(e, m, f)                                                   # all games adjudicated: every board is finished
    _same_spread(e, m, "closed")
    _same_lcb(e, m, "closed")


def test_terminal_leaves_feed_the_spread():
    """mate_in_two and ``pawns`` with the solver and the FPU reduction, 96 simulations (tests/test_gpu_search_params.py's solver case:
    the plain PUCT rule does not reach the mate within them): the search reaches
    leaves decided by the rules (value -1 / 0 from the status) and, once a node is proven, stops at it (value +1 / -1 / 0 from its proof)."""
    which = [sm.MATE2, sm.PAWNS]
    m, f = _case("hash", which=which, solver=True, max_plies=2, search=sm.SETTINGS["reduction"])
    e = _engine(_positions(which), n_playout=96, max_plies=2)
    e.set_search(**sm.SETTINGS["reduction"])
    e.set_solver(True)
    e.set_value_stats(True)
    _lockstep(e, m, f, 96, True, "mate", after_step=lambda i: _same_spread(e, m, ("mate", i)))
    assert e.stats()["terminal_leaves"] > 0 and m.nodes_proven > 0 and m.proven_stops > 0
    _same_lcb(e, m, "mate")


def test_the_planned_compact_sequence_equals_the_model():
    from test_gpu_selfplay_all_options import HashLogits, _planned_step
    from test_gpu_solver import DevicePriors
    salts = (spm.SALT,) * len(WHICH)                              # HashLogits is the hash evaluator with this one salt
    m = vsm.SpreadModel(sm.boards(WHICH), salts, sm.SEED, sm.BASE, max_plies=MOVES, evaluator=DevicePriors())
    e = _engine(_positions(), n_playout=SIMS, max_plies=MOVES, eval_cache_log2=14)
    e.set_value_stats(True)
    ev = HashLogits()
    for mv in range(MOVES):
        e.select_leaves()
        for i in range(SIMS):
            _planned_step(e, ev, i + 1 == SIMS)
            m.step()
            _same_spread(e, m, ("planned", mv, i))
        _same_lcb(e, m, ("planned", mv))
        _move(e, m, ("planned", mv))
        _same_spread(e, m, ("planned", mv, "re-rooted"))
    # the last board as a scout slot: no tree, no move, a zero row
    e.set_scouts(1)
    vs = e.root_value_stats()
    assert not vs["S"][-1].any() and vs["root_S"][-1] == 0
    live = vsm.SpreadModel.__new__(vsm.SpreadModel)
    live.__dict__.update(m.__dict__)
    live.B = m.B - 1
    _same_lcb(e, live, "scout slot", scouts=1)
    e.set_scouts(0)
    e.check_healthy()


# ---------------------------------------------------------------------------------------------------------------- 2. scouts
def _scouted(pvn, scouts, n, plies, loop, monkeypatch, lcb):
    from chinesechesszero_amd.game import Board
    from chinesechesszero_amd.mcts import MCTS
    monkeypatch.setenv("CCZ_SCOUT_DEVICE_LOOP", loop)
    mcts = MCTS(pvn.policy_value_fn, 5, n, scouts=scouts, lcb=lcb)
    board, out = Board(), []
    for ply in range(plies):
        acts, probs = mcts.get_move_probs(board, temp=1.0)
        e = mcts._engine
        rc, vs = e.root_children(), e.root_value_stats()
        out.append({"visits": rc["visits"][0].copy(), "q": _bits(rc["q"][0]).copy(), "S": _bits(vs["S"][0]).copy(), "root_S": _bits(vs["root_S"][:1]).copy(),
                    "lcb": mcts.lcb_move(), "scout_rows": bool(vs["S"][1:].any())})
        mv = int(acts[int(np.argmax(probs))])
        mcts.update_with_move(mv)
        board.push(mv)
    mcts._engine.check_healthy()
    return out


def test_the_scouted_paths_keep_the_same_spread(monkeypatch):
    """MCTS's one-game search: the device loop of ccz_scouted_run, the host loop of the same phases and the search without scouts build
    the same S (and N, Q), and name the same LCB move."""
    from test_gpu_scouts import _net
    pvn = _net()
    n, plies = 80, 3
    want = _scouted(pvn, 0, n, plies, "1", monkeypatch, True)
    assert any(w["S"].any() for w in want) and all(w["lcb"] is not None for w in want)
    for scouts, loop in ((10, "1"), (10, "0")):
        got = _scouted(pvn, scouts, n, plies, loop, monkeypatch, True)
        for ply, (a, b) in enumerate(zip(want, got)):
            assert not b["scout_rows"]
            for key in ("visits", "q", "S", "root_S"):
                assert np.array_equal(a[key], b[key]), (scouts, loop, ply, key)
            assert a["lcb"] == b["lcb"], (scouts, loop, ply)


# ---------------------------------------------------------------------------------------------------------------- 3. on is invisible, off is off
def _run(e, f, moves=MOVES, sims=SIMS):
    """A fused dense run without a model: what tells two searches apart -- every leaf, every root, every move, the records."""
    from gpu_harness import planes_to_squares
    sig = []
    for mv in range(moves):
        e.select_leaves()
        for i in range(sims):
            info = e.leaf_info()
            sig.append((info["status"].tobytes(), info["k"].tobytes(), info["depth"].tobytes(), info["ids"].tobytes(), e.leaf_input.cpu().numpy().tobytes()))
            sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
            P, V = np.zeros((e.B, 2086), np.float32), np.zeros(e.B, np.float32)
            for b in range(e.B):
                if info["status"][b] == 0:
                    P[b], V[b] = f(b, sq[b], turn[b])
            tp, tv = torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV)
            if i + 1 < sims:
                e.step(tp, tv)
            else:
                e.expand_backup(tp, tv)
        rc = e.root_children()
        sig.append(tuple(rc[k].tobytes() for k in ("k", "acts", "visits", "q", "prior", "root_visits")))
        sig.append(e.finish_move().cpu().numpy().tobytes())
    return sig


def _finish(e, f):
    sig = _run(e, f, moves=1, sims=1)            # every live root needs children; the ply cap then adjudicates
    sig.append(torch.cat(list(e.harvest_record_chunks())).cpu().numpy().tobytes())
    st = e.stats()
    sig.append(tuple(st[k] for k in ("sims", "expansions", "terminal_leaves", "sum_depth", "depth_peak")))
    e.check_healthy()
    return sig


def test_on_is_invisible_and_off_is_off():
    _, f = _case("peaked")
    never = _engine(_positions(), n_playout=SIMS, max_plies=MOVES)
    want = _run(never, f) + _finish(never, f)
    on = _engine(_positions(), n_playout=SIMS, max_plies=MOVES)
    on.set_value_stats(True)
    assert _run(on, f) + _finish(on, f) == want
    back = _engine(_positions(), n_playout=SIMS, max_plies=MOVES)
    back.set_value_stats(True)
    back.set_value_stats(False)
    assert back.get_value_stats() is False
    with pytest.raises(Exception, match="ccz_root_value_stats: the value spread is off"):
        back.root_value_stats()
    assert _run(back, f) + _finish(back, f) == want


def test_turning_it_on_again_starts_from_zeros():
    """On for a move (the pool's S slots are written), off for 20 simulations of a fresh search (nodes are made in those slots and no
    S is written), on again in mid-search: from there S is the model's whose sums were cleared at that point -- the array was zeroed."""
    m, f = _case("hash")
    e = _engine(_positions(), n_playout=SIMS, max_plies=MOVES)
    e.set_value_stats(True)
    _run(e, f, moves=1)
    e.set_value_stats(False)
    sq = np.stack([s for s, _ in _positions()]).astype(np.uint8)
    assert (e.set_positions(sq, np.array([t for _, t in _positions()], np.uint8)) == 0).all()
    _lockstep(e, m, f, 20, False, "off")
    m.clear_spread()
    e.set_value_stats(True)
    _lockstep(e, m, f, 28, True, "on again", after_step=lambda i: _same_spread(e, m, ("on again", i)))
    assert any(float(s) > 0.0 for b in range(m.B) for s in m.root_spread(b)[0])


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_in_both_orders_and_bad_arguments():
    from chinesechesszero_amd._lib import CczError
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(4, n_playout=8, seed=1)
    with pytest.raises(CczError, match="ccz_lcb_moves: the value spread is off"):
        e.lcb_moves(5.0, 0.15, 2)
    with pytest.raises(CczError, match="ccz_root_value_stats: the value spread is off"):
        e.root_value_stats()
    e.set_value_stats(True)
    with pytest.raises(CczError, match="ccz_set_width: .*ccz_set_value_stats"):
        e.set_width(2)
    with pytest.raises(CczError, match="ccz_snapshot_save: .*ccz_set_value_stats"):
        e.save_state()
    e.set_value_stats(False)
    blob = e.save_state()
    e.set_value_stats(True)
    with pytest.raises(CczError, match="ccz_snapshot_load: .*ccz_set_value_stats"):
        e.load_state(blob)
    for bad, what in (((-1.0, 0.15, 2), "z"), ((float("inf"), 0.15, 2), "z"), ((float("nan"), 0.15, 2), "z"), ((5.0, 1.5, 2), "min_visit_ratio"),
                      ((5.0, -0.1, 2), "min_visit_ratio"), ((5.0, float("nan"), 2), "min_visit_ratio"), ((5.0, 0.15, -1), "min_visits")):
        with pytest.raises(CczError, match="ccz_lcb_moves: " + what):
            e.lcb_moves(*bad)
    assert (e.lcb_moves(5.0, 0.15, 2).cpu().numpy() == -1).all()     # nothing searched: no visited child
    e.set_value_stats(False)
    e.set_width(2)
    with pytest.raises(CczError, match="ccz_set_value_stats: .*ccz_set_width"):
        e.set_value_stats(True)
    e.set_width(1)
    e.set_value_stats(True)
    h = SelfPlayEngine(4, n_playout=8, seed=1, value_f16=True)
    with pytest.raises(CczError, match="ccz_set_value_stats: .*CCZ_FLAG_VALUE_F16"):
        h.set_value_stats(True)
    assert h.get_value_stats() is False
