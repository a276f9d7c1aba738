"""GPU: the search parameters (ccz_set_search, include/cczero.h) -- first-play urgency and the visit-scaled
exploration constant -- against the sequential model of tests/search_model.py. Exact, no tolerance anywhere: after every lockstep step
the leaf (status, k, ids, depth, position) and the root children's N and Q bits, after every move the move played and the events, at
the end the counters (simulations, leaf depths, exploration, solver, resignation) and the harvested records byte for byte.

Inputs (search_model.inputs): 8 boards -- the start position, `pawns` (7 moves), `widest` (108 moves: the second 64-lane pass of the
mass and of the arg-max), `mate_in_two`, a check with one legal move, a double check with two, two opening positions --, 64
simulations a move, three moves with tree reuse, with the near-uniform ``hash`` evaluator and with the scripted peaked one of
tests/gumbel_model.py. tests/test_cpu_search_model.py asserts on the model alone that these inputs exercise the rule.

Every case but the ``off`` ones fails on the parent commit: the library has no ccz_set_search."""
import numpy as np
import pytest
import torch

import gumbel_model as gm
import resign_model as rm
import search_model as sm
import selfplay_model as spm
import solver_model as svm
from gpu_harness import planes_to_squares
from oracle import OracleBoard
from test_gpu_gumbel import _boundary as _gumbel_boundary
from test_gpu_gumbel import _close, _lockstep, _same_records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------- engine next to model
def _engine(positions, n_playout=sm.SIMS, max_plies=sm.MOVES, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(len(positions), n_playout=n_playout, seed=sm.SEED, board_id_base=sm.BASE, max_plies=max_plies, **kw)
    sq = np.stack([s for s, _ in positions]).astype(np.uint8)
    status = e.set_positions(sq, np.array([t for _, t in positions], np.uint8))
    assert (status == 0).all(), status
    return e


def _move(e, m, where):
    """One move boundary on both sides: the move played and what happened to the game."""
    live = [not o for o in m.over]
    st0 = e.game_status()
    played = e.finish_move().cpu().numpy().copy()
    events = m.finish_move()
    st1, rs = e.game_status(), e.resign_status()
    got = []
    for b in range(e.B):
        rec = m.last[b]
        if not live[b] or rec is None:                           # no game, or adjudicated at the ply cap
            assert played[b] == -1, (where, b)
        else:
            assert played[b] == rec["move"], (where, b, played[b], rec["move"])
        if st0["over"][b]:
            got.append("over")
        elif st1["over"][b] and played[b] < 0 and (rs["state"][b] & rm.RESIGNED):
            got.append("resign")
        elif st1["over"][b] and played[b] < 0:
            got.append("cap")
        else:
            got.append("playon" if (rs["state"][b] & rm.PLAYON) and rs["fire_ply"][b] == st0["plies"][b] else None)
    rm.check_events(got, events, where)
    assert [bool(x) for x in st1["over"]] == list(m.over), where
    return rs


def _depths(e, m):
    st = e.stats()
    assert (st["sims"], st["sum_depth"], st["depth_peak"]) == (m.sims, m.sum_depth, m.depth_peak), (st["sims"], st["sum_depth"], st["depth_peak"],
                                                                                                      m.sims, m.sum_depth, m.depth_peak)


def _play(e, m, f, where, sims=sm.SIMS, moves=sm.MOVES, fused=True, cap=None, after_step=None, after_move=None):
    for mv in range(moves):
        if all(m.over):
            break
        if cap is not None:
            drawn = e.draw_budgets(*cap).cpu().numpy().copy()
            assert drawn.tolist() == m.begin_move(), (where, mv)
        _lockstep(e, m, f, sims, fused, (where, mv), after_step=after_step)
        if after_move is not None:
            after_move(mv)
        _move(e, m, (where, mv))
    _depths(e, m)


# ---------------------------------------------------------------------------------------------------------------- 1. lockstep with the model
@pytest.mark.parametrize("fused", [False, True], ids=["select_expand", "step"])
@pytest.mark.parametrize("setting,evaluator", [("reduction", "hash"), ("absolute", "peaked"), ("mixed", "peaked"), ("growth", "peaked")])
def test_engine_equals_the_model(setting, evaluator, fused):
    m, f = sm.case(setting, evaluator)
    e = _engine(sm.inputs())
    e.set_search(**sm.SETTINGS[setting])
    assert e.search_settings() == dict(sm.SETTINGS[setting], enabled=True)
    _play(e, m, f, (setting, evaluator), fused=fused)
    assert m.sfacts["unvisited_not_first"] > 0 and m.sfacts["fresh_root_not_child0"] > 0
    assert evaluator != "hash" or m.sfacts["hi_before_lo"] > 0    # an unvisited child 64.. chosen ahead of a lower unvisited one
    _close(e, m, f)


def test_the_planned_compact_sequence_equals_the_model():
    from test_gpu_selfplay_all_options import HashLogits, _planned_step
    from test_gpu_solver import DevicePriors
    salts = (spm.SALT,) * sm.B                                  # HashLogits is the hash evaluator with this one salt
    m = sm.SearchModel(sm.boards(), salts, sm.SEED, sm.BASE, search=sm.SETTINGS["growth"], max_plies=sm.MOVES, evaluator=DevicePriors())
    e = _engine(sm.inputs(), eval_cache_log2=14)
    e.set_search(**sm.SETTINGS["growth"])
    ev = HashLogits()
    for mv in range(sm.MOVES):
        e.select_leaves()
        for i in range(sm.SIMS):
            _planned_step(e, ev, i + 1 == sm.SIMS)
            m.step()
        rc = e.root_children()
        for b in range(sm.B):
            if m.over[b]:
                continue
            acts, visits, q, prior = m.root_children(b)
            k = len(acts)
            assert rc["k"][b] == k and np.array_equal(rc["visits"][b][:k], visits), (mv, b, rc["visits"][b][:k], visits)
            assert np.array_equal(rc["q"][b][:k].view(np.uint32), q.view(np.uint32)), (mv, b)
            assert np.array_equal(rc["prior"][b][:k].view(np.uint32), prior.view(np.uint32)), (mv, b)
        _move(e, m, ("planned", mv))
    _depths(e, m)
    assert e.stats()["cache_probes"] == m.rows
    e.select_leaves()
    _planned_step(e, ev, True)
    e.finish_move()
    m.finish_move()
    assert e.game_status()["over"].all() and all(m.over)
    rec = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
    e.check_healthy()
    _same_records(rec, m.records(game_no=2))


# ---------------------------------------------------------------------------------------------------------------- 2. combinations
def test_with_root_exploration_forced_playouts_and_pruning():
    m, f = sm.case("growth", "peaked", explore=sm.EXPLORE)
    e = _engine(sm.inputs())
    e.set_search(**sm.SETTINGS["growth"])
    e.set_root_exploration(eps=sm.EXPLORE["eps"], alpha=None, forced_k=sm.EXPLORE["forced_k"], prune_targets=sm.EXPLORE["prune"])

    def noise(mv):
        rows, ks = e.root_noise()
        for b in range(e.B):
            if not m.over[b]:
                row = m.noise(b)
                assert ks[b] == len(row) and np.array_equal(rows[b][:len(row)].view(np.uint32), row.view(np.uint32)), (mv, b)
    _play(e, m, f, "explore", after_move=noise)
    t = m.totals()
    assert e.exploration_stats() == t and t["forced_selections"] > 0 and t["visits_pruned"] > 0
    _close(e, m, f)


def test_with_the_gumbel_root_the_tree_pair_applies_from_depth_one():
    g = dict(n_sims=32, max_considered=8, c_visit=50.0, c_scale=1.0)
    m, f = sm.case("reduction", "peaked", gumbel=g)
    e = _engine(sm.inputs(), n_playout=32)
    e.set_gumbel(**g)
    e.set_search(**sm.SETTINGS["reduction"])
    for mv in range(sm.MOVES):
        if all(m.over):
            break
        _lockstep(e, m, f, 32, True, ("gumbel", mv))
        _gumbel_boundary(e, m, ("gumbel", mv))
    _depths(e, m)
    assert m.gstats["gumbel_moves"] > 0 and m.sfacts["unvisited_not_first"] > 0
    _close(e, m, f)


def test_with_the_solver_on_mate_in_two():
    which = [sm.MATE2, sm.PAWNS]
    m, f = sm.case("reduction", "hash", which=which, solver=True, max_plies=2)
    e = _engine([sm.inputs()[j] for j in which], n_playout=96, max_plies=2)
    e.set_search(**sm.SETTINGS["reduction"])
    e.set_solver(True)

    def proofs(i):
        rp = e.root_proof()
        for b in range(e.B):
            if m.over[b]:
                continue
            st, ds, cs, cd = m.root_proof(b)
            k = len(cs)
            assert (rp["state"][b], rp["dist"][b]) == (st, ds), (i, b)
            assert np.array_equal(rp["child_state"][b][:k], cs) and np.array_equal(rp["child_dist"][b][:k], cd), (i, b)
    _play(e, m, f, "solver", sims=96, moves=2, fused=True, after_step=proofs)
    assert e.solver_stats() == m.solver_stats()
    assert m.nodes_proven > 0 and m.proven_stops > 0
    _close(e, m, f)


def test_with_drawn_budgets_and_resignation():
    rule = rm.Rule(-0.03, 1, 0, 0.5)
    cap = (sm.SIMS, 16, 0.5)
    m, f = sm.case("growth", "hash", resign=rule, cap=cap)
    e = _engine(sm.inputs())
    e.set_search(**sm.SETTINGS["growth"])
    e.set_resign(threshold=rule.threshold, consecutive=rule.consecutive, min_ply=rule.min_ply, p_playon=rule.p_playon)
    budgets = []
    _play(e, m, f, "budgets", cap=cap, after_move=lambda mv: budgets.append(list(m.budget)))
    assert {16, sm.SIMS} <= {b for row in budgets for b in row}
    assert m.xfacts["resign"] + m.xfacts["playon"] > 0
    _close(e, m, f)
    assert {k: int(v) for k, v in e.resign_stats().items() if k in rm.STAT_KEYS} == m.resign_stats()


def test_batched_self_play_planned_equals_dense():
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    from test_gpu_selfplay_all_options import HashLogits
    n, moves = 32, 2
    pos = sm.inputs()

    def run(cache):
        sp = BatchedSelfPlay(HashLogits(), sm.B, n_playout=n, seed=sm.SEED, board_id_base=sm.BASE, max_plies=moves, eval_cache_log2=cache,
                             search=sm.SETTINGS["growth"], playout_cap=(8, 0.5))
        assert sp.planned == (cache > 0) and sp.search_cfg == sm.SETTINGS["growth"]
        e = sp.engine
        assert e.search_settings() == dict(sm.SETTINGS["growth"], enabled=True)
        assert (e.set_positions(np.stack([s for s, _ in pos]).astype(np.uint8), np.array([t for _, t in pos], np.uint8)) == 0).all()
        played = [sp.run_move().cpu().numpy().copy() for _ in range(moves)]
        stats = e.stats()
        sp.simulate()
        e.finish_move()
        assert e.game_status()["over"].all()
        rec = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
        e.check_healthy()
        return played, stats, rec

    pa, sa, ra = run(14)
    pb, sb, rb = run(0)
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    assert (sa["sims"], sa["sum_depth"], sa["depth_peak"]) == (sb["sims"], sb["sum_depth"], sb["depth_peak"])
    _same_records(ra, rb)
    assert sa["cache_probes"] > 0 and sb["cache_probes"] == 0


# ---------------------------------------------------------------------------------------------------------------- 3. off means untouched
@pytest.mark.parametrize("called", [False, True], ids=["never_called", "set_search_off"])
def test_off_is_the_parents_behaviour_on_the_all_options_inputs(called):
    """The SelfPlayModel comparison of tests/test_gpu_selfplay_all_options.py, on its inputs, with the rule never mentioned and with
    it turned on and off again."""
    import test_gpu_selfplay_all_options as ao
    e = ao._engine()
    if called:
        e.set_search(fpu_mode=1, fpu_value=0.4, c_base=8.0, c_factor=2.0)
        e.set_search(False)
    assert e.search_settings() == sm.DEFAULTS
    ao._check_model(ao._drive_dense(e, True), spm.dense_run())


def test_turned_off_equals_never_called_bit_for_bit():
    f = gm.hash_evaluator(sm.SALTS)

    def run(toggle):
        e = _engine(sm.inputs(), n_playout=24)
        if toggle:
            e.set_search(fpu_mode=2, fpu_value=0.5, fpu_root_mode=1, fpu_root_value=0.2, c_base=100.0, c_factor=1.5)
            e.set_search(enabled=0)
        assert e.search_settings() == sm.DEFAULTS
        out = []
        for mv in range(2):
            e.select_leaves()
            for i in range(24):
                info = e.leaf_info()
                pl = e.leaf_input.float().cpu().numpy()
                out.append(pl.tobytes())
                sq, turn = planes_to_squares(pl)
                P, V = np.zeros((e.B, 2086), np.float32), np.zeros(e.B, np.float32)
                for b in range(e.B):
                    if info["status"][b] == svm.LEAF_EXPAND:
                        P[b], V[b] = f(b, sq[b], turn[b])
                (e.step if i + 1 < 24 else e.expand_backup)(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
            rc = e.root_children()
            out += [rc[key].tobytes() for key in ("k", "acts", "visits", "q", "prior", "root_visits")]
            out.append(e.finish_move().cpu().numpy().tobytes())
        out.append(sorted(e.stats().items()))
        e.check_healthy()
        return out
    assert run(True) == run(False)


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals():
    from chinesechesszero_amd._lib import CczError
    from chinesechesszero_amd.engine import SelfPlayEngine
    from chinesechesszero_amd.mcts import MCTS_AI
    e = SelfPlayEngine(4, n_playout=8, eval_cache_log2=10)
    inf, nan = float("inf"), float("nan")
    good = dict(fpu_mode=1, fpu_value=0.25, fpu_root_mode=2, fpu_root_value=-0.5, c_base=100.0, c_factor=1.0)
    e.set_search(**good)
    kept = dict(good, enabled=True)
    assert e.search_settings() == kept
    bad = {"fpu_mode": [dict(fpu_mode=3), dict(fpu_mode=-1)],
           "fpu_value": [dict(fpu_mode=1, fpu_value=-0.1), dict(fpu_mode=1, fpu_value=inf), dict(fpu_mode=1, fpu_value=nan),
                         dict(fpu_mode=2, fpu_value=1.5), dict(fpu_mode=2, fpu_value=-1.01), dict(fpu_mode=2, fpu_value=nan)],
           "fpu_root_mode": [dict(fpu_root_mode=3, fpu_root_value=0.0), dict(fpu_root_mode=-2, fpu_root_value=0.0)],
           "fpu_root_value": [dict(fpu_root_mode=1, fpu_root_value=-1.0), dict(fpu_root_mode=1, fpu_root_value=inf),
                              dict(fpu_root_mode=2, fpu_root_value=2.0), dict(fpu_root_mode=2, fpu_root_value=nan)],
           "c_base": [dict(c_base=0.0), dict(c_base=-1.0), dict(c_base=inf), dict(c_base=nan)],
           "c_factor": [dict(c_factor=-0.5), dict(c_factor=inf), dict(c_factor=nan)]}
    for field, cases in bad.items():
        for kw in cases:
            with pytest.raises(CczError, match=r"ccz_set_search: .*\b" + field + r"\b"):
                e.set_search(**kw)
            assert e.search_settings() == kept, (field, kw)          # the old settings survive a refused call
    # the edges of the ranges are allowed; enabled = 0 ignores the other arguments and stores the defaults
    e.set_search(fpu_mode=1, fpu_value=0.0, fpu_root_mode=2, fpu_root_value=1.0, c_base=1e-9, c_factor=0.0)
    e.set_search(fpu_mode=2, fpu_value=-1.0)
    assert e.L.ccz_set_search(e.h, e._stream(), 0, 7, nan, -3, inf, -1.0, nan) == 0
    assert e.search_settings() == sm.DEFAULTS
    # scouts, in both orders
    e.set_search(**good)
    with pytest.raises(CczError, match="ccz_set_scouts: .*ccz_set_search"):
        e.set_scouts(2)
    e.set_search(False)
    e.set_scouts(2)
    with pytest.raises(CczError, match="ccz_set_search: .*scout"):
        e.set_search(**good)
    assert e.search_settings() == sm.DEFAULTS
    e.set_scouts(0)
    e.set_search(**good)
    e.check_healthy()
    with pytest.raises(ValueError, match="scouts"):
        MCTS_AI(lambda board: None, n_playout=8, search=good, scouts=10)


# ---------------------------------------------------------------------------------------------------------------- 5. frontends
def test_mcts_ai_plays_the_models_moves():
    from oracle.evaluators import hash_eval
    from chinesechesszero_amd.game import Board, Move
    from chinesechesszero_amd.mcts import MCTS_AI
    from test_gpu_frontends_parity import _hash_policy
    salt, n = 9, 48
    s = sm.SETTINGS["growth"]

    def ev(b, board):
        p, v = hash_eval(board.squares()[None, :], np.array([1 if board.turn else 0]), salt=salt, scale=40.0)
        return p[0].astype(np.float32), np.float32(v[0])
    ai = MCTS_AI(_hash_policy(salt), c_puct=5, n_playout=n, is_selfplay=False, search=s)
    assert ai.mcts.scouts == 0
    board, ob = Board(), OracleBoard()
    for ply in range(3):
        m = sm.SearchModel([ob], (0,), 0, 0, search=s, evaluator=ev)        # a fresh tree every move (mcts.py:228-229)
        for _ in range(n):
            m.simulate(0)
        acts, visits, q, _ = m.root_children(0)
        np.random.seed(ply)
        move = ai.get_action(board, temp=1e-3)
        rc = ai.mcts.root_children()
        k = len(acts)
        assert np.array_equal(np.asarray(rc["acts"])[:k], acts) and np.array_equal(np.asarray(rc["visits"])[:k], visits), ply
        assert ai.mcts._engine.search_settings() == dict(s, enabled=True)
        top = np.nonzero(visits == visits.max())[0]
        assert int(move) in acts[top].tolist(), (ply, move)
        if len(top) == 1:
            assert int(move) == int(acts[top[0]])
        assert visits.max() > 1 and (visits == 0).any()                       # the rule acted: not one look at every move
        board.push(Move.from_id(int(move)))
        ob.push_id(int(move))


def test_analyse_returns_the_models_best_move_and_visits():
    from chinesechesszero_amd.analyse import BatchedAnalysis
    from chinesechesszero_amd.tools import move_id2move_action as uci_of
    from test_gpu_selfplay_all_options import HashLogits
    from test_gpu_solver import DevicePriors
    lines = ["startpos", "startpos moves h2e2", "startpos moves h2e2 h9g7", "startpos moves b0c2 b9c7 c2b0"]
    n = 48
    s = sm.SETTINGS["reduction"]
    boards = []
    for text in lines:
        ob = OracleBoard()
        for u in text.split()[2:]:
            ob.push(u)
        boards.append(ob)
    m = sm.SearchModel(boards, (spm.SALT,) * 4, 0, 0, search=s, evaluator=DevicePriors())
    for _ in range(n):
        m.step()
    an = BatchedAnalysis(HashLogits(), 4, n_playout=n, multipv=1, max_len=4, search=s)
    recs = an.analyse(lines)
    rc = an.engine.root_children()
    for b, r in enumerate(recs):
        acts, visits, _, _ = m.root_children(b)
        k = len(acts)
        assert r["status"] == "ok" and r["root_visits"] == n, (b, r)
        assert rc["k"][b] == k and np.array_equal(rc["visits"][b][:k], visits), (b, rc["visits"][b][:k], visits)
        assert r["bestmove"] == uci_of[int(acts[int(np.argmax(visits))])], (b, r["bestmove"])
        assert r["lines"][0]["visits"][0] == int(visits.max())
    summary = an.summary()
    assert summary["search"] == dict(s, enabled=True)
    assert summary["mean_leaf_depth"] == round(m.sum_depth / m.sims, 3)
