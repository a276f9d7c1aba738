"""GPU: the Gumbel root search (ccz_set_gumbel, include/cczero.h) against the sequential model of
tests/gumbel_model.py. Exact, no tolerance anywhere: the considered-visits sequence, after every lockstep step the leaf (status, k,
ids, depth, position) and the root children's N and Q bits, the Gumbel rows, pi', moves, counters and the harvested records byte for
byte.

Inputs (gumbel_model.inputs): 8 boards -- seven opening positions with 30 to 50 legal moves and `pawns` (7 moves: m = k below
max_considered = 16) --, six moves with tree reuse (N0 != 0 from the second move on), n = 32 / m = 16 and n = 8 / m = 4, with the
near-uniform ``hash`` evaluator and with a scripted peaked one (priors 0.6 / 0.2 / ...) that makes the logit term decide.
tests/test_cpu_gumbel_model.py asserts on the model alone that these inputs exercise the rules.

Every case fails on the parent commit: the library has no ccz_set_gumbel."""
import functools

import numpy as np
import pytest
import torch

import gumbel_model as gm
import resign_model as rm
import selfplay_model as spm
import solver_cases as sc
import solver_model as sm
from gpu_harness import planes_to_squares
from oracle import OracleBoard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAME_NO = 2             # the record header's count of games started on a slot: ccz_create starts the first, set_positions the second
SKIP, EXPAND = gm.LEAF_SKIP, sm.LEAF_EXPAND


# ---------------------------------------------------------------------------------------------------------------- 1. the sequence
def test_the_considered_visits_sequence():
    from chinesechesszero_amd import _lib
    L = _lib.lib()
    cases = [(m, n) for m in range(1, 18) for n in range(1, 71)]
    out = torch.full((len(cases), 72), -1, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for j, (m, n) in enumerate(cases):
        _lib.check(L.ccz_gumbel_sequence(s, m, n, out[j].data_ptr()))
    got = out.cpu().numpy()
    for j, (m, n) in enumerate(cases):
        assert got[j, :n].tolist() == gm.sequence(m, n), (m, n)
        assert (got[j, n:] == -1).all(), (m, n)                     # n entries and not one more
    for (m, n), want in {(4, 8): [0, 0, 0, 0, 1, 1, 2, 2], (3, 7): [0, 0, 0, 1, 1, 2, 2], (2, 5): [0, 0, 1, 1, 2]}.items():
        assert got[cases.index((m, n)), :n].tolist() == want
    assert L.ccz_gumbel_sequence(s, 4, 8, None) != 0 and L.ccz_gumbel_sequence(s, 4, -1, out.data_ptr()) != 0


# ---------------------------------------------------------------------------------------------------------------- engine next to model
def _engine(positions, n_playout, max_plies, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(len(positions), n_playout=n_playout, seed=gm.SEED, board_id_base=gm.BASE, max_plies=max_plies, **kw)
    sq = np.stack([s for s, _ in positions]).astype(np.uint8)
    status = e.set_positions(sq, np.array([t for _, t in positions], np.uint8))
    assert (status == 0).all(), status
    return e


def _same_children(e, m, where):
    rc = e.root_children()
    for b in range(e.B):
        if m.over[b]:
            continue
        acts, visits, q, prior = m.root_children(b)
        k = len(acts)
        assert rc["k"][b] == k and np.array_equal(rc["acts"][b][:k], acts.astype(np.uint16)), (where, b)
        assert np.array_equal(rc["visits"][b][:k], visits), (where, b, rc["visits"][b][:k], visits)
        assert np.array_equal(rc["q"][b][:k].view(np.uint32), q.view(np.uint32)), (where, b)
        assert np.array_equal(rc["prior"][b][:k].view(np.uint32), prior.view(np.uint32)), (where, b)
    return rc


def _lockstep(e, m, f, steps, fused, where, after_step=None):
    """``steps`` lockstep simulations of the engine and the model side by side, both fed ``f(b, squares, turn)``. After every step:
    the leaf the engine selected is the model's (status, k, ids, depth, and the position: the path), the root's children are the model's."""
    B = e.B
    e.select_leaves()
    for i in range(steps):
        info = e.leaf_info()
        sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
        want = m.step()
        P, V = np.zeros((B, 2086), np.float32), np.zeros(B, np.float32)
        for b, (status, k, depth) in enumerate(want):
            w = (where, i, b)
            if status == SKIP:
                assert info["status"][b] == SKIP, w
                continue
            assert (info["status"][b], info["k"][b], info["depth"][b]) == (status, k, depth), (w, info["status"][b], info["k"][b], info["depth"][b], status, k, depth)
            _, _, _, ids, lsq, lturn = m.leaf[b]
            if lsq is not None:                                  # (a descent stopped at a proven node generates no moves and writes no evaluator row)
                assert info["ids"][b][:k].tolist() == ids[:k] and k == len(ids), w
                assert np.array_equal(sq[b], lsq) and int(turn[b]) == lturn, w
            if status == EXPAND:
                P[b], V[b] = f(b, sq[b], turn[b])
        tp, tv = torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV)
        if fused and i + 1 < steps:
            e.step(tp, tv)
        else:
            e.expand_backup(tp, tv)
            if i + 1 < steps:
                e.select_leaves()
        _same_children(e, m, (where, i))
        if after_step is not None:
            after_step(i)


def _same_rows(e, m, where):
    g, logit, n0, k, n_eff = e.gumbel_root()
    for b in range(e.B):
        row = None if m.over[b] else m.root_row(b)
        if row is None:
            assert k[b] == 0 and not g[b].any() and not logit[b].any() and not n0[b].any() and n_eff[b] == 0, (where, b)
            continue
        kk = len(row[0])
        assert k[b] == kk and n_eff[b] == row[3], (where, b, k[b], kk, n_eff[b], row[3])
        assert g[b][:kk].tobytes() == row[0].tobytes() and logit[b][:kk].tobytes() == row[1].tobytes(), (where, b)
        assert np.array_equal(n0[b][:kk], row[2]), (where, b)
        assert not g[b][kk:].any() and not logit[b][kk:].any() and not n0[b][kk:].any(), (where, b)
    return n_eff


def _boundary(e, m, where, forced=None):
    """The rows and what the next finish_move would record, the move, what it did -- engine against model."""
    _same_rows(e, m, where)
    live = [not o for o in m.over]
    gamma, mixed, u = e.move_distribution()
    st0 = e.game_status()
    played = e.finish_move(forced_moves=forced).cpu().numpy().copy()
    events = m.finish_move(forced)
    st1, rs = e.game_status(), e.resign_status()
    for b in range(e.B):
        if not live[b]:
            assert played[b] == -1, (where, b)
            continue
        rec = m.last[b]
        if rec is None:                                          # adjudicated at the ply cap
            assert played[b] == -1 and st1["over"][b], (where, b)
            continue
        k = len(rec["acts"])
        assert mixed[b][:k].tobytes() == rec["pi64"].tobytes() and not mixed[b][k:].any(), (where, b)     # pi' in float64
        assert not gamma[b].any() and np.isnan(u[b]), (where, b)                                          # nothing is drawn
        assert played[b] == rec["move"], (where, b, played[b], rec["move"])
    got_events = []
    for b in range(e.B):
        if st0["over"][b]:
            got_events.append("over")
        elif st1["over"][b] and played[b] < 0 and (rs["state"][b] & rm.RESIGNED):
            got_events.append("resign")
        elif st1["over"][b] and played[b] < 0:
            got_events.append("cap")
        else:
            got_events.append("playon" if (rs["state"][b] & rm.PLAYON) and rs["fire_ply"][b] == st0["plies"][b] else None)
    rm.check_events(got_events, events, where)
    assert [bool(x) for x in st1["over"]] == list(m.over), where
    return played, rs


def _same_records(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        r, o = [int(x[0]) for x in np.nonzero(got != want)]
        raise AssertionError(f"record {r} (board id {got[r, 104:108].view(np.uint32)[0]}, ply {got[r, 96:98].view(np.uint16)[0]}) differs at "
                             f"byte {o}: {got[r, o]} != {want[r, o]}")


def _close(e, m, f):
    """The counters as the moves left them; one more simulation (every live root needs children) and a finish_move that adjudicates
    the running games at the ply cap; then the harvested records against the model's."""
    assert e.gumbel_stats() == m.gstats, (e.gumbel_stats(), m.gstats)
    sims = e.stats()["sims"]
    assert sims == m.sims, (sims, m.sims)
    e.select_leaves()
    info = e.leaf_info()
    sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
    P, V = np.zeros((e.B, 2086), np.float32), np.zeros(e.B, np.float32)
    for b in range(e.B):
        if info["status"][b] == EXPAND:
            P[b], V[b] = f(b, sq[b], turn[b])
    e.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
    e.finish_move()
    m.finish_move()
    assert e.game_status()["over"].all() and all(m.over)
    assert e.gumbel_stats() == m.gstats                          # a ply-cap adjudication records nothing
    rec = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
    e.check_healthy()
    assert e.stats()["pruned_subtrees"] == 0
    _same_records(rec, m.records(game_no=GAME_NO))
    return rec


# ---------------------------------------------------------------------------------------------------------------- 2, 3. the rule itself
@pytest.mark.parametrize("fused", [False, True], ids=["select_expand", "step"])
@pytest.mark.parametrize("evaluator", ["hash", "peaked"])
@pytest.mark.parametrize("setting", list(gm.SETTINGS))
def test_engine_equals_the_model(setting, evaluator, fused):
    m, f = gm.case(setting, evaluator)
    cfg = gm.SETTINGS[setting]
    e = _engine(gm.inputs(), cfg["n_sims"], gm.MOVES)
    e.set_gumbel(**cfg)
    for mv in range(gm.MOVES):
        _lockstep(e, m, f, cfg["n_sims"], fused, (setting, evaluator, mv))
        _boundary(e, m, (setting, evaluator, mv))
    assert m.gfacts["kept_n0"] > 0 and m.gfacts["target_gt0"] > 0 and m.gstats["offvisit_moves"] > 0
    rec = _close(e, m, f)
    if evaluator == "peaked":                                    # the recorded target follows the logits: far from uniform
        k = int(rec[0, 102])
        assert rec[0, 368:368 + 4 * k].view(np.float32).max() > 0.3


# ---------------------------------------------------------------------------------------------------------------- 4. odd roots
@functools.lru_cache(maxsize=None)
def _odd_positions():
    """(squares, turn) x 3: 98 legal moves (the first of cache_collision_cases' ``wide_equal_count`` pair: children 64.. exist), a
    double check with two king moves (m = k = 2 below max_considered) and a check with one legal move (k = 1: the sequence 0, 1, 2 ..)."""
    import rules_kat
    from cache_collision_cases import pairs
    wide = pairs()["wide_equal_count"][0]
    by_name = {c["name"]: c for c in rules_kat.cases()}
    out = [(np.asarray(wide[0], np.uint8)[:90].copy(), int(wide[1]))]
    for name in ("double_check_only_the_king_moves", "king_cannot_capture_a_protected_piece"):
        sq, turn, _ = rules_kat.start_of(by_name[name])
        out.append((sq, turn))
    ks = [len(OracleBoard.from_array(sq, t).legal_ids()) for sq, t in out]
    assert ks == [98, 2, 1], ks
    return tuple(out)


def test_roots_with_98_two_and_one_children():
    pos = _odd_positions()
    cfg = dict(n_sims=120, max_considered=16, c_visit=50.0, c_scale=1.0)
    f = gm.peaked_evaluator(gm.SALTS)
    m = gm.GumbelModel([OracleBoard.from_array(sq, t) for sq, t in pos], gm.SALTS, gm.SEED, gm.BASE, gumbel=cfg, max_plies=2,
                       evaluator=lambda b, board: f(b, board.squares(), int(board.turn)))
    e = _engine(pos, cfg["n_sims"], 2)
    e.set_gumbel(**cfg)
    # budgets: the wide board searches 120 simulations, the narrow ones 12 -- set on both sides
    budgets = np.array([120, 12, 12], np.int32)
    for mv in range(2):
        e.set_budgets(budgets)
        m.begin_move(budgets)
        _lockstep(e, m, f, 120, True, ("odd", mv))
        if mv == 0:
            rc = e.root_children()
            assert rc["k"].tolist() == [98, 2, 1]
            g, logit, n0, k, n_eff = e.gumbel_root()
            assert k.tolist() == [98, 2, 1] and n_eff.tolist() == [119, 11, 11]
            assert rc["visits"][2][0] == 11                                   # k = 1: every simulation goes to the one child
            assert sorted(rc["visits"][1][:2].tolist()) == [5, 6]             # m = 2, seq(2, 11) = 0 0 1 1 .. 4 4 5: the two take turns
        _boundary(e, m, ("odd", mv))
    assert m.gfacts["hi_choice"] > 0                                          # a child of index >= 64 was chosen at the root
    e.set_budgets(None)
    m.budget = [None] * m.B
    _close(e, m, f)


# ---------------------------------------------------------------------------------------------------------------- 5. budgets
def test_budgets_of_playout_cap_randomisation_set_n_eff():
    from budget_twin import twin_budgets
    cfg = gm.SETTINGS["n32_m16"]
    m, f = gm.case("n32_m16", "hash", cap=(32, 8, 0.5), max_plies=2)
    e = _engine(gm.inputs(), 32, 2)
    e.set_gumbel(**cfg)
    for mv in range(2):
        drawn = e.draw_budgets(32, 8, 0.5).cpu().numpy().copy()
        want = m.begin_move()
        assert drawn.tolist() == want and (mv > 0 or set(want) == {32, 8})
        if mv == 0:
            assert drawn.tolist() == twin_budgets(gm.SEED, gm.BASE, gm.B, 0, 32, 8, 0.5).tolist()
        seen = {}

        def rows(i, mv=mv, seen=seen):
            if i == 1:                                           # every root is expanded and has its row
                seen["n_eff"] = _same_rows(e, m, ("budgets", mv, i))
        _lockstep(e, m, f, 32, True, ("budgets", mv), after_step=rows)
        n_eff = seen["n_eff"]
        for b in range(gm.B):
            if not m.over[b]:
                assert n_eff[b] == want[b] - (1 if mv == 0 else 0), (mv, b)   # a fresh root has spent one simulation on its expansion
        _boundary(e, m, ("budgets", mv))
    rec = _close(e, m, f)
    fast = rec[:, 103] & 1
    assert fast.any() and not fast.all()                          # fast plies are flagged as before; their pi' is recorded all the same
    for r in rec[fast == 1]:
        k = int(r[102])
        assert abs(float(r[368:368 + 4 * k].view(np.float32).sum()) - 1.0) < 1e-5


def test_the_fallback_past_n_eff():
    cfg = gm.SETTINGS["n32_m16"]
    m, f = gm.case("n32_m16", "peaked", max_plies=1)
    e = _engine(gm.inputs(), 40, 1)
    e.set_gumbel(**cfg)
    _lockstep(e, m, f, 40, True, "fallback")                      # 40 steps against n_sims = 32: the last 9 take the most visited
    assert m.gfacts["fallback"] >= 8 * gm.B
    _boundary(e, m, "fallback")
    _close(e, m, f)


# ---------------------------------------------------------------------------------------------------------------- 6. resignation
def test_resignation_reads_the_counts_as_searched():
    rule = rm.Rule(-0.03, 1, 0, 0.5)
    cfg = dict(n_sims=24, max_considered=8, c_visit=50.0, c_scale=1.0)
    pos = spm.inputs()
    f = gm.hash_evaluator(spm.SALTS)
    m = gm.GumbelModel(spm.boards(), spm.SALTS, gm.SEED, gm.BASE, gumbel=cfg, resign=rule, max_plies=3,
                       evaluator=lambda b, board: f(b, board.squares(), int(board.turn)))
    e = _engine(pos, 24, 3)
    e.set_gumbel(**cfg)
    e.set_resign(threshold=rule.threshold, consecutive=rule.consecutive, min_ply=rule.min_ply, p_playon=rule.p_playon)
    for mv in range(3):
        _lockstep(e, m, f, 24, True, ("resign", mv))
        _, rs = _boundary(e, m, ("resign", mv))
        for b in range(e.B):
            w = m.games[b].status()
            assert int(rs["state"][b]) == w["state"] and tuple(int(x) for x in rs["run"][b]) == w["run"], (mv, b)
            assert int(rs["fire_ply"][b]) == w["fire_ply"] and rm.same_f32(rs["last_value"][b], w["last_value"]), (mv, b)
    assert m.xfacts["resign"] > 0 and m.xfacts["playon"] > 0
    _close(e, m, f)
    assert {k: int(v) for k, v in e.resign_stats().items() if k in rm.STAT_KEYS} == m.resign_stats()


# ---------------------------------------------------------------------------------------------------------------- 7. the solver
def test_the_solver_stops_under_the_gumbel_root():
    name, sq, turn, *_ = sc.CASES[sc.NAMES.index("mate_in_two")]
    cfg = dict(n_sims=48, max_considered=16, c_visit=50.0, c_scale=1.0)
    salts = (sc.SALTS[0],)
    f = gm.hash_evaluator(salts)
    m = gm.GumbelModel([OracleBoard.from_array(sq, turn)], salts, gm.SEED, gm.BASE, gumbel=cfg, solver=True, max_plies=2,
                       evaluator=lambda b, board: f(b, board.squares(), int(board.turn)))
    e = _engine([(sq, turn)], 48, 2)
    e.set_gumbel(**cfg)
    e.set_solver(True)

    def proofs(where):
        rp = e.root_proof()
        st, ds, cs, cd = m.root_proof(0)
        k = len(cs)
        assert (rp["state"][0], rp["dist"][0]) == (st, ds), (where, rp["state"][0], rp["dist"][0], st, ds)
        assert np.array_equal(rp["child_state"][0][:k], cs) and np.array_equal(rp["child_dist"][0][:k], cd), where
    for mv in range(2):
        if m.over[0]:
            break
        _lockstep(e, m, f, 48, mv == 1, ("solver", mv), after_step=lambda i, mv=mv: proofs((mv, i)))
        assert e.solver_stats() == m.solver_stats()
        _boundary(e, m, ("solver", mv))
    assert m.nodes_proven > 0 and m.proven_stops > 0 and m.xfacts["stops_d1"]   # a chosen root child was proven: the descent ended there
    _close(e, m, f)


# ---------------------------------------------------------------------------------------------------------------- 8. off means untouched
def test_turned_on_and_off_again_is_the_engine_that_never_heard_of_it():
    f = gm.hash_evaluator(gm.SALTS)

    def run(toggle):
        e = _engine(gm.inputs(), 16, 3)
        if toggle:
            e.set_gumbel(16, max_considered=4)
            e.set_gumbel(None)
        out = {"moves": []}
        for mv in range(3):
            e.select_leaves()
            planes = []
            for i in range(16):
                info = e.leaf_info()
                pl = e.leaf_input.float().cpu().numpy()
                planes.append(pl.tobytes())
                sq, turn = planes_to_squares(pl)
                P, V = np.zeros((e.B, 2086), np.float32), np.zeros(e.B, np.float32)
                for b in range(e.B):
                    if info["status"][b] == EXPAND:
                        P[b], V[b] = f(b, sq[b], turn[b])
                tp, tv = torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV)
                (e.step if i + 1 < 16 else e.expand_backup)(tp, tv)
            rc = e.root_children()
            dist = e.move_distribution()
            rows = e.gumbel_root()
            out["moves"].append({"planes": planes, "roots": rc, "dist": dist, "rows": rows, "played": e.finish_move().cpu().numpy().copy()})
        out["gstats"], out["stats"] = e.gumbel_stats(), e.stats()
        e.select_leaves()
        e.expand_backup(torch.zeros((e.B, 2086), device=DEV), torch.zeros(e.B, device=DEV))
        e.finish_move()
        out["records"] = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
        e.check_healthy()
        return out

    a, b = run(True), run(False)
    for ma, mb in zip(a["moves"], b["moves"]):
        assert ma["planes"] == mb["planes"]                       # every leaf input of every step
        for key in ("k", "acts", "visits", "q", "prior", "root_visits"):
            assert ma["roots"][key].tobytes() == mb["roots"][key].tobytes(), key
        for x, y in zip(ma["dist"], mb["dist"]):
            assert x.tobytes() == y.tobytes()
        assert ma["dist"][0].any() and not np.isnan(ma["dist"][2]).any()       # the sampler's Gamma draws and choice uniform: PUCT's move
        assert not ma["rows"][3].any() and not mb["rows"][3].any()            # no row was ever filled
        assert np.array_equal(ma["played"], mb["played"])
    _same_records(a["records"], b["records"])
    assert a["stats"] == b["stats"]
    assert a["gstats"] == b["gstats"] == {"gumbel_moves": 0, "considered_sum": 0, "offvisit_moves": 0}


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals():
    from chinesechesszero_amd._lib import CczError
    from chinesechesszero_amd.engine import SelfPlayEngine
    from chinesechesszero_amd.net import uniform_evaluator
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    e = SelfPlayEngine(4, n_playout=8, eval_cache_log2=10)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(n_sims=0), dict(n_sims=-3), dict(n_sims=8, max_considered=1), dict(n_sims=8, max_considered=129),
                dict(n_sims=8, c_visit=-1.0), dict(n_sims=8, c_visit=inf), dict(n_sims=8, c_visit=nan),
                dict(n_sims=8, c_scale=-0.5), dict(n_sims=8, c_scale=inf), dict(n_sims=8, c_scale=nan)):
        with pytest.raises(CczError, match="ccz_set_gumbel"):
            e.set_gumbel(**bad)
    L, s = e.L, e._stream()
    for args in ((0, 0, 16, 50.0, 1.0), (0, 8, 1, 50.0, 1.0), (0, 8, 16, nan, 1.0), (0, 8, 16, 50.0, -1.0)):   # validated when off, too
        assert L.ccz_set_gumbel(e.h, s, *args) != 0
    e.set_gumbel(8, max_considered=2, c_visit=0.0, c_scale=0.0)     # the edges of the ranges are allowed
    e.set_gumbel(8, max_considered=128)
    with pytest.raises(CczError, match="Gumbel"):
        e.set_scouts(2)
    with pytest.raises(CczError, match="Gumbel"):
        e.set_root_exploration(0.25)
    e.set_root_exploration(None)                                   # turning the other off is always allowed
    e.set_gumbel(None)
    e.set_scouts(2)
    with pytest.raises(CczError, match="scout"):
        e.set_gumbel(8)
    e.set_gumbel(None)
    e.set_scouts(0)
    e.set_root_exploration(0.25)
    with pytest.raises(CczError, match="root exploration"):
        e.set_gumbel(8)
    e.set_root_exploration(None)
    e.set_gumbel(8)
    e.check_healthy()
    with pytest.raises(ValueError, match="gumbel"):
        BatchedSelfPlay(uniform_evaluator, 4, n_playout=8, sampling="numpy", gumbel=True)
    with pytest.raises(ValueError, match="gumbel"):
        BatchedSelfPlay(uniform_evaluator, 4, n_playout=8, gumbel=dict(max_considered=4), root_exploration=dict(eps=0.25))
    sp = BatchedSelfPlay(uniform_evaluator, 4, n_playout=8, gumbel=True)
    assert sp.gumbel == {"n_sims": 8}


# ---------------------------------------------------------------------------------------------------------------- 10. BatchedSelfPlay
def test_batched_self_play_planned_equals_dense():
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    from test_gpu_selfplay_all_options import HashLogits
    n, moves = 16, 2

    def run(cache):
        sp = BatchedSelfPlay(HashLogits(), spm.B, n_playout=n, seed=gm.SEED, board_id_base=gm.BASE, max_plies=moves, eval_cache_log2=cache,
                             gumbel=dict(max_considered=8), playout_cap=(4, 0.5))
        assert sp.planned == (cache > 0) and sp.gumbel["n_sims"] == n
        e = sp.engine
        sq = np.stack([s for s, _ in spm.inputs()]).astype(np.uint8)
        assert (e.set_positions(sq, np.array([t for _, t in spm.inputs()], np.uint8)) == 0).all()
        played = [sp.run_move().cpu().numpy().copy() for _ in range(moves)]
        gstats, stats = e.gumbel_stats(), e.stats()
        sp.simulate()
        e.finish_move()
        assert e.game_status()["over"].all()
        rec = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
        e.check_healthy()
        return played, gstats, stats, rec

    pa, ga, sa, ra = run(14)
    pb, gb, sb, rb = run(0)
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    assert ga == gb and ga["gumbel_moves"] >= spm.B and sa["sims"] == sb["sims"]
    _same_records(ra, rb)
    fast = ra[:, 103] & 1
    assert fast.any() and not fast.all()
    assert sa["cache_probes"] > 0 and sb["cache_probes"] == 0
