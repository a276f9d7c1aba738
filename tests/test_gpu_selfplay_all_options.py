"""GPU: self-play with every search option on at once -- budgets drawn by playout-cap randomisation, root exploration, the
MCTS-solver, resignation with play-on -- against the one sequential model of tests/selfplay_model.py. Exact, no tolerance anywhere:
visits, Q and prior bits, proof bytes, the noise table, leaf status / k / depth, moves, resignation state and events, the counters
and the harvested records byte for byte.

Inputs (selfplay_model.inputs): 16 boards -- the seven solver fixtures, seven opening positions, `pawns` and `wide_late_mate` (105
legal moves, the only mating move at child 67: the root's WIN exists only if the second 64-lane pass of proof_backup's combine and of
the selection's proof-byte load work) --, 96 or 24 simulations a move by the Philox lot, three moves with tree reuse, a ply cap of 3.
tests/test_cpu_selfplay_model.py asserts on the model alone that every interaction occurs on these inputs and that each of them,
stated wrongly, gives other records or roots.

Launch forms: select_leaves + expand_backup and the fused dense step (the ``hash`` evaluator's priors as they are); the production
sequence of BatchedSelfPlay.advance with an evaluation cache (draw_budgets, eval_plan, gather_priors_planned, step_compact), where
the model is handed the priors as the device forms them (``DevicePriors`` of tests/test_gpu_solver.py); BatchedSelfPlay itself
against that directly driven engine; every option turned on and off again against an engine that never heard of them.

The last test is a property, not a model equality: with a node pool so tight that a re-root prunes a subtree that carries proof bytes, whatever proof the engine
reports at the top of a tree is certified by ``solver_model.negamax`` on the position."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import explore_model as em
import resign_model as rm
import selfplay_model as spm
import solver_cases as sc
import solver_model as sm
from gpu_harness import planes_to_squares
from oracle import OracleBoard
from test_gpu_solver import DevicePriors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N = spm.B, spm.N_FULL
GAME_NO = 2             # the record header's count of games started on a slot: ccz_create starts the first, the load below the second
OPTIONS = dict(playout_cap=(spm.N_FAST, spm.P_FULL),
               resign=dict(threshold=spm.RULE.threshold, consecutive=spm.RULE.consecutive, min_ply=spm.RULE.min_ply, p_playon=spm.RULE.p_playon),
               root_exploration=dict(eps=spm.EXPLORE["eps"], alpha=None, forced_k=spm.EXPLORE["forced_k"], prune_targets=spm.EXPLORE["prune"]),
               solver=True)


# ---------------------------------------------------------------------------------------------------------------- engines and evaluators
def _load(e):
    sq = np.stack([s for s, _ in spm.inputs()]).astype(np.uint8)
    turn = np.array([t for _, t in spm.inputs()], np.uint8)
    status = e.set_positions(sq, turn)
    assert (status == 0).all(), status
    return e


def _engine(cache=0, options=True):
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(B, n_playout=N, seed=spm.SEED, board_id_base=spm.BASE, max_plies=spm.MOVES, eval_cache_log2=cache)
    if options:
        e.set_root_exploration(**OPTIONS["root_exploration"])
        e.set_solver(True)
        e.set_resign(**OPTIONS["resign"])
    return _load(e)


def _hash_rows(leaf_input, rows=None):
    """(P [n,2086], V [n]) of the hash evaluator on rows of the leaf planes (a row without a fresh leaf holds an older one: unused)."""
    sq, turn = planes_to_squares(leaf_input.float().cpu().numpy())
    rows = range(len(sq)) if rows is None else rows
    PV = [em.evaluate_sq(spm.SALTS, 0, sq[b], turn[b]) for b in rows]
    return np.stack([p for p, _ in PV]) if PV else np.zeros((0, 2086), np.float32), np.array([v for _, v in PV], np.float32)


class HashLogits:
    """The hash evaluator as a stateless device evaluator that returns LOGITS (log P, float32) and accepts a plan: what the
    production sequence and BatchedSelfPlay are handed, so that both see the same bits."""
    batched = returns_logits = accepts_plan = stateless = True

    def __call__(self, leaf, plan=None):
        n_rows = leaf.shape[0]
        lg = torch.zeros((n_rows, 2086), dtype=torch.float32, device=leaf.device)
        vv = torch.zeros((n_rows,), dtype=torch.float32, device=leaf.device)
        if plan is None:
            idx = np.arange(n_rows)
        else:
            rows, n = plan
            idx = rows[:int(n.item())].cpu().numpy()
        if len(idx):
            P, V = _hash_rows(leaf, idx)
            lg[:len(idx)] = torch.from_numpy(np.log(P.astype(np.float32))).to(leaf.device)
            vv[:len(idx)] = torch.from_numpy(V).to(leaf.device)
        return lg.contiguous(), vv.contiguous()


# ---------------------------------------------------------------------------------------------------------------- driving and reading
def _events(st0, st1, rs, moves):
    out = []
    for b in range(B):
        if st0["over"][b]:
            out.append("over")
        elif st1["over"][b] and moves[b] < 0 and (rs["state"][b] & rm.RESIGNED):
            out.append("resign")
        elif st1["over"][b] and moves[b] < 0:
            out.append("cap")
        else:
            out.append("playon" if (rs["state"][b] & rm.PLAYON) and rs["fire_ply"][b] == st0["plies"][b] else None)
    return out


def _boundary(e, finish):
    """Read the tops of the trees, play the move through ``finish()``, read what it did."""
    st0 = e.game_status()
    top = {"roots": e.root_children(), "proofs": e.root_proof(), "noise": e.root_noise(), "sstats": e.solver_stats()}
    moves = finish().cpu().numpy().copy()
    st1, rs = e.game_status(), e.resign_status()
    top.update(moves=moves, events=_events(st0, st1, rs, moves), resign_status=rs, over=st1["over"].copy())
    return top


def _close(e, one_more_step):
    """The counters as the three moves left them; then one more simulation (every live root needs children) and a finish_move that
    adjudicates the running games at the ply cap, the resignation counters and the harvest."""
    out = {"xstats": e.exploration_stats(), "sstats": e.solver_stats(), "stats": e.stats()}
    one_more_step()
    e.finish_move()
    assert e.game_status()["over"].all()
    out["rstats"] = e.resign_stats()
    out["records"] = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
    e.check_healthy()
    assert e.stats()["pruned_subtrees"] == 0
    return out


def _dense_step(e):
    e.select_leaves()
    P, V = _hash_rows(e.leaf_input)
    e.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))


def _drive_dense(e, fused, leaves=None):
    """Three moves through a dense launch form with budgets by the device's lot. ``leaves(move, step, info)``: called with
    ccz_leaf_info of every pending leaf batch (the unfused form)."""
    out = {"moves": [], "budgets": []}
    for mv in range(spm.MOVES):
        out["budgets"].append(e.draw_budgets(spm.N_FULL, spm.N_FAST, spm.P_FULL).cpu().numpy().copy())
        e.select_leaves()
        for i in range(N):
            if leaves is not None:
                leaves(mv, i, e.leaf_info())
            P, V = _hash_rows(e.leaf_input)
            tp, tv = torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV)
            if fused and i + 1 < N:
                e.step(tp, tv)
            else:
                e.expand_backup(tp, tv)
                if i + 1 < N:
                    e.select_leaves()
        out["moves"].append(_boundary(e, e.finish_move))
    out.update(_close(e, lambda: _dense_step(e)))
    return out


def _planned_step(e, ev, last, digest=None):
    if digest is not None:
        digest.update(e.leaf_input.cpu().numpy().tobytes())
    lg, v = ev(e.leaf_input, plan=e.eval_plan())
    e.gather_priors_planned(lg, v)
    if last:
        e.expand_backup_compact(None)
    else:
        e.step_compact(None)


def _drive_production(e, steps=N, draw=True, digest=None):
    """BatchedSelfPlay.advance's launch sequence, written out: draw_budgets, select_leaves, (eval_plan, logits of the planned rows,
    gather_priors_planned, step_compact) x (n - 1), ..., expand_backup_compact, finish_move."""
    ev = HashLogits()
    out = {"moves": [], "budgets": []}
    for mv in range(spm.MOVES):
        if draw:
            out["budgets"].append(e.draw_budgets(spm.N_FULL, spm.N_FAST, spm.P_FULL).cpu().numpy().copy())
        e.select_leaves()
        for i in range(steps):
            _planned_step(e, ev, i + 1 == steps, digest)
        out["moves"].append(_boundary(e, e.finish_move))

    def one_more():
        e.select_leaves()
        _planned_step(e, ev, True)
    out.update(_close(e, one_more))
    return out


# ---------------------------------------------------------------------------------------------------------------- comparison
def _same_records(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        r, o = [int(x[0]) for x in np.nonzero(got != want)]
        raise AssertionError(f"record {r} (board id {got[r, 104:108].view(np.uint32)[0]}, ply {got[r, 96:98].view(np.uint16)[0]}) differs at "
                             f"byte {o}: {got[r, o]} != {want[r, o]}")


def _check_model(run, model_run):
    m, moves = model_run
    for mv, (got, want) in enumerate(zip(run["moves"], moves)):
        assert np.array_equal(run["budgets"][mv], np.array(want["budgets"], np.int32)), mv
        rc, rp, (noise, noise_k) = got["roots"], got["proofs"], got["noise"]
        for b in range(B):
            if not want["live"][b]:
                continue
            acts, visits, q, prior = want["roots"][b]
            k = len(acts)
            assert rc["k"][b] == k and np.array_equal(rc["acts"][b][:k], acts.astype(np.uint16)), (mv, b)
            assert np.array_equal(rc["visits"][b][:k], visits), (mv, b, rc["visits"][b][:k], visits)
            assert np.array_equal(rc["q"][b][:k].view(np.uint32), q.view(np.uint32)), (mv, b)
            assert np.array_equal(rc["prior"][b][:k].view(np.uint32), prior.view(np.uint32)), (mv, b)
            st, ds, cs, cd = want["proofs"][b]
            assert (rp["state"][b], rp["dist"][b]) == (st, ds), (mv, b, rp["state"][b], rp["dist"][b], st, ds)
            assert np.array_equal(rp["child_state"][b][:k], cs) and np.array_equal(rp["child_dist"][b][:k], cd), (mv, b)
            assert not rp["child_state"][b][k:].any() and not rp["child_dist"][b][k:].any()
            row = want["noise"][b]
            assert noise_k[b] == len(row), (mv, b, noise_k[b], len(row))
            assert np.array_equal(noise[b][:len(row)].view(np.uint32), row.view(np.uint32)) and not noise[b][len(row):].any(), (mv, b)
            f = want["finish"][b]
            assert got["moves"][b] == (f["move"] if f is not None else -1), (mv, b, got["moves"][b], f and f["move"])
        assert got["sstats"] == want["sstats"], (mv, got["sstats"], want["sstats"])    # roots_proven: the running games' roots
        rm.check_events(got["events"], want["events"], mv)
        for b in range(B):
            w = want["status"][b]
            rs = got["resign_status"]
            assert int(rs["state"][b]) == w["state"] and tuple(int(x) for x in rs["run"][b]) == w["run"], (mv, b)
            assert int(rs["fire_ply"][b]) == w["fire_ply"] and rm.same_f32(rs["last_value"][b], w["last_value"]), (mv, b)
        assert [bool(x) for x in got["over"]] == want["over"], mv
    assert run["xstats"] == m.totals(), (run["xstats"], m.totals())
    assert run["sstats"] == m.closing_sstats, (run["sstats"], m.closing_sstats)
    assert {k: int(run["rstats"][k]) for k in rm.STAT_KEYS} == m.resign_stats(), (run["rstats"], m.resign_stats())
    st = run["stats"]
    assert st["sims"] == m.sims == sum(mv["budgets"][b] for mv in moves for b in range(B) if mv["live"][b])
    assert st["expansions"] == m.rows and st["terminal_leaves"] == m.sims - m.rows
    _same_records(run["records"], m.records(game_no=GAME_NO))


# ---------------------------------------------------------------------------------------------------------------- 1. dense forms
@pytest.mark.parametrize("fused", [False, True], ids=["select_expand", "step"])
def test_dense_forms_equal_the_model(fused):
    model = spm.dense_run()
    seen = {"skip": 0, "stop": 0}

    def leaves(mv, i, info):
        for b, (status, k, depth) in enumerate(model[1][mv]["steps"][i]):
            if status == spm.LEAF_SKIP:
                assert info["status"][b] == spm.LEAF_SKIP, (mv, i, b)
                seen["skip"] += 1
            else:
                assert (info["status"][b], info["k"][b], info["depth"][b]) == (status, k, depth), (mv, i, b)
                seen["stop"] += status != sm.LEAF_EXPAND and k == 0
    run = _drive_dense(_engine(), fused, None if fused else leaves)
    _check_model(run, model)
    assert fused or (seen["skip"] > 0 and seen["stop"] > 0)


# ---------------------------------------------------------------------------------------------------------------- 2. the production sequence
@functools.lru_cache(maxsize=None)
def _compact_model():
    """The model on device-formed priors; the facts about the wide board hold for it as for the dense one."""
    m = spm.all_on(evaluator=DevicePriors())
    moves = spm.run(m)
    spm.close(m)
    st, ds, cs, _ = moves[0]["proofs"][spm.WIDE]
    assert (st, ds) == (sm.WIN, 1) and np.nonzero(cs)[0].tolist() == [67] and (spm.WIDE, 0, 67) in m.xfacts["stops_d1"]
    assert m.xfacts["forced_on_proven"] and m.xfacts["pruned_at_proven_root"] and m.xfacts["resign"] and m.xfacts["playon"]
    return m, moves


@functools.lru_cache(maxsize=None)
def _production_run():
    return _drive_production(_engine(cache=14))


def test_the_production_sequence_equals_the_model():
    run = _production_run()
    m, _ = model = _compact_model()
    _check_model(run, model)
    st = run["stats"]
    assert st["cache_probes"] == m.rows and st["cache_hits"] + st["cache_shared_rows"] > 0


# ---------------------------------------------------------------------------------------------------------------- 3. BatchedSelfPlay
def test_batched_self_play_is_the_directly_driven_engine():
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay(HashLogits(), B, n_playout=N, seed=spm.SEED, board_id_base=spm.BASE, max_plies=spm.MOVES, eval_cache_log2=14, **OPTIONS)
    assert sp.planned
    e = _load(sp.engine)
    moves = [sp.run_move().cpu().numpy().copy() for _ in range(spm.MOVES)]
    got = _close(e, sp.simulate)
    want = _production_run()
    for mv in range(spm.MOVES):
        assert np.array_equal(moves[mv], want["moves"][mv]["moves"]), mv
    for key in ("xstats", "sstats", "rstats"):
        assert got[key] == want[key], key
    assert got["stats"]["sims"] == want["stats"]["sims"] and got["stats"]["cache_probes"] == want["stats"]["cache_probes"]
    _same_records(got["records"], want["records"])


# ---------------------------------------------------------------------------------------------------------------- 4. off means off
def test_every_option_turned_on_and_off_again_is_the_engine_that_never_heard_of_them():
    steps = 32

    def run(toggle):
        from chinesechesszero_amd.engine import SelfPlayEngine
        e = SelfPlayEngine(B, n_playout=N, seed=spm.SEED, board_id_base=spm.BASE, max_plies=spm.MOVES, eval_cache_log2=14)
        if toggle:
            e.set_root_exploration(**OPTIONS["root_exploration"])
            e.set_solver(True)
            e.set_resign(**OPTIONS["resign"])
            e.draw_budgets(spm.N_FULL, spm.N_FAST, spm.P_FULL)
            e.set_root_exploration(None)
            e.set_solver(False)
            e.set_resign(None)
            e.set_budgets(None)
        digest = hashlib.sha256()
        out = _drive_production(_load(e), steps=steps, draw=False, digest=digest)
        out["digest"] = digest.hexdigest()
        return out

    a, b = run(True), run(False)
    assert a["digest"] == b["digest"]                                    # every leaf input of every step
    for ma, mb in zip(a["moves"], b["moves"]):
        for key in ("k", "acts", "visits", "q", "prior", "root_visits"):
            assert ma["roots"][key].tobytes() == mb["roots"][key].tobytes(), key
        assert np.array_equal(ma["moves"], mb["moves"]) and ma["events"] == mb["events"]
        assert not any(v.any() for v in ma["proofs"].values()) and not ma["noise"][1].any()
    _same_records(a["records"], b["records"])
    assert (a["records"][:, 90:96] == 0).all() and (a["records"][:, 103] == 0).all()   # no value, no flag
    grown = a["stats"].pop("hbm_bytes") - b["stats"].pop("hbm_bytes")
    assert grown > 0                                                     # (the proof bytes the first set_solver(True) allocated)
    assert a["stats"] == b["stats"] and a["stats"]["sims"] == steps * sum(int(not o) for m in [np.zeros(B)] + [x["over"] for x in a["moves"][:-1]] for o in m)
    zero = {"xstats": dict.fromkeys(a["xstats"], 0), "sstats": dict.fromkeys(a["sstats"], 0), "rstats": dict.fromkeys(a["rstats"], 0)}
    for key, z in zero.items():
        assert a[key] == b[key] == z, key


# ---------------------------------------------------------------------------------------------------------------- 5. a re-root that prunes
# 64 simulations a move leave the wide board's root unproven at its first move (the mate is child 67), so its game goes on: the reply's
# kept subtree (a few hundred nodes, proven children among them) exceeds the 129 nodes a re-root may keep here -- the smallest the
# engine allows: the pool (8192 >= 129 + 64 expansions of up to 105 children) keeps the rest free --, and the second re-root prunes
PRUNE_SIMS, PRUNE_CAP, PRUNE_KEPT, PRUNE_MOVES = 64, 8192, 129, 4


def _certified(board, state, dist, where):
    """The claim (state, dist) about ``board``'s position against the exhaustive negamax: decided in ``dist`` plies means that a
    negamax of that depth decides it, the same way and no later. A draw carries no distance: the negamax deepens until it decides."""
    if state == sm.DRAW:
        # draws are proven here only in the bare endings of `forced_draw` / `capture_to_bare` (at most 6 pieces, under 10 moves a
        # position), where 6 plies cost a few thousand nodes; a draw claimed anywhere else gets 2 plies and fails if that is not enough
        ref = sm.certify(board, 6 if np.count_nonzero(board.squares()) <= 6 else 2)
        assert sm.state_of(ref) == sm.DRAW, (where, "draw", ref, "0 here may also mean: a true draw beyond the referee's depth, not a false proof")
        return
    ref = sm.negamax(board, int(dist))
    assert sm.state_of(ref) == state, (where, state, dist, ref)
    assert dist >= sm.dist_of(ref), (where, dist, sm.dist_of(ref))


def test_proofs_stay_true_across_re_roots_that_prune():
    from chinesechesszero_amd.engine import SelfPlayEngine
    from golden_cases import STARTS, WIDTHS
    cases = [(n, sq, t) for n, sq, t, *_ in sc.CASES] + [(spm.WIDE_NAME, STARTS[spm.WIDE_NAME], WIDTHS[spm.WIDE_NAME][0])]
    n = len(cases)
    e = SelfPlayEngine(n, n_playout=PRUNE_SIMS, seed=5, max_nodes=PRUNE_CAP, reserve_nodes=PRUNE_CAP - PRUNE_KEPT)
    boards = []
    for b, (_, sq, turn) in enumerate(cases):
        e.set_position(b, sq.copy(), turn, 0)
        boards.append(OracleBoard.from_array(sq, turn))
    e.set_solver(True)
    checked = {"root": 0, "child": 0, "after_prune": 0}

    def check(where):
        rp, rc, over = e.root_proof(), e.root_children(), e.game_status()["over"]
        pm = e.proof_moves()
        pruned = e.stats()["pruned_subtrees"] > 0
        for b in range(n):
            if over[b]:
                continue
            ids = boards[b].legal_ids()
            k = int(rc["k"][b])
            assert k in (0, len(ids)) and rc["acts"][b][:k].tolist() == ids[:k], (where, b)
            assert pm[b] == -1 or int(pm[b]) in ids, (where, b, pm[b])
            if rp["state"][b]:
                _certified(boards[b], int(rp["state"][b]), int(rp["dist"][b]), (where, cases[b][0], "root"))
                checked["root"] += 1
            for i in np.nonzero(rp["child_state"][b][:k])[0]:
                c = boards[b].copy()
                c.push_id(ids[i])
                _certified(c, int(rp["child_state"][b][i]), int(rp["child_dist"][b][i]), (where, cases[b][0], "child", int(i)))
                checked["child"] += 1
                checked["after_prune"] += pruned
        e.check_healthy()
        return pm, rc, over

    for mv in range(PRUNE_MOVES):
        for _ in range(PRUNE_SIMS):
            e.select_leaves()
            sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
            PV = [em.evaluate_sq((sc.SALTS[0],) * n, 0, sq[b], turn[b]) for b in range(n)]
            e.expand_backup(torch.from_numpy(np.stack([p for p, _ in PV])).to(DEV), torch.from_numpy(np.array([v for _, v in PV], np.float32)).to(DEV))
        pm, rc, over = check(("search", mv))
        forced = np.full(n, -1, np.int32)
        for b in range(n):
            if not over[b]:
                k = int(rc["k"][b])
                forced[b] = pm[b] if pm[b] >= 0 else int(rc["acts"][b][int(np.argmax(rc["visits"][b][:k]))])
        e.finish_move(forced_moves=forced)
        for b in range(n):
            if forced[b] >= 0:
                boards[b].push_id(int(forced[b]))
        if mv == 1:                                         # two more moves of search follow
            assert e.stats()["pruned_subtrees"] > 0
            rp = e.root_proof()                             # the pruned tree carries proof bytes: its root and one of its children
            assert rp["state"][n - 1] == sm.WIN and rp["child_state"][n - 1].any() and e.root_children()["k"][n - 1] > 64
        check(("move", mv))
    assert checked["root"] > 0 and checked["child"] > 0 and checked["after_prune"] > 0, checked
