"""GPU: the MCTS-solver (ccz_set_solver) against its CPU model (tests/solver_model.py), on the certified fixtures of
tests/solver_cases.py -- one per board, 7 boards x 26 simulations per run.

The dense paths (select_leaves + expand_backup, the fused step) take the ``hash`` evaluator's priors as they are and are compared
with the model bit for bit, simulation by simulation. The compact paths (planned boundary, scouts with ccz_scouted_run) form their
priors on the device (exp(log_softmax) of the logits); there the model is handed the priors of a position as the device forms them
(a one-board engine that gathers the same logits row), so that the comparison stays exact."""
import functools

import numpy as np
import pytest
import torch

import solver_cases as sc
import solver_model as sm
from gpu_harness import make_evaluator, planes_to_squares
from test_cpu_solver_model import combine_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = len(sc.CASES)


def _engine(n_boards=B, cases=None, solver=True, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(n_boards, n_playout=64, seed=5, strict=True, **kw)
    for b, (_, sq, turn, *_) in enumerate(sc.CASES if cases is None else cases):
        e.set_position(b, sq.copy(), turn, 0)
    if solver:
        e.set_solver(True)
    return e


def _hash_rows(e, n=None):
    """(P [n,2086], V [n]) of the hash evaluator on the engine's leaf planes (a row without a fresh leaf holds an older one: unused)."""
    n = e.B if n is None else n
    sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
    return make_evaluator("hash", [sc.SALTS[0]] * n)(sq[:n], turn[:n])


def _same_top(e, m, n=B):
    """Root children (N, Q bits, P bits), root proofs and counters of the engine against the model."""
    rc, rp = e.root_children(), e.root_proof()
    for b in range(n):
        acts, N, Q, P = m.root_children(b)
        k = len(acts)
        assert rc["k"][b] == k and np.array_equal(rc["acts"][b][:k], acts.astype(np.uint16)), sc.NAMES[b]
        assert np.array_equal(rc["visits"][b][:k], N), (sc.NAMES[b], rc["visits"][b][:k], N)
        assert np.array_equal(rc["q"][b][:k].view(np.uint32), Q.view(np.uint32)), sc.NAMES[b]
        assert np.array_equal(rc["prior"][b][:k].view(np.uint32), P.view(np.uint32)), sc.NAMES[b]
        assert rc["root_visits"][b] == m.roots[b].N
        st, ds, cs, cd = m.root_proof(b)
        assert (rp["state"][b], rp["dist"][b]) == (st, ds), (sc.NAMES[b], rp["state"][b], rp["dist"][b], st, ds)
        assert np.array_equal(rp["child_state"][b][:k], cs) and np.array_equal(rp["child_dist"][b][:k], cd), sc.NAMES[b]
        assert not rp["child_state"][b][k:].any() and not rp["child_dist"][b][k:].any()
    assert e.solver_stats() == m.stats()


def _same_leaves(e, m):
    """One simulation of every model board against the engine's pending leaves: status (LEAF_WIN included), k, path length."""
    info = e.leaf_info()
    expands = 0
    for b in range(B):
        status, k, depth = m.simulate(b)
        assert (info["status"][b], info["k"][b], info["depth"][b]) == (status, k, depth), (sc.NAMES[b], m.sims)
        expands += status == sm.LEAF_EXPAND
    return expands


# ---------------------------------------------------------------------------------------------------------------- combine
def test_proof_combine_is_the_models_combine():
    from chinesechesszero_amd.engine import proof_combine
    cases = combine_cases()
    got = proof_combine([c for c, _ in cases])
    want = np.array([sm.combine(c) for c, _ in cases], np.uint8)
    assert np.array_equal(want, np.array([w for _, w in cases], np.uint8))
    assert np.array_equal(got, want), [(len(cases[i][0]), int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0]]
    assert any(len(c) > 64 and c[64] != c[0] for c, _ in cases) and any(len(c) == 128 and c[127] != c[0] for c, _ in cases)
    assert proof_combine([[]])[0] == 0


# ---------------------------------------------------------------------------------------------------------------- dense paths
@functools.lru_cache(maxsize=None)
def _dense_model():
    m = sm.SolverModel(sc.boards(), sc.SALTS)
    return m


def test_select_and_expand_backup_follow_the_model_simulation_by_simulation():
    e = _engine()
    m = sm.SolverModel(sc.boards(), sc.SALTS)
    rows = 0
    for _ in range(sc.SIMS):
        e.select_leaves()
        rows += _same_leaves(e, m)
        P, V = _hash_rows(e)
        e.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
        _same_top(e, m)
    assert rows == m.rows < m.sims and m.proven_stops > 0
    rp = e.root_proof()
    for b, (name, _, _, state, dist, *_) in enumerate(sc.CASES):       # what the negamax certified, within the budgets
        assert (rp["state"][b], rp["dist"][b]) == (state, dist), name
    st = e.stats()
    assert st["sims"] == B * sc.SIMS and st["terminal_leaves"] == m.sims - m.rows and st["expansions"] == m.rows
    e.check_healthy()


def test_fused_dense_step_follows_the_model():
    e = _engine()
    m = sm.SolverModel(sc.boards(), sc.SALTS)
    e.select_leaves()
    for i in range(sc.SIMS):
        _same_leaves(e, m)
        P, V = _hash_rows(e)
        tp, tv = torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV)
        if i + 1 < sc.SIMS:
            e.step(tp, tv)
        else:
            e.expand_backup(tp, tv)
    _same_top(e, m)
    assert e.stats()["expansions"] == m.rows
    e.check_healthy()


# ---------------------------------------------------------------------------------------------------------------- compact paths
class DevicePriors:
    """evaluator(b, board) of the model for the compact paths: the hash evaluator's logits row of the position, turned into priors by
    the device's own gather (a one-board engine whose root is the position)."""

    def __init__(self):
        from chinesechesszero_amd.engine import SelfPlayEngine
        self.e = SelfPlayEngine(1, n_playout=8, seed=1)
        self.ev = make_evaluator("hash", [sc.SALTS[0]])
        self.memo = {}

    def logits(self, P):
        return torch.from_numpy(np.log(P.astype(np.float32))).to(DEV).contiguous()

    def __call__(self, b, board):
        sq, turn = board.squares(), int(board.turn)
        key = (sq.tobytes(), turn)
        if key not in self.memo:
            P, V = self.ev(sq[None, :], np.array([turn], np.uint8))
            self.e.set_position(0, sq, turn, 0)
            self.e.select_leaves()
            self.e.gather_priors(self.logits(P), torch.from_numpy(V).to(DEV))
            pri, _ = self.e.leaf_priors(values=False)
            ids = board.legal_ids()
            info = self.e.leaf_info()
            assert info["ids"][0][:len(ids)].tolist() == ids
            row = np.zeros(2086, np.float32)
            row[ids] = pri[0][:len(ids)]
            self.memo[key] = (row, V[0])
        return self.memo[key]


@pytest.fixture(scope="module")
def device_priors():
    return DevicePriors()


@pytest.fixture(scope="module")
def compact_model(device_priors):
    """The model after SIMS simulations of every fixture on device-formed priors: shared by the planned and the scouted run."""
    m = sm.SolverModel(sc.boards(), sc.SALTS, evaluator=device_priors)
    m.search(sc.SIMS)
    return m


def test_planned_boundary_follows_the_model(device_priors, compact_model):
    e = _engine(eval_cache_log2=14)
    e.select_leaves()
    for i in range(sc.SIMS):
        rows, n = e.eval_plan()
        n = int(n.cpu()[0])
        P, V = _hash_rows(e)
        idx = rows[:n].cpu().numpy()
        lg = torch.zeros((B, 2086), dtype=torch.float32, device=DEV)
        vv = torch.zeros((B,), dtype=torch.float32, device=DEV)
        if n:
            lg[:n] = device_priors.logits(P[idx])
            vv[:n] = torch.from_numpy(V[idx]).to(DEV)
        if i + 1 < sc.SIMS:
            e.step_planned(lg, vv)
        else:
            e.expand_backup_planned(lg, vv)
    m = compact_model
    _same_top(e, m)
    st = e.stats()
    assert st["cache_probes"] == m.rows == st["expansions"] and st["sims"] == B * sc.SIMS      # leaves that asked for the evaluator
    assert st["cache_hits"] + st["cache_shared_rows"] > 0                                       # (two fixtures share their position)
    e.check_healthy()


def test_scouted_run_follows_the_model(device_priors, compact_model):
    n_slots = 12
    e = _engine(n_slots, eval_cache_log2=14, solver=False)
    e.set_scouts(n_slots - B)
    e.set_solver(True)
    ev = make_evaluator("hash", [sc.SALTS[0]] * n_slots)

    def evaluate():
        sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
        P, V = ev(sq, turn)
        return device_priors.logits(P), torch.from_numpy(V).to(DEV)

    e.select_leaves()
    e.scout_and_plan()
    need = bool((e.plan_states() == 0).any())
    left, k, calls = sc.SIMS, 0, 0
    while left > 0:
        if need:
            e.gather_priors_planned(*evaluate())
            calls += 1
        e.set_run((3, 1, 1000, 7)[k % 4], left)
        k += 1
        e.scouted_run_launch()
        done, need = e.run_outcome()
        assert 1 <= done <= left
        left -= done
    m = compact_model
    _same_top(e, m)
    st = e.stats()
    assert st["sims"] == B * sc.SIMS and st["expansions"] == m.rows and 0 < calls < sc.SIMS
    e.check_healthy()


# ---------------------------------------------------------------------------------------------------------------- the move boundary
def _search_dense(e, m, sims, boards=None):
    for _ in range(sims):
        e.select_leaves()
        for b in (range(B) if boards is None else boards):
            m.simulate(b)
        P, V = _hash_rows(e)
        e.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))


def test_re_root_carries_the_proof_bytes():
    e = _engine()
    m = sm.SolverModel(sc.boards(), sc.SALTS)
    _search_dense(e, m, sc.SIMS)
    over = [False] * B
    for ply in range(2):                                  # the proven move (else the most visited one), then the reply to it
        moves = np.full(B, -1, np.int32)
        for b in range(B):
            if over[b] or not m.roots[b].kids:
                continue
            acts, N, _, _ = m.root_children(b)
            pm = m.proof_move(b)
            moves[b] = int(acts[int(np.argmax(N))]) if pm is None else pm
        e.finish_move(forced_moves=moves)
        for b in range(B):
            if moves[b] >= 0:
                m.update_with_move(b, int(moves[b]))
                over[b] = m.boards[b].is_game_over() or m.boards[b].is_tie()
        rc, rp, go = e.root_children(), e.root_proof(), e.game_status()["over"]
        live = 0
        for b in range(B):
            assert bool(go[b]) == over[b] or moves[b] < 0, (sc.NAMES[b], ply)
            if over[b] or moves[b] < 0:
                continue
            live += 1
            st, ds, cs, cd = m.root_proof(b)
            k = len(cs)
            assert rc["k"][b] == k and (rp["state"][b], rp["dist"][b]) == (st, ds), (sc.NAMES[b], ply)
            assert np.array_equal(rp["child_state"][b][:k], cs) and np.array_equal(rp["child_dist"][b][:k], cd), (sc.NAMES[b], ply)
        assert live >= 2
        if ply == 0:                                      # the child that was proven LOSS in 2 is the root now
            b = sc.NAMES.index("mate_in_two")
            assert (rp["state"][b], rp["dist"][b]) == (sm.LOSS, 2)
    e.check_healthy()


def test_a_fresh_root_is_unproven_and_a_reused_pool_starts_from_zero_bytes():
    e = _engine()
    m = sm.SolverModel(sc.boards(), sc.SALTS)
    _search_dense(e, m, sc.SIMS)
    assert e.root_proof()["state"][0] == sm.WIN
    mv = m.proof_move(0)
    e.finish_move(forced_moves=np.array([mv] + [m.proof_move(1)] + [-1] * (B - 2), np.int32), keep_tree=False)
    rp = e.root_proof()
    assert not rp["state"][:2].any() and not rp["child_state"][:2].any()        # keep_tree = False: nothing is carried over
    assert e.game_status()["over"][0]                                           # Ra7-a9 was mate: board 0 has finished its game
    e.reset_tree()
    assert not e.root_proof()["state"].any()
    # board 0's pool held a proven tree a moment ago; another fixture searched there starts from unknown bytes
    case = sc.CASES[sc.NAMES.index("mate_in_two")]
    e.set_position(0, case[1].copy(), case[2], 0)
    from oracle import OracleBoard
    m2 = sm.SolverModel([OracleBoard.from_array(case[1], case[2])], [sc.SALTS[0]])
    e2 = e
    for _ in range(case[6]):
        e2.select_leaves()
        status, k, depth = m2.simulate(0)
        info = e2.leaf_info()
        assert (info["status"][0], info["k"][0], info["depth"][0]) == (status, k, depth)
        P, V = _hash_rows(e2)
        e2.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
    rp = e2.root_proof()
    st, ds, cs, cd = m2.root_proof(0)
    assert (rp["state"][0], rp["dist"][0]) == (st, ds) == (case[3], case[4])
    assert np.array_equal(rp["child_state"][0][:len(cs)], cs) and np.array_equal(rp["child_dist"][0][:len(cd)], cd)


# ---------------------------------------------------------------------------------------------------------------- off
def test_off_is_byte_for_byte_the_engine_without_the_solver():
    from chinesechesszero_amd.engine import SelfPlayEngine
    cases = [sc.CASES[0], sc.CASES[2]]

    def run(toggle):
        e = SelfPlayEngine(2, n_playout=64, seed=11, max_plies=3, eval_cache_log2=0)
        if toggle:
            e.set_solver(True)
            e.set_solver(False)
        for b, (_, sq, turn, *_) in enumerate(cases):
            e.set_position(b, sq.copy(), turn, 0)
        out = {"leaf": [], "roots": [], "moves": []}
        ev = make_evaluator("hash", [3, 4])
        for _ in range(3):
            for _ in range(64):
                e.select_leaves()
                planes = e.leaf_input.cpu().numpy().copy()
                info = e.leaf_info()
                out["leaf"].append((planes.tobytes(), info["status"].tobytes(), info["k"].tobytes(), info["depth"].tobytes()))
                sq, turn = planes_to_squares(planes.astype(np.float32))
                P, V = ev(sq, turn)
                e.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
            rc = e.root_children()
            out["roots"].append(tuple(rc[k].tobytes() for k in ("k", "acts", "visits", "q", "prior", "root_visits")))
            out["moves"].append(e.finish_move().cpu().numpy().tobytes())
        e.select_leaves()                                 # (one more simulation: an expanded root, which finish_move asks for)
        sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
        P, V = ev(sq, turn)
        e.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
        e.finish_move()                                   # max_plies = 3: whatever is still running is adjudicated, so it can be harvested
        out["records"] = [r.cpu().numpy().tobytes() for r in e.harvest_record_chunks()]
        out["stats"] = e.stats()
        out["proof"] = e.root_proof()
        out["solver_stats"] = e.solver_stats()
        return out

    a, b = run(True), run(False)
    grown = a["stats"].pop("hbm_bytes") - b["stats"].pop("hbm_bytes")
    assert 0 < grown <= 2 * 2 * (64 + 64) * 512 + 4096      # the proof bytes the first set_solver(True) allocated: one per node
    for key in ("leaf", "roots", "moves", "records", "stats"):
        assert a[key] == b[key], key
    assert a["records"] and a["stats"]["terminal_leaves"] > 0            # the searches did reach decided positions
    for o in (a, b):
        assert not any(v.any() for v in o["proof"].values())
        assert o["solver_stats"] == {"nodes_proven": 0, "proven_stops": 0, "roots_proven": 0}


# ---------------------------------------------------------------------------------------------------------------- front-ends
def _policy():
    """The fixtures' evaluator in the reference's form (``f(board) -> (zip(ids, P[ids]), value)``): the search is the model's."""
    from oracle.evaluators import hash_eval

    def policy(board, red_states=None, black_states=None):
        ids = board.legal_ids()
        p, v = hash_eval(board.squares()[None, :], np.array([1 if board.turn else 0]), salt=sc.SALTS[0], scale=1.0)
        return zip(ids, p[0][ids]), np.array([[v[0]]], dtype=np.float32)

    return policy


def _fen(sq, turn):
    from chinesechesszero_amd.game import _SYMBOL_INV
    rows = []
    for r in range(9, -1, -1):
        row, gap = "", 0
        for f in range(9):
            pc = int(sq[f + 9 * r])
            if not pc:
                gap += 1
                continue
            row += (str(gap) if gap else "") + (_SYMBOL_INV[pc & 7].upper() if pc < 8 else _SYMBOL_INV[pc & 7])
            gap = 0
        rows.append(row + (str(gap) if gap else ""))
    return "/".join(rows) + (" w" if turn else " b")


def _uci_go(case, solver):
    import io
    from chinesechesszero_amd.uci import UciLoop
    out = io.StringIO()
    loop = UciLoop(policy_value_fn=_policy(), n_playout=case[6], out=out)
    for line in ["uci"] + (["setoption name Solver value true"] if solver else []) + [f"position fen {_fen(case[1], case[2])}", f"go nodes {case[6]}"]:
        assert loop.handle(line)
    return out.getvalue().splitlines()


def test_uci_says_mate_and_plays_the_proven_move():
    two, lost = sc.CASES[sc.NAMES.index("two_rooks")], sc.CASES[sc.NAMES.index("mated_in_two_plies")]
    text = _uci_go(two, True)
    assert "option name Solver type check default false" in text
    pv = [l.split() for l in text if l.startswith("info depth ")]
    assert len(pv) == 1 and pv[0][5:8] == ["score", "mate", "1"] and pv[0][-1] == "a7a9"
    assert [l for l in text if l.startswith("bestmove ")] == ["bestmove a7a9"]
    text = _uci_go(lost, True)
    pv = [l.split() for l in text if l.startswith("info depth ")]
    assert len(pv) == 1 and pv[0][5:8] == ["score", "mate", "-1"]
    assert [l for l in text if l.startswith("bestmove ")] == [f"bestmove {lost[7]}"]
    text = _uci_go(two, False)                               # off: as ever
    pv = [l.split() for l in text if l.startswith("info depth ")]
    assert len(pv) == 1 and pv[0][5:7] == ["score", "cp"] and not any("mate" in l for l in text)


def test_mcts_ai_plays_the_certified_move():
    from chinesechesszero_amd.game import Board, Move
    from chinesechesszero_amd.mcts import MCTS_AI
    for name in ("two_rooks", "mate_in_two", "mated_below"):
        case = sc.CASES[sc.NAMES.index(name)]
        ai = MCTS_AI(_policy(), c_puct=5, n_playout=case[6], solver=True)
        move = ai.get_action(Board(case[1].copy(), bool(case[2]), 0))
        assert Move.from_id(int(move)).uci() == case[7], name
        rp = ai.mcts.root_proof()
        assert (rp["state"], rp["dist"]) == (case[3], case[4]), name


def test_analysis_with_the_solver_reports_the_mate():
    import json
    from chinesechesszero_amd.analyse import BatchedAnalysis
    from chinesechesszero_amd.game import Board
    cases = [sc.CASES[sc.NAMES.index(n)] for n in ("two_rooks", "mated_in_two_plies", "capture_to_bare")]
    ev = make_evaluator("hash", [sc.SALTS[0]] * len(cases))

    def evaluator(leaf):
        sq, turn = planes_to_squares(leaf.float().cpu().numpy())
        P, V = ev(sq, turn)
        return torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV)

    for solver in (True, False):
        an = BatchedAnalysis(evaluator, len(cases), n_playout=sc.SIMS, solver=solver, eval_cache_log2=0)
        recs = [json.loads(json.dumps(r)) for r in an.analyse([Board(c[1].copy(), bool(c[2]), 0) for c in cases])]
        if solver:
            assert recs[0]["mate"] == 1 and recs[0]["bestmove"] == "a7a9"
            assert recs[1]["mate"] == -1 and recs[1]["lines"][0]["mate"] == -1
            assert recs[2]["mate"] is None and "mate" in recs[2]["lines"][0]
        else:
            assert all("mate" not in r and "mate" not in r["lines"][0] for r in recs)
