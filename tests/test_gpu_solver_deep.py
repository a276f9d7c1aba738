"""GPU: the MCTS-solver on the two paths that no hash-evaluated position reaches (fixtures and the model's recorded runs:
tests/solver_deep_cases.py; what makes them mean something is asserted on the CPU by tests/test_cpu_solver_deep.py).

A. Proof walks of 64 and more plies: the mate at depth 63 (all path nodes in lanes: the control), 64, 65 and 67, and a sixty-move DRAW
   leaf at depth 66, five boards in lockstep on both dense sequences, compared with the model simulation by simulation; then the whole
   line is walked by forced moves, so that every deep node shows its N, Q, P and proof byte as the root or a root child.
B. A proven node that a pruning re-root leaves without children becomes the root, is expanded again under its WIN byte, has the byte
   withdrawn by its first DRAW child and proven again by the capture line."""
import numpy as np
import pytest
import torch

import solver_deep_cases as dc
import solver_model as sm
from gpu_harness import planes_to_squares

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def deep():
    return dc.deep_trace()


def _engine(cases, solver=True, strict=True, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(len(cases), n_playout=64, seed=5, strict=strict, **kw)
    for b, (sq, turn, half) in enumerate(cases):
        e.set_position(b, sq.copy(), turn, half)
    if solver:
        e.set_solver(True)
    return e


def _rows(e, script, boards, by_depth=True):
    """(P [B,2086], V [B]) of the scripted evaluator on the engine's pending leaves, as device tensors."""
    sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
    info = e.leaf_info()
    P = np.zeros((e.B, 2086), np.float32)
    for j, b in enumerate(boards):
        if info["status"][j] == sm.LEAF_EXPAND:
            P[j] = script.row(b, sq[j], turn[j], int(info["depth"][j]) if by_depth else 0)
    return info, torch.from_numpy(P).to(DEV), torch.zeros(e.B, dtype=torch.float32, device=DEV)


def _same_leaves(info, want, names, i):
    for j, w in enumerate(want):
        assert (info["status"][j], info["k"][j], info["depth"][j]) == w, (names[j], i, w)


def _same_tops(e, tops, stats, names, at, skip=()):
    """Root children (N, Q bits, P bits), root visits, proof bytes, the proof move and the solver's counters against the model's."""
    rc, rp, pm = e.root_children(), e.root_proof(), e.proof_moves()
    for j, t in enumerate(tops):
        if j in skip:
            continue
        k, who = len(t["acts"]), (names[j], at)
        assert rc["k"][j] == k and np.array_equal(rc["acts"][j][:k], t["acts"].astype(np.uint16)), who
        assert np.array_equal(rc["visits"][j][:k], t["N"]), who
        assert np.array_equal(rc["q"][j][:k].view(np.uint32), t["Q"].view(np.uint32)), who
        assert np.array_equal(rc["prior"][j][:k].view(np.uint32), t["P"].view(np.uint32)), who
        assert rc["root_visits"][j] == t["root_n"], who
        assert (rp["state"][j], rp["dist"][j]) == t["proof"], (who, rp["state"][j], rp["dist"][j], t["proof"])
        assert np.array_equal(rp["child_state"][j][:k], t["cs"]) and np.array_equal(rp["child_dist"][j][:k], t["cd"]), who
        assert not rp["child_state"][j][k:].any() and not rp["child_dist"][j][k:].any(), who
        assert pm[j] == t["pm"], who
    assert e.solver_stats() == stats, at


def _deep_engine(boards=None, solver=True):
    boards = range(dc.B) if boards is None else boards
    return _engine([(dc.SQUARES, dc.CASES[b][2], dc.CASES[b][3]) for b in boards], solver=solver, max_nodes=dc.MAX_NODES,
                   reserve_nodes=dc.RESERVE_NODES, max_depth=dc.MAX_DEPTH)


def _walk_the_line(e, t):
    """Every line node becomes the root in turn: forced moves with the tree kept, against the model's re-roots."""
    for s, moves in enumerate(t.moves):
        e.finish_move(forced_moves=np.array(moves, np.int32), keep_tree=True)
        over = e.game_status()["over"]
        assert [bool(x) for x in over] == t.over[s], s
        _same_tops(e, t.walk_tops[s], t.walk_stats[s], dc.NAMES, ("move", s), skip=[b for b in range(dc.B) if t.over[s][b]])
    assert all(t.over[-1])


# ---------------------------------------------------------------------------------------------------------------- A: deep walks
def test_deep_proof_walks_select_and_expand_backup(deep):
    t, sc = deep, dc.script()
    e = _deep_engine()
    for i, want in enumerate(t.leaves):
        e.select_leaves()
        info, P, V = _rows(e, sc, range(dc.B))
        _same_leaves(info, want, dc.NAMES, i)
        e.expand_backup(P, V)
        if i >= dc.FORK or i % 64 == 0:                  # (before the first decided leaf the solver has nothing to show)
            _same_tops(e, t.tops[i], t.stats[i], dc.NAMES, i)
    st = e.stats()
    assert st["depth_peak"] >= 67 and st["pruned_subtrees"] == 0 and st["sims"] == dc.B * len(t.leaves)
    assert st["expansions"] == t.counters["rows"] and st["terminal_leaves"] == t.counters["sims"] - t.counters["rows"]
    _walk_the_line(e, t)
    e.check_healthy()


def test_deep_proof_walks_fused_step(deep):
    t, sc = deep, dc.script()
    e = _deep_engine()
    e.select_leaves()
    n = len(t.leaves)
    for i, want in enumerate(t.leaves):
        info, P, V = _rows(e, sc, range(dc.B))
        _same_leaves(info, want, dc.NAMES, i)
        if i + 1 < n:
            e.step(P, V)
        else:
            e.expand_backup(P, V)
        if i >= dc.FORK:
            _same_tops(e, t.tops[i], t.stats[i], dc.NAMES, i)
    assert e.stats()["expansions"] == t.counters["rows"] and e.stats()["pruned_subtrees"] == 0
    _walk_the_line(e, t)
    e.check_healthy()


def test_deep_line_with_the_solver_off_is_the_oracles_search():
    """The control: the d = 65 board without the solver is the reference's search (the oracle's, step by step) and the solver-off
    model's, the mate is walked into again and again, and no proof byte appears."""
    from oracle import OracleMCTS
    b, sc = 2, dc.script()
    t = dc.deep_trace(solver=False, only=b)
    e = _deep_engine([b], solver=False)
    board = dc.boards()[b]
    o = OracleMCTS(None, c_puct=5, n_playout=0)
    e.select_leaves()
    n = len(t.leaves)
    for i, want in enumerate(t.leaves):
        info, P, V = _rows(e, sc, [b])
        _same_leaves(info, want, [dc.NAMES[b]], i)
        leaf, depth = o.select(board)
        ids = leaf.legal_ids()
        assert depth == info["depth"][0] and len(ids) == info["k"][0]
        o.expand_backup(leaf, ids, sc.row(b, leaf.squares(), int(leaf.turn), depth)[ids], 0.0)
        if i + 1 < n:
            e.step(P, V)
        else:
            e.expand_backup(P, V)
    assert sum(1 for r in t.leaves if r[0][:1] + r[0][2:] == (sm.LEAF_LOSS, 65)) > 1
    zero = {"nodes_proven": 0, "proven_stops": 0, "roots_proven": 0}
    _same_tops(e, t.tops[-1], zero, [dc.NAMES[b]], "end")
    acts, N, Q, _ = o.root_children()
    rc = e.root_children()
    assert np.array_equal(rc["visits"][0][:len(acts)], N) and np.array_equal(rc["q"][0][:len(acts)].view(np.uint32), Q.view(np.uint32))
    assert not any(v.any() for v in e.root_proof().values())
    e.check_healthy()


# ---------------------------------------------------------------------------------------------------------------- B: withdrawal
def _certified(board, moves, state, dist):
    b = board.copy()
    for mv in moves:
        b.push_id(int(mv))
    exact = sm.certify(b, 3)
    return exact != 0 and sm.state_of(exact) == state and (state == sm.DRAW or dist >= sm.dist_of(exact))


def _no_false_proof(e, board, pre):
    rc, rp = e.root_children(), e.root_proof()
    if rp["state"][0]:
        assert _certified(board, pre, rp["state"][0], rp["dist"][0]), pre
    for a, s, d in zip(rc["acts"][0][:rc["k"][0]], rp["child_state"][0], rp["child_dist"][0]):
        if s:
            assert _certified(board, list(pre) + [int(a)], s, d), (pre, a)


@pytest.mark.parametrize("fused", [False, True], ids=["expand_backup", "step"])
def test_pruned_proven_root_is_withdrawn_and_proven_again(fused):
    t, sc, p = dc.prune_trace(), dc.prune_script(), dc.PRUNE
    ids = sc.ids[0]
    e = _engine([(p["squares"], p["turn"], p["halfmove"])], strict=False, max_nodes=p["max_nodes"], reserve_nodes=p["reserve_nodes"])
    root, name = dc.prune_board(), ["prune"]

    def search(lo, hi, pre):
        e.select_leaves()
        for i in range(lo, hi):
            info, P, V = _rows(e, sc, [0], by_depth=False)
            _same_leaves(info, t.leaves[i], name, i)
            if fused and i + 1 < hi:
                e.step(P, V)
            else:
                e.expand_backup(P, V)
                if i + 1 < hi:
                    e.select_leaves()
            _same_tops(e, t.tops[i], t.stats[i], name, i)
            _no_false_proof(e, root, pre)

    search(0, t.reroot_at, [])
    assert e.stats()["pruned_subtrees"] == 0
    for j, (mv, top, stats, pruned, kept) in enumerate(t.reroots):
        e.finish_move(forced_moves=np.array([mv], np.int32), keep_tree=True)
        _same_tops(e, [top], stats, name, ("re-root", j))
        assert e.stats()["pruned_subtrees"] == pruned, j
        _no_false_proof(e, root, ids[:j + 1])
    rp = e.root_proof()
    assert (rp["state"][0], rp["dist"][0]) == (sm.WIN, 3) and e.root_children()["k"][0] == 0 and e.proof_moves()[0] == -1
    search(t.reroot_at, len(t.leaves), ids[:2])
    assert t.withdrawn_at is not None and t.reproven_at is not None            # (what was compared above, by name)
    rp = e.root_proof()
    assert (rp["state"][0], rp["dist"][0]) == (sm.WIN, 3) and e.proof_moves()[0] == ids[2]
    assert e.stats()["pruned_subtrees"] == t.reroots[-1][3] == 6
    e.check_healthy()
