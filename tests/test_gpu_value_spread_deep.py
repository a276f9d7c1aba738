"""GPU: the value spread S (ccz_set_value_stats) where the backup and the re-root take their other paths, on the fixtures of
tests/solver_deep_cases.py with S kept beside the model's tree (value_spread_model.tracking):

- a path of 64 and more plies -- path nodes 64.. are not a lane's own: the backup loop reads them from the path in memory (its
  ``j >= 64`` round). The scripted-prior line at d = 63 (the control: every path node is a lane's) and at d = 65. The nodes at depth
  64 and 65 are seen when the line is walked by re-roots and they come to the top of the tree.
- a pruning re-root at the smallest kept budget (129 nodes): a node that loses its children keeps N, Q, P -- and its S.

Exact, no tolerance: N, Q bits and S bits of the root's children, N and S bits of the root."""
import numpy as np
import pytest

import solver_deep_cases as dc
import solver_model as sm
import value_spread_model as vsm
from test_gpu_solver_deep import _deep_engine, _engine, _rows, _same_leaves

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same_spread(e, j, want_N, want_Q, want_S, want_root_s, where):
    rc, vs = e.root_children(), e.root_value_stats()
    k = len(want_N)
    assert rc["k"][j] == k and np.array_equal(rc["visits"][j][:k], want_N), where
    assert np.array_equal(_bits(rc["q"][j][:k]), _bits(want_Q)), where
    assert np.array_equal(_bits(vs["S"][j][:k]), _bits(want_S)), (where, vs["S"][j][:k], want_S)
    assert not vs["S"][j][k:].view(np.uint32).any(), where
    assert _bits(vs["root_S"][j:j + 1])[0] == _bits([want_root_s])[0], (where, vs["root_S"][j], want_root_s)


@pytest.fixture(scope="module")
def deep_lines():
    """The solver-off model runs of the d = 63 and the d = 65 board, S kept beside the trees: {board: (trace, tracker)}."""
    dc._sims()                                   # (the lockstep run that fixes the number of simulations: not under the tracker)
    out = {}
    for b in (dc.NAMES.index("d63"), dc.NAMES.index("d65")):
        with vsm.tracking(sm, dc) as tr:
            out[b] = (dc.deep_trace.__wrapped__(solver=False, only=b), tr)
    return out


def test_paths_of_64_plies_and_more(deep_lines):
    sc = dc.script()
    bs = sorted(deep_lines)
    e = _deep_engine(bs, solver=False)
    e.set_value_stats(True)
    traces = [deep_lines[b][0] for b in bs]
    n = len(traces[0].leaves)
    assert all(len(t.leaves) == n for t in traces)
    e.select_leaves()
    deepest = [0, 0]
    for i in range(n):
        info, P, V = _rows(e, sc, bs)
        for j, t in enumerate(traces):
            _same_leaves({k: v[j:j + 1] for k, v in info.items()}, t.leaves[i], [dc.NAMES[bs[j]]], i)
            deepest[j] = max(deepest[j], int(info["depth"][j]))
        if i + 1 < n:
            e.step(P, V)
        else:
            e.expand_backup(P, V)
        if i % 97 == 0 or i + 40 >= n:
            for j, t in enumerate(traces):
                top = t.tops[i][0]
                _same_spread(e, j, top["N"], top["Q"], top["S"], top["root_S"], (dc.NAMES[bs[j]], i))
    assert deepest == [63, 65], deepest          # the control stays inside the lanes, the other board's paths hold nodes 64 and 65
    # the line walked by re-roots with the tree kept: every line node comes to the top, the nodes at depth 64 and 65 among them
    nodes = [t.roots[0] for t in traces]
    over = [False, False]
    seen_deep = 0
    for s in range(max(dc.DEPTHS[b] for b in bs)):
        mv = [-1 if over[j] else sc.ids[b][s] for j, b in enumerate(bs)]
        e.finish_move(forced_moves=np.array(mv, np.int32), keep_tree=True)
        st = e.game_status()["over"]
        for j, b in enumerate(bs):
            if over[j]:
                continue
            nodes[j] = next(c for c in nodes[j].kids if c.move == mv[j])
            over[j] = bool(st[j])
            if over[j]:
                continue
            tr = deep_lines[b][1]
            kids = nodes[j].kids or []
            S, root_s, _ = tr.top(nodes[j])
            _same_spread(e, j, np.array([c.N for c in kids], np.int32), np.array([c.Q for c in kids], np.float32), S, root_s,
                         (dc.NAMES[b], "move", s))
            seen_deep += int(s + 1 >= 64 and float(root_s) > 0.0)
    assert all(over) and seen_deep >= 1          # a node of depth >= 64 was the root, with the S the memory round gave it
    assert e.stats()["pruned_subtrees"] == 0
    e.check_healthy()


@pytest.mark.parametrize("fused", [False, True], ids=["expand_backup", "step"])
def test_s_travels_through_a_pruning_reroot(fused):
    with vsm.tracking(sm, dc):
        t = dc.prune_trace.__wrapped__()
    sc, p = dc.prune_script(), dc.PRUNE
    e = _engine([(p["squares"], p["turn"], p["halfmove"])], strict=False, max_nodes=p["max_nodes"], reserve_nodes=p["reserve_nodes"])
    e.set_value_stats(True)
    name = ["prune"]

    def same(top, where):
        _same_spread(e, 0, top["N"], top["Q"], top["S"], top["root_S"], where)

    def search(lo, hi):
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
            same(t.tops[i][0], i)

    search(0, t.reroot_at)
    assert e.stats()["pruned_subtrees"] == 0
    for j, (mv, top, stats, pruned, kept) in enumerate(t.reroots):
        e.finish_move(forced_moves=np.array([mv], np.int32), keep_tree=True)
        assert e.stats()["pruned_subtrees"] == pruned, j
        same(top, ("re-root", j))
    assert t.reroots[-1][3] == 6 and t.reroots[0][4] <= dc.PRUNE_BUDGET          # nodes were pruned, at the 129-node budget
    assert any(float(x) > 0.0 for r in t.reroots for x in list(r[1]["S"]) + [r[1]["root_S"]])      # ... and kept nodes carry a spread
    search(t.reroot_at, len(t.leaves))                                            # the pruned nodes are expanded again: S goes on from theirs
    e.check_healthy()
