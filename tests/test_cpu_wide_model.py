"""The NumPy model of the wide search (tests/wide_model.py) against a case computed by hand: width 2 on a root with three
children, c_puct = 2, priors (0.5, 0.25, 0.25), budget 5. Every score is written out below. No GPU.

Second half: the move boundary on a kept tree and the engine's limits (re-root, node pool, depth, NaN priors, nodes of more than 64
children) -- each rule once by hand, the inputs of tests/test_gpu_wide_limits.py meeting their conditions on the model alone, and each
rule stated wrongly (wide_model.WRONG) giving another result on those inputs."""
import math

import numpy as np

from wide_model import DRAW, EXPAND, LOSS, WideModel

f32 = np.float32
INF = math.inf


def _expand(ids, priors, value):
    return {"status": EXPAND, "ids": ids, "priors": [f32(p) for p in priors], "value": f32(value)}


def test_two_steps_at_width_two_by_hand():
    m = WideModel(1, 2, c_puct=2.0, budgets=[5])
    t = m.trees[0]
    # ---- the move's first selection: the root is its own leaf; the second descent arrives there too: a collision ends the batch
    assert m.select(0) == [0]
    assert m.collisions == 1 and t.F == [1] and m.pending[0][0] == [0] and m.pending[0][1] is None
    m.backup(0, {0: _expand([10, 20, 30], [0.5, 0.25, 0.25], 0.5)})
    assert t.F[0] == 0 and t.N[0] == 1 and t.Q[0] == f32(-0.5) and m.sims[0] == 1           # the leaf gets -v
    # ---- step 1
    trace = []
    assert m.select(0, trace=trace) == [0, 1]
    (j0, l0), (j1, l1) = trace
    assert (j0, l0) == (0, [(0, [INF, INF, INF])])                                          # all unvisited: the first one
    # second descent: root N + F = 1 + 1; child 0 carries one in-flight visit = one loss: Qe = (0 * 0 - 1) / 1
    want = -1.0 + float(f32(2.0) * f32(0.5)) * math.sqrt(2.0) / 2.0
    assert (j1, l1) == (1, [(0, [want, INF, INF])]) and abs(want - (-0.2928932188134524)) < 1e-15
    assert m.moves_of(0, 0) == [10] and m.moves_of(0, 1) == [20] and t.F == [2, 1, 1, 0] and m.full_steps == 1
    # ---- step 2, phase A in slot order: child 0 is a lost position for its side to move (leaf value -1), child 1 expands
    m.backup(0, {0: {"status": LOSS}, 1: _expand([40, 50], [0.5, 0.5], 0.25)})
    assert t.F == [0, 0, 0, 0, 0, 0] and m.sims[0] == 3
    assert t.N[:4] == [3, 1, 1, 0]
    assert t.Q[1] == f32(1.0) and t.Q[2] == f32(-0.25)
    q_root = f32(f32(-0.75) + f32(f32(f32(0.25) - f32(-0.75)) / f32(3)))                    # -0.5 -> -0.75 -> -0.41666666
    assert t.Q[0] == q_root and abs(float(q_root) + 0.41666666) < 1e-7
    # ---- step 2, phase B
    trace = []
    assert m.select(0, trace=trace) == [0, 1]
    (_, l0), (_, l1) = trace
    s3 = math.sqrt(3.0)
    assert l0 == [(0, [1.0 + 1.0 * s3 / 2.0, -0.25 + 0.5 * s3 / 2.0, INF])]                 # child 2 is unvisited
    # root N + F = 3 + 1; child 2 in flight: Qe = -1; child 0 (N 1, Q 1): 1 + 1 * 2 / 2; child 1: -0.25 + 0.5 * 2 / 2
    assert l1 == [(0, [2.0, 0.25, -0.5])]
    assert m.moves_of(0, 1) == [10]                                                          # the terminal node, F = 0: selected again
    assert t.F[:4] == [2, 1, 0, 1] and m.full_steps == 2 and m.budget_cuts == 0
    # ---- step 3: both are backed up; the budget of 5 is used: nothing is selected, nothing is in flight
    m.backup(0, {0: _expand([60], [1.0], 0.0), 1: {"status": LOSS}})
    assert m.sims[0] == 5 and m.select(0) == [] and m.inflight() == 0
    assert m.repeated_terminals() == 1 and t.N[1] == 2 and t.Q[1] == f32(1.0) and t.N[0] == 5
    acts, n, q, p = t.root_children()
    assert acts.tolist() == [10, 20, 30] and n.tolist() == [2, 1, 1] and p.tolist() == [0.5, 0.25, 0.25]
    assert t.pv() == [10]


def test_budget_cuts_a_batch_and_slots_are_numbered_by_board():
    m = WideModel(3, 2, c_puct=2.0, budgets=[1, 2, 4])
    assert [m.slot(r, j) for j in range(2) for r in range(3)] == [0, 1, 2, 3, 4, 5]
    for r in range(3):
        assert m.select(r) == [0]
        m.backup(r, {0: _expand([1, 2], [0.5, 0.5], 0.0)})
    assert m.budget_cuts == 1 and m.collisions == 2   # board 0 (budget 1): the budget ended its first batch before the collision could
    assert m.select(0) == []                           # budget 1: used up
    assert m.select(1) == [0] and m.budget_cuts == 2   # budget 2: one more leaf, then the budget ends the batch
    assert m.select(2) == [0, 1]
    m.backup(2, {0: {"status": DRAW}, 1: {"status": DRAW}})
    assert m.trees[2].N[0] == 3 and m.trees[2].Q[0] == f32(0.0)
    m.drop(1)
    assert m.inflight() == 0 and m.sims[1] == 0


def test_with_no_flight_the_score_is_the_sequential_one():
    m = WideModel(1, 2, c_puct=5.0)
    t = m.trees[0]
    m.select(0)
    m.backup(0, {0: _expand([1, 2], [0.3, 0.7], 0.1)})
    t.N[1], t.Q[1], t.N[0] = 4, f32(0.2), 7
    got = t.score(0, 1, 5.0)
    want = float(f32(0.2)) + float(f32(5.0) * f32(0.3)) * np.sqrt(np.float64(7)) / np.float64(5)
    assert got == float(want)


def test_the_chosen_inputs_meet_the_conditions_on_the_cpu():
    """The inputs and budgets of tests/test_gpu_wide_search.py under a float64 restatement of the test evaluator: at every width the
    model sees a collision, a terminal leaf selected twice, a full batch and a batch cut by the budget."""
    import oracle
    import wide_model as wm
    for W in (2, 5, 16):
        roots = [oracle.OracleBoard.from_array(sq, turn) for sq, turn in wm.model_inputs()]
        m = wm.run_on_cpu(roots, W, list(wm.BUDGETS))
        assert all(wm.conditions(m).values()), (W, wm.conditions(m))
        assert m.sims == list(wm.BUDGETS) and m.inflight() == 0


# =========================================================================================================================
# The rules of the move boundary and of the engine's limits (wide_model.reroot, max_nodes, max_depth, NaN priors, nodes of more
# than 64 children): each once by hand, then on the inputs of tests/test_gpu_wide_limits.py, then stated wrongly.
import functools

import pytest

import wide_model as wm

NAN = float("nan")


def _roots(inputs):
    import oracle
    return [oracle.OracleBoard.from_array(sq, turn) for sq, turn in inputs]


def _signature(m):
    """Everything the GPU test compares at the end: the trees node by node, the counts and the counters."""
    return ([(t.N, [np.float32(q).view(np.uint32) for q in t.Q], [np.float32(p).view(np.uint32) for p in t.P], t.move, t.kids) for t in m.trees],
            m.sims, m.leaves, m.board_steps, m.collisions)


def test_reroot_by_hand():
    m = WideModel(1, 2, c_puct=2.0, budgets=[5])
    t = m.trees[0]
    m.select(0)
    m.backup(0, {0: _expand([10, 20, 30], [0.5, 0.25, 0.25], 0.5)})
    m.select(0)
    m.backup(0, {0: _expand([40, 50], [0.75, 0.25], -0.5), 1: _expand([60], [1.0], 0.25)})
    assert m.select(0) == [0, 1] and m.moves_of(0, 0) == [30] and m.moves_of(0, 1) == [10, 40] and m.inflight() == 5 and m.sims[0] == 3
    assert t.N[:4] == [3, 1, 1, 0] and t.n_nodes() == 7
    # ---- the boundary, two leaves pending: they leave F; child 10 (N 1, Q 0.5, P 0.5, two children) becomes the tree
    m.reroot(0, 10)
    k = m.trees[0]
    assert m.inflight() == 0 and m.sims[0] == 0 and m.pending[0] == [None, None]
    assert (k.N, k.Q, k.P, k.move, k.kids) == ([1, 0, 0], [f32(0.5), f32(0), f32(0)], [f32(0.5), f32(0.75), f32(0.25)], [10, 40, 50], [[1, 2], None, None])
    assert k.n_nodes() == 3                                     # (what k_finish_move leaves in BoardMeta.n_nodes)
    # ---- the budget counts from zero; the kept visit counts in sqrt(N + F)
    trace = []
    assert m.select(0, trace=trace) == [0, 1]
    assert trace[1] == (1, [(0, [-1.0 + float(f32(2.0) * f32(0.75)) * math.sqrt(2.0) / 2.0, INF])])
    assert m.moves_of(0, 0) == [40] and m.moves_of(0, 1) == [50] and m.inflight() == 4
    # ---- a child that was never expanded (nor visited: its pending leaf is dropped): a bare root with its own N, Q and P
    m.reroot(0, 50)
    b = m.trees[0]
    assert (b.N, b.Q, b.P, b.move, b.kids) == ([0], [f32(0.0)], [f32(0.25)], [50], [None]) and m.inflight() == 0 and m.sims[0] == 0
    assert m.select(0) == [0] and m.pending[0][0] == [0]         # the root is its own leaf again


def test_node_pool_by_hand():
    """max_nodes 6: the root's 3 children fit (1 + 3), a leaf with 3 children does not (4 + 3 > 6), the next slot's 2 do (4 + 2)."""
    m = WideModel(1, 2, c_puct=2.0, budgets=[9], max_nodes=6)
    t = m.trees[0]
    m.select(0)
    m.backup(0, {0: _expand([10, 20, 30], [0.5, 0.25, 0.25], 0.5)})
    assert m.select(0) == [0, 1]
    m.backup(0, {0: _expand([40, 50, 60], [0.5, 0.25, 0.25], 1.0), 1: _expand([70, 80], [0.5, 0.5], 0.25)})
    assert m.refused == [1] and m.fit_after_refusal == 1 and m.error_flags() == 1
    assert t.kids[1] is None and t.kids[2] == [4, 5] and t.n_nodes() == 6
    assert t.N[:3] == [3, 1, 1] and t.Q[1] == f32(-1.0) and m.sims[0] == 3      # the refused leaf's value is backed up, the simulation counts
    # ---- child 30 is unvisited: slot 0; slot 1: root N + F = 4, scores (-1 + 1 * 2 / 2, -0.25 + 0.5 * 2 / 2, -1 + 0.5 * 2 / 2):
    # child 20, then its first unvisited child
    assert m.select(0) == [0, 1] and m.moves_of(0, 0) == [30] and m.moves_of(0, 1) == [20, 70]
    m.backup(0, {0: _expand([90], [1.0], 0.75), 1: {"status": DRAW}})
    assert m.refused == [2] and t.n_nodes() == 6                                  # 6 + 1 > 6
    # ---- the refused leaf 10 (N 1, Q -1, no children) is selected again when its score wins, as a leaf
    t.Q[1] = f32(1.0)
    assert m.select(0)[0] == 0 and m.moves_of(0, 0) == [10] and m.refused_again == 1


def test_depth_limit_by_hand():
    """max_depth 2: paths hold 2 entries, leaves lie at depth <= 1; a descent that would write a third entry selects nothing."""
    m = WideModel(1, 3, c_puct=2.0, budgets=[9], max_depth=2)
    m.select(0)
    m.backup(0, {0: _expand([10, 20], [0.5, 0.5], 0.0)})
    assert m.select(0) == [0, 1]
    m.backup(0, {0: _expand([30], [1.0], 0.0), 1: _expand([40], [1.0], 0.0)})
    assert m.depth_stops == [0]
    # both children are expanded: the first descent goes root -> 10 -> 30, three entries
    assert m.select(0) == [] and m.depth_stops == [1] and m.empty_steps_after_stop == 1 and m.inflight() == 0 and m.error_flags() == 2
    # ---- a stop after a leaf: child 20 unexpanded again (by hand), child 10 made unattractive
    t = m.trees[0]
    t.kids[2] = None
    t.Q[1] = f32(-0.5)
    # slot 0: (-0.5 + 1 * sqrt(3) / 2, 0 + 1 * sqrt(3) / 2): 20. Slot 1: 20 carries a loss in flight, (-0.5 + 1 * 2 / 2, -0.5 + 1 * 2 / 3):
    # 10 wins and is too deep
    assert m.select(0) == [0] and m.moves_of(0, 0) == [20]
    assert m.depth_stops == [2] and m.stops_after_leaves == 1 and m.inflight() == 2 and m.pending[0][0] == [0, 2]


def test_nan_priors_by_hand():
    m = WideModel(1, 4, c_puct=2.0, budgets=[9])
    m.select(0)
    m.backup(0, {0: _expand([10, 20], [NAN, NAN], 0.5)})
    # unvisited children score +inf whatever their prior: slots 0 and 1; slot 2 finds (NaN, NaN): nothing compares, the batch ends
    trace = []
    assert m.select(0, trace=trace) == [0, 1] and m.nan_stops == [1] and m.stops_after_leaves == 1 and m.inflight() == 4
    assert trace[0][1] == [(0, [INF, INF])] and trace[1][1][0][1][1] == INF and all(math.isnan(s) for s in trace[2][1][0][1])
    m.backup(0, {0: {"status": DRAW}, 1: {"status": DRAW}})
    assert m.select(0) == [] and m.nan_stops == [2] and m.empty_steps_after_stop == 1 and m.sims[0] == 3 and m.error_flags() == 32
    assert m.trees[0].root_children()[1].tolist() == [1, 1]


def test_the_first_maximum_across_index_64_by_hand():
    """A root with 70 equal children: descents take them in child order, through index 64; with visits only on the first 66 the
    maximum (+inf) lies at index 66; a tie of finite scores between index 3 and index 67 goes to 3."""
    m = WideModel(1, 2, c_puct=2.0, budgets=[999])
    t = m.trees[0]
    m.select(0)
    m.backup(0, {0: _expand(list(range(100, 170)), [1.0 / 70] * 70, 0.0)})
    for step in range(33):
        assert m.select(0) == [0, 1] and [m.moves_of(0, j) for j in (0, 1)] == [[100 + 2 * step], [101 + 2 * step]]
        m.backup(0, {0: {"status": DRAW}, 1: {"status": DRAW}})
    assert m.upper_selected == 2 and m.ties_across_64 == 64      # 64 descents saw +inf on both sides of index 64 and took the lower
    assert m.select(0) == [0, 1] and m.moves_of(0, 0) == [166] and m.upper_selected == 4
    m.backup(0, {0: {"status": DRAW}, 1: {"status": DRAW}})
    for i in range(69, 71):
        t.N[i] = 1                                               # all 70 visited once, Q 0, equal priors: equal scores everywhere
    assert m.select(0)[0] == 0 and m.moves_of(0, 0) == [100]
    m.drop(0)
    # ---- the two mistakes a 64-lane kernel can make here (node i + 1 is child i)
    t.N[1:4] = [2, 2, 2]                                         # children 0 .. 2 score lower: the maximum is attained at 3 .. 69
    assert t.descend(2.0)[1] == 4 and t.descend(2.0, wrong="upper_children_ignored")[1] == 4
    assert t.descend(2.0, wrong="per_pass_maximum")[1] == 65     # lane 0 holds children 0 and 64, and 64 is a maximum: the lowest LANE wins
    t.N[4:65] = [2] * 61                                         # ... at 64 .. 69 only
    assert t.descend(2.0)[1] == 65 and t.descend(2.0, wrong="upper_children_ignored")[1] == 1
    t.N[65:68] = [2] * 3                                         # ... at 67 .. 69: lanes 3 .. 5 of the second pass
    t.N[5] = 1                                                   # and at index 4 (lane 4 of the first pass): child order says 4
    assert t.descend(2.0)[1] == 5 and t.descend(2.0, wrong="per_pass_maximum")[1] == 68      # the lowest lane is 3: index 67


# ---- the inputs of tests/test_gpu_wide_limits.py
@functools.lru_cache(maxsize=None)
def _limits_run(W, wrong=None):
    return wm.run_on_cpu(_roots(wm.limit_inputs()), W, list(wm.LIMIT_BUDGETS), wrong=wrong)


@functools.lru_cache(maxsize=None)
def _kept_run(W, wrong=None):
    roots, m, log = _roots(wm.limit_inputs()), None, []
    for mv in range(wm.KEPT_MOVES + 1):
        m = wm.run_on_cpu(roots, W, [wm.KEPT_BUDGET] * 4, model=m, only_steps=wm.KEPT_FIRST_STEPS if mv == 0 else None, wrong=wrong)
        log.append({"sims": list(m.sims), "inflight": m.inflight(), "nodes": [t.n_nodes() for t in m.trees], "root_n": [t.N[0] for t in m.trees],
                    "over": [r.is_game_over() for r in roots], "signature": _signature(m)})
        if mv < wm.KEPT_MOVES:
            forced = wm.kept_forced(m, roots, mv == wm.KEPT_MOVES - 1)
            wm.kept_boundary(m, roots, forced)
            log[-1].update(forced=forced, kept_n=[t.N[0] for t in m.trees], kept_nodes=[t.n_nodes() for t in m.trees])
    return m, log


@functools.lru_cache(maxsize=None)
def _pool_run(wrong=None):
    return wm.run_on_cpu(_roots(wm.pool_inputs()), wm.POOL_W, list(wm.POOL_BUDGETS), max_nodes=wm.POOL_MAX_NODES, wrong=wrong)


@functools.lru_cache(maxsize=None)
def _depth_run(wrong=None):
    return wm.run_on_cpu(_roots(wm.depth_inputs()), wm.DEPTH_W, list(wm.DEPTH_BUDGETS), max_depth=wm.DEPTH_MAX_DEPTH,
                         overrides=wm.DEPTH_OVERRIDES, wrong=wrong)


@functools.lru_cache(maxsize=None)
def _nan_run(wrong=None):
    return wm.run_on_cpu(_roots(wm.nan_inputs()), wm.NAN_W, list(wm.NAN_BUDGETS), overrides=wm.NAN_OVERRIDES, wrong=wrong)


@pytest.mark.parametrize("W", wm.LIMIT_WIDTHS)
def test_the_wide_inputs_meet_their_conditions_on_the_cpu(W):
    m = _limits_run(W)
    cond = wm.limit_conditions(m)
    assert all(cond.values()), (W, cond)
    assert m.sims == list(wm.LIMIT_BUDGETS) and m.inflight() == 0 and m.error_flags() == 0
    assert max(t.n_nodes() for t in m.trees) < wm.LIMIT_MAX_NODES
    assert sum(1 for t in m.trees for k in t.kids if k and len(k) > 64) >= 3        # "widest" has one such node, WIDE_PAIR many


@pytest.mark.parametrize("W", wm.KEPT_WIDTHS)
def test_the_kept_tree_script_meets_its_conditions_on_the_cpu(W):
    m, log = _kept_run(W)
    first = log[0]
    assert first["inflight"] > 0 and max(first["sims"]) < wm.KEPT_BUDGET            # the first boundary is crossed mid-search
    for mv in range(1, wm.KEPT_MOVES):
        assert log[mv]["sims"] == [wm.KEPT_BUDGET] * 4 and log[mv]["inflight"] == 0 and not any(log[mv]["over"])
    assert any(n > wm.KEPT_BUDGET for n in log[1]["root_n"] + log[2]["root_n"])    # a search went on on kept visits: N(root) above one budget
    assert any(n > 1 for mv in range(wm.KEPT_MOVES) for n in log[mv]["kept_nodes"]) # a kept subtree ...
    assert any(n == 1 for mv in range(wm.KEPT_MOVES) for n in log[mv]["kept_nodes"]) # ... and a child never expanded: a bare root
    # the last boundary mates on board 3: it selects nothing, the others use their budgets
    assert log[-1]["over"] == [False, False, False, True] and log[-1]["sims"] == [wm.KEPT_BUDGET] * 3 + [0]
    assert max(max(l["nodes"]) for l in log) < wm.LIMIT_MAX_NODES
    assert max(max(l["kept_nodes"]) for l in log[:-1]) < wm.LIMIT_MAX_NODES // 2    # no re-root prunes (a kept subtree may fill half the pool)


def test_the_pool_case_meets_its_conditions_on_the_cpu():
    m = _pool_run()
    assert wm.POOL_MAX_NODES >= 130                                  # (ccz_create raises anything smaller to 130)
    assert m.refused[0] > 0 and m.refused[1:] == [0, 0, 0] and m.error_flags() == 1
    assert m.fit_after_refusal >= 1 and m.refused_again >= 1
    assert m.sims == list(wm.POOL_BUDGETS) and m.inflight() == 0
    assert m.trees[0].n_nodes() <= wm.POOL_MAX_NODES and all(t.n_nodes() < wm.POOL_MAX_NODES - 128 for t in m.trees[1:])


def test_the_depth_case_meets_its_conditions_on_the_cpu():
    m = _depth_run()
    assert m.depth_stops[0] >= 2 and m.depth_stops[1:] == [0, 0, 0] and m.error_flags() == 2
    assert m.stops_after_leaves >= 1 and m.empty_steps_after_stop == 1          # a batch with t >= 1 ended by the stop, then t == 0
    assert 0 < m.sims[0] < wm.DEPTH_BUDGETS[0] and m.sims[1:] == list(wm.DEPTH_BUDGETS[1:]) and m.inflight() == 0
    assert max(t.n_nodes() for t in m.trees) < wm.LIMIT_MAX_NODES


def test_the_nan_case_meets_its_conditions_on_the_cpu():
    m = _nan_run()
    k = len(m.trees[0].kids[0])
    assert m.nan_stops[0] >= 1 and m.nan_stops[1:] == [0, 0, 0] and m.error_flags() == 32
    assert m.sims[0] == k + 1 < wm.NAN_BUDGETS[0] and m.trees[0].root_children()[1].tolist() == [1] * k
    assert m.sims[1:] == list(wm.NAN_BUDGETS[1:]) and m.inflight() == 0
    assert max(t.n_nodes() for t in m.trees) < wm.LIMIT_MAX_NODES


@pytest.mark.parametrize("wrong", wm.WRONG)
def test_each_new_rule_stated_wrongly_changes_the_result(wrong):
    if wrong in ("upper_children_ignored", "per_pass_maximum"):
        pairs = [(_limits_run(32), _limits_run(32, wrong))]
    elif wrong in ("reroot_forgets_visits", "reroot_keeps_sims"):
        pairs = [(_kept_run(8)[0], _kept_run(8, wrong)[0])]
    elif wrong == "refusal_blocks_later_slots":
        pairs = [(_pool_run(), _pool_run(wrong))]
    else:
        pairs = [(_depth_run(), _depth_run(wrong)), (_nan_run(), _nan_run(wrong))]
    for good, bad in pairs:
        assert _signature(good) != _signature(bad), wrong
