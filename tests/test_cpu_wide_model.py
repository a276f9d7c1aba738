"""The NumPy model of the wide search (tests/wide_model.py) against a case computed by hand: width 2 on a root with three
children, c_puct = 2, priors (0.5, 0.25, 0.25), budget 5. Every score is written out below. No GPU."""
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
