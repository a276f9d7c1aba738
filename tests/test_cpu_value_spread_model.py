"""CPU: the model of the value spread and of the LCB move (tests/value_spread_model.py; include/cczero.h "Value spread and the LCB move").

The statistic on a hand-computed path, against a float64 two-pass sum of squared deviations under a bound derived from n and the
float32 unit roundoff, the max(S, 0) clamp, the LCB rule's cases, and the options table. No GPU."""
import math

import numpy as np
import pytest

import value_spread_model as vsm
from explore_model import F32

U = 2.0 ** -24        # the unit roundoff of float32 (round to nearest)


# ---------------------------------------------------------------------------------------------------------------- the statistic
def test_three_backups_by_hand():
    """Values 0.5, -0.25, 1.0 into one node. By hand: after 0.5: N 1, Q 0.5, S 0 (the first value deviates from nothing). After
    -0.25: d0 = -0.75, Q = 0.5 - 0.375 = 0.125, S = (-0.75)(-0.375) = 0.28125, all exact in binary. After 1.0: d0 = 0.875,
    Q = 0.125 + 0.875 / 3 = 5/12, S = 0.28125 + 0.875 * (7/12) = 19/24 -- thirds are not binary: within two units in the last place."""
    n, q, s = vsm.spread_step(0, 0.0, 0.0, 0.5)
    assert (n, float(q), float(s)) == (1, 0.5, 0.0)
    n, q, s = vsm.spread_step(n, q, s, -0.25)
    assert (n, float(q), float(s)) == (2, 0.125, 0.28125)
    n, q, s = vsm.spread_step(n, q, s, 1.0)
    assert n == 3 and q.dtype == s.dtype == np.float32
    assert abs(float(q) - 5.0 / 12.0) <= 2 * U * (5.0 / 12.0) and abs(float(s) - 19.0 / 24.0) <= 2 * 2 * U * (19.0 / 24.0)
    # the same three values through the tree model's backup: a path of one node, so the leaf's sign flip applies (-v at the leaf)
    from solver_model import SNode
    m = vsm.SpreadModel.__new__(vsm.SpreadModel)
    m._S = {}
    node = SNode(1.0, -1)
    for v in (-0.5, 0.25, -1.0):
        m._backup([node], F32(v))
    assert node.N == 3 and node.Q == q and m.S_of(node) == s


def _bound(n):
    """|S_float32 - S_exact| after n values in [-1, 1], first order in U, doubled for the higher orders.
    The mean: q' = q + (x - q) / n has three roundings (the difference, |.| <= 2; the quotient, <= 2; the sum, <= 1): at most 5 U of new
    error a step, and the step carries old error over with weight 1 - 1/n < 1: |dq| <= 5 U i after i steps.
    The two deviations d0, d1 (|.| <= 2) each inherit a mean's error and round once: |dd| <= 5 U i + 2 U.
    The product (<= 4): 2 * 2 * (5 U i + 2 U) from its factors, 4 U from its rounding; the sum S (<= 4 i): 4 U i.
    Summed over i = 1 .. n: U * (12 n (n + 1) + 12 n)."""
    return 2.0 * U * (12.0 * n * (n + 1) + 12.0 * n)


@pytest.mark.parametrize("n,seed", [(2, 0), (17, 1), (200, 2), (800, 3)])
def test_s_is_the_two_pass_sum_of_squared_deviations(n, seed):
    rng = np.random.default_rng(seed)
    xs = rng.uniform(-1.0, 1.0, n).astype(F32)
    xs[rng.integers(0, n, n // 4)] = rng.choice(np.array([-1.0, 0.0, 1.0], F32), n // 4)     # terminal values among the net's
    N, q, s = 0, F32(0), F32(0)
    for x in xs:
        N, q, s = vsm.spread_step(N, q, s, x)
    x64 = xs.astype(np.float64)
    mean = math.fsum(x64) / n
    two_pass = math.fsum((x - mean) ** 2 for x in x64)
    print(f"n {n}: S float32 {float(s):.9g}, two-pass {two_pass:.9g}, |diff| {abs(float(s) - two_pass):.3g}, bound {_bound(n):.3g}")
    assert abs(float(s) - two_pass) <= _bound(n)
    assert abs(float(q) - mean) <= 5 * U * n


# found by a random search over (N, Q, value) on the CPU: the float32 product (val - q) * (val - qn) is negative, because qn rounds to
# the other side of val. All the search's hits have N = 0 with Q != 0, which no tree holds (an unvisited node has Q = 0); the search over
# N >= 1 found none. The clamp is what makes the rule total anyway.
NEGATIVE = (0, float.fromhex("-0x1.f2f324p-4"), float.fromhex("0x1.2bfaf2p-2"))


def test_the_clamp_on_a_negative_float32_product_that_no_tree_reaches():
    """The input is synthetic: N = 0 with Q != 0 is a state no tree holds (an unvisited node has Q = 0), and for n >= 2 the product
    cannot be negative (qn lies between q and val, and the roundings are monotone). What this shows is the model's clamp on a negative
    S handed to the rule; the engine's clamp in k_lcb_moves is the same expression and is never fed a negative S by a search."""
    n_old, q, val = NEGATIVE
    n, qn, s = vsm.spread_step(n_old, q, 0.0, val)
    assert float(s) == float.fromhex("-0x1.a8b7bcp-27") and float(qn) == float.fromhex("0x1.2bfaf4p-2")     # S < 0: qn overshot val
    # as a child's S the negative sum counts as zero spread: the bound is Q itself, not NaN
    b = vsm.lcb_bounds([5, 5], [0.25, 0.25], [s, F32(0.0)], 3.0)
    assert b[0] == b[1] == 0.25
    assert vsm.lcb_choice([5, 5], [0.25, 0.25], [s, F32(0.0)], 3.0, 0.0, 0)[0] == 0


# ---------------------------------------------------------------------------------------------------------------- the LCB rule
def test_bounds_by_hand():
    # N 4, S 3: var = 1, standard error sqrt(1 / 4) = 0.5; z = 2: Q - 1
    assert vsm.lcb_bounds([4, 1, 0], [0.5, 0.9, 0.0], [3.0, 0.0, 0.0], 2.0) == [-0.5, vsm.NINF, vsm.NINF]


CASES = {
    # name: (N, Q, S, z, ratio, min_visits, child)
    "lcb_prefers_the_steady_child": ([10, 9], [0.30, 0.28], [9.0, 0.0], 1.0, 0.15, 2, 1),      # 0.30 - sqrt(1/10) < 0.28
    "ratio_cut": ([100, 14, 15], [0.1, 0.9, 0.2], [0.0, 0.0, 0.0], 5.0, 0.15, 2, 2),            # 14 < 0.15 * 100 <= 15
    "min_visits": ([100, 30, 40], [0.1, 0.9, 0.2], [0.0, 0.0, 0.0], 5.0, 0.15, 35, 2),
    "tie_to_the_lower_index": ([10, 10, 10], [0.1, 0.4, 0.4], [0.0, 0.0, 0.0], 5.0, 0.15, 2, 1),
    "all_minus_inf_gives_istar": ([1, 1, 0], [0.2, 0.9, 0.0], [0.0, 0.0, 0.0], 5.0, 0.0, 0, 0),
    "istar_is_eligible_below_min_visits": ([3, 2], [0.5, -0.5], [0.0, 0.0], 5.0, 0.0, 10, 0),
    "z_zero_plays_the_highest_q": ([10, 5, 2], [0.1, 0.2, 0.3], [50.0, 50.0, 50.0], 0.0, 0.0, 0, 2),
    "ratio_one_plays_argmax": ([10, 9, 9], [0.1, 0.9, 0.9], [0.0, 0.0, 0.0], 5.0, 1.0, 2, 0),
    "ratio_one_with_a_visit_tie": ([10, 10, 9], [0.1, 0.9, 0.95], [0.0, 0.0, 0.0], 5.0, 1.0, 2, 1),
    "nothing_visited": ([0, 0], [0.0, 0.0], [0.0, 0.0], 5.0, 0.15, 2, -1),
    "no_children": ([], [], [], 5.0, 0.15, 2, -1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_lcb_cases(name):
    N, Q, S, z, ratio, mv, want = CASES[name]
    got, bounds = vsm.lcb_choice(N, Q, S, z, ratio, mv)
    assert got == want, (got, bounds)


# ---------------------------------------------------------------------------------------------------------------- the options table
def test_the_options_table():
    from chinesechesszero_amd import options as O
    assert list(O.MOVE_OPTIONS) == ["lcb"] and O.MOVE_OPTIONS["lcb"].setter == "set_value_stats"
    assert (O.LCB_STDEVS, O.LCB_MIN_VISIT_RATIO, O.LCB_MIN_VISITS) == (5.0, 0.15, 2)
    assert O.MOVE_OPTIONS["lcb"].of_scalar(True) == {"z": 5.0, "min_visit_ratio": 0.15, "min_visits": 2}
    assert O.MOVE_OPTIONS["lcb"].of_scalar(2.5)["z"] == 2.5
    assert O.format_lcb({"moves": 8, "differed": 2}) == ", lcb moves 8, off the most visited move 2 (share 0.2500)"
    assert "n/a" in O.format_lcb({"moves": 0, "differed": 0})


def test_the_library_has_the_calls():
    from chinesechesszero_amd import _lib
    L = _lib.lib()
    for name in ("ccz_set_value_stats", "ccz_get_value_stats", "ccz_root_value_stats", "ccz_lcb_moves"):
        assert getattr(L, name) is not None
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "cczero.h")) as f:
        header = f.read()
    assert "int ccz_lcb_moves(ccz_engine *e, void *stream, double z, double min_visit_ratio, int32_t min_visits" in header
