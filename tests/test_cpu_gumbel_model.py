"""CPU: the sequential model of the Gumbel root search (tests/gumbel_model.py) on its own -- the known answers of the
considered-visits sequence, each mis-stated rule giving another answer on a stated input, pi' at c_scale = 0, the Gumbel-max
property of the draws, and the facts that keep tests/test_gpu_gumbel.py's cases from passing vacuously."""
import math

import numpy as np
import pytest

import gumbel_model as gm
from budget_twin import twin_budgets


def test_known_sequences():
    assert gm.sequence(4, 8) == [0, 0, 0, 0, 1, 1, 2, 2]
    assert gm.sequence(16, 32) == [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4
    assert gm.sequence(2, 5) == [0, 0, 1, 1, 2]
    assert gm.sequence(3, 7) == [0, 0, 0, 1, 1, 2, 2]
    assert gm.sequence(16, 8) == [0] * 8
    assert gm.sequence(1, 4) == [0, 1, 2, 3] and gm.sequence(0, 3) == [0, 1, 2]
    for m in range(1, 18):
        for n in range(1, 71):
            s = gm.sequence(m, n)
            assert len(s) == n and s[0] == 0 and all(0 <= b - a <= 1 for a, b in zip(s, s[1:])), (m, n)


# ---------------------------------------------------------------------------------------------------------------- mis-stated rules
def test_wrong_sign_of_the_gumbel_transform():
    g, w = gm.gumbel_draw(7, 4096, 0, 0), gm.gumbel_draw(7, 4096, 0, 0, wrong="gumbel_sign")
    assert g == -w and g != 0.0
    # ... and the draw is -log(-log u) of the word's first uniform
    from budget_twin import ua
    u = ua(7, 4096, 0, child=0, draw=0xfffff)
    assert abs(g - -math.log(-math.log(u))) < 1e-12


def test_wrong_total_visits_for_move_visits():
    N, n0 = [5, 1, 0], [5, 0, 0]                       # a kept subtree of 5 visits under child 0, one simulation of this move
    M, W = gm.move_visits(N, n0), gm.move_visits(N, n0, wrong="n_not_m")
    assert M == [0, 1, 0] and W == [5, 1, 0]
    assert gm.candidates(M, 3, 7) == [0, 2]            # t = 1: seq(3, 7)[1] = 0
    assert gm.candidates(W, 3, 7) == [0]               # t = 6: seq(3, 7)[6] = 2, nobody has it: the most visited


def test_wrong_q_left_signed():
    N, Q, P = [2, 0], [np.float32(0.5), np.float32(0.0)], [np.float32(0.5), np.float32(0.5)]
    cq, v = gm.completed_q(N, Q, P, np.float32(-0.25))
    assert cq[0] == 0.75 and v == (0.625 + 2.0 * 0.375 / 0.5) / 3.0 and cq[1] == v
    cw, vw = gm.completed_q(N, Q, P, np.float32(-0.25), wrong="q_signed")
    assert cw[0] == 0.5 and vw == (0.25 + 2.0 * 0.25 / 0.5) / 3.0


def test_wrong_sign_of_the_root_value():
    N, Q, P = [0, 0], [np.float32(0.0)] * 2, [np.float32(0.5)] * 2
    assert gm.completed_q(N, Q, P, np.float32(-0.5))[1] == 0.75        # the root's stored mean is its parent's view
    assert gm.completed_q(N, Q, P, np.float32(-0.5), wrong="v0_sign")[1] == 0.25


def test_wrong_candidates_that_ignore_the_target():
    M = [1, 0, 0]
    assert gm.candidates(M, 3, 7) == [1, 2] and gm.candidates(M, 3, 7, wrong="ignore_target") == [0, 1, 2]
    assert gm.candidates([2, 2, 1], 3, 4) == [0, 1]                    # t = 5 >= n_eff: the most visited
    assert gm.first_max([1.0, 3.0, 3.0], [0, 1, 2]) == 1 and gm.first_max([float("nan")] * 2, [0, 1]) is None


@pytest.mark.parametrize("wrong", gm.WRONG)
def test_every_wrong_rule_changes_the_search(wrong):
    """... and on the GPU test's own inputs each of them grows other trees or records other targets."""
    def run(w):
        m, _ = gm.case("n8_m4", "peaked", wrong=w)
        out = []
        for _ in range(2):
            m.search(8)
            out.append([tuple(m.root_children(b)[1]) for b in range(gm.B)])
            m.finish_move()
            out.append([None if r is None else (r["move"], r["pi"].tobytes()) for r in m.last])
        return out
    assert run(wrong) != run(None)


# ---------------------------------------------------------------------------------------------------------------- pi'
def test_pi_without_sigma_is_the_normalised_prior():
    rng = np.random.RandomState(3)
    for P in (np.array([0.5, 0.25, 0.15, 0.1], np.float32), rng.dirichlet(np.ones(40)).astype(np.float32),
              (rng.dirichlet(np.ones(108)) * 0.3).astype(np.float32)):
        N = list(rng.randint(0, 5, len(P)))
        cq, _ = gm.completed_q(N, rng.uniform(-1, 1, len(P)).astype(np.float32), P, np.float32(0.1))
        pi = gm.improved_policy([gm.logit_of(p) for p in P], gm.sigmas(N, cq, 50.0, 0.0))
        want = P.astype(np.float64) / P.astype(np.float64).sum()
        assert np.abs(pi - want).max() <= 1e-15


def test_gumbel_max_samples_the_prior():
    """arg max (g + logit) is a sample of the prior: over n board ids the count of move i is binomial(n, p_i); 4 standard deviations
    (a bound derived from that, 6e-5 a move two-sided) hold for each of the four moves."""
    P = [0.5, 0.25, 0.15, 0.1]
    lg = [gm.logit_of(p) for p in P]
    n, hits = 20000, [0] * 4
    for gid in range(n):
        s = [gm.gumbel_draw(11, gid, 0, i) + lg[i] for i in range(4)]
        hits[gm.first_max(s, range(4))] += 1
    for i, p in enumerate(P):
        assert abs(hits[i] - n * p) <= 4.0 * math.sqrt(n * p * (1.0 - p)), (i, hits)


# ---------------------------------------------------------------------------------------------------------------- the GPU test's cases
def test_sequential_halving_on_a_fresh_root():
    m, _ = gm.case(dict(n_sims=9, max_considered=4, c_visit=50.0, c_scale=1.0))
    m.search(9)                                         # the root's expansion, then n_eff = 8 simulations: 0 0 0 0 1 1 2 2
    for b in range(gm.B):
        g, logit, n0, n_eff = m.root_row(b)
        assert n_eff == 8 and not n0.any()
        N = sorted(m.root_children(b)[1], reverse=True)
        assert N[:5] == [3, 3, 1, 1, 0], (b, N)


@pytest.mark.parametrize("evaluator", ["hash", "peaked"])
@pytest.mark.parametrize("setting", list(gm.SETTINGS))
def test_the_cases_exercise_the_rules(setting, evaluator):
    m, _ = gm.case(setting, evaluator)
    n = gm.SETTINGS[setting]["n_sims"]
    for _ in range(gm.MOVES):
        m.search(n)
        m.finish_move()
    f, s = m.gfacts, m.gstats
    assert f["kept_n0"] > 0 and f["target_gt0"] > 0            # rows over kept subtrees; targets past the first round
    mc = gm.SETTINGS[setting]["max_considered"]
    assert s["gumbel_moves"] >= 5 * gm.B and s["considered_sum"] <= s["gumbel_moves"] * mc
    assert (s["considered_sum"] < s["gumbel_moves"] * mc) == (mc > 7)     # `pawns` has 7 moves: m = k there when max_considered is 16
    assert s["offvisit_moves"] > 0
    if evaluator == "peaked":                                  # the logit term decides: pi' is far from uniform
        assert max(float(r["pi"].max()) for r in m.last if r is not None) > 0.3


def test_a_budget_seed_with_both_kinds():
    b = twin_budgets(gm.SEED, gm.BASE, gm.B, 0, 32, 8, 0.5)
    assert set(b.tolist()) == {32, 8}


def test_the_fallback_past_n_eff():
    m, _ = gm.case("n32_m16")
    m.search(40)
    assert m.gfacts["fallback"] >= 8 * gm.B
