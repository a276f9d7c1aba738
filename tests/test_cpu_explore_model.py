"""CPU: the model of root exploration (tests/explore_model.py) that tests/test_gpu_root_exploration.py compares the engine with.

1. With neutral settings (eps = 0, forced_k = 0, pruning off), and with the feature off, the model IS the reference's search: visits,
   Q bits and priors of ``oracle.OracleMCTS`` on the same positions and evaluator, across a re-root. This pins the model's own
   arithmetic (float32 backup, float32 c_puct * P, float64 elsewhere, first maximum) without a GPU.
2. Each rule, stated wrongly, gives another answer on a concrete input: the helpers can tell the rules apart.
3. The GPU test's inputs exercise every rule, so that an engine which ignored one could not pass."""
import numpy as np
import pytest

import explore_model as em
from oracle import OracleMCTS

F32 = np.float32


def _oracle_run(b, board, n1, n2):
    o = OracleMCTS(lambda brd, ids: (em.evaluate(em.SALTS, b, brd)[0][ids], em.evaluate(em.SALTS, b, brd)[1]), c_puct=5, n_playout=0)
    board = board.copy()
    for _ in range(n1):
        o.playout(board)
    first = o.root_children()
    mv = int(first[0][int(np.argmax(first[1]))])
    o.update_with_move(mv)
    board.push_id(mv)
    for _ in range(n2):
        o.playout(board)
    return first, mv, o.root_children()


@pytest.mark.parametrize("cfg", [None, {"eps": 0.0, "alpha": 0.2, "forced_k": 0.0, "prune": False}], ids=["off", "neutral"])
def test_neutral_model_is_the_oracles_search(cfg):
    boards, _, _ = em.inputs()
    pick = [0, 5, em.WIDE, em.FEW]
    m = em.ExploreModel([boards[b] for b in pick], [em.SALTS[b] for b in pick], em.SEED, em.BASE, cfg=cfg)
    n1, n2 = 130, 40
    m.search([n1] * len(pick))
    got1 = [m.root_children(j) for j in range(len(pick))]
    want = [_oracle_run(b, boards[b], n1, n2) for b in pick]
    forced = [w[1] for w in want]
    fin = m.finish_move(forced=forced)
    m.search([n2] * len(pick))
    for j, b in enumerate(pick):
        for got, exp in ((got1[j], want[j][0]), (m.root_children(j), want[j][2])):
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), b
            assert np.array_equal(got[2].view(np.uint32), exp[2].view(np.uint32)), b       # Q bits
            assert np.array_equal(got[3].view(np.uint32), exp[3].view(np.uint32)), b       # priors
        assert np.array_equal(fin[j]["pruned"], fin[j]["visits"])                         # pi is the raw visit distribution
    assert m.totals()["forced_selections"] == 0 and m.totals()["visits_pruned"] == 0
    assert max(len(w[0][0]) for w in want) == 108 and want[pick.index(em.WIDE)][0][1].max() > 1    # past the visit-every-child pass


# ---------------------------------------------------------------------------------------------------------------- wrong rules
def test_noise_row_and_noisy_priors():
    pri = np.array([0.5, 0.25, 0.125, 0.125], F32)
    g = em.det_gammas(9, 77, 1, 3, 4, 0.2)[0]
    row = em.noise_row(9, 77, 3, 4, 0.2, pri)
    assert row.dtype == F32 and np.array_equal(row, (g / ((((0.0 + g[0]) + g[1]) + g[2]) + g[3])).astype(F32))
    pn = em.noisy_priors(pri, row, 0.25)
    assert np.array_equal(pn, (0.75 * pri.astype(np.float64) + 0.25 * row.astype(np.float64)).astype(F32))
    assert np.array_equal(em.noisy_priors(pri, row, 0.0), pri)                      # eps = 0: the raw priors, bit for bit


def test_wrong_rule_noise_written_into_the_nodes_survives_a_re_root():
    boards, _, _ = em.inputs()
    kw = dict(cfg=dict(em.FULL))
    right = em.ExploreModel([boards[0]], [em.SALTS[0]], em.SEED, em.BASE, **kw)
    wrong = em.ExploreModel([boards[0]], [em.SALTS[0]], em.SEED, em.BASE, wrong="noise_in_nodes", **kw)
    for m in (right, wrong):
        m.search([60])
    raw = np.array([em.evaluate(em.SALTS, 0, boards[0])[0][i] for i in boards[0].legal_ids()], F32)
    assert np.array_equal(right.root_children(0)[3].view(np.uint32), raw.view(np.uint32))      # nodes keep their raw priors
    assert not np.array_equal(wrong.root_children(0)[3], raw)
    assert np.array_equal(right.root_children(0)[1], wrong.root_children(0)[1])                # (the same search so far)
    mv = int(right.root_children(0)[0][int(np.argmax(right.root_children(0)[1]))])
    i = boards[0].legal_ids().index(mv)
    for m in (right, wrong):
        m.finish_move(forced=[mv])
    assert right.roots[0].P == raw[i] and wrong.roots[0].P != raw[i]                          # the kept root carries the old noise


def test_wrong_rule_less_or_equal_in_the_forced_test():
    # forced_k * P' * S = 2 * 0.125 * 16 = 4, sqrt = 2 exactly: a child with N = 2 has had its forced playouts
    N, pn = np.array([5, 2, 1, 0]), np.array([0.5, 0.125, 0.125, 0.25], F32)
    assert em.forced_mask(N, pn, 16, 2.0).tolist() == [False, False, True, False]
    assert em.forced_mask(N, pn, 16, 2.0, wrong="le").tolist() == [False, True, True, False]
    assert not em.forced_mask(N, pn, 16, 0.0).any()
    sc, forced = em.root_scores(N, np.zeros(4, F32), pn, 17, 5, 2.0)
    assert int(np.argmax(sc)) == 2 and forced[2]                                               # first maximum among the +inf scores
    sc, forced = em.root_scores(N, np.zeros(4, F32), pn, 17, 5, 2.0, wrong="le")
    assert int(np.argmax(sc)) == 1


def _prune_input():
    # root N = 41, S = 40; c* = child 0. Child 1: a forced child far below c*'s score; child 2: better Q than c* can reach (gap <= 0);
    # child 3: pruning leaves it one visit, which is dropped; child 4: unvisited
    N = np.array([30, 4, 3, 3, 0])
    Q = np.array([0.5, -0.5, 0.95, 0.35, 0.0], F32)
    pn = np.array([0.4, 0.2, 0.05, 0.2, 0.15], F32)
    return N, Q, pn, 41, 5, 2.0


def test_pruning_rule_by_hand():
    N, Q, pn, rn, c, fk = _prune_input()
    Np, gaps = em.prune_counts(N, Q, pn, rn, c, fk)
    sq = np.sqrt(41.0)
    top = 0.5 + float(F32(5) * F32(0.4)) * sq / 31.0
    assert np.isnan(gaps[0]) and np.isnan(gaps[4]) and gaps[1] == top - float(F32(-0.5)) and gaps[2] < 0.0
    # child 1: nf = ceil(sqrt(2 * 0.2 * 40)) = 4, need = ceil(E / gap - 1) = ceil(6.40 / 1.41 - 1) = 4 -> kept whole by `need`
    # child 2: gap <= 0 -> need = N: kept whole; child 3: nf = 4, need = ceil(6.40 / 0.563 - 1) = 11 -> kept whole
    assert Np.tolist() == [30, 4, 3, 3, 0]
    # with a worse child 3 (Q = -0.9): need = ceil(6.40 / 1.81 - 1) = 3 -> kept; Q = -5: need = ceil(0.08) = 1, N - nf < 0 -> 1 -> dropped
    Q2 = Q.copy()
    Q2[3] = F32(-5.0)
    assert em.prune_counts(N, Q2, pn, rn, c, fk)[0].tolist() == [30, 4, 3, 0, 0]
    assert em.prune_counts(N, Q2, pn, rn, c, fk, prune=False)[0].tolist() == N.tolist()
    assert em.prune_counts(N, Q2, pn, rn, c, 0.0)[0].tolist() == N.tolist()                    # no forced playouts: nothing to take back


def test_wrong_rule_pruning_without_the_drop_of_a_single_visit():
    N, Q, pn, rn, c, fk = _prune_input()
    Q[3] = F32(-5.0)
    assert em.prune_counts(N, Q, pn, rn, c, fk)[0][3] == 0
    assert em.prune_counts(N, Q, pn, rn, c, fk, wrong="keep_small")[0][3] == 1


def test_wrong_rule_pruning_that_also_reduces_the_best_child():
    """In exact arithmetic c* would keep its count under the general rule as well (its gap is E_* / (1 + N_*), so need_* = N_*); in
    float64 it does not: with a prior so small that top - Q_* is a couple of ulps of Q_*, the quotient E_* / gap is off by a quarter
    and the forced term N - nf takes one visit. c* is exempt by statement: N'_* = N_*."""
    N, Q = np.array([30, 4, 3, 0]), np.array([0.5, -0.5, 0.1, 0.0], F32)
    pn = np.array([2.0 ** -54 * 1.3, 0.2, 0.05, 0.15], F32)
    assert em.prune_counts(N, Q, pn, 38, 5, 2.0)[0].tolist() == [30, 4, 3, 0]
    assert em.prune_counts(N, Q, pn, 38, 5, 2.0, wrong="best_too")[0].tolist() == [29, 4, 3, 0]
    # ties in N go to the lowest index: child 0 is c*, child 1 (same count, far worse value) is cut back to its forced floor
    N2, Q2, pn2 = np.array([9, 9, 2]), np.array([0.8, -0.9, 0.0], F32), np.array([0.3, 0.3, 0.4], F32)
    assert em.prune_counts(N2, Q2, pn2, 21, 5, 2.0)[0].tolist()[0] == 9
    assert em.prune_counts(N2, Q2, pn2, 21, 5, 2.0)[0].tolist()[1] < 9


def test_wrong_rule_sampler_mixing_left_on():
    pi = em.det_pi(np.array([40, 3, 0, 2, 1, 0, 0, 0], np.int32), 1.0)
    picks_plain = [em.choose_move(pi, 5, 11, mv, 0.25, 0.2, mix=False) for mv in range(64)]
    picks_mixed = [em.choose_move(pi, 5, 11, mv, 0.25, 0.2, mix=True) for mv in range(64)]
    assert picks_plain != picks_mixed
    assert all(pi[i] > 1e-6 for i in picks_plain)                     # without mixing an unvisited child is never played at temp 1
    assert any(pi[i] < 1e-6 for i in picks_mixed)                     # ... with it, the noise plays them
    u = em.det_choice_uniform(5, 11, 0)
    cdf = np.cumsum(pi) / np.sum(pi)
    assert picks_plain[0] == min(int(np.searchsorted(cdf, u, side="right")), len(pi) - 1)


# ---------------------------------------------------------------------------------------------------------------- the GPU test's inputs
def test_inputs_are_what_the_gpu_test_says():
    boards, lines, sims = em.inputs()
    ks = [len(b.legal_ids()) for b in boards]
    assert len(boards) == 16 and all(30 <= k <= 50 for k in ks[:14]) and ks[em.WIDE] == 108 and ks[em.FEW] < 8
    assert len({(b.squares().tobytes(), int(b.turn)) for b in boards}) == 16
    assert sims[em.WIDE] == 160 > 108 and all(s == 96 for i, s in enumerate(sims) if i != em.WIDE)
    assert all(ln is None or 2 <= len(ln) <= 6 for ln in lines)


def test_inputs_exercise_every_rule():
    r = em.run_case(0.25, 2.0, True)
    assert r["pruned_subtrees"] == 0
    bs = r["board_stats"]
    assert sum(s["forced_selections"] > 0 for s in bs) >= em.B // 2
    assert sum(s["visits_pruned"] > 0 for s in bs) >= em.B // 2
    f = r["facts"]
    assert f["big_to_zero"] >= 1            # a child with N > 1 pruned to 0
    assert f["kept_whole_gap_le0"] >= 1     # a child whose gap is not positive is kept whole
    assert f["forced_hi"] and f["pruned_hi"]  # on the wide board: a forced selection and a pruned child at an index >= 64
    assert bs[em.WIDE]["forced_selections"] > 0 and bs[em.WIDE]["children_pruned"] > 0
    # both moves are played on (nearly) every board: the second move runs on kept subtrees
    assert sum(m is not None for m in r["moves"][1]["finish"]) >= em.B - 1
    # the playout-cap case: half of the boards explored, the other half untouched
    t = tuple(int(b % 2) for b in range(em.B))
    rc = em.run_case(0.25, 2.0, True, targets=t)
    assert all((s["explored_moves"] > 0) == bool(t[b]) for b, s in enumerate(rc["board_stats"]))
