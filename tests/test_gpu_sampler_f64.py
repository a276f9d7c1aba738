"""GPU: what the device-mode move sampler draws, read through ccz_move_distribution, against its CPU twin and float64 references.

k_finish_move draws each unforced move from (1 - eps) pi + eps Dirichlet(alpha 1_k) on the board's Philox stream
(csrc/cczero_kernels.h sample_move). ccz_move_distribution runs the same root_pi and sample_move without moving and returns the
raw Gamma draws, the mixed vector and the choice uniform. Here:
- those equal oracle/xq_sample.c bit for bit, called with the float32 parameters the device holds (float(np.float32(alpha))),
  over 4096 boards and three moves, board ids past 2^32 (the high word of the Philox counter) and the width fixtures with
  103 / 108 legal moves (children 64.. of the second lane pass) and one legal move;
- the move finish_move plays is the float64 NumPy choice from that output, on every board;
- on the device's own draws: Dirichlet moments and a Gamma KS test (tests/test_cpu_sampler_f64.py has the power checks);
- root pi against a float64 NumPy softmax of the same visits;
- a per-board temperature that is 0 or NaN sets CCZ_ERR_BAD_TEMP and that board neither records nor moves; bad sampler
  parameters are refused at construction.

Tolerance of pi (test_root_pi_against_float64_softmax). The device computes x_i = (1/t) det_log(N_i + 1e-10), then
det_exp(x_i - max x) and a sequential sum. det_log is within 2 ulp of log where |log| > 1e-3 and 1.5e-14 absolute elsewhere, so
|dx_i| <= (1/t)(|log(N_i + 1e-10)| 2^-51 + 1.5e-14) =: e_i, and the exponent's argument is off by at most e_i + e_max. det_exp adds
1 ulp, the k-term sum and the division k + 1 half-ulps, NumPy's own log / exp / sum about as much again. With L = max|log(N + 1e-10)|
(23.03 for N = 0): |p - ref| <= ref (2 (1/t)(L 2^-51 + 1.5e-14) + (2k + 8) 2^-53) + 1e-300; at t = 1e-3 that is ~2e-11 relative.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = (1 << 32) + 12345


def _engine(B, n=8, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(B, n_playout=n, **kw)


def _search(e, n):
    """n simulations of every board with uniform priors and value 0 (the uniform evaluator)."""
    import torch
    P = torch.full((e.B, 2086), 1.0 / 2086, dtype=torch.float32, device=e.device)
    V = torch.zeros(e.B, dtype=torch.float32, device=e.device)
    for _ in range(n):
        e.select_leaves()
        e.expand_backup(P, V)


def _twin(seed, gid, move_no, visits, temp, eps, alpha):
    import oracle
    k = len(visits)
    pi = oracle.det_pi(visits, temp)
    _, mixed = oracle.det_sample(seed, gid, move_no, pi, float(np.float32(eps)), float(np.float32(alpha)))
    g = oracle.det_gammas(seed, gid, 1, move_no, k, float(np.float32(alpha)))[0]
    return g, mixed, oracle.det_choice_uniform(seed, gid, move_no)


def _choice(mixed, u, k):
    cdf = np.cumsum(mixed[:k])
    return min(int(np.searchsorted(cdf / cdf[-1], u, side="right")), k - 1)


def _check_against_twin(e, seed, base, move_no, eps, alpha, temp=1.0, boards=None):
    rc = e.root_children()
    g, mixed, u = e.move_distribution()
    for b in (range(e.B) if boards is None else boards):
        k = int(rc["k"][b])
        tg, tm, tu = _twin(seed, base + b, move_no, rc["visits"][b][:k], temp, eps, alpha)
        assert np.array_equal(g[b][:k].view(np.uint64), tg.view(np.uint64)), (b, move_no)
        assert np.array_equal(mixed[b][:k].view(np.uint64), tm.view(np.uint64)), (b, move_no)
        assert np.float64(u[b]).view(np.uint64) == np.float64(tu).view(np.uint64), (b, move_no)
        assert not np.any(g[b][k:]) and not np.any(mixed[b][k:])
    return rc, g, mixed, u


def _check_moves(e, rc, mixed, u, moves):
    for b in range(e.B):
        k = int(rc["k"][b])
        assert moves[b] == rc["acts"][b][_choice(mixed[b], u[b], k)], b


def test_bit_identical_to_twin_4096_boards_three_moves():
    B, seed = 4096, 77
    e = _engine(B, seed=seed, board_id_base=BASE)
    for move in range(3):
        _search(e, 8)
        rc, g, mixed, u = _check_against_twin(e, seed, BASE, move, 0.25, 0.2)
        again = e.move_distribution()                     # the hook moves nothing
        assert all(np.array_equal(a, b_, equal_nan=True) for a, b_ in zip((g, mixed, u), again))
        moves = e.finish_move().cpu().numpy()
        _check_moves(e, rc, mixed, u, moves)
    assert np.all(e.game_status()["plies"] == 3)
    e.check_healthy()


@pytest.mark.parametrize("eps", (0.0, 0.25, 1.0))
@pytest.mark.parametrize("alpha", (0.03, 0.2, 1.0, 2.5))
def test_bit_identical_over_eps_and_alpha(eps, alpha):
    B, seed = 64, 5
    e = _engine(B, seed=seed, board_id_base=BASE, eps=eps, alpha=alpha)
    _search(e, 3)
    rc, g, mixed, u = _check_against_twin(e, seed, BASE, 0, eps, alpha)
    if eps == 0.0:
        pi = e.root_pi()
        assert np.array_equal(mixed, pi)
    _check_moves(e, rc, mixed, u, e.finish_move().cpu().numpy())
    e.check_healthy()


@pytest.mark.parametrize("name", ("wide_a0", "widest", "widest_black", "one_move"))
def test_bit_identical_on_width_fixtures(name):
    """Children 64..107 are drawn by the second 64-lane pass of sample_move; one legal move is the other edge."""
    from golden_cases import STARTS, WIDTHS
    turn, k0 = WIDTHS[name]
    B, seed = 8, 31
    e = _engine(B, seed=seed, board_id_base=BASE + 1000)
    for b in range(B):
        e.set_position(b, STARTS[name], turn, 0)
    _search(e, 1 + k0 // 4)   # some children visited, some not
    rc, g, mixed, u = _check_against_twin(e, seed, BASE + 1000, 0, 0.25, 0.2)
    assert np.all(rc["k"] == k0)
    assert np.all(g[:, :k0] > 0) and np.all(g[:, k0:] == 0)
    _check_moves(e, rc, mixed, u, e.finish_move().cpu().numpy())
    e.check_healthy()


@pytest.mark.parametrize("alpha", (0.03, 0.2, 1.0))
def test_device_dirichlet_moments_and_gamma_ks(alpha):
    """eps = 1: the mixed vector is Dirichlet(alpha 1_44) from the opening root; raw draws against P(alpha, x)."""
    import torch
    B, k = 4096, 44
    e = _engine(B, seed=123, board_id_base=BASE, eps=1.0, alpha=alpha)
    _search(e, 2)
    g, mixed, _ = e.move_distribution()
    a = float(np.float32(alpha))
    var = (k - 1) / (k * k * (k * a + 1))
    x = mixed[:, :k]
    assert np.all(e.root_children()["k"] == k) and np.all(x >= 0)
    assert np.all(np.abs(x.sum(1) - 1.0) <= k * 2.0 ** -52)
    for i in (0, 21, 43):
        c = x[:, i]
        assert abs(c.mean() - 1.0 / k) < 5 * math.sqrt(var / B), (i, c.mean())
        d2 = (c - 1.0 / k) ** 2
        assert abs(d2.mean() - var) < 5 * d2.std() / math.sqrt(B), (i, d2.mean(), var)
    draws = np.sort(g[:, :k].ravel())
    n = len(draws)
    f = torch.special.gammainc(torch.full((n,), a, dtype=torch.float64), torch.from_numpy(draws)).numpy()
    i = np.arange(1, n + 1)
    D = max(float((i / n - f).max()), float((f - (i - 1) / n).max()))
    assert math.sqrt(n) * D < 2.0, math.sqrt(n) * D


def _pi_ref(visits, temp):
    x = (1.0 / temp) * np.log(visits.astype(np.float64) + 1e-10)
    p = np.exp(x - x.max())
    return p / p.sum()


def _pi_tol(visits, temp):
    L = float(np.abs(np.log(visits.astype(np.float64) + 1e-10)).max())
    return 2.0 * (1.0 / temp) * (L * 2.0 ** -51 + 1.5e-14) + (2 * len(visits) + 8) * 2.0 ** -53


@pytest.mark.parametrize("n,start", [(1, None), (8, None), (40, "widest"), (200, None)])
def test_root_pi_against_float64_softmax(n, start):
    """n = 1: every child unvisited (pi uniform); 8: ties and zeros; widest: k = 108; 200: a few boards with a spread of counts."""
    from golden_cases import STARTS, WIDTHS
    B = 4 if n == 200 else 16
    e = _engine(B, n=n, seed=9)
    if start:
        for b in range(B):
            e.set_position(b, STARTS[start], WIDTHS[start][0], 0)
    _search(e, n)
    rc = e.root_children()
    for temp in (1e-3, 0.1, 0.5, 1.0, 1e3):
        pi = e.root_pi(temps=temp)
        for b in range(B):
            k = int(rc["k"][b])
            v = rc["visits"][b][:k]
            if n == 1:
                assert not np.any(v)
            ref = _pi_ref(v, temp)
            assert np.all(np.abs(pi[b][:k] - ref) <= ref * _pi_tol(v, temp) + 1e-300), (temp, b)
            assert abs(pi[b][:k].sum() - 1.0) <= 2 * k * 2.0 ** -52
            assert not np.any(pi[b][k:])
    e.check_healthy()


def test_bad_temperature_neither_records_nor_moves():
    from chinesechesszero_amd._lib import ERR_BAD_TEMP, CczError
    B = 8
    e = _engine(B, seed=4, max_plies=2)
    _search(e, 8)
    sq0 = e.root_positions()
    temps = np.ones(B)
    temps[[1, 3, 5]] = (0.0, np.nan, -1.0)
    moves = e.finish_move(temps=temps).cpu().numpy()
    bad = np.isin(np.arange(B), [1, 3, 5])
    assert np.all(moves[bad] == -1) and np.all(moves[~bad] >= 0)
    st = e.game_status()
    assert np.all(st["plies"][bad] == 0) and np.all(st["plies"][~bad] == 1)
    assert np.array_equal(e.root_positions()[bad], sq0[bad])
    assert e.stats()["error_flags"] & ERR_BAD_TEMP
    with pytest.raises(CczError, match="temperature"):
        e.check_healthy()
    # the other boards go on to be adjudicated at max_plies; no harvested row holds a NaN
    for _ in range(2):
        _search(e, 8)
        e.finish_move()
    import torch
    states, pi, z = e.harvest()
    assert pi.shape[0] > 0 and bool(torch.isfinite(pi).all()) and bool(torch.isfinite(z).all())
    # host-side checks of the syncing accessors
    for t in (0.0, np.nan, -2.0):
        with pytest.raises(CczError, match="temps"):
            e.root_pi(temps=t)
        with pytest.raises(CczError, match="temps"):
            e.move_distribution(temps=t)


def test_constructors_refuse_bad_sampler_parameters():
    from chinesechesszero_amd._lib import CczError
    from chinesechesszero_amd.match import BatchedMatch
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    for kw in (dict(temp=0.0), dict(temp=np.nan), dict(eps=1.5), dict(eps=-0.1), dict(alpha=0.0), dict(alpha=np.nan)):
        with pytest.raises(CczError):
            _engine(2, **kw)
    with pytest.raises(CczError, match="temp"):
        BatchedSelfPlay(lambda x: None, 2, n_playout=4, temp=0)
    with pytest.raises(CczError, match="temp"):
        BatchedMatch(None, None, 2, n_playout=4, temp=0)
