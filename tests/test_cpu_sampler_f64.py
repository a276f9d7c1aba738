"""CPU: the device-mode move sampler's arithmetic against float64 references (oracle/xq_sample.c, the operation-for-operation
twin of det_log / det_exp / det_gamma / k_finish_move's choice in csrc/cczero_device.h and csrc/cczero_kernels.h).

Self-play draws each move from (1 - eps) pi + eps Dirichlet(alpha 1_k) (mcts.py:216-224); the Dirichlet noise is the only
exploration in the training data. The device reproduces the twin bit for bit (tests/test_gpu_sampler_f64.py), so what is
pinned here against libm and the Gamma distribution holds for the kernel too.

- det_log against math.log: at most 2 ulp where |log x| > 1e-3 and at most 1.5e-14 absolute elsewhere (the series in
  atanh((m-1)/(m+1)) loses relative accuracy only where the result itself is near 0).
- det_exp against math.exp on [-708, 0]: at most 1 ulp; exactly 0 below -708 (the documented cutoff).
- raw Gamma(alpha) draws against the regularised incomplete gamma P(alpha, x) (torch.special.gammainc, float64), one-sample KS
  over 20000 draws spread over board ids >= 2^20 and two move numbers. Observed sqrt(n) D (threshold 2.0; the same draws
  against Gamma(alpha + 1), the sampler without its U^(1/alpha) boost, and against Gamma(alpha / 2)):
      alpha   0.03    0.2     f32(0.2)  0.3     1.0     2.5
      D       0.657   0.546   0.546     0.448   0.590   0.514
      a+1     125.7   91.6    91.6      81.5    52.6    34.3
      a/2     35.3    36.0    36.0      36.6    43.1    56.2
  Raw draws are compared, not Dirichlet components: at alpha = 0.03, k = 2 the larger component rounds to exactly 1.0 in 16 %
  of draws (numpy.random.dirichlet does the same), which a KS test on the upper tail would flag.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle

SEED = 2024
ALPHAS = (0.03, 0.2, float(np.float32(0.2)), 0.3, 1.0, 2.5)


def _ulps(got, want):
    return abs(got - want) / math.ulp(want) if want != 0 else (0.0 if got == 0 else math.inf)


def _log_inputs():
    xs = [n + 1e-10 for n in range(0, 1_000_001)]                      # root_pi: log(N + 1e-10)
    rs = np.random.RandomState(5)
    xs += list(rs.uniform(0.0, 1.0, 20000) ** 2)                         # polar s = x1^2 + x2^2 in (0, 1)
    xs += list(np.exp(rs.uniform(math.log(1.1e-16), 0.0, 20000)))        # Philox uniforms, log-spaced
    xs += [1.1102230246251565e-16, 1.0 - 1.1102230246251565e-16, 0.5, 1.0]
    xs += [1.0 - i * 1.1102230246251565e-16 for i in range(1, 200)]      # uniforms next to 1 (|log u| tiny)
    for c in [math.sqrt(2.0)] + [2.0 ** e for e in range(-60, 61)]:      # the mantissa fold and the exponent steps
        xs += [c, math.nextafter(c, 0.0), math.nextafter(c, math.inf)]
    return [x for x in xs if x > 0.0]


def test_det_log_within_two_ulp_of_libm():
    L = oracle.lib()
    worst_ulp = worst_abs = 0.0
    for x in _log_inputs():
        got, want = L.xq_det_log(x), math.log(x)
        if abs(want) > 1e-3:
            worst_ulp = max(worst_ulp, _ulps(got, want))
        else:
            worst_abs = max(worst_abs, abs(got - want))
    assert worst_ulp <= 2.0, worst_ulp
    assert worst_abs <= 1.5e-14, worst_abs
    assert L.xq_det_log(1.0) == 0.0


def test_det_exp_within_one_ulp_of_libm_and_its_cutoff():
    L = oracle.lib()
    rs = np.random.RandomState(6)
    xs = list(rs.uniform(-708.0, 0.0, 20000)) + list(-np.exp(rs.uniform(-40, 0, 2000)))
    xs += [-708.0, -707.9999999999999, -1e-300, -0.5 * math.log(2.0), -math.log(2.0), -700.0 * math.log(2.0)]
    worst = max(_ulps(L.xq_det_exp(x), math.exp(x)) for x in xs)
    assert worst <= 1.0, worst
    assert L.xq_det_exp(0.0) == 1.0
    for x in (-708.0000000000001, -709.0, -745.0, -1e6, -math.inf):
        assert L.xq_det_exp(x) == 0.0, x


def _ks(x, cdf):
    x = np.sort(x)
    n = len(x)
    i = np.arange(1, n + 1)
    f = cdf(x)
    return math.sqrt(n) * max(float((i / n - f).max()), float((f - (i - 1) / n).max()))


def _gamma_cdf(a):
    return lambda x: torch.special.gammainc(torch.full((len(x),), a, dtype=torch.float64), torch.from_numpy(x)).numpy()


def _draws(alpha):
    # 2 moves x 500 boards x 20 children = 20000 draws; board ids past 2^20 and per-move offsets
    return np.concatenate([oracle.det_gammas(SEED, 10**6 + 977 * m, 500, m, 20, alpha).ravel() for m in range(2)])


@pytest.mark.parametrize("alpha", ALPHAS)
def test_raw_gamma_draws_follow_gamma_alpha(alpha):
    g = _draws(alpha)
    assert len(g) >= 20000 and np.all(np.isfinite(g)) and np.all(g >= 0.0)
    assert _ks(g, _gamma_cdf(alpha)) < 2.0
    # power, on the same draws: without the U^(1/alpha) boost the draws would be Gamma(alpha + 1); a halved alpha is also far off
    assert _ks(g, _gamma_cdf(alpha + 1.0)) > 20.0
    assert _ks(g, _gamma_cdf(alpha / 2.0)) > 20.0


def test_a_float32_alpha_is_its_own_stream():
    """ccz_config.alpha is a float: the device runs with 0.20000000298..., so a twin called with 0.2 draws other numbers."""
    a32 = float(np.float32(0.2))
    assert a32 != 0.2
    g, g32 = oracle.det_gammas(SEED, 0, 4, 0, 44, 0.2), oracle.det_gammas(SEED, 0, 4, 0, 44, a32)
    assert not np.array_equal(g, g32)
    assert np.allclose(g, g32, rtol=1e-6, atol=1e-300)


def _pi(k, rs):
    return oracle.det_pi(rs.randint(0, 30, size=k), 1.0)


@pytest.mark.parametrize("k", (1, 2, 44, 108))
def test_mixed_vector_invariants_and_the_choice(k):
    rs = np.random.RandomState(k)
    for board in range(200):
        pi = _pi(k, rs)
        board_id = (1 << 32) + board
        for eps in (0.0, 0.25, 1.0):
            idx, mixed = oracle.det_sample(SEED, board_id, 3, pi, eps, 0.2)
            if eps == 0.0:
                assert np.array_equal(mixed, pi)
            assert np.all(mixed >= 0.0)
            assert abs(mixed.sum() - 1.0) <= k * 2.0 ** -52
            u = oracle.det_choice_uniform(SEED, board_id, 3)
            assert 0.0 < u < 1.0
            cdf = np.cumsum(mixed)
            assert idx == min(int(np.searchsorted(cdf / cdf[-1], u, side="right")), k - 1)


@pytest.mark.parametrize("alpha", (0.03, 0.2, 1.0))
def test_dirichlet_moments_at_eps_one(alpha):
    """eps = 1: the mixed vector is Dirichlet(alpha 1_k); mean 1/k, variance (k-1)/(k^2 (k alpha + 1)), within 5 standard errors.
    At alpha = 0.2, k = 44 the variance is 2.27e-3; without the boost (Gamma(alpha + 1) draws) it would be 4.1e-4."""
    k, n = 44, 4000
    pi = np.full(k, 1.0 / k)
    x = np.stack([oracle.det_sample(SEED, 7 << 20 | b, 1, pi, 1.0, alpha)[1] for b in range(n)])
    var = (k - 1) / (k * k * (k * alpha + 1))
    for i in (0, 17, 43):
        c = x[:, i]
        assert abs(c.mean() - 1.0 / k) < 5 * math.sqrt(var / n), (i, c.mean())
        d2 = (c - 1.0 / k) ** 2
        assert abs(d2.mean() - var) < 5 * d2.std() / math.sqrt(n), (i, d2.mean(), var)
    assert abs(x.var() - var) < 0.1 * var


def test_nan_alpha_terminates_and_falls_back_to_pi():
    """The twin's det_gamma is bounded as the device's is: a NaN alpha gives 0.0 after 0xffff0 draws instead of looping."""
    g = oracle.det_gammas(SEED, 0, 1, 0, 2, math.nan)
    assert np.array_equal(g, np.zeros((1, 2)))
    pi = np.array([0.25, 0.75])
    idx, mixed = oracle.det_sample(SEED, 0, 0, pi, 0.25, math.nan)
    assert np.array_equal(mixed, pi) and idx in (0, 1)


@pytest.mark.parametrize("field,value,word", [
    ("eps", math.nan, b"eps"), ("eps", -0.01, b"eps"), ("eps", 1.5, b"eps"),
    ("alpha", math.nan, b"alpha"), ("alpha", 0.0, b"alpha"), ("alpha", -0.2, b"alpha"), ("alpha", math.inf, b"alpha"),
    ("temp", math.nan, b"temp"), ("temp", 0.0, b"temp"), ("temp", -1.0, b"temp"),
])
def test_ccz_create_rejects_sampler_parameters(field, value, word):
    """Checked before any device work, so this holds with or without a GPU."""
    from chinesechesszero_amd import _lib
    L = _lib.lib()
    kw = dict(n_boards=2, n_playout=4, c_puct=5, eps=0.25, alpha=0.2, temp=1.0)
    kw[field] = value
    cfg = _lib.Config(**kw)
    h = ctypes.c_void_p()
    assert L.ccz_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert not h.value
    msg = L.ccz_last_error()
    assert b"ccz_create" in msg and word in msg, msg
