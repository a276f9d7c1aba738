"""Float64 references of the evaluator's kernels on fixed-point operands (a plain module, imported like golden_cases).

The idea. Put the activations on the grid 2^-ea, the weights on 2^-eb and the bias on g = 2^-(ea + eb): every product is a
multiple of g. If, for an output element,

    |bias| + sum |a| |w|  <  2^24 g                                                       (the exactness guard)

then every partial sum -- in any order, through any internal tree of an MFMA -- is a multiple of g below 2^24 g and therefore
exactly representable in float32: the fp32 accumulator holds the exact real sum s, the kernel's result is ONE fp16 number, and
a float64 reference computes it with no error at all. The comparison is equality, element for element; there is no tolerance.

The guard is a condition on the operands (a second float64 pass over absolute values), not a measurement of any kernel.
tests/test_cpu_evaluator_f64.py checks this module against float32 emulations in three summation orders and against a table of
deliberately wrong emulations; tests/test_gpu_evaluator_f64.py checks every kernel form against it.

rn16 is round-to-nearest-even from float64 (NumPy's astype(float16); torch would round through float32 first). An fp16 add is
rn16 of the exact float64 sum of two fp16 numbers. The chains, as the kernels document them:

    tower / stem convolution   y = relu?( rn16( rn16(bias + S) + res ) )   two roundings with a residual, one without
    head convolutions          rn16( relu(bias + S_256) )                   [board][pos][17] and [board][pos][7]
    FC (all three kernels)     rn16( relu?(bias + S_K) )
    value output               tanh( rn16(b2 + S_256) )                     nearest-candidate check, see value_candidates
    ccz_bias_act_f16           relu( rn16( rn16(y + b) + r ) )              pure fp16 adds: any fp16 operands

The planned boundary on board-major rows (tests/test_gpu_board_major_live.py): planned_cap / live_ranges restate how net.py sizes and
k_conv3x3_c256 cuts the live boards, conv_live_expected places the chain's rows in a filled buffer, pack_live_planes_rows is the
gathering plane pack; assert_same_bits compares bit patterns, for buffers whose untouched elements must keep their fill.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

EA, EB = 5, 10                      # the main grids: activations on 2^-5, weights on 2^-10, bias on 2^-15
LIMIT = 2.0 ** 24


# ------------------------------------------------------------------ rounding
def rn16(x):
    """float64 -> fp16, round to nearest even, straight from float64 (overflow -> inf, as the hardware conversion)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def add16(a, b):
    """the fp16 add of two fp16 arrays: rn16 of the exact sum"""
    return rn16(f64(a) + f64(b))


def needs_rounding(s):
    """share of the float64 values that are NOT fp16 numbers (the rounding point is exercised, not only the indexing)"""
    s = f64(s)
    return float((f64(rn16(s)) != s).mean())


# ------------------------------------------------------------------ operands on a grid (all float64, all exact fp16 / fp32 numbers)
def grid_normal(rs, shape, std, e, clip, relu=False):
    """round(N(0, std^2) * 2^e) clipped to +-clip grid steps, / 2^e; relu: negative values become 0"""
    v = rs.standard_normal(shape) * std
    if relu:
        v = np.maximum(v, 0.0)
    return np.clip(np.rint(v * 2.0 ** e), -clip, clip) / 2.0 ** e


def grid_acts(rs, shape, e=EA, std=0.7, relu=True):
    return grid_normal(rs, shape, std, e, 127, relu)            # |a| <= 127 / 32 on the main grid


def grid_weights(rs, shape, e=EB, std=0.03):
    return grid_normal(rs, shape, std, e, 128)                  # |w| <= 128 / 1024 on the main grid


def grid_bias(rs, shape, e=EA + EB, std=0.2):
    return np.rint(rs.standard_normal(shape) * std * 2.0 ** e) / 2.0 ** e


class GuardError(AssertionError):
    pass


def assert_guard(abs_sum, g, what=""):
    """abs_sum: |bias| + sum |a| |w| per output element (float64, exact). Returns max(abs_sum) / (2^24 g), which must be < 1."""
    worst = float(np.max(abs_sum)) / (LIMIT * g)
    if not worst < 1.0:
        raise GuardError(f"{what}: exactness guard fails: max |bias| + sum|a||w| = {float(np.max(abs_sum))!r} >= 2^24 g = {LIMIT * g!r}")
    return worst


def assert_on_grid(x, e, what=""):
    """every value a multiple of 2^-e and an fp16 number (what makes the products multiples of g)"""
    x = f64(x)
    if not (np.all(np.rint(x * 2.0 ** e) == x * 2.0 ** e) and np.all(f64(rn16(x)) == x)):
        raise GuardError(f"{what}: operand is not on the fp16 grid 2^-{e}")


def grid_exponent(x):
    """the smallest e with every value of x a multiple of 2^-e (fp16 numbers: e <= 24)"""
    x = f64(x)
    for e in range(0, 25):
        if np.all(np.rint(x * 2.0 ** e) == x * 2.0 ** e):
            return e
    raise GuardError("not fp16 numbers")


# ------------------------------------------------------------------ exact sums (float64)
def conv_sum64(x, w, bias):
    """x [B, 10, 9, Cin], w [Cout, 3, 3, Cin], bias [Cout] (float64) -> bias + 3x3 convolution, padding 1, [B, 10, 9, Cout]"""
    xt = torch.from_numpy(np.ascontiguousarray(f64(x))).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(f64(w))).permute(0, 3, 1, 2)
    y = F.conv2d(xt, wt, torch.from_numpy(np.ascontiguousarray(f64(bias))), padding=1)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def conv_exact(x, w, bias, g, what=""):
    """(s, worst, share): the exact sums, the guard's fill (asserted < 1) and the share of sums that need an fp16 rounding"""
    worst = assert_guard(conv_sum64(np.abs(x), np.abs(w), np.abs(bias)), g, what)
    s = conv_sum64(x, w, bias)
    return s, worst, needs_rounding(s)


def gemm_sum64(a, w, bias):
    """a [M, K], w [N, K], bias [N] -> bias + a w^T  [M, N]"""
    return f64(bias)[None, :] + f64(a) @ f64(w).T


def gemm_exact(a, w, bias, g, what=""):
    worst = assert_guard(gemm_sum64(np.abs(a), np.abs(w), np.abs(bias)), g, what)
    s = gemm_sum64(a, w, bias)
    return s, worst, needs_rounding(s)


# ------------------------------------------------------------------ the chains
def conv_chain(s, res=None, relu=True):
    """y = relu?( rn16( rn16(s) + res ) ) as fp16: the accumulator is rounded once, the residual is added in fp16"""
    y = rn16(s)
    if res is not None:
        y = add16(y, res)
    return np.maximum(y, np.float16(0)) if relu else y


def fc_chain(s, relu):
    """rn16( relu?(s) ): ReLU in fp32, one rounding"""
    return rn16(np.maximum(s, 0.0) if relu else s)


def heads_chain(s):
    """s [..., 24] -> (policy [..., 17], value [..., 7]) = rn16(relu(s)) split"""
    y = rn16(np.maximum(s, 0.0))
    return y[..., :17], y[..., 17:24]


def bias_act_chain(y, b, r=None):
    """relu( rn16( rn16(y + b) + r ) ) on fp16 arrays, b broadcast over rows"""
    t = add16(y, np.asarray(b)[None, :])
    if r is not None:
        t = add16(t, r)
    with np.errstate(invalid="ignore"):
        return np.maximum(t, np.float16(0))


def value_candidates(s):
    """s exact float64 [M] -> (tanh64(t), tanh64(lower fp16 neighbour of t), tanh64(upper one)), t = rn16(s)"""
    t = rn16(s)
    lo, hi = np.nextafter(t, np.float16(-np.inf)), np.nextafter(t, np.float16(np.inf))
    return np.tanh(f64(t)), np.tanh(f64(lo)), np.tanh(f64(hi))


def value_mismatches(v, s):
    """Rows where the device value v (float32) is NOT strictly closer to tanh64(rn16(s)) than to tanh64 of either fp16 neighbour
    of rn16(s). For |s| < 4 neighbouring candidates are >= 5e-6 (80 fp32 ulps) apart: this pins the fp16 rounding in front of the
    tanh and asks of tanhf only that it is better than 40 ulps."""
    c, lo, hi = value_candidates(s)
    v = f64(v)
    d = np.abs(v - c)
    ok = (d < np.abs(v - lo)) & (d < np.abs(v - hi))
    return np.flatnonzero(~ok)


# ------------------------------------------------------------------ comparison
def assert_same(got, want, what, names=None):
    """Equality on VALUES (-0 equals +0; NaN equals nothing), element for element. On failure: the first failing element's
    coordinates, both values, and the number of differing elements."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.astype(np.float64), want.astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~(g == w)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        where = ", ".join(f"{n} {i}" for n, i in zip(names, at)) if names else str(at)
        raise AssertionError(f"{what}: {where}: device {g[at]!r} vs float64 chain {w[at]!r}; {int(bad.sum())} of {bad.size} elements differ")


def assert_same_bits(got, want, what, names=None):
    """Equality on BIT PATTERNS of two fp16 arrays (-0 differs from +0, a NaN equals the same NaN): for buffers whose untouched
    elements hold a fill that must survive a call, 0xFFFF included. On failure: the first differing element and the count."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float16, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint16) != want.view(np.uint16)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        where = ", ".join(f"{n} {i}" for n, i in zip(names, at)) if names else str(at)
        raise AssertionError(f"{what}: {where}: device bits 0x{int(got.view(np.uint16)[at]):04x} vs expected 0x{int(want.view(np.uint16)[at]):04x}; "
                             f"{int(bad.sum())} of {bad.size} elements differ")


# ------------------------------------------------------------------ the planned boundary on board-major rows (restatements of the host code and the kernels' addressing)
def planned_cap(boards, n_parts):
    """pixels of the largest range one launch of the board-major live form may get, as InferenceNet.tower_schedule (planned) gives them:
    ceil(ceil(B / n_parts) / 8) * 8 * 90 (it may reach past the tensor: the kernel never computes more than the live boards)"""
    return -(-(-(-boards // n_parts)) // 8) * 8 * 90


def live_ranges(live, n_parts, cap_boards):
    """k_conv3x3_c256 with a live count: the first `live` boards cut into n_parts ranges of per = ceil(ceil(live / n_parts) / 8) * 8
    boards; range `part` starts at board part * per and holds min(per, live - part * per, cap_boards) boards (none when that is <= 0).
    -> [(first board, boards)] for part = 0 .. n_parts - 1"""
    per = -(-(-(-live // n_parts)) // 8) * 8
    return [(part * per, max(0, min(per, live - part * per, cap_boards))) for part in range(n_parts)]


def conv_live_expected(s, res, relu, ranges, fill):
    """What the launches of `ranges` leave in an output that held `fill` [B, 10, 9, C] fp16: conv_chain on the boards of every range,
    the fill everywhere else. (With the ranges of live_ranges: the chain on the first `live` boards.)"""
    out = np.array(fill, dtype=np.float16, copy=True)
    for first, n in ranges:
        if n > 0:
            out[first:first + n] = conv_chain(s[first:first + n], None if res is None else res[first:first + n], relu)
    return out


def pack_live_planes_rows(leaf, rows, n_rows, out, g16=False):
    """k_pack_live_planes in its gathering (planned) form on out [R, 64] fp16, R = 90 * boards (g16: 1440 * groups): for i < n_rows
    and pixel p, channels 0..20 of output row i * 90 + p (g16: ((i >> 4) * 90 + p) * 16 + (i & 15)) are planes 49..55 and 105..118 of
    board rows[i] (leaf [B, 119, 10, 9]), channels 21..23 are zero -- three 16-byte chunks; channels 24..63 and every other row keep
    what they held. Returns a copy."""
    out = np.array(out, dtype=np.float16, copy=True)
    leaf = np.asarray(leaf)
    p = np.arange(90)
    for i in range(int(n_rows)):
        b = int(rows[i])
        live = np.concatenate([leaf[b, 49:56], leaf[b, 105:119]], axis=0).reshape(21, 90).T        # [pixel, 21]
        at = ((i >> 4) * 90 + p) * 16 + (i & 15) if g16 else i * 90 + p
        out[at, :21] = live.astype(np.float16)
        out[at, 21:24] = 0
    return out


# ------------------------------------------------------------------ float32 emulations (the checker's own check; mutants build on them)
def im2col(x):
    """x [B, 10, 9, C] -> [B * 90, 9 * C], column (tap, ci), tap = 3 (dy + 1) + (dx + 1); taps that leave the board read zeros"""
    B, _, _, Cn = x.shape
    xp = np.zeros((B, 12, 11, Cn), x.dtype)
    xp[:, 1:11, 1:10] = x
    cols = [xp[:, 1 + dy:11 + dy, 1 + dx:10 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return np.stack(cols, axis=3).reshape(B * 90, 9 * Cn)


def chunk_order(cin, chunk=32):
    """the kernels' K order: chunks of 32 input channels (outer) x 9 taps x the chunk's channels, as im2col column indices"""
    return np.array([t * cin + c0 + c for c0 in range(0, cin, chunk) for t in range(9) for c in range(chunk)], dtype=np.int64)


def sum_f32(a, w, bias, order="ascending", round_every=None, perm_seed=0):
    """float32 emulation of acc = bias; acc += a[:, k] * w[:, k]: a [M, K], w [N, K] -> [M, N] float32.
    order: 'ascending' (k = 0, 1, ...), an index array (that order; also a subset of k), 'permuted' (a fixed random order),
    'pairwise' (all products first, halves added until the length is odd, the rest in sequence, the bias last).
    round_every: the accumulator is rounded to fp16 after every `round_every` steps (a MUTANT: the kernels never do that)."""
    a32, w32, b32 = np.asarray(a, np.float32), np.asarray(w, np.float32), np.asarray(bias, np.float32)
    M, K = a32.shape
    N = w32.shape[0]
    if isinstance(order, str) and order == "pairwise":
        out = np.empty((M, N), np.float32)
        for n0 in range(0, N, 32):
            p = a32[:, None, :] * w32[None, n0:n0 + 32, :]                  # products of two fp16 numbers: exact in float32
            while p.shape[-1] % 2 == 0:
                h = p.shape[-1] // 2
                p = p[..., :h] + p[..., h:]
            acc = p[..., 0]
            for k in range(1, p.shape[-1]):
                acc = acc + p[..., k]
            out[:, n0:n0 + 32] = acc + b32[None, n0:n0 + 32]
        return out
    if isinstance(order, str):
        ks = np.arange(K) if order == "ascending" else np.random.RandomState(perm_seed).permutation(K)
    else:
        ks = np.asarray(order)
    acc = np.broadcast_to(b32[None, :], (M, N)).copy()
    for i, k in enumerate(ks):
        acc += a32[:, k:k + 1] * w32[None, :, k]
        if round_every and (i + 1) % round_every == 0:
            with np.errstate(over="ignore"):
                acc = acc.astype(np.float16).astype(np.float32)
    return acc


def rn16_f32(acc):
    """the device's float32 -> fp16 conversion"""
    with np.errstate(over="ignore"):
        return np.asarray(acc, np.float32).astype(np.float16)


# ------------------------------------------------------------------ layout helpers (moved here from test_gpu_conv.py)
def _to_g16(t):
    """[B, C, 10, 9] channels-last (rows b * 90 + pos) -> the same bytes reordered to rows (g * 90 + pos) * 16 + j, board 16 g + j"""
    B, Cn = t.shape[0], t.shape[1]
    return t.permute(0, 2, 3, 1).reshape(B // 16, 16, 90, Cn).permute(0, 2, 1, 3).contiguous()


def _pack_w(w_nhwc, cin):
    """ccz_pack_conv_weights_g16_f16 on [256, 3, 3, cin] weights; must equal the torch twin the evaluator uses"""
    from chinesechesszero_amd import _lib
    from chinesechesszero_amd.net import pack_conv_weights_g16
    wp = torch.empty(cin // 32, 9, 256, 32, dtype=torch.float16, device=w_nhwc.device)
    s = C.c_void_p(torch.cuda.current_stream(w_nhwc.device).cuda_stream)
    _lib.check(_lib.lib().ccz_pack_conv_weights_g16_f16(s, C.c_void_p(w_nhwc.data_ptr()), C.c_void_p(wp.data_ptr()), cin))
    assert torch.equal(wp, pack_conv_weights_g16(w_nhwc.view(256, 3, 3, cin)))
    return wp


def _from_g16(t, B):
    Cn = t.shape[-1]
    return t.reshape(B // 16, 90, 16, Cn).permute(0, 2, 1, 3).reshape(B, 10, 9, Cn).permute(0, 3, 1, 2)


def rows_to_g16(x):
    """numpy / torch [B, 10, 9, C] (B a multiple of 16) -> group-of-16 rows [B // 16, 90, 16, C]"""
    B, Cn = x.shape[0], x.shape[-1]
    return x.reshape(B // 16, 16, 90, Cn).transpose(0, 2, 1, 3) if isinstance(x, np.ndarray) else x.reshape(B // 16, 16, 90, Cn).permute(0, 2, 1, 3)


def rows_from_g16(y, B):
    """the inverse: [B // 16, 90, 16, C] -> [B, 10, 9, C]"""
    Cn = y.shape[-1]
    t = y.reshape(B // 16, 90, 16, Cn)
    t = t.transpose(0, 2, 1, 3) if isinstance(t, np.ndarray) else t.permute(0, 2, 1, 3)
    return t.reshape(B, 10, 9, Cn)
