"""CPU: tests/evaluator_f64.py checked against itself -- no GPU.

(1) On grid operands that pass the exactness guard, a float32 emulation of every operation equals the float64 reference bit for
    bit in three summation orders (ascending k, k permuted, pairwise): the accumulator of ANY order holds the exact sum, so the
    expected fp16 output is unique -- the claim test_gpu_evaluator_f64.py rests on.
(2) The guard refuses full-mantissa operands.
(3) A table of deliberately wrong float32 emulations (mutants). Equality with the float64 chain rejects every one of them; the
    table also records whether the rule the suite used before (max-normed 4e-3 for convolutions, allclose for FC / heads / value)
    would have accepted the mutant. The table is printed (pytest -s shows it; CHANGELOG.md quotes it)."""
import numpy as np
import pytest

import evaluator_f64 as E

G = 2.0 ** -(E.EA + E.EB)


# ------------------------------------------------------------------ operands (module-level caches: the float64 passes take seconds)
_cache = {}


def _conv_case():
    """Three boards, 256 -> 256, the operand distributions of tests/test_gpu_conv.py on the grids 2^-5 / 2^-10 / 2^-15."""
    if "conv" not in _cache:
        rs = np.random.RandomState(1)
        x = E.grid_acts(rs, (3, 10, 9, 256))
        r = E.grid_acts(rs, (3, 10, 9, 256), relu=False)
        w = E.grid_weights(rs, (256, 3, 3, 256))
        b = E.grid_bias(rs, 256)
        s, worst, share = E.conv_exact(x, w, b, G, "conv")
        X2, W2 = E.im2col(x), w.reshape(256, -1)
        acc = E.sum_f32(X2, W2, b)                                     # ascending k, float32
        _cache["conv"] = dict(x=x, r=r, w=w, b=b, s=s, worst=worst, share=share, X2=X2, W2=W2, acc=acc)
    return _cache["conv"]


def _emul_conv_chain(acc, res, relu):
    """the chain in float32 / fp16 arithmetic, as the kernel's epilogue runs it"""
    y = E.rn16_f32(acc)
    if res is not None:
        y = E.rn16_f32(y.astype(np.float32) + np.asarray(res, np.float32))   # an fp16 add (24 bits >= 2 * 11 + 2: correctly rounded)
    return np.maximum(y, np.float16(0)) if relu else y


def _fc_case():
    if "fc" not in _cache:
        rs = np.random.RandomState(2)
        M, K, N, lda = 5, 192, 130, 200
        buf = np.full((M, lda), 0.5)                                   # the columns between K and lda: never read
        buf[:, :K] = E.grid_acts(rs, (M, K), std=1.0)
        w = np.zeros((256, K))
        w[:N] = E.grid_weights(rs, (N, K))
        b = np.zeros(256)
        b[:N] = E.grid_bias(rs, N, std=0.3)
        s, worst, share = E.gemm_exact(buf[:, :K], w[:N], b[:N], G, "fc")
        _cache["fc"] = dict(M=M, K=K, N=N, lda=lda, buf=buf, a=buf[:, :K], w=w, b=b, s=s, worst=worst, share=share)
    return _cache["fc"]


def _heads_case():
    if "heads" not in _cache:
        rs = np.random.RandomState(3)
        x = E.grid_acts(rs, (2 * 90, 256), std=1.0)
        w = E.grid_weights(rs, (24, 256), std=0.08)
        b = E.grid_bias(rs, 24)
        s, worst, share = E.gemm_exact(x, w, b, G, "heads")
        _cache["heads"] = dict(x=x, w=w, b=b, s=s, worst=worst, share=share)
    return _cache["heads"]


def _value_case():
    if "value" not in _cache:
        rs = np.random.RandomState(4)
        h = E.grid_acts(rs, (64, 256), std=1.0)
        w2 = E.grid_weights(rs, (1, 256), std=0.05)
        b2 = np.array([0.125])
        s, worst, _ = E.gemm_exact(h, w2, b2, G, "value")
        assert np.abs(s).max() < 4
        _cache["value"] = dict(h=h, w2=w2, b2=b2, s=s[:, 0], worst=worst)
    return _cache["value"]


ORDERS = ["ascending", "permuted", "pairwise"]


# ------------------------------------------------------------------ (1) the reference against float32 emulations
@pytest.mark.parametrize("order", ORDERS)
def test_convolution_reference_equals_float32_emulation_in_any_order(order):
    c = _conv_case()
    assert c["worst"] < 1 and c["share"] >= 0.5, (c["worst"], c["share"])
    acc = c["acc"] if order == "ascending" else E.sum_f32(c["X2"], c["W2"], c["b"], order)
    assert np.array_equal(acc.astype(np.float64).reshape(c["s"].shape), c["s"])        # the accumulator IS the exact sum
    for res, relu in ((None, True), (c["r"], True), (None, False), (c["r"], False)):
        want = E.conv_chain(c["s"], res, relu)
        got = _emul_conv_chain(acc, None if res is None else res.reshape(-1, 256), relu).reshape(want.shape)
        E.assert_same(got, want, f"conv {order} res={res is not None} relu={relu}", ("board", "rank", "file", "channel"))
    if order == "ascending":
        print(f"\nconv 3 boards: guard fill {c['worst']:.4f} (max sum|a||w| + |b| = {c['worst'] * 512:.1f} of 512), needs rounding {c['share']:.2f}")


def test_convolution_in_the_kernels_chunk_order_equals_the_reference():
    """chunks of 32 input channels x 9 taps: the order all convolution kernels add in"""
    c = _conv_case()
    acc = E.sum_f32(c["X2"][:90], c["W2"], c["b"], E.chunk_order(256))
    assert np.array_equal(acc.astype(np.float64), c["s"][0].reshape(90, 256))


@pytest.mark.parametrize("order", ORDERS)
def test_stem_reference_equals_float32_emulation(order):
    """64 input channels, 21 live, a 0/1 input (on every grid), no residual"""
    rs = np.random.RandomState(5)
    x = np.zeros((2, 10, 9, 64))
    x[..., :21] = rs.random_sample((2, 10, 9, 21)) > 0.8
    w = np.zeros((256, 3, 3, 64))
    w[..., :21] = E.grid_weights(rs, (256, 3, 3, 21), std=0.05)
    b = E.grid_bias(rs, 256)
    s, worst, share = E.conv_exact(x, w, b, 2.0 ** -15, "stem")
    assert share >= 0.5, share
    acc = E.sum_f32(E.im2col(x), w.reshape(256, -1), b, order)
    for relu in (True, False):
        E.assert_same(_emul_conv_chain(acc, None, relu).reshape(s.shape), E.conv_chain(s, None, relu), f"stem {order}")


@pytest.mark.parametrize("order", ORDERS)
def test_head_convolution_reference_equals_float32_emulation(order):
    c = _heads_case()
    acc = E.sum_f32(c["x"], c["w"], c["b"], order)
    got = E.rn16_f32(np.maximum(acc, 0))
    pol, val = E.heads_chain(c["s"])
    E.assert_same(got[:, :17], pol, f"policy head {order}")
    E.assert_same(got[:, 17:], val, f"value head {order}")
    # ReLU zeroes about half of the sums and a zero needs no rounding: the share is taken over the outputs that survive it
    assert E.needs_rounding(np.maximum(c["s"], 0)) >= 0.25 and E.needs_rounding(c["s"]) >= 0.5


@pytest.mark.parametrize("order", ORDERS)
def test_heads_in_the_last_layer_reference_equals_float32_emulation(order):
    """The head convolution on the fp16 y of the layer above. y is a multiple of 2^-15, so the head weights sit on the coarser
    grid 2^-4 and the head bias on 2^-19: g = 2^-19 for the second guard."""
    c = _conv_case()
    rs = np.random.RandomState(6)
    y = E.conv_chain(c["s"][:1], np.maximum(c["r"][:1], 0), True).astype(np.float64).reshape(90, 256)
    E.assert_on_grid(y, 15)
    wh = E.grid_normal(rs, (24, 256), 0.08, 4, 4)
    bh = E.grid_bias(rs, 24, e=19)
    s, worst, share = E.gemm_exact(y, wh, bh, 2.0 ** -19, "heads on y")
    acc = E.sum_f32(y, wh, bh, order)
    assert np.array_equal(acc.astype(np.float64), s)
    pol, val = E.heads_chain(s)
    got = E.rn16_f32(np.maximum(acc, 0))
    E.assert_same(got[:, :17], pol, "policy")
    E.assert_same(got[:, 17:], val, "value")


@pytest.mark.parametrize("order", ORDERS)
def test_fc_reference_equals_float32_emulation(order):
    c = _fc_case()
    assert c["share"] >= 0.5
    acc = E.sum_f32(c["a"], c["w"][:c["N"]], c["b"][:c["N"]], order)
    for relu in (False, True):
        E.assert_same(E.rn16_f32(np.maximum(acc, 0) if relu else acc), E.fc_chain(c["s"], relu), f"fc {order}", ("row", "column"))


@pytest.mark.parametrize("order", ORDERS)
def test_value_output_reference_accepts_the_float32_emulation(order):
    c = _value_case()
    acc = E.sum_f32(c["h"], c["w2"], c["b2"], order)[:, 0]
    assert np.array_equal(acc.astype(np.float64), c["s"])
    v = np.tanh(E.rn16_f32(acc).astype(np.float32))
    assert E.value_mismatches(v, c["s"]).size == 0
    cand, lo, hi = E.value_candidates(c["s"])
    assert min(np.abs(cand - lo).min(), np.abs(cand - hi).min()) > 5e-6       # what the check assumes of |s| < 4


def test_bias_act_reference_equals_fp16_arithmetic_emulated_in_float32():
    rs = np.random.RandomState(7)
    bits = rs.randint(0, 0x7c00, size=(300, 64)).astype(np.uint16) | (rs.randint(0, 2, size=(300, 64)).astype(np.uint16) << 15)
    y, r = bits.view(np.float16), np.roll(bits, 7).view(np.float16)          # every finite fp16 pattern class: subnormals, huge
    b = (rs.standard_normal(64) * 100).astype(np.float16)
    for res in (None, r):
        with np.errstate(over="ignore", invalid="ignore"):
            t = (y.astype(np.float32) + b.astype(np.float32)[None, :]).astype(np.float16)
            if res is not None:
                t = (t.astype(np.float32) + res.astype(np.float32)).astype(np.float16)
            got = np.maximum(t, np.float16(0))
        E.assert_same(got, E.bias_act_chain(y, b, res), "bias_act")
    assert np.isinf(E.bias_act_chain(y, b, r).astype(np.float64)).any()       # sums that overflow are in the operand set


# ------------------------------------------------------------------ (2) the guard
def test_guard_refuses_full_mantissa_operands():
    rs = np.random.RandomState(8)
    x = np.maximum(rs.standard_normal((1, 10, 9, 256)) * 0.7, 0).astype(np.float16).astype(np.float64)
    w = (rs.standard_normal((256, 3, 3, 256)) * 0.03).astype(np.float16).astype(np.float64)
    b = rs.standard_normal(256) * 0.2
    with pytest.raises(E.GuardError):
        E.assert_on_grid(x, E.EA)
    with pytest.raises(E.GuardError):
        E.assert_on_grid(w, E.EB)
    ea, eb = E.grid_exponent(x), E.grid_exponent(w)                           # the grid such operands really are on
    assert ea > 12 and eb > 12
    with pytest.raises(E.GuardError):
        E.conv_exact(x, w, np.rint(b * 2.0 ** (ea + eb)) / 2.0 ** (ea + eb), 2.0 ** -(ea + eb), "randn")
    # and the same sums really are inexact in float32: two orders disagree
    X2, W2 = E.im2col(x)[:8], w.reshape(256, -1)
    assert not np.array_equal(E.sum_f32(X2, W2, b), E.sum_f32(X2, W2, b, "permuted"))
    # grid operands scaled up until the bound is crossed are refused too
    c = _conv_case()
    with pytest.raises(E.GuardError):
        E.assert_guard(E.conv_sum64(np.abs(c["x"][:1]), np.abs(c["w"]) * 64, np.abs(c["b"])), G, "scaled")


# ------------------------------------------------------------------ (3) the mutation table
def _old_conv(got, want):
    """tests/test_gpu_conv.py: err < 4e-3 * max(1, max|want|), one number for the whole tensor"""
    return bool(np.abs(got.astype(np.float64) - want).max() < 4e-3 * max(1.0, np.abs(want).max()))


def _old_allclose(atol, rtol):
    return lambda got, want: bool(np.all(np.abs(got.astype(np.float64) - want) <= atol + rtol * np.abs(want)))


def _conv_mutants():
    """name -> fp16 output [270, 256] of a wrong emulation; residual and ReLU on, as the evaluator runs the layer"""
    c = _conv_case()
    x, X2, W2, b, acc = c["x"], c["X2"], c["W2"], c["b"], c["acc"]
    r = c["r"].reshape(-1, 256)
    ref = E.conv_chain(c["s"], c["r"], True).reshape(-1, 256)
    out = {}

    def finish(a):
        return _emul_conv_chain(a, r, True)

    # one product dropped at a corner pixel (board 1, position 0; the channel with the largest output; a median-sized product)
    p = 90
    co = int(np.argmax(ref[p].astype(np.float64)))
    prod = np.abs(X2[p] * W2[co])
    nz = np.flatnonzero(prod)
    k = int(nz[np.argsort(prod[nz])[len(nz) // 2]])
    a = acc.copy()
    a[p, co] = E.sum_f32(X2[p:p + 1], W2[co:co + 1], b[co:co + 1], np.delete(np.arange(2304), k))[0, 0]
    out["one product dropped at a corner pixel"] = finish(a)
    # taps dx = -1 / +1 exchanged on files 0 and 8 only
    Xm = X2.reshape(3, 10, 9, 9, 256).copy()
    for f in (0, 8):
        Xm[:, :, f, [0, 2]] = Xm[:, :, f, [2, 0]]
        Xm[:, :, f, [3, 5]] = Xm[:, :, f, [5, 3]]
        Xm[:, :, f, [6, 8]] = Xm[:, :, f, [8, 6]]
    rows = np.flatnonzero(np.isin(np.arange(270) % 9, (0, 8)))
    a = acc.copy()
    a[rows] = E.sum_f32(Xm.reshape(270, -1)[rows], W2, b)
    out["taps dx -1 / +1 swapped on files 0 and 8"] = finish(a)
    # position 89 of a board reads position 0 of the next board in tap (0, +1): no zero padding across the board boundary
    Xm = X2.reshape(270, 9, 256).copy()
    for bd in range(2):
        Xm[bd * 90 + 89, 5] = x[bd + 1, 0, 0]
    a = acc.copy()
    a[[89, 179]] = E.sum_f32(Xm.reshape(270, -1)[[89, 179]], W2, b)
    out["position 89 reads position 0 of the next board"] = finish(a)
    # the group-of-16 analogue: neighbouring rows are the SAME position of the neighbouring board of the group
    Xm = X2.reshape(270, 9, 256).copy()
    for bd in range(3):
        Xm[bd * 90 + 89, 5] = x[(bd + 1) % 3, 9, 8]
    a = acc.copy()
    a[[89, 179, 269]] = E.sum_f32(Xm.reshape(270, -1)[[89, 179, 269]], W2, b)
    out["group-of-16: position 89 reads the neighbouring board"] = finish(a)
    # the residual added in fp32, one rounding
    out["residual added in fp32, single rounding"] = np.maximum(E.rn16_f32(acc + r.astype(np.float32)), np.float16(0))
    # ReLU in front of the residual add
    out["ReLU applied before the residual"] = E.rn16_f32(np.maximum(E.rn16_f32(acc), np.float16(0)).astype(np.float32) + r.astype(np.float32))
    # the bias of channel c + 1 for one channel
    a = acc.copy()
    a[:, 100] = (acc[:, 100].astype(np.float64) - b[100] + b[101]).astype(np.float32)
    out["bias of channel c+1 used for one channel"] = finish(a)
    # the accumulator rounded to fp16 between the 32-channel chunks of the K loop
    out["accumulator rounded to fp16 between 32-channel chunks"] = finish(E.sum_f32(X2, W2, b, E.chunk_order(256), round_every=288))
    want_old = np.maximum(c["s"].reshape(-1, 256) + r, 0)
    return ref, want_old, out


def _mutation_table():
    if "table" in _cache:
        return _cache["table"]
    rows = []                                                                 # (mutant, old rule accepts, equality rejects, elements that differ)

    def add(name, got, ref, old):
        with np.errstate(invalid="ignore"):
            diff = ~(np.asarray(got).astype(np.float64) == np.asarray(ref).astype(np.float64))
        rows.append((name, old, bool(diff.any()), f"{int(diff.sum())} of {diff.size}"))

    ref, want_old, mutants = _conv_mutants()
    assert _old_conv(ref, want_old)                                           # (the old rule accepts the right answer)
    for name, got in mutants.items():
        add(name, got, ref, _old_conv(got, want_old))
    # FC (the policy layer's form: no ReLU)
    c = _fc_case()
    M, K, N, lda = c["M"], c["K"], c["N"], c["lda"]
    wN, bN = c["w"][:N], c["b"][:N]
    ref = E.fc_chain(c["s"], False)
    old = _old_allclose(1.5e-2, 4e-3)
    assert old(ref, c["s"])
    add("FC: the last 64 of K dropped", E.rn16_f32(E.sum_f32(c["a"], wN, bN, np.arange(K - 64))), ref, old(E.rn16_f32(E.sum_f32(c["a"], wN, bN, np.arange(K - 64))), c["s"]))
    got = ref.copy()
    got[:, N - 1] = E.rn16_f32(E.sum_f32(c["a"], c["w"][N:N + 1], c["b"][N:N + 1]))[:, 0]
    add("FC: row N-1 taken from a zero pad row", got, ref, old(got, c["s"]))
    a_bad = c["buf"].reshape(-1)[:M * K].reshape(M, K)
    got = E.rn16_f32(E.sum_f32(a_bad, wN, bN))
    add("FC: lda ignored", got, ref, old(got, c["s"]))
    # heads
    c = _heads_case()
    pol, val = E.heads_chain(c["s"])
    ref = np.concatenate([pol, val], axis=1)
    got = ref.copy()
    got[:, [16, 17]] = got[:, [17, 16]]
    old = _old_allclose(2e-3, 2e-3)
    want = np.maximum(c["s"], 0)
    assert old(ref, want)
    add("heads: policy channel 16 and value channel 0 exchanged", got, ref, old(got, want))
    # value output: the new rule is the nearest-candidate check
    c = _value_case()
    v = np.tanh(c["s"]).astype(np.float32)
    want = np.tanh(E.rn16(c["s"]).astype(np.float64))
    bad = E.value_mismatches(v, c["s"])
    rows.append(("value output: tanh(s) without the fp16 rounding", bool(np.all(np.abs(v - want) <= 2e-3)), bad.size > 0, f"{bad.size} of {v.size} rows"))
    _cache["table"] = rows
    return rows


def format_table(rows):
    lines = ["| mutant | old rule | equality with float64 | elements that differ |", "|---|---|---|---|"]
    for name, old, new, share in rows:
        lines.append(f"| {name} | {'accepts' if old else 'rejects'} | {'rejects' if new else 'ACCEPTS'} | {share} |")
    return "\n".join(lines)


def test_mutation_table():
    rows = _mutation_table()
    print("\n" + format_table(rows))
    assert len(rows) == 13
    for name, old, new, share in rows:
        assert new, f"the equality check accepts the mutant: {name}"
    by_name = {r[0]: r for r in rows}
    # the two slips the max-normed tolerance lets through (a K-loop rewrite that keeps the accumulator in fp16 between chunks;
    # an epilogue that adds the residual before the rounding)
    assert by_name["accumulator rounded to fp16 between 32-channel chunks"][1]
    assert by_name["residual added in fp32, single rounding"][1]


# ------------------------------------------------------------------ (4) the planned boundary on board-major rows (tests/test_gpu_board_major_live.py)
def test_live_ranges_cover_the_live_boards_once_inside_the_capacity():
    """live_ranges restates the range arithmetic of k_conv3x3_c256: for every live count up to the batch and 1..6 parts the ranges
    start on multiples of 8 boards, do not overlap, never exceed the capacity the planned tower_schedule gives, and together are [0, live)."""
    assert E.planned_cap(40, 1) == 40 * 90 and E.planned_cap(40, 3) == 16 * 90 and E.planned_cap(40, 6) == 8 * 90
    assert E.planned_cap(37, 1) == 40 * 90 and E.planned_cap(600, 2) == 304 * 90 and E.planned_cap(11, 1) == 16 * 90
    assert E.live_ranges(9, 3, 16) == [(0, 8), (8, 1), (16, 0)]
    assert E.live_ranges(40, 6, 8) == [(0, 8), (8, 8), (16, 8), (24, 8), (32, 8), (40, 0)]
    assert E.live_ranges(0, 1, 40) == [(0, 0)] and E.live_ranges(17, 2, 24) == [(0, 16), (16, 1)]
    for B in (11, 37, 40, 600):
        for n_parts in range(1, 7):
            cap = E.planned_cap(B, n_parts) // 90
            for live in range(0, B + 1):
                ranges = E.live_ranges(live, n_parts, cap)
                assert len(ranges) == n_parts
                covered = np.zeros(B, np.int32)
                for first, n in ranges:
                    assert first % 8 == 0 and 0 <= n <= cap
                    covered[first:first + n] += 1
                    assert n == 0 or first + n <= B                              # (an empty range may start past the batch: it addresses nothing)
                assert np.all(covered[:live] == 1) and np.all(covered[live:] == 0), (B, n_parts, live)


def _live_case():
    """24 boards of 8 channels: any float64 sums do (the references below only place conv_chain's rows)"""
    rs = np.random.RandomState(12)
    s = rs.standard_normal((24, 10, 9, 8)) * 3
    r = E.grid_acts(rs, (24, 10, 9, 8), relu=False)
    fill = np.full((24, 10, 9, 8), -1, np.int16).view(np.float16)            # 0xFFFF: what an arena holds
    return s, r, fill


def test_live_reference_rejects_a_part_boundary_moved_by_eight_boards():
    s, r, fill = _live_case()
    ranges = E.live_ranges(17, 2, 16)
    want = E.conv_live_expected(s, r, True, ranges, fill)
    E.assert_same(want[:17], E.conv_chain(s[:17], r[:17], True), "live reference")
    assert np.all(want.view(np.int16)[17:] == -1)
    E.assert_same_bits(want, E.conv_live_expected(s, r, True, [(0, 17)], fill), "one part")       # the cut itself changes nothing
    # part 1 starts eight boards late (its end stays): boards 16.. keep the fill
    late = E.conv_live_expected(s, r, True, [(0, 16), (24, 0)], fill)
    with pytest.raises(AssertionError, match="board 16"):
        E.assert_same(late[:17], want[:17], "late part", ("board", "rank", "file", "channel"))
    with pytest.raises(AssertionError):
        E.assert_same_bits(late, want, "late part")
    # full case, three parts of eight: the middle part moved up by eight boards leaves boards 8..15 unwritten
    want24 = E.conv_live_expected(s, r, True, E.live_ranges(24, 3, 8), fill)
    moved = E.conv_live_expected(s, r, True, [(0, 8), (16, 8), (16, 8)], fill)
    with pytest.raises(AssertionError, match="board 8"):
        E.assert_same(moved, want24, "moved part", ("board", "rank", "file", "channel"))
    # the last range ends eight boards late: rows past the live count are written -- values cannot see it, the bit comparison does
    long = E.conv_live_expected(s, r, True, [(0, 16), (16, 8)], fill)
    E.assert_same(long[:17], want[:17], "long part")
    with pytest.raises(AssertionError):
        E.assert_same_bits(long, want, "long part")
    # the residual of another range (R not moved with Y)
    wrong_r = E.conv_live_expected(s, np.roll(r, 8, axis=0), True, ranges, fill)
    with pytest.raises(AssertionError):
        E.assert_same(wrong_r[:17], want[:17], "residual of another range")


@pytest.mark.parametrize("g16", [False, True])
def test_pack_restatement_against_plain_indexing_and_swapped_chunks(g16):
    rs = np.random.RandomState(5 + g16)
    B = 20
    leaf = (rs.random_sample((B, 119, 10, 9)) > 0.7).astype(np.float16)
    leaf[:, :7] = 1
    rows = rs.permutation(B).astype(np.int32)
    R = 2 * 1440 if g16 else B * 90
    for n_rows in (0, 1, 11, 20):
        out = np.full((R, 64), 7.5, np.float16)                                  # sentinel A
        out[:, 24:] = -3.25                                                      # sentinel B
        got = E.pack_live_planes_rows(leaf, rows, n_rows, out, g16)
        planes = list(range(49, 56)) + list(range(105, 119))
        want = out.copy()
        for i in range(n_rows):
            for p in range(90):
                at = ((i // 16) * 90 + p) * 16 + i % 16 if g16 else i * 90 + p
                for c in range(24):
                    want[at, c] = leaf[rows[i], planes[c], p // 9, p % 9] if c < 21 else 0
        E.assert_same_bits(got, want, f"pack restatement n_rows {n_rows}")
        assert np.all(got[:, 24:] == np.float16(-3.25))
        if n_rows == 0:
            E.assert_same_bits(got, out, "nothing written")
            continue
        assert (got[:, :24] == 7.5).sum() == (R - 90 * n_rows) * 24 and got[:, :21].astype(np.float64).sum() > 0
        swapped = got.copy()                                                     # two 16-byte chunks of every written row exchanged
        live = np.flatnonzero(got[:, 21] == 0)
        swapped[live, 0:8], swapped[live, 8:16] = got[live, 8:16], got[live, 0:8]
        with pytest.raises(AssertionError):
            E.assert_same_bits(swapped, want, "swapped chunks")
        other = E.pack_live_planes_rows(leaf, np.roll(rows, 1), n_rows, out, g16)   # the boards of another permutation
        with pytest.raises(AssertionError):
            E.assert_same_bits(other, want, "other rows")


def test_bit_comparison_sees_what_value_comparison_cannot():
    a = np.array([0.0, 1.0, np.nan], np.float16)
    b = np.array([-0.0, 1.0, np.nan], np.float16)
    E.assert_same_bits(a, a.copy(), "same NaN")
    with pytest.raises(AssertionError):
        E.assert_same_bits(a, b, "signed zero")
    E.assert_same(a[:2], b[:2], "values")
    with pytest.raises(AssertionError):
        E.assert_same(a, a.copy(), "NaN equals nothing")
