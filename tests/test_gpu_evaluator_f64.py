"""GPU: every evaluator kernel form against the float64 references of tests/evaluator_f64.py, bit for bit.

The operands sit on fixed-point grids (activations 2^-5, weights 2^-10, bias 2^-15 unless a test says otherwise) and pass the
exactness guard |bias| + sum|a||w| < 2^24 g, so the fp32 accumulator of ANY summation order holds the exact sum and the expected
fp16 output is unique (tests/test_cpu_evaluator_f64.py proves that on the CPU). Every comparison below is equality on values;
the value output's tanh uses the nearest-candidate check of evaluator_f64.value_mismatches. There is no tolerance in this file.

Every test asserts its guard and its "needs rounding" share on the float64 reference BEFORE it reads device output, and prints
both once. A failure names the first failing element, both values and the number of differing elements."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import evaluator_f64 as E

pytestmark = pytest.mark.gpu

G = 2.0 ** -(E.EA + E.EB)
NAMES = ("board", "rank", "file", "channel")


# ------------------------------------------------------------------ plumbing
def _dev():
    return torch.device("cuda", 0)


def _lib():
    from chinesechesszero_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def h16(a):
    """float64 grid values -> fp16 on the device (exact: the builders assert that every operand is an fp16 number)"""
    return torch.from_numpy(np.ascontiguousarray(E.rn16(a))).to(_dev())


def f32(a):
    a = np.ascontiguousarray(np.asarray(a, np.float64))
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)            # the bias is a float32 number
    return torch.from_numpy(a.astype(np.float32)).to(_dev())


def host(t):
    return t.cpu().numpy()


def report(what, worst, share, least=0.5):
    print(f"\n{what}: guard fill {worst:.4f} of 1, needs rounding {share:.3f}")
    assert worst < 1.0 and share >= least, (what, worst, share)


def conv(x, w, b, res, y, n_pixels, flags):
    L = _lib()
    L.check(L.lib().ccz_conv3x3_c256_f16(_stream(), P(x), P(w), P(b), P(res), P(y), n_pixels, flags))
    return y


def dev_grid(gen, shape, std, e, clip, relu):
    """grid operands made on the device (the big batches): round(N(0, std^2) 2^e) clipped, / 2^e, as fp16 -- every step exact"""
    v = torch.randn(shape, generator=gen, device=_dev()) * std
    if relu:
        v = torch.relu(v)
    return (torch.clamp(torch.round(v * 2.0 ** e), -clip, clip) / 2.0 ** e).half()


# ------------------------------------------------------------------ convolution operands + reference
@functools.lru_cache(maxsize=3)
def conv_case(boards, seed=0, sx=0, sw=0, relu_res=False):
    """x, r [B, 10, 9, 256], w [256, 3, 3, 256], b [256] in float64 and s = the exact sums. sx / sw: activations / weights
    scaled by 2^-sx / 2^-sw (the subnormal cases): the grids and the guard scale with them."""
    rs = np.random.RandomState(7919 * seed + boards)
    ea, eb = E.EA + sx, E.EB + sw
    x = E.grid_acts(rs, (boards, 10, 9, 256)) * 2.0 ** -sx
    r = E.grid_acts(rs, (boards, 10, 9, 256), relu=relu_res) * 2.0 ** -(sx + sw)
    w = E.grid_weights(rs, (256, 3, 3, 256)) * 2.0 ** -sw
    b = E.grid_bias(rs, 256) * 2.0 ** -(sx + sw)
    E.assert_on_grid(x, ea)
    E.assert_on_grid(w, eb)
    E.assert_on_grid(r, ea + sw)
    s, worst, share = E.conv_exact(x, w, b, 2.0 ** -(ea + eb), f"conv {boards}")
    return dict(x=x, r=r, w=w, b=b, s=s, worst=worst, share=share, B=boards)


COMBOS = ((False, True), (True, True), (False, False), (True, False))       # (residual, ReLU)


def _want(c, res, relu):
    return E.conv_chain(c["s"], c["r"] if res else None, relu)


# ------------------------------------------------------------------ convolution, board-major rows
@pytest.mark.parametrize("boards", [1, 2, 3, 17, 64, 65, 257])
def test_convolution_board_major_rows(boards):
    """ccz_conv3x3_c256_f16 on rows board * 90 + pos: the kernel the batch size selects (k_conv3x3_small up to 64 boards, the
    256-pixel tile kernel above), CONV_FORCE_SMALL and CONV_FORCE_TILE; residual x ReLU in all four combinations; the output
    written over the residual; descending tile order. 256 pixels per tile, 90 per board: tile edges fall inside boards and the
    last tile is partial for every size here."""
    L = _lib()
    c = conv_case(boards)
    report(f"conv board-major {boards}", c["worst"], c["share"])
    x, r, w, b = h16(c["x"]).view(-1, 256), h16(c["r"]).view(-1, 256), h16(c["w"]), f32(c["b"])
    n = boards * 90
    for force in (0, L.CONV_FORCE_SMALL, L.CONV_FORCE_TILE):
        for res, relu in COMBOS:
            y = conv(x, w, b, r if res else None, torch.full_like(x, float("nan")), n, int(relu) | force)
            E.assert_same(host(y).reshape(boards, 10, 9, 256), _want(c, res, relu), f"boards {boards} force {force} res {res} relu {relu}", NAMES)
        y = r.clone()
        conv(x, w, b, y, y, n, 1 | force)
        E.assert_same(host(y).reshape(boards, 10, 9, 256), _want(c, True, True), f"boards {boards} force {force} over the residual", NAMES)
    for flags in (1 | 2 | L.CONV_FORCE_TILE, 1 | 2, 2 | L.CONV_FORCE_TILE):
        y = conv(x, w, b, r, torch.full_like(x, float("nan")), n, flags)
        E.assert_same(host(y).reshape(boards, 10, 9, 256), _want(c, True, bool(flags & 1)), f"boards {boards} descending, flags {flags}", NAMES)


# ------------------------------------------------------------------ convolution, group-of-16 rows
def _g16_forms():
    L = _lib()
    return (("one launch of five tiles", L.CONV_G16), ("middle + edge-pair launches", L.CONV_G16 | L.CONV_G16_EDGE_TILES),
            ("middle + edge-pair tiles in one launch", L.CONV_G16 | L.CONV_G16_EDGE_TILES | L.CONV_G16_ONE_LAUNCH))


def _g16_operands(c):
    B = c["B"]
    xg = h16(np.ascontiguousarray(E.rows_to_g16(c["x"])))
    rg = h16(np.ascontiguousarray(E.rows_to_g16(c["r"])))
    wp = E._pack_w(h16(c["w"]), 256)
    return xg.view(B * 90, 256), rg.view(B * 90, 256), wp, f32(c["b"])


def _g16_host(y, B):
    return E.rows_from_g16(host(y), B)


@pytest.mark.parametrize("boards", [16, 80, 96, 272])
def test_convolution_group_of_16_rows(boards):
    """k_conv3x3_g16 alone, the middle launch + k_conv3x3_g16_edge, and k_conv3x3_g16_one: one group, odd group counts (5, 17: the
    edge kernel pairs the last group with itself) and an even one; residual x ReLU; descending order; output over the residual."""
    c = conv_case(boards)
    report(f"conv group-of-16 {boards}", c["worst"], c["share"])
    xg, rg, wp, b = _g16_operands(c)
    n = boards * 90
    for name, form in _g16_forms():
        for res, relu in COMBOS:
            y = conv(xg, wp, b, rg if res else None, torch.full_like(xg, float("nan")), n, int(relu) | form)
            E.assert_same(_g16_host(y, boards), _want(c, res, relu), f"boards {boards}, {name}, res {res} relu {relu}", NAMES)
        y = conv(xg, wp, b, rg, torch.full_like(xg, float("nan")), n, 3 | form)
        E.assert_same(_g16_host(y, boards), _want(c, True, True), f"boards {boards}, {name}, descending", NAMES)
        y = rg.clone()
        conv(xg, wp, b, y, y, n, 1 | form)
        E.assert_same(_g16_host(y, boards), _want(c, True, True), f"boards {boards}, {name}, over the residual", NAMES)


@pytest.mark.parametrize("live,n_parts", [(1, 1), (16, 2), (17, 1), (100, 3), (160, 4), (100, 6), (160, 6)])
def test_convolution_group_of_16_live_rows(live, n_parts):
    """ccz_conv3x3_c256_f16_live: the first `live` boards (a device value) cut into n_parts ranges of whole groups; together the
    parts compute exactly the groups that hold live boards -- against float64 -- and the rows beyond them stay NaN."""
    L = _lib()
    boards = 160
    c = conv_case(boards)
    report(f"conv group-of-16 live {live} in {n_parts}", c["worst"], c["share"])
    xg, rg, wp, b = _g16_operands(c)
    n_live = torch.tensor([live], dtype=torch.int32, device=_dev())
    cap = -(-(boards // 16) // n_parts) * 1440
    want = _want(c, True, True)
    groups = -(-live // 16)
    for name, form in _g16_forms():
        y = torch.full_like(xg, float("nan"))
        for part in range(n_parts):
            L.check(L.lib().ccz_conv3x3_c256_f16_live(_stream(), P(xg), P(wp), P(b), P(rg), P(y), cap, 1 | form | (2 if part & 1 else 0),
                                                      P(n_live), part, n_parts))
        got = _g16_host(y, boards)
        E.assert_same(got[:groups * 16], want[:groups * 16], f"live {live} in {n_parts} parts, {name}", NAMES)
        assert np.isnan(got[groups * 16:].astype(np.float32)).all(), (live, n_parts, name)


# ------------------------------------------------------------------ stem
def _stem_case(boards, seed, sw=0):
    rs = np.random.RandomState(31 * seed + boards)
    leaf = (rs.random_sample((boards, 119, 10, 9)) > 0.8).astype(np.float64)   # a 0/1 tensor is on every grid
    leaf[:, :7] = 1                                                            # planes outside the live set must not leak in
    x21 = np.concatenate([leaf[:, 49:56], leaf[:, 105:119]], axis=1).transpose(0, 2, 3, 1)   # [B, 10, 9, 21]
    w = np.zeros((256, 3, 3, 64))
    w[..., :21] = E.grid_weights(rs, (256, 3, 3, 21), std=0.05) * 2.0 ** -sw
    b = E.grid_bias(rs, 256) * 2.0 ** -sw
    E.assert_on_grid(w, E.EB + sw)
    s, worst, share = E.conv_exact(x21, w[..., :21], b, 2.0 ** -(E.EA + E.EB + sw), f"stem {boards}")
    return leaf, w, b, s, worst, share


@pytest.mark.parametrize("boards", [1, 65, 304])
def test_stem_through_the_plane_pack(boards):
    """ccz_pack_live_planes_f16 / _g16_f16 from a 0/1 leaf tensor, then ccz_conv3x3_stem_f16 (64 input channels, 21 live, no
    residual): board-major rows on the selected / small / tile kernel, and (whole groups of 16) k_conv3x3_g16_stem."""
    L = _lib()
    leaf, w, b, s, worst, share = _stem_case(boards, 1)
    report(f"stem {boards}", worst, share)
    leaf_d, w64, bd = h16(leaf), h16(w), f32(b)
    n = boards * 90
    x64 = torch.full((n, 64), float("nan"), device=_dev(), dtype=torch.float16)
    L.check(L.lib().ccz_pack_live_planes_f16(_stream(), P(leaf_d), P(x64), boards))
    for force in (0, L.CONV_FORCE_SMALL, L.CONV_FORCE_TILE):
        for relu in (1, 0):
            y = torch.full((n, 256), float("nan"), device=_dev(), dtype=torch.float16)
            L.check(L.lib().ccz_conv3x3_stem_f16(_stream(), P(x64), P(w64), P(bd), P(y), n, relu | force))
            E.assert_same(host(y).reshape(boards, 10, 9, 256), E.conv_chain(s, None, bool(relu)), f"stem {boards} force {force} relu {relu}", NAMES)
    if boards % 16 == 0:
        x64g = torch.full((n, 64), float("nan"), device=_dev(), dtype=torch.float16)
        L.check(L.lib().ccz_pack_live_planes_g16_f16(_stream(), P(leaf_d), P(x64g), boards, None, None))
        wp = E._pack_w(w64, 64)
        for _, form in _g16_forms():
            for relu in (1, 0):
                y = torch.full((n, 256), float("nan"), device=_dev(), dtype=torch.float16)
                L.check(L.lib().ccz_conv3x3_stem_f16(_stream(), P(x64g), P(wp), P(bd), P(y), n, relu | form))
                E.assert_same(_g16_host(y, boards), E.conv_chain(s, None, bool(relu)), f"stem g16 {boards} form {form} relu {relu}", NAMES)


# ------------------------------------------------------------------ full size
SAMPLE_4096 = [0, 1, 7, 8, 15, 16, 17, 31, 1000, 1023, 1024, 1025, 2032, 2040, 2047, 2048, 2049, 2063, 3000, 3071, 3072, 4080, 4094, 4095]


def test_convolution_full_size_group_of_16_on_a_board_sample():
    """4096 boards (256 groups), one layer on the device in each group-of-16 form; the float64 reference on 24 boards at the
    edges: first and last board of a group, groups 0, 1, 127, 128, 255, either side of the 1024- and 2048-board cuts, the last board."""
    B = 4096
    gen = torch.Generator(device=_dev()).manual_seed(11)
    x = dev_grid(gen, (B, 10, 9, 256), 0.7, E.EA, 127, True)
    r = dev_grid(gen, (B, 10, 9, 256), 0.7, E.EA, 127, False)
    rs = np.random.RandomState(11)
    w, b = E.grid_weights(rs, (256, 3, 3, 256)), E.grid_bias(rs, 256)
    idx = torch.tensor(SAMPLE_4096, device=_dev())
    xs, rsm = host(x[idx]).astype(np.float64), host(r[idx]).astype(np.float64)
    E.assert_on_grid(xs, E.EA)
    E.assert_on_grid(rsm, E.EA)
    s, worst, share = E.conv_exact(xs, w, b, G, "conv 4096 sample")
    report("conv 4096, 24 sampled boards", worst, share)
    want = E.conv_chain(s, rsm, True)
    xg, rg = E.rows_to_g16(x).contiguous().view(-1, 256), E.rows_to_g16(r).contiguous().view(-1, 256)
    del x, r
    wp, bd = E._pack_w(h16(w), 256), f32(b)
    for name, form in _g16_forms():
        y = conv(xg, wp, bd, rg, torch.full_like(xg, float("nan")), B * 90, 1 | form)
        got = host(E.rows_from_g16(y, B)[idx])
        E.assert_same(got, want, f"4096 boards, {name} (board = SAMPLE_4096[i])", NAMES)
        assert bool(torch.isfinite(y).all())


# ------------------------------------------------------------------ head convolutions
def _head_weights(rs, e, clip, sw=0):
    w32 = np.zeros((32, 256))
    w32[:24] = E.grid_normal(rs, (24, 256), 0.08, e, clip) * 2.0 ** -sw
    return w32


def _check_heads(pol, val, s24, n, fill, what):
    """pol [B, 1536] / val [B, 640] fp16 device outputs; s24 [n, 90, 24] exact sums of the first n boards"""
    wp_, wv_ = E.heads_chain(s24)
    pol, val = host(pol), host(val)
    E.assert_same(pol[:n, :1530].reshape(n, 90, 17), wp_, what + " policy", ("board", "pos", "channel"))
    E.assert_same(val[:n, :630].reshape(n, 90, 7), wv_, what + " value", ("board", "pos", "channel"))
    assert np.all(pol[:n, 1530:] == fill) and np.all(val[:n, 630:] == fill), what + ": pad columns written"
    assert np.all(pol[n:] == fill) and np.all(val[n:] == fill), what + ": boards past the live count written"


@pytest.mark.parametrize("B,g16", [(1, False), (7, False), (200, False), (80, True), (1296, True)])
def test_head_convolutions_on_their_own(B, g16):
    """ccz_heads_conv1x1_f16: rn16(relu(bias + S_256)) written as [board][pos][17] and [board][pos][7], either row layout, odd group
    counts (5, 81), with and without a live count; pad columns and boards past the count keep what they held. ReLU zeroes about
    half of the sums and a zero needs no rounding, so the asserted share of outputs that need one is 0.25 (of the sums: 0.5)."""
    L = _lib()
    rs = np.random.RandomState(40 + B)
    x = E.grid_acts(rs, (B, 90, 256), std=1.0)
    w32, b32 = _head_weights(rs, 9, 128), np.zeros(32)
    b32[:24] = E.grid_bias(rs, 24, e=14)
    g = 2.0 ** -14
    s, worst, share = E.gemm_exact(x.reshape(-1, 256), w32[:24], b32[:24], g, f"heads {B}")
    report(f"heads {B} (sums)", worst, share)
    assert E.needs_rounding(np.maximum(s, 0)) >= 0.25
    s = s.reshape(B, 90, 24)
    xr = np.ascontiguousarray(x.reshape(B // 16, 16, 90, 256).transpose(0, 2, 1, 3)) if g16 else x
    xd, wd, bd = h16(xr), h16(w32), f32(b32)
    for live in (None, max(1, B // 2), B):
        n = B if live is None else live
        pol = torch.full((B, 1536), 3.0, dtype=torch.float16, device=_dev())
        val = torch.full((B, 640), 3.0, dtype=torch.float16, device=_dev())
        nl = None if live is None else torch.tensor([live], dtype=torch.int32, device=_dev())
        L.check(L.lib().ccz_heads_conv1x1_f16(_stream(), P(xd), P(wd), P(bd), P(pol), P(val), B, L.CONV_G16 if g16 else 0, P(nl)))
        _check_heads(pol, val, s[:n], n, 3.0, f"heads B {B} g16 {g16} live {live}")


SAMPLE_1296 = [0, 1, 15, 16, 31, 640, 655, 656, 1263, 1264, 1279, 1280, 1281, 1288, 1294, 1295]


def _last_layer_reference(xs, rs_, w, b, w32, b32, g1, g2, what):
    """the composed reference on the boards given: y = relu(rn16(rn16(S) + r)) in fp16, then the head sums on y"""
    s, worst, share = E.conv_exact(xs, w, b, g1, what)
    y = E.conv_chain(s, rs_, True).astype(np.float64)
    n = y.shape[0]
    s2, worst2, share2 = E.gemm_exact(y.reshape(-1, 256), w32[:24], b32[:24], g2, what + " heads")
    return s2.reshape(n, 90, 24), (worst, share), (worst2, share2), y


@pytest.mark.parametrize("boards,live,n_parts", [(80, None, 1), (1296, None, 1), (160, 100, 3), (160, 17, 1)])
def test_heads_in_the_last_layers_epilogue(boards, live, n_parts):
    """ccz_conv3x3_c256_heads_f16 against the composed reference: the layer's fp16 output y (never stored) is a multiple of 2^-15,
    so the head weights sit on the grid 2^-4 and the head bias on 2^-19: the second guard is on g = 2^-19. Whole batch with odd
    group counts (5; 81 on a board sample), a live count cut into parts; with and without edge-pair tiles."""
    L = _lib()
    rs = np.random.RandomState(500 + boards + (live or 0))
    w, b = E.grid_weights(rs, (256, 3, 3, 256)), E.grid_bias(rs, 256)
    w32, b32 = _head_weights(rs, 4, 4), np.zeros(32)
    b32[:24] = E.grid_bias(rs, 24, e=19)
    if boards > 300:
        gen = torch.Generator(device=_dev()).manual_seed(boards)
        x = dev_grid(gen, (boards, 10, 9, 256), 0.7, E.EA, 127, True)
        r = dev_grid(gen, (boards, 10, 9, 256), 0.7, E.EA, 127, True)
        sample = SAMPLE_1296
        idx = torch.tensor(sample, device=_dev())
        xs, rsm = host(x[idx]).astype(np.float64), host(r[idx]).astype(np.float64)
        xg, rg = E.rows_to_g16(x).contiguous().view(-1, 256), E.rows_to_g16(r).contiguous().view(-1, 256)
    else:
        xs, rsm = E.grid_acts(rs, (boards, 10, 9, 256)), E.grid_acts(rs, (boards, 10, 9, 256))
        sample = list(range(boards if live is None else live))
        xg = h16(np.ascontiguousarray(E.rows_to_g16(xs))).view(-1, 256)
        rg = h16(np.ascontiguousarray(E.rows_to_g16(rsm))).view(-1, 256)
        xs, rsm = xs[sample], rsm[sample]
    E.assert_on_grid(xs, E.EA)
    E.assert_on_grid(rsm, E.EA)
    s2, (w1, sh1), (w2, sh2), y = _last_layer_reference(xs, rsm, w, b, w32, b32, G, 2.0 ** -19, f"last layer {boards}")
    E.assert_on_grid(y, 15)
    report(f"last layer {boards}: the layer", w1, sh1)
    report(f"last layer {boards}: the heads on y (sums)", w2, sh2)
    assert E.needs_rounding(np.maximum(s2, 0)) >= 0.25
    wpol, wval = E.heads_chain(s2)
    wp, bd, w32d, b32d = E._pack_w(h16(w), 256), f32(b), h16(w32), f32(b32)
    nl = None if live is None else torch.tensor([live], dtype=torch.int32, device=_dev())
    n = boards if live is None else live
    for edge in (0, L.CONV_G16_EDGE_TILES):
        fl = 1 | L.CONV_G16 | edge
        pol = torch.full((boards, 1536), 3.0, dtype=torch.float16, device=_dev())
        val = torch.full((boards, 640), 3.0, dtype=torch.float16, device=_dev())
        keep = rg.clone()
        if live is None:
            L.check(L.lib().ccz_conv3x3_c256_heads_f16(_stream(), P(xg), P(wp), P(bd), P(rg), P(w32d), P(b32d), P(pol), P(val), boards * 90, fl, None, 0, 1))
        else:
            cap = -(-(boards // 16) // n_parts) * 1440
            for part in range(n_parts):
                L.check(L.lib().ccz_conv3x3_c256_heads_f16(_stream(), P(xg), P(wp), P(bd), P(rg), P(w32d), P(b32d), P(pol), P(val), cap,
                                                           fl | (2 if part & 1 else 0), P(nl), part, n_parts))
        torch.cuda.synchronize()
        assert torch.equal(rg, keep)
        ph, vh = host(pol), host(val)
        what = f"last layer {boards} live {live} edge {edge}"
        E.assert_same(ph[sample, :1530].reshape(len(sample), 90, 17), wpol, what + " policy (board = sample[i])", ("board", "pos", "channel"))
        E.assert_same(vh[sample, :630].reshape(len(sample), 90, 7), wval, what + " value (board = sample[i])", ("board", "pos", "channel"))
        assert np.all(ph[:, 1530:] == 3.0) and np.all(vh[:, 630:] == 3.0) and np.all(ph[n:] == 3.0) and np.all(vh[n:] == 3.0), what
        assert np.all(np.isfinite(ph.astype(np.float32)))


# ------------------------------------------------------------------ FC
FC_FORMS = (("128 x 128 tiles", 2), ("256 x 144 tiles", 4), ("selected", 0))      # ccz_fc_f16's relu bits 1 / 2; M <= 16 selects k_fc_skinny_f16
FC_MS = [1, 5, 11, 16, 17, 128, 129, 300, 2048, 4096, 4097]
#           K     N    relu lda   ldc
FC_SHAPES = {
    "policy": (1536, 2086, 0, 1536, 2096),      # N = 2 (mod 4): the last dword of a row of the skinny kernel is half a store
    "value": (640, 256, 1, 640, 256),           # N = 0 (mod 4)
    "k64": (64, 130, 1, 72, 140),               # two k-steps: shorter than every pipeline
    "k512": (512, 258, 0, 520, 258),            # exactly one load batch of the skinny kernel
    "k1024": (1024, 132, 1, 1024, 134),         # exactly two
    "k1088": (1088, 2086, 0, 1096, 2086),       # one pair of k-steps past two batches
}


def _fc_rows(M):
    if M <= 300:
        return np.arange(M)
    rows = [0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 511, 512, 1023, 1024, 1025, 2047, M // 2 + 1, M - 257, M - 256, M - 129, M - 128, M - 2, M - 1]
    return np.unique(np.array([r for r in rows if 0 <= r < M]))


def _fc_operands(shape, M, sw=0, sx=0):
    """float64 operands of one FC case on the grids, the weight matrix and the bias padded to whole 128-row tiles (as net.py pads
    them: the kernels' contract), the activations in a [M, lda] buffer with NaN between K and lda; the exact sums on `rows`
    (_fc_rows) and the expected fp16 output there."""
    K, N, relu, lda, ldc = FC_SHAPES[shape]
    rs = np.random.RandomState(K + N + M)
    Np = -(-N // 128) * 128
    a = E.grid_acts(rs, (M, K), std=1.0) * 2.0 ** -sx                           # non-zero up to the last column: a real K tail
    w = np.zeros((Np, K))
    w[:N] = E.grid_weights(rs, (N, K)) * 2.0 ** -sw
    b = np.zeros(Np)
    b[:N] = E.grid_bias(rs, N, std=0.3) * 2.0 ** -(sw + sx)
    E.assert_on_grid(w, E.EB + sw)
    E.assert_on_grid(a, E.EA + sx)
    rows = _fc_rows(M)
    s, worst, share = E.gemm_exact(a[rows], w[:N], b[:N], G * 2.0 ** -(sw + sx), f"fc {shape} M {M}")
    buf = np.full((M, lda), np.nan)                                              # poison between K and lda: never read
    buf[:, :K] = a
    return dict(K=K, N=N, relu=relu, lda=lda, ldc=ldc, buf=buf, w=w, b=b, rows=rows, worst=worst, share=share, want=E.fc_chain(s, relu))


def _fc_check(shape, M, sw=0, sx=0, forms=FC_FORMS):
    L = _lib()
    o = _fc_operands(shape, M, sw, sx)
    K, N, relu, lda, ldc, rows, want = o["K"], o["N"], o["relu"], o["lda"], o["ldc"], o["rows"], o["want"]
    report(f"fc {shape} M {M}{' (subnormal weights)' if sw else ''}", o["worst"], o["share"])
    ad, wd, bd = h16(o["buf"]), h16(o["w"]), f32(o["b"])
    for live in (None, M // 2 + 1) if M > 1 else (None,):
        n = M if live is None else live
        nl = None if live is None else torch.tensor([live], dtype=torch.int32, device=_dev())
        for name, force in forms:
            c = torch.full((M, ldc), 9.0, dtype=torch.float16, device=_dev())
            L.check(L.lib().ccz_fc_f16(_stream(), P(ad), lda, P(wd), P(bd), P(c), ldc, M, N, K, relu | force, P(nl)))
            got = host(c)
            sel = rows < n
            E.assert_same(got[rows[sel], :N], want[sel], f"fc {shape} M {M} live {live}, {name} (row = rows[i])", ("row", "column"))
            assert np.all(got[:, N:] == 9.0) and np.all(got[n:] == 9.0), (shape, M, live, name)
    return want


@pytest.mark.parametrize("M", FC_MS)
@pytest.mark.parametrize("shape", ["policy", "value"])
def test_fc_policy_and_value_shapes(shape, M):
    """ccz_fc_f16 = rn16(relu?(bias + S_K)): k_fc_f16, k_fc_wide_f16 and the selected kernel (k_fc_skinny_f16 up to 16 rows); ldc > N
    and N = 2 (mod 4) for the policy shape, N = 0 (mod 4) for the value shape; a live count; columns >= N and rows >= live
    keep what they held. From 2048 rows the reference runs on a row sample (tile edges, the live boundary, the last rows)."""
    _fc_check(shape, M)


@pytest.mark.parametrize("M", [1, 16, 17, 300])
@pytest.mark.parametrize("shape", ["k64", "k512", "k1024", "k1088"])
def test_fc_at_the_k_loop_edges(shape, M):
    """K = 64 (two k-steps), 512 and 1024 (exactly one and two load batches of the skinny kernel), 1088 (one pair past two
    batches); lda > K with NaN between K and lda; ldc > N."""
    _fc_check(shape, M)


# ------------------------------------------------------------------ value output
@pytest.mark.parametrize("M", [1, 3, 4, 5, 4096])
def test_value_output_nearest_candidate(M):
    """ccz_value_out_f32 = tanhf(rn16(b2 + S_256)): s is exact under the guard; v must be strictly closer to tanh64(rn16(s)) than
    to tanh64 of either fp16 neighbour of rn16(s). |s| < 4 by construction (a row's trailing products are dropped once the sum of
    absolute values would pass 3.9). From M = 3 on, rows 0 and 1 sit exactly on fp16 ties (1 + 2^-11 and 1 + 3 * 2^-11: round to even
    goes down for one and up for the other)."""
    L = _lib()
    rs = np.random.RandomState(60 + M)
    h = E.grid_acts(rs, (M, 256), std=1.0)
    w2 = E.grid_weights(rs, 256, std=0.05)
    w2[0], w2[1] = 0.5, 2.0 ** -10
    b2 = 0.125
    h[np.abs(b2) + np.cumsum(np.abs(h) * np.abs(w2)[None, :], axis=1) >= 3.9] = 0
    if M >= 3:
        h[:2] = 0
        h[0, 0], h[0, 1] = 1.75, 0.5
        h[1, 0], h[1, 1] = 1.75, 1.5
    s, worst, share = E.gemm_exact(h, w2[None, :], np.array([b2]), G, f"value {M}")
    s = s[:, 0]
    report(f"value output {M}", worst, share, least=0.5 if M > 5 else 0.0)
    assert np.abs(s).max() < 4
    if M >= 3:
        assert s[0] == 1 + 2.0 ** -11 and s[1] == 1 + 3 * 2.0 ** -11
        assert float(E.rn16(s[0])) == 1.0 and float(E.rn16(s[1])) == 1 + 2.0 ** -9
    hd, wd = h16(h), h16(w2)
    for live in (None, M // 2 + 1) if M > 1 else (None,):
        n = M if live is None else live
        nl = None if live is None else torch.tensor([live], dtype=torch.int32, device=_dev())
        v = torch.full((M,), 5.0, device=_dev())
        L.check(L.lib().ccz_value_out_f32(_stream(), P(hd), P(wd), b2, P(v), M, P(nl)))
        v = host(v)
        bad = E.value_mismatches(v[:n], s[:n])
        if bad.size:
            i = int(bad[0])
            c, lo, hi = E.value_candidates(s[i:i + 1])
            raise AssertionError(f"value M {M} live {live}: row {i}: device {v[i]!r}, s {s[i]!r}, tanh64(rn16(s)) {c[0]!r}, neighbours {lo[0]!r} {hi[0]!r}; {bad.size} rows")
        assert np.all(v[n:] == 5.0)


# ------------------------------------------------------------------ ccz_bias_act_f16
@pytest.mark.parametrize("rows,channels", [(630, 64), (90 * 257, 256), (90 * 400, 256)])
def test_bias_act_bit_for_bit(rows, channels):
    """relu(rn16(rn16(y + b) + r)) on arbitrary finite fp16 operands -- every exponent, subnormals, sums that overflow to inf --
    with and without a residual. Pure fp16 adds: no grid is needed."""
    L = _lib()
    rs = np.random.RandomState(rows)

    def patterns(shape):
        bits = rs.randint(0, 0x7c00, size=shape).astype(np.uint16) | (rs.randint(0, 2, size=shape).astype(np.uint16) << 15)
        v = bits.view(np.float16)
        near = (rs.standard_normal(shape) * 2).astype(np.float16)              # half of the operands at ordinary magnitudes
        return np.where(rs.random_sample(shape) < 0.5, v, near)

    y0, r, b = patterns((rows, channels)), patterns((rows, channels)), patterns(channels)
    b[:4] = np.array([60000, -60000, 2.0 ** -24, 0], np.float16)
    want_plain, want_res = E.bias_act_chain(y0, b), E.bias_act_chain(y0, b, r)
    sub = float((np.abs(want_res.astype(np.float64)) < 2.0 ** -14).mean())
    print(f"\nbias_act {rows} x {channels}: inf {int(np.isinf(want_res.astype(np.float32)).sum())}, results below 2^-14: {sub:.3f}")
    assert np.isinf(want_res.astype(np.float32)).any() and not np.isnan(want_res.astype(np.float32)).any()
    yd, rd, bd = torch.from_numpy(y0).to(_dev()), torch.from_numpy(r).to(_dev()), torch.from_numpy(b).to(_dev())
    for res, want in ((None, want_plain), (rd, want_res)):
        y = yd.clone()
        L.check(L.lib().ccz_bias_act_f16(_stream(), P(y), P(bd), P(res), rows, channels))
        E.assert_same(host(y), want, f"bias_act {rows} x {channels} res {res is not None}", ("row", "channel"))


# ------------------------------------------------------------------ subnormal operands and results, one case per MFMA kernel family
def test_subnormal_convolution_all_kernel_families():
    """Activations x 2^-4, weights x 2^-8 (fp16 SUBNORMAL weights: 0.03 * 2^-8 < 2^-14), bias and residual x 2^-12: everything scales
    together, the guard holds on g = 2^-27, and a large share of the expected outputs are fp16 subnormals. Equality says that the
    f16 MFMA reads subnormal operands as they are and that the fp32 -> fp16 conversion and the fp16 add do not flush."""
    L = _lib()
    boards = 32
    c = conv_case(boards, seed=3, sx=4, sw=8)
    subn = float((np.abs(_want(c, True, False).astype(np.float64)) < 2.0 ** -14).mean())
    wsub = float(((np.abs(c["w"]) < 2.0 ** -14) & (c["w"] != 0)).mean())
    report("subnormal conv", c["worst"], c["share"])
    print(f"subnormal conv: {wsub:.2f} of the weights and {subn:.2f} of the expected outputs are fp16 subnormals")
    assert subn > 0.1 and wsub > 0.3
    x, r, w, b = h16(c["x"]).view(-1, 256), h16(c["r"]).view(-1, 256), h16(c["w"]), f32(c["b"])
    n = boards * 90
    for force in (L.CONV_FORCE_SMALL, L.CONV_FORCE_TILE):
        for res, relu in ((True, False), (False, True)):
            y = conv(x, w, b, r if res else None, torch.full_like(x, float("nan")), n, int(relu) | force)
            E.assert_same(host(y).reshape(boards, 10, 9, 256), _want(c, res, relu), f"subnormal, force {force} res {res}", NAMES)
    xg, rg, wp, bd = _g16_operands(c)
    for name, form in _g16_forms():
        for res, relu in ((True, False), (False, True)):
            y = conv(xg, wp, bd, rg if res else None, torch.full_like(xg, float("nan")), n, int(relu) | form)
            E.assert_same(_g16_host(y, boards), _want(c, res, relu), f"subnormal, {name}, res {res}", NAMES)


def test_subnormal_stem_group_of_16():
    """k_conv3x3_g16_stem (and the board-major kernels on the stem shape) with weights x 2^-8"""
    L = _lib()
    boards = 16
    leaf, w, b, s, worst, share = _stem_case(boards, 2, sw=8)
    report("subnormal stem", worst, share)
    want = E.conv_chain(s, None, False)
    assert float(((want != 0) & (np.abs(want.astype(np.float64)) < 2.0 ** -14)).mean()) > 0.01
    leaf_d, w64, bd = h16(leaf), h16(w), f32(b)
    n = boards * 90
    x64, x64g = (torch.full((n, 64), float("nan"), device=_dev(), dtype=torch.float16) for _ in range(2))
    L.check(L.lib().ccz_pack_live_planes_f16(_stream(), P(leaf_d), P(x64), boards))
    L.check(L.lib().ccz_pack_live_planes_g16_f16(_stream(), P(leaf_d), P(x64g), boards, None, None))
    for xin, wt, flags, back in ((x64, w64, L.CONV_FORCE_TILE, None), (x64, w64, L.CONV_FORCE_SMALL, None), (x64g, E._pack_w(w64, 64), L.CONV_G16, boards)):
        y = torch.full((n, 256), float("nan"), device=_dev(), dtype=torch.float16)
        L.check(L.lib().ccz_conv3x3_stem_f16(_stream(), P(xin), P(wt), P(bd), P(y), n, flags))
        got = _g16_host(y, boards) if back else host(y).reshape(boards, 10, 9, 256)
        E.assert_same(got, want, f"subnormal stem flags {flags}", NAMES)


def test_subnormal_heads():
    """ccz_heads_conv1x1_f16 and the heads in the last layer's epilogue with results below 2^-14"""
    L = _lib()
    rs = np.random.RandomState(77)
    B = 16
    # on their own: activations x 2^-4, head weights (grid 2^-9) x 2^-8
    x = E.grid_acts(rs, (B, 90, 256), std=1.0) * 2.0 ** -4
    w32, b32 = _head_weights(rs, 9, 128, sw=8), np.zeros(32)
    b32[:24] = E.grid_bias(rs, 24, e=14) * 2.0 ** -12
    s, worst, share = E.gemm_exact(x.reshape(-1, 256), w32[:24], b32[:24], 2.0 ** -26, "subnormal heads")
    report("subnormal heads", worst, share)
    pol_w, _ = E.heads_chain(s)
    assert float(((pol_w > 0) & (pol_w.astype(np.float64) < 2.0 ** -14)).mean()) > 0.1
    xd, wd, bd = h16(x), h16(w32), f32(b32)
    for g16 in (False, True):
        xr = h16(np.ascontiguousarray(x.reshape(1, 16, 90, 256).transpose(0, 2, 1, 3))) if g16 else xd
        pol = torch.full((B, 1536), 3.0, dtype=torch.float16, device=_dev())
        val = torch.full((B, 640), 3.0, dtype=torch.float16, device=_dev())
        L.check(L.lib().ccz_heads_conv1x1_f16(_stream(), P(xr), P(wd), P(bd), P(pol), P(val), B, L.CONV_G16 if g16 else 0, None))
        _check_heads(pol, val, s.reshape(B, 90, 24), B, 3.0, f"subnormal heads g16 {g16}")
    # in the last layer: the layer's y is subnormal (a multiple of 2^-24), head weights on 2^-4: g = 2^-28
    boards = 32
    c = conv_case(boards, seed=3, sx=4, sw=8)
    rpos = np.abs(c["r"])
    w32, b32 = _head_weights(rs, 4, 4), np.zeros(32)
    b32[:24] = E.grid_bias(rs, 24, e=19) * 2.0 ** -9
    s2, (w1, sh1), (w2, sh2), y = _last_layer_reference(c["x"], rpos, c["w"], c["b"], w32, b32, 2.0 ** -27, 2.0 ** -28, "subnormal last layer")
    E.assert_on_grid(y, 24)
    report("subnormal last layer: the layer", w1, sh1)
    report("subnormal last layer: the heads on y (sums)", w2, sh2)
    assert float((y < 2.0 ** -14).mean()) > 0.1
    xg = h16(np.ascontiguousarray(E.rows_to_g16(c["x"]))).view(-1, 256)
    rg = h16(np.ascontiguousarray(E.rows_to_g16(rpos))).view(-1, 256)
    wp, bd, w32d, b32d = E._pack_w(h16(c["w"]), 256), f32(c["b"]), h16(w32), f32(b32)
    for edge in (0, L.CONV_G16_EDGE_TILES):
        pol = torch.full((boards, 1536), 3.0, dtype=torch.float16, device=_dev())
        val = torch.full((boards, 640), 3.0, dtype=torch.float16, device=_dev())
        L.check(L.lib().ccz_conv3x3_c256_heads_f16(_stream(), P(xg), P(wp), P(bd), P(rg), P(w32d), P(b32d), P(pol), P(val), boards * 90,
                                                   1 | L.CONV_G16 | edge, None, 0, 1))
        _check_heads(pol, val, s2, boards, 3.0, f"subnormal last layer edge {edge}")


@pytest.mark.parametrize("M", [16, 300])
def test_subnormal_fc(M):
    """the three FC kernels with activations x 2^-4 and weights x 2^-8 (M = 16: the selected kernel is k_fc_skinny_f16)"""
    for shape in ("value", "k1088"):
        want = np.abs(_fc_check(shape, M, sw=8, sx=4).astype(np.float64))
        assert float(((want > 0) & (want < 2.0 ** -14)).mean()) > 0.1, shape
