"""GPU: the kernels for narrow towers (csrc/cczero_conv_narrow.h; ccz_conv3x3_cn_f16, ccz_conv3x3_cn_f16_live,
ccz_heads_conv1x1_cn_f16) against the float64 chains of evaluator_f64 -- bit for bit, there is no tolerance in this file.

Operands sit on the main fixed-point grids (activations 2^-5, weights 2^-10, bias 2^-15) under the exactness guard, which
evaluator_f64.conv_exact / gemm_exact assert themselves; with K <= 1152 products the guard is looser than for the 256-wide shapes.
Every (cin, cout) the evaluator uses: 128 -> 128 and 64 -> 64 (towers, the 64-plane stem of a 64-wide net, the 128-plane stem of a
128-wide one), 64 -> 128 and 128 -> 64 (the other two stems). Every device output -- and the live form's input -- is a slice of an
arena of 0xFF bytes (test_gpu_conv_tile_stream.Arena) that must come back unchanged outside the output."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import evaluator_f64 as E
from test_gpu_conv_tile_stream import Arena, P, f32, h16, host

pytestmark = pytest.mark.gpu

NAMES = ("board", "rank", "file", "channel")
F16 = torch.float16
G = 2.0 ** -(E.EA + E.EB)
SHAPES = [(128, 128), (64, 64), (64, 128), (128, 64)]
COMBOS = ((False, True), (True, True), (False, False), (True, False))       # (residual, ReLU)
BOARDS = 65          # one more than the small form takes
TILE = 256           # pixels per workgroup of k_conv3x3_narrow (kNwBM)


def _dev():
    return torch.device("cuda", 0)


def _L():
    from chinesechesszero_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=_dev())


def ff_fill(shape):
    return np.full(shape, -1, np.int16).view(np.float16)


@functools.lru_cache(maxsize=None)
def case(cin, cout):
    """65 boards: x [65, 10, 9, cin], r [65, 10, 9, cout], w [cout, 3, 3, cin], b [cout] and the exact sums; the first n boards of it
    are the n-board case (a board's sums do not depend on the other boards)."""
    rs = np.random.RandomState(1000 * cin + cout)
    x = E.grid_acts(rs, (BOARDS, 10, 9, cin))
    r = E.grid_acts(rs, (BOARDS, 10, 9, cout), relu=False)
    w = E.grid_weights(rs, (cout, 3, 3, cin))
    b = E.grid_bias(rs, cout)
    E.assert_on_grid(x, E.EA)
    E.assert_on_grid(w, E.EB)
    E.assert_on_grid(r, E.EA)
    s, worst, share = E.conv_exact(x, w, b, G, f"narrow conv {cin} -> {cout}")
    print(f"\nnarrow conv {cin} -> {cout}: guard fill {worst:.4f} of 1, needs rounding {share:.3f}")
    assert worst < 1.0 and share >= 0.5
    return dict(x=x, r=r, w=w, b=b, s=s)


@functools.lru_cache(maxsize=None)
def operands(cin, cout):
    c = case(cin, cout)
    return h16(c["x"]).view(-1, cin), h16(c["r"]).view(-1, cout), h16(c["w"]), f32(c["b"])


@functools.lru_cache(maxsize=None)
def partial_sums(cin, cout, n):
    """the exact sums of a count that is not whole boards: the rows of the last board past n_pixels read as zero (include/cczero.h)"""
    c = case(cin, cout)
    boards = -(-n // 90)
    x = np.array(c["x"][:boards], copy=True).reshape(boards * 90, cin)
    x[n:] = 0
    s, worst, _ = E.conv_exact(x.reshape(boards, 10, 9, cin), c["w"], c["b"], G, f"narrow conv {cin} -> {cout}, {n} pixels")
    assert worst < 1.0
    return s.reshape(boards * 90, cout)[:n]


def run(cin, cout, n, flags, res, what, sums=None):
    """one call on n pixels with every activation tensor in an arena; returns the output rows [n, cout] (host)"""
    L = _L()
    x, r, w, b = operands(cin, cout)
    a = Arena({"b": b, "r": r[:n], "y": ((n, cout), F16), "x": x[:n]}, outputs=("y",), last="x")
    L.check(L.lib().ccz_conv3x3_cn_f16(_stream(), P(a["x"]), P(w), P(a["b"]), P(a["r"]) if res else None, P(a["y"]), n, flags, cin, cout))
    a.assert_untouched(what)
    return host(a["y"])


def want_rows(cin, cout, n, res, relu):
    c = case(cin, cout)
    if n % 90 == 0:
        s = c["s"][:n // 90].reshape(n, cout)
    else:
        s = partial_sums(cin, cout, n)
    r = c["r"].reshape(-1, cout)[:n] if res else None
    return E.conv_chain(s, r, relu)


@pytest.mark.parametrize("boards", [1, 3])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_small_form(cin, cout, boards):
    """up to 64 boards the dispatch takes k_conv3x3_small<RES, CIN, COUT>: 90 and 270 pixels (two and five 64-pixel blocks, the last
    one partial), every combination of residual and ReLU, with and without the force bit"""
    L = _L()
    n = boards * 90
    for force in (0, L.CONV_FORCE_SMALL):
        for res, relu in COMBOS:
            what = f"small {cin} -> {cout}, {boards} boards, force {force} res {res} relu {relu}"
            got = run(cin, cout, n, int(relu) | force, res, what)
            E.assert_same(got.reshape(boards, 10, 9, cout), want_rows(cin, cout, n, res, relu).reshape(boards, 10, 9, cout), what, NAMES)


@pytest.mark.parametrize("n", [90, TILE - 1, TILE + 1, 200, BOARDS * 90])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_tile_form(cin, cout, n):
    """k_conv3x3_narrow, forced: one board (a third of a tile), one pixel fewer and one more than a whole tile, a count that is no
    multiple of 16 pixels, and 65 boards (22 tiles + 218 pixels; tile edges fall inside boards), also in descending tile order"""
    L = _L()
    for res, relu in COMBOS:
        for desc in (0, L.CONV_DESCENDING):
            what = f"tile {cin} -> {cout}, {n} pixels, res {res} relu {relu} descending {desc}"
            got = run(cin, cout, n, int(relu) | L.CONV_FORCE_TILE | desc, res, what)
            E.assert_same(got, want_rows(cin, cout, n, res, relu), what, ("pixel", "channel"))


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_small_and_tile_forms_agree(cin, cout):
    L = _L()
    for res, relu in COMBOS:
        a = run(cin, cout, 270, int(relu) | L.CONV_FORCE_SMALL, res, "small")
        b = run(cin, cout, 270, int(relu) | L.CONV_FORCE_TILE, res, "tile")
        E.assert_same_bits(a, b, f"{cin} -> {cout} res {res} relu {relu}: small against tile on 3 boards", ("pixel", "channel"))


def test_output_over_the_residual():
    """y = r: the tower's second convolution of a block writes over its residual input, both forms"""
    L = _L()
    for cin, cout in ((128, 128), (64, 64)):
        x, r, w, b = operands(cin, cout)
        for n, force in ((270, L.CONV_FORCE_SMALL), (270, L.CONV_FORCE_TILE), (BOARDS * 90, 0)):
            a = Arena({"y": r[:n].clone(), "x": x[:n]}, outputs=("y",))
            L.check(L.lib().ccz_conv3x3_cn_f16(_stream(), P(a["x"]), P(w), P(b), P(a["y"]), P(a["y"]), n, 1 | force, cin, cout))
            a.assert_untouched("over the residual")
            E.assert_same(host(a["y"]), want_rows(cin, cout, n, True, True), f"{cin} -> {cout}, {n} pixels force {force}, over the residual", ("pixel", "channel"))


# ------------------------------------------------------------------ the live form
CAP = 24     # boards of the batch: one part holds all 24, three parts 8 each (2.8 tiles)


@pytest.mark.parametrize("n_parts", [1, 3])
@pytest.mark.parametrize("live", [0, 1, CAP - 1, CAP])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_live_form(cin, cout, live, n_parts):
    """ccz_conv3x3_cn_f16_live: the first `live` boards (a device value) cut into n_parts ranges of ceil(ceil(L / n_parts) / 8) * 8 boards,
    every part launched with the capacity InferenceNet.tower_schedule gives it; the live rows are the float64 chain, every byte past
    them keeps its fill, the input arena is untouched"""
    L = _L()
    c = case(cin, cout)
    x, r, w, b = operands(cin, cout)
    cap = E.planned_cap(CAP, n_parts)
    ranges = E.live_ranges(live, n_parts, cap // 90)
    assert sum(n for _, n in ranges) == live
    for res, relu in COMBOS:
        what = f"live {cin} -> {cout}, {live} of {CAP} boards in {n_parts}, res {res} relu {relu}"
        want = E.conv_live_expected(c["s"][:CAP], c["r"][:CAP] if res else None, relu, ranges, ff_fill((CAP, 10, 9, cout)))
        a = Arena({"n": i32(live), "r": r[:CAP * 90], "y": ((CAP * 90, cout), F16), "x": x[:CAP * 90]}, outputs=("y",), last="x")
        for part in range(n_parts):
            L.check(L.lib().ccz_conv3x3_cn_f16_live(_stream(), P(a["x"]), P(w), P(b), P(a["r"]) if res else None, P(a["y"]), cap,
                                                    int(relu) | (2 if part & 1 else 0), cin, cout, P(a["n"]), part, n_parts))
        a.assert_untouched(what)
        got = host(a["y"]).reshape(CAP, 10, 9, cout)
        E.assert_same(got[:live], want[:live], what, NAMES)
        E.assert_same_bits(got, want, what + " (rows past the live boards keep their fill)", NAMES)


# ------------------------------------------------------------------ the head convolutions
@pytest.mark.parametrize("c_in", [64, 128])
def test_head_convolutions(c_in):
    """ccz_heads_conv1x1_cn_f16: rn16(relu(bias + S_C)) as [board][pos][17] and [board][pos][7] from board-major rows of 64 / 128
    channels, with a live count below the batch and without one; pad columns and boards past the count keep the arena's bytes"""
    L = _L()
    B = 7
    rs = np.random.RandomState(60 + c_in)
    x = E.grid_acts(rs, (B, 90, c_in), std=1.0)
    w32 = np.zeros((32, c_in))
    w32[:24] = E.grid_normal(rs, (24, c_in), 0.08, E.EB, 128)
    b32 = np.zeros(32)
    b32[:24] = E.grid_bias(rs, 24)
    s, worst, share = E.gemm_exact(x.reshape(-1, c_in), w32[:24], b32[:24], G, f"narrow heads {c_in}")
    print(f"\nnarrow heads {c_in}: guard fill {worst:.4f} of 1, needs rounding {share:.3f}")
    assert worst < 1.0 and share >= 0.5
    s = s.reshape(B, 90, 24)
    wp_, wv_ = E.heads_chain(s)
    xd, wd, bd = h16(x), h16(w32), f32(b32)
    for live in (5, None, 1):
        n = B if live is None else live
        what = f"narrow heads {c_in}, live {live} of {B}"
        a = Arena({"x": xd, "pol": ((B, 1536), F16), "val": ((B, 640), F16), "n": i32(n)}, outputs=("pol", "val"))
        L.check(L.lib().ccz_heads_conv1x1_cn_f16(_stream(), P(a["x"]), P(wd), P(bd), P(a["pol"]), P(a["val"]), B, c_in, None if live is None else P(a["n"])))
        a.assert_untouched(what)
        pol, val = host(a["pol"]), host(a["val"])
        E.assert_same(pol[:n, :1530].reshape(n, 90, 17), wp_[:n], what + " policy", ("board", "pos", "channel"))
        E.assert_same(val[:n, :630].reshape(n, 90, 7), wv_[:n], what + " value", ("board", "pos", "channel"))
        assert np.all(pol.view(np.int16)[:n, 1530:] == -1) and np.all(val.view(np.int16)[:n, 630:] == -1), what + ": pad columns written"
        assert np.all(pol.view(np.int16)[n:] == -1) and np.all(val.view(np.int16)[n:] == -1), what + ": boards past the live count written"


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    """an unsupported (cin, cout), a null live count, part >= n_parts, misaligned pointers: an error with a text, and the output keeps its bytes"""
    L = _L()
    lib = L.lib()
    x, r, w, b = operands(128, 128)
    a = Arena({"y": ((270, 128), F16), "pol": ((3, 1536), F16), "val": ((3, 640), F16)}, outputs=())
    n = i32(3)
    s = _stream()

    def refused(rc, what):
        assert rc != 0, what + ": accepted"
        assert lib.ccz_last_error(), what + ": no error text"
        a.assert_untouched(what)

    refused(lib.ccz_conv3x3_cn_f16(s, P(x), P(w), P(b), None, P(a["y"]), 270, 1, 256, 128), "(256, 128)")
    refused(lib.ccz_conv3x3_cn_f16(s, P(x), P(w), P(b), None, P(a["y"]), 270, 1, 64, 32), "(64, 32)")
    refused(lib.ccz_conv3x3_cn_f16_live(s, P(x), P(w), P(b), None, P(a["y"]), 720, 1, 128, 128, None, 0, 1), "null live count")
    refused(lib.ccz_conv3x3_cn_f16_live(s, P(x), P(w), P(b), None, P(a["y"]), 720, 1, 128, 128, P(n), 1, 1), "part >= n_parts")
    refused(lib.ccz_conv3x3_cn_f16_live(s, P(x), P(w), P(b), None, P(a["y"]), 720, 1, 128, 128, P(n), 3, 3), "part >= n_parts (3)")
    refused(lib.ccz_conv3x3_cn_f16(s, C.c_void_p(x.data_ptr() + 2), P(w), P(b), None, P(a["y"]), 90, 1, 128, 128), "misaligned x")
    refused(lib.ccz_conv3x3_cn_f16(s, P(x), P(w), P(b), None, P(a["y"]), 270, 1 | L.CONV_G16, 128, 128), "group-of-16 flag")
    refused(lib.ccz_heads_conv1x1_cn_f16(s, P(x), P(w), P(b), P(a["pol"]), P(a["val"]), 3, 256, None), "heads at 256")
    refused(lib.ccz_heads_conv1x1_cn_f16(s, P(x), P(w), P(b), P(a["pol"]), P(a["val"]), 3, 32, None), "heads at 32")
    assert L.ABI_VERSION == 9 and lib.ccz_abi_version() == 9
