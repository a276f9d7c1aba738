"""GPU: the board-major evaluator path -- what every batch below 640 boards runs on -- on live rows and in guarded arenas.

(1) ccz_conv3x3_c256_f16_live / ccz_conv3x3_stem_f16_live WITHOUT CONV_G16 always land on k_conv3x3_c256, which cuts the live boards (a
    device value) into n_parts ranges of ceil(ceil(L / n_parts) / 8) * 8 boards, moves X, Y and R to its range, clamps its halo rows
    into the range and leaves when the range is empty. Against the float64 chain on the first `live` boards; every row past them
    keeps its fill, down to the byte. The capacity argument is what InferenceNet.tower_schedule (planned) / _stem_fused pass
    (evaluator_f64.planned_cap), for 37 boards it reaches past the tensor.
(2) The gathering plane pack (ccz_pack_live_planes_rows_f16, ccz_pack_live_planes_g16_f16 with rows) against the NumPy restatement
    evaluator_f64.pack_live_planes_rows: output row i from board rows[i] for i < *n_rows, three 16-byte chunks of 128 bytes.
(3) The board-major family with every tensor of a call carved out of arenas of 0xFF bytes (the helpers of
    test_gpu_conv_tile_stream.py): the output equals the same call on plain tensors and the float64 chain, every byte outside the
    output slices stays what it was. A tensor is placed at the END of its arena only where the kernel's code shows that it reads
    nothing past the rows it uses (each test's docstring names the clamp).
(4) Planned against unplanned rows through InferenceNet on real leaf batches, on ONE object with descending live counts and a second
    batch, so that the persistent buffers hold stale rows past the live count.

Sections 1 and 3: operands on fixed-point grids under the exactness guard; every test asserts and prints guard fill and rounding share
on the float64 reference before device output is read. Sections 2 and 4 compare copies / two runs of the same kernels: bit patterns.
There is no tolerance in this file."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import evaluator_f64 as E
import test_gpu_evaluator_f64 as F64
from test_gpu_conv_tile_stream import Arena, P, f32, h16, host, poison, same_bits, weight_arena

pytestmark = pytest.mark.gpu

NAMES = ("board", "rank", "file", "channel")
F16 = torch.float16


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
    """the host image of a poisoned fp16 buffer: every element 0xFFFF"""
    return np.full(shape, -1, np.int16).view(np.float16)


# ================================================================== 1. live ranges of the board-major convolution
@functools.lru_cache(maxsize=None)
def live_case(boards):
    return F64.conv_case(boards)


@functools.lru_cache(maxsize=None)
def live_operands(boards):
    c = live_case(boards)
    return h16(c["x"]).view(-1, 256), h16(c["r"]).view(-1, 256), h16(c["w"]), f32(c["b"])


def launch_live(x, w, b, r, y, boards, live_dev, n_parts, relu):
    """as the planned tower_schedule: the same capacity for every part, odd parts in descending tile order (as launch_layer of the tile-stream file)"""
    L = _L()
    cap = E.planned_cap(boards, n_parts)
    for part in range(n_parts):
        L.check(L.lib().ccz_conv3x3_c256_f16_live(_stream(), P(x), P(w), P(b), P(r), P(y), cap, int(relu) | (2 if part & 1 else 0), P(live_dev), part, n_parts))


def check_live(boards, live, n_parts):
    assert 0 <= live <= boards
    c = live_case(boards)
    F64.report(f"board-major live conv, {boards} boards, live {live} in {n_parts}", c["worst"], c["share"])
    x, r, w, b = live_operands(boards)
    cap = E.planned_cap(boards, n_parts)
    ranges = E.live_ranges(live, n_parts, cap // 90)
    assert sum(n for _, n in ranges) == live
    nl = i32(live)
    for res, relu in F64.COMBOS:
        what = f"boards {boards} live {live} in {n_parts} (cap {cap // 90} boards) res {res} relu {relu}"
        want = E.conv_live_expected(c["s"], c["r"] if res else None, relu, ranges, ff_fill((boards, 10, 9, 256)))
        y = poison((boards * 90, 256), F16)
        launch_live(x, w, b, r if res else None, y, boards, nl, n_parts, relu)
        got = host(y).reshape(boards, 10, 9, 256)
        E.assert_same(got[:live], want[:live], what, NAMES)
        assert np.all(got.view(np.int16)[live:] == -1), what + ": rows past the live boards written"
    what = f"boards {boards} live {live} in {n_parts}, over the residual"
    y = r.clone()
    launch_live(x, w, b, y, y, boards, nl, n_parts, True)
    got = host(y).reshape(boards, 10, 9, 256)
    E.assert_same(got[:live], E.conv_chain(c["s"][:live], c["r"][:live], True), what, NAMES)
    E.assert_same_bits(got[live:], E.rn16(c["r"][live:]), what + ": residual rows past the live boards", NAMES)


@pytest.mark.parametrize("live,n_parts", [(0, 1), (1, 1), (7, 1), (8, 2), (9, 3), (17, 2), (24, 3), (39, 1), (39, 4), (40, 1), (40, 3), (40, 6)])
def test_live_ranges_of_the_board_major_convolution(live, n_parts):
    """40 boards = 3600 pixels = 14 tiles + 16 pixels: tile edges fall inside boards, every range ends in a partial tile. (9, 3): ranges
    of 8, 1 and 0 boards; (40, 6): five ranges of 8 and an empty sixth; live 0 writes nothing. Residual x ReLU in all four
    combinations and the output written over the residual."""
    check_live(40, live, n_parts)


@pytest.mark.parametrize("live,n_parts", [(37, 1), (33, 1), (37, 2), (33, 2)])
def test_live_ranges_with_a_capacity_past_the_tensor(live, n_parts):
    """37 boards: the capacity rounds up to 40 (one part) / 24 boards per part (two), past the tensor, as net.py makes it; the kernel
    computes min(live range, capacity) boards and the live count never exceeds the batch."""
    assert E.planned_cap(37, n_parts) * n_parts > 37 * 90
    check_live(37, live, n_parts)


@functools.lru_cache(maxsize=None)
def stem_case(boards):
    leaf, w, b, s, worst, share = F64._stem_case(boards, 3)
    x64 = np.zeros((boards, 10, 9, 64))
    x64[..., :21] = np.concatenate([leaf[:, 49:56], leaf[:, 105:119]], axis=1).transpose(0, 2, 3, 1)
    return dict(leaf=leaf, x64=x64, w=w, b=b, s=s, worst=worst, share=share)


@pytest.mark.parametrize("boards", [1, 11, 37])
def test_live_stem_board_major(boards):
    """ccz_conv3x3_stem_f16_live without CONV_G16: one part, cap = ceil(B / 8) * 8 * 90 as _stem_fused passes it; live 1, B // 2 + 1, B"""
    L = _L()
    c = stem_case(boards)
    F64.report(f"board-major live stem {boards}", c["worst"], c["share"])
    x, w, b = h16(c["x64"]).view(-1, 64), h16(c["w"]), f32(c["b"])
    cap = -(-boards // 8) * 8 * 90
    for live in sorted({1, boards // 2 + 1, boards}):
        nl = i32(live)
        for relu in (1, 0):
            y = poison((boards * 90, 256), F16)
            L.check(L.lib().ccz_conv3x3_stem_f16_live(_stream(), P(x), P(w), P(b), P(y), cap, relu, P(nl), 0, 1))
            got = host(y).reshape(boards, 10, 9, 256)
            what = f"stem boards {boards} live {live} relu {relu}"
            E.assert_same(got[:live], E.conv_chain(c["s"][:live], None, bool(relu)), what, NAMES)
            assert np.all(got.view(np.int16)[live:] == -1), what + ": rows past the live boards written"


# ================================================================== 2. the gathering plane pack
SENTINEL_A, SENTINEL_B = 7.5, -3.25


@functools.lru_cache(maxsize=None)
def pack_case(B):
    rs = np.random.RandomState(700 + B)
    leaf = (rs.random_sample((B, 119, 10, 9)) > 0.7).astype(np.float16)
    leaf[:, :7] = 1                                                          # planes outside the live set must not leak in
    leaf[:, 56:105] = (rs.random_sample((B, 49, 10, 9)) > 0.5)
    return leaf, rs.permutation(B).astype(np.int32)


def pack_prefill(B, n_rows, g16, seed):
    """[R, 64] fp16 in memory order: sentinel A everywhere in output rows at or past n_rows, sentinel B in channels 24..63 of every row,
    anything (finite) in channels 0..23 of the rows below n_rows"""
    Bp = -(-B // 16) * 16 if g16 else B
    out = np.full((Bp, 90, 64), SENTINEL_A, np.float16)
    out[:n_rows, :, :24] = (np.random.RandomState(seed).standard_normal((n_rows, 90, 24)) * 4).astype(np.float16)
    out[:, :, 24:] = SENTINEL_B
    if g16:
        out = E.rows_to_g16(out.reshape(Bp, 10, 9, 64))
    return np.ascontiguousarray(out).reshape(Bp * 90, 64)


def run_pack(form, leaf, out, B, rows, n_rows):
    L = _L()
    if form == "rows":
        L.check(L.lib().ccz_pack_live_planes_rows_f16(_stream(), P(leaf), P(out), B, P(rows), P(n_rows)))
    elif form == "g16 rows":
        L.check(L.lib().ccz_pack_live_planes_g16_f16(_stream(), P(leaf), P(out), B, P(rows), P(n_rows)))
    elif form == "g16":
        L.check(L.lib().ccz_pack_live_planes_g16_f16(_stream(), P(leaf), P(out), B, None, None))
    else:
        L.check(L.lib().ccz_pack_live_planes_f16(_stream(), P(leaf), P(out), B))


def pack_expected(form, leaf, rows, n_rows, prefill):
    """the gathering forms: the restatement; the whole-batch forms write all eight chunks of every board's rows (zeros from channel 21 on)"""
    if form in ("rows", "g16 rows"):
        return E.pack_live_planes_rows(leaf, rows, n_rows, prefill, form == "g16 rows")
    B = leaf.shape[0]
    assert prefill.shape[0] == B * 90                                       # whole groups: every row of the buffer is some board's
    want = E.pack_live_planes_rows(leaf, np.arange(B), B, prefill, form == "g16")
    want[:, 24:] = 0
    return want


def check_pack_contract(got, prefill, leaf, rows, n_rows, g16, what):
    """the written contract, spelled out on the device output (beside the equality with the restatement)"""
    B = leaf.shape[0]
    Bp = prefill.shape[0] // 90
    lg = E.rows_from_g16(got, Bp).reshape(Bp, 90, 64) if g16 else got.reshape(Bp, 90, 64)      # [output row i][pixel][channel]
    lp = E.rows_from_g16(prefill, Bp).reshape(Bp, 90, 64) if g16 else prefill.reshape(Bp, 90, 64)
    src = np.concatenate([leaf[:, 49:56], leaf[:, 105:119]], axis=1).reshape(B, 21, 90).transpose(0, 2, 1)
    assert np.array_equal(lg[:n_rows, :, :21], src[rows[:n_rows]]), what + ": channels 0..20 are not the live planes of board rows[i]"
    assert np.all(lg[:n_rows, :, 21:24].view(np.uint16) == 0), what + ": channels 21..23 are not zero"
    assert np.all(lg[:, :, 24:] == np.float16(SENTINEL_B)), what + ": channels 24..63 written"
    assert np.array_equal(lg[n_rows:].view(np.uint16), lp[n_rows:].view(np.uint16)), what + ": rows at or past n_rows written"


@pytest.mark.parametrize("form,B", [("rows", 1), ("rows", 11), ("rows", 37), ("g16 rows", 48)])
def test_gathering_plane_pack(form, B):
    """output row i (g16: at ((i >> 4) * 90 + p) * 16 + (i & 15)) is board rows[i] for i < *n_rows, rows a random permutation; n_rows 0, 1,
    B // 2 + 1 and B"""
    leaf, rows = pack_case(B)
    leaf_d, rows_d = torch.from_numpy(leaf).to(_dev()), torch.from_numpy(rows).to(_dev())
    g16 = form == "g16 rows"
    for n_rows in sorted({0, 1, B // 2 + 1, B}):
        what = f"pack {form} B {B} n_rows {n_rows}"
        prefill = pack_prefill(B, n_rows, g16, n_rows)
        want = pack_expected(form, leaf, rows, n_rows, prefill)
        out, nl = torch.from_numpy(prefill).to(_dev()), i32(n_rows)
        run_pack(form, leaf_d, out, B, rows_d, nl)
        got = host(out)
        E.assert_same_bits(got, want, what, ("row", "channel"))
        check_pack_contract(got, prefill, leaf, rows, n_rows, g16, what)


# ================================================================== 3. the board-major family in arenas
@functools.lru_cache(maxsize=1)
def arena_conv_case():
    """65 boards; boards 0..n-1 of it are the n-board cases (a board's sums do not depend on the other boards)"""
    return F64.conv_case(65)


@functools.lru_cache(maxsize=1)
def arena_conv_operands():
    c = arena_conv_case()
    return h16(c["x"]).view(-1, 256), h16(c["r"]).view(-1, 256), h16(c["w"]), f32(c["b"])


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("boards,force", [(1, ""), (11, ""), (64, ""), (11, "CONV_FORCE_TILE"), (65, "")])
def test_board_major_convolution_in_arenas(boards, force, res):
    """ccz_conv3x3_c256_f16 on rows board * 90 + pos: k_conv3x3_small up to 64 boards, k_conv3x3_c256 at 65 and forced at 11. With a
    residual the input rows are the last bytes of their arena and the weights the last of theirs: both kernels clamp their halo rows
    into the tensor (p = p < 0 ? 0 : (p > M - 1 ? M - 1 : p), cczero_conv.h / cczero_conv_small.h), the tile kernel's weight prefetch
    wraps to chunk 0 and the small kernel repeats its last weight piece."""
    L = _L()
    c = arena_conv_case()
    F64.report(f"board-major conv in arenas, boards {boards}", c["worst"], c["share"])
    X, R, w, b = arena_conv_operands()
    n = boards * 90
    x, r = X[:n], R[:n]
    flags = 1 | (getattr(L, force) if force else 0)
    tail = "end" if res else "pad"
    what = f"boards {boards} {force or 'selected'} res {res} tail {tail}"
    want = E.conv_chain(c["s"][:boards], c["r"][:boards] if res else None, True)
    wa = weight_arena(w, tail)
    a = Arena({"b": b, "r": r, "y": ((n, 256), F16), "x": x}, outputs=("y",), last="x" if tail == "end" else None)
    F64.conv(a["x"], wa["w"], a["b"], a["r"] if res else None, a["y"], n, flags)
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    plain = F64.conv(x, w, b, r if res else None, poison((n, 256), F16), n, flags)
    torch.cuda.synchronize()
    assert same_bits(a["y"], plain), what + ": differs from the call on plain tensors"
    E.assert_same(host(a["y"]).reshape(boards, 10, 9, 256), want, what, NAMES)


@pytest.mark.parametrize("live,n_parts,tail", [(17, 2, "pad"), (40, 3, "end"), (0, 1, "pad")])
def test_live_board_major_convolution_in_arenas(live, n_parts, tail):
    """the live form of section 1 (40 boards, residual on), the live count inside the arena; (40, 3): ranges of 16, 16 and 8 boards, the
    last one ends where the input's arena ends (halo rows are clamped into the RANGE: M is the range's pixels)"""
    boards = 40
    c = live_case(boards)
    F64.report(f"live board-major conv in arenas, live {live} in {n_parts}", c["worst"], c["share"])
    x, r, w, b = live_operands(boards)
    what = f"live {live} in {n_parts} tail {tail}"
    want = E.conv_chain(c["s"][:live], c["r"][:live], True)
    wa = weight_arena(w, tail)
    a = Arena({"b": b, "r": r, "n": i32(live), "y": ((boards * 90, 256), F16), "x": x}, outputs=("y",), last="x" if tail == "end" else None)
    launch_live(a["x"], wa["w"], a["b"], a["r"], a["y"], boards, a["n"], n_parts, True)
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    plain = poison((boards * 90, 256), F16)
    nl = i32(live)
    launch_live(x, w, b, r, plain, boards, nl, n_parts, True)
    torch.cuda.synchronize()
    assert same_bits(a["y"], plain), what + ": differs from the call on plain tensors"
    got = host(a["y"]).reshape(boards, 10, 9, 256)
    E.assert_same(got[:live], want, what, NAMES)
    assert np.all(got.view(np.int16)[live:] == -1), what + ": rows past the live boards written"


@pytest.mark.parametrize("boards,tail", [(1, "pad"), (65, "end")])
def test_board_major_stem_in_arenas(boards, tail):
    """ccz_conv3x3_stem_f16 on k_conv3x3_small<false, 64> (1 board) and k_conv3x3_c256 with cin = 64 (65 boards; input rows and weights
    at the end of their arenas: the same clamps, one 64-channel chunk)"""
    L = _L()
    c = stem_case(boards)
    F64.report(f"board-major stem in arenas {boards}", c["worst"], c["share"])
    x, w, b = h16(c["x64"]).view(-1, 64), h16(c["w"]), f32(c["b"])
    n = boards * 90
    what = f"stem boards {boards} tail {tail}"
    wa = weight_arena(w, tail)
    a = Arena({"b": b, "y": ((n, 256), F16), "x": x}, outputs=("y",), last="x" if tail == "end" else None)
    L.check(L.lib().ccz_conv3x3_stem_f16(_stream(), P(a["x"]), P(wa["w"]), P(a["b"]), P(a["y"]), n, 1))
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    plain = poison((n, 256), F16)
    L.check(L.lib().ccz_conv3x3_stem_f16(_stream(), P(x), P(w), P(b), P(plain), n, 1))
    torch.cuda.synchronize()
    assert same_bits(a["y"], plain), what + ": differs from the call on plain tensors"
    E.assert_same(host(a["y"]).reshape(boards, 10, 9, 256), E.conv_chain(c["s"], None, True), what, NAMES)


@pytest.mark.parametrize("form,B", [("rows", 1), ("rows", 37), ("g16 rows", 48), ("plain", 11), ("g16", 48)])
def test_plane_pack_in_arenas(form, B):
    """k_pack_live_planes in every form; leaf tensor, rows and n_rows inside the arena, the output the only writable slice (prefilled as in
    section 2). The output keeps PAD behind it; the leaf tensor is last: a board's reads end with plane 118, its last plane."""
    leaf, rows = pack_case(B)
    g16 = form.startswith("g16")
    gathering = form.endswith("rows")
    for n_rows in sorted({0, 1, B // 2 + 1, B}) if gathering else (B,):
        what = f"pack {form} B {B} n_rows {n_rows} in an arena"
        prefill = pack_prefill(B, n_rows, g16, n_rows)
        want = pack_expected(form, leaf, rows, n_rows, prefill)
        a = Arena({"out": torch.from_numpy(prefill).to(_dev()), "rows": torch.from_numpy(rows).to(_dev()), "n": i32(n_rows),
                   "leaf": torch.from_numpy(leaf).to(_dev())}, outputs=("out",), last="leaf")
        run_pack(form, a["leaf"], a["out"], B, a["rows"], a["n"])
        a.assert_untouched(what)
        plain, leaf_d, rows_d, nl = torch.from_numpy(prefill).to(_dev()), torch.from_numpy(leaf).to(_dev()), torch.from_numpy(rows).to(_dev()), i32(n_rows)
        run_pack(form, leaf_d, plain, B, rows_d, nl)
        torch.cuda.synchronize()
        assert same_bits(a["out"], plain), what + ": differs from the call on plain tensors"
        E.assert_same_bits(host(a["out"]), want, what, ("row", "channel"))


@functools.lru_cache(maxsize=None)
def heads_case(B):
    """the operands of test_head_convolutions_on_their_own"""
    rs = np.random.RandomState(40 + B)
    x = E.grid_acts(rs, (B, 90, 256), std=1.0)
    w32, b32 = F64._head_weights(rs, 9, 128), np.zeros(32)
    b32[:24] = E.grid_bias(rs, 24, e=14)
    s, worst, share = E.gemm_exact(x.reshape(-1, 256), w32[:24], b32[:24], 2.0 ** -14, f"heads {B}")
    return dict(x=x, w32=w32, b32=b32, s=s.reshape(B, 90, 24), worst=worst, share=share, relu_share=E.needs_rounding(np.maximum(s, 0)))


@pytest.mark.parametrize("B", [1, 7, 11])
def test_board_major_head_convolutions_in_arenas(B):
    """ccz_heads_conv1x1_f16 without CONV_G16 (k_head_conv1x1<false>), live None, 1 and B: pad columns and boards past the count keep 0xFF.
    At 11 boards the tower rows are the last bytes of the arena: the kernel clamps a cell's rows to n_rows - 1 and reads 256 channels."""
    L = _L()
    c = heads_case(B)
    F64.report(f"heads {B} in arenas (sums)", c["worst"], c["share"])
    assert c["relu_share"] >= 0.25
    xd, wd, bd = h16(c["x"]), h16(c["w32"]), f32(c["b32"])
    for live in (None, 1, B):
        n = B if live is None else live
        what = f"heads B {B} live {live} in an arena"
        wpol, wval = E.heads_chain(c["s"][:n])
        items = {"w32": wd, "b32": bd, "pol": ((B, 1536), F16), "val": ((B, 640), F16), "n": i32(n), "x": xd}
        a = Arena(items, outputs=("pol", "val"), last="x" if B == 11 else None)
        L.check(L.lib().ccz_heads_conv1x1_f16(_stream(), P(a["x"]), P(a["w32"]), P(a["b32"]), P(a["pol"]), P(a["val"]), B, 0, None if live is None else P(a["n"])))
        a.assert_untouched(what)
        pol, val = poison((B, 1536), F16), poison((B, 640), F16)
        nl = i32(n)
        L.check(L.lib().ccz_heads_conv1x1_f16(_stream(), P(xd), P(wd), P(bd), P(pol), P(val), B, 0, None if live is None else P(nl)))
        torch.cuda.synchronize()
        assert same_bits(a["pol"], pol) and same_bits(a["val"], val), what + ": differs from the call on plain tensors"
        ph, vh = host(a["pol"]), host(a["val"])
        E.assert_same(ph[:n, :1530].reshape(n, 90, 17), wpol, what + " policy", ("board", "pos", "channel"))
        E.assert_same(vh[:n, :630].reshape(n, 90, 7), wval, what + " value", ("board", "pos", "channel"))
        pi, vi = ph.view(np.int16), vh.view(np.int16)
        assert np.all(pi[:n, 1530:] == -1) and np.all(vi[:n, 630:] == -1), what + ": pad columns written"
        assert np.all(pi[n:] == -1) and np.all(vi[n:] == -1), what + ": boards past the live count written"


@pytest.mark.parametrize("M", [1, 11, 16, 17, 130])
@pytest.mark.parametrize("shape", ["policy", "value"])
def test_fc_in_arenas(shape, M):
    """ccz_fc_f16 at the policy (N 2086, K 1536, ldc 2096) and value (N 256, K 640) shapes: k_fc_skinny_f16 up to 16 rows, k_fc_f16 above,
    k_fc_wide_f16 forced at 17 and 130 rows; live None and M // 2 + 1. Weights and bias padded to whole 128-row tiles (2176 / 256 rows),
    the kernels' contract. At 16 and 130 rows A holds the last bytes of its arena (lda = K): all three kernels clamp their A rows to the
    live rows (m < Ml ? m : Ml - 1) and read K columns of them."""
    L = _L()
    o = F64._fc_operands(shape, M)
    K, N, relu, lda, ldc, want = o["K"], o["N"], o["relu"], o["lda"], o["ldc"], o["want"]
    assert lda == K and o["w"].shape[0] == -(-N // 128) * 128 and np.array_equal(o["rows"], np.arange(M))
    F64.report(f"fc {shape} M {M} in arenas", o["worst"], o["share"])
    ad, wd, bd = h16(o["buf"]), h16(o["w"]), f32(o["b"])
    forms = (("selected", 0),) + ((("256 x 144 tiles", 4),) if M in (17, 130) else ())
    for live in (None, M // 2 + 1):
        n = M if live is None else live
        for name, force in forms:
            what = f"fc {shape} M {M} live {live}, {name}, in an arena"
            a = Arena({"w": wd, "bias": bd, "c": ((M, ldc), F16), "n": i32(n), "a": ad}, outputs=("c",), last="a" if M in (16, 130) else None)
            L.check(L.lib().ccz_fc_f16(_stream(), P(a["a"]), lda, P(a["w"]), P(a["bias"]), P(a["c"]), ldc, M, N, K, relu | force, None if live is None else P(a["n"])))
            a.assert_untouched(what)
            plain = poison((M, ldc), F16)
            nl = i32(n)
            L.check(L.lib().ccz_fc_f16(_stream(), P(ad), lda, P(wd), P(bd), P(plain), ldc, M, N, K, relu | force, None if live is None else P(nl)))
            torch.cuda.synchronize()
            assert same_bits(a["c"], plain), what + ": differs from the call on plain tensors"
            got = host(a["c"])
            E.assert_same(got[:n, :N], want[:n], what, ("row", "column"))
            gi = got.view(np.int16)
            assert np.all(gi[:, N:] == -1) and np.all(gi[n:] == -1), what + ": pad columns or rows past the live count written"


@pytest.mark.parametrize("M", [1, 3, 5])
def test_value_output_in_arenas(M):
    """ccz_value_out_f32 with the operands of test_value_output_nearest_candidate (rows 0 and 1 on fp16 ties from M = 3 on), with and without
    a live count: the nearest-candidate check on the live rows, 0xFF in the float32 rows past them"""
    L = _L()
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
    s, worst, share = E.gemm_exact(h, w2[None, :], np.array([b2]), 2.0 ** -(E.EA + E.EB), f"value {M}")
    s = s[:, 0]
    F64.report(f"value output {M} in arenas", worst, share, least=0.0)                 # (at most five sums: the share is what it is; the ties are asserted)
    assert np.abs(s).max() < 4
    if M >= 3:
        assert float(E.rn16(s[0])) == 1.0 and float(E.rn16(s[1])) == 1 + 2.0 ** -9
    hd, wd = h16(h), h16(w2)
    for live in (None, M // 2 + 1):
        n = M if live is None else live
        what = f"value M {M} live {live} in an arena"
        a = Arena({"h": hd, "w2": wd, "n": i32(n), "v": ((M,), torch.float32)}, outputs=("v",))
        L.check(L.lib().ccz_value_out_f32(_stream(), P(a["h"]), P(a["w2"]), b2, P(a["v"]), M, None if live is None else P(a["n"])))
        a.assert_untouched(what)
        plain = poison((M,), torch.float32)
        nl = i32(n)
        L.check(L.lib().ccz_value_out_f32(_stream(), P(hd), P(wd), b2, P(plain), M, None if live is None else P(nl)))
        torch.cuda.synchronize()
        assert same_bits(a["v"], plain), what + ": differs from the call on plain tensors"
        v = host(a["v"])
        bad = E.value_mismatches(v[:n], s[:n])
        assert bad.size == 0, f"{what}: row {int(bad[0])}: device {v[int(bad[0])]!r}, s {s[int(bad[0])]!r}; {bad.size} rows"
        assert np.all(v.view(np.int32)[n:] == -1), what + ": rows past the live count written"


@pytest.mark.parametrize("res", [False, True])
def test_bias_act_in_arenas(res):
    """ccz_bias_act_f16 on 630 rows x 64 channels, in place: y is the only writable slice; finite fp16 operands of every exponent"""
    L = _L()
    rs = np.random.RandomState(630 + res)
    rows, channels = 630, 64

    def patterns(shape):
        bits = rs.randint(0, 0x7c00, size=shape).astype(np.uint16) | (rs.randint(0, 2, size=shape).astype(np.uint16) << 15)
        return np.where(rs.random_sample(shape) < 0.5, bits.view(np.float16), (rs.standard_normal(shape) * 2).astype(np.float16))

    y0, r, b = patterns((rows, channels)), patterns((rows, channels)), patterns(channels)
    want = E.bias_act_chain(y0, b, r if res else None)
    assert not np.isnan(want.astype(np.float32)).any()
    yd, rd, bd = (torch.from_numpy(t).to(_dev()) for t in (y0, r, b))
    what = f"bias_act res {res} in an arena"
    a = Arena({"y": yd, "bias": bd, "r": rd}, outputs=("y",))
    L.check(L.lib().ccz_bias_act_f16(_stream(), P(a["y"]), P(a["bias"]), P(a["r"]) if res else None, rows, channels))
    a.assert_untouched(what)
    plain = yd.clone()
    L.check(L.lib().ccz_bias_act_f16(_stream(), P(plain), P(bd), P(rd) if res else None, rows, channels))
    torch.cuda.synchronize()
    assert same_bits(a["y"], plain), what + ": differs from the call on plain tensors"
    E.assert_same(host(a["y"]), want, what, ("row", "channel"))


# ================================================================== 4. planned against unplanned rows through InferenceNet
@functools.lru_cache(maxsize=1)
def planned_net():
    """256 channels, two blocks, non-trivial BatchNorm statistics (as test_gpu_frontends.py makes them)"""
    from chinesechesszero_amd.net import InferenceNet, Net
    dev = _dev()
    torch.manual_seed(21)
    net = Net(256, 2).to(dev).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 2)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    return InferenceNet(net).to(dev).eval()


@functools.lru_cache(maxsize=1)
def leaf_batches():
    from test_gpu_evaluator_depth import _leaf_batch
    return _leaf_batch(600, 16, seed=5), _leaf_batch(600, 12, seed=23)


@pytest.mark.parametrize("B", [11, 37, 64, 65, 320, 600])
def test_planned_rows_equal_unplanned_rows_on_one_inference_net(B):
    """One unplanned call, then planned calls on the SAME InferenceNet with rows a permutation and live counts B, 1, B // 2 + 1, then a
    planned call with live count B // 2 + 1 on a second leaf batch: the rows of the persistent plan buffers past the live count hold stale
    results of the earlier calls. Planned row i equals unplanned row rows[i] in the fp16 logits and the float32 value, bit for bit, for
    every i below the live count. Up to 64 boards that is k_conv3x3_small (unplanned) against k_conv3x3_c256 (planned) on whole
    evaluations; 600 boards run as two parts."""
    inf = planned_net()
    xa, xb = (t[:B].clone() for t in leaf_batches())
    assert not torch.equal(xa, xb)
    assert inf._path(xa) == "nhwc" and inf._path(xb) == "nhwc"
    assert inf.tower_chains(600, 1, False) == 2
    assert inf.tower_chains(B, inf.tower_groups(B, False), False) == (2 if B == 600 else 1)
    rows = torch.randperm(B, generator=torch.Generator().manual_seed(B)).to(torch.int32).to(_dev())
    lg0, v0 = (t.clone() for t in inf(xa, return_logits=True))
    assert lg0.dtype == torch.float16 and v0.dtype == torch.float32 and lg0.shape == (B, 2086) and v0.shape == (B,)
    assert bool(torch.isfinite(lg0).all()) and bool((v0.abs() <= 1).all())
    assert B == 1 or not torch.equal(lg0[0], lg0[1])

    def planned(x, live, lg_ref, v_ref, what):
        lg, v = inf(x, return_logits=True, plan=(rows, i32(live)))
        torch.cuda.synchronize()
        sel = rows[:live].long()
        assert same_bits(lg[:live], lg_ref[sel]), f"B {B} {what} live {live}: planned logits differ from the unplanned rows"
        assert same_bits(v[:live], v_ref[sel]), f"B {B} {what} live {live}: planned values differ from the unplanned rows"

    for live in (B, 1, B // 2 + 1):
        planned(xa, live, lg0, v0, "first batch")
    live = B // 2 + 1
    lgp, vp = (t.clone() for t in inf(xb, return_logits=True, plan=(rows, i32(live))))   # stale rows of the FIRST batch past `live` in the plan buffers
    lg1, v1 = inf(xb, return_logits=True)
    torch.cuda.synchronize()
    sel = rows[:live].long()
    assert same_bits(lgp[:live], lg1[sel]) and same_bits(vp[:live], v1[sel]), f"B {B} second batch live {live}: planned rows differ from the unplanned rows"
    assert not torch.equal(lg1[sel], lg0[sel])
