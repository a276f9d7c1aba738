"""GPU: the group-of-16 tower kernels stream their slabs and weights through buffer descriptors (csrc/cczero_conv.h cv_blds16): the
prefetches past a tile's last chunk are issued against empty descriptors and fetch nothing. What that must not change, and what it
must never do, is checked here with every tensor of a call -- input rows, packed weights, bias, residual, output, head weights and
head outputs -- carved out of device arenas whose other bytes hold 0xFF (a NaN as fp16 and as fp32):

  * the outputs equal, bit for bit, the same call on plain tensors AND the float64 chain of tests/evaluator_f64.py (operands on
    fixed-point grids under the exactness guard: the expected fp16 value is unique, there is no tolerance);
  * every arena byte outside the output slices is what it was.

16, 32 and 48 boards = one, two and three groups (an odd count: the last edge pair is one group twice); live counts 1, 16, 17, 33 and
48 in one to three launch parts; residual on and off; the five-tile launch, middle + edge launches, both tile classes in one launch,
the stem (one chunk) and the heads layer; a two-block tower with the heads end to end. With `tail` = "end" the input rows are the last
bytes of their arena (the last launch part ends where the allocation ends) and the layer's packed weights are the last layer of a
two-layer weight arena."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import evaluator_f64 as E

pytestmark = pytest.mark.gpu

PAD = 16384                      # bytes of 0xFF around every slice (a multiple of 16: the kernels want 16-byte aligned pointers)
G = 2.0 ** -(E.EA + E.EB)
NAMES = ("board", "rank", "file", "channel")
BOARDS = 48


def _dev():
    return torch.device("cuda", 0)


def _L():
    from chinesechesszero_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def h16(a):
    return torch.from_numpy(np.ascontiguousarray(E.rn16(a))).to(_dev())


def f32(a):
    a = np.ascontiguousarray(np.asarray(a, np.float64))
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return torch.from_numpy(a.astype(np.float32)).to(_dev())


def host(t):
    return t.cpu().numpy()


def poison(shape, dtype):
    """a plain tensor of 0xFF bytes: what an arena slice holds before a kernel writes it"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=_dev()).view(dtype).view(shape)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Arena:
    """One device allocation of 0xFF bytes holding the tensors `items` (name -> tensor, or (shape, dtype) for an output that starts
    as 0xFF) PAD bytes apart; the tensor named `last` sits at the very end, nothing behind it."""

    def __init__(self, items, outputs=(), last=None):
        order = [k for k in items if k != last] + ([last] if last else [])
        self.span, off = {}, PAD
        sizes = {}
        for k in order:
            v = items[k]
            shape, dtype = (tuple(v.shape), v.dtype) if torch.is_tensor(v) else v
            sizes[k] = (shape, dtype, int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size())
        for k in order:
            n = sizes[k][2]
            self.span[k] = (off, off + n)
            off += n + (0 if k == last else PAD)
            off = -(-off // 256) * 256 if k != last else off
        self.bytes = torch.full((off,), 0xFF, dtype=torch.uint8, device=_dev())
        self.t = {}
        for k in order:
            shape, dtype, _ = sizes[k]
            a, b = self.span[k]
            self.t[k] = self.bytes[a:b].view(dtype).view(shape)
            if torch.is_tensor(items[k]):
                self.t[k].copy_(items[k])
        if last:
            assert self.span[last][1] == self.bytes.numel()
        self.outputs = tuple(outputs)
        self.before = self.bytes.clone()

    def __getitem__(self, k):
        return self.t[k]

    def assert_untouched(self, what):
        """every byte outside the output slices is what it was before the calls"""
        torch.cuda.synchronize()
        now = self.bytes.clone()
        for k in self.outputs:
            a, b = self.span[k]
            now[a:b] = self.before[a:b]
        if not torch.equal(now, self.before):
            at = int(torch.nonzero(now != self.before)[0])
            owner = [k for k, (a, b) in self.span.items() if a <= at < b] or ["padding"]
            raise AssertionError(f"{what}: arena byte {at} ({owner[0]}) changed; {int((now != self.before).sum())} bytes differ")


def weight_arena(wp, tail):
    """the layer's packed weights in a two-layer arena: `end`: as the LAST layer, the arena ends with its last byte; `pad`: as the
    first, another layer and padding behind it. The other layer holds finite weights of another seed."""
    other = (torch.randn(wp.shape, device=_dev(), generator=torch.Generator(device=_dev()).manual_seed(5)) * 0.03).half()
    if tail == "end":
        return Arena({"other": other, "w": wp}, last="w")
    return Arena({"w": wp, "other": other})


# ------------------------------------------------------------------ operands + float64 reference, once per module
@functools.lru_cache(maxsize=1)
def case():
    """48 boards on the main grids: x, r [48, 10, 9, 256], w [256, 3, 3, 256], b [256] and the exact sums; boards 0..15 / 0..31 of it are
    the 16- and 32-board cases (a board's sums do not depend on the other boards)."""
    rs = np.random.RandomState(4242)
    x = E.grid_acts(rs, (BOARDS, 10, 9, 256))
    r = E.grid_acts(rs, (BOARDS, 10, 9, 256), relu=False)
    w = E.grid_weights(rs, (256, 3, 3, 256))
    b = E.grid_bias(rs, 256)
    E.assert_on_grid(x, E.EA)
    E.assert_on_grid(w, E.EB)
    s, worst, share = E.conv_exact(x, w, b, G, "tile stream conv")
    print(f"\ntile stream conv: guard fill {worst:.4f} of 1, needs rounding {share:.3f}")
    assert worst < 1.0 and share >= 0.5
    return dict(x=x, r=r, w=w, b=b, s=s)


@functools.lru_cache(maxsize=1)
def device_operands():
    c = case()
    xg = h16(np.ascontiguousarray(E.rows_to_g16(c["x"]))).view(-1, 256)
    rg = h16(np.ascontiguousarray(E.rows_to_g16(c["r"]))).view(-1, 256)
    return xg, rg, E._pack_w(h16(c["w"]), 256), f32(c["b"])


def forms():
    L = _L()
    return (("five tiles", L.CONV_G16), ("middle + edge launches", L.CONV_G16 | L.CONV_G16_EDGE_TILES),
            ("one launch", L.CONV_G16 | L.CONV_G16_EDGE_TILES | L.CONV_G16_ONE_LAUNCH))


def launch_layer(x, w, b, r, y, boards, flags, live=None, n_parts=1):
    L = _L()
    if live is None:
        L.check(L.lib().ccz_conv3x3_c256_f16(_stream(), P(x), P(w), P(b), P(r), P(y), boards * 90, flags))
        return
    cap = -(-(boards // 16) // n_parts) * 1440
    for part in range(n_parts):
        L.check(L.lib().ccz_conv3x3_c256_f16_live(_stream(), P(x), P(w), P(b), P(r), P(y), cap, flags | (2 if part & 1 else 0), P(live), part, n_parts))


def check_layer(boards, res, live, n_parts, tail):
    c = case()
    xg, rg, wp, b = device_operands()
    xg, rg = xg[:boards * 90], rg[:boards * 90]
    n = boards if live is None else live
    groups = -(-n // 16)
    want = E.conv_chain(c["s"][:groups * 16], c["r"][:groups * 16] if res else None, True)
    for name, form in forms():
        what = f"boards {boards} res {res} live {live} in {n_parts}, {name}, tail {tail}"
        wa = weight_arena(wp, tail)
        items = {"b": b, "r": rg, "y": ((boards * 90, 256), torch.float16), "x": xg}
        if live is not None:
            items["n"] = torch.tensor([live], dtype=torch.int32, device=_dev())
        a = Arena(items, outputs=("y",), last="x" if tail == "end" else None)
        launch_layer(a["x"], wa["w"], a["b"], a["r"] if res else None, a["y"], boards, 1 | form, a["n"] if live is not None else None, n_parts)
        a.assert_untouched(what)
        wa.assert_untouched(what + " (weights)")
        plain = poison((boards * 90, 256), torch.float16)
        launch_layer(xg, wp, b, rg if res else None, plain, boards, 1 | form,
                     None if live is None else torch.tensor([live], dtype=torch.int32, device=_dev()), n_parts)
        torch.cuda.synchronize()
        assert same_bits(a["y"], plain), what + ": differs from the call on plain tensors"
        got = E.rows_from_g16(host(a["y"]), boards)
        E.assert_same(got[:groups * 16], want, what, NAMES)
        assert np.all(host(a["y"].view(torch.int16))[groups * 1440:] == -1), what + ": rows past the live groups written"


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("boards", [16, 32, 48])
def test_layer_whole_batch_in_arenas(boards, res):
    check_layer(boards, res, None, 1, "end" if boards == 48 else "pad")


@pytest.mark.parametrize("n_parts", [1, 2, 3])
@pytest.mark.parametrize("live", [1, 16, 17, 33, 48])
def test_layer_live_rows_in_arenas(live, n_parts):
    """48 boards of capacity, the first `live` hold rows, cut into n_parts launch parts; residual on for an odd number of parts,
    off for two; live 48 and 33 with the input rows at the end of their allocation and the weights as its last layer"""
    check_layer(BOARDS, n_parts != 2, live, n_parts, "end" if live in (33, 48) else "pad")


# ------------------------------------------------------------------ the stem: one chunk of 32 channels, every next-chunk prefetch is dead
@pytest.mark.parametrize("boards,live,n_parts,tail", [(16, None, 1, "pad"), (48, None, 1, "end"), (48, 17, 2, "pad"), (48, 33, 1, "end")])
def test_stem_in_arenas(boards, live, n_parts, tail):
    L = _L()
    rs = np.random.RandomState(99 + boards)
    x21 = (rs.random_sample((boards, 10, 9, 21)) > 0.8).astype(np.float64)
    w = np.zeros((256, 3, 3, 64))
    w[..., :21] = E.grid_weights(rs, (256, 3, 3, 21), std=0.05)
    b = E.grid_bias(rs, 256)
    s, worst, share = E.conv_exact(x21, w[..., :21], b, G, f"stem {boards}")
    assert worst < 1.0 and share >= 0.5
    x64 = np.zeros((boards, 10, 9, 64))
    x64[..., :21] = x21
    xg = h16(np.ascontiguousarray(E.rows_to_g16(x64))).view(-1, 64)
    wp, bd = E._pack_w(h16(w), 64), f32(b)
    n = boards if live is None else live
    groups = -(-n // 16)
    want = E.conv_chain(s[:groups * 16], None, True)
    nl = None if live is None else torch.tensor([live], dtype=torch.int32, device=_dev())
    cap = -(-(boards // 16) // n_parts) * 1440

    def run(x, w_, b_, y, n_):
        if live is None:
            L.check(L.lib().ccz_conv3x3_stem_f16(_stream(), P(x), P(w_), P(b_), P(y), boards * 90, 1 | L.CONV_G16))
        else:
            for part in range(n_parts):
                L.check(L.lib().ccz_conv3x3_stem_f16_live(_stream(), P(x), P(w_), P(b_), P(y), cap, 1 | L.CONV_G16, P(n_), part, n_parts))

    what = f"stem boards {boards} live {live} in {n_parts}, tail {tail}"
    wa = weight_arena(wp, tail)
    items = {"b": bd, "y": ((boards * 90, 256), torch.float16), "x": xg}
    if live is not None:
        items["n"] = nl
    a = Arena(items, outputs=("y",), last="x" if tail == "end" else None)
    run(a["x"], wa["w"], a["b"], a["y"], a["n"] if live is not None else None)
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    plain = poison((boards * 90, 256), torch.float16)
    run(xg, wp, bd, plain, nl)
    torch.cuda.synchronize()
    assert same_bits(a["y"], plain), what
    E.assert_same(E.rows_from_g16(host(a["y"]), boards)[:groups * 16], want, what, NAMES)
    assert np.all(host(a["y"].view(torch.int16))[groups * 1440:] == -1), what


# ------------------------------------------------------------------ the heads layer
def head_operands(rs, e_w, e_b):
    w32, b32 = np.zeros((32, 256)), np.zeros(32)
    w32[:24] = E.grid_normal(rs, (24, 256), 0.08, e_w, 4)
    b32[:24] = E.grid_bias(rs, 24, e=e_b)
    return w32, b32


def launch_heads(x, w, b, r, w32, b32, pol, val, boards, flags, live, n_parts):
    L = _L()
    if live is None:
        L.check(L.lib().ccz_conv3x3_c256_heads_f16(_stream(), P(x), P(w), P(b), P(r), P(w32), P(b32), P(pol), P(val), boards * 90, flags, None, 0, 1))
        return
    cap = -(-(boards // 16) // n_parts) * 1440
    for part in range(n_parts):
        L.check(L.lib().ccz_conv3x3_c256_heads_f16(_stream(), P(x), P(w), P(b), P(r), P(w32), P(b32), P(pol), P(val), cap,
                                                   flags | (2 if part & 1 else 0), P(live), part, n_parts))


def check_head_outputs(pol, val, s24, n, what):
    wpol, wval = E.heads_chain(s24[:n])
    ph, vh = host(pol), host(val)
    E.assert_same(ph[:n, :1530].reshape(n, 90, 17), wpol, what + " policy", ("board", "pos", "channel"))
    E.assert_same(vh[:n, :630].reshape(n, 90, 7), wval, what + " value", ("board", "pos", "channel"))
    pi, vi = host(pol.view(torch.int16)), host(val.view(torch.int16))
    assert np.all(pi[:n, 1530:] == -1) and np.all(vi[:n, 630:] == -1) and np.all(pi[n:] == -1) and np.all(vi[n:] == -1), what + ": pad or dead boards written"


@pytest.mark.parametrize("boards,live,n_parts,tail", [(16, None, 1, "pad"), (48, None, 1, "end"), (48, 33, 2, "end"), (32, 17, 1, "pad"), (48, 1, 3, "pad")])
def test_heads_layer_in_arenas(boards, live, n_parts, tail):
    """ccz_conv3x3_c256_heads_f16 (five tiles, and middle + edge-pair launches): the layer's output is never stored, the head outputs
    are slices of the arena as well. The layer's fp16 output is a multiple of 2^-15, the head weights sit on 2^-4: second guard on 2^-19."""
    L = _L()
    c = case()
    xg, rg, wp, b = device_operands()
    xg, rg = xg[:boards * 90], rg[:boards * 90]
    n = boards if live is None else live
    w32, b32 = head_operands(np.random.RandomState(17), 4, 19)
    y = E.conv_chain(c["s"][:n], np.abs(c["r"][:n]), True).astype(np.float64)
    s2, worst, share = E.gemm_exact(y.reshape(-1, 256), w32[:24], b32[:24], 2.0 ** -19, "heads on y")
    assert worst < 1.0
    s2 = s2.reshape(n, 90, 24)
    rpos = rg.abs()
    w32d, b32d = h16(w32), f32(b32)
    for edge in (0, L.CONV_G16_EDGE_TILES):
        what = f"heads layer boards {boards} live {live} in {n_parts} edge {edge} tail {tail}"
        wa = weight_arena(wp, tail)
        items = {"b": b, "r": rpos, "w32": w32d, "b32": b32d, "pol": ((boards, 1536), torch.float16), "val": ((boards, 640), torch.float16), "x": xg}
        if live is not None:
            items["n"] = torch.tensor([live], dtype=torch.int32, device=_dev())
        a = Arena(items, outputs=("pol", "val"), last="x" if tail == "end" else None)
        launch_heads(a["x"], wa["w"], a["b"], a["r"], a["w32"], a["b32"], a["pol"], a["val"], boards, 1 | L.CONV_G16 | edge,
                     a["n"] if live is not None else None, n_parts)
        a.assert_untouched(what)
        wa.assert_untouched(what + " (weights)")
        pol, val = poison((boards, 1536), torch.float16), poison((boards, 640), torch.float16)
        launch_heads(xg, wp, b, rpos, w32d, b32d, pol, val, boards, 1 | L.CONV_G16 | edge,
                     None if live is None else torch.tensor([live], dtype=torch.int32, device=_dev()), n_parts)
        torch.cuda.synchronize()
        assert same_bits(a["pol"], pol) and same_bits(a["val"], val), what + ": differs from the call on plain tensors"
        check_head_outputs(a["pol"], a["val"], s2, n, what)


# ------------------------------------------------------------------ a two-block tower with the heads, end to end
@functools.lru_cache(maxsize=1)
def tower_case():
    """Stem + two residual blocks + heads on 48 boards, exact in float64 the whole way: the stem reads 0/1 planes with weights on 2^-10,
    so its fp16 output is a multiple of 2^-10; the four tower layers have sparse weights on the grid 2^-2 (|w| = 1/4, 1.4 % of them), so
    layer k's products are multiples of 2^-(10 + 2 k) and its fp16 output (rounding only coarsens) a multiple of the same; the head
    weights sit on 2^-2 as well: the last guard is on g = 2^-20. Every guard is asserted."""
    rs = np.random.RandomState(31337)
    B = BOARDS
    x21 = (rs.random_sample((B, 10, 9, 21)) > 0.8).astype(np.float64)
    w0 = np.zeros((256, 3, 3, 64))
    w0[..., :21] = E.grid_weights(rs, (256, 3, 3, 21), std=0.05)
    b0 = E.grid_bias(rs, 256, e=10)
    s, worst, _ = E.conv_exact(x21, w0[..., :21], b0, 2.0 ** -10, "tower stem")
    acts = [E.conv_chain(s, None, True).astype(np.float64)]
    ws, bs, fills = [], [], [worst]
    for k in range(4):
        w = np.where(rs.random_sample((256, 3, 3, 256)) < 0.014, np.where(rs.random_sample((256, 3, 3, 256)) < 0.5, 0.25, -0.25), 0.0)
        b = E.grid_bias(rs, 256, e=6, std=0.1)
        e = 10 + 2 * (k + 1)
        E.assert_on_grid(acts[-1], e - 2, f"tower input of layer {k}")
        s, worst, _ = E.conv_exact(acts[-1], w, b, 2.0 ** -e, f"tower layer {k}")
        res = acts[-2] if k & 1 else None                                    # the second layer of a block adds the block's input
        acts.append(E.conv_chain(s, res, True).astype(np.float64))
        ws.append(w); bs.append(b); fills.append(worst)
    w32, b32 = np.zeros((32, 256)), np.zeros(32)
    w32[:24] = np.where(rs.random_sample((24, 256)) < 0.1, np.where(rs.random_sample((24, 256)) < 0.5, 0.25, -0.25), 0.0)
    b32[:24] = E.grid_bias(rs, 24, e=6)
    E.assert_on_grid(acts[-1], 18, "tower output")
    s2, worst, _ = E.gemm_exact(acts[-1].reshape(-1, 256), w32[:24], b32[:24], 2.0 ** -20, "tower heads")
    fills.append(worst)
    print("\ntwo-block tower: guard fills", " ".join(f"{f:.4f}" for f in fills), "; live outputs", float((acts[-1] > 0).mean()))
    assert 0.05 < float((acts[-1] > 0).mean()) < 0.95                         # the tower neither died nor saturated
    return dict(x21=x21, w0=w0, b0=b0, ws=ws, bs=bs, w32=w32, b32=b32, s2=s2.reshape(B, 90, 24))


@pytest.mark.parametrize("live,n_parts", [(None, 1), (33, 2)])
def test_two_block_tower_with_heads_in_arenas(live, n_parts):
    """stem -> (layer, layer + residual) -> (layer, heads layer + residual), every tensor of every call in ONE arena (the input rows
    last), the five packed weight sets in one weight arena with the heads layer's set as its last layer; one launch per layer and
    middle + edge launches for the heads layer. Against the same calls on plain tensors and the float64 chain."""
    L = _L()
    t = tower_case()
    B = BOARDS
    n = B if live is None else live
    x64 = np.zeros((B, 10, 9, 64))
    x64[..., :21] = t["x21"]
    xg = h16(np.ascontiguousarray(E.rows_to_g16(x64))).view(-1, 64)
    wps = [E._pack_w(h16(t["w0"]), 64)] + [E._pack_w(h16(w), 256) for w in t["ws"]]
    bds = [f32(t["b0"])] + [f32(b) for b in t["bs"]]
    w32d, b32d = h16(t["w32"]), f32(t["b32"])
    form = L.CONV_G16 | L.CONV_G16_EDGE_TILES | L.CONV_G16_ONE_LAUNCH
    nl = None if live is None else torch.tensor([live], dtype=torch.int32, device=_dev())
    cap = -(-(B // 16) // n_parts) * 1440

    def run(x, w, b, act, w32, b32, pol, val, n_):
        def conv(xi, k, res, yo):
            if n_ is None:
                if k == 0:
                    L.check(L.lib().ccz_conv3x3_stem_f16(_stream(), P(xi), P(w[0]), P(b[0]), P(yo), B * 90, 1 | L.CONV_G16))
                else:
                    L.check(L.lib().ccz_conv3x3_c256_f16(_stream(), P(xi), P(w[k]), P(b[k]), P(res), P(yo), B * 90, 1 | form))
                return
            for part in range(n_parts):
                if k == 0:
                    L.check(L.lib().ccz_conv3x3_stem_f16_live(_stream(), P(xi), P(w[0]), P(b[0]), P(yo), cap, 1 | L.CONV_G16, P(n_), part, n_parts))
                else:
                    L.check(L.lib().ccz_conv3x3_c256_f16_live(_stream(), P(xi), P(w[k]), P(b[k]), P(res), P(yo), cap, 1 | form, P(n_), part, n_parts))
        conv(x, 0, None, act[0])
        conv(act[0], 1, None, act[1])
        conv(act[1], 2, act[0], act[2])
        conv(act[2], 3, None, act[1])                                         # act[1] is free again: the evaluator's ping-pong
        launch_heads(act[1], w[4], b[4], act[2], w32, b32, pol, val, B, 1 | L.CONV_G16 | L.CONV_G16_EDGE_TILES, n_, n_parts)

    rows = ((B * 90, 256), torch.float16)
    items = {f"b{k}": bds[k] for k in range(5)}
    items.update({"w32": w32d, "b32": b32d, "a0": rows, "a1": rows, "a2": rows, "pol": ((B, 1536), torch.float16), "val": ((B, 640), torch.float16)})
    if live is not None:
        items["n"] = nl
    items["x"] = xg
    a = Arena(items, outputs=("a0", "a1", "a2", "pol", "val"), last="x")
    wa = Arena({f"w{k}": wps[k] for k in range(5)}, last="w4")
    run(a["x"], [wa[f"w{k}"] for k in range(5)], [a[f"b{k}"] for k in range(5)], [a["a0"], a["a1"], a["a2"]], a["w32"], a["b32"], a["pol"], a["val"],
        a["n"] if live is not None else None)
    what = f"two-block tower live {live} in {n_parts}"
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    act = [poison(*rows) for _ in range(3)]
    pol, val = poison((B, 1536), torch.float16), poison((B, 640), torch.float16)
    run(xg, wps, bds, act, w32d, b32d, pol, val, nl)
    torch.cuda.synchronize()
    assert same_bits(a["pol"], pol) and same_bits(a["val"], val), what + ": differs from the calls on plain tensors"
    for k in range(3):
        assert same_bits(a[f"a{k}"], act[k]), what + f": activation buffer {k} differs from the calls on plain tensors"
    check_head_outputs(a["pol"], a["val"], t["s2"], n, what)
