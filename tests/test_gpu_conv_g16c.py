"""GPU: the chunk-major "G16C" forms of the tower kernels (csrc/cczero_conv_g16.h g16c_off; include/cczero.h ccz_conv3x3_*_g16c_f16).

Inside a 16-board group the bytes are [chunk 0..7][row 0..1439][32 channels] instead of rows of 256 channels; tiles, MFMAs and their
order are the row forms'. So every output of a G16C entry point, permuted back, must equal BIT FOR BIT the output of its
CCZ_CONV_G16 twin on the same operands and the float64 chain of tests/evaluator_f64.py (fixed-point operands under the exactness
guard: no tolerance). Every tensor of a call is a slice of an arena of 0xFF bytes whose other bytes must stay what they were.
32 and 48 boards (two and three groups: the last edge pair is one group twice), live counts 1 / 16 / 17 / 33 / 48 in one to three
launch parts (three parts of 48 boards: one group of capacity per launch), residual on and off, both tile orders; the stem into G16C;
the heads layer; a two-block tower with the heads end to end; ``InferenceNet.forward`` with the option on and off, dense and planned,
and its fall-back to rows when a precondition is off. Operands and references are test_gpu_conv_tile_stream's (computed once)."""
import numpy as np
import pytest
import torch

import evaluator_f64 as E
import test_gpu_conv_tile_stream as T

pytestmark = pytest.mark.gpu

Arena, P, h16, f32, host, poison, same_bits = T.Arena, T.P, T.h16, T.f32, T.host, T.poison, T.same_bits
BOARDS = T.BOARDS


def _L():
    from chinesechesszero_amd import _lib
    return _lib


def _net():
    from chinesechesszero_amd import net
    return net


def form():
    L = _L()
    return L.CONV_G16 | L.CONV_G16_EDGE_TILES | L.CONV_G16_ONE_LAUNCH | L.CONV_G16_QUAD


def live_count(live):
    return None if live is None else torch.tensor([live], dtype=torch.int32, device=T._dev())


def launch_layer(chunk_major, x, w, b, r, y, boards, flags, live=None, n_parts=1):
    """One tower layer on the G16C entry points, or on their row twins (the yardstick)."""
    L = _L()
    dense, planned = ((L.lib().ccz_conv3x3_c256_g16c_f16, L.lib().ccz_conv3x3_c256_g16c_f16_live) if chunk_major
                      else (L.lib().ccz_conv3x3_c256_f16, L.lib().ccz_conv3x3_c256_f16_live))
    if live is None:
        L.check(dense(T._stream(), P(x), P(w), P(b), P(r), P(y), boards * 90, flags))
        return
    cap = -(-(boards // 16) // n_parts) * 1440
    for part in range(n_parts):
        L.check(planned(T._stream(), P(x), P(w), P(b), P(r), P(y), cap, flags ^ (2 if part & 1 else 0), P(live), part, n_parts))


def check_layer(boards, res, live, n_parts, tail):
    N = _net()
    c = T.case()
    xg, rg, wp, b = T.device_operands()
    xg, rg = xg[:boards * 90], rg[:boards * 90]
    xc, rc = N.g16_to_g16c(xg), N.g16_to_g16c(rg)
    n = boards if live is None else live
    groups = -(-n // 16)
    want = E.conv_chain(c["s"][:groups * 16], c["r"][:groups * 16] if res else None, True)
    for order in (0, 2):                                                       # ascending / descending tiles
        what = f"G16C boards {boards} res {res} live {live} in {n_parts}, order {order}, tail {tail}"
        wa = T.weight_arena(wp, tail)
        items = {"b": b, "r": rc, "y": ((boards * 90, 256), torch.float16), "x": xc}
        if live is not None:
            items["n"] = live_count(live)
        a = Arena(items, outputs=("y",), last="x" if tail == "end" else None)
        launch_layer(True, a["x"], wa["w"], a["b"], a["r"] if res else None, a["y"], boards, 1 | order | form(), a["n"] if live is not None else None, n_parts)
        a.assert_untouched(what)
        wa.assert_untouched(what + " (weights)")
        rows = poison((boards * 90, 256), torch.float16)
        launch_layer(False, xg, wp, b, rg if res else None, rows, boards, 1 | order | form(), live_count(live), n_parts)
        torch.cuda.synchronize()
        assert np.all(host(a["y"].view(torch.int16))[groups * 1440:] == -1), what + ": rows past the live groups written"
        back = N.g16c_to_g16(a["y"])
        assert same_bits(back[:groups * 1440], rows[:groups * 1440]), what + ": differs from the row entry point"
        E.assert_same(E.rows_from_g16(host(back), boards)[:groups * 16], want, what, T.NAMES)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("boards", [32, 48])
def test_layer_whole_batch_in_arenas(boards, res):
    check_layer(boards, res, None, 1, "end" if boards == 48 else "pad")


@pytest.mark.parametrize("n_parts", [1, 2, 3])
@pytest.mark.parametrize("live", [1, 16, 17, 33, 48])
def test_layer_live_rows_in_arenas(live, n_parts):
    """48 boards of capacity, the first `live` hold rows, in n_parts launch parts (odd parts in the other tile order); residual on for
    an odd number of parts, off for two"""
    check_layer(BOARDS, n_parts != 2, live, n_parts, "end" if live in (33, 48) else "pad")


def test_layer_in_place_over_the_residual():
    """the second convolution of a block writes its output over its residual input: a tile reads R at, and writes Y to, the same bytes"""
    N = _net()
    xg, rg, wp, b = T.device_operands()
    xc = N.g16_to_g16c(xg)
    a = Arena({"b": b, "r": N.g16_to_g16c(rg), "x": xc}, outputs=("r",))
    launch_layer(True, a["x"], wp, a["b"], a["r"], a["r"], BOARDS, 1 | form())
    a.assert_untouched("in place")
    rows = poison((BOARDS * 90, 256), torch.float16)
    launch_layer(False, xg, wp, b, rg, rows, BOARDS, 1 | form())
    torch.cuda.synchronize()
    assert same_bits(N.g16c_to_g16(a["r"]), rows)


def test_refused_forms():
    """only the quad one-launch form exists in G16C: anything else is an error, not another kernel"""
    L = _L()
    xg, rg, wp, b = T.device_operands()
    y = poison((BOARDS * 90, 256), torch.float16)
    for fl in (L.CONV_G16, L.CONV_G16 | L.CONV_G16_EDGE_TILES, L.CONV_G16 | L.CONV_G16_EDGE_TILES | L.CONV_G16_ONE_LAUNCH,
               L.CONV_G16 | L.CONV_G16_EDGE_TILES | L.CONV_G16_QUAD, form() & ~L.CONV_G16):
        assert L.lib().ccz_conv3x3_c256_g16c_f16(T._stream(), P(xg), P(wp), P(b), None, P(y), BOARDS * 90, 1 | fl) != 0
    torch.cuda.synchronize()
    assert np.all(host(y.view(torch.int16)) == -1)


# ------------------------------------------------------------------ the stem: rows of packed planes in, G16C out
@pytest.mark.parametrize("boards,live,n_parts,tail", [(32, None, 1, "pad"), (48, None, 1, "end"), (48, 17, 2, "pad"), (48, 33, 1, "end")])
def test_stem_into_g16c(boards, live, n_parts, tail):
    L, N = _L(), _net()
    rs = np.random.RandomState(99 + boards)
    x21 = (rs.random_sample((boards, 10, 9, 21)) > 0.8).astype(np.float64)
    w = np.zeros((256, 3, 3, 64))
    w[..., :21] = E.grid_weights(rs, (256, 3, 3, 21), std=0.05)
    b = E.grid_bias(rs, 256)
    s, worst, share = E.conv_exact(x21, w[..., :21], b, T.G, f"stem {boards}")
    assert worst < 1.0 and share >= 0.5
    x64 = np.zeros((boards, 10, 9, 64))
    x64[..., :21] = x21
    xg = h16(np.ascontiguousarray(E.rows_to_g16(x64))).view(-1, 64)
    wp, bd = E._pack_w(h16(w), 64), f32(b)
    n = boards if live is None else live
    groups = -(-n // 16)
    want = E.conv_chain(s[:groups * 16], None, True)
    cap = -(-(boards // 16) // n_parts) * 1440

    def run(chunk_major, x, w_, b_, y, n_):
        lib = L.lib()
        if live is None:
            fn = lib.ccz_conv3x3_stem_g16c_f16 if chunk_major else lib.ccz_conv3x3_stem_f16
            L.check(fn(T._stream(), P(x), P(w_), P(b_), P(y), boards * 90, 1 | L.CONV_G16))
        else:
            fn = lib.ccz_conv3x3_stem_g16c_f16_live if chunk_major else lib.ccz_conv3x3_stem_f16_live
            for part in range(n_parts):
                L.check(fn(T._stream(), P(x), P(w_), P(b_), P(y), cap, 1 | L.CONV_G16, P(n_), part, n_parts))

    what = f"G16C stem boards {boards} live {live} in {n_parts}, tail {tail}"
    wa = T.weight_arena(wp, tail)
    items = {"b": bd, "y": ((boards * 90, 256), torch.float16), "x": xg}
    if live is not None:
        items["n"] = live_count(live)
    a = Arena(items, outputs=("y",), last="x" if tail == "end" else None)
    run(True, a["x"], wa["w"], a["b"], a["y"], a["n"] if live is not None else None)
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    rows = poison((boards * 90, 256), torch.float16)
    run(False, xg, wp, bd, rows, live_count(live))
    torch.cuda.synchronize()
    assert np.all(host(a["y"].view(torch.int16))[groups * 1440:] == -1), what
    back = N.g16c_to_g16(a["y"])
    assert same_bits(back[:groups * 1440], rows[:groups * 1440]), what + ": differs from the row entry point"
    E.assert_same(E.rows_from_g16(host(back), boards)[:groups * 16], want, what, T.NAMES)


# ------------------------------------------------------------------ the heads layer: reads X and R in G16C, head outputs in board order
def launch_heads(chunk_major, x, w, b, r, w32, b32, pol, val, boards, flags, live, n_parts):
    L = _L()
    fn = L.lib().ccz_conv3x3_c256_heads_g16c_f16 if chunk_major else L.lib().ccz_conv3x3_c256_heads_f16
    if live is None:
        L.check(fn(T._stream(), P(x), P(w), P(b), P(r), P(w32), P(b32), P(pol), P(val), boards * 90, flags, None, 0, 1))
        return
    cap = -(-(boards // 16) // n_parts) * 1440
    for part in range(n_parts):
        L.check(fn(T._stream(), P(x), P(w), P(b), P(r), P(w32), P(b32), P(pol), P(val), cap, flags | (2 if part & 1 else 0), P(live), part, n_parts))


@pytest.mark.parametrize("boards,live,n_parts,tail", [(32, None, 1, "pad"), (48, None, 1, "end"), (48, 33, 2, "end"), (32, 17, 1, "pad"), (48, 1, 3, "pad")])
def test_heads_layer_in_arenas(boards, live, n_parts, tail):
    L, N = _L(), _net()
    c = T.case()
    xg, rg, wp, b = T.device_operands()
    xg, rg = xg[:boards * 90], rg[:boards * 90]
    n = boards if live is None else live
    w32, b32 = T.head_operands(np.random.RandomState(17), 4, 19)
    y = E.conv_chain(c["s"][:n], np.abs(c["r"][:n]), True).astype(np.float64)
    s2, worst, share = E.gemm_exact(y.reshape(-1, 256), w32[:24], b32[:24], 2.0 ** -19, "heads on y")
    assert worst < 1.0
    s2 = s2.reshape(n, 90, 24)
    rpos = rg.abs()
    w32d, b32d = h16(w32), f32(b32)
    flags = 1 | L.CONV_G16 | L.CONV_G16_EDGE_TILES
    what = f"G16C heads layer boards {boards} live {live} in {n_parts} tail {tail}"
    wa = T.weight_arena(wp, tail)
    items = {"b": b, "r": N.g16_to_g16c(rpos), "w32": w32d, "b32": b32d, "pol": ((boards, 1536), torch.float16), "val": ((boards, 640), torch.float16),
             "x": N.g16_to_g16c(xg)}
    if live is not None:
        items["n"] = live_count(live)
    a = Arena(items, outputs=("pol", "val"), last="x" if tail == "end" else None)
    launch_heads(True, a["x"], wa["w"], a["b"], a["r"], a["w32"], a["b32"], a["pol"], a["val"], boards, flags, a["n"] if live is not None else None, n_parts)
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    pol, val = poison((boards, 1536), torch.float16), poison((boards, 640), torch.float16)
    launch_heads(False, xg, wp, b, rpos, w32d, b32d, pol, val, boards, flags, live_count(live), n_parts)
    torch.cuda.synchronize()
    assert same_bits(a["pol"], pol) and same_bits(a["val"], val), what + ": differs from the row entry point"
    T.check_head_outputs(a["pol"], a["val"], s2, n, what)


# ------------------------------------------------------------------ a two-block tower with the heads, end to end
@pytest.mark.parametrize("live,n_parts", [(None, 1), (33, 2)])
def test_two_block_tower_with_heads_in_arenas(live, n_parts):
    """stem -> (layer, layer + residual IN PLACE) -> (layer, heads layer + residual), as the evaluator ping-pongs its two buffers, every
    tensor in ONE arena; against the row entry points on plain tensors and the float64 chain."""
    L = _L()
    t = T.tower_case()
    B = BOARDS
    n = B if live is None else live
    x64 = np.zeros((B, 10, 9, 64))
    x64[..., :21] = t["x21"]
    xg = h16(np.ascontiguousarray(E.rows_to_g16(x64))).view(-1, 64)
    wps = [E._pack_w(h16(t["w0"]), 64)] + [E._pack_w(h16(w), 256) for w in t["ws"]]
    bds = [f32(t["b0"])] + [f32(b) for b in t["bs"]]
    w32d, b32d = h16(t["w32"]), f32(t["b32"])
    cap = -(-(B // 16) // n_parts) * 1440

    def run(cm, x, w, b, act, w32, b32, pol, val, n_):
        lib = L.lib()
        stem = (lib.ccz_conv3x3_stem_g16c_f16, lib.ccz_conv3x3_stem_g16c_f16_live) if cm else (lib.ccz_conv3x3_stem_f16, lib.ccz_conv3x3_stem_f16_live)
        if n_ is None:
            L.check(stem[0](T._stream(), P(x), P(w[0]), P(b[0]), P(act[0]), B * 90, 1 | L.CONV_G16))
        else:
            for part in range(n_parts):
                L.check(stem[1](T._stream(), P(x), P(w[0]), P(b[0]), P(act[0]), cap, 1 | L.CONV_G16, P(n_), part, n_parts))
        launch_layer(cm, act[0], w[1], b[1], None, act[1], B, 1 | 2 | form(), n_, n_parts)
        launch_layer(cm, act[1], w[2], b[2], act[0], act[0], B, 1 | form(), n_, n_parts)     # in place over the block's input
        launch_layer(cm, act[0], w[3], b[3], None, act[1], B, 1 | 2 | form(), n_, n_parts)
        launch_heads(cm, act[1], w[4], b[4], act[0], w32, b32, pol, val, B, 1 | L.CONV_G16 | L.CONV_G16_EDGE_TILES, n_, n_parts)

    rows = ((B * 90, 256), torch.float16)
    items = {f"b{k}": bds[k] for k in range(5)}
    items.update({"w32": w32d, "b32": b32d, "a0": rows, "a1": rows, "pol": ((B, 1536), torch.float16), "val": ((B, 640), torch.float16)})
    if live is not None:
        items["n"] = live_count(live)
    items["x"] = xg
    a = Arena(items, outputs=("a0", "a1", "pol", "val"), last="x")
    wa = Arena({f"w{k}": wps[k] for k in range(5)}, last="w4")
    run(True, a["x"], [wa[f"w{k}"] for k in range(5)], [a[f"b{k}"] for k in range(5)], [a["a0"], a["a1"]], a["w32"], a["b32"], a["pol"], a["val"],
        a["n"] if live is not None else None)
    what = f"G16C two-block tower live {live} in {n_parts}"
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    act = [poison(*rows) for _ in range(2)]
    pol, val = poison((B, 1536), torch.float16), poison((B, 640), torch.float16)
    run(False, xg, wps, bds, act, w32d, b32d, pol, val, live_count(live))
    torch.cuda.synchronize()
    assert same_bits(a["pol"], pol) and same_bits(a["val"], val), what + ": differs from the row entry points"
    groups = -(-n // 16)
    for k in range(2):
        assert same_bits(_net().g16c_to_g16(a[f"a{k}"])[:groups * 1440], act[k][:groups * 1440]), what + f": activation buffer {k}"
    T.check_head_outputs(a["pol"], a["val"], t["s2"], n, what)


# ------------------------------------------------------------------ InferenceNet.forward: option on / off, and the fall-back
class Names:
    """stands in for the loaded library: notes which entry points are called"""

    def __init__(self, real):
        self.real, self.names = real, set()

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.names.add(name)
            return fn(*args)
        return call


G16C_ENTRIES = {"ccz_conv3x3_stem_g16c_f16", "ccz_conv3x3_stem_g16c_f16_live", "ccz_conv3x3_c256_g16c_f16", "ccz_conv3x3_c256_g16c_f16_live",
                "ccz_conv3x3_c256_heads_g16c_f16"}


def test_forward_with_the_option_on_and_off(monkeypatch):
    """a two-block net, 72 boards (padded to five groups) with the edge tiles forced on: dense and planned, logits and values with the
    chunk-major tower equal those with rows bit for bit; a precondition switched off falls back to the row entry points"""
    import test_gpu_tower_launch_trace as TR
    L = _L()
    from chinesechesszero_amd.net import EvalOptions
    inf = TR.make_net()
    d = EvalOptions(env={})
    base = {f: getattr(d, f) for f in EvalOptions.FIELDS}
    base.update(layout="g16", edge_tiles=True)
    B = 72
    for planned in (False, True):
        leaf, plan = TR.inputs(B, planned, T._dev())
        n = B if plan is None else int(plan[1].item())
        out = {}
        for cm in (True, False):
            inf.set_options(**dict(base, chunk_major=cm))
            rec = Names(L.lib())
            with monkeypatch.context() as m:
                m.setattr(L, "lib", lambda: rec)
                logits, v = inf(leaf, return_logits=True, plan=plan)
            torch.cuda.synchronize()
            out[cm] = (logits[:n].clone(), v[:n].clone())
            assert bool(rec.names & G16C_ENTRIES) == cm, (planned, cm, sorted(rec.names))
            if cm:
                assert {"ccz_conv3x3_c256_heads_g16c_f16"} <= rec.names and not rec.names & {"ccz_conv3x3_c256_f16", "ccz_conv3x3_c256_f16_live", "ccz_conv3x3_c256_heads_f16"}
        assert same_bits(out[True][0], out[False][0]) and same_bits(out[True][1], out[False][1]), f"planned {planned}"
        assert torch.isfinite(out[True][0].float()).all() and float(out[True][0].float().abs().max()) > 0
        if not planned:
            dense = out[False]
    leaf, _ = TR.inputs(B, False, T._dev())
    for off in ({"quad": False}, {"one_launch": False}, {"fused_last": False}, {"edge_tiles": False}, {"fused_heads": False}):
        inf.set_options(**dict(base, **off))
        rec = Names(L.lib())
        with monkeypatch.context() as m:
            m.setattr(L, "lib", lambda: rec)
            logits, v = inf(leaf, return_logits=True)
        torch.cuda.synchronize()
        assert not rec.names & G16C_ENTRIES, (off, sorted(rec.names))
        if "fused_heads" not in off:   # (the torch heads round differently; every tower form gives the same bits)
            assert same_bits(logits, dense[0]) and same_bits(v, dense[1]), off
    inf.set_options(**{f: getattr(d, f) for f in EvalOptions.FIELDS})
