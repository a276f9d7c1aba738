"""GPU: the QUAD middle tiles of the group-of-16 tower convolution (CCZ_CONV_G16_QUAD, csrc/cczero_conv_g16.h g5q_tile): four ranks x
128 output channels instead of two ranks x 256 -- the same MFMAs in the same order on another wave-to-tile map and another staging.
Checked as tests/test_gpu_conv_tile_stream.py checks the two-rank tiles, with its arenas of 0xFF bytes, its operands and its float64
references (computed once, shared through its caches):

  * the outputs with the flag equal, bit for bit, the outputs without it AND the float64 chain of tests/evaluator_f64.py;
  * every arena byte outside the output slices is what it was (input rows and packed weights as the last bytes of their allocations
    in the `end` cases);
  * 16, 32 and 48 boards (one group: the five-tile launch, the flag has no effect; two and three: quad tiles), live counts 1, 16, 17,
    33 and 48 in one to three launch parts, residual on and off, ascending and descending tile order, middle + edge as two launches
    and as one;
  * weights and bias that are non-zero in ONE half of the output channels only: a tile that takes the other half's bias, residual or
    output columns cannot pass (random data in both halves could hide a swap of equal-looking halves);
  * a two-block tower with the heads end to end: quad layers feed the two-rank heads layer."""
import numpy as np
import pytest
import torch

import evaluator_f64 as E
import test_gpu_conv_tile_stream as TS
from test_gpu_conv_tile_stream import Arena, P, host, poison, same_bits

pytestmark = pytest.mark.gpu

BOARDS = TS.BOARDS


def quad_forms():
    L = TS._L()
    base = L.CONV_G16 | L.CONV_G16_EDGE_TILES
    return (("middle + edge launches", base), ("one launch", base | L.CONV_G16_ONE_LAUNCH))


def check_quad_layer(boards, res, live, n_parts, tail, down, operands=None, want=None):
    """One layer with CCZ_CONV_G16_QUAD in arenas, against the same form without the flag on plain tensors and against `want`."""
    L = TS._L()
    c = TS.case()
    xg, rg, wp, b = operands or TS.device_operands()
    xg, rg = xg[:boards * 90], rg[:boards * 90]
    n = boards if live is None else live
    groups = -(-n // 16)
    if want is None:
        want = E.conv_chain(c["s"][:groups * 16], c["r"][:groups * 16] if res else None, True)
    for name, form in quad_forms():
        what = f"quad: boards {boards} res {res} live {live} in {n_parts}, {name}, descending {down}, tail {tail}"
        flags = 1 | form | (2 if down else 0)
        wa = TS.weight_arena(wp, tail)
        items = {"b": b, "r": rg, "y": ((boards * 90, 256), torch.float16), "x": xg}
        if live is not None:
            items["n"] = torch.tensor([live], dtype=torch.int32, device=TS._dev())
        a = Arena(items, outputs=("y",), last="x" if tail == "end" else None)
        TS.launch_layer(a["x"], wa["w"], a["b"], a["r"] if res else None, a["y"], boards, flags | L.CONV_G16_QUAD,
                        a["n"] if live is not None else None, n_parts)
        a.assert_untouched(what)
        wa.assert_untouched(what + " (weights)")
        plain = poison((boards * 90, 256), torch.float16)
        TS.launch_layer(xg, wp, b, rg if res else None, plain, boards, flags,
                        None if live is None else torch.tensor([live], dtype=torch.int32, device=TS._dev()), n_parts)
        torch.cuda.synchronize()
        assert same_bits(a["y"], plain), what + ": differs from the two-rank tiles"
        got = E.rows_from_g16(host(a["y"]), boards)
        E.assert_same(got[:groups * 16], want[:groups * 16], what, TS.NAMES)
        assert np.all(host(a["y"].view(torch.int16))[groups * 1440:] == -1), what + ": rows past the live groups written"


@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("boards", [16, 32, 48])
def test_quad_layer_whole_batch_in_arenas(boards, res, down):
    """48 boards: the input rows end where their allocation ends, the packed weights are the last bytes of theirs"""
    check_quad_layer(boards, res, None, 1, "end" if boards == 48 else "pad", down)


@pytest.mark.parametrize("n_parts", [1, 2, 3])
@pytest.mark.parametrize("live", [1, 16, 17, 33, 48])
def test_quad_layer_live_rows_in_arenas(live, n_parts):
    """48 boards of capacity, the first `live` hold rows, cut into n_parts launch parts (odd parts run descending: launch_layer);
    residual on for an odd number of parts; live 33 and 48 with input rows and weights at the end of their allocations"""
    check_quad_layer(BOARDS, n_parts != 2, live, n_parts, "end" if live in (33, 48) else "pad", False)


@pytest.mark.parametrize("half", [0, 1])
def test_quad_channel_halves_are_not_mixed_up(half):
    """Weights and bias non-zero in output channels 128 half .. 128 half + 127 only: an output channel depends on its own weights and
    bias alone, so the exact sums are those of the full case in the live half and 0 in the dead one, where the output is relu(residual)."""
    c = TS.case()
    xg, rg, _, _ = TS.device_operands()
    dead = slice(128, 256) if half == 0 else slice(0, 128)
    w, b, s = c["w"].copy(), c["b"].copy(), c["s"][:32].copy()
    w[dead], b[dead], s[..., dead] = 0.0, 0.0, 0.0
    operands = (xg, rg, E._pack_w(TS.h16(w), 256), TS.f32(b))
    want = E.conv_chain(s, c["r"][:32], True)
    assert (E.f64(want[..., dead]) == np.maximum(c["r"][:32][..., dead], 0.0)).all() and float((want != 0).mean()) > 0.2
    for down in (False, True):
        check_quad_layer(32, True, None, 1, "pad", down, operands, want)


@pytest.mark.parametrize("live,n_parts", [(None, 1), (33, 2)])
def test_quad_two_block_tower_with_heads_in_arenas(live, n_parts):
    """stem -> (layer, layer + residual) -> (layer, heads layer + residual) as in tests/test_gpu_conv_tile_stream.py, the three tower
    layers on quad tiles (the heads layer ignores the flag: two-rank tiles), on sparse 2^-2 weights: against the same calls without
    the flag on plain tensors, bit for bit, and against the float64 chain."""
    L = TS._L()
    t = TS.tower_case()
    B = BOARDS
    n = B if live is None else live
    x64 = np.zeros((B, 10, 9, 64))
    x64[..., :21] = t["x21"]
    xg = TS.h16(np.ascontiguousarray(E.rows_to_g16(x64))).view(-1, 64)
    wps = [E._pack_w(TS.h16(t["w0"]), 64)] + [E._pack_w(TS.h16(w), 256) for w in t["ws"]]
    bds = [TS.f32(t["b0"])] + [TS.f32(b) for b in t["bs"]]
    w32d, b32d = TS.h16(t["w32"]), TS.f32(t["b32"])
    base = L.CONV_G16 | L.CONV_G16_EDGE_TILES | L.CONV_G16_ONE_LAUNCH
    nl = None if live is None else torch.tensor([live], dtype=torch.int32, device=TS._dev())
    cap = -(-(B // 16) // n_parts) * 1440
    s_ = TS._stream

    def run(x, w, b, act, w32, b32, pol, val, n_, form):
        def conv(xi, k, res, yo):
            if n_ is None:
                if k == 0:
                    L.check(L.lib().ccz_conv3x3_stem_f16(s_(), P(xi), P(w[0]), P(b[0]), P(yo), B * 90, 1 | L.CONV_G16))
                else:
                    L.check(L.lib().ccz_conv3x3_c256_f16(s_(), P(xi), P(w[k]), P(b[k]), P(res), P(yo), B * 90, 1 | form))
                return
            for part in range(n_parts):
                if k == 0:
                    L.check(L.lib().ccz_conv3x3_stem_f16_live(s_(), P(xi), P(w[0]), P(b[0]), P(yo), cap, 1 | L.CONV_G16, P(n_), part, n_parts))
                else:
                    L.check(L.lib().ccz_conv3x3_c256_f16_live(s_(), P(xi), P(w[k]), P(b[k]), P(res), P(yo), cap, 1 | form, P(n_), part, n_parts))
        conv(x, 0, None, act[0])
        conv(act[0], 1, None, act[1])
        conv(act[1], 2, act[0], act[2])
        conv(act[2], 3, None, act[1])
        TS.launch_heads(act[1], w[4], b[4], act[2], w32, b32, pol, val, B, 1 | (form & ~L.CONV_G16_ONE_LAUNCH), n_, n_parts)

    rows = ((B * 90, 256), torch.float16)
    items = {f"b{k}": bds[k] for k in range(5)}
    items.update({"w32": w32d, "b32": b32d, "a0": rows, "a1": rows, "a2": rows, "pol": ((B, 1536), torch.float16), "val": ((B, 640), torch.float16)})
    if live is not None:
        items["n"] = nl
    items["x"] = xg
    a = Arena(items, outputs=("a0", "a1", "a2", "pol", "val"), last="x")
    wa = Arena({f"w{k}": wps[k] for k in range(5)}, last="w4")
    run(a["x"], [wa[f"w{k}"] for k in range(5)], [a[f"b{k}"] for k in range(5)], [a["a0"], a["a1"], a["a2"]], a["w32"], a["b32"], a["pol"], a["val"],
        a["n"] if live is not None else None, base | L.CONV_G16_QUAD)
    what = f"quad two-block tower live {live} in {n_parts}"
    a.assert_untouched(what)
    wa.assert_untouched(what + " (weights)")
    act = [poison(*rows) for _ in range(3)]
    pol, val = poison((B, 1536), torch.float16), poison((B, 640), torch.float16)
    run(xg, wps, bds, act, w32d, b32d, pol, val, nl, base)
    torch.cuda.synchronize()
    assert same_bits(a["pol"], pol) and same_bits(a["val"], val), what + ": heads differ from the two-rank tiles"
    for k in range(3):
        assert same_bits(a[f"a{k}"], act[k]), what + f": activation buffer {k} differs from the two-rank tiles"
    TS.check_head_outputs(a["pol"], a["val"], t["s2"], n, what)
