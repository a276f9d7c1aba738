"""GPU: the quad tile's two-step weight ring (csrc/cczero_conv_g16.h g5_step, kG5QPair): six slots, four ahead, ONE workgroup barrier
per two half-steps. The two-rank tile keeps a ring of five and a barrier per half-step, and it is the yardstick here: the quad
one-launch form -- chunk-major (k_conv3x3_g16c_one_quad, what the evaluator runs) and on rows (k_conv3x3_g16_one_quad) -- must
give, byte for byte, what the two-rank one-launch form (k_conv3x3_g16_one, CCZ_CONV_G16_QUAD off) gives on the same operands.

  * one 256 -> 256 layer, residual on and off: 16 boards (one group: the edge pair has one member), 32 (one full edge pair), 48 (an
    odd group count), 272 (17 groups: more tiles than one XCD's slice, an odd tail) and 4096 boards;
  * the planned form: 1, 16, 17, 255 and 3703 live boards in one and three launch parts; the rows past the live groups keep their
    0xFF fill; one case whose capacity reaches past the tensor, the tensor being the last bytes of its allocation;
  * slot reuse, by data: every (chunk, tap) weight half-tile is a ternary pattern times its OWN integer 1 + 9 chunk + tap (1..72), on
    the weights' fixed-point grid. A half-step that reads a ring slot before its half-tile has landed, or after the next one has,
    multiplies by another scale, and a slab read one chunk early or late meets other activations: the sums change. The expected
    fp16 value is unique (tests/evaluator_f64.py, exactness guard), the comparison is equality with the float64 chain;
  * a three-block tower with the heads in its last layer at 32 and 272 boards: policy and value head outputs of the quad path equal
    the two-rank path's.
"""
import functools

import numpy as np
import pytest
import torch

import evaluator_f64 as E
import test_gpu_conv_tile_stream as T

pytestmark = pytest.mark.gpu

Arena, P, h16, f32, host, poison, same_bits = T.Arena, T.P, T.h16, T.f32, T.host, T.poison, T.same_bits


def _L():
    from chinesechesszero_amd import _lib
    return _lib


def _net():
    from chinesechesszero_amd import net
    return net


def two_rank():
    L = _L()
    return L.CONV_G16 | L.CONV_G16_EDGE_TILES | L.CONV_G16_ONE_LAUNCH


def quad():
    return two_rank() | _L().CONV_G16_QUAD


def live_count(live):
    return None if live is None else torch.tensor([live], dtype=torch.int32, device=T._dev())


def launch(chunk_major, x, w, b, r, y, boards, flags, live=None, n_parts=1):
    L = _L()
    dense, planned = ((L.lib().ccz_conv3x3_c256_g16c_f16, L.lib().ccz_conv3x3_c256_g16c_f16_live) if chunk_major
                      else (L.lib().ccz_conv3x3_c256_f16, L.lib().ccz_conv3x3_c256_f16_live))
    if live is None:
        L.check(dense(T._stream(), P(x), P(w), P(b), P(r), P(y), boards * 90, flags))
        return
    cap = -(-(boards // 16) // n_parts) * 1440
    for part in range(n_parts):
        L.check(planned(T._stream(), P(x), P(w), P(b), P(r), P(y), cap, flags ^ (2 if part & 1 else 0), P(live), part, n_parts))


@functools.lru_cache(maxsize=1)
def big():
    """4096 boards of G16 rows (post-ReLU input, signed residual), one weight set, and their chunk-major twins; the smaller cases are
    its first groups (a group's outputs do not depend on the other groups)"""
    N = _net()
    dev = T._dev()
    g = torch.Generator(device=dev).manual_seed(1207)
    x = torch.relu(torch.randn(4096 * 90, 256, generator=g, device=dev) * 0.5).half()
    r = (torch.randn(4096 * 90, 256, generator=g, device=dev) * 0.5).half()
    w = (torch.randn(256, 3, 3, 256, generator=g, device=dev) * 0.03).half()
    b = torch.randn(256, generator=g, device=dev) * 0.1
    return dict(x=x, r=r, xc=N.g16_to_g16c(x.view(256, 1440, 256)).view(-1, 256), rc=N.g16_to_g16c(r.view(256, 1440, 256)).view(-1, 256),
                wp=N.pack_conv_weights_g16(w), b=b)


@functools.lru_cache(maxsize=None)
def two_rank_rows(boards, res, live, n_parts):
    """the yardstick, once per case: the two-rank one-launch form on rows, into 0xFF bytes"""
    o = big()
    y = poison((boards * 90, 256), torch.float16)
    launch(False, o["x"][:boards * 90], o["wp"], o["b"], o["r"][:boards * 90] if res else None, y, boards, 1 | two_rank(), live_count(live), n_parts)
    torch.cuda.synchronize()
    return y


def cm(t, boards):
    return _net().g16_to_g16c(t.view(boards // 16, 1440, 256)).view(-1, 256)


def rows(t, boards):
    return _net().g16c_to_g16(t.view(boards // 16, 1440, 256)).view(-1, 256)


def check_against_two_rank(boards, res, live=None, n_parts=1):
    o = big()
    n = boards if live is None else live
    groups = -(-n // 16)
    want = two_rank_rows(boards, res, live, n_parts)
    assert torch.isfinite(want[:groups * 1440].float()).all() and int((want[:groups * 1440] != 0).sum()) > groups * 1440 * 64
    assert np.all(host(want.view(torch.int16)[groups * 1440:]) == -1)
    for chunk_major in (True, False):
        what = f"boards {boards} res {res} live {live} in {n_parts}, {'G16C' if chunk_major else 'rows'}"
        x, r = (o["xc"], o["rc"]) if chunk_major else (o["x"], o["r"])
        y = poison((boards * 90, 256), torch.float16)
        launch(chunk_major, x[:boards * 90], o["wp"], o["b"], r[:boards * 90] if res else None, y, boards, 1 | quad(), live_count(live), n_parts)
        torch.cuda.synchronize()
        assert np.all(host(y.view(torch.int16)[groups * 1440:]) == -1), what + ": rows past the live groups written"
        got = rows(y, boards) if chunk_major else y
        assert same_bits(got[:groups * 1440], want[:groups * 1440]), what + ": differs from the two-rank form"


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("boards", [16, 32, 48, 272, 4096])
def test_layer_equals_the_two_rank_form(boards, res):
    check_against_two_rank(boards, res)


@pytest.mark.parametrize("n_parts", [1, 3])
@pytest.mark.parametrize("live", [1, 16, 17, 255, 3703])
def test_live_layer_equals_the_two_rank_form(live, n_parts):
    """the capacity is 272 boards (17 groups; three parts: 6 groups each) for the small counts and 4096 for 3703; residual on"""
    check_against_two_rank(4096 if live > 272 else 272, True, live, n_parts)


def test_live_capacity_past_the_tensor():
    """48 boards in two parts: the capacity is two groups per part, the second part's reaches one group past the tensor -- and the input
    rows are the last bytes of their arena. The kernel runs min(live range, capacity) groups: nothing outside the output changes."""
    o = big()
    B, n_parts = 48, 2
    assert -(-(B // 16) // n_parts) * n_parts * 16 > B
    for live in (48, 33):
        want = two_rank_rows(B, True, live, n_parts)
        groups = -(-live // 16)
        a = Arena({"b": o["b"], "r": o["rc"][:B * 90].clone(), "n": live_count(live), "y": ((B * 90, 256), torch.float16), "x": o["xc"][:B * 90].clone()},
                  outputs=("y",), last="x")
        wa = T.weight_arena(o["wp"], "end")
        launch(True, a["x"], wa["w"], a["b"], a["r"], a["y"], B, 1 | quad(), a["n"], n_parts)
        a.assert_untouched(f"live {live}")
        wa.assert_untouched(f"live {live} (weights)")
        assert np.all(host(a["y"].view(torch.int16)[groups * 1440:]) == -1)
        assert same_bits(rows(a["y"], B)[:groups * 1440], want[:groups * 1440])


# ------------------------------------------------------------------ slot reuse, by data: one scale per (chunk, tap) half-tile
SCALED_BOARDS = 48


@functools.lru_cache(maxsize=1)
def scaled_case():
    rs = np.random.RandomState(1212)
    x = E.grid_acts(rs, (SCALED_BOARDS, 10, 9, 256))
    r = E.grid_acts(rs, (SCALED_BOARDS, 10, 9, 256), relu=False)
    tern = rs.randint(-1, 2, size=(256, 3, 3, 256)).astype(np.float64)
    scale = np.empty((3, 3, 256))
    for tap in range(9):
        for chunk in range(8):
            scale[tap // 3, tap % 3, 32 * chunk:32 * chunk + 32] = 1 + 9 * chunk + tap      # 72 distinct integers: exact in fp16 on 2^-10
    assert len(np.unique(scale)) == 72
    w = tern * scale[None] / 2.0 ** E.EB
    b = E.grid_bias(rs, 256)
    E.assert_on_grid(x, E.EA)
    E.assert_on_grid(w, E.EB)
    s, worst, share = E.conv_exact(x, w, b, T.G, "scaled half-tiles")
    print(f"\nscaled half-tiles: guard fill {worst:.4f} of 1, needs rounding {share:.3f}")
    assert worst < 1.0 and share >= 0.5
    return dict(x=x, r=r, w=w, b=b, s=s)


@pytest.mark.parametrize("res", [False, True])
def test_distinct_scale_per_half_tile_against_float64(res):
    """48 boards = 12 quad tiles and two edge pairs; both tile orders; the quad forms against the float64 chain AND the two-rank form"""
    c = scaled_case()
    B = SCALED_BOARDS
    xg = h16(np.ascontiguousarray(E.rows_to_g16(c["x"]))).view(-1, 256)
    rg = h16(np.ascontiguousarray(E.rows_to_g16(c["r"]))).view(-1, 256)
    wp, b = E._pack_w(h16(c["w"]), 256), f32(c["b"])
    want = E.conv_chain(c["s"], c["r"] if res else None, True)
    ref = poison((B * 90, 256), torch.float16)
    launch(False, xg, wp, b, rg if res else None, ref, B, 1 | two_rank())
    torch.cuda.synchronize()
    E.assert_same(E.rows_from_g16(host(ref), B), want, "two-rank form", T.NAMES)
    for chunk_major in (True, False):
        for order in (0, 2):
            what = f"scaled half-tiles res {res} {'G16C' if chunk_major else 'rows'} order {order}"
            y = poison((B * 90, 256), torch.float16)
            launch(chunk_major, cm(xg, B) if chunk_major else xg, wp, b, (cm(rg, B) if chunk_major else rg) if res else None, y, B, 1 | order | quad())
            torch.cuda.synchronize()
            got = rows(y, B) if chunk_major else y
            E.assert_same(E.rows_from_g16(host(got), B), want, what, T.NAMES)
            assert same_bits(got, ref), what + ": differs from the two-rank form"


# ------------------------------------------------------------------ a three-block tower, the heads in its last layer
def launch_heads(chunk_major, x, w, b, r, w32, b32, pol, val, boards):
    L = _L()
    fn = L.lib().ccz_conv3x3_c256_heads_g16c_f16 if chunk_major else L.lib().ccz_conv3x3_c256_heads_f16
    L.check(fn(T._stream(), P(x), P(w), P(b), P(r), P(w32), P(b32), P(pol), P(val), boards * 90, 1 | L.CONV_G16 | L.CONV_G16_EDGE_TILES, None, 0, 1))


@pytest.mark.parametrize("boards", [32, 272])
def test_three_block_tower_with_heads(boards):
    """stem -> three blocks (layer, layer + residual in place), the last layer with the heads in its epilogue, as the evaluator ping-pongs
    its two buffers: the chunk-major quad path against the two-rank path on rows"""
    L, N = _L(), _net()
    dev = T._dev()
    g = torch.Generator(device="cpu").manual_seed(77 + boards)
    x64 = torch.zeros(boards * 90, 64)
    x64[:, :21] = (torch.rand(boards * 90, 21, generator=g) > 0.8).float()
    xg = x64.half().to(dev)
    w0 = torch.zeros(256, 3, 3, 64)
    w0[..., :21] = torch.randn(256, 3, 3, 21, generator=g) * 0.05
    wps = [E._pack_w(w0.half().to(dev), 64)] + [N.pack_conv_weights_g16((torch.randn(256, 3, 3, 256, generator=g) * 0.02).half().to(dev)) for _ in range(6)]
    bs = [(torch.randn(256, generator=g) * 0.1).to(dev) for _ in range(7)]
    w32 = torch.zeros(32, 256)
    w32[:24] = torch.randn(24, 256, generator=g) * 0.05
    b32 = torch.zeros(32)
    b32[:24] = torch.randn(24, generator=g) * 0.1
    w32, b32 = w32.half().to(dev), b32.to(dev)

    def run(chunk_major, flags):
        lib = L.lib()
        act = [poison((boards * 90, 256), torch.float16) for _ in range(2)]
        pol, val = poison((boards, 1536), torch.float16), poison((boards, 640), torch.float16)
        stem = lib.ccz_conv3x3_stem_g16c_f16 if chunk_major else lib.ccz_conv3x3_stem_f16
        L.check(stem(T._stream(), P(xg), P(wps[0]), P(bs[0]), P(act[0]), boards * 90, 1 | L.CONV_G16))
        for blk in range(3):
            launch(chunk_major, act[0], wps[1 + 2 * blk], bs[1 + 2 * blk], None, act[1], boards, 1 | 2 | flags)
            if blk < 2:
                launch(chunk_major, act[1], wps[2 + 2 * blk], bs[2 + 2 * blk], act[0], act[0], boards, 1 | flags)
        launch_heads(chunk_major, act[1], wps[6], bs[6], act[0], w32, b32, pol, val, boards)
        torch.cuda.synchronize()
        return pol, val, act

    pol_q, val_q, act_q = run(True, quad())
    pol_t, val_t, act_t = run(False, two_rank())
    pos = torch.arange(90, device=dev)
    live_pol = (pos[:, None] * 17 + torch.arange(17, device=dev)[None]).reshape(-1)
    live_val = (pos[:, None] * 7 + torch.arange(7, device=dev)[None]).reshape(-1)
    assert torch.isfinite(pol_t[:, live_pol].float()).all() and float(pol_t[:, live_pol].float().abs().max()) > 0
    assert torch.isfinite(val_t[:, live_val].float()).all() and float(val_t[:, live_val].float().abs().max()) > 0
    assert same_bits(pol_q, pol_t) and same_bits(val_q, val_t), "head outputs differ from the two-rank path"
    for k in range(2):
        assert same_bits(rows(act_q[k], boards), act_t[k]), f"activation buffer {k}"
