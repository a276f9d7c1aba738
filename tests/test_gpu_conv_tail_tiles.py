"""CCZ_CONV_G16_ONE_LAUNCH: the middle tiles and the edge-pair tiles of a tower layer in ONE launch (k_conv3x3_g16_one,
csrc/cczero_conv_g16e.h) instead of a middle launch followed by an edge-pair launch. The same tiles compute the same rows, so every
byte must equal the two-launch form (and the five-tiles-per-group form without edge tiles): one layer over live-row counts and
launch-chain cuts, the whole-batch form, and a 40-block tower with the heads in its last layer."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BOARDS = 4096


def _to_g16(t):
    B, Cn = t.shape[0], t.shape[1]
    return t.permute(0, 2, 3, 1).reshape(B // 16, 16, 90, Cn).permute(0, 2, 1, 3).contiguous()


@pytest.fixture(scope="module")
def layer():
    """Group-of-16 input, residual, packed weights and bias of one 256 -> 256 layer at 4096 boards."""
    from chinesechesszero_amd.net import pack_conv_weights_g16
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(707)
    cl = torch.channels_last
    x = torch.relu(torch.randn(BOARDS, 256, 10, 9, generator=g, device=dev) * 0.7).half().contiguous(memory_format=cl)
    r = (torch.randn(BOARDS, 256, 10, 9, generator=g, device=dev) * 0.7).half().contiguous(memory_format=cl)
    w = (torch.randn(256, 256, 3, 3, generator=g, device=dev) * 0.03).half().contiguous(memory_format=cl)
    b = (torch.randn(256, generator=g, device=dev) * 0.2).float()
    wp = pack_conv_weights_g16(w.permute(0, 2, 3, 1).contiguous().view(256, 3, 3, 256)).contiguous()
    return _to_g16(x), _to_g16(r), wp, b


def _run(layer, flags, res, live=None, n_parts=1, boards=BOARDS):
    """One layer over `boards` boards; with `live`, as n_parts live-row launches (device count, the evaluator's cut). Rows no launch
    writes stay NaN."""
    from chinesechesszero_amd import _lib
    L = _lib.lib()
    xg, rg, wp, b = layer
    dev = xg.device
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n = boards // 16
    xg, rg = xg[:n], rg[:n]
    y = torch.full_like(xg, float("nan"))
    rp = C.c_void_p(rg.data_ptr()) if res else None
    args = (C.c_void_p(xg.data_ptr()), C.c_void_p(wp.data_ptr()), C.c_void_p(b.data_ptr()), rp, C.c_void_p(y.data_ptr()))
    if live is None:
        _lib.check(L.ccz_conv3x3_c256_f16(s, *args, boards * 90, flags))
    else:
        n_live = torch.tensor([live], dtype=torch.int32, device=dev)
        cap = -(-n // n_parts) * 1440
        for part in range(n_parts):
            _lib.check(L.ccz_conv3x3_c256_f16_live(s, *args, cap, flags | (2 if part & 1 else 0), C.c_void_p(n_live.data_ptr()), part, n_parts))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("n_parts", [1, 2, 3])
@pytest.mark.parametrize("live", [1, 15, 16, 17, 1000, 3703, 4095, 4096])
def test_one_launch_equals_two_launches_on_live_rows(layer, live, n_parts):
    from chinesechesszero_amd import _lib
    base = 1 | _lib.CONV_G16
    plain = _run(layer, base, True, live, n_parts)                                  # five tiles per group
    two = _run(layer, base | _lib.CONV_G16_EDGE_TILES, True, live, n_parts)          # middle launch + edge-pair launch
    one = _run(layer, base | _lib.CONV_G16_EDGE_TILES | _lib.CONV_G16_ONE_LAUNCH, True, live, n_parts)
    groups = -(-live // 16)
    assert torch.equal(one[:groups], two[:groups]) and torch.equal(one[:groups], plain[:groups])
    assert torch.isnan(one[groups:].float()).all() and torch.isnan(two[groups:].float()).all()
    assert torch.isfinite(one[:groups].float()).all()


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("boards", [32, 48, 1296, 4096])   # 2, 3, 81 (odd: the last edge pair is one group twice), 256 groups
def test_one_launch_equals_two_launches_on_whole_batches(layer, boards, res):
    from chinesechesszero_amd import _lib
    base = 1 | _lib.CONV_G16
    two = _run(layer, base | _lib.CONV_G16_EDGE_TILES, res, boards=boards)
    one = _run(layer, base | _lib.CONV_G16_EDGE_TILES | _lib.CONV_G16_ONE_LAUNCH, res, boards=boards)
    assert torch.isfinite(one.float()).all()
    assert torch.equal(one, two)
    assert torch.equal(one, _run(layer, base, res, boards=boards))


def test_tower_with_heads_one_launch_equals_two_launches():
    """The 40 x 256 evaluator at 4096 boards, heads in the last layer: logits and values are the same bits with one launch or two per
    layer and chain, for 1 / 2 / 3 chains, whole batch and planned rows."""
    from chinesechesszero_amd.net import InferenceNet, Net
    dev = torch.device("cuda", 0)
    torch.manual_seed(77)
    net = Net(256, 40).to(dev).eval()
    inf = InferenceNet(net).to(dev).eval()
    g = torch.Generator().manual_seed(78)
    B = BOARDS
    leaf = torch.zeros(B, 17, 7, 10, 9, dtype=torch.float16)
    leaf.view(B, 119, 90)[:, 49:56] = (torch.rand(B, 7, 90, generator=g) < 0.1).half()
    leaf.view(B, 119, 90)[:, 105:119] = (torch.rand(B, 14, 90, generator=g) < 0.1).half()
    leaf = leaf.to(dev)
    perm = torch.randperm(B, generator=g).to(torch.int32).to(dev)
    for live in (1, 17, 3703, 4096):
        rows = perm[:live].contiguous()
        n_rows = torch.tensor([live], dtype=torch.int32, device=dev)
        want = None
        for chains in (1, 2, 3):
            for one_launch in (False, True):
                inf.set_options(layout="g16", edge_tiles=True, chains=chains, one_launch=one_launch)
                inf._chain_streams = None
                plan = inf(leaf, return_logits=True, plan=(rows, n_rows))
                got = [plan[0][:live].clone(), plan[1][:live].clone()]
                if live == B:
                    full = inf(leaf, return_logits=True)
                    got += [full[0].clone(), full[1].clone()]
                torch.cuda.synchronize()
                if want is None:
                    want = got
                    assert torch.isfinite(got[0].float()).all() and float(got[0].float().abs().max()) > 0
                else:
                    for a, b in zip(want, got):
                        assert torch.equal(a, b), (live, chains, one_launch)
