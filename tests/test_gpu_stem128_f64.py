"""GPU: the 128-channel plane pack and stem of the leaf history planes (ccz_pack_planes128_*, ccz_conv3x3_stem128_f16[_live]; DESIGN.md
section 8l) against the float64 chain of tests/evaluator_f64.py, bit for bit: 0/1 planes (on every grid), weights on the 2^-10 grid,
bias on 2^-15, under the exactness guard -- every partial sum of any order is exact in fp32, so the kernels have ONE correct fp16
output. The float64 sums are formed on the device (im2col + a float64 product: exact in any order for the same reason) because the
group-of-16 cases have 59,040 pixels x 119 planes; the guard is asserted on them before any kernel output is read.

  board-major at 65 and 200 boards; group-of-16 at 640 and 656 boards; planned rows (gathering pack + live stem) into buffers that
  hold stale rows, live counts 1, 16 and 17, in both layouts; the board-major call inside 0xFF arenas that must come back unchanged.
  Control: with weights that are zero outside groups 7 / 15 / 16, pack128 + stem128 give the bits of the 64-channel pack + stem.
  Guard: an engine with history on refuses a PolicyValueNet with history off; with both on the search runs and the older planes
  change the logits.

Every test but the guard's first half fails on the parent commit: the entry points do not exist."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import evaluator_f64 as E
from test_gpu_conv_tile_stream import Arena, P, f32, h16, host, poison

pytestmark = pytest.mark.gpu
F16 = torch.float16
NAMES = ("board", "rank", "file", "channel")
G = 2.0 ** -(E.EA + E.EB)


def _dev():
    return torch.device("cuda", 0)


def _L():
    from chinesechesszero_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=_dev())


def _sum64(x, w, b):
    """bias + 3x3 convolution, padding 1, in float64 on the device: x [B,10,9,Cin], w [256,3,3,Cin], b [256] -> [B,10,9,256] (host)"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(_dev()).double().permute(0, 3, 1, 2)
    cols = torch.nn.functional.unfold(xt, 3, padding=1)                                   # [B, Cin * 9, 90], (channel, tap) order
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(_dev()).double().permute(0, 3, 1, 2).reshape(256, -1)
    y = torch.einsum("bkp,ok->bpo", cols, wt) + torch.from_numpy(np.asarray(b, np.float64)).to(_dev())
    return y.reshape(x.shape[0], 10, 9, 256).cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(boards, live_groups_only=False):
    rs = np.random.RandomState(131 * boards + 7)
    leaf = (rs.random_sample((boards, 119, 10, 9)) > 0.8).astype(np.float64)
    w = np.zeros((256, 3, 3, 128))
    w[..., :119] = E.grid_weights(rs, (256, 3, 3, 119), std=0.03)
    if live_groups_only:
        w[..., :49] = 0
        w[..., 56:105] = 0
    b = E.grid_bias(rs, 256)
    E.assert_on_grid(w, E.EB)
    x = leaf.transpose(0, 2, 3, 1)
    worst = E.assert_guard(_sum64(x, np.abs(w[..., :119]), np.abs(b)), G, f"stem128 {boards}")
    s = _sum64(x, w[..., :119], b)
    share = E.needs_rounding(s)
    print(f"\nstem128 {boards}: guard fill {worst:.4f} of 1, needs rounding {share:.3f}")
    assert worst < 1.0 and share >= 0.5
    return dict(leaf=leaf, w=w, b=b, s=s)


def _packed_rows(leaf):
    """what ccz_pack_planes128_f16 must write: [B, 90, 128], the 119 planes then 9 zeros"""
    B = leaf.shape[0]
    out = np.zeros((B, 90, 128), np.float16)
    out[..., :119] = leaf.reshape(B, 119, 90).transpose(0, 2, 1)
    return out


# ---------------------------------------------------------------------------------------------------------------- whole batches
@pytest.mark.parametrize("boards", [65, 200])
def test_board_major(boards):
    L = _L()
    c = case(boards)
    leaf, w, b = h16(c["leaf"]), h16(c["w"]), f32(c["b"])
    n = boards * 90
    x = poison((n, 128), F16)
    L.check(L.lib().ccz_pack_planes128_f16(_stream(), P(leaf), P(x), boards))
    assert host(x).tobytes() == _packed_rows(c["leaf"]).tobytes()
    for relu in (1, 0, 1 | 2):
        y = poison((n, 256), F16)
        L.check(L.lib().ccz_conv3x3_stem128_f16(_stream(), P(x), P(w), P(b), P(y), n, relu))
        E.assert_same(host(y).reshape(boards, 10, 9, 256), E.conv_chain(c["s"], None, bool(relu & 1)), f"stem128 board-major {boards} flags {relu}", NAMES)


@pytest.mark.parametrize("boards", [640, 656])
def test_group_of_16(boards):
    L = _L()
    c = case(boards)
    leaf, b = h16(c["leaf"]), f32(c["b"])
    wp = E._pack_w(h16(c["w"]), 128)                     # (asserts ccz_pack_conv_weights_g16_f16 at cin = 128 against its torch twin)
    n = boards * 90
    x = poison((n, 128), F16)
    L.check(L.lib().ccz_pack_planes128_g16_f16(_stream(), P(leaf), P(x), boards, None, None))
    assert host(x).reshape(boards // 16, 90, 16, 128).tobytes() == np.ascontiguousarray(E.rows_to_g16(_packed_rows(c["leaf"]).reshape(boards, 10, 9, 128))).tobytes()
    for relu in (1, 0):
        y = poison((n, 256), F16)
        L.check(L.lib().ccz_conv3x3_stem128_f16(_stream(), P(x), P(wp), P(b), P(y), n, relu | L.CONV_G16))
        E.assert_same(E.rows_from_g16(host(y), boards), E.conv_chain(c["s"], None, bool(relu)), f"stem128 group-of-16 {boards} relu {relu}", NAMES)


# ---------------------------------------------------------------------------------------------------------------- planned rows
@pytest.mark.parametrize("live", [1, 16, 17])
@pytest.mark.parametrize("g16", [False, True], ids=["board_major", "group_of_16"])
def test_planned_rows_into_stale_buffers(live, g16):
    """The gathering pack writes compact row i from board rows[i] for i < live; the live stem computes those rows. The buffers hold
    another batch's rows (finite, stale) in front of the call; the output starts as 0xFF and keeps it past the rows a live range covers
    (board-major: past the live boards; group-of-16: past the last live group)."""
    L = _L()
    boards = 640 if g16 else 200
    c = case(boards)
    leaf, b = h16(c["leaf"]), f32(c["b"])
    w = E._pack_w(h16(c["w"]), 128) if g16 else h16(c["w"])
    rs = np.random.RandomState(live)
    rows_h = rs.permutation(boards).astype(np.int32)
    rows, nl = torch.from_numpy(rows_h).to(_dev()), i32(live)
    n = boards * 90
    x = torch.from_numpy(_packed_rows(c["leaf"][::-1])).to(_dev()).reshape(n, 128).contiguous()   # another batch's rows: finite, stale
    before = host(x).copy()
    pack = L.lib().ccz_pack_planes128_g16_f16 if g16 else L.lib().ccz_pack_planes128_rows_f16
    L.check(pack(_stream(), P(leaf), P(x), boards, P(rows), P(nl)))
    want_rows = _packed_rows(c["leaf"][rows_h[:live]])
    got = host(x)
    if g16:
        got_b, before_b = E.rows_from_g16(got, boards), E.rows_from_g16(before, boards)
    else:
        got_b, before_b = got.reshape(boards, 10, 9, 128), before.reshape(boards, 10, 9, 128)
    assert got_b[:live].tobytes() == want_rows.reshape(live, 10, 9, 128).tobytes()
    assert got_b[live:].tobytes() == before_b[live:].tobytes(), "rows past the live count were written"
    y = poison((n, 256), F16)
    cap = n if g16 else -(-boards // 8) * 8 * 90
    L.check(L.lib().ccz_conv3x3_stem128_f16_live(_stream(), P(x), P(w), P(b), P(y), cap, 1 | (L.CONV_G16 if g16 else 0), P(nl), 0, 1))
    out = E.rows_from_g16(host(y), boards) if g16 else host(y).reshape(boards, 10, 9, 256)
    E.assert_same(out[:live], E.conv_chain(c["s"][rows_h[:live]], None, True), f"planned stem128 live {live} g16 {g16}", NAMES)
    keep = -(-live // 16) * 16 if g16 else live
    assert np.all(out.view(np.int16)[keep:] == -1), "rows past the live range were written"


# ---------------------------------------------------------------------------------------------------------------- arenas
def test_board_major_inside_arenas():
    L = _L()
    boards = 65
    c = case(boards)
    n = boards * 90
    a = Arena({"leaf": h16(c["leaf"]), "x": ((n, 128), F16), "w": h16(c["w"]), "b": f32(c["b"]), "y": ((n, 256), F16)}, outputs=("x", "y"))
    L.check(L.lib().ccz_pack_planes128_f16(_stream(), P(a["leaf"]), P(a["x"]), boards))
    L.check(L.lib().ccz_conv3x3_stem128_f16(_stream(), P(a["x"]), P(a["w"]), P(a["b"]), P(a["y"]), n, 1))
    E.assert_same(host(a["y"]).reshape(boards, 10, 9, 256), E.conv_chain(c["s"], None, True), "stem128 in arenas", NAMES)
    assert host(a["x"]).tobytes() == _packed_rows(c["leaf"]).tobytes()
    a.assert_untouched("stem128 in arenas")


# ---------------------------------------------------------------------------------------------------------------- control
@pytest.mark.parametrize("boards,g16", [(65, False), (640, True)])
def test_weights_on_the_live_groups_give_the_64_channel_stem(boards, g16):
    L = _L()
    c = case(boards, True)
    live = list(range(49, 56)) + list(range(105, 119))
    w64 = np.zeros((256, 3, 3, 64))
    w64[..., :21] = c["w"][..., live]
    leaf, b = h16(c["leaf"]), f32(c["b"])
    wa, wb = h16(c["w"]), h16(w64)
    if g16:
        wa, wb = E._pack_w(wa, 128), E._pack_w(wb, 64)
    n = boards * 90
    lay = L.CONV_G16 if g16 else 0
    xa, xb = poison((n, 128), F16), poison((n, 64), F16)
    ya, yb = poison((n, 256), F16), poison((n, 256), F16)
    if g16:
        L.check(L.lib().ccz_pack_planes128_g16_f16(_stream(), P(leaf), P(xa), boards, None, None))
        L.check(L.lib().ccz_pack_live_planes_g16_f16(_stream(), P(leaf), P(xb), boards, None, None))
    else:
        L.check(L.lib().ccz_pack_planes128_f16(_stream(), P(leaf), P(xa), boards))
        L.check(L.lib().ccz_pack_live_planes_f16(_stream(), P(leaf), P(xb), boards))
    L.check(L.lib().ccz_conv3x3_stem128_f16(_stream(), P(xa), P(wa), P(b), P(ya), n, 1 | lay))
    L.check(L.lib().ccz_conv3x3_stem_f16(_stream(), P(xb), P(wb), P(b), P(yb), n, 1 | lay))
    assert host(ya).tobytes() == host(yb).tobytes()
    out = E.rows_from_g16(host(ya), boards) if g16 else host(ya).reshape(boards, 10, 9, 256)
    E.assert_same(out, E.conv_chain(c["s"], None, True), f"control {boards}", NAMES)


# ---------------------------------------------------------------------------------------------------------------- the guard, end to end
def test_engine_and_network_must_agree_on_history():
    from chinesechesszero_amd.net import PolicyValueNet
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    torch.manual_seed(3)
    net = PolicyValueNet(device="cuda:0", num_channels=256, resblocks_num=1)
    with pytest.raises(ValueError, match="history planes"):
        BatchedSelfPlay(net.evaluate_leaves_logits, 32, n_playout=8, seed=2, leaf_history=True, eval_cache_log2=12)
    v0 = net.weights_version
    net.set_leaf_history(True)
    assert net.leaf_history and net.weights_version > v0
    sp = BatchedSelfPlay(net.evaluate_leaves_logits, 32, n_playout=8, seed=2, leaf_history=True, eval_cache_log2=12)
    assert sp.planned
    for _ in range(3):
        assert (sp.run_move().cpu().numpy() >= 0).all()
    sp.engine.check_healthy()
    assert hasattr(net._infer, "stem_w128_g16") and net._infer.history and "stem_w128_g16" in net._infer.derived_parameter_names()
    # the older planes reach the network: the row of a mid-game root against the same leaf as the search without history writes it
    e = sp.engine
    e.reset_tree()
    on = e.select_leaves().clone()
    off = torch.zeros_like(on)
    off[:, 7], off[:, 15], off[:, 16] = on[:, 0], on[:, 8], on[:, 16]
    lg_on = net.evaluate_leaves_logits(on)[0].float()
    net.set_leaf_history(False)
    lg_off = net.evaluate_leaves_logits(off)[0].float()
    assert torch.isfinite(lg_on).all() and not torch.equal(lg_on, lg_off)
    with pytest.raises(ValueError, match="history planes"):
        sp.simulate()                                   # the network went back to 21 channels under an engine that writes 119


def test_the_collector_closes_the_loop_with_the_option_on(tmp_path):
    """collect --leaf-history --train-every: search and network read the eight-position input, the trainer trains on the rows of the
    same games, the retrained net searches on; the setting is part of the checkpoint signature."""
    import os
    from chinesechesszero_amd.collect import CollectPipeline, parse_args
    os.environ.setdefault("CCZ_MIOPEN_FIND", "0")
    args = parse_args(["--boards", "32", "--leaf-history"])
    assert args.options["leaf_history"] == {"enabled": True} and parse_args(["--boards", "32"]).options["leaf_history"] is None
    torch.manual_seed(20251)
    pipe = CollectPipeline(init_model=str(tmp_path / "no_such_model.pkl"), n_boards=32, n_playout=6, data_dir=str(tmp_path / "data"), seed=5,
                           num_channels=256, resblocks_num=1, max_plies=4, eval_cache_log2=12, replay_plies=256, train_every=2, train_batch=16,
                           leaf_history=args.options["leaf_history"])
    pipe.load_model()
    pipe.run(max_calls=10, finalize=False)
    rep = pipe.training_report()
    assert rep["trainer_steps"] >= 2 and rep["error_flags"] == 0
    assert pipe.selfplay.engine.get_leaf_history() and pipe.policy_value_net.leaf_history   # (every rebuilt inference copy reads the 119 planes)
    assert pipe._signature()["option leaf_history"] == {"enabled": True}
    assert pipe.selfplay.engine.leaf_input[:, 1:7].any()
    pipe.sink.close()
