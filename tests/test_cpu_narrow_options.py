"""CPU: the host side of the evaluator for narrow towers -- the option (``EvalOptions.narrow``, ``CCZ_FUSED_NARROW``), the derived weights
``InferenceNet(narrow=True)`` builds and repacks, ``--fused-narrow`` on the three command lines, the three additive C calls."""
import ctypes as C
import os
import re

import pytest
import torch

from chinesechesszero_amd import _lib
from chinesechesszero_amd.net import EvalOptions, InferenceNet, Net, PolicyValueNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ccz_conv3x3_cn_f16", "ccz_conv3x3_cn_f16_live", "ccz_heads_conv1x1_cn_f16")
NARROW_ONLY = ("stem_w64", "stem_b32", "head_w32", "head_b32", "policy_fc_wp", "policy_fc_b32", "value_fc1_wp", "value_fc1_b32")


def test_the_option_is_off_by_default_and_read_from_the_environment():
    assert "narrow" in EvalOptions.FIELDS
    assert EvalOptions(env={}).narrow is False and "narrow" not in EvalOptions(env={}).non_default()
    assert EvalOptions(env={"CCZ_FUSED_NARROW": "0"}).narrow is False
    on = EvalOptions(env={"CCZ_FUSED_NARROW": "1"})
    assert on.narrow is True and on.non_default() == {"narrow": True}


def _net(channels=128, blocks=1, seed=0):
    torch.manual_seed(seed)
    net = Net(channels, blocks).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return net


@pytest.mark.parametrize("channels", [128, 64])
def test_the_derived_weights_of_a_narrow_net(channels, monkeypatch):
    monkeypatch.delenv("CCZ_FUSED_NARROW", raising=False)
    net = _net(channels)
    inf = InferenceNet(net, narrow=True)
    assert inf.opt.narrow and inf.narrow_width == channels
    assert tuple(inf.stem_w64.shape) == (channels, 3, 3, 64) and inf.stem_w64.dtype == torch.float16 and inf.stem_w64.is_contiguous()
    assert tuple(inf.stem_b32.shape) == (channels,) and inf.stem_b32.dtype == torch.float32
    assert tuple(inf.head_w32.shape) == (32, channels) and tuple(inf.head_b32.shape) == (32,)
    assert tuple(inf.policy_fc_wp.shape) == (2176, 1536) and tuple(inf.value_fc1_wp.shape) == (256, 640)
    assert len(inf.bs32) == 2 and all(b.dtype == torch.float32 and tuple(b.shape) == (channels,) for b in inf.bs32)
    # ... from the folded parameters: zero padding around them, nothing else
    assert torch.equal(inf.stem_w64[..., :21], inf.stem_w.permute(0, 2, 3, 1)) and not inf.stem_w64[..., 21:].any()
    assert torch.equal(inf.head_w32[:24], inf.head_wT.t()) and not inf.head_w32[24:].any() and not inf.head_b32[24:].any()
    assert inf.stem_w64[..., :21].any() and inf.head_w32[:24].any()
    assert torch.equal(inf.policy_fc_wp[:2086, :1530], inf.policy_fc_w) and not inf.policy_fc_wp[2086:].any() and not inf.policy_fc_wp[:, 1530:].any()
    assert torch.equal(inf.value_fc1_wp[:, :630], inf.value_fc1_w) and not inf.value_fc1_wp[:, 630:].any()
    # no group-of-16 forms, no chunk-major layout, never the heads in the last layer
    assert not hasattr(inf, "ws_g16") and not hasattr(inf, "stem_w64_g16")
    assert not inf._g16(4096) and not inf._g16c(4096)
    # off the GPU nothing is batch-invariant, and the CPU path is the torch one
    assert not inf.batch_invariant
    x = torch.zeros((2, 17, 7, 10, 9), dtype=torch.float16)
    assert inf._path(x) == "torch"


def test_history_mode_builds_the_128_channel_stem():
    inf = InferenceNet(_net(64), history=True, narrow=True)
    assert tuple(inf.stem_w128.shape) == (64, 3, 3, 128) and not hasattr(inf, "stem_w64") and not hasattr(inf, "stem_w128_g16")
    assert torch.equal(inf.stem_w128[..., :119], inf.stem_w.permute(0, 2, 3, 1)) and not inf.stem_w128[..., 119:].any()
    assert "stem_w128" in inf.derived_parameter_names()


def test_a_repack_refreshes_the_derived_weights():
    """``replay.broadcast_model(what="inference")`` overwrites the primaries in place and calls ``repack_derived``"""
    a, b = InferenceNet(_net(128, seed=1), narrow=True), InferenceNet(_net(128, seed=2), narrow=True)
    derived = a.derived_parameter_names()
    assert derived == {"stem_w64", "head_w32", "policy_fc_wp", "policy_fc_b32", "value_fc1_wp", "value_fc1_b32"}
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert derived <= set(pa)
    assert not torch.equal(pa["stem_w64"], pb["stem_w64"])
    addr = {n: p.data_ptr() for n, p in pa.items()}
    with torch.no_grad():
        for n, p in pa.items():
            if n not in derived:
                p.copy_(pb[n])
    a.repack_derived()
    for n, p in a.named_parameters():
        assert torch.equal(p, pb[n]), n
        assert p.data_ptr() == addr[n], n


def test_nothing_is_built_with_the_option_off(monkeypatch):
    monkeypatch.delenv("CCZ_FUSED_NARROW", raising=False)
    for kw in ({}, {"narrow": False}):
        inf = InferenceNet(_net(128), **kw)
        assert not inf.opt.narrow and inf.narrow_width == 0 and not inf.batch_invariant
        assert not [n for n in NARROW_ONLY if hasattr(inf, n)]
        assert inf.derived_parameter_names() == set()
        with pytest.raises(ValueError):
            inf.set_options(narrow=True)
    # other widths and precisions: the option changes nothing
    for net, kw in ((_net(32), {}), (_net(128), {"dtype": torch.float32})):
        inf = InferenceNet(net, narrow=True, **kw)
        assert inf.narrow_width == 0 and not [n for n in NARROW_ONLY if hasattr(inf, n)]
    wide = InferenceNet(_net(256), narrow=True)
    assert wide.narrow_width == 0 and hasattr(wide, "ws_g16") and hasattr(wide, "stem_w64_g16") and tuple(wide.head_w32.shape) == (32, 256)
    monkeypatch.setenv("CCZ_FUSED_NARROW", "1")
    assert InferenceNet(_net(128)).narrow_width == 128
    assert InferenceNet(_net(128), narrow=False).narrow_width == 0


def test_the_switch_of_a_live_object():
    inf = InferenceNet(_net(128), narrow=True)
    assert inf._narrow()
    inf.set_options(narrow=False)
    assert not inf._narrow()
    inf.set_options(narrow=True, fused_heads=False)
    assert not inf._narrow()          # stem, tower and heads on the hand-written kernels, or none of them
    inf.set_options(fused_heads=True)
    assert inf._narrow()


def test_tower_schedule_is_the_one_of_the_wide_tower():
    narrow, wide = InferenceNet(_net(128), narrow=True), InferenceNet(_net(256))
    for B in (1, 11, 64, 65, 300, 1024, 4096):
        for planned in (False, True):
            for capturing in (False, True):
                assert narrow.tower_schedule(B, False, planned, capturing) == wide.tower_schedule(B, False, planned, capturing)


def test_policy_value_net_passes_the_option_to_every_copy_it_builds():
    pvn = PolicyValueNet(device="cpu", num_channels=64, resblocks_num=1, fused_narrow=True)
    assert pvn.fused_narrow and pvn.refresh_inference_copy().narrow_width == 64
    pvn.invalidate_inference_copy()           # what train_step and a hot reload do
    assert pvn._infer is None
    assert pvn.batch_invariant is False and pvn._infer.narrow_width == 64      # (rebuilt; on the CPU nothing is batch-invariant)
    assert PolicyValueNet(device="cpu", num_channels=64, resblocks_num=1).refresh_inference_copy().narrow_width == 0


# ------------------------------------------------------------------ command lines
class _Stop(Exception):
    pass


def test_collect_parses_the_flag_and_passes_it_on(tmp_path, monkeypatch):
    from chinesechesszero_amd import collect
    assert collect.parse_args(["--fused-narrow", "--channels", "128", "--blocks", "10"]).fused_narrow is True
    assert collect.parse_args([]).fused_narrow is False
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise _Stop()
    monkeypatch.setattr(collect, "PolicyValueNet", fake)
    for flag in (True, False):
        pipe = collect.CollectPipeline(n_boards=1, data_dir=str(tmp_path / str(flag)), num_channels=128, resblocks_num=1, fused_narrow=flag)
        with pytest.raises(_Stop):
            pipe.load_model()
    # (load_model falls back to a random net when the model file cannot be read: both constructions carry the keyword)
    assert [kw["fused_narrow"] for kw in seen] == [True, True, False, False] and all(kw["num_channels"] == 128 for kw in seen)


def test_arena_parses_the_flag_and_passes_it_on(monkeypatch):
    from chinesechesszero_amd import arena, net
    seen = []

    def fake_load(spec, channels, blocks, device, fused_narrow=False):
        seen.append((spec, channels, fused_narrow))
        if len(seen) == 2:
            raise _Stop()
    monkeypatch.setattr(arena, "_load", fake_load)
    with pytest.raises(_Stop):
        arena.main(["--a", "random:1", "--b", "random:2", "--channels", "64", "--blocks", "2", "--fused-narrow"])
    assert seen == [("random:1", 64, True), ("random:2", 64, True)]
    monkeypatch.undo()
    made = []
    monkeypatch.setattr(net, "PolicyValueNet", lambda **kw: made.append(kw) or kw)
    arena._load("random:3", 64, 2, 0, True)
    arena._load("random:3", 64, 2, 0)
    assert [kw["fused_narrow"] for kw in made] == [True, False]


def test_analyse_parses_the_flag_and_passes_it_on(tmp_path, monkeypatch):
    from chinesechesszero_amd import analyse, net
    f = tmp_path / "positions.txt"
    f.write_text("startpos\n")
    made = []

    def fake(**kw):
        made.append(kw)
        raise _Stop()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(net, "PolicyValueNet", fake)
    for argv, want in (([str(f), "--channels", "128", "--blocks", "3", "--fused-narrow"], True), ([str(f)], False)):
        with pytest.raises(_Stop):
            analyse.main(argv)
        assert made[-1]["fused_narrow"] is want
    assert made[0]["num_channels"] == 128 and made[0]["resblocks_num"] == 3 and made[1]["num_channels"] == 256 and made[1]["resblocks_num"] == 40


def test_the_flag_is_described_once():
    from chinesechesszero_amd import options
    import argparse
    ap = argparse.ArgumentParser()
    options.add_fused_narrow_args(ap)
    assert options.fused_narrow_from_args(ap, ap.parse_args(["--fused-narrow"])) is True
    assert options.fused_narrow_from_args(ap, ap.parse_args([])) is False
    for name in ("collect", "arena", "analyse"):
        src = open(os.path.join(ROOT, "chinesechesszero_amd", name + ".py"), encoding="utf-8").read()
        assert '"--fused-narrow"' not in src and "add_fused_narrow_args(" in src


# ------------------------------------------------------------------ the C side
def test_the_header_declares_the_three_calls_at_abi_9():
    h = open(os.path.join(ROOT, "include", "cczero.h"), encoding="utf-8").read()
    assert re.search(r"#define CCZ_ABI_VERSION 9\b", h)
    for name in CALLS:
        assert re.search(r"\bint " + name + r"\(void \*stream,", h), name
    assert _lib.ABI_VERSION == 9


def test_the_library_binds_and_refuses():
    for name in CALLS:
        assert name in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["ccz_conv3x3_cn_f16"][1]) == 10 and len(_lib.PROTOTYPES["ccz_conv3x3_cn_f16_live"][1]) == 13
    assert len(_lib.PROTOTYPES["ccz_heads_conv1x1_cn_f16"][1]) == 9
    L = _lib.lib()
    assert L.ccz_abi_version() == 9
    p = C.c_void_p(4096)          # never dereferenced: every call below is refused on the host
    for cin, cout in ((256, 128), (64, 32), (128, 256), (0, 64)):
        assert L.ccz_conv3x3_cn_f16(None, p, p, p, None, C.c_void_p(8192), 90, 1, cin, cout) != 0
        assert b"unsupported" in L.ccz_last_error()
    assert L.ccz_conv3x3_cn_f16_live(None, p, p, p, None, C.c_void_p(8192), 720, 1, 128, 128, None, 0, 1) != 0
    assert L.ccz_conv3x3_cn_f16_live(None, p, p, p, None, C.c_void_p(8192), 720, 1, 128, 128, p, 2, 2) != 0
    assert L.ccz_conv3x3_cn_f16(None, C.c_void_p(4098), p, p, None, C.c_void_p(8192), 90, 1, 128, 128) != 0
    assert b"aligned" in L.ccz_last_error()
    assert L.ccz_conv3x3_cn_f16(None, p, p, p, None, p, 90, 1, 128, 128) != 0          # y = x
    assert L.ccz_heads_conv1x1_cn_f16(None, p, p, p, p, p, 1, 256, None) != 0
    with pytest.raises(_lib.CczError):
        _lib.check(L.ccz_heads_conv1x1_cn_f16(None, p, p, p, p, p, 1, 48, None))
