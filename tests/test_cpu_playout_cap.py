"""CPU: the host side of playout-cap randomisation -- the trainer's policy mask, the collector's options and the sink's
``policy_targets.npy`` (the engine side, per-board simulation budgets, is tests/test_gpu_budgets.py)."""
import copy
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net_and_batch(seed=0, n=6):
    from chinesechesszero_amd.net import PolicyValueNet
    torch.manual_seed(seed)
    pvn = PolicyValueNet(device="cpu", num_channels=8, resblocks_num=1)
    g = torch.Generator().manual_seed(seed + 1)
    states = (torch.rand(n, 119, 10, 9, generator=g) < 0.1).float().reshape(n, 17, 7, 10, 9)
    pi = torch.rand(n, 2086, generator=g) ** 8
    pi = pi / pi.sum(dim=1, keepdim=True)
    z = torch.tensor([1.0, -1.0, 0.0, 1.0, -1.0, 1.0])[:n]
    return pvn, states, pi, z


def _step(pvn, states, pi, z, mask):
    """One Trainer.step on a private copy of the net: (losses, the updated weights, the log-probabilities BEFORE the update)."""
    from chinesechesszero_amd.trainer import Trainer
    pvn = copy.deepcopy(pvn)
    pvn.policy_value_net.train()
    with torch.no_grad():   # what the step's own forward pass computes: train mode, the same batch statistics
        logp, value = copy.deepcopy(pvn.policy_value_net)(states.float())
    tr = Trainer(pvn)
    out = tr.step(states, pi, z) if mask is None else tr.step(states, pi, z, policy_mask=mask)
    return out, [p.detach().clone() for p in pvn.policy_value_net.parameters()], logp, value


def test_a_mask_of_ones_is_the_unmasked_step_bit_for_bit():
    pvn, states, pi, z = _net_and_batch()
    a, wa, _, _ = _step(pvn, states, pi, z, None)
    for ones in (torch.ones(6), torch.ones(6, dtype=torch.uint8)):
        b, wb, _, _ = _step(pvn, states, pi, z, ones)
        assert a == b                                                   # floats of the same bits
        assert len(wa) == len(wb) and all(torch.equal(x, y) for x, y in zip(wa, wb))
    assert any(not torch.equal(x, y) for x, y in zip(wa, pvn.policy_value_net.parameters()))   # (the step did move the weights)


def test_a_mask_keeps_the_fast_rows_out_of_the_policy_term_only():
    pvn, states, pi, z = _net_and_batch(3)
    full, w_full, logp, value = _step(pvn, states, pi, z, None)
    mask = torch.tensor([1, 0, 0, 1, 1, 0], dtype=torch.uint8)
    got, w_got, _, _ = _step(pvn, states, pi, z, mask)
    eps = 0.05
    target = (1 - eps) * pi + eps / 2086
    rows = -(target * logp.float()).sum(dim=1)
    want_policy = float((rows * mask.float()).sum() / 3.0)
    want_value = float(torch.nn.functional.mse_loss(value.flatten().float(), z))
    assert got["policy_loss"] == pytest.approx(want_policy, rel=1e-6)
    assert got["value_loss"] == pytest.approx(want_value, rel=1e-6) and got["value_loss"] == full["value_loss"]
    assert got["entropy"] == full["entropy"]                            # the report takes every row
    assert got["loss"] == pytest.approx(want_policy + want_value, rel=1e-6)
    assert got["policy_loss"] != full["policy_loss"] and any(not torch.equal(x, y) for x, y in zip(w_full, w_got))


def test_an_all_zero_mask_leaves_the_value_loss():
    pvn, states, pi, z = _net_and_batch(5)
    full, _, _, _ = _step(pvn, states, pi, z, None)
    got, w, _, _ = _step(pvn, states, pi, z, torch.zeros(6))
    assert np.isfinite(got["loss"]) and got["policy_loss"] == 0.0 and got["loss"] == got["value_loss"] == full["value_loss"]
    assert all(bool(torch.isfinite(p).all()) for p in w)


def test_collector_options_go_together(tmp_path):
    from chinesechesszero_amd.collect import CollectPipeline, build_parser
    p = build_parser()
    d = p.parse_args([])
    assert d.playout_cap_fast == 0 and d.playout_cap_prob is None
    a = p.parse_args(["--playout-cap-fast", "100", "--playout-cap-prob", "0.25", "--boards", "64"])
    assert a.playout_cap_fast == 100 and a.playout_cap_prob == 0.25
    bad = [dict(playout_cap_fast=100), dict(playout_cap_prob=0.25), dict(playout_cap_fast=100, playout_cap_prob=1.5),
           dict(playout_cap_fast=100, playout_cap_prob=-0.1), dict(playout_cap_fast=500, playout_cap_prob=0.25),
           dict(playout_cap_fast=100, playout_cap_prob=0.25, n_boards=1), dict(playout_cap_fast=100, playout_cap_prob=0.25, dense_shards=True),
           dict(playout_cap_fast=100, playout_cap_prob=0.25, gatherer=object())]   # a dense-row gatherer: neither post nor _payload
    for i, kw in enumerate(bad):
        kw.setdefault("n_boards", 64)
        with pytest.raises(ValueError):
            CollectPipeline(n_playout=400, data_dir=str(tmp_path / f"bad{i}"), **kw)
        assert not os.path.exists(tmp_path / f"bad{i}")                 # refused before anything is created
    ok = CollectPipeline(n_boards=64, n_playout=400, playout_cap_fast=100, playout_cap_prob=0.25, data_dir=str(tmp_path / "ok"))
    assert ok.playout_cap == (100, 0.25)
    ok.sink.close()
    off = CollectPipeline(n_boards=64, n_playout=400, data_dir=str(tmp_path / "off"))
    assert off.playout_cap is None
    off.sink.close()


def test_selfplay_refuses_a_bad_playout_cap_before_it_builds_an_engine():
    from chinesechesszero_amd.net import uniform_evaluator
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    for cap in ((0, 0.5), (25, 0.5), (6, 1.5), (6, -0.5), (2.5, 0.5)):
        with pytest.raises(ValueError, match="playout_cap"):
            BatchedSelfPlay(uniform_evaluator, 4, n_playout=24, playout_cap=cap)


def _rows(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.rand(n, 17, 7, 10, 9) < 0.1).astype(np.float16), np.full((n, 2086), 1.0 / 2086), rs.choice([-1.0, 0.0, 1.0], n).astype(np.float32)


def test_the_sink_writes_policy_targets_only_once_a_row_is_flagged(tmp_path):
    from chinesechesszero_amd.collect import TupleSink
    d = str(tmp_path)
    s = TupleSink(d)
    s.append(*_rows(5, 1))
    s.append(*_rows(3, 2), targets=np.ones(3, np.uint8))                # targets, none of them fast: no flag to keep
    assert s.finalize() == 8
    before = {n: open(os.path.join(d, n), "rb").read() for n in ("states.npy", "mcts.npy", "winners.npy")}
    assert sorted(os.listdir(d)) == sorted([".collector.lock", "collect_state.json", "meta.json", "mcts.npy", "states.npy", "winners.npy"])
    # flagged rows arrive: the file appears, row-aligned, the rows stored before count as targets
    t = np.array([1, 0, 0, 1], np.uint8)
    s.append(*_rows(4, 3), targets=torch.from_numpy(t))
    s.append(*_rows(2, 4))
    assert s.finalize() == 14
    got = np.load(os.path.join(d, "policy_targets.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, np.r_[np.ones(8, np.uint8), t, np.ones(2, np.uint8)])
    assert len(np.load(os.path.join(d, "states.npy"), mmap_mode="r")) == 14
    for n, b in before.items():                                         # the other files grew as they always do
        assert np.array_equal(np.load(os.path.join(d, n), mmap_mode="r")[:8], np.load(__import__("io").BytesIO(b)))
    # once there, the file keeps pace with the arrays, flagged shards or not
    s.append(*_rows(3, 5))
    assert s.finalize() == 17
    got = np.load(os.path.join(d, "policy_targets.npy"))
    assert np.array_equal(got, np.r_[np.ones(8, np.uint8), t, np.ones(5, np.uint8)])
    assert not [n for n in os.listdir(d) if n.startswith(".shard_") or n.endswith(".tmp")]
    with pytest.raises(ValueError, match="policy-target"):
        s.append(*_rows(3, 6), targets=np.ones(2, np.uint8))
    s.close()
