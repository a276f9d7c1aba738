"""CPU: the host side of the recorded root values -- TupleSink's ``root_values.npy`` (written only once a row carried a value,
merged across shards like ``policy_targets.npy``), the z / q blend of ``Trainer.step`` and the collector's ``--resign-*`` flags."""
import copy
import os

import numpy as np
import pytest
import torch

NAN = float("nan")


def _rows(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.rand(n, 17, 7, 10, 9) < 0.1).astype(np.float16), np.full((n, 2086), 1.0 / 2086), rs.choice([-1.0, 0.0, 1.0], n).astype(np.float32)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_the_sink_writes_root_values_only_once_a_row_carried_one(tmp_path):
    from chinesechesszero_amd.collect import TupleSink
    d = str(tmp_path)
    s = TupleSink(d)
    s.append(*_rows(5, 1))
    s.append(*_rows(3, 2), values=np.full(3, NAN, np.float32))           # values, none of them known: nothing to keep
    assert s.finalize() == 8
    before = {n: open(os.path.join(d, n), "rb").read() for n in ("states.npy", "mcts.npy", "winners.npy")}
    assert sorted(os.listdir(d)) == sorted([".collector.lock", "collect_state.json", "meta.json", "mcts.npy", "states.npy", "winners.npy"])
    # rows with values arrive: the file appears, row-aligned, NaN for the rows stored before and for the shard without values
    v = np.array([-0.95, NAN, 0.25, 0.0], np.float32)
    s.append(*_rows(4, 3), values=v)
    s.append(*_rows(2, 4))
    assert s.finalize() == 14
    got = np.load(os.path.join(d, "root_values.npy"))
    assert got.dtype == np.float32 and _same(got, np.concatenate([np.full(8, NAN), v, np.full(2, NAN)]))
    assert not os.path.exists(os.path.join(d, "policy_targets.npy"))
    for n, raw in before.items():                                        # the first 8 rows of the other files are what they were
        a, b = np.load(os.path.join(d, n)), np.load(__import__("io").BytesIO(raw))
        assert np.array_equal(a[:8], b)
    # a later merge without values keeps the file at the new length; values and target bytes live side by side
    s.append(*_rows(3, 5), targets=np.array([1, 0, 1], np.uint8), values=np.array([0.5, -0.5, NAN], np.float32))
    assert s.finalize() == 17
    got = np.load(os.path.join(d, "root_values.npy"))
    assert _same(got, np.concatenate([np.full(8, NAN), v, np.full(2, NAN), [0.5, -0.5, NAN]]))
    assert np.array_equal(np.load(os.path.join(d, "policy_targets.npy")), np.array([1] * 14 + [1, 0, 1], np.uint8))
    assert not [n for n in os.listdir(d) if n.startswith(".shard_")]
    with pytest.raises(ValueError, match="root values"):
        s.append(*_rows(3, 6), values=np.zeros(2, np.float32))
    s.close()
    # a second sink on the directory merges on top of the file
    s2 = TupleSink(d)
    s2.append(*_rows(1, 7))
    assert s2.finalize() == 18 and np.isnan(np.load(os.path.join(d, "root_values.npy"))[-1])
    s2.close()


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


def _step(pvn, states, pi, z, **kw):
    """One Trainer.step on a private copy of the net: (losses, updated weights, the value head's output BEFORE the update)."""
    from chinesechesszero_amd.trainer import Trainer
    pvn = copy.deepcopy(pvn)
    pvn.policy_value_net.train()
    with torch.no_grad():   # what the step's own forward pass computes: train mode, the same batch statistics
        _, value = copy.deepcopy(pvn.policy_value_net)(states.float())
    out = Trainer(pvn).step(states, pi, z, **kw)
    return out, [p.detach().clone() for p in pvn.policy_value_net.parameters()], value.flatten()


def test_q_none_or_weight_zero_is_the_step_as_it_was():
    pvn, states, pi, z = _net_and_batch()
    q = torch.tensor([-0.9, 0.3, NAN, 0.1, NAN, -0.2])
    base, w0, _ = _step(pvn, states, pi, z)
    for kw in ({"q": None}, {"q": None, "q_weight": 0.5}, {"q": q, "q_weight": 0.0}, {"q": q}):
        out, w, _ = _step(pvn, states, pi, z, **kw)
        assert out == base, kw
        assert all(torch.equal(a, b) for a, b in zip(w, w0)), kw


def test_the_value_target_blends_z_and_q_where_q_is_known():
    pvn, states, pi, z = _net_and_batch()
    q = torch.tensor([-0.9, 0.3, NAN, 0.1, NAN, -0.2])
    base, w0, value = _step(pvn, states, pi, z)
    out, w, _ = _step(pvn, states, pi, z, q=q, q_weight=0.5)
    target = torch.tensor([0.5 * 1.0 + 0.5 * -0.9, 0.5 * -1.0 + 0.5 * 0.3, 0.0, 0.5 * 1.0 + 0.5 * 0.1, -1.0, 0.5 * 1.0 + 0.5 * -0.2])
    want = float(torch.mean((value.float() - target) ** 2))
    assert out["value_loss"] == pytest.approx(want, rel=1e-6, abs=1e-7)
    assert out["policy_loss"] == base["policy_loss"]                      # the policy term does not see q
    assert out["value_loss"] != base["value_loss"] and not all(torch.equal(a, b) for a, b in zip(w, w0))
    # lambda = 1: q alone where it is known, z on the NaN rows
    out1, _, _ = _step(pvn, states, pi, z, q=q, q_weight=1.0)
    t1 = torch.where(torch.isnan(q), z, q)
    assert out1["value_loss"] == pytest.approx(float(torch.mean((value.float() - t1) ** 2)), rel=1e-6, abs=1e-7)
    # all NaN: z everywhere, whatever the weight
    outn, wn, _ = _step(pvn, states, pi, z, q=torch.full((6,), NAN), q_weight=0.7)
    assert outn == base and all(torch.equal(a, b) for a, b in zip(wn, w0))
    from chinesechesszero_amd.trainer import Trainer
    with pytest.raises(ValueError, match="q_weight"):
        Trainer(copy.deepcopy(pvn)).step(states, pi, z, q=q, q_weight=1.5)


def test_the_collect_parser_refuses_resign_flags_without_a_threshold(capsys):
    from chinesechesszero_amd import collect
    a = collect.parse_args([])
    assert a.resign is None and a.resign_threshold is None and a.value_q_weight == 0.0
    a = collect.parse_args(["--resign-threshold", "-0.9"])
    assert a.resign == {"threshold": -0.9, "consecutive": 2, "min_ply": 30, "p_playon": 0.1}
    a = collect.parse_args(["--resign-threshold", "-0.8", "--resign-moves", "3", "--resign-min-ply", "0", "--resign-playon", "0.25"])
    assert a.resign == {"threshold": -0.8, "consecutive": 3, "min_ply": 0, "p_playon": 0.25}
    for extra in (["--resign-moves", "3"], ["--resign-min-ply", "10"], ["--resign-playon", "0.2"]):
        with pytest.raises(SystemExit) as exc:
            collect.parse_args(extra)
        assert exc.value.code == 2
        assert "without --resign-threshold" in capsys.readouterr().err


def test_the_pipeline_refuses_settings_that_could_never_take_effect(tmp_path):
    from chinesechesszero_amd.collect import CollectPipeline
    with pytest.raises(ValueError, match="batched path"):
        CollectPipeline(n_boards=1, data_dir=str(tmp_path / "a"), resign=-0.9)
    with pytest.raises(ValueError, match="value_q_weight"):
        CollectPipeline(n_boards=4, data_dir=str(tmp_path / "b"), value_q_weight=0.5)
    with pytest.raises(ValueError, match="value_q_weight"):
        CollectPipeline(n_boards=4, data_dir=str(tmp_path / "c"), value_q_weight=1.5, replay_plies=4096, train_every=1)
