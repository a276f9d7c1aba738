"""GPU: the evaluator of 64- and 128-wide nets on the hand-written kernels for narrow towers (``InferenceNet(narrow=True)``,
``PolicyValueNet(fused_narrow=True)``): a board's logits and value are the same bits in every batch and on the planned boundary, the
result agrees with the MIOpen path the same net takes with the option off, a captured graph replays the eager call, and a search
does not depend on the evaluation cache or on scout slots -- the things that path cannot promise."""
import functools
import logging

import numpy as np
import pytest
import torch

from test_gpu_evaluator_depth import _leaf_batch

pytestmark = pytest.mark.gpu

DP, DV = 1e-2, 3e-2     # the bounds test_gpu_evaluator_depth.py applies between the 256-wide kernels and MIOpen


def _dev():
    return torch.device("cuda", 0)


def _net(channels, blocks, seed=7):
    """random weights, BatchNorm statistics that are not the identity"""
    from chinesechesszero_amd.net import Net
    torch.manual_seed(seed)
    net = Net(channels, blocks).to(_dev()).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return net


@functools.lru_cache(maxsize=None)
def leaves():
    """300 real leaf rows (12 random plies, staggered)"""
    return _leaf_batch(300, 12, seed=21)


def _infer(net, **kw):
    from chinesechesszero_amd.net import InferenceNet
    return InferenceNet(net, **kw).to(_dev()).eval()


@pytest.mark.parametrize("channels,blocks", [(128, 3), (64, 2)])
def test_one_board_is_the_same_bits_in_every_batch(channels, blocks, caplog):
    """alone, among 11 and 64 boards (k_conv3x3_small), among 65 and 300 (k_conv3x3_narrow; 300: one chain of 106 tiles)"""
    net = _net(channels, blocks)
    inf = _infer(net, narrow=True)
    assert inf.batch_invariant and inf.narrow_width == channels
    assert not _infer(net).batch_invariant and not _infer(net, narrow=False).batch_invariant
    x = leaves()
    probe = x[123].clone()
    with caplog.at_level(logging.INFO, logger="chinesechesszero_amd"):
        for B in (1, 11, 64, 65, 300):
            xb = x[:B].clone()
            xb[B // 2] = probe
            assert inf._path(xb) == "nhwc"
            lg, v = inf(xb, return_logits=True)
            if B == 1:
                lg1, v1 = lg[0].clone(), v[0].clone()
                assert torch.isfinite(lg1.float()).all() and abs(float(v1)) < 1 and float(lg1.float().std()) > 0
            else:
                assert torch.equal(lg[B // 2], lg1) and torch.equal(v[B // 2], v1), B
            t = inf.tower_activations(xb)
            assert tuple(t.shape) == (B, channels, 10, 9)
    assert not [r for r in caplog.records if "off the fused" in r.getMessage()]


@pytest.mark.parametrize("channels,blocks", [(128, 3), (64, 2)])
def test_planned_rows_equal_the_unplanned_evaluation(channels, blocks):
    """48 boards: unplanned they run the small form, planned the live tile form. One object, a first planned call on other rows so that
    the persistent buffers hold stale results, then descending live counts with a shuffled ``rows``"""
    inf = _infer(_net(channels, blocks), narrow=True)
    B = 48
    x = leaves()[100:100 + B].contiguous()
    full_lg, full_v = inf(x, return_logits=True)
    full_lg, full_v = full_lg.clone(), full_v.clone()
    other = leaves()[200:200 + B].contiguous()
    g = torch.Generator(device="cpu").manual_seed(5)
    inf(other, return_logits=True, plan=(torch.arange(B, dtype=torch.int32, device=_dev()), torch.tensor([B], dtype=torch.int32, device=_dev())))
    for n_rows in (B, 37, 1):
        rows = torch.randperm(B, generator=g).to(torch.int32).to(_dev())
        lg, v = inf(x, return_logits=True, plan=(rows, torch.tensor([n_rows], dtype=torch.int32, device=_dev())))
        idx = rows[:n_rows].long()
        assert torch.equal(lg[:n_rows], full_lg[idx]) and torch.equal(v[:n_rows], full_v[idx]), n_rows


@pytest.mark.parametrize("channels,blocks", [(128, 3), (64, 2)])
def test_agreement_with_the_miopen_path_of_the_same_net(channels, blocks):
    net = _net(channels, blocks)
    x = leaves()[:200].contiguous()
    p_n, v_n = _infer(net, narrow=True)(x)
    off = _infer(net)
    assert off._path(x) == "torch"
    p_t, v_t = off(x)
    dp, dv = float((p_n - p_t).abs().max()), float((v_n - v_t).abs().max())
    print(f"\nnarrow {blocks} x {channels} against MIOpen, 200 boards: max |dp| {dp:.3e}, max |dv| {dv:.3e}")
    assert torch.isfinite(p_n).all() and torch.isfinite(v_n).all()
    assert dp < DP and dv < DV


@pytest.mark.parametrize("B", [11, 70])
def test_a_captured_graph_replays_the_eager_call(B):
    """inside a stream capture the evaluator is one chain on the capturing stream (no parallel branches)"""
    inf = _infer(_net(128, 3), narrow=True)
    x = leaves()[:B].contiguous()
    lg0, v0 = inf(x, return_logits=True)
    lg0, v0 = lg0.clone(), v0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lg, v = inf(x, return_logits=True)
    lg.zero_()
    v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lg, lg0) and torch.equal(v, v0)


def test_history_mode():
    """all 17 plane groups filled: the 128-channel pack + the 128 -> 128 stem against the torch stem of the same net; one board at batch
    sizes 1, 11 and 70"""
    net = _net(128, 1)
    inf = _infer(net, history=True, narrow=True)
    assert inf.batch_invariant and hasattr(inf, "stem_w128") and not hasattr(inf, "stem_w128_g16")
    rs = np.random.RandomState(3)
    x = torch.from_numpy((rs.random_sample((70, 17, 7, 10, 9)) > 0.8).astype(np.float16)).to(_dev())
    p_n, v_n = inf(x)
    off = _infer(net, history=True)
    assert off._path(x) == "torch"
    p_t, v_t = off(x)
    dp, dv = float((p_n - p_t).abs().max()), float((v_n - v_t).abs().max())
    print(f"\nnarrow history 1 x 128 against the torch stem, 70 boards: max |dp| {dp:.3e}, max |dv| {dv:.3e}")
    assert dp < DP and dv < DV
    # the older planes reach the network
    y = x.clone()
    y[:, :7] = 0
    assert not torch.equal(inf(y)[0], p_n)
    probe = x[33].clone()
    for B in (1, 11, 70):
        xb = x[:B].clone()
        xb[B // 2] = probe
        lg, v = inf(xb, return_logits=True)
        if B == 1:
            lg1, v1 = lg[0].clone(), v[0].clone()
        else:
            assert torch.equal(lg[B // 2], lg1) and torch.equal(v[B // 2], v1), B


def _pvn():
    from chinesechesszero_amd.net import PolicyValueNet
    torch.manual_seed(11)
    pvn = PolicyValueNet(device="cuda:0", num_channels=128, resblocks_num=2, fused_narrow=True)
    for m in pvn.policy_value_net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    pvn.refresh_inference_copy()
    assert pvn.batch_invariant and pvn._infer.opt.narrow
    return pvn


def test_a_search_does_not_depend_on_the_evaluation_cache():
    """32 boards x 16 simulations x 2 moves: with the cache the planned boundary computes the live rows on the live tile form, without
    it whole batches run the small form -- same visit counts, Q and moves"""
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    pvn = _pvn()
    out = {}
    for log2 in (12, 0):
        sp = BatchedSelfPlay(pvn.evaluate_leaves_logits, 32, n_playout=16, seed=5, eval_cache_log2=log2)
        assert sp.planned == (log2 > 0)
        seen = []
        for _ in range(2):
            sp.search()
            rc = sp.engine.root_children()
            seen.append({k: np.array(v).copy() for k, v in rc.items()})
            seen[-1]["moves"] = sp.finish_move().cpu().numpy().copy()
        sp.engine.check_healthy()
        out[log2] = seen
        sp.engine.close()
    for move, (a, b) in enumerate(zip(out[12], out[0])):
        for key in ("k", "acts", "visits", "q", "moves"):
            assert np.array_equal(a[key], b[key]), (move, key)
        assert (a["moves"] >= 0).all() and a["visits"].sum() > 0
    # the option reaches every inference copy PolicyValueNet rebuilds
    pvn.invalidate_inference_copy()
    assert pvn.batch_invariant and pvn._infer.narrow_width == 128


def test_one_game_search_with_and_without_scouts():
    from chinesechesszero_amd.game import Board
    from chinesechesszero_amd.mcts import MCTS_AI
    pvn = _pvn()
    out = {}
    for scouts in (7, 0):
        np.random.seed(3)
        ai = MCTS_AI(pvn.policy_value_fn, c_puct=5, n_playout=24, is_selfplay=True, scouts=scouts)
        assert ai.mcts.scouts == scouts
        board, seen = Board(), []
        for _ in range(3):
            acts, probs = ai.mcts.get_move_probs(board, temp=1.0)
            rc = ai.mcts.root_children()
            mv = int(acts[int(np.argmax(probs))])
            seen.append((mv, np.array(rc["acts"]).copy(), np.array(rc["visits"]).copy()))
            ai.mcts.update_with_move(mv)
            board.push(mv)
        ai.mcts._engine.check_healthy()
        s = ai.mcts._scouted
        assert (s is not None and s.simulations == 3 * 24 and 0 < s.evaluator_calls < 3 * 24) if scouts else s is None
        out[scouts] = seen
    for (m0, a0, n0), (m1, a1, n1) in zip(out[7], out[0]):
        assert m0 == m1 and np.array_equal(a0, a1) and np.array_equal(n0, n1)
