"""GPU: the replay ring of compact ply records (replay.RecordReplayBuffer: ccz_ring_retire + ccz_sample_records).

The reference is the existing ``engine.expand_records`` on the same records (itself pinned byte for byte to ``ccz_harvest`` by
test_gpu_harvest.py): whatever the ring serves for a ply and a pass must be the dense row ``expand_records`` writes for it.
Row map: a game that starts at record ``f`` of a buffer, ``T`` plies long, puts ply ``t``, pass ``q`` at dense row
``mul * f + q * T + t`` (per game: the T samples, then their T mirror images)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_cases import STARTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_PLIES = 14


def _play_out(B, seed, quirks, mirror, plane_of_type=None):
    """As test_gpu_harvest._play_out: self-play with the stub evaluator until every board has finished a game; games end at
    different plies (captures to bare kings, repetition, the 14-ply cap)."""
    from chinesechesszero_amd.net import uniform_evaluator
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay(uniform_evaluator, B, n_playout=4, seed=seed, max_plies=MAX_PLIES, reference_quirks=quirks, mirror=mirror,
                         plane_of_type=plane_of_type)
    e = sp.engine
    e.set_position(1, STARTS["capture_to_bare"], 1, 3)
    e.set_position(2, STARTS["two_rooks"], 1, 0)
    e.set_position(3, STARTS["rook_knight"], 0, 100)
    for _ in range(16):
        sp.run_move()
    assert sp.engine.game_status()["over"].all()
    return sp


def _records(B=12, seed=21, quirks=False, mirror=True, pot=None):
    sp = _play_out(B, seed, quirks, mirror, pot)
    rec = torch.cat(list(sp.engine.harvest_record_chunks(1 << 16)))
    flags = sp.engine.record_flags()
    sp.engine.check_healthy()
    return rec, flags


def _t_T(rec):
    hdr = rec[:, 96:112].cpu().numpy()
    return hdr[:, 0:2].copy().view(np.uint16).ravel().astype(np.int64), hdr[:, 2:4].copy().view(np.uint16).ravel().astype(np.int64)


def _games(rec):
    """The buffer's games, in order, as views (whole games only)."""
    t, T = _t_T(rec)
    out, p = [], 0
    while p < rec.shape[0]:
        assert t[p] == 0 and p + T[p] <= rec.shape[0] and (t[p:p + T[p]] == np.arange(T[p])).all()
        out.append(rec[p:p + int(T[p])])
        p += int(T[p])
    return out


def _dense_rows_in_draw_order(rec, mul):
    """For a buffer of whole games: the dense row of draw r = 0 .. P*mul - 1 (ply r // mul, pass r % mul)."""
    t, T = _t_T(rec)
    r = np.arange(rec.shape[0] * mul)
    ply, q = r // mul, r % mul
    f = ply - t[ply]
    return torch.from_numpy(mul * f + q * T[ply] + t[ply]).cuda()


def _bad():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _assert_serves(ring, rec_live, flags, pot, tail, head):
    """Drawing every live row once gives exactly the dense rows of ``rec_live`` (the games of the window, in order), bad == 0."""
    from chinesechesszero_amd.engine import expand_records
    mul = ring.mul
    live = (head - tail) * mul
    assert rec_live.shape[0] == head - tail
    bad = _bad()
    S, P, Z = expand_records(rec_live.contiguous(), flags, pot, bad=bad)
    idx = _dense_rows_in_draw_order(rec_live, mul)
    assert sorted(idx.tolist()) == list(range(live)) == list(range(S.shape[0]))      # no row is left out of the comparison
    s, p, z = ring.sample_at(torch.arange(live, device="cuda"), bad=bad)
    assert s.shape == (live, 17, 7, 10, 9) and s.dtype == torch.float16 and p.shape == (live, 2086) and p.dtype == torch.float32
    assert z.shape == (live,) and z.dtype == torch.float32
    assert torch.equal(s, S[idx]) and torch.equal(p, P[idx]) and torch.equal(z, Z[idx])
    assert int(bad.item()) == 0


@pytest.mark.parametrize("quirks,mirror,pot", [(False, True, None), (True, True, None), (False, False, (0, 6, 5, 4, 3, 2, 1, 0))])
def test_every_row_of_the_ring_is_the_dense_row_byte_for_byte(quirks, mirror, pot):
    from chinesechesszero_amd.replay import RecordReplayBuffer
    rec, flags = _records(12, 21, quirks, mirror, pot)
    P = int(rec.shape[0])
    ring = RecordReplayBuffer(P + 37, "cuda", flags, pot, max_game_plies=MAX_PLIES)
    bad = _bad()
    mul = 2 if mirror else 1
    assert ring.append_records(rec, bad=bad) == P * mul and ring.size == ring.total == P * mul
    assert ring.window() == (0, P) and int(bad.item()) == 0
    _assert_serves(ring, rec, flags, pot, 0, P)
    # draws beyond the live rows wrap: u and u + live are the same row
    live = P * mul
    u = torch.tensor([0, 5, live - 1], device="cuda")
    a, b = ring.sample_at(u), ring.sample_at(u + 3 * live)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(ring.bad.item()) == 0


def test_the_window_advances_by_whole_games_when_the_ring_wraps():
    from chinesechesszero_amd.replay import RecordReplayBuffer
    rec_a, flags = _records(12, 21)
    rec_b, _ = _records(12, 4)
    games = _games(rec_a) + _games(rec_b)
    assert len({int(g.shape[0]) for g in games}) >= 3          # games of several lengths
    cap = 200
    ring = RecordReplayBuffer(cap, "cuda", flags, None, max_game_plies=MAX_PLIES)
    starts, lens, stored = [], [], []      # every game appended so far: logical start, plies, records
    head = 0
    nxt = 0
    mid_game = straddled = split = 0
    sizes = [3, 7, 1, 11, 5, 2, 9, 30, 4, 13, 6, 1, 8, 40, 3, 10]      # games per append, uneven; the large ones are more plies than the ring holds
    for n in sizes:
        chunk = [games[(nxt + i) % len(games)] for i in range(n)]
        nxt += n
        for g in chunk:
            starts.append(head)
            lens.append(int(g.shape[0]))
            stored.append(g)
            head += int(g.shape[0])
        buf = torch.cat(chunk)
        split += int(buf.shape[0] > cap)
        assert ring.append_records(buf) == 2 * buf.shape[0]
        tail, h = ring.window()
        lo = max(0, head - cap)
        later = [s for s in starts if s >= lo]
        want_tail = later[0] if later else head          # the earliest game start >= head - cap
        assert h == head and tail == want_tail and head - tail <= cap and (tail in starts or tail == head)
        mid_game += int(lo > 0 and lo not in starts)     # max(tail, head - cap) fell inside a game: the rounding was needed
        live = [k for k, s in enumerate(starts) if s >= tail]
        straddled += int(any(starts[k] % cap + lens[k] > cap for k in live))      # a live game wraps around the physical end
        _assert_serves(ring, torch.cat([stored[k] for k in live]), flags, None, tail, head)
    print(f"appended {head} plies in {len(starts)} games to a ring of {cap}: tail rounded mid-game {mid_game}x, "
          f"a live game across the physical end {straddled}x, appends larger than the ring {split}")
    assert head > 4 * cap and mid_game >= 1 and straddled >= 1 and split >= 1      # the test met the cases it is about
    assert int(ring.bad.item()) == 0 and ring.total == 2 * head and ring.size <= 2 * cap


def test_sampling_is_a_function_of_the_generator_state():
    from chinesechesszero_amd.replay import RecordReplayBuffer
    rec, flags = _records(8, 4)
    ring = RecordReplayBuffer(512, "cuda", flags, None, max_game_plies=MAX_PLIES)
    ring.append_records(rec)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    a = ring.sample(96, generator=g)
    g.manual_seed(5)
    b = ring.sample(96, generator=g)
    g.manual_seed(5)
    draws = torch.randint(0, 2 ** 62, (96,), device="cuda", dtype=torch.int64, generator=g)
    c = ring.sample_at(draws)
    assert all(torch.equal(x, y) and torch.equal(x, w) for x, y, w in zip(a, b, c))
    live = 2 * rec.shape[0]
    assert len(set((draws % live).tolist())) > 48        # the draws spread over the window
    sums = a[1].sum(dim=1)
    assert ((sums > 0.99) & (sums < 1.01)).all() and int(ring.bad.item()) == 0


def test_cut_and_overlong_games_are_never_served():
    from chinesechesszero_amd import _lib
    from chinesechesszero_amd.engine import expand_records
    from chinesechesszero_amd.replay import RecordReplayBuffer
    rec, flags = _records(8, 4)
    games = _games(rec)
    P, T0, Tl = int(rec.shape[0]), int(games[0].shape[0]), int(games[-1].shape[0])
    assert T0 > 1 and Tl > 1
    # a buffer that starts in the middle of a game, appended to an empty ring: the window starts at the next game
    ring = RecordReplayBuffer(512, "cuda", flags, None, max_game_plies=MAX_PLIES)
    ring.append_records(rec[1:])
    assert ring.window() == (T0 - 1, P - 1)
    _assert_serves(ring, rec[T0:], flags, None, T0 - 1, P - 1)
    # a buffer whose last game is cut: its plies count as bad and come out as zeros; every other row is served
    ring = RecordReplayBuffer(512, "cuda", flags, None, max_game_plies=MAX_PLIES)
    ring.append_records(rec[:-1])
    assert ring.window() == (0, P - 1)
    whole = P - Tl
    S, Pi, Z = expand_records(rec[:whole].contiguous(), flags)
    bad = _bad()
    s, p, z = ring.sample_at(torch.arange(2 * (P - 1), device="cuda"), bad=bad)
    idx = _dense_rows_in_draw_order(rec[:whole], 2)
    assert torch.equal(s[:2 * whole], S[idx]) and torch.equal(p[:2 * whole], Pi[idx]) and torch.equal(z[:2 * whole], Z[idx])
    assert int(bad.item()) == 2 * (Tl - 1)
    assert not s[2 * whole:].any() and not p[2 * whole:].any() and not z[2 * whole:].any()
    # a game longer than max_game_plies at the tail is counted and skipped
    t, T = _t_T(rec)
    long_T = int(T.max())
    short = [g for g in games if g.shape[0] < long_T]
    longest = [g for g in games if g.shape[0] == long_T][0]
    assert short
    ring = RecordReplayBuffer(512, "cuda", flags, None, max_game_plies=long_T - 1)
    ring.append_records(torch.cat([longest] + short))
    assert ring.window() == (long_T, long_T + sum(int(g.shape[0]) for g in short)) and int(ring.bad.item()) == 1
    # an empty window serves zeros and counts
    ring = RecordReplayBuffer(512, "cuda", flags, None, max_game_plies=long_T - 1)
    ring.append_records(longest)
    s, p, z = ring.sample_at(torch.arange(4, device="cuda"))
    assert ring.window() == (long_T, long_T) and int(ring.bad.item()) == 1 + 4 and not s.any() and not p.any()
    # arguments
    with pytest.raises(ValueError):
        RecordReplayBuffer(2 * MAX_PLIES - 1, "cuda", flags, None, max_game_plies=MAX_PLIES)
    ring = RecordReplayBuffer(512, "cuda", flags, None, max_game_plies=MAX_PLIES)
    with pytest.raises(ValueError):
        ring.sample(4)                                   # nothing was ever appended
    with pytest.raises(ValueError):
        ring.append_records(rec, flags | _lib.FLAG_NO_MIRROR)
    with pytest.raises(ValueError):
        ring.append_records(rec, flags, (0, 6, 5, 4, 3, 2, 1, 0))
    with pytest.raises(ValueError):
        ring.sample_at(torch.arange(4, device="cuda", dtype=torch.int32))
    assert ring.append_records(rec, flags, (0, 0, 1, 2, 3, 4, 5, 6)) == 2 * P      # the identity map is the ring's own


def test_a_trainer_step_runs_on_a_minibatch_of_the_ring():
    from chinesechesszero_amd.net import PolicyValueNet
    from chinesechesszero_amd.replay import RecordReplayBuffer
    from chinesechesszero_amd.trainer import Trainer
    rec, flags = _records(12, 21)
    ring = RecordReplayBuffer(1024, "cuda", flags, None, max_game_plies=MAX_PLIES)
    ring.append_records(rec)
    s, p, z = ring.sample(256)
    sums = p.sum(dim=1)
    assert ((sums > 0.99) & (sums < 1.01)).all() and (z.abs() <= 1).all()
    trainer = Trainer(PolicyValueNet(device="cuda", num_channels=32, resblocks_num=2), amp_dtype="bf16")
    out = trainer.step(*ring.sample(64), sync=False)
    assert trainer.steps == 1 and all(isinstance(v, torch.Tensor) and bool(torch.isfinite(v).all()) for v in out.values())
    assert set(out) >= {"loss", "policy_loss", "value_loss"} and int(ring.bad.item()) == 0


def _collect_cli(model, data_dir, *extra):
    cmd = [sys.executable, "-m", "chinesechesszero_amd.collect", "--boards", "64", "--playout", "8", "--moves", "34", "--max-plies", str(MAX_PLIES),
           "--blocks", "2", "--channels", "32", "--seed", "3", "--eval-cache-log2", "0", "--model", model, "--data-dir", data_dir, *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def _npy(data_dir):
    return [np.load(os.path.join(data_dir, n)) for n in ("states.npy", "mcts.npy", "winners.npy")]


def test_collect_and_train_as_one_job_from_the_command_line(tmp_path):
    """``python -m chinesechesszero_amd.collect --replay-plies N --train-every K`` on one rank: trainer steps happen, nothing is
    flagged; a ring that is fed but never drawn from leaves the stored data exactly as a run without the two options writes it."""
    from chinesechesszero_amd.net import PolicyValueNet
    torch.manual_seed(7)
    model = str(tmp_path / "init.pkl")
    PolicyValueNet(device="cuda", num_channels=32, resblocks_num=2).save_model(model)
    plain = _collect_cli(model, str(tmp_path / "plain"))
    assert "collect+train" not in plain.stdout
    fed = _collect_cli(model, str(tmp_path / "fed"), "--replay-plies", "4096", "--train-every", "1000000", "--train-batch", "64")
    rep = json.loads([l for l in fed.stdout.splitlines() if l.startswith("collect+train: ")][-1].split(": ", 1)[1])
    assert rep["trainer_steps"] == 0 and rep["error_flags"] == 0 and rep["ring_bad_records"] == 0
    a, b = _npy(str(tmp_path / "plain")), _npy(str(tmp_path / "fed"))
    assert a[0].shape[0] >= 2 * 64 * MAX_PLIES and rep["ring_head"] * 2 == a[0].shape[0] and rep["ring_tail"] == 0
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    trained = _collect_cli(model, str(tmp_path / "trained"), "--replay-plies", "4096", "--train-every", "4", "--train-batch", "64")
    rep = json.loads([l for l in trained.stdout.splitlines() if l.startswith("collect+train: ")][-1].split(": ", 1)[1])
    assert rep["trainer_steps"] >= 1 and rep["error_flags"] == 0 and rep["ring_bad_records"] == 0
    assert all(np.isfinite(rep[k]) for k in ("loss", "policy_loss", "value_loss"))
    assert _npy(str(tmp_path / "trained"))[0].shape[0] > 0


def test_collect_and_train_with_two_ranks_publishes_rank_0s_weights(tmp_path):
    """Two ranks sharing the GPU (gloo rehearsal, as test_collect_cli_two_ranks_one_store): rank 0 keeps the union of BOTH ranks'
    games in its ring and trains on it; every ``--train-every`` moves both ranks drain the exchange and take rank 0's weights."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env["CCZ_MIOPEN_FIND"] = "0"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "chinesechesszero_amd.collect", "--boards", "32", "--playout", "4", "--blocks", "1",
           "--channels", "32", "--max-plies", "5", "--moves", "13", "--model", "no_such_model.pkl", "--data-dir", str(tmp_path / "data"),
           "--backend", "gloo", "--share-gpu", "--replay-plies", "4096", "--train-every", "3", "--train-batch", "64"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("collect+train: ")]
    assert len(lines) == 1                                   # rank 0 alone trains and reports
    rep = json.loads(lines[0].split(": ", 1)[1])
    # 13 moves with a 5-ply cap: every board of both ranks is adjudicated twice -> 2 ranks x 32 boards x 2 games x 5 plies in the ring
    assert rep["ring_head"] == 2 * 32 * 2 * 5 and rep["ring_tail"] == 0 and rep["ring_bad_records"] == 0 and rep["error_flags"] == 0
    assert rep["trainer_steps"] >= 2 and all(np.isfinite(rep[k]) for k in ("loss", "policy_loss", "value_loss"))
    meta = json.load(open(tmp_path / "data" / "meta.json"))
    assert meta["total_count"] == 2 * rep["ring_head"]       # the store and the ring hold the same games
