"""GPU: a collecting job killed between two checkpoints and resumed leaves exactly the files, the replay ring and the net of a job
that was never interrupted; and the replay ring's own state round trip, with a head that has wrapped.

The job: ``CollectPipeline``, one rank, 16 boards, 16 simulations a move, a random-init net of 2 blocks x 32 channels under a fixed
torch seed, games adjudicated at 3 plies (every fourth move ends all 16 games: 96 rows reach the sink and the ring), a trainer step
every 2 moves on 32 rows of the ring. Run A plays 8 moves with a checkpoint every 3. Run B plays 5 and is dropped without finalize:
its checkpoint is from move 3, the harvest of move 4 is in its data directory. Run C resumes in B's directories and goes on to
move 8: it replays moves 4 and 5 -- the same games, so the sink must drop the 96 rows it already holds -- and its trainer steps (after
moves 4, 6, 8) must draw the minibatches of A's."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BOARDS, PLAYOUT, PLIES = 16, 16, 3


def job(tmp_path, name, resume=False):
    from chinesechesszero_amd.collect import CollectPipeline
    torch.manual_seed(20240)            # the random-init net every run starts from (a resumed one loads the checkpoint's over it)
    p = CollectPipeline(init_model=str(tmp_path / "no_such_model.pkl"), n_boards=BOARDS, n_playout=PLAYOUT, seed=9, max_plies=PLIES,
                        data_dir=str(tmp_path / name / "data"), num_channels=32, resblocks_num=2, replay_plies=64, train_every=2, train_batch=32,
                        checkpoint_dir=str(tmp_path / name / "ck"), checkpoint_every=3, resume=resume)
    p.load_model()
    return p


@pytest.fixture
def deterministic_training():
    """Equal nets after equal steps on equal minibatches need convolution gradients that are summed in a fixed order: MIOpen is asked
    for its deterministic algorithms while the three jobs run (the collector itself never needs that: self-play does not train through
    atomics, and a resumed job is not expected to reproduce rounding noise the uninterrupted one would not reproduce either)."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def test_killed_and_resumed_job_equals_the_uninterrupted_one(tmp_path, deterministic_training):
    from chinesechesszero_amd import checkpoint
    a = job(tmp_path, "a")
    a.collect_batched(8)
    a.sink.finalize()
    assert a.trainer is not None and a.trainer.steps == 3 and a.moves_done == 8
    assert [m for m, _ in checkpoint.complete(str(tmp_path / "a" / "ck"))] == [3, 6]

    b = job(tmp_path, "b")
    b.collect_batched(5)
    assert b.sink.total_rows() == 2 * BOARDS * PLIES and [m for m, _ in checkpoint.complete(str(tmp_path / "b" / "ck"))] == [3]
    b.sink.close()                       # the process is gone: no finalize, its shards stay where they are
    del b

    c = job(tmp_path, "b", resume=True)
    c.collect_batched(5)
    assert c.moves_done == 8 and c.trainer.steps == 3
    assert c.sink.finalize() == a.sink.total_rows() == 2 * 2 * BOARDS * PLIES and c.sink.games == a.sink.games == 2 * BOARDS
    da, dc = str(tmp_path / "a" / "data"), str(tmp_path / "b" / "data")
    names = sorted(n for n in os.listdir(da) if n.endswith(".npy"))
    assert names == sorted(n for n in os.listdir(dc) if n.endswith(".npy")) and {"states.npy", "mcts.npy", "winners.npy"} <= set(names)
    for n in names:                      # byte for byte, side files included: nothing twice, nothing missing, the same order
        with open(os.path.join(da, n), "rb") as f, open(os.path.join(dc, n), "rb") as g:
            assert f.read() == g.read(), n
    assert np.load(os.path.join(dc, "winners.npy")).shape[0] == 2 * 2 * BOARDS * PLIES
    # the ring serves the same rows
    ga, gc = (torch.Generator(device="cuda:0").manual_seed(5) for _ in range(2))
    assert a.ring.window() == c.ring.window()
    for x, y in zip(a.ring.sample(64, generator=ga, targets=True, values=True), c.ring.sample(64, generator=gc, targets=True, values=True)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # the same trainer steps on the same minibatches
    sa, sc = a.policy_value_net.policy_value_net.state_dict(), c.policy_value_net.policy_value_net.state_dict()
    assert sa.keys() == sc.keys()
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert a._sample_gen.get_state().tolist() == c._sample_gen.get_state().tolist()

def test_ring_state_round_trip_with_a_wrapped_head():
    from chinesechesszero_amd.replay import RecordReplayBuffer
    from test_gpu_snapshot import make
    sp = make("cap", n_boards=16, max_plies=3)
    e = sp.engine
    games = []
    for _ in range(12):                  # every fourth move ends the games still running; resignations end some earlier
        sp.run_move()
        games += [c.clone() for c in sp.harvest_record_chunks()]
    assert len(games) >= 3
    cap = 40                             # less than two harvests: the head wraps
    ring = RecordReplayBuffer(cap, e.device, e.record_flags(), e.plane_of_type, max_game_plies=3)
    for g in games[:-1]:
        ring.append_records(g)
    tail, head = ring.window()
    assert head > cap and head % cap != 0 and 0 < head - tail <= cap and tail % cap > head % cap      # wrapped: the window crosses the end
    state = ring.state_dict()
    assert tuple(state["records"].shape) == (head - tail, 880)                                       # the retained window only
    twin = RecordReplayBuffer(cap, e.device, e.record_flags(), e.plane_of_type, max_game_plies=3)
    twin.load_state_dict(state)
    assert twin.window() == (tail, head) and (twin.head, twin.size, twin.total) == (ring.head, ring.size, ring.total)

    def draws_equal():
        ga, gb = (torch.Generator(device="cuda:0").manual_seed(17) for _ in range(2))
        for x, y in zip(ring.sample(64, generator=ga, targets=True, values=True), twin.sample(64, generator=gb, targets=True, values=True)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    draws_equal()
    ring.append_records(games[-1])       # and both go on alike
    twin.append_records(games[-1])
    assert ring.window() == twin.window()
    draws_equal()
    assert int(ring.bad.item()) == int(twin.bad.item()) == 0
    with pytest.raises(ValueError, match="capacity_plies"):
        RecordReplayBuffer(cap + 8, e.device, e.record_flags(), e.plane_of_type, max_game_plies=3).load_state_dict(state)
