"""GPU: policy surprise weighting (ccz_set_surprise, ccz_sample_records_weighted) against tests/surprise_model.py.
Exact, no tolerance anywhere: the surprise of every recorded ply (float32 bits), the harvested records byte for byte (bytes 90..91 and
flag 16 included), the counters, the draw every output row of the weighted sampler took and the rows it formed, a snapshot taken with
the option on, and the collector's two uses of the weights.

8 boards (gumbel_model.inputs: seven openings with 30 to 50 legal moves and `pawns`), 16 simulations, the hash evaluator, three moves and
a ply cap of three so that every game ends. Every test but the labelled control fails on the parent commit: it has none of the calls."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import explore_model as em
import gumbel_model as gm
import surprise_model as sm
from gpu_harness import planes_to_squares
from selfplay_model import SelfPlayModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N, MOVES = gm.B, 16, 3
GAME_NO = 2             # the record header's count of games started on a slot: ccz_create starts the first, set_positions the second
EXPAND, SKIP = 0, 3
SURPRISE = dict(alpha=0.5, cap=8.0)
N_FAST, P_FULL = 4, 0.5
SETTINGS = {
    "plain": dict(),
    "explore_pruned": dict(explore=dict(em.FULL)),
    "gumbel": dict(gumbel=dict(n_sims=N, max_considered=8, c_visit=50.0, c_scale=1.0)),
    "playout_cap": dict(cap=(N, N_FAST, P_FULL)),
}


# ---------------------------------------------------------------------------------------------------------------- engine next to model
def _model(setting, surprise=SURPRISE):
    f = gm.hash_evaluator(gm.SALTS)
    ev = lambda b, board: f(b, board.squares(), int(board.turn))
    cfg = dict(SETTINGS[setting])
    if "gumbel" in cfg:
        m = sm.with_surprise(gm.GumbelModel)(gm.boards(), gm.SALTS, gm.SEED, gm.BASE, evaluator=ev, max_plies=MOVES, surprise=surprise, **cfg)
    else:
        m = sm.with_surprise(SelfPlayModel)(gm.boards(), gm.SALTS, gm.SEED, gm.BASE, evaluator=ev, max_plies=MOVES, surprise=surprise, **cfg)
    return m, f


def _engine(setting, surprise=SURPRISE):
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(B, n_playout=N, seed=gm.SEED, board_id_base=gm.BASE, max_plies=MOVES)
    cfg = SETTINGS[setting]
    if "explore" in cfg:
        x = cfg["explore"]
        e.set_root_exploration(eps=x["eps"], alpha=None, forced_k=x["forced_k"], prune_targets=x["prune"])
    if "gumbel" in cfg:
        e.set_gumbel(**cfg["gumbel"])
    if surprise is not None:
        e.set_surprise(**surprise)
    pos = gm.inputs()
    status = e.set_positions(np.stack([s for s, _ in pos]).astype(np.uint8), np.array([t for _, t in pos], np.uint8))
    assert (status == 0).all(), status
    return e


def _search(e, m, f, setting):
    """One move's N lockstep simulations on both sides, both fed ``f(b, squares, turn)``; the playout cap's budgets by the device's lot."""
    if "cap" in SETTINGS[setting]:
        e.draw_budgets(N, N_FAST, P_FULL)
    if m is not None:
        m.begin_move()
    e.select_leaves()
    for i in range(N):
        info = e.leaf_info()
        sq, turn = planes_to_squares(e.leaf_input.float().cpu().numpy())
        want = m.step() if m is not None else None
        P, V = np.zeros((B, 2086), np.float32), np.zeros(B, np.float32)
        for b in range(B):
            if want is not None:
                assert (info["status"][b] == SKIP) == (want[b][0] == SKIP), (setting, i, b)
            if info["status"][b] == EXPAND:
                P[b], V[b] = f(b, sq[b], turn[b])
        e.expand_backup(torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV))
        if i + 1 < N:
            e.select_leaves()


def _same_surprise(e, m, where):
    kl, has = e.ply_surprise()
    plies = e.game_status()["plies"]
    for b in range(B):
        wk, wh = m.ply_surprise(b)
        n = len(wk)
        assert plies[b] == n, (where, b, plies[b], n)
        assert np.array_equal(has[b][:n], wh), (where, b, has[b][:n], wh)
        assert kl[b][:n].tobytes() == wk.tobytes(), (where, b, kl[b][:n], wk)
        assert not kl[b][:n][wh == 0].any(), (where, b)            # a fast ply carries none


def _play(setting, surprise=SURPRISE, after_move=None):
    """MOVES moves of engine and model side by side, then the adjudication at the ply cap. Returns (engine, model, evaluator)."""
    m, f = _model(setting, surprise)
    e = _engine(setting, surprise)
    for mv in range(MOVES):
        _search(e, m, f, setting)
        played = e.finish_move().cpu().numpy()
        m.finish_move()
        for b in range(B):
            if m.last[b] is not None:
                assert played[b] == m.last[b]["move"], (setting, mv, b)
        if after_move is not None:
            after_move(e, m, mv)
    return e, m, f


def _close(e, m, f, setting):
    """One more simulation (every live root needs children) and the finish_move that adjudicates the running games; the records."""
    _search(e, m, f, setting)
    e.finish_move()
    assert e.game_status()["over"].all()
    if m is not None:
        m.finish_move()
        assert all(m.over)
    rec = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
    e.check_healthy()
    return rec


def _same_records(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        r, o = [int(x[0]) for x in np.nonzero(got != want)]
        raise AssertionError(f"record {r} (ply {got[r, 96:98].view(np.uint16)[0]}) differs at byte {o}: {got[r, o]} != {want[r, o]}")


# ---------------------------------------------------------------------------------------------------------------- 1. the surprise of a ply
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_surprise_of_every_ply_is_the_models(setting):
    e, m, f = _play(setting, after_move=lambda e, m, mv: _same_surprise(e, m, (setting, mv)))
    kinds = [h for b in range(B) for _, h in m.kl[b]]
    values = [float(s) for b in range(B) for s, h in m.kl[b] if h]
    assert len(kinds) == B * MOVES and min(values) > 0.0 and len(set(values)) > len(values) // 2      # the search moved off the prior, ply by ply differently
    if setting == "playout_cap":
        assert 0 < sum(kinds) < len(kinds)                           # the lot gave both kinds of ply on these boards
        assert any(0 < sum(h for _, h in m.kl[b]) < MOVES for b in range(B))      # and both kinds inside one game
    else:
        assert all(kinds)
    if setting == "explore_pruned":
        assert m.totals()["visits_pruned"] > 0                       # pi is formed from pruned counts
    st = e.surprise_stats()
    assert st["target_plies"] == sum(kinds) and st["weights_clipped"] == 0
    assert np.float64(st["surprise_sum"]).tobytes() == np.float64(m.surprise_stats()["surprise_sum"]).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2. the records
@pytest.mark.parametrize("setting,cap", [("plain", 8.0), ("playout_cap", 8.0), ("gumbel", 1.0625)])
def test_harvested_records_and_counters_are_the_models(setting, cap):
    cfg = dict(alpha=0.5, cap=cap)
    e, m, f = _play(setting, cfg)
    rec = _close(e, m, f, setting)
    want = m.records(game_no=GAME_NO)
    _same_records(rec, want)
    assert (rec[:, sm.FLAGS] & sm.REC_WEIGHT).all() and len(rec) == B * MOVES
    wq = rec[:, 90:92].copy().view(np.uint16)[:, 0]
    assert wq.max() <= int(cap * 4096) and len(set(wq.tolist())) > 2
    ms = m.surprise_stats()
    st = e.surprise_stats()
    assert (st["target_plies"], st["weights_clipped"]) == (ms["target_plies"], ms["weights_clipped"])
    assert np.float64(st["surprise_sum"]).tobytes() == np.float64(ms["surprise_sum"]).tobytes()
    if cap < 2:
        assert ms["weights_clipped"] > 0 and (wq == int(cap * 4096)).sum() == ms["weights_clipped"]     # a game whose weights clip
    else:
        assert ms["weights_clipped"] == 0
    if setting == "playout_cap":
        fast = (rec[:, sm.FLAGS] & 1) != 0
        assert fast.any() and (wq[fast] == 4096).all()               # a fast ply weighs 1
    from chinesechesszero_amd.replay import record_weights
    assert np.array_equal(record_weights(torch.from_numpy(rec).to(DEV)).cpu().numpy(), sm.weights_of(want))


def test_control_with_the_option_off_the_records_carry_no_weight():
    """(Passes on the parent commit too: it uses no new call.)"""
    m, f = _model("plain", None)
    e = _engine("plain", None)
    for mv in range(MOVES):
        _search(e, m, f, "plain")
        e.finish_move()
        m.finish_move()
    rec = _close(e, m, f, "plain")
    _same_records(rec, m.records(game_no=GAME_NO))
    assert not (rec[:, sm.FLAGS] & 16).any() and not rec[:, 90:92].any()


def test_the_setter_refuses_bad_values_and_clears_older_plies():
    from chinesechesszero_amd._lib import CczError
    e, m, f = _play("plain")
    assert e.ply_surprise()[1][:, :MOVES].all()
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(cap=0.5), dict(cap=16.0), dict(cap=float("nan"))):
        with pytest.raises(CczError, match="ccz_set_surprise"):
            e.set_surprise(**bad)
    assert e.ply_surprise()[1][:, :MOVES].all()                      # a refused call changed nothing
    e.set_surprise(None)
    assert not e.ply_surprise()[1].any()                             # plies recorded before a call carry none
    rec = _close(e, None, f, "plain")
    assert not (rec[:, sm.FLAGS] & 16).any() and not rec[:, 90:92].any()


# ---------------------------------------------------------------------------------------------------------------- 3. the weighted draw
CAP_PLIES, MAX_GAME, TAIL, HEAD = 20, 8, 3, 23
CAP = 4.0


@functools.lru_cache(maxsize=None)
def _ring_bytes():
    """A ring of 20 slots, window [3, 23): a cut game at the tail (logical plies 0..5: 3, 4, 5 lie in the window, its first plies were
    overwritten), a game with weights {0, 0.5, 1, 4, 0} at [6, 11), a game without the flag at [11, 17), a game with weights at [17, 23)
    that wraps around the physical end (slots 17, 18, 19, 0, 1, 2)."""
    games = [(0, sm.hand_game(6, [4.0] * 6, 11)), (6, sm.hand_game(5, [0.0, 0.5, 1.0, 4.0, 0.0], 12)), (11, sm.hand_game(6, None, 13)),
             (17, sm.hand_game(6, [2.0, 0.25, 0.0, 3.5, 1.0, 0.75], 14))]
    ring = np.zeros((CAP_PLIES, 880), np.uint8)
    for first, g in games:                                           # in order: the last game overwrites the cut one's first plies
        for t in range(len(g)):
            ring[(first + t) % CAP_PLIES] = g[t]
    return ring


def _ring(bytes_):
    from chinesechesszero_amd.replay import RecordReplayBuffer
    ring = RecordReplayBuffer(CAP_PLIES, DEV, max_game_plies=MAX_GAME)
    ring.records.copy_(torch.from_numpy(bytes_))
    ring._window.copy_(torch.tensor([TAIL, HEAD], dtype=torch.int64))
    ring.head, ring.size, ring.total = HEAD, 2 * (HEAD - TAIL), 2 * HEAD
    return ring


def _seed_of(gen_seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(gen_seed)
    return int(torch.randint(0, 2 ** 63 - 1, (1,), device=DEV, dtype=torch.int64, generator=g).item())


def _check_batch(ring, bytes_, batch, gen_seed):
    """One weighted batch against the model of the rejection and against sample_at(chosen). Returns (chosen, model fallbacks, model bad)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(gen_seed)
    bad0, fb0 = int(ring.bad.item()), int(ring.fallbacks.item())
    st, pi, z, tg, val, chosen = ring.sample(batch, generator=g, targets=True, values=True, weighted=True, cap=CAP, chosen=True)
    seed = _seed_of(gen_seed)
    want = [sm.weighted_draw(bytes_, CAP_PLIES, TAIL, HEAD, seed, j, int(CAP * 4096)) for j in range(batch)]
    assert chosen.cpu().tolist() == [u for u, _, _ in want]
    other_bad = torch.zeros((1,), dtype=torch.int32, device=DEV)
    ref = ring.sample_at(chosen, bad=other_bad, targets=True, values=True)
    for a, b in zip((st, pi, z, tg, val), ref):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    fell, bad = sum(f for _, f, _ in want), sum(x for _, _, x in want)
    assert int(ring.fallbacks.item()) - fb0 == fell and int(ring.bad.item()) - bad0 == bad == int(other_bad.item())
    assert np.array_equal(ring.records.cpu().numpy(), bytes_)        # the ring's bytes are unchanged
    return chosen.cpu().numpy(), fell, bad


@pytest.mark.parametrize("batch", [1, 64, 300])
def test_the_weighted_draw_is_the_models_rejection(batch):
    bytes_ = _ring_bytes()
    ring = _ring(bytes_)
    chosen, fell, bad = _check_batch(ring, bytes_, batch, 100 + batch)
    assert fell == 0 and bad == 0
    w = sm.weights_of(bytes_)
    drawn = set()
    for u in chosen:
        ok, p, q, wq = sm.locate(bytes_, CAP_PLIES, TAIL, HEAD, int(u), 2)
        assert ok and p >= 6 and w[p % CAP_PLIES] > 0                # never a ply of the cut game, never a weight-0 ply
        drawn.add((p, q))
    if batch == 300:
        plies = {p for p, _ in drawn}
        assert plies == {p for p in range(6, HEAD) if w[p % CAP_PLIES] > 0}       # every ply with weight is drawn, wrapped slots included
        assert {q for _, q in drawn} == {0, 1}
        counts = np.bincount([sm.locate(bytes_, CAP_PLIES, TAIL, HEAD, int(u), 2)[1] for u in chosen], minlength=HEAD)
        assert counts[9] > counts[7]                                 # weight 4 against weight 0.5 (expected 63 against 8 of 300)


def test_a_ring_of_zero_weights_falls_back_to_the_first_candidate():
    bytes_ = _ring_bytes().copy()
    bytes_[:, 90:92] = 0
    bytes_[:, sm.FLAGS] |= sm.REC_WEIGHT
    ring = _ring(bytes_)
    batch = 40
    chosen, fell, bad = _check_batch(ring, bytes_, batch, 7)
    assert fell == batch == int(ring.fallbacks.item())
    seed = _seed_of(7)
    assert chosen.tolist() == [sm.candidate(seed, j, 0, 0)[0] for j in range(batch)]
    assert 0 < bad < batch                                           # 3 of the window's 20 plies belong to the cut game: zeros, counted
    # the uniform path and the arguments it refuses
    with pytest.raises(ValueError):
        ring.sample(4, chosen=True)
    with pytest.raises(ValueError):
        ring.sample(4, weighted=True, cap=16.0)
    assert len(ring.sample(4)) == 3 and int(ring.fallbacks.item()) == batch


# ---------------------------------------------------------------------------------------------------------------- 4. the snapshot
def test_a_snapshot_with_the_option_on_resumes_bit_for_bit():
    from chinesechesszero_amd import snapshot
    from chinesechesszero_amd._lib import CczError
    setting = "playout_cap"
    e, m, f = _play(setting)                                         # MOVES - 1 would do; the games are in progress until the adjudication
    blob = e.save_state()
    info = snapshot.snapshot_info(blob)
    assert info["sections"] & snapshot.SNAP_SURPRISE and info["surprise"] == {"enabled": 1, "alpha": 0.5, "cap": 8.0}
    assert np.array_equal(info["section_sizes"], snapshot.section_bytes(info["n_nodes"], info["ply"], info["pi_used"], info["sections"]))
    kl, has = e.ply_surprise()
    for b in range(B):
        skl, shas, counters = snapshot.surprise_rows(blob, info, b)
        assert skl.tobytes() == kl[b][:MOVES].tobytes() and np.array_equal(shas, has[b][:MOVES])
        assert int(counters["target_plies"]) == int(has[b][:MOVES].sum())
    want = _close(e, m, f, setting)
    for other, name in ((None, "surprise.enabled"), (dict(alpha=0.25, cap=8.0), "surprise.alpha"), (dict(alpha=0.5, cap=4.0), "surprise.cap")):
        with pytest.raises(CczError, match=name):
            _engine(setting, other).load_state(blob)
    e2 = _engine(setting)
    e2.load_state(blob)
    before = _replay_model(setting)                                  # (the model as it stood when the snapshot was taken)
    _same_surprise(e2, before, "loaded")
    assert e2.surprise_stats() == before.surprise_stats()
    got = _close(e2, None, f, setting)
    _same_records(got, want)
    # with the option off the blob has no such section and the header bytes are zero
    off = snapshot.snapshot_info(_engine("plain", None).save_state())
    assert not off["sections"] & snapshot.SNAP_SURPRISE and off["surprise"] == {"enabled": 0, "alpha": 0.0, "cap": 0.0}


def _replay_model(setting):
    """The model after MOVES moves (what the snapshot holds)."""
    m, _ = _model(setting)
    for mv in range(MOVES):
        m.begin_move()
        for i in range(N):
            m.step()
        m.finish_move()
    return m


# ---------------------------------------------------------------------------------------------------------------- 5. the collector
def _pipeline(tmp_path, **kw):
    from chinesechesszero_amd.collect import CollectPipeline
    os.environ.setdefault("CCZ_MIOPEN_FIND", "0")
    torch.manual_seed(20250)                                         # the random-init net
    pipe = CollectPipeline(init_model=str(tmp_path / "no_such_model.pkl"), n_boards=B, n_playout=N, data_dir=str(tmp_path / "data"), seed=5,
                           num_channels=32, resblocks_num=2, max_plies=4, eval_cache_log2=0, surprise=dict(SURPRISE), **kw)
    pipe.load_model()
    return pipe


def test_the_collector_trains_on_weighted_draws(tmp_path):
    pipe = _pipeline(tmp_path, replay_plies=64, train_every=1, train_batch=16)
    pipe.run(max_calls=12, finalize=False)
    rep = pipe.training_report()
    json.dumps(rep)
    assert rep["trainer_steps"] >= 2 and rep["error_flags"] == 0 and rep["ring_bad_records"] == 0
    assert 0 <= rep["ring_fallbacks"] <= 1                           # weights of mean 1 under a cap of 8: (7 / 8)^256 = 1.4e-15 per row
    assert pipe.ring.head > 0 and (pipe.ring.records[:min(pipe.ring.head, 64), sm.FLAGS] & sm.REC_WEIGHT).all()
    st = pipe.selfplay.engine.surprise_stats()
    assert st["target_plies"] > 0 and st["surprise_sum"] > 0.0
    assert pipe._signature()["option surprise"] == SURPRISE
    pipe.sink.close()


def test_without_a_ring_the_sink_writes_the_weights_in_row_order(tmp_path):
    from chinesechesszero_amd.replay import record_weights
    pipe = _pipeline(tmp_path)
    pipe.run(max_calls=12, finalize=False)
    shards = sorted(p for p, _, _, _ in pipe.sink._rshards)
    assert shards
    rec = np.concatenate([np.load(p) for p in shards])
    total = pipe.sink.finalize()
    w = np.load(os.path.join(pipe.sink.out_dir, "sample_weights.npy"))
    assert w.dtype == np.float32 and w.shape == (total,) and total == 2 * len(rec)
    want, at = [], 0
    rw = record_weights(torch.from_numpy(rec)).numpy()
    while at < len(rec):                                             # per game: its T samples, then their T mirror images
        T = int(rec[at, 98:100].copy().view(np.uint16)[0])
        want += [rw[at:at + T], rw[at:at + T]]
        at += T
    assert np.array_equal(w, np.concatenate(want)) and len(set(w.tolist())) > 2
    assert np.load(os.path.join(pipe.sink.out_dir, "winners.npy")).shape == (total,)
    pipe.sink.close()
