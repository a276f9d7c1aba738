"""Record ring against dense ring, the same games in both (replay.RecordReplayBuffer / replay.ReplayBuffer).

  (a) sample(2048): ccz_sample_records forms the 2048 rows (61 MB written, <= 3.2 MB of record bytes read: 8 positions, a header, <= 128 sparse pi entries per row) against the dense
      ring's three index gathers (61 MB read + 61 MB written).
  (b) append of one 4096-board move's finished games (~14 k plies): a 12.5 MB copy + ccz_ring_retire against
      ccz_expand_records writing 847 MB of rows.
  (c) bytes resident per retained ply, and the window a fixed 30 GB holds.

Games come from self-play with the stub evaluator (the rows' content does not change what is timed). Timing: HIP events
around ``inner`` back-to-back calls, after a warm-up of every shape, ``reps`` repetitions with the two rings alternating;
medians and the spread (max - min) of the repetitions are reported. One JSON object on stdout and in ``--out``.

    python profiles/replay_sample_microbench.py --out profiles/r08_replay_sample.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_BYTES = 17 * 7 * 10 * 9 * 2 + 2086 * 4 + 4      # 29,768: fp16 planes + float32 pi + float32 z
REC_BYTES = 880
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12                # B/s: HBM3E spec peak; what a float4 copy reaches on this chip


def play_games(boards, max_plies, seed):
    """Every board plays (at least) one game to its end: compact records of whole games, plies in order."""
    from chinesechesszero_amd.net import uniform_evaluator
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay(uniform_evaluator, boards, n_playout=4, seed=seed, max_plies=max_plies)
    chunks = []
    for _ in range(max_plies + 2):
        sp.run_move()
        if int(sp.engine.game_status()["over"].sum()):
            chunks += list(sp.engine.harvest_record_chunks(1 << 16))
    sp.engine.check_healthy()
    return torch.cat(chunks), sp.engine.record_flags()


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner      # ms per call


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "reps_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=1024)
    ap.add_argument("--max-plies", type=int, default=160)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--append-plies", type=int, default=14000, help="plies of the timed append (one move of 4096 boards ends ~100 games)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replay_sample_microbench: no GPU (a timing taken elsewhere says nothing)")
    from chinesechesszero_amd.engine import game_aligned_chunks
    from chinesechesszero_amd.replay import RecordReplayBuffer, ReplayBuffer
    dev = torch.device("cuda")
    rec, flags = play_games(a.boards, a.max_plies, 1)
    plies = int(rec.shape[0])
    rows = 2 * plies
    dense = ReplayBuffer(rows, dev)
    ring = RecordReplayBuffer(max(plies, 2 * a.max_plies), dev, flags, None, max_game_plies=a.max_plies)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    assert dense.append_records(rec, flags, None, bad=bad) == rows and ring.append_records(rec) == rows
    assert ring.window() == (0, plies) and int(bad.item()) == 0 and int(ring.bad.item()) == 0
    # the two rings serve the same rows: draw r of the ring is ply r // 2, pass r % 2 -- spot-check against the dense ring's layout
    hdr = rec[:, 96:100].contiguous().cpu().view(torch.int16).to(torch.int64) & 0xffff
    t, T = hdr[:, 0], hdr[:, 1]
    u = torch.randint(0, rows, (4096,))
    ply, q = u // 2, u % 2
    idx = (2 * (ply - t[ply]) + q * T[ply] + t[ply]).to(dev)
    s, p, z = ring.sample_at(u.to(dev))
    assert torch.equal(s, dense.states[idx]) and torch.equal(p, dense.pi[idx]) and torch.equal(z, dense.z[idx])

    # (a) sample(batch)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    f_dense, f_ring = (lambda: dense.sample(a.batch, generator=g)), (lambda: ring.sample(a.batch, generator=g))
    for f in (f_dense, f_ring):
        timed(f, 10)
    ms_dense, ms_ring = [], []
    for _ in range(a.reps):
        ms_dense.append(timed(f_dense, a.inner))
        ms_ring.append(timed(f_ring, a.inner))
    sd, sr = summary(ms_dense), summary(ms_ring)
    out_bytes = a.batch * ROW_BYTES
    sample = {"batch": a.batch, "dense": sd, "records": sr, "bytes_written": out_bytes,
              "records_bytes_read_at_most": a.batch * (8 * 96 + 16 + 128 * 6), "dense_bytes_read": out_bytes,
              "records_write_rate_TBps": out_bytes / (sr["median_ms"] * 1e-3) / 1e12,
              "records_frac_of_hbm_spec_8TBps": out_bytes / HBM_SPEC / (sr["median_ms"] * 1e-3),
              "records_frac_of_hbm_copy_6.29TBps": out_bytes / HBM_COPY / (sr["median_ms"] * 1e-3),
              "bar": "records median <= dense median + spread (max - min) of the dense repetitions",
              "pass": sr["median_ms"] <= sd["median_ms"] + sd["spread_ms"]}

    # (b) append of one move's finished games
    part = next(iter(game_aligned_chunks(rec, a.append_plies))).contiguous()
    n = int(part.shape[0])
    inner_b = max(1, a.inner // 5)
    f_dense, f_ring = (lambda: dense.append_records(part, flags)), (lambda: ring.append_records(part))
    for f in (f_dense, f_ring):
        timed(f, 3)
    ms_dense, ms_ring = [], []
    for _ in range(a.reps):
        ms_dense.append(timed(f_dense, inner_b))
        ms_ring.append(timed(f_ring, inner_b))
    append = {"plies": n, "dense": summary(ms_dense), "records": summary(ms_ring),
              "dense_bytes_written": 2 * n * ROW_BYTES, "records_bytes_copied": n * REC_BYTES}
    assert int(ring.bad.item()) == 0

    # (c) residency
    gb30 = 30e9
    resident = {"dense_bytes_per_ply": 2 * ROW_BYTES, "records_bytes_per_ply": REC_BYTES, "ratio": 2 * ROW_BYTES / REC_BYTES,
                "plies_in_30GB_dense": int(gb30 // (2 * ROW_BYTES)), "plies_in_30GB_records": int(gb30 // REC_BYTES),
                "measured_dense_ring_bytes": sum(x.numel() * x.element_size() for x in (dense.states, dense.pi, dense.z)),
                "measured_record_ring_bytes": ring.records.numel() + ring._window.numel() * 8 + 4, "plies_held": plies}
    res = {"what": "replay ring of compact records vs dense ring, same games", "device": torch.cuda.get_device_name(0),
           "games_from": {"boards": a.boards, "max_plies": a.max_plies, "plies": plies, "rows": rows},
           "method": f"HIP events around {a.inner} (sample) / {inner_b} (append) back-to-back calls, warm-up first, {a.reps} repetitions, rings alternating",
           "sample": sample, "append": append, "resident": resident}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
