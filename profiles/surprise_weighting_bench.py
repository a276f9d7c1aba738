"""Policy surprise weighting: what the weighted draw and the surprise of a ply cost.

  (a) ``RecordReplayBuffer.sample(2048, weighted=True)`` against ``sample(2048)`` on the same ring, in the same process. The ring is filled
      as in profiles/r08_replay_sample.json (profiles/replay_sample_microbench.py: 1024 boards, games of at most 160 plies, the uniform
      evaluator), with the option on so that the records carry weights.
  (b) ``finish_move`` (k_finish_move + the half flip) at 4096 boards with the option off against on, the two alternating on the same engine
      in the pattern off on on off (the boards move in lockstep, so plain alternation would give one kind all of red's moves), each move
      searched with 16 simulations of the uniform evaluator.

Timing: HIP events, a warm-up first, the median of ``--reps`` repetitions (>= 20) and their spread (max - min). ``--finish-only`` runs (b)
alone and, on a tree without ``set_surprise`` (the parent commit), its "off" half alone: the one-word gate is judged by comparing that
figure of the two trees, taken in the same visit. One JSON object on stdout and in ``--out``.

    python profiles/surprise_weighting_bench.py --out profiles/surprise_weighting.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner      # ms per call


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "reps": len(ms)}


def play_games(boards, max_plies, seed):
    """Every board plays (at least) one game to its end with the option on: compact records of whole games, plies in order."""
    from chinesechesszero_amd.net import uniform_evaluator
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay(uniform_evaluator, boards, n_playout=4, seed=seed, max_plies=max_plies, surprise={"alpha": 0.5, "cap": 8.0})
    chunks = []
    for _ in range(max_plies + 2):
        sp.run_move()
        if int(sp.engine.game_status()["over"].sum()):
            chunks += list(sp.engine.harvest_record_chunks(1 << 16))
    sp.engine.check_healthy()
    return torch.cat(chunks), sp.engine.record_flags(), sp.engine.surprise_stats()


def sample_ab(a):
    from chinesechesszero_amd.replay import RecordReplayBuffer, record_weights
    dev = torch.device("cuda")
    rec, flags, stats = play_games(a.boards, a.max_plies, 1)
    plies = int(rec.shape[0])
    ring = RecordReplayBuffer(max(plies, 2 * a.max_plies), dev, flags, None, max_game_plies=a.max_plies)
    ring.append_records(rec)
    assert ring.window() == (0, plies) and int(ring.bad.item()) == 0
    w = record_weights(rec)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    f_uni, f_wtd = (lambda: ring.sample(a.batch, generator=g)), (lambda: ring.sample(a.batch, generator=g, weighted=True, cap=8.0))
    for f in (f_uni, f_wtd):
        timed(f, 10)
    ms_uni, ms_wtd = [], []
    for _ in range(a.reps):
        ms_uni.append(timed(f_uni, a.inner))
        ms_wtd.append(timed(f_wtd, a.inner))
    su, sw = summary(ms_uni), summary(ms_wtd)
    rows = a.reps * a.inner * a.batch + 10 * a.batch
    return {"batch": a.batch, "ring": {"boards": a.boards, "max_plies": a.max_plies, "plies": plies},
            "weights": {"mean": float(w.mean()), "max": float(w.max()), "zero_share": float((w == 0).float().mean()), "engine_stats": stats},
            "uniform": su, "weighted": sw, "ratio_weighted_over_uniform": sw["median_ms"] / su["median_ms"],
            "fallbacks": int(ring.fallbacks.item()), "weighted_rows_drawn": rows, "bad": int(ring.bad.item()),
            "method": f"HIP events around {a.inner} back-to-back calls, warm-up first, {a.reps} repetitions, the two draws alternating"}


def finish_ab(a):
    from chinesechesszero_amd.net import uniform_evaluator
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay(uniform_evaluator, a.finish_boards, n_playout=16, seed=2, max_plies=4 * a.reps + 64)
    e = sp.engine
    has = hasattr(e, "set_surprise")
    kinds = ("off", "on") if has else ("off",)
    ms = {k: [] for k in kinds}
    for i in range(8 + len(kinds) * a.reps):           # 8 warm-up moves, then the kinds alternate
        kind = kinds[(i % 4 in (1, 2)) if has else 0]     # off on on off: each kind times as many red moves as black ones
        if has:
            e.set_surprise(0.5 if kind == "on" else None)
        sp.search()
        t = timed(sp.finish_move)
        if i >= 8:
            ms[kind].append(t)
    e.check_healthy()
    out = {"boards": a.finish_boards, "sims_per_move": 16, "evaluator": "uniform", "has_set_surprise": has,
           "method": f"HIP events around finish_move alone (k_finish_move + the half flip), 8 warm-up moves, {a.reps} moves per kind in the pattern off on on off"}
    out.update({k: summary(v) for k, v in ms.items()})
    if has:
        out["ratio_on_over_off"] = out["on"]["median_ms"] / out["off"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=1024)
    ap.add_argument("--max-plies", type=int, default=160)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--finish-boards", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--finish-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surprise_weighting_bench: no GPU (a timing taken elsewhere says nothing)")
    res = {"what": "policy surprise weighting: the weighted draw against the uniform one; finish_move with the option off against on",
           "device": torch.cuda.get_device_name(0)}
    if not a.finish_only:
        res["sample"] = sample_ab(a)
    res["finish_move"] = finish_ab(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
