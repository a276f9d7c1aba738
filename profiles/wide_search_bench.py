"""Measurements of the wide search (include/cczero.h "Wide search") on one GPU, one process, configurations interleaved.

    python profiles/wide_search_bench.py --part game|analyse|steps [--out FILE.json] [--repeats R]

game:    MCTS_AI.get_action on the start position at n_playout 200 and 1600: the scouted sequential search (the default, whose code
         this feature does not touch) against width 8 / 16 / 32. Every call searches a fresh tree; sims/s = n_playout / wall time of
         the call (it ends in a device synchronise). Also the mean leaves per board-step and the collision share.
analyse: BatchedAnalysis of 16 and of 64 positions x 400 simulations: width 1 against 4 / 8 / 16 (16 positions x width 4 = 64 slots:
         the largest engine whose every step is one call of the small-batch convolution kernel).
steps:   time per launch of ccz_step_wide (widths 8 and 16) against ccz_step_compact at A = 1 and 16 searched boards, device events
         around 100 launches of (ccz_gather_priors + the step) on constant logits; the environment variable CCZ_WIDE_TAIL_WAVES=1
         makes one wave do everything (run the part once with and once without it to compare the two kernel shapes).
The net is the full-size tower with random weights drawn from ``--seed``: playing strength is not measured here, but the tree -- and
with it the scouted search's table hit rate, 20 to 49 evaluator calls per 200 simulations from one unseeded process to the next -- does
depend on the weights, so runs are comparable only under one seed.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(xs):
    return round(statistics.median(xs), 1)


def part_game(repeats):
    from chinesechesszero_amd.game import Board
    from chinesechesszero_amd.mcts import MCTS_AI
    from chinesechesszero_amd.net import PolicyValueNet
    pvn = PolicyValueNet(device="cuda:0")
    out = {}
    for n in (200, 1600):
        players = {"scouted": MCTS_AI(pvn.policy_value_fn, n_playout=n)}
        for w in (8, 16, 32):
            players[f"width{w}"] = MCTS_AI(pvn.policy_value_fn, n_playout=n, width=w)
        rates = {k: [] for k in players}
        board = Board()
        for rep in range(repeats + 1):          # pass 0 warms every configuration up (graph captures, code objects)
            for name, ai in players.items():
                if ai.mcts._engine is not None:
                    ai.mcts._engine.clear_eval_cache()   # the same position again: without this every leaf would be a table hit
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ai.get_action(board)            # fresh tree every call (mcts.py:228-229)
                torch.cuda.synchronize()
                if rep:
                    rates[name].append(n / (time.perf_counter() - t0))
        res = {}
        for name, ai in players.items():
            res[name] = {"sims_per_s_median": _median(rates[name]), "sims_per_s_all": [round(r, 1) for r in rates[name]]}
            if ai.mcts._wide is not None:
                s = ai.mcts._wide.summary()
                res[name].update(mean_leaves_per_step=s["mean_leaves_per_step"], collision_share=s["collision_share"],
                                 graph=ai.mcts._wide.use_graph)
        out[f"n_playout_{n}"] = res
    return out


def _positions(n, seed=1):
    from chinesechesszero_amd.game import Board, Move
    g = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        b = Board()
        for _ in range(int(g.randint(0, 12))):
            ids = b.legal_ids()
            if not ids or b.is_game_over():
                break
            b.push(Move.from_id(int(ids[g.randint(len(ids))])))
        out.append(b)
    return out


def part_analyse(repeats):
    from chinesechesszero_amd.analyse import BatchedAnalysis
    from chinesechesszero_amd.net import PolicyValueNet
    pvn = PolicyValueNet(device="cuda:0")
    out = {}
    for n_pos in (16, 64):
        pos = _positions(n_pos)
        ans = {f"width{w}": BatchedAnalysis(pvn, n_pos, n_playout=400, width=w) for w in (1, 4, 8, 16)}
        secs = {k: [] for k in ans}
        for rep in range(repeats + 1):
            for name, an in ans.items():
                an.engine.clear_eval_cache()             # the same file again: without this every leaf would be a table hit
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                recs = an.analyse(pos)
                torch.cuda.synchronize()
                assert all(r["status"] == "ok" or r["status"].startswith("game over") for r in recs)
                if rep:
                    secs[name].append(time.perf_counter() - t0)
        res = {}
        for name, an in ans.items():
            med = statistics.median(secs[name])
            res[name] = {"seconds_median": round(med, 4), "sims_per_s_median": round(n_pos * 400 / med, 1), "seconds_all": [round(s, 4) for s in secs[name]]}
            if an.wide is not None:
                s = an.wide.summary()
                res[name].update(mean_leaves_per_step=s["mean_leaves_per_step"], collision_share=s["collision_share"])
        out[f"positions_{n_pos}"] = res
    return out


def part_steps(repeats, launches=100):
    from chinesechesszero_amd.engine import SelfPlayEngine
    out = {"tail_waves_env": os.environ.get("CCZ_WIDE_TAIL_WAVES", "")}
    for A in (1, 16):
        res = {}
        for W in (1, 8, 16):
            times = []
            for rep in range(repeats + 1):
                e = SelfPlayEngine(A * W, n_playout=launches, max_nodes=launches * max(W, 2) * 64, eps=0.0, seed=2)
                logits = torch.zeros((e.B, 2086), dtype=torch.float32, device=e.device)
                value = torch.zeros((e.B,), dtype=torch.float32, device=e.device)
                if W > 1:
                    e.set_width(W)
                    e.select_wide()
                    step = lambda: e.step_wide(value)
                else:
                    e.select_leaves()
                    step = lambda: e.step_compact(value)
                for _ in range(5):
                    e.gather_priors(logits, value)
                    step()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(launches):
                    e.gather_priors(logits, value)
                    step()
                t1.record()
                torch.cuda.synchronize()
                e.check_healthy()
                if rep:
                    times.append(t0.elapsed_time(t1) * 1000.0 / launches)
                leaves = e.stats()["sims"]
                e.close()
            res[f"width{W}"] = {"us_per_gather_plus_step_median": round(statistics.median(times), 2), "all": [round(t, 2) for t in times],
                                "sims_backed_up": int(leaves)}
        out[f"A_{A}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("game", "analyse", "steps"), required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0, help="torch seed of the net's random weights")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("wide_search_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    torch.manual_seed(args.seed)
    res = {"part": args.part, "seed": args.seed, "device": torch.cuda.get_device_name(0),
           **{"game": part_game, "analyse": part_analyse, "steps": part_steps}[args.part](args.repeats)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
