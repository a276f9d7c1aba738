"""Playout-cap randomisation at the benchmark workload: what a lockstep move costs when most boards stop searching early.

    python profiles/playout_cap_bench.py --out profiles/playout_cap.json                      # (b) uncapped / capped
    python profiles/playout_cap_bench.py --default-path PARENT_TREE --out profiles/playout_cap.json   # (a) default_path

(a) ``--default-path PARENT_TREE`` (a built checkout of the parent commit): ``python bench.py`` there and here, budgets off, in
three interleaved pairs on one box, every run a process of its own; ``default_path`` holds every run's sims/s, the two means, the
parent's min-max spread over its three runs (the only noise figure there is) and ``within_parent_spread``: this tree's mean is not
below the parent's mean by more than that spread (the exit status says so too). This mode opens no GPU itself.

(b) Two runs on one box, one after the other, the same net, seed, board states (bench.py's preroll: boards spread over plies 1..200 of
their games) and one untimed warm move each: ``uncapped`` (every board searches --playout simulations per move) and ``capped``
(``BatchedSelfPlay(playout_cap=(--fast, --prob))``: the same --playout lockstep steps per move, but a board on a fast move stops
after --fast simulations and costs no evaluator row from then on). Per step of every timed move: HIP-event milliseconds and the
evaluator rows the plan asked for (``ccz_eval_plan``'s count, read on the device); per run: moves / s, plies / s and full-search
plies / s (the plies whose pi is a policy target). Recorded, not gated: DESIGN.md quotes the file."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def one_run(a, cap):
    import bench
    from chinesechesszero_amd.net import PolicyValueNet
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    torch.manual_seed(0)
    pvn = PolicyValueNet(device="cuda:0", num_channels=a.channels, resblocks_num=a.blocks)
    sp = BatchedSelfPlay(pvn.evaluate_leaves_logits, a.boards, n_playout=a.playout, seed=0, max_plies=a.max_plies,
                         eval_cache_log2=a.eval_cache_log2, playout_cap=cap)
    e = sp.engine
    if a.preroll_plies > 0:
        bench.preroll(e, a.preroll_plies, stagger=True)
    n = a.playout
    rows = torch.zeros((n,), dtype=torch.int64, device=e.device)
    ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(n)]

    def hooks(stage, i):
        if stage == "eval0":
            ev0[i].record()
        elif stage == "eval1":
            rows[i] += e.n_miss[0]
        elif stage == "step1":
            ev1[i].record()

    def boundary():
        moves = sp.finish_move()
        if e.game_status()["over"].any():
            for _ in sp.harvest_record_chunks(1 << 16):
                pass
        return moves

    sp.advance(n, boundary=boundary)            # the warm move (untimed): allocator, inference copy, a searched tree on every board
    ms = np.zeros((a.moves, n))
    full = live = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for m in range(a.moves):
        alive_mask = e.game_status()["over"] == 0
        alive = int(alive_mask.sum())
        sp.advance(n, hooks=hooks, boundary=boundary)
        torch.cuda.synchronize()
        ms[m] = [ev0[i].elapsed_time(ev1[i]) for i in range(n)]
        live += alive
        full += alive if cap is None else int(((e.budgets_out == n).cpu().numpy() & alive_mask).sum())   # full searches among the boards counted in live
    wall = time.perf_counter() - t0
    r = rows.cpu().numpy() / a.moves
    k = n if cap is None else cap[0]
    e.check_healthy()
    st = e.stats()
    out = {"moves": a.moves, "wall_s": wall, "moves_per_s": a.moves / wall, "plies_per_s": live / wall, "full_search_plies_per_s": full / wall,
           "full_search_fraction": full / max(1, live),
           "ms_per_step_first": float(ms[:, :k].mean()), "ms_per_step_rest": float(ms[:, k:].mean()) if k < n else None,
           "rows_per_step_first": float(r[:k].mean()), "rows_per_step_rest": float(r[k:].mean()) if k < n else None,
           "first_steps": k, "ms_per_move_in_steps": float(ms.sum(axis=1).mean()),
           "cache_hits": st["cache_hits"], "cache_probes": st["cache_probes"], "error_flags": st["error_flags"]}
    e.close()
    del sp, pvn
    torch.cuda.empty_cache()
    return out


def default_path(parent_root, pairs, limit_s):
    """``python bench.py`` in the parent's tree and in this one, interleaved, one fresh process per run."""
    import subprocess
    trees = (("parent", os.path.abspath(parent_root)), ("this", ROOT))
    runs = {k: [] for k, _ in trees}
    for i in range(pairs):
        for name, root in trees:
            p = subprocess.run([sys.executable, "bench.py"], cwd=root, capture_output=True, text=True, timeout=limit_s)
            lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
            if p.returncode != 0 or not lines:   # nothing more is started on a GPU that a run may have faulted
                raise RuntimeError(f"bench.py in {root} ended with {p.returncode}: {p.stderr[-2000:]}")
            d = json.loads(lines[-1])
            runs[name].append({"sims_per_s": d["value"], "ms_per_step": d["ms_per_step"], "steps": d["steps"],
                               "code_hash": d.get("roofline", {}).get("code_hash"), "error_flags_any": d.get("error_flags_any")})
            print(f"pair {i} {name}: {d['value']:.1f} sims/s", flush=True)
    v = {k: [r["sims_per_s"] for r in rs] for k, rs in runs.items()}
    mean = {k: float(np.mean(x)) for k, x in v.items()}
    spread = max(v["parent"]) - min(v["parent"])
    return {"command": "python bench.py", "pairs": pairs, "order": "parent, this, parent, this, ...", "runs": runs,
            "mean_sims_per_s": mean, "parent_min_max_spread": spread, "this_minus_parent": mean["this"] - mean["parent"],
            "this_over_parent": mean["this"] / mean["parent"], "within_parent_spread": bool(mean["this"] >= mean["parent"] - spread)}


def merge_out(path, res):
    """Write ``res`` over the file's keys and keep what else the file holds (the other measurement)."""
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
        for k, v in old.items():
            res.setdefault(k, v)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--playout", type=int, default=400)
    ap.add_argument("--fast", type=int, default=100)
    ap.add_argument("--prob", type=float, default=0.25)
    ap.add_argument("--moves", type=int, default=2, help="timed moves per run (after one warm move)")
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--preroll-plies", type=int, default=200)
    ap.add_argument("--max-plies", type=int, default=200)
    ap.add_argument("--eval-cache-log2", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_cap.json"))
    ap.add_argument("--default-path", metavar="PARENT_TREE", default=None, help="measurement (a) only: bench.py there against bench.py here")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--run-limit", type=float, default=240.0, help="seconds one bench.py run may take")
    a = ap.parse_args(argv)
    from chinesechesszero_amd.build import code_hash
    if a.default_path is not None:
        dp = default_path(a.default_path, a.pairs, a.run_limit)
        merge_out(a.out, {"default_path": dp})
        return 0 if dp["within_parent_spread"] else 1
    res = {"what": "profiles/playout_cap_bench.py", "head": code_hash(), "device": torch.cuda.get_device_name(0),
           "workload": {k: getattr(a, k) for k in ("boards", "playout", "fast", "prob", "moves", "blocks", "channels", "preroll_plies",
                                                    "max_plies", "eval_cache_log2")}}
    res["uncapped"] = one_run(a, None)
    res["capped"] = one_run(a, (a.fast, a.prob))
    u, c = res["uncapped"], res["capped"]
    res["capped_over_uncapped"] = {k: c[k] / u[k] for k in ("moves_per_s", "plies_per_s", "full_search_plies_per_s")}
    merge_out(a.out, res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
