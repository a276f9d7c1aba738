"""What the mate search costs: ``ccz_mate_search`` on 4096 positions of a self-play run of this tree, at
max_plies 7 and 15 and budgets 256 / 2048 / 16384 -- the median and the worst of 30 calls between HIP events, nodes per second, the share
of boards in each state -- and beside them what a 400-simulation move of the same 4096 boards costs (select, 399 fused steps,
expand_backup, finish_move with a stub evaluator: uniform priors, fixed values, so it is the ENGINE's share of a move; a network adds its
own time on top). Recorded, not gated.

    python profiles/mate_search.py --out profiles/mate_search.json [--baseline-tree DIR]

``--baseline-tree DIR``: a checkout of the parent commit with its library built; the move is then timed there too, in a fresh process
that imports DIR's package, and the ratios are given against it. Budgets above the library's cap are skipped and listed."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PLIES, BUDGETS, CALLS, SIMS = (7, 15), (256, 2048, 16384), 30, 400


def _tree(argv):
    return argv[argv.index("--tree") + 1] if "--tree" in argv else os.path.dirname(HERE)


sys.path.insert(0, os.path.abspath(_tree(sys.argv)))


def _stub(e):
    import torch
    P = torch.full((e.B, 2086), 1.0 / 2086, dtype=torch.float32, device=e.device)
    V = (torch.arange(e.B, device=e.device, dtype=torch.float32) % 7 - 3.0) / 10.0
    return P, V


def positions(boards: int, seed: int = 1):
    """``boards`` move lists from the start position: a self-play run of this tree (16 simulations per move, the stub evaluator, moves
    drawn by the device sampler), board b cut at ply 20 + b % 41 (or at its last ply, had the game ended before)."""
    import numpy as np
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(boards, n_playout=16, seed=seed)
    P, V = _stub(e)
    played = np.full((boards, 60), -1, np.int32)
    for ply in range(60):
        e.select_leaves()
        for _ in range(15):
            e.step(P, V)
        e.expand_backup(P, V)
        played[:, ply] = e.finish_move().cpu().numpy()
    e.check_healthy()
    length = (played >= 0).sum(axis=1)
    over = e.game_status()["over"] != 0
    cut = np.minimum(20 + np.arange(boards) % 41, np.where(over, length - 1, length))
    moves = np.where(np.arange(60)[None, :] < cut[:, None], played, -1).astype(np.int32)
    return moves, cut


_START = None


def _load(e, moves):
    import numpy as np
    from chinesechesszero_amd.engine import SelfPlayEngine  # noqa: F401
    global _START
    if _START is None:
        _START = type(e)(1, n_playout=1).root_positions()[0]      # (a new engine stands at the start position)
    start = _START
    B = e.B
    status = e.set_positions(np.repeat(start[None, :], B, axis=0), np.ones(B, np.uint8), np.zeros(B, np.int32), moves)
    if status.any():
        raise RuntimeError(f"positions refused: {status[status != 0][:8].tolist()}")


def _timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def move_ms(moves, reps: int = 3):
    """Milliseconds of one 400-simulation move of all boards (fresh trees each time: the positions are loaded again)."""
    import torch
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(moves.shape[0], n_playout=SIMS, seed=2, mirror=False)
    P, V = _stub(e)
    out = []
    for _ in range(reps + 1):            # (the first one warms up)
        _load(e, moves)
        torch.cuda.synchronize()

        def move():
            e.select_leaves()
            for _ in range(SIMS - 1):
                e.step(P, V)
            e.expand_backup(P, V)
            e.finish_move(keep_tree=False)
        out.append(_timed(move, 1)[0])
    e.check_healthy()
    return out[1:]


def mate_runs(moves, extra=()):
    import numpy as np
    import torch
    from chinesechesszero_amd import _lib
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(moves.shape[0], n_playout=SIMS, seed=2, mirror=False)
    _load(e, moves)
    out_dev = torch.empty((4, e.B), dtype=torch.int32, device=e.device)
    runs, skipped = [], []
    for plies, budget, calls in [(p, b, CALLS) for p in PLIES for b in BUDGETS] + [(int(p), int(b), 3) for p, b in extra]:
        if budget > _lib.MATE_MAX_NODES:
            skipped.append([plies, budget])
            continue

        def call():
            _lib.check(e.L.ccz_mate_search(e.h, e._stream(), plies, budget, out_dev[0].data_ptr(), out_dev[1].data_ptr(), out_dev[2].data_ptr(),
                                           out_dev[3].data_ptr()))
        call()
        torch.cuda.synchronize()
        ms = _timed(call, calls)
        res = out_dev.cpu().numpy()
        nodes = int(res[3].sum())
        med = statistics.median(ms)
        runs.append({"max_plies": plies, "node_budget": budget, "calls": calls, "median_us": round(med * 1e3, 1), "worst_us": round(max(ms) * 1e3, 1),
                     "nodes": nodes, "nodes_per_s": round(nodes / (med * 1e-3), 1), "max_nodes_of_a_board": int(res[3].max()),
                     "state_share": {str(s): round(float((res[0] == s).mean()), 5) for s in range(4)},
                     "mates_by_dist": {str(d): int(((res[0] == 1) & (res[1] == d)).sum()) for d in sorted(set(res[1][res[0] == 1].tolist()))}})
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    e.check_healthy()
    return runs, skipped


def main(argv=None) -> int:
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--extra", nargs="*", default=(), metavar="PLIES:BUDGET", help="settings past the six, three calls each: what the budget cap is chosen from")
    ap.add_argument("--tree", default=None, help="import the package from this checkout (the baseline's child process)")
    ap.add_argument("--move-only", default=None, metavar="NPY", help="time the 400-simulation move on the move lists in NPY, print JSON")
    a = ap.parse_args(argv)
    if a.move_only:
        print(json.dumps({"move_ms": move_ms(np.load(a.move_only))}))
        return 0
    moves, cut = positions(a.boards)
    out = {"boards": a.boards, "plies_of_positions": {"min": int(cut.min()), "median": float(np.median(cut)), "max": int(cut.max())},
           "calls_per_setting": CALLS}
    out["mate_search"], out["skipped_above_the_cap"] = mate_runs(moves, [x.split(":") for x in a.extra])
    out["move_400_sims_ms_this_tree"] = move_ms(moves)
    if a.baseline_tree:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "moves.npy")
            np.save(path, moves)
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", a.baseline_tree, "--move-only", path],
                                   capture_output=True, text=True, check=True)
        out["move_400_sims_ms_parent"] = json.loads(child.stdout.strip().splitlines()[-1])["move_ms"]
    base = statistics.median(out.get("move_400_sims_ms_parent", out["move_400_sims_ms_this_tree"]))
    out["baseline"] = "parent" if a.baseline_tree else "this tree"
    for r in out["mate_search"]:
        r["share_of_a_400_sim_move"] = round(r["median_us"] * 1e-3 / base, 5)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
