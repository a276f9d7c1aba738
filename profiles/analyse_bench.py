#!/usr/bin/env python3
"""The three figures of the batched position analysis (profiles/analyse_cli.json), from ONE GPU visit:

(a) throughput of ``python -m chinesechesszero_amd.analyse`` on 1024 positions at 400 simulations with the random-init 40 x 256
    net (the CLI runs as a child process; its own summary line is what is recorded, first-launch costs included), against the
    one-game front end -- ``MCTS_AI``, one position at a time -- on a 32-position subset, per position;
(b) one ``set_positions`` of 2048 boards x 6 moves between HIP events, against the ``set_position`` loop the arena ran before;
(c) ``ccz_principal_variations`` at 4096 boards x 400 simulations, multipv 1 and 4, between HIP events.

usage: python profiles/analyse_bench.py [out.json]     (sizes: env CCZ_AB_POSITIONS / CCZ_AB_PLAYOUT / CCZ_AB_PV_BOARDS)
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chinesechesszero_amd import tools  # noqa: E402
from chinesechesszero_amd.build import code_hash  # noqa: E402
from chinesechesszero_amd.engine import SelfPlayEngine, apply_moves, legal_moves  # noqa: E402
from chinesechesszero_amd.game import start_squares  # noqa: E402

N_POS = int(os.environ.get("CCZ_AB_POSITIONS", 1024))
N_PLAY = int(os.environ.get("CCZ_AB_PLAYOUT", 400))
PV_BOARDS = int(os.environ.get("CCZ_AB_PV_BOARDS", 4096))
UCI = tools.move_id2move_action


def random_lines(n, max_plies, seed):
    """n seeded random legal lines from the start position, line i of i % (max_plies + 1) plies (device rules)."""
    rng = np.random.default_rng(seed)
    want = np.arange(n) % (max_plies + 1)
    sq = np.repeat(start_squares()[None, :], n, axis=0)
    turn = np.ones(n, np.uint8)
    lines = [[] for _ in range(n)]
    for p in range(max_plies):
        mask, cnt, _ = legal_moves(sq, turn)
        ids = np.zeros(n, np.int32)
        go = (want > p) & (cnt > 0)
        for i in np.flatnonzero(go):
            legal = np.flatnonzero(mask[i])
            ids[i] = legal[rng.integers(len(legal))]
            lines[i].append(int(ids[i]))
        nsq, nturn, _ = apply_moves(sq, turn, ids)
        sq[go], turn[go] = nsq[go], nturn[go]
    return lines


def events(fn, reps):
    """Mean device time of fn() in microseconds over reps calls (one warm-up call first)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def cli_throughput(lines):
    with tempfile.TemporaryDirectory() as d:
        path, out = os.path.join(d, "positions.txt"), os.path.join(d, "out.jsonl")
        with open(path, "w") as f:
            f.write("# seeded random lines from the start position\n")
            for l in lines:
                f.write("startpos" + (" moves " + " ".join(UCI[m] for m in l) if l else "") + "\n")
        cmd = [sys.executable, "-m", "chinesechesszero_amd.analyse", path, "--playout", str(N_PLAY), "--boards", str(len(lines)), "--out", out]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(f"analyse CLI failed ({r.returncode}): {r.stderr[-2000:]}")
        last = r.stderr.strip().splitlines()[-1]
        m = re.search(r"analysed (\d+) positions in ([\d.]+) s: ([\d.]+) positions/s, ([\d.]+) sims/s, ([\d.]+) evaluator rows per step", last)
        recs = [json.loads(x) for x in open(out)]
        ok = [x for x in recs if x["status"] == "ok"]
        assert m and len(recs) == len(lines) and len(ok) >= 0.9 * len(recs) and all(x["root_visits"] == N_PLAY for x in ok), last
        return {"cmd": " ".join(["python"] + cmd[1:3] + ["FILE"] + cmd[4:-1] + ["OUT"]), "positions": int(m.group(1)), "seconds": float(m.group(2)),
                "positions_per_s": float(m.group(3)), "sims_per_s": float(m.group(4)), "evaluator_rows_per_step": float(m.group(5)),
                "process_wall_s": round(wall, 2), "summary_line": last}, recs


def one_game_baseline(lines, recs):
    """The parent commit's only way to do the job: MCTS_AI, one position at a time (its default scouts and hipGraphs)."""
    from chinesechesszero_amd.game import Board, Move
    from chinesechesszero_amd.mcts import MCTS_AI
    from chinesechesszero_amd.net import PolicyValueNet
    pvn = PolicyValueNet(device="cuda:0")
    ai = MCTS_AI(pvn.policy_value_fn, c_puct=5, n_playout=N_PLAY)

    def search(line):
        b = Board()
        for m in line:
            b.push(Move.from_id(m))
        ai.mcts.get_move_probs(b)
        ai.mcts.update_with_move(-1)
        rc = ai.mcts.root_children()
        return int(rc["root_visits"]), int(rc["visits"].max())

    search(lines[0])                      # warm-up: captures, allocator, first launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = [search(l) for l in lines]
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    assert all(g[0] == N_PLAY for g in got)
    return {"positions": len(lines), "seconds": round(sec, 3), "seconds_per_position": round(sec / len(lines), 5),
            "sims_per_s": round(len(lines) * N_PLAY / sec, 1), "note": "random-init weights differ from the CLI's process: times only"}


def loading(seed=1):
    B = 2048
    lines = random_lines(B, 6, seed)
    lines = [l if len(l) == 6 else lines[6] for l in lines]          # every board: 6 moves
    e = SelfPlayEngine(B, n_playout=8, max_nodes=256)
    sq = np.zeros((B, 96), np.uint8)
    sq[:, :90] = start_squares()
    d_sq = torch.from_numpy(sq).cuda()
    d_turn = torch.ones(B, dtype=torch.uint8, device="cuda")
    d_mv = torch.from_numpy(np.asarray(lines, np.int32)).cuda()
    d_n = torch.full((B,), 6, dtype=torch.int32, device="cuda")
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    from chinesechesszero_amd.engine import _ptr
    from chinesechesszero_amd._lib import check

    def launch():
        check(e.L.ccz_set_positions(e.h, e._stream(), _ptr(d_sq), _ptr(d_turn), None, _ptr(d_mv), _ptr(d_n), 6, None, _ptr(status)))

    us = events(launch, 20)
    assert not status.cpu().numpy().any()
    t0 = time.perf_counter()
    st = e.set_positions(sq[:, :90], np.ones(B, np.uint8), None, lines)
    py = time.perf_counter() - t0
    assert not st.any()
    reached = e.root_positions()
    t0 = time.perf_counter()
    for b in range(B):                                               # the parent's arena loop: one board, one launch, one sync
        e.set_position(b, reached[b], 1, 0)
    torch.cuda.synchronize()
    loop = time.perf_counter() - t0
    return {"boards": B, "moves_per_board": 6, "set_positions_kernel_us": round(us, 1), "set_positions_python_call_ms": round(py * 1e3, 2),
            "set_position_loop_ms": round(loop * 1e3, 1), "note": "the loop loads the squares only (it cannot carry moves); kernel time between HIP events, mean of 20"}


def pv_kernel():
    from chinesechesszero_amd.analyse import BatchedAnalysis
    from chinesechesszero_amd.net import PolicyValueNet
    B = PV_BOARDS
    pvn = PolicyValueNet(device="cuda:0")
    an = BatchedAnalysis(pvn, B, n_playout=N_PLAY)
    lines = random_lines(B, 12, 2)
    e = an.engine
    sq = np.repeat(start_squares()[None, :], B, axis=0)
    assert not e.set_positions(sq, np.ones(B, np.uint8), None, lines).any()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    an.sp.search()
    torch.cuda.synchronize()
    search_s = time.perf_counter() - t0
    out = {"boards": B, "n_playout": N_PLAY, "search_s": round(search_s, 2), "sims_per_s": round(B * N_PLAY / search_s, 1)}
    from chinesechesszero_amd.engine import _ptr
    from chinesechesszero_amd._lib import check
    for K in (1, 4):
        M = 32
        bufs = [torch.empty((B, K, M), dtype=torch.int16, device="cuda"), torch.empty((B, K), dtype=torch.int32, device="cuda"),
                torch.empty((B, K, M), dtype=torch.int32, device="cuda"), torch.empty((B, K), dtype=torch.float32, device="cuda"),
                torch.empty((B, K), dtype=torch.float32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")]

        def launch():
            check(e.L.ccz_principal_variations(e.h, e._stream(), K, M, *[_ptr(t) for t in bufs]))

        out[f"multipv{K}_kernel_us"] = round(events(launch, 20), 1)
        out[f"multipv{K}_mean_len"] = round(float(bufs[1].float().mean().item()), 2)
    e.check_healthy()
    return out


def main():
    assert torch.cuda.is_available(), "analyse_bench.py measures on the GPU"
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "analyse_cli.json")
    lines = random_lines(N_POS, 23, 0)
    res = {"head": code_hash(), "device": torch.cuda.get_device_name(0), "net": "40x256 random init", "n_playout": N_PLAY}
    res["a_cli"], recs = cli_throughput(lines)
    res["a_one_game"] = one_game_baseline(lines[:: max(1, N_POS // 32)][:32], recs)
    res["a_ratio_seconds_per_position"] = round(res["a_one_game"]["seconds_per_position"] / (res["a_cli"]["seconds"] / res["a_cli"]["positions"]), 1)
    res["b_loading"] = loading()
    res["c_pv"] = pv_kernel()
    res["note"] = "single-visit figures (one MI355X, one run each); (a) the CLI's seconds include its first launches"
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert res["a_ratio_seconds_per_position"] > 1.0, "the batched path must take less time per position than the one-game path"


if __name__ == "__main__":
    main()
