"""On-path figures of the value spread: HIP-event medians of ccz_step and ccz_finish_move at 4096 boards with the
option off and on, of ccz_lcb_moves, the array's size, and MCTS_AI(n_playout = 200 / 1600) with the option off and on. Recorded, not
gated. Prints one JSON object; ``python profiles/value_spread.py [--boards 4096] [--out FILE]``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps=21):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def kernels(boards: int) -> dict:
    import torch
    from chinesechesszero_amd.engine import SelfPlayEngine
    res = {"boards": boards}
    for on in (False, True, False, True):
        e = SelfPlayEngine(boards, n_playout=400, seed=1)
        if on:
            free0 = torch.cuda.mem_get_info()[0]
            e.set_value_stats(True)
            torch.cuda.synchronize()
            res["array_bytes"] = free0 - torch.cuda.mem_get_info()[0]      # 4 B x 2 x max_nodes x boards, as the allocator rounds it
        P = torch.full((boards, 2086), 1.0 / 2086, dtype=torch.float32, device=e.device)
        V = (torch.arange(boards, device=e.device, dtype=torch.float32) % 7 - 3.0) / 10.0
        e.select_leaves()
        for _ in range(96):                 # into the middle of a move: trees a few plies deep
            e.step(P, V)
        key = "on" if on else "off"
        res.setdefault("step_ms_" + key, []).append(_median_ms(lambda: e.step(P, V)))
        e.expand_backup(P, V)
        if on:
            res.setdefault("lcb_moves_ms", []).append(_median_ms(lambda: e.lcb_moves(5.0, 0.15, 2)))

        def move():
            e.finish_move()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        move()
        b.record()
        b.synchronize()
        res.setdefault("finish_move_ms_" + key, []).append(a.elapsed_time(b))
        e.check_healthy()
        del e
        torch.cuda.empty_cache()
    return res


def one_game(n_playout: int, lcb, moves: int = 6) -> float:
    """Seconds per move of MCTS_AI on the start position's first ``moves`` moves with a random-init 2 x 32 net."""
    import torch
    from chinesechesszero_amd.game import Board
    from chinesechesszero_amd.mcts import MCTS_AI
    from chinesechesszero_amd.net import PolicyValueNet
    torch.manual_seed(3)
    pvn = PolicyValueNet(device="cuda:0", num_channels=32, resblocks_num=2)
    ai = MCTS_AI(pvn.policy_value_fn, c_puct=5, n_playout=n_playout, is_selfplay=False, lcb=lcb)
    board = Board()
    board.push(ai.get_action(board))        # warm: engine creation, graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(moves):
        board.push(ai.get_action(board))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / moves


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-one-game", action="store_true")
    a = ap.parse_args(argv)
    os.environ.setdefault("CCZ_MIOPEN_FIND", "0")
    out = {"kernel": kernels(a.boards)}
    if not a.no_one_game:
        out["mcts_ai_s_per_move"] = {str(n): {"off": [one_game(n, None), one_game(n, None)], "on": [one_game(n, True), one_game(n, True)]} for n in (200, 1600)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
