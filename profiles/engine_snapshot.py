"""What an engine snapshot costs at the benchmark workload (writes profiles/engine_snapshot.json).

4096 boards x 400 simulations a move with the real 40 x 256 net and the evaluation cache on, brought to bench.py's steady state the way
bench.py does it (``preroll`` over 200 plies, then two whole searched moves through the collector's own loop). Then, on one GPU:
  * the blob's bytes next to the size of the allocations it replaces (B x 2 x cap x 20 + the record arrays);
  * ``ccz_snapshot_save`` and ``ccz_snapshot_load`` between HIP events, median of 5, next to a device-to-device copy of the same bytes;
  * one full ``CollectPipeline.save_checkpoint()`` to local disk, wall clock.
Run from the repository root:  python profiles/engine_snapshot.py [--out FILE] [--boards N] [--playout N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "engine_snapshot.json"))
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--playout", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--warm-moves", type=int, default=2)
    a = ap.parse_args()
    import torch

    from bench import preroll
    from chinesechesszero_amd.build import code_hash
    from chinesechesszero_amd.collect import CollectPipeline
    from chinesechesszero_amd.snapshot import sections_start, snapshot_info

    work = tempfile.mkdtemp(prefix="ccz_snapshot_")
    torch.manual_seed(0)
    pipe = CollectPipeline(init_model=os.path.join(work, "none.pkl"), n_boards=a.boards, n_playout=a.playout, max_plies=200, seed=1,
                           data_dir=os.path.join(work, "data"), num_channels=a.channels, resblocks_num=a.blocks, replay_plies=1 << 20,
                           train_every=8, checkpoint_dir=os.path.join(work, "ck"))
    pipe.collect_batched(0)                     # builds the net and the boards
    e = pipe.selfplay.engine
    preroll(e, 200, stagger=True)
    pipe.collect_batched(a.warm_moves)
    torch.cuda.synchronize()
    st = e.stats()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = e.snapshot_size()
    blob = torch.empty((n,), dtype=torch.uint8, device=e.device)
    other = torch.empty_like(blob)
    got = C.c_uint64(0)

    def timed(fn, reps=5):
        ms = []
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return {"median_ms": statistics.median(ms), "all_ms": [round(x, 3) for x in ms]}

    def save():
        assert e.L.ccz_snapshot_save(e.h, stream, C.c_void_p(blob.data_ptr()), n, C.byref(got)) == 0

    def load():
        assert e.L.ccz_snapshot_load(e.h, stream, C.c_void_p(blob.data_ptr()), n, 0) == 0

    t_save = timed(save)
    info = snapshot_info(blob[:sections_start(a.boards)])     # (header + directory: all the counts)
    t_copy = timed(lambda: other.copy_(blob))
    t_load = timed(load)                        # (its own blob: the engine is what it was; includes the cold-cache memset)
    cache_bytes = (1 << e.eval_cache_log2) * 532 if e.eval_cache_log2 else 0
    t_clear = timed(e.clear_eval_cache)
    del other
    t0 = time.perf_counter()
    path = pipe.save_checkpoint()
    t_ck = time.perf_counter() - t0
    B, cap, plies, pi_cap = info["B"], info["cap"], info["max_plies"], info["pi_cap"]
    replaced = B * 2 * cap * 20 + B * plies * (96 + 1 + 1 + 4 + 1 + 4 + 1) + B * pi_cap * 6
    out = {"head": code_hash(), "device": torch.cuda.get_device_name(0),
           "workload": {"boards": a.boards, "playout": a.playout, "blocks": a.blocks, "channels": a.channels, "preroll_plies": 200,
                        "warm_moves": a.warm_moves, "eval_cache_log2": e.eval_cache_log2},
           "blob_bytes": n, "allocations_replaced_bytes": replaced, "blob_over_allocations": n / replaced,
           "proof_bytes_included": bool(info["sections"] & 1),
           "n_nodes": {"mean": float(info["n_nodes"].mean()), "max": int(info["n_nodes"].max())}, "nodes_peak": st["nodes_peak"],
           "ply_mean": float(info["ply"].mean()), "pi_used_mean": float(info["pi_used"].mean()),
           "ccz_snapshot_save": t_save, "ccz_snapshot_load": t_load, "device_to_device_copy_of_blob": t_copy,
           "eval_cache_clear_inside_load": dict(t_clear, bytes=cache_bytes),
           "save_over_copy": t_save["median_ms"] / t_copy["median_ms"], "save_gb_per_s": n / t_save["median_ms"] / 1e6,
           "collect_checkpoint": {"seconds": t_ck, "file_bytes": os.path.getsize(path), "ring_plies": 0 if pipe.ring is None else
                                  int(pipe.ring.window()[1] - pipe.ring.window()[0]), "disk": "local temporary directory"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
