"""Host enqueue time of ``InferenceNet._tower_fused`` (CHANGELOG.md, "one launch schedule for dense and planned batches").

    python profiles/tower_schedule_ab.py [--tree OTHER_CHECKOUT] [--reps 9]

A 40 x 256 net; the whole batch and a planned batch (permuted rows, four fifths live) at 1024 and 4096 boards, driven as
``InferenceNet.forward`` drives them (heads in the last layer). ``time.perf_counter`` around the call alone: what the host spends building
the launch structure and enqueuing 80 layers on its chains -- no synchronisation inside the timed region, one between repetitions. Prints
one JSON line: per shape the median and the min / max of the repetitions, in microseconds. ``--tree``: import the package from another
built checkout (the parent commit's, for the A/B); one process per run, the two trees alternately."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from chinesechesszero_amd.net import InferenceNet, Net
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    inf = InferenceNet(Net(256, 40).to(dev).eval()).to(dev).eval()
    inf.bind_chain_streams(dev)
    out = {"reps": a.reps, "unit": "us"}
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for B in (1024, 4096):
            leaf = torch.zeros(B, 17, 7, 10, 9, dtype=torch.float16)
            leaf.view(B, 119, 90)[:, 49:56] = (torch.rand(B, 7, 90, generator=g) < 0.1).half()
            leaf.view(B, 119, 90)[:, 105:119] = (torch.rand(B, 14, 90, generator=g) < 0.1).half()
            leaf = leaf.to(dev)
            rows = torch.randperm(B, generator=g).to(torch.int32).to(dev).contiguous()
            n_rows = torch.tensor([B - B // 5], dtype=torch.int32, device=dev)
            g16 = inf._g16(B)
            for form, plan in (("dense", None), ("planned", (rows, n_rows))):
                times = []
                for r in range(a.warm + a.reps):
                    x = inf._stem_fused(leaf, plan, g16)
                    heads = inf._head_buffers(x.shape[0], dev)[:2] if g16 else None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    inf._tower_fused(x, plan, g16, heads)
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    if r >= a.warm:
                        times.append((t1 - t0) * 1e6)
                out[f"{form}_{B}"] = {"median": round(statistics.median(times), 1), "min": round(min(times), 1), "max": round(max(times), 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
