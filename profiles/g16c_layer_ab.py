"""Does a chunk-major activation layout ("G16C") take bytes out of the tower tile's L2->L1 stream?  

One quad one-launch tower layer (residual on, post-ReLU input) in ONE process on ONE device, arms interleaved:
  rows  : PARENT library, ccz_conv3x3_c256_f16 with G16 | EDGE_TILES | ONE_LAUNCH | QUAD -- k_conv3x3_g16_one_quad
  rows2 : THIS library, the same call (the same instructions: the two must time the same)
  g16c  : THIS library, ccz_conv3x3_c256_g16c_f16 -- k_conv3x3_g16c_one_quad: the same tiles, input, residual and output chunk-major
The outputs must be identical bytes (the g16c arm's after the permutation back to rows).
(The first measurement with this script, profiles/r10_g16c.json "reader_probe", was of a reader-only build of the g16c arm: input
chunk-major, residual and output still rows.)

usage: python profiles/g16c_layer_ab.py PARENT_LIB [--boards 4096 3696] [--rounds 7] [--iters 10] [--out FILE.json]
       rocprofv3 --pmc TCP_TCC_READ_REQ_sum SQ_INSTS_VMEM_RD -d DIR -o pmc --output-format csv -- python profiles/g16c_layer_ab.py PARENT_LIB --pmc 1
       python profiles/g16c_layer_ab.py --summarize DIR     (counters per launch and arm from DIR/**/*counter_collection.csv)
"""
import argparse
import collections
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = 1 | 64 | 128 | 512 | 65536  # ReLU | CCZ_CONV_G16 | _EDGE_TILES | _ONE_LAUNCH | _QUAD


def summarize(d):
    acc = collections.defaultdict(lambda: collections.defaultdict(lambda: [0.0, set()]))
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            arm = "g16c" if "g16c_one_quad" in name else "rows" if "g16_one_quad" in name else None
            if arm:
                a = acc[arm][r["Counter_Name"]]
                a[0] += float(r["Counter_Value"])
                a[1].add(r["Dispatch_Id"])
    out = {arm: {c: {"per_launch": v[0] / len(v[1]), "launches": len(v[1])} for c, v in sorted(cs.items())} for arm, cs in acc.items()}
    if "rows" in out and "g16c" in out:
        out["g16c_over_rows"] = {c: out["g16c"][c]["per_launch"] / out["rows"][c]["per_launch"] for c in out["rows"] if c in out["g16c"] and out["rows"][c]["per_launch"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?")
    ap.add_argument("--boards", type=int, nargs="+", default=[4096, 3696])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pmc", type=int, default=0, help="1: three launches per arm at the first board count, no timing (for a rocprofv3 --pmc pass)")
    ap.add_argument("--summarize")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarize:
        print(json.dumps(summarize(a.summarize), indent=1))
        return
    import torch
    sys.path.insert(0, ROOT)
    from chinesechesszero_amd.net import g16_to_g16c, g16c_to_g16, pack_conv_weights_g16

    def load(path, probe):
        L = C.CDLL(os.path.abspath(path))
        for f in ("ccz_conv3x3_c256_f16",) + (("ccz_conv3x3_c256_g16c_f16",) if probe else ()):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_int32]
        return L

    parent = load(a.parent, False)
    mine = load(os.path.join(ROOT, "chinesechesszero_amd", "libcczero.so"), True)
    dev = torch.device("cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = {"flags": FLAGS, "rounds": a.rounds, "iters": a.iters, "layers": []}
    for B in a.boards[:1] if a.pmc else a.boards:
        assert B % 16 == 0
        G = B // 16
        g = torch.Generator(device="cpu").manual_seed(1)
        x = torch.relu(torch.randn(G, 1440, 256, generator=g) * 0.5).to(dev).half()   # G16 rows
        res = torch.relu(torch.randn(G, 1440, 256, generator=g) * 0.5).to(dev).half()
        w = (torch.randn(256, 3, 3, 256, generator=g) * 0.03).to(dev).half()
        bias = (torch.randn(256, generator=g) * 0.1).to(dev)
        wp = pack_conv_weights_g16(w)
        xc, rc = g16_to_g16c(x), g16_to_g16c(res)                                     # G16C: [group][chunk][row][32]
        arms = [("rows", parent.ccz_conv3x3_c256_f16, x, res), ("rows2", mine.ccz_conv3x3_c256_f16, x, res),
                ("g16c", mine.ccz_conv3x3_c256_g16c_f16, xc, rc)]
        ys = [torch.zeros_like(x) for _ in arms]

        def run(i):
            _, fn, xin, rin = arms[i]
            assert fn(s, xin.data_ptr(), wp.data_ptr(), bias.data_ptr(), rin.data_ptr(), ys[i].data_ptr(), B * 90, FLAGS) == 0

        for rep in range(3 if a.pmc else 1):
            for i in range(len(arms)):
                run(i)
        torch.cuda.synchronize()
        same = [bool(torch.equal(g16c_to_g16(y) if n == "g16c" else y, ys[0])) for (n, *_), y in zip(arms, ys)]
        layer = {"boards": B, "outputs_identical_to_rows": same, "nonzero_out": int((ys[0] != 0).sum().item())}
        if not a.pmc:
            times = {n: [] for n, *_ in arms}
            for rnd in range(a.rounds):
                order = list(range(len(arms)))
                order = order[rnd % len(arms):] + order[:rnd % len(arms)]              # the first arm alternates
                for i in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    run(i)
                    e0.record()
                    for _ in range(a.iters):
                        run(i)
                    e1.record()
                    torch.cuda.synchronize()
                    times[arms[i][0]].append(e0.elapsed_time(e1) / a.iters * 1e3)
            layer["us"] = {n: {"median": statistics.median(t), "min": min(t), "max": max(t), "all": [round(v, 2) for v in t]} for n, t in times.items()}
        result["layers"].append(layer)
        assert all(same), "outputs differ"
    txt = json.dumps(result, indent=1)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
