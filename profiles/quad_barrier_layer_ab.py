"""One quad one-launch tower layer, the quad tile's ring of five (a barrier per half-step) against its two-step ring.

As profiles/g16c_layer_ab.py (residual on, post-ReLU input, ONE process, ONE device, arms interleaved, the first arm alternates), but
both libraries run both layouts: rows (k_conv3x3_g16_one_quad) and chunk-major (k_conv3x3_g16c_one_quad, what the evaluator runs).
OTHER is a library built with -DCCZ_G5Q_PAIR=0 (make -C chinesechesszero_amd/csrc ab NAME=g5q_ring5 ABFLAGS=-DCCZ_G5Q_PAIR=0) or the
parent commit's library: the two are the same instructions. The four outputs must be identical bytes.

usage: python profiles/quad_barrier_layer_ab.py OTHER_LIB [--boards 4096 3696] [--rounds 7] [--iters 100] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = 1 | 64 | 128 | 512 | 65536  # ReLU | CCZ_CONV_G16 | _EDGE_TILES | _ONE_LAUNCH | _QUAD


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--boards", type=int, nargs="+", default=[4096, 3696])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from chinesechesszero_amd.net import g16_to_g16c, g16c_to_g16, pack_conv_weights_g16

    def load(path):
        L = C.CDLL(os.path.abspath(path))
        for f in ("ccz_conv3x3_c256_f16", "ccz_conv3x3_c256_g16c_f16"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_int32]
        return L

    ring5, pair = load(a.other), load(os.path.join(ROOT, "chinesechesszero_amd", "libcczero.so"))
    dev = torch.device("cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = {"flags": FLAGS, "rounds": a.rounds, "iters": a.iters, "layers": []}
    for B in a.boards:
        G = B // 16
        g = torch.Generator(device="cpu").manual_seed(1)
        x = torch.relu(torch.randn(G, 1440, 256, generator=g) * 0.5).to(dev).half()
        res = torch.relu(torch.randn(G, 1440, 256, generator=g) * 0.5).to(dev).half()
        w = (torch.randn(256, 3, 3, 256, generator=g) * 0.03).to(dev).half()
        bias = (torch.randn(256, generator=g) * 0.1).to(dev)
        wp = pack_conv_weights_g16(w)
        xc, rc = g16_to_g16c(x), g16_to_g16c(res)
        arms = [("ring5_rows", ring5.ccz_conv3x3_c256_f16, x, res), ("pair_rows", pair.ccz_conv3x3_c256_f16, x, res),
                ("ring5_g16c", ring5.ccz_conv3x3_c256_g16c_f16, xc, rc), ("pair_g16c", pair.ccz_conv3x3_c256_g16c_f16, xc, rc)]
        ys = [torch.zeros_like(x) for _ in arms]

        def run(i):
            _, fn, xin, rin = arms[i]
            assert fn(s, xin.data_ptr(), wp.data_ptr(), bias.data_ptr(), rin.data_ptr(), ys[i].data_ptr(), B * 90, FLAGS) == 0

        for i in range(len(arms)):
            run(i)
        torch.cuda.synchronize()
        same = [bool(torch.equal(g16c_to_g16(y) if n.endswith("g16c") else y, ys[0])) for (n, *_), y in zip(arms, ys)]
        assert all(same), "outputs differ"
        for _ in range(3):                                                             # load the chip before the first timed round
            for i in range(len(arms)):
                for _ in range(a.iters):
                    run(i)
        torch.cuda.synchronize()
        times = {n: [] for n, *_ in arms}
        for rnd in range(a.rounds):
            order = list(range(len(arms)))
            order = order[rnd % len(arms):] + order[:rnd % len(arms)]
            for i in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                run(i)
                e0.record()
                for _ in range(a.iters):
                    run(i)
                e1.record()
                torch.cuda.synchronize()
                times[arms[i][0]].append(e0.elapsed_time(e1) / a.iters * 1e3)
        us = {n: {"median": statistics.median(t), "min": min(t), "max": max(t), "all": [round(v, 2) for v in t]} for n, t in times.items()}
        result["layers"].append({"boards": B, "outputs_identical": same, "nonzero_out": int((ys[0] != 0).sum().item()), "us": us,
                                 "pair_over_ring5_median": {k: us["pair_" + k]["median"] / us["ring5_" + k]["median"] for k in ("rows", "g16c")}})
    txt = json.dumps(result, indent=1)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
