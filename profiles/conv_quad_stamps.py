"""What the quad tile's meeting point costs a wave (diagnostic builds with -DCCZ_STAMPS, never the shipped library).

One quad one-launch G16C tower layer (residual on, post-ReLU random input), launched back to back for >= 2 s; then, per workgroup and
wave of the LAST launch (csrc/cczero_conv_g16.h g_g5q_stamps): cycles in the counted vmcnt waits, cycles in the workgroup barriers,
how many times the wave met the others, cycles of the whole K loop and its real time (the in-kernel clock). Medians over the quad
workgroups' waves. A stamp is s_memtime + lgkmcnt(0), about 40 cycles: every wait and every barrier segment holds one.

build: make -C chinesechesszero_amd/csrc stamps                                      (the shipped body: one barrier per two half-steps)
       hipcc ... -DCCZ_STAMPS -DCCZ_G5Q_PAIR=0 -o build/diag/libcczero_stamps_ring5.so (the ring of five: one barrier per half-step)
usage: python profiles/conv_quad_stamps.py [--boards 4096 3696] [--seconds 2.5] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = 1 | 64 | 128 | 512 | 65536  # ReLU | CCZ_CONV_G16 | _EDGE_TILES | _ONE_LAUNCH | _QUAD
LIBS = (("pair", "libcczero_stamps.so"), ("ring5", "libcczero_stamps_ring5.so"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, nargs="+", default=[4096, 3696])
    ap.add_argument("--seconds", type=float, default=2.5)
    ap.add_argument("--libdir", default=os.path.join(ROOT, "build", "diag"), help="where the two diagnostic libraries are")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from chinesechesszero_amd.net import g16_to_g16c, pack_conv_weights_g16
    dev = torch.device("cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = {"flags": FLAGS, "seconds": a.seconds, "half_steps": 72, "stamp_cost_note": "a stamp is about 40 cycles; each wait and each barrier segment holds one",
              "layers": []}
    libs = []
    for name, f in LIBS:
        p = os.path.join(a.libdir, f)
        if os.path.exists(p):
            L = C.CDLL(p)
            L.ccz_conv3x3_c256_g16c_f16.restype = C.c_int
            L.ccz_conv3x3_c256_g16c_f16.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_int32]
            L.ccz_debug_g5q_stamps.restype = C.c_int
            L.ccz_debug_g5q_stamps.argtypes = [C.c_void_p, C.c_int]
            libs.append((name, L))
    assert libs, "no diagnostic library in " + a.libdir
    for B in a.boards:
        G = B // 16
        g = torch.Generator(device="cpu").manual_seed(1)
        x = g16_to_g16c(torch.relu(torch.randn(G, 1440, 256, generator=g) * 0.5).to(dev).half())
        res = g16_to_g16c(torch.relu(torch.randn(G, 1440, 256, generator=g) * 0.5).to(dev).half())
        w = (torch.randn(256, 3, 3, 256, generator=g) * 0.03).to(dev).half()
        bias = (torch.randn(256, generator=g) * 0.1).to(dev)
        wp = pack_conv_weights_g16(w)
        y = torch.zeros_like(x)
        layer = {"boards": B, "quad_workgroups": G * 4}
        for name, L in libs:
            st = np.zeros(4096 * 8 * 8, np.uint64)
            assert L.ccz_debug_g5q_stamps(st.ctypes.data_as(C.c_void_p), 1) == 0
            t0, n = time.time(), 0
            while time.time() - t0 < a.seconds:  # keep the chip loaded: the clock read is the loaded clock
                for _ in range(200):
                    assert L.ccz_conv3x3_c256_g16c_f16(s, x.data_ptr(), wp.data_ptr(), bias.data_ptr(), res.data_ptr(), y.data_ptr(), B * 90, FLAGS) == 0
                torch.cuda.synchronize()
                n += 200
            assert L.ccz_debug_g5q_stamps(st.ctypes.data_as(C.c_void_p), 0) == 0
            v = st.reshape(4096, 8, 8)[:min(4096, G * 4)].astype(np.float64)
            vm, bar, loop, real, meet = (v[:, :, i] for i in range(5))
            assert (meet > 0).all()
            med = lambda t: float(np.median(t))
            layer[name] = {
                "launches": n, "meetings_per_tile": med(meet),
                "vmcnt_wait_cycles_per_meeting": med(vm / meet), "barrier_cycles_per_meeting": med(bar / meet),
                "vmcnt_wait_cycles_per_half_step": med(vm / 72), "barrier_cycles_per_half_step": med(bar / 72),
                "half_step_cycles": med(loop / 72), "loop_cycles": med(loop),
                "wait_plus_barrier_share_of_loop": med((vm + bar) / loop),
                "wait_plus_barrier_share_less_stamps": med((vm + bar - 80 * meet) / (loop - 120 * meet)),
                "slowest_wave_over_fastest_barrier_cycles": med(bar.max(axis=1) / np.maximum(bar.min(axis=1), 1)),
                "clock_ghz": med(loop / np.maximum(real, 1)) * 0.1,
            }
        result["layers"].append(layer)
    txt = json.dumps(result, indent=1)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
