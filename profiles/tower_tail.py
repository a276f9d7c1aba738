"""Where the tower's CUs sit idle: the kernel traces of bench runs (rocprofv3 --kernel-trace --output-format csv) reduced to idle
CU-us per step, split into the tower's layer boundaries and the step boundary. Companion of tower_timeline.py (which it leaves as it is).

    python profiles/tower_tail.py <tile_us> <trace.csv> <bench.json> [<trace.csv> <bench.json> ...]

The kernels skip their dead tiles on the device, so the trace's grid sizes are capacities; the live tiles are derived from the
bench line's mean computed rows per step exactly as the kernels derive them (ceil(rows / 16) groups cut into `chains` equal parts,
4 middle + 1 edge-pair tile per group, the edge tile counted as `EDGE` of a middle one). `tile_us` is what one middle tile costs a CU
when the chip is full (e.g. 256 x the cache-off layer time / its tile-equivalents). Per step:
  * tower span = first to last tower-layer kernel of the step (stem, heads layer and everything between them excluded);
  * layer-boundary idle = 256 x span - live tile-equivalents x tile_us (every CU-us in the span that no live tile fills: the tail
    rounds of the chains' launches, launch gaps, and the dead workgroups' exits);
  * step-boundary idle = 256 x the time per step with no tower-layer kernel in flight (stem, heads, FC, gather, k_step).
"""
import csv
import json
import sys

import numpy as np

EDGE = 0.76   # an edge-pair tile (six live taps) against a middle tile (nine): profiles/r04_conv_g16.json


def reduce(trace, bench, tile_us):
    line = json.loads([l for l in open(bench) if l.startswith("{")][-1])
    rows, steps_t = [], []
    with open(trace) as f:
        for x in csv.DictReader(f):
            name = x["Kernel_Name"]
            if "k_step" in name:
                steps_t.append(int(x["Start_Timestamp"]))
            if "k_conv3x3_g16" not in name or "g16_stem" in name or "heads" in name:
                continue
            rows.append((int(x["Start_Timestamp"]), int(x["End_Timestamp"])))
    rows.sort()
    steps_t.sort()
    ms_step = line["ms_per_step"]
    # the timed window: the last run of k_step launches spaced like the bench's steps (the full-batch passes after it are not steps)
    ok = [0.7 * ms_step < (b - a) / 1e6 < 1.4 * ms_step for a, b in zip(steps_t, steps_t[1:])]
    end = max(i for i, v in enumerate(ok) if v) + 1
    start = end
    while start > 0 and ok[start - 1]:
        start -= 1
    t0, t1 = steps_t[start], steps_t[end]
    steps = end - start
    w = [x for x in rows if t0 <= x[0] < t1]
    # time with no tower-layer kernel in flight
    ev = sorted([(t0, 0)] + [(s, 1) for s, _ in w] + [(min(e, t1), -1) for _, e in w] + [(t1, 0)])
    n, last, none = 0, t0, 0
    for t, d in ev:
        if n == 0:
            none += t - last
        last = t
        n += d
    span_us = (t1 - t0 - none) / 1e3 / steps
    rows_step = line["eval_cache"]["rows_computed_per_step"] if line.get("eval_cache") else line["config"]["boards_per_gpu"]
    G = -(-int(round(rows_step)) // 16)
    tiles = G * (4 + EDGE) * 79   # 79 tower layers outside the heads layer
    busy = tiles * tile_us
    return {"boards": line["config"].get("boards_per_gpu"), "sims_per_s": round(line["value"], 1), "ms_per_step": round(ms_step, 4),
            "rows_computed_per_step": round(rows_step, 1), "live_groups": G, "steps_in_window": steps,
            "tower_span_us_per_step": round(span_us, 1), "us_per_tower_layer": round(span_us / 79, 2),
            "ns_per_row_per_layer": round(span_us / 79 / (G * 16) * 1e3, 2),
            "idle_cu_us_per_step_layer_boundaries": round(256 * span_us - busy, 0),
            "idle_share_of_tower_span": round(1 - busy / (256 * span_us), 4),
            "idle_cu_us_per_step_step_boundary": round(256 * none / 1e3 / steps, 0),
            "step_boundary_us_per_step": round(none / 1e3 / steps, 1)}


def main(argv):
    tile_us = float(argv[0])
    out = {"tile_us": tile_us, "edge_tile_equivalent": EDGE, "runs": {}}
    for trace, bench in zip(argv[1::2], argv[2::2]):
        out["runs"][bench] = reduce(trace, bench, tile_us)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
