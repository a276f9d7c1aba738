"""The evaluator of narrow nets (10 x 128 and 6 x 64, random initialisation) at 11, 1024 and 4096 boards: time per call and per tower
layer, as medians between HIP events. Runs on this tree AND on a checkout of the commit before the narrow kernels: ``narrow`` is used
only where the tree has it, so the baseline is that commit's MIOpen path measured on the same box, never this tree with the option off.

    python profiles/narrow_tower.py --label parent --out a.json        (from the parent checkout)
    python profiles/narrow_tower.py --label narrow --out b.json        (from this tree)
    ... three interleaved pairs ...
    python profiles/narrow_tower.py --merge a1.json b1.json a2.json ... --out profiles/narrow_tower.json

Per call: ``PolicyValueNet.evaluate_leaves_logits`` on real-shaped rows (random 0/1 planes in the three live groups), warm-up first (MIOpen's
find step, buffers), then ``--iters`` calls each between its own pair of events. Per tower layer: the same net with ONE block is timed
the same way, layer = (T(blocks) - T(1)) / (2 (blocks - 1)) -- a difference of medians that needs no hook inside either tree.
``--planned``: also the planned boundary with a live count of B / 2 (trees whose evaluator skips dead rows get faster, the others do not)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = ((128, 10), (64, 6))
SIZES = (11, 1024, 4096)


def measure(args):
    import torch
    from chinesechesszero_amd.net import EvalOptions, PolicyValueNet
    has_narrow = "narrow" in EvalOptions.FIELDS and not args.no_narrow
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    out = {"label": args.label, "narrow": bool(has_narrow), "iters": args.iters, "device": torch.cuda.get_device_name(0), "cases": []}

    def make(channels, blocks):
        torch.manual_seed(7)
        kw = {"fused_narrow": True} if has_narrow else {}
        pvn = PolicyValueNet(device=dev, num_channels=channels, resblocks_num=blocks, **kw)
        pvn.refresh_inference_copy()
        return pvn

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts), min(ts)

    for channels, blocks in NETS:
        deep, one = make(channels, blocks), make(channels, 1)
        for B in SIZES:
            x = torch.zeros((B, 17, 7, 10, 9), dtype=torch.float16)
            for grp in (7, 15):
                x[:, grp] = (torch.rand((B, 7, 10, 9), generator=g) > 0.9).half()
            x[:, 16] = 1
            x = x.to(dev)
            t_deep, t_deep_min = timed(lambda: deep.evaluate_leaves_logits(x))
            t_one, _ = timed(lambda: one.evaluate_leaves_logits(x))
            case = {"net": f"{blocks}x{channels}", "boards": B, "call_us": round(t_deep, 2), "call_us_min": round(t_deep_min, 2),
                    "one_block_call_us": round(t_one, 2), "layer_us": round((t_deep - t_one) / (2 * (blocks - 1)), 3)}
            if args.planned and B >= 64:
                rows = torch.randperm(B, generator=g).to(torch.int32).to(dev)
                n_rows = torch.tensor([B // 2], dtype=torch.int32, device=dev)
                t_plan, _ = timed(lambda: deep.evaluate_leaves_logits(x, plan=(rows, n_rows)))
                case.update(planned_live_rows=B // 2, planned_call_us=round(t_plan, 2))
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
    return out


def collect_run(args):
    """``collect --boards 4096 --channels 128 --blocks 10 --playout 400 --moves 3`` as the command line builds it (``--fused-narrow`` where the
    tree has it and ``--no-narrow`` is not given), one ``collect_data`` call at a time: seconds per lockstep move, and the evaluator rows the
    planned boundary asked for per step (cache misses that are not shared with another board) against the batch."""
    import tempfile
    import time
    import torch
    from chinesechesszero_amd import collect
    argv = ["--boards", "4096", "--channels", "128", "--blocks", "10", "--playout", "400", "--moves", "3", "--model", "none"]
    has_narrow = hasattr(collect.parse_args(argv), "fused_narrow") and not args.no_narrow
    a = collect.parse_args(argv + (["--fused-narrow"] if has_narrow else []))
    with tempfile.TemporaryDirectory() as tmp:
        kw = {"fused_narrow": True} if has_narrow else {}
        pipe = collect.CollectPipeline(init_model=a.model, n_boards=a.boards, n_playout=a.playout, data_dir=tmp, seed=a.seed, num_channels=a.channels,
                                       resblocks_num=a.blocks, eval_cache_log2=a.eval_cache_log2, **a.options, **kw)
        secs = []
        for _ in range(a.moves):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.collect_data()
            torch.cuda.synchronize()
            secs.append(round(time.perf_counter() - t0, 3))
        e = pipe.selfplay.engine
        st = e.stats()
        steps = a.moves * a.playout
        rows = (st["cache_probes"] - st["cache_hits"] - st["cache_shared_rows"]) / steps
        inf = pipe.policy_value_net._infer
        out = {"label": args.label, "narrow": bool(has_narrow), "command": "collect " + " ".join(argv[:10]) + (" --fused-narrow" if has_narrow else ""),
               "seconds_per_move": secs, "sims": int(st["sims"]), "planned_rows_per_step": round(rows, 1), "boards": a.boards,
               "rows_the_evaluator_computes_per_step": round(rows, 1) if getattr(inf, "batch_invariant", False) else a.boards,
               "batch_invariant": bool(getattr(inf, "batch_invariant", False))}
        pipe.sink.finalize()
    print(json.dumps(out), flush=True)
    return out


def merge(files):
    runs = [json.load(open(f)) for f in files]
    labels = sorted({r["label"] for r in runs})
    table = {}
    for r in runs:
        for c in r["cases"]:
            table.setdefault((c["net"], c["boards"]), {}).setdefault(r["label"], []).append(c)
    rows = []
    for (net, boards), by in sorted(table.items()):
        row = {"net": net, "boards": boards}
        for lab in labels:
            cs = by.get(lab, [])
            if cs:
                for key in ("call_us", "layer_us", "planned_call_us"):
                    vals = [c[key] for c in cs if key in c]
                    if vals:
                        row[f"{lab}_{key}"] = round(statistics.median(vals), 2)
                        row[f"{lab}_{key}_runs"] = vals
        if "parent_call_us" in row and "narrow_call_us" in row:
            row["narrow_over_parent"] = round(row["narrow_call_us"] / row["parent_call_us"], 3)
        rows.append(row)
    return {"what": "evaluator time per call and per tower layer (us, medians between HIP events; per label the median over the interleaved runs)",
            "device": runs[0].get("device"), "runs_per_label": {lab: sum(r["label"] == lab for r in runs) for lab in labels}, "rows": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--label", default="narrow")
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-narrow", action="store_true", help="this tree with the option off (a curiosity, NOT the baseline)")
    ap.add_argument("--planned", action="store_true")
    ap.add_argument("--collect", action="store_true", help="the collector run instead of the evaluator timings")
    ap.add_argument("--merge", nargs="+", default=None, metavar="JSON")
    ap.add_argument("--extra", default=None, help="with --merge: a JSON file whose content is stored under 'collect' (the collector runs)")
    a = ap.parse_args()
    if a.merge:
        res = merge(a.merge)
        if a.extra:
            res["collect"] = json.load(open(a.extra))
    elif a.collect:
        res = collect_run(a)
    else:
        res = measure(a)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
