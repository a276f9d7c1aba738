"""Leaf history planes (ccz_set_leaf_history): what the option costs in the search, recorded and not gated.

  python profiles/leaf_history.py run [--out FILE]          on an MI355X: two interleaved off / on pairs, one process per run, of
      4096 boards x 400 simulations x 3 moves on the planned boundary (evaluation cache 2^22) with a device stub evaluator that reads
      all 119 planes of a row in either mode (so the evaluator's cost is the same and the searches are position-dependent): sims/s,
      ms per step, cache hit share, evaluator rows. Then, in one more process, HIP-event medians (21) of ccz_select_leaves at 4096
      boards in the middle of a move with the option off and on: the difference is k_leaf_history.
  python profiles/leaf_history.py merge --run FILE [--parent-lib LIB]     no GPU: writes profiles/leaf_history.json from a run's output
      and the gfx950 instruction counts of this tree's library (and, given the parent commit's library, of the parent's next to them:
      every kernel of the parent must have kept its count).

The on / off searches use a stub whose answer depends on the planes, so they are different searches (their mean leaf depths differ):
the hit shares are not like for like. The real network's 128-channel pack + stem are not timed here."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SIMS, MOVES, CACHE_LOG2 = 4096, 400, 3, 22
WATCHED = ("k_step", "k_select", "k_expand_backup", "k_finish_move", "k_conv3x3", "k_leaf_history")


class PlaneStub:
    """logits = (row . W1) . W2 in fp16, value = tanh of one feature: a function of all 119 planes, the same work in both modes."""
    batched = returns_logits = accepts_plan = stateless = leaf_history = True

    def __init__(self, torch, dev):
        g = torch.Generator().manual_seed(11)
        self.torch = torch
        self.w1 = (torch.randint(-8, 9, (10710, 64), generator=g).half() / 16).to(dev)
        self.w2 = (torch.randint(-2, 3, (64, 2086), generator=g).half() / 64).to(dev)
        self.lg = torch.zeros((B, 2086), dtype=torch.float16, device=dev)
        self.vv = torch.zeros((B,), dtype=torch.float32, device=dev)
        self.rows = 0

    def __call__(self, leaf, plan):
        rows, n = plan
        n = int(n.item())
        if n:
            h = leaf[rows[:n].long()].reshape(n, -1) @ self.w1
            self.lg[:n] = h @ self.w2
            self.vv[:n] = self.torch.tanh(h[:, 0].float() / 8)
        self.rows += n
        return self.lg, self.vv


def child_search(on: bool) -> dict:
    import torch
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(B, n_playout=SIMS, seed=1, eval_cache_log2=CACHE_LOG2)
    e.set_leaf_history(on)
    ev = PlaneStub(torch, e.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(MOVES):
        e.select_leaves()
        for i in range(SIMS):
            e.gather_priors_planned(*ev(e.leaf_input, e.eval_plan()))
            e.expand_backup_compact(None) if i + 1 == SIMS else e.step_compact(None)
        e.finish_move()
    t1.record()
    torch.cuda.synchronize()
    e.check_healthy()
    ms, st = t0.elapsed_time(t1), e.stats()
    return {"leaf_history": on, "sims": int(st["sims"]), "ms": ms, "sims_per_s": st["sims"] / ms * 1e3, "ms_per_step": ms / (MOVES * SIMS),
            "cache_probes": int(st["cache_probes"]), "cache_hit_share": (st["cache_hits"] + st["cache_shared_rows"]) / max(1, st["cache_probes"]),
            "evaluator_rows": ev.rows, "mean_leaf_depth": st["sum_depth"] / max(1, st["sims"])}


def child_kernel() -> dict:
    import statistics
    import torch
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(B, n_playout=SIMS, seed=1, eval_cache_log2=CACHE_LOG2)
    ev = PlaneStub(torch, e.device)
    e.select_leaves()
    for i in range(100):                                    # the middle of a move: paths of the depth a search has
        e.gather_priors_planned(*ev(e.leaf_input, e.eval_plan()))
        e.step_compact(None)
    out = {"boards": B, "mean_leaf_depth": e.stats()["sum_depth"] / max(1, e.stats()["sims"])}
    for on in (False, True, False, True):
        e.set_leaf_history(on)
        torch.cuda.synchronize()
        ms = []
        for _ in range(23):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            e.select_leaves()                               # (the pending leaf is selected again: the trees do not change)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        out.setdefault("select_on_ms" if on else "select_off_ms", []).append(statistics.median(ms[2:]))
    out["k_leaf_history_ms"] = min(out["select_on_ms"]) - min(out["select_off_ms"])
    e.check_healthy()
    return out


def run(out_path):
    def child(*args):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", *args], capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            raise SystemExit(f"child {args} ended with {r.returncode}:\n{r.stdout}\n{r.stderr}")   # (nothing more is started on the GPU)
        return json.loads(r.stdout.strip().splitlines()[-1])
    res = {"workload": {"boards": B, "sims_per_move": SIMS, "moves": MOVES, "eval_cache_log2": CACHE_LOG2, "evaluator": "PlaneStub (fp16, all 119 planes)"},
           "runs": [child("search", mode) for mode in ("off", "on", "off", "on")]}
    res["kernel"] = child("kernel")
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def instruction_counts(lib):
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    fat, co = lib + ".fatbin.tmp", lib + ".co.tmp"
    try:
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                        f"--output={co}", "--unbundle"], check=True)
        text = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    finally:
        for p in (fat, co):
            if os.path.exists(p):
                os.remove(p)
    counts, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            name = m.group(1)
            counts[name] = 0
        elif name and line.startswith("\t") and "//" in line:
            counts[name] += 1
    return counts


def merge(run_path, parent_lib):
    with open(run_path) as f:
        res = json.load(f)
    mine = instruction_counts(os.path.join(ROOT, "chinesechesszero_amd", "libcczero.so"))
    ic = {"kernels": len(mine), "watched": {k: v for k, v in sorted(mine.items()) if any(w in k for w in WATCHED)}}
    if parent_lib:
        theirs = instruction_counts(parent_lib)
        ic["parent_kernels"] = len(theirs)
        ic["changed_or_gone"] = {k: [theirs[k], mine.get(k)] for k in sorted(theirs) if mine.get(k) != theirs[k]}
        ic["new"] = {k: mine[k] for k in sorted(mine) if k not in theirs}
        assert not ic["changed_or_gone"], ic["changed_or_gone"]
    res["instruction_counts"] = ic
    runs = res["runs"]
    for key in ("sims_per_s", "ms_per_step", "cache_hit_share", "evaluator_rows"):
        res.setdefault("summary", {})[key] = {m: [r[key] for r in runs if r["leaf_history"] == (m == "on")] for m in ("off", "on")}
    with open(os.path.join(ROOT, "profiles", "leaf_history.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["summary"]), json.dumps(res["kernel"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--out", default=os.path.join(ROOT, "profiles", "leaf_history_run.json"))
    c = sub.add_parser("child")
    c.add_argument("what", choices=("search", "kernel"))
    c.add_argument("mode", nargs="?", default="off")
    m = sub.add_parser("merge")
    m.add_argument("--run", required=True)
    m.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.cmd == "run":
        run(a.out)
    elif a.cmd == "child":
        print(json.dumps(child_search(a.mode == "on") if a.what == "search" else child_kernel()))
    else:
        merge(a.run, a.parent_lib)
