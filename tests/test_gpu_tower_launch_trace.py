"""GPU: the launch sequence of the evaluator's stem and tower, entry for entry (net.py ``tower_schedule`` / ``_tower_fused``).

The value tests show that every launch structure gives the same bits; they cannot show that the INTENDED structure is the one launched
(a wrong chain count or flag word is slower and still correct). Here a recorder stands in for ``_lib.lib()``: it logs every call -- entry
point, stream, scalars, pointers -- and forwards it to the real library, and the log is compared with ``tower_launch_trace.json``.

That file was recorded with this module's own recorder in a checkout of the commit BEFORE the two launch loops became one schedule
(``python tests/test_gpu_tower_launch_trace.py --write tests/tower_launch_trace.json`` with this file copied into that checkout): the
refactored host path must launch exactly what the two loops launched. Record it again only when the launch structure is meant to change.

A pointer is logged independent of where the allocator put things: a parameter by its name, the leaf / plan / row / head buffers as
[name, byte offset], any other buffer (the packed planes, the tower's second activation buffer) as ["bufN", byte offset] in order of
first appearance. A stream is "cur" or the index in ``chain_streams``. Fork and join events do not pass through the library and are
not traced."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

TRACE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tower_launch_trace.json")

# (boards, options): the sizes at which the schedule changes form -- one chain, two, three, three with edge tiles, two groups; a batch
# that pads its last group of 16; no heads in the last layer; middle and edge-pair tiles as two launches
SHAPES = [(8, {}), (600, {}), (640, {}), (650, {}), (1024, {}), (4096, {}), (4352, {}),
          (1024, {"fused_last": False}), (4096, {"one_launch": False})]
CASES = [(B, opts, planned) for B, opts in SHAPES for planned in (False, True)]


def case_id(case):
    B, opts, planned = case
    return "-".join([str(B), "planned" if planned else "dense"] + [f"{k}={v}" for k, v in opts.items()])


class Recorder:
    """Stands in for the loaded library: every call is logged as (name, raw arguments with pointers resolved to (allocation, offset))
    and forwarded."""

    def __init__(self, real, prototypes):
        self.real, self.prototypes, self.calls = real, prototypes, []

    @staticmethod
    def _blocks():
        """(base, size) of every live block of the caching allocator: a tensor's storage is one block."""
        out = []
        for seg in torch.cuda.memory_snapshot():
            at = seg["address"]
            for blk in seg["blocks"]:
                base = blk.get("address", at)
                if blk["state"] == "active_allocated":
                    out.append((base, blk["size"]))
                at = base + blk["size"]
        return out

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        argtypes = self.prototypes[name][1]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            blocks = self._blocks()
            logged = []
            for i, (a, t) in enumerate(zip(args, argtypes)):
                v = getattr(a, "value", a)
                if i == 0:
                    logged.append(("stream", v or 0))
                elif t is not C.c_void_p:
                    logged.append(("scalar", v))
                elif v is None:
                    logged.append(("ptr", None))
                else:
                    (base, size), = [b for b in blocks if b[0] <= v < b[0] + b[1]]
                    logged.append(("ptr", (base, size, v - base)))
            self.calls.append((name, logged))
            return fn(*args)
        return call

    def encoded(self, names, streams, cur):
        """The log with streams and pointers by name. ``names``: {base address: name} of the tensors known by name."""
        anon, out = {}, []
        for name, logged in self.calls:
            row = [name]
            for kind, v in logged:
                if kind == "stream":
                    row.append("cur" if v == cur else streams.index(v))
                elif kind == "scalar" or v is None:
                    row.append(v)
                else:
                    base, size, off = v
                    if base in names:
                        row.append(names[base] if names[base].startswith("param:") and off == 0 else [names[base], off])
                    else:
                        row.append([anon.setdefault((base, size), f"buf{len(anon)}"), off])
            out.append(row)
        return out


@pytest.fixture(scope="module")
def inf():
    return make_net()


def make_net():
    from chinesechesszero_amd.net import InferenceNet, Net
    dev = torch.device("cuda", 0)
    torch.manual_seed(21)
    return InferenceNet(Net(256, 2).to(dev).eval()).to(dev).eval()   # four layers: a plain block and the last block with the heads


def inputs(B, planned, dev):
    g = torch.Generator().manual_seed(1000 + B)
    leaf = torch.zeros(B, 17, 7, 10, 9, dtype=torch.float16)
    leaf.view(B, 119, 90)[:, 49:56] = (torch.rand(B, 7, 90, generator=g) < 0.1).half()
    leaf.view(B, 119, 90)[:, 105:119] = (torch.rand(B, 14, 90, generator=g) < 0.1).half()
    leaf = leaf.to(dev)
    if not planned:
        return leaf, None
    live = B - B // 5 if B > 8 else 5      # a live count below B, rows permuted
    rows = torch.randperm(B, generator=g).to(torch.int32).to(dev).contiguous()
    return leaf, (rows, torch.tensor([live], dtype=torch.int32, device=dev))


def evaluate(inf, leaf, plan):
    """Stem + tower as ``InferenceNet.forward`` and bench.py drive them. Returns (x, heads or None)."""
    g16 = inf._g16(leaf.shape[0])
    x = inf._stem_fused(leaf, plan, g16)
    heads = inf._head_buffers(x.shape[0], x.device)[:2] if (g16 and inf.opt.fused_last and inf._fused_heads_ok(x)) else None
    assert inf._tower_fused(x, plan, g16, heads) is x
    return x, heads


def traced(inf, case, monkeypatch):
    """One case under the recorder: (encoded trace, x, heads), the outputs cloned."""
    from chinesechesszero_amd import _lib
    from chinesechesszero_amd.net import EvalOptions, chain_streams
    B, opts, planned = case
    dev = torch.device("cuda", 0)
    d = EvalOptions(env={})
    inf.set_options(**{f: getattr(d, f) for f in EvalOptions.FIELDS})
    inf.set_options(**opts)
    leaf, plan = inputs(B, planned, dev)
    streams = [s.cuda_stream for s in chain_streams(dev)]
    Bp = -(-B // 16) * 16 if inf._g16(B) else B
    pol, val = inf._head_buffers(Bp, dev)[:2]
    torch.cuda.synchronize()
    rec = Recorder(_lib.lib(), _lib.PROTOTYPES)
    with monkeypatch.context() as m:
        m.setattr(_lib, "lib", lambda: rec)
        x, heads = evaluate(inf, leaf, plan)
    torch.cuda.synchronize()
    names = {p.data_ptr(): "param:" + n for n, p in inf.named_parameters()}
    names.update({leaf.data_ptr(): "leaf", x.data_ptr(): "x", pol.data_ptr(): "pol", val.data_ptr(): "val"})
    if plan is not None:
        names.update({plan[0].data_ptr(): "rows", plan[1].data_ptr(): "n_rows"})
    trace = rec.encoded(names, streams, torch.cuda.current_stream(dev).cuda_stream)
    return trace, leaf, plan, x.clone(), [h.clone() for h in heads or ()]


@pytest.fixture(scope="module")
def recorded():
    with open(TRACE_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tower_launches_are_the_recorded_ones(inf, recorded, monkeypatch, case):
    """Entry points, streams, flag words, pixel counts, parts and pointers of every launch equal the recording; and the traced run's
    activations and head buffers equal, bit for bit, a run without the recorder."""
    trace, leaf, plan, x, heads = traced(inf, case, monkeypatch)
    want = recorded[case_id(case)]
    got = json.loads(json.dumps(trace))
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    x2, heads2 = evaluate(inf, leaf, plan)
    torch.cuda.synchronize()
    assert torch.equal(x2, x) and torch.isfinite(x.float()).all() and float(x.float().abs().max()) > 0
    assert len(heads2 or ()) == len(heads) == (2 if inf._g16(case[0]) and inf.opt.fused_last else 0)
    for a, b in zip(heads2 or (), heads):
        assert torch.equal(a, b) and float(b.float().abs().max()) > 0


def main():
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        raise SystemExit("usage: python tests/test_gpu_tower_launch_trace.py --write PATH")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    net = make_net()
    out = {}
    with torch.no_grad():
        for case in CASES:
            out[case_id(case)] = traced(net, case, pytest.MonkeyPatch())[0]
    with open(sys.argv[2], "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} traces, {sum(len(v) for v in out.values())} launches -> {sys.argv[2]}")


if __name__ == "__main__":
    main()
