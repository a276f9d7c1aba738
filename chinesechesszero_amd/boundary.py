"""The evaluator boundary of the host front ends (``selfplay``, ``wide``, ``mcts``, ``arena``, ``match``, ``analyse``): ONE definition
of what an evaluator can do and what says that its weights changed (:func:`describe`), of noticing that they did
(:class:`WeightsWatch`), of warm-up + hipGraph capture (:func:`capture`, :func:`may_graph`), of handing the evaluator's answer to the
tree (:func:`deliver`) and of the reference's throttled progress callback (:class:`PlayoutTicker`). None of it is on the GPU's hot
path; all of it is where a silent mistake means searching with stale weights."""
from __future__ import annotations

from typing import Callable, NamedTuple


class Evaluator(NamedTuple):
    fn: Callable            # leaf fp16 [B,17,7,10,9] (, plan=) -> (prob | logits, value)
    batched: bool           # takes the device leaf tensor (else: a reference-style f(board))
    returns_logits: bool    # policy-head logits, not probabilities: the engine gathers the legal priors itself
    accepts_plan: bool      # fn(leaf, plan=(rows, n)) computes the planned rows only, outputs compact
    graph_safe: bool        # static shapes, no host sync: may be captured into a hipGraph
    stateless: bool         # no weights that could change
    version: Callable       # () -> what changes when the weights do (None: nothing says so)
    has_version: bool       # ``version`` means something, or there is nothing to tell apart (stateless)


def describe(evaluator, version_fn=None) -> Evaluator:
    """``evaluator``: a network object with ``evaluate_leaves_logits`` (``PolicyValueNet``) or a callable carrying the capability
    attributes. The weights version is ``version_fn()`` if given, else the ``weights_version`` of the first that has one of: the
    object passed in, the object the callable is a bound method of, the callable itself. ``PolicyValueNet`` bumps it whenever its
    inference copy is rebuilt or invalidated (training step, hot reload): a captured graph holds that copy's addresses and an
    evaluation cache its results, so both must follow. A lambda / partial / closure has no such owner: pass ``version_fn``."""
    fn = getattr(evaluator, "evaluate_leaves_logits", evaluator)
    flags = [bool(getattr(fn, k, False)) for k in Evaluator._fields[1:6]]
    owner = next((o for o in (evaluator, getattr(fn, "__self__", None), fn) if hasattr(o, "weights_version")), None)
    version = version_fn or (lambda: getattr(owner, "weights_version", None))
    return Evaluator(fn, *flags, version, version_fn is not None or owner is not None or flags[4])


def kind_of(evaluator, planned: bool = False) -> str:
    """The boundary kind :func:`deliver` takes: "planned", else "logits" or "prob" by what the evaluator returns."""
    return "planned" if planned else "logits" if getattr(evaluator, "returns_logits", False) else "prob"


def need_version(ev: Evaluator, who: str = "", planned: bool = False, consequence: str = ""):
    """An evaluator that nothing can tell the weights of: a planned boundary refuses it (its cached evaluations could never be
    invalidated), a captured graph or a scouted table says so once and goes on."""
    if ev.has_version:
        return
    if planned:
        raise ValueError(f"{who}planned evaluator boundary (evaluation cache) with an evaluator that exposes no weights_version: "
                         "pass version_fn=... (what changes when its weights do), mark it `stateless = True`, or use eval_cache_log2=0")
    from .tools import log
    log(f"{who}the evaluator exposes no weights_version and no version_fn was given: {consequence}", "WARNING")


def reads_history(evaluator) -> bool:
    """Whether the evaluator reads all 17 plane groups of a leaf row: a true ``leaf_history`` attribute (or a callable of that name
    returning true) on the callable, on the object it is a bound method of, or on the object passed in. Nothing says so: it does not
    -- ``InferenceNet`` packs the 21 live channels of groups 7, 15 and 16 and would drop the other 98 planes without a word."""
    fn = getattr(evaluator, "evaluate_leaves_logits", evaluator)
    for o in (fn, getattr(fn, "__self__", None), evaluator):
        v = getattr(o, "leaf_history", None)
        if v is not None:
            return bool(v() if callable(v) else v)
    return False


def need_history(engine, evaluator, who: str = ""):
    """An engine that writes leaf history planes (``SelfPlayEngine.set_leaf_history``) with an evaluator that does not read them is
    refused: the search would run, on inputs the net never saw and with cache keys that tell apart rows the evaluator cannot."""
    if getattr(engine, "leaf_history", False) and not reads_history(evaluator):
        raise ValueError(f"{who}the engine writes leaf history planes (set_leaf_history) but the evaluator does not read them: it packs "
                         "plane groups 7, 15 and 16 only. Use an evaluator that declares `leaf_history = True`, or turn the option off")


class WeightsWatch:
    """The last weights version seen. What follows a change (clear the cache, drop graphs, re-capture, re-salt) is the caller's.
    It holds the value only, never the evaluator or its owner: a front end and its engine die with their last reference."""

    def __init__(self, seen=None):
        self.seen = seen

    def moved(self, version) -> bool:
        before, self.seen = self.seen, version
        return version != before


def may_graph(use_graph, ev, device) -> bool:
    return bool(use_graph and ev.graph_safe and device.type == "cuda")


def capture(device, body, warm=None, warmup: int = 3):
    """``body()`` as a hipGraph (captured, not executed). ``warm`` (the evaluator call of ``body``) first runs ``warmup`` times
    eagerly on a side stream, results discarded: the MIOpen find step, allocator warm-up and the rebuild of a stale inference copy
    must happen OUTSIDE the capture."""
    import torch   # (here: the arena's statistics import this module and need no torch)
    if warm is not None:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                warm()
        torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


def deliver(engine, kind: str, out, value, last: bool, between=None):
    """Hand the evaluator's ``(out, value)`` to the tree and step (fused expand + backup + next selection: returns the next leaf
    batch) or, on a move's ``last`` simulation, only expand and back up (returns None). ``between()`` runs after the softmax +
    gather of the legal priors, which belongs to the evaluator side of the split, and before the simulator kernel."""
    if kind == "planned":       # compact rows of the planned boards; step / backup use the engine-owned leaf values
        engine.gather_priors_planned(out, value)
        value = None
    elif kind == "logits":
        engine.gather_priors(out, value)
    if between is not None:
        between()
    if kind == "prob":
        return engine.expand_backup(out, value) if last else engine.step(out, value)
    return engine.expand_backup_compact(value) if last else engine.step_compact(value)


class PlayoutTicker:
    """Reference mcts.py:153-160: ``on_playout(count)`` every ``max(1, n_playout // 100)`` simulations and after a move's last
    one; what it raises is swallowed."""

    def __init__(self, n_playout: int, on_playout=None):
        self.interval, self.on_playout, self.acc = max(1, n_playout // 100), on_playout, 0

    def room(self, left: int) -> int:
        """How many of the ``left`` simulations may run before a report is due."""
        return left if self.on_playout is None else min(left, self.interval - self.acc)

    def tick(self, n: int = 1, last: bool = False):
        self.acc += n
        if self.on_playout is not None and self.acc and (self.acc >= self.interval or last):
            try:
                self.on_playout(self.acc)
            except Exception:
                pass
            self.acc = 0
        if last:
            self.acc = 0
