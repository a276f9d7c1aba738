"""CPU: chinesechesszero_amd.boundary -- what an evaluator can do and what says that its weights changed (one lookup order), the
policy for an evaluator that says nothing, the weights watch, the delivery of an evaluator's answer and the playout ticker."""
import logging

import pytest

from chinesechesszero_amd import boundary as B


class Owner:
    weights_version = 3

    def evaluate_leaves_logits(self, leaf, plan=None):
        return "logits", "value"
    evaluate_leaves_logits.batched = evaluate_leaves_logits.returns_logits = evaluate_leaves_logits.accepts_plan = True
    evaluate_leaves_logits.graph_safe = True

    def ev(self, leaf):
        return "prob", "value"
    ev.batched = True


def test_a_network_object_and_a_callable_describe_alike():
    o = Owner()
    for given in (o, o.evaluate_leaves_logits):
        d = B.describe(given)
        assert d.fn == o.evaluate_leaves_logits and d.fn("leaf") == ("logits", "value")
        assert (d.batched, d.returns_logits, d.accepts_plan, d.graph_safe, d.stateless) == (True, True, True, True, False)
        assert d.has_version and d.version() == 3
    d = B.describe(o.ev)
    assert (d.batched, d.returns_logits, d.accepts_plan, d.graph_safe, d.stateless) == (True, False, False, False, False)
    assert B.kind_of(d) == B.kind_of(o.ev) == "prob" and B.kind_of(o.evaluate_leaves_logits) == "logits"
    assert B.kind_of(o.evaluate_leaves_logits, planned=True) == "planned"
    with pytest.raises(AttributeError):
        d.batched = False                     # a record, not a place to keep state


def test_version_lookup_order_version_fn_then_object_then_owner_then_the_callable():
    class Wrapper:                            # an object handed in as the network: it has the method and a version of its own
        weights_version = 10

        def __init__(self, inner):
            self.evaluate_leaves_logits = inner.evaluate_leaves_logits
    o = Owner()
    w = Wrapper(o)
    assert B.describe(w, version_fn=lambda: 99).version() == 99      # 1. version_fn
    assert B.describe(w).version() == 10                             # 2. the object passed in
    assert B.describe(o.evaluate_leaves_logits).version() == 3       # 3. the bound method's owner

    def free(leaf):
        return None
    free.weights_version = 7
    assert B.describe(free).version() == 7                           # 4. the callable itself
    # the version is read when asked for, not when described
    d = B.describe(o.evaluate_leaves_logits)
    o.weights_version = 4
    assert d.version() == 4
    w.weights_version = 11
    assert B.describe(w).version() == 11 != B.describe(w.evaluate_leaves_logits).version()


def test_has_version_in_each_of_the_four_cases():
    def bare(leaf):
        return None
    assert not B.describe(bare).has_version and B.describe(bare).version() is None
    assert B.describe(bare, version_fn=lambda: 1).has_version
    assert B.describe(Owner().ev).has_version
    bare.stateless = True
    d = B.describe(bare)
    assert d.has_version and d.stateless and d.version() is None


def test_no_version_policy_planned_raises_graph_or_table_warns_and_the_uniform_stub_is_silent(caplog):
    from chinesechesszero_amd.net import uniform_evaluator

    def bare(leaf, plan=None):
        return None
    bare.returns_logits = bare.accepts_plan = True
    with caplog.at_level(logging.WARNING):
        with pytest.raises(ValueError):
            B.need_version(B.describe(bare), "X: ", planned=True)
        assert not caplog.records
        B.need_version(B.describe(bare), "X: ", consequence="stale weights")
        assert len(caplog.records) == 1 and "X: the evaluator exposes no weights_version" in caplog.text and "stale weights" in caplog.text
        caplog.clear()
        for ok in (B.describe(uniform_evaluator), B.describe(bare, version_fn=lambda: 0), B.describe(Owner())):
            B.need_version(ok, "X: ")
            B.need_version(ok, "X: ", planned=True)
        assert not caplog.records


def test_weights_watch_says_once_that_the_version_moved():
    o = Owner()
    version = B.describe(o).version
    w = B.WeightsWatch(version())
    assert not w.moved(version()) and w.seen == 3
    o.weights_version = 4
    assert w.moved(version()) and w.seen == 4 and not w.moved(version())
    w = B.WeightsWatch()                      # nothing seen yet: the first look counts as a change
    assert w.moved(version()) and not w.moved(version())


def test_may_graph_needs_all_three():
    import torch
    d = B.describe(Owner())
    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    assert B.may_graph(True, d, gpu) and not B.may_graph(False, d, gpu) and not B.may_graph(True, d, cpu)
    assert not B.may_graph(True, B.describe(Owner().ev), gpu)


class Rec:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name,) + a)
            return "next leaf" if name.startswith("step") else None
        return f


@pytest.mark.parametrize("kind, last, want", [
    ("prob", False, [("step", "out", "v")]),
    ("prob", True, [("expand_backup", "out", "v")]),
    ("logits", False, [("gather_priors", "out", "v"), "between", ("step_compact", "v")]),
    ("logits", True, [("gather_priors", "out", "v"), "between", ("expand_backup_compact", "v")]),
    ("planned", False, [("gather_priors_planned", "out", "v"), "between", ("step_compact", None)]),
    ("planned", True, [("gather_priors_planned", "out", "v"), "between", ("expand_backup_compact", None)])])
def test_deliver_calls_the_engine_methods_of_its_kind_in_order(kind, last, want):
    e = Rec()
    got = B.deliver(e, kind, "out", "v", last, between=lambda: e.calls.append("between"))
    if kind == "prob":
        want = ["between"] + want
    assert e.calls == want and got == (None if last else "next leaf")
    e.calls.clear()
    B.deliver(e, kind, "out", "v", last)
    assert e.calls == [c for c in want if c != "between"]


def _reference(n, sims):
    interval, acc, out = max(1, n // 100), 0, []
    for i in range(sims):
        acc += 1
        if acc >= interval or i == sims - 1:
            out.append(acc)
            acc = 0
    return out


@pytest.mark.parametrize("n", [1, 37, 250, 1999])
def test_ticker_reports_where_the_reference_does(n):
    got = []
    t = B.PlayoutTicker(n, got.append)
    for i in range(n):
        assert t.room(n - i) == min(n - i, t.interval - t.acc) >= 1
        t.tick(1, i == n - 1)
    assert got == _reference(n, n) and t.acc == 0
    # a callback that raises is swallowed; without a callback nothing is held back and nothing is due
    t = B.PlayoutTicker(n, lambda k: 1 / 0)
    t.tick(n, last=True)
    t = B.PlayoutTicker(n)
    assert t.room(n) == n
    t.tick(3)
    t.tick(0, last=True)
    assert t.acc == 0
    # several simulations at once (the wide search's steps), the rest at the end -- and no empty report
    got.clear()
    t = B.PlayoutTicker(300, got.append)
    for k in (2, 2, 1):
        t.tick(k)
    t.tick(0, last=True)
    t.tick(0, last=True)
    assert got == [4, 1]
