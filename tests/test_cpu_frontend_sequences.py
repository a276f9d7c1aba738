"""CPU: the engine calls of ONE move of every host front end -- ScoutedSearch (host and device loop), WideSearch (planned and not),
MCTS.get_move_probs (fused, no scouts), Arena.search -- against a recording stand-in for the engine, in the manner of
test_cpu_selfplay_loop.py. The stand-in's composite methods (``step_logits`` = gather + ``step_compact`` ...) are composed as
``SelfPlayEngine`` composes them and record nothing themselves: what is pinned is the sequence of library-level calls, with the
evaluator's calls ("ev") in their place among them. And: a moved ``weights_version`` empties the evaluation cache before the next
plan, exactly once. No graphs: the stand-in's device is the CPU."""
import numpy as np
import pytest
import torch

from test_cpu_selfplay_loop import FakeEngine


class SeqEngine(FakeEngine):
    n_scouts = 10

    def __init__(self, n_boards, n_playout=400, eval_cache_log2=0, **kw):
        super().__init__(n_boards, n_playout, eval_cache_log2, **kw)
        self.plan_states, self.outcomes, self.leaves = [], [], []
        self.n_miss2 = torch.zeros((2,), dtype=torch.int32)

    # composites, as engine.py composes them
    def step_logits(self, logits, value):
        self.gather_priors(logits, value)
        return self.step_compact(value)

    def expand_backup_logits(self, logits, value):
        self.gather_priors(logits, value)
        self.expand_backup_compact(value)

    def step_planned(self, logits, value):
        self.gather_priors_planned(logits, value)
        return self.step_compact(None)

    def expand_backup_planned(self, logits, value):
        self.gather_priors_planned(logits, value)
        self.expand_backup_compact(None)

    def step_routed(self, *a):
        self.gather_priors_routed(*a)
        return self.step_compact(None)

    def expand_backup_routed(self, *a):
        self.gather_priors_routed(*a)
        self.expand_backup_compact(None)

    # scouts
    def scout_and_plan(self):
        self._rec("scout_and_plan")

    def plan_state_of_board0(self):
        self._rec("plan_state")
        return self.plan_states.pop(0)

    def set_run(self, budget, left):
        self._rec(f"set_run({budget},{left})")

    def scouted_run_launch(self):
        self._rec("run")

    def run_outcome(self):
        self._rec("run_outcome")
        return self.outcomes.pop(0)

    # wide search
    def set_width(self, width):
        self._rec("set_width")

    def set_budgets(self, budgets=None, targets=None):
        self._rec("set_budgets")

    def select_wide(self):
        self._rec("select_wide")
        return self.leaf_input

    def step_wide(self, value):
        self._rec("step_wide" if value is not None else "step_wide(engine values)")
        return self.leaf_input

    def n_leaves(self):
        self._rec("n_leaves")
        return np.array([self.leaves.pop(0)], np.int32)

    # routing (arena)
    def set_routing(self, red_net, salts=(0, 0)):
        self._rec("set_routing")
        self.salts = salts

    def set_positions(self, sq, turn, half, *a, **k):
        return np.zeros(len(sq), np.int32)

    def eval_plan_routed(self):
        self._rec("plan_routed")
        return ("rows0", "n0"), ("rows1", "n1")

    def gather_priors_routed(self, *a):
        self._rec("gather_routed")

    # what a front end reads after the search
    def root_children(self):
        self._rec("root_children")
        return {"k": np.array([2]), "acts": np.array([[7, 9]], np.uint16), "visits": np.array([[2, 1]], np.int32)}

    def check_healthy(self):
        self._rec("check_healthy")


class Net:
    """An evaluator's owner: ``ev`` is marked like PolicyValueNet.evaluate_leaves_logits and writes "ev" into the engine's record."""
    weights_version = 0
    calls = None

    def ev(self, leaf, plan=None):
        self.calls.append("ev" if plan is None else "ev(plan)")
        return torch.zeros((leaf.shape[0], 2086), dtype=torch.float16), torch.zeros(leaf.shape[0])
    ev.batched = ev.returns_logits = ev.accepts_plan = True


def _scouted(device_loop):
    from chinesechesszero_amd.selfplay import ScoutedSearch
    net, e = Net(), SeqEngine(11, eval_cache_log2=16)
    net.calls = e.calls
    return net, e, ScoutedSearch(e, net.ev, use_graph=False, device_loop=device_loop)


def test_scouted_host_loop_a_miss_then_two_hits():
    net, e, s = _scouted(False)
    e.plan_states = [0, 1, 1]
    s.begin_move()
    for i in range(3):
        s.simulate(last=i == 2)
    assert e.calls == ["select", "scout_and_plan",
                       "plan_state", "ev", "gather_planned", "step_compact(engine values)", "scout_and_plan",
                       "plan_state", "step_compact(engine values)", "scout_and_plan",
                       "plan_state", "expand_backup_compact(engine values)"]
    assert s.simulations == 3 and s.evaluator_calls == 1
    # new weights: the table is emptied before the next move's first selection and plan, once
    e.calls.clear()
    net.weights_version = 1
    e.plan_states = [1]
    s.begin_move()
    s.simulate(last=True)
    s.begin_move()
    assert e.calls == ["clear_cache", "select", "scout_and_plan", "plan_state", "expand_backup_compact(engine values)", "select", "scout_and_plan"]


def test_scouted_device_loop_runs_of_two_one_one():
    net, e, s = _scouted(True)
    assert s.device_loop
    e.plan_states = [0]
    e.outcomes = [(2, True), (1, False), (1, False)]
    s.begin_move()
    left = 4
    while left > 0:
        left -= s.run(left, left)
    assert e.calls == ["select", "scout_and_plan", "plan_state",
                       "set_run(4,4)", "ev", "gather_planned", "run", "run_outcome",
                       "set_run(2,2)", "ev", "gather_planned", "run", "run_outcome",
                       "set_run(1,1)", "run", "run_outcome"]
    assert s.simulations == 4 and s.evaluator_calls == 2
    e.calls.clear()
    net.weights_version = 1
    e.plan_states = [1, 1]
    s.begin_move()
    s.begin_move()
    assert e.calls == ["clear_cache", "select", "scout_and_plan", "plan_state", "select", "scout_and_plan", "plan_state"]


@pytest.mark.parametrize("planned", [True, False])
def test_wide_search_three_steps(planned, monkeypatch):
    from chinesechesszero_amd import wide
    monkeypatch.setattr(wide, "SelfPlayEngine", SeqEngine)
    net = Net()
    ws = wide.WideSearch(net.ev, 1, 4, n_playout=8, eval_cache_log2=12, planned=planned, use_graph=False)
    e = ws.engine
    net.calls = e.calls
    assert ws.planned == planned and not ws.use_graph and e.calls == ["set_width"]
    e.calls.clear()
    e.leaves = [4, 3, 1, 0]
    assert ws.search() == 3
    step = ["plan", "ev(plan)", "gather_planned", "step_wide(engine values)", "n_leaves"] if planned else ["ev", "gather", "step_wide", "n_leaves"]
    assert e.calls == ["set_budgets", "select_wide", "n_leaves"] + 3 * step
    assert ws.steps == ws.evaluator_calls == 3
    # new weights: the table is emptied before the next search's selection and plan, once
    e.calls.clear()
    net.weights_version = 1
    e.leaves = [2, 0, 0]
    assert ws.search() == 1 and ws.search() == 0
    assert e.calls == ["clear_cache", "set_budgets", "select_wide", "n_leaves"] + step + ["set_budgets", "select_wide", "n_leaves"]


def test_batched_self_play_clears_the_cache_once_when_the_weights_moved(monkeypatch):
    from chinesechesszero_amd import selfplay
    monkeypatch.setattr(selfplay, "SelfPlayEngine", SeqEngine)
    net = Net()
    sp = selfplay.BatchedSelfPlay(net.ev, 2, n_playout=3, eval_cache_log2=12)
    net.calls = sp.engine.calls
    assert sp.planned
    sp.advance(1)
    assert sp.engine.calls == ["select", "plan", "ev(plan)", "gather_planned", "step_compact(engine values)"]
    sp.engine.calls.clear()
    net.weights_version = 1
    sp.advance(2)
    assert sp.engine.calls == ["clear_cache", "plan", "ev(plan)", "gather_planned", "step_compact(engine values)",
                               "plan", "ev(plan)", "gather_planned", "expand_backup_compact(engine values)", "finish_move"]
    # simulate(): one simulation outside advance's bookkeeping, the same boundary
    sp.engine.calls.clear()
    sp.simulate()
    assert sp.engine.calls == ["select", "plan", "ev(plan)", "gather_planned", "expand_backup_compact(engine values)"]


@pytest.mark.parametrize("logits", [True, False])
def test_mcts_fused_move_without_scouts(logits, monkeypatch):
    from chinesechesszero_amd import mcts as M
    e = SeqEngine(1)

    def ev(leaf):
        e.calls.append("ev")
        return torch.zeros((1, 2086)), torch.zeros(1)
    ev.batched = True
    ev.returns_logits = logits
    m = M.MCTS(ev, 5, 3, scouts=0)
    assert m.scouts == 0
    m._engine = e
    monkeypatch.setattr(m, "_sync_root", lambda board: None)
    seen = []
    acts, probs = m.get_move_probs(None, temp=1.0, on_playout=seen.append)
    one = ["ev", "gather", "step_compact"] if logits else ["ev", "step"]
    last = ["ev", "gather", "expand_backup_compact"] if logits else ["ev", "expand_backup"]
    assert e.calls == ["select"] + 2 * one + last + ["root_children", "check_healthy"]
    assert seen == [1, 1, 1] and acts == (7, 9)
    # playout(): one simulation of the root on its own
    e.calls.clear()
    m.playout()
    assert e.calls == ["select"] + last


def test_arena_search_two_steps(monkeypatch):
    from chinesechesszero_amd import arena, engine
    monkeypatch.setattr(engine, "SelfPlayEngine", SeqEngine)
    monkeypatch.setattr(arena, "make_openings", lambda n, plies, seed=0, device=0: (np.zeros((n, 90), np.uint8), np.ones(n, np.uint8), np.zeros(n, np.int32)))
    a, b = Net(), Net()
    b.weights_version = 5
    ar = arena.Arena(a.ev, b.ev, 1, n_playout=2, eval_cache_log2=12)
    e = ar.engine
    a.calls = b.calls = e.calls
    ar.search()
    step = ["plan_routed", "ev(plan)", "ev(plan)", "gather_routed"]
    assert e.calls == ["set_routing", "select"] + step + ["step_compact(engine values)"] + step + ["expand_backup_compact(engine values)"]
    assert e.salts == arena.cache_salts(0, 5)
    # the routing is set again only when a network's version moved: that network alone gets a new salt
    e.calls.clear()
    ar.search()
    assert "set_routing" not in e.calls
    b.weights_version = 6
    ar.search()
    assert e.calls.count("set_routing") == 1 and e.salts == arena.cache_salts(0, 6)


def test_front_ends_die_with_their_last_reference(monkeypatch):
    """No front end refers to itself (a weights watch that held a bound method of its owner would): the engine, its device memory and
    any captured graph go when the last reference does, not when the cycle collector happens to run."""
    import gc
    import weakref
    from chinesechesszero_amd import mcts as M, selfplay, wide
    monkeypatch.setattr(selfplay, "SelfPlayEngine", SeqEngine)
    monkeypatch.setattr(wide, "SelfPlayEngine", SeqEngine)
    net = Net()
    net.calls = []
    gc.collect()
    gc.disable()
    try:
        sp = selfplay.BatchedSelfPlay(net.ev, 2, n_playout=2, eval_cache_log2=12)
        sp.run_move(on_playout=lambda k: sp.B)        # a callback that refers to the object is not kept past the call
        ws = wide.WideSearch(net.ev, 1, 4, n_playout=8, eval_cache_log2=12, planned=True)
        ws.engine.leaves = [0]
        ws.search()
        e = SeqEngine(11, eval_cache_log2=16)
        sc = selfplay.ScoutedSearch(e, net.ev, use_graph=False, device_loop=False)
        sc.begin_move()
        m = M.MCTS(net.ev, 5, 2, scouts=0)
        m._engine = SeqEngine(1)
        m._sync_root = lambda board: None
        m.get_move_probs(None, on_playout=lambda k: m.scouts)
        engines = [weakref.ref(x) for x in (sp.engine, ws.engine, e, m._engine)]
        del sp, ws, sc, e, m
        assert [r() for r in engines] == [None] * 4
    finally:
        gc.enable()
