"""Wide search: several leaves of ONE tree per evaluator call, kept apart by virtual loss (``include/cczero.h`` "Wide search").

The lockstep engine searches every board strictly sequentially: one leaf per board and step. That fills the chip at thousands of
boards; with a handful of positions (one game, a short analysis file) every step pays the evaluator's latency for a few rows.
``WideSearch`` turns an engine of ``n_positions * width`` slots into ``n_positions`` searched boards that each gather up to
``width`` leaves per step (``ccz_set_width``), sets every board's simulation budget to ``n_playout`` per move and loops

    plan -> evaluator on the planned rows -> gather -> step_wide -> read n_leaves

until no board selected a leaf. ``n_leaves`` lies in pinned host memory: one stream wait per step. The trees differ from the
sequential search's (virtual loss changes which leaves are visited); at width 1 nothing here is used.
"""
from __future__ import annotations

import torch

from .boundary import WeightsWatch, capture, describe, may_graph, need_version
from .engine import SelfPlayEngine
from .parameters import ALPHA, C_PUCT, EPS


class WideSearch:
    """``evaluator``: a batched evaluator that returns LOGITS (``returns_logits``; ``PolicyValueNet.evaluate_leaves_logits``, or
    any ``leaf fp16 [B,17,7,10,9] -> (logits [B,2086], value f32 [B])`` marked so). With ``eval_cache_log2 > 0`` and a
    plan-capable evaluator (``accepts_plan``) the loop can run on the planned boundary: slots that reach one position share a row,
    positions evaluated before cost none. ``planned``: None (default) plans from ``PLAN_MIN_SLOTS`` slots on; below, the whole
    batch is ONE latency-bound evaluator call on the small-batch convolution kernel (up to 64 rows cost what one costs), which the
    live-row kernels of a planned batch do not have: measured 3.6 ms against 0.5 ms per step at 8 .. 32 slots
    (profiles/wide_search.json). ``use_graph``: replay one step (evaluator, gather, ``step_wide``) as a hipGraph when the
    evaluator is ``graph_safe``."""

    PLAN_MIN_SLOTS = 65     # engines of up to 64 slots evaluate every row, every step (see ``planned``)

    def __init__(self, evaluator, n_positions: int, width: int, n_playout: int = 400, c_puct: float = C_PUCT, device: int = 0, seed: int = 0,
                 use_graph: bool = False, version_fn=None, warmup: int = 3, planned: bool | None = None, **engine_kw):
        ev = describe(evaluator, version_fn)
        if not callable(ev.fn) or not ev.returns_logits:
            raise ValueError("WideSearch: the evaluator must be batched and return logits (returns_logits; PolicyValueNet.evaluate_leaves_logits)")
        if int(n_positions) < 1 or not 2 <= int(width) <= 64 or int(n_playout) < 1:
            raise ValueError("WideSearch: n_positions and n_playout must be >= 1 and width in 2..64 (width 1 is the sequential search)")
        self.evaluator = ev.fn
        self.A, self.width, self.n_playout = int(n_positions), int(width), int(n_playout)
        engine_kw.setdefault("eps", EPS)
        engine_kw.setdefault("alpha", ALPHA)
        self.engine = SelfPlayEngine(self.A * self.width, n_playout=self.n_playout, c_puct=c_puct, device=device, seed=seed, **engine_kw)
        self.engine.set_width(self.width)
        can_plan = bool(self.engine.eval_cache_log2 > 0 and ev.accepts_plan)
        if planned and not can_plan:
            raise ValueError("WideSearch: planned=True needs eval_cache_log2 > 0 and an evaluator that accepts a plan")
        self.planned = can_plan and (self.engine.B >= self.PLAN_MIN_SLOTS if planned is None else bool(planned))
        if self.planned:
            need_version(ev, "WideSearch: ", planned=True)
        self._version, self._weights = ev.version, WeightsWatch(ev.version())
        self.use_graph = may_graph(use_graph, ev, self.engine.device)
        self.warmup = int(warmup)
        self._graph = None
        self._budgets = torch.zeros((self.engine.B,), dtype=torch.int32, device=self.engine.device)
        self._done = 0              # simulations every board has been given since its last move boundary
        self.steps = self.evaluator_calls = 0

    def _check_weights(self):
        if self._weights.moved(self._version()):     # cached evaluations (and captured addresses) of other weights must not reach the tree
            self.engine.clear_eval_cache()
            self._graph = None

    def _iteration(self):
        """Evaluate the pending slots and step: back them up, select the next ones."""
        e = self.engine
        if self.planned:
            logits, value = self.evaluator(e.leaf_input, plan=e.eval_plan())
            e.gather_priors_planned(logits, value)
            e.step_wide(None)
        else:
            logits, value = self.evaluator(e.leaf_input)
            e.gather_priors(logits, value)
            e.step_wide(value)

    def _replay(self):
        if self._graph is None:
            e = self.engine
            # warm-up in the form the capture uses (a plan of all rows: the engine's own plan is not touched)
            plan = (torch.arange(e.B, dtype=torch.int32, device=e.device), torch.full((1,), e.B, dtype=torch.int32, device=e.device))
            warm = (lambda: self.evaluator(e.leaf_input, plan=plan)) if self.planned else (lambda: self.evaluator(e.leaf_input))
            self._graph = capture(e.device, self._iteration, warm=warm, warmup=self.warmup)
        self._graph.replay()

    # ------------------------------------------------------------------ the search
    def boundary(self):
        """A move boundary happened on the engine (finish_move, reset, reset_tree, set_position[s]): budgets count from zero again."""
        self._done = 0

    def search(self, on_step=None) -> int:
        """``n_playout`` more simulations on every running board; returns the number of steps. ``on_step(n_leaves int32 [A])`` is
        called after every step's selection (the leaves about to be evaluated)."""
        e = self.engine
        self._check_weights()
        self._done += self.n_playout
        self._budgets.fill_(self._done)
        e.set_budgets(self._budgets)
        e.select_wide()
        steps = 0
        while True:
            nl = e.n_leaves()           # the one stream wait of the step
            if not nl.any():
                break
            if on_step is not None:
                on_step(nl)
            if self.use_graph:
                self._replay()
            else:
                self._iteration()
            steps += 1
        self.steps += steps
        self.evaluator_calls += steps
        return steps

    def finish_move(self, forced_moves=None, temps=None, keep_tree: bool = True) -> torch.Tensor:
        """``SelfPlayEngine.finish_move`` on the searched boards (entries past ``n_positions`` of a forced-move array are unused)."""
        self.boundary()
        return self.engine.finish_move(forced_moves=forced_moves, temps=temps, keep_tree=keep_tree)

    def summary(self) -> dict:
        ws = self.engine.wide_stats()
        return {"width": self.width, "steps": self.steps, "board_steps": ws["steps"], "leaves": ws["leaves"],
                "mean_leaves_per_step": round(ws["leaves"] / max(1, ws["steps"]), 3),
                "collision_share": round(ws["collisions"] / max(1, ws["steps"]), 4), "inflight_now": ws["inflight_now"]}
