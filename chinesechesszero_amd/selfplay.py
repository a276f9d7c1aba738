"""Lockstep batched self-play: the GPU-native form of reference collect.py:133-143 + game.py:133-237.

The reference plays ONE game at a time, one batch-1 net call per playout. Here B games advance in
lockstep: per simulation ``select_leaves -> evaluator -> expand_backup`` for all boards (the
evaluator is PyTorch-ROCm on the same stream), per move ``finish_move``; finished games are
harvested into (state, pi, z) rows and restart immediately.
"""
from __future__ import annotations

import os

import numpy as np

from .boundary import PlayoutTicker, WeightsWatch, capture, deliver, describe, kind_of, may_graph, need_history, need_version
from .engine import SelfPlayEngine
from .options import SearchOptions
from .parameters import ALPHA, C_PUCT, EPS
from .stopcfg import StopPoll


class GraphedStep:
    """hipGraph of one inner iteration ``evaluator(leaf) -> ccz_step`` (capture launch-bound loops in graphs).

    At B = 4096 a step is 47 ms of GPU work and launches do not matter; at small B (single-board play, UCI)
    the ~130 launches of a batch-1 forward are host-bound, and replaying one captured graph per simulation
    removes that. The evaluator must be capture-safe (no host sync, static shapes): the MIOpen find step and
    allocator warm-up therefore run eagerly on a side stream first.
    """

    def __init__(self, engine: SelfPlayEngine, evaluator, warmup: int = 3, version_fn=None):
        """``version_fn() -> hashable``: what tells this object that the evaluator's weights changed (a re-capture follows);
        default and lookup order: :func:`boundary.describe`. An evaluator nothing says that of is logged once: its graph can
        never notice a weight change."""
        self.engine = engine
        self.evaluator = evaluator
        self.warmup = warmup
        self.captures = 0
        self._ev = describe(evaluator, version_fn)
        need_version(self._ev, "GraphedStep: ", consequence="the captured hipGraph will keep replaying the weights it was captured "
                     "with (pass version_fn=... if they can change)")
        self._weights = WeightsWatch(self._ev.version())
        self._capture()

    def _capture(self):
        engine, ev = self.engine, self._ev
        need_history(engine, self.evaluator, "GraphedStep: ")
        self._history = engine.history_version   # (the captured launches are those of this setting: set_leaf_history moves it)
        # warm-up: the pending leaf is only evaluated, never stepped (and a stale inference copy is rebuilt OUTSIDE the capture,
        # which moves the version: it is read after that); capture does not execute: nothing is applied to the trees yet
        self.graph = capture(engine.device, lambda: deliver(engine, kind_of(ev), *ev.fn(engine.leaf_input), False),
                             warm=lambda: ev.fn(engine.leaf_input), warmup=self.warmup)
        self._weights.moved(ev.version())
        self.captures += 1

    def replay(self):
        if self._weights.moved(self._ev.version()) or self._history != self.engine.history_version:
            self._capture()  # weights changed since the capture (train_step / refresh_inference_copy / broadcast_model), or the step's launches did
        self.graph.replay()


class ScoutedSearch:
    """One game at a time with SCOUT SLOTS (``include/cczero.h`` ccz_scout; round 6). The reference's first-maximum rule makes the
    children of a node first-visited in ``legal_moves`` order (mcts.py:47-48,59-61), so the leaves the next simulations will ask
    for are known: the pending leaf's next siblings. The engine has ``1 + scouts`` boards; board 0 is searched, the scout slots
    carry those siblings through the evaluation cache. Per simulation: ``ccz_step_compact`` (expand + backup + select) ->
    ``ccz_scout`` -> probe + plan -> the HOST reads whether board 0's leaf is already in the table; only if it is not, the
    evaluator runs -- once, on all ``1 + scouts`` rows (latency-bound: 11 rows -- one round of blocks -- cost what 1 costs) -- and the scouts' results are
    stored for the simulations to come. Two hipGraphs (step + scout + plan; evaluator + gather), one stream sync per simulation.
    Same visit counts, bit for bit: the table returns what the evaluator returns for a position, and the evaluator's result for
    a row does not depend on the batch it sits in (tests/test_gpu_scouts.py)."""

    def __init__(self, engine: SelfPlayEngine, evaluator, version_fn=None, use_graph: bool = True, warmup: int = 3, device_loop=None):
        ev = describe(evaluator, version_fn)
        if not (ev.returns_logits and ev.batched):
            raise ValueError("scouts need a batched evaluator that returns logits (PolicyValueNet.evaluate_leaves_logits)")
        if getattr(engine, "n_scouts", 0) < 1:
            raise ValueError("the engine has no scout slots (SelfPlayEngine.set_scouts)")
        self.engine, self.evaluator, self._version = engine, ev.fn, ev.version
        self.use_graph = may_graph(use_graph, ev, engine.device)
        self.warmup = warmup
        need_version(ev, "ScoutedSearch: ", consequence="evaluations cached for other weights cannot be told apart (pass version_fn=... "
                     "if its weights can change)")
        self._weights = WeightsWatch(ev.version())
        self._g_step = self._g_eval = self._g_run = self._g_eval_run = None
        self.evaluator_calls = self.simulations = 0
        # simulations that hit the table are repeated ON THE DEVICE (ccz_scouted_run: one launch per evaluator call instead of two
        # launches, a replay and a stream sync per simulation); CCZ_SCOUT_DEVICE_LOOP=0: the host loop (:meth:`simulate`), for A/B
        self.device_loop = (os.environ.get("CCZ_SCOUT_DEVICE_LOOP", "1") != "0") if device_loop is None else bool(device_loop)
        self.device_loop = self.device_loop and engine.B <= 16
        self._need = True

    def _check_weights(self):
        if self._weights.moved(self._version()):        # cached evaluations (and captured addresses) of other weights must not reach the tree
            self.engine.clear_eval_cache()
            self._g_eval = self._g_eval_run = None

    def _warm(self):
        self.evaluator(self.engine.leaf_input)

    def _evaluate(self):
        e = self.engine
        logits, value = self.evaluator(e.leaf_input)
        e.gather_priors_planned(logits, value)

    def _do(self, name: str, body, warm=None):
        """``body()``: eagerly, or as a replay of the hipGraph kept in attribute ``name`` (captured when first needed)."""
        if not self.use_graph:
            return body()
        if getattr(self, name) is None:
            setattr(self, name, capture(self.engine.device, body, warm=warm, warmup=self.warmup))
        getattr(self, name).replay()

    def begin_move(self):
        """After a re-root / new position: select board 0's first leaf, scout, plan."""
        self._check_weights()
        self.engine.select_leaves()
        self.engine.scout_and_plan()
        if self.device_loop:
            self._need = self.engine.plan_state_of_board0() == 0

    def run(self, left: int, budget: int) -> int:
        """Up to ``budget`` simulations of the move (``left`` = how many it still has, the pending one included) with ONE launch
        sequence: the evaluator on all rows if board 0's pending leaf is not in the table, then ``ccz_scouted_run`` -- expand +
        backup, select, scout, probe, plan, again and again on the device until a leaf misses, the budget is used or the move's
        last simulation is backed up. Returns the number of simulations done (>= 1)."""
        e = self.engine
        e.set_run(min(budget, left), left)
        if self._need:
            self._do("_g_eval_run", lambda: (self._evaluate(), e.scouted_run_launch()), self._warm)
            self.evaluator_calls += 1
        else:
            self._do("_g_run", e.scouted_run_launch)
        done, self._need = e.run_outcome()
        if done < 1:
            raise RuntimeError("ccz_scouted_run reported no simulation")
        self.simulations += done
        return done

    def simulate(self, last: bool):
        """One simulation of board 0: the evaluator only if its pending leaf is not in the table; then expand + backup (+ the next
        selection, scouting and plan unless ``last``)."""
        e = self.engine
        if e.plan_state_of_board0() == 0:
            self._do("_g_eval", self._evaluate, self._warm)
            self.evaluator_calls += 1
        self.simulations += 1
        if last:
            e.expand_backup_compact(None)
        else:
            self._do("_g_step", lambda: (e.step_compact(None), e.scout_and_plan()))


class BatchedSelfPlay:
    """``evaluator(leaf_input fp16 [B,17,7,10,9]) -> (prob f32 [B,2086], value f32 [B])`` on the device."""

    def __init__(self, evaluator, n_boards: int, n_playout: int = 400, c_puct: float = C_PUCT, eps: float = EPS,
                 alpha: float = ALPHA, temp: float = 1.0, seed: int = 0, board_id_base: int = 0, device: int = 0,
                 sampling: str = "device", use_graph: bool = False, version_fn=None, playout_cap=None, resign=None,
                 root_exploration=None, solver: bool = False, gumbel=None, search=None, early_stop=None, surprise=None, leaf_history: bool = False,
                 **engine_kw):
        """``leaf_history``: the evaluator input of a leaf shows the eight positions a training row shows (:meth:`SelfPlayEngine.set_leaf_history`):
        the game's recorded plies, the root and the selection path. The evaluator must read all 17 plane groups and say so (a true
        ``leaf_history`` attribute, ``boundary.reads_history``); one that does not is refused here. Not with ``reference_quirks``. False: off.
        ``surprise``: True, a weight in [0, 1], or a dict of :meth:`SelfPlayEngine.set_surprise`'s arguments (``alpha``, ``cap``): policy
        surprise weighting -- the records of harvested games carry a sampling weight (``REC_WEIGHT``) that ``RecordReplayBuffer.sample(weighted=True)``
        draws by. Changes no search and no move; works with every other option and both sampling modes. None (default): off.
        ``early_stop``: a dict of :meth:`SelfPlayEngine.set_early_stop`'s arguments (``single_reply``, ``gap_factor``,
        ``kld_interval``, ``min_gain``, ``min_sims``; see :func:`stopcfg.make_early_stop`): a board stops searching its move when the
        outcome can no longer change or its visit distribution has stopped moving, and selects nothing for the rest of the move's
        ``n_playout`` lockstep steps (no evaluator row with an evaluation cache). None (default): off. (``options.SearchOptions``: what
        excludes what -- ``gumbel`` this and ``root_exploration`` --, and why ``resign``, ``root_exploration``, ``gumbel`` need device sampling.)
        ``search``: a dict of :meth:`SelfPlayEngine.set_search`'s arguments (``fpu_mode``, ``fpu_value``, ``fpu_root_mode``,
        ``fpu_root_value``, ``c_base``, ``c_factor``): first-play urgency and the visit-scaled c_puct inside the tree. Works with every
        other option here (under ``gumbel`` from depth 1). None (default): off, the reference's PUCT.
        ``gumbel``: True, or a dict of :meth:`SelfPlayEngine.set_gumbel`'s arguments (``n_sims`` defaults to ``n_playout``;
        ``max_considered``, ``c_visit``, ``c_scale``): Gumbel root search with sequential halving; pi' from the completed Q is the
        recorded policy target of every move, fast moves of ``playout_cap`` included (they still carry ``REC_FAST``). None / False: off.
        ``solver``: search with the MCTS-solver (:meth:`SelfPlayEngine.set_solver`). Only the search changes: moves are sampled,
        recorded and targeted as without it.
        ``playout_cap`` = ``(n_fast, p_full)``: playout-cap randomisation -- every move of every board is a full search of
        ``n_playout`` simulations with probability ``p_full``, else a fast one of ``n_fast``; fast plies carry ``REC_FAST`` in their
        record header so that a trainer can keep them out of the policy loss (``engine.draw_budgets``). The loop still runs
        ``n_playout`` lockstep steps per move: a board that has used its budget selects nothing for the rest of them, and on the
        planned boundary (``eval_cache_log2`` > 0 with a planning evaluator) it gets no evaluator row; an evaluator without a plan
        still computes all B rows. The budgets are drawn by :meth:`advance` (so by :meth:`search` and :meth:`run_move`) at a move's
        first simulation; :meth:`simulate` draws nothing and searches with the budgets the engine holds.
        None (default): every board searches ``n_playout`` simulations, as ever.
        ``resign``: a threshold in [-1, 0], or a dict of :meth:`SelfPlayEngine.set_resign`'s arguments (``threshold``,
        ``consecutive``, ``min_ply``, ``p_playon``): self-play resignation with play-on calibration. None (default): off.
        ``root_exploration``: a dict of :meth:`SelfPlayEngine.set_root_exploration`'s arguments (``eps``, and optionally ``alpha``,
        ``forced_k``, ``prune_targets``): the Dirichlet noise acts on the root's priors inside the search, with forced playouts and
        policy target pruning, on full-search moves; fast moves of ``playout_cap`` are left alone. None (default): off.
        ``version_fn() -> hashable``: what tells the evaluation cache (and a captured hipGraph) that the evaluator's weights
        changed; default: ``weights_version`` of the evaluator's owner. An evaluator that accepts a plan but exposes neither is
        refused: its cached evaluations could never be invalidated."""
        if sampling not in ("device", "numpy"):
            raise ValueError("sampling must be 'device' (Philox on the GPU) or 'numpy' (reference-exact host RNG)")
        self.options = o = SearchOptions(n_playout, sampling, resign=resign, root_exploration=root_exploration, gumbel=gumbel, solver=solver,
                                         search=search, early_stop=early_stop, surprise=surprise, leaf_history=leaf_history)       # (ValueError: what excludes what)
        (self.resign, self.root_exploration, self.gumbel, self.solver, self.search_cfg, self.early_stop, self.surprise,
         self.leaf_history) = o.keywords().values()
        self.leaf_history = self.leaf_history is not None
        self.playout_cap = None
        if playout_cap is not None:
            n_fast, p_full = playout_cap
            if int(n_fast) != n_fast or not 1 <= int(n_fast) <= int(n_playout):
                raise ValueError(f"playout_cap: n_fast must be an integer in 1..n_playout (got {n_fast})")
            if not 0.0 <= float(p_full) <= 1.0:
                raise ValueError(f"playout_cap: p_full must be in [0, 1] (got {p_full})")
            self.playout_cap = (int(n_fast), float(p_full))
        self.evaluator = evaluator
        self.engine = SelfPlayEngine(n_boards, n_playout=n_playout, c_puct=c_puct, eps=eps, alpha=alpha, temp=temp,
                                     seed=seed, board_id_base=board_id_base, device=device, **engine_kw)
        o.apply(self.engine)
        need_history(self.engine, evaluator, "BatchedSelfPlay: ")   # (at every evaluation too: the evaluator can be swapped, the option set later)
        self.B = n_boards
        self.n_playout = n_playout
        self.sampling = sampling
        self.eps, self.alpha, self.temp = eps, alpha, temp
        # reference-exact host sampling: one legacy RandomState per board (mcts.py:216-224 uses the global one)
        self.rngs = [np.random.RandomState((seed + board_id_base + b) % (2**32)) for b in range(n_boards)] if sampling == "numpy" else None
        self.use_graph = use_graph
        self._graph = None
        # planned evaluator boundary: the engine holds an evaluation cache (eval_cache_log2 > 0) and the evaluator can compute a
        # planned subset of the rows (PolicyValueNet.evaluate_leaves_logits): positions evaluated before are not sent through
        # the network again (include/cczero.h ccz_eval_plan). Same results, bit for bit.
        ev = describe(evaluator, version_fn)
        self.planned = bool(self.engine.eval_cache_log2 > 0 and ev.accepts_plan and ev.returns_logits)
        self.version_fn = version_fn
        if self.planned:
            need_version(ev, planned=True)
        # (``evaluator`` and ``planned`` stay plain attributes read at every call -- bench.py swaps a stub in and out --: the version
        # is asked of whatever evaluator is current)
        self._weights = WeightsWatch(self._evaluator_version())
        self._sim = 0        # simulations done of the current move
        self._leaf = None    # the pending leaf batch (None: the next simulation starts with select_leaves)
        self._ticker = PlayoutTicker(n_playout)

    def _evaluator_version(self):
        """What tells the evaluation cache that the evaluator's weights changed (:func:`boundary.describe`)."""
        return describe(self.evaluator, self.version_fn).version()

    @property
    def _cache_version(self):
        return self._weights.seen

    @_cache_version.setter
    def _cache_version(self, v):
        self._weights.seen = v

    def _planned_eval(self, leaf):
        """(logits, value) of the planned rows; cached evaluations of other weights are dropped first."""
        e = self.engine
        if self._weights.moved(self._evaluator_version()):
            e.clear_eval_cache()
        return self.evaluator(leaf, plan=e.eval_plan())

    def _evaluate(self, leaf):
        """``(boundary kind, outputs, value)`` of the pending leaf batch from the evaluator that is current."""
        need_history(self.engine, self.evaluator, "BatchedSelfPlay: ")
        if self.planned:   # cache probe + plan, the network on the planned rows only
            return ("planned", *self._planned_eval(leaf))
        return (kind_of(self.evaluator), *self.evaluator(leaf))

    # one lockstep simulation of every board (outside advance's move bookkeeping: no playout-cap draw happens here)
    def simulate(self):
        deliver(self.engine, *self._evaluate(self.engine.select_leaves()), True)

    def advance(self, steps: int, hooks=None, boundary=None, on_playout=None):
        """``steps`` lockstep simulations of every board from wherever the search stands in its move; a move that completes on the
        way (simulation ``n_playout``) is played: ``boundary()`` if given (it must call :meth:`finish_move` itself -- bench.py wraps
        the harvest / exchange and its timers around it), else :meth:`finish_move`. Returns the moves of the last move played in
        this call (device int32 [B]) or None.

        Launch sequence of a move: select, (evaluator, fused step) x (n-1), evaluator, expand_backup -- with an evaluation cache:
        (probe + plan, evaluator on the planned rows, softmax + gather + store, fused step).
        ``hooks(stage, sim)`` -- stage "eval0" / "eval1" / "step1" = before the evaluator, between evaluator and simulator
        kernel, after the simulator kernel of simulation index ``sim`` (0-based within its move): where bench.py records its HIP
        events and triggers the concurrent trainer. THE loop: ``run_move``, the bench, the soak and the tests all run this one."""
        e = self.engine
        n = self.n_playout
        self._ticker.on_playout = on_playout
        between = None if hooks is None else lambda: hooks("eval1", self._sim)
        moves = None
        for _ in range(int(steps)):
            i = self._sim
            last = i + 1 == n
            if self._leaf is None:
                if self.playout_cap is not None and i == 0:   # the move's budgets, after a harvest restarted boards
                    e.draw_budgets(n, *self.playout_cap)
                self._leaf = e.select_leaves()
                # (not boundary.may_graph: this front end captures whatever it is given when asked to -- bench.py --graph captures a
                # stub that is not marked graph_safe, and tests/test_gpu_above_4096_boards.py expects a graph exactly when use_graph)
                if self.use_graph and self._graph is None and not self.planned:
                    self._graph = GraphedStep(e, self.evaluator, version_fn=self.version_fn)
            if hooks is not None:
                hooks("eval0", i)
            if self._graph is not None and not last and hooks is None:
                self._graph.replay()   # evaluator + fused step as one captured graph (launch-bound small batches)
            else:
                self._leaf = deliver(e, *self._evaluate(self._leaf), last, between)
            if hooks is not None:
                hooks("step1", i)
            self._sim = 0 if last else i + 1
            self._ticker.tick(1, last)
            if last:
                moves = boundary() if boundary is not None else self.finish_move()
        self._ticker.on_playout = None   # (the caller's callback is not kept past the call: it may refer to this object)
        return moves

    def search(self, on_playout=None, hooks=None, poll: bool = False):
        """The simulations that are left of the current move (all ``n_playout`` from a move's start) WITHOUT playing it: the roots
        can be read (``engine.root_children()``) before :meth:`finish_move`. ``poll`` (an arg-max front end with ``early_stop``):
        ``engine.searching()`` is asked every ``stopcfg.POLL_EVERY`` steps and the move's loop ends when no board would select any more."""
        stop = StopPoll(self.engine, self.early_stop if poll and self._graph is None else None)
        while stop.on and self.n_playout - self._sim > 1:
            if stop.done(self._sim):   # (no leaf is pending either)
                self._sim, self._leaf, self._ticker.acc = 0, None, 0
                return
            self.advance(1, hooks=hooks, on_playout=on_playout)
        left = self.n_playout - self._sim
        if left > 1:
            self.advance(left - 1, hooks=hooks, on_playout=on_playout)
        self.advance(1, hooks=hooks, on_playout=on_playout, boundary=lambda: None)

    def run_move(self, on_playout=None):
        """n_playout simulations then one move on every board. Returns the moves (device int32 [B])."""
        return self.advance(self.n_playout - self._sim, on_playout=on_playout)

    def watch(self, board_index: int, viewer):
        """Show ONE selected board of the batch in a viewer (``examples/viewer.py``'s ``ChessWindow`` or anything with
        ``update_board(svg, status)``): its position is pushed after every move (one small device read per move; nothing is
        read when no board is watched). The batched counterpart of ``Game.graphic`` (reference game.py:47-75)."""
        self._watch = (int(board_index), viewer)

    def _show(self, moves):
        b, viewer = self._watch
        from .boardsvg import board_svg
        from .tools import MOVE_FROM, MOVE_TO
        sq = self.engine.root_positions()[b]
        st = self.engine.game_status()
        mv = int(moves[b].item())
        lm = (int(MOVE_FROM[mv]), int(MOVE_TO[mv])) if mv >= 0 else None
        viewer.update_board(board_svg(sq, lm), f"board {b} - to move: {'red' if st['turn'][b] else 'black'} - ply: {int(st['plies'][b])}"
                            + (" - game over" if st["over"][b] else ""))

    def finish_move(self):
        self._sim, self._leaf, self._ticker.acc = 0, None, 0   # whatever leaf was pending belongs to the old root
        moves = self._finish_move()
        if getattr(self, "_watch", None) is not None:
            self._show(moves)
        return moves

    def _finish_move(self):
        e = self.engine
        if self.sampling == "device":
            return e.finish_move()
        # reference-exact: pi by the reference's own NumPy formula, Dirichlet + choice from legacy MT19937
        rc = e.root_children()
        st = e.game_status()
        forced = np.full(self.B, -1, np.int32)
        temps = np.ones(self.B, np.float64)
        for b in range(self.B):
            if st["over"][b]:
                continue
            k = int(rc["k"][b])
            temp = self.temp if (st["plies"][b] + 1) <= 30 else max(0.1, self.temp * 0.5)  # game.py:159
            temps[b] = temp
            visits = rc["visits"][b][:k].astype(np.int64)
            x = 1.0 / temp * np.log(visits + 1e-10)
            probs = np.exp(x - np.max(x))
            probs /= np.sum(probs)
            rs = self.rngs[b]
            p = (1 - self.eps) * probs + self.eps * rs.dirichlet(self.alpha * np.ones(k))
            forced[b] = int(rs.choice(rc["acts"][b][:k].astype(np.int64), p=p))
        return e.finish_move(forced_moves=forced, temps=temps)

    # ------------------------------------------------------------------ snapshots (include/cczero.h "Engine snapshots")
    def _need_move_boundary(self, what: str):
        if self._sim != 0 or self._leaf is not None:
            raise RuntimeError(f"{what}: the search stands inside a move ({self._sim} of {self.n_playout} simulations done, "
                               f"{'a' if self._leaf is not None else 'no'} leaf pending): a snapshot is taken at a move boundary, after finish_move")

    def state_dict(self) -> dict:
        """Everything that decides what this object does next, at a move boundary (after :meth:`finish_move` / :meth:`run_move`, before
        or after the harvest; RuntimeError inside a move): the engine's snapshot (``engine.save_state()``: a uint8 device tensor),
        the playout ticker, and under ``sampling="numpy"`` the per-board ``RandomState``s. The playout-cap draws have no host side:
        they come from the boards' Philox streams, which the engine's snapshot carries. ``torch.save`` takes the dict as it is."""
        self._need_move_boundary("state_dict")
        return {"engine": self.engine.save_state(), "ticker_acc": int(self._ticker.acc), "sampling": self.sampling,
                "n_playout": int(self.n_playout), "playout_cap": self.playout_cap, "leaf_history": bool(self.engine.leaf_history),
                "rngs": None if self.rngs is None else [r.get_state() for r in self.rngs]}

    def load_state_dict(self, state: dict, keep_board_id_base: bool = False):
        """Continue from :meth:`state_dict` of an object built with the same arguments (the engine's load is strict: ``CczError`` names
        what differs, and nothing has changed then). The evaluation cache starts cold and its weights version is re-read from the
        evaluator that is current."""
        self._need_move_boundary("load_state_dict")
        for name, mine in (("sampling", self.sampling), ("n_playout", int(self.n_playout)), ("playout_cap", self.playout_cap)):
            theirs = state[name]
            if (tuple(theirs) if isinstance(theirs, (list, tuple)) else theirs) != mine:
                raise ValueError(f"load_state_dict: {name} differs: the state has {theirs!r}, this object {mine!r}")
        if bool(state.get("leaf_history", False)) != bool(self.engine.leaf_history):   # (a state from before the option: off)
            raise ValueError(f"load_state_dict: leaf_history differs: the state has {bool(state.get('leaf_history', False))}, this object "
                             f"{bool(self.engine.leaf_history)}: the rows and cache keys of the two settings are not the same search")
        if (state["rngs"] is None) != (self.rngs is None) or (self.rngs is not None and len(state["rngs"]) != len(self.rngs)):
            raise ValueError("load_state_dict: the per-board RandomStates of the state do not match this object's boards")
        self.engine.load_state(state["engine"], keep_board_id_base=keep_board_id_base)
        if self.rngs is not None:
            for r, s in zip(self.rngs, state["rngs"]):
                r.set_state(s)
        self._sim, self._leaf, self._ticker.acc = 0, None, int(state["ticker_acc"])
        self._weights.seen = self._evaluator_version()   # the load cleared the cache: what it holds from here on is of these weights

    def harvest(self):
        return self.engine.harvest()

    def harvest_chunks(self, max_rows: int = 1 << 19):
        return self.engine.harvest_chunks(max_rows)

    def harvest_record_chunks(self, max_plies: int = 1 << 16):
        """Finished games as compact ply records (the exchange format, ``replay.RecordGatherer``)."""
        return self.engine.harvest_record_chunks(max_plies)
