"""Host mirror of reference mcts.py: ``MCTS`` and ``MCTS_AI`` with the reference's call surface,
backed by the HIP lockstep engine (one board per player object).

Same constructor arguments, methods and return conventions as reference mcts.py:81-233, so
``Game.start_self_play(player)`` and the reference's own call sites read unchanged. The tree lives
in device memory; ``Node`` objects do not exist on the host. pi and the move choice follow the
reference's NumPy code literally (softmax(1/temp*log(N+1e-10)), global ``np.random`` Dirichlet +
choice), so under ``np.random.seed`` a single game reproduces the reference's moves.

Evaluator forms accepted as ``policy_value_fn``:
  * a callable with attribute ``batched = True`` taking the fp16 leaf tensor [B,17,7,10,9] on the
    device and returning ``(prob float32 [B,2086], value float32 [B])`` (the fast path; e.g.
    ``PolicyValueNet.evaluate_leaves``),
  * ``PolicyValueNet.policy_value_fn`` (bound method): routed to ``evaluate_leaves`` of the same object,
  * any reference-style ``f(board) -> (iterable[(move_id, prob)], value)`` (compatibility path: the
    leaf is handed to ``f`` as a light ``LeafView``; one device round trip per playout).
"""
from __future__ import annotations

import numpy as np
import torch

from .boundary import PlayoutTicker, deliver, describe, kind_of, may_graph
from .engine import SelfPlayEngine
from .options import SearchOptions
from .parameters import ALPHA, C_PUCT, EPS
from .searchcfg import resolve_scouts
from .selfplay import GraphedStep, ScoutedSearch
from .tools import softmax


class LeafView:
    """What a reference-style evaluator may ask of the leaf board (net.py:151-177)."""

    def __init__(self, squares: np.ndarray, turn: bool, ids: list[int]):
        self._sq = squares
        self.turn = turn
        self._ids = ids

    def squares(self):
        return self._sq.copy()

    def legal_ids(self):
        return list(self._ids)

    @property
    def legal_moves(self):
        from .game import Move
        return [Move.from_id(i) for i in self._ids]

    def piece_at(self, square):
        from .game import Piece
        pc = int(self._sq[square])
        return Piece(pc & 7, not bool(pc & 8)) if pc else None


def _planes_to_squares(planes: np.ndarray):
    from . import tools
    p = planes.reshape(17, 7, 90)
    types = np.zeros(7, np.int64)
    for t in range(1, 8):
        types[tools.PLANE_OF_TYPE[t]] = t   # channel -> piece type
    types = types.reshape(7, 1)
    return ((p[7] * types).sum(0) + (p[15] * (types + 8)).sum(0)).astype(np.uint8), bool(p[16, 0, 0] > 0)


SCOUTS = 10  # scout slots of a one-game search (ScoutedSearch): 1 + 10 = 11 rows = 990 pixels = 16 x 16 blocks of k_conv3x3_small = ONE round of the 256
             # CUs, at the price of one row (7.0 against 6.5 us per tower layer), and an evaluator call answers 4.2 simulations on average: 6,000
             # sims/s against 5,626 with 7 and 3,494 with 15 (a second round of blocks); profiles/r06_single_board.json. env CCZ_SCOUTS, 0 = off


class MCTS:
    def __init__(self, policy_value_fn, c_puct=5, n_playout=10000, device: int = 0, seed: int = 0, scouts: int | None = None,
                 solver: bool = False, search=None, width: int | None = None, lcb=None, mate_search=None):
        """``mate_search``: plies, or the dict of ``options.make_mate_search``: :meth:`mate_move` then looks for a forced mate by
        consecutive checks from a board's position (``SelfPlayEngine.mate_search``: no evaluator call).
        ``lcb``: keep the value spread of every node (``SelfPlayEngine.set_value_stats``) so that :meth:`lcb_move` can name the
        lower-confidence-bound move (``options.MOVE_OPTIONS``: True, a multiple z of the standard error, or a dict); not with ``width`` > 1.
        ``width``: None / 1 (default): the sequential search, scouted as below. 2..64: the wide search (``wide.WideSearch``): up to
        ``width`` leaves of the tree per evaluator call, kept apart by virtual loss -- another tree than the reference's; needs a
        batched evaluator that returns logits, and excludes ``scouts`` > 0, ``solver`` and ``search`` (ValueError).
        ``search``: a dict of ``SelfPlayEngine.set_search``'s arguments (first-play urgency, visit-scaled c_puct). Scout slots rest
        on children being first visited in legal-move order, which the rule ends: with ``search`` given and ``scouts`` None the search
        runs with ``scouts=0``; both given explicitly raise ValueError.
        ``scouts``: scout slots of the one-game search (``selfplay.ScoutedSearch``; same visit counts, fewer evaluator calls);
        None = ``SCOUTS`` (env ``CCZ_SCOUTS``) when the evaluator is a batched one that returns logits, else 0. ``solver``: the
        MCTS-solver (``SelfPlayEngine.set_solver``): decided positions are proven in the tree, :meth:`proof_move` names the move
        a proven root asks for."""
        self.policy = policy_value_fn
        self.width = 1 if width is None else int(width)
        if not 1 <= self.width <= 64:
            raise ValueError(f"width must be in 1..64 (got {width})")
        self.options = SearchOptions(n_playout, width=self.width, solver=solver, search=search, lcb=lcb, mate_search=mate_search)
        self.solver, self.search_cfg, self.lcb = self.options.keywords().values()
        self.mate_search = self.options.mate_search
        if self.width > 1 and scouts:
            raise ValueError("width > 1 (the wide search) excludes scouts")
        self._wide = None
        scouts = 0 if self.width > 1 else resolve_scouts(self.search_cfg, scouts)
        self.c_puct = c_puct
        self.n_playout = n_playout
        self.red_history = None
        self.black_history = None
        self._device = device
        self._seed = seed
        self._engine: SelfPlayEngine | None = None
        self._synced: list[int] | None = None   # move ids pushed on the engine since its start position
        self._start = None
        self._discard = False
        self._graph = None
        self.use_graph = True   # single-board play is launch-bound: replay (evaluator, k_step) as one hipGraph
        # (the module docstring's forms: batched as it is, policy_value_fn routed to its object's batched one, else a callback: _ev None)
        owner = getattr(policy_value_fn, "__self__", None)
        ev = describe(policy_value_fn)
        if not ev.batched and hasattr(owner, "evaluate_leaves") and getattr(policy_value_fn, "__name__", "") == "policy_value_fn":
            ev = describe(getattr(owner, "evaluate_leaves_logits", owner.evaluate_leaves))
        self._ev = ev if ev.batched else None
        self._kind = kind_of(self._ev)
        import os
        want = int(os.environ.get("CCZ_SCOUTS", SCOUTS)) if scouts is None else int(scouts)
        ok = self._ev is not None and ev.returns_logits
        self.scouts = max(0, min(want, 63)) if ok else 0
        if self.width > 1:
            if not ok:
                raise ValueError("width > 1 (the wide search) needs a batched evaluator that returns logits (PolicyValueNet.policy_value_fn)")
            self.scouts = 0
        self._scouted = None

    # ---- engine management -----------------------------------------------------------------------
    def _ensure_engine(self):
        if self._engine is None and self.width > 1:
            # one searched board, `width` slots for its pending leaves: every step is one evaluator call on all (at most 64) rows
            from .wide import WideSearch
            self._wide = WideSearch(self._ev.fn, 1, self.width, n_playout=max(1, self.n_playout), c_puct=self.c_puct, device=self._device,
                                    seed=self._seed, use_graph=self.use_graph, mirror=True, strict=True)
            self._engine = self._wide.engine
        if self._engine is None:
            # board 0 is the game; the scout slots behind it (no tree, no game of their own) carry the leaves board 0 will ask for next
            # through a small evaluation cache (2^16 positions, 34 MB)
            self._engine = SelfPlayEngine(1 + self.scouts, n_playout=max(1, self.n_playout), c_puct=self.c_puct, eps=EPS, alpha=ALPHA,
                                          device=self._device, seed=self._seed, mirror=True, eval_cache_log2=16 if self.scouts else 0,
                                          strict=True)   # the reference's tree and game are unbounded: a prune or an adjudication raises here
            if self.scouts:
                self._engine.set_scouts(self.scouts)
            self.options.apply(self._engine)
        return self._engine

    def _forced(self, mid: int):
        f = np.full(self._engine.B, -1, np.int32)   # (the scout slots are not played: the simulator kernels run on board 0 only)
        f[0] = int(mid)
        return f

    def _sync_root(self, board):
        """Make the engine's root the position of ``board`` (same move history => same repetition state)."""
        e = self._ensure_engine()
        ids = [m.id for m in board.move_stack]
        start = board._start
        same_start = self._start is not None and np.array_equal(self._start[0], start[0]) and self._start[1:] == start[1:]
        if not same_start or self._synced is None or ids[:len(self._synced)] != self._synced:
            e.set_position(0, start[0], 1 if start[1] else 0, start[2])
            self._boundary()
            self._start = (start[0].copy(), start[1], start[2])
            self._synced = []
            self._discard = False
        new = ids[len(self._synced):]
        for mid in new:
            e.finish_move(forced_moves=self._forced(mid), keep_tree=not self._discard)
            self._boundary()
            self._synced.append(mid)
        if self._discard and not new:
            self._reset_tree_keep_position(board)
        self._discard = False
        assert np.array_equal(e.root_positions()[0], board.squares()), "engine root out of sync with the board"

    def _reset_tree_keep_position(self, board):
        # Node(None, 1.0) (mcts.py:176-178): one launch; position, history chain and clocks stay on the engine
        self._engine.reset_tree()
        self._boundary()
        self._discard = False

    def _boundary(self):
        if self._wide is not None:
            self._wide.boundary()   # the board's simulation count starts over: the next search is n_playout simulations again

    # ---- reference surface ------------------------------------------------------------------------
    def _callback(self, leaf, red_states, black_states):
        """The compatibility path: the leaf goes to the reference-style ``f(board)`` as a ``LeafView``; (prob, value) on the device."""
        e = self._engine
        info = e.leaf_info()
        sq, turn = _planes_to_squares(leaf[0].float().cpu().numpy())
        k = int(info["k"][0])
        view = LeafView(sq, turn, info["ids"][0][:k].astype(np.int64).tolist())
        act_probs, leaf_value = self.policy(view, red_states, black_states)
        p = np.zeros((1, 2086), np.float32)
        for a, pr in act_probs:
            p[0, int(a)] = np.float32(pr)
        return torch.from_numpy(p).to(e.device), torch.from_numpy(np.asarray(leaf_value, np.float32).reshape(1)).to(e.device)

    def playout(self, board=None, red_states=None, black_states=None):
        """One simulation (mcts.py:101-129) of the engine's root."""
        e = self._ensure_engine()
        leaf = e.select_leaves()
        deliver(e, self._kind, *(self._ev.fn(leaf) if self._ev is not None else self._callback(leaf, red_states, black_states)), True)

    def get_move_probs(self, board, temp=1e-3, red_states=None, black_states=None, on_playout=None):
        """mcts.py:131-166: run n_playout simulations, return (acts, probs) over the root's children."""
        self.red_history = red_states
        self.black_history = black_states
        self._sync_root(board)
        self._strategy()(PlayoutTicker(self.n_playout, on_playout))
        return self._root_probs(temp)

    def _strategy(self):
        """How this object searches a move: one of the ``_search_*`` methods below (each takes the move's ``PlayoutTicker``)."""
        if self._wide is not None:
            return self._search_wide
        if self._ev is None:
            return self._search_callback
        if not self.scouts:
            return self._search_fused
        if self._scouted is None:
            self._scouted = ScoutedSearch(self._engine, self._ev.fn, use_graph=self.use_graph)
        return self._search_scouted_device if self._scouted.device_loop else self._search_scouted_host

    def _search_wide(self, ticker):
        # every step backs up and selects up to `width` leaves; on_playout sees the leaves of each step
        self._wide.search(on_step=lambda nl: ticker.tick(int(nl[0])))
        ticker.tick(0, last=True)

    def _search_callback(self, ticker):
        for i in range(self.n_playout):
            self.playout(None, self.red_history, self.black_history)
            ticker.tick(1, i + 1 == self.n_playout)

    def _search_scouted_device(self, ticker):
        # one game at a time with scout slots: the evaluator runs only when board 0's leaf is not in the table yet, on 1 + scouts rows.
        # Simulations that find their leaf in the table repeat on the device (ccz_scouted_run): the host sees the search when the
        # evaluator has to run -- and at the playouts on_playout is due at, the same ones as in the host loop
        self._scouted.begin_move()
        left = self.n_playout
        while left > 0:
            done = self._scouted.run(left, ticker.room(left))
            left -= done
            ticker.tick(done, left == 0)

    def _search_scouted_host(self, ticker):
        self._scouted.begin_move()
        for i in range(self.n_playout):
            self._scouted.simulate(last=i + 1 == self.n_playout)
            ticker.tick(1, i + 1 == self.n_playout)

    def _search_fused(self, ticker):
        # launch sequence of a move: select, (evaluator, fused step) x (n-1), evaluator, expand_backup; the inner iteration replayed
        # as one hipGraph where that may be
        e, ev = self._engine, self._ev
        leaf = e.select_leaves()
        if self._graph is None and may_graph(self.use_graph, ev, e.device):
            self._graph = GraphedStep(e, ev.fn)
        for i in range(self.n_playout):
            last = i + 1 == self.n_playout
            if self._graph is not None and not last:
                self._graph.replay()
            else:
                leaf = deliver(e, self._kind, *ev.fn(leaf), last)
            ticker.tick(1, last)

    def _root_probs(self, temp):
        rc = self._engine.root_children()
        self._engine.check_healthy()
        k = int(rc["k"][0])
        acts = tuple(int(a) for a in rc["acts"][0][:k])
        visits = rc["visits"][0][:k].astype(np.int64)
        act_probs = softmax(1.0 / temp * np.log(np.array(visits) + 1e-10))
        return acts, act_probs

    def update_with_move(self, last_move):
        """mcts.py:168-178: keep the subtree of ``last_move``; -1 (or an unknown move) starts a fresh root."""
        if last_move == -1 or self._engine is None or self._synced is None:
            self._discard = True
            return
        self._engine.finish_move(forced_moves=self._forced(last_move), keep_tree=True)
        self._boundary()
        self._synced.append(int(last_move))

    def root_children(self):
        rc = self._ensure_engine().root_children()
        k = int(rc["k"][0])
        return {key: (val[0][:k] if val.ndim == 2 else val[0]) for key, val in rc.items()}

    def root_proof(self):
        """``SelfPlayEngine.root_proof`` of the game's board: ``state`` / ``dist`` of the root, ``child_state`` / ``child_dist`` [k]."""
        e = self._ensure_engine()
        k = int(e.root_children()["k"][0])
        return {key: (val[0][:k] if val.ndim == 2 else val[0]) for key, val in e.root_proof().items()}

    def proof_move(self):
        """The move id a proven root asks for (``engine.proof_move``: the fastest mate, or the longest defence), or None."""
        if not self.solver or self._engine is None:
            return None
        from .engine import proof_move
        rp, rc = self._engine.root_proof(), self._engine.root_children()
        return proof_move(rp["state"][0], rp["dist"][0], rp["child_state"][0], rp["child_dist"][0], rc["acts"][0])


    def mate_move(self, board, cfg=None):
        """``(move id, dist in plies, nodes)`` of the forced mate by consecutive checks from ``board``'s position, or None: the option
        is off (and no ``cfg`` is given), the game is over, or the search found none. ``cfg``: settings for this one call
        (``options.make_mate_search``). The engine's root is synced to the board first; no evaluator call is made."""
        cfg = self.mate_search if cfg is None else cfg
        if cfg is None:
            return None
        self._sync_root(board)
        res = self._engine.mate_search(cfg["max_plies"], cfg["node_budget"])
        c = self.options.mate_counts
        c["boards"] += int(res["state"][0] != 0)
        c["mates"] += int(res["state"][0] == 1)
        c["nodes"] += int(res["nodes"][0])
        self.last_mate_nodes = int(res["nodes"][0])
        if int(res["state"][0]) != 1:
            return None
        return int(res["move"][0]), int(res["dist"][0]), int(res["nodes"][0])

    def lcb_move(self):
        """The move id the LCB rule plays at the root (``SelfPlayEngine.lcb_moves`` with this search's ``lcb`` settings), or None:
        the option is off, nothing was searched, or the game is over."""
        if self.lcb is None or self._engine is None:
            return None
        mv = int(self._engine.lcb_moves(self.lcb["z"], self.lcb["min_visit_ratio"], self.lcb["min_visits"])[0].item())
        return mv if mv >= 0 else None


class MCTS_AI:
    """reference mcts.py:181-233"""

    def __init__(self, policy_value_fn, c_puct=5, n_playout=2000, is_selfplay=False, device: int = 0, seed: int = 0, scouts: int | None = None,
                 solver: bool = False, search=None, width: int | None = None, lcb=None, mate_search=None):
        """``mate_search``: as in :class:`MCTS`; :meth:`get_action` then runs the mate search before the playouts and, where it finds a
        forced mate, returns its first move (``return_prob``: one-hot) without any evaluator call; ``last_mate`` holds (move, dist, nodes)
        of that move, None after a searched one.
        ``lcb``: as in :class:`MCTS`; a match player (``is_selfplay`` False) then plays :meth:`MCTS.lcb_move` instead of drawing from
        the visit counts at temperature ``temp`` (a proven move wins over it; the self-play branch is untouched).
        ``width``: as in :class:`MCTS` (None / 1: the scouted sequential search; 2..64: the wide search).
        ``search``: as in :class:`MCTS` (with it, ``scouts`` None means 0 and ``scouts`` > 0 raises ValueError).
        ``solver``: search with the MCTS-solver and play the proven move when the root is decided (the fastest mate, the longest
        defence) instead of drawing from the visit counts."""
        self.mcts = MCTS(policy_value_fn, c_puct, n_playout, device=device, seed=seed, scouts=scouts, solver=solver, search=search, width=width, lcb=lcb,
                         mate_search=mate_search)
        self.last_mate = None
        self.is_selfplay = is_selfplay
        self.agent = "AI"

    def set_player_idx(self, p):
        self.player = p

    def reset_player(self):
        self.mcts.update_with_move(-1)

    def get_action(self, board, temp=1e-3, return_prob=False, on_playout=None, mate_search=None):
        """``mate_search``: the mate search's settings for this one call (``options.make_mate_search``; None: the player's own)."""
        move_probs = np.zeros(2086)
        self.last_mate = self.mcts.mate_move(board, mate_search)
        if self.last_mate is not None:       # a forced mate by checks: played as it is, no playout, no evaluator call
            move = self.last_mate[0]
            move_probs[move] = 1.0
            self.mcts.update_with_move(move if self.is_selfplay else -1)
            return (move, move_probs) if return_prob else move
        acts, probs = self.mcts.get_move_probs(board, temp, on_playout=on_playout)
        move_probs[list(acts)] = probs
        proven = self.mcts.proof_move()
        if proven is not None:
            move = proven
            self.mcts.update_with_move(move if self.is_selfplay else -1)
        elif self.is_selfplay:
            # Dirichlet noise on the sampling distribution only (mcts.py:216-221)
            move = np.random.choice(acts, p=(1 - EPS) * probs + EPS * np.random.dirichlet(ALPHA * np.ones(len(probs))))
            self.mcts.update_with_move(move)
        else:
            lcb = self.mcts.lcb_move()
            move = np.random.choice(acts, p=probs) if lcb is None else lcb
            self.mcts.update_with_move(-1)
        if return_prob:
            return move, move_probs
        return move
