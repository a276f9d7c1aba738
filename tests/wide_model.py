"""Sequential NumPy model of the wide search ("wide PUCT", include/cczero.h "Wide search"): float32 running means, the float64
score with in-flight counts F, the first maximum, collisions, the budget cut-off and the slot numbering s(r, j) = r + j * A.

The model never generates moves or evaluates: like the sequential oracles of the other parity tests it is FED, per selected slot,
what the engine reports for that leaf (status, legal ids, priors, value), and says which leaves the next step selects. It also
states the move boundary on a kept tree (``reroot``) and the engine's limits as the wide kernels meet them: the node pool
(``max_nodes``), the path capacity (``max_depth``) and NaN priors. Used by tests/test_gpu_wide_search.py and
tests/test_gpu_wide_limits.py (against the engine) and tests/test_cpu_wide_model.py (against hand-computed cases).
"""
from __future__ import annotations

import functools
import math

import numpy as np

EXPAND, DRAW, LOSS, NONE = 0, 1, 2, 3
f32 = np.float32


class Tree:
    """Nodes in creation order; node 0 is the root ``Node(None, 1.0)``."""

    def __init__(self):
        self.N = [0]
        self.Q = [f32(0.0)]
        self.P = [f32(1.0)]
        self.F = [0]
        self.move = [-1]
        self.kids = [None]          # list of node indices once expanded
        self.terminal_visits = {}   # node -> times it was selected as a terminal leaf

    def add(self, move, prior):
        self.N.append(0)
        self.Q.append(f32(0.0))
        self.P.append(f32(prior))
        self.F.append(0)
        self.move.append(int(move))
        self.kids.append(None)
        return len(self.N) - 1

    def score(self, x, i, c_puct):
        """Score of child node ``i`` of node ``x``: every operation rounded on its own, float32 product, float64 elsewhere."""
        ne = self.N[i] + self.F[i]
        if ne == 0:
            return math.inf
        if self.F[i] == 0:
            qe = float(self.Q[i])
        else:
            qe = (float(self.N[i]) * float(self.Q[i]) - float(self.F[i])) / float(ne)
        return qe + float(f32(c_puct) * self.P[i]) * math.sqrt(float(self.N[x] + self.F[x])) / float(1 + ne)

    def descend(self, c_puct, trace=None, max_depth=None, wrong=None):
        """Path (node indices) from the root to the first node without children; the first maximum in child order wins.
        ``None`` after a stop, with ``self.stop`` = "nan" (no comparable child: every score NaN) or "depth" (the path would reach
        ``max_depth`` moves, i.e. more than ``max_depth`` entries); the NaN test of a level comes before its depth test, as in
        wide_descend. ``self.seen``: what the descent met at nodes with more than 64 children (see WideModel)."""
        path = [0]
        self.stop, self.seen = None, {"upper": 0, "tie64": 0}
        while self.kids[path[-1]]:
            x = path[-1]
            sc = [self.score(x, i, c_puct) for i in self.kids[x]]
            if trace is not None:
                trace.append((x, sc))
            best, besti, at = -math.inf, None, -1
            if wrong == "per_pass_maximum":         # each lane keeps its own first maximum over the passes, the lowest lane wins
                lanes = {}
                for c, s in enumerate(sc):
                    if s > lanes.get(c % 64, (-math.inf, -1))[0]:
                        lanes[c % 64] = (s, c)
                for lane in sorted(lanes):
                    if lanes[lane][0] > best:
                        best, at = lanes[lane]
                besti = None if at < 0 else self.kids[x][at]
            else:
                for c, (i, s) in enumerate(zip(self.kids[x], sc)):
                    if wrong == "upper_children_ignored" and c >= 64:
                        break
                    if s > best:                    # (a NaN never compares greater)
                        best, besti, at = s, i, c
            if besti is None:
                self.stop = "nan"
                return None
            if len(sc) > 64:
                self.seen["upper"] += at >= 64
                self.seen["tie64"] += at < 64 and any(s == best for s in sc[64:])
            if max_depth is not None and len(path) >= max_depth:
                self.stop = "depth"
                return None
            path.append(besti)
        return path

    def backup(self, path, v):
        """Node.update_recursive(-v) along the path: the leaf gets -v, its parent +v, ...; float32 incremental mean."""
        d = len(path) - 1
        for j, node in enumerate(path):
            val = f32(v) if ((d - j) & 1) else f32(-f32(v))
            n = self.N[node] + 1
            delta = f32(val - self.Q[node])
            delta = f32(delta / f32(n))
            self.Q[node] = f32(self.Q[node] + delta)
            self.N[node] = n

    def n_nodes(self):
        return len(self.N)

    def subtree(self, top):
        """The tree below node ``top`` as a tree of its own, as k_finish_move copies it (breadth first; child order, N, Q and the
        node's OWN prior kept -- the new root keeps the P it had as a child, not Node(None, 1.0)'s)."""
        t = Tree()
        t.N, t.Q, t.P, t.move = [self.N[top]], [self.Q[top]], [self.P[top]], [self.move[top]]
        old = [top]
        head = 0
        while head < len(old):
            kids = self.kids[old[head]]
            if kids:
                t.kids[head] = []
                for i in kids:
                    t.kids[head].append(t.add(self.move[i], self.P[i]))
                    t.N[-1], t.Q[-1] = self.N[i], self.Q[i]
                    old.append(i)
            if old[head] in self.terminal_visits:
                t.terminal_visits[head] = self.terminal_visits[old[head]]
            head += 1
        return t

    def root_children(self):
        k = self.kids[0] or []
        return (np.array([self.move[i] for i in k], np.uint16), np.array([self.N[i] for i in k], np.int32),
                np.array([self.Q[i] for i in k], np.float32), np.array([self.P[i] for i in k], np.float32))

    def pv(self, max_len=32):
        """ccz_principal_variations, line 0: the first child of maximal N with N > 0, level by level."""
        moves, node = [], 0
        while self.kids[node] and len(moves) < max_len:
            best = max(self.kids[node], key=lambda i: (self.N[i], -i))
            if self.N[best] <= 0:
                break
            moves.append(self.move[best])
            node = best
        return moves


# Each rule of the model stated wrongly (tests/test_cpu_wide_model.py shows that every one changes the result on the inputs of
# tests/test_gpu_wide_limits.py: a kernel with that mistake cannot pass there)
WRONG = ("upper_children_ignored", "per_pass_maximum", "reroot_forgets_visits", "reroot_keeps_sims", "refusal_blocks_later_slots",
         "stop_drops_the_batch")


class WideModel:
    """``A`` searched boards, ``W`` slots each. ``budgets[r]``: simulations board r may back up per move (None: unlimited).
    ``max_nodes``: the node pool per board (``Dev.cap``: ccz_create raises anything below 130 to 130; None: unbounded);
    ``max_depth``: path entries (``Dev.maxd``: ccz_config.max_depth, at least 64, 0 means 512; None: unbounded).
    ``wrong``: one of ``WRONG``."""

    def __init__(self, A, W, c_puct=5.0, budgets=None, max_nodes=None, max_depth=None, wrong=None):
        assert wrong is None or wrong in WRONG
        self.A, self.W, self.c_puct = int(A), int(W), float(c_puct)
        self.max_nodes, self.max_depth, self.wrong = max_nodes, max_depth, wrong
        self.budgets = [None] * self.A if budgets is None else list(budgets)
        self.trees = [Tree() for _ in range(self.A)]
        self.sims = [0] * self.A
        self.pending = [[None] * self.W for _ in range(self.A)]     # per slot: the path of its pending leaf
        # what the run has seen (the tests assert that the MODEL meets their conditions)
        self.collisions = self.full_steps = self.budget_cuts = self.leaves = self.board_steps = 0
        self.terminal_leaves = 0        # terminal leaves backed up (ccz_stats.terminal_leaves)
        self.max_t = 0                  # the most leaves one board selected in one step
        self.upper_selected = 0         # descents through a child of index >= 64
        self.ties_across_64 = 0         # ... at a node with > 64 children whose maximum is attained below AND from index 64: the lower wins
        self.refused = [0] * self.A     # EXPAND leaves the pool refused (CCZ_ERR_NODE_POOL), per board
        self.refused_again = 0          # ... selected again later
        self.fit_after_refusal = 0      # steps in which a slot was refused and a LATER slot with fewer children still fitted
        self.depth_stops = [0] * self.A  # batches ended by CCZ_ERR_DEPTH, per board ...
        self.nan_stops = [0] * self.A    # ... by CCZ_ERR_NAN
        self.stops_after_leaves = 0     # ... of either kind with t >= 1: the earlier slots stay selected
        self.empty_steps_after_stop = 0  # selections with t == 0 ended by such a stop
        self._refused_nodes = [set() for _ in range(self.A)]

    def slot(self, r, j):
        return r + j * self.A

    def moves_of(self, r, j):
        """Move ids from the root to the pending leaf of slot (r, j)."""
        t = self.trees[r]
        return [t.move[n] for n in self.pending[r][j][1:]]

    def error_flags(self):
        """The sticky error word the engine must show: CCZ_ERR_NODE_POOL 1, CCZ_ERR_DEPTH 2, CCZ_ERR_NAN 32."""
        return (1 if any(self.refused) else 0) | (2 if any(self.depth_stops) else 0) | (32 if any(self.nan_stops) else 0)

    # ---- phase B
    def select(self, r, over=False, trace=None):
        """Returns the list of j that received a leaf (always 0 .. t-1)."""
        t_ = self.trees[r]
        assert all(p is None for p in self.pending[r]), "select with leaves pending"
        got, ended = [], bool(over)
        for j in range(self.W):
            if ended:
                continue
            if self.budgets[r] is not None and self.sims[r] + len(got) >= self.budgets[r]:
                if got and j == len(got):
                    self.budget_cuts += 1       # the budget ended a batch that had begun
                ended = True
                continue
            tr = None if trace is None else []
            path = t_.descend(self.c_puct, tr, self.max_depth, self.wrong)
            if trace is not None:
                trace.append((j, tr))
            if path is None:                    # CCZ_ERR_NAN / CCZ_ERR_DEPTH: the slot gets nothing, the batch ends; earlier slots stay
                (self.nan_stops if t_.stop == "nan" else self.depth_stops)[r] += 1
                if got:
                    self.stops_after_leaves += 1
                else:
                    self.empty_steps_after_stop += 1
                if self.wrong == "stop_drops_the_batch":
                    for jj in got:
                        for n in self.pending[r][jj]:
                            t_.F[n] -= 1
                        self.pending[r][jj] = None
                    got = []
                ended = True
                continue
            if t_.F[path[-1]] > 0:
                self.collisions += 1
                ended = True
                continue
            self.upper_selected += t_.seen["upper"]
            self.ties_across_64 += t_.seen["tie64"]
            if path[-1] in self._refused_nodes[r]:
                self.refused_again += 1
            for n in path:
                t_.F[n] += 1
            self.pending[r][j] = path
            got.append(j)
        if got:
            self.board_steps += 1
            self.leaves += len(got)
        if len(got) == self.W:
            self.full_steps += 1
        self.max_t = max(self.max_t, len(got))
        return got

    # ---- phase A
    def backup(self, r, feed):
        """``feed[j]`` for every pending slot j: dict(status, ids, priors, value)."""
        t_ = self.trees[r]
        refused_k = None                        # the fewest children the pool refused in this step
        for j in range(self.W):
            path = self.pending[r][j]
            if path is None:
                continue
            f = feed[j]
            for n in path:
                t_.F[n] -= 1
                assert t_.F[n] >= 0
            leaf = path[-1]
            if f["status"] == EXPAND:
                assert t_.kids[leaf] is None
                k = len(f["ids"])
                fits = self.max_nodes is None or t_.n_nodes() + k <= self.max_nodes
                if self.wrong == "refusal_blocks_later_slots" and refused_k is not None:
                    fits = False
                if fits:
                    t_.kids[leaf] = [t_.add(m, p) for m, p in zip(f["ids"], f["priors"])]
                    if refused_k is not None and k < refused_k:
                        self.fit_after_refusal += 1
                else:                           # the leaf stays unexpanded; its value is backed up and the simulation counts
                    self.refused[r] += 1
                    self._refused_nodes[r].add(leaf)
                    refused_k = k if refused_k is None else min(refused_k, k)
                v = f32(f["value"])
            else:
                t_.terminal_visits[leaf] = t_.terminal_visits.get(leaf, 0) + 1
                self.terminal_leaves += 1
                v = f32(0.0) if f["status"] == DRAW else f32(-1.0)
            t_.backup(path, v)
            self.sims[r] += 1
            self.pending[r][j] = None

    def drop(self, r, new_tree=False):
        """A move boundary: pending leaves leave F; the simulation count starts over."""
        t_ = self.trees[r]
        for j in range(self.W):
            if self.pending[r][j] is not None:
                for n in self.pending[r][j]:
                    t_.F[n] -= 1
                self.pending[r][j] = None
        self.sims[r] = 0
        if new_tree:
            self.trees[r] = Tree()
            self._refused_nodes[r] = set()

    def reroot(self, r, move):
        """The move boundary with keep_tree: pending leaves leave F (as in ``drop``), the subtree below the root child with
        ``move`` becomes the tree (a child never expanded: a bare root with that child's N, Q and P), the simulation count starts
        over. The node count is the kept subtree's, as k_finish_move accounts it."""
        keep_sims = self.sims[r]
        self.drop(r)
        t_ = self.trees[r]
        top = [i for i in (t_.kids[0] or []) if t_.move[i] == int(move)]
        assert len(top) == 1, "the move is no child of the root"
        assert sum(t_.F) == 0
        self.trees[r] = Tree() if self.wrong == "reroot_forgets_visits" else t_.subtree(top[0])
        self._refused_nodes[r] = set()
        if self.wrong == "reroot_keeps_sims":
            self.sims[r] = keep_sims

    def most_visited(self, r):
        """The move of the most visited root child (first maximum)."""
        acts, n, _, _ = self.trees[r].root_children()
        return int(acts[int(np.argmax(n))])

    def inflight(self):
        return sum(sum(t.F) for t in self.trees)

    def repeated_terminals(self):
        return sum(1 for t in self.trees for c in t.terminal_visits.values() if c >= 2)


# ---------------------------------------------------------------------------------------------------------------------------
# The evaluator of the wide-search tests: a fixed random projection of the three live plane groups (7: red, 15: black, 16: side to
# move) with small INTEGER weights -- every logit is an exact float32 whatever the batch size or summation order, so a row's result
# does not depend on the batch it sits in (what the evaluation cache and the planned boundary assume) -- and a tanh value.
LIVE_GROUPS = (7, 15, 16)
N_FEATURES = 21 * 90
LOGIT_SCALE, VALUE_SCALE = 1.0 / 16.0, 1.0 / 32.0


@functools.lru_cache(maxsize=None)
def projection(seed=5):
    g = np.random.RandomState(seed)
    return g.randint(-6, 7, size=(N_FEATURES, 2086)).astype(np.float32), g.randint(-6, 7, size=(N_FEATURES,)).astype(np.float32)


def make_torch_evaluator(device, seed=5):
    """``ev(leaf fp16 [B,17,7,10,9], plan=None) -> (logits f32 [B,2086], value f32 [B])``; with a plan ``(miss_rows, n_miss)`` row i
    is slot ``miss_rows[i]`` (all B rows are computed: the ones past ``n_miss`` are never read)."""
    import torch
    wp, wv = projection(seed)
    wp_t, wv_t = torch.from_numpy(wp).to(device), torch.from_numpy(wv).to(device)
    groups = torch.tensor(LIVE_GROUPS, device=device)

    def ev(leaf, plan=None):
        x = leaf if plan is None else leaf[plan[0].long()]
        x = x.index_select(1, groups).reshape(x.shape[0], N_FEATURES).float()
        return ((x @ wp_t) * LOGIT_SCALE).contiguous(), torch.tanh((x @ wv_t) * VALUE_SCALE).contiguous()

    ev.returns_logits = ev.accepts_plan = ev.batched = ev.stateless = True
    ev.graph_safe = False
    return ev


_ROWS = {}


def cpu_feed(board, wp, wv):
    """What the engine would report for the leaf ``board`` (an ``oracle.OracleBoard``), restated on the CPU in float64 -- close to,
    not bit for bit, the engine's priors: good enough to try inputs out without a GPU, never used to judge the engine."""
    ids = board.legal_ids()
    end, tie = board.is_game_over(), board.is_tie()
    status = EXPAND if (not end and not tie) else (DRAW if (end and tie) else LOSS)
    if status != EXPAND:
        return {"status": status}
    key = (board.squares().tobytes(), int(board.turn), id(wp), id(wv))
    if key not in _ROWS:            # (a row depends on the position alone: the runs of one test file meet the same positions again)
        x = board.leaf_planes().reshape(17, 7, 90)[list(LIVE_GROUPS)].reshape(N_FEATURES).astype(np.float64)
        _ROWS[key] = ((x @ wp.astype(np.float64)) * LOGIT_SCALE, f32(np.tanh((x @ wv.astype(np.float64)) * VALUE_SCALE)))
    lg, v = _ROWS[key]
    z = lg[ids] - lg[ids].max()     # (the engine's softmax runs over the legal ids only as well)
    p = np.exp(z) / np.exp(z).sum()
    return {"status": EXPAND, "ids": ids, "priors": p.astype(np.float32), "value": v}


def leaf_board(root, moves):
    b = root.copy()
    for m in moves:
        b.push_id(int(m))
    return b


# Per-board evaluator overrides of the limit cases, applied to a board's rows after the projection (the forms of
# tests/engine_limit_cases.py): ("nan",): every logit NaN, the value stays; ("sharp", salt): prior 0.97 on one hash-chosen legal move,
# 0.03 / k on each, value 0 -- nothing tells lines apart but the prior, so PUCT digs one long line.
def sharp_priors(squares, turn, ids, salt):
    """float32 [k] over the legal ``ids`` of the position."""
    from oracle.evaluators import position_hash
    p = np.full(len(ids), np.float32(0.03 / len(ids)), np.float32)
    p[int(position_hash(np.asarray(squares)[None], np.array([int(turn)]), salt)[0] % np.uint64(len(ids)))] = np.float32(0.97)
    return p


def override_rows(kind, leaf, logits, value):
    """The GPU side: ``leaf`` fp16 [n,17,7,10,9], ``logits`` [n,2086], ``value`` [n] (torch, one board's rows) -> (logits, value).
    log(prior) on the legal ids and -1e4 (exp underflows to 0) on all others: the softmax hands the engine the sharp priors whether
    it runs over the legal ids or over the whole row."""
    import torch
    if kind[0] == "nan":
        return logits * float("nan"), value
    assert kind[0] == "sharp"
    from gpu_harness import planes_to_squares
    from oracle import OracleBoard
    sq, turn = planes_to_squares(leaf.float().cpu().numpy())
    out = np.full((len(sq), 2086), -1e4, np.float32)
    for i in range(len(sq)):
        if sq[i].any():                 # (a slot that never held a leaf: an empty row nobody reads)
            ids = OracleBoard.from_array(sq[i], int(turn[i])).legal_ids()
            if ids:
                out[i, ids] = np.log(sharp_priors(sq[i], turn[i], ids, kind[1]))
    return torch.from_numpy(out).to(logits.device), value * 0.0


def with_overrides(ev, A, overrides):
    """The evaluator ``ev`` (make_torch_evaluator) with the rows of board r -- slots r, r + A, ... -- overridden as ``overrides[r]``
    says. Whole batches only (no plan: a cached or shared row would carry one board's override to another)."""
    def ev2(leaf):
        logits, value = ev(leaf)
        for r, kind in overrides.items():
            logits[r::A], value[r::A] = override_rows(kind, leaf[r::A], logits[r::A], value[r::A])
        return logits, value

    ev2.returns_logits = ev2.batched = ev2.stateless = True
    ev2.accepts_plan = ev2.graph_safe = False
    return ev2


def cpu_feed_override(board, wp, wv, kind):
    """:func:`cpu_feed` under an override (same caveat: close to the engine's numbers, never used to judge it)."""
    f = cpu_feed(board, wp, wv)
    if f["status"] != EXPAND or kind is None:
        return f
    if kind[0] == "nan":
        return dict(f, priors=np.full(len(f["ids"]), np.nan, np.float32))
    return dict(f, priors=sharp_priors(board.squares(), board.turn, f["ids"], kind[1]), value=f32(0.0))


def run_on_cpu(roots, W, budgets, c_puct=5.0, max_steps=10000, overrides=None, model=None, only_steps=None, **model_kw):
    """The model alone on ``roots`` (OracleBoards) with :func:`cpu_feed`, until every budget is used (``only_steps``: at most that many
    steps; the last selection stays pending). ``overrides``: {board: ("nan",) or ("sharp", salt)}; ``model``: go on with this model (after a
    move boundary); ``model_kw``: max_nodes, max_depth, wrong. ``m.host_steps``: the selections that found a leaf, over all calls."""
    wp, wv = projection()
    overrides = overrides or {}
    m = model if model is not None else WideModel(len(roots), W, c_puct=c_puct, budgets=budgets, **model_kw)
    m.budgets = list(budgets)
    m.host_steps = getattr(m, "host_steps", 0)
    for step in range(max_steps):
        gots = [m.select(r, over=root.is_game_over()) for r, root in enumerate(roots)]
        if not any(gots):
            return m
        m.host_steps += 1
        if only_steps is not None and step == only_steps:
            return m
        for r, root in enumerate(roots):
            m.backup(r, {j: cpu_feed_override(leaf_board(root, m.moves_of(r, j)), wp, wv, overrides.get(r)) for j in gots[r]})
    raise AssertionError("the model did not finish")


# The three inputs of the model tests, on boards 0, 1, 2 (A = 3: r + j * A with A not a power of two), and their budgets: a budget
# ends a batch mid-step on every board. Chosen by running the model on the CPU (run_on_cpu; tests/test_cpu_wide_model.py keeps the
# conditions true): the start position fills whole batches (t == W); "two_rooks" is one ply from mate (terminal leaves); in the bare
# ending -- three legal moves, the capture leaves bare kings -- descents collide and the same terminal node is selected again.
BUDGETS = (64, 40, 7)


def model_inputs():
    """[(squares uint8 [90], turn)] of the three boards."""
    from golden_cases import STARTS
    from oracle import OracleBoard
    return [(OracleBoard().squares().copy(), 1), (STARTS["two_rooks"].copy(), 1), (STARTS["capture_to_bare"].copy(), 1)]


def conditions(m):
    """What a run must have seen for the comparison to mean something (asserted on the MODEL: a silent no-op cannot pass)."""
    return {"collisions": m.collisions >= 1, "terminal leaf selected twice": m.repeated_terminals() >= 1,
            "a step with t == W": m.full_steps >= 1, "a step cut by the budget": m.budget_cuts >= 1}


# ---------------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_wide_limits.py (tests/test_cpu_wide_model.py keeps every statement here true on the model alone).
# A = 4 searched boards: the start position (44 moves: whole batches), "widest" (108 moves against a bare king: the root is the one
# node of more than 64 children whose first expansion ties +inf scores across index 64), WIDE_PAIR of tests/engine_limit_cases.py
# (100 moves, 67 in reply: many such nodes, children of index >= 64 selected on their scores) and "two_rooks" (terminal leaves).
LIMIT_WIDTHS = (24, 32, 64)
LIMIT_BUDGETS = (128, 128, 128, 100)
LIMIT_MAX_NODES = 8192


def limit_inputs():
    from engine_limit_cases import WIDE_PAIR
    from golden_cases import STARTS
    from oracle import OracleBoard
    return [(OracleBoard().squares().copy(), 1), (STARTS["widest"].copy(), 1), (WIDE_PAIR[0].copy(), 1), (STARTS["two_rooks"].copy(), 1)]


def limit_conditions(m):
    """:func:`conditions` and what only the widths above 16 and nodes of more than 64 children can show."""
    return dict(conditions(m), **{"a step with t > 16": m.max_t > 16, "a selected child of index >= 64": m.upper_selected >= 1,
                                  "a maximum attained below and from index 64": m.ties_across_64 >= 1})


# ---- kept trees: KEPT_MOVES moves of KEPT_BUDGET simulations on the four boards; the first boundary is crossed after
# KEPT_FIRST_STEPS backed-up steps, with the next selection pending. Every boundary forces the model's most visited root child (first
# maximum) among those that do not end the game; on "two_rooks" (board 3) the last boundary forces the mating move instead.
KEPT_WIDTHS = (8, 32)
KEPT_MOVES, KEPT_BUDGET, KEPT_FIRST_STEPS = 3, 48, 2


def kept_forced(m, roots, last):
    """The moves the boundary forces, from the model's roots (``roots``: OracleBoards, not changed)."""
    out = []
    for r, root in enumerate(roots):
        acts, n, _, _ = m.trees[r].root_children()
        ends = [leaf_board(root, [a]).is_game_over() for a in acts]
        pick = [i for i in range(len(acts)) if ends[i] == (last and r == 3)]
        assert pick, (r, "no such move")
        out.append(int(acts[max(pick, key=lambda i: (n[i], -i))]))
    return out


def kept_boundary(m, roots, forced):
    for r, mv in enumerate(forced):
        m.reroot(r, mv)
        roots[r].push_id(mv)


# ---- the node pool: board 0 (the start position) fills POOL_MAX_NODES nodes; the others stay far below
POOL_W, POOL_MAX_NODES, POOL_BUDGETS = 16, 523, (64, 24, 24, 24)


def pool_inputs():
    from golden_cases import STARTS
    from oracle import OracleBoard
    return [(OracleBoard().squares().copy(), 1), (STARTS["two_rooks"].copy(), 1), (STARTS["widest"].copy(), 1), (STARTS["pawns"].copy(), 1)]


# ---- the depth limit: board 0 ("pawns", black to move, sharp priors with salt 2) digs a line of 64 path entries. ccz_create takes
# no max_depth below 64, and every node on a line needs a visit to each of its children before the line goes on below it (an
# unvisited child scores +inf), so the line takes some 520 simulations: DEPTH_BUDGETS[0] lies above that, the board must stop below it.
DEPTH_W, DEPTH_MAX_DEPTH, DEPTH_BUDGETS = 8, 64, (640, 24, 24, 24)
DEPTH_OVERRIDES = {0: ("sharp", 2)}


def depth_inputs():
    from golden_cases import STARTS
    from oracle import OracleBoard
    return [(STARTS["pawns"].copy(), 0), (STARTS["two_rooks"].copy(), 1), (OracleBoard().squares().copy(), 1), (STARTS["pawns"].copy(), 1)]


# ---- NaN priors: board 0 (the start position) gets NaN logits. An unvisited child scores +inf whatever its prior, so the root's k
# children are visited once each; the descent after that finds k NaN scores.
NAN_W, NAN_BUDGETS = 8, (64, 24, 24, 24)
NAN_OVERRIDES = {0: ("nan",)}
nan_inputs = pool_inputs
