"""Sequential NumPy model of the wide search ("wide PUCT", include/cczero.h "Wide search"): float32 running means, the float64
score with in-flight counts F, the first maximum, collisions, the budget cut-off and the slot numbering s(r, j) = r + j * A.

The model never generates moves or evaluates: like the sequential oracles of the other parity tests it is FED, per selected slot,
what the engine reports for that leaf (status, legal ids, priors, value), and says which leaves the next step selects. Used by
tests/test_gpu_wide_search.py (against the engine) and tests/test_cpu_wide_model.py (against a hand-computed case).
"""
from __future__ import annotations

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

    def descend(self, c_puct, trace=None):
        """Path (node indices) from the root to the first node without children; the first maximum in child order wins."""
        path = [0]
        while self.kids[path[-1]]:
            x = path[-1]
            sc = [self.score(x, i, c_puct) for i in self.kids[x]]
            if trace is not None:
                trace.append((x, sc))
            best, besti = -math.inf, None
            for i, s in zip(self.kids[x], sc):
                if s > best:                    # (a NaN never compares greater)
                    best, besti = s, i
            assert besti is not None, "no comparable child"
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


class WideModel:
    """``A`` searched boards, ``W`` slots each. ``budgets[r]``: simulations board r may back up per move (None: unlimited)."""

    def __init__(self, A, W, c_puct=5.0, budgets=None):
        self.A, self.W, self.c_puct = int(A), int(W), float(c_puct)
        self.budgets = [None] * self.A if budgets is None else list(budgets)
        self.trees = [Tree() for _ in range(self.A)]
        self.sims = [0] * self.A
        self.pending = [[None] * self.W for _ in range(self.A)]     # per slot: the path of its pending leaf
        # what the run has seen (the tests assert that the MODEL meets their conditions)
        self.collisions = self.full_steps = self.budget_cuts = self.leaves = self.board_steps = 0

    def slot(self, r, j):
        return r + j * self.A

    def moves_of(self, r, j):
        """Move ids from the root to the pending leaf of slot (r, j)."""
        t = self.trees[r]
        return [t.move[n] for n in self.pending[r][j][1:]]

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
            path = t_.descend(self.c_puct, tr)
            if trace is not None:
                trace.append((j, tr))
            if t_.F[path[-1]] > 0:
                self.collisions += 1
                ended = True
                continue
            for n in path:
                t_.F[n] += 1
            self.pending[r][j] = path
            got.append(j)
        if got:
            self.board_steps += 1
            self.leaves += len(got)
        if len(got) == self.W:
            self.full_steps += 1
        return got

    # ---- phase A
    def backup(self, r, feed):
        """``feed[j]`` for every pending slot j: dict(status, ids, priors, value)."""
        t_ = self.trees[r]
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
                t_.kids[leaf] = [t_.add(m, p) for m, p in zip(f["ids"], f["priors"])]
                v = f32(f["value"])
            else:
                t_.terminal_visits[leaf] = t_.terminal_visits.get(leaf, 0) + 1
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


def cpu_feed(board, wp, wv):
    """What the engine would report for the leaf ``board`` (an ``oracle.OracleBoard``), restated on the CPU in float64 -- close to,
    not bit for bit, the engine's priors: good enough to try inputs out without a GPU, never used to judge the engine."""
    ids = board.legal_ids()
    end, tie = board.is_game_over(), board.is_tie()
    status = EXPAND if (not end and not tie) else (DRAW if (end and tie) else LOSS)
    if status != EXPAND:
        return {"status": status}
    x = board.leaf_planes().reshape(17, 7, 90)[list(LIVE_GROUPS)].reshape(N_FEATURES).astype(np.float64)
    lg = (x @ wp.astype(np.float64)) * LOGIT_SCALE
    z = lg[ids] - lg[ids].max()     # (the engine's softmax runs over the legal ids only as well)
    p = np.exp(z) / np.exp(z).sum()
    return {"status": EXPAND, "ids": ids, "priors": p.astype(np.float32), "value": f32(np.tanh((x @ wv.astype(np.float64)) * VALUE_SCALE))}


def leaf_board(root, moves):
    b = root.copy()
    for m in moves:
        b.push_id(int(m))
    return b


def run_on_cpu(roots, W, budgets, c_puct=5.0, max_steps=10000):
    """The model alone on ``roots`` (OracleBoards) with :func:`cpu_feed`, until every budget is used."""
    wp, wv = projection()
    m = WideModel(len(roots), W, c_puct=c_puct, budgets=budgets)
    for _ in range(max_steps):
        any_leaf = False
        for r, root in enumerate(roots):
            got = m.select(r, over=root.is_game_over())
            any_leaf = any_leaf or bool(got)
            m.backup(r, {j: cpu_feed(leaf_board(root, m.moves_of(r, j)), wp, wv) for j in got})
        if not any_leaf:
            return m
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
