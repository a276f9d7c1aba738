"""CPU model of the value spread and the LCB move (ccz_set_value_stats / ccz_lcb_moves, include/cczero.h).

``SpreadModel`` is ``search_model.SearchModel`` plus S, the running sum of squared deviations of the values backed up through a node,
under the engine's rule, in NumPy float32 with the engine's operation order:

    d0 = val - q;   qn = q + d0 / (float)n;      (the backup as it is)
    S  = S + d0 * (val - qn);                    (one multiply, one add)

S is kept beside the tree (the model's nodes have ``__slots__``): a node that is re-rooted on, or kept below the new root, keeps its
S because it is the same object; a node made by an expansion or a fresh root has none yet, which reads as 0. S never feeds back:
selection, expansion, N, Q and the move boundary are SearchModel's.

The LCB rule is restated in Python floats (IEEE float64): ``lcb_bounds`` and ``lcb_choice``.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np

import selfplay_model as spm
from explore_model import F32
from search_model import SearchModel

NINF = float("-inf")


# ---------------------------------------------------------------------------------------------------------------- the statistic
def spread_step(n_old, q, s, val):
    """One backup of ``val`` into a node holding (N = n_old, Q = q, S = s): the new (N, Q, S), float32 operation by operation."""
    val, q, s = F32(val), F32(q), F32(s)
    n = int(n_old) + 1
    d0 = F32(val - q)
    delta = F32(d0 / F32(n))
    qn = F32(q + delta)
    d1 = F32(val - qn)
    prod = F32(d0 * d1)
    return n, qn, F32(s + prod)


class Tracker:
    """S beside a tree whose model is not SearchModel (tests/solver_model.SolverModel, the model of tests/solver_deep_cases.py): the
    backup under the rule above, to stand in for a module's ``backup(path, v)`` (:func:`tracking`)."""

    def __init__(self):
        self._S = {}   # id(node) -> [node, S]: the reference keeps the node alive, so an id is never reused for another node

    def S_of(self, node):
        e = self._S.get(id(node))
        return F32(0.0) if e is None else e[1]

    def backup(self, path, v):
        v = F32(v)
        d = len(path) - 1
        for j, node in enumerate(path):
            val = v if ((d - j) & 1) else F32(-v)
            n, qn, s = spread_step(node.N, node.Q, self.S_of(node), val)
            node.N, node.Q = n, qn
            self._S[id(node)] = [node, s]

    def top(self, root):
        """(S float32 [k] of the children, S of the node, Q of the node)."""
        return np.array([self.S_of(c) for c in (root.kids or [])], F32), self.S_of(root), F32(root.Q)


@contextlib.contextmanager
def tracking(module, cases=None):
    """For the length of the block ``module.backup`` is a :class:`Tracker`'s, and -- with ``cases`` = tests/solver_deep_cases -- every
    tree top that module records (``top(m, b)``) also holds ``S`` / ``root_S`` / ``root_Q``. Yields the tracker."""
    tr = Tracker()
    saved, saved_top = module.backup, getattr(cases, "top", None)
    module.backup = tr.backup
    if cases is not None:
        def top(m, b):
            s, rs, rq = tr.top(m.roots[b])
            return dict(saved_top(m, b), S=s, root_S=rs, root_Q=rq)
        cases.top = top
    try:
        yield tr
    finally:
        module.backup = saved
        if cases is not None:
            cases.top = saved_top


class SpreadModel(SearchModel):
    """SearchModel whose backup also keeps S per node (``S_of``)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._S = {}   # id(node) -> [node, S]: the reference keeps the node alive, so an id is never reused for another node

    def S_of(self, node):
        e = self._S.get(id(node))
        return F32(0.0) if e is None else e[1]

    def clear_spread(self):
        """ccz_set_value_stats(1) after (0): every S is zero again."""
        self._S = {}

    def _backup(self, path, v):
        v = F32(v)
        d = len(path) - 1
        for j, node in enumerate(path):
            val = v if ((d - j) & 1) else F32(-v)
            n, qn, s = spread_step(node.N, node.Q, self.S_of(node), val)
            node.N, node.Q = n, qn
            self._S[id(node)] = [node, s]

    def simulate(self, b):
        # SelfPlayModel.simulate calls the module's ``backup(path, v)``: for the length of this call it is this model's
        saved = spm.backup
        spm.backup = self._backup
        try:
            return super().simulate(b)
        finally:
            spm.backup = saved

    def root_spread(self, b):
        """(S float32 [k] of the root's children in child order, S of the root): what ccz_root_value_stats reports for a live board."""
        root = self.roots[b]
        return np.array([self.S_of(c) for c in (root.kids or [])], F32), self.S_of(root)


# ---------------------------------------------------------------------------------------------------------------- the LCB rule
def lcb_bounds(N, Q, S, z):
    """float64 [k]: lcb_i = (double)Q_i - z * sqrt(max((double)S_i, 0) / (N_i - 1) / N_i) for N_i >= 2, else -inf."""
    out = []
    for n, q, s in zip(N, Q, S):
        n = int(n)
        if n < 2:
            out.append(NINF)
            continue
        sd = float(F32(s))
        var = (sd if sd > 0.0 else 0.0) / float(n - 1)
        se = math.sqrt(var / float(n))
        out.append(float(F32(q)) - float(z) * se)
    return out


def first_max_visits(N):
    """i*: the first index of maximal N (None without children)."""
    best = None
    for i, n in enumerate(N):
        if best is None or int(n) > int(N[best]):
            best = i
    return best


def lcb_choice(N, Q, S, z, min_visit_ratio, min_visits):
    """(child index or -1, bounds): the rule of ccz_lcb_moves on one live root."""
    bounds = lcb_bounds(N, Q, S, z)
    star = first_max_visits(N)
    if star is None or int(N[star]) <= 0:
        return -1, bounds
    nmax = int(N[star])
    need = float(min_visit_ratio) * float(nmax)
    best = None
    for i, n in enumerate(N):
        n = int(n)
        if not (i == star or (n >= 2 and n >= int(min_visits) and float(n) >= need)):
            continue
        if bounds[i] > NINF and (best is None or bounds[i] > bounds[best]):
            best = i
    return (star if best is None else best), bounds


def lcb_moves(model, z, min_visit_ratio, min_visits, scouts=0):
    """What ccz_lcb_moves writes for the model's boards followed by ``scouts`` scout slots: moves int32 [B], child int32 [B],
    lcb float64 [B,128] (0 past k; all zero on a finished board and on a scout slot)."""
    B = model.B + scouts
    moves, child, lcb = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.zeros((B, 128), np.float64)
    for b in range(model.B):
        if model.over[b]:
            continue
        acts, N, Q, _ = model.root_children(b)
        S, _ = model.root_spread(b)
        ci, bounds = lcb_choice(N, Q, S, z, min_visit_ratio, min_visits)
        lcb[b, :len(bounds)] = bounds
        child[b] = ci
        moves[b] = int(acts[ci]) if ci >= 0 else -1
    return moves, child, lcb
