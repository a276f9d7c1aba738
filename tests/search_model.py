"""CPU model of the search parameters (ccz_set_search, include/cczero.h): first-play urgency and the
visit-scaled exploration constant.

Plain Python + NumPy, one sequential MCTS per board, on top of ``selfplay_model.SelfPlayModel`` by way of ``gumbel_model.GumbelModel``
(which is SelfPlayModel plus the Gumbel root and the bookkeeping of the leaf a simulation reached; with ``gumbel=None`` it is
SelfPlayModel as it is). Overridden is the child selection only -- and, for R6, the exploration constant that target pruning is handed.
R1-R6 are restated here in Python floats (IEEE float64, no contraction); ``det_log`` is the oracle's ``xq_det_log``, as
tests/gumbel_model.py takes it.

  R1  c_eff(X) = c_puct (float32) when c_factor == 0, else (float32)((double)c_puct + c_factor * det_log(((double)N_X + c_base + 1) / c_base));
      it enters the score as the float32 product c_eff * P.
  R2  M(X) = sum of (double)P_i over children with N_i > 0: lane l forms m_l = a + b (a: child l, b: child l + 64; 0.0 where the child
      does not exist or has no visits), then m_l = m_l + m_{l xor s} for s = 32, 16, 8, 4, 2, 1. Raw priors, also at an explored root.
  R3  mode / value: the root pair at depth 0, the tree pair below. Mode 1: f = (double)(-Q_X) - value * sqrt(M). Mode 2: f = value.
      Mode 0: +inf. No clamping.
  R4  an unvisited child scores f + (double)(c_eff * P_i) * sqrt((double)N_X); first maximum in child order.
  R5  a visited root child short of its forced playouts still scores +inf; an unvisited child of an explored root uses P'_i in R4; at a
      Gumbel root the rule is Gumbel's and the tree pair applies from depth 1.
  R6  target pruning uses c_eff(root) where it uses c_puct.

``wrong=`` names a mis-stated rule for the CPU test (tests/test_cpu_search_model.py); the model itself never does:
``parent_sign`` (+Q_X for -Q_X), ``mass_all`` (M over all children), ``mass_noisy`` (M over P' at an explored root), ``root_uses_tree``
(the root pair ignored), ``growth_child_visits`` (N_i for N_X in R1), ``first_is_child0`` (a freshly expanded root hands out child 0),
``prune_plain_cpuct`` (R6 not applied)."""
from __future__ import annotations

import functools
import math

import numpy as np

import explore_model as em
import gumbel_model as gm
import solver_cases as sc
from explore_model import F32, forced_mask, noisy_priors, prune_counts
from gumbel_model import GumbelModel, det_log
from oracle import OracleBoard, det_pi

INF = float("inf")
WRONG = ("parent_sign", "mass_all", "mass_noisy", "root_uses_tree", "growth_child_visits", "first_is_child0", "prune_plain_cpuct")
OFF, REDUCTION, ABSOLUTE = 0, 1, 2
C_BASE = 19652.0
DEFAULTS = {"enabled": False, "fpu_mode": 0, "fpu_value": 0.0, "fpu_root_mode": 0, "fpu_root_value": 0.0, "c_base": C_BASE, "c_factor": 0.0}


def settings(fpu_mode=0, fpu_value=0.0, fpu_root_mode=None, fpu_root_value=None, c_base=C_BASE, c_factor=0.0):
    """The dict SelfPlayEngine.set_search takes, with the root defaulting to the tree's pair; a mode that is off has value 0."""
    if fpu_root_mode is None:
        fpu_root_mode, fpu_root_value = fpu_mode, (fpu_value if fpu_root_value is None else fpu_root_value)
    elif fpu_root_value is None:
        fpu_root_value = 0.0
    return {"fpu_mode": int(fpu_mode), "fpu_value": float(fpu_value) if fpu_mode else 0.0, "fpu_root_mode": int(fpu_root_mode),
            "fpu_root_value": float(fpu_root_value) if fpu_root_mode else 0.0, "c_base": float(c_base), "c_factor": float(c_factor)}


# ---------------------------------------------------------------------------------------------------------------- R1 - R4
def c_eff(c_puct, cfg, n):
    """R1, as a float32."""
    c = F32(c_puct)
    if cfg is None or cfg["c_factor"] == 0.0:
        return c
    return F32(float(c) + cfg["c_factor"] * det_log((float(n) + cfg["c_base"] + 1.0) / cfg["c_base"]))


def visited_mass(N, P):
    """R2: the butterfly sum over 64 lanes of two children each."""
    k = len(N)

    def term(i):
        return float(F32(P[i])) if i < k and int(N[i]) > 0 else 0.0
    assert k <= 128
    m = [term(l) + term(l + 64) for l in range(64)]
    for s in (32, 16, 8, 4, 2, 1):
        m = [m[l] + m[l ^ s] for l in range(64)]
    return m[0]


def urgency(mode, value, q, mass, wrong=None):
    """R3. q: the node's running mean as stored (float32)."""
    if mode == REDUCTION:
        v = float(F32(q)) if wrong == "parent_sign" else float(F32(-F32(q)))
        return v - float(value) * math.sqrt(mass)
    if mode == ABSOLUTE:
        return float(value)
    return INF


def scores(N, Q, pp, node_n, c, f, forced=None):
    """R4 and the visited formula: float64 [k]. ``pp``: the priors of the U term (float32), ``c``: c_eff (float32, or one per child),
    ``f``: the urgency, ``forced``: children that score +inf whatever else."""
    k = len(N)
    sq = math.sqrt(float(node_n))
    out = []
    for i in range(k):
        n = int(N[i])
        ci = c[i] if isinstance(c, (list, np.ndarray)) else c
        if (forced is not None and forced[i]) or (n == 0 and f == INF):
            out.append(INF)
            continue
        u = float(F32(F32(ci) * F32(pp[i])))
        out.append((f if n == 0 else float(F32(Q[i]))) + u * sq / float(1 + n))
    return out


def first_max(sc):
    best, bi = None, None
    for i, s in enumerate(sc):
        if s == s and (best is None or s > best):
            best, bi = s, i
    return bi


# ---------------------------------------------------------------------------------------------------------------- the search
class SearchModel(GumbelModel):
    """B boards, each a sequential search. ``search``: the dict of ``settings`` or None (off: the base model as it is); ``explore`` /
    ``gumbel`` / ``solver`` / ``resign`` / ``cap`` / ``max_plies`` / ``evaluator(b, board)`` as in SelfPlayModel and GumbelModel."""

    def __init__(self, boards, salts, seed, board_id_base=0, c_puct=5, search=None, explore=None, gumbel=None, wrong=None, **kw):
        assert wrong is None or wrong in WRONG
        assert explore is None or gumbel is None
        super().__init__(boards, salts, seed, board_id_base, c_puct, gumbel=gumbel, **kw)
        self.cfg = None if explore is None else dict(explore)     # (GumbelModel constructs its base with exploration off)
        self.scfg = None if search is None else dict(search)
        self.swrong = wrong
        self.depth_peak = self.sum_depth = 0
        self.sfacts = {"hi_before_lo": 0, "fresh_root_not_child0": 0, "unvisited_not_first": 0}

    # -------------------------------------------------------------------------------------------------------- selection
    def _select_child(self, b, node, depth):
        if self.scfg is None or (depth == 0 and self.gcfg is not None):       # off, or the Gumbel root (R5)
            return super()._select_child(b, node, depth)
        i = self._search_child(b, node, depth)
        self._moves.append(node.kids[i].move)
        return i

    def _search_child(self, b, node, depth):
        s, w = self.scfg, self.swrong
        kids = node.kids
        N = [int(c.N) for c in kids]
        Q = [c.Q for c in kids]
        P = np.array([c.P for c in kids], F32)
        explored = depth == 0 and self.explored(b)
        pp, forced = P, None
        if explored:
            pp = self._root_priors(b, node)
            forced = forced_mask(N, pp, node.N - 1, self.cfg["forced_k"])
        if w == "first_is_child0" and depth == 0 and node.N == 1 and not any(N):
            return 0
        root_pair = depth == 0 and w != "root_uses_tree"
        mode, value = (s["fpu_root_mode"], s["fpu_root_value"]) if root_pair else (s["fpu_mode"], s["fpu_value"])
        mass = visited_mass([1] * len(N) if w == "mass_all" else N, pp if (w == "mass_noisy" and explored) else P)
        f = urgency(mode, value, node.Q, mass, w)
        c = [c_eff(self.c_puct, s, n) for n in N] if w == "growth_child_visits" else c_eff(self.c_puct, s, node.N)
        i = first_max(scores(N, Q, pp, node.N, c, f, forced))
        assert i is not None, "NaN scores: the model's evaluators give none"
        if forced is not None and forced[i]:
            self.board_stats[b]["forced_selections"] += 1
        if N[i] == 0:
            lower = [j for j in range(i) if N[j] == 0]
            self.sfacts["unvisited_not_first"] += int(bool(lower))
            self.sfacts["hi_before_lo"] += int(i >= 64 and bool(lower))
            self.sfacts["fresh_root_not_child0"] += int(depth == 0 and node.N == 1 and i != 0)
        return i

    def simulate(self, b):
        status, k, depth = super().simulate(b)
        self.sum_depth += depth
        self.depth_peak = max(self.depth_peak, depth)
        return status, k, depth

    # -------------------------------------------------------------------------------------------------------- R6
    def targets_of(self, b):
        if self.scfg is None or self.swrong == "prune_plain_cpuct" or not (self.explored(b) and self.roots[b].kids):
            return super().targets_of(b)
        root = self.roots[b]
        _, N, Q, P = self.root_children(b)
        pn = noisy_priors(P, self._noise(b, root), self.cfg["eps"])
        Np, gaps = prune_counts(N, Q, pn, root.N, c_eff(self.c_puct, self.scfg, root.N), self.cfg["forced_k"], self.cfg["prune"])
        return Np, det_pi(Np.astype(np.int32), self.temp), gaps

    def root_visited(self, b):
        return sum(1 for c in (self.roots[b].kids or []) if c.N > 0)


# ---------------------------------------------------------------------------------------------------------------- the GPU test's inputs
B = 8
SEED, BASE = 41, 12288
SALTS = tuple(range(303, 303 + B))     # (board WIDE: the peak of the scripted priors falls on root child 104)
SIMS, MOVES = 64, 3
START, PAWNS, WIDE, MATE2, ONE, TWO, OPEN_A, OPEN_B = range(B)
SETTINGS = {
    "reduction": settings(REDUCTION, 0.33),
    "absolute": settings(ABSOLUTE, -0.25),
    "mixed": settings(REDUCTION, 0.5, ABSOLUTE, 0.75),
    "growth": settings(REDUCTION, 0.33, c_base=8.0, c_factor=2.0),
    "growth_only": settings(OFF, c_base=8.0, c_factor=2.0),
}
EVALUATORS = gm.EVALUATORS
EXPLORE = dict(em.FULL)


@functools.lru_cache(maxsize=None)
def inputs():
    """8 boards as (squares, turn): the start position, ``pawns`` (7 moves), ``widest`` (108 moves: children 64.. exist),
    ``mate_in_two``, a check with one legal move and a double check with two (the odd roots of tests/test_gpu_gumbel.py), and two of
    selfplay_model.inputs()'s opening positions (30 to 50 moves)."""
    import rules_kat
    import selfplay_model as spm
    from golden_cases import STARTS
    by_name = {c["name"]: c for c in rules_kat.cases()}
    _, msq, mturn, *_ = sc.CASES[sc.NAMES.index("mate_in_two")]
    out = [(OracleBoard().squares(), 1), (STARTS["pawns"].copy(), 1), (STARTS["widest"].copy(), 1), (msq.copy(), int(mturn))]
    for name in ("king_cannot_capture_a_protected_piece", "double_check_only_the_king_moves"):
        sq, turn, _ = rules_kat.start_of(by_name[name])
        out.append((np.asarray(sq, np.uint8).copy(), int(turn)))
    out += [spm.inputs()[7], spm.inputs()[9]]
    ks = [len(OracleBoard.from_array(sq, t).legal_ids()) for sq, t in out]
    assert ks[ONE] == 1 and ks[TWO] == 2 and ks[WIDE] >= 98 and ks[PAWNS] == 7, ks
    return tuple(out)


def boards(which=None):
    pos = inputs() if which is None else [inputs()[j] for j in which]
    return [OracleBoard.from_array(sq, turn) for sq, turn in pos]


def case(setting, evaluator="peaked", wrong=None, which=None, **kw):
    """(model, f): the model of one case of tests/test_gpu_search_params.py and the evaluator ``f(b, squares, turn)`` both sides are
    fed. ``setting``: a name of SETTINGS, a dict, or None (off). ``which``: board indices of ``inputs()`` (default: all eight)."""
    idx = list(range(B)) if which is None else list(which)
    salts = tuple(SALTS[j] for j in idx)
    f = EVALUATORS[evaluator](salts)
    cfg = dict(search=SETTINGS[setting] if isinstance(setting, str) else setting, max_plies=MOVES)
    cfg.update(kw)
    m = SearchModel(boards(idx), salts, SEED, BASE, evaluator=lambda b, board: f(b, board.squares(), int(board.turn)), wrong=wrong, **cfg)
    return m, f


def run(m, sims=SIMS, moves=MOVES, budgets=None):
    """``moves`` moves of ``sims`` lockstep steps each with tree reuse. Per move: the leaves of every step, the root children, what
    finish_move recorded."""
    out = []
    for _ in range(moves):
        if all(m.over):
            break
        if m.cap is not None or budgets is not None:
            m.begin_move(budgets)
        steps = [m.step() for _ in range(sims)]
        rc = [m.root_children(b) for b in range(m.B)]
        visited = [m.root_visited(b) for b in range(m.B)]
        events = m.finish_move()
        out.append({"steps": steps, "roots": rc, "visited": visited, "events": events, "finish": m.last})
    return out


def signature(moves):
    """What tells two runs apart: every step's leaves, every root's counts and Q bits, every recorded pi and move."""
    sig = []
    for mv in moves:
        sig.append(tuple(mv["steps"][i][b] for i in range(len(mv["steps"])) for b in range(len(mv["steps"][i]))))
        sig.append(tuple((r[1].tobytes(), r[2].tobytes()) for r in mv["roots"]))
        sig.append(tuple(None if f is None else (f["pi"].tobytes(), f["move"]) for f in mv["finish"]))
    return tuple(sig)
