"""CPU model of root exploration in the search (ccz_set_root_exploration, include/cczero.h): Dirichlet noise in
the root's priors, forced playouts, policy target pruning, the move drawn from the pruned pi without the sampler's mixing.

Plain Python + NumPy, one sequential MCTS per board. The rules come from ``oracle.OracleBoard``, the Gamma draws from
``oracle.det_gammas``, pi and the choice uniform from ``oracle.det_pi`` / ``oracle.det_choice_uniform``, priors and values from the
harness's ``make_evaluator("hash", salts)``. What the model restates itself is the arithmetic the feature touches: the backup in
float32 (``delta = val - q; delta /= n; q += delta``, mcts.py:68-71), the score (float32 product ``c_puct * P``, float64 elsewhere,
mcts.py:41-61) and the four rules below. tests/test_cpu_explore_model.py pins the neutral model to ``oracle.OracleMCTS`` and shows
that each rule, stated wrongly, gives another answer; tests/test_gpu_root_exploration.py compares the engine with the model, exactly.

The helpers take a ``wrong=`` name so that a test can ask for a mis-stated rule; the model itself never does."""
from __future__ import annotations

import functools
import math

import numpy as np

from gpu_harness import make_evaluator
from oracle import OracleBoard, det_choice_uniform, det_gammas, det_pi, det_sample

INF = float("inf")
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- the four rules
def noise_row(seed, gid, move_no, k, alpha, priors):
    """dir_i float32 [k]: g_i / G, G summed in index order in float64; the raw prior where G is not positive."""
    g = det_gammas(seed, gid, 1, move_no, k, alpha)[0]
    G = 0.0
    for x in g:
        G += float(x)
    return np.array([F32(float(g[i]) / G) if G > 0.0 else F32(priors[i]) for i in range(k)], F32)


def noisy_priors(priors, dirs, eps):
    """P'_i = (float32)((1 - eps) (double)P_i + eps (double)dir_i), from the STORED float32 dir_i."""
    p, d = np.asarray(priors, F32).astype(np.float64), np.asarray(dirs, F32).astype(np.float64)
    return ((1.0 - float(eps)) * p + float(eps) * d).astype(F32)


def forced_mask(N, pn, S, forced_k, wrong=None):
    """Children that score +inf although visited: N_i > 0 and (double)N_i < sqrt(forced_k * P'_i * S)."""
    N = np.asarray(N, np.int64)
    if not forced_k > 0.0:
        return np.zeros(len(N), bool)
    bound = np.sqrt(float(forced_k) * np.asarray(pn, F32).astype(np.float64) * float(S))
    n = N.astype(np.float64)
    return (N > 0) & ((n <= bound) if wrong == "le" else (n < bound))


def root_scores(N, Q, pn, root_n, c_puct, forced_k, wrong=None):
    """(scores float64 [k], forced bool [k]) of the root's children under exploration; the first maximum wins."""
    N = np.asarray(N, np.int64)
    u = (F32(c_puct) * np.asarray(pn, F32)).astype(np.float64)          # float32 product
    sc = np.asarray(Q, F32).astype(np.float64) + u * np.sqrt(np.float64(root_n)) / (1 + N).astype(np.float64)
    forced = forced_mask(N, pn, root_n - 1, forced_k, wrong)
    sc[(N == 0) | forced] = INF
    return sc, forced


def prune_counts(N, Q, pn, root_n, c_puct, forced_k, prune=True, wrong=None):
    """N' int64 [k] (include/cczero.h, rule 3). Returns (N', info) with info = per child ``gap`` (NaN for c* and unvisited)."""
    N = np.asarray(N, np.int64)
    k = len(N)
    out = N.copy()
    gaps = np.full(k, np.nan)
    if not prune or k == 0:
        return out, gaps
    cs = int(np.argmax(N))                                               # first maximum
    sq, S = math.sqrt(float(root_n)), float(root_n - 1)
    E = [float(F32(c_puct) * F32(pn[i])) * sq for i in range(k)]
    top = float(Q[cs]) + E[cs] / float(1 + int(N[cs]))
    for i in range(k):
        n = int(N[i])
        if n <= 0 or (i == cs and wrong != "best_too"):
            continue
        nf = math.ceil(math.sqrt(float(forced_k) * float(F32(pn[i])) * S))
        gap = top - float(Q[i])
        gaps[i] = gap
        if gap > 0.0:
            t = E[i] / gap - 1.0
            need = n if t >= n else max(0, math.ceil(t))                 # (anything >= n gives N' = n: no need for the huge integer)
        else:
            need = n
        np_ = min(n, max(need, n - nf, 0))
        if np_ < n and np_ <= 1 and wrong != "keep_small":
            np_ = 0
        out[i] = np_
    return out, gaps


def choose_move(pi, seed, gid, move_no, sampler_eps, sampler_alpha, mix):
    """Child index drawn on the choice word (0xfff). mix False (an explored move): from pi itself, searchsorted(cdf / sum, u, right)."""
    pi = np.asarray(pi, np.float64)
    if mix:
        return det_sample(seed, gid, move_no, pi, eps=sampler_eps, alpha=sampler_alpha)[0]
    acc, cdf = 0.0, []
    for x in pi:
        acc += float(x)
        cdf.append(acc)
    u = det_choice_uniform(seed, gid, move_no)
    idx = 0
    for i, c in enumerate(cdf):
        if c / acc <= u:
            idx = i + 1
    return min(idx, len(pi) - 1)


# ---------------------------------------------------------------------------------------------------------------- the tree
class Node:
    __slots__ = ("N", "Q", "P", "move", "kids")

    def __init__(self, prior, move):
        self.N, self.Q, self.P, self.move, self.kids = 0, F32(0.0), F32(prior), move, None


def backup(path, v):
    """Node.update_recursive(-leaf_value) (mcts.py:73-78): the leaf gets -v, its parent +v, ...; float32 throughout."""
    v = F32(v)
    d = len(path) - 1
    for j, node in enumerate(path):
        val = v if ((d - j) & 1) else F32(-v)
        node.N += 1
        delta = F32(val - node.Q)
        delta = F32(delta / F32(node.N))
        node.Q = F32(node.Q + delta)


@functools.lru_cache(maxsize=None)
def _evaluator(salts):
    return make_evaluator("hash", salts)


_EVAL_CACHE: dict = {}


def evaluate_sq(salts, b, sq, turn):
    """(P float32 [2086], v float32) of the harness's hash evaluator for board b's salt (memoised: every case re-visits the same leaves)."""
    sq = np.ascontiguousarray(sq, np.uint8)
    key = (salts[b], sq.tobytes(), int(turn))
    if key not in _EVAL_CACHE:
        P, V = _evaluator(tuple(salts))(sq[None, :], np.array([int(turn)], np.uint8), rows=[b])
        _EVAL_CACHE[key] = (P[0], V[0])
    return _EVAL_CACHE[key]


def evaluate(salts, b, board):
    return evaluate_sq(salts, b, board.squares(), int(board.turn))


class ExploreModel:
    """B boards, each a sequential search. ``cfg`` = dict(eps, alpha, forced_k, prune) or None (off); ``targets`` [B] (1 = policy
    target; exploration applies to those boards only). ``sampler_eps`` / ``sampler_alpha``: the engine's own (ccz_config), used on
    boards that are not explored. ``move_no`` [B]: the boards' move counters. ``wrong``: a mis-stated rule for the CPU tests."""

    def __init__(self, boards, salts, seed, board_id_base=0, c_puct=5, cfg=None, targets=None, sampler_eps=0.25, sampler_alpha=0.2,
                 temp=1.0, move_no=None, wrong=None, pool_budget=None):
        self.B = len(boards)
        self.boards = [b.copy() for b in boards]
        self.salts = tuple(salts)
        self.seed, self.base, self.c_puct = int(seed), int(board_id_base), c_puct
        self.cfg = None if cfg is None else dict(cfg)
        self.targets = [1] * self.B if targets is None else [int(t) for t in targets]
        self.sampler_eps, self.sampler_alpha = sampler_eps, float(F32(sampler_alpha))
        self.temp = temp
        self.move_no = [0] * self.B if move_no is None else list(move_no)
        self.wrong = wrong
        self.roots = [Node(1.0, -1) for _ in range(self.B)]
        self.over = [False] * self.B
        self.plies = [0] * self.B
        self.dirs = [None] * self.B          # (move_no, k, float32 row)
        self.stats = {"explored_moves": 0, "forced_selections": 0, "visits_pruned": 0, "children_pruned": 0}
        self.board_stats = [dict(self.stats) for _ in range(self.B)]
        self.facts = {"forced_hi": False, "pruned_hi": False, "big_to_zero": 0, "kept_whole_gap_le0": 0}
        self.pool_budget = pool_budget
        self.pruned_subtrees = 0

    # -------------------------------------------------------------------------------------------------------- search
    def explored(self, b):
        return self.cfg is not None and self.targets[b] != 0

    def _noise(self, b, root):
        k = len(root.kids)
        d = self.dirs[b]
        if d is None or d[0] != self.move_no[b] or d[1] != k:
            row = noise_row(self.seed, self.base + b, self.move_no[b], k, self.cfg["alpha"], [c.P for c in root.kids])
            self.dirs[b] = d = (self.move_no[b], k, row)
        return d[2]

    def _root_priors(self, b, root):
        raw = np.array([c.P for c in root.kids], F32)
        if self.wrong == "noise_in_nodes":       # the noise is written into the nodes, once per move
            d = self.dirs[b]
            if d is None or d[0] != self.move_no[b] or d[1] != len(root.kids):
                pn = noisy_priors(raw, self._noise(b, root), self.cfg["eps"])
                for c, p in zip(root.kids, pn):
                    c.P = F32(p)
                return pn
            return raw
        return noisy_priors(raw, self._noise(b, root), self.cfg["eps"])

    def _select_child(self, b, node, depth):
        kids = node.kids
        N = np.array([c.N for c in kids], np.int64)
        Q = np.array([c.Q for c in kids], F32)
        if depth == 0 and self.explored(b):
            sc, forced = root_scores(N, Q, self._root_priors(b, node), node.N, self.c_puct, self.cfg["forced_k"],
                                     "le" if self.wrong == "le" else None)
            i = int(np.argmax(sc))
            if forced[i]:
                self.board_stats[b]["forced_selections"] += 1
                if i >= 64:
                    self.facts["forced_hi"] = True
            return i
        P = np.array([c.P for c in kids], F32)
        u = (F32(self.c_puct) * P).astype(np.float64)
        sc = Q.astype(np.float64) + u * np.sqrt(np.float64(node.N)) / (1 + N).astype(np.float64)
        sc[N == 0] = INF
        return int(np.argmax(sc))

    def simulate(self, b):
        """One playout of board b (mcts.py:101-129)."""
        node, board, path, depth = self.roots[b], self.boards[b].copy(), [self.roots[b]], 0
        while node.kids:
            node = node.kids[self._select_child(b, node, depth)]
            board.push_id(node.move)
            path.append(node)
            depth += 1
        ids = board.legal_ids()
        end, tie = board.is_game_over(), board.is_tie()
        if not end and not tie:
            P, v = evaluate(self.salts, b, board)
            node.kids = [Node(P[i], i) for i in ids]
        else:
            v = F32(0.0) if (end and tie) else F32(-1.0)
        backup(path, v)

    def search(self, sims):
        """sims[b] playouts on every live board."""
        for b in range(self.B):
            if not self.over[b]:
                for _ in range(int(sims[b])):
                    self.simulate(b)

    # -------------------------------------------------------------------------------------------------------- inspection
    def root_children(self, b):
        kids = self.roots[b].kids or []
        return (np.array([c.move for c in kids], np.int32), np.array([c.N for c in kids], np.int32), np.array([c.Q for c in kids], F32),
                np.array([c.P for c in kids], F32))

    def noise(self, b):
        """float32 [k] of the move being searched, or an empty row."""
        d = self.dirs[b]
        root = self.roots[b]
        if d is None or not root.kids or d[0] != self.move_no[b] or d[1] != len(root.kids):
            return np.zeros(0, F32)
        return d[2]

    def targets_of(self, b):
        """(N', pi float64 [k]) the next finish_move records for board b; counts nothing."""
        root = self.roots[b]
        acts, N, Q, P = self.root_children(b)
        if self.explored(b) and len(N):
            pn = P if self.wrong == "noise_in_nodes" else noisy_priors(P, self._noise(b, root), self.cfg["eps"])
            Np, gaps = prune_counts(N, Q, pn, root.N, self.c_puct, self.cfg["forced_k"], self.cfg["prune"], self.wrong)
        else:
            Np, gaps = N.astype(np.int64), np.full(len(N), np.nan)
        return Np, det_pi(Np.astype(np.int32), self.temp), gaps

    # -------------------------------------------------------------------------------------------------------- the move boundary
    def finish_move(self, forced=None):
        """Records pi, chooses (or takes ``forced[b]`` >= 0), re-roots with the subtree kept, pushes. Returns per board a dict
        (pi float32 [k], acts, move, n_pruned [k]) or None for a finished board."""
        out = []
        for b in range(self.B):
            if self.over[b]:
                out.append(None)
                continue
            root = self.roots[b]
            acts, N, _, _ = self.root_children(b)
            assert len(N), "the model's boards are searched before they move"
            assert sum(int(n) for n in N) == root.N - 1, "S: the children's visits are the root's but one (no pruned subtree, no failed expansion)"
            Np, pi, gaps = self.targets_of(b)
            ex = self.explored(b)
            if ex:
                st = self.board_stats[b]
                st["explored_moves"] += 1
                st["visits_pruned"] += int((N - Np).sum())
                gone = (N > 0) & (Np == 0)
                st["children_pruned"] += int(gone.sum())
                self.facts["big_to_zero"] += int(((N > 1) & gone).sum())
                self.facts["kept_whole_gap_le0"] += int(((gaps <= 0.0) & (Np == N) & (N > 0)).sum())
                if gone[64:].any():
                    self.facts["pruned_hi"] = True
            want = -1 if forced is None else int(forced[b])
            if want >= 0:
                ci = int(np.nonzero(acts == want)[0][0])
            else:
                mix = (not ex) or self.wrong == "mix"
                ci = choose_move(pi, self.seed, self.base + b, self.move_no[b], self.sampler_eps, self.sampler_alpha, mix)
            move = int(acts[ci])
            out.append({"pi": pi.astype(F32), "pi64": pi, "explored": ex, "acts": acts, "move": move, "visits": N, "pruned": Np})
            self.roots[b] = root.kids[ci]                 # MCTS.update_with_move: the subtree is kept, priors as stored
            if self.pool_budget is not None:
                self.pruned_subtrees += int(_count(self.roots[b]) > self.pool_budget)
            self.boards[b].push_id(move)
            self.move_no[b] += 1
            self.plies[b] += 1
            self.over[b] = self.boards[b].is_game_over() or self.boards[b].is_tie()
        return out

    def totals(self):
        return {k: sum(s[k] for s in self.board_stats) for k in self.stats}


def _count(node):
    n, stack = 0, [node]
    while stack:
        x = stack.pop()
        n += 1
        if x.kids:
            stack.extend(x.kids)
    return n


# ---------------------------------------------------------------------------------------------------------------- the GPU test's inputs
B = 16
SEED, BASE = 7, 4096
SIMS_NARROW, SIMS_WIDE = 96, 160
WIDE, FEW = 14, 15                     # board indices of the 108-move position and of the position with fewer than 8 moves
SALTS = tuple(range(100, 100 + B))
FULL = {"eps": 0.25, "alpha": float(F32(0.2)), "forced_k": 2.0, "prune": True}
# the engine's default pool: (n_playout + 64) * 512 nodes per half, of which min(n_playout * 128, half of it) stay free at a re-root
N_PLAYOUT = SIMS_WIDE
POOL_BUDGET = (N_PLAYOUT + 64) * 512 - min(N_PLAYOUT * 128, (N_PLAYOUT + 64) * 256)


@functools.lru_cache(maxsize=None)
def inputs():
    """(boards, opening move lists or None, sims): 14 boards a few forced plies from the opening, at distinct positions with 30 to 50
    legal moves; board 14 on ``widest`` (108 moves); board 15 on ``pawns`` (7 moves). The plies are child (3 j + 5 p) mod k of ply p."""
    from golden_cases import STARTS
    boards, lines, seen = [], [], set()
    j = 0
    while len(boards) < 14:
        b, line = OracleBoard(), []
        for p in range(2 + j % 5):
            ids = b.legal_ids()
            mv = ids[(3 * j + 5 * p) % len(ids)]
            b.push_id(mv)
            line.append(int(mv))
        j += 1
        key = (b.squares().tobytes(), int(b.turn))
        if key in seen or b.is_game_over() or b.is_tie() or not 30 <= len(b.legal_ids()) <= 50:
            continue
        seen.add(key)
        boards.append(b)
        lines.append(line)
    boards.append(OracleBoard.from_array(STARTS["widest"], 1))
    boards.append(OracleBoard.from_array(STARTS["pawns"], 1))
    lines += [None, None]
    sims = [SIMS_NARROW] * B
    sims[WIDE] = SIMS_WIDE
    return boards, lines, sims


@functools.lru_cache(maxsize=None)
def run_case(eps, forced_k, prune, targets=None, moves=2, enabled=True, sampler_eps=0.25):
    """The model's answer for one case of tests/test_gpu_root_exploration.py: ``moves`` moves with tree reuse. Per move: root children,
    noise rows, what finish_move records and plays; then the counters and the facts that keep the case from passing vacuously."""
    boards, _, sims = inputs()
    cfg = {"eps": eps, "alpha": FULL["alpha"], "forced_k": forced_k, "prune": prune} if enabled else None
    m = ExploreModel(boards, SALTS, SEED, BASE, cfg=cfg, targets=None if targets is None else list(targets), sampler_eps=sampler_eps,
                     pool_budget=POOL_BUDGET)
    out = {"moves": []}
    for _ in range(moves):
        live = [not o for o in m.over]
        m.search(sims)
        rc = [m.root_children(b) for b in range(B)]
        noise = [m.noise(b) for b in range(B)]
        fin = m.finish_move()
        out["moves"].append({"live": live, "roots": rc, "noise": noise, "finish": fin})
    out["stats"] = m.totals()
    out["board_stats"] = m.board_stats
    out["facts"] = dict(m.facts)
    out["pruned_subtrees"] = m.pruned_subtrees
    return out
