"""CPU model of the Gumbel root search (ccz_set_gumbel, include/cczero.h): one Gumbel draw per root child and
move, sequential halving over the considered moves by the considered-visits sequence, completed Q and sigma, the played move and the
policy target pi' = softmax(logit + sigma).

Plain Python + NumPy, one sequential MCTS per board. The tree node, the float32 backup and the evaluator come from
tests/explore_model.py; the budgets, the solver's stop rule and proof walk, resignation and the records from tests/selfplay_model.py
(``SelfPlayModel`` is the base class, with root exploration off: the two exclude each other); Philox from tests/budget_twin.py; log and
exp from the oracle's ``xq_det_log`` / ``xq_det_exp``. Restated here are the five rules of the header comment, in Python floats (IEEE
float64, no contraction), with every sum in child order.

The helpers take a ``wrong=`` name so that a test can ask for a mis-stated rule; the model itself never does:
``gumbel_sign`` (g = +log(-log u)), ``n_not_m`` (total visits where move-visits are meant), ``q_signed`` (Q left in [-1, 1]),
``v0_sign`` (the root's mean not turned to its side to move), ``ignore_target`` (every child a candidate, whatever the sequence says)."""
from __future__ import annotations

import numpy as np

import oracle
from budget_twin import ua
from explore_model import F32
from resign_model import root_value64
from selfplay_model import LEAF_SKIP, SelfPlayModel
from solver_model import SNode

WRONG = ("gumbel_sign", "n_not_m", "q_signed", "v0_sign", "ignore_target")
GUMBEL_DRAW = 0xfffff            # the draw index of the Gumbel word; the Gamma loop of a child stops below 0xffff2


def det_log(x):
    return float(oracle.lib().xq_det_log(float(x)))


def det_exp(x):
    return float(oracle.lib().xq_det_exp(float(x)))


# ---------------------------------------------------------------------------------------------------------------- the five rules
def gumbel_draw(seed, gid, move_no, i, wrong=None):
    """g_i = -log(-log(ua)) on word (child i, draw 0xfffff) of the board's Philox stream for the move."""
    u = ua(seed, gid, move_no, child=i, draw=GUMBEL_DRAW)
    g = det_log(-det_log(u))
    return g if wrong == "gumbel_sign" else -g


def logit_of(p):
    return det_log(float(F32(p)))


def sequence(m, n):
    """seq(m, n): the move-visits of the child to visit at simulation t of a move, t = 0 .. n - 1."""
    if m <= 1:
        return list(range(n))
    L = (m - 1).bit_length()                     # ceil(log2 m)
    out, v, c = [], 0, m
    while len(out) < n:
        x = max(1, n // (L * c))
        for _ in range(x):
            out.extend([v] * c)
            v += 1
        c = max(2, c // 2)
    return out[:n]


def completed_q(N, Q, P, root_q, wrong=None):
    """(cq float64 [k], v_mix): the visited children's own value in [0, 1], v_mix for the others."""
    k = len(N)
    signed = wrong == "q_signed"
    qt = [float(F32(Q[i])) if signed else (float(F32(Q[i])) + 1.0) / 2.0 for i in range(k)]
    rq = float(F32(root_q))
    if wrong == "v0_sign":
        v0 = rq if signed else (rq + 1.0) / 2.0
    else:
        v0 = -rq if signed else (-rq + 1.0) / 2.0
    S = float(sum(int(n) for n in N))
    wsum = psum = 0.0
    any_visited = False
    for i in range(k):
        if int(N[i]) > 0:
            any_visited = True
            wsum += float(F32(P[i])) * qt[i]
            psum += float(F32(P[i]))
    with np.errstate(all="ignore"):
        v_mix = float((np.float64(v0) + np.float64(S) * np.float64(wsum) / np.float64(psum)) / np.float64(1.0 + S)) if any_visited else v0
    return [qt[i] if int(N[i]) > 0 else v_mix for i in range(k)], v_mix


def sigmas(N, cq, c_visit, c_scale):
    top = float(max(int(n) for n in N)) if len(N) else 0.0
    return [(float(c_visit) + top) * float(c_scale) * q for q in cq]


def move_visits(N, n0, wrong=None):
    """M_i = N_i - N0_i: the visits of this move, without the kept subtree's."""
    return [int(n) for n in N] if wrong == "n_not_m" else [int(n) - int(z) for n, z in zip(N, n0)]


def candidates(M, m, n_eff, wrong=None):
    """Child indices the root may choose among, given the move-visits M."""
    k = len(M)
    if wrong == "ignore_target":
        return list(range(k))
    t = sum(int(x) for x in M)
    if t < n_eff:
        want = sequence(m, n_eff)[t]
        c = [i for i in range(k) if int(M[i]) == want]
        if c:
            return c
    top = max(int(x) for x in M)
    return [i for i in range(k) if int(M[i]) == top]


def first_max(scores, cand):
    """First maximum in child order among ``cand``; None when every candidate's score is NaN."""
    best, bi = None, None
    for i in cand:
        s = scores[i]
        if s == s and (best is None or s > best):
            best, bi = s, i
    return bi


def improved_policy(logits, sig):
    """pi' float64 [k] = softmax(logit + sigma) with the deterministic exp and the sum in child order."""
    s = [l + x for l, x in zip(logits, sig)]
    mx = max(s)
    e = [det_exp(x - mx) for x in s]
    acc = 0.0
    for x in e:
        acc += x
    return np.array([x / acc for x in e], np.float64)


# ---------------------------------------------------------------------------------------------------------------- evaluators
def hash_evaluator(salts):
    """``f(b, squares, turn) -> (P float32 [2086], v float32)``: the harness's hash evaluator with board b's salt (near-uniform priors)."""
    from explore_model import evaluate_sq
    return lambda b, sq, turn: evaluate_sq(tuple(salts), b, sq, turn)


def peaked_evaluator(salts):
    """A scripted evaluator with peaked priors: 0.6 and 0.2 on two legal moves the position's hash picks, the remaining 0.2 spread
    evenly over the others (k = 2: 0.75 / 0.25, k = 1: 1); the value is the hash evaluator's. The hash evaluator's priors are all about
    1 / 2086, which leaves the logit term of the score idle."""
    import zlib
    from explore_model import evaluate_sq
    from oracle import OracleBoard

    memo = {}

    def f(b, sq, turn):
        sq = np.ascontiguousarray(sq, np.uint8)
        key = (salts[b], sq.tobytes(), int(turn))
        if key not in memo:
            ids = OracleBoard.from_array(sq, int(turn)).legal_ids()
            k = len(ids)
            P = np.zeros(2086, F32)
            if k:
                h = zlib.crc32(sq.tobytes() + bytes([int(turn), salts[b] & 0xff]))
                w = [1.0] if k == 1 else [0.75, 0.25] if k == 2 else [0.6, 0.2] + [0.2 / (k - 2)] * (k - 2)
                for j, x in enumerate(w):                 # the peak starts at child h mod k and runs on in child order
                    P[ids[(h + j) % k]] = F32(x)
            memo[key] = (P, evaluate_sq(tuple(salts), b, sq, turn)[1])
        return memo[key]
    return f


# ---------------------------------------------------------------------------------------------------------------- the search
class GumbelModel(SelfPlayModel):
    """B boards, each a sequential search. ``gumbel`` = dict(n_sims, max_considered, c_visit, c_scale) or None (off: SelfPlayModel as it
    is). ``solver`` / ``resign`` / ``cap`` / ``max_plies`` / ``evaluator(b, board)`` as in SelfPlayModel. ``wrong``: see WRONG."""

    def __init__(self, boards, salts, seed, board_id_base=0, c_puct=5, gumbel=None, solver=False, resign=None, cap=None, max_plies=None,
                 evaluator=None, sampler_eps=0.25, temp=1.0, wrong=None):
        super().__init__(boards, salts, seed, board_id_base, c_puct, explore=None, solver=solver, resign=resign, cap=cap,
                         sampler_eps=sampler_eps, temp=temp, max_plies=max_plies, evaluator=evaluator)
        assert wrong is None or wrong in WRONG
        self.gcfg = None if gumbel is None else dict(gumbel)
        self.gwrong = wrong
        self.grow = [None] * self.B                 # per board: the row of its current move
        self.gstats = {"gumbel_moves": 0, "considered_sum": 0, "offvisit_moves": 0}
        self.leaf = [None] * self.B                 # per board: (status, k, depth, ids, squares, turn) of its last leaf
        self._moves = []                            # the moves of the descent under way
        self.gfacts = {"kept_n0": 0, "fallback": 0, "hi_choice": 0, "target_gt0": 0}

    # -------------------------------------------------------------------------------------------------------- rows
    def _make_row(self, b, root):
        kids = root.kids
        k = len(kids)
        gid, mv = self.base + b, self.move_no[b]
        n_b = self.budget[b] if self.budget[b] is not None else int(self.gcfg["n_sims"])
        return {"move_no": mv, "k": k,
                "g": [gumbel_draw(self.seed, gid, mv, i, self.gwrong) for i in range(k)],
                "logit": [logit_of(c.P) for c in kids],
                "n0": [int(c.N) for c in kids],
                "n_eff": max(1, n_b - self.used[b]),
                "m": min(int(self.gcfg["max_considered"]), k)}

    def _row(self, b, root, store):
        r = self.grow[b]
        if r is not None and r["move_no"] == self.move_no[b] and r["k"] == len(root.kids):
            return r
        r = self._make_row(b, root)
        if store:
            self.grow[b] = r
            self.gfacts["kept_n0"] += int(any(r["n0"]))
        return r

    def root_row(self, b):
        """(g, logit, n0, n_eff) as ccz_gumbel_root reports them, or None on a board without a row for its current move."""
        r, root = self.grow[b], self.roots[b]
        if r is None or not root.kids or r["move_no"] != self.move_no[b] or r["k"] != len(root.kids):
            return None
        return np.array(r["g"], np.float64), np.array(r["logit"], np.float64), np.array(r["n0"], np.int32), r["n_eff"]

    def _scores(self, root, r):
        kids = root.kids
        N = [int(c.N) for c in kids]
        cq, _ = completed_q(N, [c.Q for c in kids], [c.P for c in kids], root.Q, self.gwrong)
        sig = sigmas(N, cq, self.gcfg["c_visit"], self.gcfg["c_scale"])
        M = move_visits(N, r["n0"], self.gwrong)
        return [r["g"][i] + r["logit"][i] + sig[i] for i in range(len(kids))], sig, M

    # -------------------------------------------------------------------------------------------------------- selection
    def _select_child(self, b, node, depth):
        i = self._root_child(b, node) if depth == 0 and self.gcfg is not None else super()._select_child(b, node, depth)
        self._moves.append(node.kids[i].move)
        return i

    def _root_child(self, b, node):
        r = self._row(b, node, True)
        sc, _, M = self._scores(node, r)
        t = sum(M)
        cand = candidates(M, r["m"], r["n_eff"], self.gwrong)
        if t >= r["n_eff"]:
            self.gfacts["fallback"] += 1
        elif sequence(r["m"], r["n_eff"])[t] > 0:
            self.gfacts["target_gt0"] += 1
        i = first_max(sc, cand)
        assert i is not None, "NaN scores: the model's evaluators give none"
        self.gfacts["hi_choice"] += int(i >= 64)
        return i

    def simulate(self, b):
        """One playout of board b (SelfPlayModel.simulate); keeps the leaf it reached: (status, k, depth, ids, squares, turn), the last
        three None when the descent stopped at a proven node (no move generation, no evaluator row)."""
        self._moves = []
        stops = self.proven_stops
        status, k, depth = super().simulate(b)
        ids = sq = turn = None
        if self.proven_stops == stops:
            board = self.boards[b].copy()
            for mv in self._moves:
                board.push_id(mv)
            ids, sq, turn = board.legal_ids(), board.squares(), int(board.turn)
        self.leaf[b] = (status, k, depth, ids, sq, turn)
        return status, k, depth

    # -------------------------------------------------------------------------------------------------------- the move boundary
    def gumbel_targets(self, b):
        """(pi' float64 [k], child the rule plays, m) of the next finish_move of board b; counts nothing."""
        root = self.roots[b]
        r = self._row(b, root, False)
        sc, sig, M = self._scores(root, r)
        top = max(M)
        ci = first_max(sc, [i for i in range(len(M)) if M[i] == top])
        return improved_policy(r["logit"], sig), ci, r["m"]

    def finish_move(self, forced=None):
        """SelfPlayModel.finish_move with the Gumbel rule's pi' and move in place of the visit softmax and the draw."""
        if self.gcfg is None:
            return super().finish_move(forced)
        events, self.last = [], []
        for b in range(self.B):
            g = self.games[b]
            if self.over[b]:
                events.append("over")
                self.last.append(None)
                continue
            root = self.roots[b]
            if self.max_plies is not None and self.plies[b] >= self.max_plies:
                g.end(-1)
                self.over[b] = True
                events.append("cap")
                self.last.append(None)
                continue
            board = self.boards[b]
            acts, N, Q, _ = self.root_children(b)
            assert len(N), "the model's boards are searched before they move"
            pi, ci, m = self.gumbel_targets(b)
            want = -1 if forced is None else int(forced[b])
            if want >= 0:
                ci = int(np.nonzero(acts == want)[0][0])
            self.gstats["gumbel_moves"] += 1
            self.gstats["considered_sum"] += m
            self.gstats["offvisit_moves"] += int(ci != int(np.argmax(N)))
            self.plies_rec[b].append({"sq": board.squares(), "turn": int(board.turn), "ids": acts.astype(np.uint16), "pi": pi.astype(F32)})
            v64 = root_value64(N, Q)
            u = ua(self.seed, self.base + b, self.move_no[b], 0xffd)
            ev = g.record(int(board.turn), v64, self.targets[b], want >= 0, u, enabled=self.rule is not None)
            if self.rule is not None and ev:
                self.xfacts[ev] += 1
            rec = {"pi": pi.astype(F32), "pi64": pi, "acts": acts, "visits": N, "move": -1, "child": ci}
            self.last.append(rec)
            self.move_no[b] += 1
            self.plies[b] += 1
            self.used[b] = 0
            if ev == "resign":
                self.roots[b] = SNode(1.0, -1)
                self.over[b] = True
                events.append(ev)
                continue
            rec["move"] = int(acts[ci])
            self.roots[b] = root.kids[ci]
            board.push_id(rec["move"])
            if board.is_game_over() or board.is_tie():
                o = board.outcome()
                g.end(-1 if (o is None or o.winner is None) else int(o.winner))
                self.over[b] = True
            events.append(ev)
        return events


__all__ = ["GumbelModel", "LEAF_SKIP", "WRONG", "candidates", "completed_q", "first_max", "gumbel_draw", "improved_policy", "logit_of",
           "sequence", "sigmas"]


# ---------------------------------------------------------------------------------------------------------------- the GPU test's inputs
B = 8
SEED, BASE = 31, 8192
SALTS = tuple(range(200, 200 + B))
MOVES = 6
SETTINGS = {"n32_m16": dict(n_sims=32, max_considered=16, c_visit=50.0, c_scale=1.0),
            "n8_m4": dict(n_sims=8, max_considered=4, c_visit=50.0, c_scale=1.0)}
EVALUATORS = {"hash": hash_evaluator, "peaked": peaked_evaluator}


def inputs():
    """8 boards as (squares, turn): the seven opening positions of selfplay_model.inputs() (30 to 50 legal moves) and ``pawns`` (7)."""
    import selfplay_model as spm
    return spm.inputs()[7:15]


def boards():
    from oracle import OracleBoard
    return [OracleBoard.from_array(sq, turn) for sq, turn in inputs()]


def case(setting, evaluator="hash", wrong=None, **kw):
    """(model, f): the model of one case of tests/test_gpu_gumbel.py and the evaluator ``f(b, squares, turn)`` both sides are fed."""
    f = EVALUATORS[evaluator](SALTS)
    cfg = dict(gumbel=SETTINGS[setting] if isinstance(setting, str) else setting, max_plies=MOVES)
    cfg.update(kw)
    m = GumbelModel(boards(), SALTS, SEED, BASE, evaluator=lambda b, board: f(b, board.squares(), int(board.turn)), wrong=wrong, **cfg)
    return m, f
