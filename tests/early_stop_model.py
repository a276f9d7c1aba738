"""CPU model of the early stop per board (ccz_set_early_stop, include/cczero.h): single reply, visit gap, KLD gain.

Plain Python + NumPy, one sequential MCTS per board, on top of ``search_model.SearchModel`` (and through it the budgets, root
exploration, the solver, resignation and the records of tests/selfplay_model.py). Added is only what runs in front of a board's
simulation in a lockstep step: rules S1-S5, restated in Python floats (IEEE float64, no contraction) with ``det_log`` from
tests/gumbel_model.py.

  S1  the rules run when the game is not over, s < n_b, the root has children, the board is not stopped in this move and
      s >= min_sims; S2, S3, S4 in this order, the first that fires wins. s: the simulations of the move backed up so far; n_b: the
      board's budget, else the setting n_sims.
  S2  single_reply and k == 1: reason 1.
  S3  gap_factor f != 0: i1 the first maximum of N, N2 the maximum of the others (0 when k == 1); (N1 - N2) * f > n_b - s: reason 2.
  S4  kld_interval I > 0, s > 0, s % I == 0, s != snap_s: if there is a snapshot p and S_c = sum N > S_p = sum p, then with
      o = p_i / S_p, n = N_i / S_c, t_i = o * det_log(o / n) where p_i > 0, T the butterfly sum over 64 lanes of two children each,
      G = T / (S_c - S_p) < min_gain: reason 3. The snapshot becomes N, snap_s = s.
  S5  a stopped board selects nothing for the rest of the move (LEAF_SKIP); stops[reason] += 1, sims_saved += n_b - s; stopped and
      snap_s are cleared at the move boundary.

``wrong=`` names a mis-stated rule for the CPU test (tests/test_cpu_early_stop_model.py); the model itself never does: see WRONG."""
from __future__ import annotations

import search_model as sm
from gumbel_model import det_log
from selfplay_model import LEAF_SKIP

WRONG = ("gap_not_strict", "s_without_patch", "runner_up_low_half", "kld_reversed", "kld_not_per_node", "snapshot_same_s", "stale_after_move")
SINGLE_REPLY, VISIT_GAP, KLD_GAIN = 1, 2, 3
REASON_KEYS = {SINGLE_REPLY: "single_reply", VISIT_GAP: "visit_gap", KLD_GAIN: "kld_gain"}
OFF = {"enabled": False, "single_reply": False, "gap_factor": 0.0, "kld_interval": 0, "min_gain": 0.0, "min_sims": 0, "n_sims": 0}


def settings(single_reply=False, gap_factor=0.0, kld_interval=0, min_gain=0.0, min_sims=0):
    """The dict SelfPlayEngine.set_early_stop takes (without ``n_sims``: the engine's n_playout, the model's ``n_sims``)."""
    return {"single_reply": bool(single_reply), "gap_factor": float(gap_factor), "kld_interval": int(kld_interval),
            "min_gain": float(min_gain), "min_sims": int(min_sims)}


# ---------------------------------------------------------------------------------------------------------------- S3, S4
def visit_gap(N, wrong=None):
    """(N1, N2) of S3: the first maximum and the best of the other children."""
    N = [int(n) for n in N]
    i1 = max(range(len(N)), key=lambda i: (N[i], -i))
    others = [N[i] for i in range(len(N)) if i != i1 and (wrong != "runner_up_low_half" or i < 64)]
    return N[i1], max(others, default=0)


def butterfly(t):
    """The sum of R2 (search_model.visited_mass) over per-child terms t[0 .. k-1], k <= 128."""
    k = len(t)
    assert k <= 128
    m = [(t[l] if l < k else 0.0) + (t[l + 64] if l + 64 < k else 0.0) for l in range(64)]
    for s in (32, 16, 8, 4, 2, 1):
        m = [m[l] + m[l ^ s] for l in range(64)]
    return m[0]


def kld_gain(p, N, wrong=None):
    """G of S4, or None when it is not computed (no new visit among the root's children)."""
    p, N = [int(x) for x in p], [int(x) for x in N]
    Sp, Sc = sum(p), sum(N)
    if not Sc > Sp:
        return None
    t = []
    for pi, ni in zip(p, N):
        if wrong == "kld_reversed":
            o, n = float(ni) / float(Sc), float(pi) / float(Sp)
            t.append(o * det_log(o / n) if ni > 0 and pi > 0 else 0.0)
        elif pi > 0:
            o, n = float(pi) / float(Sp), float(ni) / float(Sc)
            t.append(o * det_log(o / n))
        else:
            t.append(0.0)
    T = butterfly(t)
    return T if wrong == "kld_not_per_node" else T / float(Sc - Sp)


# ---------------------------------------------------------------------------------------------------------------- the search
class EarlyStopModel(sm.SearchModel):
    """``early_stop``: the dict of ``settings`` or None (off: SearchModel as it is); ``n_sims``: the simulations of a move on a board
    without a budget. Everything else as in SearchModel."""

    def __init__(self, boards, salts, seed, board_id_base=0, c_puct=5, early_stop=None, n_sims=sm.SIMS, wrong=None, **kw):
        assert wrong is None or wrong in WRONG
        super().__init__(boards, salts, seed, board_id_base, c_puct, **kw)
        self.ecfg = None if early_stop is None else dict(early_stop)
        self.n_sims = int(n_sims)
        self.ewrong = wrong
        self.stopped = [0] * self.B
        self.snap = [None] * self.B
        self.snap_s = [-1] * self.B
        self.backed = [False] * self.B       # the selection under way follows a backup of the same launch
        self.estats = {"single_reply": 0, "visit_gap": 0, "kld_gain": 0, "sims_saved": 0, "evaluations": 0}
        self.stop_log = []                   # (board, move number, reason, s, n_b) of every stop
        self.efacts = {"gap_runner_up_hi": 0, "gap_leader_hi": 0, "reselect_at_interval": 0}

    def n_b(self, b):
        return self.budget[b] if self.budget[b] is not None else self.n_sims

    def searching(self):
        return sum(1 for b in range(self.B) if not self.over[b] and not (self.budget[b] is not None and self.used[b] >= self.budget[b])
                   and not (self.ecfg is not None and self.stopped[b]))

    def _rules(self, b):
        """S1-S5 at one selection of board b (not over, budget not spent): the reason it is stopped with, 0: it searches on."""
        c, w = self.ecfg, self.ewrong
        if self.stopped[b]:
            return self.stopped[b]
        kids = self.roots[b].kids
        if not kids:
            return 0
        s = self.used[b] - (1 if (w == "s_without_patch" and self.backed[b]) else 0)
        n_b = self.n_b(b)
        if s >= n_b or s < c["min_sims"]:
            return 0
        N = [int(k.N) for k in kids]
        reason = 0
        if c["single_reply"] and len(N) == 1:
            reason = SINGLE_REPLY
        if not reason and c["gap_factor"] != 0.0:
            n1, n2 = visit_gap(N, w)
            lhs, rhs = float(n1 - n2) * c["gap_factor"], float(n_b - s)
            if lhs >= rhs if w == "gap_not_strict" else lhs > rhs:
                reason = VISIT_GAP
                i1 = N.index(n1)
                self.efacts["gap_leader_hi"] += int(i1 >= 64)
                self.efacts["gap_runner_up_hi"] += int(n2 > 0 and n2 not in [N[i] for i in range(min(64, len(N))) if i != i1])
        I = c["kld_interval"]
        if not reason and I > 0 and s > 0 and s % I == 0 and (s != self.snap_s[b] or w == "snapshot_same_s"):
            if self.snap_s[b] >= 0:
                g = kld_gain(self.snap[b], N, w)
                if g is not None and g < c["min_gain"]:
                    reason = KLD_GAIN
            self.snap[b], self.snap_s[b] = N, s
            self.estats["evaluations"] += 1
        if reason:
            self.stopped[b] = reason
            self.estats[REASON_KEYS[reason]] += 1
            self.estats["sims_saved"] += n_b - s
            self.stop_log.append((b, self.move_no[b], reason, s, n_b))
        return reason

    def step(self, reselect=False):
        """One lockstep step (SelfPlayModel.step) with the rules in front of every board's simulation. ``reselect``: the selection
        is made twice without a backup in between (ccz_select_leaves after ccz_step): the rules run again and the leaf is found
        -- and its depth counted -- a second time."""
        if self.ecfg is None and not reselect:
            return super().step()
        out, skipped, proved = [], False, False
        for b in range(self.B):
            if self.over[b] or (self.budget[b] is not None and self.used[b] >= self.budget[b]):
                out.append((LEAF_SKIP, None, None))
                skipped |= not self.over[b]
                continue
            stop = self._rules(b) if self.ecfg is not None else 0
            if not stop and reselect:
                self.backed[b] = False
                if self.ecfg is not None:
                    I = self.ecfg["kld_interval"]
                    self.efacts["reselect_at_interval"] += int(I > 0 and self.used[b] > 0 and self.used[b] % I == 0)
                    stop = self._rules(b)
            if stop:
                out.append((LEAF_SKIP, None, None))
                skipped = True
                continue
            before = self.board_proven[b]
            out.append(self.simulate(b))
            if reselect:
                self.sum_depth += out[-1][2]
            self.backed[b] = True
            proved |= self.board_proven[b] > before
        self.xfacts["skip_while_proving"] += int(skipped and proved)
        return out

    def finish_move(self, forced=None):
        live = [not o for o in self.over]
        events = super().finish_move(forced)
        for b in range(self.B):
            if live[b]:
                self.backed[b] = False
                if self.ewrong != "stale_after_move":
                    self.stopped[b], self.snap_s[b], self.snap[b] = 0, -1, None
        return events

    def status(self):
        """(reason uint8 list, sims list) as ccz_early_stop_status reports them."""
        return list(self.stopped), list(self.used)


# ---------------------------------------------------------------------------------------------------------------- the GPU test's inputs
B, SIMS, MOVES = sm.B, sm.SIMS, sm.MOVES
SETTINGS = {
    "gap": settings(single_reply=True, gap_factor=1.0),
    "gap_1p5": settings(gap_factor=1.5),
    "kld": settings(kld_interval=16, min_gain=0.002),
    "all": settings(single_reply=True, gap_factor=1.0, kld_interval=16, min_gain=0.002, min_sims=24),
}
RESELECT = (16, 33)            # steps of every move whose selection is made twice (16: s is a multiple of the KLD interval)


def case(setting, evaluator="peaked", wrong=None, which=None, n_sims=SIMS, **kw):
    """(model, f): the model of one case of tests/test_gpu_early_stop.py and the evaluator ``f(b, squares, turn)`` both sides are fed.
    ``setting``: a name of SETTINGS, a dict, or None (off). ``which``: board indices of ``search_model.inputs()`` (default: all)."""
    idx = list(range(B)) if which is None else list(which)
    salts = tuple(sm.SALTS[j] for j in idx)
    f = sm.EVALUATORS[evaluator](salts)
    cfg = dict(early_stop=SETTINGS[setting] if isinstance(setting, str) else setting, max_plies=MOVES, n_sims=n_sims)
    cfg.update(kw)
    m = EarlyStopModel(sm.boards(idx), salts, sm.SEED, sm.BASE, evaluator=lambda b, board: f(b, board.squares(), int(board.turn)), wrong=wrong, **cfg)
    return m, f


def run(m, sims=SIMS, moves=MOVES, budgets=None, reselect=RESELECT, forced=None):
    """``moves`` moves of ``sims`` lockstep steps each with tree reuse. ``budgets``: per move a list of per-board budgets (None: none).
    ``forced``: per move the moves to play (None: the model's own). Per move: the leaves and the stop status of every step, the
    root children, what finish_move recorded."""
    out = []
    for mv in range(moves):
        if all(m.over):
            break
        if m.cap is not None:
            m.begin_move()
        elif budgets is not None:
            m.begin_move(budgets[mv])
        steps, status = [], []
        for i in range(sims):
            steps.append(m.step(reselect=i in reselect))
            status.append(m.status())
        rc = [m.root_children(b) for b in range(m.B)]
        events = m.finish_move(None if forced is None else forced[mv])
        out.append({"steps": steps, "status": status, "roots": rc, "events": events, "finish": m.last})
    return out


def signature(m, moves):
    """What tells two runs apart: every step's leaves and stop status, every root's counts and Q bits, every recorded pi and move,
    the counters."""
    sig = []
    for mv in moves:
        sig.append(tuple(tuple(row) for row in mv["steps"]))
        sig.append(tuple((tuple(r), tuple(s)) for r, s in mv["status"]))
        sig.append(tuple((r[1].tobytes(), r[2].tobytes()) for r in mv["roots"]))
        sig.append(tuple(None if f is None else (f["pi"].tobytes(), f["move"]) for f in mv["finish"]))
    sig.append(tuple(sorted(m.estats.items())))
    return tuple(sig)


def stop_sims(m, n_moves):
    """Per move a list of per-board budgets: the simulations the board's move ended with (s at its stop, else n_sims) -- what the
    twin run without the feature is given (S5's consequence)."""
    rows = [[m.n_sims] * m.B for _ in range(n_moves)]
    for b, move_no, _, s, _ in m.stop_log:
        if move_no < n_moves:
            rows[move_no][b] = max(1, s)
    return rows
