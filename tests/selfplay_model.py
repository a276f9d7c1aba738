"""CPU model of self-play with EVERY search option on at once: per-board budgets drawn by playout-cap randomisation, root
exploration (noise, forced playouts, target pruning), the MCTS-solver and resignation with play-on -- the combination the README's
``collect`` command lines run and that ``BatchedSelfPlay.advance`` drives through the planned, cached, compact launch sequence.

Plain Python + NumPy, one sequential MCTS per board, composed from what the three single-feature models state: the tree node, the
float32 backup and the four exploration rules of tests/explore_model.py (``ExploreModel`` is the base class: noise rows, noisy root
priors, pruned targets), the proof byte, ``combine``, the proven-stop rule and the proof walk of tests/solver_model.py
(``SolverModel._prove`` / ``root_proof`` / ``proof_move`` are borrowed as they are), ``root_value64`` and the per-game state machine
``Game`` of tests/resign_model.py, the Philox twins of tests/budget_twin.py. Restated here is only the glue, i.e. what
include/cczero.h says about how the features meet:

* selection: at depth 0 of an explored board (exploration on, the move a policy target) the score uses the noisy priors and the
  forced rule; whatever child is chosen, at any depth and by whatever rule, its proof byte then ends the descent (status WIN / LOSS /
  DRAW, k = 0, value +1 / -1 / 0, the proof walk) exactly as in ``SolverModel.simulate``;
* a board searches ``budget`` simulations per move and shows ``LEAF_SKIP`` afterwards; exploration applies to target boards only;
* the move boundary, in k_finish_move's order: the ply cap; pi from the pruned counts on an explored board (the exploration counters
  move here, also on a ply that then resigns); the root value from the counts AS SEARCHED; the resignation state machine with the
  lot on word 0xffd; the move drawn unmixed on an explored board and mixed otherwise; the re-root with the proof bytes kept.

``wrong=`` names a mis-stated interaction for the CPU test (tests/test_cpu_selfplay_model.py); the model itself never does."""
from __future__ import annotations

import functools

import numpy as np

import explore_model as em
import solver_cases as sc
from budget_twin import ua
from explore_model import F32, ExploreModel, backup, choose_move, evaluate
from oracle import OracleBoard
from resign_model import Game, Rule, root_value64, stats_of
from solver_model import DRAW, LEAF_DRAW, LEAF_EXPAND, LEAF_LOSS, LEAF_WIN, LOSS, WIN, SNode, SolverModel, state_of

LEAF_SKIP = 3
REC_BYTES, HDR, IDS, PI = 880, 96, 112, 368
WRONG = ("forced_ignores_proof", "reroot_drops_proof", "resign_on_pruned_counts")


class SelfPlayModel(ExploreModel):
    """B boards, each a sequential search. ``explore``: dict(eps, alpha, forced_k, prune) or None; ``solver``: bool; ``resign``: a
    ``resign_model.Rule`` or None; ``cap``: (n_full, n_fast, p_full) of ccz_draw_budgets or None (then ``begin_move`` takes the
    budgets); ``max_plies``: the ply cap (None: none); ``evaluator(b, board) -> (P float32 [2086], v float32)`` as in SolverModel."""

    _prove = SolverModel._prove
    root_proof = SolverModel.root_proof
    proof_move = SolverModel.proof_move

    def __init__(self, boards, salts, seed, board_id_base=0, c_puct=5, explore=None, solver=False, resign=None, cap=None,
                 sampler_eps=0.25, sampler_alpha=0.2, temp=1.0, max_plies=None, evaluator=None, wrong=None):
        super().__init__(boards, salts, seed, board_id_base, c_puct, cfg=explore, sampler_eps=sampler_eps, sampler_alpha=sampler_alpha,
                         temp=temp)
        assert wrong is None or wrong in WRONG
        self.glue_wrong = wrong
        self.roots = [SNode(1.0, -1) for _ in range(self.B)]
        self.solver = bool(solver)
        self.evaluator = evaluator if evaluator is not None else (lambda b, board: evaluate(self.salts, b, board))
        self.nodes_proven = self.proven_stops = self.rows = self.sims = 0
        self.board_proven = [0] * self.B
        self.rule, self.cap, self.max_plies = resign, cap, max_plies
        self.games = [Game(resign if resign is not None else Rule(-1.0, 0, 0, 0.0)) for _ in range(self.B)]
        self.budget = [None] * self.B                  # None: unlimited
        self.used = [0] * self.B
        self.plies_rec = [[] for _ in range(self.B)]   # per board: the recorded plies of its game
        self.xfacts = {"forced_on_proven": 0, "pruned_at_proven_root": 0, "root_proven_at_boundary": set(), "proofs_after_reroot": set(),
                       "fast_with_proofs": 0, "resign": 0, "playon": 0, "below_no_fire": 0, "skip_while_proving": 0, "stops_d1": set()}

    # -------------------------------------------------------------------------------------------------------- one simulation
    def _select(self, b, node, depth):
        """(child index, whether the forced rule chose it): ExploreModel's selection, which counts a forced choice where it makes it."""
        st = self.board_stats[b]
        before = st["forced_selections"]
        i = self._select_child(b, node, depth)
        return i, st["forced_selections"] > before

    def simulate(self, b):
        """One playout of board b. Returns (status, k, depth) of its leaf as the engine reports them."""
        node, path, moves, stopped = self.roots[b], [self.roots[b]], [], 0
        while node.kids:
            i, forced = self._select(b, node, len(moves))
            node = node.kids[i]
            path.append(node)
            moves.append(node.move)
            if self.solver and state_of(node.proof):
                if forced:
                    self.xfacts["forced_on_proven"] += 1
                    if self.glue_wrong == "forced_ignores_proof":
                        continue
                stopped = state_of(node.proof)
                if len(moves) == 1:
                    self.xfacts["stops_d1"].add((b, self.plies[b], i))   # (board, ply, child index)
                break
        depth = len(path) - 1
        if stopped:
            status = {WIN: LEAF_WIN, LOSS: LEAF_LOSS, DRAW: LEAF_DRAW}[stopped]
            k = 0
            v = {WIN: F32(1.0), LOSS: F32(-1.0), DRAW: F32(0.0)}[stopped]
        else:
            board = self.boards[b].copy()
            for mv in moves:
                board.push_id(mv)
            ids = board.legal_ids()
            end, tie = board.is_game_over(), board.is_tie()
            k = len(ids)
            if not end and not tie:
                status = LEAF_EXPAND
                P, v = self.evaluator(b, board)
                node.kids = [SNode(P[i], i) for i in ids]
                self.rows += 1
            else:
                status = LEAF_DRAW if (end and tie) else LEAF_LOSS
                v = F32(0.0) if status == LEAF_DRAW else F32(-1.0)
        backup(path, v)
        self.sims += 1
        self.used[b] += 1
        if self.solver and status != LEAF_EXPAND:
            before = self.nodes_proven
            self._prove(path, status, stopped)
            self.board_proven[b] += self.nodes_proven - before
        return status, k, depth

    # -------------------------------------------------------------------------------------------------------- a move's search
    def begin_move(self, budgets=None, targets=None):
        """The budgets of the move about to be searched: drawn on word 0xffe (``cap``), or as given (None: unlimited, all targets)."""
        for b in range(self.B):
            if self.cap is not None:
                n_full, n_fast, p_full = self.cap
                full = ua(self.seed, self.base + b, self.move_no[b]) < p_full
                self.budget[b], self.targets[b] = (n_full if full else n_fast), int(full)
            else:
                self.budget[b] = None if budgets is None else max(1, int(budgets[b]))
                self.targets[b] = 1 if (budgets is None or targets is None) else int(targets[b] != 0)
            self.used[b] = 0
        return [self.budget[b] for b in range(self.B)]

    def step(self):
        """One lockstep step: per board (status, k, depth), or (LEAF_SKIP, None, None) where the board selects nothing."""
        out, skipped, proved = [], False, False
        for b in range(self.B):
            if self.over[b] or (self.budget[b] is not None and self.used[b] >= self.budget[b]):
                out.append((LEAF_SKIP, None, None))
                skipped |= not self.over[b]
                continue
            before = self.board_proven[b]
            out.append(self.simulate(b))
            proved |= self.board_proven[b] > before
        self.xfacts["skip_while_proving"] += int(skipped and proved)
        return out

    def search(self, steps):
        return [self.step() for _ in range(int(steps))]

    def solver_stats(self):
        """ccz_get_solver_stats: the two running sums, and the boards whose game is running and whose root is proven now."""
        live = sum(1 for b in range(self.B) if self.solver and not self.over[b] and state_of(self.roots[b].proof))
        return {"nodes_proven": self.nodes_proven, "proven_stops": self.proven_stops, "roots_proven": live}

    # -------------------------------------------------------------------------------------------------------- the move boundary
    def finish_move(self, forced=None):
        """Per board: "over" (no game), "cap", "resign", "playon" or None (a move was played); ``self.last`` holds per board what was
        recorded (pi float32, acts, move, visits, pruned) or None."""
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
            assert len(N), "the model's boards are searched before they move"   # (sum N may be < root.N - 1: a kept proven node was visited, not descended)
            Np, pi, gaps = self.targets_of(b)
            ex = self.explored(b)
            proven_kids = sum(1 for c in root.kids if state_of(c.proof)) if self.solver else 0
            if ex:
                st = self.board_stats[b]
                st["explored_moves"] += 1
                st["visits_pruned"] += int((N - Np).sum())
                st["children_pruned"] += int(((N > 0) & (Np == 0)).sum())
                self.xfacts["pruned_at_proven_root"] += int((N - Np).sum() > 0 and proven_kids > 0)
            if self.solver and state_of(root.proof):
                self.xfacts["root_proven_at_boundary"].add(b)
            if not self.targets[b] and self.board_proven[b] > 0:
                self.xfacts["fast_with_proofs"] += 1
            self.plies_rec[b].append({"sq": board.squares(), "turn": int(board.turn), "ids": acts.astype(np.uint16), "pi": pi.astype(F32)})
            want = -1 if forced is None else int(forced[b])
            v64 = root_value64(Np if self.glue_wrong == "resign_on_pruned_counts" else N, Q)
            u = ua(self.seed, self.base + b, self.move_no[b], 0xffd)
            ev = g.record(int(board.turn), v64, self.targets[b], want >= 0, u, enabled=self.rule is not None)
            if self.rule is not None:
                if ev:
                    self.xfacts[ev] += 1
                self.xfacts["below_no_fire"] += int(ev is None and v64 < self.rule.threshold and self.rule.consecutive > 0)
            rec = {"pi": pi.astype(F32), "pi64": pi, "explored": ex, "acts": acts, "visits": N, "pruned": Np, "move": -1}
            self.last.append(rec)
            self.move_no[b] += 1
            self.plies[b] += 1
            self.used[b] = 0
            if ev == "resign":                            # no move is pushed; the board's tree is an empty root
                self.roots[b] = SNode(1.0, -1)
                self.over[b] = True
                events.append(ev)
                continue
            if want >= 0:
                ci = int(np.nonzero(acts == want)[0][0])
            else:
                ci = choose_move(pi, self.seed, self.base + b, self.move_no[b] - 1, self.sampler_eps, self.sampler_alpha, not ex)
            rec["move"] = int(acts[ci])
            self.roots[b] = root.kids[ci]
            if self.glue_wrong == "reroot_drops_proof":
                for node, _ in SolverModel.walk(self, b):
                    node.proof = 0
            if self.solver and any(state_of(node.proof) for node, _ in SolverModel.walk(self, b)):
                self.xfacts["proofs_after_reroot"].add(b)
            board.push_id(rec["move"])
            if board.is_game_over() or board.is_tie():
                o = board.outcome()
                g.end(-1 if (o is None or o.winner is None) else int(o.winner))
                self.over[b] = True
            events.append(ev)
        return events

    # -------------------------------------------------------------------------------------------------------- records and counters
    def records(self, game_no=0):
        """uint8 [P, 880]: the records ccz_harvest_records writes for the finished games (boards in index order, plies in order).
        ``game_no``: the header's count of games started on the slot (the engine's business: it is handed in)."""
        rows = []
        for b in range(self.B):
            g = self.games[b]
            if not g.over or not self.plies_rec[b]:
                continue
            T, flags = len(self.plies_rec[b]), g.flags()
            for t, p in enumerate(self.plies_rec[b]):
                r = np.zeros(REC_BYTES, np.uint8)
                k = len(p["ids"])
                r[:90] = p["sq"]
                if g.values[t] is not None:
                    r[92:96] = np.frombuffer(np.float32(g.values[t]).tobytes(), np.uint8)
                r[HDR:HDR + 4] = np.array([t, T], np.uint16).view(np.uint8)
                r[HDR + 4] = np.array([g.winner], np.int8).view(np.uint8)[0]
                r[HDR + 5], r[HDR + 6], r[HDR + 7] = p["turn"], k, flags[t]
                r[HDR + 8:HDR + 12] = np.array([(self.base + b) & 0xffffffff], np.uint32).view(np.uint8)
                r[HDR + 12:HDR + 16] = np.array([game_no], np.uint32).view(np.uint8)
                r[IDS:IDS + 2 * k] = p["ids"].view(np.uint8)
                r[PI:PI + 4 * k] = p["pi"].view(np.uint8)
                rows.append(r)
        return np.stack(rows) if rows else np.zeros((0, REC_BYTES), np.uint8)

    def resign_stats(self):
        return stats_of([g for g in self.games if g.over])


# ---------------------------------------------------------------------------------------------------------------- the GPU test's inputs
B = 16
SEED, BASE = 23, 4096
N_FULL, N_FAST, P_FULL = 96, 24, 0.75
MOVES = 3
SALT = sc.SALTS[0]
SALTS = (SALT,) * B                     # one salt: the evaluator is a function of the position alone, as an evaluation cache assumes
EXPLORE = dict(em.FULL)
RULE = Rule(-0.03, 2, 0, 0.5)
WIDE_NAME = "wide_late_mate"
OPENINGS = (0, 3, 5, 8, 11, 13, 6)       # boards of explore_model.inputs()
WIDE = len(sc.CASES) + len(OPENINGS) + 1
assert WIDE == B - 1


@functools.lru_cache(maxsize=None)
def inputs():
    """16 boards as (squares, turn) from the squares alone (no history, clock 0): the seven solver fixtures, seven of
    explore_model.inputs()'s opening positions, ``pawns`` and the wide fixture whose only mating move is a child of index >= 64."""
    from golden_cases import STARTS, WIDTHS
    out = [(sq.copy(), int(turn)) for _, sq, turn, *_ in sc.CASES]
    eb = em.inputs()[0]
    out += [(eb[j].squares(), int(eb[j].turn)) for j in OPENINGS]
    out.append((STARTS["pawns"].copy(), 1))
    out.append((STARTS[WIDE_NAME].copy(), WIDTHS[WIDE_NAME][0]))
    assert len(out) == B
    return out


def boards():
    return [OracleBoard.from_array(sq, turn) for sq, turn in inputs()]


def all_on(evaluator=None, wrong=None, **kw):
    cfg = dict(explore=EXPLORE, solver=True, resign=RULE, cap=(N_FULL, N_FAST, P_FULL), max_plies=MOVES)
    cfg.update(kw)
    return SelfPlayModel(boards(), SALTS, SEED, BASE, evaluator=evaluator, wrong=wrong, **cfg)


def run(m, moves=MOVES, per_step=None):
    """``moves`` moves of N_FULL lockstep steps each. Per move: budgets, the leaves of every step, root children / proofs / noise,
    events, what was recorded. ``per_step(move, step, leaves)``: called after every step."""
    out = []
    for mv in range(moves):
        live = [not o for o in m.over]
        budgets = m.begin_move()
        steps = []
        for i in range(N_FULL):
            steps.append(m.step())
            if per_step is not None:
                per_step(mv, i, steps[-1])
        rc = [m.root_children(b) for b in range(m.B)]
        rp = [m.root_proof(b) for b in range(m.B)]
        noise = [m.noise(b) if m.explored(b) else np.zeros(0, F32) for b in range(m.B)]
        targets = list(m.targets)
        sstats = m.solver_stats()
        events = m.finish_move()
        out.append({"live": live, "budgets": budgets, "targets": targets, "steps": steps, "roots": rc, "proofs": rp, "noise": noise,
                    "sstats": sstats, "events": events, "finish": m.last, "status": [g.status() for g in m.games], "over": list(m.over)})
    return out


@functools.lru_cache(maxsize=None)
def dense_run(wrong=None):
    """The model on the ``hash`` evaluator's priors as they are (the dense launch forms), with what the CPU test asserts."""
    m = all_on(wrong=wrong)
    moves = run(m)
    close(m)
    return m, moves


def close(m):
    """After the last move: the solver counters as the moves left them, then every game still running is adjudicated at the ply cap."""
    m.closing_sstats = m.solver_stats()
    m.finish_move()
