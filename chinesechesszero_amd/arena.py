"""Checkpoint arena: many different, colour-balanced games between two networks in one lockstep batch.

Reference ``Game.start_play`` (game.py:77-130) with two non-self-play ``MCTS_AI`` players (mcts.py:225-229): the player to move
at the root searches with ITS OWN network -- which evaluates every leaf of that search, whoever is to move at the leaf --, plays
the arg-max-visit move (temperature 1e-3, no Dirichlet noise) and discards the tree. The reference's gating step
(``policy_evaluate``, train.py:313-319) is a stub returning 0.6; :func:`policy_evaluate` is what it was meant to return.

Boards come in pairs: boards 2i and 2i+1 start from the same randomised opening i (:func:`make_openings`) with the colours
swapped -- network A plays red on even boards and black on odd ones. Every simulation runs both networks one after the other
on the engine's stream, each on the planned rows of the boards whose search it owns (``ccz_eval_plan_routed``): one evaluation
cache serves both, under a salt per network, so an evaluation of one is never served to the other. Finished boards produce no
rows. (``match.BatchedMatch`` plays every board from the opening position with one evaluator per ply: one game, B times.)
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time

import numpy as np

from .boundary import WeightsWatch, describe
from .parameters import C_PUCT
from .options import (SearchOptions, add_fused_narrow_args, fused_narrow_from_args, add_lcb_args, add_leaf_history_args, add_resign_args, lcb_from_args, lcb_moves, leaf_history_from_args,
                      add_mate_search_args, mate_moves, mate_search_from_args,
                      proven_moves, resign_from_args, search_move)
from .searchcfg import add_search_args, search_from_args
from .stopcfg import StopPoll, add_early_stop_args, early_stop_from_args

_RESIGNED = 2   # _lib.RESIGN_RESIGNED (this module imports the engine lazily: its statistics run without a GPU)
PROMOTE_THRESHOLD = 0.55   # AlphaGo Zero's gate, kept by the AlphaZero_Gomoku lineage the reference cites


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return x ^ (x >> 31)


def cache_salts(version_a, version_b) -> tuple[int, int]:
    """The two networks' cache salts: a function of (network slot, weights version), never equal to each other."""
    s = [_splitmix64((int(v) & (2**62 - 1)) << 1 | k) or 1 for k, v in enumerate((version_a, version_b))]
    if s[0] == s[1]:
        s[1] ^= 1
    return s[0], s[1]


# ---------------------------------------------------------------------- openings
def _check_opening_args(n, plies, seed):
    for name, v in (("n", n), ("plies", plies), ("seed", seed)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"make_openings: {name} must be an integer, got {type(v).__name__}")
    if n < 1:
        raise ValueError(f"make_openings: n must be >= 1 (got {n})")
    if plies < 0:
        raise ValueError(f"make_openings: plies must be >= 0 (got {plies})")
    if plies == 0 and n > 1:
        raise ValueError("make_openings: with plies = 0 there is only one opening (the start position)")


def make_openings(n: int, plies: int, seed: int = 0, device: int = 0):
    """``n`` distinct positions, each ``plies`` uniformly random legal moves from the start position, drawn with a host RNG
    seeded by ``seed`` and played with the device rules (:func:`engine.legal_moves` / :func:`engine.apply_moves`). A line that
    reaches a finished position (no legal move, bare material) is dropped, and so is a position met before (same squares and
    side to move). Deterministic for a given (n, plies, seed). Returns (squares uint8 [n,90], turn uint8 [n], halfmove int32 [n])."""
    _check_opening_args(n, plies, seed)
    from . import tools
    from .engine import legal_moves, apply_moves
    from .game import start_squares
    rng = np.random.default_rng(int(seed))
    mover_from = np.array([(ord(u[0]) - ord("a")) + 9 * int(u[1]) for _, u in sorted(tools.move_id2move_action.items())], np.int64)
    seen, out_sq, out_turn, out_half = set(), [], [], []
    batch = max(64, 2 * int(n))
    for _ in range(64):
        sq = np.repeat(start_squares()[None, :], batch, axis=0)
        turn = np.ones(batch, np.uint8)
        half = np.zeros(batch, np.int32)
        alive = np.ones(batch, bool)
        for _p in range(plies):
            mask, cnt, _flags = legal_moves(sq, turn, device=device)
            alive &= cnt > 0
            ids = np.zeros(batch, np.int32)
            for i in range(batch):
                if alive[i]:
                    legal = np.flatnonzero(mask[i])
                    ids[i] = legal[rng.integers(len(legal))]
            pawn = np.zeros(batch, bool)
            if tools.PAWN_MOVE_RESETS_CLOCK:   # (the rule preset's clock: pawn moves restart it too)
                pawn = (sq[np.arange(batch), mover_from[ids]] & 7) == 1
            # (a finished line is frozen in place with a legal id of no consequence: it is dropped below)
            nsq, nturn, cap = apply_moves(sq, turn, np.where(alive, ids, 0), device=device)
            sq = np.where(alive[:, None], nsq, sq)
            turn = np.where(alive, nturn, turn).astype(np.uint8)
            half = np.where(alive, np.where((cap != 0) | pawn, 0, half + 1), half).astype(np.int32)
        _mask, cnt, flags = legal_moves(sq, turn, half, device=device)
        alive &= (cnt > 0) & ((flags & 6) == 0)          # the side to move can move; no bare material, no sixty-move draw
        for i in np.flatnonzero(alive):
            key = (bytes(sq[i]), int(turn[i]))
            if key in seen:
                continue
            seen.add(key)
            out_sq.append(sq[i].copy())
            out_turn.append(int(turn[i]))
            out_half.append(int(half[i]))
            if len(out_sq) == n:
                return np.stack(out_sq), np.array(out_turn, np.uint8), np.array(out_half, np.int32)
    raise ValueError(f"make_openings: found only {len(out_sq)} distinct unfinished positions after {plies} plies (asked for {n})")


# ---------------------------------------------------------------------- statistics
def pair_layout(n_pairs: int):
    """(opening index [2P], A's colour [2P], 1 RED / 0 BLACK; red_net [2P], 0 = A plays red): boards 2i, 2i+1 play opening i,
    A is red on the even board and black on the odd one."""
    b = np.arange(2 * int(n_pairs))
    a_colour = (1 - (b & 1)).astype(np.uint8)
    red_net = (b & 1).astype(np.uint8)
    return b // 2, a_colour, red_net


def elo_of_score(s: float, games: int) -> float:
    """Logistic Elo difference of a score. A score of 0 or 1 has no finite Elo: the score is clamped to half a game from either
    end, ``[0.5 / games, 1 - 0.5 / games]``, so the result stays finite (and grows with the number of games)."""
    lo = 0.5 / max(1, int(games))
    s = min(max(float(s), lo), 1.0 - lo)
    return -400.0 * math.log10(1.0 / s - 1.0)


def pair_stats(points_a) -> dict:
    """Score and Elo of A from the per-pair points (0, .5, 1, 1.5 or 2 per pair: the pentanomial). The two games of a pair
    share an opening, so the PAIR is the independent sample: score = mean(points) / 2, its standard error
    sqrt(var(points / 2) / pairs) (population variance of the per-pair scores), 95 % interval = score +- 1.96 se, and the Elo
    interval is the Elo of the interval's ends (clamped as :func:`elo_of_score`)."""
    x = np.asarray(points_a, np.float64)
    P = int(x.size)
    if P == 0:
        raise ValueError("pair_stats: no pairs")
    if np.any((x * 2) % 1 != 0) or np.any(x < 0) or np.any(x > 2):
        raise ValueError("pair_stats: points per pair must be 0, 0.5, 1, 1.5 or 2")
    penta = [int(np.sum(x == v)) for v in (0.0, 0.5, 1.0, 1.5, 2.0)]
    y = x / 2.0
    s = float(y.mean())
    se = float(math.sqrt(float(((y - s) ** 2).mean()) / P))
    lo, hi = max(0.0, s - 1.96 * se), min(1.0, s + 1.96 * se)
    G = 2 * P
    return {"pairs": P, "pentanomial": penta, "score": s, "score_se": se, "score_ci95": [lo, hi],
            "elo": elo_of_score(s, G), "elo_ci95": [elo_of_score(lo, G), elo_of_score(hi, G)]}


def promote(result, threshold: float = PROMOTE_THRESHOLD) -> bool:
    """Gating rule: the candidate (network A) replaces the best network iff its score -- wins + half the draws (truncated games
    count as the draws they are adjudicated as), over all games -- is strictly above ``threshold``. ``result`` is
    :meth:`Arena.play`'s dict or a score."""
    s = float(result["score"] if isinstance(result, dict) else result)
    if not (0.0 <= threshold <= 1.0):
        raise ValueError("promote: threshold must be in [0, 1]")
    return s > float(threshold)


# ---------------------------------------------------------------------- the arena
def _as_evaluator(net, name):
    ev = describe(net)
    if not callable(ev.fn) or not (ev.accepts_plan and ev.returns_logits):
        raise TypeError(f"Arena: network {name} must be a plan-capable logits evaluator (a PolicyValueNet, or a callable marked "
                        "accepts_plan and returns_logits: ev(leaf, plan=(rows, n)) -> compact (logits, value))")
    return ev


class Arena:
    """``n_pairs`` pairs of games between ``net_a`` (A) and ``net_b`` (B). Engine: eps 0, temperature 1e-3, tree discarded after
    every move, evaluation cache of 2^``eval_cache_log2`` positions shared by both networks (salted per network).
    ``n_playout_b``: playout odds -- A searches ``n_playout`` simulations per move, B ``n_playout_b`` (per-board simulation budgets,
    ``engine.set_budgets``: the lockstep loop runs max(nA, nB) steps and a board that has used its budget costs no evaluator row);
    None: both search ``n_playout``. ``resign``: a threshold in [-1, 0] or a dict with ``threshold`` and optionally ``consecutive`` /
    ``min_ply`` (``engine.set_resign``): the side to move resigns when its root value stayed below the threshold -- a resigned game
    is a win for the other side like any other, counted in ``result()["resigned"]``; no game is played on (``p_playon`` = 0).
    None (default): games end by the rules or the ply cap only. ``solver`` / ``search`` / ``early_stop``: the engine options
    (``options.OPTIONS``; None / False: off), for both sides alike: with the solver the proven move is played where the root is decided
    (``options.proven_moves``), with the early stop the move's loop ends when no board would select any more (``options.search_move``).
    ``lcb``: the LCB move (``options.MOVE_OPTIONS``: True, a multiple z of the standard error, or a dict) instead of the most visited one,
    for the side(s) ``lcb_side`` names -- "both", "a" or "b": a board's move is the LCB move only when the owner of the side to move has
    the option, so ``Arena(X, X, lcb=True, lcb_side="a")`` measures it. A proven move wins over it. ``result()["lcb"]`` then holds, per
    side, the moves played by the rule and how many of them were not the most visited move."""

    def __init__(self, net_a, net_b, n_pairs: int, n_playout: int = 400, opening_plies: int = 6, seed: int = 0,
                 max_plies: int = 0, c_puct: float = C_PUCT, eval_cache_log2: int = 22, device: int = 0,
                 cache_verify: bool = False, n_playout_b: int | None = None, resign=None, solver: bool = False, search=None, early_stop=None,
                 leaf_history=None, lcb=None, lcb_side: str = "both", mate_search=None):
        from .boundary import need_history
        from .engine import SelfPlayEngine
        self.nets = (net_a, net_b)
        described = (_as_evaluator(net_a, "A"), _as_evaluator(net_b, "B"))
        self.ev = (described[0].fn, described[1].fn)
        # the two weights versions as the cache salts take them (an evaluator that exposes none counts as version 0)
        self._versions = lambda: tuple(int(d.version() or 0) for d in described)
        self._weights = WeightsWatch()       # nothing seen: the first search sets the routing
        if int(n_pairs) < 1:
            raise ValueError("Arena: n_pairs must be >= 1")
        if int(eval_cache_log2) < 1:
            raise ValueError("Arena: the two networks are routed through the evaluation cache: eval_cache_log2 must be >= 1")
        self.P = int(n_pairs)
        self.B = 2 * self.P
        self.n_playout = int(n_playout)
        self.n_playout_b = None if n_playout_b is None else int(n_playout_b)
        if self.n_playout < 1 or (self.n_playout_b is not None and self.n_playout_b < 1):
            raise ValueError("Arena: n_playout and n_playout_b must be >= 1")
        self.n_steps = self.n_playout if self.n_playout_b is None else max(self.n_playout, self.n_playout_b)   # lockstep steps per move
        self.options = o = SearchOptions(self.n_steps, resign=resign, solver=solver, search=search, early_stop=early_stop, lcb=lcb,
                                         leaf_history=leaf_history, mate_search=mate_search)
        self.mate_search = o.mate_search     # both sides look for a forced mate by checks before the move (options.mate_moves)
        self.resign,self.solver, self.search_cfg, self.early_stop, self.lcb, self.leaf_history = o.keywords().values()
        if lcb_side not in ("both", "a", "b"):
            raise ValueError(f"Arena: lcb_side must be 'both', 'a' or 'b' (got {lcb_side!r})")
        if self.lcb is None and lcb_side != "both":
            raise ValueError("Arena: lcb_side without lcb: the LCB move is off")
        self.lcb_side = lcb_side
        self.lcb_sides = {s: {"moves": 0, "differed": 0} for s in ("a", "b") if self.lcb is not None and lcb_side in ("both", s)}
        if self.resign is not None:          # (the dict ``o.apply`` hands to the engine)
            if self.resign.get("p_playon", 0.0) != 0.0:
                raise ValueError("Arena: a match plays no game on after the resignation rule fired (p_playon is fixed at 0)")
            self.resign["p_playon"] = 0.0
        self.temp = 1e-3
        self.engine = e = SelfPlayEngine(self.B, n_playout=self.n_steps, c_puct=c_puct, eps=0.0, alpha=0.2, temp=self.temp,
                                         seed=seed, device=device, max_plies=max_plies, mirror=False,
                                         eval_cache_log2=eval_cache_log2, cache_verify=cache_verify)
        self.max_plies = e.max_plies
        self.proven_moves = 0                # moves played from a proof
        o.apply(e)
        for name, net in zip("AB", self.nets):   # leaf history: both networks must read the 119 planes the engine then writes
            need_history(e, net, f"Arena: evaluator {name}: ")
        self._poll = StopPoll(e, self.early_stop)
        self.opening_of, self.a_colour, self.red_net = pair_layout(self.P)
        self.openings = make_openings(self.P, int(opening_plies), seed=seed, device=device)
        sq, turn, half = self.openings
        of = np.asarray(self.opening_of)
        status = e.set_positions(np.asarray(sq)[of], np.asarray(turn)[of], np.asarray(half)[of])   # one launch (no moves: as set_position)
        if status.any():
            raise ValueError(f"Arena: opening positions refused by the engine (status {status.tolist()})")
        self._turn = np.asarray(turn)[of].astype(np.uint8)      # side to move on every board (kept from the per-move status read)
        self._temps = np.full(self.B, self.temp, np.float64)
        self.moves = []                      # host int32 [B] per lockstep move (-1: no move on that board)
        self.truncated = np.zeros(self.B, bool)
        self.steps = 0
        import torch
        self._rows = torch.zeros((2,), dtype=torch.int64, device=e.device)   # evaluator rows per network, summed on the device

    def _sync_routing(self):
        """(Re)set the routing when a network's weights version changed: that network gets a new salt, and its old entries can
        never be served again (the other network's stay valid)."""
        if self._weights.moved(self._versions()):
            self.engine.set_routing(self.red_net, cache_salts(*self._weights.seen))

    def search(self, on_step=None):
        """``n_playout`` routed simulations on every unfinished board (fresh trees). ``on_step(arena, plan0, plan1)`` runs after
        each plan (tests)."""
        e, (ev0, ev1) = self.engine, self.ev
        self._sync_routing()
        if self.n_playout_b is not None:
            e.set_budgets(self.move_budgets())
        def step(leaf, last):
            p0, p1 = e.eval_plan_routed()
            self._rows += e.n_miss2
            if on_step is not None:
                on_step(self, p0, p1)
            lg0, v0 = ev0(leaf, plan=p0)
            lg1, v1 = ev1(leaf, plan=p1)
            leaf = e.expand_backup_routed(lg0, v0, lg1, v1) if last else e.step_routed(lg0, v0, lg1, v1)
            self.steps += 1
            return leaf
        search_move(e, self.n_steps, step, self._poll)

    def move_budgets(self) -> np.ndarray:
        """int32 [B]: the simulations every board searches in the move at hand -- ``n_playout`` where A is to move, ``n_playout_b``
        (``n_playout`` without odds) where B is."""
        nb = self.n_playout if self.n_playout_b is None else self.n_playout_b
        return np.where(self._turn == self.a_colour, self.n_playout, nb).astype(np.int32)

    def play_move(self, on_step=None, before_move=None):
        """One lockstep move of every unfinished board: search, move at temperature 1e-3, tree discarded. Returns the moves
        (host int32 [B], -1 where no move was played). ``before_move(arena)`` runs between the search and the move (tests)."""
        self.search(on_step)
        if before_move is not None:
            before_move(self)
        return self.finish_move()

    def finish_move(self):
        """The move after a :meth:`search`: arg-max visits up to ties (temperature 1e-3), the tree is discarded."""
        e = self.engine
        over = e.game_status()["over"]
        forced, proven = proven_moves(e, self.solver, over)
        self.proven_moves += proven
        if self.mate_search is not None:   # (off: no call is made) the mating move wins over the LCB move and the most visited one
            forced, _ = mate_moves(e, self.mate_search, forced, over, counts=self.options.mate_counts)
        a_moves = self._turn == self.a_colour
        if self.lcb is not None:   # (off: no call is made) one call; the counts are split by the owner of the side to move
            allow = None if self.lcb_side == "both" else (a_moves if self.lcb_side == "a" else ~a_moves)
            forced, _, fill, off = lcb_moves(e, self.lcb, forced, over, allow=allow, counts=self.options.lcb_counts, detail=True)
            for side, c in self.lcb_sides.items():
                mine = a_moves if side == "a" else ~a_moves
                c["moves"] += int((fill & mine).sum())
                c["differed"] += int((off & mine).sum())
        moves = e.finish_move(forced_moves=forced, temps=self._temps, keep_tree=False).cpu().numpy().copy()
        # a game adjudicated at max_plies ends INSTEAD of a move (finish_move plays none on that board); so does a resigned one
        st = e.game_status()
        ended = (over == 0) & (st["over"] == 1) & (moves < 0)
        if self.resign is not None and ended.any():
            ended &= (e.resign_status()["state"] & _RESIGNED) == 0
        self.truncated |= ended
        self._turn = st["turn"].astype(np.uint8)
        self.moves.append(moves)
        return moves

    def game_moves(self, b: int) -> list[int]:
        """The moves board ``b`` played from its opening."""
        return [int(m[b]) for m in self.moves if m[b] >= 0]

    def play(self, before_move=None, on_step=None) -> dict:
        """Play every board to the end; returns :meth:`result`."""
        import torch
        e = self.engine
        t0 = time.perf_counter()
        while not e.game_status()["over"].all():
            self.play_move(on_step, before_move)
        torch.cuda.synchronize(e.device)
        wall = time.perf_counter() - t0
        e.check_healthy()
        return self.result(wall)

    def result(self, wall: float | None = None) -> dict:
        st = self.engine.game_status()
        w, plies = st["winner"].astype(np.int64), st["plies"]
        a_pts = np.where(w == -1, 0.5, np.where(w == self.a_colour, 1.0, 0.0))
        pair_pts = a_pts[0::2] + a_pts[1::2]
        rows = self._rows.cpu().numpy()
        steps = max(1, self.steps)
        out = {"pairs": self.P, "games": self.B, "n_playout": self.n_playout,
               "n_playout_b": self.n_playout if self.n_playout_b is None else self.n_playout_b,
               "wins": int(np.sum(w == self.a_colour)), "draws": int(np.sum(w == -1)), "losses": int(np.sum((w != -1) & (w != self.a_colour))),
               "truncated": int(self.truncated.sum()), "unfinished": int((st["over"] == 0).sum())}
        if self.resign is not None:
            out["resigned"] = int(((self.engine.resign_status()["state"] & _RESIGNED) != 0).sum())
        out.update(pair_stats(pair_pts))
        out.update({"plies_mean": float(plies.mean()), "plies_min": int(plies.min()), "plies_max": int(plies.max()),
                    "steps": self.steps, "rows_per_step": [float(rows[0]) / steps, float(rows[1]) / steps]})
        if wall is not None:
            out["wall_s"] = wall
            out["games_per_s"] = self.B / wall if wall > 0 else float("nan")
        out.update(self.options.report(self.engine))
        if self.solver:
            out["solver"]["proven_moves"] = self.proven_moves
        if self.lcb is not None:
            out["lcb"] = dict(self.lcb, side=self.lcb_side, **{s: dict(c) for s, c in self.lcb_sides.items()})
        s = self.engine.stats()
        out["cache"] = {k: s[k] for k in ("cache_probes", "cache_hits", "cache_shared_rows", "cache_stores",
                                           "cache_verified", "cache_verify_mismatches")}
        return out


def policy_evaluate(current, best, **kw) -> float:
    """The win ratio of ``current`` against ``best`` -- wins + half the draws, over all games -- from a colour-balanced
    :class:`Arena` (``kw``: its arguments, e.g. ``n_pairs=256``): what the reference's stub (train.py:313-319) stands in for."""
    kw.setdefault("n_pairs", 64)
    return float(Arena(current, best, **kw).play()["score"])


# ---------------------------------------------------------------------- CLI
def _load(spec: str, channels: int, blocks: int, device: int, fused_narrow: bool = False):
    import torch
    from .net import PolicyValueNet
    dev = f"cuda:{device}"
    if spec.startswith("random:"):
        torch.manual_seed(int(spec.split(":", 1)[1]))
        return PolicyValueNet(device=dev, num_channels=channels, resblocks_num=blocks, fused_narrow=fused_narrow)
    return PolicyValueNet(model=spec, device=dev, num_channels=channels, resblocks_num=blocks, fused_narrow=fused_narrow)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m chinesechesszero_amd.arena",
                                 description="Colour-balanced arena between two checkpoints; prints one JSON line (A's point of view).")
    ap.add_argument("--a", required=True, help="candidate weights (state_dict file), or random:<seed> for a random-init net")
    ap.add_argument("--b", required=True, help="opponent weights (state_dict file), or random:<seed>")
    ap.add_argument("--pairs", type=int, default=512, help="pairs of games (one opening, both colours)")
    ap.add_argument("--playout", type=int, default=400, help="simulations per move")
    ap.add_argument("--playout-b", type=int, default=None, help="playout odds: simulations per move of B (default: as A)")
    ap.add_argument("--opening-plies", type=int, default=6, help="random legal plies of every opening")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-plies", type=int, default=0, help="ply cap (0 = the engine's 2048); a capped game is a draw, counted as truncated")
    ap.add_argument("--eval-cache-log2", type=int, default=22, help="evaluation cache of 2^n positions, shared by both nets")
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--threshold", type=float, default=PROMOTE_THRESHOLD, help="promotion threshold of the score")
    ap.add_argument("--device", type=int, default=0)
    add_resign_args(ap, playon=False)
    ap.add_argument("--solver", action="store_true", help="MCTS-solver on both sides: decided positions are proven in the tree and the proven move is played")
    add_search_args(ap)
    add_early_stop_args(ap)
    add_leaf_history_args(ap)
    add_lcb_args(ap)
    add_fused_narrow_args(ap)
    add_mate_search_args(ap)
    ap.add_argument("--lcb-side", choices=("both", "a", "b"), default=None, help="... which side plays the LCB move (default both); "
                    "--a X --b X --lcb --lcb-side a measures the option")
    a = ap.parse_args(argv)
    search = search_from_args(ap, a)
    early_stop = early_stop_from_args(ap, a)
    resign = resign_from_args(ap, a)
    mate_search = mate_search_from_args(ap, a)
    narrow =fused_narrow_from_args(ap, a)
    na = _load(a.a, a.channels, a.blocks, a.device, narrow)
    nb = _load(a.b, a.channels, a.blocks, a.device, narrow)
    lcb = lcb_from_args(ap, a)
    if lcb is None and a.lcb_side is not None:
        ap.error("--lcb-side without --lcb: the LCB move is off")
    leaf_history = leaf_history_from_args(ap, a)
    if leaf_history is not None:
        na.set_leaf_history(True)
        nb.set_leaf_history(True)
    arena = Arena(na, nb, a.pairs, n_playout=a.playout, opening_plies=a.opening_plies, seed=a.seed, max_plies=a.max_plies,
                  eval_cache_log2=a.eval_cache_log2, device=a.device, n_playout_b=a.playout_b, resign=resign, solver=a.solver, search=search,
                  early_stop=early_stop, leaf_history=leaf_history, lcb=lcb, lcb_side=a.lcb_side or "both", mate_search=mate_search)
    r = arena.play()
    r.update({"a": a.a, "b": a.b, "opening_plies": a.opening_plies, "seed": a.seed, "net": f"{a.blocks}x{a.channels}",
              "promote": promote(r, a.threshold), "threshold": a.threshold})
    print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
