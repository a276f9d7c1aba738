"""Batched position analysis: "what does the search think of these N positions?" on the lockstep engine.

``BatchedAnalysis`` loads ``n_boards`` positions at a time -- each with the moves that led to it, so that repetitions and the
sixty-move clock count as they would in the game -- with ONE ``set_positions`` launch, searches them in lockstep
(``BatchedSelfPlay.search``: no move is played) and reads the principal variations of every tree with ONE
``principal_variations`` launch. The one-game front ends (``MCTS_AI``, the UCI loop) answer the same question one position at a
time; this is the path for a file of positions: a test suite, an opening book, games to label.

Command line::

    python -m chinesechesszero_amd.analyse FILE [--playout N] [--boards B] [--multipv K] [--max-len L] [--weights PATH] [--out FILE.jsonl]

FILE holds one UCI position per line (``startpos [moves ...]`` or ``fen <fen> [moves ...]``; blank lines and ``#`` comments are
skipped); one JSON object per position goes to ``--out`` (stdout without it), a one-line summary to stderr.
"""
from __future__ import annotations

import json
import math
import sys
import time

import numpy as np

from ._lib import CczError
from .boundary import describe
from .game import Board
from .options import (SearchOptions, add_mate_search_args, mate_search_from_args, add_fused_narrow_args, add_lcb_args, add_leaf_history_args, fused_narrow_from_args, lcb_from_args,
                      leaf_history_from_args)
from .searchcfg import add_search_args, search_from_args
from .stopcfg import add_early_stop_args, early_stop_from_args


def cp_of(q: float, visits: int) -> int:
    """Centipawn DISPLAY value of a stored Q (side to move's view, -1 .. 1): the project's logistic convention,
    ``round(arena.elo_of_score((1 + Q) / 2, games=max(1, N)))`` -- the score is clamped half a "game" (visit) from either end, so
    a forced win shows as a large finite number that grows with the visits. A mapping for GUIs, nothing more: Q is not calibrated
    in pawns."""
    from .arena import elo_of_score
    return int(round(elo_of_score((1.0 + float(q)) / 2.0, games=max(1, int(visits)))))


def parse_positions(lines) -> list[tuple[int, Board]]:
    """``[(line number, Board)]`` of an iterable of text lines, one UCI position each (the arguments of ``position``); blank lines
    and ``#`` comments are skipped. Moves are NOT checked here (the device does that where they are played); a line that cannot be
    read at all raises ``ValueError`` naming its line number."""
    from .uci import parse_position
    out = []
    for no, raw in enumerate(lines, 1):
        text = raw.split("#", 1)[0].strip()
        if not text:
            continue
        tok = text.split()
        if tok[0] == "position":
            tok = tok[1:]
        try:
            out.append((no, parse_position(tok, validate=False)))
        except (ValueError, KeyError, IndexError) as e:
            raise ValueError(f"line {no}: {e} ({text!r})") from None
    return out


def make_record(status: str, root_visits: int = 0, lines=(), solver=None, lcb=None, mate=None) -> dict:
    """One result record: ``status`` ("ok", "illegal move i", "invalid position", "history too long", "game over: ..."),
    ``bestmove`` (the first move of line 0, or None), ``root_visits``, ``lines`` = [{moves (uci), visits, q, prior}].
    ``solver`` (an analysis with the MCTS-solver; None without): ``{"proven": uci or None, "mates": {uci: N}}`` -- the record and
    every line gain ``"mate"``: N in moves (``engine.mate_score``; negative: the side to move is mated) or None, and ``bestmove``
    is the proven move where the root is decided. ``lcb`` (an analysis with the LCB move; None without): ``{"move": uci or None,
    "stats": {uci: (stdev, lcb)}}`` -- every line gains ``"stdev"`` (the sample standard deviation of the values backed up through its
    first move; None below two visits) and ``"lcb"`` (its lower confidence bound; None where it has none), and ``bestmove`` is the LCB
    move unless the root is proven. The lines stay ranked by visits.
    ``mate`` (an analysis with the mate search; None without): ``{"move": uci or None, "mate": N or None}`` -- the record gains ``"mate"``
    (with or without the solver), and where a mate by checks was found ``bestmove`` is its first move and ``"mate"`` its length in moves,
    unless the solver has proven a mate of at most that length."""
    keep = [dict(moves=list(l["moves"]), visits=[int(v) for v in l["visits"]], q=float(l["q"]), prior=float(l["prior"])) for l in lines]
    rec = {"status": status, "bestmove": keep[0]["moves"][0] if keep and keep[0]["moves"] else None,
           "root_visits": int(root_visits), "lines": keep}
    if lcb is not None:
        for l in keep:
            l["stdev"], l["lcb"] = lcb["stats"].get(l["moves"][0], (None, None)) if l["moves"] else (None, None)
        if lcb.get("move") is not None and rec["bestmove"] is not None:
            rec["bestmove"] = lcb["move"]
    if solver is not None:
        for l in keep:
            l["mate"] = solver["mates"].get(l["moves"][0]) if l["moves"] else None
        if solver.get("proven") is not None:
            rec["bestmove"] = solver["proven"]
        rec["mate"] = solver["mates"].get(rec["bestmove"]) if rec["bestmove"] is not None else None
    if mate is not None:
        # a forced mate by checks: it is the best move and the record's "mate", unless the tree has proven a mate that is no longer
        quicker = solver is not None and rec.get("mate") is not None and 0 < rec["mate"] <= (mate.get("mate") or 0)
        rec.setdefault("mate", None)
        if mate.get("move") is not None and not quicker:
            rec["bestmove"], rec["mate"] = mate["move"], mate["mate"]
    return rec


def _winner_text(winner) -> str:
    return "game over: draw" if winner is None or winner < 0 else f"game over: {'red' if winner else 'black'} wins"


class BatchedAnalysis:
    """``evaluator``: what ``BatchedSelfPlay`` takes (``leaf fp16 [B,17,7,10,9] -> (prob | logits, value)``), or an object with
    ``evaluate_leaves_logits`` (a ``PolicyValueNet``). With a plan-capable evaluator and ``eval_cache_log2 > 0`` (the default for
    192 boards and more, as in self-play) the search runs on the planned boundary with the evaluation cache; the cache is kept
    across chunks and cleared only when the evaluator's weights version changes."""

    def __init__(self, evaluator, n_boards: int, n_playout: int = 400, multipv: int = 1, max_len: int = 32, solver: bool = False, search=None,
                 width: int = 1, early_stop=None, leaf_history=None, lcb=None, mate_search=None, **engine_kw):
        """``width`` > 1: every position gathers up to ``width`` leaves of its tree per step, kept apart by virtual loss
        (``wide.WideSearch``: an engine of ``n_boards * width`` slots) -- for a handful of positions, where the sequential search
        runs at the evaluator's latency; another tree than the sequential one; excludes ``solver`` and ``search``.
        ``solver`` / ``search`` / ``early_stop``: the engine options (``options.OPTIONS``; None / False: off). With the early stop a position
        stops being searched when its best move can no longer change, and a chunk's loop ends when no board would select any more.
        ``lcb``: the LCB move (``options.MOVE_OPTIONS``): ``bestmove`` is it, every line gains ``stdev`` and ``lcb``; not with ``width`` > 1."""
        from .selfplay import BatchedSelfPlay
        desc = describe(evaluator)
        ev = desc.fn
        if not callable(ev):
            raise TypeError("BatchedAnalysis: the evaluator must be callable or have evaluate_leaves_logits")
        if not 1 <= int(multipv) <= 128 or int(max_len) < 1 or int(n_playout) < 1:
            raise ValueError("BatchedAnalysis: multipv must be 1..128, max_len and n_playout >= 1")
        # ``mate_search``: plies or the dict of ``options.make_mate_search``: every position is also searched for a forced mate by checks
        # (``ccz_mate_search``, no evaluator rows); records gain "mate", and bestmove is the mating move where one is found
        self.mate_opts = SearchOptions(n_playout, width=width, solver=solver, search=search, early_stop=early_stop, leaf_history=leaf_history,
                                       lcb=lcb, mate_search=mate_search)   # (ValueError: width > 1 excludes the others)
        self.mate_search = self.mate_opts.mate_search
        if "eval_cache_log2" not in engine_kw:
            engine_kw["eval_cache_log2"] = 22 if (int(n_boards) >= 192 and desc.accepts_plan) else 0
        engine_kw.setdefault("mirror", False)
        self.width = int(width)
        self.wide = None
        self.B, self.n_playout, self.multipv, self.max_len = int(n_boards), int(n_playout), int(multipv), int(max_len)
        self.positions = self.steps = self.sims = 0
        self.seconds = 0.0
        self._rows = None   # evaluator rows, summed on the device (planned boundary: the plan's count per step)
        if self.width != 1:
            from .wide import WideSearch
            if engine_kw["eval_cache_log2"] == 0 and desc.accepts_plan:
                engine_kw["eval_cache_log2"] = 16   # slots of one tree reach one position often: they share an evaluator row
            engine_kw.setdefault("eps", 0.0)
            self.wide = WideSearch(ev, int(n_boards), self.width, n_playout=int(n_playout), **engine_kw)   # ValueError: width not in 2..64
            self.sp = None
            self.engine = self.wide.engine
            self.solver, self.lcb = False, None
            return
        self.sp = BatchedSelfPlay(ev, int(n_boards), n_playout=int(n_playout), eps=0.0, search=search, early_stop=early_stop, leaf_history=leaf_history, **engine_kw)   # no GPU: CczError
        self.engine = self.sp.engine
        opts = SearchOptions(solver=solver, lcb=lcb)     # (search and early stop: the self-play front end's own, above; it samples from pi and takes no lcb)
        self.lcb = opts.lcb
        self.solver = opts.solver               # the MCTS-solver: records gain "mate", bestmove follows the proof (make_record)
        opts.apply(self.engine)

    def _count_rows(self, stage, _sim):
        if stage == "eval1":
            self.steps += 1
            if self.sp.planned:
                self._rows += self.engine.n_miss[0]

    def analyse(self, positions) -> list[dict]:
        """One record (:func:`make_record`) per position, in input order. ``positions``: ``game.Board`` objects (their start
        position and move stack are loaded) or UCI ``position`` argument strings."""
        import torch
        from .tools import move_id2move_action as uci_of
        from .uci import parse_position
        boards = [p if isinstance(p, Board) else parse_position(str(p).split(), validate=False) for p in positions]
        e, sp, B = self.engine, self.sp, self.B
        S = e.B             # slots of the engine: B, or B * width (only the first B carry positions)
        if self._rows is None:
            self._rows = torch.zeros((), dtype=torch.int64, device=e.device)
        out = []
        t0 = time.perf_counter()
        sims0 = e.stats()["sims"]
        for c0 in range(0, len(boards), B):
            chunk = boards[c0:c0 + B]
            n = len(chunk)
            sq = np.zeros((S, 90), np.uint8)
            turn = np.ones(S, np.uint8)
            half = np.zeros(S, np.int32)
            moves = [[] for _ in range(S)]
            for j, bd in enumerate(chunk):
                sq[j], turn[j], half[j] = bd._start[0], 1 if bd._start[1] else 0, bd._start[2]
                moves[j] = [m.id for m in bd.move_stack]
            status = e.set_positions(sq, turn, half, moves, park=np.arange(S) >= n)   # the tail of the last chunk is parked
            if sp is not None:
                sp._sim, sp._leaf, sp._ticker.acc = 0, None, 0      # fresh roots: whatever leaf was pending belongs to the old ones
            st = e.game_status()
            ms = None
            if self.mate_search is not None:     # (off: no call is made) the roots as loaded; the search below runs all the same
                from .options import mate_moves
                ms = mate_moves(e, self.mate_search, None, st["over"], counts=self.mate_opts.mate_counts, detail=True)[2]
            if self.wide is not None:
                self.wide.boundary()
                if not st["over"][:n].all():
                    self.steps += self.wide.search()
            elif not st["over"][:n].all():
                sp.search(hooks=self._count_rows, poll=True)
            pv = e.principal_variations(self.multipv, self.max_len)
            e.check_healthy()
            rp, rc = (e.root_proof(), e.root_children()) if self.solver else (None, None)
            lb = None
            if self.lcb is not None:
                got = e.lcb_moves(self.lcb["z"], self.lcb["min_visit_ratio"], self.lcb["min_visits"], with_bounds=True)
                lb = {"moves": got["moves"].cpu().numpy(), "lcb": got["lcb"].cpu().numpy(), "S": e.root_value_stats()["S"]}
                rc = e.root_children() if rc is None else rc
            for j, bd in enumerate(chunk):
                s = int(status[j])
                if s > 0:
                    out.append(make_record(f"illegal move {s - 1}"))
                elif s < 0:
                    out.append(make_record("invalid position" if s == -1 else "history too long"))
                elif st["over"][j]:
                    out.append(make_record(_winner_text(int(st["winner"][j]))))
                else:
                    lines = []
                    for r in range(self.multipv):
                        ln = int(pv["len"][j, r])
                        if ln:
                            lines.append({"moves": [uci_of[int(i)] for i in pv["moves"][j, r, :ln]], "visits": pv["visits"][j, r, :ln],
                                          "q": pv["q"][j, r], "prior": pv["prior"][j, r]})
                    sv = None
                    if self.solver:
                        from .engine import mate_score, proof_move
                        k = int(rc["k"][j])
                        pm = proof_move(rp["state"][j], rp["dist"][j], rp["child_state"][j], rp["child_dist"][j], rc["acts"][j])
                        sv = {"proven": None if pm is None else uci_of[pm],
                              "mates": {uci_of[int(rc["acts"][j][i])]: mate_score(rp["child_state"][j][i], rp["child_dist"][j][i]) for i in range(k)}}
                    lc = None
                    if lb is not None:
                        stats = {}
                        for i in range(int(rc["k"][j])):
                            n_i, s_i, b_i = int(rc["visits"][j][i]), float(lb["S"][j][i]), float(lb["lcb"][j][i])
                            stats[uci_of[int(rc["acts"][j][i])]] = (math.sqrt(max(s_i, 0.0) / (n_i - 1)) if n_i >= 2 else None,
                                                                    b_i if b_i > float("-inf") else None)
                        lc = {"move": uci_of[int(lb["moves"][j])] if lb["moves"][j] >= 0 else None, "stats": stats}
                    mt = None
                    if ms is not None:
                        from .engine import mate_score
                        hit = int(ms["state"][j]) == 1
                        mt = {"move": uci_of[int(ms["move"][j])] if hit else None,
                              "mate": mate_score(2, int(ms["dist"][j]) - 1) if hit else None}   # (the child is LOSS in dist - 1 plies)
                    if lines:
                        out.append(make_record("ok", pv["root_visits"][j], lines, solver=sv, lcb=lc, mate=mt))
                    else:   # a position given without moves that is already decided: the root never got children
                        oc = bd.outcome()
                        out.append(make_record("ok" if oc is None else _winner_text(None if oc.winner is None else int(bool(oc.winner))),
                                               pv["root_visits"][j]))
        torch.cuda.synchronize(e.device)
        self.seconds += time.perf_counter() - t0
        self.positions += len(boards)
        self.sims += e.stats()["sims"] - sims0
        return out

    def summary(self) -> dict:
        if self.wide is not None:
            sec = max(self.seconds, 1e-9)
            return {"positions": self.positions, "seconds": round(self.seconds, 3), "positions_per_s": round(self.positions / sec, 2),
                    "sims_per_s": round(self.sims / sec, 1), **self.wide.summary()}
        rows = int(self._rows.item()) if (self._rows is not None and self.sp.planned) else self.steps * self.B
        sec = max(self.seconds, 1e-9)
        out = {"positions": self.positions, "seconds": round(self.seconds, 3), "positions_per_s": round(self.positions / sec, 2),
               "sims_per_s": round(self.sims / sec, 1), "evaluator_rows_per_step": round(rows / max(1, self.steps), 2)}
        out.update(self.sp.options.report(self.engine))   # search: the settings as the kernels read them, and how deep the leaves lay
        if self.mate_search is not None:
            from .options import mate_report
            out["mate_search"] = mate_report(self.mate_search, self.mate_opts.mate_counts)
        if "search" in out:
            out["mean_leaf_depth"] = round(out["mean_leaf_depth"], 3)
        if "early_stop" in out:                 # stops per reason, and what a position cost on average
            out["early_stop"]["mean_sims_per_position"] = round(self.sims / max(1, self.positions), 3)
        return out


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m chinesechesszero_amd.analyse", description=__doc__.split("\n\n")[0])
    ap.add_argument("file", metavar="FILE", help="one UCI position per line: startpos [moves ...] | fen <fen> [moves ...]")
    ap.add_argument("--playout", type=int, default=400)
    ap.add_argument("--boards", type=int, default=1024)
    ap.add_argument("--multipv", type=int, default=1)
    ap.add_argument("--max-len", type=int, default=32)
    ap.add_argument("--weights", default=None, help="model file (default: random initialisation)")
    ap.add_argument("--channels", type=int, default=256, help="width of the net's tower")
    ap.add_argument("--blocks", type=int, default=40, help="residual blocks of the net's tower")
    ap.add_argument("--out", default=None, help="JSON lines file (default: stdout)")
    ap.add_argument("--width", type=int, default=1, help="leaves per position and evaluator call (virtual loss); 1: the sequential search")
    ap.add_argument("--solver", action="store_true", help="MCTS-solver: prove decided positions in the tree; every record gains \"mate\": N or null")
    add_search_args(ap)
    add_early_stop_args(ap)
    add_leaf_history_args(ap)
    add_lcb_args(ap)
    add_fused_narrow_args(ap)
    add_mate_search_args(ap)
    args = ap.parse_args(argv)
    mate_search = mate_search_from_args(ap, args)
    leaf_history = leaf_history_from_args(ap, args)
    lcb = lcb_from_args(ap, args)
    search = search_from_args(ap, args)
    early_stop = early_stop_from_args(ap, args)
    with open(args.file, encoding="utf-8") as f:
        try:
            parsed = parse_positions(f)
        except ValueError as e:
            print(f"{args.file}: {e}", file=sys.stderr)
            return 2
    import torch
    if not torch.cuda.is_available():
        print("analyse: no GPU visible to PyTorch-ROCm; the analysis has no CPU fallback", file=sys.stderr)
        return 1
    from .net import PolicyValueNet
    try:
        pvn = PolicyValueNet(model=args.weights, device="cuda:0", num_channels=args.channels, resblocks_num=args.blocks,
                             fused_narrow=fused_narrow_from_args(ap, args))
        if leaf_history is not None:
            pvn.set_leaf_history(True)
        an = BatchedAnalysis(pvn, max(1, min(args.boards, len(parsed) or 1)), n_playout=args.playout, multipv=args.multipv,
                             max_len=args.max_len, solver=args.solver, search=search, width=args.width,
                             early_stop=early_stop, leaf_history=leaf_history, lcb=lcb, mate_search=mate_search)
        records = an.analyse([b for _, b in parsed])
    except CczError as e:
        print(f"analyse: {e}", file=sys.stderr)
        return 1
    out = open(args.out, "w", encoding="utf-8") if args.out else sys.stdout
    try:
        for (no, _), rec in zip(parsed, records):
            out.write(json.dumps({"line": no, **rec}) + "\n")
    finally:
        if args.out:
            out.close()
    s = an.summary()
    print(f"analysed {s['positions']} positions in {s['seconds']} s: {s['positions_per_s']} positions/s, {s['sims_per_s']} sims/s, "
          + (f"width {s['width']}: {s['mean_leaves_per_step']} leaves per board-step, collision share {s['collision_share']}" if "width" in s
             else f"{s['evaluator_rows_per_step']} evaluator rows per step")
          + (f", mean leaf depth {s['mean_leaf_depth']}, search {json.dumps(s['search'])}" if "search" in s else ""), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
