"""Batched evaluation matches: many concurrent games between two evaluators on the lockstep engine.

GPU-native form of reference ``Game.start_play`` (game.py:77-130) with two non-self-play ``MCTS_AI``
players (mcts.py:225-229): temperature 1e-3 (visit-count arg-max up to ties), no Dirichlet noise, the
tree is discarded after every move. All games start together from the opening, so every unfinished
board has the same side to move and ONE evaluator call per simulation serves the whole batch; finished
boards idle until the batch is done. (The reference's own evaluator hook is commented out,
train.py:313-319; this is SURVEY 8f row 2.)
"""
from __future__ import annotations

import numpy as np

from .boundary import deliver, kind_of
from .engine import SelfPlayEngine
from .options import SearchOptions, lcb_moves, mate_moves, proven_moves, search_move
from .parameters import C_PUCT
from .stopcfg import StopPoll


class BatchedMatch:
    def __init__(self, evaluator_red, evaluator_black, n_boards: int, n_playout: int = 400, c_puct: float = C_PUCT,
                 seed: int = 0, device: int = 0, max_plies: int = 0, temp: float = 1e-3, solver: bool = False, search=None, early_stop=None, lcb=None,
                 mate_search=None):
        """``solver`` / ``search`` / ``early_stop``: the engine options (``options.OPTIONS``: what ``engine.set_solver`` / ``set_search`` /
        ``set_early_stop`` take; None / False: off), for both sides alike. With the solver the proven move is played where the root is decided
        (``options.proven_moves``); with the early stop the move's loop ends when no board would select any more (``options.search_move``).
        ``lcb``: both sides play the LCB move (``options.MOVE_OPTIONS``) instead of the most visited one; a proven move wins over it.
        ``mate_search``: plies, or the dict of ``options.make_mate_search``: before every move ``ccz_mate_search`` looks for a forced mate by
        consecutive checks, and the mating move is played where one is found (``options.mate_moves``); the search runs all the same."""
        self.options = o = SearchOptions(n_playout, solver=solver, search=search, early_stop=early_stop, lcb=lcb, mate_search=mate_search)
        self.mate_search = o.mate_search
        self.solver, self.search_cfg, self.early_stop, self.lcb = o.keywords().values()
        self.ev = {1: evaluator_red, 0: evaluator_black}
        self.B = n_boards
        self.n_playout = n_playout
        self.temp = temp
        # eps = 0: the sampling distribution is pi itself (mcts.py:227), drawn from the board's Philox stream
        self.engine = SelfPlayEngine(n_boards, n_playout=n_playout, c_puct=c_puct, eps=0.0, alpha=0.2, temp=temp,
                                     seed=seed, device=device, max_plies=max_plies, mirror=False)
        self.proven_moves = 0
        o.apply(self.engine)
        self._poll = StopPoll(self.engine, self.early_stop)
        self.before_move = self.on_move = None
        self._temps = np.full(n_boards, temp, np.float64)

    def play_move(self, turn: int):
        """One lockstep move of every unfinished board by the player of colour ``turn`` (1 RED, 0 BLACK): n_playout
        simulations on a fresh tree, move ~ pi at temperature 1e-3, tree discarded (mcts.py:225-229). Returns the moves
        played (host int32 [B], -1 on finished boards)."""
        e, o = self.engine, self.options
        ev = self.ev[turn]
        search_move(e, self.n_playout, lambda leaf, last: deliver(e, kind_of(ev), *ev(leaf), last), self._poll)
        if self.before_move is not None:
            self.before_move(self)
        forced, proven = proven_moves(e, self.solver)
        self.proven_moves += proven
        if self.mate_search is not None:
            forced, _ = mate_moves(e, self.mate_search, forced, counts=o.mate_counts)
        if self.lcb is not None:
            forced, _ = lcb_moves(e, self.lcb, forced, counts=self.options.lcb_counts)
        moves = e.finish_move(forced_moves=forced, temps=self._temps, keep_tree=False).cpu().numpy()
        if self.on_move is not None:
            self.on_move(self, moves)
        return moves

    def play(self, max_moves: int = 4096, before_move=None, on_move=None):
        """Play every board to the end. Returns dict(red_wins, black_wins, draws, plies). ``before_move(match)`` runs after
        the search and before the move of every lockstep ply, ``on_move(match, moves)`` right after it (tests, logging)."""
        e = self.engine
        self.before_move, self.on_move = before_move, on_move
        self._temps = np.full(self.B, self.temp, np.float64)
        turn = 1
        for _ in range(max_moves):
            st = e.game_status()
            if st["over"].all():
                break
            self.play_move(turn)
            turn ^= 1
        st = e.game_status()
        e.check_healthy()
        w = st["winner"]
        done = st["over"] == 1
        return {"red_wins": int(((w == 1) & done).sum()), "black_wins": int(((w == 0) & done).sum()),
                "draws": int(((w == -1) & done).sum()), "unfinished": int((~done).sum()), "plies": st["plies"].copy()}
