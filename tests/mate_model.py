"""Sequential model of ``ccz_mate_search`` (include/cczero.h "Mate search") on ``oracle.OracleBoard``.

Plain Python, recursive where the kernel keeps an explicit stack. The rules come from the oracle: legal moves in the installed
``legal_moves`` order, ``in_check`` after the push for "gives check", ``xq_repetition_count`` on a board that was pushed through the
fixture's history and the DFS path for "equals an earlier position" (the oracle's chain restarts at a zeroing move, after which no
earlier position can recur), its halfmove clock and ``is_insufficient_material``.

``wrong=`` names a mis-stated rule, so that a test can show that the fixtures tell the difference; the model itself never does:
``repeats_ok`` (a repeated position does not block), ``first_reply`` (the defender is stopped at its first reply), ``budget_per_iteration``
(the node count restarts with every iteration)."""
from __future__ import annotations

import ctypes as C

import oracle

NONE, FOUND, NO_MATE, BUDGET = 0, 1, 2, 3
MAX_PLIES, MAX_NODES = 31, 131072      # CCZ_MATE_MAX_PLIES, CCZ_MATE_MAX_NODES (test_cpu_mate_model.py compares them with the header)
WRONG = ("repeats_ok", "first_reply", "budget_per_iteration")


class _Budget(Exception):
    pass


class MateSearch:
    def __init__(self, max_plies: int, node_budget: int, wrong=None):
        assert max_plies % 2 == 1 and 1 <= max_plies <= MAX_PLIES and node_budget >= 1
        assert wrong is None or wrong in WRONG
        self.max_plies, self.budget, self.wrong = int(max_plies), int(node_budget), wrong
        self.nodes = 0
        self.L = oracle.lib()

    def _count(self):
        self.nodes += 1
        if self.nodes >= self.budget:
            raise _Budget

    def _blocked(self, board) -> bool:
        repeated = self.L.xq_repetition_count(C.byref(board.b)) >= 2 and self.wrong != "repeats_ok"
        return repeated or board.halfmove >= 120 or board.is_insufficient_material()

    def attacker(self, board, r: int, root: bool = False):
        """The first move, in order, that gives check and whose defender node succeeds; None: the node fails."""
        if not root and self._blocked(board):
            return None
        self._count()
        for mv in board.legal_ids():
            c = board.copy()
            c.push_id(mv)
            if c.in_check() and self.defender(c, r - 1):
                return mv
        return None

    def defender(self, board, r: int) -> bool:
        self._count()
        ids = board.legal_ids()
        if not ids:
            return True
        if self._blocked(board) or r == 0:
            return False
        for mv in ids:
            c = board.copy()
            c.push_id(mv)
            if self.attacker(c, r - 1) is None:
                return False
            if self.wrong == "first_reply":
                return True
        return True

    def run(self, board, searched: bool = True):
        """(state, dist, move, nodes) of a root; ``searched`` False: a finished / parked / inactive board."""
        if not searched:
            return NONE, 0, -1, 0
        total = 0
        try:
            for n in range(1, self.max_plies + 1, 2):
                if self.wrong == "budget_per_iteration":
                    total += self.nodes
                    self.nodes = 0
                mv = self.attacker(board, n, root=True)
                if mv is not None:
                    return FOUND, n, int(mv), total + self.nodes
        except _Budget:
            return BUDGET, 0, -1, total + self.nodes
        return NO_MATE, 0, -1, total + self.nodes


def mate_search(board, max_plies: int, node_budget: int, wrong=None, searched: bool = True):
    return MateSearch(max_plies, node_budget, wrong).run(board, searched)


def forced_win(board, plies: int, quiet_plies: int = 3) -> bool:
    """Independent AND/OR replay with the oracle's exact game rules (``is_tie``: the FOURTH repeat, the sixty-move rule, material) on a
    board that carries the real history: the side to move wins within ``plies`` plies against every defence. The defender has all
    replies; a position that ``is_tie()`` is no win for the attacker. The attacker may use any legal move: the checking ones are tried
    first, the quiet ones only with at most ``quiet_plies`` plies left (a full-width attacker seven plies deep does not end; leaving
    moves of the attacker out can only make the replay say no where a win exists, never yes where none does)."""
    ids = board.legal_ids()
    if board.is_tie() or not ids or plies <= 0:
        return False
    kids = []
    for mv in ids:
        c = board.copy()
        c.push_id(mv)
        kids.append((not c.in_check(), c))
    for quiet, c in sorted(kids, key=lambda t: t[0]):           # (stable: checks first, each class in `legal_moves` order)
        if quiet and plies > quiet_plies:
            break
        if _defender_lost(c, plies - 1, quiet_plies):
            return True
    return False


def _defender_lost(board, plies: int, quiet_plies: int) -> bool:
    ids = board.legal_ids()
    if board.is_tie():
        return False
    if not ids:
        return True
    if plies <= 0:
        return False
    for mv in ids:
        c = board.copy()
        c.push_id(mv)
        if not forced_win(c, plies - 1, quiet_plies):
            return False
    return True
