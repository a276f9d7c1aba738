"""Pairs of positions for forced full-key collisions in the evaluation cache (tests/test_gpu_cache_key_collisions.py).

``ccz_set_routing(salt0, salt1)`` XORs a caller-chosen salt into every cache key, so for two positions X and Y with keys kX and kY
a salt of kX ^ kY puts X's evaluation under Y's full 64-bit key. What then keeps Y from being served X's priors is the tag of
cache_tag (csrc/cczero_kernels.h): the legal-move count (8 bits) and a 24-bit hash of the ordered legal-move list. A pair is
therefore described by the relation between the two ``legal_ids()`` lists:

- ``same_list``: the lists are equal although the positions differ (a *twin*): the tags are equal, the documented residual. These
  pairs are the positive controls -- a forged key that does NOT serve the twin's entry means the construction is broken;
- ``different_count``: the counts differ, the ``k`` byte of the tag separates them;
- ``equal_count``: equal counts, different lists: only the 24-bit list hash separates them;
- ``wide_equal_count``: equal counts above 64, lists that agree on entries 0..63 and differ after them: only the ``64 + lane`` term of
  the list hash (the second id of a lane) separates them.

tests/test_cpu_cache_collision_fixtures.py asserts every pair on the CPU oracle."""
import functools

import numpy as np

from golden_cases import STARTS, sq, start_position

# squares a piece type may stand on (red's view; black's are the mirrored ones): king and advisors in the palace, elephants on their
# seven points, a pawn on its own side only on the five pawn files from rank 3 on
_PALACE = {f + 9 * r for f in (3, 4, 5) for r in (0, 1, 2)}
_ADVISOR = {sq(s) for s in ("d0", "f0", "e1", "d2", "f2")}
_ELEPHANT = {sq(s) for s in ("c0", "g0", "a2", "e2", "i2", "c4", "g4")}
_PAWN = {f + 9 * r for f in (0, 2, 4, 6, 8) for r in (3, 4)} | {f + 9 * r for f in range(9) for r in range(5, 10)}
ALLOWED = {1: _PAWN, 5: _ELEPHANT, 6: _ADVISOR, 7: _PALACE}


def misplaced(squares):
    """Squares whose piece may not stand there ([] for a position that can occur in a game)."""
    bad = []
    for s in range(90):
        pc = int(squares[s])
        if not pc:
            continue
        t, black = pc & 7, pc >= 8
        seen = (s % 9) + 9 * (9 - s // 9) if black else s
        if t in ALLOWED and seen not in ALLOWED[t]:
            bad.append(s)
    return bad


def loadable(squares, halfmove=0, n_moves=0, max_moves=0):
    """What ccz_set_positions validates before it loads a board (k_set_positions, include/cczero.h): piece codes, exactly one king
    and at most 16 pieces per side, a clock >= 0 and a move count inside the row."""
    s = np.asarray(squares, np.int64)
    if s.shape != (90,) or ((s > 15) | (s == 8) | (s < 0)).any():
        return False
    red, black = (s >= 1) & (s <= 7), (s >= 9) & (s <= 15)
    return int((s == 7).sum()) == 1 and int((s == 15).sum()) == 1 and red.sum() <= 16 and black.sum() <= 16 \
        and halfmove >= 0 and -1 <= n_moves <= max_moves


def _swapped(squares, a, b):
    out = np.array(squares, np.uint8)
    out[a], out[b] = out[b], out[a]
    return out


def _moved(squares, a, b):
    out = np.array(squares, np.uint8)
    assert out[a] and not out[b]
    out[b], out[a] = out[a], 0
    return out


def _pool():
    from test_gpu_above_4096_boards import pool
    return pool()


@functools.lru_cache(maxsize=1)
def pool_lists():
    """The oracle's legal ids of every midgame pool position (test_gpu_above_4096_boards.pool)."""
    from oracle import OracleBoard
    squares, turn, P = _pool()
    return [tuple(OracleBoard.from_array(squares[i], int(turn[i]), 0).legal_ids()) for i in range(P)]


def one_entry_pool_pairs():
    """Pool pairs of one side to move and one count whose ordered lists differ in exactly one entry."""
    _, turn, P = _pool()
    ls = pool_lists()
    return [(i, j) for i in range(P) for j in range(i + 1, P)
            if turn[i] == turn[j] and len(ls[i]) == len(ls[j]) and sum(x != y for x, y in zip(ls[i], ls[j])) == 1]


@functools.lru_cache(maxsize=1)
def pairs():
    """name -> (X, Y, relation), X and Y = (squares uint8 [90], side to move). X is the position whose evaluation is stored first."""
    squares, turn, P = _pool()
    ls = pool_lists()
    start = start_position()
    # a midgame position (past the first 20 of the pool: several plies into a walk) whose count is not the opening's 44
    mid = next(i for i in range(20, P) if len(ls[i]) != 44)
    # the first two pool positions with one side to move and one count, but another list
    eq = next((i, j) for i in range(P) for j in range(i + 1, P)
              if turn[i] == turn[j] and len(ls[i]) == len(ls[j]) and ls[i] != ls[j])
    pos = lambda i: (squares[i].copy(), int(turn[i]))
    return {
        # black's a9 rook and b9 knight exchanged: nothing red can do on its first move reaches them
        "twin": ((start, 1), (_swapped(start, sq("a9"), sq("b9")), 1), "same_list"),
        # the lone black king on d9 instead of f9: red's 108 moves are the same
        "wide_twin": ((STARTS["widest"].copy(), 1), (_moved(STARTS["widest"], sq("f9"), sq("d9")), 1), "same_list"),
        "different_count": ((start, 1), pos(mid), "different_count"),
        "equal_count": (pos(eq[0]), pos(eq[1]), "equal_count"),
        "wide_different": ((STARTS["widest"].copy(), 1), (STARTS["wide_a0"].copy(), 1), "different_count"),
        # `widest` with its c1 rook on i6 and on i8: 98 moves each, the same first 73 entries, 19 later entries differ
        "wide_equal_count": ((_moved(STARTS["widest"], sq("c1"), sq("i6")), 1), (_moved(STARTS["widest"], sq("c1"), sq("i8")), 1),
                             "wide_equal_count"),
    }


PAIRS = ("twin", "wide_twin", "different_count", "equal_count", "wide_different", "wide_equal_count")
TWINS = ("twin", "wide_twin")


def search_positions():
    """For the routed search under adversarial salts: the opening, and the red first moves that lead to P (quiet), Q (the cannon
    capture b2xb9: another black reply list) and Q' (a second quiet move, the same black reply list as P: a twin of P)."""
    from oracle import lib
    L = lib()
    mv = lambda s: int(L.xq_move_id(sq(s[:2]), sq(s[2:])))
    return {"P": mv("a3a4"), "Q": mv("b2b9"), "Q_twin": mv("c3c4")}


def after(move_id):
    """(squares, side to move) of the opening after red's ``move_id``."""
    from oracle import OracleBoard
    b = OracleBoard()
    b.push_id(move_id)
    return b.squares()[:90], int(b.turn)
