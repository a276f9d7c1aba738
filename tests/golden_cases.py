"""Start positions of the golden search traces (data mirrored from tests/golden/make_golden.py)."""
import numpy as np


def sq(name: str) -> int:
    return (ord(name[0]) - 97) + 9 * int(name[1])


def _place(spec):
    b = np.zeros(90, dtype=np.uint8)
    for name, pc in spec.items():
        b[sq(name)] = pc
    return b


STARTS = {
    "two_rooks": _place({"d0": 7, "a7": 3, "b8": 3, "e9": 15}),
    "capture_to_bare": _place({"e0": 7, "d0": 6, "e1": 9, "d9": 15, "c9": 13}),
    "rook_knight": _place({"e0": 7, "e1": 6, "c2": 4, "h4": 3, "d9": 15, "e8": 14, "a5": 11, "g6": 9}),
    "wide80": _place({"e1": 7, "a2": 3, "i7": 3, "b4": 2, "h5": 2, "c3": 4, "g6": 4, "a6": 1, "c7": 1, "e6": 1, "g7": 1, "i6": 1,
                      "d0": 6, "f0": 6, "c0": 5, "g0": 5, "d9": 15, "e8": 14, "a9": 11}),
    "pawns": _place({"d0": 7, "a3": 1, "c3": 1, "e3": 1, "g3": 1, "i3": 1, "f9": 15, "a6": 9, "c6": 9, "e6": 9, "g6": 9, "i6": 9}),
    # widths around one wave (64 lanes): every per-board kernel holds legal move i and 64 + i in lane i (red to move)
    "wide64": _place({"f0": 6, "e1": 7, "c3": 4, "b4": 2, "h5": 2, "a6": 1, "e6": 1, "g6": 4, "i6": 1, "c7": 1, "g7": 1, "d9": 15}),
    "wide65": _place({"c0": 5, "g0": 5, "e1": 7, "g2": 3, "b3": 2, "e6": 1, "g6": 4, "g7": 2, "i7": 3, "d9": 15, "h9": 1}),
    # 108 legal moves (a seeded hill-climb on the oracle); i2g0 (id 2067) is legal, so its mirror has id 2085 (i7g9) legal
    "widest": _place({"e0": 7, "c1": 3, "d2": 6, "e2": 5, "g2": 4, "i2": 5, "h3": 2, "b4": 2, "a5": 3, "e6": 4, "g6": 1, "d7": 1,
                      "f7": 1, "e8": 1, "g8": 1, "f9": 15}),
    # the widest one with its a5 rook on a0: 103 legal moves, a0a1 (id 0, the first logit of the row) among them
    "wide_a0": _place({"e0": 7, "a0": 3, "c1": 3, "d2": 6, "e2": 5, "g2": 4, "i2": 5, "h3": 2, "b4": 2, "e6": 4, "g6": 1, "d7": 1,
                       "f7": 1, "e8": 1, "g8": 1, "f9": 15}),
    "one_move": _place({"e0": 7, "b1": 11, "a2": 11, "d9": 15}),     # red king: f0 only (rank 1 is covered, d0 faces the king)
    "mated": _place({"e0": 7, "b1": 11, "a0": 11, "d9": 15}),        # red king in check from a0, no legal move
}
# the widest one plus a black knight on h7 and a black rook on a9: 105 legal moves, of which exactly one ends the game -- a5a9, child
# 67 of the root, i.e. in the second 64-lane pass of every per-node loop -- and nothing else is decided within 2 plies
STARTS["wide_late_mate"] = STARTS["widest"].copy()
STARTS["wide_late_mate"][[sq("h7"), sq("a9")]] = (12, 11)


def perpetual_case(checker_is_red: bool):
    """A rook that checks a bare king back and forth (a9+ Ke8, a8+ Ke9, ...): (squares, side to move, the 4-ply cycle)."""
    if checker_is_red:
        return _place({"d0": 7, "a8": 3, "e9": 7 + 8}), 1, ["a8a9", "e9e8", "a9a8", "e8e9"]
    return _place({"d9": 7 + 8, "a1": 3 + 8, "e0": 7}), 0, ["a1a0", "e0e1", "a0a1", "e1e0"]


def perpetual_quiet_cycle(checker_is_red: bool):
    """From the position of perpetual_case: the rook shuffles without giving check, the king steps aside and back."""
    return ["a8a7", "e9f9", "a7a8", "f9e9"] if checker_is_red else ["a1a2", "e0f0", "a2a1", "f0e0"]


def mirrored(squares: np.ndarray) -> np.ndarray:
    """The same position seen from the other side: ranks reversed, colours swapped. With the other side to move it has the
    same number of legal moves."""
    b = np.asarray(squares, np.uint8).reshape(10, 9)[::-1].reshape(90).copy()
    nz = b != 0
    b[nz] ^= 8
    return b


for _name in ("wide64", "wide65", "widest", "wide_a0", "one_move", "mated"):
    STARTS[_name + "_black"] = mirrored(STARTS[_name])

# (side to move, number of legal moves) of the width fixtures; tests/test_cpu_wide_positions.py keeps them true
WIDTHS = {"wide64": (1, 64), "wide65": (1, 65), "widest": (1, 108), "wide_a0": (1, 103), "one_move": (1, 1), "mated": (1, 0),
          "wide80": (1, 80)}
WIDTHS.update({n + "_black": (0, k) for n, (t, k) in list(WIDTHS.items()) if n != "wide80"})
WIDTHS["wide_late_mate"] = (1, 105)

START_ROWS = ["RNBAKABNR", ".........", ".C.....C.", "P.P.P.P.P", ".........",
              ".........", "p.p.p.p.p", ".c.....c.", ".........", "rnbakabnr"]
_PC = {"p": 1, "c": 2, "r": 3, "n": 4, "b": 5, "a": 6, "k": 7}


def start_position() -> np.ndarray:
    b = np.zeros(90, dtype=np.uint8)
    for r, row in enumerate(START_ROWS):
        for f, ch in enumerate(row):
            if ch != ".":
                b[f + 9 * r] = _PC[ch.lower()] + (0 if ch.isupper() else 8)
    return b


def case_start(case):
    """(squares uint8[90], turn, halfmove) of a golden case."""
    if case["start"] == "start":
        return start_position(), 1, 0
    return STARTS[case["start"]].copy(), case["turn"], case["halfmove"]


def case_order(case, move_from=None, move_to=None):
    """(move_rank uint16[2086] | None, type_rank list[8] | None) of a golden case: the `board.legal_moves` order it was
    generated with. ``order_seed``: a random permutation of the ids. ``order == "scan_desc_pawns_last"``: the scheme of
    bitboard libraries in the python-chess family -- non-pawn moves by from-square then to-square in DESCENDING square order,
    pawn moves after them -- which needs the major key by piece type (move_from / move_to: the action table's squares)."""
    if "order_seed" in case:
        return np.random.RandomState(case["order_seed"]).permutation(2086).astype(np.uint16), None
    if case.get("order") == "scan_desc_pawns_last":
        order = np.lexsort((-np.asarray(move_to, np.int64), -np.asarray(move_from, np.int64)))
        rank = np.empty(2086, np.uint16)
        rank[order] = np.arange(2086, dtype=np.uint16)
        return rank, [0, 1, 0, 0, 0, 0, 0, 0]
    return None, None
