"""NumPy restatement of the leaf history planes (ccz_set_leaf_history, include/cczero.h): the evaluator input row
of a pending leaf and its history key, from the positions alone.

  positions = [S_0, ..., S_te]: the recorded root positions of the board's game (S_0 .. S_{p-1}), the root S_p, the positions along
  the selection path (S_{p+1} .. S_{p+d}); te = p + d. History slot i (0..7) shows S_{max(te - i, 0)}. Groups 0..7 hold the red pieces
  of slots 0..7, groups 8..15 the black ones, group 16 is all ones iff red is to move at the leaf; the channel of piece type t is
  plane_of_type[t].

  history key = mix64(leaf_key ^ h_7), h_0 = SEED, h_i = mix64(h_{i-1} ^ P(slot i)); leaf_key = P(S_te) ^ (TURN_KEY if red is to move),
  P(S) = XOR of zob[piece * 90 + square] over the pieces, zob[j] = mix64(GOLDEN * (j + 1)), mix64 = the splitmix64 finaliser.

A mailbox is uint8 [90] (square = rank * 9 + file), a piece is its type 1..7, plus 8 for black. ``HistoryModel`` is the sequential
search model of tests/search_model.py that also keeps, per board, the moves of the descent of its last simulation: the host replay
the GPU test takes the path positions from."""
import numpy as np

import search_model as sm

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SEED = GOLDEN
TURN_KEY = 0x9D39247E33776D41
DEFAULT_PLANES = (0, 0, 1, 2, 3, 4, 5, 6)


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


ZOB = [mix64(GOLDEN * (j + 1)) for j in range(16 * 90)]


def piece_hash(sq):
    h = 0
    for s in range(90):
        if int(sq[s]) & 7:
            h ^= ZOB[(int(sq[s]) & 15) * 90 + s]
    return h


def leaf_key(sq, turn):
    """The engine's Zobrist key of a position with ``turn`` (1 red) to move."""
    return piece_hash(sq) ^ (TURN_KEY if turn else 0)


def slots(positions):
    """The eight positions the row of the leaf ``positions[-1]`` shows, newest first."""
    te = len(positions) - 1
    return [positions[max(te - i, 0)] for i in range(8)]


def history_key(positions, turn):
    h = SEED
    for sq in slots(positions)[1:]:
        h = mix64(h ^ piece_hash(sq))
    return mix64(leaf_key(positions[-1], turn) ^ h)


def row(positions, turn, plane_of_type=None):
    """float16 [17,7,10,9]: the evaluator input of the leaf ``positions[-1]`` with ``turn`` (1 red) to move there."""
    pot = DEFAULT_PLANES if plane_of_type is None else tuple(int(x) for x in plane_of_type)
    out = np.zeros((17, 7, 90), np.float16)
    for i, sq in enumerate(slots(positions)):
        for s in range(90):
            pc = int(sq[s])
            if pc & 7:
                out[(8 if pc & 8 else 0) + i, pot[pc & 7], s] = 1
    out[16] = 1 if turn else 0
    return out.reshape(17, 7, 10, 9)


def squares_of_planes(red, black, plane_of_type=None):
    """A mailbox from the 7 red and 7 black planes of one position (int [7,10,9] each)."""
    pot = DEFAULT_PLANES if plane_of_type is None else tuple(int(x) for x in plane_of_type)
    sq = np.zeros(90, np.uint8)
    for t in range(1, 8):
        sq[np.flatnonzero(np.asarray(red)[pot[t]].reshape(90))] = t
        sq[np.flatnonzero(np.asarray(black)[pot[t]].reshape(90))] = t + 8
    return sq


def move_id(frm, to):
    """The id of the move from square ``frm`` to square ``to`` (square = rank * 9 + file)."""
    from chinesechesszero_amd.tools import MOVE_FROM, MOVE_TO
    hit = np.flatnonzero((np.asarray(MOVE_FROM) == frm) & (np.asarray(MOVE_TO) == to))
    assert hit.size == 1, (frm, to)
    return int(hit[0])


class HistoryModel(sm.SearchModel):
    """SearchModel + per board the moves of its last simulation's descent (``paths[b]``) and the positions S_0 .. S_te of its leaf."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.paths = [[] for _ in range(self.B)]

    def simulate(self, b):
        out = super().simulate(b)
        self.paths[b] = list(self._moves)
        return out

    def positions(self, b):
        """[S_0 .. S_te] of board b's last leaf, and the side to move there."""
        board = self.boards[b].copy()
        pos = [np.asarray(r["sq"], np.uint8).copy() for r in self.plies_rec[b]] + [board.squares().copy()]
        for mv in self.paths[b]:
            board.push_id(mv)
            pos.append(board.squares().copy())
        return pos, int(board.turn)

    def reset_tree(self):
        """ccz_reset_tree on every board."""
        from solver_model import SNode
        for b in range(self.B):
            self.roots[b] = SNode(1.0, -1)


# ---------------------------------------------------------------------------------------------------------------- the GPU test's scenario
# Eight boards from the start position play one forced line: eight quiet pawn moves, then red's cannon takes the knight on b9 (ply 8),
# then one free ply. Boards 0..3 are searched with the line evaluator (paths of d >= 8), boards 4..7 with the near-uniform hash
# evaluator (short paths); the first-play urgency is an absolute 0 on every board. The tree is dropped before ply RESET_AT.
B = 8
SEED_, BASE_ = 77, 4096
SALTS = tuple(range(901, 901 + B))
LINE = ((27, 36), (54, 45), (29, 38), (56, 47), (31, 40), (58, 49), (33, 42), (60, 51), (19, 82))
PLIES = len(LINE) + 1
RESET_AT = 3


def sims_of_ply(t):
    return 14 if t == 0 else 6


def forced_of_ply(t):
    return None if t >= len(LINE) else [move_id(*LINE[t])] * B


def scenario():
    """(model, f): the model of tests/test_gpu_leaf_history.py's row test and the evaluator ``f(b, squares, turn)`` both sides are fed."""
    import gumbel_model as gm
    from oracle import OracleBoard
    line, hashed = line_evaluator(), gm.hash_evaluator(SALTS)
    f = lambda b, sq, turn: line(b, sq, turn) if b < 4 else hashed(b, sq, turn)   # noqa: E731
    m = HistoryModel([OracleBoard() for _ in range(B)], SALTS, SEED_, BASE_, search=sm.settings(sm.ABSOLUTE, 0.0), max_plies=PLIES + 1,
                     evaluator=lambda b, board: f(b, board.squares(), int(board.turn)))
    return m, f


def line_evaluator(peak=0.9):
    """``f(b, squares, turn)``: 0.9 on the first legal move, the rest spread evenly, value 0: with an absolute first-play urgency of 0 the
    search walks one line, a ply deeper with every simulation."""
    from oracle import OracleBoard
    memo = {}

    def f(b, sq, turn):
        sq = np.ascontiguousarray(sq, np.uint8)
        key = (sq.tobytes(), int(turn))
        if key not in memo:
            ids = OracleBoard.from_array(sq, int(turn)).legal_ids()
            P = np.zeros(2086, np.float32)
            if len(ids) == 1:
                P[ids[0]] = 1.0
            elif ids:
                P[ids] = np.float32((1.0 - peak) / (len(ids) - 1))
                P[ids[0]] = np.float32(peak)
            memo[key] = (P, np.float32(0.0))
        return memo[key]
    return f
