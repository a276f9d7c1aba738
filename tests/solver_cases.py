"""Positions with a short forced result, for the MCTS-solver tests (tests/test_cpu_solver_model.py, tests/test_gpu_solver.py).

Squares only. ``state`` / ``dist`` are what an exhaustive negamax over ``oracle.OracleBoard`` of at most 5 plies returns
(tests/solver_model.py ``certify``): the CPU test recomputes them. ``budget``: simulations after which the model has proven the root
with the ``hash`` evaluator of ``gpu_harness.make_evaluator`` under the case's ``salt`` (found by running the model; the CPU test
asserts them). Every case has the same salt: the evaluator is a function of the position alone, as an evaluation cache assumes. ``move``: the move a front-end plays from the proof (``proof_move``), in UCI, or None."""
from golden_cases import STARTS, _place

WIN, LOSS, DRAW = 1, 2, 3

# (name, squares, side to move (1 red), state, dist, salt, budget, move)
CASES = [
    # red Ra7-a9 mates
    ("two_rooks", STARTS["two_rooks"], 1, WIN, 1, 21, 12, "a7a9"),
    # red mates in two: Ri7-i8 (Kf9 forced: d9 faces the red king, e8 is on the rook's rank), Ri8-i9; the pawn on g7 ... g8 holds f8
    ("mate_in_two", _place({"d0": 7, "i7": 3, "g7": 1, "e9": 15}), 1, WIN, 3, 21, 22, "i7i8"),
    # black to move is mated in 2 plies whatever it plays (Kf9 or the pawn): Ra7-a9 follows
    ("mated_in_two_plies", _place({"d0": 7, "a7": 3, "b8": 3, "e9": 15, "i5": 9}), 0, LOSS, 2, 21, 26, "i5i4"),
    # red is in check from the last attacking piece on the board and can only capture it: bare kings, advisors and a bishop remain
    ("forced_draw", _place({"e0": 7, "d0": 6, "f0": 6, "e1": 9, "d9": 15, "c9": 13}), 1, DRAW, 0, 21, 6, None),
    # `mated` one ply below the root (black Ra2-a0); Rb1-f1, which leaves red without a legal move, comes first in the move order
    ("mated_below", STARTS["one_move"], 0, WIN, 1, 21, 16, "b1f1"),
    # `mated_black` one ply below the root: red plays Ra7-a9
    ("mated_black_below", STARTS["one_move_black"], 1, WIN, 1, 21, 12, "a7a9"),
    # the candidate the forced draw was derived from: the king can step aside, nothing is decided within 5 plies
    ("capture_to_bare", STARTS["capture_to_bare"], 1, 0, 0, 21, 0, None),
]
NAMES = [c[0] for c in CASES]
SALTS = tuple(c[5] for c in CASES)
SIMS = max(c[6] for c in CASES)          # the GPU test runs every board this many simulations in lockstep: 7 x 26 = 182 <= 256
assert len(CASES) <= 8 and len(CASES) * SIMS <= 256


def boards():
    from oracle import OracleBoard
    return [OracleBoard.from_array(sq, turn) for _, sq, turn, *_ in CASES]
