"""Fixtures for the engine's sticky error paths (``CCZ_ERR_*``, include/cczero.h): one engine per case, a few FAULTY boards that run
into one bounded resource among CLEAN boards that never do, and the script both backends are driven through -- the host twins of
oracle/ccz_ref.c, which know the engine's limits, on the CPU (tests/test_cpu_engine_limits.py asserts every number stated here on
them and on the oracle), libcczero.so on the GPU (tests/test_gpu_engine_limits.py compares it with the twins byte for byte).

The driver is ``drive()`` of tests/test_gpu_ref_twins.py: per move ``n`` lockstep simulations, the roots, the move, the status. A case
adds what that script has no word for through ``Scripted``, a shim both backends are wrapped in: forced moves and fresh roots per
move, and the sticky error word in every status event. The evaluator is per board (``evals``):
  ("uniform",)      1 / k on the legal moves, value 0 (oracle.evaluators.uniform_eval)
  ("hash", salt)    a position hash (oracle.evaluators.hash_eval)
  ("sharp", salt)   prior 0.97 on one hash-chosen legal move, 0.03 / k on each, value 0: PUCT digs one long line
                    (tests/test_gpu_search.py::test_deep_paths_beyond_one_wave)
  ("nan",)          every prior NaN, value 0

The limits, as ccz_create derives them: ``max_nodes`` nodes per board (a leaf whose k children do not fit stays unexpanded: bit 1),
``max_depth`` path entries (a descent that would reach that many moves is dropped: bit 2), 80 x ``max_plies`` pi entries per board (a
ply whose k entries do not fit ends the game: bit 8); a re-root keeps at most ``max_nodes - reserve_nodes`` nodes, which every case
here stays below (pruning is pinned elsewhere)."""
import numpy as np

from golden_cases import STARTS, _place, sq as S, start_position

START = (start_position(), 1, 0)
TWO_ROOKS = (STARTS["two_rooks"].copy(), 1, 0)                  # K + 2 R against a bare king: a sparse endgame
PAWNS = STARTS["pawns"]                                         # kings and five pawns each: long quiet lines
# A red rook pinned on the e-file by a black rook (e4 may not leave the file), a red rook on a0 behind its own pawn on a3
PIN = (_place({"e0": 7, "e4": 3, "a0": 3, "a3": 1, "d9": 15, "e8": 11}), 1, 0)
# Both sides wide. No width fixture of golden_cases has a wide reply (black is a bare king there), so this is its "widest" position with
# a black army added (a hill-climb on the oracle): 100 legal moves for red, and 67 for black after red's first one, Ke0-e1 (id 81)
WIDE_PAIR = (STARTS["widest"].copy(), 1, 0)
for _name, _pc in {"f0": 10, "a3": 11, "e4": 12, "g4": 12, "i5": 11, "c9": 10}.items():
    WIDE_PAIR[0][S(_name)] = _pc


def move_id(uci: str) -> int:
    from oracle import lib
    return int(lib().xq_move_id(S(uci[:2]), S(uci[2:])))


def case_evaluator(evals):
    """Batched evaluator on (squares [B,90], turn [B]) -> (P float32 [B,2086], V float32 [B]), board b by ``evals[b]``."""
    from oracle import OracleBoard
    from oracle.evaluators import hash_eval, position_hash, uniform_eval

    def ev(sq, turn):
        P = np.zeros((len(sq), 2086), np.float32)
        V = np.zeros(len(sq), np.float32)
        for b, spec in enumerate(evals):
            if not sq[b].any():                                  # no pending leaf: an empty row nobody reads
                continue
            if spec[0] == "uniform":
                p, v = uniform_eval(sq[b:b + 1], turn[b:b + 1])
                P[b], V[b] = p[0], v[0]
            elif spec[0] == "hash":
                p, v = hash_eval(sq[b:b + 1], turn[b:b + 1], salt=spec[1], scale=1.0)
                P[b], V[b] = p[0], v[0]
            elif spec[0] == "sharp":
                ids = OracleBoard.from_array(sq[b], int(turn[b]), 0).legal_ids()
                if ids:
                    P[b, ids] = np.float32(0.03 / len(ids))
                    P[b, ids[int(position_hash(sq[b:b + 1], turn[b:b + 1], spec[1])[0] % np.uint64(len(ids)))]] = np.float32(0.97)
            else:
                assert spec[0] == "nan"
                P[b] = np.float32("nan")
        return P, V

    return ev


class Scripted:
    """The call surface of ``drive()`` around a backend ``x`` (RefEngine, or the GPU tests' device wrappers), plus the case's script:
    ``forced[mv]``: int32 [B] forced ids of move mv (-1: sampled; absent: all sampled); ``fresh[mv]``: boards whose tree is reset
    right before move mv (``reset_tree``: a root that is not searched). ``flags()``: the backend's sticky error word, which joins
    every status event."""

    def __init__(self, x, case, flags):
        self.x, self.case, self.flags, self.mv = x, case, flags, 0
        self.usage = []          # the twins only: (usage before move mv, usage after it)

    def set_position(self, *a):
        self.x.set_position(*a)

    def select_leaves(self):
        return self.x.select_leaves()

    def expand_backup(self, P, V):
        self.x.expand_backup(P, V)

    def finish_move(self, forced_moves=None):
        assert forced_moves is None
        fresh = self.case.get("fresh", {}).get(self.mv)
        if fresh:
            self.x.reset_tree(np.isin(np.arange(self.case["B"]), fresh).astype(np.uint8))
        f = self.case.get("forced", {}).get(self.mv)
        self.mv += 1
        before = self.x.usage() if hasattr(self.x, "usage") else None
        out = self.x.finish_move(forced_moves=None if f is None else np.asarray(f, np.int32))
        if before is not None:
            self.usage.append((before, self.x.usage()))
        return out

    def root_children(self):
        return self.x.root_children()

    def game_status(self):
        st = dict(self.x.game_status())
        st["error_flags"] = np.array([self.flags()], np.int32)
        return st

    def leaf_info(self):
        return self.x.leaf_info()

    def root_positions(self):
        return self.x.root_positions()


def run(x, case, flags):
    """Drive backend ``x`` through the case: (the log of ``drive()`` -- n + 3 events per move; with ``finish_first`` after the two
    events of a ``finish_move`` with nothing searched --, the twins' usage around every move)."""
    import test_gpu_ref_twins as T
    s = Scripted(x, case, flags)
    log = []
    for b, st in enumerate(case["starts"]):
        x.set_position(b, *st)
    if case.get("finish_first"):
        log.append(("moves", x.finish_move()))
        log.append(("status", s.game_status(), x.root_positions()))
    saved = T.make_evaluator
    T.make_evaluator = lambda kind, salts: case_evaluator(case["evals"])   # drive() asks for its evaluator by name: the case's own
    try:
        return log + T.drive(s, "case", (), case["n"], case["moves"]), s.usage
    finally:
        T.make_evaluator = saved


def ref_engine(case):
    from oracle import RefEngine
    return RefEngine(case["B"], **case["engine"])


def run_ref(case):
    """(log, usage around every move, usage at the end) of the host twins."""
    ref = ref_engine(case)
    try:
        return run(ref, case, ref.error_flags) + (ref.usage(),)
    finally:
        ref.close()


_COMMON = dict(seed=9, board_id_base=1000, eps=0.25, alpha=0.2, temp=1.0)

CASES = {}

# ---- pool: 200 nodes hold the start position's root and three of its children's expansions (1 + 4 x 44 = 177; a fifth needs 221).
# Uniform priors visit the root's children in order, one simulation each. The kept subtree of the sampled move is a child and at most
# its 44 children; budget 200 - 70 = 130. In the second search the pool has room again (three more expansions), then runs out again.
CASES["pool"] = dict(
    B=6, n=20, moves=2, engine=dict(n_playout=20, max_nodes=200, reserve_nodes=70, **_COMMON),
    starts=[START, START, START, TWO_ROOKS, TWO_ROOKS, (TWO_ROOKS[0], 0, 0)],
    evals=[("uniform",), ("hash", 3), ("hash", 4), ("uniform",), ("hash", 5), ("hash", 6)],
    forced={0: [0, -1, -1, -1, -1, -1]},      # board 0 keeps its first child a0a1 (id 0), which was expanded: 45 nodes
    faulty=[0, 1, 2], bit=1, flags=1, word="node pool")

# ---- depth: 64 path entries = leaves at depth <= 63. The sharp evaluator's line reaches depth 63 after DEPTH_FIRST_DROP[b] simulations
# on board b; the next descent along it is dropped, and so is every later one until the board moves. (found on the twin, asserted there)
DEPTH_FIRST_DROP = {0: 575, 1: 508}      # the first dropped selection of board b, counting from 1
DEPTH_N = 580                           # both boards frozen, and a few lockstep simulations more
CASES["depth"] = dict(
    B=4, n=DEPTH_N, moves=2, engine=dict(n_playout=DEPTH_N, max_depth=64, **_COMMON),
    starts=[(PAWNS, 1, 0), (PAWNS, 0, 0), (PAWNS, 1, 0), (PAWNS, 0, 0)],
    evals=[("sharp", 1), ("sharp", 2), ("uniform",), ("uniform",)],
    faulty=[0, 1], bit=2, flags=2, word="max_depth")

# ---- nan: root + 44 children take 45 simulations (an unvisited child scores +inf whatever its prior); the 46th descent finds
# 44 NaN scores. After the move the new root is an unexpanded child: its expansion and its children's first visits, then NaN again.
CASES["nan"] = dict(
    B=4, n=50, moves=2, engine=dict(n_playout=50, **_COMMON),
    starts=[START, START, TWO_ROOKS, START],
    evals=[("nan",), ("hash", 7), ("hash", 8), ("uniform",)],
    faulty=[0], bit=32, flags=32, word="NaN")

# ---- record: max_plies = 2 -> 160 pi entries per board. Ply 0 of WIDE_PAIR takes RECORD_K0, the reply to its first move would take
# RECORD_K1: more than 160 together, so the game ends at ply 1 with ply 0 recorded. The clean boards (44 + 44) run to the ply cap.
RECORD_K0, RECORD_K1, RECORD_FIRST = 100, 67, 81
CASES["record"] = dict(
    B=4, n=3, moves=3, engine=dict(n_playout=3, max_plies=2, **_COMMON),
    starts=[WIDE_PAIR, WIDE_PAIR, START, START],
    evals=[("uniform",), ("hash", 9), ("uniform",), ("hash", 10)],
    forced={0: [RECORD_FIRST, RECORD_FIRST, -1, -1]},
    faulty=[0, 1], bit=8, flags=8, word="arena")

# ---- bad move: after 8 simulations boards 0..4 are handed a move that is not legal, the others legal ones. PIN's 8-simulation tree
# fits 200 nodes once and not twice, which is how a refused board that kept its old node count shows in the second search.
BAD_IDS = {0: 2086,                     # outside the action table
           1: "b5b6",                   # from an empty square
           2: "e8e7",                   # the opponent's rook
           3: "a0a5",                   # the rook through its own pawn on a3
           4: "e4a4"}                   # the pinned rook leaves the file: own king in check; on a root that is not searched
CASES["bad_move"] = dict(
    B=8, n=8, moves=2, engine=dict(n_playout=8, max_nodes=200, reserve_nodes=70, **_COMMON),
    starts=[PIN] * 6 + [TWO_ROOKS, PIN],
    evals=[("hash", 20 + b) for b in range(8)],
    fresh={0: [4, 6]},                  # board 6: a legal forced move on a root that is not searched
    forced={0: [BAD_IDS[0]] + [move_id(BAD_IDS[b]) for b in (1, 2, 3, 4)] + [move_id("e4e5"), move_id("a7a0"), -1]},
    faulty=[0, 1, 2, 3, 4], bit=16, flags=16, word="forced move")

# ---- nothing to move: finish_move before any search refuses every board; the search and the move after it are ordinary
CASES["nothing"] = dict(
    B=4, n=12, moves=1, engine=dict(n_playout=12, **_COMMON), finish_first=True,
    starts=[START, TWO_ROOKS, PIN, START],
    evals=[("hash", 30), ("hash", 31), ("uniform",), ("uniform",)],
    faulty=[0, 1, 2, 3], bit=16, flags=16, word="forced move")
