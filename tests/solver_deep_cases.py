"""Fixtures for the two paths of the MCTS-solver that no hash-evaluated position reaches, and the model's run on them, recorded once
(tests/test_cpu_solver_deep.py asserts every condition stated here on the model and the oracle; tests/test_gpu_solver_deep.py compares
the engine with the recorded run).

A. Deep proof walks. One quiet line that ends in a mate at depth d = 63, 64, 65, 67 (``proof_backup`` holds path nodes 0..63 in lane
   registers and reads deeper ones through ``path[]``: d = 63 is the all-lanes control, 64 the first leaf read from memory, 65 and 67
   walk one and three levels in the memory form before they hand over to the lanes at level 63). Red: K f0, R g5, R h7, P d6,
   elephant e2; black: K e8, pawn a4. Each side shuffles -- the elephant cycles e2 g4 i2 g0, the pawn walks a snake that never steps
   back and then paces rank 0 -- then Rg5-g8+ Ke8-e9 (the only reply) Rh7-h9 mate. The evaluator is scripted: prior 1.0 on the line's
   move at the line's position OF THAT DEPTH (the rank-0 tail revisits squares), uniform over the legal moves elsewhere, value 0.
   A fifth board plays the d = 67 line from halfmove 54: the sixty-move rule ends it at depth 66, a DRAW leaf whose walk ends inside
   the memory form.

B. Withdrawal at a pruned, proven root (``PRUNE``; found by a random placement search over the oracle). The root has halfmove 117;
   after Ra0-i0 and the elephant's g5-i7 the node N, red to move at halfmove 119, is WIN in 3 by its only capture, Ri0xi7+ (the
   advisor's e8-f7 is the only reply, Rc5-e5 mates), and every quiet move of N is a DRAW leaf under the sixty-move rule. g5-i7 is
   the last of black's nine moves, so in the re-root on Ra0-i0 with the smallest budget the engine allows (129 nodes) the children
   of N's first three siblings use the budget up: N keeps N, Q, P and its byte and loses its children. The second re-root makes it
   the root. The evaluator is scripted by position: prior 1.0 on the five moves above, uniform elsewhere, value 0."""
import functools

import numpy as np

import solver_model as sm
from golden_cases import _place

# ---------------------------------------------------------------------------------------------------------------- A: the line
SQUARES = _place({"f0": 7, "g5": 3, "h7": 3, "d6": 1, "e2": 5, "e8": 15, "a4": 9})
ELEPHANT = ["e2", "g4", "i2", "g0"]
PAWN = ["a4", "b4", "c4", "d4", "e4", "e3", "d3", "c3", "b3", "a3", "a2", "b2", "c2", "d2", "d1", "c1", "b1", "a1", "a0", "b0", "c0", "d0",
        "c0", "b0", "a0", "b0", "c0", "d0", "c0", "b0", "a0", "b0", "c0"]
END = ["g5g8", "e8e9", "h7h9"]

# (name, depth of the mate, side to move at the root (1 red), halfmove clock of the root)
CASES = [("d63", 63, 1, 0), ("d64", 64, 0, 0), ("d65", 65, 1, 0), ("d67", 67, 1, 0), ("d67_sixty", 67, 1, 54)]
NAMES = [c[0] for c in CASES]
DEPTHS = [c[1] for c in CASES]
B = len(CASES)
FORK = 1300                                # simulations every board has run before its first decided leaf: where a mis-stated walk may start
PAST = 40                                  # simulations run past the first decided leaf of the slowest board
MAX_NODES, RESERVE_NODES = 16384, 128      # per pool half, and what a re-root keeps free of it: nothing is pruned (asserted on the CPU)
MAX_DEPTH = 128                            # >= 68 path nodes

# ---------------------------------------------------------------------------------------------------------------- B: the pruned root
PRUNE = {
    "squares": _place({"a0": 3, "d2": 7, "h3": 9, "c5": 3, "g5": 13, "e7": 15, "e8": 14, "f9": 1}),
    "turn": 1, "halfmove": 117,
    "line": ["a0i0", "g5i7", "i0i7", "e8f7", "c5e5"],      # two quiet moves to N, the capture with check, the only reply, the mate
    "max_nodes": 2048, "reserve_nodes": 2048 - 129,        # the kept subtree's budget: 129 nodes, the engine's minimum
    "past": 5,                                             # simulations after N is proven / after the root is proven again
}
PRUNE_BUDGET = PRUNE["max_nodes"] - PRUNE["reserve_nodes"]


def line_uci(d, turn):
    """The d moves of the line in UCI. Red root: (d - 3) / 2 shuffles each; black root: black shuffles once more and first."""
    n_red, n_black = ((d - 3) // 2, (d - 3) // 2) if turn else ((d - 4) // 2, (d - 2) // 2)
    red = [ELEPHANT[i % 4] + ELEPHANT[(i + 1) % 4] for i in range(n_red)]
    black = [PAWN[i] + PAWN[i + 1] for i in range(n_black)]
    out = []
    for i in range(max(n_red, n_black)):
        out += (red[i:i + 1] + black[i:i + 1]) if turn else (black[i:i + 1] + red[i:i + 1])
    assert len(out) == d - 3
    return out + END


def move_id(board, uci):
    """The id of a legal move given in UCI (raises where it is not legal)."""
    return board.legal_ids()[board.legal_moves.index(uci)]


def boards():
    from oracle import OracleBoard
    return [OracleBoard.from_array(SQUARES, turn, half) for _, _, turn, half in CASES]


def prune_board():
    from oracle import OracleBoard
    return OracleBoard.from_array(PRUNE["squares"], PRUNE["turn"], PRUNE["halfmove"])


class Script:
    """A scripted evaluator: ``row(b, squares, turn, depth) -> P float32 [2086]``, prior 1.0 on board b's line move where the
    position is the line's (``by_depth``: the line's position of that depth), uniform over the legal moves elsewhere; value 0."""

    def __init__(self, roots, lines, by_depth):
        self.by_depth = by_depth
        self.ids, self.pos = [], []
        for board, line in zip(roots, lines):
            board = board.copy()
            ids, pos = [], []
            for uci in line:
                pos.append((board.squares().tobytes(), int(board.turn)))
                ids.append(move_id(board, uci))
                board.push_id(ids[-1])
            self.ids.append(ids)
            self.pos.append(pos)
        self.legal = {}

    def row(self, b, sq, turn, depth):
        key = (np.ascontiguousarray(sq, np.uint8).tobytes(), int(turn))
        P = np.zeros(2086, np.float32)
        if self.by_depth:
            at = depth if depth < len(self.ids[b]) and self.pos[b][depth] == key else -1
        else:
            at = self.pos[b].index(key) if key in self.pos[b] else -1
        if at >= 0:
            P[self.ids[b][at]] = np.float32(1.0)
            return P
        if key not in self.legal:
            from oracle import OracleBoard
            self.legal[key] = OracleBoard.from_array(np.frombuffer(key[0], np.uint8), key[1]).legal_ids()
        ids = self.legal[key]
        if ids:
            P[ids] = np.float32(1.0 / len(ids))
        return P

    def model_evaluator(self):
        """``evaluator(b, board)`` of ``SolverModel``: the depth is the board's ply count (a fixture's root is at ply 0)."""
        return lambda b, board: (self.row(b, board.squares(), int(board.turn), int(board.b.ply)), np.float32(0.0))


@functools.lru_cache(maxsize=None)
def script():
    return Script(boards(), [line_uci(d, turn) for _, d, turn, _ in CASES], by_depth=True)


@functools.lru_cache(maxsize=None)
def prune_script():
    return Script([prune_board()], [PRUNE["line"]], by_depth=False)


# ---------------------------------------------------------------------------------------------------------------- the recorded runs
def top(m, b):
    """What the engine shows of board b's tree top: root children, root visits, proof bytes, the proof move."""
    acts, N, Q, P = m.root_children(b)
    st, ds, cs, cd = m.root_proof(b)
    pm = m.proof_move(b)
    return {"acts": acts, "N": N, "Q": Q, "P": P, "root_n": m.roots[b].N, "proof": (st, ds), "cs": cs, "cd": cd, "pm": -1 if pm is None else pm}


def stats(m, over=()):
    """``solver_stats()`` of the engine: its ``roots_proven`` counts the boards whose game is running."""
    s = m.stats()
    s["roots_proven"] = sum(1 for b, r in enumerate(m.roots) if m.solver and sm.state_of(r.proof) and not (over and over[b]))
    return s


def clone_tree(root):
    def one(o):
        n = sm.SNode(o.P, o.move)
        n.N, n.Q, n.proof = o.N, o.Q, o.proof
        return n
    new = one(root)
    stack = [(root, new)]
    while stack:
        o, n = stack.pop()
        if o.kids is not None:
            n.kids = [one(c) for c in o.kids]
            stack.extend(zip(o.kids, n.kids))
    return new


def line_nodes(m, b, ids):
    """The nodes of board b's tree along the move ids, the root first, as far as the tree goes."""
    node, out = m.roots[b], [m.roots[b]]
    for i in ids:
        node = next((c for c in (node.kids or []) if c.move == i), None)
        if node is None:
            break
        out.append(node)
    return out


class Trace:
    pass


def _search(m, t, n):
    for _ in range(n):
        t.leaves.append([m.simulate(b) for b in range(m.B)])
        t.tops.append([top(m, b) for b in range(m.B)])
        t.stats.append(stats(m))


def _deep_facts(m, t):
    sc = script()
    t.nodes = [sum(1 for _ in m.walk(b)) for b in range(B)]
    t.line = [[(n.N, n.Q, n.proof, len(n.kids or [])) for n in line_nodes(m, b, sc.ids[b])] for b in range(B)]
    t.first = [next((i for i, row in enumerate(t.leaves) if row[b][0] != sm.LEAF_EXPAND), None) for b in range(B)]
    t.counters = {"rows": m.rows, "sims": m.sims}


@functools.lru_cache(maxsize=None)
def deep_trace(solver=True, only=None):
    """The model's run on the boards of ``CASES`` (``only``: that board alone) in lockstep: ``leaves[i][b]`` (status, k, depth),
    ``tops[i][b]``, ``stats[i]`` after simulation i; ``first[b]``: the first decided simulation; ``nodes`` / ``line``: the trees after
    the search; ``moves[s]`` / ``over[s]`` / ``walk_tops[s]`` / ``walk_stats[s]``: the line walked by re-roots. ``fork``: the roots
    after FORK simulations."""
    sc = script()
    sel = list(range(B)) if only is None else [only]
    ev = sc.model_evaluator()
    m = sm.SolverModel([boards()[b] for b in sel], [0] * len(sel), solver=solver, evaluator=lambda b, board: ev(sel[b], board))
    t = Trace()
    t.leaves, t.tops, t.stats = [], [], []
    _search(m, t, FORK)
    t.fork = [clone_tree(r) for r in m.roots]
    t.fork_counters = (m.rows, m.sims)
    assert m.stats() == {"nodes_proven": 0, "proven_stops": 0, "roots_proven": 0}
    if only is not None:
        _search(m, t, _sims() - FORK)
        t.roots = m.roots
        return t
    decided, last = set(), None
    while last is None or len(t.leaves) < last + 1 + PAST:
        _search(m, t, 1)
        decided |= {b for b in range(B) if t.leaves[-1][b][0] != sm.LEAF_EXPAND}
        if last is None and len(decided) == B:
            last = len(t.leaves) - 1
        assert len(t.leaves) < 4 * FORK
    _deep_facts(m, t)
    t.moves, t.over, t.walk_tops, t.walk_stats = [], [], [], []
    over = [False] * B
    for s in range(max(DEPTHS)):
        mv = [-1 if over[b] else sc.ids[b][s] for b in range(B)]
        for b in range(B):
            if mv[b] >= 0:
                m.update_with_move(b, mv[b])
                over[b] = m.boards[b].is_game_over() or m.boards[b].is_tie()
        t.moves.append(mv)
        t.over.append(list(over))
        t.walk_tops.append([top(m, b) for b in range(B)])
        t.walk_stats.append(stats(m, over))
    return t


def _sims():
    return len(deep_trace().leaves)


def wrong_deep_trace(wrong):
    """The same run from the fork on with a mis-stated walk: (leaves, stats, nodes / line / first / counters as in ``deep_trace``)."""
    ref = deep_trace()
    m = sm.SolverModel(boards(), [0] * B, evaluator=script().model_evaluator(), wrong=wrong)
    m.roots = [clone_tree(r) for r in ref.fork]
    m.rows, m.sims = ref.fork_counters
    t = Trace()
    t.leaves, t.tops, t.stats = list(ref.leaves[:FORK]), list(ref.tops[:FORK]), list(ref.stats[:FORK])
    _search(m, t, len(ref.leaves) - FORK)
    _deep_facts(m, t)
    return t


@functools.lru_cache(maxsize=None)
def prune_trace(wrong=None):
    """The model's run on ``PRUNE``: search until N is proven and ``past`` simulations more, the two re-roots under the budget, search
    until the root is proven again and ``past`` more (a mis-stated model: as many simulations as the model itself). ``leaves`` /
    ``tops`` / ``stats`` per simulation as in ``deep_trace``; ``reroot_at``: the simulations done before the re-roots; ``tree_before``:
    a copy of the tree the first re-root starts from; ``reroots[j]``: (move id, top, stats, pruned_subtrees, nodes kept) after re-root
    j; ``withdrawn_at`` / ``reproven_at``: the simulations at which the root's byte went to unknown and came back."""
    sc = prune_script()
    ids = sc.ids[0]
    ref = None if wrong is None else prune_trace()
    m = sm.SolverModel([prune_board()], [0], evaluator=lambda b, board: (sc.row(0, board.squares(), int(board.turn), 0), np.float32(0.0)), wrong=wrong)
    t = Trace()
    t.model = m
    t.leaves, t.tops, t.stats = [], [], []
    if ref is not None:
        _search(m, t, ref.reroot_at)
    else:
        while True:
            _search(m, t, 1)
            nodes = line_nodes(m, 0, ids[:2])
            if len(nodes) == 3 and nodes[2].proof:
                break
            assert len(t.leaves) < 1000
        t.proven_at = len(t.leaves) - 1
        _search(m, t, PRUNE["past"])
    t.nodes_before = sum(1 for _ in m.walk(0))
    t.tree_before = clone_tree(m.roots[0])
    t.reroot_at = len(t.leaves)
    t.reroots = []
    for j in range(2):
        m.update_with_move(0, ids[j], budget=PRUNE_BUDGET)
        t.reroots.append((ids[j], top(m, 0), stats(m), m.pruned_subtrees, sum(1 for _ in m.walk(0))))
    t.withdrawn_at = t.reproven_at = None
    while len(t.leaves) < (len(ref.leaves) if ref is not None else t.reroot_at + 300):
        before = m.roots[0].proof
        _search(m, t, 1)
        after = m.roots[0].proof
        if before and not after and t.withdrawn_at is None:
            t.withdrawn_at = len(t.leaves) - 1
        if after and not before and t.reproven_at is None:
            t.reproven_at = len(t.leaves) - 1
            if ref is None:
                _search(m, t, PRUNE["past"])
                break
    t.nodes_after = sum(1 for _ in m.walk(0))
    return t
