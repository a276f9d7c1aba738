"""CPU model of the MCTS-solver (ccz_set_solver, include/cczero.h): one proof byte per tree node, proved from
terminal leaves upwards, and a descent that stops at a proven node.

Plain Python + NumPy, one sequential MCTS per board. The rules come from ``oracle.OracleBoard``, priors and values from the harness's
``make_evaluator("hash", salts)`` (through tests/explore_model.py, whose tree node and float32 backup this model reuses). What the
model restates itself is the reference's selection arithmetic (float32 ``c_puct * P``, float64 score, first maximum) and the four
solver rules: combine, backup, expansion, selection -- and the re-root. tests/test_cpu_solver_model.py pins the model to
``oracle.OracleMCTS`` with the solver off and certifies its proofs with an exhaustive negamax; tests/test_gpu_solver.py compares the
engine with the model, exactly. tests/test_cpu_solver_deep.py and tests/test_gpu_solver_deep.py do the same for proof walks of 64 and
more plies (scripted priors) and for a re-root that prunes (``prune_copy``, the budgeted breadth-first copy of ``k_finish_move``).

``wrong=`` names a mis-stated rule so that a test can show that its fixtures tell the difference; the model itself never does.

A proof byte: bits 0..1 the state in the view of the side to move at the node (0 unknown, WIN, LOSS, DRAW), bits 2..7 the distance
to the end in plies, saturating at 63 (0 for a draw)."""
from __future__ import annotations

import numpy as np

from explore_model import F32, INF, Node, backup, evaluate

UNKNOWN, WIN, LOSS, DRAW = 0, 1, 2, 3
LEAF_EXPAND, LEAF_DRAW, LEAF_LOSS, LEAF_WIN = 0, 1, 2, 4
DIST_MAX = 63


def pack(state, dist=0):
    return int(state) | (min(int(dist), DIST_MAX) << 2)


def state_of(byte):
    return int(byte) & 3


def dist_of(byte):
    return int(byte) >> 2


def combine(children):
    """The byte of a node from its children's bytes, in this order: a LOSS child -> WIN in 1 + the smallest such distance; else an
    unknown child -> unknown; else a DRAW child -> DRAW; else every child is WIN -> LOSS in 1 + the largest distance. No children:
    unknown (the rule is never asked about such a node)."""
    children = [int(c) for c in children]
    if not children:
        return 0
    losses = [dist_of(c) for c in children if state_of(c) == LOSS]
    if losses:
        return pack(WIN, 1 + min(losses))
    if any(state_of(c) == UNKNOWN for c in children):
        return 0
    if any(state_of(c) == DRAW for c in children):
        return pack(DRAW)
    return pack(LOSS, 1 + max(dist_of(c) for c in children))


def negamax(board, depth):
    """Exhaustive, depth-limited: the exact byte of ``board``'s position if it is decided within ``depth`` plies, else 0. A distance
    it returns is the true one: a LOSS child it cannot see within depth - 1 plies is further away than every one it sees."""
    ids = board.legal_ids()
    if board.is_tie():
        return pack(DRAW)
    if not ids:
        return pack(LOSS, 0)
    if depth == 0:
        return 0
    kids = []
    for i in ids:
        c = board.copy()
        c.push_id(i)
        kids.append(negamax(c, depth - 1))
    return combine(kids)


def certify(board, max_depth=5):
    """The byte of the position by iterative deepening (the first depth that decides it; 0: not decided within ``max_depth``)."""
    for d in range(max_depth + 1):
        r = negamax(board, d)
        if r:
            return r
    return 0


class SNode(Node):
    __slots__ = ("proof",)

    def __init__(self, prior, move):
        super().__init__(prior, move)
        self.proof = 0


WRONG_WALKS = ("deep_not_written", "stop_at_63", "no_substitution")
WRONG_PRUNES = ("prune_zeroes_byte", "root_not_recombined")


def prune_copy(root, budget, wrong=None):
    """The re-root's copy of the subtree under ``root`` into a pool that may hold ``budget`` nodes (``k_finish_move``), in place:
    breadth-first, in batches of 64 nodes of that order. Within a batch a node keeps its children while
    n_new + inclusive_sum(nc) <= budget -- n_new: the nodes placed when the batch starts, the sum: over the batch in order, the
    children that end up dropped included. A node that fails becomes a leaf again and keeps N, Q, P and its proof byte.
    Returns (nodes kept, [(node, n_new, inclusive sum) of every node that lost its children])."""
    order, head, n_new, dropped = [root], 0, 1, []
    while head < n_new:
        batch = order[head:head + 64]
        incl = total = 0
        for node in batch:
            nc = len(node.kids or [])
            incl += nc
            if nc and n_new + incl <= budget:
                order.extend(node.kids)
                total = incl
            elif nc:
                dropped.append((node, n_new, incl))
                node.kids = None
                if wrong == "prune_zeroes_byte":
                    node.proof = 0
        head += len(batch)
        n_new += total
    assert n_new == len(order)
    return n_new, dropped


class SolverModel:
    """B boards, each a sequential search; ``solver`` on or off for all of them."""

    def __init__(self, boards, salts, c_puct=5, solver=True, evaluator=None, wrong=None):
        """``evaluator(b, board) -> (P float32 [2086], v float32)``: where the priors of an expanded leaf come from (default: the
        harness's ``hash`` evaluator under ``salts[b]``; the GPU test's compact paths pass the priors as the device's softmax forms
        them)."""
        self.B = len(boards)
        self.boards = [b.copy() for b in boards]
        self.salts = tuple(salts)
        self.c_puct = c_puct
        self.solver = bool(solver)
        self.evaluator = evaluator if evaluator is not None else (lambda b, board: evaluate(self.salts, b, board))
        self.roots = [SNode(1.0, -1) for _ in range(self.B)]
        self.nodes_proven = 0          # bytes that left "unknown"
        self.proven_stops = 0          # simulations whose descent ended at a node proven earlier
        self.rows = 0                  # leaves that asked for the evaluator (status EXPAND)
        self.sims = 0
        self.pruned_subtrees = 0       # nodes that lost their children in a re-root (stats()["pruned_subtrees"] of the engine)
        assert wrong is None or wrong in WRONG_WALKS + WRONG_PRUNES
        self.wrong = wrong

    # -------------------------------------------------------------------------------------------------------- one simulation
    def _select_child(self, node):
        kids = node.kids
        N = np.array([c.N for c in kids], np.int64)
        Q = np.array([c.Q for c in kids], F32)
        P = np.array([c.P for c in kids], F32)
        u = (F32(self.c_puct) * P).astype(np.float64)                       # float32 product
        sc = Q.astype(np.float64) + u * np.sqrt(np.float64(node.N)) / (1 + N).astype(np.float64)
        sc[N == 0] = INF
        return int(np.argmax(sc))                                           # first maximum

    def simulate(self, b):
        """One playout of board b. Returns (status, k, depth) of its leaf as the engine reports them."""
        node, path, moves = self.roots[b], [self.roots[b]], []
        stopped = 0
        while node.kids:
            node = node.kids[self._select_child(node)]
            path.append(node)
            moves.append(node.move)
            if self.solver and state_of(node.proof):                        # never the root: it is path[0]
                stopped = state_of(node.proof)
                break
        depth = len(path) - 1
        if stopped:
            status = {WIN: LEAF_WIN, LOSS: LEAF_LOSS, DRAW: LEAF_DRAW}[stopped]
            k = 0
            v = {WIN: F32(1.0), LOSS: F32(-1.0), DRAW: F32(0.0)}[stopped]
        else:
            board = self.boards[b].copy()
            for mv in moves:
                board.push_id(mv)
            ids = board.legal_ids()
            end, tie = board.is_game_over(), board.is_tie()
            k = len(ids)
            if not end and not tie:
                status = LEAF_EXPAND
                P, v = self.evaluator(b, board)
                node.kids = [SNode(P[i], i) for i in ids]                    # (new children are unknown)
                self.rows += 1
            else:
                status = LEAF_DRAW if (end and tie) else LEAF_LOSS
                v = F32(0.0) if status == LEAF_DRAW else F32(-1.0)
        backup(path, v)
        self.sims += 1
        if self.solver and status != LEAF_EXPAND:
            self._prove(path, status, stopped)
        return status, k, depth

    def _prove(self, path, status, stopped):
        """The leaf's byte, then parent <- combine(children) from the leaf's parent up to the root until a byte does not change. The
        child just rewritten enters its parent's combine as the new byte (the engine carries it in registers)."""
        w, d, leaf = self.wrong, len(path) - 1, path[-1]
        child_old = cur = leaf.proof
        if stopped:
            self.proven_stops += 1
        elif status == LEAF_WIN:
            return
        else:
            cur = pack(DRAW) if status == LEAF_DRAW else pack(LOSS, 0)
            if not (w == "deep_not_written" and d >= 64):
                leaf.proof = cur
            self.nodes_proven += 1
        child = leaf
        for j in range(d - 1, -1, -1):
            node = path[j]
            if (w == "stop_at_63" and j == 63) or (w == "root_not_recombined" and j == 0):
                break
            sub = child_old if w == "no_substitution" else cur
            new = combine([sub if c is child else c.proof for c in node.kids])
            if new == node.proof:
                break
            if state_of(node.proof) == UNKNOWN and state_of(new) != UNKNOWN:
                self.nodes_proven += 1
            child_old = node.proof
            if not (w == "deep_not_written" and j >= 64):
                node.proof = new
            cur, child = new, node

    def search(self, sims):
        """sims[b] (or the same int for all) playouts per board; returns the per-board lists of (status, k, depth)."""
        out = []
        for b in range(self.B):
            n = int(sims) if np.isscalar(sims) else int(sims[b])
            out.append([self.simulate(b) for _ in range(n)])
        return out

    # -------------------------------------------------------------------------------------------------------- inspection
    def root_children(self, b):
        kids = self.roots[b].kids or []
        return (np.array([c.move for c in kids], np.int32), np.array([c.N for c in kids], np.int32), np.array([c.Q for c in kids], F32),
                np.array([c.P for c in kids], F32))

    def root_proof(self, b):
        """(state, dist, child_state [k], child_dist [k]); zeros while the solver is off."""
        root = self.roots[b]
        kids = root.kids or []
        if not self.solver:
            return 0, 0, np.zeros(len(kids), np.uint8), np.zeros(len(kids), np.uint8)
        return (state_of(root.proof), dist_of(root.proof), np.array([state_of(c.proof) for c in kids], np.uint8),
                np.array([dist_of(c.proof) for c in kids], np.uint8))

    def roots_proven(self):
        return sum(1 for r in self.roots if self.solver and state_of(r.proof))

    def stats(self):
        return {"nodes_proven": self.nodes_proven, "proven_stops": self.proven_stops, "roots_proven": self.roots_proven()}

    def proof_move(self, b):
        """What chinesechesszero_amd.engine.proof_move returns for board b, restated: WIN root -> the first LOSS child of the smallest
        distance, LOSS root -> the first WIN child of the largest distance, else None."""
        st, _, cs, cd = self.root_proof(b)
        acts = self.root_children(b)[0]
        want = {WIN: LOSS, LOSS: WIN}.get(st)
        best = None
        for i in range(len(acts)):
            if want is not None and cs[i] == want:
                if best is None or (cd[i] < cd[best] if st == WIN else cd[i] > cd[best]):
                    best = i
        return None if best is None else int(acts[best])

    # -------------------------------------------------------------------------------------------------------- the move boundary
    def update_with_move(self, b, move, keep_tree=True, budget=None):
        """MCTS.update_with_move: re-root on the child that plays ``move`` with its subtree and proof bytes; a move that is no child
        of the root, or ``keep_tree`` False: a fresh, unknown root. The move is pushed on the board. ``budget``: the nodes the kept
        subtree may use (the engine's max_nodes - reserve_nodes; None: the reference's unbounded tree), see ``prune_copy``."""
        root = self.roots[b]
        kid = next((c for c in (root.kids or []) if c.move == int(move)), None)
        self.roots[b] = kid if (keep_tree and kid is not None) else SNode(1.0, -1)
        if budget is not None and keep_tree and kid is not None:
            self.pruned_subtrees += len(prune_copy(kid, int(budget), self.wrong)[1])
        self.boards[b].push_id(int(move))

    def walk(self, b):
        """Every (node, moves from the root) of board b's tree."""
        stack = [(self.roots[b], [])]
        while stack:
            node, mv = stack.pop()
            yield node, mv
            for c in node.kids or []:
                stack.append((c, mv + [c.move]))
