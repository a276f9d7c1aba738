"""CPU: the fixtures of tests/solver_deep_cases.py do what tests/test_gpu_solver_deep.py relies on. Model and oracle only.

A. The deep line is legal and quiet, the model's first decided leaf lies at depth d = 63, 64, 65, 67, that simulation proves exactly
   four bytes (negamax agrees), later simulations stop at depth d - 3 -- for d = 67 at depth 64, a byte no lane holds -- and three
   mis-stated walks give other bytes or counters. The sixty-move board ends in a DRAW leaf at depth 66.
B. ``solver_model.prune_copy`` keeps what ``k_finish_move`` keeps; on ``PRUNE`` the model shows a proven node that loses its
   children, becomes the root, has its byte withdrawn by the first DRAW child and proven again; two mis-stated prunes differ."""
import numpy as np
import pytest

import solver_deep_cases as dc
import solver_model as sm

W, L, D = sm.WIN, sm.LOSS, sm.DRAW
FOUR = range(4)                      # the boards whose line ends in the mate


def _line_boards(b):
    """The oracle boards along board b's line: [root, after move 0, ...]; asserts that every move is legal where it is played."""
    board = dc.boards()[b]
    out = [board.copy()]
    for uci in dc.line_uci(dc.CASES[b][1], dc.CASES[b][2]):
        assert uci in board.legal_moves, (dc.NAMES[b], len(out) - 1, uci)
        board.push(uci)
        out.append(board.copy())
    return out


# ---------------------------------------------------------------------------------------------------------------- A: the fixture
@pytest.mark.parametrize("b", FOUR, ids=dc.NAMES[:4])
def test_line_is_legal_quiet_and_ends_in_the_mate(b):
    _, d, turn, half = dc.CASES[b]
    line = _line_boards(b)
    assert len(line) == d + 1 and 1 + d <= 128                                   # the history chain holds the root and d positions
    assert sum(int((x.squares() != 0).sum()) for x in (line[0], line[-1])) == 2 * 7     # no capture
    assert all(x.halfmove == half + j < 70 for j, x in enumerate(line))
    assert not any(x.is_tie() or x.is_game_over() for x in line[:-1])            # (no fourfold repetition, nothing ends early)
    assert not line[-1].legal_ids() and not line[-1].is_tie() and line[-1].in_check()
    assert line[d - 2].legal_moves == ["e8e9"]                                   # the check has one answer
    # no child of a line node up to depth d - 3 is decided: a descent along the line cannot stop early
    for j in range(d - 2):
        for i in line[j].legal_ids():
            c = line[j].copy()
            c.push_id(i)
            assert c.legal_ids() and not c.is_tie(), (dc.NAMES[b], j, i)
    # depth d - 4 has other moves than the line's: it stays unknown when d - 3 is proven won
    assert len(line[d - 4].legal_ids()) > 1


@pytest.mark.parametrize("b", FOUR, ids=dc.NAMES[:4])
def test_negamax_certifies_the_four_bytes(b):
    d = dc.DEPTHS[b]
    line = _line_boards(b)
    for j, want in ((d, sm.pack(L, 0)), (d - 1, sm.pack(W, 1)), (d - 2, sm.pack(L, 2)), (d - 3, sm.pack(W, 3))):
        assert sm.negamax(line[j], d - j) == want, (dc.NAMES[b], j)


def test_first_decided_leaf_is_the_deep_mate_and_proves_four_bytes():
    t = dc.deep_trace()
    assert t.first[:4] == [1364, 1366, 1406, 1454] and min(t.first) >= dc.FORK
    assert len(t.leaves) == max(t.first) + 1 + dc.PAST
    for b in FOUR:
        d, i = dc.DEPTHS[b], t.first[b]
        assert t.leaves[i][b] == (sm.LEAF_LOSS, 0, d), dc.NAMES[b]
        got = [p for _, _, p, _ in t.line[b]]
        assert len(got) == d + 1                                                 # the tree holds the whole line
        assert got[d - 3:] == [sm.pack(W, 3), sm.pack(L, 2), sm.pack(W, 1), sm.pack(L, 0)] and not any(got[:d - 3]), dc.NAMES[b]
        # the next simulations are stops at the node proven won in 3 (some 50 of them: then black's Q there has sunk below its
        # other moves', and it leaves the line one ply earlier: expansions below lane 60 with proven bytes in the tree)
        assert all(row[b] == (sm.LEAF_WIN, 0, d - 3) for row in t.leaves[i + 1:i + 1 + dc.PAST]), dc.NAMES[b]
    assert max(t.nodes) <= dc.MAX_NODES - dc.RESERVE_NODES and max(dc.DEPTHS) + 1 <= dc.MAX_DEPTH       # the pool and the path hold every tree
    # d = 67: the stopped descent's byte is path node 64's, which no lane holds
    assert sum(1 for row in t.leaves if row[3] == (sm.LEAF_WIN, 0, 64)) >= dc.PAST
    # the counters: 4 bytes per mate board, 2 on the sixty-move board; every decided leaf but each board's first is a stop
    assert t.stats[-1]["nodes_proven"] == 4 * 4 + 2 and t.stats[-1]["roots_proven"] == 0
    assert t.stats[-1]["proven_stops"] == sum(1 for row in t.leaves for x in row if x[0] != sm.LEAF_EXPAND) - dc.B > 5 * dc.PAST


def test_sixty_move_board_ends_in_a_draw_leaf_inside_the_deep_branch():
    """Root halfmove 54: the position after 66 plies has halfmove 120. Its leaf is DRAW; depth 65 (black, in check, one reply) has
    that single child and is DRAW too; depth 64 (red) has other, unknown children and stays unknown: the walk rewrites one node
    through ``path[]`` and ends at the next, before any lane-held node."""
    t, b = dc.deep_trace(), 4
    line = _line_boards(b)
    assert line[66].halfmove == 120 and line[66].is_tie() and line[66].legal_ids() and not line[65].is_tie()
    assert t.leaves[t.first[b]][b] == (sm.LEAF_DRAW, len(line[66].legal_ids()), 66)
    got = [p for _, _, p, _ in t.line[b]]
    assert len(got) == 67 and got[64:] == [0, sm.pack(D), sm.pack(D)] and not any(got[:64])
    assert sm.negamax(line[65], 1) == sm.pack(D) and sm.negamax(line[66], 0) == sm.pack(D) and sm.negamax(line[64], 2) == 0
    # afterwards the descent stops at the DRAW node of depth 65
    assert all(row[b] == (sm.LEAF_DRAW, 0, 65) for row in t.leaves[t.first[b] + 1:])


def test_walk_by_re_roots_shows_every_deep_node():
    """The forced moves make every line node the root in turn: its N, Q and byte are what the search left there."""
    t = dc.deep_trace()
    for b in range(dc.B):
        for s, tops in enumerate(t.walk_tops):
            if s + 1 >= len(t.line[b]) or (s > 0 and t.over[s - 1][b]):
                continue
            n, q, p, k = t.line[b][s + 1]
            top = tops[b]
            assert top["root_n"] == n and top["proof"] == (sm.state_of(p), sm.dist_of(p)) and len(top["acts"]) == k, (dc.NAMES[b], s)
        ends = [s for s in range(len(t.over)) if t.over[s][b]]
        assert ends[0] == (dc.DEPTHS[b] if b < 4 else 66) - 1, dc.NAMES[b]
    assert t.walk_stats[-1]["roots_proven"] == 0                               # every game is over in the end


@pytest.mark.parametrize("wrong", sm.WRONG_WALKS)
def test_mis_stated_walks_are_told_apart(wrong):
    t, w = dc.deep_trace(), dc.wrong_deep_trace(wrong)
    differs = [b for b in FOUR if [p for *_, p, _ in w.line[b]] != [p for *_, p, _ in t.line[b]]
               or [r[b] for r in w.leaves] != [r[b] for r in t.leaves]]
    assert differs and w.stats[-1] != t.stats[-1], wrong
    same = [b for b in FOUR if b not in differs]
    if wrong in ("deep_not_written", "stop_at_63"):                            # the all-lanes control cannot tell
        assert 0 in same
    if wrong == "deep_not_written":                                           # d = 64: only the leaf is that deep, and nothing reads it again
        assert [r[1] for r in w.leaves] == [r[1] for r in t.leaves] and [p for *_, p, _ in w.line[1]][-1] == 0
    if wrong == "stop_at_63":                                                 # d = 67 proves its four bytes at depths 64..67 and ends at 63 by itself
        assert differs == [1, 2]
    else:
        assert 2 in differs and 3 in differs


def test_solver_off_is_the_oracles_search_on_the_d65_board():
    from oracle import OracleMCTS
    sc, b = dc.script(), 2
    t = dc.deep_trace(solver=False, only=b)
    board = dc.boards()[b]
    o = OracleMCTS(None, c_puct=5, n_playout=0)
    for i in range(len(t.leaves)):
        leaf, depth = o.select(board)
        ids = leaf.legal_ids()
        end, tie = leaf.is_game_over(), leaf.is_tie()
        status = sm.LEAF_EXPAND if (not end and not tie) else (sm.LEAF_DRAW if (end and tie) else sm.LEAF_LOSS)
        assert t.leaves[i][0] == (status, len(ids), depth), i
        o.expand_backup(leaf, ids, sc.row(b, leaf.squares(), int(leaf.turn), depth)[ids], 0.0)
    acts, N, Q, P = o.root_children()
    top = t.tops[-1][0]
    assert np.array_equal(top["acts"], acts) and np.array_equal(top["N"], N)
    assert np.array_equal(top["Q"].view(np.uint32), Q.view(np.uint32)) and np.array_equal(top["P"].view(np.uint32), P.view(np.uint32))
    assert sum(1 for r in t.leaves if r[0][0] == sm.LEAF_LOSS and r[0][2] == 65) > 1       # without the solver the mate is walked into again
    assert all(node.proof == 0 for node in _walk(t.roots[0]))


def _walk(root):
    stack = [root]
    while stack:
        n = stack.pop()
        yield n
        stack.extend(n.kids or [])


# ---------------------------------------------------------------------------------------------------------------- B: the pruning copy
def _bfs(root):
    order, i = [root], 0
    while i < len(order):
        order.extend(order[i].kids or [])
        i += 1
    return order


def _tree_for_pruning():
    t = dc.prune_trace()
    root = dc.clone_tree(t.tree_before)
    return next(c for c in root.kids if c.move == dc.prune_script().ids[0][0])


def test_prune_copy_with_room_is_the_identity():
    root = _tree_for_pruning()
    before = [(n.move, n.N, n.proof, len(n.kids or [])) for n in _bfs(root)]
    for budget in (len(before), len(before) + 1, 1 << 20):
        kept, dropped = sm.prune_copy(root, budget)
        assert kept == len(before) and not dropped
        assert [(n.move, n.N, n.proof, len(n.kids or [])) for n in _bfs(root)] == before


@pytest.mark.parametrize("budget", [129, 130, 160, 200, 257, 300, 398])
def test_prune_copy_keeps_within_the_budget_and_drops_with_cause(budget):
    root = _tree_for_pruning()
    full = _bfs(root)
    had = {id(n): len(n.kids or []) for n in full}
    record = {id(n): (n.N, n.Q, n.P, n.proof, n.move) for n in full}
    assert len(full) > budget
    kept, dropped = sm.prune_copy(root, budget)
    after = _bfs(root)
    assert kept == len(after) <= budget
    assert dropped and all(had[id(n)] > 0 and n.kids is None for n, _, _ in dropped)                 # only nodes with children lose them
    lost = {id(n) for n, _, _ in dropped}
    for n in after:
        assert (n.N, n.Q, n.P, n.proof, n.move) == record[id(n)]                                      # N, Q, P and the byte stay
        assert len(n.kids or []) == (0 if id(n) in lost else had[id(n)])                              # nobody else lost anything
    # the cause, restated over the copy's order: batches of 64 in breadth-first order of the KEPT tree; a node is dropped exactly
    # if the nodes placed before its batch plus the children of the batch up to and including it exceed the budget
    placed, head = 1, 0
    while head < len(after):
        batch = after[head:head + 64]
        incl = 0
        for n in batch:
            incl += had[id(n)]
            if had[id(n)]:
                assert (id(n) in lost) == (placed + incl > budget)
        placed += sum(had[id(n)] for n in batch if id(n) not in lost)
        head += len(batch)
    assert placed == kept


def test_prune_fixture_is_what_the_issue_asks_for():
    """N: red to move at halfmove 119, WIN in 3 by its only capture, which gives check and has one answer; every quiet move ends the
    game in a draw; no move mates at once."""
    root = dc.prune_board()
    line = dc.PRUNE["line"]
    assert root.halfmove == 117 and root.turn
    P1 = root.copy()
    P1.push(line[0])
    assert P1.legal_moves[-1] == line[1] and len(P1.legal_moves) == 9                  # N is the last of its siblings
    N = P1.copy()
    N.push(line[1])
    assert N.halfmove == 119 and N.turn and not N.is_tie()
    assert sm.certify(N, 3) == sm.pack(W, 3)
    captures = 0
    for uci, i in zip(N.legal_moves, N.legal_ids()):
        c = N.copy()
        c.push_id(i)
        if uci == line[2]:
            captures += 1
            assert c.halfmove == 0 and c.in_check() and c.legal_moves == [line[3]] and sm.negamax(c, 2) == sm.pack(L, 2)
        else:
            assert c.halfmove == 120 and c.is_tie() and c.legal_ids()              # quiet: a DRAW leaf, not a mate or stalemate
    assert captures == 1
    # N's earlier siblings are all expanded by one visit each and fill the budget on their own
    kids = []
    for i in P1.legal_ids()[:-1]:
        c = P1.copy()
        c.push_id(i)
        assert c.legal_ids() and not c.is_tie()
        kids.append(len(c.legal_ids()))
    assert 1 + 9 + sum(kids) > dc.PRUNE_BUDGET >= 129 > 1 + 9


def _certified(board, moves, byte):
    b = board.copy()
    for mv in moves:
        b.push_id(mv)
    exact = sm.certify(b, 3)
    return exact != 0 and sm.state_of(exact) == sm.state_of(byte) and (sm.state_of(byte) == D or sm.dist_of(byte) >= sm.dist_of(exact))


def test_model_withdraws_and_re_proves_the_pruned_root():
    t = dc.prune_trace()
    ids = dc.prune_script().ids[0]
    assert t.nodes_before < dc.PRUNE["max_nodes"] and t.nodes_after + 129 < dc.PRUNE["max_nodes"]
    (_, top1, st1, pruned1, kept1), (_, top2, st2, pruned2, kept2) = t.reroots
    # re-root 1: N is the last root child, WIN in 3; six of the nine siblings lost their children, N among them
    assert kept1 <= dc.PRUNE_BUDGET and pruned1 == 6 and (top1["cs"][-1], top1["cd"][-1]) == (W, 3) and top1["proof"] == (0, 0)
    assert top1["N"][-1] > 40                                                    # (N had been searched: its children were real)
    # re-root 2: N is the root, proven, childless; nothing more is pruned; a WIN root without children names no move
    assert (kept2, pruned2) == (1, 6) and top2["proof"] == (W, 3) and len(top2["acts"]) == 0 and top2["pm"] == -1
    assert top2["root_n"] == top1["N"][-1] and st2["roots_proven"] == 1
    # simulation 1 expands N under its WIN byte; the first quiet child withdraws it; the capture line proves it again
    r = t.reroot_at
    assert t.leaves[r][0][0] == sm.LEAF_EXPAND and t.leaves[r][0][2] == 0 and t.tops[r][0]["proof"] == (W, 3)
    assert t.withdrawn_at == r + 1 and t.leaves[r + 1][0][0] == sm.LEAF_DRAW and t.leaves[r + 1][0][2] == 1
    assert t.tops[r + 1][0]["proof"] == (0, 0) and t.stats[r + 1]["roots_proven"] == 0
    assert t.stats[r + 1]["nodes_proven"] == t.stats[r]["nodes_proven"] + 1      # the DRAW leaf; the withdrawal proves nothing
    assert t.reproven_at is not None and t.reproven_at > t.withdrawn_at
    assert t.leaves[t.reproven_at][0] == (sm.LEAF_LOSS, 0, 3) and t.tops[t.reproven_at][0]["proof"] == (W, 3)
    assert t.tops[-1][0]["pm"] == ids[2]                                         # the capture
    # no byte anywhere in the final tree, and none at a tree top on the way, contradicts the negamax
    m = t.model
    checked = 0
    for node, moves in m.walk(0):
        if node.proof:
            assert _certified(m.boards[0], moves, node.proof), moves
            checked += 1
    assert checked > 20
    root = dc.prune_board()
    for i, tops in enumerate(t.tops):
        pre = [] if i < t.reroot_at else ids[:2]
        top = tops[0]
        if top["proof"][0]:
            assert _certified(root, pre, sm.pack(*top["proof"]))
        for a, s, d in zip(top["acts"], top["cs"], top["cd"]):
            if s:
                assert _certified(root, list(pre) + [int(a)], sm.pack(s, d)), (i, a)


def test_mis_stated_prunes_are_told_apart():
    t = dc.prune_trace()
    z = dc.prune_trace("prune_zeroes_byte")
    assert z.reroots[0][1]["cs"][-1] == 0 and z.reroots[1][1]["proof"] == (0, 0) and z.withdrawn_at is None
    assert t.reroots[0][1]["cs"][-1] == W and t.reroots[1][1]["proof"] == (W, 3)
    n = dc.prune_trace("root_not_recombined")
    assert [x[0]["proof"] for x in n.tops[n.reroot_at:]] == [(W, 3)] * (len(n.tops) - n.reroot_at)     # stale, and true here
    assert n.leaves == t.leaves and n.withdrawn_at is None
    assert n.stats[-1]["nodes_proven"] == t.stats[-1]["nodes_proven"] - 1
