"""CPU: the model of the MCTS-solver (tests/solver_model.py) that tests/test_gpu_solver.py compares the engine with.

1. Solver off, the model IS the reference's search: N, Q bits and P of every root child of ``oracle.OracleMCTS``.
2. Solver on, where no terminal is in reach, likewise.
3. Every fixture of tests/solver_cases.py carries the state and distance an exhaustive negamax gives it; the model proves each root
   within the fixture's budget, to that state and distance, and no byte anywhere in its trees contradicts the negamax.
4. ``combine`` on hand-written byte lists: every size at which the device function changes pass or lane, the deciding byte at the
   first and last lane of either pass, and a distance past the saturation.
5. The C ABI carries the four entry points (this one fails on a library without the feature)."""
import functools

import numpy as np
import pytest

import explore_model as em
import solver_cases as sc
import solver_model as sm
from golden_cases import STARTS
from oracle import OracleBoard, OracleMCTS

W, L, D = sm.WIN, sm.LOSS, sm.DRAW


def _oracle_children(board, salt, n):
    o = OracleMCTS(lambda brd, ids: (em.evaluate((salt,), 0, brd)[0][ids], em.evaluate((salt,), 0, brd)[1]), c_puct=5, n_playout=0)
    board = board.copy()
    for _ in range(n):
        o.playout(board)
    return o.root_children(), o.root_visits()


def _same_children(got, exp):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert np.array_equal(got[2].view(np.uint32), exp[2].view(np.uint32))       # Q bits
    assert np.array_equal(got[3].view(np.uint32), exp[3].view(np.uint32))       # priors


@pytest.mark.parametrize("name", ["two_rooks", "rook_knight", "start"])
def test_model_with_the_solver_off_is_the_oracles_search(name):
    board = OracleBoard() if name == "start" else OracleBoard.from_array(STARTS[name], 1)
    m = sm.SolverModel([board], [31], solver=False)
    m.search(200)
    exp, n = _oracle_children(board, 31, 200)
    _same_children(m.root_children(0), exp)
    assert m.roots[0].N == n == 200
    assert m.stats() == {"nodes_proven": 0, "proven_stops": 0, "roots_proven": 0}
    assert all(node.proof == 0 for node, _ in m.walk(0))


def test_model_with_the_solver_on_is_the_oracles_search_where_nothing_ends():
    board = OracleBoard()
    m = sm.SolverModel([board], [31], solver=True)
    leaves = m.search(64)[0]
    exp, _ = _oracle_children(board, 31, 64)
    _same_children(m.root_children(0), exp)
    assert all(st == sm.LEAF_EXPAND for st, _, _ in leaves) and m.rows == 64
    assert m.stats() == {"nodes_proven": 0, "proven_stops": 0, "roots_proven": 0}


# ---------------------------------------------------------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def _searched():
    """The model after SIMS simulations of every fixture, and the simulation at which each root was proven (None: never)."""
    m = sm.SolverModel(sc.boards(), sc.SALTS)
    proven_at = [None] * m.B
    for b in range(m.B):
        for i in range(sc.SIMS):
            m.simulate(b)
            if proven_at[b] is None and sm.state_of(m.roots[b].proof):
                proven_at[b] = i + 1
    return m, proven_at


@pytest.mark.parametrize("b", range(len(sc.CASES)), ids=sc.NAMES)
def test_fixture_is_certified_by_negamax(b):
    name, sq, turn, state, dist, *_ = sc.CASES[b]
    got = sm.certify(OracleBoard.from_array(sq, turn), 5)
    assert (sm.state_of(got), sm.dist_of(got)) == (state, dist)


def test_fixtures_cover_the_results():
    kinds = {(c[3], c[4]) for c in sc.CASES}
    assert {(W, 1), (W, 3), (L, 2), (D, 0), (0, 0)} <= kinds
    two = OracleBoard.from_array(STARTS["two_rooks"], 1)
    two.push("a7a9")
    assert not two.legal_ids() and not two.is_tie()                             # Ra7-a9 is mate
    for root, below, mv in (("one_move", "mated", "a2a0"), ("one_move_black", "mated_black", "a7a9")):
        case = sc.CASES[sc.NAMES.index("mated_below" if below == "mated" else "mated_black_below")]
        b = OracleBoard.from_array(case[1], case[2])
        b.push(mv)
        assert np.array_equal(b.squares(), STARTS[below]) and not b.legal_ids()   # the mated position is one ply below the root
    assert len(OracleBoard.from_array(*sc.CASES[sc.NAMES.index("mated_in_two_plies")][1:3]).legal_ids()) > 1


@pytest.mark.parametrize("b", range(len(sc.CASES)), ids=sc.NAMES)
def test_model_proves_the_fixture_within_its_budget(b):
    name, sq, turn, state, dist, salt, budget, move = sc.CASES[b]
    m, proven_at = _searched()
    st, ds, cs, cd = m.root_proof(b)
    assert (st, ds) == (state, dist)
    if state:
        assert proven_at[b] is not None and proven_at[b] <= budget
    else:
        assert proven_at[b] is None
    pm = m.proof_move(b)
    root = OracleBoard.from_array(sq, turn)
    assert (None if pm is None else root.legal_moves[root.legal_ids().index(pm)]) == move
    assert int(m.root_children(b)[1].sum()) == m.roots[b].N - 1 == sc.SIMS - 1          # a proven root keeps descending


def test_no_proof_contradicts_the_negamax():
    m, _ = _searched()
    checked = 0
    for b in range(m.B):
        for node, moves in m.walk(b):
            if not node.proof or len(moves) > 4:
                continue
            board = m.boards[b].copy()
            for mv in moves:
                board.push_id(mv)
            exact = sm.certify(board, 3)
            if exact:
                checked += 1
                assert sm.state_of(node.proof) == sm.state_of(exact), (sc.NAMES[b], moves)
                if sm.state_of(exact) != D:       # the tree has seen a subset of the lines: its distance is an upper bound
                    assert sm.dist_of(node.proof) >= sm.dist_of(exact), (sc.NAMES[b], moves)
    assert checked >= m.nodes_proven // 2 > 0
    assert m.proven_stops > 0 and m.rows < m.sims


def test_re_root_keeps_the_proof_and_a_fresh_root_has_none():
    m = sm.SolverModel(sc.boards()[:1], sc.SALTS[:1])
    m.search(sc.SIMS)
    acts = m.root_children(0)[0]
    mv = m.proof_move(0)
    child = m.root_proof(0)[2][list(acts).index(mv)], m.root_proof(0)[3][list(acts).index(mv)]
    m.update_with_move(0, mv)
    assert m.root_proof(0)[:2] == (L, 0) == child
    m2 = sm.SolverModel(sc.boards()[:1], sc.SALTS[:1])
    m2.search(sc.SIMS)
    m2.update_with_move(0, mv, keep_tree=False)
    assert m2.root_proof(0)[:2] == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- combine
def combine_cases():
    """(children bytes, expected byte): the list tests/test_gpu_solver.py hands ccz_proof_combine as well."""
    out = []
    u, w1, d0 = 0, sm.pack(W, 1), sm.pack(D)
    for nc in (1, 63, 64, 65, 128):
        for pos in sorted({p for p in (0, 63, 64, nc - 1) if p < nc}):
            def lst(fill, at):
                x = [fill] * nc
                x[pos] = at
                return x
            out.append((lst(w1, sm.pack(L, 4)), sm.pack(W, 5)))                 # the single LOSS among WINs
            out.append((lst(u, sm.pack(L, 0)), sm.pack(W, 1)))                  # ... among unknowns: a LOSS child decides first
            out.append((lst(w1, u), 0))                                           # the single unknown
            out.append((lst(w1, d0), d0))                                        # the single DRAW
            out.append((lst(w1, sm.pack(W, 9)), sm.pack(L, 10)))                # the maximum distance
            out.append((lst(sm.pack(L, 7), sm.pack(L, 2)), sm.pack(W, 3)))      # the minimum distance
            out.append((lst(d0, u), 0))                                          # unknown beats DRAW
    out.append(([sm.pack(W, 63), sm.pack(W, 62)], sm.pack(L, 63)))              # past the saturation
    out.append(([sm.pack(L, 63)] * 65, sm.pack(W, 63)))
    out.append(([sm.pack(W, 62)] * 128, sm.pack(L, 63)))
    return out


def test_combine_on_hand_written_lists():
    cases = combine_cases()
    assert {len(c) for c, _ in cases} >= {1, 63, 64, 65, 128}
    for kids, want in cases:
        assert sm.combine(kids) == want, (len(kids), kids[:4], want)
    assert sm.combine([]) == 0
    assert sm.pack(W, 200) == sm.pack(W, 63) and sm.dist_of(sm.pack(D)) == 0


def test_proof_move_helper():
    from chinesechesszero_amd.engine import mate_score, proof_move
    acts = np.array([10, 20, 30, 40], np.uint16)
    assert proof_move(W, 3, [W, L, L, 0], [1, 4, 2, 0], acts) == 30           # the fastest mate
    assert proof_move(W, 3, [L, L, L, 0], [2, 2, 2, 0], acts) == 10           # first in insertion order on ties
    assert proof_move(L, 4, [W, W, W, W], [1, 3, 3, 1], acts) == 20           # the longest defence, first on ties
    assert proof_move(D, 0, [D, W, W, W], [0, 1, 1, 1], acts) is None
    assert proof_move(0, 0, [0, 0, 0, 0], [0, 0, 0, 0], acts) is None
    assert mate_score(L, 0) == 1 and mate_score(L, 2) == 2 and mate_score(W, 1) == -1 and mate_score(W, 3) == -2
    assert mate_score(D, 0) is None and mate_score(0, 0) is None


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_has_the_solver_entry_points():
    from chinesechesszero_amd import _lib
    lib = _lib.lib()
    for name in ("ccz_set_solver", "ccz_root_proof", "ccz_get_solver_stats", "ccz_proof_combine"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
    assert lib.ccz_abi_version() == 9 == _lib.ABI_VERSION
    assert _lib.LEAF_WIN == 4


# ---------------------------------------------------------------------------------------------------------------- front-ends, host side
def test_uci_takes_the_solver_option():
    import io
    from chinesechesszero_amd.uci import UciLoop
    out = io.StringIO()
    loop = UciLoop(policy_value_fn=lambda *a: None, out=out)
    loop.handle("uci")
    assert "option name Solver type check default false" in out.getvalue().splitlines() and loop.solver is False
    loop.handle("setoption name Solver value true")
    assert loop.solver is True
    loop.handle("setoption name Solver value false")
    assert loop.solver is False


def test_analysis_records_gain_mate_only_with_the_solver():
    from chinesechesszero_amd.analyse import make_record
    lines = [{"moves": ["a7a9", "e9f9"], "visits": [9, 1], "q": 0.5, "prior": 0.1}, {"moves": ["b8b9"], "visits": [2], "q": 0.1, "prior": 0.2}]
    plain = make_record("ok", 12, lines)
    assert "mate" not in plain and "mate" not in plain["lines"][0] and plain["bestmove"] == "a7a9"
    rec = make_record("ok", 12, lines, solver={"proven": "b8b9", "mates": {"a7a9": None, "b8b9": 2}})
    assert rec["bestmove"] == "b8b9" and rec["mate"] == 2 and [l["mate"] for l in rec["lines"]] == [None, 2]
    rec = make_record("ok", 12, lines, solver={"proven": None, "mates": {"a7a9": -1}})
    assert rec["bestmove"] == "a7a9" and rec["mate"] == -1 and rec["lines"][1]["mate"] is None
    assert {k: v for k, v in rec.items() if k != "mate"}["status"] == "ok"
