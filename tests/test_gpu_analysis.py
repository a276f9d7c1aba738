"""GPU: batched position analysis -- ccz_set_positions (many boards with their move history in one launch), parked boards,
ccz_principal_variations against the oracle's tree, BatchedAnalysis end to end, MultiPV in the UCI loop. Every comparison is
exact: move ids, visit counts, Q / P as uint32 bit patterns."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHUFFLE = ("h2h3 h7h6 h3h2 h6h7 " * 2 + "h2h3 h7h6 h3h2").split()   # 11 plies, no capture: h6h7 next is the start position's 4th occurrence
SHUFFLE_SALT = 5     # a salt at which the history changes the 128-simulation root visits on the CPU oracle (checked below)
MATE_CASE, MATE_MOVE = "pinned_rook_moves_along_the_pin_line_only", "e3e8"   # red mates in one


def _ids():
    import oracle
    return {u: i for i, u in enumerate(oracle.move_table())}


def _engine(B, n=128, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(B, n_playout=n, device=0, seed=1, **kw)


def _replayed(start, moves):
    from oracle import OracleBoard
    b = OracleBoard.from_array(*start)
    for m in moves:
        b.push_id(m)
    return b


def _kat_case(name):
    import rules_kat
    return next(c for c in rules_kat.cases() if c["name"] == name)


def _load_cases():
    """[(label, (squares, turn, halfmove), move ids)]: the rules_kat cases with moves, cut to the longest prefix on which the oracle
    reports neither game over nor tie before the last position; eight seeded 40-ply random legal walks; the shuffle line."""
    import rules_kat
    from oracle import OracleBoard
    ID = _ids()
    out = []
    for c in rules_kat.cases():
        if not c.get("moves"):
            continue
        start = rules_kat.start_of(c)
        b = OracleBoard.from_array(*start)
        keep = []
        for u in c["moves"]:
            if b.is_game_over() or b.is_tie():
                break
            keep.append(ID[u])
            b.push_id(ID[u])
        out.append((c["name"], start, keep))
    rs = np.random.RandomState(11)
    first = OracleBoard()
    origin = (first.squares(), 1, 0)
    for w in range(8):
        b, line = OracleBoard(), []
        while len(line) < 40:
            ids = b.legal_ids()
            assert ids and not b.is_game_over()
            line.append(ids[rs.randint(len(ids))])
            b.push_id(line[-1])
            if b.is_game_over() or b.is_tie():   # keep the walks alive: start this one again (seeded, so the set is fixed)
                b, line = OracleBoard(), []
        out.append((f"walk{w}", origin, line))
    out.append(("shuffle", origin, [ID[u] for u in SHUFFLE]))
    return out


@pytest.fixture(scope="module")
def cases():
    return _load_cases()


class _Cached:
    """make_evaluator with a memo: engine B asks for the positions engine A asked for."""

    def __init__(self, kind, salts):
        from gpu_harness import make_evaluator
        self.ev, self.memo = make_evaluator(kind, salts), {}

    def __call__(self, sq, turn):
        P = np.zeros((len(sq), 2086), np.float32)
        V = np.zeros(len(sq), np.float32)
        for b in range(len(sq)):
            key = (b, sq[b].tobytes(), int(turn[b]))
            if key not in self.memo:
                p, v = self.ev(sq[b:b + 1], turn[b:b + 1], rows=[b])
                self.memo[key] = (p[0], v[0])
            P[b], V[b] = self.memo[key]
        return P, V


def _sequential_load(e, loads):
    """The parent's way: set_position, then one forced finish_move(keep_tree=False) per ply. Boards with fewer moves are loaded
    later, so that all lines end together; until its turn comes a board idles on the shuffle from the start position (a finished
    board ignores its forced move)."""
    ID = _ids()
    idle = [ID[u] for u in "h2h3 h7h6 h3h2 h6h7".split()]
    T = max(len(m) for _, _, m in loads)
    for b, (_, start, m) in enumerate(loads):
        if len(m) == T:
            e.set_position(b, *start)
    for t in range(T):
        forced = np.zeros(e.B, np.int32)
        for b, (_, start, m) in enumerate(loads):
            first = T - len(m)
            forced[b] = m[t - first] if t >= first else idle[t % 4]
        e.finish_move(forced_moves=forced, keep_tree=False)
        for b, (_, start, m) in enumerate(loads):
            if T - len(m) == t + 1:
                e.set_position(b, *start)


def _arrays(loads):
    sq = np.stack([s[0] for _, s, _ in loads])
    turn = np.array([s[1] for _, s, _ in loads], np.uint8)
    half = np.array([s[2] for _, s, _ in loads], np.int32)
    return sq, turn, half, [m for _, _, m in loads]


def test_shuffle_history_changes_the_search_on_the_oracle():
    """The condition the loading test's inputs meet: with its history the shuffle position reaches a draw leaf and ends 128
    simulations with other root visits than the same squares without history (CPU oracle, hash_sharp evaluator)."""
    from oracle import OracleBoard, OracleMCTS
    from oracle.evaluators import hash_eval
    ID = _ids()

    def ev(board, ids):
        p, v = hash_eval(board.squares()[None], np.array([1 if board.turn else 0], np.uint8), salt=SHUFFLE_SALT, scale=40.0)
        return p[0][ids], v[0]

    first = OracleBoard()
    with_history = _replayed((first.squares(), 1, 0), [ID[u] for u in SHUFFLE])
    bare = OracleBoard.from_array(with_history.squares(), 1 if with_history.turn else 0, 0)
    visits = []
    for b in (with_history, bare):
        m = OracleMCTS(ev, n_playout=128)
        for _ in range(128):
            m.playout(b)
        visits.append(m.root_children()[1])
    assert not np.array_equal(visits[0], visits[1])


def test_loading_equals_the_sequential_path_and_the_oracle(cases):
    from gpu_harness import Lockstep, planes_to_squares
    from oracle import OracleBoard
    loads = list(cases)
    sh = next(c for c in loads if c[0] == "shuffle")
    reached = _replayed(sh[1], sh[2])
    loads.append(("shuffle_bare", (reached.squares(), 1 if reached.turn else 0, 0), []))   # the same squares, moves=None
    B = len(loads)
    salts = [SHUFFLE_SALT if name.startswith("shuffle") else 20 + b for b, (name, _, _) in enumerate(loads)]
    a, b_eng = _engine(B), _engine(B)
    sq, turn, half, moves = _arrays(loads)
    status = a.set_positions(sq, turn, half, moves)
    assert not status.any(), status
    _sequential_load(b_eng, loads)
    assert np.array_equal(a.root_positions(), b_eng.root_positions())
    sa, sb = a.game_status(), b_eng.game_status()
    for f in ("turn", "over", "winner"):
        assert np.array_equal(sa[f], sb[f]), f
    assert not sa["plies"].any()
    boards = [_replayed(s, m) for _, s, m in loads]
    for j, ob in enumerate(boards):
        assert np.array_equal(sa["over"][j] != 0, ob.is_game_over() or ob.is_tie()), loads[j][0]
        assert np.array_equal(a.root_positions()[j], ob.squares()) and sa["turn"][j] == int(ob.turn)
    assert sa["over"].sum() >= 3 and (sa["over"] == 0).sum() >= 10     # decided positions and live ones are both in the set
    ls = Lockstep(a, boards, kind="hash_sharp", salts=salts)
    ev = _Cached("hash_sharp", salts)
    ls.ev = ev
    for _ in range(128):
        ls.step(check_leaf=True)
    rc = ls.compare_roots()
    for _ in range(128):
        b_eng.select_leaves()
        s, t = planes_to_squares(b_eng.leaf_input.float().cpu().numpy())
        P, V = ev(s, t)
        b_eng.expand_backup(torch.from_numpy(P).to(b_eng.device), torch.from_numpy(V).to(b_eng.device))
    rb = b_eng.root_children()
    live = sa["over"] == 0
    for f in ("k", "acts", "visits", "root_visits"):
        assert np.array_equal(rc[f][live], rb[f][live]), f
    for f in ("q", "prior"):
        assert np.array_equal(rc[f][live].view(np.uint32), rb[f][live].view(np.uint32)), f
    i, j = B - 2, B - 1
    assert loads[i][0] == "shuffle" and live[i] and live[j]
    assert np.array_equal(rc["acts"][i], rc["acts"][j]) and not np.array_equal(rc["visits"][i], rc["visits"][j])
    a.check_healthy()
    b_eng.check_healthy()
    assert a.stats()["moves"] == 0 and a.stats()["games"] == 0          # loading is not playing


def test_no_moves_equals_set_position():
    import rules_kat
    from chinesechesszero_amd import _lib
    starts = [rules_kat.start_of(c) for c in rules_kat.cases()][:23]
    sixty = rules_kat.start_of(_kat_case("sixty_moves_not_yet_at_119"))
    step = _ids()[_kat_case("sixty_moves_not_yet_at_119")["moves"][0]]
    starts.append(sixty)
    B = len(starts)
    a, b = _engine(B, 8, mirror=False), _engine(B, 8, mirror=False)
    for e in (a, b):
        e.reset()                                  # game numbers differ from the freshly created state
    status = a.set_positions(np.stack([s[0] for s in starts]), [s[1] for s in starts], [s[2] for s in starts])
    assert not status.any()
    for j, s in enumerate(starts):
        b.set_position(j, *s)
    sa, sb = a.game_status(), b.game_status()
    for f in ("over", "winner", "plies", "turn"):
        assert np.array_equal(sa[f], sb[f]), f
    assert not sa["over"].any()                    # no moves: no game-end test, exactly as set_position
    assert np.array_equal(a.root_positions(), b.root_positions())
    for e in (a, b):
        assert e.root_children()["k"].sum() == 0 and (e.leaf_info()["status"] == _lib.LEAF_SKIP).all()
    # a board that then plays the move ending its game by the sixty-move rule: its record's header carries the game number
    heads = []
    for loader in ("set_positions", "set_position"):
        e = _engine(1, 8, mirror=False)
        e.reset()
        if loader == "set_positions":
            assert not e.set_positions(sixty[0][None], [sixty[1]], [sixty[2]]).any()
        else:
            e.set_position(0, *sixty)
        e.finish_move(forced_moves=np.array([step], np.int32), keep_tree=False)
        st = e.game_status()
        assert st["over"][0] and st["plies"][0] == 1 and st["winner"][0] == -1
        recs = list(e.harvest_record_chunks())
        assert len(recs) == 1 and recs[0].shape[0] == 1
        heads.append(recs[0][0, _lib.REC_HDR:_lib.REC_HDR + 16].cpu().numpy().copy())
        e.check_healthy()
    assert np.array_equal(heads[0], heads[1])
    assert int(heads[0][12:16].view(np.uint32)[0]) == 3      # created (1), reset (2), loaded (3)


def test_status_codes_and_parked_boards():
    import rules_kat
    from gpu_harness import Lockstep
    from oracle import OracleBoard
    from chinesechesszero_amd import _lib
    ID = _ids()
    first = OracleBoard()
    origin = (first.squares(), 1, 0)
    good = [ID[u] for u in "h2e2 h9g7".split()]
    pinned = rules_kat.start_of(_kat_case(MATE_CASE))
    ob = OracleBoard.from_array(*pinned)
    assert ID["e3d3"] not in ob.legal_ids() and ob.squares()[rules_kat.sq("e3")] == 3     # the pinned rook may not leave the file
    quiet, reply = ID["e0e1"], ID["d9d8"]            # both kings step aside: the rook on e3 stays pinned by the one on e8
    after = ob.copy()
    for m in (quiet, reply):
        assert m in after.legal_ids()
        after.push_id(m)
    assert ID["e3d3"] not in after.legal_ids() and after.squares()[rules_kat.sq("e3")] == 3 and after.squares()[rules_kat.sq("d3")] == 0
    two_kings = first.squares().copy()
    two_kings[rules_kat.sq("a3")] = 7
    long_line = [ID[u] for u in ("h2h3 h7h6 h3h2 h6h7 " * 33).split()][:130]
    walk = OracleBoard()
    for m in long_line:
        assert m in walk.legal_ids()
        walk.push_id(m)
    loads = [("good0", origin, good), ("illegal", origin, good + [ID["a0a5"]] + good), ("in_check", pinned, [quiet, reply, ID["e3d3"]]),
             ("two_kings", (two_kings, 1, 0), []), ("long", origin, long_line), ("parked", origin, []), ("good1", origin, []),
             ("bad_code", (np.where(np.arange(90) == 40, 8, first.squares()).astype(np.uint8), 1, 0), []),
             ("bad_id", origin, [good[0], 2086])]
    want = np.array([0, 3, 3, -1, -2, 0, 0, -1, 2], np.int32)
    B = len(loads)
    e = _engine(B, 32, eval_cache_log2=10, mirror=False)
    sq, turn, half, moves = _arrays(loads)
    park = np.array([name == "parked" for name, _, _ in loads])
    status = e.set_positions(sq, turn, half, moves, park=park)
    assert np.array_equal(status, want), status
    parked = (want != 0) | park
    st = e.game_status()
    assert np.array_equal(st["over"] != 0, parked) and (st["winner"][parked] == -1).all() and not st["plies"].any()
    assert e.stats()["error_flags"] == 0
    assert not e.root_positions()[parked].any() and e.root_children()["k"].sum() == 0
    e.select_leaves()
    info = e.leaf_info()
    assert (info["status"][parked] == _lib.LEAF_SKIP).all() and (info["status"][~parked] == _lib.LEAF_EXPAND).all()
    rows, n_miss = e.eval_plan()
    n_miss = int(n_miss.item())
    planned = set(rows[:n_miss].cpu().tolist())
    assert planned and planned <= set(np.flatnonzero(~parked).tolist())      # no evaluator row for a parked board
    pending = C.c_int64(-1)
    _lib.check(e.L.ccz_harvest_rows(e.h, e._stream(), C.byref(pending)))
    assert pending.value == 0
    assert e.harvest()[2].shape[0] == 0 and list(e.harvest_record_chunks()) == []
    for call in (lambda got: e.L.ccz_harvest(e.h, e._stream(), None, None, None, 0, C.byref(got)),      # the calls themselves: nothing
                 lambda got: e.L.ccz_harvest_records(e.h, e._stream(), None, 0, C.byref(got))):         # to emit, and no failure
        got = C.c_int64(-1)
        _lib.check(call(got))
        assert got.value == 0
    assert np.array_equal(e.game_status()["over"] != 0, parked)                # the harvest left them parked
    # the good boards of the same call search normally
    boards = [_replayed(s, m) if not parked[j] else OracleBoard() for j, (_, s, m) in enumerate(loads)]
    ls = Lockstep(e, boards, kind="hash", salts=list(range(40, 40 + B)))
    ls.run_fused(32, check_leaf=True)
    rc = ls.compare_roots()
    assert (rc["root_visits"][~parked] == 32).all() and not rc["root_visits"][parked].any()
    pv = e.principal_variations(multipv=2, max_len=4)
    assert not pv["len"][parked].any() and (pv["len"][~parked, 0] >= 1).all()
    e.check_healthy()
    # a parked board is loaded again by the next call that masks it
    mask = np.zeros(B, np.uint8)
    mask[1] = 1
    again = e.set_positions(sq, turn, half, [m if j != 1 else good for j, m in enumerate(moves)], mask=mask)
    assert again[1] == 0 and not e.game_status()["over"][1] and np.array_equal(e.root_positions()[1], boards[0].squares())
    assert np.array_equal(e.game_status()["over"] != 0, parked & (np.arange(B) != 1))


class _Logged:
    """Lockstep whose oracle backups are logged, so that a fresh oracle tree of any board can be rebuilt without the evaluator."""

    def __init__(self, engine, boards, kind, salts):
        from gpu_harness import Lockstep
        self.ls = Lockstep(engine, boards, kind=kind, salts=salts)
        self.log = [[] for _ in boards]
        inner = self.ls._oracle_backup

        def backup(P, V, pending):
            for b, item in enumerate(pending):
                if item is not None:
                    self.log[b].append((np.array(item[1], np.uint16), P[b][item[1]].copy(), V[b]))
            inner(P, V, pending)

        self.ls._oracle_backup = backup

    def fresh(self, b):
        from oracle import OracleMCTS
        m = OracleMCTS(None, c_puct=5, n_playout=0)
        for ids, prob, v in self.log[b]:
            leaf, _ = m.select(self.ls.boards[b])
            m.expand_backup(leaf, ids, prob, v)
        return m


def _oracle_line(m, rank, max_len):
    """The walk root_children -> (rank-th, then first) arg-max of visits -> update_with_move, until no children or no visits."""
    acts, visits, q, prior = m.root_children()
    if len(acts) == 0:
        return [], [], None, None
    order = sorted(range(len(acts)), key=lambda i: (-int(visits[i]), i))
    if rank >= len(order) or visits[order[rank]] == 0:
        return [], [], None, None
    i = order[rank]
    first_q, first_p = q[i], prior[i]
    moves, ns = [], []
    while len(moves) < max_len:
        moves.append(int(acts[i]))
        ns.append(int(visits[i]))
        m.update_with_move(int(acts[i]))
        acts, visits, q, prior = m.root_children()
        if len(acts) == 0 or visits.max() == 0:
            break
        i = int(np.argmax(visits))
    return moves, ns, first_q, first_p


def _check_lines(lg, e, pv, rc, boards, multipv, max_len):
    longest = 0
    for b in boards:
        for r in range(multipv):
            moves, ns, fq, fp = _oracle_line(lg.fresh(b), r, max_len)
            ln = int(pv["len"][b, r])
            assert ln == len(moves), (b, r, ln, moves)
            assert pv["moves"][b, r, :ln].tolist() == moves and pv["visits"][b, r, :ln].tolist() == ns, (b, r)
            assert not pv["moves"][b, r, ln:].any() and not pv["visits"][b, r, ln:].any()
            if ln:
                k = int(rc["k"][b])
                c = rc["acts"][b][:k].tolist().index(moves[0])
                assert pv["q"][b, r].view(np.uint32) == rc["q"][b][c].view(np.uint32) == np.float32(fq).view(np.uint32)
                assert pv["prior"][b, r].view(np.uint32) == rc["prior"][b][c].view(np.uint32) == np.float32(fp).view(np.uint32)
                longest = max(longest, ln)
        assert pv["root_visits"][b] == rc["root_visits"][b]
    return longest


def test_principal_variations_equal_the_oracles_tree():
    from oracle import OracleBoard
    B, n = 8, 600
    e = _engine(B, n)
    lg = _Logged(e, [OracleBoard() for _ in range(B)], "hash", list(range(1, B + 1)))
    lg.ls.run_fused(n, check_leaf=False)
    rc = lg.ls.compare_roots()
    pv = e.principal_variations(multipv=4, max_len=16)
    assert pv["moves"].dtype == np.uint16 and pv["moves"].shape == (B, 4, 16) and pv["len"].shape == (B, 4)
    assert _check_lines(lg, e, pv, rc, range(B), 4, 16) >= 3            # the walk below the root is exercised
    for b in range(B):                                                   # rank 0 is the first maximum: the arg-max move
        k = int(rc["k"][b])
        assert pv["moves"][b, 0, 0] == rc["acts"][b][int(np.argmax(rc["visits"][b][:k]))]
        firsts = pv["moves"][b, :, 0][pv["len"][b] > 0].tolist()
        assert len(set(firsts)) == len(firsts) == 4                      # four different root moves
    one = e.principal_variations(multipv=4, max_len=1)                   # max_len = 1 truncates
    assert (one["len"] == np.minimum(pv["len"], 1)).all() and np.array_equal(one["moves"][:, :, 0], pv["moves"][:, :, 0])
    assert np.array_equal(one["visits"][:, :, 0], pv["visits"][:, :, 0])
    assert np.array_equal(one["q"].view(np.uint32), pv["q"].view(np.uint32))
    # on the engine alone: forcing the line's moves with the tree kept shows the next one as the first arg-max of the new root
    steps = int(pv["len"][:, 0].min()) - 1
    assert steps >= 1
    for t in range(steps):
        e.finish_move(forced_moves=pv["moves"][:, 0, t].astype(np.int32), keep_tree=True)
        now = e.root_children()
        for b in range(B):
            k = int(now["k"][b])
            c = int(np.argmax(now["visits"][b][:k]))
            assert now["acts"][b][c] == pv["moves"][b, 0, t + 1] and now["visits"][b][c] == pv["visits"][b, 0, t + 1]
            assert now["root_visits"][b] == pv["visits"][b, 0, t]
    e.check_healthy()


def test_principal_variation_ends_at_a_terminal_node_and_finished_boards_have_none():
    import rules_kat
    from oracle import OracleBoard
    ID = _ids()
    mate = rules_kat.start_of(_kat_case(MATE_CASE))
    first = OracleBoard()
    loads = [("mate_in_one", mate, []), ("start", (first.squares(), 1, 0), []), ("mated", mate, [ID[MATE_MOVE]])]
    e = _engine(3, 96)
    sq, turn, half, moves = _arrays(loads)
    assert not e.set_positions(sq, turn, half, moves).any()
    st = e.game_status()
    assert st["over"].tolist() == [0, 0, 1] and st["winner"][2] == 1 and st["turn"][2] == 0      # red has mated
    boards = [_replayed(s, m) for _, s, m in loads]
    lg = _Logged(e, boards, "hash", [3, 4, 5])
    lg.ls.run_fused(96, check_leaf=True)
    rc = lg.ls.compare_roots()
    pv = e.principal_variations(multipv=3, max_len=8)
    _check_lines(lg, e, pv, rc, [0, 1], 3, 8)
    assert not pv["len"][2].any() and pv["root_visits"][2] == 0 and not pv["moves"][2].any()    # over: zero lines
    ln = int(pv["len"][0, 0])
    end = boards[0].copy()
    for m in pv["moves"][0, 0, :ln]:
        end.push_id(int(m))
    assert pv["moves"][0, 0, 0] == ID[MATE_MOVE] and ln == 1 and not end.legal_ids()   # the line stops at the mated position ...
    assert pv["visits"][0, 0, 0] > 1                                                # ... which was visited again and again
    e.check_healthy()


def _tiny_net(seed=4):
    from chinesechesszero_amd.net import PolicyValueNet
    torch.manual_seed(seed)
    return PolicyValueNet(device="cuda:0", num_channels=32, resblocks_num=2)


def test_batched_analysis_end_to_end():
    import rules_kat
    from chinesechesszero_amd.analyse import BatchedAnalysis
    from chinesechesszero_amd.game import Board
    from chinesechesszero_amd.mcts import MCTS_AI
    from chinesechesszero_amd.uci import parse_position
    import oracle
    from oracle import OracleBoard
    uci = oracle.move_table()
    rs = np.random.RandomState(23)
    positions = []
    for w in range(35):
        b, line = OracleBoard(), []
        for _ in range(w % 12):
            ids = b.legal_ids()
            line.append(ids[rs.randint(len(ids))])
            b.push_id(line[-1])
        assert not (b.is_game_over() or b.is_tie())
        positions.append("startpos" + (" moves " + " ".join(uci[m] for m in line) if line else ""))
    positions.insert(9, "startpos moves h2e2 h9g7 a0a5 a9a8")             # move 2 is illegal
    mate = rules_kat.start_of(_kat_case(MATE_CASE))
    mated = Board(mate[0], bool(mate[1]), mate[2])
    mated.push(MATE_MOVE)
    positions.insert(20, mated)                                           # already mated
    assert len(positions) == 37
    pvn = _tiny_net()
    n = 24
    res = {}
    for cache in (12, 0):
        an = BatchedAnalysis(pvn, 16, n_playout=n, multipv=2, max_len=8, eval_cache_log2=cache)
        assert an.sp.planned == bool(cache)
        res[cache] = an.analyse(positions)
        s = an.summary()
        assert s["positions"] == 37 and s["sims_per_s"] > 0 and 0 < s["evaluator_rows_per_step"] <= 16
        assert an.engine.stats()["sims"] == 35 * n                        # the parked tail and the refused boards cost nothing
    got = res[12]
    assert len(got) == 37 and [r["status"] for r in got] == ["ok"] * 9 + ["illegal move 2"] + ["ok"] * 10 + ["game over: red wins"] + ["ok"] * 16
    for j, r in enumerate(got):
        if r["status"] != "ok":
            assert r["bestmove"] is None and not r["lines"]
            continue
        assert r["root_visits"] == n and r["bestmove"] == r["lines"][0]["moves"][0] and 1 <= len(r["lines"]) <= 2
        board = parse_position(positions[j].split(), validate=False)      # results are in input order: the move fits ITS position
        assert r["bestmove"] in [m.uci() for m in board.legal_moves], j
        assert all(l["visits"][0] >= l2["visits"][0] for l, l2 in zip(r["lines"], r["lines"][1:]))
    assert [r["lines"] for r in res[12]] == [r["lines"] for r in res[0]]  # the evaluation cache changes nothing
    for j in (0, 5, 17, 36):                                              # the one-game front end chooses the same move
        board = parse_position(positions[j].split(), validate=False)
        ai = MCTS_AI(pvn.policy_value_fn, c_puct=5, n_playout=n, scouts=0)
        ai.mcts.use_graph = False
        ai.mcts.get_move_probs(board)
        rc = ai.mcts.root_children()
        assert uci[int(rc["acts"][int(np.argmax(rc["visits"]))])] == got[j]["bestmove"], j
        assert int(rc["visits"].max()) == got[j]["lines"][0]["visits"][0]


def test_uci_prints_one_info_line_per_principal_variation():
    from test_gpu_frontends_parity import _hash_policy
    from chinesechesszero_amd.uci import UciLoop
    for multipv in (3, None):
        out = io.StringIO()
        loop = UciLoop(policy_value_fn=_hash_policy(9), n_playout=64, out=out)
        script = ["uci", "ucinewgame"] + ([f"setoption name MultiPV value {multipv}"] if multipv else []) + ["position startpos moves h2e2 h9g7", "go nodes 96"]
        for line in script:
            assert loop.handle(line)
        text = out.getvalue().splitlines()
        pvs = [l.split() for l in text if l.startswith("info depth ")]
        assert len(pvs) == (multipv or 1)
        best = [l for l in text if l.startswith("bestmove ")]
        assert len(best) == 1 and len([l for l in text if l.startswith("info nodes 96 string visits ")]) == 1
        assert text.index(" ".join(pvs[-1])) < text.index(best[0]) - 1        # the PV lines come before the existing two
        for i, w in enumerate(pvs):
            assert w[:2] == ["info", "depth"] and w[3] == "multipv" and int(w[4]) == i + 1 and w[5:7] == ["score", "cp"] and w[8] == "nodes"
            assert int(w[9]) == 96 and w[10] == "pv" and int(w[2]) == len(w) - 11 >= 1 and abs(int(w[7])) < 4000
        assert pvs[0][11] == best[0].split()[1]
