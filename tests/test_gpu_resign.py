"""GPU: self-play resignation with play-on calibration and recorded root values (ccz_set_resign / ccz_resign_status /
ccz_get_resign_stats / ccz_expand_record_values / ccz_sample_record_values, include/cczero.h). Everything is exact, no tolerance:
the engine is driven next to the host model of tests/resign_model.py, which is fed what ccz_root_children returns and the host
twin of the device's Philox word, and every move boundary, status read, counter and record byte is compared.

The stub evaluator returns uniform priors and value = -c_b where the leaf's turn plane says red is to move, +c_b otherwise: every
child of a red root then holds Q = -c_b exactly and every child of a black root +c_b, so a root value is -c_b or +c_b to the bit
(the float64 mean of equal float32 values is that value). Boards by index mod 4: 0 red sees -0.95 (resigns under -0.9), 1 the signs
flipped (black resigns), 2 c = 0.5 (nobody resigns), 3 c = float32(0.9) = the threshold itself (`<`: nobody resigns)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resign_model as rm
from chinesechesszero_amd import _lib
from resign_model import PLAYON, RESIGNED, Game, Rule

pytestmark = pytest.mark.gpu

B, N, SEED, BASE, MAXP = 32, 16, 7, 4096, 10
THRESHOLD = -0.9
C_OF_GROUP = np.array([0.95, 0.95, 0.5, np.float32(0.9)], np.float32)
SIGN_OF_GROUP = np.array([1.0, -1.0, 1.0, 1.0], np.float32)
GROUP = np.arange(B) % 4


def _ua(seed, board_id, move_no, child, draw=0):
    """uniform2's first uniform (csrc/cczero_device.h) on the oracle's Philox: the route test_gpu_budgets.py::_ua takes."""
    import oracle
    o = (C.c_uint32 * 4)()
    lo = ((move_no << 32) | ((child & 0xfff) << 20) | (draw & 0xfffff)) & (2**64 - 1)
    oracle.lib().xq_philox4x32(C.c_uint64(seed), C.c_uint64(board_id), C.c_uint64(lo), o)
    return float(2 * (((o[0] << 32) | o[1]) >> 12) + 1) * 1.1102230246251565e-16


class Stub:
    """value[b] = -c[b] * sign[b] where red is to move at the leaf (turn plane = ones), + otherwise; uniform priors."""

    def __init__(self, c=None, sign=None, n=B):
        dev = torch.device("cuda", 0)
        c = C_OF_GROUP[np.arange(n) % 4] if c is None else np.broadcast_to(np.asarray(c, np.float32), (n,))
        sign = SIGN_OF_GROUP[np.arange(n) % 4] if sign is None else np.broadcast_to(np.asarray(sign, np.float32), (n,))
        self.amp = torch.from_numpy(np.ascontiguousarray(c * sign, dtype=np.float32)).to(dev)
        self.prob = torch.full((n, 2086), 1.0 / 2086, dtype=torch.float32, device=dev)

    def flip(self, boards):
        self.amp[torch.as_tensor(np.asarray(boards), device=self.amp.device)] *= -1.0

    def __call__(self, leaf):
        red = leaf[:, 16, 0, 0, 0] > 0
        return self.prob, torch.where(red, -self.amp, self.amp).contiguous()


def _engine(base=BASE, maxp=MAXP, n_boards=B, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(n_boards, n_playout=N, seed=SEED, board_id_base=base, max_plies=maxp, **kw)


def _header(rec):
    t = rec[:, 96:98].copy().view(np.uint16).ravel().astype(np.int64)
    T = rec[:, 98:100].copy().view(np.uint16).ravel().astype(np.int64)
    winner = rec[:, 100].copy().view(np.int8).astype(np.int64)
    board = rec[:, 104:108].copy().view(np.uint32).ravel().astype(np.int64)
    return t, T, winner, board


class Play:
    """An engine and, per board, the model of its current game. ``rule`` None: an engine that never hears of the feature."""

    def __init__(self, e, stub, rule=None, base=BASE, maxp=MAXP, configure=True):
        self.e, self.stub, self.rule, self.base, self.maxp = e, stub, rule, base, maxp
        self.n = e.B
        self.enabled = rule is not None
        if rule is not None and configure:
            e.set_resign(rule.threshold, consecutive=rule.consecutive, min_ply=rule.min_ply, p_playon=rule.p_playon)
        self._rule = rule if rule is not None else Rule(-1.0, 0, 0, 0.0)
        self.games = [Game(self._rule) for _ in range(self.n)]
        self.done = []                      # (board, model, records uint8 [T, 880]) of every harvested game, in harvest order
        self.counter = np.zeros(self.n, np.int64)   # the boards' move counters: plies ever recorded on the slot
        self.steps = N                      # lockstep simulations per move
        self.trace = []

    def search(self, steps=N):
        e = self.e
        leaf = e.select_leaves()
        for i in range(steps):
            prob, value = self.stub(leaf)
            if i + 1 < steps:
                leaf = e.step(prob, value)
            else:
                e.expand_backup(prob, value)

    def move(self, budgets=None, targets=None, force=(), gamma=False, where=""):
        """One lockstep move of every live board, checked against the models. ``force``: boards whose move the host forces (the
        most visited child). Returns the moves."""
        e, n = self.e, self.n
        st0, sq0 = e.game_status(), e.root_positions()
        if budgets is not None:
            e.set_budgets(budgets, targets)
        rc0 = e.root_children()
        visits0, children0 = rc0["root_visits"], rc0["visits"].sum(axis=1)
        self.search(self.steps)
        rc = e.root_children()
        g = e.move_distribution()[0] if gamma else None
        forced = None
        if len(force):
            forced = np.full(n, -1, np.int32)
            for b in force:
                forced[b] = int(rc["acts"][b][int(np.argmax(rc["visits"][b][:rc["k"][b]]))])
        moves = e.finish_move(forced_moves=forced).cpu().numpy().copy()
        st1, rs, sq1 = e.game_status(), e.resign_status(), e.root_positions()
        want, got = [], []
        for b in range(n):
            if st0["over"][b]:
                want.append("over"), got.append("over")
                assert moves[b] == -1 and st1["plies"][b] == st0["plies"][b]
                continue
            game, ply, turn = self.games[b], int(st0["plies"][b]), int(st0["turn"][b])
            if ply >= self.maxp:
                game.end(-1)
                want.append("cap")
            else:
                k = int(rc["k"][b])
                v64 = rm.root_value64(rc["visits"][b, :k], rc["q"][b, :k])
                u = _ua(SEED, self.base + b, int(self.counter[b]), 0xffd)
                ev = game.record(turn, v64, 1 if targets is None else int(targets[b]), forced is not None and forced[b] >= 0, u,
                                 enabled=self.enabled)
                self.counter[b] += 1
                if ev != "resign" and st1["over"][b]:
                    game.end(int(st1["winner"][b]))          # an end by the rules: the engine's word (tested elsewhere)
                want.append(ev)
            ended = bool(st1["over"][b])
            if ended and moves[b] < 0 and (rs["state"][b] & RESIGNED):
                got.append("resign")
                assert rs["fire_ply"][b] == ply and rs["state"][b] == RESIGNED | turn, (where, b)
                assert st1["winner"][b] == turn ^ 1 and st1["plies"][b] == ply + 1 and st1["turn"][b] == turn, (where, b)
                assert np.array_equal(sq1[b], sq0[b]), (where, b)                  # no move was pushed
            elif ended and moves[b] < 0:
                got.append("cap")
                assert st1["winner"][b] == -1 and st1["plies"][b] == ply, (where, b)
            else:
                got.append("playon" if (rs["state"][b] & PLAYON) and rs["fire_ply"][b] == ply else None)
                assert moves[b] >= 0 and st1["plies"][b] == ply + 1 and st1["turn"][b] == turn ^ 1, (where, b)
                assert not np.array_equal(sq1[b], sq0[b]), (where, b)
        rm.check_events(got, want, where)
        rm.check_status(rs, self.games, where)
        self.trace.append({"roots": rc, "moves": moves, "gamma": g, "status": st1, "visits0": visits0, "children0": children0, "events": got})
        return moves

    def harvest(self, where=""):
        """Harvest the finished games, check every record header against the game's model, restart the models."""
        chunks = list(self.e.harvest_record_chunks())
        if not chunks:
            return 0
        rec = torch.cat(chunks).cpu().numpy()
        t, T, winner, board = _header(rec)
        p, games = 0, 0
        while p < len(rec):
            n = int(T[p])
            b = int((board[p] - self.base) & 0xffffffff)
            game = self.games[b]
            assert game.over and n == game.plies and np.array_equal(t[p:p + n], np.arange(n)), (where, b, n, game.plies)
            assert (board[p:p + n] == board[p]).all() and (winner[p:p + n] == game.winner).all(), (where, b)
            assert (rec[p:p + n, 90:92] == 0).all(), (where, b)
            rm.check_record_flags(rec[p:p + n, _lib.REC_FLAGS], rec[p:p + n, 92:96].copy().view(np.float32).ravel(), game, (where, b))
            self.done.append((b, game, rec[p:p + n]))
            self.games[b] = Game(self._rule)
            p += n
            games += 1
        rm.check_status(self.e.resign_status(), self.games, (where, "after the harvest"))   # the restarted boards are clear
        return games

    def finish(self):
        over = [g for g in self.games if g.over]
        assert self.e.stats()["games"] == len(self.done) + len(over)
        rm.check_stats(self.e.resign_stats(), [g for _, g, _ in self.done] + over)
        self.e.check_healthy()


def _same_roots(a, b, boards, where=""):
    for key in ("k", "acts", "visits", "root_visits"):
        assert np.array_equal(a[key][boards], b[key][boards]), (where, key)
    for key in ("q", "prior"):
        assert np.array_equal(a[key][boards].view(np.uint32), b[key][boards].view(np.uint32)), (where, key)


def _strip_values(rec):
    """Records with bytes 92..95 zeroed and CCZ_REC_VALUE cleared: all that the recorded values may change."""
    r = rec.copy()
    r[:, 92:96] = 0
    r[:, _lib.REC_FLAGS] &= ~np.uint8(_lib.REC_VALUE)
    return r


@functools.lru_cache(maxsize=None)
def _featureless(base=BASE, moves=MAXP + 1):
    """The engine that never hears of resignation: its trace (roots, Dirichlet draws, moves) and the records of its first games."""
    p = Play(_engine(base), Stub(), None, base=base)
    for mv in range(moves):
        p.move(gamma=True, where=("featureless", mv))
    p.harvest("featureless")
    p.finish()
    assert p.e.resign_stats() == dict.fromkeys(rm.STAT_KEYS, 0)
    return p


# ---------------------------------------------------------------------- the root value
def test_the_recorded_root_value_is_the_visit_weighted_mean_of_q():
    """consecutive = 0: values are recorded, nothing resigns. Kept trees (the children carry visits from earlier moves) and board 5
    with budget 1 (a fresh root's only simulation expands it: no visited child -> 0.0). last_value after every move and bytes
    92..95 of every record equal root_value(ccz_root_children), bit for bit (Play.move / Play.harvest)."""
    p = Play(_engine(), Stub(), Rule(THRESHOLD, 0, 0, 0.0))
    budgets = np.full(B, N, np.int32)
    budgets[5] = 1
    for mv in range(MAXP + 1):
        p.move(budgets=budgets, where=("values", mv))
        if mv < MAXP:
            last = p.e.resign_status()["last_value"]
            assert last[5] == 0.0 and p.trace[-1]["roots"]["k"][5] > 0 and (p.trace[-1]["roots"]["visits"][5] == 0).all()
        if mv < 4:                                                           # (later a search may meet a terminal leaf: Q = +-1 there)
            grp = np.arange(B) != 5
            want = np.where(p.trace[-1]["status"]["turn"] == 0, -1.0, 1.0) * (C_OF_GROUP * SIGN_OF_GROUP)[GROUP]   # turn AFTER the move
            assert np.array_equal(last[grp], want[grp].astype(np.float32)), mv   # -c where red moved, +c where black did: exact
    assert any((tr["visits0"] > 0).any() for tr in p.trace[1:])                   # trees were kept
    assert p.harvest("values") == B
    assert all(g.state == 0 and g.plies == MAXP and all(v is not None for v in g.values) for _, g, _ in p.done)
    assert (np.concatenate([r for _, _, r in p.done])[:, _lib.REC_FLAGS] == _lib.REC_VALUE).all()
    p.finish()
    # 64 simulations per move visit every child once and then go deeper: the kept root's CHILDREN carry visits from earlier moves
    deep = Play(_engine(), Stub(), Rule(THRESHOLD, 0, 0, 0.0))
    deep.steps = 64
    for mv in range(3):
        deep.move(where=("deep", mv))
    assert (deep.trace[0]["children0"] == 0).all() and (deep.trace[2]["children0"] > 0).any()
    deep.e.check_healthy()


# ---------------------------------------------------------------------- neutral settings
def test_an_engine_that_records_values_is_otherwise_the_engine_without_the_feature():
    maxp = 3
    a = Play(_engine(maxp=maxp), Stub(), None, maxp=maxp)
    b = Play(_engine(maxp=maxp), Stub(), Rule(THRESHOLD, 0, 0, 0.5), maxp=maxp)
    every = np.arange(B)

    def game(tag):
        for mv in range(maxp + 1):
            ma, mb = a.move(where=(tag, "a", mv)), b.move(where=(tag, "b", mv))
            assert np.array_equal(ma, mb), (tag, mv)
            _same_roots(a.trace[-1]["roots"], b.trace[-1]["roots"], every, (tag, mv))
            for key in ("over", "winner", "plies", "turn"):
                assert np.array_equal(a.trace[-1]["status"][key], b.trace[-1]["status"][key]), (tag, mv, key)
        assert a.e.stats() == b.e.stats(), tag
        na, nb = len(a.done), len(b.done)
        assert a.harvest(tag) == B and b.harvest(tag) == B
        return np.concatenate([r for _, _, r in a.done[na:]]), np.concatenate([r for _, _, r in b.done[nb:]])

    ra, rb = game("first")
    assert (ra[:, 90:96] == 0).all() and (ra[:, _lib.REC_FLAGS] == 0).all()           # never configured: the bytes of old
    assert (rb[:, _lib.REC_FLAGS] == _lib.REC_VALUE).all() and (rb[:, 92:96] != 0).any()
    assert np.array_equal(_strip_values(rb), ra)
    b.e.set_resign(None)                                                              # off again: the next game is byte for byte a's
    b.enabled = False
    ra, rb = game("second")
    assert np.array_equal(ra, rb) and (rb[:, 90:96] == 0).all() and (rb[:, _lib.REC_FLAGS] == 0).all()
    a.finish()
    b.finish()
    assert b.e.resign_stats() == dict.fromkeys(rm.STAT_KEYS, 0)


# ---------------------------------------------------------------------- the rule
def _fire(s, consecutive, min_ply):
    """The ply at which side s (1 red: even plies of a game red starts) resigns when all its values are low."""
    p = (0 if s else 1) + 2 * (consecutive - 1)
    while p < min_ply:
        p += 2
    return p


@pytest.mark.parametrize("consecutive,min_ply", [(1, 0), (2, 0), (3, 0), (1, 5), (2, 5), (3, 5)])
def test_the_rule_against_the_model(consecutive, min_ply):
    """Red-resigning and black-resigning boards in one engine, harvested after every move: a restarted board's next game resigns
    again, on its own clock. The boards whose value never drops (groups 2 and 3: c = 0.5, and c = the threshold itself) are bit
    for bit the boards of the feature-less engine."""
    p = Play(_engine(), Stub(), Rule(THRESHOLD, consecutive, min_ply, 0.0))
    ref = _featureless()
    calm = np.flatnonzero(GROUP >= 2)
    for mv in range(MAXP + 1):
        p.move(where=(consecutive, min_ply, mv))
        _same_roots(p.trace[-1]["roots"], ref.trace[mv]["roots"], calm, mv)
        assert np.array_equal(p.trace[-1]["moves"][calm], ref.trace[mv]["moves"][calm]), mv
        p.harvest((consecutive, min_ply, mv))
    p.finish()
    # the first game of every board: where the model says it ends
    first = {}
    for b, g, rec in p.done:
        first.setdefault(b, (g, rec))
    for b in range(B):
        g, rec = first[b]
        if GROUP[b] < 2:
            s = 1 if GROUP[b] == 0 else 0                                 # red resigns on group 0, black on group 1
            fire = _fire(s, consecutive, min_ply)
            assert g.state == RESIGNED | s and g.fire_ply == fire and g.plies == fire + 1 and g.winner == s ^ 1, (b, g.status())
            assert (rec[:, _lib.REC_FLAGS] == (_lib.REC_RESIGNED | _lib.REC_VALUE)).all()
        else:
            assert g.state == 0 and g.plies == MAXP and g.winner == -1
            want = np.concatenate([r for bb, _, r in ref.done if bb == b])
            assert np.array_equal(_strip_values(rec), want), b                # trees, moves, pi: the feature-less board's records
    st = p.e.resign_stats()
    assert st["resigned_games"] >= B // 2 and 0 < st["resigned_by_red"] < st["resigned_games"] and st["playon_games"] == 0
    if (consecutive, min_ply) == (1, 0):
        assert st["resigned_games"] > B                                        # restarted boards resigned again, and again


# ---------------------------------------------------------------------- the play-on lot
@pytest.mark.parametrize("p_playon", [0.0, 0.5, 1.0])
def test_the_play_on_lot_is_the_host_twin_and_a_played_on_game_never_resigns(p_playon):
    """Board ids past 2^32. consecutive = 1: group 0 fires at ply 0, group 1 at ply 1. The lot is word 0xffd of the board's
    Philox stream for that move (Play.move feeds the model the host twin); a game that drew it runs to the cap -- the model never
    lets it fire again -- and is, trees, Dirichlet draws and moves, the game of the feature-less engine."""
    base = 2**32 + 77
    p = Play(_engine(base), Stub(), Rule(THRESHOLD, 1, 0, p_playon), base=base)
    ref = _featureless(base)
    first_game = np.ones(B, bool)
    for mv in range(MAXP + 1):
        p.move(gamma=True, where=(p_playon, mv))
        live = np.flatnonzero(first_game)                                     # up to and including the fire ply
        _same_roots(p.trace[-1]["roots"], ref.trace[mv]["roots"], live, mv)
        assert np.array_equal(p.trace[-1]["gamma"][live], ref.trace[mv]["gamma"][live]), mv
        played = np.array([ev != "resign" for ev in p.trace[-1]["events"]])
        keep = live[played[live]]
        assert np.array_equal(p.trace[-1]["moves"][keep], ref.trace[mv]["moves"][keep]), mv
        first_game &= played
        p.harvest((p_playon, mv))
    p.finish()
    firing = np.flatnonzero(GROUP < 2)
    twin = {b: _ua(SEED, base + b, 0 if GROUP[b] == 0 else 1, 0xffd) < p_playon for b in firing}
    first = {}
    for b, g, rec in p.done:
        first.setdefault(b, (g, rec))
    for b in firing:
        g, rec = first[b]
        s = 1 if GROUP[b] == 0 else 0
        if twin[b]:
            assert g.state == PLAYON | s and g.fire_ply == 1 - s and g.plies == MAXP and g.winner == -1, (b, g.status())
            assert (rec[:, _lib.REC_FLAGS] == (_lib.REC_PLAYON | _lib.REC_VALUE)).all()
            want = np.concatenate([r for bb, _, r in ref.done if bb == b])
            want[:, _lib.REC_FLAGS] |= _lib.REC_PLAYON
            assert np.array_equal(_strip_values(rec), want), b
        else:
            assert g.state == RESIGNED | s and g.plies == 2 - s, (b, g.status())
    n_on = sum(twin.values())
    assert n_on == {0.0: 0, 1.0: len(firing)}.get(p_playon, n_on) and (p_playon != 0.5 or 0 < n_on < len(firing))
    st = p.e.resign_stats()
    played_on = [g for _, g, _ in p.done if g.state & PLAYON]
    assert st["playon_games"] == len(played_on) == st["playon_drawn"] and st["playon_won"] == 0
    assert st["playon_plies_after"] == sum(g.plies - g.fire_ply for g in played_on)
    if p_playon == 1.0:
        assert st["resigned_games"] == 0


def _helpmate(board, side, max_plies=4):
    """Shortest cooperative line (move ids) after which ``side`` has won by the rules, by breadth-first search on the CPU oracle."""
    frontier = [(board, [])]
    for _ in range(max_plies):
        nxt = []
        for b, line in frontier:
            for m in b.legal_ids():
                c = b.copy()
                c.push_id(m)
                o = c.outcome()
                if o is not None:
                    if o.winner is not None and int(o.winner) == side:
                        return line + [m]
                    continue
                nxt.append((c, line + [m]))
        frontier = nxt
    return None


def test_a_played_on_game_that_its_side_wins_counts_as_a_false_positive():
    """King and two rooks against a bare king, red to move and seeing -0.95: the rule fires at ply 0, every board draws the lot
    (p_playon = 1) and plays its sampled move; from there the host forces a cooperative mate found on the CPU oracle (forced
    moves never fire the rule, and a played-on game could not resign anyway). Red -- the side that would have resigned -- wins:
    playon_won, and playon_plies_after = T - 0."""
    from oracle import OracleBoard
    n = 4
    sq = np.zeros(90, np.uint8)
    sq[3], sq[0 + 9 * 7], sq[1 + 9 * 6], sq[4 + 9 * 9] = 7, 3, 3, 15     # red king d0, red rooks a7 b6, black king e9
    e = _engine(n_boards=n)
    assert not e.set_positions(np.repeat(sq[None], n, 0), np.ones(n, np.uint8)).any()
    p = Play(e, Stub(0.95, 1.0, n), Rule(THRESHOLD, 1, 0, 1.0))
    m0 = p.move(where="fire")
    assert all(ev == "playon" for ev in p.trace[-1]["events"])
    lines = []
    for b in range(n):
        ob = OracleBoard.from_array(sq, 1, 0)
        ob.push_id(int(m0[b]))
        if ob.outcome() is not None:                                       # the sampled move mated on the spot
            assert ob.outcome().winner and p.games[b].over
            lines.append([])
            continue
        line = _helpmate(ob, 1)
        assert line is not None and len(line) <= 4
        lines.append(line)
    for i in range(max(len(x) for x in lines)):
        live = [b for b in range(n) if i < len(lines[b])]
        e_forced = {b: lines[b][i] for b in live}
        _forced_move(p, e_forced, ("line", i))
    st = e.game_status()
    assert st["over"].all() and (st["winner"] == 1).all()
    assert all(g.state == PLAYON | 1 and g.fire_ply == 0 and g.winner == 1 for g in p.games)
    want = {"resigned_games": 0, "resigned_by_red": 0, "resigned_plies": 0, "playon_games": n, "playon_won": n, "playon_drawn": 0,
            "playon_plies_after": int(sum(1 + len(x) for x in lines))}
    assert e.resign_stats() == want
    assert p.harvest("won") == n
    assert all((rec[:, _lib.REC_FLAGS] == (_lib.REC_PLAYON | _lib.REC_VALUE)).all() for _, _, rec in p.done)
    p.finish()


def _forced_move(p, forced_of_board, where):
    """Play.move with host-chosen move ids on some boards (the others are over)."""
    e = p.e
    st0 = e.game_status()
    p.search()
    rc = e.root_children()
    forced = np.full(p.n, -1, np.int32)
    for b, m in forced_of_board.items():
        forced[b] = m
    moves = e.finish_move(forced_moves=forced).cpu().numpy()
    st1, rs = e.game_status(), e.resign_status()
    for b in range(p.n):
        if st0["over"][b]:
            continue
        assert b in forced_of_board and moves[b] == forced_of_board[b], (where, b)
        k = int(rc["k"][b])
        ev = p.games[b].record(int(st0["turn"][b]), rm.root_value64(rc["visits"][b, :k], rc["q"][b, :k]), 1, True,
                               _ua(SEED, p.base + b, int(p.counter[b]), 0xffd))
        p.counter[b] += 1
        assert ev is None, (where, b)
        if st1["over"][b]:
            p.games[b].end(int(st1["winner"][b]))
    rm.check_status(rs, p.games, where)


# ---------------------------------------------------------------------- fast plies and forced moves
def test_fast_plies_leave_the_run_alone_and_a_forced_move_is_played():
    """consecutive = 2. Moves 2 and 3 are fast plies of playout-cap randomisation (target 0, 6 simulations) during which the
    stub's sign is flipped on half of the resigning boards: their value is HIGH on the fast ply, and the run must neither advance
    (boards that stay low) nor reset (boards that go high). Move 4: the run of the red boards completes; on boards 0 and 8 the
    host forces the move, which is played, and they resign at their next own ply instead."""
    p = Play(_engine(), Stub(), Rule(THRESHOLD, 2, 0, 0.0))
    full, fast = (np.full(B, N, np.int32), np.ones(B, np.uint8)), (np.full(B, 6, np.int32), np.zeros(B, np.uint8))
    flipped = np.flatnonzero((GROUP < 2) & (np.arange(B) % 8 < 4) & (np.arange(B) >= 16))
    runs = []
    for mv in range(8):
        budgets, targets = fast if mv in (2, 3) else full
        if mv in (2, 4):
            p.stub.flip(flipped)
        p.move(budgets=budgets, targets=targets, force=(0, 8) if mv == 4 else (), where=("fast", mv))
        runs.append(p.e.resign_status()["run"].copy())
        p.harvest(("fast", mv))
    red, black = np.flatnonzero(GROUP == 0), np.flatnonzero(GROUP == 1)
    assert (runs[0][red, 1] == 1).all() and (runs[2][red, 1] == 1).all() and (runs[3][black, 0] == 1).all()   # fast plies: untouched
    first = {}
    for b, g, rec in p.done:
        first.setdefault(b, (g, rec))
    highs = [first[b][0].values[2] for b in flipped if GROUP[b] == 0]
    assert highs and all(v > 0 for v in highs)                                   # ... although the value WAS high on these
    for b in red:
        g, rec = first[b]
        assert g.fire_ply == (6 if b in (0, 8) else 4) and g.state == RESIGNED | 1, (b, g.status())
        assert rec[2, _lib.REC_FLAGS] == (_lib.REC_FAST | _lib.REC_RESIGNED | _lib.REC_VALUE) and rec[4, _lib.REC_FLAGS] == 10
    for b in black:
        g, _ = first[b]
        assert g.fire_ply == 5 and g.state == RESIGNED | 0, (b, g.status())
    p.e.set_budgets(None)
    p.finish()


# ---------------------------------------------------------------------- restarts
def test_reset_tree_keeps_the_state_and_a_new_game_clears_it():
    p = Play(_engine(), Stub(), Rule(THRESHOLD, 3, 0, 0.0))
    for mv in range(3):
        p.move(where=("restart", mv))
    before = p.e.resign_status()
    assert (before["run"][GROUP == 0, 1] == 2).all() and (before["run"][GROUP == 1, 0] == 1).all()
    p.e.reset_tree()
    rm.check_status(p.e.resign_status(), p.games, "reset_tree")              # unchanged
    # a new game on the even boards: the current root positions loaded as starting positions
    mask = (np.arange(B) % 2 == 0).astype(np.uint8)
    st = p.e.game_status()
    assert not p.e.set_positions(p.e.root_positions(), st["turn"], mask=mask).any()
    for b in np.flatnonzero(mask):
        p.games[b] = Game(p._rule)
    after = p.e.resign_status()
    rm.check_status(after, p.games, "set_positions")
    assert (after["state"][mask == 1] == 0).all() and (after["run"][mask == 1] == 0).all() and (after["fire_ply"][mask == 1] == -1).all()
    assert np.isnan(after["last_value"][mask == 1]).all() and np.array_equal(after["run"][mask == 0], before["run"][mask == 0])
    p.e.set_position(1, p.e.root_positions()[1], int(st["turn"][1]))
    p.games[1] = Game(p._rule)
    rm.check_status(p.e.resign_status(), p.games, "set_position")
    p.e.reset(mask=(np.arange(B) == 3).astype(np.uint8))
    p.games[3] = Game(p._rule)
    rm.check_status(p.e.resign_status(), p.games, "reset")
    for mv in range(6):                                                      # and everybody goes on by the model
        p.move(where=("restart, on", mv))
    assert any(g.state & RESIGNED for g in p.games)
    p.e.check_healthy()


# ---------------------------------------------------------------------- the values calls
@functools.lru_cache(maxsize=None)
def _mixed_records():
    """Whole games with values (a resigning run: short and long games) and without (the feature-less run); the last one has values."""
    p = Play(_engine(), Stub(), Rule(THRESHOLD, 2, 0, 0.0))
    for mv in range(MAXP + 1):
        p.move(where=("records", mv))
        p.harvest(("records", mv))
    with_v = [r for _, _, r in p.done]
    without = [r for _, _, r in _featureless().done[:6]]
    parts = with_v[:5] + without[:3] + with_v[5:-1] + without[3:] + with_v[-1:]
    return torch.from_numpy(np.concatenate(parts)).cuda().contiguous()


def _row_values(rec, mul):
    r = rec.cpu().numpy()
    t, T, _, _ = _header(r)
    has = (r[:, _lib.REC_FLAGS] & _lib.REC_VALUE) != 0
    v = np.where(has, r[:, 92:96].copy().view(np.float32).ravel(), np.float32("nan")).astype(np.float32)
    p = np.arange(len(t))
    want = np.full(len(t) * mul, np.float32(7.0), np.float32)
    for q in range(mul):
        want[mul * (p - t) + q * T + t] = v
    assert not (want == 7.0).any()
    return want, v


@pytest.mark.parametrize("flags", [0, _lib.FLAG_NO_MIRROR])
def test_record_values_are_row_aligned_with_the_targets_calls(flags):
    from chinesechesszero_amd.engine import expand_record_targets, expand_record_values
    from chinesechesszero_amd.replay import RecordReplayBuffer, ReplayBuffer
    rec = _mixed_records()
    mul = 1 if flags else 2
    rows, v = _row_values(rec, mul)
    assert np.isnan(v).any() and (~np.isnan(v)).any() and len(np.unique(v[~np.isnan(v)])) >= 3
    got = expand_record_values(rec, flags)
    assert got.dtype == torch.float32 and got.shape == expand_record_targets(rec, flags).shape
    assert rm.same_f32(got.cpu().numpy(), rows)
    t, T, _, _ = _header(rec.cpu().numpy())
    if mul == 2:                                                             # a mirror row carries its sample's value
        g = got.cpu().numpy()
        first = np.arange(len(t)) - t
        assert rm.same_f32(g[2 * first + t], g[2 * first + T + t])
    # a game cut at the buffer end: NaN on the rows it leaves unwritten, everybody else's stay
    last = len(t) - int(T[-1])
    assert not np.isnan(rows[mul * last:]).any()
    cut = expand_record_values(rec[:-1].contiguous(), flags).cpu().numpy()
    assert len(cut) == mul * (len(t) - 1) and rm.same_f32(cut[:mul * last], rows[:mul * last]) and np.isnan(cut[mul * last:]).all()
    # a ring of rows written at an offset, wrapping
    ring = torch.full((mul * len(t) + 3,), 5.0, dtype=torch.float32, device="cuda")
    expand_record_values(rec, flags, out=ring, head_row=len(ring) - 4)
    rg = ring.cpu().numpy()
    assert rm.same_f32(np.concatenate([rg[-4:], rg[:mul * len(t) - 4]]), rows) and (rg[mul * len(t) - 4:-4] == 5.0).all()
    # the dense ring keeps the value next to the row it belongs to, and stores what append is given
    rb = ReplayBuffer(mul * len(t) + 5, "cuda")
    rb.append_records(rec, flags)
    assert rm.same_f32(rb.values[:mul * len(t)].cpu().numpy(), rows) and torch.isnan(rb.values[mul * len(t):]).all()
    idx = torch.arange(mul * len(t), device="cuda")
    out = rb.sample_at(idx, targets=True, values=True)
    assert len(out) == 5 and rm.same_f32(out[4].cpu().numpy(), rows) and len(rb.sample(8, values=True)) == 4 and len(rb.sample(8)) == 3
    s, pi, z = rb.sample_at(idx[:4])
    rb.append(s, pi, z, values=torch.tensor([0.5, float("nan"), -0.5, 0.25], device="cuda"))
    assert rm.same_f32(rb.values[mul * len(t):mul * len(t) + 4].cpu().numpy(), np.array([0.5, np.nan, -0.5, 0.25], np.float32))
    # the record ring, wrapped: every live row's value is its ply's, for the sample and for the mirror image
    cap = 2 * MAXP + 5
    rr = RecordReplayBuffer(cap, "cuda", flags, None, max_game_plies=MAXP)
    p = 0
    while p < len(t):
        rr.append_records(rec[p:p + int(T[p])])
        p += int(T[p])
    tail, head = rr.window()
    assert head == len(t) > cap and 0 < head - tail <= cap
    live = (head - tail) * mul
    draws = torch.arange(3 * live, device="cuda")
    out = rr.sample_at(draws, targets=True, values=True)
    assert len(out) == 5
    r = np.arange(3 * live) % live
    assert rm.same_f32(out[4].cpu().numpy(), v[tail + r // mul])
    assert np.array_equal(out[3].cpu().numpy(), 1 - (rec[:, _lib.REC_FLAGS].cpu().numpy()[tail + r // mul] & 1))
    assert int(rr.bad.item()) == 0
    assert len(rr.sample_at(draws[:4], values=True)) == 4 and len(rr.sample(8, values=True)) == 4 and len(rr.sample(8)) == 3
    vals = rr.sample_at(torch.tensor([0, -1, 1], device="cuda"), values=True)[3].cpu().numpy()
    assert np.isnan(vals[1]) and int(rr.bad.item()) == 1                      # a bad draw has no value


def test_the_sink_stores_the_values_of_the_records(tmp_path):
    from chinesechesszero_amd.collect import TupleSink
    rec = _mixed_records()
    s = TupleSink(str(tmp_path))
    s.append_records(rec, 0, games=1)
    assert s.finalize() == 2 * rec.shape[0]
    assert rm.same_f32(np.load(tmp_path / "root_values.npy"), _row_values(rec, 2)[0])
    s.close()
    plain = TupleSink(str(tmp_path / "plain"))
    plain.append_records(torch.from_numpy(np.concatenate([r for _, _, r in _featureless().done[:4]])), 0, games=4)
    assert plain.finalize() > 0 and not (tmp_path / "plain" / "root_values.npy").exists()
    plain.close()


# ---------------------------------------------------------------------- validation
def test_refused_arguments():
    e = _engine(n_boards=4)
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 2, 30, 0.1), (inf, 2, 30, 0.1), (-inf, 2, 30, 0.1), (-1.5, 2, 30, 0.1), (0.1, 2, 30, 0.1), (-0.9, -1, 30, 0.1),
                (-0.9, 256, 30, 0.1), (-0.9, 2, -1, 0.1), (-0.9, 2, 30, -0.1), (-0.9, 2, 30, 1.5), (-0.9, 2, 30, nan)):
        with pytest.raises(_lib.CczError, match="ccz_set_resign"):
            e.set_resign(*bad)
    for ok in ((-1.0, 0, 0, 0.0), (0.0, 255, 0, 1.0), (-0.9, 2, 30, 0.1)):
        e.set_resign(*ok)
    e.set_resign(None)
    st = e.resign_status()
    assert (st["state"] == 0).all() and (st["run"] == 0).all() and (st["fire_ply"] == -1).all() and np.isnan(st["last_value"]).all()
    e.check_healthy()
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    stub = Stub(n=4)
    for sampling in ("host", "numpy"):
        with pytest.raises(ValueError):
            BatchedSelfPlay(stub, 4, n_playout=N, sampling=sampling, resign=-0.9)
    with pytest.raises(ValueError, match="resign"):
        BatchedSelfPlay(stub, 4, n_playout=N, sampling="numpy", resign={"threshold": -0.9})


def test_batched_self_play_resigns():
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay(Stub(), B, n_playout=N, seed=SEED, board_id_base=BASE, max_plies=MAXP,
                         resign={"threshold": THRESHOLD, "consecutive": 1, "min_ply": 0, "p_playon": 0.0})
    moves = sp.run_move().cpu().numpy()
    st, rs = sp.engine.game_status(), sp.engine.resign_status()
    assert np.array_equal(st["over"] == 1, GROUP == 0) and np.array_equal(moves < 0, GROUP == 0)
    assert (rs["state"][GROUP == 0] == RESIGNED | 1).all() and sp.engine.resign_stats()["resigned_games"] == B // 4
    sp.engine.check_healthy()
