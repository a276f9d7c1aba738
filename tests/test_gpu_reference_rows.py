"""GPU: default-mode training rows against per-ply histories produced by the reference itself (tests/golden/reference_rows.*:
the reference's update_states_history snapshotted while its Game.start_self_play runs; tests/reference_rows.py assembles the
expectation). Every ply and every mirror row of every fixture game -- a red win, black wins, a sixty-move draw, a fourfold-repetition
draw, games past 256 plies -- through the three device paths that form rows, and through the host mirror:

  dense harvest   k_harvest                                  engine.harvest()
  records         k_harvest_records -> k_expand_records      engine.harvest_record_chunks() + expand_records()
  ring            k_ring_retire, k_sample_records            RecordReplayBuffer.append_records() + sample_at()

The games of one playout count share ONE engine (one board per game, its own salt), driven by the Lockstep harness with the fixture's
moves forced, trees reused and strict mode on: boards finish at different plies and a finished board waits for the harvest. The same
games are played a second time on a twin engine that is fed the same evaluator outputs, because a harvest consumes its games: one
engine is harvested densely, the other as records."""
import time

import numpy as np
import pytest
import torch

import reference_rows as R

pytestmark = pytest.mark.gpu
_, META = R.load()
GAMES = list(range(len(META["games"])))
# Games of one playout count share an engine (the harness runs the same number of simulations on every board). A game past 400 plies
# gets an engine of its own: the harness evaluates every board at every step, and four finished boards idling through its last 240
# plies doubled the test's time for nothing.
GROUPS = {}                                                # (playout count, long game or -1) -> games, in fixture order
for _g in GAMES:
    _m = META["games"][_g]
    GROUPS.setdefault((_m["n_playout"], _g if _m["plies"] > 400 else -1), []).append(_g)
GROUP_IDS = [f"{k[0]} playouts, game{'s' if len(v) > 1 else ''} {'-'.join(str(g) for g in sorted({v[0], v[-1]}))}" for k, v in sorted(GROUPS.items())]
_played = {}


class _Twin:
    """Two engines behind the calls of one: every call goes to both, the first one answers."""

    def __init__(self, a, b):
        self._a, self._b = a, b

    def __getattr__(self, name):
        x = getattr(self._a, name)
        if not callable(x):
            return x
        y = getattr(self._b, name)

        def both(*args, **kw):
            r = x(*args, **kw)
            y(*args, **kw)
            return r
        return both


def _play(group):
    """The group's games on twin engines, the search checked at every ply; returns what the two harvests gave (cached)."""
    if group in _played:
        return _played[group]
    n_playout = group[0]
    from gpu_harness import Lockstep
    from oracle import OracleBoard
    from chinesechesszero_amd.engine import SelfPlayEngine, expand_records
    t0 = time.perf_counter()
    games = GROUPS[group]
    fx = [R.game_arrays(g) for g in games]
    T = [META["games"][g]["plies"] for g in games]
    B = len(games)
    # max_plies bounds the recorded plies of a game and, x 80 sparse entries, its pi arena: sized for the longest game
    kw = dict(n_playout=n_playout, seed=1, reference_quirks=False, strict=True, max_plies=max(T) + 64)
    dense, compact = SelfPlayEngine(B, **kw), SelfPlayEngine(B, **kw)
    ls = Lockstep(_Twin(dense, compact), [OracleBoard() for _ in games], kind="hash_sharp", salts=[META["games"][g]["salt"] for g in games])
    for t in range(max(T)):
        ls.run_fused(n_playout, check_leaf=False)
        rc = ls.compare_roots()
        root_pi = dense.root_pi()                          # the engine's schedule: temperature 1.0 for 30 moves, then 0.5
        forced = []
        for b in range(B):
            if t >= T[b]:
                forced.append(-1)                          # finished: waits for the harvest
                continue
            k = int(rc["k"][b])
            acts, want = rc["acts"][b][:k].astype(int), fx[b]["pi"][t]
            assert np.count_nonzero(want) == np.count_nonzero(want[acts]), (games[b], t)        # no support outside the root's children
            assert np.allclose(root_pi[b][:k], want[acts], rtol=0, atol=1e-12), (games[b], t)
            forced.append(int(fx[b]["moves"][t]))
        ls.play(forced)
        over = dense.game_status()["over"]
        assert over.tolist() == [1 if t + 1 >= T[b] else 0 for b in range(B)], t                # the rules end each game at its last ply
    for e in (dense, compact):
        st = e.game_status()
        assert st["over"].tolist() == [1] * B and st["plies"].tolist() == T
        assert st["winner"].tolist() == [-1 if META["games"][g]["winner"] is None else int(META["games"][g]["winner"]) for g in games]
    flags = compact.record_flags()
    S, P, Z = dense.harvest()
    rec = torch.cat(list(compact.harvest_record_chunks(1 << 16)))
    s1, p1, z1 = expand_records(rec, flags)
    out = dict(games=games, T=T, flags=flags, records=rec.cpu(), dense=(S.cpu().numpy(), P.cpu().numpy(), Z.cpu().numpy()),
               expanded_is_dense=(torch.equal(s1, S), torch.equal(p1, P), torch.equal(z1, Z)),
               expanded=(s1.cpu().numpy(), p1.cpu().numpy(), z1.cpu().numpy()))
    dense.check_healthy()                                  # no CCZ_ERR_RECORD / CCZ_ERR_CHAIN / CCZ_ERR_TRUNCATED (strict) on either engine
    compact.check_healthy()
    out["seconds"] = time.perf_counter() - t0
    print(f"\n{n_playout} playouts, games {games}, {sum(T)} plies: played twice, harvested, expanded in {out['seconds']:.1f} s")
    _played[group] = out
    return out


def _per_game(rows, T):
    """(states, pi, z) of several games, game after game (T samples, T mirror images each) -> one triple per game."""
    lo = 0
    for t in T:
        yield tuple(x[lo:lo + 2 * t] for x in rows)
        lo += 2 * t
    assert lo == rows[0].shape[0]


@pytest.mark.parametrize("group", sorted(GROUPS), ids=GROUP_IDS)
def test_dense_harvest_equals_the_reference_rows_at_every_ply(group):
    """k_harvest: states and z equal, pi within 1e-6 of the reference's float64, all 2T rows of every game."""
    got = _play(group)
    worst = 0.0
    for g, rows in zip(got["games"], _per_game(got["dense"], got["T"])):
        dev = R.compare_rows(rows, R.expected_rows(g), pi_atol=1e-6, label=f"dense harvest, game {g}")
        print(f"game {g} ({META['games'][g]['plies']} plies): largest |pi - reference| = {dev:.3e}")
        worst = max(worst, dev)
    print(f"largest pi deviation of the dense harvest, {group[0]} playouts: {worst:.3e}")


@pytest.mark.parametrize("group", sorted(GROUPS), ids=GROUP_IDS)
def test_expanded_records_equal_the_dense_harvest_and_the_reference_rows(group):
    """k_harvest_records + k_expand_records on the twin engine: byte for byte the dense harvest, and the reference's rows."""
    got = _play(group)
    assert got["records"].shape == (sum(got["T"]), 880)
    assert got["expanded_is_dense"] == (True, True, True)
    for g, rows in zip(got["games"], _per_game(got["expanded"], got["T"])):
        R.compare_rows(rows, R.expected_rows(g), pi_atol=1e-6, label=f"expanded records, game {g}")


def test_record_ring_serves_the_reference_rows_while_it_wraps_inside_a_long_game():
    """Every game's records into a RecordReplayBuffer smaller than their sum: first while all appended games are still live, then after
    the window has wrapped inside the longest game and retired the earliest ones. sample_at over every live row, mirror passes included,
    equals the reference's rows of the games in the window; no record is refused."""
    from chinesechesszero_amd.replay import RecordReplayBuffer
    recs, flags = [], None
    for group in sorted(GROUPS):
        got = _play(group)
        flags = got["flags"]
        lo = 0
        for g, t in zip(got["games"], got["T"]):
            recs.append((g, t, got["records"][lo:lo + t]))
            lo += t
    recs.sort(key=lambda x: x[0])
    T = [t for _, t, _ in recs]
    longest, total = max(T), sum(T)
    assert longest > 256 and T[-1] == longest              # the last game appended is the long one: the ring wraps inside it
    max_game = longest + 17
    cap = 2 * max_game
    assert longest < cap < total
    ring = RecordReplayBuffer(cap, "cuda", flags=flags, max_game_plies=max_game)

    def check_window(first_live, head):
        tail = sum(T[:first_live])
        assert ring.window() == (tail, head)
        live = head - tail
        s, p, z = (x.cpu().numpy() for x in ring.sample_at(torch.arange(2 * live, device="cuda", dtype=torch.int64)))
        lo = 0
        for g, t, _ in recs[first_live:]:
            if lo >= live:
                break
            rows = tuple(np.concatenate((x[2 * lo:2 * (lo + t):2], x[2 * lo + 1:2 * (lo + t):2])) for x in (s, p, z))   # row r: ply r // 2, pass r % 2
            R.compare_rows(rows, R.expected_rows(g), pi_atol=1e-6, label=f"ring window ({tail}, {head}), game {g}")
            lo += t
        assert lo == live
        assert int(ring.bad.item()) == 0

    # (1) as many games as fit, appended game by game: nothing retired yet, every one of them is served
    fit = max(i for i in range(1, len(T) + 1) if sum(T[:i]) <= cap)
    assert fit >= 3
    for _, _, r in recs[:fit]:
        ring.append_records(r.cuda(), flags)
    check_window(0, sum(T[:fit]))
    # (2) the rest in ONE append: the window wraps around the physical end inside the longest game and moves past whole games
    ring.append_records(torch.cat([r for _, _, r in recs[fit:]]).cuda(), flags)
    first_live = min(i for i in range(len(T)) if total - sum(T[:i]) <= cap)
    assert first_live >= 1 and sum(T[:-1]) < cap < total   # an earlier game is gone; slot `cap` lies inside the last game
    check_window(first_live, total)


def _policy(salt, scale):
    from oracle.evaluators import hash_eval

    def policy(board, red_states=None, black_states=None):
        ids = board.legal_ids()
        p, v = hash_eval(board.squares()[None, :], np.array([1 if board.turn else 0]), salt=salt, scale=scale)
        return zip(ids, p[0][ids]), np.array([[v[0]]], dtype=np.float32)

    return policy


@pytest.mark.parametrize("g", GAMES)
def test_host_mirror_reproduces_the_reference_rows_at_every_ply(g, tmp_path):
    """game.Game(reference_quirks=False) + mcts.MCTS_AI under the fixture's policy and seed, then CollectPipeline.preprocess and
    flip_data: the same moves, and all 2T rows equal to the reference's -- states and z exactly, pi bit for bit in float64."""
    from chinesechesszero_amd.collect import CollectPipeline
    from chinesechesszero_amd.game import Game
    from chinesechesszero_amd.mcts import MCTS_AI
    m, a = META["games"][g], R.game_arrays(g)
    player = MCTS_AI(_policy(m["salt"], m["scale"]), c_puct=5, n_playout=m["n_playout"], is_selfplay=True)
    game = Game(reference_quirks=False)
    np.random.seed(m["seed"])
    play_data = game.start_self_play(player, is_shown=False, temp=1.0, game_index=7)
    assert [mv.id for mv in game.board.move_stack] == a["moves"].tolist()
    o = game.board.outcome()
    assert game.board.is_game_over() and o.winner is m["winner"]
    if m["winner"] is None:
        assert getattr(game.board, "is_" + m["termination"])()
    cp = CollectPipeline(init_model=None, n_boards=1, data_dir=str(tmp_path), reference_quirks=False)
    rows = cp.flip_data(cp.preprocess(play_data))
    assert len(rows) == 2 * m["plies"]
    z = np.array([r[2] for r in rows])
    assert z.dtype == np.float64 and np.array_equal(z, np.concatenate((a["z"], a["z"])))
    R.compare_rows((np.stack([np.asarray(r[0]) for r in rows]), np.stack([r[1] for r in rows]), z.astype(np.float32)), R.expected_rows(g),
                   label=f"host mirror, game {g}")
