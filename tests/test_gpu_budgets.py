"""GPU: per-board simulation budgets (ccz_set_budgets / ccz_draw_budgets, include/cczero.h), the flag they leave in the game
records (CCZ_REC_FAST, ccz_expand_record_targets / ccz_sample_record_targets), playout-cap randomisation in BatchedSelfPlay and
playout odds in the arena. Everything here is exact: a board with budget n is, bit for bit, the same board of an engine that runs
n lockstep steps, and the draws are those of a host twin of the device's Philox stream."""
import functools

import numpy as np
import pytest
import torch

from budget_twin import twin_budgets as _twin_budgets, ua as _ua
from chinesechesszero_amd import _lib

pytestmark = pytest.mark.gpu

B, N_FULL, N_FAST, SEED, BASE = 32, 24, 6, 5, 640
MOVES = 3
MIXED = np.where(np.arange(B) % 2 == 0, N_FAST, N_FULL).astype(np.int32)


def _engine(n_playout, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    kw.setdefault("max_plies", MOVES)
    return SelfPlayEngine(B, n_playout=n_playout, seed=SEED, board_id_base=BASE, **kw)


def _run(e, n_steps, before_move=None):
    """MOVES moves with tree reuse (Dirichlet noise on, uniform evaluator), ``n_steps`` lockstep steps each, then one more search
    whose finish_move adjudicates every game at the ply cap, and the harvest. ``before_move(e)`` runs in front of every move's
    first selection."""
    from chinesechesszero_amd.net import uniform_evaluator
    out = {"roots": [], "moves": [], "status": [], "visits0": []}
    for _ in range(MOVES + 1):
        if before_move is not None:
            before_move(e)
        out["visits0"].append(e.root_children()["root_visits"])
        leaf = e.select_leaves()
        sts = []
        for i in range(n_steps):
            sts.append(e.leaf_info()["status"].copy())       # the leaf pending for simulation i of the move
            prob, value = uniform_evaluator(leaf)
            if i + 1 < n_steps:
                leaf = e.step(prob, value)
            else:
                e.expand_backup(prob, value)
        out["status"].append(np.stack(sts))
        out["roots"].append(e.root_children())
        out["moves"].append(e.finish_move().cpu().numpy().copy())
    assert e.game_status()["over"].all() and (out["moves"][-1] == -1).all()
    rec = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
    assert rec.shape == (B * MOVES, 880)
    out["records"] = rec.reshape(B, MOVES, 880)              # boards are harvested in index order, MOVES plies each
    out["sims"] = e.stats()["sims"]
    e.check_healthy()
    return out


@functools.lru_cache(maxsize=None)
def _uniform(n):
    return _run(_engine(n), n)


@functools.lru_cache(maxsize=None)
def _mixed():
    e = _engine(N_FULL)
    e.set_budgets(MIXED)
    return _run(e, N_FULL)


def _same_board(a, b, boards):
    for mv in range(MOVES + 1):
        ra, rb = a["roots"][mv], b["roots"][mv]
        for key in ("k", "acts", "visits", "root_visits"):
            assert np.array_equal(ra[key][boards], rb[key][boards]), (mv, key)
        for key in ("q", "prior"):
            assert np.array_equal(ra[key][boards].view(np.uint32), rb[key][boards].view(np.uint32)), (mv, key)
        assert np.array_equal(a["moves"][mv][boards], b["moves"][mv][boards]), mv
    assert np.array_equal(a["records"][boards], b["records"][boards])


def test_budgets_at_the_full_count_change_nothing():
    """Engine A never hears of budgets; engine B has budget 24 on every board; engine C draws its budgets with p_full = 1."""
    a = _uniform(N_FULL)
    eb = _engine(N_FULL)
    eb.set_budgets(np.full(B, N_FULL, np.int32))
    b = _run(eb, N_FULL)
    drawn = []
    c = _run(_engine(N_FULL), N_FULL, before_move=lambda e: drawn.append(e.draw_budgets(N_FULL, N_FAST, 1.0).cpu().numpy().copy()))
    every = np.arange(B)
    _same_board(a, b, every)
    _same_board(a, c, every)
    assert all((d == N_FULL).all() for d in drawn) and len(drawn) == MOVES + 1
    assert a["sims"] == b["sims"] == c["sims"] == B * N_FULL * (MOVES + 1)
    assert (a["records"][:, :, _lib.REC_FLAGS] == 0).all()               # budgets off: the flags byte is the 0 it always was
    assert (b["records"][:, :, _lib.REC_FLAGS] == 0).all() and (c["records"][:, :, _lib.REC_FLAGS] == 0).all()
    assert (np.stack(a["moves"][:MOVES]) >= 0).all()


def test_a_board_with_budget_n_is_the_board_of_an_engine_that_runs_n_steps():
    """Even boards budget 6, odd boards 24, 24 lockstep steps per move: every even board equals the same board of a uniform
    6-step engine, every odd board that of the uniform 24-step engine (same seed, same board_id_base)."""
    m, lo, hi = _mixed(), _uniform(N_FAST), _uniform(N_FULL)
    even, odd = np.arange(0, B, 2), np.arange(1, B, 2)
    _same_board(m, lo, even)
    _same_board(m, hi, odd)
    for mv in range(MOVES + 1):
        st = m["status"][mv]                                             # [step, board]
        assert (st[N_FAST:, even] == _lib.LEAF_SKIP).all()               # CCZ_LEAF_NONE: no leaf, no evaluator row
        assert (st[:N_FAST, even] != _lib.LEAF_SKIP).all() and (st[:, odd] != _lib.LEAF_SKIP).all()
        assert np.array_equal(m["roots"][mv]["root_visits"], m["visits0"][mv] + MIXED)   # kept visits + exactly the budget
    assert np.array_equal(m["roots"][0]["root_visits"], MIXED) and (m["visits0"][0] == 0).all()
    assert m["sims"] == int(MIXED.sum()) * (MOVES + 1)
    assert not np.array_equal(lo["records"][odd], hi["records"][odd])    # (the two uniform engines do differ)


def test_the_planned_boundary_plans_no_row_for_a_board_that_is_done():
    """The mixed run through the evaluation cache with a real net: from step 6 on only the 16 odd boards can miss, and what the
    tree is handed (ccz_leaf_priors) and the trees are those of the uncached mixed run."""
    from chinesechesszero_amd.net import PolicyValueNet
    torch.manual_seed(11)
    pvn = PolicyValueNet(device="cuda:0", num_channels=256, resblocks_num=1)
    ev = pvn.evaluate_leaves_logits
    cached, plain = _engine(N_FULL, eval_cache_log2=12, max_plies=0), _engine(N_FULL, max_plies=0)
    for e in (cached, plain):
        e.set_budgets(MIXED)
    even = np.arange(0, B, 2)
    for mv in range(MOVES):
        leaf, pleaf = cached.select_leaves(), plain.select_leaves()
        for i in range(N_FULL):
            rows, n = cached.eval_plan()
            n_miss = int(n.item())
            assert n_miss <= (B if i < N_FAST else B // 2), (mv, i, n_miss)
            lg, v = ev(leaf, plan=(rows, n))
            cached.gather_priors_planned(lg, v)
            pri, val = cached.leaf_priors()
            plg, pv = ev(pleaf)
            plain.gather_priors(plg, pv)
            want, _ = plain.leaf_priors(values=False)
            info, pinfo = cached.leaf_info(), plain.leaf_info()
            assert np.array_equal(info["status"], pinfo["status"]) and np.array_equal(info["k"], pinfo["k"])
            if i >= N_FAST:
                assert (info["status"][even] == _lib.LEAF_SKIP).all()
            live = np.flatnonzero(info["status"] == _lib.LEAF_EXPAND)
            assert len(live) > 0
            for b in live:
                k = int(info["k"][b])
                assert np.array_equal(pri[b, :k].view(np.uint32), want[b, :k].view(np.uint32)), (mv, i, b)
            assert np.array_equal(val[live].view(np.uint32), pv.cpu().numpy()[live].view(np.uint32)), (mv, i)
            if i + 1 < N_FULL:
                leaf, pleaf = cached.step_compact(None), plain.step_compact(pv)
            else:
                cached.expand_backup_compact(None)
                plain.expand_backup_compact(pv)
        ra, rb = cached.root_children(), plain.root_children()
        for key in ("k", "acts", "visits", "root_visits"):
            assert np.array_equal(ra[key], rb[key]), (mv, key)
        for key in ("q", "prior"):
            assert np.array_equal(ra[key].view(np.uint32), rb[key].view(np.uint32)), (mv, key)
        assert np.array_equal(cached.finish_move().cpu().numpy(), plain.finish_move().cpu().numpy())
    assert cached.stats()["sims"] == plain.stats()["sims"] == int(MIXED.sum()) * MOVES
    cached.check_healthy()
    plain.check_healthy()


# ---------------------------------------------------------------------- the draws
def test_the_draws_are_the_host_twins():
    from chinesechesszero_amd.engine import SelfPlayEngine
    from chinesechesszero_amd.net import uniform_evaluator
    n, seed, base = 64, 9, 1000
    e = SelfPlayEngine(n, n_playout=N_FULL, seed=seed, board_id_base=base)
    for played in range(3):                                               # the draws of move counters 0, 1 and 2
        want = _twin_budgets(seed, base, n, played, N_FULL, N_FAST, 0.25)
        assert np.array_equal(e.draw_budgets(N_FULL, N_FAST, 0.25).cpu().numpy(), want), played
        assert 0 < (want == N_FULL).sum() < n                             # a mix of full and fast moves
        if played == 2:
            break
        kept = e.root_children()["root_visits"]
        leaf = e.select_leaves()
        for i in range(N_FULL):
            prob, value = uniform_evaluator(leaf)
            if i + 1 < N_FULL:
                leaf = e.step(prob, value)
            else:
                e.expand_backup(prob, value)
        assert np.array_equal(e.root_children()["root_visits"], kept + want)   # and they are what the boards then search
        e.finish_move()
    assert int(e.stats()["moves"]) == 2 * n
    assert (e.draw_budgets(N_FULL, N_FAST, 0.0).cpu().numpy() == N_FAST).all()
    assert (e.draw_budgets(N_FULL, N_FAST, 1.0).cpu().numpy() == N_FULL).all()
    for bad in ((0, 6, 0.5), (24, 0, 0.5), (24, 6, 1.5), (24, 6, float("nan"))):
        with pytest.raises(_lib.CczError, match="ccz_draw_budgets"):
            e.draw_budgets(*bad)
    e.check_healthy()


def test_budgets_and_scout_slots_exclude_each_other():
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(4, n_playout=8, eval_cache_log2=10)
    e.set_scouts(2)
    with pytest.raises(_lib.CczError, match="scout"):
        e.set_budgets(np.full(4, 3, np.int32))
    with pytest.raises(_lib.CczError, match="scout"):
        e.draw_budgets(8, 3, 0.5)
    e.set_scouts(0)
    e.set_budgets(np.full(4, 3, np.int32), np.ones(4, np.uint8))
    with pytest.raises(_lib.CczError, match="budgets"):
        e.set_scouts(2)
    e.set_budgets(None)                                                   # off again: scouts are welcome
    e.set_scouts(2)
    with pytest.raises(ValueError):
        SelfPlayEngine(4, n_playout=8).set_budgets(np.ones(3, np.int32))


# ---------------------------------------------------------------------- the flag, end to end
CAP_B, CAP_N, CAP_FAST, CAP_P, CAP_SEED, CAP_BASE, CAP_PLIES = 16, 8, 3, 0.5, 13, 77, 12


@functools.lru_cache(maxsize=None)
def _capped_records():
    from chinesechesszero_amd.net import uniform_evaluator
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay(uniform_evaluator, CAP_B, n_playout=CAP_N, seed=CAP_SEED, board_id_base=CAP_BASE, max_plies=CAP_PLIES,
                         playout_cap=(CAP_FAST, CAP_P))
    visits = []
    for _ in range(CAP_PLIES + 1):
        sp.search()
        visits.append((sp.engine.game_status()["over"].copy(), sp.engine.root_children()["root_visits"]))
        sp.finish_move()
    assert sp.engine.game_status()["over"].all()
    rec = torch.cat(list(sp.engine.harvest_record_chunks()))
    sp.engine.check_healthy()
    return rec, sp.engine.record_flags(), visits


def _header(rec):
    r = rec.cpu().numpy()
    t = r[:, 96:98].copy().view(np.uint16).ravel().astype(np.int64)
    T = r[:, 98:100].copy().view(np.uint16).ravel().astype(np.int64)
    board = r[:, 104:108].copy().view(np.uint32).ravel().astype(np.int64)
    return t, T, board, r[:, _lib.REC_FLAGS].astype(np.int64)


def _row_targets(rec, mul):
    """The expected target byte of every dense row of a buffer of whole games: game at record f, T plies -> the sample of ply t
    at row mul * f + t, its mirror image at mul * f + T + t."""
    t, T, _, fl = _header(rec)
    p = np.arange(len(t))
    want = np.full(len(t) * mul, 255, np.uint8)
    for q in range(mul):
        want[mul * (p - t) + q * T + t] = 1 - (fl & 1)
    assert (want != 255).all()
    return want


def test_fast_plies_are_flagged_in_the_records_and_in_the_rows_formed_from_them():
    from chinesechesszero_amd.engine import expand_record_targets, expand_records
    from chinesechesszero_amd.replay import RecordReplayBuffer, ReplayBuffer
    rec, flags, visits = _capped_records()
    t, T, board, fl = _header(rec)
    assert len(t) > CAP_B and set(np.unique(fl)) == {0, 1}
    # a fresh engine's first game: ply t of a board is the move its counter t drew
    want = np.array([0 if _ua(CAP_SEED, int(b), int(p)) < CAP_P else _lib.REC_FAST for b, p in zip(board, t)])
    assert np.array_equal(fl, want)
    first = _twin_budgets(CAP_SEED, CAP_BASE, CAP_B, 0, CAP_N, CAP_FAST, CAP_P)
    assert np.array_equal(visits[0][1], first)                           # and the search was the one the flag stands for
    mul = 2
    rows = _row_targets(rec, mul)
    got = expand_record_targets(rec.contiguous(), flags)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), rows)
    assert 0 < rows.sum() < len(rows)
    # a cut game: its rows are 0, everybody else's stay
    cut = rec[:-1].contiguous()
    last = len(t) - int(T[-1])
    got = expand_record_targets(cut, flags).cpu().numpy()
    assert len(got) == mul * (len(t) - 1) and np.array_equal(got[:mul * last], rows[:mul * last]) and (got[mul * last:] == 0).all()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    expand_records(cut, flags, bad=bad)
    assert int(bad.item()) == int(T[-1]) - 1                             # (the same records ccz_expand_records refuses)
    # the dense ring keeps the byte next to the row it belongs to
    rb = ReplayBuffer(mul * len(t) + 5, "cuda")
    rb.append_records(rec, flags)
    assert np.array_equal(rb.targets[:mul * len(t)].cpu().numpy(), rows) and (rb.targets[mul * len(t):] == 1).all()
    # the record ring, wrapped: every live row's byte is its ply's, for the sample and for the mirror image
    cap = 2 * CAP_PLIES + 5
    ring = RecordReplayBuffer(cap, "cuda", flags, None, max_game_plies=CAP_PLIES)
    p = 0
    while p < len(t):
        ring.append_records(rec[p:p + int(T[p])])
        p += int(T[p])
    tail, head = ring.window()
    assert head == len(t) > cap and 0 < head - tail <= cap
    live = (head - tail) * mul
    draws = torch.arange(3 * live, device="cuda")
    s, pi, z, tg = ring.sample_at(draws, targets=True)
    r = np.arange(3 * live) % live
    slot = (tail + r // mul) % cap
    assert np.array_equal(tg.cpu().numpy(), 1 - (ring.records[:, _lib.REC_FLAGS].cpu().numpy()[slot] & 1))
    assert np.array_equal(tg.cpu().numpy(), 1 - (fl[tail + r // mul] & 1))
    assert int(ring.bad.item()) == 0 and 0 < int(tg.sum()) < 3 * live
    assert len(ring.sample_at(draws[:4])) == 3 and len(ring.sample(8, targets=True)) == 4 and len(ring.sample(8)) == 3
    tg = ring.sample_at(torch.tensor([0, -1, 1], device="cuda"), targets=True)[3].cpu().numpy()
    assert tg[1] == 0 and int(ring.bad.item()) == 1                       # a bad draw is no target


def test_the_sink_stores_the_flags_of_a_capped_run(tmp_path):
    from chinesechesszero_amd.collect import TupleSink
    rec, flags, _ = _capped_records()
    s = TupleSink(str(tmp_path))
    s.append_records(rec, flags, games=CAP_B)
    assert s.finalize() == 2 * rec.shape[0]
    assert np.array_equal(np.load(tmp_path / "policy_targets.npy"), _row_targets(rec, 2))
    s.close()
    plain = TupleSink(str(tmp_path / "plain"))
    r = rec.clone()
    r[:, _lib.REC_FLAGS] = 0
    plain.append_records(r, flags, games=CAP_B)
    assert plain.finalize() == 2 * rec.shape[0] and not (tmp_path / "plain" / "policy_targets.npy").exists()
    plain.close()


# ---------------------------------------------------------------------- playout odds in the arena
def _arena(**kw):
    from test_gpu_eval_cache import LogitsEvaluator
    from chinesechesszero_amd.arena import Arena
    dev = torch.device("cuda", 0)
    return Arena(LogitsEvaluator(dev, seed=4), LogitsEvaluator(dev, seed=4), 4, opening_plies=4, seed=2, max_plies=10, eval_cache_log2=12, **kw)


def test_arena_odds_give_each_side_its_own_budget():
    ar = _arena(n_playout=N_FAST, n_playout_b=N_FULL)
    assert ar.n_steps == N_FULL
    moves = 0
    while not ar.engine.game_status()["over"].all():
        st = ar.engine.game_status()
        a_to_move = (st["turn"] == 1) == (np.arange(ar.B) % 2 == 0)      # A plays red on the even boards
        want = np.where(a_to_move, N_FAST, N_FULL)
        assert np.array_equal(ar.move_budgets(), want)
        ar.search()
        rv = ar.engine.root_children()["root_visits"]
        live = st["over"] == 0
        assert np.array_equal(rv[live], want[live])
        ar.finish_move()
        moves += 1
    assert moves >= 10
    r = ar.result()
    assert r["n_playout"] == N_FAST and r["n_playout_b"] == N_FULL
    ar.engine.check_healthy()


def test_arena_without_odds_plays_the_moves_it_always_played():
    """``n_playout_b=None`` is the arena as it was: it runs ``n_playout`` steps and never touches the engine's budgets (they stay off, the
    state every engine had before budgets existed). And budgets switched on at that same count play the same moves, so the two paths
    cannot drift apart unnoticed."""
    plain = _arena(n_playout=N_FAST)

    def no_budgets(*a, **kw):
        raise AssertionError("the arena without odds set budgets")
    plain.engine.set_budgets = no_budgets
    assert plain.n_steps == N_FAST
    even = _arena(n_playout=N_FAST, n_playout_b=N_FAST)                  # budgets on, at the count the loop runs anyway
    ra, rb = plain.play(), even.play()
    assert len(plain.moves) == len(even.moves) and all(np.array_equal(x, y) for x, y in zip(plain.moves, even.moves))
    assert ra["n_playout_b"] == rb["n_playout_b"] == N_FAST and plain.n_playout_b is None
    for k in ("wins", "draws", "losses", "truncated", "steps", "rows_per_step"):
        assert ra[k] == rb[k], k
