"""CPU: the combined self-play model (tests/selfplay_model.py) that tests/test_gpu_selfplay_all_options.py compares the engine with.

1. The new wide fixture is what the GPU test needs: more than 64 legal moves, exactly one that ends the game, at a child index >= 64,
   nothing else decided within 2 plies -- certified with ``solver_model.negamax``.
2. Every interaction the GPU comparison is about occurs in the model's run on the GPU test's inputs (the fact table), so that the
   comparison cannot pass vacuously; and each interaction, stated wrongly, gives other records or roots on these inputs.
3. With one feature on, the model is that feature's own model; with everything off it is ``oracle.OracleMCTS``."""
import numpy as np
import pytest

import explore_model as em
import resign_model as rm
import selfplay_model as spm
import solver_cases as sc
import solver_model as sm
from budget_twin import ua
from oracle import OracleBoard, OracleMCTS

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- the wide fixture
def test_the_wide_fixture_has_one_mating_move_in_the_second_pass_and_nothing_else_decided():
    sq, turn = spm.inputs()[spm.WIDE]
    b = OracleBoard.from_array(sq, turn)
    ids = b.legal_ids()
    assert len(ids) == 105 > 64
    ends = []
    for i, mv in enumerate(ids):
        c = b.copy()
        c.push_id(mv)
        byte = sm.negamax(c, 1)                                   # the child's position within 1 ply: 2 plies from the root
        if c.is_game_over() or c.is_tie():
            ends.append(i)
            assert byte == sm.pack(sm.LOSS, 0)
        else:
            assert byte == 0, (i, byte)
    assert ends == [67]
    assert sm.negamax(b, 0) == 0 and sm.negamax(b, 1) == sm.pack(sm.WIN, 1) == sm.certify(b)


# ---------------------------------------------------------------------------------------------------------------- the fact table
def test_inputs_are_what_the_gpu_test_says():
    boards = spm.boards()
    assert len(boards) == spm.B == 16
    assert [tuple(x.squares()) for x in boards[:7]] == [tuple(x.squares()) for x in sc.boards()]
    ks = [len(x.legal_ids()) for x in boards]
    assert all(30 <= k <= 50 for k in ks[7:14]) and ks[14] == 7 and ks[spm.WIDE] == 105
    assert spm.N_FAST < spm.N_FULL <= em.SIMS_NARROW and spm.MOVES == 3 and spm.RULE.consecutive == 2 and spm.RULE.min_ply == 0


def test_the_models_run_shows_every_interaction():
    m, moves = spm.dense_run()
    f = m.xfacts
    assert f["forced_on_proven"] >= 1                    # forced selections whose chosen child was already proven
    assert f["pruned_at_proven_root"] >= 1               # explored moves with visits_pruned > 0 at a root with a proven child
    assert len(f["root_proven_at_boundary"]) >= 2 and len(f["proofs_after_reroot"]) >= 2
    assert f["fast_with_proofs"] >= 1                    # fast moves (target byte 0) on a board with nodes_proven > 0
    assert f["resign"] >= 1 and f["playon"] >= 1 and f["below_no_fire"] >= 1
    assert f["skip_while_proving"] >= 1                  # a budget-exhausted board in a step where another board proves a node
    # the wide board: WIN in 1, proven by child 67 alone, and a later descent of the same move stops at that child
    st, ds, cs, cd = moves[0]["proofs"][spm.WIDE]
    assert (st, ds) == (sm.WIN, 1) and np.nonzero(cs)[0].tolist() == [67] and (cs[67], cd[67]) == (sm.LOSS, 0)
    steps = [s[spm.WIDE] for s in moves[0]["steps"]]
    first = next(i for i, s in enumerate(steps) if s[0] == sm.LEAF_LOSS and s[2] == 1)      # the mate itself: decided by the rules
    assert steps[first][1] == 0 and any(s == (sm.LEAF_LOSS, 0, 1) for s in steps[first + 1:])
    assert (spm.WIDE, 0, 67) in f["stops_d1"] and moves[0]["targets"][spm.WIDE] == 1
    # budgets: fast and full moves on every ply, LEAF_SKIP after the budget
    for mv in moves:
        assert 0 < sum(t == 0 for t in mv["targets"]) < spm.B
        for b in range(spm.B):
            n = sum(s[b][0] != spm.LEAF_SKIP for s in mv["steps"])
            assert n == (mv["budgets"][b] if mv["live"][b] else 0)
    assert m.sims == sum(mv["budgets"][b] for mv in moves for b in range(spm.B) if mv["live"][b])
    ev = [e for mv in moves for e in mv["events"]]
    assert "resign" in ev and "playon" in ev and m.records().shape[0] >= spm.B
    st = m.resign_stats()
    assert st["resigned_games"] == f["resign"] and st["playon_games"] == f["playon"]


@pytest.mark.parametrize("wrong", spm.WRONG)
def test_each_interaction_stated_wrongly_gives_other_records_or_roots(wrong):
    m, moves = spm.dense_run()
    w, wmoves = spm.dense_run(wrong)
    same_roots = all(np.array_equal(x, y) for a, c in zip(moves, wmoves) for b in range(spm.B) for x, y in zip(a["roots"][b], c["roots"][b]))
    r, rw = m.records(), w.records()
    same_records = r.shape == rw.shape and np.array_equal(r, rw)
    assert not (same_roots and same_records)
    if wrong == "resign_on_pruned_counts":               # the search is the same: only what the boundary decides and records differs
        assert same_roots and not same_records
    if wrong == "reroot_drops_proof":
        assert any(not np.array_equal(a["proofs"][b][2], c["proofs"][b][2]) for a, c in zip(moves[1:], wmoves[1:]) for b in range(spm.B))


# ---------------------------------------------------------------------------------------------------------------- reductions
def test_with_only_exploration_on_it_is_the_exploration_model():
    boards, _, sims = em.inputs()
    want = em.run_case(0.25, 2.0, True)
    m = spm.SelfPlayModel(boards, em.SALTS, em.SEED, em.BASE, explore=em.FULL)
    for mv in want["moves"]:
        m.begin_move(budgets=sims)
        m.search(max(sims))
        for b in range(em.B):
            if not mv["live"][b]:
                continue
            for x, y in zip(m.root_children(b), mv["roots"][b]):
                assert np.array_equal(x, y) and x.tobytes() == y.tobytes(), b
            assert m.noise(b).tobytes() == mv["noise"][b].tobytes(), b
        m.finish_move()
        for b in range(em.B):
            if mv["finish"][b] is not None:
                assert m.last[b]["move"] == mv["finish"][b]["move"] and m.last[b]["pi"].tobytes() == mv["finish"][b]["pi"].tobytes(), b
                assert np.array_equal(m.last[b]["pruned"], mv["finish"][b]["pruned"])
    assert m.totals() == want["stats"] and want["stats"]["forced_selections"] > 0 and want["stats"]["visits_pruned"] > 0
    assert m.solver_stats() == {"nodes_proven": 0, "proven_stops": 0, "roots_proven": 0}


def test_with_only_the_solver_on_it_is_the_solver_model():
    want = sm.SolverModel(sc.boards(), sc.SALTS)
    m = spm.SelfPlayModel(sc.boards(), sc.SALTS, 5, solver=True)
    m.begin_move()
    for _ in range(sc.SIMS):
        assert m.step() == [want.simulate(b) for b in range(len(sc.CASES))]
    for b in range(len(sc.CASES)):
        for x, y in zip(m.root_children(b), want.root_children(b)):
            assert x.tobytes() == y.tobytes(), sc.NAMES[b]
        for x, y in zip(m.root_proof(b), want.root_proof(b)):
            assert np.array_equal(x, y), sc.NAMES[b]
        assert m.proof_move(b) == want.proof_move(b)
    assert m.solver_stats() == want.stats() and want.proven_stops > 0 and (m.rows, m.sims) == (want.rows, want.sims)
    assert m.totals()["forced_selections"] == 0 and all(g.values == [] for g in m.games)


def test_with_everything_off_it_is_the_oracles_search():
    boards = spm.boards()
    pick = [1, 8, 14, spm.WIDE]
    m = spm.SelfPlayModel([boards[b] for b in pick], [spm.SALT] * len(pick), spm.SEED, spm.BASE)
    n1, n2 = 130, 40
    m.begin_move()
    m.search(n1)
    forced = []
    for j, b in enumerate(pick):
        o = OracleMCTS(lambda brd, ids: (em.evaluate(spm.SALTS, 0, brd)[0][ids], em.evaluate(spm.SALTS, 0, brd)[1]), c_puct=5, n_playout=0)
        board = boards[b].copy()
        for _ in range(n1):
            o.playout(board)
        first = o.root_children()
        for x, y in zip(m.root_children(j), first):
            assert x.tobytes() == np.asarray(y).astype(x.dtype).tobytes(), b
        mv = int(first[0][int(np.argmax(first[1]))])
        forced.append(mv)
        o.update_with_move(mv)
        board.push_id(mv)
        for _ in range(n2):
            o.playout(board)
        forced[-1] = (mv, o.root_children())
    assert m.finish_move(forced=[f[0] for f in forced]) == [None] * len(pick)
    m.begin_move()
    m.search(n2)
    for j, b in enumerate(pick):
        for x, y in zip(m.root_children(j), forced[j][1]):
            assert x.tobytes() == np.asarray(y).astype(x.dtype).tobytes(), b
        assert np.array_equal(m.last[j]["pruned"], m.last[j]["visits"]) and not m.last[j]["explored"]
    assert m.solver_stats() == {"nodes_proven": 0, "proven_stops": 0, "roots_proven": 0} and m.totals()["explored_moves"] == 0


def test_with_only_resignation_and_budgets_on_the_events_are_the_resignation_models():
    rule = rm.Rule(-0.01, 1, 0, 0.5)
    cap = (48, 12, 0.6)
    m = spm.SelfPlayModel(spm.boards(), spm.SALTS, spm.SEED, spm.BASE, resign=rule, cap=cap, max_plies=4)
    games = [rm.Game(rule) for _ in range(spm.B)]
    seen = set()
    for mv in range(4):
        budgets = m.begin_move()
        m.search(cap[0])
        want = []
        for b in range(spm.B):
            if m.over[b]:
                want.append("over")
                continue
            _, N, Q, _ = m.root_children(b)
            full = ua(spm.SEED, spm.BASE + b, mv) < cap[2]
            assert budgets[b] == (cap[0] if full else cap[1]) and m.roots[b].N - (1 if mv == 0 else 0) >= budgets[b] - 1
            want.append(games[b].record(int(m.boards[b].turn), rm.root_value64(N, Q), int(full), False, ua(spm.SEED, spm.BASE + b, mv, 0xffd)))
        got = m.finish_move()
        assert got == want, mv
        seen |= set(got)
        for b in range(spm.B):
            if m.over[b] and not games[b].over:
                games[b].end(m.games[b].winner)
            assert games[b].status()["state"] == m.games[b].status()["state"] and games[b].flags() == m.games[b].flags()
            assert rm.same_f32(np.array([v for v in games[b].values], F32), np.array([v for v in m.games[b].values], F32))
    assert {"resign", "playon", None} <= seen
    assert m.finish_move().count("cap") > 0
    for g in games:
        if not g.over:
            g.end(-1)
    rec = m.records()
    assert rec.shape[0] == sum(g.plies for g in m.games) and set(np.unique(rec[:, spm.HDR + 7] & 1)) == {0, 1}
    assert m.resign_stats() == rm.stats_of(games)
