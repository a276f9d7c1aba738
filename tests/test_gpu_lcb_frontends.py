"""GPU: the LCB move in the front ends (``lcb=`` of Arena, BatchedMatch, BatchedAnalysis, MCTS / MCTS_AI; the UCI option). The move each
front end plays is the move assembled by hand from the same search: root children and S read back, the rule of
tests/value_spread_model.py applied on the CPU. Every test asserts that the LCB move does depart from the most visited move somewhere:
a run in which it never does shows nothing."""
import io

import numpy as np
import pytest
import torch

import value_spread_model as vsm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z0 = {"z": 0.0, "min_visit_ratio": 0.0, "min_visits": 0}          # the highest-Q child with two visits: far from the arg-max move
SALT = 9


def _hash_dense(leaf):
    """The hash evaluator on every row of the leaf planes: dense priors and values on the device."""
    from gpu_harness import planes_to_squares
    from oracle.evaluators import hash_eval
    sq, turn = planes_to_squares(leaf.float().cpu().numpy())
    p, v = hash_eval(sq, np.asarray(turn).astype(np.int64), salt=SALT, scale=40.0)
    return torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(leaf.device), torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1)).to(leaf.device)


def _by_hand(e, cfg):
    """(LCB move, arg-max child's move, LCB child, arg-max child) per board from what the engine shows of its roots; -1 on finished boards."""
    rc, vs, over = e.root_children(), e.root_value_stats(), e.game_status()["over"]
    out = np.full((e.B, 4), -1, np.int64)
    for b in range(e.B):
        k = int(rc["k"][b])
        if over[b] or k == 0:
            continue
        N, Q, S = rc["visits"][b][:k], rc["q"][b][:k], vs["S"][b][:k]
        ci, _ = vsm.lcb_choice(N, Q, S, cfg["z"], cfg["min_visit_ratio"], cfg["min_visits"])
        star = vsm.first_max_visits(N)
        out[b] = (rc["acts"][b][ci], rc["acts"][b][star], ci, star) if ci >= 0 else -1
    return out


def test_batched_match_plays_the_move_assembled_by_hand():
    from chinesechesszero_amd.match import BatchedMatch
    m = BatchedMatch(_hash_dense, _hash_dense, 3, n_playout=96, seed=2, max_plies=6, lcb=Z0)
    assert m.lcb == Z0 and m.engine.get_value_stats()
    want, seen = [], {"plies": 0, "filled": 0, "departed": 0}

    def before(match):
        want.append(_by_hand(match.engine, Z0))

    def after(match, moves):
        w = want[-1]
        moves = np.asarray(moves)
        filled = w[:, 0] >= 0
        live = filled & (moves >= 0)            # (at the ply cap the game is adjudicated INSTEAD of a move: the forced move is not played)
        assert np.array_equal(moves[live], w[live, 0]), (seen["plies"], moves, w)
        assert match.engine.game_status()["over"][filled & ~live].all()
        seen["plies"] += int(live.sum())
        seen["filled"] += int(filled.sum())
        seen["departed"] += int((w[filled, 2] != w[filled, 3]).sum())
    m.play(before_move=before, on_move=after)
    assert seen["plies"] >= 12 and seen["departed"] > 0
    assert m.options.lcb_counts == {"moves": seen["filled"], "differed": seen["departed"]}


def test_arena_plays_it_for_the_side_that_has_it():
    from test_gpu_arena import _logits_evaluators
    from chinesechesszero_amd.arena import Arena
    ev = _logits_evaluators([3, 3])
    ar = Arena(ev[0], ev[1], 2, n_playout=128, opening_plies=2, seed=4, max_plies=8, eval_cache_log2=12, lcb=Z0, lcb_side="a")
    seen = {"a": 0, "b": 0, "departed": 0}
    want = []

    def before(arena):
        want.append((_by_hand(arena.engine, Z0), (arena._turn == arena.a_colour).copy(), arena.engine.root_children()))
    while not ar.engine.game_status()["over"].all():
        moves = ar.play_move(before_move=before)
        w, a_moves, rc = want[-1]
        for b in range(ar.B):
            if w[b, 0] < 0:
                continue
            if a_moves[b]:
                assert moves[b] == w[b, 0] or (moves[b] < 0 and ar.engine.game_status()["over"][b]), (b, moves[b], w[b])   # (-1: adjudicated at the ply cap instead)
                seen["a"] += 1
                seen["departed"] += int(w[b, 2] != w[b, 3])
            elif moves[b] >= 0:                  # B's side: a most visited move, as without the option (temperature 1e-3)
                k = int(rc["k"][b])
                i = int(np.nonzero(rc["acts"][b][:k] == moves[b])[0][0])
                assert rc["visits"][b][i] == rc["visits"][b][:k].max(), b
                seen["b"] += 1
    r = ar.result()
    assert seen["a"] > 0 and seen["b"] > 0 and seen["departed"] > 0
    assert r["lcb"] == dict(Z0, side="a", a={"moves": seen["a"], "differed": seen["departed"]})
    with pytest.raises(ValueError, match="lcb_side"):
        Arena(ev[0], ev[1], 2, n_playout=8, lcb_side="a")


def test_a_proven_root_overrides_lcb():
    """mate_in_two with the solver: once the root is proven the move is the proof's, whatever the bounds say."""
    import solver_cases as sc
    from chinesechesszero_amd.match import BatchedMatch
    from chinesechesszero_amd.options import lcb_moves, proven_moves
    _, sq, turn, *_ = sc.CASES[sc.NAMES.index("mate_in_two")]
    m = BatchedMatch(_hash_dense, _hash_dense, 2, n_playout=256, seed=2, max_plies=4, solver=True, lcb=Z0)
    e = m.engine
    e.set_position(0, np.asarray(sq, np.uint8).copy(), int(turn), 0)
    from chinesechesszero_amd.boundary import deliver, kind_of
    from chinesechesszero_amd.options import search_move
    search_move(e, 256, lambda leaf, last: deliver(e, kind_of(_hash_dense), *_hash_dense(leaf), last), m._poll)
    forced, proven = proven_moves(e, True)
    assert proven >= 1 and forced[0] >= 0
    hand = _by_hand(e, Z0)
    got, _ = lcb_moves(e, Z0, forced.copy())
    assert got[0] == forced[0] and got[1] == hand[1, 0]          # board 0: the proof's move stays; board 1 (not proven): the LCB move
    assert proven == 2 or forced[1] == -1


def _ai(lcb, n=96):
    from test_gpu_frontends_parity import _hash_policy
    from chinesechesszero_amd.mcts import MCTS_AI
    ai = MCTS_AI(_hash_policy(SALT), c_puct=5, n_playout=n, is_selfplay=False, scouts=0, lcb=lcb)
    ai.mcts.use_graph = False
    return ai


def test_mcts_ai_plays_the_lcb_move():
    from chinesechesszero_amd.game import Board
    board = Board()
    ai = _ai(Z0)
    acts, probs = ai.mcts.get_move_probs(board)
    want = ai.mcts.lcb_move()
    hand = _by_hand(ai.mcts._engine, Z0)
    assert want == hand[0, 0] and hand[0, 2] != hand[0, 3]       # ... and it is not the most visited move
    assert _ai(Z0).get_action(Board()) == want
    assert _ai(None).mcts.lcb_move() is None
    plain = _ai(None).get_action(Board())
    assert plain == hand[0, 1] and plain != want


def test_the_uci_option_changes_bestmove():
    from test_gpu_frontends_parity import _hash_policy
    from chinesechesszero_amd.uci import UciLoop
    best, infos = {}, {}
    for lcb in (False, True):
        out = io.StringIO()
        loop = UciLoop(policy_value_fn=_hash_policy(SALT), n_playout=96, out=out)
        script = ["uci", "ucinewgame"] + (["setoption name LCB value true", "setoption name LCBStdevs value 0", "setoption name LCBMinVisitRatio value 0"] if lcb else [])
        for line in script + ["position startpos", "go nodes 96"]:
            assert loop.handle(line)
        text = out.getvalue().splitlines()
        best[lcb] = [l for l in text if l.startswith("bestmove ")]
        infos[lcb] = [l for l in text if l.startswith("info depth ")]
        assert len(best[lcb]) == 1 and "option name LCB type check default false" in text
    assert best[True] != best[False]                              # the scripted position is one where they differ
    assert infos[True] == infos[False]                            # the info lines stay as they are


def test_analysis_records_carry_stdev_and_lcb():
    import math
    from chinesechesszero_amd.analyse import BatchedAnalysis
    import oracle
    uci = oracle.move_table()
    cfg = {"z": 1.0, "min_visit_ratio": 0.0, "min_visits": 0}
    an = BatchedAnalysis(_hash_dense, 2, n_playout=64, multipv=4, max_len=4, lcb=cfg)
    recs = an.analyse(["startpos", "startpos moves h2e2 h9g7"])
    e = an.engine
    rc, vs = e.root_children(), e.root_value_stats()
    hand = _by_hand(e, cfg)
    plain = BatchedAnalysis(_hash_dense, 2, n_playout=64, multipv=4, max_len=4).analyse(["startpos", "startpos moves h2e2 h9g7"])
    departed = 0
    for b, (r, p) in enumerate(zip(recs, plain)):
        assert r["status"] == "ok" and r["bestmove"] == uci[int(hand[b, 0])]
        assert [l["moves"] for l in r["lines"]] == [l["moves"] for l in p["lines"]]          # ranked by visits, as without the option
        assert "stdev" not in p["lines"][0] and p["bestmove"] == p["lines"][0]["moves"][0]
        departed += int(r["bestmove"] != p["bestmove"])
        acts = [uci[int(a)] for a in rc["acts"][b][:rc["k"][b]]]
        for l in r["lines"]:
            i = acts.index(l["moves"][0])
            n, s, q = int(rc["visits"][b][i]), float(vs["S"][b][i]), float(rc["q"][b][i])
            if n < 2:
                assert l["stdev"] is None and l["lcb"] is None
            else:
                sd = math.sqrt(max(s, 0.0) / (n - 1))
                assert l["stdev"] == sd and l["lcb"] == q - 1.0 * math.sqrt(max(s, 0.0) / (n - 1) / n)
    assert departed > 0
