"""GPU: the wide search (include/cczero.h "Wide search") where tests/test_gpu_wide_search.py does not reach -- widths above 16, nodes
of more than 64 children, kept trees and the engine's limits -- against the sequential NumPy model of tests/wide_model.py, exactly:
visit counts, Q and prior bits, slot status, k, depth, ids, positions and counters. Nothing here takes a tolerance.

Inputs (wide_model.limit_inputs, A = 4 searched boards, an engine of 4 * W slots): the start position, "widest" (108 legal moves),
WIDE_PAIR of tests/engine_limit_cases.py (100 moves, 67 in reply) and "two_rooks" (one ply from mate). The limit cases put ONE faulty
board (board 0) among three clean ones (wide_model.pool_inputs / depth_inputs / nan_inputs). tests/test_cpu_wide_model.py asserts on
the model alone, without a GPU, every condition relied on here, and that each rule stated wrongly changes the result on these inputs.

Launch forms. Widths 17 .. 64 all run k_wide<16>: 1024 threads, 16 waves; the tail loop gives a wave the slots w, w + 16, ... -- 1..2
slots at width 24, 2 at 32, 4 at 64 -- in ONE SelectShared block, and s_depth / s_undo are indexed up to 63. Widths 8 and 16 run
k_wide<8> / k_wide<16> with a wave per slot. Planned (evaluation cache, ccz_eval_plan / ccz_gather_priors_planned, engine-owned leaf
values) is what WideSearch chooses from 65 slots on; unplanned hands the whole batch to ccz_gather_priors. The limit cases override
one board's evaluator rows and therefore run unplanned.

The evaluator is the integer projection of wide_model.make_torch_evaluator; the model is fed what ccz_leaf_priors / ccz_leaf_info
report per slot, so what is judged is the search, not the evaluator."""
import functools

import numpy as np
import pytest

import wide_model as wm
from chinesechesszero_amd import _lib
from test_gpu_wide_search import SEED, Twin, _evaluator

pytestmark = pytest.mark.gpu


def _all_slots_none(e):
    info = e.leaf_info()
    return bool((info["status"] == wm.NONE).all() and (info["k"] == 0).all() and (info["depth"] == 0).all())


def _end_of_search(t, budgets):
    """Roots bit for bit, the wide counters, the simulation counts, nothing in flight."""
    m, e = t.model, t.e
    t.compare_roots()
    ws, st = e.wide_stats(), e.stats()
    assert ws == {"steps": m.board_steps, "leaves": m.leaves, "collisions": m.collisions, "inflight_now": 0}
    assert m.sims == list(budgets) and st["sims"] == sum(budgets) and m.inflight() == 0
    assert st["terminal_leaves"] == m.terminal_leaves == sum(sum(tr.terminal_visits.values()) for tr in m.trees)
    return st


# ---------------------------------------------------------------------------------------------------- a. widths above 16
@pytest.mark.parametrize("W,planned", [(24, True), (32, True), (64, True), (64, False)])
def test_widths_above_sixteen_grow_the_models_tree_step_by_step(W, planned):
    """k_wide<16> with several slots per wave, and the second 64-lane pass of wide_descend: a selected child of index >= 64, and the
    h0 / h1 vote on a maximum attained on both sides of index 64."""
    t = Twin(W, wm.limit_inputs(), wm.LIMIT_BUDGETS, planned=planned, max_nodes=wm.LIMIT_MAX_NODES).run()
    cond = wm.limit_conditions(t.model)
    assert all(cond.values()), cond             # the MODEL saw all of them: a silent no-op cannot pass
    _end_of_search(t, wm.LIMIT_BUDGETS)
    t.e.check_healthy()


# ---------------------------------------------------------------------------------------------------- b. kept trees
@pytest.mark.parametrize("W", wm.KEPT_WIDTHS)
def test_three_moves_on_kept_trees(W):
    """ccz_finish_move(keep_tree) under a width: k_wide_drop in front of the re-root into the other pool half, F in that half, the
    per-move budget counting from zero and a search that goes on on kept visits; then a board mated by its last move."""
    B = [wm.KEPT_BUDGET] * 4
    t = Twin(W, wm.limit_inputs(), B, max_nodes=wm.LIMIT_MAX_NODES)
    m, e = t.model, t.e
    for mv in range(wm.KEPT_MOVES):
        if mv == 0:                             # the first boundary is crossed mid-search, with leaves pending
            e.select_wide()
            for _ in range(wm.KEPT_FIRST_STEPS):
                assert t.compare_selection().any()
                t.step()
            assert t.compare_selection().any()
            assert e.wide_stats()["inflight_now"] == m.inflight() > 0 and max(m.sims) < wm.KEPT_BUDGET
        else:
            t.run()
            assert m.sims == B and e.wide_stats()["inflight_now"] == 0
        last = mv == wm.KEPT_MOVES - 1
        t.finish_move(wm.kept_forced(m, t.roots, last))
        # ---- before any step: the re-rooted trees, nothing in flight, every slot empty, the budget counts from zero
        assert e.wide_stats()["inflight_now"] == 0 and m.inflight() == 0 and m.sims == [0] * 4
        rc = t.compare_roots()
        assert [int(n) for n in rc["root_visits"][:3]] == [tr.N[0] for tr in m.trees[:3]]
        assert _all_slots_none(e)
        assert np.array_equal(e.root_positions()[:4], np.stack([r.squares() for r in t.roots]))
    # ---- board 3 was mated by its last move: it selects nothing; the others search their budget on their kept trees
    over = e.game_status()["over"][:4]
    assert over.tolist() == [0, 0, 0, 1] and t.roots[3].is_game_over()
    e.select_wide()
    nl = t.compare_selection()
    assert nl[3] == 0 and nl[:3].all() and (e.leaf_info()["status"][3::4] == wm.NONE).all()
    t.step()
    t.run(select=False)
    assert m.sims == B[:3] + [0]
    t.compare_roots()
    st = e.stats()
    assert st["pruned_subtrees"] == 0 and e.wide_stats()["inflight_now"] == 0
    e.check_healthy()


# ---------------------------------------------------------------------------------------------------- c. the front end that keeps trees
def test_mcts_at_width_eight_over_three_plies_equals_the_driven_engine():
    """MCTS (mcts.py) is the one front end that crosses move boundaries with keep_tree under a width: get_move_probs /
    update_with_move three times against an engine driven by hand (Twin: no WideSearch), same seed, same evaluator."""
    from chinesechesszero_amd.game import Board, Move
    from chinesechesszero_amd.mcts import MCTS
    from chinesechesszero_amd.tools import softmax
    from oracle import OracleBoard
    n = 32
    mcts = MCTS(_evaluator(), c_puct=5, n_playout=n, seed=SEED, width=8)
    mcts.use_graph = False
    board = Board()
    t = Twin(8, [(OracleBoard().squares().copy(), 1)], [n], planned=False, check_leaves=False, engine_kw=dict(mirror=True, strict=True))
    for ply in range(3):
        acts, probs = mcts.get_move_probs(board, temp=1e-3)
        t.run()
        rc = t.compare_roots()
        k = int(rc["k"][0])
        assert acts == tuple(int(a) for a in rc["acts"][0][:k]), ply
        got = mcts.root_children()
        for key in ("visits", "q", "prior"):
            assert np.array_equal(got[key].view(np.uint32), rc[key][0][:k].view(np.uint32)), (ply, key)
        assert got["root_visits"] == rc["root_visits"][0] == t.model.trees[0].N[0]
        want = softmax(1.0 / 1e-3 * np.log(rc["visits"][0][:k].astype(np.int64) + 1e-10))
        assert np.array_equal(probs, want), ply
        move = t.model.most_visited(0)
        assert move == acts[int(np.argmax(probs))]
        mcts.update_with_move(move)
        board.push(Move.from_id(move))
        t.finish_move([move])
        assert mcts._engine.wide_stats()["inflight_now"] == t.e.wide_stats()["inflight_now"] == 0
    assert mcts._engine.stats()["sims"] == t.e.stats()["sims"] == 3 * n
    assert t.model.trees[0].N[0] > 0                # the last re-root kept visits: the trees compared above were kept ones
    mcts._engine.check_healthy()
    t.e.check_healthy()


# ---------------------------------------------------------------------------------------------------- d, e, f. the limits
CASES = {
    "pool": dict(W=wm.POOL_W, inputs=wm.pool_inputs, budgets=wm.POOL_BUDGETS, bit=1, word="node pool", kw=dict(max_nodes=wm.POOL_MAX_NODES)),
    "depth": dict(W=wm.DEPTH_W, inputs=wm.depth_inputs, budgets=wm.DEPTH_BUDGETS, bit=2, word="max_depth",
                  kw=dict(max_nodes=wm.LIMIT_MAX_NODES, max_depth=wm.DEPTH_MAX_DEPTH, overrides=wm.DEPTH_OVERRIDES)),
    "nan": dict(W=wm.NAN_W, inputs=wm.nan_inputs, budgets=wm.NAN_BUDGETS, bit=32, word="NaN",
                kw=dict(max_nodes=wm.LIMIT_MAX_NODES, overrides=wm.NAN_OVERRIDES)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's engine driven step by step next to the model until nothing is selected (shared by d/e/f and g; not changed after)."""
    c = CASES[name]
    return Twin(c["W"], c["inputs"](), c["budgets"], planned=False, **c["kw"]).run(max_steps=400)


def _clean_boards_and_flags(t, c):
    m, e = t.model, t.e
    t.compare_roots()                           # the faulty board's tree and the clean boards', bit for bit
    st, ws = e.stats(), e.wide_stats()
    assert st["error_flags"] == c["bit"] == m.error_flags()
    assert ws == {"steps": m.board_steps, "leaves": m.leaves, "collisions": m.collisions, "inflight_now": 0} and m.inflight() == 0
    assert m.sims[1:] == list(c["budgets"][1:]) and st["sims"] == sum(m.sims)
    assert _all_slots_none(e)
    with pytest.raises(_lib.CczError, match=c["word"]):
        e.check_healthy()


def test_node_pool_refuses_a_slot_and_a_later_slot_still_fits():
    """Phase A chains the node count through the slots of one step: a slot whose k children do not fit is refused
    (CCZ_ERR_NODE_POOL), a later slot with fewer children still fits; the refused leaf's value is backed up, its simulation counts,
    and it is selected again."""
    c, t = CASES["pool"], _case("pool")
    m = t.model
    assert m.refused[0] > 0 and m.refused[1:] == [0, 0, 0] and m.fit_after_refusal >= 1 and m.refused_again >= 1
    assert m.sims[0] == c["budgets"][0]         # the faulty board uses its whole budget
    assert m.trees[0].n_nodes() <= wm.POOL_MAX_NODES
    _clean_boards_and_flags(t, c)


def test_depth_limit_ends_a_batch_and_keeps_its_earlier_slots():
    """CCZ_ERR_DEPTH in wide_descend: the slot gets nothing and the batch ends; the slots selected before it stay selected and are
    backed up; the next selection finds the same line and selects nothing (t == 0): the board ends below its budget."""
    c, t = CASES["depth"], _case("depth")
    m = t.model
    assert m.depth_stops[0] >= 2 and m.depth_stops[1:] == [0, 0, 0] and m.stops_after_leaves >= 1 and m.empty_steps_after_stop == 1
    assert 0 < m.sims[0] < c["budgets"][0]
    _clean_boards_and_flags(t, c)


def test_nan_priors_end_the_batch_once_every_root_child_was_visited():
    """CCZ_ERR_NAN in wide_descend. An unvisited child scores +inf whatever its prior (cczero.h: "score_i = +inf if Ne == 0"), so the
    root's k children are visited once each, k + 1 simulations; every descent after that finds k NaN scores."""
    c, t = CASES["nan"], _case("nan")
    m = t.model
    rc = t.e.root_children()
    k = int(rc["k"][0])
    assert k == 44 and np.isnan(rc["prior"][0][:k]).all() and rc["visits"][0][:k].tolist() == [1] * k
    assert m.nan_stops[0] >= 1 and m.nan_stops[1:] == [0, 0, 0] and m.sims[0] == k + 1 < c["budgets"][0]
    assert m.stops_after_leaves + m.empty_steps_after_stop == m.nan_stops[0] and m.empty_steps_after_stop == 1
    _clean_boards_and_flags(t, c)


# ---------------------------------------------------------------------------------------------------- g. the host loop ends
@pytest.mark.parametrize("name", list(CASES))
def test_the_host_loop_ends_under_an_error_flag(name):
    """WideSearch.search() loops until no board selected a leaf: with a board stopped by a limit that rests on the kernel reporting
    t == 0 for it. ``on_step`` raises a few steps past the model's count, so a regression fails instead of spinning."""
    from chinesechesszero_amd.wide import WideSearch
    c, t = CASES[name], _case(name)
    kw = dict(c["kw"])
    A, ev = t.A, _evaluator()
    if kw.get("overrides"):
        ev = wm.with_overrides(ev, A, kw.pop("overrides"))
    ws = WideSearch(ev, A, c["W"], n_playout=max(c["budgets"]), planned=False, eval_cache_log2=0, seed=SEED, eps=0.0, **kw)
    e = ws.engine
    for r, (sq, turn) in enumerate(c["inputs"]()):
        e.set_position(r, sq, turn)
    # search() gives every board n_playout simulations; the case's budgets are per board: they replace the uniform ones on their way
    # to the engine (the loop under test is untouched)
    set_budgets = e.set_budgets
    e.set_budgets = lambda _uniform: set_budgets(np.array(list(c["budgets"]) + [1] * (e.B - A), np.int32))
    cap, seen = t.steps + 3, []

    def on_step(nl):
        seen.append(nl.copy())
        if len(seen) > cap:
            raise AssertionError(f"search() is at step {len(seen)}: the model ends after {t.steps}")

    assert ws.search(on_step=on_step) == t.steps == len(seen)
    assert not e.n_leaves().any() and e.wide_stats()["inflight_now"] == 0
    ra, rb = e.root_children(), t.e.root_children()
    assert all(np.array_equal(ra[key][:A].view(np.uint8), rb[key][:A].view(np.uint8)) for key in ra)
    assert e.stats()["error_flags"] == c["bit"]
    with pytest.raises(_lib.CczError, match=c["word"]):
        e.check_healthy()
