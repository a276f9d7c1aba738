"""GPU: the wide search (ccz_set_width / ccz_select_wide / ccz_step_wide, include/cczero.h "Wide search") -- several leaves of one
tree per step, kept apart by virtual loss -- against the sequential NumPy model of tests/wide_model.py, step by step.

The evaluator is a fixed integer projection of the leaf planes (wide_model.make_torch_evaluator): a row's logits are exact whatever
the batch, so the planned and the unplanned boundary must grow the same trees. The model is fed what ccz_leaf_priors / ccz_leaf_info
report per slot; what it selects is checked against the rules oracle (position, legal ids, status) and the engine's slots.

Width 1 through ccz_select_wide / ccz_step_wide is refused (the sequential calls ARE that search; F does not exist): test 1 has two
engines, not three."""
import functools
import io

import numpy as np
import pytest
import torch

import wide_model as wm
from chinesechesszero_amd import _lib
from gpu_harness import planes_to_squares
from oracle import OracleBoard

pytestmark = pytest.mark.gpu

MAX_NODES, CACHE_LOG2, SEED = 8192, 12, 11


def _engine(n_boards, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    kw.setdefault("max_nodes", MAX_NODES)
    kw.setdefault("eval_cache_log2", CACHE_LOG2)
    kw.setdefault("seed", SEED)
    kw.setdefault("eps", 0.0)
    return SelfPlayEngine(n_boards, n_playout=64, **kw)


@functools.lru_cache(maxsize=None)
def _evaluator():
    return wm.make_torch_evaluator(torch.device("cuda", 0))


class Twin:
    """A wide engine next to the model. ``inputs``: [(squares, turn)] of the A searched boards; ``budgets`` [A] or None.
    ``max_nodes`` / ``max_depth``: the engine's limits, which the model is told as ccz_create derives them; ``overrides``: {board:
    an evaluator override of wide_model.override_rows} (unplanned only); ``model_kw`` / ``engine_kw``: further arguments of both."""

    def __init__(self, W, inputs, budgets, planned=True, check_leaves=True, max_nodes=None, max_depth=None, overrides=None, model_kw=None,
                 engine_kw=None):
        self.A, self.W, self.planned, self.check_leaves = len(inputs), W, planned, check_leaves
        limits = {k: v for k, v in (("max_nodes", max_nodes), ("max_depth", max_depth)) if v is not None}
        self.e = e = _engine(self.A * W, eval_cache_log2=CACHE_LOG2 if planned else 0, **limits, **(engine_kw or {}))
        for r, (sq, turn) in enumerate(inputs):
            e.set_position(r, sq, turn)
        e.set_width(W)
        self.budgets = None if budgets is None else list(budgets)
        if budgets is not None:
            e.set_budgets(np.array(list(budgets) + [1] * (e.B - self.A), np.int32))
        self.roots = [OracleBoard.from_array(sq, turn) for sq, turn in inputs]
        if max_nodes is not None:
            limits["max_nodes"] = max(130, max_nodes)       # (Dev.cap: root + one full expansion at the least)
        self.model = wm.WideModel(self.A, W, c_puct=5.0, budgets=self.budgets, **limits, **(model_kw or {}))
        self.keys = {}          # position bytes -> leaf key: one key per position, one position per key
        self.ev = _evaluator()
        if overrides:
            assert not planned, "an override cannot go through the plan"
            self.ev = wm.with_overrides(self.ev, self.A, overrides)
        self.steps = 0

    # what the engine's slots hold after a selection, against what the model selects
    def compare_selection(self):
        e, A, W = self.e, self.A, self.W
        nl = e.n_leaves()
        info = e.leaf_info()
        keys = e.leaf_keys()[0].cpu().numpy()
        planes = e.leaf_input.float().cpu().numpy() if self.check_leaves else None
        over = e.game_status()["over"]
        for r in range(A):
            got = self.model.select(r, over=bool(over[r]))
            assert nl[r] == len(got), (self.steps, r, nl[r], got)
            for j in range(W):
                s = r + j * A
                if j not in got:
                    assert (info["status"][s], info["k"][s], info["depth"][s]) == (wm.NONE, 0, 0), (self.steps, r, j)
                    continue
                moves = self.model.moves_of(r, j)
                assert info["depth"][s] == len(moves), (self.steps, r, j, info["depth"][s], moves)
                if not self.check_leaves:
                    continue
                leaf = wm.leaf_board(self.roots[r], moves)
                ids = leaf.legal_ids()
                end, tie = leaf.is_game_over(), leaf.is_tie()
                want = wm.EXPAND if (not end and not tie) else (wm.DRAW if (end and tie) else wm.LOSS)
                assert info["status"][s] == want, (self.steps, r, j, info["status"][s], want)
                assert info["k"][s] == len(ids) and info["ids"][s][:len(ids)].tolist() == ids, (self.steps, r, j)
                sq, turn = planes_to_squares(planes[s:s + 1])
                assert np.array_equal(sq[0], leaf.squares()) and int(turn[0]) == int(leaf.turn), (self.steps, r, j)
                pos = bytes(leaf.squares().tobytes()) + bytes([int(leaf.turn)])
                assert self.keys.setdefault(pos, int(keys[s])) == int(keys[s]), "one position, two keys"
        if self.check_leaves:
            assert len(set(self.keys.values())) == len(self.keys), "two positions, one key"
        return nl

    # evaluate the pending slots, feed the model what the engine will back up, step both
    def step(self, engine_step=True):
        e, A, W = self.e, self.A, self.W
        info = e.leaf_info()
        if self.planned:
            logits, value = self.ev(e.leaf_input, plan=e.eval_plan())
            e.gather_priors_planned(logits, value)
            pri, val = e.leaf_priors(values=True)
            vdev = None
        else:
            logits, vdev = self.ev(e.leaf_input)
            e.gather_priors(logits, vdev)
            pri, _ = e.leaf_priors(values=False)
            val = vdev.cpu().numpy()
        for r in range(A):
            feed = {}
            for j in range(W):
                s = r + j * A
                if self.model.pending[r][j] is not None:
                    k = int(info["k"][s])
                    feed[j] = {"status": int(info["status"][s]), "ids": info["ids"][s][:k].tolist(), "priors": pri[s][:k], "value": val[s]}
            self.model.backup(r, feed)
        if engine_step:
            e.step_wide(vdev)
            self.steps += 1

    def run(self, max_steps=200, select=True):
        """A whole search: select (unless the slots hold a selection already), then (evaluate, step) until nothing is selected."""
        if select:
            self.e.select_wide()
        for _ in range(max_steps):
            if not self.compare_selection().any():
                return self
            self.step()
        raise AssertionError("the search did not end")

    def finish_move(self, forced):
        """The move boundary with keep_tree: ``forced`` [A] move ids, on the engine, the model and the rules oracle."""
        f = np.full(self.e.B, -1, np.int32)
        f[:self.A] = forced
        assert np.array_equal(self.e.finish_move(forced_moves=f, keep_tree=True).cpu().numpy()[:self.A], f[:self.A])
        for r in range(self.A):
            self.model.reroot(r, int(forced[r]))
            self.roots[r].push_id(int(forced[r]))

    def compare_roots(self):
        rc = self.e.root_children()
        over = self.e.game_status()["over"]
        for r in range(self.A):
            if over[r]:
                continue    # a finished board has no live tree (its pool half is recycled by the flip)
            acts, n, q, p = self.model.trees[r].root_children()
            k = len(acts)
            assert rc["k"][r] == k, (r, rc["k"][r], k)
            assert np.array_equal(rc["acts"][r][:k], acts), r
            assert np.array_equal(rc["visits"][r][:k], n), (r, rc["visits"][r][:k], n)
            assert np.array_equal(rc["q"][r][:k].view(np.uint32), q.view(np.uint32)), r
            assert np.array_equal(rc["prior"][r][:k].view(np.uint32), p.view(np.uint32)), r
            assert rc["root_visits"][r] == self.model.trees[r].N[0], r
        return rc


# ---------------------------------------------------------------------------------------------------- 1. width 1 is today's search
def test_width_one_is_the_sequential_search_bit_for_bit():
    """Two engines with one seed, 4 boards, 3 moves x 64 simulations on the compact boundary: one never hears of the feature, the
    other is told ccz_set_width(1) before every move. Leaf info at every step, root children (acts, N, Q, P) and visits before
    every move, the moves played, the root positions and the counters are equal bit for bit; nothing wide is allocated."""
    ev = _evaluator()
    B = 4
    a, b = _engine(B, eval_cache_log2=0, eps=0.25), _engine(B, eval_cache_log2=0, eps=0.25)
    for _ in range(3):
        b.set_width(1)
        la, lb = a.select_leaves(), b.select_leaves()
        for i in range(64):
            ia, ib = a.leaf_info(), b.leaf_info()
            for key in ia:
                assert np.array_equal(ia[key], ib[key]), (i, key)
            assert torch.equal(la, lb)
            (lga, va), (lgb, vb) = ev(la), ev(lb)
            a.gather_priors(lga, va)
            b.gather_priors(lgb, vb)
            if i + 1 < 64:
                la, lb = a.step_compact(va), b.step_compact(vb)
            else:
                a.expand_backup_compact(va)
                b.expand_backup_compact(vb)
        ra, rb = a.root_children(), b.root_children()
        for key in ra:
            assert np.array_equal(ra[key].view(np.uint8), rb[key].view(np.uint8)), key
        assert ra["root_visits"].min() >= 64
        assert torch.equal(a.finish_move(), b.finish_move())
        assert np.array_equal(a.root_positions(), b.root_positions())
    sa, sb = a.stats(), b.stats()
    assert {k: v for k, v in sa.items() if k != "hbm_bytes"} == {k: v for k, v in sb.items() if k != "hbm_bytes"}
    assert sa["hbm_bytes"] == sb["hbm_bytes"] and sa["sims"] == 3 * 64 * B          # width 1 allocates nothing
    assert b.wide_stats() == {"steps": 0, "leaves": 0, "collisions": 0, "inflight_now": 0}
    a.check_healthy()
    b.check_healthy()


# ---------------------------------------------------------------------------------------------------- 2. the sequential model
@pytest.mark.parametrize("W", [2, 5, 16])
def test_the_engine_grows_the_models_tree_step_by_step(W):
    t = Twin(W, wm.model_inputs(), wm.BUDGETS).run()
    m, e = t.model, t.e
    cond = wm.conditions(m)
    assert all(cond.values()), cond             # the MODEL saw all of them: a silent no-op cannot pass
    t.compare_roots()
    ws, st = e.wide_stats(), e.stats()
    assert ws == {"steps": m.board_steps, "leaves": m.leaves, "collisions": m.collisions, "inflight_now": 0}
    assert m.sims == list(wm.BUDGETS) and st["sims"] == sum(wm.BUDGETS) and m.inflight() == 0
    assert st["terminal_leaves"] == sum(sum(tr.terminal_visits.values()) for tr in m.trees)
    e.check_healthy()


# ---------------------------------------------------------------------------------------------------- 3. shared rows
def test_planned_boundary_with_the_cache_equals_the_unplanned_one_at_width_eight():
    """Two boards with the SAME position: their slots reach one position in one step, so the plan shares rows
    (cache_shared_rows > 0). The trees of the planned run equal those of the unplanned run (ccz_gather_priors), and the model's."""
    start = (OracleBoard().squares().copy(), 1)
    runs = [Twin(8, [start, start], (48, 48), planned=p, check_leaves=False).run() for p in (True, False)]
    rcs = [t.compare_roots() for t in runs]
    for key in rcs[0]:
        assert np.array_equal(rcs[0][key][:2].view(np.uint8), rcs[1][key][:2].view(np.uint8)), key
    assert np.array_equal(rcs[0]["visits"][0], rcs[0]["visits"][1])                  # (equal positions, equal trees)
    sp, su = runs[0].e.stats(), runs[1].e.stats()
    assert sp["cache_shared_rows"] > 0 and su["cache_probes"] == 0
    assert sp["sims"] == su["sims"] == 96 and runs[0].steps == runs[1].steps
    pv = [t.e.principal_variations(1, 8) for t in runs]
    assert np.array_equal(pv[0]["moves"][:2], pv[1]["moves"][:2]) and np.array_equal(pv[0]["visits"][:2], pv[1]["visits"][:2])
    for t in runs:
        t.e.check_healthy()


# ---------------------------------------------------------------------------------------------------- 4. in-flight hygiene
def _pending_twin(W=8):
    """Three boards in the middle of a search: leaves pending, F > 0."""
    t = Twin(W, wm.model_inputs(), (40, 40, 40), check_leaves=False)
    t.e.select_wide()
    for _ in range(3):
        assert t.compare_selection().any()
        t.step()
    assert t.compare_selection().any()
    assert t.e.wide_stats()["inflight_now"] == t.model.inflight() > 0
    return t


def _search_again(t):
    """The search that follows a move boundary equals the model started with F = 0."""
    assert t.e.wide_stats()["inflight_now"] == 0 and t.model.inflight() == 0
    info = t.e.leaf_info()
    assert (info["status"] == wm.NONE).all() and (info["k"] == 0).all()
    t.run()
    t.compare_roots()
    assert t.e.wide_stats()["inflight_now"] == 0
    t.e.check_healthy()


def test_nothing_is_in_flight_after_a_finished_search():
    t = Twin(8, wm.model_inputs(), (24, 24, 24), check_leaves=False).run()
    assert t.e.wide_stats()["inflight_now"] == 0 and t.e.stats()["sims"] == 72


def test_finish_move_with_leaves_pending_empties_the_counts():
    t = _pending_twin()
    rc = t.e.root_children()
    forced = np.full(t.e.B, -1, np.int32)
    forced[:3] = [rc["acts"][r][0] for r in range(3)]
    assert np.array_equal(t.e.finish_move(forced_moves=forced, keep_tree=False).cpu().numpy()[:3], forced[:3])
    for r in range(3):
        t.model.drop(r, new_tree=True)
        t.roots[r].push_id(int(forced[r]))
    t.check_leaves = True
    _search_again(t)


def test_reset_tree_with_leaves_pending_empties_the_counts():
    t = _pending_twin()
    t.e.reset_tree(mask=np.array([1, 0, 1] + [0] * (t.e.B - 3), np.uint8))
    assert t.e.wide_stats()["inflight_now"] == sum(t.model.trees[1].F)     # board 1 was not masked: its leaves stay pending
    t.model.drop(0, new_tree=True)
    t.model.drop(2, new_tree=True)
    t.step()                                                                # board 1 goes on where it was; 0 and 2 had nothing pending
    t.run(select=False)
    t.compare_roots()
    assert t.e.wide_stats()["inflight_now"] == 0
    t.e.check_healthy()


def test_set_positions_with_leaves_pending_empties_the_counts():
    t = _pending_twin()
    inputs = wm.model_inputs()[::-1]
    S = t.e.B
    sq = np.zeros((S, 90), np.uint8)
    turn = np.ones(S, np.uint8)
    for r, (s, tn) in enumerate(inputs):
        sq[r], turn[r] = s, tn
    assert (t.e.set_positions(sq, turn, park=np.arange(S) >= 3) == 0).all()
    t.roots = [OracleBoard.from_array(s, tn) for s, tn in inputs]
    for r in range(3):
        t.model.drop(r, new_tree=True)
    t.check_leaves = True
    _search_again(t)


# ---------------------------------------------------------------------------------------------------- 5. refusals
def _refused(call, *needles):
    with pytest.raises(_lib.CczError) as ei:
        call()
    text = str(ei.value)
    assert all(n in text for n in needles), (text, needles)


def test_excluded_combinations_are_refused_both_ways_and_leave_everything_as_it_was():
    ev = _evaluator()
    e = _engine(8)
    # ---- the width itself
    _refused(lambda: e.set_width(0), "ccz_set_width", "1 .. 64")
    _refused(lambda: e.set_width(65), "ccz_set_width", "1 .. 64")
    _refused(lambda: e.set_width(3), "ccz_set_width", "does not divide")
    _refused(lambda: _lib.check(e.L.ccz_select_wide(e.h, e._stream(), None, None)), "ccz_select_wide", "ccz_set_width")
    _refused(lambda: _lib.check(e.L.ccz_step_wide(e.h, e._stream(), None, None, None)), "ccz_step_wide", "ccz_set_width")
    # ---- an option is on: the width is refused, naming the option's call; the option stays on, the width 1
    options = [("ccz_set_scouts", lambda on: e.set_scouts(2 if on else 0)),
               ("ccz_set_root_exploration", lambda on: e.set_root_exploration(0.25) if on else _lib.check(
                   e.L.ccz_set_root_exploration(e.h, e._stream(), 0, 0.25, 0.2, 2.0, 1))),
               ("ccz_set_gumbel", lambda on: e.set_gumbel(16) if on else _lib.check(e.L.ccz_set_gumbel(e.h, e._stream(), 0, 16, 16, 50.0, 1.0))),
               ("ccz_set_solver", lambda on: e.set_solver(on)),
               ("ccz_set_search", lambda on: e.set_search(on, fpu_mode=1, fpu_value=0.3)),
               ("ccz_set_routing", lambda on: e.set_routing(np.zeros(8, np.uint8), salts=(1, 2)) if on else _lib.check(
                   e.L.ccz_set_routing(e.h, e._stream(), None, 0, 0)))]
    for name, switch in options:
        switch(True)
        _refused(lambda: e.set_width(4), "ccz_set_width", name)
        assert e.L.ccz_select_wide(e.h, e._stream(), None, None) < 0                    # still width 1
        switch(False)
    # ---- the width is on: every option is refused, naming ccz_set_width; the width stays
    a, b = _engine(8, eval_cache_log2=0), _engine(8, eval_cache_log2=0)                  # b: the twin that is never disturbed
    for x in (a, b):
        x.set_width(4)
        x.set_budgets(np.full(8, 24, np.int32))
        x.select_wide()
    e = a
    for name, switch in options:
        _refused(lambda: switch(True), name, "ccz_set_width")
    # ---- the sequential step calls would silently use slot 0 of each board: refused while the width is above 1
    prob = torch.zeros((8, 2086), device=e.device)
    value = torch.zeros((8,), device=e.device)
    for name, call in [("ccz_select_leaves", e.select_leaves), ("ccz_step", lambda: e.step(prob, value)),
                       ("ccz_expand_backup", lambda: e.expand_backup(prob, value)), ("ccz_step_compact", lambda: e.step_compact(value)),
                       ("ccz_expand_backup_compact", lambda: e.expand_backup_compact(value)),
                       ("ccz_scout", lambda: _lib.check(e.L.ccz_scout(e.h, e._stream(), e.leaf_input.data_ptr()))),
                       ("ccz_eval_plan_scouted", lambda: _lib.check(e.L.ccz_eval_plan_scouted(e.h, e._stream(), None, None, None))),
                       ("ccz_scout_and_plan", lambda: _lib.check(e.L.ccz_scout_and_plan(e.h, e._stream(), None, None, None, None))),
                       ("ccz_scouted_run", lambda: _lib.check(e.L.ccz_scouted_run(e.h, e._stream(), None, None, None, None, None)))]:
        _refused(call, name, "ccz_set_width")
    _refused(lambda: e.set_width(3), "does not divide")
    # ---- and the tree continues bit-identically after all those refused calls
    for _ in range(12):
        for x in (a, b):
            lg, v = ev(x.leaf_input)
            x.gather_priors(lg, v)
            x.step_wide(v)
        assert np.array_equal(a.n_leaves(), b.n_leaves())
        ia, ib = a.leaf_info(), b.leaf_info()
        assert all(np.array_equal(ia[k], ib[k]) for k in ia)
    ra, rb = a.root_children(), b.root_children()
    assert all(np.array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8)) for k in ra)
    assert a.stats()["sims"] == b.stats()["sims"] == 48 and a.wide_stats() == b.wide_stats()
    a.check_healthy()


# ---------------------------------------------------------------------------------------------------- 6. drivers
def test_batched_analysis_at_width_eight_equals_the_model():
    """5 positions x 64 simulations through BatchedAnalysis(width=8): fresh roots, so root_visits are exactly 64 (no kept visits),
    and the principal variations are the model's."""
    from chinesechesszero_amd.analyse import BatchedAnalysis
    from chinesechesszero_amd.tools import move_id2move_action as uci_of
    lines = ["startpos", "startpos moves h2e2", "startpos moves h2e2 h9g7", "startpos moves b2e2 b9c7", "startpos moves a3a4"]
    an = BatchedAnalysis(_evaluator(), 5, n_playout=64, multipv=1, max_len=8, width=8, max_nodes=MAX_NODES, eval_cache_log2=CACHE_LOG2, seed=SEED)
    recs = an.analyse(lines)
    assert [r["status"] for r in recs] == ["ok"] * 5 and [r["root_visits"] for r in recs] == [64] * 5
    s = an.summary()
    assert s["width"] == 8 and s["inflight_now"] == 0 and s["leaves"] == 5 * 64 and 1.0 < s["mean_leaves_per_step"] <= 8.0
    # the model on the same positions, fed by a twin engine driven step by step
    from chinesechesszero_amd.uci import parse_position
    inputs = []
    for ln in lines:
        bd = parse_position(ln.split(), validate=False)
        ob = OracleBoard()
        for mv in bd.move_stack:
            ob.push_id(mv.id)
        inputs.append((ob.squares().copy(), int(ob.turn)))
    t = Twin(8, inputs, [64] * 5, check_leaves=False).run()
    for r, rec in enumerate(recs):
        want = [uci_of[m] for m in t.model.trees[r].pv(8)]
        assert rec["lines"][0]["moves"] == want, (r, rec["lines"][0]["moves"], want)
        assert rec["lines"][0]["visits"][0] == max(t.model.trees[r].root_children()[1])
    # a second file on the same object: the boundary resets the budgets, again exactly 64
    assert [r["root_visits"] for r in an.analyse(lines[:2])] == [64, 64]


def test_mcts_ai_at_width_eight_plays_a_legal_move_in_strict_mode():
    from chinesechesszero_amd.game import Board, Move
    from chinesechesszero_amd.mcts import MCTS_AI
    ai = MCTS_AI(_evaluator(), n_playout=64, width=8)
    ai.mcts.use_graph = False
    board = Board()
    seen = []
    move = ai.get_action(board, on_playout=seen.append)
    assert move in board.legal_ids() and sum(seen) == 64
    e = ai.mcts._engine
    st = e.stats()
    assert st["error_flags"] == 0 and st["sims"] == 64 and e.strict and e.wide_stats()["inflight_now"] == 0
    assert ai.mcts.root_children()["visits"].sum() == 63
    # the next move of the game: the tree is discarded (mcts.py:228-229), the budget starts over
    board.push(Move.from_id(int(move)))
    move2 = ai.get_action(board)
    assert move2 in board.legal_ids() and e.stats()["sims"] == 128 and e.stats()["error_flags"] == 0
    with pytest.raises(ValueError):
        MCTS_AI(_evaluator(), n_playout=64, width=8, solver=True)
    with pytest.raises(ValueError):
        MCTS_AI(_evaluator(), n_playout=64, width=8, scouts=4)


def test_graph_replay_of_a_wide_step_equals_the_eager_loop():
    """WideSearch with the project's own evaluator (a small PolicyValueNet), on the planned boundary and on the whole batch (the
    form a one-game search uses): one step captured as a hipGraph and replayed grows the tree the eager launches grow."""
    import os
    os.environ.setdefault("CCZ_MIOPEN_FIND", "0")   # tiny net: skip MIOpen's per-shape find step
    from chinesechesszero_amd.net import PolicyValueNet
    from chinesechesszero_amd.wide import WideSearch
    torch.manual_seed(3)
    pvn = PolicyValueNet(device="cuda:0", num_channels=32, resblocks_num=2)
    for planned in (True, False):
        out = []
        for graph in (False, True):
            ws = WideSearch(pvn, 2, 8, n_playout=48, use_graph=graph, planned=planned, max_nodes=MAX_NODES, eval_cache_log2=CACHE_LOG2,
                            seed=SEED, eps=0.0)
            assert ws.planned == planned and ws.use_graph == graph
            ws.search()
            ws.engine.check_healthy()
            s = ws.summary()
            assert s["inflight_now"] == 0 and s["leaves"] == 96 and ws.engine.stats()["sims"] == 96
            out.append((ws.engine.root_children(), ws.steps))
        (ra, na), (rb, nb) = out
        assert na == nb and all(np.array_equal(ra[k][:2].view(np.uint8), rb[k][:2].view(np.uint8)) for k in ra), planned
    assert WideSearch(pvn, 2, 8, eval_cache_log2=CACHE_LOG2).planned is False and WideSearch(pvn, 9, 8, eval_cache_log2=CACHE_LOG2).planned is True


def test_uci_width_option_answers_bestmove():
    from chinesechesszero_amd.uci import UciLoop
    out = io.StringIO()
    loop = UciLoop(policy_value_fn=_evaluator(), n_playout=64, out=out)
    for line in ["uci", "setoption name Width value 99", "setoption name Width value 8", "position startpos moves h2e2 h9g7", "go nodes 64"]:
        assert loop.handle(line)
    text = out.getvalue().splitlines()
    assert "option name Width type spin default 1 min 1 max 64" in text
    assert any(l.startswith("info string error") and "Width" in l for l in text)
    assert loop.width == 8 and loop.ai.mcts.width == 8 and loop.ai.mcts._engine.B == 8
    best = [l for l in text if l.startswith("bestmove ")]
    assert len(best) == 1 and len(best[0].split()[1]) == 4
    assert any(l.startswith("info depth") and " nodes 64 " in l for l in text)
