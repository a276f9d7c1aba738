"""GPU: leaf history planes (ccz_set_leaf_history, include/cczero.h) against the NumPy model of
tests/leaf_history_model.py. Exact, no tolerance anywhere. The path positions come from the host replay of the sequential search
model (``HistoryModel.positions``), never from what the kernel wrote.

1. Rows and keys. Eight boards play leaf_history_model's forced line (tests/test_cpu_leaf_history.py asserts on the model alone what
   it reaches): after every select phase the row of every pending leaf is the model's, byte for byte, and its key the model's
   history key -- d = 0 on a fresh tree and after ccz_reset_tree, d >= 8, 0 < d < 7 at p = 0 and at 0 < p < 7 - d, p >= 7 across a
   capture, black to move; once through select / expand_backup, once through the fused step with a permuted plane_of_type.
2. Train = search. Short games with ccz_reset_tree before each move: the first leaf is the root and its row is kept. The harvested
   state of ply t (pass 0) is the kept row of ply t. The boards the harvest restarted show the start position in all eight slots:
   nothing of the longer game before.
3. Keys and cache. Same leaf, other slot 3: other key, a row of its own, its own priors back from the table. Same eight slots: one
   row. A cached search equals the uncached one over three moves, and every plan is what a host model of the table makes of the keys.
4. Off is off: never set, and set then cleared, give the same rows, keys, trees and moves; the 14 dead groups are zero again.
5. The refusals in both call orders, the evaluator guard, and a captured step that follows the setting.

Everything but the ``off`` halves of 4 fails on the parent commit: the library has no ccz_set_leaf_history."""
import numpy as np
import pytest
import torch

import leaf_history_model as hm
import search_model as sm
from oracle import OracleBoard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POT = (0, 3, 0, 6, 1, 5, 2, 4)


def _engine(n, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(n, **kw)


def _dev(P, V):
    return torch.from_numpy(P).to(DEV), torch.from_numpy(V).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. rows and keys
@pytest.mark.parametrize("fused,pot", [(False, None), (True, POT)], ids=["select_expand", "step_permuted_planes"])
def test_rows_and_keys_equal_the_model(fused, pot):
    m, f = hm.scenario()
    kw = {} if pot is None else {"plane_of_type": pot}
    e = _engine(hm.B, n_playout=14, seed=hm.SEED_, board_id_base=hm.BASE_, max_plies=hm.PLIES + 1, **kw)
    e.set_search(**sm.settings(sm.ABSOLUTE, 0.0))
    assert not e.get_leaf_history()
    e.set_leaf_history(True)
    assert e.get_leaf_history() and e.leaf_history and e.history_version == 1
    rows_checked = 0
    for t in range(hm.PLIES):
        if t == hm.RESET_AT:
            e.reset_tree()
            m.reset_tree()
        n = hm.sims_of_ply(t)
        e.select_leaves()
        for i in range(n):
            info = e.leaf_info()
            rows = e.leaf_input.cpu().numpy()
            keys = e.leaf_keys()[0].cpu().numpy().view(np.uint64)
            P, V = np.zeros((hm.B, 2086), np.float32), np.zeros(hm.B, np.float32)
            for b, (status, k, d) in enumerate(m.step()):
                w = (t, i, b)
                assert (info["status"][b], info["k"][b], info["depth"][b]) == (status, k, d), w
                if status != 0:
                    continue
                pos, turn = m.positions(b)
                assert len(pos) == t + d + 1, w
                assert rows[b].tobytes() == hm.row(pos, turn, pot).tobytes(), w
                assert int(keys[b]) == hm.history_key(pos, turn), w
                P[b], V[b] = f(b, pos[-1], turn)
                rows_checked += 1
            if fused and i + 1 < n:
                e.step(*_dev(P, V))
            else:
                e.expand_backup(*_dev(P, V))
                if i + 1 < n:
                    e.select_leaves()
        if t + 1 < hm.PLIES:
            forced = hm.forced_of_ply(t)
            played = e.finish_move(forced_moves=np.asarray(forced, np.int32)).cpu().numpy()
            m.finish_move(forced)
            assert played.tolist() == forced and not any(m.over), t
    e.check_healthy()
    assert rows_checked > 400


# ---------------------------------------------------------------------------------------------------------------- 2. train = search
def test_harvested_states_are_the_rows_the_search_saw_and_a_restart_shows_no_stale_history():
    B, T, SIMS = 8, 10, 4
    e = _engine(B, n_playout=SIMS, seed=5, max_plies=T, mirror=False)
    e.set_leaf_history(True)
    prob = torch.full((B, 2086), 1.0 / 2086, dtype=torch.float32, device=DEV)
    value = torch.zeros((B,), dtype=torch.float32, device=DEV)

    def search():
        e.reset_tree()
        leaf = e.select_leaves().cpu().numpy().copy()
        assert (e.leaf_info()["depth"] == 0).all() and (e.leaf_info()["status"] == 0).all()
        for i in range(SIMS):
            e.expand_backup(prob, value)
            if i + 1 < SIMS:
                e.select_leaves()
        return leaf
    kept = []
    for t in range(T):
        kept.append(search())
        assert (e.finish_move().cpu().numpy() >= 0).all()
    if not e.game_status()["over"].all():          # the ply cap adjudicates at the next boundary
        search()
        e.finish_move()
    st = e.game_status()
    assert st["over"].all() and (st["plies"] == T).all()
    states = e.harvest()[0].cpu().numpy()
    e.check_healthy()
    assert states.shape == (B * T, 17, 7, 10, 9)
    for b in range(B):
        for t in range(T):
            assert states[b * T + t].tobytes() == kept[t][b].tobytes(), (b, t)
    assert len({kept[T - 1][b].tobytes() for b in range(B)}) > 1    # (the boards played different games)
    # the harvest restarted every board: ply 0 of a new game on slots whose previous game was ten plies long
    st = e.game_status()
    assert not st["over"].any() and (st["plies"] == 0).all()
    leaf = e.select_leaves().cpu().numpy()
    start = OracleBoard().squares()
    want = hm.row([start], 1).tobytes()
    keys = e.leaf_keys()[0].cpu().numpy().view(np.uint64)
    for b in range(B):
        assert leaf[b].tobytes() == want, b
        assert int(keys[b]) == hm.history_key([start], 1), b


# ---------------------------------------------------------------------------------------------------------------- 3. keys and cache
class RowLogits:
    """A device evaluator whose answer is a function of ALL 119 planes of a row and of nothing else, exact in any summation order:
    0/1 planes times multiples of 1/16, then multiples of 1/4, in float64. Accepts a plan (compact outputs)."""
    batched = returns_logits = accepts_plan = stateless = leaf_history = True

    def __init__(self):
        g = torch.Generator().manual_seed(11)
        self.w1 = (torch.randint(-8, 9, (10710, 64), generator=g).double() / 16).to(DEV)
        self.w2 = (torch.randint(-2, 3, (64, 2086), generator=g).double() / 4).to(DEV)
        self.rows = 0

    def of(self, x):
        h = x.reshape(x.shape[0], -1).double() @ self.w1
        return ((h @ self.w2) / 4).float(), torch.tanh(h[:, 0] / 8).float()

    def __call__(self, leaf, plan=None):
        lg = torch.zeros((leaf.shape[0], 2086), dtype=torch.float32, device=leaf.device)
        vv = torch.zeros((leaf.shape[0],), dtype=torch.float32, device=leaf.device)
        idx = torch.arange(leaf.shape[0], device=leaf.device) if plan is None else plan[0][: int(plan[1].item())].long()
        if len(idx):
            lg[: len(idx)], vv[: len(idx)] = self.of(leaf[idx])
        self.rows += len(idx)
        return lg, vv


def _transposed(e):
    """Boards 0..2 play a3-a4 a6-a5 c3-c4 c6-c5, board 3 the same four moves with red's two swapped: one position, another history."""
    a, c, x, y = hm.move_id(27, 36), hm.move_id(29, 38), hm.move_id(54, 45), hm.move_id(56, 47)
    prob = torch.full((e.B, 2086), 1.0 / 2086, dtype=torch.float32, device=DEV)
    value = torch.zeros((e.B,), dtype=torch.float32, device=DEV)
    for ply in ((a, a, a, c), (x,) * 4, (c, c, c, a), (y,) * 4):
        e.select_leaves()
        e.expand_backup(prob, value)
        e.finish_move(forced_moves=np.asarray(ply, np.int32))
    sq = e.root_positions()
    assert all(np.array_equal(sq[0], sq[b]) for b in range(4))
    return [sq[0].copy()]


def test_the_key_tells_histories_apart_and_the_table_serves_each_its_own():
    e = _engine(4, n_playout=2, seed=9, max_plies=16, eval_cache_log2=12)
    e.set_leaf_history(True)
    _transposed(e)
    ev = RowLogits()
    e.clear_eval_cache()
    st0 = e.stats()
    want = None
    for rnd in range(2):
        e.reset_tree()
        leaf = e.select_leaves()
        assert (e.leaf_info()["depth"] == 0).all()
        rows = leaf.cpu().numpy()
        keys = e.leaf_keys()[0].cpu().numpy().view(np.uint64)
        assert np.array_equal(rows[0, [0, 8, 16]], rows[3, [0, 8, 16]])                       # the same leaf position and side to move
        assert not np.array_equal(rows[0, 3], rows[3, 3]) and rows[0].tobytes() == rows[1].tobytes() == rows[2].tobytes()
        assert keys[0] == keys[1] == keys[2] and keys[3] != keys[0]
        miss, n = e.eval_plan()
        n = int(n.item())
        if rnd == 0:
            assert n == 2 and miss[:2].cpu().tolist() == [0, 3]       # identical histories share one row, the other history gets its own
            lg, vv = ev(leaf, plan=(miss, torch.tensor([n], device=DEV)))
            e.gather_priors_planned(lg, vv)
            want = e.leaf_priors()
            assert np.array_equal(want[0][0], want[0][1]) and not np.array_equal(want[0][0], want[0][3])
        else:
            assert n == 0                                               # all four from the table ...
            got = e.leaf_priors()
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()   # ... each what its own row gave
        e.expand_backup_compact(None)
    st = e.stats()
    assert st["cache_stores"] - st0["cache_stores"] == 2 and st["cache_hits"] - st0["cache_hits"] == 4
    assert st["cache_shared_rows"] - st0["cache_shared_rows"] == 2
    e.check_healthy()


class _Table:
    """Host model of the direct-mapped table and of one step's plan, fed the keys the engine reports."""

    def __init__(self, log2):
        self.mask, self.entry = (1 << log2) - 1, {}

    def plan(self, keys, status):
        keys = [int(k) for k in keys]
        slot = [(k ^ (k >> 29)) & self.mask for k in keys]
        miss = [b for b in range(len(keys)) if status[b] == 0 and self.entry.get(slot[b]) != keys[b]]
        claim = {}
        for b in miss:
            claim.setdefault(slot[b], b)                                # the lowest board that missed on the slot
        reps = [b for b in miss if not (claim[slot[b]] < b and keys[claim[slot[b]]] == keys[b])]
        for s, b in claim.items():
            self.entry[s] = keys[b]                                     # the claim winner's evaluation is stored
        return reps


def test_a_cached_search_equals_the_uncached_one_and_plans_by_the_history_keys():
    B, SIMS, MOVES, LOG2 = 16, 24, 3, 12
    kw = dict(n_playout=SIMS, seed=31, board_id_base=640, max_plies=32)
    cached, plain = _engine(B, eval_cache_log2=LOG2, **kw), _engine(B, **kw)
    ev, table = RowLogits(), _Table(LOG2)
    for e in (cached, plain):
        e.set_leaf_history(True)
    for mv in range(MOVES):
        cached.select_leaves()
        plain.select_leaves()
        for i in range(SIMS):
            last = i + 1 == SIMS
            keys, status = (x.cpu().numpy() for x in cached.leaf_keys())
            miss, n = cached.eval_plan()
            n = int(n.item())
            assert miss[:n].cpu().tolist() == table.plan(keys.view(np.uint64), status), (mv, i)
            cached.gather_priors_planned(*ev(cached.leaf_input, plan=(miss, torch.tensor([n], device=DEV))))
            lg, vv = ev(plain.leaf_input)
            plain.gather_priors(lg, vv)
            if last:
                cached.expand_backup_compact(None)
                plain.expand_backup_compact(vv)
            else:
                cached.step_compact(None)
                plain.step_compact(vv)
                assert cached.leaf_input.cpu().numpy().tobytes() == plain.leaf_input.cpu().numpy().tobytes(), (mv, i)
        a, b = cached.root_children(), plain.root_children()
        for name in ("k", "acts", "visits", "q", "prior", "root_visits"):
            assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), (mv, name)
        assert cached.finish_move().cpu().tolist() == plain.finish_move().cpu().tolist()
    st = cached.stats()
    assert st["cache_hits"] + st["cache_shared_rows"] > 0 and ev.rows < 2 * B * SIMS * MOVES
    cached.check_healthy()
    plain.check_healthy()


# ---------------------------------------------------------------------------------------------------------------- 4. off is off
def test_never_set_and_set_then_cleared_are_the_same_engine():
    B, SIMS, MOVES = 8, 12, 2
    kw = dict(n_playout=SIMS, seed=17, board_id_base=96, max_plies=32, eval_cache_log2=10)
    never, cleared, used = _engine(B, **kw), _engine(B, **kw), _engine(B, **kw)
    cleared.set_leaf_history(True)
    cleared.set_leaf_history(False)
    ev = RowLogits()
    # `used` searches a move with the option on, then starts over with it off: its leaf tensor held all 17 groups
    used.set_leaf_history(True)
    used.select_leaves()
    for i in range(SIMS):
        used.gather_priors_planned(*ev(used.leaf_input, plan=used.eval_plan()))
        used.expand_backup_compact(None) if i + 1 == SIMS else used.step_compact(None)
    assert used.leaf_input[:, 1:7].any() and used.leaf_input[:, 9:15].any()
    used.set_leaf_history(False)
    assert not used.get_leaf_history() and used.history_version == 2
    used.reset()
    for e in (never, cleared, used):
        assert not e.leaf_history
    for mv in range(MOVES):
        for e in (never, cleared, used):
            e.select_leaves()
        for i in range(SIMS):
            ref = never.leaf_input.cpu().numpy()
            assert not ref[:, :7].any() and not ref[:, 8:15].any()
            kref = never.leaf_keys()[0].cpu().numpy()
            for name, e in (("cleared", cleared), ("used", used)):
                info = e.leaf_info()["status"]
                live = np.flatnonzero(info == 0)
                assert np.array_equal(info, never.leaf_info()["status"]), (name, mv, i)
                assert e.leaf_input.cpu().numpy()[live].tobytes() == ref[live].tobytes(), (name, mv, i)
                got = e.leaf_input.cpu().numpy()
                assert not got[:, :7].any() and not got[:, 8:15].any(), (name, mv, i)     # the 14 dead groups are zero again
                assert np.array_equal(e.leaf_keys()[0].cpu().numpy()[live], kref[live]), (name, mv, i)
            for e in (never, cleared, used):
                e.gather_priors_planned(*ev(e.leaf_input, plan=e.eval_plan()))
                e.expand_backup_compact(None) if i + 1 == SIMS else e.step_compact(None)
        want = never.root_children()
        for e in (cleared, used):
            got = e.root_children()
            for name in ("k", "acts", "visits", "q", "prior", "root_visits"):
                assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), (mv, name)
        moves = never.finish_move().cpu().tolist()
        assert cleared.finish_move().cpu().tolist() == moves and used.finish_move().cpu().tolist() == moves
    for e in (never, cleared, used):
        e.check_healthy()


# ---------------------------------------------------------------------------------------------------------------- 5. refusals, guard, graph
def test_refusals_in_both_call_orders():
    from chinesechesszero_amd._lib import CczError
    e = _engine(4, n_playout=2, eval_cache_log2=10)
    e.set_scouts(2)
    with pytest.raises(CczError, match="scout"):
        e.set_leaf_history(True)
    assert not e.get_leaf_history() and not e.leaf_history
    e.set_scouts(0)
    e.set_leaf_history(True)
    with pytest.raises(CczError, match="leaf history"):
        e.set_scouts(2)
    with pytest.raises(CczError, match="leaf history"):
        e.set_width(2)
    e.set_leaf_history(False)
    e.set_width(2)
    with pytest.raises(CczError, match="width"):
        e.set_leaf_history(True)
    e.set_width(1)
    e.set_leaf_history(True)
    assert e.get_leaf_history()
    q = _engine(4, n_playout=2, reference_quirks=True)
    with pytest.raises(CczError, match="QUIRKS"):
        q.set_leaf_history(True)
    assert not q.get_leaf_history()


class _Uniform:
    """A capturable stub: uniform priors, zero values, out of tensors it owns."""
    batched = graph_safe = stateless = True

    def __init__(self, n, reads):
        self.prob = torch.full((n, 2086), 1.0 / 2086, dtype=torch.float32, device=DEV)
        self.value = torch.zeros((n,), dtype=torch.float32, device=DEV)
        self.leaf_history = reads

    def __call__(self, leaf):
        return self.prob, self.value


def test_an_engine_with_history_refuses_an_evaluator_without_and_a_captured_step_follows_the_setting():
    from chinesechesszero_amd.net import PolicyValueNet
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    B = 8
    sp = BatchedSelfPlay(_Uniform(B, False), B, n_playout=4, seed=3)
    sp.engine.set_leaf_history(True)
    with pytest.raises(ValueError, match="history planes"):
        sp.simulate()
    net = PolicyValueNet(device=DEV, num_channels=32, resblocks_num=1)
    sp.evaluator = net.evaluate_leaves_logits          # the 21-channel pack would drop 98 planes without a word
    with pytest.raises(ValueError, match="history planes"):
        sp.simulate()
    # a captured graph of the step holds the launches of the setting it was captured under
    sp = BatchedSelfPlay(_Uniform(B, True), B, n_playout=4, seed=3, use_graph=True)
    sp.run_move()
    assert sp._graph is not None and sp._graph.captures == 1 and not sp.engine.leaf_input[:, :7].any()
    sp.engine.set_leaf_history(True)
    sp.run_move()
    assert sp._graph.captures == 2
    leaf = sp.engine.leaf_input.cpu().numpy()
    assert leaf[:, 1].any() and leaf[:, 9].any()        # the replayed step wrote the older slots too
    sp.engine.check_healthy()


# ---------------------------------------------------------------------------------------------------------------- 6. the front end
class GraphableRowLogits(RowLogits):
    graph_safe = True


def test_batched_self_play_with_history_is_one_search_graphed_or_planned():
    """BatchedSelfPlay(leaf_history=True), 32 boards x 16 simulations x 3 moves, on the planned boundary and through graph capture. The
    planned run is followed by the sequential model, fed per leaf what the boundary hands the tree (ccz_leaf_priors: from the
    evaluator's row, another board's row or the table): leaf, row, root children and move of every board equal the model's. The graphed
    run (no hook can look inside a replay) equals the planned one."""
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    B, SIMS, MOVES = 32, 16, 3
    ev = GraphableRowLogits()
    planned = BatchedSelfPlay(ev, B, n_playout=SIMS, seed=7, leaf_history=True, eval_cache_log2=12)
    graphed = BatchedSelfPlay(ev, B, n_playout=SIMS, seed=7, leaf_history=True, use_graph=True)
    assert planned.planned and not graphed.planned and planned.engine.get_leaf_history() and graphed.engine.get_leaf_history()
    assert planned.options.report(planned.engine)["leaf_history"] is True
    e, feed = planned.engine, {}

    def handed(b, board):                                  # the model's evaluator: what the boundary handed board b's leaf
        ids, pri, val = feed[b]
        assert board.legal_ids() == ids, b
        row = np.zeros(2086, np.float32)
        row[ids] = pri
        return row, val
    m = hm.HistoryModel([OracleBoard() for _ in range(B)], tuple(range(B)), 7, 0, evaluator=handed)
    checked = [0]

    def follow(stage, sim):
        if stage != "eval1":                               # after the gather, before the simulator kernel
            return
        info, (pri, val), rows = e.leaf_info(), e.leaf_priors(), e.leaf_input.cpu().numpy()
        for b in range(B):
            k = int(info["k"][b])
            feed[b] = (info["ids"][b][:k].tolist(), pri[b][:k].copy(), val[b])
        for b, (status, k, d) in enumerate(m.step()):
            assert (info["status"][b], info["depth"][b]) == (status, d), (sim, b)
            if status == 0:
                pos, turn = m.positions(b)
                assert rows[b].tobytes() == hm.row(pos, turn).tobytes(), (sim, b)
                checked[0] += 1
    for mv in range(MOVES):
        planned.advance(SIMS - 1, hooks=follow)
        planned.advance(1, hooks=follow, boundary=lambda: None)
        graphed.search()
        a, b = planned.engine.root_children(), graphed.engine.root_children()
        for name in ("k", "acts", "visits", "q", "prior", "root_visits"):
            assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), (mv, name)
        for bd in range(B):
            acts, visits, q, prior = m.root_children(bd)
            k = len(acts)
            assert a["k"][bd] == k and np.array_equal(a["visits"][bd][:k], visits), (mv, bd)
            assert np.array_equal(a["q"][bd][:k].view(np.uint32), q.view(np.uint32)), (mv, bd)
            assert np.array_equal(a["prior"][bd][:k].view(np.uint32), prior.view(np.uint32)), (mv, bd)
        played = planned.finish_move().cpu().tolist()
        assert played == graphed.finish_move().cpu().tolist()
        m.finish_move()
        assert played == [m.last[bd]["move"] for bd in range(B)], mv
    assert checked[0] > B * SIMS * MOVES // 2
    assert graphed._graph is not None and graphed._graph.captures == 1
    share = planned.options.report(planned.engine)["cache_hit_share"]
    assert share is not None and 0.0 <= share < 1.0 and "cache hit share" in planned.options.log_line(planned.engine)
    # the older planes reach the evaluator: the same leaf as the search without history writes it gets other logits
    e = planned.engine
    e.reset_tree()
    on = e.select_leaves().clone()
    off = torch.zeros_like(on)
    off[:, 7], off[:, 15], off[:, 16] = on[:, 0], on[:, 8], on[:, 16]
    assert on[:, 1:8].any() and not torch.equal(ev.of(on)[0], ev.of(off)[0])
    for sp in (planned, graphed):
        sp.engine.check_healthy()
    with pytest.raises(ValueError, match="history planes"):
        BatchedSelfPlay(_Uniform(B, False), B, n_playout=SIMS, leaf_history=True)


def test_a_saved_state_names_the_setting():
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    on = BatchedSelfPlay(_Uniform(8, True), 8, n_playout=2, seed=1, leaf_history=True)
    off = BatchedSelfPlay(_Uniform(8, True), 8, n_playout=2, seed=1)
    on.run_move()
    state = on.state_dict()
    assert state["leaf_history"] is True and off.state_dict()["leaf_history"] is False
    with pytest.raises(ValueError, match="leaf_history differs"):
        off.load_state_dict(state)
    again = BatchedSelfPlay(_Uniform(8, True), 8, n_playout=2, seed=1, leaf_history=True)
    again.load_state_dict(state)
    assert again.run_move().cpu().tolist() == on.run_move().cpu().tolist()
