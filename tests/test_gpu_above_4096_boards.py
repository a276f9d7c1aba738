"""GPU: the engine and the evaluator above 4096 boards -- the code that exists only there.

- cache_plan_block (csrc/cczero_kernels.h, k_cache_plan / k_cache_plan_routed) is ONE workgroup that walks the boards 4096 per pass:
  the carry of s_base from pass to pass, a miss whose representative got its row in an earlier pass (row_of[rep] read back), the
  `w < b` rule and the routed second segment at miss_rows[B + pos] run only with more than one pass. B = 4097 puts one board into
  pass 2, B = 8200 has a third pass.
- InferenceNet.tower_groups (net.py, TOWER_GROUP_BOARDS_G16 = 4096): on the group-of-16 layout groups > 1 happens only above 4096
  boards; tower_schedule then cuts the batch at gstep, _tower_fused launches every range with pointer offsets into the rows and the head buffers, and
  a planned batch runs groups x chains = 6 (or 9) launch parts.

The plan is compared with a NumPy restatement of the comments above cache_probe_wave and cache_plan_block (exactly: rows and count);
priors with the float64 softmax and the derived bound of test_gpu_boundary_f64.py (no tolerance of this file's own); values,
searches and evaluator outputs bit for bit. Every class of input a test needs (the same key in two passes, two keys on one slot
across passes, ...) is asserted on the keys read back from the device before the plan is looked at."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_boundary_f64 import LEAF_EXPAND, assert_priors_f64, host_logits

pytestmark = pytest.mark.gpu

PASS = 4096                     # boards per pass of cache_plan_block
SMALL = 10                      # the smallest table ccz_create accepts (eval_cache_log2 = 10..28): 1024 slots
LEAF_NONE = 3


def _dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ positions
@functools.lru_cache(maxsize=1)
def pool():
    """(squares uint8 [P + 2, 90], turn uint8 [P + 2], P): P > 256 distinct non-terminal positions from seeded random walks on the
    oracle (enough for several to share a slot of a 2^10 table: _assignment finds such a pair on the device's keys), then a mated
    position and bare kings. A position is taken as the engine gets it: without history."""
    from golden_cases import STARTS
    from oracle import OracleBoard
    rs = np.random.RandomState(20)
    seen, sq, turn = set(), [], []
    for _ in range(12):
        b = OracleBoard()
        for _ply in range(40):
            ids = b.legal_ids()
            if not ids or b.is_game_over() or b.is_tie():
                break
            b.push_id(ids[rs.randint(len(ids))])
            s, t = b.squares()[:90], int(b.turn)
            fresh = OracleBoard.from_array(s, t, 0)
            if (s.tobytes(), t) in seen or fresh.is_game_over() or fresh.is_tie():
                continue
            seen.add((s.tobytes(), t))
            sq.append(s)
            turn.append(t)
    P = len(sq)
    assert 256 < P < 600, P
    bare = np.zeros(90, np.uint8)
    bare[4], bare[3 + 9 * 9] = 7, 15                                  # e0, d9
    mated = OracleBoard.from_array(STARTS["mated"], 1, 0)
    assert mated.is_game_over() and not mated.is_tie() and not mated.legal_ids()
    assert OracleBoard.from_array(bare, 1, 0).is_tie()
    sq += [STARTS["mated"].copy(), bare]
    turn += [1, 1]
    return np.stack(sq).astype(np.uint8), np.array(turn, np.uint8), P


def _load(e, pos_of, park=None):
    sq, turn, _ = pool()
    st = e.set_positions(sq[pos_of], turn[pos_of], park=park)
    assert not st.any(), st[st != 0][:8]
    e.select_leaves()


def _inputs(e):
    """What the plan is a function of, read from the device: keys uint64 [B], leaf_info."""
    keys = e.leaf_keys()[0].cpu().numpy().view(np.uint64)
    return keys, e.leaf_info()


# ------------------------------------------------------------------ the plan, restated
def cache_slot(key, mask):
    """csrc/cczero_kernels.h cache_slot: (uint32_t)(key ^ (key >> 29)) & mask"""
    key = np.asarray(key, np.uint64)
    return ((key ^ (key >> np.uint64(29))) & np.uint64(0xFFFFFFFF) & np.uint64(mask)).astype(np.int64)


def same_list(info, a, b):
    """The tag of cache_tag is the legal-move count and a hash of the ordered list: equal tags <=> equal lists (up to 2^-24)."""
    k, ids = info["k"], info["ids"]
    past = np.arange(128)[None, :] >= k[b][:, None]
    return (k[a] == k[b]) & ((ids[a] == ids[b]) | past).all(axis=1)


def expected_plan(skey, owner, info, miss, mask):
    """cache_probe_wave: every missing board bids for its slot, the lowest board wins (atomicMin on claim[slot]) = w.
    cache_plan_block: rep(b) = w(b) if w(b) < b and w(b) holds the same (salted) key and tag -- routed: and belongs to the same
    evaluator --, else b; the evaluator's rows are the boards with rep(b) == b in ascending order, one segment per evaluator.
    Returns (slot [B], w per slot (B: no bidder), rep [B], [rows of evaluator 0, rows of evaluator 1])."""
    B = len(skey)
    b = np.arange(B)
    slot = cache_slot(skey, mask)
    w = np.full(mask + 1, B, np.int64)
    np.minimum.at(w, slot[miss], b[miss])
    wb = np.where(miss, w[slot], B)
    cand = miss & (wb < b)
    wc = np.where(cand, wb, 0)
    same = cand & (skey[wc] == skey) & (owner[wc] == owner) & same_list(info, wc, b)
    rep = np.where(same, wc, b)
    rows = [b[miss & (rep == b) & (owner == n)] for n in (0, 1)]
    return slot, w, rep, rows


def table_hits(skey, slot, w, live):
    """After a round on an empty table every slot with a bidder holds its claim winner's entry (softmax_gather_board: D.cins):
    the boards that hit next time are those whose (salted) key is the one their slot stores."""
    B = len(skey)
    ws = w[slot]
    return live & (ws < B) & (skey[np.minimum(ws, B - 1)] == skey)


# ------------------------------------------------------------------ logits: a pure function of the position
def pool_outputs(e, pos_of, live, seed, dtype):
    """One LogitsEvaluator row per POSITION (the leaf planes of the first live board that holds it), then spread over the boards:
    (dense logits [B, 2086] `dtype`, dense values float32 [B]) -- equal positions get equal bits by construction."""
    from test_gpu_eval_cache import LogitsEvaluator
    n_all = len(pool()[0])
    first = np.zeros(n_all, np.int64)
    lb = np.flatnonzero(live)[::-1]
    first[pos_of[lb]] = lb
    ev = LogitsEvaluator(_dev(), seed=seed)
    lg, _ = ev(e.leaf_input.index_select(0, torch.from_numpy(first).to(_dev())))
    v = torch.tanh(lg.mean(dim=1) * 0.3)         # (LogitsEvaluator's own value saturates at 1.0 with red to move: every net would agree)
    idx = torch.from_numpy(np.asarray(pos_of, np.int64)).to(_dev())
    return lg.index_select(0, idx).to(dtype).contiguous(), v.index_select(0, idx).contiguous(), lg, v


def compact(dense, rows, n):
    """The planned evaluator's output: row i = board rows[i] for i < n; NaN past them (a row nobody may read)."""
    out = torch.full_like(dense, float("nan"))
    out[:n] = dense.index_select(0, rows[:n].long())
    return out.contiguous()


def check_boundary(e, info, live, lgd, vd, before, what):
    """Every EXPAND board's prior row against the float64 softmax of ITS position's logits (the bound of test_gpu_boundary_f64.py),
    its vleaf bit for bit; every other board's prior row untouched. Returns the priors."""
    pri, val = e.leaf_priors()
    assert_priors_f64(pri, info["ids"], info["k"], host_logits(lgd), np.flatnonzero(live), what)
    assert np.array_equal(val[live].view(np.uint32), vd.cpu().numpy()[live].view(np.uint32)), what
    assert np.array_equal(pri[~live].view(np.uint32), before[~live].view(np.uint32)), what
    return pri


def _assignment(e, log2, rs, salts=(0, 0), collide=False):
    """Seeded board -> position map and park mask. The keys of the pool are read from the device first (every position loaded
    once), so that the boards the case is about can be placed on purpose; the classes are asserted again on the real batch."""
    sq, _, P = pool()
    B = e.B
    mask = (1 << log2) - 1
    _load(e, np.arange(B) % len(sq))
    kp = _inputs(e)[0][:P]
    pos_of = rs.randint(P, size=B)
    pos_of[rs.choice(B, 48, replace=False)] = P + rs.randint(2, size=48)        # terminal leaves in every pass
    pos_of[PASS] = rs.randint(P)                                                # (the first board of pass 2 is a live one)
    if collide:
        # two positions on one slot: the lower board (0, pass 1) wins the slot, the last board (the last pass) holds the other key
        s = cache_slot(kp, mask)
        order = np.argsort(s, kind="stable")
        pairs = np.flatnonzero(s[order][1:] == s[order][:-1])
        assert pairs.size, "no two pool positions on one slot"
        j = int(pairs[0])
        pb, pa = int(order[j]), int(order[j + 1])
        assert kp[pa] != kp[pb]
        pos_of[0] = pb
    else:
        # a position that shares its slot with no other one, under either salt: its lowest board is the slot's claim winner
        sk = np.unique(np.concatenate([kp ^ np.uint64(x) for x in salts]))
        crowded = np.bincount(cache_slot(sk, mask), minlength=mask + 1) > 1
        alone = np.flatnonzero(~crowded[cache_slot(kp ^ np.uint64(salts[0]), mask)] & ~crowded[cache_slot(kp ^ np.uint64(salts[1]), mask)])
        assert alone.size
        pa = int(alone[rs.randint(alone.size)])
    pos_of[B - 1] = pos_of[7] = pa                                              # the same key in the first and the last pass
    pos_of[20] = pos_of[21]                                                     # the same key twice inside one pass
    pos_of[3], pos_of[B - 3] = P, P + 1                                         # mated, bare kings
    park = np.zeros(B, bool)
    park[[11, 4000, B - 2]] = True
    return pos_of, park


def _assert_classes(keys, info, pos_of, park, log2, collide=False):
    status = info["status"]
    _, turn, P = pool()
    B = len(keys)
    live = status == LEAF_EXPAND
    assert (status[park] == LEAF_NONE).all() and park.sum() == 3                                  # parked boards
    assert (status[~park] != LEAF_NONE).all()
    assert (status[~park & (pos_of == P)] == 2).all() and (status[~park & (pos_of == P + 1)] == 1).all()
    assert (live == (~park & (pos_of < P))).all() and (status == 2).any() and (status == 1).any()  # boards that are not EXPAND
    # equal positions <=> equal keys
    act = ~park
    kp = np.zeros(P + 2, np.uint64)
    kp[pos_of[act]] = keys[act]
    assert (kp[pos_of[act]] == keys[act]).all()
    present = np.unique(pos_of[act])
    assert len(np.unique(kp[present])) == len(present)
    # the same key in two passes / twice inside one pass
    lb = np.flatnonzero(live)
    u, inv = np.unique(keys[lb], return_inverse=True)
    p = lb // PASS
    lo, hi = np.full(len(u), 99), np.full(len(u), -1)
    np.minimum.at(lo, inv, p)
    np.maximum.at(hi, inv, p)
    last = (B - 1) // PASS
    assert last >= 1 and ((lo == 0) & (hi == last)).any()
    assert (np.unique(inv * 8 + p, return_counts=True)[1] >= 2).any()
    if collide:
        # two different keys on one slot, the lower board in an earlier pass
        slot = cache_slot(keys, (1 << log2) - 1)
        w = np.full(1 << log2, B, np.int64)
        np.minimum.at(w, slot[live], lb)
        wb = np.where(live, w[slot], 0)
        assert (live & (keys[wb] != keys) & (wb // PASS < np.arange(B) // PASS)).any()
    return live


def _assert_plan(rows, n, want, what):
    got, n = rows.cpu().numpy(), int(n.cpu().numpy()[0])
    assert n == len(want), (what, n, len(want))
    if not np.array_equal(got[:n], want):
        i = int(np.flatnonzero(got[:n] != want)[0])
        raise AssertionError(f"{what}: row {i} is board {got[i]}, expected {want[i]}; {int((got[:n] != want).sum())} of {n} rows differ")
    return n


def _plan_rounds(B, log2, verify):
    from chinesechesszero_amd.engine import SelfPlayEngine
    rs = np.random.RandomState(1000 + B + log2)
    e = SelfPlayEngine(B, n_playout=16, seed=1, eval_cache_log2=log2, cache_verify=verify)
    mask = (1 << log2) - 1
    collide = log2 == SMALL
    pos_of, park = _assignment(e, log2, rs, collide=collide)
    _load(e, pos_of, park)
    keys, info = _inputs(e)
    live = _assert_classes(keys, info, pos_of, park, log2, collide)
    owner = np.zeros(B, np.int64)
    dtype = torch.float32 if collide else torch.float16
    lgd, vd, _, _ = pool_outputs(e, pos_of, live, 1, dtype)
    lanes = np.arange(128)[None, :] < info["k"][:, None]
    # ---- round 1: an empty table, every EXPAND board misses
    slot, w1, rep1, want = expected_plan(keys, owner, info, live, mask)
    if not collide:
        assert rep1[B - 1] < PASS                                               # the last board's row was assigned in the first pass
    if (B, log2) != (4097, SMALL):   # (there the only board of pass 2 is the one that loses its slot to another key)
        assert (rep1[live] // PASS < np.flatnonzero(live) // PASS).any()        # a representative of an earlier pass
    rows, nm = e.eval_plan()
    n = _assert_plan(rows, nm, want[0], f"B {B} 2^{log2} round 1")
    before = e.leaf_priors(values=False)[0]
    e.gather_priors_planned(compact(lgd, rows, n), compact(vd, rows, n))
    pri1 = check_boundary(e, info, live, lgd, vd, before, f"B {B} 2^{log2} round 1")
    e.expand_backup_compact(None)
    # ---- round 2: fresh trees on the same positions, the table holds every slot's claim winner
    e.reset_tree()
    e.select_leaves()
    keys2, info2 = _inputs(e)
    assert np.array_equal(keys2[~park], keys[~park]) and np.array_equal(info2["status"], info["status"])
    assert np.array_equal(info2["k"][live], info["k"][live]) and np.array_equal(info2["ids"][live][lanes[live]], info["ids"][live][lanes[live]])
    hit = table_hits(keys, slot, w1, live)
    miss2 = live & ~hit
    assert hit.any() and (miss2.any() or log2 == 16)
    _, w2, rep2, want2 = expected_plan(keys, owner, info, miss2, mask)
    rows, nm = e.eval_plan()
    n_ver = 0
    if not verify:
        n = _assert_plan(rows, nm, want2[0], f"B {B} 2^{log2} round 2")
    else:
        # CCZ_FLAG_CACHE_VERIFY: a hit in 128 (a hash) is planned as well; it does not bid, so the rest of the plan is unchanged
        got, n = rows.cpu().numpy(), int(nm.cpu().numpy()[0])
        got = got[:n]
        assert (np.diff(got) > 0).all() and ((got >= 0) & (got < B)).all() and (hit | miss2)[got].all()
        assert np.isin(keys[miss2], keys[got]).all()
        assert np.array_equal(got[miss2[got]], want2[0])
        n_ver = int(hit[got].sum())
    before = e.leaf_priors(values=False)[0]
    e.gather_priors_planned(compact(lgd, rows, n), compact(vd, rows, n))
    pri2 = check_boundary(e, info, live, lgd, vd, before, f"B {B} 2^{log2} round 2")
    m = live[:, None] & lanes
    assert np.array_equal(pri2[m].view(np.uint32), pri1[m].view(np.uint32))     # a hit returns the bits the first round produced
    e.expand_backup_compact(None)
    st = e.stats()
    shared = int((live & (rep1 != np.arange(B))).sum() + (miss2 & (rep2 != np.arange(B))).sum())
    stores = int((w1 < B).sum() + (w2 < B).sum())
    assert st["cache_probes"] == 2 * int(live.sum()) and st["cache_hits"] == int(hit.sum()) - n_ver, st
    assert st["cache_shared_rows"] == shared and st["cache_stores"] == stores, (st, shared, stores)
    if verify:
        assert st["cache_verified"] == n_ver and n_ver > 0 and st["cache_verify_mismatches"] == 0, (st, n_ver)
    assert st["error_flags"] == 0
    e.check_healthy()
    e.close()


@pytest.mark.parametrize("B,log2", [(4097, SMALL), (4097, 16), (8200, SMALL), (8200, 16)])
def test_plan_of_two_and_three_passes_against_the_numpy_restatement(B, log2):
    """ccz_eval_plan + ccz_gather_priors_planned: miss_rows[:n_miss] and n_miss exactly, priors against float64, values bit for bit,
    then the same positions again from fresh trees (hits = the boards whose key their slot's claim winner stored)."""
    _plan_rounds(B, log2, False)


def test_plan_of_three_passes_with_cache_verify():
    """CCZ_FLAG_CACHE_VERIFY at 8200 boards: the verify draw is a hash, so the second round asserts invariants -- ascending rows,
    every missing board's key on a planned row, the plan without the verified boards is the plan -- and no mismatch."""
    _plan_rounds(8200, 16, True)


# ------------------------------------------------------------------ routed plan
def test_routed_plan_of_two_passes_against_the_numpy_restatement():
    """ccz_set_routing + ccz_eval_plan_routed + ccz_gather_priors_routed at 4100 boards: both segments [0, n0) and [B, B + n1)
    exactly, no row shared across evaluators, every board's priors and value from its owner's logits; then a second round of hits
    under both salts. 2^10 slots for ~800 salted keys: a slot's claim winner is often the other evaluator's board."""
    from chinesechesszero_amd.engine import SelfPlayEngine
    B, log2 = 4100, 10
    mask = (1 << log2) - 1
    rs = np.random.RandomState(77)
    e = SelfPlayEngine(B, n_playout=16, seed=2, eval_cache_log2=log2)
    salts = (0x1234567, 0x89ABCDEF0F1E2D3C)
    pos_of, park = _assignment(e, log2, rs, salts)
    _load(e, pos_of, park)
    keys, info = _inputs(e)
    live = _assert_classes(keys, info, pos_of, park, log2)
    red_net = rs.randint(2, size=B).astype(np.uint8)
    red_net[B - 1] = red_net[7]                                                 # the same position AND owner in both passes
    turn = pool()[1][pos_of]
    if (turn[PASS] == turn[B - 1]) == (red_net[PASS] == red_net[B - 1]):
        red_net[PASS] ^= 1                                                      # the two live boards of pass 2: one per evaluator
    e.set_routing(red_net, salts=salts)
    owner = np.where(turn == 1, red_net, 1 - red_net).astype(np.int64)
    skey = keys ^ np.array(salts, np.uint64)[owner]
    # both evaluators in both passes, equal positions on both evaluators
    for n in (0, 1):
        assert (live & (owner == n))[:PASS].any() and (live & (owner == n))[PASS:].any()
    both = np.intersect1d(pos_of[live & (owner == 0)], pos_of[live & (owner == 1)])
    assert both.size > 100
    d0, w0, p0, pv0 = pool_outputs(e, pos_of, live, 1, torch.float32)
    d1, w1_, p1, pv1 = pool_outputs(e, pos_of, live, 2, torch.float32)
    P = pool()[2]
    assert bool((p0[:P] != p1[:P]).any(dim=1).all()) and bool((pv0[:P] != pv1[:P]).all())       # they disagree on every position
    m = torch.from_numpy(owner.astype(bool)).to(_dev())
    lgd = torch.where(m[:, None], d1, d0).contiguous()
    vd = torch.where(m, w1_, w0).contiguous()
    lanes = np.arange(128)[None, :] < info["k"][:, None]
    miss, pri1, hits = live, None, 0
    shared = stores = 0
    for rnd in (1, 2):
        what = f"routed round {rnd}"
        slot, w, rep, want = expected_plan(skey, owner, info, miss, mask)
        (r0, n0), (r1, n1) = e.eval_plan_routed()
        assert r1.data_ptr() == r0.data_ptr() + 4 * B                            # the second segment starts at miss_rows[B]
        c0 = _assert_plan(r0, n0, want[0], what + " evaluator 0")
        c1 = _assert_plan(r1, n1, want[1], what + " evaluator 1")
        g0, g1 = r0.cpu().numpy()[:c0], r1.cpu().numpy()[:c1]
        assert (np.diff(g0) > 0).all() and (np.diff(g1) > 0).all()
        assert (owner[g0] == 0).all() and (owner[g1] == 1).all()                 # no row across evaluators ...
        for n, g in ((0, g0), (1, g1)):                                          # ... every missing board's position is on ITS segment
            assert np.isin(pos_of[miss & (owner == n)], pos_of[g]).all()
        if rnd == 1:
            assert c0 > 0 and c1 > 0 and np.intersect1d(pos_of[g0], pos_of[g1]).size > 100
            assert rep[B - 1] < PASS                                             # a row assigned in the first pass, read back in the second
        before = e.leaf_priors(values=False)[0]
        e.gather_priors_routed(compact(d0, r0, c0), compact(w0, r0, c0), compact(d1, r1, c1), compact(w1_, r1, c1))
        pri = check_boundary(e, info, live, lgd, vd, before, what)
        e.expand_backup_compact(None)
        shared += int((miss & (rep != np.arange(B))).sum())
        stores += int((w < B).sum())
        if rnd == 1:
            pri1 = pri
            e.reset_tree()
            e.select_leaves()
            keys2, info2 = _inputs(e)
            assert np.array_equal(keys2[~park], keys[~park]) and np.array_equal(info2["status"], info["status"])
            hit = table_hits(skey, slot, w, live)
            for n in (0, 1):
                assert (hit & (owner == n)).any() and (live & ~hit & (owner == n)).any()
            miss, hits = live & ~hit, int(hit.sum())
        else:
            mm = live[:, None] & lanes
            assert np.array_equal(pri[mm].view(np.uint32), pri1[mm].view(np.uint32))
    st = e.stats()
    assert st["cache_probes"] == 2 * int(live.sum()) and st["cache_hits"] == hits, st
    assert st["cache_shared_rows"] == shared and st["cache_stores"] == stores, (st, shared, stores)
    assert st["error_flags"] == 0
    e.check_healthy()
    e.close()


# ------------------------------------------------------------------ the search through it
def _same_search(t0, t1, what):
    assert len(t0) == len(t1)
    for mv, ((a, ma), (b, mb)) in enumerate(zip(t0, t1)):
        for key in ("k", "acts", "visits", "root_visits"):
            assert np.array_equal(a[key], b[key]), (what, mv, key)
        for key in ("q", "prior"):
            assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (what, mv, key)
        assert np.array_equal(ma, mb), (what, mv)


def test_cached_search_of_4100_boards_is_the_uncached_search():
    """4100 boards, 12 simulations, three moves with the evaluation cache off, 2^10 (slots overwritten all the time, collisions
    inside every step) and 2^16: root children, Q and prior bits and every move equal; the stats equalities of
    test_gpu_eval_cache.py hold."""
    from test_gpu_eval_cache import _play
    dev = _dev()
    B, n, moves = 4100, 12, 3
    sp0, ev0, t0 = _play(B, n, moves, 0, dev)
    s0 = sp0.engine.stats()
    assert s0["cache_probes"] == 0 and ev0.rows_asked == B * n * moves and s0["error_flags"] == 0
    for log2 in (10, 16):
        sp1, ev1, t1 = _play(B, n, moves, log2, dev)
        _same_search(t0, t1, f"2^{log2}")
        s1 = sp1.engine.stats()
        for key in ("sims", "moves", "games", "expansions", "terminal_leaves", "sum_depth", "sum_children"):
            assert s0[key] == s1[key], (log2, key)
        assert s1["cache_probes"] == s1["expansions"]
        assert s1["cache_shared_rows"] > 0 and s1["cache_hits"] > 0 and s1["cache_stores"] > 0
        assert ev1.rows_asked == s1["cache_probes"] - s1["cache_hits"] - s1["cache_shared_rows"]
        assert s1["error_flags"] == 0
        sp1.engine.check_healthy()
        sp1.engine.close()
    sp0.engine.close()


def _play_net(pvn, B, n, moves, log2, use_graph):
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    sp = BatchedSelfPlay(pvn.evaluate_leaves_logits, B, n_playout=n, seed=4, max_plies=30, eval_cache_log2=log2, use_graph=use_graph)
    assert sp.planned == (log2 > 0)
    trace = []
    for _ in range(moves):
        sp.search()
        rc = sp.engine.root_children()
        trace.append((rc, sp.finish_move().cpu().numpy().copy()))
    assert (sp._graph is not None) == use_graph
    sp.engine.check_healthy()
    return sp, trace


def test_real_evaluator_search_of_4112_boards_planned_graphed_and_eager():
    """The fused evaluator (256 x 1) at 4112 boards, default layout (group-of-16 rows, edge-pair tiles): without a cache the tower
    runs as two sequential groups cut at gstep, on the planned boundary as 2 groups x 3 chains = 6 launch parts, in a captured
    graph as one group and one chain -- three moves of 12 simulations are the same search in all three."""
    from chinesechesszero_amd.net import PolicyValueNet
    dev = _dev()
    B, n, moves = 4112, 12, 3
    torch.manual_seed(2)
    pvn = PolicyValueNet(device=dev, num_channels=256, resblocks_num=1)
    inf = pvn.refresh_inference_copy()
    assert inf._g16(B) and inf.tower_groups(B, True) == 2 and inf._edge(B, True) and inf.tower_chains(B, 2, True) == 3
    sp0, t0 = _play_net(pvn, B, n, moves, 0, False)
    sp1, t1 = _play_net(pvn, B, n, moves, 16, False)
    _same_search(t0, t1, "planned")
    s0, s1 = sp0.engine.stats(), sp1.engine.stats()
    for key in ("sims", "moves", "games", "expansions", "terminal_leaves", "sum_depth", "sum_children"):
        assert s0[key] == s1[key], key
    assert s1["cache_probes"] == s1["expansions"] and s1["cache_shared_rows"] > 0 and s1["cache_hits"] > 0
    assert s0["error_flags"] == 0 and s1["error_flags"] == 0
    sp1.engine.close()
    sp2, t2 = _play_net(pvn, B, n, moves, 0, True)
    _same_search(t0, t2, "graphed")
    assert sp2.engine.stats()["error_flags"] == 0
    sp2.engine.close()
    sp0.engine.close()


# ------------------------------------------------------------------ the evaluator: the same bits above 4096
B_MAX = 8208


@functools.lru_cache(maxsize=1)
def evaluator_case():
    """A 256 x 2 net with perturbed BatchNorm statistics (test_gpu_conv.py), 8208 random leaf batches, and the reference: the
    same boards in chunks of at most 4096 (4096 + 4096 + 16: one tower group each, the last chunk on the small-batch kernels) --
    the path that is pinned to float64 and to the reference architecture. Computed once for every test below."""
    from chinesechesszero_amd.net import InferenceNet, Net
    dev = _dev()
    torch.manual_seed(9)
    net = Net(256, 2).to(dev).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 2)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    inf = InferenceNet(net).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(5)
    leaf = torch.zeros(B_MAX, 119, 90, dtype=torch.float16, device=dev)
    leaf[:, 49:56] = (torch.rand(B_MAX, 7, 90, generator=g, device=dev) < 0.1).half()
    leaf[:, 105:119] = (torch.rand(B_MAX, 14, 90, generator=g, device=dev) < 0.1).half()
    leaf = leaf.view(B_MAX, 17, 7, 10, 9)
    lgs, vs = [], []
    for a in range(0, B_MAX, 4096):
        chunk = leaf[a:a + 4096]
        assert inf.tower_groups(-(-chunk.shape[0] // 16) * 16, inf._g16(chunk.shape[0])) == 1
        lg, v = inf(chunk, return_logits=True)
        lgs.append(lg.clone())
        vs.append(v.clone())
    lg, v = torch.cat(lgs), torch.cat(vs)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lg.float()).all()) and float(lg.float().std()) > 0.01 and float(v.std()) > 1e-3
    assert bool((lg[1:] != lg[:-1]).any(dim=1).all())                            # neighbouring boards differ: a row swap cannot hide
    return inf, leaf, lg, v


@pytest.mark.parametrize("B", [4097, 4112, B_MAX])
def test_dense_evaluator_above_4096_boards_has_the_bits_of_4096_board_chunks(B):
    """_tower_fused with 2 (3) sequential groups cut at gstep = 2176 (2816) boards, every group as three chains with pointer
    offsets into the group-of-16 rows and the head buffers: logits and values of every board are the bits of the chunked run."""
    inf, leaf, want_lg, want_v = evaluator_case()
    Bp = -(-B // 16) * 16
    groups = inf.tower_groups(Bp, True)
    assert inf._g16(B) and groups == -(-Bp // 4096) and groups > 1
    lg, v = inf(leaf[:B], return_logits=True)
    torch.cuda.synchronize()
    assert lg.shape == (B, 2086) and v.shape == (B,)
    bad = torch.nonzero((lg != want_lg[:B]).any(dim=1) | (v != want_v[:B])).flatten()
    assert bad.numel() == 0, f"{bad.numel()} boards differ, first {bad[:8].tolist()}"


def _byte_fill(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=dev).view(dtype).view(shape)


@pytest.mark.parametrize("B", [4097, 4112, B_MAX])
def test_planned_evaluator_above_4096_boards_live_rows_only(B):
    """_tower_fused on a planned batch with groups x chains = 6 (9) launch parts: live counts 1, 4096, 4097 and B with permuted rows. The live rows
    carry the bits of the chunked run; in the evaluator's persistent buffers (plane pack, stem output = tower ping-pong buffer,
    head outputs, hidden value layer), poisoned before the call, nothing outside the live rows -- whole groups of 16 for the
    group-of-16 buffers -- is written."""
    inf, leaf, want_lg, want_v = evaluator_case()
    dev = _dev()
    Bp = -(-B // 16) * 16
    groups = inf.tower_groups(Bp, True)
    assert groups > 1 and groups * inf.tower_chains(Bp, groups, inf._edge(Bp, True)) == 3 * groups
    gen = torch.Generator().manual_seed(B)
    x = leaf[:B]
    for live in sorted({1, 4096, 4097, B}):
        rows = torch.randperm(B, generator=gen).to(torch.int32).to(dev).contiguous()
        n_rows = torch.tensor([live], dtype=torch.int32, device=dev)
        x64 = torch.zeros((Bp, 90, 64), dtype=torch.float16, device=dev)       # channels 24..63 must stay zero (never written)
        x64.view(Bp // 16, 90, 16, 64)[..., :24] = 3.0
        y = _byte_fill((Bp, 256, 10, 9), torch.float16, dev).contiguous(memory_format=torch.channels_last)
        pol = torch.zeros((Bp, 1536), dtype=torch.float16, device=dev)
        val = torch.zeros((Bp, 640), dtype=torch.float16, device=dev)
        pol[:, :1530] = 3.0
        val[:, :630] = 3.0
        h1 = _byte_fill((Bp, 256), torch.float16, dev)
        inf.__dict__["_plan_bufs"] = {(Bp, dev, True): (x64, y)}
        inf.__dict__["_head_bufs"] = {(Bp, dev): (pol, val, h1)}
        lg, v = inf(x, return_logits=True, plan=(rows, n_rows))
        torch.cuda.synchronize()
        assert inf.__dict__["_plan_bufs"][(Bp, dev, True)][1] is y and inf.__dict__["_head_bufs"][(Bp, dev)][0] is pol   # the buffers it used
        r = rows[:live].long()
        bad = torch.nonzero((lg[:live] != want_lg[r]).any(dim=1) | (v[:live] != want_v[r])).flatten()
        assert bad.numel() == 0, f"B {B} live {live}: {bad.numel()} rows differ, first {bad[:8].tolist()}"
        G = -(-live // 16)                                                       # groups of 16 that hold live rows
        xs = x64.view(Bp // 16, 90, 16, 64).permute(0, 2, 1, 3).reshape(Bp, 90, 64)    # slot-major: row i = compact row i
        assert bool((xs[live:, :, :24] == 3.0).all()) and bool((xs[:, :, 24:] == 0).all()), (B, live)
        assert bool(((xs[:live, :, :24] == 0) | (xs[:live, :, :24] == 1)).all()), (B, live)
        yb = y.permute(0, 2, 3, 1).reshape(Bp // 16, -1).view(torch.uint8)
        assert bool((yb[G:] == 0xFF).all()), (B, live)
        assert bool(torch.isfinite(y.permute(0, 2, 3, 1).reshape(Bp // 16, 90, 16, 256)[:G].permute(0, 2, 1, 3).reshape(G * 16, -1)[:live].float()).all())
        assert bool((pol[live:, :1530] == 3.0).all()) and bool((pol[:, 1530:] == 0).all()), (B, live)
        assert bool((val[live:, :630] == 3.0).all()) and bool((val[:, 630:] == 0).all()), (B, live)
        assert bool((pol[:live, :1530] != 3.0).any(dim=1).all())
        assert bool((h1.view(torch.uint8)[live:] == 0xFF).all()) and bool(torch.isfinite(h1[:live].float()).all()), (B, live)
    inf.__dict__.pop("_plan_bufs")
    inf.__dict__.pop("_head_bufs")
