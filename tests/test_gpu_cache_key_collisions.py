"""GPU: the evaluation cache on FORCED collisions of the full 64-bit key -- the tag defence of cache_tag.

What keeps a position from being served another position's priors once both have one key (csrc/cczero_kernels.h):

- cache_probe_wave: ``hit = ekey == key && ek == tag``;
- cache_plan_block: ``D.ctag[w] == tag`` and, routed, ``nw == nt`` before two leaves of one step share an evaluator row;
- cache_tag: the legal-move count in the low byte, a 24-bit hash of the ordered id list above it.

On natural play two positions never share a key, so none of these ever decides. ``ccz_set_routing(salt0, salt1)`` XORs a salt of
the caller's choice into every key, slot and stored key alike, and the table survives ``ccz_set_positions``, ``ccz_reset_tree`` and
a new routing; with the keys kX, kY of two positions read from the device (leaf_keys of a fresh root):

- salts (s, s ^ kX ^ kY) give X under evaluator 0 and Y under evaluator 1 ONE salted key, in one step or across steps;
- X stored under evaluator 0 with salt0 = kX ^ kY carries the key kY: with routing off, a plain probe of Y meets an entry with its
  own full key and X's tag.

The pairs are those of tests/cache_collision_cases.py (asserted on the CPU oracle by test_cpu_cache_collision_fixtures.py). The
twins -- other position, same legal-move list: equal tags, the residual include/cczero.h documents -- are the positive controls: they
ARE served the foreign entry, which proves that the forged key met it; without them the other cases would pass vacuously on a broken
construction. The plan is compared with the NumPy restatement of test_gpu_above_4096_boards.py on the salted keys, the table with a
host model (per slot: salted key, count and id list of the last claim winner), every prior row with the float64 softmax under the
derived bound of test_gpu_boundary_f64.py, values and served hits bit for bit. No tag is read from the device.

The pair ``wide_equal_count`` (98 moves each, the same first 73 entries) is separated by the ``64 + lane`` term of cache_tag alone.

Not reachable through the ABI, and so still unpinned: two positions with one key under the SAME evaluator in one step (salts are per
evaluator; on a cross-evaluator collision ``nw == nt`` and the tag comparison of the plan guard the same decision, only a twin
isolates ``nw == nt``): dropping ``D.ctag[w] == tag`` alone in cache_plan_block changes nothing any test here can see."""
import functools

import numpy as np
import pytest
import torch

from cache_collision_cases import PAIRS, TWINS, after, pairs, search_positions
from test_gpu_above_4096_boards import _assert_plan, cache_slot, check_boundary, compact, expected_plan
from test_gpu_boundary_f64 import LEAF_EXPAND

pytestmark = pytest.mark.gpu

LOG2 = 10
S = 0x0123456789ABCDEF                                     # evaluator 0's salt where any salt will do
M64 = (1 << 64) - 1


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _evaluator(seed, sharp=6.0):
    from test_gpu_eval_cache import LogitsEvaluator
    return LogitsEvaluator(_dev(), seed=seed, sharp=sharp)


def _dense(e, seed, dtype, pos_of=None):
    """Evaluator `seed` on the leaf planes, one row per POSITION (`pos_of` [B]: a number per board, equal for equal positions;
    None: one position on all boards) and then spread over the boards, so that equal positions get equal bits by construction
    (two rows of one matrix product need not): (logits [B, 2086] `dtype`, value float32 [B]); the value as in
    test_gpu_above_4096_boards.pool_outputs (LogitsEvaluator's own saturates)."""
    pos_of = np.zeros(e.B, np.int64) if pos_of is None else np.asarray(pos_of)
    _, first, inv = np.unique(pos_of, return_index=True, return_inverse=True)
    lg, _ = _evaluator(seed)(e.leaf_input.index_select(0, torch.from_numpy(first).to(_dev())))
    v = torch.tanh(lg.mean(dim=1) * 0.3)
    idx = torch.from_numpy(inv.astype(np.int64)).to(_dev())
    return lg.index_select(0, idx).to(dtype).contiguous(), v.index_select(0, idx).contiguous()


def _engine(B, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(B, n_playout=16, seed=1, eval_cache_log2=LOG2, **kw)


def _load(e, squares, turn):
    """Fresh roots, the first selection (the leaf is the root): (keys uint64 [B], leaf_info), all boards CCZ_LEAF_EXPAND."""
    B = e.B
    sq = np.broadcast_to(np.asarray(squares, np.uint8), (B, 90)) if np.ndim(squares) == 1 else np.asarray(squares, np.uint8)
    st = e.set_positions(sq, np.broadcast_to(np.asarray(turn, np.uint8), (B,)))
    assert not st.any(), st
    return _select(e)


def _select(e):
    e.select_leaves()
    keys = e.leaf_keys()[0].cpu().numpy().view(np.uint64)
    info = e.leaf_info()
    assert (info["status"] == LEAF_EXPAND).all()
    return keys, info


def _assert_oracle_ids(info, b, pos):
    from oracle import OracleBoard
    ids = OracleBoard.from_array(pos[0], pos[1], 0).legal_ids()
    assert info["k"][b] == len(ids) and info["ids"][b][:len(ids)].tolist() == ids


def _red_net(turn, owner):
    """ccz_set_routing: the evaluator that plays red, so that `owner` is the evaluator of the root's side to move."""
    return np.where(np.asarray(turn) == 1, owner, 1 - np.asarray(owner)).astype(np.uint8)


# ------------------------------------------------------------------ the table, on the host
class TableModel:
    """Per slot the last claim winner's salted key, legal-move count and id list (softmax_gather_board: D.cins), with where its
    numbers came from; a probe hits iff key, count and list are the entry's (cache_probe_wave; equal tags <=> equal lists up to
    2^-24). The counters are those of ccz_stats."""

    def __init__(self, B, log2=LOG2):
        self.B, self.mask = B, (1 << log2) - 1
        self.entry = {}
        self.count = {"cache_probes": 0, "cache_hits": 0, "cache_shared_rows": 0, "cache_stores": 0}

    def hits(self, skey, info):
        slot = cache_slot(skey, self.mask)
        hit = np.zeros(self.B, bool)
        for b in range(self.B):
            en = self.entry.get(int(slot[b]))
            k = int(info["k"][b])
            hit[b] = en is not None and en["skey"] == int(skey[b]) and en["k"] == k and en["ids"] == info["ids"][b][:k].tolist()
        return hit

    def plan(self, skey, owner, info, verified=None):
        """One probe + plan of all boards (all CCZ_LEAF_EXPAND): (hit, miss, winner per slot, rows of the two evaluators)."""
        hit = self.hits(skey, info)
        ver = np.zeros(self.B, bool) if verified is None else hit & verified
        miss = ~hit
        slot, w, rep, rows = expected_plan(skey, owner, info, miss, self.mask)
        self.count["cache_probes"] += self.B
        self.count["cache_hits"] += int((hit & ~ver).sum())
        self.count["cache_shared_rows"] += int((miss & (rep != np.arange(self.B))).sum())
        self.count["cache_stores"] += int((w < self.B).sum())
        return hit, miss, w, rows

    def store(self, skey, info, w, pri, val, lg, v):
        """After the gather: every slot with a bidder holds its winner's evaluation."""
        for s in np.flatnonzero(w < self.B):
            b = int(w[s])
            k = int(info["k"][b])
            self.entry[int(s)] = {"skey": int(skey[b]), "k": k, "ids": info["ids"][b][:k].tolist(), "pri": pri[b].copy(),
                                  "val": val[b].copy(), "lg": lg[b].clone(), "v": v[b].clone()}

    def of(self, skey, b):
        return self.entry[int(cache_slot(skey, self.mask)[b])]

    def assert_stats(self, e, what):
        st = e.stats()
        for key, want in self.count.items():
            assert st[key] == want, (what, key, st[key], want)
        assert st["error_flags"] == 0, what


def _round(e, model, skey, owner, info, outs, routed, what, foreign=False):
    """Probe + plan + gather + expand of one step against the model. `outs` = [(logits, value) of evaluator 0, of evaluator 1],
    dense. Every board's priors against the float64 softmax of its OWN position's logits from its OWN evaluator and its value bit
    for bit; a board the table answered carries the entry's bits. `foreign`: the twin control -- a board that hit is expected to
    carry what the entry's author computed (another position), which is what the float64 check is then made against.
    Returns (hit, rows of the two evaluators, priors, values)."""
    B = e.B
    hit, miss, w, want = model.plan(skey, owner, info)
    (d0, v0), (d1, v1) = outs
    m = torch.from_numpy(owner.astype(bool)).to(_dev())
    lgd, vd = torch.where(m[:, None], d1, d0).contiguous(), torch.where(m, v1, v0).contiguous()
    own_lg, own_v = lgd.clone(), vd.clone()
    if foreign:
        for b in np.flatnonzero(hit):
            en = model.of(skey, b)
            lgd[b], vd[b] = en["lg"], en["v"]
    before = e.leaf_priors(values=False)[0]
    if routed:
        (r0, n0), (r1, n1) = e.eval_plan_routed()
        c0 = _assert_plan(r0, n0, want[0], what + " evaluator 0")
        c1 = _assert_plan(r1, n1, want[1], what + " evaluator 1")
        e.gather_priors_routed(compact(d0, r0, c0), compact(v0, r0, c0), compact(d1, r1, c1), compact(v1, r1, c1))
    else:
        assert not owner.any()
        rows, nm = e.eval_plan()
        c0 = _assert_plan(rows, nm, want[0], what)
        e.gather_priors_planned(compact(d0, rows, c0), compact(v0, rows, c0))
    live = np.ones(B, bool)
    pri = check_boundary(e, info, live, lgd, vd, before, what)
    val = e.leaf_priors()[1]
    lanes = np.arange(128)[None, :] < info["k"][:, None]
    for b in np.flatnonzero(hit):                                # a hit returns the bits the entry's author produced
        en = model.of(skey, b)
        assert np.array_equal(pri[b][lanes[b]].view(np.uint32), en["pri"][lanes[b]].view(np.uint32)), (what, b)
        assert val[b].view(np.uint32) == en["val"].view(np.uint32), (what, b)
    model.store(skey, info, w, pri, val, own_lg, own_v)
    e.expand_backup_compact(None)
    model.assert_stats(e, what)
    return hit, want, pri, val


def _assert_outputs_differ(info, b, x, y):
    """Two rows of evaluator outputs (logits, value) differ on board b's legal ids -- on nearly all of them: two fp16 logits may
    round to one number -- and in the value."""
    ids = torch.from_numpy(info["ids"][b][:info["k"][b]].astype(np.int64)).to(_dev())
    assert float((x[0].index_select(0, ids) != y[0].index_select(0, ids)).float().mean()) > 0.9 and bool(x[1] != y[1])


# ------------------------------------------------------------------ a. the probe, on the plain path
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("name", PAIRS)
def test_plain_probe_meets_a_foreign_entry_under_its_own_key(name, dtype):
    """X is stored routed under evaluator 0 with salt0 = kX ^ kY: the entry carries Y's plain key. Routing off, Y on all boards:
    the probe of cache_probe_wave finds its own 64 key bits and X's tag. Another list: a miss, one row (board 0), Y's priors,
    then hits of Y's own bits. A twin: every board is served X's evaluation (the control)."""
    X, Y, rel = pairs()[name]
    twin = rel == "same_list"
    assert twin == (name in TWINS)
    B = 8
    e = _engine(B)
    zero = np.zeros(B, np.int64)
    kY = _load(e, *Y)[0]
    kX, info = _load(e, *X)
    _assert_oracle_ids(info, 0, X)
    assert (kX == kX[0]).all() and (kY == kY[0]).all() and kX[0] != kY[0]
    salt0 = int(kX[0] ^ kY[0])
    # ---- round 1: X under evaluator 0, stored under Y's key
    e.set_routing(_red_net(np.full(B, X[1]), zero), salts=(salt0, salt0 ^ M64))
    model = TableModel(B)
    skey = kX ^ np.uint64(salt0)
    assert np.array_equal(skey, kY)
    outs_x = [_dense(e, 1, dtype), _dense(e, 2, dtype)]
    _, rows, pri1, val1 = _round(e, model, skey, zero, info, outs_x, True, f"{name} round 1")
    assert rows[0].tolist() == [0] and rows[1].size == 0                        # all boards of evaluator 0, one row
    assert model.count == {"cache_probes": B, "cache_hits": 0, "cache_shared_rows": B - 1, "cache_stores": 1}
    # ---- round 2: routing off, Y probes plainly
    e.set_routing(None)
    keys, info = _load(e, *Y)
    _assert_oracle_ids(info, 0, Y)
    assert np.array_equal(keys, kY)
    outs_y = [_dense(e, 1, dtype), _dense(e, 2, dtype)]
    _assert_outputs_differ(info, 0, (outs_x[0][0][0], outs_x[0][1][0]), (outs_y[0][0][0], outs_y[0][1][0]))
    hit, rows, pri2, val2 = _round(e, model, keys, zero, info, outs_y, False, f"{name} round 2", foreign=twin)
    lanes = np.arange(128)[None, :] < info["k"][:, None]
    if twin:
        # the documented residual: other position, same list -- the forged key met the entry
        assert hit.all() and rows[0].size == 0
        assert model.count == {"cache_probes": 2 * B, "cache_hits": B, "cache_shared_rows": B - 1, "cache_stores": 1}
        assert np.array_equal(pri2[lanes].view(np.uint32), pri1[lanes].view(np.uint32))
        assert np.array_equal(val2.view(np.uint32), val1.view(np.uint32))
    else:
        assert not hit.any() and rows[0].tolist() == [0]
        assert model.count == {"cache_probes": 2 * B, "cache_hits": 0, "cache_shared_rows": 2 * (B - 1), "cache_stores": 2}
        # ---- round 3: Y again from fresh trees: its own entry now
        e.reset_tree()
        keys3, info3 = _select(e)
        assert np.array_equal(keys3, kY) and np.array_equal(info3["k"], info["k"])
        hit, rows, pri3, val3 = _round(e, model, keys3, zero, info3, outs_y, False, f"{name} round 3")
        assert hit.all() and rows[0].size == 0
        assert model.count == {"cache_probes": 3 * B, "cache_hits": B, "cache_shared_rows": 2 * (B - 1), "cache_stores": 2}
        assert np.array_equal(pri3[lanes].view(np.uint32), pri2[lanes].view(np.uint32))
        assert np.array_equal(val3.view(np.uint32), val2.view(np.uint32))
    e.check_healthy()
    e.close()


# ------------------------------------------------------------------ b. plan and probe, routed
@pytest.mark.parametrize("name", PAIRS)
def test_routed_plan_and_probe_of_two_evaluators_on_one_salted_key(name):
    """Even boards hold X under evaluator 0, odd boards Y under evaluator 1, salts (s, s ^ kX ^ kY): one salted key, one slot,
    board 0 wins the claim. Round 1: the X boards share board 0's row, every Y board is its own row of segment 1 -- on a twin the
    tags are equal and only ``nw == nt`` keeps it off board 0's row. Round 2: X hits; Y misses on the tag, shares board 1's row,
    board 1 overwrites the entry (a twin is served evaluator 0's entry: the control). Round 3: X misses, Y hits its own bits."""
    X, Y, rel = pairs()[name]
    twin = rel == "same_list"
    B = 8
    e = _engine(B)
    owner = np.arange(B) % 2
    odd, even = np.flatnonzero(owner == 1), np.flatnonzero(owner == 0)
    squares = np.where(owner[:, None] == 1, Y[0][None, :], X[0][None, :]).astype(np.uint8)
    turn = np.where(owner == 1, Y[1], X[1])
    keys, info = _load(e, squares, turn)
    _assert_oracle_ids(info, 0, X)
    _assert_oracle_ids(info, 1, Y)
    kX, kY = keys[0], keys[1]
    assert (keys[even] == kX).all() and (keys[odd] == kY).all() and kX != kY
    salts = (S, S ^ int(kX ^ kY))
    e.set_routing(_red_net(turn, owner), salts=salts)
    skey = keys ^ np.array(salts, np.uint64)[owner]
    assert (skey == skey[0]).all() and (cache_slot(skey, (1 << LOG2) - 1) == cache_slot(skey, (1 << LOG2) - 1)[0]).all()
    outs = [_dense(e, 1, torch.float32, owner), _dense(e, 2, torch.float32, owner)]
    _assert_outputs_differ(info, 1, (outs[0][0][0], outs[0][1][0]), (outs[1][0][1], outs[1][1][1]))      # X by 0 against Y by 1 ...
    _assert_outputs_differ(info, 1, (outs[0][0][1], outs[0][1][1]), (outs[1][0][1], outs[1][1][1]))      # ... and Y by 0 against Y by 1
    model = TableModel(B)
    # ---- round 1
    hit, rows, _, _ = _round(e, model, skey, owner, info, outs, True, f"{name} round 1")
    assert not hit.any() and rows[0].tolist() == [0] and rows[1].tolist() == odd.tolist()   # (the segments are the owners)
    assert model.count == {"cache_probes": B, "cache_hits": 0, "cache_shared_rows": B // 2 - 1, "cache_stores": 1}
    # ---- round 2: the table holds board 0's entry (X, evaluator 0)
    e.reset_tree()
    keys2, info2 = _select(e)
    assert np.array_equal(keys2, keys) and np.array_equal(info2["k"], info["k"])
    hit, rows, _, _ = _round(e, model, skey, owner, info2, outs, True, f"{name} round 2", foreign=twin)
    if twin:
        assert hit.all() and rows[0].size == 0 and rows[1].size == 0
        assert model.count == {"cache_probes": 2 * B, "cache_hits": B, "cache_shared_rows": B // 2 - 1, "cache_stores": 1}
    else:
        assert np.array_equal(hit, owner == 0) and rows[0].size == 0 and rows[1].tolist() == [1]
        assert model.count == {"cache_probes": 2 * B, "cache_hits": B // 2, "cache_shared_rows": 2 * (B // 2 - 1), "cache_stores": 2}
        # ---- round 3: board 1 overwrote the entry (Y, evaluator 1)
        e.reset_tree()
        keys3, info3 = _select(e)
        assert np.array_equal(keys3, keys)
        hit, rows, _, _ = _round(e, model, skey, owner, info3, outs, True, f"{name} round 3")
        assert np.array_equal(hit, owner == 1) and rows[0].tolist() == [0] and rows[1].size == 0
        assert model.count == {"cache_probes": 3 * B, "cache_hits": B, "cache_shared_rows": 3 * (B // 2 - 1), "cache_stores": 3}
    e.check_healthy()
    e.close()


# ------------------------------------------------------------------ c. verify mode
def _mix64(z):
    """csrc/cczero_device.h mix64 on uint64 arrays."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _verify_draw(key, probes, B):
    """cache_probe_wave: the hits CCZ_FLAG_CACHE_VERIFY sends through the evaluator again -- a hash of the key, the board's probe
    count so far and the board. This restates the draw's constants and mix64, and takes one probe count for all boards (true here:
    every board probes in every round): the test below is tied to the exact hash on purpose -- the planned rows must be the DRAWN
    boards, not merely some boards. A change of the draw has to change this function with it."""
    with np.errstate(over="ignore"):
        z = key + np.uint64(0x632BE59BD9B4E019) * np.full(B, probes, np.uint64) + np.uint64(0xD1342543DE82EF95) * np.arange(B, dtype=np.uint64)
    return (_mix64(z) & np.uint64(127)) == 0


@pytest.mark.parametrize("name", ["twin", "equal_count"])
def test_cache_verify_sees_a_colliding_position(name):
    """CCZ_FLAG_CACHE_VERIFY with one entry of X under Y's key and Y on 512 boards. A twin hits the foreign entry, and every hit
    that is drawn for verification is a mismatch: the rows planned are exactly the drawn boards, ascending, and after the gather
    they hold the fresh, correct priors (everybody else X's). Another list of the same count: no hit on the foreign entry; the
    hits of later rounds are Y's own entry, and verified ones match."""
    X, Y, rel = pairs()[name]
    twin = rel == "same_list"
    B = 512
    e = _engine(B, cache_verify=True)
    zero = np.zeros(B, np.int64)
    kY = _load(e, *Y)[0]
    kX, info = _load(e, *X)
    salt0 = int(kX[0] ^ kY[0])
    e.set_routing(_red_net(np.full(B, X[1]), zero), salts=(salt0, salt0 ^ M64))
    model = TableModel(B)
    outs_x = [_dense(e, 1, torch.float32), _dense(e, 2, torch.float32)]
    _, rows, _, _ = _round(e, model, kX ^ np.uint64(salt0), zero, info, outs_x, True, f"{name} store")
    assert rows[0].tolist() == [0] and model.count["cache_stores"] == 1
    e.set_routing(None)
    keys, info = _load(e, *Y)
    assert np.array_equal(keys, kY)
    d, v = _dense(e, 1, torch.float32)
    probes = 1                                                                  # every board has probed once
    if not twin:
        # the foreign entry is not served; board 0 stores Y's own evaluation over it
        hit, rows, _, _ = _round(e, model, keys, zero, info, [(d, v), (d, v)], False, f"{name} first probe of Y")
        assert not hit.any() and rows[0].tolist() == [0] and model.count["cache_hits"] == 0
        st = e.stats()
        assert st["cache_verified"] == 0 and st["cache_verify_mismatches"] == 0
        probes += 1
        e.reset_tree()
        keys, info = _select(e)
    en = model.of(keys, 0)
    lanes = np.arange(128)[None, :] < info["k"][:, None]
    verified = 0
    for rnd in range(8):                                                        # a cap: 8 x 512 draws of 1/128 without one is ~1e-14
        what = f"{name} verify round {rnd}"
        ver = _verify_draw(keys, probes, B)
        probes += 1
        rows, nm = e.eval_plan()
        n = _assert_plan(rows, nm, np.flatnonzero(ver), what)                   # exactly the drawn boards, ascending
        pri, val = e.leaf_priors()                                              # the probe served every board the entry
        assert (pri[lanes].view(np.uint32).reshape(B, -1) == en["pri"][lanes[0]].view(np.uint32)[None, :]).all(), what
        assert (val.view(np.uint32) == en["val"].view(np.uint32)).all(), what
        model.count["cache_probes"] += B
        model.count["cache_hits"] += B - n
        lgd, vd = d.clone(), v.clone()
        if twin:                                                                # (what the unverified boards hold is X's evaluation)
            lgd[torch.from_numpy(~ver).to(_dev())] = en["lg"]
            vd[torch.from_numpy(~ver).to(_dev())] = en["v"]
        before = pri.copy()
        e.gather_priors_planned(compact(d, rows, n), compact(v, rows, n))
        pri2 = check_boundary(e, info, np.ones(B, bool), lgd, vd, before, what)
        keep = lanes & ~ver[:, None]
        assert np.array_equal(pri2[keep].view(np.uint32), pri[keep].view(np.uint32)), what
        if twin and n:                                                          # fresh priors replaced the foreign ones
            assert (pri2[ver][:, :info["k"][0]].view(np.uint32) != pri[ver][:, :info["k"][0]].view(np.uint32)).any(axis=1).all(), what
        verified += n
        model.assert_stats(e, what)
        st = e.stats()
        assert st["cache_verified"] == verified and st["cache_verify_mismatches"] == (verified if twin else 0), (what, st)
        if verified:
            break
        e.reset_tree()
        keys2, info = _select(e)
        assert np.array_equal(keys2, keys)
    assert verified > 0
    e.check_healthy()
    e.close()


# ------------------------------------------------------------------ d. a routed search under adversarial salts
SEARCH_B, SEARCH_N, SEARCH_MOVES = 16, 48, 2


class _Rowwise:
    """LogitsEvaluator's function, every row as a product of its own on a copy of its own: a row's bits depend neither on where in
    the batch it stands (the dense twin evaluates board b in row b, the planned evaluator in its compact row) nor on the address
    it has there."""

    def __init__(self, ev):
        self.W, self.w = ev.W, ev.w

    def __call__(self, leaf, plan=None):
        B = leaf.shape[0]
        if plan is not None:
            leaf = leaf.index_select(0, plan[0].long().clamp(0, B - 1))
        x = leaf.view(B, 17, 630)
        x = torch.cat([x[:, 7], x[:, 15], x[:, 16]], dim=1).float()
        rows = [x[i:i + 1].clone() for i in range(B)]
        lg = torch.cat([r @ self.W for r in rows])
        v = torch.cat([torch.tanh(r @ self.w) for r in rows])
        return lg.contiguous(), v.contiguous()


def _search_evaluators():
    return _Rowwise(_evaluator(1)), _Rowwise(_evaluator(2))


def _search_engine(log2):
    from chinesechesszero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(SEARCH_B, n_playout=SEARCH_N, eps=0.0, temp=1e-3, seed=5, max_plies=40, mirror=False, eval_cache_log2=log2)


def _legal_lanes(pri, info):
    """The prior bits of the legal moves (a table hit writes all 128 lanes of the row, a fresh gather lanes 0 .. k - 1: what lies
    past k is nobody's)."""
    return np.where(np.arange(128)[None, :] < info["k"][:, None], pri, np.float32(0)).view(np.uint32)


def _owner_now(e, red_net):
    return np.where(e.game_status()["turn"] == 1, red_net, 1 - red_net).astype(np.int64)


@functools.lru_cache(maxsize=1)
def _dense_search():
    """The cache-less twin: both evaluators on all rows, torch.where by owner. (per-step (live, priors of the live boards),
    per-move (root children, moves))."""
    ev0, ev1 = _search_evaluators()
    red_net = (np.arange(SEARCH_B) % 2).astype(np.uint8)
    ref = _search_engine(0)
    steps, trace = [], []
    for _ in range(SEARCH_MOVES):
        owner = _owner_now(ref, red_net)
        m = torch.from_numpy(owner.astype(bool)).to(_dev())
        leaf = ref.select_leaves()
        for i in range(SEARCH_N):
            (l0, v0), (l1, v1) = ev0(leaf), ev1(leaf)
            lg, v = torch.where(m[:, None], l1, l0).contiguous(), torch.where(m, v1, v0).contiguous()
            ref.gather_priors(lg, v)
            info = ref.leaf_info()
            live = info["status"] == LEAF_EXPAND
            steps.append((live, _legal_lanes(ref.leaf_priors(values=False)[0], info)[live], v.cpu().numpy()[live].view(np.uint32)))
            if i + 1 < SEARCH_N:
                leaf = ref.step_compact(v)
            else:
                ref.expand_backup_compact(v)
        rc = ref.root_children()
        trace.append((rc, ref.finish_move(keep_tree=False).cpu().numpy().copy()))
    ref.check_healthy()
    ref.close()
    return steps, trace


def _routed_search(salts):
    ev0, ev1 = _search_evaluators()
    red_net = (np.arange(SEARCH_B) % 2).astype(np.uint8)
    e = _search_engine(14)
    e.set_routing(red_net, salts=salts)
    steps, trace = [], []
    for _ in range(SEARCH_MOVES):
        leaf = e.select_leaves()
        for i in range(SEARCH_N):
            p0, p1 = e.eval_plan_routed()
            lg0, v0 = ev0(leaf, plan=p0)
            lg1, v1 = ev1(leaf, plan=p1)
            e.gather_priors_routed(lg0, v0, lg1, v1)
            info = e.leaf_info()
            live = info["status"] == LEAF_EXPAND
            pri, val = e.leaf_priors()
            steps.append((live, _legal_lanes(pri, info)[live], val[live].view(np.uint32)))
            if i + 1 < SEARCH_N:
                leaf = e.step_compact(None)
            else:
                e.expand_backup_compact(None)
        rc = e.root_children()
        trace.append((rc, e.finish_move(keep_tree=False).cpu().numpy().copy()))
    st = e.stats()
    assert st["error_flags"] == 0
    e.check_healthy()
    e.close()
    return steps, trace, st


def _first_difference(steps, want):
    for i, (a, b) in enumerate(zip(steps, want)):
        if not all(np.array_equal(x, y) for x, y in zip(a, b)):
            return i
    return None


def _search_keys():
    """The keys of P, Q and Q' (the opening after one red move, black to move), read from the device."""
    e = _engine(4)
    m = search_positions()
    out = {}
    for name, mv in m.items():
        out[name] = int(_load(e, *after(mv))[0][0])
    e.close()
    assert len(set(out.values())) == 3
    return m, out


def test_routed_search_under_adversarial_salts_is_the_dense_search():
    """16 boards on the opening, red's evaluator alternating, 48 simulations (every root child is reached), two moves without a
    kept tree. Salts (s, s ^ kP ^ kQ): evaluator 0's leaf P and evaluator 1's leaf Q -- black's reply lists differ: 44 and 41 moves --
    have one salted key. Leaf priors and values of every step, root children (counts, ids, visits, Q and prior bits) and the moves
    are those of the cache-less dense twin. Control: with Q', a twin of P, in Q's place the same search IS served foreign entries:
    more hits than under benign salts, and leaf priors that differ from the dense twin's."""
    from test_gpu_above_4096_boards import _same_search
    m, key = _search_keys()
    want_steps, want_trace = _dense_search()
    # every root child was searched in the first move, on boards of both evaluators: P, Q and Q' were leaves of both
    rc = want_trace[0][0]
    for b in (0, 1):
        k = rc["k"][b]
        assert k == 44 and (rc["visits"][b][:k] >= 1).all()
        assert all(mv in rc["acts"][b][:k] for mv in m.values())
    benign = (S, S ^ 0x5DEECE66D)
    steps, trace, st_benign = _routed_search(benign)
    assert _first_difference(steps, want_steps) is None and len(steps) == len(want_steps)
    _same_search(want_trace, trace, "benign salts")
    steps, trace, st = _routed_search((S, S ^ key["P"] ^ key["Q"]))
    d = _first_difference(steps, want_steps)
    assert d is None and len(steps) == len(want_steps), f"leaf priors differ from the dense twin's at step {d}"
    _same_search(want_trace, trace, "adversarial salts")
    assert st["cache_probes"] == st_benign["cache_probes"]   # (hits and stores may differ: P and Q overwrite each other in one slot)
    # control: the twin is served the other evaluator's entry
    steps, trace, st_twin = _routed_search((S, S ^ key["P"] ^ key["Q_twin"]))
    assert st_twin["cache_hits"] > st_benign["cache_hits"], (st_twin["cache_hits"], st_benign["cache_hits"])
    assert _first_difference(steps, want_steps) is not None
