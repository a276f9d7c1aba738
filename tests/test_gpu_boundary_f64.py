"""GPU: the compact evaluator boundary against a float64 softmax, on positions with more than 64 legal moves.

Every per-board kernel of csrc/cczero_kernels.h is one wave64 wave; lane i holds legal move i and 64 + i. What the tree consumes on
the compact / planned / routed boundary is ``prior128`` and ``vleaf``, written by

- softmax_gather_board :654-747 (plain, planned, routed): the fp16 dword loop :672-700 (max :685-695, sum :696-700), the fp32
  loop :701-708, the wave sum :710, the two halves p0 / p1 :713-714, the verify check :717-731, the cache store :736-742;
- cache_probe_wave on a table hit (out[lane] = q0, out[64 + lane] = q1 :793-794);
- expand_backup_phase<true> (cp0 / cp1 :515, children 0..63 / 64..127 :533-541), also the body of k_scouted_run (:1034, :1051).

The reference of every check here is the same: the leaf's logits exactly as the kernel reads them (fp16 or fp32, promoted to
float64), ``exp(x - logsumexp(x))`` over all 2086 entries in float64, taken at ``leaf_info()['ids'][b][:k]`` -- ids that are first
asserted to be the oracle's ``legal_ids()`` wherever the oracle follows the board.

Tolerance (derived, not measured). u = 2^-24 (float32 round-to-nearest). With m = max(x), d_i = m - x_i, ref_i the float64 value
and d̄ = Σ_j ref_j d_j::

    |p_i - ref_i| <= ref_i (2 d_i + 2 d̄ + 64) u + 2^-126

- the exponent: ``__expf(y)`` is ``v_exp_f32(fl(0x1.715476p+0 * y))`` (clang's __clang_hip_math.h), y = fl(x_i - m). The
  subtraction rounds by <= u, the float32 log2(e) is off by 0.155 u, the product rounds by <= u: the exponential of -d_i is taken
  at -d_i (1 + e) with |e| <= 2.16 u, a relative error of 2.16 d_i u. Beyond d_i = 87.3, ref_i < 2^-126 and the absolute term
  covers everything; below it, and with d̄ <= ln(2086) + 1 < 9 (a softmax over 2086 entries has no more spread), the 0.16 (d_i + d̄) u
  excess over 2 (d_i + d̄) u is < 16 u and comes out of the slack of the constant below;
- v_exp_f32 itself: one ulp, <= 2 u relative, once in the numerator and once in every term of the sum;
- the sum: <= 34 sequential adds per lane (33 fp32 elements or 17 fp16 dwords x 2) and 6 levels of the wave reduction,
  <= 40 u; the terms' own exponent errors add Σ_j ref_j 2.16 d_j u = 2.16 d̄ u;
- the division: u (correctly rounded: no fast-math);
- 2 + 2 + 40 + 1 = 45 u, plus < 16 u of the exponent excess: 61 u <= 64 u;
- flush-to-zero of denormal exp2 results and priors: the sum is >= 1 (the maximum contributes exp2(0) = 1), so either costs at
  most 2^-126 absolute.

Values (``vleaf``) are compared bit for bit with the evaluator's value of the board's row. A board whose leaf is not
CCZ_LEAF_EXPAND keeps its prior128 row byte for byte. If hardware ever exceeds the bound, find out why before widening it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126
LEAF_EXPAND = 0


# ------------------------------------------------------------------ the float64 reference
def softmax64(x):
    """[R, 2086] logits (any float dtype) -> (ref float64 [R, 2086], d = max - x, d̄ [R])."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    d = m - x
    e = np.exp(-d)                                   # d = inf (a -inf logit) -> 0
    ref = e / e.sum(axis=1, keepdims=True)
    dbar = np.where(ref > 0, ref * np.where(np.isfinite(d), d, 0.0), 0.0).sum(axis=1)
    return ref, d, dbar


def assert_priors_f64(pri, ids, k, logits, boards, what=""):
    """pri float32 [B,128] (leaf_priors), ids uint16 [B,128], k int [B], logits [B,2086] as the kernel read them: every board in
    ``boards`` within the derived bound of the float64 softmax of its row."""
    boards = np.asarray(boards, dtype=np.int64)
    if boards.size == 0:
        return
    x = logits[boards]
    ref, d, dbar = softmax64(x)
    lanes = np.arange(128)[None, :]
    live = lanes < np.asarray(k)[boards][:, None]
    sel = np.asarray(ids)[boards].astype(np.int64)
    r = np.take_along_axis(ref, sel, axis=1)
    di = np.take_along_axis(d, sel, axis=1)
    p = np.asarray(pri)[boards].astype(np.float64)
    rel = np.where(r > 0, r * (2.0 * np.where(np.isfinite(di), di, 0.0) + 2.0 * dbar[:, None] + 64.0) * U, 0.0)
    bound = rel + TINY
    ok = (np.abs(p - r) <= bound) | ~live               # NaN / inf priors fail
    if not ok.all():
        j, lane = np.argwhere(~ok)[0]
        b = int(boards[j])
        raise AssertionError(f"{what}: board {b} lane {lane} (id {sel[j, lane]}, k {k[b]}): prior {p[j, lane]!r} vs float64 "
                             f"{r[j, lane]!r} (bound {bound[j, lane]:.3e}, d_i {di[j, lane]:.3f}); {int((~ok).sum())} lanes out")


def host_logits(t):
    """The logits exactly as the kernel reads them, on the host (fp16 / fp32 promoted to float64 by softmax64)."""
    return t.float().cpu().numpy() if t.dtype == torch.float16 else t.cpu().numpy()


def check_boundary(e, logits, value, what, plain=True):
    """After gather_priors_planned / _routed: every CCZ_LEAF_EXPAND board's prior128 row against the float64 softmax of
    ``logits[b]`` (its evaluator's dense row: bit-identical to the planned row), its vleaf bit-identical to ``value[b]``; with
    ``plain`` also bit-identical to the unplanned gather of the same logits. Returns (leaf_info, expand mask)."""
    info = e.leaf_info()
    pri, val = e.leaf_priors()
    live = info["status"] == LEAF_EXPAND
    x = host_logits(logits)
    assert_priors_f64(pri, info["ids"], info["k"], x, np.flatnonzero(live), what)
    v = value.cpu().numpy()
    assert np.array_equal(val[live].view(np.uint32), v[live].view(np.uint32)), what
    if plain:
        # The plain kernel on the same rows: same arithmetic, same bits. It overwrites prior128, so after this the tree expands from
        # the plain kernel's priors -- bit-identical to the planned / table-hit ones by the assertion below. The search where the
        # planned output itself is what the tree consumes is test_planned_search_on_wide_roots_... (plain=False).
        e.gather_priors(logits, value)
        pri2, _ = e.leaf_priors(values=False)
        lanes = np.arange(128)[None, :] < info["k"][:, None]
        m = live[:, None] & lanes
        assert np.array_equal(pri[m].view(np.uint32), pri2[m].view(np.uint32)), what
    return info, live


def hit_boards(e, info, rows, n):
    """EXPAND boards whose leaf the table answered this step: their key is on no planned evaluator row."""
    keys = e.leaf_keys()[0].cpu().numpy()
    n = int(n.cpu().numpy()[0])
    planned = set(keys[rows.cpu().numpy()[:n]].tolist())
    return np.array([b for b in range(e.B) if info["status"][b] == LEAF_EXPAND and keys[b] not in planned], dtype=np.int64)


# ------------------------------------------------------------------ fixtures
WIDE = ["wide64", "wide65", "widest", "wide_a0", "wide80", "one_move", "mated"]


def _positions(names):
    from golden_cases import STARTS, WIDTHS
    out = []
    for n in names:
        for sfx in ("", "_black"):
            if n + sfx in WIDTHS:
                t, k = WIDTHS[n + sfx]
                out.append((n + sfx, STARTS[n + sfx].copy(), t, k))
    return out


def _engine(pos, **kw):
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(len(pos), **kw)
    for b, (_, sq, t, _) in enumerate(pos):
        e.set_position(b, sq, t, 0)
    return e


def _assert_oracle_ids(info, pos):
    from oracle import OracleBoard
    for b, (name, sq, t, k) in enumerate(pos):
        ids = OracleBoard.from_array(sq, t, 0).legal_ids()
        assert len(ids) == k and info["k"][b] == k, name
        assert info["ids"][b][:k].tolist() == ids, name


def _family(name, B, dtype, legal, rs):
    """[B, 2086] logits of one family (float32 values first, then cast: the reference reads the cast values back)."""
    x = np.zeros((B, 2086), np.float32)
    for b in range(B):
        ill = np.setdiff1d(np.arange(2086), legal[b])
        if name.startswith("normal"):
            x[b] = rs.standard_normal(2086) * float(name.split("_")[1])
        elif name == "constant":
            x[b] = 1.5
        elif name == "max_illegal":                     # the maximum is not among the priors: legal d_i ~ 20-30
            x[b] = rs.standard_normal(2086) * 2.0
            x[b, ill[rs.randint(len(ill))]] = x[b].max() + 20.0
        elif name in ("max_2085", "max_0"):             # last / first element of the row, 100+ above the rest: a reduction that
            x[b] = rs.standard_normal(2086) * 2.0       # misses it overflows exp2 -- seen where that id is legal (prior 1, not NaN)
            x[b, 2085 if name == "max_2085" else 0] = 120.0
        elif name == "pm65000":                          # fp16-range extremes on legal and illegal ids
            x[b] = rs.standard_normal(2086) * 3.0
            if len(legal[b]):
                x[b, legal[b][rs.randint(len(legal[b]))]] = 65000.0 if b % 2 == 0 else -65000.0
            x[b, ill[rs.choice(len(ill), 8, replace=False)]] = -65000.0
            if b % 2:
                x[b, ill[rs.randint(len(ill))]] = 65000.0
        elif name == "ninf_illegal":
            x[b] = rs.standard_normal(2086) * 3.0
            x[b, ill[rs.choice(len(ill), 300, replace=False)]] = -np.inf
        else:
            raise ValueError(name)
    return torch.from_numpy(x).to("cuda:0").to(dtype).contiguous()


FAMILIES = ["normal_0.5", "normal_3", "normal_12", "constant", "max_illegal", "max_2085", "max_0", "pm65000", "ninf_illegal"]


# ------------------------------------------------------------------ (a) plain gather
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_plain_gather_against_float64_on_wide_and_edge_positions(dtype):
    """ccz_gather_priors (k_softmax_gather<T, false>: softmax_gather_board :654-747, fp16 dword loop :672-700, fp32 loop :701-708,
    p0 / p1 :713-714) on roots of 64 / 65 / 80 / 103 / 108 / 1 / 0 legal moves, both colours, for every logit family: each prior
    within the float64 bound; the mated board (CCZ_LEAF_LOSS) keeps its prior128 row byte for byte. A row maximum far above the rest
    sits on a LEGAL id at both ends of the row, so a max reduction that missed it (overflow: NaN) cannot pass: id 2085 on
    widest_black (the high half of the last, partial fp16 dword) and id 0 on wide_a0 (the low half of lane 0's first dword, lane
    0's first fp32 element)."""
    pos = _positions(WIDE)
    B = len(pos)
    e = _engine(pos, n_playout=8, seed=1)
    e.select_leaves()
    info = e.leaf_info()
    _assert_oracle_ids(info, pos)
    live = info["status"] == LEAF_EXPAND
    assert (~live).sum() == 2 and max(info["k"]) == 108           # the two mated roots are CCZ_LEAF_LOSS
    legal = [info["ids"][b][:info["k"][b]].astype(np.int64) for b in range(B)]
    rs = np.random.RandomState(11 if dtype == torch.float16 else 12)
    value = torch.zeros(B, dtype=torch.float32, device="cuda:0")
    for fam in FAMILIES:
        before, _ = e.leaf_priors(values=False)
        lg = _family(fam, B, dtype, legal, rs)
        e.gather_priors(lg, value)
        pri, _ = e.leaf_priors(values=False)
        assert_priors_f64(pri, info["ids"], info["k"], host_logits(lg), np.flatnonzero(live), f"{fam} {dtype}")
        assert np.array_equal(pri[~live].view(np.uint32), before[~live].view(np.uint32)), fam
        if fam == "constant":
            for b in np.flatnonzero(live):
                assert np.all(pri[b][:info["k"][b]] == np.float32(1.0 / 2086)), b
        if fam == "max_2085":
            b = [p[0] for p in pos].index("widest_black")
            assert info["ids"][b][info["k"][b] - 1] == 2085 and pri[b][info["k"][b] - 1] == 1.0
        if fam == "max_0":
            b = [p[0] for p in pos].index("wide_a0")
            assert info["k"][b] > 64 and info["ids"][b][0] == 0 and pri[b][0] == 1.0
    e.check_healthy()


# ------------------------------------------------------------------ (b) planned gather + cache hits on wide leaves
def _planned_sims(e, ev, n, tag, want_hits=None):
    """n planned simulations; every step checked against float64 and the plain gather. Returns the number of table hits on
    leaves with k > 64 that were checked."""
    leaf = e.select_leaves()
    wide_hits = 0
    for i in range(n):
        rows, nm = e.eval_plan()
        lg, v = ev(leaf, plan=(rows, nm))
        e.gather_priors_planned(lg, v)
        lgd, vd = ev(leaf)                               # the same evaluator densely: row b = board b's leaf
        info, live = check_boundary(e, lgd, vd, f"{tag} sim {i}")
        hits = hit_boards(e, info, rows, nm)
        wide_hits += int((info["k"][hits] > 64).sum()) if hits.size else 0
        if i + 1 < n:
            leaf = e.step_compact(None)
        else:
            e.expand_backup_compact(None)
    return wide_hits


@pytest.mark.parametrize("verify", [False, True])
def test_planned_gather_and_cache_hits_against_float64_on_wide_leaves(verify):
    """ccz_eval_plan + ccz_gather_priors_planned (softmax_gather_board<T, true>; the cache store :736-742, the verify check
    :717-731) and the probe's hit path (cache_probe_wave :775-806, out[64 + lane] = q1 :794) on duplicated wide roots: every
    CCZ_LEAF_EXPAND board's prior row -- fresh, shared or a table hit -- is bit-identical to the plain gather of its evaluator row
    and within the float64 bound; vleaf is the evaluator's value bit for bit. The search is repeated from fresh trees so that it
    meets its own positions in the table (hits on leaves with k > 64 are asserted). verify: CCZ_FLAG_CACHE_VERIFY recomputes
    one hit in 128 and compares all 128 lanes bit for bit (d0 / d1) -- no mismatch."""
    from test_gpu_eval_cache import LogitsEvaluator
    names = ["widest", "wide65", "wide64", "wide80", "widest", "wide65"]
    pos = [p for p in _positions(names) if p[3] > 64]
    pos = pos + pos[:4]                                  # duplicated positions: shared rows in one step
    e = _engine(pos, n_playout=48, seed=5, eval_cache_log2=14, cache_verify=verify)
    e.select_leaves()
    _assert_oracle_ids(e.leaf_info(), pos)
    ev = LogitsEvaluator(torch.device("cuda", 0), seed=3)
    _planned_sims(e, ev, 48, "first search")
    e.reset_tree()                                       # the same search again: its leaves are in the table now
    again = _planned_sims(e, ev, 48, "repeated search")
    for r in range(64):                                  # a search's first 65..108 simulations expand the root's (narrow) children:
        e.reset_tree()                                   # the wide leaves that come back are the roots, one hit per board each time
        again += _planned_sims(e, ev, 1, f"root again {r}")
    st = e.stats()
    assert again > 400, again
    assert st["cache_hits"] > 0 and st["cache_shared_rows"] > 0 and st["cache_stores"] > 0
    if verify:
        assert st["cache_verified"] > 0 and st["cache_verify_mismatches"] == 0, st
    e.check_healthy()


# ------------------------------------------------------------------ (c) routed gather
def test_routed_gather_against_float64_of_the_owners_logits():
    """ccz_eval_plan_routed + ccz_gather_priors_routed (k_softmax_gather_routed -> softmax_gather_board<T, true> with the owner's
    logits, value and salt): two evaluators, both colours of every wide fixture, each board's evaluator the owner of the root's
    side to move. Every board's priors are within the float64 bound of ITS OWNER's dense logits (and the plain gather of them),
    its value the owner's; the search is repeated from fresh trees for table hits under both salts."""
    from test_gpu_eval_cache import LogitsEvaluator
    pos = [p for p in _positions(["widest", "wide65", "wide64", "wide80"])]
    pos = pos + pos
    B = len(pos)
    e = _engine(pos, n_playout=24, seed=2, eval_cache_log2=14)
    red_net = np.array([b % 2 for b in range(B)], np.uint8)
    e.set_routing(red_net, salts=(0x1234567, 0x89ABCDEF))
    turn = np.array([p[2] for p in pos])
    owner = np.where(turn == 1, red_net, 1 - red_net).astype(bool)
    assert owner.any() and (~owner).any()
    dev = torch.device("cuda", 0)
    ev0, ev1 = LogitsEvaluator(dev, seed=1), LogitsEvaluator(dev, seed=2)
    m = torch.from_numpy(owner).to(dev)
    wide = 0
    for rep in range(18):                                # one search, then the roots again and again (table hits, both salts)
        if rep:
            e.reset_tree()
        leaf = e.select_leaves()
        n = 24 if rep == 0 else 1
        for i in range(n):
            p0, p1 = e.eval_plan_routed()
            lg0, v0 = ev0(leaf, plan=p0)
            lg1, v1 = ev1(leaf, plan=p1)
            e.gather_priors_routed(lg0, v0, lg1, v1)
            (d0, w0), (d1, w1) = ev0(leaf), ev1(leaf)
            lg = torch.where(m[:, None], d1, d0).contiguous()
            v = torch.where(m, w1, w0).contiguous()
            info, live = check_boundary(e, lg, v, f"routed rep {rep} sim {i}")
            wide += int((info["k"][live] > 64).sum())
            leaf = e.step_compact(None) if i + 1 < n else e.expand_backup_compact(None)
    assert wide > 100                                    # wide leaves met many times over (roots: fresh and table hits)
    st = e.stats()
    assert st["cache_hits"] > 0 and st["error_flags"] == 0
    e.check_healthy()


# ------------------------------------------------------------------ (d) compact search vs the oracle on wide roots
def _net():
    from test_gpu_scouts import _net as scouts_net
    return scouts_net()                                  # 2 x 256, hand-written: a row's result does not depend on its batch


def _safe_move(mcts_root_children, board):
    """The most visited root move after which the game goes on (a finished board has no live tree to compare)."""
    acts, visits, _, _ = mcts_root_children
    for j in np.argsort(-visits, kind="stable"):
        nb = board.copy()
        nb.push_id(int(acts[j]))
        if not nb.is_game_over():
            return int(acts[j])
    raise AssertionError("no move keeps the game going")


def _mirrored_planned_search(e, sm, pvn, n, tag):
    leaf = e.select_leaves()
    for i in range(n):
        rows, nm = e.eval_plan()
        lg, v = pvn.evaluate_leaves_logits(leaf, plan=(rows, nm))
        e.gather_priors_planned(lg, v)
        pri, val = e.leaf_priors()
        lgd, vd = pvn.evaluate_leaves_logits(leaf)
        check_boundary(e, lgd, vd, f"{tag} sim {i}", plain=False)   # first the float64 check of what the oracle will be fed
        sm.backup_on_oracles_compact(pri, val)
        if i + 1 < n:
            leaf = e.step_compact(None)
        else:
            e.expand_backup_compact(None)
    return sm.compare_roots()


def test_planned_search_on_wide_roots_matches_the_oracle_bit_for_bit():
    """expand_backup_phase<true> (cp0 / cp1 :515, children 64..127 :538-541) on roots of 64 .. 108 legal moves, both colours:
    11 boards, 2 moves x 100 simulations with tree reuse, the planned boundary, every board mirrored on a sequential oracle that is
    fed what the boundary hands the tree (after its float64 check): N / Q / P of every root bit-exact, before and after the move."""
    from gpu_harness import SampleMirror
    from oracle import OracleBoard
    pos = _positions(["widest", "wide65", "wide64", "wide80"])
    pos = pos + pos[:4]
    B = len(pos)
    pvn = _net()
    e = _engine(pos, n_playout=100, seed=7, eval_cache_log2=14)
    sm = SampleMirror(e, range(B), boards=[OracleBoard.from_array(sq, t, 0) for _, sq, t, _ in pos], check_every=1)
    for move in range(2):
        rc = _mirrored_planned_search(e, sm, pvn, 100, f"move {move}")
        assert np.all(rc["root_visits"] >= 100)
        if move == 0:
            assert min(rc["k"]) >= 64 and max(rc["k"]) == 108
        forced = np.array([_safe_move(sm.mcts[j].root_children(), sm.boards[j]) for j in range(B)], np.int32)
        e.finish_move(forced_moves=forced)
        sm.played(forced)
        sm.compare_roots()
    st = e.stats()
    assert st["cache_shared_rows"] > 0 and st["error_flags"] == 0
    e.check_healthy()


def _long_history(sq, turn, plies, seed):
    """`plies` quiet moves from (sq, turn) chosen on the oracle: no capture, no pawn move, no check, no repeated position, the
    game goes on -- the history chain (keys since the last capture) grows past one wave. The replies keep the position wide."""
    from oracle import OracleBoard
    rs = np.random.RandomState(seed)
    b = OracleBoard.from_array(sq, turn, 0)
    seen = {(b.squares().tobytes(), b.turn)}
    moves = []
    for _ in range(plies):
        cand = []
        for m in b.legal_ids():
            s = b.squares()
            from_, to = _move_squares(m)
            if s[to] or (s[from_] & 7) == 1:
                continue
            nb = b.copy()
            nb.push_id(m)
            key = (nb.squares().tobytes(), nb.turn)
            if key in seen or nb.in_check() or nb.is_game_over() or nb.is_tie():
                continue
            cand.append((m, nb, key))
        assert cand, "no quiet move left"
        if b.turn == (turn == 0):                        # the other side's reply: the one that leaves the root side the most moves
            m, b, key = max(cand, key=lambda c: len(c[1].legal_ids()))
        else:
            m, b, key = cand[rs.randint(len(cand))]
        seen.add(key)
        moves.append(m)
    return moves, b


def _move_squares(m):
    import oracle
    L = oracle.lib()
    return int(L.xq_move_from(m)), int(L.xq_move_to(m))


def _scout_roots():
    """(name, squares, turn, history moves): a wide root of each colour and one whose history chain is 67 keys long."""
    from golden_cases import STARTS
    hist, _ = _long_history(STARTS["wide80"], 1, 66, seed=4)    # 69 legal moves at the end
    return [("widest", STARTS["widest"], 1, []), ("wide65_black", STARTS["wide65_black"], 0, []), ("wide80+66", STARTS["wide80"], 1, hist)]


def _play_history(e, hist, B):
    forced = np.full(B, -1, np.int32)
    for m in hist:
        forced[0] = m
        e.finish_move(forced_moves=forced, keep_tree=False)
    e.check_healthy()


@pytest.mark.parametrize("root", [0, 1, 2], ids=["widest", "wide65_black", "chain67"])
def test_scouted_search_from_a_wide_root_is_the_unscouted_tree_and_the_oracle(root):
    """Scouts (scout_wave :443-488, the chain's second half :483; k_scouted_run :1034, its expansion from prior128 :1051) from a wide root: the tree of
    ScoutedSearch -- host loop and device loop -- equals, bit for bit, the tree of the unscouted planned search, which is checked
    against float64 at every step and against the sequential oracle (N / Q / P) at the end. One root has a history chain of 67
    keys (66 quiet plies played onto it): scout_wave reads chain entries 64.."""
    from gpu_harness import SampleMirror
    from oracle import OracleBoard
    from chinesechesszero_amd.engine import SelfPlayEngine
    from chinesechesszero_amd.selfplay import ScoutedSearch
    name, sq, turn, hist = _scout_roots()[root]
    pvn = _net()
    n = 200
    # the unscouted search, mirrored on the oracle
    e = SelfPlayEngine(1, n_playout=n, seed=9, eval_cache_log2=16, strict=True)
    e.set_position(0, sq, turn, 0)
    _play_history(e, hist, 1)
    ob = OracleBoard.from_array(sq, turn, 0)
    for m in hist:
        f, t = _move_squares(m)
        s = ob.squares()
        assert s[f] and not s[t] and (s[f] & 7) != 1, m      # no capture, no pawn move: nothing restarts the history chain
        ob.push_id(m)
    assert ob.halfmove == len(hist)
    if name == "wide80+66":
        assert len(hist) == 66                           # chain_len = 1 + 66 = 67 > 64: scout_wave :483 reads chain entries 64..
    sm = SampleMirror(e, [0], boards=[ob], check_every=1)
    want = _mirrored_planned_search(e, sm, pvn, n, name)
    assert int(want["k"][0]) > 64 and int(want["root_visits"][0]) == n
    e.check_healthy()
    for device_loop in (False, True):
        s_e = SelfPlayEngine(8, n_playout=n, seed=9, eval_cache_log2=16, strict=True)
        s_e.set_scouts(7)
        s_e.set_position(0, sq, turn, 0)
        _play_history(s_e, hist, 8)
        s = ScoutedSearch(s_e, pvn.evaluate_leaves_logits, use_graph=False, device_loop=device_loop)
        s.begin_move()
        left = n
        while left > 0:
            if device_loop:
                left -= s.run(left, left)
            else:
                s.simulate(last=left == 1)
                left -= 1
        got = s_e.root_children()
        for key in ("k", "acts", "visits", "root_visits"):
            assert np.array_equal(got[key][:1], want[key][:1]), (name, device_loop, key)
        for key in ("q", "prior"):
            assert np.array_equal(got[key][:1].view(np.uint32), want[key][:1].view(np.uint32)), (name, device_loop, key)
        assert 0 < s.evaluator_calls < n
        st = s_e.stats()
        assert st["sims"] == n and st["error_flags"] == 0
        s_e.check_healthy()
        s_e.close()
    e.close()


# ------------------------------------------------------------------ (e) the timed configuration, every board
def test_timed_path_every_expanded_board_against_float64():
    """The configuration bench.py times (test_gpu_timed_path.py: 4096 boards, the 40 x 256 net, a 2^20-entry table, after its
    preroll), with every 16th board moved onto a wide fixture: 8 planned simulations. At each, the same leaf batch is evaluated
    densely without a plan (bit-identical to the planned rows: test_gpu_evaluator_depth.py), and EVERY CCZ_LEAF_EXPAND board --
    fresh, shared or a table hit -- gets priors within the float64 bound of its dense logits and its dense value bit for bit."""
    from golden_cases import STARTS, WIDTHS
    from test_gpu_timed_path import preroll
    from chinesechesszero_amd.net import PolicyValueNet
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pvn = PolicyValueNet(device=dev)
    B, n = 4096, 8
    sp = BatchedSelfPlay(pvn.evaluate_leaves_logits, B, n_playout=n, seed=7, max_plies=64, eval_cache_log2=20)
    assert sp.planned
    e = sp.engine
    preroll(e, 6)
    wide = [w for w in WIDTHS if WIDTHS[w][1] > 64]
    for i, b in enumerate(range(0, B, 16)):
        w = wide[i % len(wide)]
        e.set_position(b, STARTS[w].copy(), WIDTHS[w][0], 0)
    leaf = e.select_leaves()
    checked = wide_checked = 0
    for i in range(n):
        lg, v = sp._planned_eval(leaf)
        e.gather_priors_planned(lg, v)
        info = e.leaf_info()
        pri, val = e.leaf_priors()
        lgd, vd = pvn.evaluate_leaves_logits(leaf)
        live = info["status"] == LEAF_EXPAND
        assert_priors_f64(pri, info["ids"], info["k"], host_logits(lgd), np.flatnonzero(live), f"timed sim {i}")
        assert np.array_equal(val[live].view(np.uint32), vd.cpu().numpy()[live].view(np.uint32)), i
        checked += int(live.sum())
        wide_checked += int((info["k"][live] > 64).sum())
        leaf = e.step_compact(None) if i + 1 < n else e.expand_backup_compact(None)
    assert checked > 0.9 * B * n and wide_checked >= 256      # (the wide roots; their children are the other side's, narrow)
    st = e.stats()
    assert st["cache_hits"] > 0 and st["cache_shared_rows"] > 0 and st["error_flags"] == 0
    e.check_healthy()
    e.close()
