"""GPU: engine snapshots (include/cczero.h "Engine snapshots") -- a self-play run saved at a move boundary and resumed in another
engine object goes on bit for bit: harvested records, moves, the tops of the trees, proof bytes, game status and every counter but the
evaluation cache's. Exact, no tolerance anywhere.

Set-up of every run: ``BatchedSelfPlay`` with 70 boards (no multiple of 64), 24 simulations a move, a ply cap of 8 (so that games are
adjudicated, harvested and restarted inside the eleven moves of a run) and a pool of 4096 nodes per half. The evaluator is a hash of
the leaf planes computed on the device in 64-bit integers: a deterministic function of the position whose bits do not depend on the
batch a row sits in. A run plays 5 moves (five flips: pool half 1 is live), saves, and plays 6 more with a harvest after each.

The issue's case (b) names Gumbel and the early stop together; the engine refuses that pair (options.SearchOptions: sequential halving
plans the whole budget), so it is run as the two closest legal halves: ``gumbel`` = Gumbel + search parameters + solver and ``stop``
= search parameters + early stop + solver.

``root_children()`` is read after the move's harvest: a board that was adjudicated at the ply cap stays in the pool half it was left
in when the halves flipped, so until the harvest restarts it the live half holds an older move's nodes at its index -- memory no
later call depends on, and the one thing a snapshot (which saves the board's own half) does not carry."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from budget_twin import ua

pytestmark = pytest.mark.gpu
B, N, PLIES, CAP, SEED = 70, 24, 8, 4096, 11
N_FAST, P_FULL = 8, 0.5
CASES = {
    "cap": dict(playout_cap=(N_FAST, P_FULL), root_exploration=dict(eps=0.25), solver=True,
                resign=dict(threshold=-0.2, consecutive=1, min_ply=2, p_playon=0.3)),
    "gumbel": dict(gumbel=dict(max_considered=8), search=dict(fpu_mode=1, fpu_value=0.3, c_factor=1.0), solver=True),
    "stop": dict(search=dict(fpu_mode=1, fpu_value=0.3, c_factor=1.0), solver=True,
                 early_stop=dict(single_reply=True, gap_factor=1.0, kld_interval=8, min_gain=1e-3, min_sims=4)),
    # a pool so tight that re-roots prune kept subtrees (not strict: pruning only counts): 100 kept nodes, room for a move's expansions
    "tight": dict(root_exploration=dict(eps=0.25), solver=True, max_nodes=1500, reserve_nodes=1400),
}


class HashEval:
    """Logits and value as a hash of the leaf planes, in int64 on the device (wrap-around products, exact sums)."""
    batched = returns_logits = stateless = graph_safe = True

    def __init__(self, salt=7):
        r = np.random.RandomState(salt)
        odd = lambda n: torch.from_numpy((r.randint(0, 2**62, size=n, dtype=np.int64) | 1)).to("cuda:0")
        self.c, self.a, self.av = odd(17 * 7 * 10 * 9), odd(2086), odd(1)

    def __call__(self, leaf):
        x = (leaf.reshape(leaf.shape[0], -1) != 0).to(torch.int64)
        key = (x * self.c).sum(1)
        logits = (((key[:, None] * self.a[None, :]) >> 40) & 0xFF).to(torch.float32) / 32.0
        value = (((key * self.av) >> 40) & 0xFF).to(torch.float32) / 128.0 - 1.0
        return logits.contiguous(), value.contiguous()


def make(case, n_boards=B, seed=SEED, base=0, **over):
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    kw = dict(n_playout=N, seed=seed, board_id_base=base, max_plies=PLIES, max_nodes=CAP)
    kw.update(CASES[case])
    kw.update(over)
    return BatchedSelfPlay(HashEval(), n_boards, **kw)


def observe(sp):
    e = sp.engine
    return dict(roots=e.root_children(), proof=e.root_proof(), status=e.game_status(),
                stats={k: v for k, v in e.stats().items() if not k.startswith("cache_") and k != "hbm_bytes"},   # (hbm_bytes: an allocation figure)
                resign=e.resign_stats(), resign_status=e.resign_status(), explore=e.exploration_stats(), gumbel=e.gumbel_stats(),
                solver=e.solver_stats(), stop=e.early_stop_stats())


def play_move(sp, harvest=True):
    moves = sp.run_move().cpu().numpy().copy()
    rec = [c.cpu().numpy().copy() for c in sp.harvest_record_chunks()] if harvest else []
    out = observe(sp)
    out.update(moves=moves, records=np.concatenate(rec) if rec else np.zeros((0,), np.uint8))
    return out


def play(sp, n, harvest=True):
    return [play_move(sp, harvest) for _ in range(n)]


def same(a, b, path="run"):
    """Bit for bit: arrays by their bytes (NaN payloads included), everything else by ==."""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{path}: {a.dtype}{a.shape} / {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.nonzero(a.reshape(a.shape[0], -1).view(np.uint8) != b.reshape(b.shape[0], -1).view(np.uint8))[0] if a.ndim else [0]
            raise AssertionError(f"{path} differs (first axis indices {sorted(set(int(i) for i in bad))[:8]})")
    else:
        assert a == b, f"{path}: {a!r} != {b!r}"


@functools.lru_cache(maxsize=None)
def reference(case):
    """5 moves, state_dict, 6 more moves: (the state, what the 6 moves did). Computed once per case and left unchanged."""
    sp = make(case)
    play(sp, 5)
    state = sp.state_dict()
    state["engine"] = state["engine"].cpu()      # (kept on the host between the tests)
    tail = play(sp, 6)
    sp.engine.check_healthy()
    assert sum(len(t["records"]) for t in tail) > 0, "no game ended inside the run: the harvest was never compared"
    sp.engine.close()
    return state, tail


# ------------------------------------------------------------------------------------------------------------------ 1: continuation
@pytest.mark.parametrize("case", ["cap", "gumbel", "stop"])
def test_continuation(case):
    state, tail = reference(case)
    from chinesechesszero_amd.snapshot import snapshot_info
    assert snapshot_info(state["engine"])["half"] == 1      # five flips
    sp = make(case)
    sp.load_state_dict(state)
    same(tail, play(sp, 6))


@pytest.mark.parametrize("dirty_moves", [3, 4])
def test_continuation_into_a_dirty_engine(dirty_moves):
    """The receiver has played other games (its first move forced to every root's last child), holds trees, records and counters of
    its own and an allocated proof array; after 3 moves its live half is the blob's, after 4 the other one."""
    state, tail = reference("cap")
    sp = make("cap")
    e = sp.engine
    sp.search()
    rc = e.root_children()
    e.finish_move(forced_moves=rc["acts"][np.arange(B), rc["k"] - 1].astype(np.int32))
    play(sp, dirty_moves - 1, harvest=False)
    assert e.stats()["moves"] > B and e.snapshot_size() != state["engine"].numel()
    sp.load_state_dict(state)
    same(tail, play(sp, 6))


# ------------------------------------------------------------------------------------------------------------------ 2: saving changes nothing
def test_saving_changes_nothing():
    _, tail = reference("cap")
    sp = make("cap")
    play(sp, 5)
    same(tail, play(sp, 6))


# ------------------------------------------------------------------------------------------------------------------ 3: every lifecycle state
def test_every_lifecycle_state():
    """One blob with a board that is over and awaits its harvest, a freshly reset board, a board one ply below the cap and a board whose
    kept tree was pruned at a re-root; read back from the blob with snapshot_info, then the continuation."""
    from chinesechesszero_amd.snapshot import fixed_row, snapshot_info

    def prefix(sp):
        e = sp.engine
        for i in range(1, PLIES + 2):        # the last finish_move adjudicates the boards that stand at the ply cap
            play_move(sp, harvest=False)
            if i in (1, 2):
                e.reset(np.arange(B) % 4 == i)
        e.reset(np.arange(B) == 3)

    sp = make("tight")
    prefix(sp)
    state = sp.state_dict()                  # before the harvest
    blob = state["engine"]
    info = snapshot_info(blob)
    n_nodes, ply, over = info["n_nodes"], info["ply"], info["over"]
    pruned = np.array([fixed_row(blob, info, b, "stats").view("<u8")[8] for b in range(B)])
    assert (over == 1).any() and ((over == 1) & (ply == PLIES)).any()
    assert n_nodes[3] == 1 and ply[3] == 0 and over[3] == 0
    assert ((ply == PLIES - 1) & (over == 0)).any()
    assert ((pruned > 0) & (n_nodes > 1) & (over == 0)).any()
    assert n_nodes[over == 0].max() <= 1500 - 1400          # (a kept tree fits what the re-root leaves it; a board that is over
    assert n_nodes[over == 1].max() > 1500 - 1400           # holds its last search whole: it never re-rooted)
    tail = play(sp, 6)
    sp2 = make("tight")
    sp2.load_state_dict(state)
    same(tail, play(sp2, 6))


# ------------------------------------------------------------------------------------------------------------------ 4: file and host
def test_round_trip_through_a_file_and_the_host(tmp_path):
    state, tail = reference("gumbel")
    blob = state["engine"]
    path = str(tmp_path / "engine.pt")
    torch.save(blob, path)
    sp = make("gumbel")
    sp.engine.load_state(path)
    same(tail, play(sp, 6))
    sp2 = make("gumbel")
    sp2.engine.load_state(blob.to("cuda:0"))                 # host -> device: a device tensor is taken as it is
    same(tail[:2], play(sp2, 2))


# ------------------------------------------------------------------------------------------------------------------ 5: size
def test_size_identity_and_capacity_contract():
    from chinesechesszero_amd import snapshot as S
    sp = make("cap")
    play(sp, 5, harvest=False)
    e = sp.engine
    blob = e.save_state()
    info = S.snapshot_info(blob)
    assert info["sections"] == S.SNAP_PROOF | S.SNAP_VALUES
    sizes = S.section_bytes(info["n_nodes"], info["ply"], info["pi_used"], info["sections"])
    want = S.HEADER_BYTES + S.directory_bytes(B)
    want = (want + 15) // 16 * 16 + int(sizes.sum())
    assert blob.numel() == want == e.snapshot_size() == info["total_bytes"]
    assert (info["section_sizes"] == sizes).all() and info["sections_start"] % 16 == 0 and (info["offsets"] % 16 == 0).all()
    # what is copied is the live prefixes, not the pool: B x 2 x cap x 20 bytes of node records alone
    assert blob.numel() < B * 2 * CAP * 20 // 2
    n = blob.numel()
    arena = torch.full((n + 256,), 0xFF, dtype=torch.uint8, device="cuda:0")
    got = C.c_uint64(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert e.L.ccz_snapshot_save(e.h, stream, C.c_void_p(arena.data_ptr()), n - 1, C.byref(got)) == -1
    assert got.value == n and bool((arena == 0xFF).all())                       # refused, nothing written
    from chinesechesszero_amd import _lib
    assert b"capacity" in _lib.lib().ccz_last_error()
    assert e.L.ccz_snapshot_save(e.h, stream, C.c_void_p(arena.data_ptr()), n, C.byref(got)) == 0
    assert got.value == n and bool((arena[n:] == 0xFF).all()) and torch.equal(arena[:n], blob)


# ------------------------------------------------------------------------------------------------------------------ 6: the layout kernel
@pytest.mark.parametrize("n_boards", [1, 64, 65, 257, 8209])
@pytest.mark.parametrize("sections", [0, 1, 2, 3])
def test_layout_kernel_against_cumsum(n_boards, sections):
    from chinesechesszero_amd import snapshot as S
    from chinesechesszero_amd.engine import snapshot_layout
    cap, max_plies = (400 + 64) * 512, 2048           # the sizes of a default engine
    r = np.random.RandomState(n_boards * 4 + sections)
    n_nodes = r.randint(1, cap + 1, size=n_boards).astype(np.int32)
    ply = r.randint(0, max_plies + 1, size=n_boards).astype(np.int32)
    pi_used = r.randint(0, max_plies * 80 + 1, size=n_boards).astype(np.uint32)
    off = snapshot_layout(n_nodes, ply, pi_used, sections)
    want = np.concatenate([[np.uint64(0)], np.cumsum(S.section_bytes(n_nodes, ply, pi_used, sections), dtype=np.uint64)])
    assert off.dtype == np.uint64 and (off == want).all()
    if n_boards == 8209:
        assert int(off[-1]) > 2**32                    # full-size counts: the total does not fit 32 bits


def test_layout_kernel_at_the_limits():
    """Every board at its caps (the largest section there is), and the smallest one."""
    from chinesechesszero_amd import snapshot as S
    from chinesechesszero_amd.engine import snapshot_layout
    cap, max_plies = (400 + 64) * 512, 2048
    for n, p, u in ((cap, max_plies, max_plies * 80), (1, 0, 0)):
        off = snapshot_layout(np.full(1025, n, np.int32), np.full(1025, p, np.int32), np.full(1025, u, np.uint32), 3)
        assert (off == np.arange(1026, dtype=np.uint64) * S.section_bytes(n, p, u, 3)).all()


# ------------------------------------------------------------------------------------------------------------------ 7: refusals
def _refused(fn, *words):
    from chinesechesszero_amd._lib import CczError
    with pytest.raises(CczError) as ei:
        fn()
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


def test_refusals_leave_the_engine_untouched():
    from chinesechesszero_amd import snapshot as S
    state, tail = reference("cap")
    good = state["engine"]
    info = S.snapshot_info(good)
    sp = make("cap")
    play(sp, 5)
    # inside a move
    sp.advance(3)
    with pytest.raises(RuntimeError, match="inside a move"):
        sp.state_dict()
    with pytest.raises(RuntimeError, match="inside a move"):
        sp.load_state_dict(state)
    sp.advance(N - 3 - 1)
    sp.advance(1, boundary=lambda: None)      # the move's last simulation, not played: a move boundary for this object again ...
    e = sp.engine
    before = e.save_state().cpu()
    # ... malformed blobs into the engine that stands in the middle of its run
    bad = good.clone(); bad[0] ^= 0xFF
    _refused(lambda: e.load_state(bad), "magic")
    _refused(lambda: e.load_state(good[:-16]), "total size")
    _refused(lambda: e.load_state(good[:300]), "truncated")
    bad = good.clone()
    off = bad[S.HEADER_BYTES:S.HEADER_BYTES + 8 * (B + 1)].numpy().view("<u8")
    off[5], off[6] = off[6], off[5]
    _refused(lambda: e.load_state(bad), "offsets", "monotone")
    bad = good.clone()
    meta = bad[S.HEADER_BYTES + 8 * (B + 1):S.HEADER_BYTES + S.directory_bytes(B)].numpy().view(S.META_DTYPE)
    meta["n_nodes"][9] = CAP + 1
    _refused(lambda: e.load_state(bad), "n_nodes", "cap")
    bad = good.clone()
    meta = bad[S.HEADER_BYTES + 8 * (B + 1):S.HEADER_BYTES + S.directory_bytes(B)].numpy().view(S.META_DTYPE)
    meta["ply"][9] = PLIES + 1
    _refused(lambda: e.load_state(bad), "ply", "max_plies")
    assert torch.equal(before, e.save_state().cpu())
    # ... and the good blob into engines that differ in one thing each
    others = {
        "B": dict(n_boards=64), "cap": dict(max_nodes=CAP + 16), "max_plies": dict(max_plies=PLIES + 1), "seed": dict(seed=SEED + 1),
        "flags": dict(mirror=False), "rule_flags": dict(perpetual_check=not e.perpetual_check), "board_id_base": dict(base=4096),
        "resign.threshold": dict(resign=dict(threshold=-0.25, consecutive=1, min_ply=2, p_playon=0.3)), "solver": dict(solver=False),
        "root_exploration.enabled": dict(root_exploration=None),
    }
    for field, kw in others.items():
        o = make("cap", **kw)
        was = o.engine.save_state().cpu()
        _refused(lambda: o.engine.load_state(good), field + " ", "differs")
        assert torch.equal(was, o.engine.save_state().cpu()), field
        o.engine.close()
    # the engine that refused all of the above goes on as if nothing had happened: its sixth move was searched above
    moves = sp.finish_move().cpu().numpy().copy()
    rec = [c.cpu().numpy().copy() for c in sp.harvest_record_chunks()]
    got = observe(sp)
    got.update(moves=moves, records=np.concatenate(rec) if rec else np.zeros((0,), np.uint8))
    same(tail, [got] + play(sp, 5))


# ------------------------------------------------------------------------------------------------------------------ 8: keep_board_id_base
def test_keep_board_id_base():
    """A blob saved at base 0 in an engine created at base 4096: from the load on every Philox word of board b is drawn with id
    4096 + b. Seen directly in the playout-cap lot (word 0xffe of the move, tests/budget_twin.py), move after move."""
    from chinesechesszero_amd.snapshot import snapshot_info
    state, tail = reference("cap")
    sp = make("cap", base=4096)
    sp.load_state_dict(state, keep_board_id_base=True)
    e = sp.engine
    differs = False
    for i in range(6):
        mc = snapshot_info(e.save_state())["meta"]["move_counter"]
        sp.advance(1)                                   # the move's first simulation draws the budgets
        got = e.budgets_out.cpu().numpy()
        u_here = np.array([ua(SEED, 4096 + b, int(mc[b])) for b in range(B)])
        u_base0 = np.array([ua(SEED, b, int(mc[b])) for b in range(B)])
        assert (got == np.where(u_here < P_FULL, N, N_FAST)).all(), i
        differs |= bool(((u_here < P_FULL) != (u_base0 < P_FULL)).any())
        moves = sp.run_move().cpu().numpy()
        if i == 0:
            assert (moves != tail[0]["moves"]).any()    # other budgets, other noise, other draws: not the games of base 0
        list(sp.harvest_record_chunks())
    assert differs
    assert snapshot_info(e.save_state())["board_id_base"] == 4096
    e.check_healthy()
