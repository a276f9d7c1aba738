"""GPU: the checkpoint arena (chinesechesszero_amd/arena.py) and its routed evaluator boundary (ccz_set_routing /
ccz_eval_plan_routed / ccz_gather_priors_routed, include/cczero.h). The bar: the arena searches exactly what a driver built
from the already-validated dense calls searches -- both networks evaluate every row, each board takes the rows of the network
that owns its move -- and one network's evaluation is never served to the other."""
import numpy as np
import pytest
import torch

from chinesechesszero_amd import _lib

pytestmark = pytest.mark.gpu


def _nets(seeds, channels=256, blocks=2):
    from chinesechesszero_amd.net import PolicyValueNet
    out = []
    for s in seeds:
        torch.manual_seed(s)
        out.append(PolicyValueNet(device="cuda:0", num_channels=channels, resblocks_num=blocks))
    return out


def _logits_evaluators(seeds):
    from test_gpu_eval_cache import LogitsEvaluator
    return [LogitsEvaluator(torch.device("cuda", 0), seed=s) for s in seeds]


def _dense_twin(ar, seed=0):
    """A cache-less engine on the arena's openings, the same settings: what the reference driver searches on."""
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(ar.B, n_playout=ar.n_playout, eps=0.0, alpha=0.2, temp=ar.temp, seed=seed, max_plies=ar.max_plies, mirror=False)
    sq, turn, half = ar.openings
    for b in range(ar.B):
        i = ar.opening_of[b]
        e.set_position(b, sq[i], int(turn[i]), int(half[i]))
    return e


def _owner(ar, turn):
    """Board b's evaluator for the move: the owner of the root's side to move."""
    return np.where(turn == 1, ar.red_net, 1 - ar.red_net).astype(np.uint8)


def _dense_select(lg0, v0, lg1, v1, owner):
    m = torch.from_numpy(owner.astype(bool)).to(lg0.device)
    return torch.where(m[:, None], lg1, lg0).contiguous(), torch.where(m, v1, v0).contiguous()


def _same_roots(a, b, boards=None):
    sl = slice(None) if boards is None else boards
    for key in ("k", "acts", "visits", "root_visits"):
        assert np.array_equal(a[key][sl], b[key][sl]), key
    assert np.array_equal(a["q"][sl].view(np.uint32), b["q"][sl].view(np.uint32))
    assert np.array_equal(a["prior"][sl].view(np.uint32), b["prior"][sl].view(np.uint32))


@pytest.mark.parametrize("layout", ["nhwc", "g16"])
def test_routing_is_exact_against_the_dense_driver(layout, monkeypatch):
    """40 pairs (80 boards: from 65 boards on CCZ_CONV_LAYOUT=g16 takes the group-of-16 rows), two different 2-block nets, 16
    playouts, 4-ply openings, a 40-ply cap: root children (visits, acts, Q and prior bits) on ALL boards before every move and the
    moves played are those of the reference driver -- select_leaves, both nets on ALL rows densely, torch.where by owner,
    step_logits / expand_backup_logits, finish_move(keep_tree=False) at the same temperatures."""
    monkeypatch.setenv("CCZ_CONV_LAYOUT", layout)
    from chinesechesszero_amd.arena import Arena
    na, nb = _nets((1, 2))
    ar = Arena(na, nb, 40, n_playout=16, opening_plies=4, seed=0, max_plies=40, eval_cache_log2=16)
    ev0, ev1 = ar.ev
    ref = _dense_twin(ar)
    n, moves_played = ar.n_playout, 0
    while not ar.engine.game_status()["over"].all():
        st = ref.game_status()
        assert np.array_equal(st["turn"], ar.engine.game_status()["turn"])
        owner = _owner(ar, st["turn"])
        leaf = ref.select_leaves()
        for i in range(n):
            lg, v = _dense_select(*ev0(leaf), *ev1(leaf), owner)
            if i + 1 < n:
                leaf = ref.step_logits(lg, v)
            else:
                ref.expand_backup_logits(lg, v)
        ar.search()
        _same_roots(ar.engine.root_children(), ref.root_children())
        m_ref = ref.finish_move(temps=np.full(ar.B, ar.temp), keep_tree=False).cpu().numpy()
        m_ar = ar.finish_move()
        assert np.array_equal(m_ar, m_ref)
        moves_played += int((m_ar >= 0).sum())
    assert moves_played > 10 * ar.B
    assert np.array_equal(ar.engine.game_status()["winner"], ref.game_status()["winner"])
    s = ar.engine.stats()
    assert s["cache_hits"] > 0 and s["error_flags"] == 0
    ar.engine.check_healthy()


def test_no_cross_net_cache_hits():
    """Move 1: boards 2i and 2i+1 hold the same position, searched by opposite networks. Every board's leaf priors and value
    (leaf_priors) are its OWN network's dense output for that position -- in the first simulation (one key, two owners: the
    salted keys keep them apart) and in the next ones (entries of the other network are in the table by then)."""
    from chinesechesszero_amd.arena import Arena
    na, nb = _nets((1, 2))
    ar = Arena(na, nb, 40, n_playout=8, opening_plies=4, seed=3, eval_cache_log2=16)
    ev0, ev1 = ar.ev
    e, ref = ar.engine, _dense_twin(ar)
    owner = _owner(ar, e.game_status()["turn"])
    assert np.array_equal(owner[0::2], np.zeros(ar.P)) and np.array_equal(owner[1::2], np.ones(ar.P))
    ar._sync_routing()
    leaf, rleaf = e.select_leaves(), ref.select_leaves()
    for i in range(ar.n_playout):
        p0, p1 = e.eval_plan_routed()
        lg0, v0 = ev0(leaf, plan=p0)
        lg1, v1 = ev1(leaf, plan=p1)
        e.gather_priors_routed(lg0, v0, lg1, v1)
        pri, val = e.leaf_priors()
        # the expected numbers: both nets densely on the same leaves, each board's owner picked, the unplanned gather
        assert torch.equal(leaf, rleaf)
        lg, v = _dense_select(*ev0(rleaf), *ev1(rleaf), owner)
        ref.gather_priors(lg, v)
        want, _ = ref.leaf_priors(values=False)
        info = e.leaf_info()
        live = info["status"] == _lib.LEAF_EXPAND
        assert live.sum() > 0
        assert np.array_equal(pri[live].view(np.uint32), want[live].view(np.uint32)), i
        assert np.array_equal(val[live].view(np.uint32), v.cpu().numpy()[live].view(np.uint32)), i
        if i == 0:   # the pair's boards share the position but not the network: their numbers differ
            assert np.all(info["status"] == _lib.LEAF_EXPAND)
            assert np.all(val[0::2] != val[1::2])
            n = e.n_miss2.cpu().numpy()
            assert n[0] == ar.P and n[1] == ar.P          # one row per opening, per network
        leaf = e.step_compact(None)
        rleaf = ref.step_compact(v)
    assert e.stats()["cache_stores"] >= 2 * ar.P
    e.check_healthy()


def _unique_argmax(rc, b):
    k = rc["k"][b]
    v = rc["visits"][b][:k]
    return k > 0 and int((v == v.max()).sum()) == 1


def test_identical_weights_play_identical_pairs():
    """A and B with the same weights: the two games of a pair are the same game, move for move, and a pair scores exactly 1
    point -- up to exact visit-count ties at the root, which the per-board random stream breaks (temperature 1e-3 samples among
    the tied arg-max children): a pair is compared up to its first tied move, and a pair that never meets one must score 1."""
    from chinesechesszero_amd.arena import Arena
    ea, eb = _logits_evaluators((7, 7))
    ar = Arena(ea, eb, 32, n_playout=48, opening_plies=6, seed=1, max_plies=30, eval_cache_log2=16)
    tie_at = np.full(ar.P, -1)          # moves of the pair's games before its first tied root (-1: none so far)

    def before_move(a):
        rc = a.engine.root_children()
        over = a.engine.game_status()["over"]
        for i in range(a.P):
            if tie_at[i] >= 0 or over[2 * i] or over[2 * i + 1]:
                continue
            for key in ("k", "acts", "visits"):
                assert np.array_equal(rc[key][2 * i], rc[key][2 * i + 1]), (i, key)
            assert np.array_equal(rc["q"][2 * i].view(np.uint32), rc["q"][2 * i + 1].view(np.uint32))
            if not _unique_argmax(rc, 2 * i):
                tie_at[i] = len(a.game_moves(2 * i))

    r = ar.play(before_move=before_move)
    st = ar.engine.game_status()
    w = st["winner"].astype(int)
    compared = 0
    for i in range(ar.P):
        g0, g1 = ar.game_moves(2 * i), ar.game_moves(2 * i + 1)
        if tie_at[i] < 0:
            assert g0 == g1, i
            pts = sum(0.5 if w[b] == -1 else float(w[b] == ar.a_colour[b]) for b in (2 * i, 2 * i + 1))
            assert pts == 1.0, i
            compared += len(g0)
        else:
            assert g0[:tie_at[i]] == g1[:tie_at[i]], i
            compared += tie_at[i]
    assert compared >= 3 * ar.P, compared
    assert r["unfinished"] == 0 and r["wins"] + r["draws"] + r["losses"] == ar.B


def test_cache_verify_over_a_short_match():
    """CCZ_FLAG_CACHE_VERIFY for a whole short match: a sample of the hits is evaluated again -- by the hit's own network, in that
    network's segment -- and every one agrees bit for bit."""
    from chinesechesszero_amd.arena import Arena
    na, nb = _nets((1, 2))
    ar = Arena(na, nb, 40, n_playout=16, opening_plies=4, seed=5, max_plies=24, eval_cache_log2=16, cache_verify=True)
    r = ar.play()
    s = ar.engine.stats()
    assert s["cache_verified"] > 0 and s["cache_verify_mismatches"] == 0 and s["error_flags"] == 0
    assert r["cache"]["cache_verified"] == s["cache_verified"]


def test_only_live_rows_are_planned():
    """In every step the two segments together hold no more rows than there are boards with an expansion pending, every row is
    a board owned by its segment's network; once every game is over, both counts are 0."""
    from chinesechesszero_amd.arena import Arena
    ea, eb = _logits_evaluators((1, 2))
    ar = Arena(ea, eb, 24, n_playout=12, opening_plies=6, seed=2, max_plies=50, eval_cache_log2=14)
    seen = {"steps": 0, "rows": 0}

    def on_step(a, p0, p1):
        info = a.engine.leaf_info()
        owner = _owner(a, a.engine.game_status()["turn"])
        pending = info["status"] == _lib.LEAF_EXPAND
        n0, n1 = (int(p[1].item()) for p in (p0, p1))
        assert n0 + n1 <= int(pending.sum())
        for k, (rows, n) in enumerate(((p0[0], n0), (p1[0], n1))):
            r = rows[:n].cpu().numpy()
            assert np.all(np.diff(r) > 0) and np.all(pending[r]) and np.all(owner[r] == k), k
        seen["steps"] += 1
        seen["rows"] += n0 + n1

    res = ar.play(on_step=on_step)
    assert seen["steps"] == res["steps"] and seen["rows"] == round(sum(res["rows_per_step"]) * res["steps"])
    assert ar.engine.game_status()["over"].all()
    ar.engine.select_leaves()
    ar.engine.eval_plan_routed()
    assert ar.engine.n_miss2.cpu().numpy().tolist() == [0, 0]


def test_games_replay_on_the_oracle():
    """Every game, from its opening, replays legally on the CPU oracle's rules, ends where the engine says, with the winner the
    engine reports (a game cut at max_plies is a draw, counted as truncated). The openings are distinct, and the pairs play
    different games."""
    from oracle import OracleBoard
    from chinesechesszero_amd.arena import Arena
    ea, eb = _logits_evaluators((1, 2))
    cap = 80
    ar = Arena(ea, eb, 24, n_playout=16, opening_plies=6, seed=4, max_plies=cap, eval_cache_log2=14)
    sq, turn, half = ar.openings
    assert len({(bytes(sq[i]), int(turn[i])) for i in range(ar.P)}) == ar.P
    res = ar.play()
    st = ar.engine.game_status()
    truncated = 0
    for b in range(ar.B):
        i = ar.opening_of[b]
        ob = OracleBoard.from_array(sq[i], int(turn[i]), int(half[i]))
        mv = ar.game_moves(b)
        for t, m in enumerate(mv):
            assert not ob.is_game_over() and m in ob.legal_ids(), (b, t, m)
            ob.push_id(m)
        assert len(mv) == st["plies"][b]
        if ob.is_game_over():
            o = ob.outcome()
            assert int(st["winner"][b]) == (-1 if o.winner is None else int(o.winner)), b
            assert not ar.truncated[b]
        else:
            assert ar.truncated[b] and st["plies"][b] == cap and st["winner"][b] == -1
            truncated += 1
    assert res["truncated"] == truncated
    assert len({tuple(ar.game_moves(b)) for b in range(0, ar.B, 2)}) == ar.P
    assert sum(res["pentanomial"]) == ar.P and res["wins"] + res["draws"] + res["losses"] == ar.B


def test_refusals():
    from chinesechesszero_amd.arena import Arena
    from chinesechesszero_amd.engine import SelfPlayEngine
    from chinesechesszero_amd.net import uniform_evaluator
    red = np.array([0, 1, 0, 1], np.uint8)
    e = SelfPlayEngine(4, n_playout=4)
    with pytest.raises(_lib.CczError, match="evaluation cache"):
        e.set_routing(red, (1, 2))
    e = SelfPlayEngine(4, n_playout=4, eval_cache_log2=10)
    with pytest.raises(_lib.CczError, match="no routing"):
        e.miss_rows2 = torch.zeros(8, dtype=torch.int32, device=e.device)
        e.n_miss2 = torch.zeros(2, dtype=torch.int32, device=e.device)
        e.eval_plan_routed()
    with pytest.raises(_lib.CczError, match="different salts"):
        e.set_routing(red, (5, 5))
    with pytest.raises(_lib.CczError, match="0 or 1"):
        e.set_routing(np.array([0, 2, 0, 1], np.uint8), (1, 2))
    e.set_scouts(1)
    with pytest.raises(_lib.CczError, match="scout"):
        e.set_routing(red, (1, 2))
    e.set_scouts(0)
    e.set_routing(red, (1, 2))       # accepted once the scouts are gone
    e.set_routing(None)
    ea, = _logits_evaluators((1,))
    with pytest.raises(TypeError, match="plan-capable"):
        Arena(ea, uniform_evaluator, 2, n_playout=4)
    with pytest.raises(ValueError, match="eval_cache_log2"):
        Arena(ea, ea, 2, n_playout=4, eval_cache_log2=0)
