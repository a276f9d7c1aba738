"""GPU: root exploration in the search (ccz_set_root_exploration, include/cczero.h) against the CPU model of
tests/explore_model.py. Exact, no tolerance: visits, Q and prior bits, the noise table, the recorded pi bytes, moves and counters.

Inputs (explore_model.inputs): 16 boards -- 14 a few forced plies from the opening with 30 to 50 legal moves, `widest` (108 moves:
the second pass of the child loop) and `pawns` (7 moves) --, 96 simulations a move (160 on the wide board, past its visit-every-child
pass) set through ccz_set_budgets, two moves with tree reuse. tests/test_cpu_explore_model.py asserts on the model alone that these
inputs exercise every rule (forced selections of visited children, pruned visits, a child with N > 1 pruned to 0, a child kept
whole because its gap is not positive, both at an index >= 64 on the wide board, no pruned subtree).

Neutral settings (enabled = 1, eps = 0, forced_k = 0, prune off) are defined with the sampler's mixing OFF, as for every enabled
engine (enabled alone decides, include/cczero.h): they equal a twin engine that never had the call and whose own sampler eps is 0 --
leaf inputs, trees, records, moves and ccz_get_stats, bit for bit --, and on an engine with the default sampler eps the mixed vector
is pi itself.

Every case fails on the parent commit: the library has no ccz_set_root_exploration."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import explore_model as em
from gpu_harness import planes_to_squares

pytestmark = pytest.mark.gpu

B = em.B
HDR, IDS, PI = 96, 112, 368


def _engine(sampler_eps=0.25):
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(B, n_playout=em.N_PLAYOUT, seed=em.SEED, board_id_base=em.BASE, max_plies=2, eps=sampler_eps)
    from golden_cases import STARTS, start_position
    boards, lines, _ = em.inputs()
    sq = np.stack([start_position() if ln is not None else b.squares() for b, ln in zip(boards, lines)]).astype(np.uint8)
    status = e.set_positions(sq, np.ones(B, np.uint8), moves=[ln or [] for ln in lines])
    assert (status == 0).all(), status
    assert np.array_equal(e.root_positions(), np.stack([b.squares() for b in boards]))
    assert np.array_equal(sq[em.WIDE], STARTS["widest"])
    return e


def _search(e, fused, n_steps, digest=None):
    """``n_steps`` lockstep simulations with the hash evaluator on the engine's own leaf inputs."""
    dev = e.device
    e.select_leaves()
    for i in range(n_steps):
        planes = e.leaf_input.float().cpu().numpy()
        if digest is not None:
            digest.update(planes.tobytes())
        sq, turn = planes_to_squares(planes)
        PV = [em.evaluate_sq(em.SALTS, b, sq[b], turn[b]) for b in range(B)]
        tp = torch.from_numpy(np.stack([p for p, _ in PV])).to(dev)
        tv = torch.from_numpy(np.array([v for _, v in PV], np.float32)).to(dev)
        if fused and i + 1 < n_steps:
            e.step(tp, tv)
        else:
            e.expand_backup(tp, tv)
            if i + 1 < n_steps:
                e.select_leaves()


def _drive(e, fused, targets=None, moves=2):
    """Two moves with tree reuse through one launch form, then the adjudication at the ply cap and the harvest."""
    _, _, sims = em.inputs()
    e.set_budgets(np.asarray(sims, np.int32), None if targets is None else np.asarray(targets, np.uint8))
    out = {"moves": [], "digest": hashlib.sha256()}
    for _ in range(moves):
        _search(e, fused, max(sims), out["digest"])
        rc = e.root_children()
        noise, nk = e.root_noise()
        gamma, mixed, u = e.move_distribution()
        played = e.finish_move().cpu().numpy().copy()
        out["moves"].append({"roots": rc, "noise": noise, "noise_k": nk, "gamma": gamma, "mixed": mixed, "played": played})
    out["xstats"] = e.exploration_stats()
    out["stats"] = e.stats()
    e.set_root_exploration(None)
    _search(e, False, 1)                       # every live root has children: the next finish_move adjudicates at the ply cap
    assert (e.finish_move().cpu().numpy() == -1).all() and e.game_status()["over"].all()
    out["records"] = torch.cat(list(e.harvest_record_chunks())).cpu().numpy()
    e.check_healthy()
    assert e.stats()["pruned_subtrees"] == 0
    out["digest"] = out["digest"].hexdigest()
    return out


def _records_by_board(rec):
    by, i = {}, 0
    while i < len(rec):
        t, T = rec[i, HDR:HDR + 4].view(np.uint16)
        assert t == 0
        b = int(rec[i, HDR + 8:HDR + 12].view(np.uint32)[0]) - em.BASE
        by[b] = rec[i:i + T]
        i += int(T)
    return by


def _check_model(run, model, boards=range(B), exact_stats=True):
    recs = _records_by_board(run["records"])
    for mv, (got, want) in enumerate(zip(run["moves"], model["moves"])):
        rc = got["roots"]
        for b in boards:
            if not want["live"][b]:
                continue
            acts, visits, q, prior = want["roots"][b]
            k = len(acts)
            assert rc["k"][b] == k, (mv, b)
            assert np.array_equal(rc["acts"][b][:k], acts.astype(np.uint16)), (mv, b)
            assert np.array_equal(rc["visits"][b][:k], visits), (mv, b, rc["visits"][b][:k], visits)
            assert np.array_equal(rc["q"][b][:k].view(np.uint32), q.view(np.uint32)), (mv, b)
            assert np.array_equal(rc["prior"][b][:k].view(np.uint32), prior.view(np.uint32)), (mv, b)   # raw priors, also in a kept subtree
            assert rc["root_visits"][b] == int(visits.sum()) + 1
            row = want["noise"][b]                          # the table as the score used it, bit for bit; fresh for every move
            assert got["noise_k"][b] == len(row), (mv, b)
            assert np.array_equal(got["noise"][b][:len(row)].view(np.uint32), row.view(np.uint32)), (mv, b)
            assert not got["noise"][b][len(row):].any()
            f = want["finish"][b]
            assert got["played"][b] == f["move"], (mv, b, got["played"][b], f["move"])
            r = recs[b][mv]
            assert r[HDR + 6] == k and (r[HDR + 7] & 1) == (0 if model["targets"][b] else 1)
            assert np.array_equal(r[IDS:IDS + 2 * k].view(np.uint16), acts.astype(np.uint16)), (mv, b)
            assert r[PI:PI + 4 * k].tobytes() == f["pi"].tobytes(), (mv, b)          # the recorded pi: of the pruned counts
            assert not r[PI + 4 * k:].any()
            if f["explored"]:                               # no Dirichlet mixing on an explored move; the draws are still reported
                assert np.array_equal(got["mixed"][b][:k], f["pi64"]), (mv, b)
                assert np.array_equal(got["gamma"][b][:k], em.det_gammas(em.SEED, em.BASE + b, 1, mv, k, em.FULL["alpha"])[0]), (mv, b)
    if exact_stats:
        assert run["xstats"] == model["stats"], (run["xstats"], model["stats"])


@functools.lru_cache(maxsize=None)
def _model(eps, forced_k, prune, targets=None, enabled=True):
    m = dict(em.run_case(eps, forced_k, prune, targets=targets, enabled=enabled))
    m["targets"] = [1] * B if targets is None else list(targets)
    assert m["pruned_subtrees"] == 0
    return m


def _explored_run(fused, eps, forced_k, prune, targets=None):
    e = _engine()
    e.set_root_exploration(eps, alpha=None, forced_k=forced_k, prune_targets=prune)
    return _drive(e, fused, targets)


@pytest.mark.parametrize("fused", [False, True], ids=["select_expand", "step"])
def test_full_path_equals_the_model(fused):
    run = _explored_run(fused, 0.25, 2.0, True)
    model = _model(0.25, 2.0, True)
    _check_model(run, model)
    assert model["stats"]["forced_selections"] > 0 and model["stats"]["visits_pruned"] > 0 and model["stats"]["explored_moves"] >= 2 * B - 1
    assert run["stats"]["sims"] == sum(em.inputs()[2][b] for mv in model["moves"] for b in range(B) if mv["live"][b])


# Without noise the hash evaluator's priors are about 1 / 2086 each, and a visited child is forced only while N < sqrt(forced_k P S):
# with S <= 159 that needs forced_k P S > 1, i.e. forced_k > 13. The cases without noise use FORCED_ALONE = 200 (a bound of 2 to 4
# visits late in the search); tests/test_cpu_explore_model.py's full case shows KataGo's 2 firing under the noise.
FORCED_ALONE = 200.0


@pytest.mark.parametrize("eps,forced_k,prune", [(0.25, 0.0, False), (0.0, FORCED_ALONE, False), (0.0, 0.0, True), (0.0, FORCED_ALONE, True)],
                         ids=["noise_only", "forced_only", "pruning_only", "forced_and_pruning"])
def test_each_part_alone(eps, forced_k, prune):
    run = _explored_run(True, eps, forced_k, prune)
    model = _model(eps, forced_k, prune)
    _check_model(run, model)
    s = model["stats"]
    assert (s["forced_selections"] > 0) == (forced_k > 0)
    assert (s["visits_pruned"] > 0) == (prune and forced_k > 0)      # without forced playouts nf = 0: pruning takes nothing back


def test_neutral_settings_equal_an_engine_without_the_call():
    a, b = _engine(sampler_eps=0.0), _engine(sampler_eps=0.0)
    a.set_root_exploration(0.0, alpha=None, forced_k=0.0, prune_targets=False)
    ra, rb = _drive(a, True), _drive(b, True)
    assert ra["digest"] == rb["digest"]                               # every leaf input of every step
    for ma, mb in zip(ra["moves"], rb["moves"]):
        for key in ("k", "acts", "visits", "root_visits"):
            assert np.array_equal(ma["roots"][key], mb["roots"][key]), key
        for key in ("q", "prior"):
            assert np.array_equal(ma["roots"][key].view(np.uint32), mb["roots"][key].view(np.uint32)), key
        assert np.array_equal(ma["played"], mb["played"])
    assert ra["records"].tobytes() == rb["records"].tobytes()
    assert ra["stats"] == rb["stats"]
    assert ra["xstats"] == {"explored_moves": sum(int(m["played"][i] >= 0) for m in ra["moves"] for i in range(B)),
                            "forced_selections": 0, "visits_pruned": 0, "children_pruned": 0}
    assert rb["xstats"] == {"explored_moves": 0, "forced_selections": 0, "visits_pruned": 0, "children_pruned": 0}
    # ... and the model agrees that neutral settings are the reference's search
    _check_model(ra, _model(0.0, 0.0, False), exact_stats=False)
    # the sampler's mixing is off on every enabled engine, whatever its own eps
    c = _engine(sampler_eps=0.25)
    c.set_root_exploration(0.0, alpha=None, forced_k=0.0, prune_targets=False)
    _search(c, True, 8)
    gamma, mixed, _ = c.move_distribution()
    assert np.array_equal(mixed, c.root_pi()) and gamma.any()
    c.set_root_exploration(None)
    assert not np.array_equal(c.move_distribution()[1], c.root_pi())


def test_fast_moves_of_playout_cap_randomisation_are_left_alone():
    targets = tuple(int(b % 2) for b in range(B))
    run = _explored_run(True, 0.25, 2.0, True, targets)
    _check_model(run, _model(0.25, 2.0, True, targets))
    plain = _engine()
    rp = _drive(plain, True, targets)
    recs, recp = _records_by_board(run["records"]), _records_by_board(rp["records"])
    for b in range(B):
        if targets[b]:
            continue
        for ma, mb in zip(run["moves"], rp["moves"]):
            for key in ("k", "acts", "visits", "q", "prior", "root_visits"):
                assert ma["roots"][key][b].tobytes() == mb["roots"][key][b].tobytes(), (b, key)
            assert ma["played"][b] == mb["played"][b]
            assert np.array_equal(ma["mixed"][b], mb["mixed"][b]) and not ma["noise_k"][b]      # sampler mixing included
        assert recs[b].tobytes() == recp[b].tobytes()


def test_refusals():
    from chinesechesszero_amd._lib import CczError
    from chinesechesszero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(4, n_playout=8, eval_cache_log2=10)
    for bad in (dict(eps=-0.01), dict(eps=1.01), dict(eps=float("nan")), dict(eps=0.25, alpha=0.0), dict(eps=0.25, alpha=-1.0),
                dict(eps=0.25, forced_k=-1.0)):
        with pytest.raises(CczError, match="ccz_set_root_exploration"):
            e.set_root_exploration(**bad)
    e.set_root_exploration(0.25)
    with pytest.raises(CczError, match="root exploration"):
        e.set_scouts(2)
    e.set_root_exploration(None)
    e.set_scouts(2)
    with pytest.raises(CczError, match="scout"):
        e.set_root_exploration(0.25)
    e.set_root_exploration(None)                                   # turning it off is always allowed
    e.set_scouts(0)
    e.set_root_exploration(1.0, alpha=0.03, forced_k=0.0, prune_targets=False)
    from chinesechesszero_amd.net import uniform_evaluator
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    with pytest.raises(ValueError, match="root_exploration"):
        BatchedSelfPlay(uniform_evaluator, 4, n_playout=8, sampling="numpy", root_exploration=dict(eps=0.25))
