"""No GPU: the model of the early stop per board (tests/early_stop_model.py; ccz_set_early_stop) on its own -- the rules by hand,
every mis-stated rule told apart on the GPU test's inputs, S5's consequence, the facts that keep tests/test_gpu_early_stop.py from
passing vacuously -- and the host side: command-line flags, ``make_early_stop``, the declared / bound / exported entry points."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import early_stop_model as esm
import search_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- 1. by hand
def test_the_visit_gap_by_hand():
    assert esm.visit_gap([3, 9, 9, 1]) == (9, 9)                 # the first maximum leads; the second 9 is the runner-up
    assert esm.visit_gap([5]) == (5, 0)
    N = [1] * 64 + [7] + [6] + [0] * 10                          # leader 64, runner-up 65: both in the second 64-lane pass
    assert esm.visit_gap(N) == (7, 6) and esm.visit_gap(N, "runner_up_low_half") == (7, 1)


def test_the_kld_gain_by_hand():
    p, N = [2, 2], [4, 4]
    assert esm.kld_gain(p, N) == 0.0                              # the same distribution
    assert esm.kld_gain(p, p) is None                             # no new visit: not computed
    p, N = [1, 3, 0], [2, 5, 1]
    want = (0.25 * math.log(0.25 / 0.25) + 0.75 * math.log(0.75 / 0.625)) / 4.0
    assert abs(esm.kld_gain(p, N) - want) < 1e-15
    rev = (0.25 * math.log(0.25 / 0.25) + 0.625 * math.log(0.625 / 0.75)) / 4.0
    assert abs(esm.kld_gain(p, N, "kld_reversed") - rev) < 1e-15
    assert abs(esm.kld_gain(p, N, "kld_not_per_node") - want * 4.0) < 1e-15
    t = [float(i) * 1e-3 for i in range(108)]
    m = [t[l] + (t[l + 64] if l + 64 < 108 else 0.0) for l in range(64)]
    for s in (32, 16, 8, 4, 2, 1):
        m = [m[l] + m[l ^ s] for l in range(64)]
    assert esm.butterfly(t) == m[0] and abs(m[0] - sum(t)) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- 2. the runs
@functools.lru_cache(maxsize=None)
def _run(setting, evaluator="peaked", wrong=None, wide=False):
    """(model, moves, signature) of one run on the GPU test's inputs; ``wide``: the 108-move board alone at 128 simulations."""
    try:
        if wide:
            m, _ = esm.case(setting, evaluator, wrong, which=[sm.WIDE], n_sims=128)
            moves = esm.run(m, sims=128, moves=1)
        else:
            m, _ = esm.case(setting, evaluator, wrong)
            moves = esm.run(m)
    except AssertionError as ex:                                  # (a board that never searches a move has nothing to record)
        return None, None, ("raised", str(ex))
    return m, moves, esm.signature(m, moves)


@pytest.mark.parametrize("wrong,setting,wide", [("gap_not_strict", "gap", False), ("s_without_patch", "gap", False),
                                                ("runner_up_low_half", "gap", True), ("kld_reversed", "kld", False),
                                                ("kld_not_per_node", "kld", False), ("snapshot_same_s", "kld", False),
                                                ("stale_after_move", "gap", False), ("stale_after_move", "kld", False)])
def test_each_wrong_model_is_told_apart(wrong, setting, wide):
    assert wrong in esm.WRONG
    right = _run(setting, "peaked", None, wide)[2]
    assert right[0] != "raised"
    assert _run(setting, "peaked", wrong, wide)[2] != right


def test_every_wrong_variant_has_a_case():
    marks = test_each_wrong_model_is_told_apart.pytestmark[0].args[1]
    assert {w for w, _, _ in marks} == set(esm.WRONG)


def test_off_is_the_search_model():
    m, _ = esm.case(None, "peaked")
    a = esm.run(m, reselect=())
    p, _ = sm.case(None, "peaked")
    b = sm.run(p)
    assert sm.signature(a) == sm.signature(b) and not m.stop_log and m.estats["evaluations"] == 0


def test_the_inputs_exercise_the_rules():
    """What the issue's CPU run saw, asserted so that the GPU comparison is not vacuous: each reason fires, a board stops with at
    least a quarter of its budget left, a board never stops; the KLD rule stops at 32 and 48; the 108-move board stops at 121 of
    128 with the leader 104 and the runner-up 105 (both past lane 63)."""
    m, moves, _ = _run("all")
    assert m.estats["single_reply"] > 0 and m.estats["visit_gap"] > 0 and m.estats["kld_gain"] > 0
    assert any(n_b - s >= n_b // 4 for _, _, _, s, n_b in m.stop_log)
    stopped = {(b, mv) for b, mv, *_ in m.stop_log}
    assert all((sm.WIDE, mv) not in stopped for mv in range(esm.MOVES))
    assert all(s >= 24 for _, _, _, s, _ in m.stop_log)                          # min_sims
    assert m.estats["sims_saved"] == sum(n_b - s for _, _, _, s, n_b in m.stop_log)
    k, _, _ = _run("kld")
    assert {s for _, _, r, s, _ in k.stop_log} == {32, 48} and all(r == esm.KLD_GAIN for _, _, r, _, _ in k.stop_log)
    assert k.efacts["reselect_at_interval"] > 0 and len({b for b, *_ in k.stop_log}) < esm.B
    g, _, _ = _run("gap")
    assert (sm.ONE, 0, esm.SINGLE_REPLY, 1, 64) in g.stop_log                    # the root is expanded by simulation 1
    w, wm, _ = _run("gap", wide=True)
    assert w.stop_log == [(0, 0, esm.VISIT_GAP, 121, 128)] and w.efacts["gap_leader_hi"] == 1 and w.efacts["gap_runner_up_hi"] == 1
    N = wm[0]["roots"][0][1]
    order = np.argsort(-N, kind="stable")
    assert (int(order[0]), int(order[1])) == (104, 105)
    # a stopped board shows LEAF_SKIP for the rest of its move and counts nothing
    b, mv, _, s, _ = g.stop_log[1]
    _, gm_, _ = _run("gap")
    assert all(gm_[mv]["steps"][i][b][0] == esm.LEAF_SKIP for i in range(s, esm.SIMS))
    assert gm_[mv]["status"][-1][1][b] == s


@pytest.mark.parametrize("evaluator", ["peaked", "hash"])
def test_a_stopped_board_is_the_board_of_budget_s_and_plays_the_full_runs_first_maximum(evaluator):
    """S5's consequence with f = 1, the solver and root exploration off: the run with the feature equals, leaf for leaf and bit for
    bit, the run without it whose budgets are the simulations each board stopped at; and at every move the first maximum of the
    stopped root is the first maximum of the same search run to n_b."""
    m, moves, _ = _run("gap", evaluator)
    budgets = esm.stop_sims(m, len(moves))
    assert all(s >= 1 for _, _, _, s, _ in m.stop_log)
    played = [[None if f is None else f["move"] for f in mv["finish"]] for mv in moves]
    for j in range(len(moves) + 1):
        rows = [list(r) for r in budgets[:j]] + ([[esm.SIMS] * esm.B] if j < len(moves) else [])
        t, _ = esm.case(None, evaluator)
        tw = esm.run(t, moves=len(rows), budgets=rows, reselect=())
        assert [[None if f is None else f["move"] for f in mv["finish"]] for mv in tw[:j]] == played[:j]   # the same games up to move j
        if j == len(moves):                                      # the twin of the whole run
            for a, b in zip(moves, tw):
                assert [(r[1].tobytes(), r[2].tobytes()) for r in a["roots"]] == [(r[1].tobytes(), r[2].tobytes()) for r in b["roots"]]
                assert [None if f is None else f["pi"].tobytes() for f in a["finish"]] == [None if f is None else f["pi"].tobytes() for f in b["finish"]]
            continue
        for b in range(esm.B):                                   # move j searched to n_b from the same tree
            if moves[j]["finish"][b] is None:
                continue
            full, cut = tw[j]["roots"][b][1], moves[j]["roots"][b][1]
            assert int(np.argmax(full)) == int(np.argmax(cut)), (j, b)


# ---------------------------------------------------------------------------------------------------------------- 3. the host side
def test_make_early_stop_and_the_flags():
    import argparse
    from chinesechesszero_amd.stopcfg import KLD_INTERVAL, add_early_stop_args, early_stop_from_args, make_early_stop
    assert make_early_stop() is None
    assert make_early_stop(single_reply=True) == {"single_reply": True, "gap_factor": 0.0, "kld_interval": 0, "min_gain": 0.0, "min_sims": 0}
    assert make_early_stop(gap=1.5, kld_gain=0.002, min_sims=24) == {"single_reply": False, "gap_factor": 1.5, "kld_interval": KLD_INTERVAL,
                                                                     "min_gain": 0.002, "min_sims": 24}
    assert KLD_INTERVAL == 16
    for kw in (dict(gap=0.5), dict(gap=float("inf")), dict(gap=float("nan")), dict(kld_gain=-1.0), dict(kld_gain=float("nan")),
               dict(kld_gain=0.1, kld_interval=0), dict(kld_interval=8), dict(min_sims=4), dict(gap=1.0, min_sims=-1)):
        with pytest.raises(ValueError):
            make_early_stop(**kw)
    ap = argparse.ArgumentParser()
    add_early_stop_args(ap)
    a = ap.parse_args([])
    assert early_stop_from_args(ap, a) is None
    a = ap.parse_args(["--stop-gap", "--stop-single-reply"])
    assert early_stop_from_args(ap, a) == esm.SETTINGS["gap"]
    a = ap.parse_args(["--stop-gap", "1.5"])
    assert early_stop_from_args(ap, a) == esm.SETTINGS["gap_1p5"]
    a = ap.parse_args(["--stop-kld-gain", "0.002"])
    assert early_stop_from_args(ap, a) == esm.SETTINGS["kld"]
    a = ap.parse_args(["--stop-single-reply", "--stop-gap", "1", "--stop-kld-gain", "0.002", "--stop-kld-interval", "16", "--stop-min-sims", "24"])
    assert early_stop_from_args(ap, a) == esm.SETTINGS["all"]
    with pytest.raises(SystemExit):
        early_stop_from_args(ap, ap.parse_args(["--stop-gap", "0.5"]))


def test_the_front_ends_take_the_flags():
    from chinesechesszero_amd import collect
    a = collect.parse_args(["--stop-gap", "--stop-single-reply"])
    assert a.early_stop == esm.SETTINGS["gap"]
    assert collect.parse_args([]).early_stop is None
    for mod in ("arena", "analyse"):
        src = open(os.path.join(ROOT, "chinesechesszero_amd", mod + ".py"), encoding="utf-8").read()
        assert "add_early_stop_args(ap)" in src and "early_stop_from_args(ap" in src and "early_stop=early_stop" in src, mod
    for mod in ("match", "selfplay"):
        src = open(os.path.join(ROOT, "chinesechesszero_amd", mod + ".py"), encoding="utf-8").read()
        assert "early_stop" in src and "set_early_stop" in src, mod


def test_entry_points_are_declared_bound_and_exported():
    from chinesechesszero_amd import _lib
    header = open(os.path.join(ROOT, "include", "cczero.h"), encoding="utf-8").read()
    names = ("ccz_set_early_stop", "ccz_get_early_stop", "ccz_get_early_stop_stats", "ccz_early_stop_status", "ccz_searching")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
    assert "#define CCZ_ABI_VERSION 9 " in header
    assert [f for f, _ in _lib.EarlyStopCfg._fields_] == ["enabled", "single_reply", "kld_interval", "min_sims", "n_sims", "reserved",
                                                          "gap_factor", "min_gain"]
    assert C.sizeof(_lib.EarlyStopCfg) == 40 and C.sizeof(_lib.EarlyStopStats) == 48
    L = _lib.lib()
    assert L.ccz_abi_version() == 9 == _lib.ABI_VERSION
    for name in names:
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
        assert getattr(L, name)(*([None] * len(_lib.PROTOTYPES[name][1]))) != 0 and name.encode() in L.ccz_last_error()
    from chinesechesszero_amd.engine import SelfPlayEngine
    for meth in ("set_early_stop", "early_stop_settings", "early_stop_stats", "early_stop_status", "searching"):
        assert callable(getattr(SelfPlayEngine, meth)), meth
