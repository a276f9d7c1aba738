"""No GPU: the model of the search parameters (tests/search_model.py; ccz_set_search) on its own -- hand-computed scores, every
mis-stated rule told apart on the GPU test's inputs, the facts that keep tests/test_gpu_search_params.py from passing vacuously --
and the host side: command-line flags, the UCI options, MCTS's scout rule, the declared / bound / exported entry points."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import search_model as sm
from explore_model import F32, ExploreModel
from search_model import ABSOLUTE, INF, OFF, REDUCTION

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- 1. by hand
def test_scores_of_a_three_child_node_by_hand():
    # node X: N_X = 4, Q_X = -0.5 (its side to move stands at +0.5); children: visited (N 2, Q 0.25, P 0.5), unvisited P 0.25 and P 0.125
    N, Q, P = [2, 0, 0], [F32(0.25), F32(0.0), F32(0.0)], np.array([0.5, 0.25, 0.125], F32)
    c = sm.c_eff(5, None, 4)
    assert c == F32(5.0) and c.dtype == np.float32
    assert sm.visited_mass(N, P) == 0.5
    # mode 1, reduction 0.5: f = 0.5 - 0.5 * sqrt(0.5)
    f1 = sm.urgency(REDUCTION, 0.5, F32(-0.5), 0.5)
    assert f1 == 0.5 - 0.5 * math.sqrt(0.5)
    s = sm.scores(N, Q, P, 4, c, f1)
    assert s == [0.25 + 2.5 * 2.0 / 3.0, f1 + 1.25 * 2.0, f1 + 0.625 * 2.0] and sm.first_max(s) == 1
    # mode 2, absolute -1: the visited child wins
    f2 = sm.urgency(ABSOLUTE, -1.0, F32(-0.5), 0.5)
    s = sm.scores(N, Q, P, 4, c, f2)
    assert f2 == -1.0 and s == [0.25 + 5.0 / 3.0, -1.0 + 2.5, -1.0 + 1.25] and sm.first_max(s) == 0
    # mode 0: +inf, the first unvisited child
    f0 = sm.urgency(OFF, 0.0, F32(-0.5), 0.5)
    s = sm.scores(N, Q, P, 4, c, f0)
    assert f0 == INF and s[1:] == [INF, INF] and sm.first_max(s) == 1
    # the mis-stated sign
    assert sm.urgency(REDUCTION, 0.5, F32(-0.5), 0.5, "parent_sign") == -0.5 - 0.5 * math.sqrt(0.5)


def test_the_exploration_constant():
    off = sm.settings(REDUCTION, 0.3)
    for n in (0, 1, 7, 400, 10 ** 6):
        assert sm.c_eff(5, off, n).tobytes() == F32(5.0).tobytes()              # c_factor = 0: c_puct exactly, whatever N
        assert sm.c_eff(F32(1.25), off, n).tobytes() == F32(1.25).tobytes()
    g = sm.settings(OFF, c_base=8.0, c_factor=2.0)
    want = F32(5.0 + 2.0 * sm.det_log((10.0 + 8.0 + 1.0) / 8.0))
    assert sm.c_eff(5, g, 10).tobytes() == want.tobytes() and abs(float(want) - (5.0 + 2.0 * math.log(19.0 / 8.0))) < 1e-6
    assert float(sm.c_eff(5, g, 0)) > 5.0 and float(sm.c_eff(5, g, 100)) > float(sm.c_eff(5, g, 10))


def test_the_mass_is_the_butterfly_sum():
    rng = np.random.RandomState(5)
    P = rng.dirichlet(np.ones(108)).astype(F32)
    N = (rng.rand(108) < 0.5).astype(int)
    got = sm.visited_mass(N, P)
    assert abs(got - float(P[N > 0].astype(np.float64).sum())) < 1e-12
    m = [(float(P[l]) if N[l] else 0.0) + ((float(P[l + 64]) if N[l + 64] else 0.0) if l + 64 < 108 else 0.0) for l in range(64)]
    for s in (32, 16, 8, 4, 2, 1):
        m = [m[l] + m[l ^ s] for l in range(64)]
    assert len(set(m)) == 1 and got == m[17]                                    # every lane ends with the same bits
    assert sm.visited_mass([0, 0], P[:2]) == 0.0 and sm.visited_mass([], []) == 0.0


def test_settings_default_the_root_to_the_tree():
    s = sm.settings(REDUCTION, 0.4)
    assert (s["fpu_root_mode"], s["fpu_root_value"]) == (REDUCTION, 0.4)
    s = sm.settings(REDUCTION, 0.4, ABSOLUTE, 1.0)
    assert (s["fpu_mode"], s["fpu_value"], s["fpu_root_mode"], s["fpu_root_value"]) == (REDUCTION, 0.4, ABSOLUTE, 1.0)
    assert sm.settings(OFF, 0.7)["fpu_value"] == 0.0                             # a mode that is off has no value


def test_rule_off_is_the_base_models_choice_on_every_node():
    m, _ = sm.case(None, "peaked", which=[sm.START, sm.PAWNS, sm.OPEN_A], explore=sm.EXPLORE)
    seen = {"n": 0}
    plain = ExploreModel._select_child

    def both(self, b, node, depth):
        i = plain(self, b, node, depth)
        seen["n"] += 1
        return i
    # the model with the rule off goes through ExploreModel's selection and nothing else
    ExploreModel._select_child = both
    try:
        sm.run(m, sims=32, moves=2)
    finally:
        ExploreModel._select_child = plain
    assert seen["n"] > 3 * 32 and m.sfacts == {"hi_before_lo": 0, "fresh_root_not_child0": 0, "unvisited_not_first": 0}
    # ... and with mode 0 and c_factor 0 turned ON it makes the same choices (the rule with nothing to say)
    a, _ = sm.case(sm.settings(OFF), "peaked", which=[sm.START, sm.PAWNS, sm.OPEN_A], explore=sm.EXPLORE)
    b, _ = sm.case(None, "peaked", which=[sm.START, sm.PAWNS, sm.OPEN_A], explore=sm.EXPLORE)
    assert sm.signature(sm.run(a, sims=32, moves=2)) == sm.signature(sm.run(b, sims=32, moves=2))


# ---------------------------------------------------------------------------------------------------------------- 2, 3. the GPU test's inputs
def _run(setting, *a, **kw):
    """(model, moves, signature) of the model's run on all eight boards; ``setting``: a name of search_model.SETTINGS, a dict or None."""
    return _run_cached(tuple(sorted(setting.items())) if isinstance(setting, dict) else setting, *a, **kw)


@functools.lru_cache(maxsize=None)
def _run_cached(setting, evaluator="peaked", wrong=None, explore=False, sims=sm.SIMS, moves=2):
    kw = dict(explore=sm.EXPLORE) if explore else {}
    m, _ = sm.case(dict(setting) if isinstance(setting, tuple) else setting, evaluator, wrong=wrong, **kw)
    out = sm.run(m, sims=sims, moves=moves)
    return m, out, sm.signature(out)


@pytest.mark.parametrize("wrong,setting,explore", [
    ("parent_sign", "reduction", False), ("mass_all", "reduction", False), ("mass_noisy", "reduction", True),
    ("root_uses_tree", "mixed", False), ("growth_child_visits", "growth", False), ("first_is_child0", "reduction", False),
    ("prune_plain_cpuct", "growth", True)])
def test_each_wrong_model_is_told_apart(wrong, setting, explore):
    assert _run(setting, "peaked", wrong, explore)[2] != _run(setting, "peaked", None, explore)[2]


def test_fewer_root_children_and_deeper_leaves():
    on, mon, _ = _run("reduction", moves=1)
    off, moff, _ = _run(None, moves=1)
    k = len(mon[0]["roots"][sm.START][0])
    assert k >= 40
    assert moff[0]["visited"][sm.START] == min(k, 63)                            # PUCT: one look at every root move
    assert mon[0]["visited"][sm.START] < k
    assert on.depth_peak > off.depth_peak and on.sum_depth > off.sum_depth


def test_the_inputs_exercise_the_rule():
    m, moves, sig = _run("reduction")
    assert len(moves[0]["roots"][sm.WIDE][0]) >= 98
    assert m.sfacts["hi_before_lo"] > 0             # an unvisited child of index >= 64 chosen while a lower one is still unvisited
    assert m.sfacts["fresh_root_not_child0"] > 0    # a root expanded in a step hands out a child other than child 0
    # R3: the reduction term acts (against reduction 0, the bare parent value), and mode 1 is not mode 2
    assert sig != _run(sm.settings(REDUCTION, 0.0))[2] and sig != _run("absolute")[2]
    # R1 with c_base 8 changes a choice within 64 simulations, with and without an urgency
    assert _run("growth")[2] != sig and _run("growth_only")[2] != _run(None)[2]
    # the mixed pair is neither of its halves
    assert _run("mixed")[2] not in (_run(sm.settings(REDUCTION, 0.5))[2], _run(sm.settings(ABSOLUTE, 0.75))[2])


def test_the_options_meet_on_the_inputs():
    m, moves, _ = _run("growth", "peaked", None, True)
    t = m.totals()
    assert t["explored_moves"] > 0 and t["forced_selections"] > 0 and t["visits_pruned"] > 0
    # the solver on mate_in_two: nodes are proven and descents stop under the rule
    s, _ = sm.case("reduction", "hash", which=[sm.MATE2], solver=True)
    sm.run(s, sims=96, moves=2)
    assert s.nodes_proven > 0 and s.proven_stops > 0
    # the Gumbel root: the tree pair acts from depth 1 (another tree than Gumbel alone grows)
    g = dict(n_sims=32, max_considered=8, c_visit=50.0, c_scale=1.0)
    a, _ = sm.case("reduction", "peaked", gumbel=g)
    b, _ = sm.case(None, "peaked", gumbel=g)
    assert sm.signature(sm.run(a, sims=32, moves=2)) != sm.signature(sm.run(b, sims=32, moves=2))
    assert a.gstats["gumbel_moves"] > 0 and a.sfacts["unvisited_not_first"] > 0


# ---------------------------------------------------------------------------------------------------------------- 4. the host side
def test_command_line_flags():
    from chinesechesszero_amd import collect
    from chinesechesszero_amd.searchcfg import C_BASE, make_search
    a = collect.parse_args(["--fpu-reduction", "0.3"])
    assert a.search == {"fpu_mode": 1, "fpu_value": 0.3, "fpu_root_mode": 1, "fpu_root_value": 0.3, "c_base": C_BASE, "c_factor": 0.0}
    a = collect.parse_args(["--fpu-absolute", "-0.5", "--fpu-root-reduction", "0.1", "--cpuct-base", "8", "--cpuct-factor", "2"])
    assert a.search == {"fpu_mode": 2, "fpu_value": -0.5, "fpu_root_mode": 1, "fpu_root_value": 0.1, "c_base": 8.0, "c_factor": 2.0}
    assert collect.parse_args([]).search is None
    assert collect.parse_args(["--cpuct-factor", "1"]).search["fpu_mode"] == 0
    for bad in (["--fpu-reduction", "0.3", "--fpu-absolute", "0"], ["--fpu-root-reduction", "0.3", "--fpu-root-absolute", "0"],
                ["--fpu-reduction", "-1"], ["--fpu-absolute", "1.5"], ["--cpuct-base", "0"], ["--cpuct-factor", "-1"],
                ["--fpu-reduction", "nan"], ["--fpu-absolute", "nan"], ["--cpuct-factor", "inf"]):
        with pytest.raises(SystemExit):
            collect.parse_args(bad)
    assert make_search() is None
    with pytest.raises(ValueError, match="exclude"):
        make_search(fpu_reduction=0.1, fpu_absolute=0.0)
    text = collect.format_search(dict(sm.DEFAULTS, enabled=True, fpu_mode=1, fpu_value=0.3, fpu_root_mode=2, fpu_root_value=1.0, c_factor=2.0,
                                      c_base=8.0), {"sum_depth": 700, "sims": 200})
    assert "fpu reduction 0.3 (root absolute 1)" in text and "base 8 factor 2" in text and "mean leaf depth 3.50" in text


def test_arena_and_analyse_take_the_flags():
    import argparse
    from chinesechesszero_amd.searchcfg import add_search_args, search_from_args
    for mod in ("arena", "analyse"):
        src = open(os.path.join(ROOT, "chinesechesszero_amd", mod + ".py"), encoding="utf-8").read()
        assert "add_search_args(ap)" in src and "search_from_args(ap" in src and "search=search" in src, mod
    ap = argparse.ArgumentParser()
    add_search_args(ap)
    assert search_from_args(ap, ap.parse_args(["--fpu-root-absolute", "1"])) == {
        "fpu_mode": 0, "fpu_value": 0.0, "fpu_root_mode": 2, "fpu_root_value": 1.0, "c_base": 19652.0, "c_factor": 0.0}


def test_scouts_and_search_exclude_each_other_in_the_one_game_search():
    from chinesechesszero_amd.mcts import MCTS, MCTS_AI
    s = sm.settings(REDUCTION, 0.3)
    with pytest.raises(ValueError, match="scouts"):
        MCTS_AI(lambda board: None, n_playout=8, search=s, scouts=10)
    with pytest.raises(ValueError, match="scouts"):
        MCTS(lambda board: None, n_playout=8, search=s, scouts=1)

    class Batched:
        batched = returns_logits = True

        def __call__(self, leaf):
            raise AssertionError("not evaluated here")
    assert MCTS(Batched(), n_playout=8).scouts > 0                               # scouts=None without search: the default slots
    assert MCTS(Batched(), n_playout=8, search=s).scouts == 0                    # ... with search: none
    assert MCTS(Batched(), n_playout=8, search=s, scouts=0).scouts == 0


def test_uci_options():
    import io
    from chinesechesszero_amd.uci import UciLoop
    out = io.StringIO()
    u = UciLoop(policy_value_fn=lambda b: None, out=out)
    assert u._search() is None
    u.handle("setoption name FpuReduction value 0.3")
    u.handle("setoption name CpuctFactor value 2")
    u.handle("setoption name CpuctBase value 8")
    assert u._search() == {"fpu_mode": 1, "fpu_value": 0.3, "fpu_root_mode": 1, "fpu_root_value": 0.3, "c_base": 8.0, "c_factor": 2.0}
    assert out.getvalue().count("scout slots are off for this session") == 3
    u.handle("setoption name FpuAbsolute value -0.5")                            # the later form stands
    assert (u._search()["fpu_mode"], u._search()["fpu_value"]) == (2, -0.5)
    u.handle("setoption name FpuAbsolute value 7")                               # refused: the old setting stands
    assert "info string error" in out.getvalue() and u._search()["fpu_value"] == -0.5
    u.handle("uci")
    for name in ("FpuReduction", "FpuAbsolute", "CpuctBase", "CpuctFactor"):
        assert f"option name {name} " in out.getvalue()


def test_entry_points_are_declared_bound_and_exported():
    from chinesechesszero_amd import _lib
    header = open(os.path.join(ROOT, "include", "cczero.h"), encoding="utf-8").read()
    for name in ("ccz_set_search", "ccz_get_search"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
    assert "#define CCZ_ABI_VERSION 9 " in header
    assert [f for f, _ in _lib.SearchCfg._fields_] == ["enabled", "fpu_mode", "fpu_root_mode", "reserved", "fpu_value", "fpu_root_value",
                                                       "c_base", "c_factor"]
    assert C.sizeof(_lib.SearchCfg) == 48
    L = _lib.lib()
    assert L.ccz_abi_version() == 9 == _lib.ABI_VERSION
    for name in ("ccz_set_search", "ccz_get_search"):
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    # null engine: refused with the call's name, nothing touched
    assert L.ccz_set_search(None, None, 1, 1, 0.3, 1, 0.3, 19652.0, 0.0) != 0 and b"ccz_set_search" in L.ccz_last_error()
    assert L.ccz_get_search(None, None, None) != 0 and b"ccz_get_search" in L.ccz_last_error()
    from chinesechesszero_amd.engine import SelfPlayEngine
    assert callable(SelfPlayEngine.set_search) and callable(SelfPlayEngine.search_settings)
