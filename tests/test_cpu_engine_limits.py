"""CPU: the limit-aware host twins (oracle/ccz_ref.c) on the fixtures of tests/engine_limit_cases.py. What a board looks like after
it hits a bounded resource is derived here BY HAND from the rules the twins restate -- which leaf no longer expands, which descent
is dropped, which ply ends the game, which forced move is refused -- and never read off the twin. The same file asserts what the GPU
cases (tests/test_gpu_engine_limits.py) rely on, so that a fixture cannot drift into testing nothing: every faulty board hits its
limit within the simulations the case runs, no clean board ever does, the record case overflows at the ply it names, and no
re-root prunes."""
import functools
import os
import subprocess

import numpy as np
import pytest

import engine_limit_cases as E
from engine_limit_cases import CASES
from oracle import OracleBoard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def ref(name):
    return E.run_ref(CASES[name])


def events(log, kind):
    return [e for e in log if e[0] == kind]


def limits(engine):
    """(cap, budget of a kept subtree, path capacity, pi arena) by ccz_create's arithmetic (include/cczero.h: ccz_config)."""
    n = engine.get("n_playout", 400)
    cap = max(engine.get("max_nodes", 0) or (n + 64) * 512, 130)
    reserve = min(n * 128, cap // 2)
    if engine.get("reserve_nodes", 0) > 0:
        reserve = min(engine["reserve_nodes"], cap - 129)
    return cap, cap - reserve, engine.get("max_depth", 0) or 512, 80 * (engine.get("max_plies", 0) or 2048)


@pytest.mark.parametrize("name", sorted(CASES))
def test_faulty_boards_hit_the_limit_and_clean_boards_never_do(name):
    case = CASES[name]
    log, usage, end = ref(name)
    flags = end["board_flags"]
    for b in range(case["B"]):
        assert flags[b] == (case["bit"] if b in case["faulty"] else 0), (name, b, flags)
    assert events(log, "status")[-1][1]["error_flags"].tolist() == [case["flags"]]
    assert len(log) == case["moves"] * (case["n"] + 3) + (2 if case.get("finish_first") else 0)
    # no re-root prunes: what a board holds after a move is within the budget of a kept subtree; nothing exceeds the pool
    cap, budget, _, pi_cap = limits(case["engine"])
    for before, after in usage:
        assert (before["n_nodes"] <= cap).all() and (after["n_nodes"] <= budget).all(), (name, before, after, budget)
        assert (after["pi_used"] <= pi_cap).all()
    assert end["nodes_peak"] <= cap


def test_pool_the_fifth_expansion_is_refused_and_every_simulation_still_counts():
    case = CASES["pool"]
    log, usage, end = ref("pool")
    cap = case["engine"]["max_nodes"]
    # board 0, uniform priors on the start position: an unvisited child scores +inf, so simulation 1 expands the root and
    # simulation 1 + i visits child i. The root and the children that still fit hold 1 + 44 + k_1 + k_2 + ... nodes.
    root = OracleBoard()
    ids = root.legal_ids()
    assert len(ids) == 44
    widths = []
    for i in ids[:19]:
        c = root.copy()
        c.push_id(i)
        widths.append(len(c.legal_ids()))
    nodes, expanded = 1 + 44, 0
    for w in widths:                               # in visiting order; a child that does not fit stays a leaf, a later narrower one may fit
        if nodes + w <= cap:
            nodes, expanded = nodes + w, expanded + 1
    assert expanded == 3 and nodes + min(widths) > cap     # three children, then the pool is shut for every other one
    before, after = usage[0]
    assert before["n_nodes"][0] == nodes
    roots = events(log, "roots")[0][1]
    assert roots["k"][0] == 44 and roots["root_visits"][0] == 20
    assert roots["visits"][0, :44].tolist() == [1] * 19 + [0] * 25           # every refused expansion still added its visit
    leaves = events(log, "leaf")[:20]
    assert [int(e[2]["depth"][0]) for e in leaves] == [0] + [1] * 19
    assert all(int(e[2]["status"][0]) == 0 for e in leaves)                  # the refused leaves were EXPAND leaves like the others
    assert before["sims"] == 20 * case["B"]
    # the forced first child was expanded: the kept subtree is that child and its children, and the pool has room again
    assert events(log, "moves")[0][1][0] == ids[0] == 0
    assert after["n_nodes"][0] == 1 + widths[0]
    assert end["sims"] == 2 * 20 * case["B"]
    # the clean boards' whole search fits
    for b in (3, 4, 5):
        assert usage[0][0]["n_nodes"][b] <= cap and usage[1][0]["n_nodes"][b] <= cap


def test_depth_the_descent_that_would_reach_max_depth_is_dropped_and_the_board_freezes():
    case = CASES["depth"]
    log, usage, end = ref("depth")
    n = case["n"]
    leaves = events(log, "leaf")
    roots = events(log, "roots")
    for b, first in E.DEPTH_FIRST_DROP.items():
        assert first <= n - 3                                                  # the case runs a few simulations past the drop
        status = [int(e[2]["status"][b]) for e in leaves[:n]]
        depth = [int(e[2]["depth"][b]) for e in leaves[:n]]
        assert status.index(3) == first - 1 and set(status[first - 1:]) == {3}   # frozen from the first drop on
        assert max(depth) == 63 and depth[first - 2] < 64                    # 64 path entries: the deepest leaf sits 63 moves down
        assert roots[0][1]["root_visits"][b] == first - 1                     # a dropped descent is no visit
    for b in (2, 3):
        assert all(int(e[2]["status"][b]) != 3 for e in leaves) and roots[0][1]["root_visits"][b] == n
    # no simulation is counted for a dropped descent
    assert usage[0][0]["sims"] == sum(f - 1 for f in E.DEPTH_FIRST_DROP.values()) + 2 * n
    # after the move the boards search again (their kept line is one move shorter)
    for b in E.DEPTH_FIRST_DROP:
        assert int(leaves[n][2]["status"][b]) != 3
    assert max(int(e[2]["depth"].max()) for e in leaves) <= 63


def test_nan_the_board_freezes_once_the_root_and_its_children_are_visited():
    log, usage, end = ref("nan")
    leaves, roots = events(log, "leaf"), events(log, "roots")
    status = [int(e[2]["status"][0]) for e in leaves[:50]]
    assert status == [0] * 45 + [3] * 5                                        # root + 44 first visits (+inf each), then no comparable child
    r = roots[0][1]
    assert r["k"][0] == 44 and r["root_visits"][0] == 45 and r["visits"][0, :44].tolist() == [1] * 44
    assert np.isnan(r["prior"][0, :44]).all()
    assert usage[0][0]["sims"] == 45 + 3 * 50
    assert (r["root_visits"][1:] == 50).all()


def test_record_the_arena_overflows_at_ply_one():
    case = CASES["record"]
    log, usage, end = ref("record")
    sq, turn, half = E.WIDE_PAIR
    b0 = OracleBoard.from_array(sq, turn, half)
    ids = b0.legal_ids()
    b1 = b0.copy()
    b1.push_id(E.RECORD_FIRST)
    assert len(ids) == E.RECORD_K0 and ids[0] == E.RECORD_FIRST and len(b1.legal_ids()) == E.RECORD_K1
    assert not b1.is_game_over() and not b1.is_tie()
    # (another first move has few enough replies for both plies to fit: the GPU test's engine that never overflows)
    narrow = []
    for m in ids:
        c = b0.copy()
        c.push_id(m)
        if not c.is_game_over() and not c.is_tie():
            narrow.append(len(c.legal_ids()))
    assert E.RECORD_K0 + min(narrow) <= 160
    _, _, _, pi_cap = limits(case["engine"])
    assert pi_cap == 160 and E.RECORD_K0 <= pi_cap < E.RECORD_K0 + E.RECORD_K1 and E.RECORD_K1 > 64
    moves, status, roots = events(log, "moves"), events(log, "status"), events(log, "roots")
    assert roots[0][1]["k"].tolist() == [100, 100, 44, 44] and roots[1][1]["k"][:2].tolist() == [67, 67]
    assert moves[0][1][:2].tolist() == [81, 81] and (moves[0][1][2:] >= 0).all()
    assert status[0][1]["error_flags"].tolist() == [0] and status[0][1]["over"].tolist() == [0, 0, 0, 0]
    assert moves[1][1][:2].tolist() == [-1, -1] and (moves[1][1][2:] >= 0).all()
    assert status[1][1]["over"].tolist() == [1, 1, 0, 0] and status[1][1]["plies"].tolist() == [1, 1, 2, 2]
    assert status[1][1]["error_flags"].tolist() == [8]
    assert usage[1][1]["pi_used"][:2].tolist() == [100, 100]                   # ply 0 stays recorded
    # the clean boards run on to the ply cap, which is no error outside strict mode
    assert moves[2][1].tolist() == [-1] * 4 and status[2][1]["over"].tolist() == [1] * 4
    assert status[2][1]["winner"].tolist() == [-1] * 4 and status[2][1]["error_flags"].tolist() == [8]
    assert end["truncated_games"] == 4


def test_bad_moves_are_what_their_names_say_and_refused_boards_restart_at_one_node():
    case = CASES["bad_move"]
    log, usage, end = ref("bad_move")
    sq, turn, half = E.PIN
    root = OracleBoard.from_array(sq, turn, half)
    legal = root.legal_ids()
    ids = case["forced"][0]
    assert ids[0] == 2086
    for b, uci in [(1, "b5b6"), (2, "e8e7"), (3, "a0a5"), (4, "e4a4")]:
        assert ids[b] == E.move_id(uci) and 0 <= ids[b] < 2086 and ids[b] not in legal
    S = E.S
    assert sq[S("b5")] == 0                                                    # an empty from-square
    assert sq[S("e8")] == 11 and turn == 1                                     # the opponent's rook
    assert sq[S("a0")] == 3 and sq[S("a3")] == 1 and E.move_id("a0a2") in legal    # the own pawn stands between a0 and a5
    after = root.copy()
    after.push_id(ids[4])
    assert after.b.pos.turn == 0
    from oracle import lib
    import ctypes as C
    assert lib().xq_in_check(C.byref(after.b.pos), 1)                          # e4a4 uncovers the e-file: the red king stands in check
    assert not root.in_check() and ids[5] in legal
    moves, status = events(log, "moves"), events(log, "status")
    assert moves[0][1][:5].tolist() == [-1] * 5 and moves[0][1][5:7].tolist() == ids[5:7] and moves[0][1][7] in legal
    st = status[0][1]
    assert st["plies"].tolist() == [0] * 5 + [1] * 3 and st["turn"][:5].tolist() == [1] * 5 and st["error_flags"].tolist() == [16]
    assert all(np.array_equal(status[0][2][b], sq) for b in range(5))          # the position did not move
    before, after_u = usage[0]
    assert after_u["n_nodes"][:5].tolist() == [1] * 5 and after_u["pi_used"][:5].tolist() == [0] * 5
    # the tight pool: a refused board's first tree and its second one each fit the pool, together they would not
    cap = case["engine"]["max_nodes"]
    n1, n2 = before["n_nodes"], usage[1][0]["n_nodes"]
    for b in (0, 1, 2, 3):
        assert n1[b] <= cap and n2[b] <= cap and n1[b] + n2[b] - 1 > cap, (b, n1, n2)
    assert status[1][1]["error_flags"].tolist() == [16]                        # ... and the second search of 8 simulations fits
    assert (moves[1][1][:5] >= 0).all()                                        # a refused board moves like any other afterwards


def test_nothing_to_move_refuses_every_board_and_the_engine_goes_on():
    log, usage, end = ref("nothing")
    assert log[0][0] == "moves" and log[0][1].tolist() == [-1] * 4
    assert log[1][1]["error_flags"].tolist() == [16] and log[1][1]["plies"].tolist() == [0] * 4
    assert (events(log, "moves")[1][1] >= 0).all() and events(log, "status")[-1][1]["plies"].tolist() == [1] * 4


def test_create_checks_the_path_capacity_like_the_engine():
    from oracle import RefEngine
    for bad in (63, 513):
        with pytest.raises(RuntimeError):
            RefEngine(1, max_depth=bad)
    for ok in (64, 512):
        RefEngine(1, max_depth=ok).close()


def test_the_twins_are_clean_under_asan_and_ubsan():
    """The limit paths of the C twins as a program of its own, built with the oracle sources under ASan/UBSan."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "limits_selftest_asan"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "oracle", "limits_selftest_asan")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "limits_selftest: ok" in out.stdout, out.stderr
