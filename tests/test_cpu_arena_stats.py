"""CPU: the arena's statistics (score, Elo and its interval from the pair pentanomial), the promotion rule, the pair / colour
layout, the opening generator's argument checks and the CLI's --help (chinesechesszero_amd/arena.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from chinesechesszero_amd import arena


def test_all_draws_is_zero_elo_with_a_zero_width_interval():
    r = arena.pair_stats([1.0] * 8)
    assert r["pentanomial"] == [0, 0, 8, 0, 0]
    assert r["score"] == 0.5 and r["elo"] == 0.0 and r["score_se"] == 0.0
    assert r["score_ci95"] == [0.5, 0.5] and r["elo_ci95"] == [0.0, 0.0]


def test_all_wins_is_clamped_to_half_a_game_from_the_end():
    # 8 pairs = 16 games: the score 1 is clamped to 1 - 0.5 / 16 = 31 / 32 -> 400 log10(31)
    r = arena.pair_stats([2.0] * 8)
    assert r["pentanomial"] == [0, 0, 0, 0, 8] and r["score"] == 1.0
    assert r["elo"] == pytest.approx(400.0 * math.log10(31.0), abs=1e-9)
    assert math.isfinite(r["elo"]) and r["elo_ci95"][1] == r["elo"]
    assert arena.pair_stats([0.0] * 8)["elo"] == pytest.approx(-400.0 * math.log10(31.0), abs=1e-9)


def test_a_mixed_pentanomial_worked_out_by_hand():
    # points per pair 2, 1.5, 1, 1 -> per-pair scores 1, .75, .5, .5: mean 11/16 = 0.6875
    # deviations 5/16, 1/16, -3/16, -3/16 -> population variance (25 + 1 + 9 + 9) / 256 / 4 = 11/256; se = sqrt(11/256 / 4)
    r = arena.pair_stats([2.0, 1.5, 1.0, 1.0])
    assert r["pentanomial"] == [0, 0, 2, 1, 1]
    assert r["score"] == 0.6875
    assert r["score_se"] == pytest.approx(math.sqrt(11.0 / 1024.0), rel=1e-12)
    assert r["elo"] == pytest.approx(-400.0 * math.log10(1.0 / 0.6875 - 1.0), rel=1e-12)
    assert r["elo"] == pytest.approx(136.969, abs=1e-3)
    lo, hi = 0.6875 - 1.96 * math.sqrt(11.0 / 1024.0), 0.6875 + 1.96 * math.sqrt(11.0 / 1024.0)
    assert r["score_ci95"] == pytest.approx([lo, hi], rel=1e-12)
    assert r["elo_ci95"] == pytest.approx([-400.0 * math.log10(1.0 / lo - 1.0), -400.0 * math.log10(1.0 / hi - 1.0)], rel=1e-12)
    assert r["elo_ci95"][0] < r["elo"] < r["elo_ci95"][1]


def test_pair_stats_refuses_what_is_not_a_pair_score():
    with pytest.raises(ValueError):
        arena.pair_stats([])
    with pytest.raises(ValueError):
        arena.pair_stats([0.25])
    with pytest.raises(ValueError):
        arena.pair_stats([2.5])


def test_promote_rule():
    assert arena.PROMOTE_THRESHOLD == 0.55
    assert arena.promote(0.56) and not arena.promote(0.55) and not arena.promote(0.3)
    assert arena.promote({"score": 0.6}) and not arena.promote({"score": 0.6}, threshold=0.6)
    assert arena.promote(0.51, threshold=0.5)
    with pytest.raises(ValueError):
        arena.promote(0.6, threshold=1.5)


def test_pair_and_colour_layout():
    opening, a_colour, red_net = arena.pair_layout(3)
    assert opening.tolist() == [0, 0, 1, 1, 2, 2]
    assert a_colour.tolist() == [1, 0, 1, 0, 1, 0]       # A plays red on even boards, black on odd ones
    assert red_net.tolist() == [0, 1, 0, 1, 0, 1]        # the evaluator that plays red: A (0) on even boards, B (1) on odd ones
    # the same opening, opposite owners of each colour within a pair
    for i in range(3):
        assert opening[2 * i] == opening[2 * i + 1] and red_net[2 * i] != red_net[2 * i + 1]


def test_cache_salts_differ_and_follow_the_weights_version():
    s = arena.cache_salts(0, 0)
    assert s[0] != s[1] and all(0 < x < 2**64 for x in s)
    assert arena.cache_salts(0, 0) == s
    t = arena.cache_salts(1, 0)
    assert t[0] != s[0] and t[1] == s[1]


@pytest.mark.parametrize("args,exc", [((0, 4), ValueError), ((-3, 4), ValueError), ((4, -1), ValueError), ((2, 0), ValueError),
                                      ((1.5, 4), TypeError), ((4, 2.0), TypeError), ((True, 4), TypeError)])
def test_opening_generator_argument_checks(args, exc):
    with pytest.raises(exc):
        arena.make_openings(*args, seed=0)
    with pytest.raises(TypeError):
        arena.make_openings(4, 4, seed=0.5)


def test_cli_help():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "chinesechesszero_amd.arena", "--help"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for flag in ("--a", "--b", "--pairs", "--playout", "--opening-plies", "--seed"):
        assert flag in r.stdout
