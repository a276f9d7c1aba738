"""CPU: the host restatement of self-play resignation (tests/resign_model.py) on hand-written sequences, and proof that the
comparison helpers the GPU tests use (check_events / check_status / check_stats / check_record_flags) reject three plausible
wrong models: a run counter that a fast ply resets, `<=` in place of `<`, and a play-on lot drawn anew at every firing."""
import math

import numpy as np
import pytest

import resign_model as rm
from resign_model import PLAYON, RESIGNED, Game, Rule

LOW, HIGH = -0.95, 0.95


def _play(game, plies, enabled=True):
    """``plies``: (turn, v, target, forced, u) per ply. Returns (events, status after every ply); stops at a resignation."""
    events, status = [], []
    for turn, v, target, forced, u in plies:
        ev = game.record(turn, v, target, forced, u, enabled=enabled)
        events.append(ev)
        status.append(game.status())
        if ev == "resign":
            break
    return events, status


def _alternating(n, red=LOW, black=HIGH, target=1, forced=False, u=1.0):
    return [(1 - (t & 1), red if t % 2 == 0 else black, target, forced, u) for t in range(n)]


def _arrays(statuses):
    """The shape ccz_resign_status hands the helpers: arrays indexed by board."""
    return {"state": np.array([s["state"] for s in statuses], np.uint8), "run": np.array([s["run"] for s in statuses], np.uint8),
            "fire_ply": np.array([s["fire_ply"] for s in statuses], np.int32),
            "last_value": np.array([s["last_value"] for s in statuses], np.float32)}


def test_root_value_is_the_visit_weighted_mean_in_float64():
    assert rm.root_value([3, 1, 0], [-0.5, 0.25, 0.7]) == np.float32(-0.3125)
    assert rm.root_value([0, 0], [0.3, -0.3]) == np.float32(0.0) and rm.root_value([], []) == np.float32(0.0)
    tenth = np.float32(0.1)
    assert rm.root_value([1, 1, 1], [tenth] * 3).view(np.uint32) == tenth.view(np.uint32)
    # float64 accumulation: the float32 sum of these three would lose the small term
    v = rm.root_value64([1, 1, 1], np.array([1e8, -1e8, 3.0], np.float32))
    assert v == 1.0 and rm.root_value([1, 1, 1], np.array([1e8, -1e8, 3.0], np.float32)) == np.float32(1.0)
    assert rm.root_value([2, 2], [-1.0, 1.0]) == 0.0 and isinstance(rm.root_value([1], [0.5]), np.float32)


@pytest.mark.parametrize("consecutive,min_ply,fire", [(1, 0, 0), (2, 0, 2), (3, 0, 4), (1, 5, 6), (2, 5, 6), (3, 5, 6), (4, 5, 6), (5, 5, 8)])
def test_red_resigns_after_enough_low_plies(consecutive, min_ply, fire):
    g = Game(Rule(-0.9, consecutive, min_ply, 0.0))
    events, status = _play(g, _alternating(12))
    assert events == [None] * fire + ["resign"]
    assert g.over and g.winner == 0 and g.plies == fire + 1 and g.state == RESIGNED | 1 and g.fire_ply == fire
    assert g.flags() == [rm.REC_RESIGNED | rm.REC_VALUE] * (fire + 1)
    assert status[-1]["run"] == (0, fire // 2 + 1) and status[-1]["last_value"] == np.float32(LOW)
    assert rm.stats_of([g]) == dict(zip(rm.STAT_KEYS, (1, 1, fire + 1, 0, 0, 0, 0)))


def test_black_resigns_with_the_signs_flipped_and_nobody_resigns_at_half_a_pawn():
    g = Game(Rule(-0.9, 2, 0, 0.0))
    events, _ = _play(g, _alternating(12, red=HIGH, black=LOW))
    assert events == [None, None, None, "resign"] and g.winner == 1 and g.state == RESIGNED | 0 and g.fire_ply == 3
    assert rm.stats_of([g])["resigned_by_red"] == 0
    calm = Game(Rule(-0.9, 1, 0, 0.0))
    events, status = _play(calm, _alternating(12, red=-0.5, black=0.5))
    assert events == [None] * 12 and status[-1]["run"] == (0, 0) and calm.state == 0 and not calm.over
    # a value above the threshold resets the run
    g = Game(Rule(-0.9, 3, 0, 0.0))
    seq = [(1, LOW), (0, HIGH), (1, LOW), (0, HIGH), (1, -0.2), (0, HIGH), (1, LOW), (0, HIGH), (1, LOW), (0, HIGH), (1, LOW)]
    events, status = _play(g, [(t, v, 1, False, 1.0) for t, v in seq])
    assert [s["run"][1] for s in status] == [1, 1, 2, 2, 0, 0, 1, 1, 2, 2, 3] and events[-1] == "resign" and events[:-1] == [None] * 10


def test_consecutive_zero_and_off():
    g = Game(Rule(-0.9, 0, 0, 0.0))
    events, status = _play(g, _alternating(8))
    assert events == [None] * 8 and status[-1]["run"] == (0, 4) and g.flags() == [rm.REC_VALUE] * 8
    g.end(-1)
    assert rm.stats_of([g]) == dict.fromkeys(rm.STAT_KEYS, 0)
    off = Game(Rule(-0.9, 1, 0, 0.0))
    events, status = _play(off, _alternating(4), enabled=False)
    assert events == [None] * 4 and off.flags() == [0] * 4 and math.isnan(status[-1]["last_value"]) and status[-1]["run"] == (0, 0)
    sat = Game(Rule(-0.9, 0, 0, 0.0))
    _play(sat, [(1, LOW, 1, False, 1.0)] * 300)
    assert sat.run == [0, 255]


def test_a_forced_move_is_played_and_the_next_unforced_ply_fires():
    g = Game(Rule(-0.9, 2, 0, 0.0))
    plies = _alternating(8)
    plies[2] = (1, LOW, 1, True, 1.0)                     # the run is complete here, but the host has decided
    events, status = _play(g, plies)
    assert events == [None, None, None, None, "resign"] and status[2]["run"] == (0, 2) and g.fire_ply == 4


def _fast_sequence(fast_value):
    plies = _alternating(10)
    plies[2] = (1, fast_value, 0, False, 1.0)             # red's second ply is a fast one
    return plies


@pytest.mark.parametrize("fast_value", [LOW, HIGH])
def test_a_fast_ply_neither_advances_nor_resets_the_run(fast_value):
    g = Game(Rule(-0.9, 2, 0, 0.0))
    events, status = _play(g, _fast_sequence(fast_value))
    assert events == [None] * 4 + ["resign"] and status[2]["run"] == (0, 1) and status[2]["last_value"] == np.float32(fast_value)
    assert g.flags() == [10, 10, 11, 10, 10]


def test_play_on_is_drawn_once_per_game():
    g = Game(Rule(-0.9, 2, 0, 0.5))
    plies = _alternating(8, u=0.9)
    plies[2] = (1, LOW, 1, False, 0.25)                   # the first firing draws 0.25 < 0.5: played on
    events, status = _play(g, plies)                      # ... and the later firings (u = 0.9) are never consulted
    assert events == [None, None, "playon"] + [None] * 5 and g.state == PLAYON | 1 and g.fire_ply == 2 and not g.over
    assert status[-1]["run"] == (0, 4)
    g.end(1)                                              # the side that would have resigned wins: a false positive
    assert rm.stats_of([g]) == dict(zip(rm.STAT_KEYS, (0, 0, 0, 1, 1, 0, 6)))
    assert g.flags() == [rm.REC_PLAYON | rm.REC_VALUE] * 8
    h = Game(Rule(-0.9, 1, 0, 1.0))
    _play(h, _alternating(5, u=0.999))
    h.end(-1)
    k = Game(Rule(-0.9, 1, 0, 0.0))
    _play(k, _alternating(5, u=0.0))                      # p_playon 0: even u = 0 resigns
    assert k.state == RESIGNED | 1
    assert rm.stats_of([g, h, k]) == dict(zip(rm.STAT_KEYS, (1, 1, 1, 2, 1, 1, 6 + 5)))


# ---------------------------------------------------------------------- the helpers reject wrong models
def _rejected(right: Game, wrong: Game, plies):
    """Play the same plies on both; the right model stands in for the device. Returns the helpers that raised."""
    ev_r, st_r = _play(right, plies)
    ev_w, st_w = _play(wrong, plies)
    for g in (right, wrong):
        if not g.over:
            g.end(-1)
    raised = []
    n = min(len(ev_r), len(ev_w))
    for name, fn in (("events", lambda: rm.check_events(ev_r[:n], ev_w[:n])),
                     ("status", lambda: [rm.check_status(_arrays([st_r[i]]), [_Frozen(st_w[i])]) for i in range(n)]),
                     ("stats", lambda: rm.check_stats(rm.stats_of([right]), [wrong])),
                     ("flags", lambda: rm.check_record_flags(right.flags(), [0.0 if v is None else v for v in right.values], wrong))):
        try:
            fn()
        except AssertionError:
            raised.append(name)
    return raised


class _Frozen:
    def __init__(self, status):
        self._s = status

    def status(self):
        return self._s


def test_the_helpers_accept_the_right_model():
    for plies in (_fast_sequence(HIGH), _alternating(10), _alternating(10, red=float(np.float32(-0.9)))):
        assert _rejected(Game(Rule(-0.9, 2, 0, 0.0)), Game(Rule(-0.9, 2, 0, 0.0)), plies) == []


def test_a_counter_that_a_fast_ply_resets_is_rejected():
    got = _rejected(Game(Rule(-0.9, 2, 0, 0.0)), Game(Rule(-0.9, 2, 0, 0.0), fast_resets=True), _fast_sequence(HIGH))
    assert {"events", "status", "stats", "flags"} <= set(got)
    # even where the fast value is low (no event differs yet) the status read after the fast ply gives it away
    assert "status" in _rejected(Game(Rule(-0.9, 3, 0, 0.0)), Game(Rule(-0.9, 3, 0, 0.0), fast_resets=True), _fast_sequence(LOW)[:4])


def test_le_in_place_of_lt_is_rejected():
    at = float(np.float32(-0.9))                          # a root value that EQUALS the threshold is not below it
    right = Game(Rule(-0.9, 2, 0, 0.0))
    got = _rejected(right, Game(Rule(-0.9, 2, 0, 0.0), le=True), _alternating(10, red=at))
    assert {"events", "status", "stats", "flags"} <= set(got) and right.state == 0


def test_a_lot_drawn_at_every_firing_is_rejected():
    plies = _alternating(10, u=0.9)
    plies[2] = (1, LOW, 1, False, 0.25)
    right = Game(Rule(-0.9, 2, 0, 0.5))
    got = _rejected(right, Game(Rule(-0.9, 2, 0, 0.5), redraw=True), plies)
    assert {"events", "stats", "flags"} <= set(got) and right.state == PLAYON | 1 and right.plies == 10
