"""Host restatement of self-play resignation (include/cczero.h, ccz_set_resign): the root value, the per-board state machine of
k_finish_move's resignation block, the calibration counters and the record flags -- and the comparison helpers the GPU tests
(test_gpu_resign.py) check the engine with. tests/test_cpu_resign_model.py runs it on hand-written sequences and shows that the
helpers reject three plausible wrong models.

Nothing here imports the package: the model is written from the interface's text, not from the kernel."""
import math

import numpy as np

RESIGNED, PLAYON = 2, 4                      # state: | side (1 RED, 0 BLACK) in bit 0
REC_FAST, REC_RESIGNED, REC_PLAYON, REC_VALUE = 1, 2, 4, 8
STAT_KEYS = ("resigned_games", "resigned_by_red", "resigned_plies", "playon_games", "playon_won", "playon_drawn", "playon_plies_after")


def root_value64(visits, q) -> float:
    """sum_i N_i * (double)Q_i / sum_i N_i over the root's children in child order, one float64 accumulator; no visit: 0.0."""
    acc, n = np.float64(0.0), 0
    for ni, qi in zip(np.asarray(visits).tolist(), np.asarray(q, np.float32)):
        acc = acc + np.float64(ni) * np.float64(qi)
        n += int(ni)
    return float(acc / np.float64(n)) if n else 0.0


def root_value(visits, q) -> np.float32:
    """What the engine stores with the ply (and ccz_resign_status returns as last_value): the float64 mean rounded to float32."""
    return np.float32(root_value64(visits, q))


class Rule:
    def __init__(self, threshold, consecutive=2, min_ply=30, p_playon=0.1):
        self.threshold = float(np.float32(threshold))     # the ABI takes a float; the comparison widens it to double
        self.consecutive, self.min_ply, self.p_playon = int(consecutive), int(min_ply), float(p_playon)


class Game:
    """One board's current game. ``record`` is called for every ply the engine records, in order; ``end`` when the game ends
    by any other path (the rules, the ply cap). The keyword switches build the WRONG models of the CPU test."""

    def __init__(self, rule: Rule, fast_resets=False, le=False, redraw=False):
        self.rule = rule
        self.fast_resets, self.le, self.redraw = fast_resets, le, redraw
        self.state, self.run, self.fire_ply, self.last_value = 0, [0, 0], -1, math.nan
        self.over, self.winner, self.plies = False, None, 0
        self.values, self.targets = [], []                # per recorded ply: float32 value (None: none), target byte

    def record(self, turn, v64, target=1, forced=False, u=1.0, enabled=True):
        """One recorded ply: side to move ``turn``, root value ``v64`` (float64), the ply's target byte, whether the host forced
        the move, the lot ``u`` (consulted only if the rule fires). Returns "resign", "playon" or None (the game goes on)."""
        assert not self.over
        ply = self.plies
        self.plies += 1
        self.targets.append(1 if target else 0)
        if not enabled:
            self.values.append(None)
            return None
        self.values.append(np.float32(v64))
        self.last_value = np.float32(v64)
        r = self.rule
        s = int(turn)
        below = (v64 <= r.threshold) if self.le else (v64 < r.threshold)
        if target:
            self.run[s] = min(self.run[s] + 1, 255) if below else 0
        elif self.fast_resets:
            self.run[s] = 0
        fire = bool(target) and r.consecutive > 0 and self.run[s] >= r.consecutive and ply >= r.min_ply and not forced \
            and (self.redraw or not (self.state & PLAYON))
        if not fire:
            return None
        if u < r.p_playon:
            if not (self.state & PLAYON):
                self.state, self.fire_ply = PLAYON | s, ply
            return "playon"
        self.state, self.fire_ply = RESIGNED | s, ply
        self.over, self.winner = True, s ^ 1
        return "resign"

    def end(self, winner):
        """The game ended by the rules (winner 1 / 0 / -1) or at the ply cap (-1) after ``self.plies`` recorded plies."""
        assert not self.over
        self.over, self.winner = True, int(winner)

    def flags(self):
        """The record header's flags byte of every ply of the finished game."""
        return [(0 if t else REC_FAST) | (self.state & (RESIGNED | PLAYON)) | (REC_VALUE if v is not None else 0)
                for t, v in zip(self.targets, self.values)]

    def status(self):
        return {"state": self.state, "run": tuple(self.run), "fire_ply": self.fire_ply, "last_value": self.last_value}


def stats_of(games) -> dict:
    """ccz_resign_stats over finished games."""
    out = dict.fromkeys(STAT_KEYS, 0)
    for g in games:
        assert g.over
        if g.state & RESIGNED:
            out["resigned_games"] += 1
            out["resigned_by_red"] += g.state & 1
            out["resigned_plies"] += g.plies
        elif g.state & PLAYON:
            out["playon_games"] += 1
            out["playon_won"] += int(g.winner == (g.state & 1))
            out["playon_drawn"] += int(g.winner == -1)
            out["playon_plies_after"] += g.plies - g.fire_ply
    return out


# ---------------------------------------------------------------------- comparison helpers (exact: no tolerance anywhere)
def same_f32(a, b) -> bool:
    """Bit equality of float32 arrays; a NaN equals a NaN whatever its payload."""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32)))


def check_status(got: dict, games, where=""):
    """``got``: the arrays of ccz_resign_status; ``games``: the boards' models."""
    for b, g in enumerate(games):
        w = g.status()
        assert int(got["state"][b]) == w["state"], (where, b, "state", int(got["state"][b]), w["state"])
        assert tuple(int(x) for x in got["run"][b]) == w["run"], (where, b, "run", got["run"][b], w["run"])
        assert int(got["fire_ply"][b]) == w["fire_ply"], (where, b, "fire_ply", int(got["fire_ply"][b]), w["fire_ply"])
        gv, wv = np.float32(got["last_value"][b]), np.float32(w["last_value"])
        assert (np.isnan(gv) and np.isnan(wv)) or gv.view(np.uint32) == wv.view(np.uint32), (where, b, "last_value", gv, wv)


def check_events(got, want, where=""):
    """Per board: what the engine did at a move boundary ("resign" / "playon" / None / "cap") against the models' answers."""
    assert list(got) == list(want), (where, [(b, g, w) for b, (g, w) in enumerate(zip(got, want)) if g != w])


def check_stats(got: dict, games, where=""):
    want = stats_of(games)
    assert {k: int(got[k]) for k in STAT_KEYS} == want, (where, got, want)


def check_record_flags(flags, values, game: Game, where=""):
    """``flags`` / ``values``: the flags byte and bytes 92..95 (as float32) of the harvested records of one game, in ply order."""
    assert [int(f) for f in flags] == game.flags(), (where, list(flags), game.flags())
    for t, (v, w) in enumerate(zip(values, game.values)):
        w = np.float32(0.0) if w is None else w
        assert np.float32(v).view(np.uint32) == np.float32(w).view(np.uint32), (where, t, v, w)
