"""CPU: the fixture of reference-produced per-ply histories (tests/golden/reference_rows.*) and the comparison every row-forming path
is held to (tests/reference_rows.py), checked against themselves -- no GPU.

(1) The fixture holds what the issue asks of it: the 72-ply game of reference_game.npz, a red win, two black wins, a draw by the
    rules with all z == 0, a game longer than 256 plies, a game that ends by fourfold repetition.
(2) A table of deliberately wrong rows (mutants): correct rows with exactly one defect each. The comparison helper rejects every one.
    The table also records whether the check this suite had before -- four plies and two of eight history slots of the 72-ply game,
    tests/test_gpu_reference_game.py -- would have accepted the mutant. It is printed (pytest -s shows it; CHANGELOG.md quotes it).

The rows of the mutants come from an index rule over the fixture's positions (slot 0 of every snapshot): ``_rows_by_rule``. The
unmutated rule must itself pass the comparison first -- the expectation does not come from it.

The host mirror (game.Game + mcts.MCTS_AI + CollectPipeline) answers every rule and runs every search on the HIP engine: its
comparison with this fixture needs the GPU and sits in tests/test_gpu_reference_rows.py."""
import numpy as np
import pytest

import reference_rows as R

_, META = R.load()
GAMES = list(range(len(META["games"])))
_cache = {}


# ------------------------------------------------------------------ (1) the fixture
def test_fixture_holds_the_games_the_comparison_needs():
    games = META["games"]
    assert (games[0]["n_playout"], games[0]["seed"], games[0]["salt"], games[0]["plies"], games[0]["winner"]) == (24, 321, 17, 72, False)
    assert sum(g["winner"] is True for g in games) >= 1 and sum(g["winner"] is False for g in games) >= 2
    assert any(g["winner"] is None and g["termination"] == "sixty_moves" for g in games)
    assert any(g["winner"] is None and g["termination"] == "fourfold_repetition" for g in games)
    assert any(g["plies"] > 256 for g in games)
    for g in GAMES:
        a = R.game_arrays(g)
        T = games[g]["plies"]
        assert a["hist"].shape == (T, 16, 7, 10, 9) and a["hist"].dtype == np.int8 and a["turn"].shape == (T,) and a["turn"].dtype == np.uint8
        assert a["pi"].shape == a["pi_mirror"].shape == (T, 2086) and a["pi"].dtype == a["pi_mirror"].dtype == np.float64
        assert a["z"].shape == (T,) and a["z"].dtype == np.float64 and a["moves"].shape == (T,) and a["moves"].dtype == np.int32
        assert a["turn"].tolist() == [1 - t % 2 for t in range(T)]                   # red starts, the sides alternate
        w = games[g]["winner"]
        assert np.array_equal(a["z"], np.zeros(T) if w is None else np.where(a["turn"] == int(w), 1.0, -1.0))
        assert np.allclose(a["pi"].sum(1), 1.0, atol=1e-12) and np.array_equal(np.sort(a["pi"], axis=1), np.sort(a["pi_mirror"], axis=1))
        assert (a["pi"][np.arange(T), a["moves"]] > 0).all()                       # the move played is in the support of its pi
    # the first game IS the game of reference_game.npz: its last snapshot is the history the reference aliases into every tuple
    import os
    old = np.load(os.path.join(R.GOLDEN, "reference_game.npz"))
    a = R.game_arrays(0)
    assert np.array_equal(a["moves"], old["moves"]) and np.array_equal(a["pi"], old["pi"]) and np.array_equal(a["z"], old["z"])
    assert np.array_equal(a["pi_mirror"], old["flipped_pi"])
    assert np.array_equal(a["hist"][-1], np.concatenate((old["final_red_states"], old["final_black_states"])))
    assert np.array_equal(R.expected_rows(0)[0][71][:16], old["processed_state"][:16])


def test_expected_rows_are_assembled_from_the_stored_arrays():
    for g in GAMES:
        a = R.game_arrays(g)
        T = a["hist"].shape[0]
        s, p, z = R.expected_rows(g)
        assert s.shape == (2 * T, 17, 7, 10, 9) and s.dtype == np.float16 and p.dtype == np.float64 and z.dtype == np.float32
        assert np.array_equal(s[:T, :16], a["hist"]) and np.array_equal(s[:T, 16, 0, 0, 0], a["turn"]) and (s[:, 16] == s[:, 16, :1, :1, :1]).all()
        assert np.array_equal(s[T:], s[:T, :, :, :, ::-1]) and np.array_equal(p[:T], a["pi"]) and np.array_equal(p[T:], a["pi_mirror"])
        assert np.array_equal(z[:T], a["z"]) and np.array_equal(z[T:], a["z"])
        assert R.compare_rows((s, p, z), (s, p, z)) == 0.0 and R.compare_rows((s, p.astype(np.float32), z), (s, p, z), pi_atol=1e-6) < 1e-7


# ------------------------------------------------------------------ (2) the mutation table
def _rows_by_rule(g, slot_ply=lambda t, i, T: t - i, pad="start", src_ply=lambda t: t, turn_of=lambda turn, t: turn[t], mirror_axis=-1,
                  permute_pi=True, z_of=None, swap_colours=False):
    """Rows of game ``g`` formed by an index rule over its positions, the way a kernel forms them. Defaults = the right rule:
    history slot i of ply t is the position of ply max(t - i, 0) (game.py:23-44), plane 16 the side to move, the mirror image reverses
    the files and permutes pi, z as the reference assigned it."""
    a = R.game_arrays(g)
    T = a["hist"].shape[0]
    red, black = a["hist"][:, 0], a["hist"][:, 8]                                   # the position each move is played in
    st = np.zeros((T, 17, 7, 10, 9), np.float16)
    pi = np.empty((T, 2086))
    pim = np.empty((T, 2086))
    z = np.empty(T, np.float32)
    for t in range(T):
        s = src_ply(t)
        for i in range(8):
            tp = slot_ply(s, i, T)
            if tp < 0:
                if pad == "zeros":
                    continue
                tp = 0
            st[t, i], st[t, 8 + i] = (black[tp], red[tp]) if swap_colours else (red[tp], black[tp])
        st[t, 16] = turn_of(a["turn"], s)
        pi[t], pim[t] = a["pi"][s], (a["pi_mirror"] if permute_pi else a["pi"])[s]
        z[t] = a["z"][s] if z_of is None else z_of(a, s)
    return np.concatenate((st, np.flip(st, axis=mirror_axis))), np.concatenate((pi, pim)), np.concatenate((z, z))


MUTANTS = {
    "history slot i taken from ply t-i-1": dict(slot_ply=lambda t, i, T: t - i - 1 if i else t),
    "the same, on red-to-move plies only": dict(slot_ply=lambda t, i, T: t - i - (1 if i and t % 2 == 0 else 0)),
    "early plies padded with zeros, not the start position": dict(pad="zeros"),
    "turn plane inverted": dict(turn_of=lambda turn, t: 1 - turn[t]),
    "turn plane constant (the quirk leaking into default mode)": dict(turn_of=lambda turn, t: 1),
    "mirror along ranks instead of files": dict(mirror_axis=-2),
    "mirror pi not permuted": dict(permute_pi=False),
    "z sign swapped for black's plies": dict(z_of=lambda a, t: a["z"][t] * (1 if a["turn"][t] else -1)),
    "z nonzero in the drawn game (draw scored as a red win)": dict(z_of=lambda a, t: a["z"][t] if a["z"].any() else (1.0 if a["turn"][t] else -1.0)),
    "ply index taken mod 256": dict(src_ply=lambda t: t % 256),
    "history read relative to ply t mod 256": dict(slot_ply=lambda t, i, T: t % 256 - i),
    "red and black plane blocks swapped": dict(swap_colours=True),
}


def _old_four_ply_check(rows):
    """What test_device_harvest_reproduces_the_reference_tuples[quirks=False] asserted before this fixture, on the one game it ran on
    (the 72-ply game): pi and z at all rows; states at t in (0, 1, 9, T-1), history slots 0 and 3 of either colour, the turn plane,
    the mirror row; all 16 history planes of the last ply."""
    a = R.game_arrays(0)
    states, pi, z = rows
    T = a["hist"].shape[0]
    red, black = a["hist"][:, 0], a["hist"][:, 8]
    ok = np.allclose(pi[:T], a["pi"], rtol=0, atol=1e-6) and np.allclose(pi[T:], a["pi_mirror"], rtol=0, atol=1e-6)
    ok = ok and np.array_equal(z[:T], a["z"].astype(np.float32)) and np.array_equal(z[T:], a["z"].astype(np.float32))
    for t in (0, 1, 9, T - 1):
        back = max(0, t - 3)
        ok = ok and np.array_equal(states[t][0], red[t]) and np.array_equal(states[t][8], black[t]) and bool(np.all(states[t][16] == a["turn"][t]))
        ok = ok and np.array_equal(states[t][3], red[back]) and np.array_equal(states[t][11], black[back])
        ok = ok and np.array_equal(states[T + t], states[t][:, :, :, ::-1])
    return bool(ok and np.array_equal(states[T - 1][:16], a["hist"][T - 1]))


def _mutation_table():
    if "table" not in _cache:
        for g in GAMES:                                                             # the right rule passes, on every game
            R.compare_rows(_rows_by_rule(g), R.expected_rows(g), label=f"game {g}")
        assert _old_four_ply_check(_rows_by_rule(0))
        rows = []                                                                   # (mutant, old check accepts, games rejected, first finding)
        for name, kw in MUTANTS.items():
            rejected, first = [], ""
            for g in GAMES:
                try:
                    R.compare_rows(_rows_by_rule(g, **kw), R.expected_rows(g), label=f"game {g}")
                except AssertionError as e:
                    rejected.append(g)
                    first = first or str(e).split(";")[0]
            rows.append((name, _old_four_ply_check(_rows_by_rule(0, **kw)), rejected, first))
        _cache["table"] = rows
    return _cache["table"]


def format_table(rows):
    lines = ["| mutant | four-ply check (72-ply game) | comparison with the fixture | games rejected | first finding |", "|---|---|---|---|---|"]
    for name, old, rejected, first in rows:
        lines.append(f"| {name} | {'accepts' if old else 'rejects'} | {'rejects' if rejected else 'ACCEPTS'} | {len(rejected)} of {len(GAMES)} | {first} |")
    return "\n".join(lines)


def test_mutation_table():
    rows = _mutation_table()
    print("\n" + format_table(rows))
    assert len(rows) == 12
    for name, old, rejected, first in rows:
        assert rejected, f"the comparison accepts the mutant: {name}"
    by_name = {r[0]: r for r in rows}
    long_games = [g for g in GAMES if META["games"][g]["plies"] > 256]
    drawn = [g for g in GAMES if META["games"][g]["winner"] is None]
    # what the four-ply check let through, the documented reason for the fixture: it never saw a ply past 255 or a draw, and a slot
    # slip that spares the four plies it looked at
    for name in ("ply index taken mod 256", "history read relative to ply t mod 256"):
        assert by_name[name][1] and by_name[name][2] == long_games
    assert by_name["the same, on red-to-move plies only"][1] and len(by_name["the same, on red-to-move plies only"][2]) == len(GAMES)
    assert by_name["z nonzero in the drawn game (draw scored as a red win)"][1] and by_name["z nonzero in the drawn game (draw scored as a red win)"][2] == drawn
    # every defect that is not tied to a length or a result shows in every game
    for name in ("history slot i taken from ply t-i-1", "early plies padded with zeros, not the start position", "turn plane inverted",
                 "turn plane constant (the quirk leaking into default mode)", "mirror along ranks instead of files", "mirror pi not permuted",
                 "red and black plane blocks swapped"):
        assert len(by_name[name][2]) == len(GAMES), name


@pytest.mark.parametrize("defect", ["dtype", "outside support", "one ulp"])
def test_comparison_helper_is_strict_about_pi(defect):
    s, p, z = R.expected_rows(2)
    if defect == "dtype":        # float32 pi is not "bit for bit" the reference's float64
        with pytest.raises(AssertionError, match="bit for bit"):
            R.compare_rows((s, p.astype(np.float32), z), (s, p, z))
    elif defect == "outside support":
        q = p.astype(np.float32)
        q[5, int(np.flatnonzero(p[5] == 0)[0])] = 1e-9
        with pytest.raises(AssertionError, match="outside the support"):
            R.compare_rows((s, q, z), (s, p, z), pi_atol=1e-6)
    else:
        q = p.copy()
        k = int(p[40].argmax())
        q[40, k] = np.nextafter(q[40, k], 0)
        with pytest.raises(AssertionError, match="ply 40"):
            R.compare_rows((s, q, z), (s, p, z))
