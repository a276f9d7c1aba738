"""CPU: the model of the leaf history planes (tests/leaf_history_model.py) against the reference-produced per-ply histories
(tests/reference_rows.py, tests/golden/reference_rows.*), the key rule, the host plumbing of the option and the facts the GPU test's
scenario must show. No GPU.

(1) For every ply te of the six golden games the model's row of (S_0 .. S_te) is, byte for byte, the state the reference formed at
    that ply -- plies te < 7 (the clamp) and both sides to move included. The positions are slot 0 of each snapshot; the expectation
    is the whole snapshot, which the reference assembled itself.
(2) The history key: positions shown alike hash alike (a clamped prefix and a real repeat), any other slot tells two leaves apart.
(3) ``boundary.need_history``: an engine that writes history planes refuses an evaluator that does not declare that it reads them.
(4) The scenario of tests/test_gpu_leaf_history.py reaches every case its docstring lists (asserted on the model alone)."""
import os

import numpy as np
import pytest

import leaf_history_model as hm
import reference_rows as R

_, META = R.load()
GAMES = list(range(len(META["games"])))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- (1) rows
@pytest.mark.parametrize("g", GAMES)
def test_model_rows_are_the_reference_states(g):
    a = R.game_arrays(g)
    want = R.expected_rows(g)[0]
    T = a["hist"].shape[0]
    pos = [hm.squares_of_planes(a["hist"][t, 0], a["hist"][t, 8]) for t in range(T)]
    turns = set()
    for te in range(T):
        got = hm.row(pos[: te + 1], int(a["turn"][te]))
        assert got.dtype == np.float16 and got.tobytes() == want[te].tobytes(), (g, te)
        turns.add(int(a["turn"][te]))
    assert turns == {0, 1} and T > 8


def test_plane_of_type_moves_the_channels_only():
    a = R.game_arrays(1)
    pos = [hm.squares_of_planes(a["hist"][t, 0], a["hist"][t, 8]) for t in range(12)]
    pot = (0, 3, 0, 6, 1, 5, 2, 4)
    plain, moved = hm.row(pos, 1), hm.row(pos, 1, pot)
    for t in range(1, 8):
        assert np.array_equal(moved[:16, pot[t]], plain[:16, hm.DEFAULT_PLANES[t]])
    assert np.array_equal(moved[16], plain[16])
    assert np.array_equal(hm.squares_of_planes(moved[0], moved[8], pot), pos[-1])


# ---------------------------------------------------------------------------------------------------------------- (2) keys
def test_history_key_follows_the_positions_shown():
    a = R.game_arrays(0)
    pos = [hm.squares_of_planes(a["hist"][t, 0], a["hist"][t, 8]) for t in range(20)]
    assert hm.ZOB[0] == hm.mix64(hm.GOLDEN) and len(set(hm.ZOB)) == len(hm.ZOB)
    # a clamped prefix and a real repeat of the same positions: the same input, the same key
    short, padded = pos[:3], [pos[0]] * 5 + pos[:3]
    assert hm.row(short, 1).tobytes() == hm.row(padded, 1).tobytes() and hm.history_key(short, 1) == hm.history_key(padded, 1)
    # plies in front of the window do not count
    assert hm.history_key(pos[:12], 1) == hm.history_key(pos[4:12], 1)
    # the same leaf behind another slot 3, another slot 7, the other side to move: other keys
    keys = {hm.history_key(pos[:12], 1)}
    for i in (1, 3, 7):
        other = list(pos[:12])
        other[11 - i] = pos[19]
        assert hm.row(other, 1).tobytes() != hm.row(pos[:12], 1).tobytes()
        keys.add(hm.history_key(other, 1))
    keys.add(hm.history_key(pos[:12], 0))
    assert len(keys) == 5
    # two slots swapped: the hash is ordered
    swapped = list(pos[:12])
    swapped[8], swapped[9] = swapped[9], swapped[8]
    assert hm.history_key(swapped, 1) not in keys
    assert hm.leaf_key(pos[5], 1) ^ hm.leaf_key(pos[5], 0) == hm.TURN_KEY


# ---------------------------------------------------------------------------------------------------------------- (3) host plumbing
class _Engine:
    def __init__(self, on):
        self.leaf_history = on


def test_an_evaluator_that_does_not_read_history_is_refused():
    from chinesechesszero_amd import boundary

    def plain(leaf):
        return None

    def full(leaf):
        return None
    full.leaf_history = True

    class Net:
        leaf_history = False

        def evaluate_leaves_logits(self, leaf):
            return None
    net = Net()
    assert not boundary.reads_history(plain) and boundary.reads_history(full) and not boundary.reads_history(net)
    boundary.need_history(_Engine(False), plain)
    boundary.need_history(_Engine(True), full)
    with pytest.raises(ValueError, match="history planes"):
        boundary.need_history(_Engine(True), plain, "test: ")
    with pytest.raises(ValueError, match="history planes"):
        boundary.need_history(_Engine(True), net)
    net.leaf_history = lambda: True                      # a mode that can change: asked at every call
    boundary.need_history(_Engine(True), net)
    from chinesechesszero_amd.net import PolicyValueNet
    assert not boundary.reads_history(PolicyValueNet.evaluate_leaves_logits)   # (no object, no mode: a network says so through set_leaf_history)


def test_the_abi_declares_the_option():
    from chinesechesszero_amd import _lib
    with open(os.path.join(ROOT, "include", "cczero.h")) as f:
        header = f.read()
    for name in ("ccz_set_leaf_history", "ccz_get_leaf_history"):
        assert name in _lib.PROTOTYPES and f"int {name}(ccz_engine *e" in header
    assert "#define CCZ_ABI_VERSION 9 " in header and _lib.ABI_VERSION == 9


# ---------------------------------------------------------------------------------------------------------------- (4) the scenario
def test_the_scenario_reaches_every_case():
    m, _ = hm.scenario()
    seen, capture, black = set(), False, False
    for t in range(hm.PLIES):
        if t == hm.RESET_AT:
            m.reset_tree()
        for i in range(hm.sims_of_ply(t)):
            for b, (status, k, d) in enumerate(m.step()):
                if status != 0:
                    continue
                pos, turn = m.positions(b)
                p = len(m.plies_rec[b])
                assert p == t and len(pos) == p + d + 1
                seen.add((p, d, i))
                shown = hm.slots(pos)
                capture |= p >= 7 and np.count_nonzero(shown[0]) < np.count_nonzero(shown[7])
                black |= turn == 0
        if t + 1 < hm.PLIES:
            m.finish_move(hm.forced_of_ply(t))
            assert not any(m.over)
    pd = {(p, d) for p, d, _ in seen}
    assert (0, 0) in pd and (hm.RESET_AT, 0, 0) in seen               # a fresh tree's first leaf is the root
    assert any(d >= 8 for _, d in pd)                                   # the history lies inside the path
    assert any(p == 0 and 0 < d < 7 for p, d in pd)
    assert any(0 < p and 0 < d and p + d < 7 for p, d in pd)            # the clamp inside the game
    assert any(p >= 7 for p, _ in pd) and capture and black


def test_the_option_is_one_entry_of_the_front_ends_tables():
    from chinesechesszero_amd import options as O
    assert list(O.INPUT_OPTIONS) == ["leaf_history"] and list(O.ALL_OPTIONS)[-1] == "leaf_history" and "leaf_history" not in O.OPTIONS
    on = O.SearchOptions(16, leaf_history=True, solver=False)
    assert on.on == {"leaf_history": {"enabled": True}} and on.keywords() == {"solver": False, "leaf_history": {"enabled": True}}
    assert O.SearchOptions(16, leaf_history=False).on == {} and O.SearchOptions(16, leaf_history=None).leaf_history is None
    with pytest.raises(ValueError, match="width"):
        O.SearchOptions(16, width=2, leaf_history=True)
    with pytest.raises(ValueError, match="batched path"):
        O.SearchOptions(16, batched=False, leaf_history=True)          # the one-game scouted path
    calls = []

    class E:
        def set_leaf_history(self, enabled):
            calls.append(enabled)

        def stats(self):
            return {"cache_probes": 8, "cache_hits": 1, "cache_shared_rows": 1}
    on.apply(E())
    assert calls == [True]
    assert on.report(E()) == {"leaf_history": True, "cache_hit_share": 0.25} and on.log_line(E()).endswith("cache hit share 0.2500")
    assert O.history_report({"cache_probes": 0, "cache_hits": 0, "cache_shared_rows": 0})["cache_hit_share"] is None
