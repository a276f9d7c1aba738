"""CPU: policy surprise weighting without a GPU -- the option and its command line (options.py), the header constants, ``record_weights``
on hand-built records, the weight rule and the rejection draw of tests/surprise_model.py on hand cases.

Every test calls what the parent commit does not have."""
import argparse
import math
import os
import re

import numpy as np
import pytest
import torch

import surprise_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- 1. the option
def _parse(argv):
    from chinesechesszero_amd.options import add_surprise_args, surprise_from_args
    ap = argparse.ArgumentParser()
    add_surprise_args(ap)
    return surprise_from_args(ap, ap.parse_args(argv))


def test_make_surprise_and_the_argument_trio(capsys):
    from chinesechesszero_amd.options import SURPRISE_CAP, SURPRISE_WEIGHT, make_surprise
    assert (SURPRISE_WEIGHT, SURPRISE_CAP) == (0.5, 8.0)
    assert make_surprise(None) is None and make_surprise(None, 4.0) is None
    assert make_surprise(0.5) == {"alpha": 0.5, "cap": 8.0}
    assert make_surprise(0.0, 1.0) == {"alpha": 0.0, "cap": 1.0} and make_surprise(1.0, 15.0) == {"alpha": 1.0, "cap": 15.0}
    for bad in ((-0.01, None), (1.01, None), (float("nan"), None), (0.5, 0.99), (0.5, 15.01), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            make_surprise(*bad)
    assert _parse([]) is None
    assert _parse(["--surprise-weight", "0.5"]) == {"alpha": 0.5, "cap": 8.0}
    assert _parse(["--surprise-weight", "0.25", "--surprise-cap", "4"]) == {"alpha": 0.25, "cap": 4.0}
    for argv, text in ((["--surprise-cap", "4"], "--surprise-cap without --surprise-weight"), (["--surprise-weight", "2"], "must be in [0, 1]"),
                       (["--surprise-weight", "0.5", "--surprise-cap", "16"], "must be in [1, 15]")):
        with pytest.raises(SystemExit):
            _parse(argv)
        assert text in capsys.readouterr().err


def test_the_engine_default_is_the_command_lines():
    import inspect

    from chinesechesszero_amd.engine import SelfPlayEngine
    from chinesechesszero_amd.options import SURPRISE_CAP, SURPRISE_WEIGHT
    p = inspect.signature(SelfPlayEngine.set_surprise).parameters
    assert (p["alpha"].default, p["cap"].default) == (SURPRISE_WEIGHT, SURPRISE_CAP)


OTHERS = {"resign": {"threshold": -0.9}, "root_exploration": {"eps": 0.25}, "solver": True,
          "search": {"fpu_mode": 1, "fpu_value": 0.3}, "early_stop": {"single_reply": True, "gap_factor": 1.0, "kld_interval": 0, "min_gain": 0.0, "min_sims": 0}}


def test_the_option_goes_with_every_other_one_and_not_with_the_one_game_path():
    from chinesechesszero_amd.options import SearchOptions
    cfg = {"alpha": 0.5, "cap": 8.0}
    o = SearchOptions(16, surprise=cfg, **OTHERS)
    assert list(o.on) == list(OTHERS) + ["surprise"] and o.surprise == cfg and o.surprise is not cfg
    assert list(o.keywords())[-1] == "surprise"
    assert SearchOptions(16, surprise=cfg, gumbel=True, solver=True, resign=-0.9).on["surprise"] == cfg
    assert SearchOptions(16, "numpy", surprise=cfg).on == {"surprise": cfg}              # both sampling modes
    assert SearchOptions(16, surprise=0.25).surprise == {"alpha": 0.25} and SearchOptions(16, surprise=True).surprise == {}
    assert SearchOptions(16, surprise=None).on == {} and SearchOptions(16, surprise=None).surprise is None
    assert not hasattr(SearchOptions(16, resign=-0.9), "surprise")                       # a front end that does not take the keyword
    with pytest.raises(ValueError, match="policy surprise weighting runs on the batched path"):
        SearchOptions(16, batched=False, surprise=cfg)

    class Engine:
        calls = []

        def set_surprise(self, **kw):
            self.calls.append(kw)

        def surprise_stats(self):
            return {"target_plies": 200, "surprise_sum": 50.0, "weights_clipped": 5}
    e = Engine()
    o = SearchOptions(16, surprise=cfg)
    o.apply(e)
    assert e.calls == [cfg]
    assert o.log_line(e) == ", surprise per target ply 0.2500 over 200, weights clipped 0.0250"
    assert o.report(e) == {"surprise": {"target_plies": 200, "surprise_sum": 50.0, "weights_clipped": 5, "mean_surprise": 0.25, "clipped_share": 0.025}}


def test_the_collector_takes_it_and_arena_and_analysis_do_not(capsys):
    import inspect

    from chinesechesszero_amd import collect
    from chinesechesszero_amd.arena import Arena
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    a = collect.parse_args(["--boards", "8", "--surprise-weight", "0.5", "--gumbel", "--solver"])
    assert a.options["surprise"] == {"alpha": 0.5, "cap": 8.0}
    assert collect.parse_args(["--boards", "8"]).options["surprise"] is None
    with pytest.raises(SystemExit):
        collect.parse_args(["--boards", "1", "--surprise-weight", "0.5"])
    assert "batched path" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        collect.parse_args(["--boards", "8", "--surprise-cap", "4"])
    assert "--surprise-cap without --surprise-weight" in capsys.readouterr().err
    assert "surprise" in inspect.signature(BatchedSelfPlay.__init__).parameters
    assert "surprise" in inspect.signature(collect.CollectPipeline.__init__).parameters
    assert "surprise" not in inspect.signature(Arena.__init__).parameters


# ---------------------------------------------------------------------------------------------------------------- 2. the header
def test_the_header_has_the_flag_and_the_abi_is_still_9():
    from chinesechesszero_amd import _lib
    with open(os.path.join(ROOT, "include", "cczero.h")) as f:
        text = f.read()
    assert re.search(r"#define CCZ_REC_WEIGHT 16\b", text) and re.search(r"#define CCZ_ABI_VERSION 9\b", text)
    assert re.search(r"#define CCZ_SNAP_SURPRISE 4u", text)
    assert (_lib.REC_WEIGHT, _lib.REC_WEIGHT_OFF, _lib.REC_WEIGHT_ONE, _lib.ABI_VERSION) == (16, 90, 4096, 9)
    for name in ("ccz_set_surprise", "ccz_get_surprise_stats", "ccz_ply_surprise", "ccz_sample_records_weighted"):
        assert re.search(r"\bint " + name + r"\(", text), name
    L = _lib.lib()
    assert L.ccz_abi_version() == 9 and L.ccz_sample_records_weighted is not None


# ---------------------------------------------------------------------------------------------------------------- 3. record_weights
def test_record_weights_with_and_without_the_flag():
    from chinesechesszero_amd.replay import record_weights
    rec = np.concatenate([sm.hand_game(4, [0.0, 0.5, 1.0, 4.0], 3), sm.hand_game(3, None, 4), sm.hand_game(2, [15.0, 1.0 + 1.0 / 4096], 5)])
    rec[5, 90:92] = 255                                    # bytes without the flag are not a weight
    w = record_weights(torch.from_numpy(rec))
    assert w.dtype == torch.float32 and w.shape == (9,)
    assert w.tolist() == [0.0, 0.5, 1.0, 4.0, 1.0, 1.0, 1.0, 15.0, 1.0 + 1.0 / 4096]
    assert np.array_equal(w.numpy(), sm.weights_of(rec))
    with pytest.raises(ValueError):
        record_weights(torch.zeros((3, 879), dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- 4. the weight rule
def test_the_weight_rule_on_hand_cases():
    f = np.float32
    # S = 0: every ply weighs 1, whatever alpha says
    wq, c = sm.game_weights([f(0), f(0), f(0)], [1, 1, 1], 0.5, 8.0)
    assert wq.tolist() == [4096] * 3 and c == 0
    # n = 1: the one target ply gets (1 - a) + a = 1; the fast plies 1
    wq, c = sm.game_weights([f(0), f(0.7), f(0)], [0, 1, 0], 0.5, 8.0)
    assert wq.tolist() == [4096] * 3 and c == 0
    # a game of fast plies only: F is empty
    wq, c = sm.game_weights([f(0), f(0)], [0, 0], 1.0, 8.0)
    assert wq.tolist() == [4096, 4096] and c == 0
    # the rule itself: s = (1, 3), alpha = 0.5: w = 0.5 + 0.5 * 2 * s / 4 = (0.75, 1.25); the weights of F sum to n
    wq, c = sm.game_weights([f(1), f(3)], [1, 1], 0.5, 8.0)
    assert wq.tolist() == [3072, 5120] and c == 0
    # a fast ply between them keeps 1 and does not count in n
    wq, c = sm.game_weights([f(1), f(9), f(3)], [1, 0, 1], 0.5, 8.0)
    assert wq.tolist() == [3072, 4096, 5120] and c == 0
    # alpha = 1, all the surprise on one of 10 plies: w = 10, clipped at 8 (and counted); the others 0 -- plies that are never drawn
    wq, c = sm.game_weights([f(0)] * 9 + [f(2)], [1] * 10, 1.0, 8.0)
    assert wq.tolist() == [0] * 9 + [8 * 4096] and c == 1
    # a weight exactly at the cap is not clipped
    wq, c = sm.game_weights([f(1), f(3)], [1, 1], 0.5, 1.25)
    assert wq.tolist() == [3072, 5120] and c == 0
    wq, c = sm.game_weights([f(1), f(3)], [1, 1], 0.5, 1.0)
    assert wq.tolist() == [3072, 4096] and c == 1
    # quantisation: floor(w * 4096 + 0.5). s = (8191, 8193) / 16384 with alpha = 1, n = 2, S = 1: w * 4096 = 4095.5 and 4096.5 exactly
    wq, c = sm.game_weights([f(8191 / 16384), f(8193 / 16384)], [1, 1], 1.0, 8.0)
    assert wq.tolist() == [4096, 4097]
    wq, c = sm.game_weights([f(8190 / 16384), f(8194 / 16384)], [1, 1], 1.0, 8.0)     # 4095.0 and 4097.0: no rounding at all
    assert wq.tolist() == [4095, 4097]
    wq, c = sm.game_weights([f(16381 / 32768), f(16387 / 32768)], [1, 1], 1.0, 8.0)   # 4095.25 rounds down, 4096.75 up
    assert wq.tolist() == [4095, 4097]


def test_the_surprise_of_a_ply_on_hand_cases():
    from gumbel_model import det_log
    # pi = prior: 0 (a sum that rounds below 0 is clamped)
    P = np.array([0.5, 0.25, 0.25], np.float32)
    assert sm.surprise_of(P.astype(np.float64), P) == 0.0
    # the search overturned the prior: pi = (0, 1) on P = (0.75, 0.25): log 4
    s = sm.surprise_of(np.array([0.0, 1.0]), np.array([0.75, 0.25], np.float32))
    assert s == np.float32(det_log(1.0) - det_log(0.25)) and abs(float(s) - math.log(4.0)) < 1e-6
    # a prior of 0 under a visited child is floored at 2^-100, not infinite
    s = sm.surprise_of(np.array([1.0]), np.array([0.0], np.float32))
    assert np.isfinite(s) and abs(float(s) - 100 * math.log(2.0)) < 1e-4
    # entries with pi = 0 add nothing, whatever their prior
    assert sm.surprise_of(np.array([0.0, 0.5, 0.5]), np.array([0.0, 0.5, 0.5], np.float32)) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 5. the rejection draw
N_DRAWS, SEED, CAP_Q = 1200, 0x1234_5678_9abc_def1, 4 * 4096


def _window():
    """A ring of 16 slots, window [2, 12): a cut game at the tail (logical plies 0..3, of which 2 and 3 lie in the window), the game of four
    plies with weights {0, 0.5, 1, 4} at [4, 8), a game without the flag at [8, 12) (each ply weighs 1)."""
    ring = np.zeros((16, 880), np.uint8)
    ring[0:4] = sm.hand_game(4, [4.0] * 4, 1)
    ring[4:8] = sm.hand_game(4, [0.0, 0.5, 1.0, 4.0], 2)
    ring[8:12] = sm.hand_game(4, None, 3)
    return ring, 2, 12


def test_the_rejection_draw_follows_the_weights():
    ring, tail, head = _window()
    counts, passes, fallbacks = np.zeros(16, int), np.zeros(2, int), 0
    for j in range(N_DRAWS):
        u, fell, bad = sm.weighted_draw(ring, 16, tail, head, SEED, j, CAP_Q)
        ok, p, q, _ = sm.locate(ring, 16, tail, head, u, 2)
        assert ok and not bad
        fallbacks += fell
        counts[p] += 1
        passes[q] += 1
    assert fallbacks == 0                      # mean acceptance 9.5 / 10 / 4 per candidate: 0.76^256 per row
    w = np.array([0, 0, 0, 0, 0.0, 0.5, 1.0, 4.0, 1, 1, 1, 1, 0, 0, 0, 0])
    assert counts[w == 0].sum() == 0           # the weight-0 ply and the plies of the cut game are never drawn
    for p in np.nonzero(w)[0]:
        prob = w[p] / w.sum()
        sd = math.sqrt(N_DRAWS * prob * (1 - prob))
        assert abs(counts[p] - N_DRAWS * prob) <= 5 * sd, (p, counts[p], N_DRAWS * prob, sd)
    assert abs(passes[0] - N_DRAWS / 2) <= 5 * math.sqrt(N_DRAWS / 4)    # the pass comes from u: both share the ply's weight
    # N is large enough for the check to say something: the rarest drawn ply (weight 0.5 of 9.5) is expected 63 times, more than 5 sd (5 x 7.9)
    # above 0, so its band excludes "never drawn"; and a uniform draw (1200 / 10 = 120 per ply) would miss the weight-4 ply's 505 +- 5 x 17 by far
    assert N_DRAWS * 0.5 / 9.5 > 5 * math.sqrt(N_DRAWS * (0.5 / 9.5))
    assert abs(120 - N_DRAWS * 4 / 9.5) > 5 * math.sqrt(N_DRAWS * (4 / 9.5) * (5.5 / 9.5))


def test_the_rejection_draw_at_its_edges():
    ring, tail, head = _window()
    # all weights 0: every row falls back to candidate (0, 0); bad iff that candidate is no whole game of the window
    zero = ring.copy()
    zero[:, 90:92] = 0
    zero[:, sm.FLAGS] |= sm.REC_WEIGHT
    seen = set()
    for j in range(40):
        u, fell, bad = sm.weighted_draw(zero, 16, tail, head, SEED, j, CAP_Q)
        assert fell and u == sm.candidate(SEED, j, 0, 0)[0]
        assert bad == (not sm.locate(zero, 16, tail, head, u, 2)[0])
        seen.add(bad)
    assert seen == {False, True}               # 2 of the window's 10 plies belong to the cut game
    # an empty window: nothing is ok
    u, fell, bad = sm.weighted_draw(ring, 16, 5, 5, SEED, 0, CAP_Q)
    assert fell and bad
    # candidates are 62-bit and a < 1; another row or another seed draws other candidates
    us = {sm.candidate(SEED, j, r, lane) for j in range(2) for r in range(4) for lane in range(64)}
    assert len(us) == 512 and all(0 <= u < 2 ** 62 and 0.0 <= a < 1.0 for u, a in us)
    assert sm.candidate(SEED + 1, 0, 0, 0) != sm.candidate(SEED, 0, 0, 0)
    # the cap scales the acceptance: with cap_q = the largest weight, that ply is always accepted
    for j in range(20):
        for r in range(2):
            u, a = sm.candidate(SEED, j, r, 0)
            ok, p, _, wq = sm.locate(ring, 16, tail, head, u, 2)
            if ok and wq == CAP_Q:
                assert a * float(CAP_Q) < float(wq)
