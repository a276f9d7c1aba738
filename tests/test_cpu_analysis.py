"""CPU: the host side of the batched position analysis (chinesechesszero_amd/analyse.py): the two engine entry points are
declared, bound and exported; the input-file parser; the result record; the centipawn display mapping; no GPU, no analysis."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ccz_set_positions", "ccz_principal_variations")


def test_new_entry_points_are_declared_bound_and_exported():
    from chinesechesszero_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cczero.h")).read()
    declared = set(re.findall(r"\b(ccz_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/cczero.h"
        assert name in _lib.PROTOTYPES, f"{name} is not bound in _lib.PROTOTYPES"
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert len(_lib.PROTOTYPES["ccz_set_positions"][1]) == 10 and len(_lib.PROTOTYPES["ccz_principal_variations"][1]) == 10
    assert L.ccz_abi_version() == 9     # (the number these additions left alone; ABI 9 is the record calls)


def test_null_engine_is_refused_by_both_entry_points():
    from chinesechesszero_amd import _lib
    L = _lib.lib()
    assert L.ccz_set_positions(None, None, None, None, None, None, None, 0, None, None) == -1
    assert b"null engine" in L.ccz_last_error()
    assert L.ccz_principal_variations(None, None, 1, 1, None, None, None, None, None, None) == -1
    assert b"null engine" in L.ccz_last_error()


def test_parser_skips_comments_reads_fen_with_moves_and_names_the_bad_line():
    from chinesechesszero_amd import analyse
    from chinesechesszero_amd.game import Board, start_squares
    text = ["# an opening book\n", "\n", "startpos\n", "startpos moves h2e2 h9g7   # central cannon\n",
            "   \n", "position fen 4k4/9/9/9/9/9/9/9/4R4/3K5 b - - 7 1 moves e9d9\n"]
    got = analyse.parse_positions(text)
    assert [no for no, _ in got] == [3, 4, 6]
    b0, b1, b2 = (b for _, b in got)
    assert isinstance(b0, Board) and not b0.move_stack and np.array_equal(b0.squares(), start_squares())
    assert [m.uci() for m in b1.move_stack] == ["h2e2", "h9g7"] and b1.turn is True
    assert np.array_equal(b1._start[0], start_squares())          # the start position travels with the moves: the device replays them
    sq = b2._start[0]
    assert sq[4 + 9 * 9] == 7 + 8 and sq[4 + 9 * 1] == 3 and sq[3] == 7 and int(sq.astype(bool).sum()) == 3
    assert b2._start[1] is False and b2._start[2] == 7 and [m.uci() for m in b2.move_stack] == ["e9d9"] and b2.halfmove_clock == 8
    for bad in ("startpos moves h2e2 zz99\n", "fen 9/9/9 w\n", "somewhere else\n"):
        with pytest.raises(ValueError, match=r"^line 3: "):
            analyse.parse_positions(["startpos\n", "# c\n", bad])


def test_moves_are_not_checked_on_the_host():
    """The parser must not ask the (GPU-backed) rules: an illegal but well-formed move is the device's to refuse."""
    from chinesechesszero_amd import analyse
    (no, b), = analyse.parse_positions(["startpos moves a0a5 a9a4"])
    assert no == 1 and [m.uci() for m in b.move_stack] == ["a0a5", "a9a4"]


def test_record_shape_and_json_round_trip():
    from chinesechesszero_amd import analyse
    rec = analyse.make_record("ok", np.int32(400), [{"moves": ["h2e2", "h9g7"], "visits": np.array([120, 30], np.int32), "q": np.float32(0.25),
                                                     "prior": np.float32(0.5)},
                                                    {"moves": ["b2e2"], "visits": np.array([90], np.int32), "q": np.float32(-0.5), "prior": np.float32(0.125)}])
    assert list(rec) == ["status", "bestmove", "root_visits", "lines"]
    assert rec["status"] == "ok" and rec["bestmove"] == "h2e2" and rec["root_visits"] == 400
    assert rec["lines"][0] == {"moves": ["h2e2", "h9g7"], "visits": [120, 30], "q": 0.25, "prior": 0.5}
    assert rec["lines"][1] == {"moves": ["b2e2"], "visits": [90], "q": -0.5, "prior": 0.125}
    assert json.loads(json.dumps(rec)) == rec                      # plain Python numbers only
    for status in ("illegal move 3", "invalid position", "game over: red wins"):
        bad = analyse.make_record(status)
        assert bad == {"status": status, "bestmove": None, "root_visits": 0, "lines": []}


def test_cp_is_the_arena_elo_of_the_first_moves_score():
    from chinesechesszero_amd import analyse, arena
    for q, n in ((0.0, 100), (0.25, 37), (-0.6, 400), (1.0, 12), (-1.0, 12), (1.0, 0), (0.999, 5)):
        assert analyse.cp_of(q, n) == round(arena.elo_of_score((1 + q) / 2, games=max(1, n)))
    assert analyse.cp_of(0.0, 10) == 0 and analyse.cp_of(0.5, 1000) == -analyse.cp_of(-0.5, 1000) == 191
    assert analyse.cp_of(1.0, 400) > analyse.cp_of(1.0, 40) > 0     # a forced win: finite, growing with the visits (the clamp)


def test_uci_announces_and_sets_multipv_without_a_gpu():
    import io
    from chinesechesszero_amd.uci import UciLoop
    out = io.StringIO()
    loop = UciLoop(policy_value_fn=lambda *a: None, out=out)
    assert loop.multipv == 1
    loop.handle("uci")
    assert "option name MultiPV type spin default 1 min 1 max 128" in out.getvalue().splitlines()
    loop.handle("setoption name MultiPV value 3")
    assert loop.multipv == 3
    loop.handle("setoption name Playouts value 77")
    assert loop.n_playout == 77 and loop.multipv == 3


def test_batched_analysis_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from chinesechesszero_amd import analyse
    from chinesechesszero_amd._lib import CczError
    with pytest.raises(CczError):
        analyse.BatchedAnalysis(lambda leaf: None, 4, n_playout=8)
