"""CPU: the width fixtures of tests/golden_cases.py (STARTS / WIDTHS) have the legal-move counts the GPU boundary tests rely on.

The per-board kernels hold legal move i and 64 + i in lane i of one wave64 wave (csrc/cczero_kernels.h: softmax_gather_board,
expand_backup_phase, cache_probe_wave), so 64 / 65 / the widest position found, one legal move and none are the edges. The counts
are asserted on the CPU oracle so that the fixtures cannot drift."""
import numpy as np
import pytest

from golden_cases import STARTS, WIDTHS, mirrored
from oracle import OracleBoard


@pytest.mark.parametrize("name", sorted(WIDTHS))
def test_legal_count_of_each_width_fixture(name):
    turn, k = WIDTHS[name]
    b = OracleBoard.from_array(STARTS[name], turn, 0)
    ids = b.legal_ids()
    assert len(ids) == k, (name, len(ids))
    assert ids == sorted(ids)
    assert b.is_game_over() == (k == 0) and not b.is_tie()
    # a legal position: the side that has just moved does not stand in check
    assert not OracleBoard.from_array(STARTS[name], 1 - turn, 0).in_check()


def test_the_mated_fixtures_are_checkmate():
    for name in ("mated", "mated_black"):
        turn, _ = WIDTHS[name]
        b = OracleBoard.from_array(STARTS[name], turn, 0)
        assert b.in_check() and b.legal_ids() == [] and b.outcome().winner == (turn == 0)


def test_black_fixtures_are_the_mirrored_red_ones():
    for name, (turn, k) in WIDTHS.items():
        if name.endswith("_black"):
            assert turn == 0 and WIDTHS[name[:-6]] == (1, k)
            assert np.array_equal(STARTS[name], mirrored(STARTS[name[:-6]]))
            assert np.array_equal(mirrored(STARTS[name]), STARTS[name[:-6]])


def test_widest_fixtures_reach_the_last_dword_of_the_logit_row():
    """The widest pair has legal ids in the last, partial iteration of the fp16 dword loop (ids 2048..2085): red i2g0 (2067), and
    black i7g9 (2085, the high half of the last dword). A row maximum placed there is a LEGAL prior."""
    red = OracleBoard.from_array(STARTS["widest"], 1, 0).legal_ids()
    black = OracleBoard.from_array(STARTS["widest_black"], 0, 0).legal_ids()
    assert len(red) > 100 and 2067 in red
    assert len(black) > 100 and 2085 in black and black[-1] == 2085


def test_a_wide_fixture_has_the_first_logit_of_the_row_legal():
    """wide_a0 has a0a1 (id 0: the low half of lane 0's first fp16 dword, lane 0's first fp32 element) legal, as its first legal id:
    a row maximum placed on id 0 is a LEGAL prior."""
    ids = OracleBoard.from_array(STARTS["wide_a0"], 1, 0).legal_ids()
    assert len(ids) > 64 and ids[0] == 0
