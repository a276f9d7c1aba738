"""CPU: the position pairs of tests/cache_collision_cases.py are what the forced-collision tests of the evaluation cache
(tests/test_gpu_cache_key_collisions.py) take them for. Asserted on the CPU oracle so that the fixtures cannot drift: both positions
of a pair are live, legal and loadable, and their ``legal_ids()`` lists stand in the stated relation -- the relation decides which
part of cache_tag (csrc/cczero_kernels.h) has to tell the two apart once a salt has given them one 64-bit key."""
import numpy as np
import pytest

import cache_collision_cases as ccc
from oracle import OracleBoard


def _ids(p):
    return OracleBoard.from_array(p[0], p[1], 0).legal_ids()


@pytest.mark.parametrize("name", ccc.PAIRS)
def test_both_positions_of_a_pair_are_live_legal_and_loadable(name):
    X, Y, _ = ccc.pairs()[name]
    assert not (np.array_equal(X[0], Y[0]) and X[1] == Y[1])                    # two positions
    for squares, turn in (X, Y):
        b = OracleBoard.from_array(squares, turn, 0)
        assert not b.is_game_over() and not b.is_tie() and b.legal_ids()
        assert not OracleBoard.from_array(squares, 1 - turn, 0).in_check()      # the side that has just moved is not in check
        assert ccc.misplaced(squares) == []
        assert ccc.loadable(squares)


@pytest.mark.parametrize("name", ccc.PAIRS)
def test_the_stated_relation_between_the_legal_move_lists(name):
    X, Y, rel = ccc.pairs()[name]
    a, b = _ids(X), _ids(Y)
    if rel == "same_list":
        assert a == b and name in ccc.TWINS
    elif rel == "different_count":
        assert len(a) != len(b) and len(a) & 0xff != len(b) & 0xff
    elif rel == "wide_equal_count":
        # lanes 0..63 of the probe's wave see the same first id and the same count: only the second id of a lane (entry 64 + lane) differs
        assert len(a) == len(b) > 64 and X[1] == Y[1] and a[:64] == b[:64] and a[64:] != b[64:]
    else:
        assert rel == "equal_count" and len(a) == len(b) and a != b and X[1] == Y[1]
    assert (rel == "same_list") == (name in ccc.TWINS)


def test_counts_of_the_named_pairs():
    p = ccc.pairs()
    assert [len(_ids(x)) for x in p["twin"][:2]] == [44, 44]
    assert [len(_ids(x)) for x in p["wide_twin"][:2]] == [108, 108]             # live lanes 64 and up on both sides of the probe
    assert [len(_ids(x)) for x in p["wide_different"][:2]] == [108, 103]
    assert len(_ids(p["different_count"][0])) == 44
    a, b = (_ids(x) for x in p["wide_equal_count"][:2])
    assert len(a) == len(b) == 98 and [i for i in range(98) if a[i] != b[i]][0] == 73 and sum(x != y for x, y in zip(a, b)) == 19
    # the twins differ in one swap / one king move only
    assert int((p["twin"][0][0] != p["twin"][1][0]).sum()) == 2 and int((p["wide_twin"][0][0] != p["wide_twin"][1][0]).sum()) == 2


def test_the_pool_has_no_pair_whose_lists_differ_in_exactly_one_entry():
    """No two pool positions of one side to move and one count have ordered lists that differ in exactly ONE entry (two positions
    that differ in where one piece may go differ in several ids, or in the count). Recorded so that a pool that grows such a pair
    is noticed: it would be the weakest input of the 24-bit list hash and belongs among the pairs."""
    assert ccc.one_entry_pool_pairs() == []


def test_the_checks_of_this_file_reject_what_they_should():
    start = ccc.start_position()
    bad = start.copy()
    bad[ccc.sq("e0")], bad[ccc.sq("e4")] = 0, 7                                 # a king outside its palace
    assert ccc.misplaced(bad) == [ccc.sq("e4")]
    bad = start.copy()
    bad[ccc.sq("a6")], bad[ccc.sq("b6")] = 0, 9                                 # a black pawn on its own side, off the pawn files
    assert ccc.misplaced(bad) == [ccc.sq("b6")]
    two_kings = start.copy()
    two_kings[40] = 7
    assert not ccc.loadable(two_kings) and ccc.loadable(start) and not ccc.loadable(start, halfmove=-1)
    code8 = start.copy()
    code8[40] = 8
    assert not ccc.loadable(code8)


def test_search_moves_of_the_adversarial_salts_test():
    """P and Q: red first moves after which black's reply lists differ (the cannon capture b2xb9 takes a knight: 41 replies against
    44); Q': a second quiet move with P's reply list, in the same order -- a twin of P."""
    m = ccc.search_positions()
    o = OracleBoard()
    assert all(x in o.legal_ids() for x in m.values()) and len(set(m.values())) == 3
    lists = {}
    for name, mv in m.items():
        squares, turn = ccc.after(mv)
        assert turn == 0 and ccc.misplaced(squares) == [] and ccc.loadable(squares)
        b = OracleBoard.from_array(squares, turn, 0)
        assert not b.is_game_over() and not b.is_tie() and not OracleBoard.from_array(squares, 1, 0).in_check()
        lists[name] = b.legal_ids()
    assert int((ccc.after(m["Q"])[0] != 0).sum()) == 31                         # a capture
    assert len(lists["P"]) == 44 and len(lists["Q"]) == 41
    assert lists["Q_twin"] == lists["P"] and not np.array_equal(ccc.after(m["P"])[0], ccc.after(m["Q_twin"])[0])
