"""CPU: the LCB move's option (``options.MOVE_OPTIONS``): the command-line trio and its errors, what ``SearchOptions`` refuses, the order of
``ALL_OPTIONS``, and which library calls the front ends make with it off (none) and on. No GPU."""
import argparse

import numpy as np
import pytest

from chinesechesszero_amd import options as O


def _parser():
    ap = argparse.ArgumentParser()
    O.add_lcb_args(ap)
    return ap


def test_the_cli_trio():
    ap = _parser()
    assert O.lcb_from_args(ap, ap.parse_args([])) is None
    assert O.lcb_from_args(ap, ap.parse_args(["--lcb"])) == {"z": 5.0, "min_visit_ratio": 0.15, "min_visits": 2}
    assert O.lcb_from_args(ap, ap.parse_args(["--lcb", "2.5"]))["z"] == 2.5
    assert O.lcb_from_args(ap, ap.parse_args(["--lcb", "0"])) == {"z": 0.0, "min_visit_ratio": 0.15, "min_visits": 2}     # z = 0 is a setting, not "off"
    got = O.lcb_from_args(ap, ap.parse_args(["--lcb", "--lcb-min-visit-ratio", "0.5", "--lcb-min-visits", "7"]))
    assert got == {"z": 5.0, "min_visit_ratio": 0.5, "min_visits": 7}


@pytest.mark.parametrize("argv", [["--lcb-min-visit-ratio", "0.5"], ["--lcb-min-visits", "3"], ["--lcb", "-1"], ["--lcb", "inf"], ["--lcb", "nan"],
                                  ["--lcb", "--lcb-min-visit-ratio", "1.5"], ["--lcb", "--lcb-min-visit-ratio", "-0.1"],
                                  ["--lcb", "--lcb-min-visits", "-1"]])
def test_the_cli_errors(argv, capsys):
    ap = _parser()
    with pytest.raises(SystemExit):
        O.lcb_from_args(ap, ap.parse_args(argv))
    assert "--lcb" in capsys.readouterr().err


def test_make_lcb():
    assert O.make_lcb(None) is None and O.make_lcb(False) is None
    assert O.make_lcb(True) == {"z": O.LCB_STDEVS, "min_visit_ratio": O.LCB_MIN_VISIT_RATIO, "min_visits": O.LCB_MIN_VISITS}
    with pytest.raises(ValueError, match="--lcb must be finite"):
        O.make_lcb(float("inf"))


def test_search_options_refusals():
    assert O.SearchOptions(8, lcb=None).lcb is None and O.SearchOptions(8, lcb=False).on == {}
    assert O.SearchOptions(8, lcb=True).lcb == O.make_lcb(True)
    assert O.SearchOptions(8, lcb={"z": 1.0}).lcb == {"z": 1.0, "min_visit_ratio": 0.15, "min_visits": 2}
    assert O.SearchOptions(8, lcb=True, solver=True, search={"fpu_mode": 1}).on.keys() == {"solver", "search", "lcb"}
    with pytest.raises(ValueError, match="lcb and gumbel"):
        O.SearchOptions(8, lcb=True, gumbel=True)
    with pytest.raises(ValueError, match="width > 1 .*lcb"):
        O.SearchOptions(8, lcb=True, width=2)
    with pytest.raises(ValueError, match="lcb needs sampling='device'"):
        O.SearchOptions(8, lcb=True, sampling="host")
    with pytest.raises(ValueError, match="min-visit-ratio"):
        O.SearchOptions(8, lcb={"z": 1.0, "min_visit_ratio": 2.0})


def test_the_order_of_all_options():
    assert list(O.OPTIONS) == ["resign", "root_exploration", "gumbel", "solver", "search", "early_stop"]
    assert list(O.INPUT_OPTIONS) == ["leaf_history"] and list(O.MOVE_OPTIONS) == ["lcb"]
    assert list(O.ALL_OPTIONS) == list(O.OPTIONS) + list(O.RECORD_OPTIONS) + ["lcb", "leaf_history"]


class _Engine:
    """What ``SearchOptions.apply`` and ``options.lcb_moves`` touch of an engine, recording the calls."""
    B = 4

    def __init__(self):
        self.calls = []

    def set_value_stats(self, enabled=True):
        self.calls.append(("set_value_stats", enabled))

    def set_solver(self, enabled=True):
        self.calls.append(("set_solver", enabled))

    def lcb_moves(self, z, r, n, with_bounds=False):
        import torch
        self.calls.append(("lcb_moves", z, r, n))
        return {"moves": torch.tensor([10, 20, -1, 40], dtype=torch.int32), "child": torch.tensor([0, 2, -1, 1], dtype=torch.int32), "lcb": None}

    def root_children(self):
        v = np.zeros((4, 128), np.int32)
        v[0, :3], v[1, :3], v[3, :3] = (5, 3, 1), (4, 4, 2), (2, 7, 7)      # arg-max children 0, 0, -, 1
        return {"visits": v}

    def game_status(self):
        return {"over": np.array([0, 0, 1, 0], np.uint8)}


def test_apply_and_the_forced_moves():
    e = _Engine()
    O.SearchOptions(8, solver=True, lcb=2.0).apply(e)
    assert e.calls == [("set_solver", True), ("set_value_stats", True)]
    e = _Engine()
    O.SearchOptions(8).apply(e)
    forced, differed = O.lcb_moves(e, None, None)
    assert e.calls == [] and forced is None and differed == 0                       # off: no call at all
    cfg = O.make_lcb(2.0)
    proven = np.array([-1, -1, -1, 99], np.int32)                                   # board 3's move is proven: it stays
    forced, differed = O.lcb_moves(e, cfg, proven.copy())
    assert e.calls == [("lcb_moves", 2.0, 0.15, 2)]
    e.calls.clear()
    assert forced.tolist() == [10, 20, -1, 99] and differed == 1                    # board 1 plays child 2, not the most visited child 0
    o = O.SearchOptions(8, lcb=True)
    assert o.lcb_counts == {"moves": 0, "differed": 0} and not hasattr(O.SearchOptions(8), "lcb_counts")
    forced, differed = O.lcb_moves(e, cfg, proven.copy(), counts=o.lcb_counts)
    assert o.lcb_counts == {"moves": 2, "differed": 1}
    forced, differed, fill, off = O.lcb_moves(e, cfg, None, allow=np.array([True, False, True, True]), counts=o.lcb_counts, detail=True)
    assert forced.tolist() == [10, -1, -1, 40] and differed == 0 and fill.tolist() == [True, False, False, True] and not off.any()
    assert o.lcb_counts == {"moves": 4, "differed": 1}
    assert o.report(e) == {"lcb": {"moves": 4, "differed": 1}}
    assert o.log_line(e) == ", lcb moves 4, off the most visited move 1 (share 0.2500)"
    assert not hasattr(e, "lcb_counts")                                             # nothing is hung on the engine
