"""CPU: the collector's side of the Gumbel root search (``collect --gumbel ...``): what the command line refuses, the defaults, what
reaches ``CollectPipeline`` and ``BatchedSelfPlay``, and the log fields, computed here from fabricated counters."""
import pytest


def _parse(argv):
    from chinesechesszero_amd.collect import parse_args
    return parse_args(argv)


def test_the_feature_is_off_without_the_flag():
    a = _parse([])
    assert a.gumbel is False and a.gumbel_cfg is None
    assert _parse(["--boards", "64", "--root-noise-eps", "0.25"]).gumbel_cfg is None


@pytest.mark.parametrize("argv", [["--gumbel-considered", "8"], ["--gumbel-c-visit", "25"], ["--gumbel-c-scale", "0.5"],
                                  ["--gumbel-c-visit", "25", "--gumbel-c-scale", "0.5"]])
def test_the_other_flags_are_refused_without_it(argv, capsys):
    with pytest.raises(SystemExit):
        _parse(argv)
    err = capsys.readouterr().err
    assert "without --gumbel" in err and argv[0] in err


def test_gumbel_and_root_noise_exclude_each_other(capsys):
    with pytest.raises(SystemExit):
        _parse(["--gumbel", "--root-noise-eps", "0.25"])
    assert "--root-noise-eps" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--gumbel", "--gumbel-considered", "1"], ["--gumbel", "--gumbel-considered", "129"],
                                  ["--gumbel", "--gumbel-c-visit", "-1"], ["--gumbel", "--gumbel-c-visit", "inf"], ["--gumbel", "--gumbel-c-visit", "nan"],
                                  ["--gumbel", "--gumbel-c-scale", "-0.5"], ["--gumbel", "--gumbel-c-scale", "nan"], ["--gumbel", "--gumbel-c-scale", "inf"],
                                  ["--gumbel", "--boards", "1"], ["--gumbel", "--playout", "0"]])
def test_values_out_of_range_are_refused(argv):
    with pytest.raises(SystemExit):
        _parse(argv)


def test_defaults_and_what_reaches_the_pipeline():
    from chinesechesszero_amd import collect
    a = _parse(["--gumbel", "--playout", "64"])
    assert a.gumbel_cfg == {"n_sims": 64, "max_considered": 16, "c_visit": 50.0, "c_scale": 1.0}
    a = _parse(["--gumbel", "--gumbel-considered", "2", "--gumbel-c-visit", "0", "--gumbel-c-scale", "0", "--playout-cap-fast", "16",
                "--playout-cap-prob", "0.25", "--playout", "128"])
    assert a.gumbel_cfg == {"n_sims": 128, "max_considered": 2, "c_visit": 0.0, "c_scale": 0.0} and a.playout_cap_fast == 16
    assert _parse(["--gumbel", "--gumbel-considered", "128"]).gumbel_cfg["max_considered"] == 128
    with pytest.raises(ValueError, match="batched path"):
        collect.CollectPipeline(n_boards=1, gumbel=True)
    with pytest.raises(ValueError, match="exclude each other"):
        collect.CollectPipeline(n_boards=8, gumbel=True, root_exploration={"eps": 0.25})


def test_the_help_text_says_what_a_fast_ply_records():
    from chinesechesszero_amd.collect import build_parser
    text = " ".join(build_parser().format_help().split())
    assert "fast ply is a valid target" in text and "still flagged" in text


def test_log_fields_from_fabricated_counters():
    from chinesechesszero_amd.collect import format_gumbel
    from chinesechesszero_amd.options import OPTIONS, SearchOptions
    x = {"gumbel_moves": 400, "considered_sum": 6100, "offvisit_moves": 30}
    line = format_gumbel(x)
    assert line == ", gumbel moves 400, mean considered 15.25, off-visit share 0.0750"
    zero = format_gumbel({"gumbel_moves": 0, "considered_sum": 0, "offvisit_moves": 0})
    assert "mean considered n/a" in zero and "off-visit share n/a" in zero

    class _Engine:
        def gumbel_stats(self):
            return x

    assert OPTIONS["gumbel"].log(_Engine()) == line == SearchOptions(8, gumbel={}).log_line(_Engine())
    assert SearchOptions(8, gumbel=None).log_line(_Engine()) == ""               # off: the log line is what it was


def test_selfplay_refusals_come_before_an_engine_is_built():
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    with pytest.raises(ValueError, match="gumbel needs sampling='device'"):
        BatchedSelfPlay(lambda leaf: None, 4, n_playout=8, sampling="numpy", gumbel=True)
    with pytest.raises(ValueError, match="exclude each other"):
        BatchedSelfPlay(lambda leaf: None, 4, n_playout=8, gumbel={"max_considered": 4}, root_exploration={"eps": 0.25})
