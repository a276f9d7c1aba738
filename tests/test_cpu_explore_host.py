"""CPU: the collector's side of root exploration (``collect --root-noise-eps ...``): what the command line refuses, what it hands
to ``CollectPipeline``, and the log fields, computed here from fabricated counters."""
import pytest


def _parse(argv):
    from chinesechesszero_amd.collect import parse_args
    return parse_args(argv)


def test_the_feature_is_off_without_root_noise_eps():
    assert _parse([]).root_exploration is None
    assert _parse(["--boards", "64", "--playout-cap-fast", "50", "--playout-cap-prob", "0.25"]).root_exploration is None


@pytest.mark.parametrize("argv", [["--root-noise-alpha", "0.3"], ["--forced-playouts", "2"], ["--no-target-pruning"],
                                  ["--forced-playouts", "0", "--no-target-pruning"]])
def test_the_other_flags_are_refused_without_it(argv, capsys):
    with pytest.raises(SystemExit):
        _parse(argv)
    err = capsys.readouterr().err
    assert "without --root-noise-eps" in err and argv[0] in err


@pytest.mark.parametrize("argv", [["--root-noise-eps", "1.5"], ["--root-noise-eps", "-0.1"], ["--root-noise-eps", "0.25", "--root-noise-alpha", "0"],
                                  ["--root-noise-eps", "0.25", "--forced-playouts", "-1"], ["--root-noise-eps", "0.25", "--boards", "1"]])
def test_values_out_of_range_are_refused(argv):
    with pytest.raises(SystemExit):
        _parse(argv)


def test_defaults_and_what_reaches_the_pipeline():
    from chinesechesszero_amd import collect
    a = _parse(["--root-noise-eps", "0.25"])
    assert a.root_exploration == {"eps": 0.25, "alpha": None, "forced_k": 2.0, "prune_targets": True}      # alpha None: the sampler's
    a = _parse(["--root-noise-eps", "0.1", "--root-noise-alpha", "0.03", "--forced-playouts", "0", "--no-target-pruning"])
    assert a.root_exploration == {"eps": 0.1, "alpha": 0.03, "forced_k": 0.0, "prune_targets": False}
    with pytest.raises(ValueError, match="batched path"):
        collect.CollectPipeline(n_boards=1, root_exploration={"eps": 0.25})


def test_log_fields_from_fabricated_counters():
    from chinesechesszero_amd.collect import format_exploration
    from chinesechesszero_amd.options import OPTIONS, SearchOptions
    x = {"explored_moves": 200, "forced_selections": 1500, "visits_pruned": 12000, "children_pruned": 3100}
    line = format_exploration(x, 80000)
    assert line == ", explored moves 200, forced selections per move 7.50, pruned share of visits 0.1500 (3100 children dropped)"
    zero = format_exploration({"explored_moves": 0, "forced_selections": 0, "visits_pruned": 0, "children_pruned": 0}, 0)
    assert "forced selections per move n/a" in zero and "pruned share of visits n/a" in zero

    class _Engine:
        def exploration_stats(self):
            return x

        def stats(self):
            return {"sims": 80000}

    assert OPTIONS["root_exploration"].log(_Engine()) == line == SearchOptions(8, root_exploration={"eps": 0.25}).log_line(_Engine())
    assert SearchOptions(8, root_exploration=None).log_line(_Engine()) == ""          # off: the log line is what it was


def test_selfplay_refuses_host_sampling_before_it_builds_an_engine():
    from chinesechesszero_amd.selfplay import BatchedSelfPlay
    with pytest.raises(ValueError, match="root_exploration needs sampling='device'"):
        BatchedSelfPlay(lambda leaf: None, 4, n_playout=8, sampling="numpy", root_exploration={"eps": 0.25})
