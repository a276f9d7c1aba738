"""CPU: the engine options of the front ends (``chinesechesszero_amd/options.py``) -- which ``SelfPlayEngine.set_*`` calls every
front end makes for every legal combination of the options it allows, what is refused before an engine exists, and the reports.

The recording stand-in is test_cpu_frontend_sequences.py's, extended so that each setter records ``("set_x", kwargs)`` and every
construction is counted. The expected calls (``EXPECTED``) are literals: they were taken from the commit BEFORE ``options.py``
existed, by running this file's recorder (``_setter_calls``) on that commit's front ends, and pasted here. Per front end the calls
and their arguments are those; the order is that commit's too, except for ``Arena`` and ``BatchedMatch``, which called solver,
search, early stop(, resign) and now call them in ``BatchedSelfPlay``'s order (resign, root exploration, gumbel, solver, search,
early stop): for these two the comparison is of the sorted lists."""
import numpy as np
import pytest
import torch

from test_cpu_frontend_sequences import Net, SeqEngine

SETTERS = ("set_resign", "set_root_exploration", "set_gumbel", "set_solver", "set_search", "set_early_stop")


class OptEngine(SeqEngine):
    built = 0

    def __init__(self, *a, **kw):
        OptEngine.built += 1
        super().__init__(*a, **kw)
        self.setters = []

    def set_scouts(self, n):
        self._rec("set_scouts")

    def set_solver(self, enabled=True):
        self.setters.append(("set_solver", {"enabled": enabled}))


for _name in SETTERS:
    if _name != "set_solver":
        setattr(OptEngine, _name, (lambda name: lambda self, **kw: self.setters.append((name, kw)))(_name))

RESIGN = {"threshold": -0.9, "consecutive": 3, "min_ply": 10, "p_playon": 0.25}
RESIGN_MATCH = {"threshold": -0.9, "consecutive": 3}          # (a match plays no game on)
ROOT = {"eps": 0.25, "forced_k": 2.0}
GUMBEL = {"max_considered": 4}
SEARCH = {"fpu_mode": 1, "fpu_value": 0.3, "fpu_root_mode": 1, "fpu_root_value": 0.3, "c_base": 19652.0, "c_factor": 0.0}
STOP = {"single_reply": False, "gap_factor": 1.0, "kld_interval": 0, "min_gain": 0.0, "min_sims": 0}

# every option alone (resign and gumbel in both their forms), the two largest legal sets (gumbel excludes root exploration and the
# early stop), none
CASES = {
    "none": {},
    "resign": {"resign": RESIGN}, "resign_scalar": {"resign": -0.8}, "root_exploration": {"root_exploration": ROOT},
    "gumbel": {"gumbel": GUMBEL}, "gumbel_true": {"gumbel": True}, "solver": {"solver": True}, "search": {"search": SEARCH},
    "early_stop": {"early_stop": STOP},
    "all_but_gumbel": {"resign": RESIGN, "root_exploration": ROOT, "solver": True, "search": SEARCH, "early_stop": STOP},
    "all_with_gumbel": {"resign": RESIGN, "gumbel": GUMBEL, "solver": True, "search": SEARCH},
}
ALLOWS = {"selfplay": SETTERS, "collect": SETTERS, "arena": ("set_resign", "set_solver", "set_search", "set_early_stop"),
          "match": ("set_solver", "set_search", "set_early_stop"), "analysis": ("set_solver", "set_search", "set_early_stop"),
          "mcts": ("set_solver", "set_search")}
REORDERED = ("arena", "match")


def dense(leaf):
    return torch.zeros((leaf.shape[0], 2086)), torch.zeros(leaf.shape[0])


@pytest.fixture
def fake(monkeypatch, tmp_path):
    """Every front end's engine is the stand-in; ``build(front_end, **options) -> engine`` (None: none was made)."""
    from chinesechesszero_amd import arena, collect, engine, match, mcts, selfplay
    for mod in (engine, match, mcts, selfplay):
        monkeypatch.setattr(mod, "SelfPlayEngine", OptEngine)
    monkeypatch.setattr(arena, "make_openings", lambda n, plies, seed=0, device=0: (np.zeros((n, 90), np.uint8), np.ones(n, np.uint8), np.zeros(n, np.int32)))
    OptEngine.built = 0
    dirs = iter(range(1000))

    def build(front_end, **opts):
        if front_end == "selfplay":
            return selfplay.BatchedSelfPlay(dense, 4, n_playout=8, **opts).engine
        if front_end == "arena":
            if opts.get("resign") is RESIGN:
                opts = dict(opts, resign=RESIGN_MATCH)
            return arena.Arena(Net().ev, Net().ev, 2, n_playout=8, eval_cache_log2=12, **opts).engine
        if front_end == "match":
            return match.BatchedMatch(dense, dense, 4, n_playout=8, **opts).engine
        if front_end == "analysis":
            from chinesechesszero_amd.analyse import BatchedAnalysis
            return BatchedAnalysis(dense, 4, n_playout=8, **opts).engine
        if front_end == "mcts":
            return mcts.MCTS(lambda board: None, n_playout=8, scouts=0, **opts)._ensure_engine()
        pipe = collect.CollectPipeline(n_boards=4, n_playout=8, data_dir=str(tmp_path / f"d{next(dirs)}"), **opts)
        pipe.load_model = lambda: None
        pipe.policy_value_net = type("N", (), {"evaluate_leaves_logits": staticmethod(dense)})()
        pipe.collect_batched(0)
        pipe.sink.close()
        return pipe.selfplay.engine
    return build


def _setter_calls(build, front_end, case):
    opts = {k: v for k, v in CASES[case].items() if "set_" + k in ALLOWS[front_end]}
    return build(front_end, **opts).setters


_R, _RS = ("set_resign", RESIGN), ("set_resign", {"threshold": -0.8})
_RM, _RMS = ("set_resign", dict(RESIGN_MATCH, p_playon=0.0)), ("set_resign", {"threshold": -0.8, "p_playon": 0.0})
_X, _G, _GT = ("set_root_exploration", ROOT), ("set_gumbel", dict(GUMBEL, n_sims=8)), ("set_gumbel", {"n_sims": 8})
_S, _P, _E = ("set_solver", {"enabled": True}), ("set_search", SEARCH), ("set_early_stop", STOP)
_SELFPLAY = {"none": [], "resign": [_R], "resign_scalar": [_RS], "root_exploration": [_X], "gumbel": [_G], "gumbel_true": [_GT], "solver": [_S],
             "search": [_P], "early_stop": [_E], "all_but_gumbel": [_R, _X, _S, _P, _E], "all_with_gumbel": [_R, _G, _S, _P]}
_THREE = {"none": [], "resign": [], "resign_scalar": [], "root_exploration": [], "gumbel": [], "gumbel_true": [], "solver": [_S], "search": [_P],
          "early_stop": [_E], "all_but_gumbel": [_S, _P, _E], "all_with_gumbel": [_S, _P]}
EXPECTED = {
    "selfplay": _SELFPLAY,
    "collect": _SELFPLAY,
    "arena": dict(_THREE, resign=[_RM], resign_scalar=[_RMS], all_but_gumbel=[_S, _P, _E, _RM], all_with_gumbel=[_S, _P, _RM]),
    "match": _THREE,
    "analysis": dict(_THREE, all_but_gumbel=[_P, _E, _S], all_with_gumbel=[_P, _S]),     # (the solver after the self-play front end's own)
    "mcts": dict(_THREE, early_stop=[], all_but_gumbel=[_S, _P]),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("front_end", list(ALLOWS))
def test_setter_calls_are_those_of_the_commit_before(fake, front_end, case):
    got, want = _setter_calls(fake, front_end, case), EXPECTED[front_end][case]
    key = (lambda calls: sorted(calls, key=lambda c: c[0])) if front_end in REORDERED else list
    assert key(got) == key(want)
    if front_end in REORDERED:          # the one order there is now
        assert [c[0] for c in got] == [s for s in SETTERS if s in [c[0] for c in got]]
    if case == "none":
        assert got == []


# ---------------------------------------------------------------------------------------------------------------- refusals
REFUSED = [   # (front end, its keywords, substring of the message)
    ("selfplay", {"gumbel": True, "root_exploration": ROOT}, "exclude each other"),
    ("collect", {"gumbel": True, "root_exploration": ROOT}, "exclude each other"),
    ("selfplay", {"gumbel": True, "early_stop": STOP}, "exclude each other"),
    ("collect", {"gumbel": True, "early_stop": STOP}, "exclude each other"),
    ("selfplay", {"sampling": "numpy", "resign": -0.9}, "resign needs sampling='device'"),
    ("selfplay", {"sampling": "numpy", "root_exploration": ROOT}, "root_exploration needs sampling='device'"),
    ("selfplay", {"sampling": "numpy", "gumbel": True}, "gumbel needs sampling='device'"),
    ("analysis", {"width": 4, "solver": True}, "width > 1"),
    ("analysis", {"width": 4, "search": SEARCH}, "width > 1"),
    ("analysis", {"width": 4, "early_stop": STOP}, "width > 1"),
    ("mcts", {"width": 4, "solver": True}, "width > 1"),
    ("mcts", {"width": 4, "search": SEARCH}, "width > 1"),
    ("mcts", {"width": 4, "scouts": 4}, "scouts"),
    ("mcts", {"search": SEARCH, "scouts": 4}, "scouts"),
    ("arena", {"resign": {"threshold": -0.9, "p_playon": 0.1}}, "p_playon"),
] + [("collect", {"n_boards": 1, k: v}, "batched path") for k, v in (("resign", -0.9), ("root_exploration", ROOT), ("gumbel", True), ("solver", True),
                                                                      ("early_stop", STOP))]


@pytest.mark.parametrize("front_end,kw,text", REFUSED, ids=[f"{f}-{'-'.join(k)}" for f, k, _ in REFUSED])
def test_refusals_come_before_an_engine_is_built(fake, tmp_path, front_end, kw, text):
    from chinesechesszero_amd import collect, mcts
    with pytest.raises(ValueError, match=text):
        if front_end == "collect":
            collect.CollectPipeline(**dict({"n_boards": 4, "n_playout": 8, "data_dir": str(tmp_path / "r")}, **kw))
        elif front_end == "mcts":
            mcts.MCTS(Net().ev, n_playout=8, **kw)
        else:
            fake(front_end, **kw)
    assert OptEngine.built == 0


ARGV = {"gumbel": ["--gumbel"], "root_exploration": ["--root-noise-eps", "0.25"], "early_stop": ["--stop-gap"], "resign": ["--resign-threshold", "-0.9"],
        "solver": ["--solver"]}


@pytest.mark.parametrize("pair", [("gumbel", "root_exploration"), ("gumbel", "early_stop")])
def test_an_illegal_pair_is_refused_by_one_rule_in_all_three_places(fake, tmp_path, capsys, pair):
    """``BatchedSelfPlay``, ``CollectPipeline`` and the collector's parser: the message is ``SearchOptions``' own in all three."""
    from chinesechesszero_amd import collect
    from chinesechesszero_amd.options import SearchOptions
    kw = {"gumbel": True, "root_exploration": ROOT, "early_stop": STOP}
    kw = {k: kw[k] for k in pair}
    with pytest.raises(ValueError) as rule:
        SearchOptions(8, **kw)
    assert "exclude each other" in str(rule.value)
    for make in (lambda: fake("selfplay", **kw), lambda: collect.CollectPipeline(n_boards=4, n_playout=8, data_dir=str(tmp_path / "p"), **kw)):
        with pytest.raises(ValueError) as exc:
            make()
        assert str(exc.value) == str(rule.value)
    with pytest.raises(SystemExit):
        collect.parse_args(["--boards", "64"] + ARGV[pair[0]] + ARGV[pair[1]])
    assert str(rule.value) in capsys.readouterr().err
    assert OptEngine.built == 0


@pytest.mark.parametrize("name", ["gumbel", "root_exploration", "early_stop", "resign", "solver"])
def test_the_parser_refuses_the_one_game_path_as_the_pipeline_does(capsys, tmp_path, name):
    from chinesechesszero_amd import collect
    with pytest.raises(SystemExit):
        collect.parse_args(["--boards", "1"] + ARGV[name])
    err = capsys.readouterr().err
    with pytest.raises(ValueError, match="batched path") as exc:
        collect.CollectPipeline(n_boards=1, data_dir=str(tmp_path / "q"), **{name: {"gumbel": True, "root_exploration": ROOT, "early_stop": STOP,
                                                                                  "resign": -0.9, "solver": True}[name]})
    assert str(exc.value) in err
    assert collect.parse_args(["--boards", "1", "--fpu-reduction", "0.3"]).search is not None      # the one-game loop takes these


def test_normalisation_and_public_attributes(fake):
    from chinesechesszero_amd.options import SearchOptions
    o = SearchOptions(64, resign=-0.8, root_exploration=None, gumbel=True, solver=1, search=SEARCH, early_stop=False)
    assert o.keywords() == {"resign": {"threshold": -0.8}, "root_exploration": None, "gumbel": {"n_sims": 64}, "solver": True, "search": SEARCH,
                            "early_stop": None}
    assert o.search is not SEARCH                                  # dicts are copied
    assert SearchOptions(64, gumbel={"n_sims": 32}).gumbel == {"n_sims": 32}
    off = SearchOptions(64, solver=False, search=None)
    assert off.keywords() == {"solver": False, "search": None} and off.on == {} and not hasattr(off, "resign")
    with pytest.raises(TypeError, match="no such search option"):
        SearchOptions(64, pondering=True)
    from chinesechesszero_amd import selfplay
    sp = selfplay.BatchedSelfPlay(dense, 4, n_playout=8, **CASES["all_with_gumbel"])
    assert (sp.resign, sp.root_exploration, sp.gumbel, sp.solver, sp.search_cfg, sp.early_stop) == (RESIGN, None, dict(GUMBEL, n_sims=8), True, SEARCH, None)
    sp = selfplay.BatchedSelfPlay(dense, 4, n_playout=8)
    assert (sp.resign, sp.root_exploration, sp.gumbel, sp.solver, sp.search_cfg, sp.early_stop, sp.playout_cap) == (None, None, None, False, None, None, None)


# ---------------------------------------------------------------------------------------------------------------- reports
class StatsEngine:
    """Fabricated counters: those of test_cpu_gumbel_cli.py and test_cpu_explore_host.py, and the like for the other options."""

    def resign_stats(self):
        return {"resigned_games": 12, "playon_games": 4, "playon_won": 1, "playon_plies_after": 90}

    def exploration_stats(self):
        return {"explored_moves": 200, "forced_selections": 1500, "visits_pruned": 12000, "children_pruned": 3100}

    def gumbel_stats(self):
        return {"gumbel_moves": 400, "considered_sum": 6100, "offvisit_moves": 30}

    def solver_stats(self):
        return {"nodes_proven": 7, "proven_stops": 5, "roots_proven": 1}

    def search_settings(self):
        return dict(SEARCH, enabled=True)

    def early_stop_stats(self):
        return {"single_reply": 3, "visit_gap": 20, "kld_gain": 1, "sims_saved": 900, "evaluations": 50}

    def stats(self):
        return {"sims": 80000, "moves": 1000, "sum_depth": 280000}


LOG = {"resign": ", resigned 12, play-on 4 (false positives 0.250, mean plies after 22.5)",
       "root_exploration": ", explored moves 200, forced selections per move 7.50, pruned share of visits 0.1500 (3100 children dropped)",
       "gumbel": ", gumbel moves 400, mean considered 15.25, off-visit share 0.0750",
       "solver": ", nodes proven 7, simulations ended at a proven node 5, roots proven 1",
       "search": ", fpu reduction 0.3 (root reduction 0.3), c_puct constant, mean leaf depth 3.50",
       "early_stop": ", early stops 3 single reply / 20 gap / 1 kld, 80.0 simulations per move"}


def test_log_line_and_report_from_fabricated_counters():
    from chinesechesszero_amd.options import OPTIONS, SearchOptions
    e = StatsEngine()
    assert list(OPTIONS) == list(LOG)
    for name, o in OPTIONS.items():
        assert o.log(e) == LOG[name]
    assert SearchOptions(8).log_line(object()) == "" and SearchOptions(8, solver=False, resign=None).report(object()) == {}      # off: no engine call
    o = SearchOptions(8, **CASES["all_but_gumbel"])
    assert o.log_line(e) == LOG["resign"] + LOG["root_exploration"] + LOG["solver"] + LOG["search"] + LOG["early_stop"]
    stop = {"single_reply": 3, "visit_gap": 20, "kld_gain": 1, "sims_saved": 900, "mean_sims_per_move": 80.0}
    assert o.report(e) == {"solver": e.solver_stats(), "search": e.search_settings(), "mean_leaf_depth": 3.5, "early_stop": stop}
    assert SearchOptions(8, gumbel=True, search=SEARCH).log_line(e) == LOG["gumbel"] + LOG["search"]


def test_the_move_loop_and_the_proven_moves():
    from chinesechesszero_amd.options import proven_moves, search_move
    from chinesechesszero_amd.stopcfg import POLL_EVERY, StopPoll

    class E:
        left = 0

        def select_leaves(self):
            return "leaf0"

        def searching(self):
            return self.left

        def proof_moves(self):
            return np.array([5, -1, 9, 11], np.int32)

        def game_status(self):
            return {"over": np.array([0, 0, 1, 0])}
    e, seen = E(), []
    step = lambda leaf, last: seen.append((leaf, last)) or f"leaf{len(seen)}"
    search_move(e, 3, step, StopPoll(e, None))
    assert seen == [("leaf0", False), ("leaf1", False), ("leaf2", True)]
    del seen[:]
    search_move(e, 3 * POLL_EVERY, step, StopPoll(e, STOP))          # asked at step POLL_EVERY: nothing searches any more
    assert len(seen) == POLL_EVERY == 16 and not seen[-1][1]
    assert proven_moves(e, False) == (None, 0)
    forced, n = proven_moves(e, True)
    assert forced.tolist() == [5, -1, -1, 11] and n == 2
    forced, n = proven_moves(e, True, over=np.array([1, 0, 0, 0]))
    assert forced.tolist() == [-1, -1, 9, 11] and n == 2
