"""The engine options of the search front ends -- resign, root exploration, the Gumbel root, the MCTS-solver, the search parameters, the
early stop -- each described ONCE (:data:`OPTIONS`), and what a front end does with them (:class:`SearchOptions`): refuse what excludes
what, call the setters in one order, report. Also the command line of resign / root exploration / Gumbel in the shape of ``searchcfg`` /
``stopcfg`` (which keep the search parameters' and the early stop's), and the move of the arg-max front ends. No GPU here. Adding an
option: ``ccz_set_x`` on the C side (which refuses what it excludes), the setter in ``engine.py``, ONE entry in ``OPTIONS`` (and a rule
in ``SearchOptions.__init__`` if it excludes another), the keyword on the front ends that allow it. ``RECORD_OPTIONS`` holds, in the same
shape, what decides how a recorded game is trained on (policy surprise weighting), ``INPUT_OPTIONS`` what decides the evaluator's input (leaf
history planes), ``MOVE_OPTIONS`` what decides which move is played after the search (the LCB move); ``SearchOptions`` handles the four tables alike."""
from __future__ import annotations

from collections import namedtuple

from .searchcfg import mean_leaf_depth
from .stopcfg import stop_report

RESIGN_MOVES, RESIGN_MIN_PLY, RESIGN_PLAYON, FORCED_PLAYOUTS = 2, 30, 0.1, 2.0
GUMBEL_CONSIDERED, GUMBEL_C_VISIT, GUMBEL_C_SCALE = 16, 50.0, 1.0
SURPRISE_WEIGHT, SURPRISE_CAP = 0.5, 8.0
# The LCB move's defaults are KataGo's published lcbStdevs = 5.0 and minVisitPropForLCB = 0.15, with at least two visits (below that a child
# has no sample variance). They are conventions taken from that engine, NOT measurements of this one: no trained weights exist here to measure
# strength with (arena --a X --b X --lcb --lcb-side a is the experiment).
LCB_STDEVS, LCB_MIN_VISIT_RATIO, LCB_MIN_VISITS = 5.0, 0.15, 2


# ---------------------------------------------------------------------- fragments of the collector's periodic log line
def format_resign(r: dict) -> str:
    """``r`` = ``SelfPlayEngine.resign_stats()``: games resigned, the false-positive rate ``playon_won / playon_games`` of the games
    played on, and their mean plies after the fire ply."""
    n = r["playon_games"]
    fp = f"{r['playon_won'] / n:.3f}" if n else "n/a"
    after = f"{r['playon_plies_after'] / n:.1f}" if n else "n/a"
    return f", resigned {r['resigned_games']}, play-on {n} (false positives {fp}, mean plies after {after})"


def format_exploration(x: dict, sims: int) -> str:
    """``x`` = ``SelfPlayEngine.exploration_stats()``, ``sims`` = the simulations backed up so far (``stats()['sims']``, fast moves
    included): explored moves, forced selections per explored move, and the visits pruned from the policy targets as a share of
    the simulations run."""
    n = x["explored_moves"]
    forced = f"{x['forced_selections'] / n:.2f}" if n else "n/a"
    share = f"{x['visits_pruned'] / sims:.4f}" if sims else "n/a"
    return f", explored moves {n}, forced selections per move {forced}, pruned share of visits {share} ({x['children_pruned']} children dropped)"


def format_gumbel(x: dict) -> str:
    """``x`` = ``SelfPlayEngine.gumbel_stats()``: the moves played by the Gumbel root rule, the mean number of moves considered, and the
    share of them whose played move was not the most visited one."""
    n = x["gumbel_moves"]
    m = f"{x['considered_sum'] / n:.2f}" if n else "n/a"
    off = f"{x['offvisit_moves'] / n:.4f}" if n else "n/a"
    return f", gumbel moves {n}, mean considered {m}, off-visit share {off}"


def surprise_report(x: dict) -> dict:
    """``x`` = ``SelfPlayEngine.surprise_stats()`` and what the log line says of it: the mean surprise per policy-target ply and the
    share of those plies whose weight the harvest clipped at the cap (None before the first)."""
    n = x["target_plies"]
    return dict(x, mean_surprise=x["surprise_sum"] / n if n else None, clipped_share=x["weights_clipped"] / n if n else None)


def format_surprise(x: dict) -> str:
    r = surprise_report(x)
    mean = f"{r['mean_surprise']:.4f}" if r["target_plies"] else "n/a"
    share = f"{r['clipped_share']:.4f}" if r["target_plies"] else "n/a"
    return f", surprise per target ply {mean} over {r['target_plies']}, weights clipped {share}"


def format_search(cfg: dict, stats: dict) -> str:
    """``cfg`` = ``SelfPlayEngine.search_settings()``, ``stats`` = ``SelfPlayEngine.stats()``: the urgency of the tree and of the root,
    the growth of c_puct, and the mean depth of the leaves selected so far."""
    def fpu(mode, value):
        return {0: "off", 1: f"reduction {value:g}", 2: f"absolute {value:g}"}[int(mode)]
    growth = f"base {cfg['c_base']:g} factor {cfg['c_factor']:g}" if cfg["c_factor"] else "constant"
    return (f", fpu {fpu(cfg['fpu_mode'], cfg['fpu_value'])} (root {fpu(cfg['fpu_root_mode'], cfg['fpu_root_value'])}), c_puct {growth}, "
            f"mean leaf depth {mean_leaf_depth(stats):.2f}")


def engine_stop_report(e) -> dict:
    """:func:`stopcfg.stop_report` of an engine's counters so far (syncs)."""
    st = e.stats()
    return stop_report(e.early_stop_stats(), st["moves"], st["sims"])


# ``setter``: the SelfPlayEngine method that takes the option's dict; ``what``: its name in messages; ``log(engine)``: its fragment of the log
# line; ``report(engine)``: its entries in the JSON of Arena.result / BatchedAnalysis.summary (None: none); ``of_scalar``: the dict of a value
# that is not one; ``device_only``: why it needs sampling='device' (None: it does not); ``one_game``: it also runs in the collector's one-game loop
# ``setter_args(cfg)``: the setter's keywords when they are not the option's dict itself (None: they are)
Option = namedtuple("Option", "setter what log report of_scalar device_only one_game setter_args", defaults=(None, dict, None, False, None))
SOLVER_LOG = ", nodes proven {nodes_proven}, simulations ended at a proven node {proven_stops}, roots proven {roots_proven}"
STOP_LOG = ", early stops {single_reply} single reply / {visit_gap} gap / {kld_gain} kld, {mean_sims_per_move} simulations per move"

# (in the order SearchOptions.apply calls the setters and log_line joins the fragments)
OPTIONS = {
    "resign": Option("set_resign", "resignation", lambda e: format_resign(e.resign_stats()), of_scalar=lambda x: {"threshold": float(x)},
                     device_only="with host sampling every move is forced, and a forced board never resigns"),
    "root_exploration": Option("set_root_exploration", "root exploration", lambda e: format_exploration(e.exploration_stats(), e.stats()["sims"]),
                               device_only="the host sampler mixes Dirichlet noise into pi after the search"),
    "gumbel": Option("set_gumbel", "the Gumbel root search", lambda e: format_gumbel(e.gumbel_stats()), of_scalar=lambda x: {},
                     device_only="the rule plays the move itself, a host-sampled move would be forced over it"),
    "solver": Option("set_solver", "the solver option of the collector", lambda e: SOLVER_LOG.format(**e.solver_stats()),
                     report=lambda e: {"solver": e.solver_stats()}, of_scalar=lambda x: {"enabled": True}),
    "search": Option("set_search", "the search parameters", lambda e: format_search(e.search_settings(), e.stats()),
                     report=lambda e: {"search": e.search_settings(), "mean_leaf_depth": mean_leaf_depth(e.stats())}, one_game=True),
    "early_stop": Option("set_early_stop", "the early stop of the collector", lambda e: STOP_LOG.format(**engine_stop_report(e)),
                         report=lambda e: {"early_stop": engine_stop_report(e)}),
}


# What decides how a recorded game is trained on, not how it is searched: the same description, applied and reported after OPTIONS. Only the
# front ends that record games (BatchedSelfPlay, the collector) take these keywords.
RECORD_OPTIONS = {
    "surprise": Option("set_surprise", "policy surprise weighting", lambda e: format_surprise(e.surprise_stats()),
                       report=lambda e: {"surprise": surprise_report(e.surprise_stats())},
                       of_scalar=lambda x: {} if x is True else {"alpha": float(x)}),
}


def history_report(stats: dict) -> dict:
    """``stats`` = ``SelfPlayEngine.stats()``: the setting, and the share of the probed leaves the evaluation cache answered (from the table
    or from another board's row of the same step; None without a cache) -- with history planes a transposition is another input and misses."""
    n = stats["cache_probes"]
    return {"leaf_history": True, "cache_hit_share": (stats["cache_hits"] + stats["cache_shared_rows"]) / n if n else None}


def format_history(stats: dict) -> str:
    share = history_report(stats)["cache_hit_share"]
    return ", leaf history planes on, cache hit share " + ("n/a" if share is None else f"{share:.4f}")


# What decides the evaluator's INPUT: applied and reported after the two tables above. The evaluator of a front end that turns it on must read
# all 17 plane groups (``boundary.need_history``).
INPUT_OPTIONS = {
    "leaf_history": Option("set_leaf_history", "leaf history planes", lambda e: format_history(e.stats()),
                           report=lambda e: history_report(e.stats()), of_scalar=lambda x: {"enabled": True}),
}


def format_lcb(c: dict) -> str:
    share = f"{c['differed'] / c['moves']:.4f}" if c["moves"] else "n/a"
    return f", lcb moves {c['moves']}, off the most visited move {c['differed']} (share {share})"


def _lcb_of_scalar(x):
    return {"z": LCB_STDEVS if x is True else float(x), "min_visit_ratio": LCB_MIN_VISIT_RATIO, "min_visits": LCB_MIN_VISITS}


# What decides which move is PLAYED after the search (the search itself is untouched): applied and reported after the tables above, before the
# input options. The engine's side of it is the value spread S per node (``set_value_stats``); the rule's numbers stay on the host and go to
# ``SelfPlayEngine.lcb_moves`` at every move (:func:`lcb_moves`). Its log and report take the front end's own counters
# (``SearchOptions.lcb_counts``: moves played by the rule, and how many of them were not the most visited move), not the engine.
MOVE_OPTIONS = {
    "lcb": Option("set_value_stats", "the LCB move", lambda c: format_lcb(c), report=lambda c: {"lcb": dict(c)},
                  of_scalar=_lcb_of_scalar, device_only="with host sampling every move is drawn on the host, and the LCB move is a forced one",
                  one_game=True, setter_args=lambda cfg: {"enabled": True}),
}
ALL_OPTIONS = {**OPTIONS, **RECORD_OPTIONS, **MOVE_OPTIONS, **INPUT_OPTIONS}


class SearchOptions:
    """The options of ONE front end, from the keywords it was given (``resign=..., solver=..., ...``: the options it allows). None / False: off;
    a dict is copied, another value goes through ``of_scalar``; ``gumbel`` searches ``n_playout`` (the front end's simulations per move) unless
    it says otherwise. ``sampling``: ``BatchedSelfPlay``'s; ``batched``: False on the collector's one-game path; ``width``: ``wide.WideSearch``'s.
    Raises ValueError for every combination that is refused before an engine exists (``csrc/cczero.hip`` refuses them again, and more: it stays the
    authority). Then every allowed option is an attribute: its dict, None when off (``solver``: a bool); ``on``: those that are on, in OPTIONS' order."""

    def __init__(self, n_playout=None, sampling: str = "device", batched: bool = True, width: int = 1, mate_search=None, **given):
        # the mate search is a query before the move, not an engine setting: it has no setter and no entry in the tables (``keywords``
        # and ``on`` are what they are without it); its dict, its counters, its report and its log fragment live next to them
        self.mate_search = mate_search_of(mate_search)
        self.mate_counts = {"boards": 0, "mates": 0, "nodes": 0}   # what :func:`mate_moves` is handed as ``counts``
        self.on = on = {}
        for name, o in ALL_OPTIONS.items():
            if name in given:
                cfg = given.pop(name)
                if cfg is not None and cfg is not False and (cfg or name != "solver"):
                    on[name] = dict(cfg) if isinstance(cfg, dict) else o.of_scalar(cfg)
                setattr(self, name, on.get(name) if name != "solver" else name in on)
        if given:
            raise TypeError(f"no such search option: {', '.join(given)}")
        if "gumbel" in on:
            on["gumbel"].setdefault("n_sims", n_playout)
        for name in on:
            if sampling != "device" and ALL_OPTIONS[name].device_only:
                raise ValueError(f"{name} needs sampling='device': {ALL_OPTIONS[name].device_only}")
            if not batched and not ALL_OPTIONS[name].one_game:
                raise ValueError(f"{ALL_OPTIONS[name].what} runs on the batched path: n_boards (--boards) must be > 1")
        if "gumbel" in on and "root_exploration" in on:
            raise ValueError("gumbel and root_exploration (--gumbel, --root-noise-eps) exclude each other: the Gumbel draw is the root's exploration")
        if "gumbel" in on and "early_stop" in on:
            raise ValueError("the early stop (--stop-*) and the Gumbel root search (--gumbel) exclude each other: sequential halving plans the whole budget")
        if int(width) > 1 and any(name in on for name in ("solver", "search", "early_stop")):
            raise ValueError("width > 1 (the wide search) excludes scouts, the solver, the search parameters and the early stop")
        if "lcb" in on:
            on["lcb"] = make_lcb(**{"z": True, **on["lcb"]})   # (a dict may leave the defaults out; the numbers are checked here)
            self.lcb = on["lcb"]
            self.lcb_counts = {"moves": 0, "differed": 0}   # what :func:`lcb_moves` is handed as ``counts``
        if "lcb" in on and "gumbel" in on:
            raise ValueError("lcb and gumbel (--lcb, --gumbel) exclude each other: the Gumbel rule plays its own move")
        if "lcb" in on and int(width) > 1:
            raise ValueError("width > 1 (the wide search) excludes lcb: a virtual loss is no value, the spread of a wide search is a follow-up")
        if int(width) > 1 and "leaf_history" in on:
            raise ValueError("width > 1 (the wide search) excludes leaf history planes: a wide step's leaves are not replayed one path each")

    def keywords(self) -> dict:
        """``{keyword: value}`` of every allowed option, on or off, as a front end takes them (and in OPTIONS' order)."""
        return {name: getattr(self, name) for name in ALL_OPTIONS if hasattr(self, name)}

    def apply(self, engine):
        """Call the setters of the options that are on, and no others: resign, root exploration, gumbel, solver, search, early stop, surprise,
        lcb (the value spread), leaf history.
        Every setter writes its own settings block only, so the order decides nothing."""
        for name, cfg in self.on.items():
            o = ALL_OPTIONS[name]
            getattr(engine, o.setter)(**(cfg if o.setter_args is None else o.setter_args(cfg)))

    def report(self, engine) -> dict:
        """The entries of the options that are on in a front end's JSON result (syncs)."""
        out = {k: v for name in self.on if ALL_OPTIONS[name].report
               for k, v in ALL_OPTIONS[name].report(self.lcb_counts if name == "lcb" else engine).items()}
        if self.mate_search is not None:
            out["mate_search"] = mate_report(self.mate_search, self.mate_counts)
        return out

    def log_line(self, engine) -> str:
        """The fragments of the options that are on, for the collector's periodic log line (empty with none on; syncs)."""
        return "".join(ALL_OPTIONS[name].log(self.lcb_counts if name == "lcb" else engine) for name in self.on) + (
            format_mate(self.mate_counts) if self.mate_search is not None else "")


# ---------------------------------------------------------------------- the move of an arg-max front end
def search_move(engine, n_steps: int, step, poll):
    """One move's search of ``Arena`` / ``BatchedMatch``: select, then up to ``n_steps`` times ``step(leaf, last) -> next leaf batch``;
    ``poll`` (:class:`stopcfg.StopPoll`) ends the loop when no board would select any more (no leaf is pending then either)."""
    leaf = engine.select_leaves()
    for i in range(n_steps):
        if poll.done(i):
            break
        leaf = step(leaf, i + 1 == n_steps)


def proven_moves(engine, solver: bool, over=None):
    """``(forced_moves for finish_move, how many of them are proven)`` after a search with the MCTS-solver: the proven move where a running game's
    root is decided, -1 (the sampler's choice) elsewhere; ``(None, 0)`` with the solver off. ``over``: ``game_status()["over"]`` if already read."""
    if not solver:
        return None, 0
    forced = engine.proof_moves()
    forced[(engine.game_status()["over"] if over is None else over) != 0] = -1
    return forced, int((forced >= 0).sum())


def lcb_moves(engine, cfg, forced, over=None, allow=None, counts=None, detail: bool = False):
    """The LCB move of every running game whose entry of ``forced`` is still -1 (a proven move wins over it), after a search with the value
    spread on. ``cfg``: the ``lcb`` dict of :class:`SearchOptions` (None: off, ``forced`` comes back as it is); ``forced``: int32 [B] numpy, or
    None (all -1); ``allow``: bool [B], the boards whose mover plays the LCB move (None: all); ``counts``: the front end's ``{"moves", "differed"}`` (``SearchOptions.lcb_counts``),
    moved in place. Returns ``(forced, how many of the moves filled in are not the arg-max move)``; with ``detail`` also the two bool [B] masks (filled,
    filled and not the arg-max move). One launch, one read of the root children. Syncs."""
    if cfg is None:
        return (forced, 0, None, None) if detail else (forced, 0)
    import numpy as np
    out = engine.lcb_moves(cfg["z"], cfg["min_visit_ratio"], cfg["min_visits"], with_bounds=True)
    moves, child = out["moves"].cpu().numpy(), out["child"].cpu().numpy()
    over = engine.game_status()["over"] if over is None else over
    if forced is None:
        forced = np.full(engine.B, -1, np.int32)
    rc = engine.root_children()
    fill = (forced < 0) & (np.asarray(over) == 0) & (moves >= 0)
    if allow is not None:
        fill &= np.asarray(allow, bool)
    star = rc["visits"].argmax(axis=1)          # the first index of maximal N: the arg-max player's move
    off = fill & (child != star)
    differed = int(off.sum())
    forced[fill] = moves[fill]
    if counts is not None:
        counts["moves"] += int(fill.sum())
        counts["differed"] += differed
    return (forced, differed, fill, off) if detail else (forced, differed)


# ---------------------------------------------------------------------- the mate search (ccz_mate_search): a query before the move
MATE_MAX_PLIES, MATE_MAX_NODES = 31, 131072   # CCZ_MATE_MAX_PLIES / CCZ_MATE_MAX_NODES (no GPU here: tests compare them with _lib's)
MATE_NODES = 2048                            # the budget per board when none is given
_PROOF_WIN = 1                               # CCZ_PROOF_WIN


def make_mate_search(plies, nodes=None):
    """The ``mate_search`` dict of the front ends -- ``{"max_plies", "node_budget"}``, what ``SelfPlayEngine.mate_search`` takes -- or None
    when ``plies`` is None, False or 0. ValueError: what ``ccz_mate_search`` refuses."""
    if plies is None or plies is False or plies == 0:
        if nodes is not None:
            raise ValueError("--mate-nodes without --mate-search: the mate search is off")
        return None
    plies = int(plies)
    if not 1 <= plies <= MATE_MAX_PLIES or plies % 2 == 0:
        raise ValueError(f"--mate-search must be odd and in 1..{MATE_MAX_PLIES} plies (got {plies})")
    nodes = MATE_NODES if nodes is None else int(nodes)
    if not 1 <= nodes <= MATE_MAX_NODES:
        raise ValueError(f"--mate-nodes must be in 1..{MATE_MAX_NODES} (got {nodes})")
    return {"max_plies": plies, "node_budget": nodes}


def mate_search_of(value):
    """The ``mate_search`` keyword of a front end as its dict: None / False / 0 off, a number of plies, or a dict (``max_plies`` /
    ``plies``, ``node_budget`` / ``nodes``), checked by :func:`make_mate_search`."""
    if isinstance(value, dict):
        extra = set(value) - {"max_plies", "plies", "node_budget", "nodes"}
        if extra:
            raise ValueError(f"mate_search: no such setting: {', '.join(sorted(extra))}")
        return make_mate_search(value.get("max_plies", value.get("plies")), value.get("node_budget", value.get("nodes")))
    return make_mate_search(value)


def add_mate_search_args(ap):
    """--mate-search PLIES / --mate-nodes N."""
    ap.add_argument("--mate-search", type=int, default=None, metavar="PLIES", help="before every move, look for a forced mate by consecutive "
                    f"checks of at most PLIES plies (odd, 1..{MATE_MAX_PLIES}) on the device -- no evaluator rows -- and play it where one is "
                    "found; absent = off")
    ap.add_argument("--mate-nodes", type=int, default=None, metavar="N", help=f"... at most N positions per board, 1..{MATE_MAX_NODES} "
                    f"(default {MATE_NODES})")


def mate_search_from_args(ap, a):
    return _from_args(ap, a, "--mate-search", "the mate search is off", ("--mate-nodes",), make_mate_search, a.mate_search, a.mate_nodes)


def mate_report(cfg: dict, counts: dict) -> dict:
    """The settings, the boards searched, the mates found, and the mean nodes per searched board (None before the first)."""
    n = counts["boards"]
    return dict(cfg, boards=n, mates=counts["mates"], mean_nodes=counts["nodes"] / n if n else None)


def format_mate(counts: dict) -> str:
    n = counts["boards"]
    mean = f"{counts['nodes'] / n:.1f}" if n else "n/a"
    return f", mate search boards {n}, mates {counts['mates']}, mean nodes {mean}"


def mate_moves(engine, cfg, forced, over=None, counts=None, detail: bool = False):
    """The mating move of every running game on which ``SelfPlayEngine.mate_search`` finds one (state 1), written into ``forced``: it
    wins over the LCB move and the most visited move (call :func:`lcb_moves` after this), and over the tree's proven move unless the
    tree holds a WIN proof of at most the mate's distance (solver on). ``cfg``: the ``mate_search`` dict of :class:`SearchOptions`
    (None: off, no call is made, ``forced`` comes back as it is); ``forced``: int32 [B] numpy or None (all -1); ``counts``:
    ``SearchOptions.mate_counts``, moved in place. Returns ``(forced, mates written)``; with ``detail`` also the result arrays. Syncs."""
    if cfg is None:
        return (forced, 0, None) if detail else (forced, 0)
    import numpy as np
    res = engine.mate_search(cfg["max_plies"], cfg["node_budget"])
    over = engine.game_status()["over"] if over is None else over
    if forced is None:
        forced = np.full(engine.B, -1, np.int32)
    found = (res["state"] == 1) & (np.asarray(over) == 0) & (res["move"] >= 0)
    if getattr(engine, "solver", False) and found.any():
        rp = engine.root_proof()
        found &= ~((rp["state"] == _PROOF_WIN) & (rp["dist"].astype(np.int64) <= res["dist"]) & (forced >= 0))
    forced[found] = res["move"][found]
    if counts is not None:
        searched = res["state"] != 0
        counts["boards"] += int(searched.sum())
        counts["mates"] += int((res["state"] == 1).sum())
        counts["nodes"] += int(res["nodes"][searched].sum())
    n = int(found.sum())
    return (forced, n, res) if detail else (forced, n)


# ---------------------------------------------------------------------- command lines: make_x (ValueError), add_x_args, x_from_args (ap.error)
def _from_args(ap, a, main: str, off: str, extras, make, *values):
    """``make(*values)``; a ValueError ends in ``ap.error``, and so does an extra flag without the main one (it would silently do nothing)."""
    def is_set(flag):
        v = getattr(a, flag[2:].replace("-", "_"), None)
        return v is not None and v is not False
    if not is_set(main) and any(map(is_set, extras)):
        ap.error(f"{', '.join(filter(is_set, extras))} without {main}: {off}")
    try:
        return make(*values)
    except ValueError as ex:
        ap.error(str(ex))


def make_resign(threshold, moves=None, min_ply=None, playon=None, with_playon: bool = True):
    """The dict of ``SelfPlayEngine.set_resign``'s arguments (None without a threshold); ``with_playon`` False (a match): no ``p_playon``."""
    if threshold is None:
        return None
    cfg = {"threshold": threshold, "consecutive": RESIGN_MOVES if moves is None else moves, "min_ply": RESIGN_MIN_PLY if min_ply is None else min_ply}
    return dict(cfg, p_playon=RESIGN_PLAYON if playon is None else playon) if with_playon else cfg


def add_resign_args(ap, playon: bool, what: str = "resignation"):
    """--resign-threshold / --resign-moves / --resign-min-ply, and with ``playon`` (the collector) --resign-playon."""
    ap.add_argument("--resign-threshold", type=float, default=None, help=f"{what}: the side to move resigns when its root value stayed below this "
                    "(in [-1, 0]); absent = off" + (". Root values are then recorded with every ply (root_values.npy)" if playon else ""))
    ap.add_argument("--resign-moves", type=int, default=None, help=f"... for this many of its full-search moves in a row (default {RESIGN_MOVES})")
    ap.add_argument("--resign-min-ply", type=int, default=None, help=f"... and not before this ply (default {RESIGN_MIN_PLY})")
    if playon:
        ap.add_argument("--resign-playon", type=float, default=None,
                        help=f"fraction of such games played on to measure the false positives (default {RESIGN_PLAYON}, AlphaGo Zero's)")


def resign_from_args(ap, a):
    return _from_args(ap, a, "--resign-threshold", "resignation is off", ("--resign-moves", "--resign-min-ply", "--resign-playon"), make_resign,
                      a.resign_threshold, a.resign_moves, a.resign_min_ply, getattr(a, "resign_playon", None), hasattr(a, "resign_playon"))


def make_root_exploration(eps, alpha=None, forced_playouts=None, prune_targets: bool = True):
    """The dict of ``SelfPlayEngine.set_root_exploration``'s arguments (None without ``eps``). ValueError: what ``ccz_set_root_exploration`` refuses."""
    if eps is None:
        return None
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"--root-noise-eps must be in [0, 1] (got {eps})")
    if alpha is not None and not alpha > 0.0:
        raise ValueError(f"--root-noise-alpha must be > 0 (got {alpha})")
    if forced_playouts is not None and not forced_playouts >= 0.0:
        raise ValueError(f"--forced-playouts must be >= 0 (got {forced_playouts})")
    return {"eps": eps, "alpha": alpha, "forced_k": FORCED_PLAYOUTS if forced_playouts is None else forced_playouts, "prune_targets": bool(prune_targets)}


def add_root_exploration_args(ap):
    """--root-noise-eps / --root-noise-alpha / --forced-playouts / --no-target-pruning."""
    ap.add_argument("--root-noise-eps", type=float, default=None, help="exploration inside the search on full-search moves: weight of the "
                    "Dirichlet noise in the ROOT's priors (in [0, 1]); absent = off (the noise is mixed into pi after the search)")
    ap.add_argument("--root-noise-alpha", type=float, default=None, help="... its Dirichlet alpha (default: the sampler's)")
    ap.add_argument("--forced-playouts", type=float, default=None, help=f"... forced playouts: a root child is searched until N >= sqrt(k P' S) "
                    f"(default k = {FORCED_PLAYOUTS}, KataGo's; 0 = none)")
    ap.add_argument("--no-target-pruning", action="store_true", default=False, help="... keep the forced visits in the recorded policy targets")


def root_exploration_from_args(ap, a):
    return _from_args(ap, a, "--root-noise-eps", "root exploration is off", ("--root-noise-alpha", "--forced-playouts", "--no-target-pruning"),
                      make_root_exploration, a.root_noise_eps, a.root_noise_alpha, a.forced_playouts, not a.no_target_pruning)


def make_gumbel(on, n_sims, considered=None, c_visit=None, c_scale=None):
    """The dict of ``SelfPlayEngine.set_gumbel``'s arguments (None when not ``on``). ValueError: what ``ccz_set_gumbel`` would refuse."""
    if not on:
        return None
    if considered is not None and not 2 <= considered <= 128:
        raise ValueError(f"--gumbel-considered must be in 2..128 (got {considered})")
    for name, v in (("--gumbel-c-visit", c_visit), ("--gumbel-c-scale", c_scale)):
        if v is not None and not 0.0 <= v < float("inf"):
            raise ValueError(f"{name} must be finite and >= 0 (got {v})")
    if n_sims < 1:
        raise ValueError(f"--gumbel needs --playout >= 1 (got {n_sims})")
    return {"n_sims": n_sims, "max_considered": GUMBEL_CONSIDERED if considered is None else considered,
            "c_visit": GUMBEL_C_VISIT if c_visit is None else c_visit, "c_scale": GUMBEL_C_SCALE if c_scale is None else c_scale}


def add_gumbel_args(ap):
    """--gumbel / --gumbel-considered / --gumbel-c-visit / --gumbel-c-scale."""
    ap.add_argument("--gumbel", action="store_true", default=False, help="batched path: Gumbel root search -- one Gumbel draw per move, sequential "
                    "halving over the considered moves within the move's simulations, the winner is played and pi' = softmax(logits + "
                    "sigma(completed Q)) is the recorded policy target. With --playout-cap-fast the pi' of a fast ply is a valid target too "
                    "(it improves on the prior at any simulation count); such plies are still flagged and the trainer treats the flag as before. "
                    "Not with --root-noise-eps")
    ap.add_argument("--gumbel-considered", type=int, default=None, help=f"... moves considered at the root, 2..128 (default {GUMBEL_CONSIDERED})")
    ap.add_argument("--gumbel-c-visit", type=float, default=None, help=f"... c_visit of sigma, >= 0 (default {GUMBEL_C_VISIT})")
    ap.add_argument("--gumbel-c-scale", type=float, default=None, help=f"... c_scale of sigma, >= 0 (default {GUMBEL_C_SCALE})")


def gumbel_from_args(ap, a):
    """(``a.playout``: the simulations of a move.)"""
    return _from_args(ap, a, "--gumbel", "the Gumbel root search is off", ("--gumbel-considered", "--gumbel-c-visit", "--gumbel-c-scale"),
                      make_gumbel, a.gumbel, a.playout, a.gumbel_considered, a.gumbel_c_visit, a.gumbel_c_scale)


def make_leaf_history(on):
    """The value of the ``leaf_history`` keyword of the front ends: ``{"enabled": True}`` (the dict of ``SelfPlayEngine.set_leaf_history``'s
    arguments) or None."""
    return {"enabled": True} if on else None


def add_leaf_history_args(ap):
    """--leaf-history."""
    ap.add_argument("--leaf-history", action="store_true", default=False, help="batched path: the search shows the network the eight-position "
                    "input a training row holds (the game's recorded plies, the root, the selection path) instead of the leaf alone; the network "
                    "reads all 119 planes (a 128-channel stem) and the evaluation cache keys on the history, so transpositions miss. For nets "
                    "trained on this project's rows; absent = off (the reference's search input)")


def leaf_history_from_args(ap, a):
    return _from_args(ap, a, "--leaf-history", "leaf history planes are off", (), make_leaf_history, a.leaf_history)


def make_surprise(weight, cap=None):
    """The dict of ``SelfPlayEngine.set_surprise``'s arguments (None without a weight). ValueError: what ``ccz_set_surprise`` refuses."""
    if weight is None:
        return None
    if not 0.0 <= weight <= 1.0:
        raise ValueError(f"--surprise-weight must be in [0, 1] (got {weight})")
    if cap is not None and not 1.0 <= cap <= 15.0:
        raise ValueError(f"--surprise-cap must be in [1, 15] (got {cap})")
    return {"alpha": float(weight), "cap": SURPRISE_CAP if cap is None else float(cap)}


def add_surprise_args(ap):
    """--surprise-weight / --surprise-cap."""
    ap.add_argument("--surprise-weight", type=float, default=None, metavar="A", help="batched path: policy surprise weighting -- every recorded "
                    "ply gets a sampling weight: the share 1 - A of its game's weight spread evenly, the share A (in [0, 1], KataGo's "
                    f"{SURPRISE_WEIGHT}) over the full-search plies by KL(search policy || prior). With --train-every the ring draws by it; "
                    "without a ring the weights are written to sample_weights.npy; absent = off")
    ap.add_argument("--surprise-cap", type=float, default=None, metavar="C", help=f"... the largest weight of a ply, in [1, 15] (default {SURPRISE_CAP:g})")


def surprise_from_args(ap, a):
    return _from_args(ap, a, "--surprise-weight", "policy surprise weighting is off", ("--surprise-cap",), make_surprise, a.surprise_weight,
                      a.surprise_cap)


def make_lcb(z, min_visit_ratio=None, min_visits=None):
    """The ``lcb`` dict of the front ends (None when ``z`` is None or False): ``z`` True = the default multiple of the standard error.
    ValueError: what ``ccz_lcb_moves`` refuses."""
    if z is None or z is False:
        return None
    z = LCB_STDEVS if z is True else float(z)
    if not 0.0 <= z < float("inf"):
        raise ValueError(f"--lcb must be finite and >= 0 (got {z})")
    if min_visit_ratio is not None and not 0.0 <= min_visit_ratio <= 1.0:
        raise ValueError(f"--lcb-min-visit-ratio must be in [0, 1] (got {min_visit_ratio})")
    if min_visits is not None and not min_visits >= 0:
        raise ValueError(f"--lcb-min-visits must be >= 0 (got {min_visits})")
    return {"z": z, "min_visit_ratio": LCB_MIN_VISIT_RATIO if min_visit_ratio is None else float(min_visit_ratio),
            "min_visits": LCB_MIN_VISITS if min_visits is None else int(min_visits)}


def add_lcb_args(ap):
    """--lcb [Z] / --lcb-min-visit-ratio / --lcb-min-visits."""
    ap.add_argument("--lcb", type=float, nargs="?", const=True, default=None, metavar="Z", help="play the lower-confidence-bound move instead of "
                    "the most visited one: among the root's children searched enough, the one of largest Q - Z * standard error of its backed-up "
                    f"values (default Z = {LCB_STDEVS:g}, KataGo's lcbStdevs: a convention, not a measurement of this engine); absent = off")
    ap.add_argument("--lcb-min-visit-ratio", type=float, default=None, metavar="R", help="... a child is considered from this share of the most "
                    f"visited child's visits, in [0, 1] (default {LCB_MIN_VISIT_RATIO:g}, KataGo's minVisitPropForLCB)")
    ap.add_argument("--lcb-min-visits", type=int, default=None, metavar="N", help=f"... and from this many visits (default {LCB_MIN_VISITS})")


def lcb_from_args(ap, a):
    return _from_args(ap, a, "--lcb", "the LCB move is off", ("--lcb-min-visit-ratio", "--lcb-min-visits"), make_lcb, a.lcb,
                      a.lcb_min_visit_ratio, a.lcb_min_visits)


# ---------------------------------------------------------------------- the evaluator's own switch (no engine setter: it goes to PolicyValueNet)
def add_fused_narrow_args(ap):
    """--fused-narrow."""
    ap.add_argument("--fused-narrow", action="store_true", default=False, help="nets of 64 or 128 channels (--channels): run the whole evaluator on "
                    "the hand-written kernels for narrow towers instead of MIOpen / hipBLASLt, so that a board's logits and value are the same "
                    "bits at every batch size -- what the evaluation cache, scout slots and planned batches assume (PolicyValueNet(fused_narrow=True), "
                    "CCZ_FUSED_NARROW=1). No effect on other widths; absent = off")


def fused_narrow_from_args(ap, a) -> bool:
    """The value of the ``fused_narrow`` keyword of ``PolicyValueNet``."""
    return bool(a.fused_narrow)
