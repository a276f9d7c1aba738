"""The early-stop settings of ``ccz_set_early_stop`` (include/cczero.h) as the front-ends spell them: the
command-line flags of ``collect`` / ``arena`` / ``analyse`` and the dict that ``SelfPlayEngine.set_early_stop`` takes. No GPU here."""
from __future__ import annotations

import math

SINGLE_REPLY, VISIT_GAP, KLD_GAIN = 1, 2, 3
REASONS = {SINGLE_REPLY: "single_reply", VISIT_GAP: "visit_gap", KLD_GAIN: "kld_gain"}
GAP_DEFAULT = 1.0          # the exact rule: the runner-up cannot catch the leader
KLD_INTERVAL = 16
POLL_EVERY = 16            # steps between two questions of an arg-max front end's move loop to the engine (StopPoll)


def make_early_stop(single_reply=False, gap=None, kld_gain=None, kld_interval=None, min_sims=None):
    """The dict of ``SelfPlayEngine.set_early_stop``'s arguments for these settings, or None when no rule is asked for (the feature
    stays off). ``gap``: the factor f of the visit-gap rule (>= 1); ``kld_gain``: the gain per new visit below which a board stops,
    looked at every ``kld_interval`` simulations (default 16). Raises ValueError on what ``ccz_set_early_stop`` would refuse."""
    if not single_reply and gap is None and kld_gain is None:
        if kld_interval is not None or min_sims is not None:
            raise ValueError("kld interval / min sims without a stop rule (single reply, gap or kld gain)")
        return None
    f = 0.0
    if gap is not None:
        f = float(gap)
        if not (math.isfinite(f) and f >= 1.0):
            raise ValueError(f"stop gap {gap} must be finite and >= 1")
    g, interval = 0.0, 0
    if kld_gain is not None:
        g = float(kld_gain)
        if not (math.isfinite(g) and g >= 0.0):
            raise ValueError(f"stop kld gain {kld_gain} must be finite and >= 0")
        interval = KLD_INTERVAL if kld_interval is None else int(kld_interval)
        if interval < 1:
            raise ValueError(f"stop kld interval {kld_interval} must be >= 1")
    elif kld_interval is not None:
        raise ValueError("stop kld interval without a stop kld gain")
    n = 0 if min_sims is None else int(min_sims)
    if n < 0:
        raise ValueError(f"stop min sims {min_sims} must be >= 0")
    return {"single_reply": bool(single_reply), "gap_factor": f, "kld_interval": interval, "min_gain": g, "min_sims": n}


def add_early_stop_args(ap):
    """--stop-single-reply / --stop-gap [F] / --stop-kld-gain G / --stop-kld-interval I / --stop-min-sims N on an ArgumentParser."""
    g = ap.add_argument_group("early stop per board (absent = every move searches all its simulations)")
    g.add_argument("--stop-single-reply", action="store_true", help="a board with one legal move stops searching it")
    g.add_argument("--stop-gap", type=float, nargs="?", const=GAP_DEFAULT, default=None, metavar="F",
                   help=f"a board stops when (N1 - N2) * F exceeds the simulations left (default F = {GAP_DEFAULT:g}: the runner-up cannot catch up)")
    g.add_argument("--stop-kld-gain", type=float, default=None, metavar="G",
                   help="a board stops when the KL divergence of its root visits per new visit falls below G")
    g.add_argument("--stop-kld-interval", type=int, default=None, metavar="I", help=f"simulations between two looks at the gain (default {KLD_INTERVAL})")
    g.add_argument("--stop-min-sims", type=int, default=None, metavar="N", help="no rule runs below N simulations of a move (default 0)")


def early_stop_from_args(ap, a):
    """``make_early_stop`` of the parsed flags; a bad value ends in ``ap.error``."""
    try:
        return make_early_stop(a.stop_single_reply, a.stop_gap, a.stop_kld_gain, a.stop_kld_interval, a.stop_min_sims)
    except ValueError as ex:
        ap.error(str(ex))


def stop_report(stats: dict, moves: int, sims: int) -> dict:
    """What the front ends log: the stops per reason and the mean simulations per move, from ``SelfPlayEngine.early_stop_stats()``
    and the moves played / simulations run over the same span."""
    out = {k: int(stats.get(k, 0)) for k in ("single_reply", "visit_gap", "kld_gain", "sims_saved")}
    out["mean_sims_per_move"] = round(float(sims) / float(moves), 3) if moves else 0.0
    return out


class StopPoll:
    """The move loop of an arg-max front end: ``done(step)`` is True when no board would select any more -- asked of the engine
    every ``every`` steps (one small kernel and a 4-byte copy), never when the feature is off."""

    def __init__(self, engine, cfg, every: int = POLL_EVERY):
        self.engine, self.on, self.every = engine, cfg is not None, int(every)

    def done(self, step: int) -> bool:
        return self.on and step > 0 and step % self.every == 0 and self.engine.searching() == 0
