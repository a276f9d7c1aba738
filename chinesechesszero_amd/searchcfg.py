"""The search parameters of ``ccz_set_search`` (include/cczero.h) as the front-ends spell them: the command-line
flags of ``collect`` / ``arena`` / ``analyse``, the UCI options, and the dict that ``SelfPlayEngine.set_search`` takes. No GPU here."""
from __future__ import annotations

import math

FPU_OFF, FPU_REDUCTION, FPU_ABSOLUTE = 0, 1, 2
C_BASE = 19652.0          # AlphaZero's; idle while c_factor is 0


def make_search(fpu_reduction=None, fpu_absolute=None, fpu_root_reduction=None, fpu_root_absolute=None, cpuct_base=None,
                cpuct_factor=None):
    """The dict of ``SelfPlayEngine.set_search``'s arguments for these settings, or None when none is given (the rule stays off).
    Reduction and absolute exclude each other; the root takes the tree's setting unless it is given one. Raises ValueError on
    what ``ccz_set_search`` would refuse."""
    given = (fpu_reduction, fpu_absolute, fpu_root_reduction, fpu_root_absolute, cpuct_base, cpuct_factor)
    if all(x is None for x in given):
        return None
    if fpu_reduction is not None and fpu_absolute is not None:
        raise ValueError("fpu reduction and fpu absolute exclude each other")
    if fpu_root_reduction is not None and fpu_root_absolute is not None:
        raise ValueError("fpu root reduction and fpu root absolute exclude each other")

    def pair(red, ab, what):
        if red is not None:
            if not (math.isfinite(red) and red >= 0.0):
                raise ValueError(f"{what} reduction {red} must be finite and >= 0")
            return FPU_REDUCTION, float(red)
        if ab is not None:
            if not -1.0 <= ab <= 1.0:
                raise ValueError(f"{what} absolute {ab} must be in [-1, 1]")
            return FPU_ABSOLUTE, float(ab)
        return FPU_OFF, 0.0

    mode, value = pair(fpu_reduction, fpu_absolute, "fpu")
    rmode, rvalue = (mode, value) if fpu_root_reduction is None and fpu_root_absolute is None else pair(fpu_root_reduction, fpu_root_absolute, "fpu root")
    base = C_BASE if cpuct_base is None else float(cpuct_base)
    factor = 0.0 if cpuct_factor is None else float(cpuct_factor)
    if not (math.isfinite(base) and base > 0.0):
        raise ValueError(f"cpuct base {base} must be finite and > 0")
    if not (math.isfinite(factor) and factor >= 0.0):
        raise ValueError(f"cpuct factor {factor} must be finite and >= 0")
    return {"fpu_mode": mode, "fpu_value": value, "fpu_root_mode": rmode, "fpu_root_value": rvalue, "c_base": base, "c_factor": factor}


def add_search_args(ap):
    """--fpu-reduction / --fpu-absolute / --fpu-root-reduction / --fpu-root-absolute / --cpuct-base / --cpuct-factor on an ArgumentParser."""
    g = ap.add_argument_group("search parameters (first-play urgency, visit-scaled c_puct; absent = the reference's PUCT)")
    t = g.add_mutually_exclusive_group()
    t.add_argument("--fpu-reduction", type=float, default=None, metavar="R",
                   help="an unvisited child scores its parent's value minus R * sqrt(visited prior mass) instead of +inf (Lc0 / KataGo)")
    t.add_argument("--fpu-absolute", type=float, default=None, metavar="V", help="an unvisited child scores V in [-1, 1] (AlphaZero)")
    r = g.add_mutually_exclusive_group()
    r.add_argument("--fpu-root-reduction", type=float, default=None, metavar="R", help="the same at the root (default: the tree's setting)")
    r.add_argument("--fpu-root-absolute", type=float, default=None, metavar="V", help="the same at the root (default: the tree's setting)")
    g.add_argument("--cpuct-base", type=float, default=None, help=f"c_puct grows by factor * log((N + base + 1) / base) (default {C_BASE:g})")
    g.add_argument("--cpuct-factor", type=float, default=None, help="weight of that growth (default 0: c_puct is constant)")


def search_from_args(ap, a):
    """``make_search`` of the parsed flags; a bad value ends in ``ap.error``."""
    try:
        s = make_search(a.fpu_reduction, a.fpu_absolute, a.fpu_root_reduction, a.fpu_root_absolute, a.cpuct_base, a.cpuct_factor)
    except ValueError as ex:
        ap.error(str(ex))
    return s


def resolve_scouts(search, scouts):
    """The scout slots of a one-game search: with search parameters given and ``scouts`` None it runs without scouts; both given
    explicitly is a ValueError."""
    if search is None:
        return scouts
    if scouts is not None and int(scouts) > 0:
        raise ValueError("search parameters and scouts exclude each other: scout slots rest on children being first visited in "
                         "legal-move order (pass scouts=0 or leave it None)")
    return 0


def mean_leaf_depth(stats: dict) -> float:
    """Mean depth of the leaves selected so far, from ``SelfPlayEngine.stats()`` (``sum_depth`` over ``sims``)."""
    return float(stats["sum_depth"]) / float(stats["sims"]) if stats.get("sims") else 0.0
