"""python bench.py with something swapped in, for the measurements of the search parameters (ccz_set_search; CHANGELOG.md; bench.py
itself is not touched).

    python profiles/search_bench.py --lib PATH/libcczero_parent.so [bench args]     # the bench on another libcczero.so (the parent commit's:
                                                                                     # the off-cost A/B, profiles/search_off_ab.json)
    python profiles/search_bench.py --fpu-reduction 0.33 [--cpuct-base 19652 --cpuct-factor 2] [bench args]
                                                                                     # the bench with ccz_set_search on its engine
                                                                                     # (profiles/search_on_report.json)

Both print bench.py's one JSON line, followed by one JSON line of this script's own: the settings the kernels read (none on another
library), the simulation count and the mean leaf depth of the bench's engine at the end of the run. An older library exports no
ccz_set_search / ccz_get_search: their prototypes are left out for it (the bench calls neither)."""
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OWN = {"--lib": str, "--fpu-reduction": float, "--fpu-absolute": float, "--cpuct-base": float, "--cpuct-factor": float}


def main():
    argv = sys.argv[1:]
    own = {}
    for flag, kind in OWN.items():
        if flag in argv:
            i = argv.index(flag)
            own[flag] = kind(argv[i + 1])
            del argv[i:i + 2]
    from chinesechesszero_amd import _lib
    from chinesechesszero_amd.searchcfg import make_search, mean_leaf_depth
    lib = own.get("--lib")
    if lib is not None:
        _lib.LIB_PATH = os.path.abspath(lib)
        for name in ("ccz_set_search", "ccz_get_search"):
            _lib.PROTOTYPES.pop(name, None)
    search = make_search(own.get("--fpu-reduction"), own.get("--fpu-absolute"), None, None, own.get("--cpuct-base"), own.get("--cpuct-factor"))
    if search is not None and lib is not None:
        raise SystemExit("--lib names a library without ccz_set_search: the search flags cannot go with it")
    seen = {"engine": None}
    from chinesechesszero_amd.engine import SelfPlayEngine
    init = SelfPlayEngine.__init__

    def init_seen(self, *a, **kw):
        init(self, *a, **kw)
        if search is not None:
            self.set_search(**search)
        seen["engine"] = self

    SelfPlayEngine.__init__ = init_seen
    sys.argv = [os.path.join(ROOT, "bench.py")] + argv
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        e = seen["engine"]
        if e is not None:
            st = e.stats()
            print(json.dumps({"search": None if lib is not None else e.search_settings(), "sims": st["sims"],
                              "mean_leaf_depth": round(mean_leaf_depth(st), 4), "depth_peak": st["depth_peak"]}), flush=True)


if __name__ == "__main__":
    main()
