"""python bench.py with something swapped in, for the Gumbel root search's measurements (CHANGELOG.md; bench.py itself is not touched).

    python profiles/gumbel_bench.py --lib build/diag/libcczero_parent.so [bench args]   # the bench on another libcczero.so (the parent
                                                                                         # commit's: the off-cost A/B, profiles/gumbel_off_ab.json)
    python profiles/gumbel_bench.py --gumbel [bench args]                                # the bench with ccz_set_gumbel(1, n_sims = --playout) on its engine

Both print bench.py's one JSON line; ``--gumbel`` follows it with one JSON line of its own: ``gumbel_stats()`` and the simulation count
of the bench's engine at the end of the run. An older library exports no Gumbel entry points: their prototypes are left out for it
(the bench calls none)."""
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    lib, gumbel = None, False
    if "--lib" in argv:
        i = argv.index("--lib")
        lib = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    if "--gumbel" in argv:
        argv.remove("--gumbel")
        gumbel = True
    from chinesechesszero_amd import _lib
    if lib is not None:
        _lib.LIB_PATH = lib
        for name in ("ccz_set_gumbel", "ccz_get_gumbel_stats", "ccz_gumbel_root", "ccz_gumbel_sequence"):
            _lib.PROTOTYPES.pop(name, None)
    seen = {"engine": None}
    if gumbel:
        from chinesechesszero_amd.engine import SelfPlayEngine
        init = SelfPlayEngine.__init__

        def init_on(self, *a, **kw):
            init(self, *a, **kw)
            self.set_gumbel(self.n_playout)
            seen["engine"] = self

        SelfPlayEngine.__init__ = init_on
    sys.argv = [os.path.join(ROOT, "bench.py")] + argv
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        if gumbel and seen["engine"] is not None:
            e = seen["engine"]
            print(json.dumps({"gumbel": e.gumbel_stats(), "sims": e.stats()["sims"]}), flush=True)


if __name__ == "__main__":
    main()
