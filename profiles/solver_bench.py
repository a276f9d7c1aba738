"""python bench.py with something swapped in, for the MCTS-solver's measurements (CHANGELOG.md; bench.py itself is not touched).

    python profiles/solver_bench.py --lib build/diag/libcczero_parent.so [bench args]   # the bench on another libcczero.so (the parent
                                                                                         # commit's: the off-cost A/B, profiles/solver_off_ab.json)
    python profiles/solver_bench.py --solver [bench args]                                # the bench with ccz_set_solver(1) on its engine

Both print bench.py's one JSON line; ``--solver`` follows it with one JSON line of its own: ``solver_stats()`` of the bench's engine at
the end of the run, the moves it played, and how many of the games that ended by the rules had their last move played from a root the
solver had proven. An older library exports no solver entry points: their prototypes are left out for it (the bench calls none)."""
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    lib, solver = None, False
    if "--lib" in argv:
        i = argv.index("--lib")
        lib = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    if "--solver" in argv:
        argv.remove("--solver")
        solver = True
    from chinesechesszero_amd import _lib
    if lib is not None:
        _lib.LIB_PATH = lib
        for name in ("ccz_set_solver", "ccz_root_proof", "ccz_get_solver_stats", "ccz_proof_combine"):
            _lib.PROTOTYPES.pop(name, None)
    seen = {"engine": None, "moves": 0, "games_ended_by_rules": 0, "of_them_last_root_proven": 0}
    if solver:
        from chinesechesszero_amd.engine import SelfPlayEngine
        init, finish = SelfPlayEngine.__init__, SelfPlayEngine.finish_move

        def init_on(self, *a, **kw):
            init(self, *a, **kw)
            self.set_solver(True)
            seen["engine"] = self

        def finish_counted(self, *a, **kw):
            before, proven = self.game_status(), self.root_proof()["state"] != 0
            out = finish(self, *a, **kw)
            after = self.game_status()
            ended = (before["over"] == 0) & (after["over"] == 1) & (out.cpu().numpy() >= 0)     # a move ended it: not the ply cap, not a resignation
            seen["moves"] += 1
            seen["games_ended_by_rules"] += int(ended.sum())
            seen["of_them_last_root_proven"] += int((ended & proven).sum())
            return out

        SelfPlayEngine.__init__, SelfPlayEngine.finish_move = init_on, finish_counted
    sys.argv = [os.path.join(ROOT, "bench.py")] + argv
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        if solver and seen["engine"] is not None:
            e = seen.pop("engine")
            print(json.dumps({"solver": e.solver_stats(), **seen, "sims": e.stats()["sims"], "terminal_leaves": e.stats()["terminal_leaves"]}), flush=True)


if __name__ == "__main__":
    main()
