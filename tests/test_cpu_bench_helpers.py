"""CPU: the parts of bench.py that need no GPU -- which committed profile a bench line may quote (round 5: a profile is tied to
the code it was taken with), and that the code hash moves when a kernel source does."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WL = {"boards_per_gpu": 4096, "sims_per_move": 400, "evaluator": "net", "max_plies": 200, "blocks": 40, "channels": 256,
      "preroll_plies": 200, "align": True}


def _profile(tmp_path, **kw):
    pm = {"k_step": {"avg_ns": 33000.0, "window": {"hbm_bytes_per_launch": 4.0e7}},
          "workload": {"boards_per_gpu": 4096, "sims_per_move": 400, "evaluator": "net", "max_plies": 200}, "head": "aaaabbbbccccdddd", "tag": "r05"}
    pm.update(kw)
    p = tmp_path / "pmc_summary.json"
    p.write_text(json.dumps(pm))
    return str(p)


def test_a_profile_of_other_code_or_another_workload_is_refused(tmp_path):
    import bench
    pm, why, head = bench.committed_profile(_profile(tmp_path), "aaaabbbbccccdddd", WL)
    assert pm is not None and why is None and head == "aaaabbbbccccdddd" and pm["k_step"]["avg_ns"] == 33000.0
    pm, why, head = bench.committed_profile(_profile(tmp_path), "0000111122223333", WL)           # the code changed since the profile
    assert pm is None and "other code" in why and head == "aaaabbbbccccdddd"
    pm, why, _ = bench.committed_profile(_profile(tmp_path, head=None), "aaaabbbbccccdddd", WL)   # a profile that does not say
    assert pm is None and "no head" in why
    for key, val in (("boards_per_gpu", 1024), ("sims_per_move", 800), ("evaluator", "stub"), ("blocks", 2), ("align", False)):
        pm, why, _ = bench.committed_profile(_profile(tmp_path), "aaaabbbbccccdddd", dict(WL, **{key: val}))
        assert pm is None and "another workload" in why and key in why
    pm, why, _ = bench.committed_profile(str(tmp_path / "missing.json"), "x", WL)
    assert pm is None and "no committed profile" in why


def test_the_committed_profile_names_its_head_and_holds_no_kernel_that_no_longer_runs():
    """profiles/pmc_summary.json as committed: it says which code it was taken with, and every kernel block in it belongs to a kernel
    the profiled run launched (round 4 shipped a k_head_conv1x1 block of a kernel that had left the timed path)."""
    with open(os.path.join(ROOT, "profiles", "pmc_summary.json")) as f:
        pm = json.load(f)
    assert isinstance(pm.get("head"), str) and len(pm["head"]) == 16 and pm.get("tag")
    stats = os.path.join(ROOT, "profiles", f"{pm['tag']}_kernel_stats.csv")
    assert os.path.exists(stats)
    names = open(stats).read()
    for k, v in pm.items():
        if isinstance(v, dict) and k.startswith("k_"):
            assert k in names, f"{k}: in the PMC summary, not in {pm['tag']}_kernel_stats.csv"


def test_the_committed_profile_is_of_this_code():
    """The profile bench.py will quote was taken with the code in this tree: whoever changes a kernel, the C ABI, the launch loop or the
    evaluator re-runs profiles/run_profile.sh (or this test says so). bench.py itself would fall back to its raw HIP-event figure."""
    from chinesechesszero_amd.build import code_hash
    with open(os.path.join(ROOT, "profiles", "pmc_summary.json")) as f:
        pm = json.load(f)
    assert pm["head"] == code_hash(), (f"profiles/pmc_summary.json was taken with code {pm['head']}, the tree is {code_hash()}: "
                                       "re-run `bash profiles/run_profile.sh rNN trace fetch write sq` (and the c* passes) on a GPU box")
    assert "head_warning" not in pm, pm.get("head_warning")


def test_code_hash_follows_the_kernel_sources(tmp_path, monkeypatch):
    from chinesechesszero_amd import build
    h0 = build.code_hash()
    assert len(h0) == 16 and h0 == build.code_hash()
    # a copy of the package tree with one byte more in one kernel header hashes differently
    import shutil
    dst = tmp_path / "repo" / "chinesechesszero_amd"
    shutil.copytree(os.path.join(ROOT, "chinesechesszero_amd"), dst, ignore=shutil.ignore_patterns("*.so", "__pycache__", ".pytest_cache"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "repo" / "include")     # (round 6: the C header and bench.py are hashed too)
    shutil.copy(os.path.join(ROOT, "bench.py"), tmp_path / "repo" / "bench.py")
    monkeypatch.setattr(build, "_HERE", str(dst))
    assert build.code_hash() == h0
    with open(dst / "csrc" / "cczero_kernels.h", "a") as f:
        f.write("\n")
    h1 = build.code_hash()
    assert h1 != h0
    with open(tmp_path / "repo" / "include" / "cczero.h", "a") as f:
        f.write("\n")
    assert build.code_hash() not in (h0, h1)


def test_a_library_older_than_its_sources_is_refused(tmp_path, monkeypatch):
    """The csrc Makefile stamps libcczero.so with a digest of the sources it was built from; `_lib.lib()` refuses a library whose stamp is
    not the digest of the sources in the tree (round 5 ran a whole round of GPU calls through a library built before the last kernel edit)."""
    import shutil
    from chinesechesszero_amd import _lib
    assert _lib.stale_build() is None and _lib.source_hash() == open(_lib.LIB_PATH + ".srchash").read().strip()
    root = tmp_path / "repo"
    shutil.copytree(os.path.join(ROOT, "chinesechesszero_amd"), root / "chinesechesszero_amd", ignore=shutil.ignore_patterns("__pycache__", ".pytest_cache"))
    shutil.copytree(os.path.join(ROOT, "include"), root / "include")
    monkeypatch.setattr(_lib, "_HERE", str(root / "chinesechesszero_amd"))
    monkeypatch.setattr(_lib, "LIB_PATH", str(root / "chinesechesszero_amd" / "libcczero.so"))
    assert _lib.stale_build() is None
    with open(root / "chinesechesszero_amd" / "csrc" / "cczero_kernels.h", "a") as f:
        f.write("// edited after the build\n")
    assert "built from other sources" in _lib.stale_build()
    monkeypatch.setattr(_lib, "_lib", None)
    import pytest
    with pytest.raises(_lib.CczError, match="rebuild"):
        _lib.lib()
    os.remove(root / "chinesechesszero_amd" / "libcczero.so.srchash")
    assert "carries no source stamp" in _lib.stale_build()


class _FakeEngine:
    """The inspection calls bench.dump_outputs makes, with the shapes and dtypes of SelfPlayEngine's (engine.py)."""

    def __init__(self, B):
        import numpy as np
        import torch
        rs = np.random.RandomState(B)
        self.B = B
        self._rc = {"k": rs.randint(0, 128, B).astype(np.int32), "acts": rs.randint(0, 2086, (B, 128)).astype(np.uint16),
                    "visits": rs.randint(0, 400, (B, 128)).astype(np.int32), "q": rs.randn(B, 128).astype(np.float32),
                    "prior": rs.rand(B, 128).astype(np.float32), "root_visits": rs.randint(0, 400, B).astype(np.int32)}
        self._leaf = {"status": rs.randint(0, 3, B).astype(np.uint8), "k": rs.randint(0, 128, B).astype(np.int32),
                      "ids": rs.randint(0, 2086, (B, 128)).astype(np.uint16), "depth": rs.randint(0, 30, B).astype(np.int32)}
        self._st = {"over": rs.randint(0, 2, B).astype(np.uint8), "winner": rs.randint(-1, 2, B).astype(np.int8),
                    "plies": rs.randint(0, 200, B).astype(np.int32), "turn": rs.randint(0, 2, B).astype(np.uint8)}
        self.pi = rs.rand(B, 128)
        self.moves_out = torch.from_numpy(rs.randint(-1, 2086, B).astype(np.int32))

    def root_children(self):
        return self._rc

    def leaf_info(self):
        return self._leaf

    def game_status(self):
        return self._st

    def root_pi(self):
        return self.pi


def test_dump_outputs_writes_every_board_as_float_arrays(tmp_path):
    import numpy as np
    import bench
    e = _FakeEngine(48)
    bench.dump_outputs(e, str(tmp_path / "out"))
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) >= {"board_index", "root_actions", "root_visits", "root_q", "root_prior", "root_pi", "leaf_ids", "last_moves", "game_plies"}
    assert all(v.dtype in (np.float32, np.float64) and v.shape[0] == 48 for v in got.values())
    assert np.array_equal(got["board_index"], np.arange(48)) and got["root_pi"].dtype == np.float64
    assert np.array_equal(got["root_visits"], e._rc["visits"]) and np.array_equal(got["root_actions"], e._rc["acts"])
    assert np.array_equal(got["root_q"], e._rc["q"]) and np.array_equal(got["root_pi"], e.pi)
    assert np.array_equal(got["leaf_ids"], e._leaf["ids"]) and np.array_equal(got["game_winner"], e._st["winner"])
    assert np.array_equal(got["last_moves"], e.moves_out.numpy())


def test_dump_outputs_samples_a_fixed_set_of_boards_under_the_size_cap(tmp_path, monkeypatch):
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40 * (128 * 28 + 48))   # room for 40 of the 100 boards
    e = _FakeEngine(100)
    for d in ("a", "b"):
        bench.dump_outputs(e, str(tmp_path / d))
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))   # (minus each .npy header)
    assert total <= bench.DUMP_MAX_BYTES
    idx = np.load(tmp_path / "a" / "board_index.npy")
    assert len(idx) == 40 and np.all(np.diff(idx) > 0) and np.array_equal(idx, np.load(tmp_path / "b" / "board_index.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "root_q.npy"), e._rc["q"][idx.astype(np.int64)])
