"""CPU: the host side of engine snapshots and of the collector's checkpoints -- ``snapshot_info`` on a blob the test writes itself
from the documented layout, the checkpoint directory (atomic rename, newest two kept, half-written files ignored, no silent fresh
start), the sink's no-row-twice logic on rows fed by hand, the three flags, and the ABI: still 9, four new calls."""
import os
import re

import numpy as np
import pytest
import torch

from chinesechesszero_amd import _lib, checkpoint, collect
from chinesechesszero_amd import snapshot as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the blob
def synthetic_blob(counts, sections):
    """A snapshot of len(counts) boards written from the layout as include/cczero.h and snapshot.py document it."""
    B = len(counts)
    sizes = [S.FIXED_BYTES + 16 * n + -(-4 * n // 16) * 16 + (-(-n // 16) * 16 if sections & 1 else 0)
             + 96 * p + -(-4 * p // 16) * 16 + 3 * (-(-p // 16) * 16) + ((-(-4 * p // 16) * 16 + -(-p // 16) * 16) if sections & 2 else 0)
             + -(-2 * u // 16) * 16 + -(-4 * u // 16) * 16 for n, p, u in counts]
    start = -(-(512 + 8 * (B + 1) + 40 * B) // 16) * 16
    blob = np.zeros(start + sum(sizes), np.uint8)
    h = blob[:512].view(S.HEADER_DTYPE)
    h["magic"], h["version"], h["header_bytes"], h["total_bytes"], h["sections_start"] = S.MAGIC, 1, 512, blob.size, start
    h["B"], h["cap"], h["max_plies"], h["pi_cap"], h["seed"], h["board_id_base"] = B, 4096, 12, 960, 77, 4096
    h["sections"], h["fixed_bytes"], h["meta_bytes"], h["half"] = sections, S.FIXED_BYTES, 40, 1
    h["resign"]["enabled"], h["resign"]["threshold"] = 1, -0.5
    blob[512:512 + 8 * (B + 1)].view("<u8")[:] = np.concatenate([[0], np.cumsum(sizes)])
    meta = blob[512 + 8 * (B + 1):512 + 8 * (B + 1) + 40 * B].view(S.META_DTYPE)
    for b, (n, p, u) in enumerate(counts):
        meta[b]["n_nodes"], meta[b]["ply"], meta[b]["pi_used"], meta[b]["over"] = n, p, u, b % 2
    off = start + int(np.cumsum([0] + sizes)[1])            # board 1's section: its root mailbox and its budget
    blob[off:off + 90] = 9
    blob[off + 5048:off + 5052].view("<i4")[:] = 24
    return blob, sizes, start


@pytest.mark.parametrize("sections", [0, 1, 2, 3])
def test_snapshot_info_on_a_synthetic_blob(sections, tmp_path):
    counts = [(1, 0, 0), (37, 5, 211), (4096, 12, 960), (16, 16, 16), (15, 1, 7)]
    blob, sizes, start = synthetic_blob(counts, sections)
    for form in (blob, torch.from_numpy(blob.copy()), blob.tobytes()):
        info = S.snapshot_info(form)
        assert info["B"] == 5 and info["seed"] == 77 and info["board_id_base"] == 4096 and info["half"] == 1 and info["sections"] == sections
        assert info["resign"] == {"enabled": 1, "consecutive": 0, "min_ply": 0, "threshold": -0.5, "p_playon": 0.0}
        assert [tuple(x) for x in zip(info["n_nodes"], info["ply"], info["pi_used"])] == counts
        assert list(info["over"]) == [0, 1, 0, 1, 0]
        assert list(info["section_sizes"]) == sizes and info["sections_start"] == start == S.sections_start(5)
        # the documented formula, from the counts alone
        assert list(S.section_bytes(info["n_nodes"], info["ply"], info["pi_used"], sections)) == sizes
        assert info["total_bytes"] == info["bytes"] == S.sections_start(5) + sum(sizes)
    assert (S.fixed_row(blob, info, 1, "root_sq")[:90] == 9).all() and S.fixed_row(blob, info, 1, "budget")[0] == 24
    path = tmp_path / "blob.pt"
    torch.save(torch.from_numpy(blob), str(path))
    assert S.snapshot_info(str(path))["bytes"] == blob.size
    with pytest.raises(ValueError, match="magic"):
        bad = blob.copy(); bad[0] ^= 1
        S.snapshot_info(bad)
    with pytest.raises(ValueError, match="truncated"):
        S.snapshot_info(blob[:600])


def test_fixed_rows_tile_the_fixed_part():
    spans = sorted((o, o + np.dtype(dt).itemsize * n) for o, dt, n in S.FIXED_ROWS.values())
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))      # no gap, no overlap
    assert spans[-1][1] <= S.FIXED_BYTES < spans[-1][1] + 16 and S.FIXED_BYTES % 16 == 0


# ------------------------------------------------------------------------------------------------------------------ the checkpoint directory
def test_checkpoint_directory(tmp_path):
    d = str(tmp_path / "ck")
    with pytest.raises(FileNotFoundError, match="does not exist"):
        checkpoint.newest(d)
    os.makedirs(d)
    with pytest.raises(FileNotFoundError, match="no complete checkpoint"):
        checkpoint.newest(d)
    with open(checkpoint.path_of(d, 9) + ".tmp", "wb") as f:      # what a process that died inside a write leaves
        f.write(b"half")
    with pytest.raises(FileNotFoundError, match="no complete checkpoint"):
        checkpoint.newest(d)
    seen = []
    real = os.replace

    def spy(a, b):
        seen.append((os.path.basename(a), os.path.basename(b), os.path.exists(b)))
        real(a, b)
    os.replace = spy
    try:
        for m in (3, 6, 12):
            assert checkpoint.write(d, m, {"moves_done": m}) == checkpoint.path_of(d, m)
    finally:
        os.replace = real
    assert seen == [(f"ckpt_{m:09d}.pt.tmp", f"ckpt_{m:09d}.pt", False) for m in (3, 6, 12)]      # written under another name, renamed
    assert [m for m, _ in checkpoint.complete(d)] == [6, 12]                                    # the newest two
    assert sorted(os.listdir(d)) == ["ckpt_000000006.pt", "ckpt_000000009.pt.tmp", "ckpt_000000012.pt"]
    moves, payload = checkpoint.load_newest(d)                  # (the half-written 9 is not "newest complete")
    assert moves == 12 and payload == {"moves_done": 12}
    assert checkpoint.differences({"a": 1, "b": (2, 0.5)}, {"a": 1, "b": (2, 0.5)}) == []
    diff = checkpoint.differences({"n_playout": 400, "seed": 1}, {"n_playout": 200, "seed": 1})
    assert len(diff) == 1 and "n_playout" in diff[0] and "400" in diff[0] and "200" in diff[0]


def test_pipeline_refuses_what_it_cannot_resume(tmp_path):
    kw = dict(n_boards=4, n_playout=8, data_dir=str(tmp_path / "data"))
    with pytest.raises(FileNotFoundError):
        collect.CollectPipeline(checkpoint_dir=str(tmp_path / "missing"), resume=True, **kw)
    os.makedirs(tmp_path / "empty")
    with pytest.raises(FileNotFoundError, match="no complete checkpoint"):
        collect.CollectPipeline(checkpoint_dir=str(tmp_path / "empty"), resume=True, **dict(kw, data_dir=str(tmp_path / "d2")))
    with pytest.raises(ValueError, match="checkpoint_dir"):
        collect.CollectPipeline(checkpoint_every=3, **dict(kw, data_dir=str(tmp_path / "d3")))
    with pytest.raises(ValueError, match="n_boards"):
        collect.CollectPipeline(n_boards=1, checkpoint_dir=str(tmp_path / "c"), data_dir=str(tmp_path / "d4"))

    class TwoRanks:
        world, rank = 2, 0
    with pytest.raises(ValueError, match="exchange"):
        collect.CollectPipeline(checkpoint_dir=str(tmp_path / "c"), gatherer=TwoRanks(), **dict(kw, data_dir=str(tmp_path / "d5")))
    # other options than the checkpoint's: named
    p = collect.CollectPipeline(checkpoint_dir=str(tmp_path / "c"), **dict(kw, data_dir=str(tmp_path / "d6")))
    q = collect.CollectPipeline(checkpoint_dir=str(tmp_path / "c"), solver=True, **dict(kw, n_playout=16, data_dir=str(tmp_path / "d7")))
    diff = checkpoint.differences(p._signature(), q._signature())
    assert len(diff) == 2 and any(x.startswith("n_playout:") for x in diff) and any(x.startswith("option solver:") for x in diff)


# ------------------------------------------------------------------------------------------------------------------ no row twice
def _rows(r, n):
    return (r.rand(n, 17, 7, 10, 9).astype(np.float16), r.dirichlet(np.ones(2086), size=n), r.choice([-1.0, 0.0, 1.0], size=n).astype(np.float32))


def test_sink_skips_exactly_the_replayed_rows(tmp_path):
    r = np.random.RandomState(3)
    X, Y, Z = _rows(r, 10), _rows(r, 6), _rows(r, 4)
    whole = collect.TupleSink(str(tmp_path / "whole"))          # the uninterrupted run
    for part in (X, Y, Z):
        whole.append(*part, games=1)
    assert whole.finalize() == 20
    whole.close()
    d = str(tmp_path / "killed")
    dead = collect.TupleSink(d)
    dead.append(*X, games=1)
    rows_ck, games_ck = dead.total_rows(), dead.games           # the checkpoint: 10 rows, 1 game
    dead.append(*Y, games=1)                                    # appended after it; then the process dies (no finalize)
    dead.close()
    again = collect.TupleSink(d)                                # the resumed job's sink adopts what it finds ...
    assert again.total_rows() == 16 and again.games == 2
    again.resume_from(rows_ck, games_ck)
    assert again.games == 1
    again.append(*(a[:4] for a in Y), games=0)                  # ... and the replay delivers Y again, here in two pieces
    again.append(*(a[4:] for a in Y), games=1)
    assert again.total_rows() == 16 and again.games == 2        # nothing new on disk
    again.append(*Z, games=1)
    assert again.finalize() == 20 and again.games == 3
    again.close()
    for name in ("states.npy", "mcts.npy", "winners.npy"):
        with open(tmp_path / "whole" / name, "rb") as f, open(os.path.join(d, name), "rb") as g:
            assert f.read() == g.read(), name
    # an append that straddles the boundary keeps its tail
    d2 = str(tmp_path / "straddle")
    s = collect.TupleSink(d2)
    s.append(*X, games=1)
    s.close()
    s = collect.TupleSink(d2)
    s.resume_from(7, 0)
    s.append(*(np.concatenate([x[7:], y]) for x, y in zip(X, Y)), games=1)     # the replay's first append after a checkpoint at 7 rows:
    assert s.total_rows() == 16                                 # rows 7..9 are found (dropped), Y is new (kept)
    assert s.finalize() == 16
    s.close()
    assert np.array_equal(np.load(os.path.join(d2, "winners.npy")), np.concatenate([X[2], Y[2]]))
    # record shards: plies count twice with mirror images
    d3 = str(tmp_path / "records")
    s = collect.TupleSink(d3)
    rec = np.zeros((5, 880), np.uint8)
    s.append_records(rec, flags=0, games=1)
    s.close()
    s = collect.TupleSink(d3)
    assert s.total_rows() == 10
    s.resume_from(4, 0)
    s.append_records(rec, flags=0, games=1)                     # the checkpoint saw 2 plies, 5 are found: of the replay's next 5 plies
    assert s.total_rows() == 10 + 4                             # the first 3 are dropped, 2 are new
    s.close()
    # fewer rows than the checkpoint saw: data was removed, no resume on top of that
    s = collect.TupleSink(str(tmp_path / "fresh"))
    with pytest.raises(ValueError, match="fewer"):
        s.resume_from(5, 0)
    s.close()


# ------------------------------------------------------------------------------------------------------------------ flags
def test_flags(monkeypatch, capsys):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = collect.parse_args(["--boards", "16"])
    assert a.checkpoint == {"checkpoint_dir": None, "checkpoint_every": 0, "resume": False}
    a = collect.parse_args(["--boards", "16", "--checkpoint-dir", "ck", "--checkpoint-every", "50", "--resume"])
    assert a.checkpoint == {"checkpoint_dir": "ck", "checkpoint_every": 50, "resume": True}
    for argv, word in ((["--boards", "16", "--resume"], "--checkpoint-dir"), (["--boards", "16", "--checkpoint-every", "5"], "--checkpoint-dir"),
                       (["--boards", "1", "--checkpoint-dir", "ck"], "--boards"),
                       (["--boards", "16", "--checkpoint-dir", "ck", "--checkpoint-every", "-1"], "negative")):
        with pytest.raises(SystemExit):
            collect.parse_args(argv)
        assert word in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        collect.parse_args(["--boards", "16", "--checkpoint-dir", "ck"])
    err = capsys.readouterr().err
    assert "single-rank" in err and "exchange" in err
    assert collect.parse_args(["--boards", "16"]).checkpoint["checkpoint_dir"] is None      # several ranks without checkpoints: as ever


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_is_still_9_with_four_new_calls():
    with open(os.path.join(ROOT, "include", "cczero.h"), encoding="utf-8") as f:
        header = f.read()
    assert "#define CCZ_ABI_VERSION 9 " in header and _lib.ABI_VERSION == 9
    L = _lib.lib()
    assert L.ccz_abi_version() == 9
    for name in ("ccz_snapshot_size", "ccz_snapshot_save", "ccz_snapshot_load", "ccz_snapshot_layout"):
        assert name in _lib.PROTOTYPES and hasattr(L, name)
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]), name
    assert f"#define CCZ_SNAP_FIXED_BYTES {S.FIXED_BYTES}" in header and f"#define CCZ_SNAP_HEADER_BYTES {S.HEADER_BYTES}" in header
    # the calls refuse nonsense without touching a device
    assert L.ccz_snapshot_size(None, None, None) == -1 and L.ccz_snapshot_layout(None, 0, None, None, None, 0, None) == -1
