"""CPU: the surface of the record replay ring (ccz_ring_retire / ccz_sample_records, replay.RecordReplayBuffer, the
collector's --replay-plies / --train-every) -- everything that needs no device."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_arity(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/cczero.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_library_and_shim_agree_on_the_two_entry_points():
    from chinesechesszero_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cczero.h")).read()
    L = _lib.lib()
    for name in ("ccz_ring_retire", "ccz_sample_records"):
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == _declared_arity(hdr, name)
        assert hasattr(L, name)
    # the shim's arity rule holds for the call the new ones are modelled on, too
    assert len(_lib.PROTOTYPES["ccz_expand_records"][1]) == _declared_arity(hdr, "ccz_expand_records")
    # ABI 9: both calls gained target_dev / value_dev and the four side calls went away
    assert L.ccz_abi_version() == _lib.ABI_VERSION == 9
    assert _declared_arity(hdr, "ccz_sample_records") == 14 and _declared_arity(hdr, "ccz_expand_records") == 13
    assert not any(n.endswith(("_record_targets", "_record_values")) for n in _lib.PROTOTYPES)


def test_entry_points_validate_their_arguments_before_any_launch():
    from chinesechesszero_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bad_map = (ctypes.c_uint8 * 8)(0, 1, 1, 2, 3, 4, 5, 6)
    assert L.ccz_ring_retire(None, p, 0, p, 0, 14, None) != 0 and b"ccz_ring_retire" in L.ccz_last_error()
    assert L.ccz_ring_retire(None, p, 27, p, 0, 14, None) != 0             # smaller than two games
    assert L.ccz_ring_retire(None, p, 64, p, 0, 0, None) != 0
    assert L.ccz_ring_retire(None, p, 64, p, 0, 70000, None) != 0          # T is 16 bits
    assert L.ccz_ring_retire(None, None, 64, p, 0, 14, None) != 0
    assert L.ccz_ring_retire(None, p, 64, p, -1, 14, None) != 0
    assert L.ccz_sample_records(None, p, 0, p, p, 4, 0, None, p, p, p, None, None, None) != 0 and b"ccz_sample_records" in L.ccz_last_error()
    assert L.ccz_sample_records(None, p, 64, p, p, -1, 0, None, p, p, p, None, None, None) != 0
    assert L.ccz_sample_records(None, p, 64, None, p, 4, 0, None, p, p, p, None, None, None) != 0
    assert L.ccz_sample_records(None, p, 64, p, p, 4, 0, bad_map, p, p, p, None, None, None) != 0 and b"permutation" in L.ccz_last_error()
    assert L.ccz_sample_records(None, p, 64, p, p, 0, 0, None, p, p, p, None, None, None) == 0      # an empty batch launches nothing
    # ccz_expand_records: the dense outputs are all given, or none of them and then a side output (the side-only mode)
    assert L.ccz_expand_records(None, p, 4, 0, None, None, None, None, 0, 0, None, None, None) != 0 and b"ccz_expand_records: null buffer" in L.ccz_last_error()
    for trio in ((None, p, p), (p, None, p), (p, p, None), (p, None, None)):
        assert L.ccz_expand_records(None, p, 4, 0, None, *trio, 0, 0, None, p, p) != 0 and b"ccz_expand_records: null buffer" in L.ccz_last_error()
    assert L.ccz_expand_records(None, p, 4, 0, None, None, None, None, 0, 3, None, p, None) != 0 and b"head_row needs ring_rows" in L.ccz_last_error()
    assert L.ccz_expand_records(None, p, 4, 0, None, None, None, None, 7, 0, None, p, None) != 0 and b"do not fit" in L.ccz_last_error()
    assert L.ccz_expand_records(None, p, 4, 0, None, None, None, None, 0, 0, None, None, ctypes.c_void_p(p.value + 2)) != 0 and b"4-byte aligned" in L.ccz_last_error()
    assert L.ccz_sample_records(None, p, 64, p, p, 4, 0, None, p, p, p, None, None, ctypes.c_void_p(p.value + 2)) != 0 and b"4-byte aligned" in L.ccz_last_error()
    assert L.ccz_expand_records(None, p, 0, 0, None, None, None, None, 0, 0, None, None, None) == 0      # no records: nothing to refuse


def test_record_ring_refuses_bad_arguments_without_a_device():
    from chinesechesszero_amd import _lib
    from chinesechesszero_amd.replay import REC_BYTES, RecordReplayBuffer
    with pytest.raises(ValueError):
        RecordReplayBuffer(4095, "cpu")                      # default max_game_plies = 2048: two games do not fit
    with pytest.raises(ValueError):
        RecordReplayBuffer(27, "cpu", max_game_plies=14)
    with pytest.raises(ValueError):
        RecordReplayBuffer(64, "cpu", max_game_plies=0)
    with pytest.raises(ValueError):
        RecordReplayBuffer(1 << 20, "cpu", max_game_plies=70000)
    with pytest.raises(ValueError):
        RecordReplayBuffer(64, "cpu", flags=_lib.FLAG_VALUE_F16, max_game_plies=14)
    with pytest.raises(ValueError):
        RecordReplayBuffer(64, "cpu", plane_of_type=(0, 1, 1, 2, 3, 4, 5, 6), max_game_plies=14)
    ring = RecordReplayBuffer(64, "cpu", flags=_lib.FLAG_NO_MIRROR, plane_of_type=(0, 6, 5, 4, 3, 2, 1, 0), max_game_plies=14)
    assert ring.cap == 64 and ring.mul == 1 and ring.size == ring.total == ring.head == 0 and ring.records.shape == (64, REC_BYTES)
    rec = torch.zeros((3, REC_BYTES), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ring.append_records(rec, 0)                          # mirror images on, the ring's are off
    with pytest.raises(ValueError):
        ring.append_records(rec, _lib.FLAG_NO_MIRROR, (0, 0, 1, 2, 3, 4, 5, 6))
    with pytest.raises(ValueError):
        ring.append_records(rec[:, :100])
    with pytest.raises(ValueError):
        ring.sample(8)                                       # nothing was ever appended
    with pytest.raises(ValueError):
        ring.sample_at(torch.zeros(8, dtype=torch.int64))
    assert ring.append_records(rec[:0]) == 0
    # None, all zero and the identity are one plane map
    assert RecordReplayBuffer._plane_map(None) is RecordReplayBuffer._plane_map((0,) * 8) is RecordReplayBuffer._plane_map(range(-1, 7)) is None


def test_replay_still_does_not_import_the_oracle():
    code = "import sys; import chinesechesszero_amd.replay as r; assert hasattr(r, 'RecordReplayBuffer'); " \
           "assert not [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')], 'oracle imported'"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]


def test_collector_command_line_takes_the_two_options(tmp_path):
    from chinesechesszero_amd.collect import CollectPipeline, build_parser
    from chinesechesszero_amd.parameters import BATCH_SIZE
    p = build_parser()
    d = p.parse_args([])
    assert d.replay_plies == 0 and d.train_every == 0 and d.train_batch == BATCH_SIZE and d.boards == 4096
    a = p.parse_args(["--replay-plies", "1000000", "--train-every", "8", "--boards", "64"])
    assert a.replay_plies == 1000000 and a.train_every == 8
    with pytest.raises(ValueError):      # one without the other is a mistake, as is the one-game-at-a-time path
        CollectPipeline(n_boards=64, replay_plies=4096, train_every=0, data_dir=str(tmp_path / "a"))
    with pytest.raises(ValueError):
        CollectPipeline(n_boards=1, replay_plies=4096, train_every=2, data_dir=str(tmp_path / "b"))
    assert not os.path.exists(tmp_path / "a") and not os.path.exists(tmp_path / "b")      # refused before anything is created
