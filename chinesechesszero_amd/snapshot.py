"""Engine snapshots on the host: the blob's format constants and :func:`snapshot_info` (NumPy only: a file can be inspected
without a GPU). The blob is written by ``ccz_snapshot_save`` (``include/cczero.h`` "Engine snapshots",
``csrc/cczero_snapshot.h``); all little-endian::

    [0, 512)                  header (HEADER_DTYPE)
    [512, 512 + 8 (B + 1))    uint64 offsets[B + 1]: exclusive scan of the section sizes, offsets[B] = their sum
    then                      META_DTYPE meta[B] (40 bytes each)
    sections_start            = the above rounded up to 16; board b's section is
                              [sections_start + offsets[b], sections_start + offsets[b + 1])

A section: FIXED_BYTES of per-board rows (FIXED_ROWS), then ``nodeA [n_nodes][16]``, ``nodeB [n_nodes][4]``, ``proof [n_nodes]``
(with SNAP_PROOF), ``rec_sq [ply][96]``, ``rec_off [ply][4]``, ``rec_turn`` / ``rec_k`` / ``rec_target [ply]``, ``rec_value
[ply][4]`` and ``rec_hasv [ply]`` (with SNAP_VALUES), ``rec_kl [ply][4]``, ``rec_hask [ply]`` and the board's 24-byte surprise counter
row (with SNAP_SURPRISE: only while policy surprise weighting is on), ``rec_ids [pi_used][2]``, ``rec_pi [pi_used][4]``; every array is rounded up
to 16 bytes with zeros (:func:`section_bytes`).
"""
from __future__ import annotations

import numpy as np

MAGIC = 0x0050414E535A4343           # b"CCZSNAP\0"
VERSION = 1
HEADER_BYTES = 512
FIXED_BYTES = 5088
META_BYTES = 40
SNAP_PROOF, SNAP_VALUES, SNAP_SURPRISE = 1, 2, 4

_RESIGN = np.dtype([("enabled", "<i4"), ("consecutive", "<i4"), ("min_ply", "<i4"), ("threshold", "<f4"), ("p_playon", "<f8")])
_EXPLORE = np.dtype([("enabled", "<i4"), ("prune", "<i4"), ("eps", "<f8"), ("alpha", "<f8"), ("forced_k", "<f8")])
_GUMBEL = np.dtype([("enabled", "<i4"), ("n_sims", "<i4"), ("max_considered", "<i4"), ("pad", "<i4"), ("c_visit", "<f8"), ("c_scale", "<f8")])
_SEARCH = np.dtype([("enabled", "<i4"), ("fpu_mode", "<i4"), ("fpu_root_mode", "<i4"), ("pad", "<i4"), ("fpu_value", "<f8"),
                    ("fpu_root_value", "<f8"), ("c_base", "<f8"), ("c_factor", "<f8")])
_STOP = np.dtype([("enabled", "<i4"), ("single_reply", "<i4"), ("kld_interval", "<i4"), ("min_sims", "<i4"), ("n_sims", "<i4"), ("pad", "<i4"),
                  ("gap_factor", "<f8"), ("min_gain", "<f8")])
_SURPRISE = np.dtype([("enabled", "<i4"), ("pad", "<i4"), ("alpha", "<f8"), ("cap", "<f8")])   # (zeros while the option never was on)
SURPRISE_STATS_DTYPE = np.dtype([("target_plies", "<u8"), ("surprise_sum", "<f8"), ("weights_clipped", "<u8")])
HEADER_DTYPE = np.dtype([
    ("magic", "<u8"), ("version", "<u4"), ("header_bytes", "<u4"), ("total_bytes", "<u8"), ("sections_start", "<u8"),
    ("B", "<i4"), ("cap", "<i4"), ("maxd", "<i4"), ("max_plies", "<i4"), ("pi_cap", "<i4"), ("reserve", "<i4"),
    ("c_puct", "<f4"), ("flags", "<u4"), ("eps", "<f8"), ("alpha", "<f8"), ("temp", "<f8"), ("seed", "<u8"), ("board_id_base", "<u8"),
    ("rule_flags", "<u4"), ("chanpack", "<u4"), ("typepack", "<u4"), ("trankpack", "<u4"), ("rank_hash", "<u8"),
    ("sections", "<u4"), ("width", "<i4"), ("solver_enabled", "<i4"), ("budgets_on", "<i4"), ("err", "<i4"), ("half", "<i4"),
    ("fixed_bytes", "<u4"), ("meta_bytes", "<u4"),
    ("resign", _RESIGN), ("root_exploration", _EXPLORE), ("gumbel", _GUMBEL), ("search", _SEARCH), ("early_stop", _STOP),
    ("surprise", _SURPRISE), ("pad", "u1", (HEADER_BYTES - 360,))])
assert HEADER_DTYPE.itemsize == HEADER_BYTES
META_DTYPE = np.dtype([("key", "<u8"), ("halfmove", "<i4"), ("chain_len", "<i4"), ("ply", "<i4"), ("move_counter", "<u4"), ("n_nodes", "<i4"),
                       ("turn", "u1"), ("over", "u1"), ("winner", "i1"), ("half", "u1"), ("pi_used", "<u4"), ("game_no", "<u4")])
assert META_DTYPE.itemsize == META_BYTES

# the fixed rows of a section: name -> (byte offset, dtype, count); the per-board counter rows are raw bytes here
FIXED_ROWS = {
    "root_sq": (0, "u1", 96), "chain": (96, "<u8", 128), "chain_chk": (1120, "<u8", 2), "gm_g": (1136, "<f8", 128),
    "gm_logit": (2160, "<f8", 128), "gm_n0": (3184, "<i4", 128), "ex_dir": (3696, "<f4", 128), "es_snap": (4208, "<i4", 128),
    "gm_stamp": (4720, "<u4", 4), "stats": (4736, "u1", 104), "rs_stats": (4840, "u1", 56), "ex_stats": (4896, "u1", 32),
    "sv_stats": (4928, "u1", 16), "gm_stats": (4944, "u1", 24), "es_stats": (4968, "u1", 48), "wide_stats": (5016, "u1", 24),
    "ex_stamp": (5040, "<u4", 2), "budget": (5048, "<i4", 1), "move_sims": (5052, "<i4", 1), "rs_fire": (5056, "<i4", 1),
    "rs_last": (5060, "<f4", 1), "es_snap_s": (5064, "<i4", 1), "target": (5068, "u1", 1), "rs_state": (5069, "u1", 1),
    "rs_run": (5070, "u1", 2), "es_stopped": (5072, "u1", 1),
}


def pad16(n):
    return (np.asarray(n, dtype=np.uint64) + np.uint64(15)) & ~np.uint64(15)


def section_bytes(n_nodes, ply, pi_used, sections: int = SNAP_VALUES):
    """Bytes of a board's section from its counts (scalars or arrays; uint64): the documented formula of ``ccz_snapshot_layout``."""
    n = np.asarray(n_nodes).clip(min=0).astype(np.uint64)
    p = np.asarray(ply).clip(min=0).astype(np.uint64)
    u = np.asarray(pi_used).astype(np.uint64)
    c = np.uint64
    s = c(FIXED_BYTES) + n * c(16) + pad16(n * c(4))
    if sections & SNAP_PROOF:
        s = s + pad16(n)
    s = s + p * c(96) + pad16(p * c(4)) + c(3) * pad16(p)
    if sections & SNAP_VALUES:
        s = s + pad16(p * c(4)) + pad16(p)
    if sections & SNAP_SURPRISE:
        s = s + pad16(p * c(4)) + pad16(p) + pad16(c(SURPRISE_STATS_DTYPE.itemsize))
    return s + pad16(u * c(2)) + pad16(u * c(4))


def directory_bytes(B: int) -> int:
    return (int(B) + 1) * 8 + int(B) * META_BYTES


def sections_start(B: int) -> int:
    return (HEADER_BYTES + directory_bytes(B) + 15) & ~15


def _as_bytes(blob) -> np.ndarray:
    if isinstance(blob, str) or hasattr(blob, "__fspath__"):
        import torch
        blob = torch.load(blob, map_location="cpu")
    if isinstance(blob, (bytes, bytearray, memoryview)):
        return np.frombuffer(blob, dtype=np.uint8)
    if hasattr(blob, "detach"):                       # a torch tensor, wherever it lives
        blob = blob.detach().cpu().contiguous().view(-1).numpy()
    a = np.ascontiguousarray(blob)
    if a.dtype != np.uint8:
        raise TypeError("an engine snapshot is a uint8 blob")
    return a.reshape(-1)


def snapshot_info(blob) -> dict:
    """The header fields, the per-board ``n_nodes`` / ``ply`` / ``pi_used`` (and the whole ``meta`` record array), the section
    offsets and sizes of a snapshot: a uint8 tensor or array, bytes, or the path of a ``torch.save``d tensor. Parsed on the host.
    Raises ValueError on a blob that is no snapshot or is shorter than its header says."""
    a = _as_bytes(blob)
    if a.size < HEADER_BYTES:
        raise ValueError(f"truncated: {a.size} bytes are less than the header's {HEADER_BYTES}")
    h = a[:HEADER_BYTES].view(HEADER_DTYPE)[0]
    if int(h["magic"]) != MAGIC:
        raise ValueError(f"bad magic 0x{int(h['magic']):016x} (not an engine snapshot)")
    if int(h["version"]) != VERSION:
        raise ValueError(f"format version {int(h['version'])}, this module reads {VERSION}")
    B = int(h["B"])
    start = sections_start(B)
    if B < 1 or a.size < start:
        raise ValueError(f"truncated: {a.size} bytes do not hold the directory of {B} boards")
    off = a[HEADER_BYTES:HEADER_BYTES + 8 * (B + 1)].view("<u8").copy()
    meta = a[HEADER_BYTES + 8 * (B + 1):HEADER_BYTES + directory_bytes(B)].view(META_DTYPE).copy()
    out = {}
    for name in HEADER_DTYPE.names:
        if name == "pad":
            continue
        v = h[name]
        out[name] = {f: v[f].item() for f in v.dtype.names if f != "pad"} if v.dtype.names else v.item()
    out.update(offsets=off, meta=meta, n_nodes=meta["n_nodes"].copy(), ply=meta["ply"].copy(), pi_used=meta["pi_used"].copy(),
               over=meta["over"].copy(), section_sizes=np.diff(off), directory_bytes=directory_bytes(B), bytes=int(a.size))
    return out


def fixed_row(blob, info: dict, board: int, name: str) -> np.ndarray:
    """Row ``name`` (FIXED_ROWS) of board ``board``'s section, as a copy."""
    a = _as_bytes(blob)
    o, dt, n = FIXED_ROWS[name]
    p = int(info["sections_start"]) + int(info["offsets"][board]) + o
    return a[p:p + n * np.dtype(dt).itemsize].view(dt).copy()


def surprise_rows(blob, info: dict, board: int):
    """``(kl float32 [ply], has uint8 [ply], counters)`` of board ``board``'s section in a snapshot with SNAP_SURPRISE (ValueError without):
    the surprise stored with the plies of its game and its ``SURPRISE_STATS_DTYPE`` counter row, as copies."""
    sections = int(info["sections"])
    if not sections & SNAP_SURPRISE:
        raise ValueError("the snapshot has no surprise section (policy surprise weighting was off when it was saved)")
    a = _as_bytes(blob)
    n, ply = int(info["n_nodes"][board]), int(info["ply"][board])
    before = section_bytes(n, ply, 0, sections & ~SNAP_SURPRISE)          # (pi_used = 0: the arrays behind the surprise section left out)
    p = int(info["sections_start"]) + int(info["offsets"][board]) + int(before)
    kl = a[p:p + 4 * ply].view("<f4").copy()
    p += int(pad16(4 * ply))
    has = a[p:p + ply].copy()
    p += int(pad16(ply))
    return kl, has, a[p:p + SURPRISE_STATS_DTYPE.itemsize].view(SURPRISE_STATS_DTYPE)[0].copy()
