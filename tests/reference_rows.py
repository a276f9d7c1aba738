"""Default-mode training rows as the reference's own per-ply histories give them (tests/golden/reference_rows.{npz,json}, written by
tests/golden/make_golden_game.py while the reference's Game.start_self_play runs): the expectation every path that forms rows is held
to -- the host mirror, k_harvest, k_harvest_records + k_expand_records, the record ring.

``expected_rows`` only ASSEMBLES stored arrays: history planes are the snapshots of the reference's red_states / black_states, plane 16
is the snapshotted side to move, the mirror pi is what the reference's flip_data returned, mirror states are the planes reversed along
their last axis (the generator asserts that this is what flip_data does). No history is recomputed from positions by an index rule:
that rule is what is under test."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def load():
    """(arrays of reference_rows.npz, its json). Loaded once; treat as read-only."""
    if "fx" not in _cache:
        with np.load(os.path.join(GOLDEN, "reference_rows.npz"), allow_pickle=False) as f:
            arrays = {k: f[k] for k in f.files}
        for a in arrays.values():
            a.setflags(write=False)
        with open(os.path.join(GOLDEN, "reference_rows.json")) as f:
            meta = json.load(f)
        _cache["fx"] = (arrays, meta)
    return _cache["fx"]


def game_arrays(g):
    arrays, _ = load()
    return {k: arrays[f"g{g}_{k}"] for k in ("hist", "turn", "moves", "pi", "z", "pi_mirror")}


def expected_rows(g):
    """Game ``g`` of the fixture -> (states fp16 [2T,17,7,10,9], pi f64 [2T,2086], z f32 [2T]): the T plies, then their T mirror images
    (collect.py:112-131: data + data_flip). Built once per game and shared; read-only."""
    if ("rows", g) not in _cache:
        a = game_arrays(g)
        T = a["hist"].shape[0]
        st = np.empty((T, 17, 7, 10, 9), np.float16)
        st[:, :16] = a["hist"]
        st[:, 16] = a["turn"].astype(np.float16)[:, None, None, None]
        states = np.concatenate((st, st[..., ::-1]))
        pi = np.concatenate((a["pi"], a["pi_mirror"]))
        z = np.concatenate((a["z"], a["z"])).astype(np.float32)
        for x in (states, pi, z):
            x.setflags(write=False)
        _cache["rows", g] = (states, pi, z)
    return _cache["rows", g]


def _where(row, T):
    return f"ply {row % T}{' (mirror image)' if row >= T else ''}"


def compare_rows(got, want, pi_atol=None, label=""):
    """``got`` = (states, pi, z) of ONE game, 2T rows, against ``want`` = :func:`expected_rows`. States and z must be equal element for
    element (and fp16 / float32); pi bit for bit as float64 when ``pi_atol`` is None, else within ``pi_atol`` of the float64 reference with
    no mass outside its support. Raises AssertionError naming the first differing (ply, mirror, plane); returns the largest pi deviation."""
    gs, gp, gz = (np.asarray(x) for x in got)
    ws, wp, wz = want
    T = ws.shape[0] // 2
    assert gs.shape == ws.shape and gs.dtype == np.float16, f"{label}: states {gs.shape} {gs.dtype}, want {ws.shape} float16"
    assert gp.shape == wp.shape and gz.shape == wz.shape, f"{label}: pi {gp.shape} z {gz.shape}, want {wp.shape} {wz.shape}"
    bad = np.flatnonzero((gs.view(np.uint16).reshape(2 * T, 17, -1) != ws.view(np.uint16).reshape(2 * T, 17, -1)).any(axis=2).ravel())
    if bad.size:
        row, plane = divmod(int(bad[0]), 17)
        what = "turn plane" if plane == 16 else f"{'red' if plane < 8 else 'black'} history slot {plane & 7}"
        raise AssertionError(f"{label}: states differ first at {_where(row, T)}, plane {plane} ({what}); {bad.size} planes differ in all")
    zbad = np.flatnonzero(gz.astype(np.float64) != wz.astype(np.float64))
    if zbad.size or gz.dtype != wz.dtype:
        raise AssertionError(f"{label}: z differs first at {_where(int(zbad[0]), T)}: {gz[zbad[0]]} for {wz[zbad[0]]}; {zbad.size} rows"
                             if zbad.size else f"{label}: z is {gz.dtype}, want {wz.dtype}")
    dev = np.abs(gp.astype(np.float64) - wp)
    if pi_atol is None:
        same = gp.dtype == np.float64 and np.array_equal(gp.view(np.uint64), wp.view(np.uint64))
        if not same:
            rows = np.flatnonzero((gp != wp).any(axis=1)) if gp.dtype == np.float64 else np.arange(1)
            raise AssertionError(f"{label}: pi ({gp.dtype}) is not the reference's float64 bit for bit, first at {_where(int(rows[0]), T)}, "
                                 f"largest deviation {dev.max():.3e}")
    else:
        rows = np.flatnonzero((dev > pi_atol).any(axis=1) | ((gp != 0) & (wp == 0)).any(axis=1))
        if rows.size:
            r = int(rows[0])
            raise AssertionError(f"{label}: pi differs first at {_where(r, T)}: deviation {dev[r].max():.3e} at move {int(dev[r].argmax())}, "
                                 f"{int(((gp[r] != 0) & (wp[r] == 0)).sum())} entries outside the support; {rows.size} rows differ")
    return float(dev.max())
