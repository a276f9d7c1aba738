"""GPU: the one record -> row path (k_expand_records / k_sample_records writing rows, policy-target bytes and root values in one
launch) on HAND-BUILT records: no engine, no search. Everything is exact, no tolerance. The shapes are the smallest at which
this code can go wrong: games of 1, 3, 9 and 2 plies (9 exceeds the 8-deep history, 1 is the shortest game), k of 0, 1 and 128,
mixed REC_FAST / REC_VALUE flags, both turns, all three winners. That k_harvest forms the same rows is test_gpu_harvest.py's."""
import numpy as np
import pytest
import torch

from chinesechesszero_amd import _lib

pytestmark = pytest.mark.gpu

GAMES = (1, 3, 9, 2)          # plies per game
P = sum(GAMES)
FLAGS = [0, _lib.FLAG_NO_MIRROR, _lib.FLAG_REFERENCE_QUIRKS]
S16, S32, S8 = 0x5a5a, 7.0, 255   # sentinels: fp16 bits of the planes, pi / z / value, target byte


def _build_games(order=GAMES):
    """uint8 [P, 880]: the games of ``order`` back to back. A game's content depends on its length alone, not on where it lies."""
    out = []
    for gi, T in enumerate(order):
        rng = np.random.default_rng(1000 + T)
        rec = np.zeros((T, _lib.REC_BYTES), np.uint8)
        winner = {1: -1, 3: 1, 9: 0, 2: 1}[T]
        for t in range(T):
            rec[t, :90] = rng.integers(0, 15, 90)
            k = (0, 1, 128)[(t + T) % 3]
            fl = (_lib.REC_FAST if (t + T) % 2 else 0) | (_lib.REC_VALUE if (t + 2 * T) % 3 else 0) | (_lib.REC_RESIGNED if T == 3 else 0)
            if fl & _lib.REC_VALUE:
                rec[t, 92:96] = np.array([np.float32(-1.0 + 0.125 * ((5 * t + T) % 16))]).view(np.uint8)
            hdr = np.zeros(16, np.uint8)
            hdr[0:2] = np.array([t], np.uint16).view(np.uint8)
            hdr[2:4] = np.array([T], np.uint16).view(np.uint8)
            hdr[4] = np.array([winner], np.int8).view(np.uint8)[0]
            hdr[5], hdr[6], hdr[7] = t % 2 if T != 2 else 1 - t % 2, k, fl
            hdr[8:12] = np.array([40 + T], np.uint32).view(np.uint8)
            hdr[12:16] = np.array([gi], np.uint32).view(np.uint8)
            rec[t, 96:112] = hdr
            rec[t, 112:112 + 2 * k] = rng.choice(_lib.NMOVES, k, replace=False).astype(np.uint16).view(np.uint8)
            rec[t, 368:368 + 4 * k] = rng.random(k, dtype=np.float32).view(np.uint8)
        out.append(rec)
    return np.concatenate(out)


def _hdr(rec):
    return rec[:, 96:98].copy().view(np.uint16).ravel().astype(np.int64), rec[:, 98:100].copy().view(np.uint16).ravel().astype(np.int64)


def _side_of_headers(rec, mul):
    """numpy, from the headers alone: the target byte and root value of every dense row of a buffer of whole games (game at
    record f, T plies: the sample of ply t at row mul * f + t, its mirror image at mul * f + T + t)."""
    t, T = _hdr(rec)
    fl = rec[:, _lib.REC_FLAGS]
    v = np.where(fl & _lib.REC_VALUE, rec[:, 92:96].copy().view(np.float32).ravel(), np.float32("nan")).astype(np.float32)
    p = np.arange(len(t))
    tg, val = np.full(len(t) * mul, S8, np.uint8), np.full(len(t) * mul, np.float32(S32), np.float32)
    for q in range(mul):
        tg[mul * (p - t) + q * T + t] = 1 - (fl & _lib.REC_FAST)
        val[mul * (p - t) + q * T + t] = v
    assert (tg != S8).all() and not (val == S32).any()
    return tg, val


def _np(ts):
    return [x.cpu().numpy() if x.dtype != torch.float16 else x.view(torch.int16).cpu().numpy() for x in ts]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _sentinel_out(n, dev="cuda"):
    return (torch.full((n, 17, 7, 10, 9), S16, dtype=torch.int16, device=dev).view(torch.float16), torch.full((n, _lib.NMOVES), S32, device=dev),
            torch.full((n,), S32, device=dev), torch.full((n,), S8, dtype=torch.uint8, device=dev), torch.full((n,), S32, device=dev))


_FULL = {}


def _full(flags):
    """(records on the device, the five outputs of the fused expansion as numpy), computed once per flags and left unchanged."""
    if flags not in _FULL:
        from chinesechesszero_amd.engine import expand_records
        rec = torch.from_numpy(_build_games()).cuda()
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        _FULL[flags] = (rec, _np(expand_records(rec, flags, targets=True, values=True, bad=bad)))
        assert int(bad.item()) == 0
    return _FULL[flags]


def test_the_hand_built_records_cover_what_they_should():
    rec = _build_games()
    t, T = _hdr(rec)
    assert len(rec) == P and sorted(set(T)) == [1, 2, 3, 9]
    assert set(rec[:, 102]) == {0, 1, 128} and set(rec[:, 101]) == {0, 1} and set(rec[:, 100].view(np.int8)) == {-1, 0, 1}
    fl = rec[:, _lib.REC_FLAGS]
    assert {int(f) & 9 for f in fl} == {0, 1, 8, 9}
    _, v = _side_of_headers(rec, 1)
    assert np.isnan(v).any() and len(np.unique(v[~np.isnan(v)])) >= 3 and rec[:, :90].max() == 14


@pytest.mark.parametrize("flags", FLAGS)
def test_fused_expansion_agrees_with_the_plain_call_numpy_and_the_wrappers(flags):
    from chinesechesszero_amd.engine import expand_record_targets, expand_record_values, expand_records
    rec, full = _full(flags)
    mul = 1 if flags & _lib.FLAG_NO_MIRROR else 2
    plain = _np(expand_records(rec, flags))
    assert len(plain) == 3 and len(full) == 5 and all(_same(a, b) for a, b in zip(plain, full))
    assert full[0].shape == (P * mul, 17, 7, 10, 9) and set(np.unique(full[0])) == {0, 0x3c00}
    tg, val = _side_of_headers(rec.cpu().numpy(), mul)
    assert full[3].dtype == np.uint8 and full[4].dtype == np.float32 and _same(full[3], tg) and _same(full[4], val)
    assert _same(expand_record_targets(rec, flags).cpu().numpy(), tg) and _same(expand_record_values(rec, flags).cpu().numpy(), val)
    only_v = _np(expand_records(rec, flags, values=True))
    assert len(only_v) == 4 and _same(only_v[3], val)


def _game_rows(first, T, mul):
    return np.arange(mul * first, mul * (first + T))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("end", ["last", "first"])
def test_a_cut_game_at_either_end_keeps_its_rows_unwritten_and_gets_zero_and_nan(flags, end):
    from chinesechesszero_amd.engine import expand_record_targets, expand_record_values, expand_records
    mul = 1 if flags & _lib.FLAG_NO_MIRROR else 2
    _, full = _full(flags)
    where = dict(zip(GAMES, np.cumsum((0,) + GAMES[:-1])))            # first record of each game in the buffer of _full
    if end == "last":
        order, buf = GAMES, _build_games()[:-1]                       # the 2-ply game loses its last record
        cut_T, starts, present = GAMES[-1], np.cumsum((0,) + GAMES[:-1]), np.array([P - 2])
    else:
        order = (3, 9, 2, 1)
        buf = _build_games(order)[1:]                                 # the 3-ply game loses its first record: first < 0
        cut_T, starts, present = 3, np.cumsum((0,) + order[:-1]) - 1, np.array([0, 1])
    rec = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    n = len(buf) * mul
    out = _sentinel_out(n)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    expand_records(rec, flags, out=out, bad=bad)
    got = _np(out)
    cut_rows = (mul * present[:, None] + np.arange(mul)[None, :]).ravel()
    seen = np.zeros(n, bool)
    for T, f in zip(order, starts):
        if T == cut_T:
            continue
        rows, src = _game_rows(f, T, mul), _game_rows(where[T], T, mul)
        seen[rows] = True
        assert all(_same(g[rows], w[src]) for g, w in zip(got, full))
    seen[cut_rows] = True
    assert seen.all()
    assert (got[0][cut_rows] == S16).all() and (got[1][cut_rows] == S32).all() and (got[2][cut_rows] == S32).all()
    assert (got[3][cut_rows] == 0).all() and np.isnan(got[4][cut_rows]).all()
    assert int(bad.item()) == len(present)
    # the stand-alone wrappers give the same side outputs
    assert _same(expand_record_targets(rec, flags).cpu().numpy(), got[3]) and _same(expand_record_values(rec, flags).cpu().numpy(), got[4])


@pytest.mark.parametrize("flags", FLAGS)
def test_ring_placement_wraps_all_five_outputs_alike(flags):
    from chinesechesszero_amd.engine import expand_records
    rec, full = _full(flags)
    R = len(full[2])
    N, head = R + 3, R + 3 - 4
    out = _sentinel_out(N)
    res = expand_records(rec, flags, out=out, head_row=head)
    assert len(res) == 5 and all(a is b for a, b in zip(res, out))
    got = _np(out)
    at = (head + np.arange(R)) % N
    assert at.max() == N - 1 and at.min() == 0                         # the written block wraps
    rest = np.setdiff1d(np.arange(N), at)
    assert len(rest) == 3
    assert all(_same(g[at], w) for g, w in zip(got, full))
    assert (got[0][rest] == S16).all() and all((g[rest] == s).all() for g, s in zip(got[1:], (S32, S32, S8, S32)))


@pytest.mark.parametrize("flags", FLAGS)
def test_the_record_ring_serves_the_same_rows_bytes_and_values_across_its_physical_end(flags):
    from chinesechesszero_amd.engine import expand_records
    from chinesechesszero_amd.replay import RecordReplayBuffer
    mul = 1 if flags & _lib.FLAG_NO_MIRROR else 2
    cap = 2 * 9 + 1
    ring = RecordReplayBuffer(cap, "cuda", flags=flags, max_game_plies=9)
    games, lo = [], 0
    all_rec = _build_games()
    for T in GAMES:
        games.append(all_rec[lo:lo + T])
        lo += T
    fed, head = [], 0
    for g in games * 3:                                                # the four games, then again, until one wraps the physical end
        ring.append_records(torch.from_numpy(g).cuda())
        fed.append(g)
        wrapped = head // cap != (head + len(g) - 1) // cap
        head += len(g)
        if wrapped:
            break
    assert wrapped and len(fed[-1]) == 9
    tail, h = ring.window()
    assert h == head and head - tail < head and int(ring.bad.item()) == 0
    live = head - tail
    window = np.concatenate(fed)[tail:head]                            # whole games only
    t, T = _hdr(window)
    assert t[0] == 0 and (tail // cap) != ((head - 1) // cap)
    want = _np(expand_records(torch.from_numpy(np.ascontiguousarray(window)).cuda(), flags, targets=True, values=True))
    r = np.arange(mul * live)
    ply, pas = r // mul, r % mul
    rows = mul * (ply - t[ply]) + pas * T[ply] + t[ply]
    got = _np(ring.sample_at(torch.arange(mul * live, device="cuda"), targets=True, values=True))
    assert len(got) == 5 and all(_same(g, w[rows]) for g, w in zip(got, want))
    plain = _np(ring.sample_at(torch.arange(mul * live, device="cuda")))
    assert len(plain) == 3 and all(_same(a, b) for a, b in zip(plain, got))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _np(ring.sample_at(torch.tensor([0, -1, 1], device="cuda"), bad=bad, targets=True, values=True))
    assert all(_same(g[[0, 2]], w[rows[:2]]) for g, w in zip(got, want))
    assert not got[0][1].any() and not got[1][1].any() and got[2][1] == 0 and got[3][1] == 0 and np.isnan(got[4][1])
    assert int(bad.item()) == 1                                        # counted once, not once per output
