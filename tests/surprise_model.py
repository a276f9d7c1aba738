"""CPU model of policy surprise weighting (ccz_set_surprise / ccz_sample_records_weighted, include/cczero.h): the
surprise of a ply, the weight of a ply in its game, the weight bytes of the harvested records, and the rejection draw of the replay ring.

Plain Python + NumPy. The search, pi and the records come from tests/selfplay_model.py and tests/gumbel_model.py (``with_surprise`` wraps
either model class: the surprise is computed from what the model records, ``pi64``, and the priors of the root it recorded it at); log from
the oracle's ``xq_det_log`` (gumbel_model.det_log), Philox from the oracle's ``xq_philox4x32`` (the twin tests/budget_twin.py uses).
Restated here, in Python floats (IEEE float64, no contraction) with every sum in order, is only what the header says of the feature."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from explore_model import F32
from gumbel_model import det_log

REC_BYTES, HDR, FLAGS, WEIGHT_OFF = 880, 96, 103, 90
REC_WEIGHT, ONE = 16, 4096
TINY = 2.0 ** -100
MAX_LEGAL = 128


# ---------------------------------------------------------------------------------------------------------------- the surprise of a ply
def surprise_of(pi64, priors) -> np.float32:
    """(float)s, s = sum_i pi_i (log pi_i - log max(P_i, 2^-100)) over pi_i > 0 in child order, a negative sum clamped to 0."""
    s = 0.0
    for p, q in zip(pi64, priors):
        p = float(p)
        if p > 0.0:
            s = s + p * (det_log(p) - det_log(max(float(F32(q)), TINY)))
    return F32(s if s > 0.0 else 0.0)


# ---------------------------------------------------------------------------------------------------------------- the weight of a ply
def game_weights(kl, has, alpha, cap):
    """(wq uint16 [T], plies clipped) of one game: ``kl`` float32 [T] as stored, ``has`` [T] which plies carry one."""
    S, n = 0.0, 0
    for s, h in zip(kl, has):
        if h:
            S = S + float(F32(s))
            n += 1
    wq, clipped = [], 0
    for s, h in zip(kl, has):
        w = 1.0
        if h and S > 0.0:
            w = (1.0 - alpha) + alpha * float(n) * float(F32(s)) / S
        if w > cap:
            w = cap
            clipped += 1
        wq.append(int(math.floor(w * 4096.0 + 0.5)))
    return np.array(wq, np.uint16), clipped


def weights_of(records: np.ndarray) -> np.ndarray:
    """float32 [P]: what replay.record_weights says of records (uint8 [P, 880])."""
    wq = records[:, WEIGHT_OFF:WEIGHT_OFF + 2].copy().view(np.uint16)[:, 0]
    return np.where(records[:, FLAGS] & REC_WEIGHT, wq.astype(np.float32) / np.float32(ONE), np.float32(1.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- a self-play model with it
def with_surprise(base):
    """``base`` (SelfPlayModel or GumbelModel) with ``surprise=dict(alpha, cap)`` (None: off, the base as it is)."""

    class SurpriseModel(base):
        def __init__(self, *a, surprise=None, **kw):
            super().__init__(*a, **kw)
            self.scfg = None if surprise is None else dict(surprise)
            self.kl = [[] for _ in range(self.B)]          # per board: (float32 surprise, has) of every recorded ply of its game
            self.sboard = [[0, 0.0, 0] for _ in range(self.B)]   # per board: target plies, sum, clipped

        def finish_move(self, forced=None):
            priors = [np.array([c.P for c in (self.roots[b].kids or [])], F32) for b in range(self.B)]
            targets = [int(t) for t in self.targets]
            events = super().finish_move(forced)
            if self.scfg is None:
                return events
            for b in range(self.B):
                rec = self.last[b]
                if rec is None:                            # no game, or adjudicated at the ply cap: nothing was recorded
                    continue
                if targets[b]:
                    s = surprise_of(rec["pi64"], priors[b])
                    self.kl[b].append((s, 1))
                    self.sboard[b][0] += 1
                    self.sboard[b][1] = self.sboard[b][1] + float(s)
                else:
                    self.kl[b].append((F32(0.0), 0))
            return events

        def ply_surprise(self, b):
            """(kl float32 [plies], has uint8 [plies]) of board b's game so far."""
            return np.array([s for s, _ in self.kl[b]], F32), np.array([h for _, h in self.kl[b]], np.uint8)

        def records(self, game_no=0):
            rec = super().records(game_no)
            if self.scfg is None:
                return rec
            i = 0
            for b in range(self.B):
                if not self.games[b].over or not self.plies_rec[b]:
                    continue
                T = len(self.plies_rec[b])
                kl, has = self.ply_surprise(b)
                assert len(kl) == T
                wq, clipped = game_weights(kl, has, self.scfg["alpha"], self.scfg["cap"])
                self.sboard[b][2] = clipped            # (a board of the model plays one game)
                rec[i:i + T, WEIGHT_OFF:WEIGHT_OFF + 2] = wq.view(np.uint8).reshape(T, 2)
                rec[i:i + T, FLAGS] |= REC_WEIGHT
                i += T
            assert i == len(rec)
            return rec

        def surprise_stats(self):
            """ccz_get_surprise_stats: the boards summed in board order."""
            total = 0.0
            for _, s, _ in self.sboard:
                total = total + s
            return {"target_plies": sum(x[0] for x in self.sboard), "surprise_sum": total, "weights_clipped": sum(x[2] for x in self.sboard)}

    return SurpriseModel


# ---------------------------------------------------------------------------------------------------------------- the rejection draw
def philox(key, hi, lo):
    import oracle
    o = (C.c_uint32 * 4)()
    oracle.lib().xq_philox4x32(C.c_uint64(key & (2**64 - 1)), C.c_uint64(hi), C.c_uint64(lo), o)
    return [int(x) for x in o]


def candidate(seed, j, r, lane):
    """(u, a) of candidate (r, lane) of output row j: a 62-bit draw and a uniform in [0, 1)."""
    o = philox(seed, j, 64 * r + lane)
    return ((o[0] << 32) | o[1]) >> 2, float(((o[2] << 32) | o[3]) >> 11) * 2.0 ** -53


def locate(ring, cap_plies, tail, head, u, mul):
    """locate_sampled_ply: (ok, logical ply, pass, wq) of draw u in the window [tail, head) of ``ring`` (uint8 [cap_plies, 880])."""
    if not (tail >= 0 and head > tail and head - tail <= cap_plies and u >= 0):
        return False, None, None, ONE
    r = u % ((head - tail) * mul)
    p, q = tail + r // mul, r % mul
    rec = ring[p % cap_plies]
    t, T = (int(x) for x in rec[HDR:HDR + 4].copy().view(np.uint16))
    first = p - t
    ok = t < T and int(rec[HDR + 6]) <= MAX_LEGAL and first >= tail and first + T <= head
    wq = int(rec[WEIGHT_OFF:WEIGHT_OFF + 2].copy().view(np.uint16)[0]) if (ok and rec[FLAGS] & REC_WEIGHT) else ONE
    return ok, p, q, wq


def weighted_draw(ring, cap_plies, tail, head, seed, j, cap_q, mul=2):
    """(u, fell back, bad) of output row j: the first accepted candidate in (round, lane) order of 4 x 64, else candidate (0, 0)."""
    for r in range(4):
        for lane in range(64):
            u, a = candidate(seed, j, r, lane)
            ok, _, _, wq = locate(ring, cap_plies, tail, head, u, mul)
            if ok and a * float(cap_q) < float(wq):
                return u, False, False
    u, _ = candidate(seed, j, 0, 0)
    return u, True, not locate(ring, cap_plies, tail, head, u, mul)[0]


# ---------------------------------------------------------------------------------------------------------------- hand-built records
def hand_game(T, weights, board_id, game_no=1, winner=1, k=3, squares=None):
    """uint8 [T, 880]: a game of T plies with the given weights (a list of T floats; None: records without REC_WEIGHT). Positions: the
    opening with one piece code moved along per ply (any bytes form a row); pi: k entries on ids t, t + 1, .."""
    if squares is None:
        from oracle import OracleBoard
        squares = OracleBoard().squares()
    rec = np.zeros((T, REC_BYTES), np.uint8)
    for t in range(T):
        sq = np.array(squares, np.uint8).copy()
        sq[(36 + t) % 90] = 1 + (t + board_id) % 14
        rec[t, :90] = sq
        rec[t, 92:96] = np.frombuffer(np.float32(0.125 * (t % 7) - 0.25).tobytes(), np.uint8)
        rec[t, HDR:HDR + 4] = np.array([t, T], np.uint16).view(np.uint8)
        rec[t, HDR + 4] = np.array([winner], np.int8).view(np.uint8)[0]
        rec[t, HDR + 5], rec[t, HDR + 6] = t & 1, k
        rec[t, FLAGS] = 8 | (t % 3 == 2) | (REC_WEIGHT if weights is not None else 0)
        rec[t, HDR + 8:HDR + 12] = np.array([board_id], np.uint32).view(np.uint8)
        rec[t, HDR + 12:HDR + 16] = np.array([game_no], np.uint32).view(np.uint8)
        rec[t, 112:112 + 2 * k] = (np.arange(k, dtype=np.uint16) + 7 * t + board_id).view(np.uint8)
        pi = np.arange(1, k + 1, dtype=np.float32)
        rec[t, 368:368 + 4 * k] = (pi / pi.sum()).astype(np.float32).view(np.uint8)
        if weights is not None:
            rec[t, WEIGHT_OFF:WEIGHT_OFF + 2] = np.array([int(math.floor(weights[t] * 4096.0 + 0.5))], np.uint16).view(np.uint8)
    return rec
