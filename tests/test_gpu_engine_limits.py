"""GPU: the engine's sticky error paths (``CCZ_ERR_*``) against the limit-aware host twins, byte for byte.

Every case of tests/engine_limit_cases.py is one engine whose FAULTY boards run into one bounded resource of a hand-written kernel --
the node pool (bit 1), the path array (2), the arg-max over NaN scores (32), the pi arena (8), the forced-move input (16) -- among
CLEAN boards that never do. Device and twins are driven through ``drive()`` of tests/test_gpu_ref_twins.py, and every leaf, root,
move and status event is compared, the sticky word included: containment is the same comparison (a clean board matches a twin that
hit nothing), and the word is compared as a whole (one per engine). tests/test_cpu_engine_limits.py derives by hand what the twins
must show and asserts that every faulty board hits its limit. Each case runs twice: through ccz_select_leaves + ccz_expand_backup,
and through the fused ccz_step, whose prefetch and root patch differ.

Against the bounds-checked build (``make bounds``, ``CCZ_LIB``) the same file shows that no index left its array on the way:
bit 128 stays clear in every case.

Not covered, because no legal position reaches them: CCZ_ERR_CHAIN -- a history chain is never longer than the half-move clock plus
one, and a leaf at clock >= 120 is a draw that is not expanded, so no chain passes 121 of its 128 entries -- and CCZ_ERR_MOVES -- no
xiangqi position has more than 128 legal moves. Pruning re-roots, scouts, the planned and compact boundaries, resignation, root
exploration and the solver are off in every case; they are pinned by their own files."""
import functools

import numpy as np
import pytest
import torch

import engine_limit_cases as E
from engine_limit_cases import CASES
from test_gpu_ref_twins import Device, same

pytestmark = pytest.mark.gpu


class Dev(Device):
    """A NON-strict engine behind the twins' call surface: select_leaves + expand_backup, two launches per simulation."""

    def __init__(self, B, **kw):
        from chinesechesszero_amd.engine import SelfPlayEngine
        self.e = SelfPlayEngine(B, strict=False, **kw)
        self.B = B

    def reset_tree(self, mask):
        self.e.reset_tree(mask)

    def flags(self):
        return int(self.e.stats()["error_flags"])

    def close(self):
        self.e.close()


class Fused(Dev):
    """The fused form: expand_backup is ccz_step, whose selection is handed out by the next select_leaves. A move boundary drops it."""

    pending = None

    def select_leaves(self):
        if self.pending is None:
            return super().select_leaves()
        out, self.pending = self.pending, None
        return out

    def expand_backup(self, P, V):
        self.pending = self.e.step(torch.from_numpy(P).to(self.e.device), torch.from_numpy(V).to(self.e.device)).cpu().numpy()

    def finish_move(self, *a, **kw):
        self.pending = None
        return super().finish_move(*a, **kw)

    def reset_tree(self, mask):
        self.pending = None
        super().reset_tree(mask)


def packed(log):
    """The log with every leaf event's planes (0 / 1 floats) as bits: a case of 580 simulations a move stays small."""
    out = []
    for ev in log:
        if ev[0] == "leaf":
            assert np.isin(ev[1], (0.0, 1.0)).all()
            ev = ("leaf", np.packbits(ev[1] != 0), ev[2])
        out.append(ev)
    return out


@functools.lru_cache(maxsize=None)
def twin(name):
    log, usage, end = E.run_ref(CASES[name])
    return packed(log), usage, end


def run_device(case, form):
    """(log, stats, harvested rows) of the case on the device; the rows after everything else, since a harvest restarts the boards."""
    from chinesechesszero_amd._lib import CczError
    dev = (Fused if form == "fused" else Dev)(case["B"], **case["engine"])
    try:
        log, _ = E.run(dev, case, dev.flags)
        st = dev.e.stats()
        with pytest.raises(CczError, match=case["word"]):
            dev.e.check_healthy()
        rows = tuple(t.cpu().numpy() for t in dev.e.harvest()) if case.get("harvest") else None
        return packed(log), st, rows
    finally:
        dev.close()


@pytest.mark.parametrize("form", ["two_launches", "fused"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_and_limit_aware_twins_return_the_same_bytes(name, form):
    case = CASES[name]
    want, usage, end = twin(name)
    got, st, _ = run_device(case, form)
    assert len(got) == len(want)
    for i, (u, v) in enumerate(zip(got, want)):
        same(u, v, f"{name}/{form}: event {i} ({u[0]})")
    assert st["error_flags"] == case["flags"], st                     # the exact word: the case's bit and no other (128: no stray index)
    assert st["sims"] == end["sims"] and st["truncated_games"] == end["truncated_games"]
    cap = case["engine"].get("max_nodes", 0)
    if cap:
        assert st["nodes_peak"] <= cap
        assert st["nodes_peak"] == end["nodes_peak"]
    assert st["depth_peak"] <= (case["engine"].get("max_depth", 0) or 512) - 1
    assert st["pruned_subtrees"] == 0


@pytest.mark.parametrize("form", ["two_launches", "fused"])
def test_an_overflowed_record_keeps_the_rows_of_the_plies_before_it(form):
    """The harvest of the record case: the adjudicated boards yield their ply-0 rows, byte-equal to the ply-0 rows of an engine whose
    arena never overflowed -- the same engine with red's ply-0 move forced to the one with the fewest replies --, with z = 0."""
    from oracle import OracleBoard
    case = dict(CASES["record"], harvest=True)
    root = OracleBoard.from_array(*E.WIDE_PAIR)
    replies = {}
    for m in root.legal_ids():
        c = root.copy()
        c.push_id(m)
        if not c.is_game_over() and not c.is_tie():
            replies[m] = len(c.legal_ids())
    narrow = min(replies, key=replies.get)
    assert E.RECORD_K0 + replies[narrow] <= 160 and narrow != E.RECORD_FIRST
    calm = dict(case, forced={0: [narrow, narrow, -1, -1]}, flags=0, word=None)
    _, st, rows = run_device(case, form)
    dev = Dev(calm["B"], **calm["engine"])
    try:
        E.run(dev, calm, dev.flags)
        assert dev.flags() == 0
        dev.e.check_healthy()
        ref_rows = tuple(t.cpu().numpy() for t in dev.e.harvest())
    finally:
        dev.close()
    assert st["error_flags"] == 8
    # rows come game by game in board order, a game's plies and then their mirror images: boards 0 and 1 have one ply here and two there
    assert rows[0].shape[0] == 2 * (1 + 1 + 2 + 2) and ref_rows[0].shape[0] == 2 * (2 + 2 + 2 + 2)
    for a, r in zip(rows, ref_rows):
        for b in (0, 1):
            assert a[2 * b].tobytes() == r[4 * b].tobytes() and a[2 * b + 1].tobytes() == r[4 * b + 2].tobytes()
        assert a[4:].tobytes() == r[8:].tobytes()                      # the clean boards' games are the same games
    assert not rows[2].any() and rows[1][:4].sum(axis=1).tolist() == pytest.approx([1.0] * 4, abs=1e-6)
