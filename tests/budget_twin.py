"""Host twins of the device's per-move Philox draws (csrc/cczero_device.h ``uniform2``): the playout-cap lot (word 0xffe,
ccz_draw_budgets) and any other word of a board's stream for a move (0xffd: the play-on lot of ccz_set_resign). Shared by
tests/test_gpu_budgets.py and tests/selfplay_model.py."""
import ctypes as C

import numpy as np


def ua(seed, board_id, move_no, child=0xffe, draw=0):
    """uniform2's first uniform on the oracle's Philox."""
    import oracle
    o = (C.c_uint32 * 4)()
    lo = ((move_no << 32) | ((child & 0xfff) << 20) | (draw & 0xfffff)) & (2**64 - 1)
    oracle.lib().xq_philox4x32(C.c_uint64(seed), C.c_uint64(board_id), C.c_uint64(lo), o)
    return float(2 * (((o[0] << 32) | o[1]) >> 12) + 1) * 1.1102230246251565e-16


def twin_budgets(seed, base, n_boards, move_no, n_full, n_fast, p_full):
    """What ccz_draw_budgets draws for boards base .. base + n_boards - 1 that all stand at move counter ``move_no``."""
    return np.array([n_full if ua(seed, base + b, move_no) < p_full else n_fast for b in range(n_boards)], np.int32)
