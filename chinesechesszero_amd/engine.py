"""SelfPlayEngine -- thin Python handle on the gfx950 lockstep engine (libcczero.so).

B boards advance in lockstep; one simulation of every board is
``select_leaves() -> evaluator (PyTorch-ROCm, same stream) -> expand_backup()`` and one move is
``finish_move()``. PyTorch is only used for device memory and the stream.
Replaces, for all boards at once, reference mcts.py:101-178 + the cchess calls of SURVEY a17.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import MAX_LEGAL, NMOVES, SQ_STRIDE, CczError, Config, Stats, check


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return C.c_void_p(t.data_ptr())
    if isinstance(t, np.ndarray):
        return C.c_void_p(t.ctypes.data)
    raise TypeError(type(t))


class SelfPlayEngine:
    def __init__(self, n_boards: int, n_playout: int = 400, c_puct: float = 5, eps: float = 0.25,
                 alpha: float = 0.2, temp: float = 1.0, seed: int = 0, board_id_base: int = 0,
                 device: int = 0, max_nodes: int = 0, max_depth: int = 0, max_plies: int = 0,
                 reference_quirks: bool = False, mirror: bool = True, reserve_nodes: int = 0,
                 move_rank="tools", plane_of_type="tools", value_f16: bool = False, type_rank="tools",
                 pawn_move_resets_clock="tools", perpetual_check="tools", eval_cache_log2: int = 0,
                 cache_verify: bool = False, strict: bool = False):
        """``move_rank`` (uint16[2086] permutation, None = ascending id) and ``plane_of_type`` (8 entries, None = type-1)
        are the run-time rule tables of ``ccz_config`` (ABI 2); the default "tools" takes the process-wide choice of
        :func:`chinesechesszero_amd.tools.set_rules`. ``eval_cache_log2`` = n > 0: an evaluation cache of 2^n positions
        (528 B each) for the planned evaluator boundary (:meth:`eval_plan`, ``include/cczero.h`` ccz_eval_plan);
        ``cache_verify``: its debug mode (CCZ_FLAG_CACHE_VERIFY): one hit in 128 is evaluated again and compared bit for bit
        (``stats()['cache_verified']`` / ``['cache_verify_mismatches']``). ``strict`` (CCZ_FLAG_STRICT): parity mode -- a kept
        subtree pruned to fit the node pool and a game adjudicated at ``max_plies`` (the reference knows neither: mcts.py:31-39,
        game.py:155) set sticky error bits that :meth:`check_healthy` raises on, instead of only moving ``pruned_subtrees`` /
        ``truncated_games``."""
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise CczError("no GPU visible to PyTorch-ROCm; the engine has no CPU fallback")
        self.device = torch.device("cuda", device)
        self.B = int(n_boards)
        self.n_playout = int(n_playout)
        self.alpha = float(np.float32(alpha))   # the sampler's Dirichlet alpha as ccz_config carries it (float32): the default of set_root_exploration
        flags = (_lib.FLAG_REFERENCE_QUIRKS if reference_quirks else 0) | (0 if mirror else _lib.FLAG_NO_MIRROR) \
            | (_lib.FLAG_VALUE_F16 if value_f16 else 0) | (_lib.FLAG_CACHE_VERIFY if cache_verify else 0) | (_lib.FLAG_STRICT if strict else 0)
        self.strict = bool(strict)
        # value_f16: Q accumulated in float16 as on the reference's CUDA path
        self.mirror = mirror
        self.reference_quirks = bool(reference_quirks)
        self.max_plies = int(max_plies) if int(max_plies) > 0 else 2048  # recorded plies per game (ccz_config.max_plies)
        from . import tools
        if isinstance(move_rank, str):
            move_rank = tools.MOVE_RANK
        if isinstance(plane_of_type, str):
            plane_of_type = tools.PLANE_OF_TYPE
        if isinstance(type_rank, str):
            type_rank = tools.TYPE_RANK
        cfg = Config(n_boards=self.B, n_playout=self.n_playout, c_puct=float(c_puct), eps=float(eps),
                     alpha=float(alpha), temp=float(temp), max_nodes=int(max_nodes), max_depth=int(max_depth),
                     max_plies=int(max_plies), flags=flags, seed=int(seed) & (2**64 - 1),
                     board_id_base=int(board_id_base), device=int(device), reserve_nodes=int(reserve_nodes))
        self.move_rank = None if move_rank is None else np.ascontiguousarray(move_rank, dtype=np.uint16)
        if self.move_rank is not None:
            if self.move_rank.shape != (NMOVES,):
                raise ValueError("move_rank must have 2086 entries")
            cfg.move_rank_host = self.move_rank.ctypes.data
        self.plane_of_type = (0, 0, 1, 2, 3, 4, 5, 6) if plane_of_type is None else tuple(int(x) for x in plane_of_type)
        if plane_of_type is not None:
            cfg.plane_of_type = (C.c_uint8 * 8)(*self.plane_of_type)
        if isinstance(pawn_move_resets_clock, str):
            pawn_move_resets_clock = tools.PAWN_MOVE_RESETS_CLOCK
        self.pawn_move_resets_clock = bool(pawn_move_resets_clock)
        if isinstance(perpetual_check, str):
            perpetual_check = tools.PERPETUAL_CHECK
        self.perpetual_check = bool(perpetual_check)
        cfg.rule_flags = (_lib.RULE_PAWN_MOVE_RESETS_CLOCK if self.pawn_move_resets_clock else 0) \
            | (_lib.RULE_PERPETUAL_CHECK if self.perpetual_check else 0)
        self.type_rank = None if type_rank is None else tuple(int(x) for x in type_rank)
        if self.type_rank is not None:
            if len(self.type_rank) != 8:
                raise ValueError("type_rank must have 8 entries")
            cfg.type_rank = (C.c_uint8 * 8)(*self.type_rank)
        self.eval_cache_log2 = int(eval_cache_log2)
        cfg.eval_cache_log2 = self.eval_cache_log2
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.L.ccz_create(C.byref(cfg), C.byref(h)))
        self.h = h
        # the evaluation plan of the current step (planned evaluator boundary): rows the evaluator has to compute, their number
        self.miss_rows = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.n_miss = torch.zeros((1,), dtype=torch.int32, device=self.device)
        # torch-owned boundary buffers (evaluator input / outputs, move buffers)
        self.leaf_input = torch.zeros((self.B, 17, 7, 10, 9), dtype=torch.float16, device=self.device)
        self.leaf_history = False   # set_leaf_history: the host's shadow of the engine's setting, and a counter of its changes
        self.history_version = 0
        self.moves_out = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
        self._forced = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
        self.budgets_out = torch.zeros((self.B,), dtype=torch.int32, device=self.device)   # what draw_budgets drew last
        self._temps = torch.ones((self.B,), dtype=torch.float64, device=self.device)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.ccz_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ games
    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        check(self.L.ccz_reset(self.h, self._stream(), _ptr(m)))

    def reset_tree(self, mask=None):
        """Fresh root on the masked boards (all if None); position, history and game record stay (mcts.py:176-178)."""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        check(self.L.ccz_reset_tree(self.h, self._stream(), _ptr(m)))

    def set_position(self, board: int, squares, turn: int, halfmove: int = 0):
        sq = np.ascontiguousarray(squares, dtype=np.uint8)
        assert sq.shape == (90,)
        check(self.L.ccz_set_position(self.h, self._stream(), int(board), _ptr(sq), int(turn), int(halfmove)))

    def set_positions(self, squares, turn, halfmove=None, moves=None, park=None, mask=None) -> np.ndarray:
        """Load all boards in ONE launch, each with the moves that led to its position (``ccz_set_positions``: validated and
        replayed on the device with the engine's own rules; history chain, clocks and game end as after as many
        :meth:`finish_move` calls). ``squares`` uint8 [B,90] (or [B,96]), ``turn`` [B] (1 red), ``halfmove`` [B] or None,
        ``moves``: a list of B move-id lists or a padded int array [B,M] whose unused entries are negative, ``park`` [B]: boards
        to park (no game: the simulator skips them), ``mask`` [B]: boards to touch (None = all). Returns the status int32 [B]:
        0 loaded (or parked on request), 1 + i move i is illegal where it is played, -1 invalid position, -2 history chain
        overflow; a board with a non-zero status is parked. Syncs once, for the status."""
        B = self.B
        sq = np.asarray(squares, dtype=np.uint8)
        if sq.ndim != 2 or sq.shape[0] != B or sq.shape[1] not in (90, SQ_STRIDE):
            raise ValueError(f"squares must be [{B},90]")
        sq96 = np.zeros((B, SQ_STRIDE), np.uint8)
        sq96[:, :90] = sq[:, :90]
        tn = np.array(np.broadcast_to(np.asarray(turn), (B,)), dtype=np.uint8)          # (a copy: broadcasts are read-only)
        n = np.zeros(B, np.int32)
        mv = None
        if moves is not None:
            if isinstance(moves, np.ndarray) and moves.ndim == 2:
                if moves.shape[0] != B:
                    raise ValueError(f"moves must have {B} rows")
                mv = np.ascontiguousarray(moves, dtype=np.int32)
                n = (mv >= 0).sum(axis=1).astype(np.int32)
                if ((mv >= 0) != (np.arange(mv.shape[1])[None, :] < n[:, None])).any():
                    raise ValueError("moves: the unused (negative) entries of a padded row must follow its moves")
            else:
                if len(moves) != B:
                    raise ValueError(f"moves must have {B} rows")
                n = np.array([len(r) for r in moves], np.int32)
                mv = np.full((B, max(1, int(n.max()) if B else 1)), -1, np.int32)
                for b, r in enumerate(moves):
                    mv[b, :len(r)] = np.asarray(r, np.int32)
        if park is not None:
            n = np.where(np.asarray(park, bool), np.int32(-1), n).astype(np.int32)
        dev = self.device
        d_sq = torch.from_numpy(sq96).to(dev)
        d_turn = torch.from_numpy(tn).to(dev)
        d_half = None if halfmove is None else torch.from_numpy(np.array(np.broadcast_to(np.asarray(halfmove), (B,)), dtype=np.int32)).to(dev)
        d_mv = None if mv is None else torch.from_numpy(mv).to(dev)
        d_n = None if (mv is None and park is None) else torch.from_numpy(n).to(dev)
        status = torch.zeros((B,), dtype=torch.int32, device=dev)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        check(self.L.ccz_set_positions(self.h, self._stream(), _ptr(d_sq), _ptr(d_turn), _ptr(d_half), _ptr(d_mv), _ptr(d_n),
                                       0 if mv is None else int(mv.shape[1]), _ptr(m), _ptr(status)))
        return status.cpu().numpy()

    # ------------------------------------------------------------------ one simulation
    def select_leaves(self) -> torch.Tensor:
        """PUCT descent + leaf rules + evaluator input for all boards; returns [B,17,7,10,9] fp16."""
        check(self.L.ccz_select_leaves(self.h, self._stream(), _ptr(self.leaf_input)))
        return self.leaf_input

    def expand_backup(self, prob: torch.Tensor, value: torch.Tensor):
        """prob float32 [B,2086] (= exp(log_act_probs)), value float32 [B]."""
        if prob.dtype != torch.float32 or value.dtype != torch.float32:
            raise TypeError("prob and value must be float32")
        if tuple(prob.shape) != (self.B, NMOVES) or value.numel() != self.B:
            raise ValueError(f"prob must be [{self.B},{NMOVES}] and value [{self.B}]")
        if not (prob.is_cuda and value.is_cuda and prob.is_contiguous() and value.is_contiguous()):
            raise ValueError("prob/value must be contiguous device tensors")
        check(self.L.ccz_expand_backup(self.h, self._stream(), _ptr(prob), _ptr(value)))

    def step(self, prob: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
        """Fused expand_backup(prob, value) for the pending leaf + select_leaves() for the next simulation."""
        if prob.dtype != torch.float32 or value.dtype != torch.float32:
            raise TypeError("prob and value must be float32")
        if tuple(prob.shape) != (self.B, NMOVES) or value.numel() != self.B:
            raise ValueError(f"prob must be [{self.B},{NMOVES}] and value [{self.B}]")
        if not (prob.is_cuda and value.is_cuda and prob.is_contiguous() and value.is_contiguous()):
            raise ValueError("prob/value must be contiguous device tensors")
        check(self.L.ccz_step(self.h, self._stream(), _ptr(prob), _ptr(value), _ptr(self.leaf_input)))
        return self.leaf_input

    def _check_logits(self, logits, value):
        if logits.dtype not in (torch.float16, torch.float32) or value.dtype != torch.float32:
            raise TypeError("logits must be float16/float32 and value float32")
        if tuple(logits.shape) != (self.B, NMOVES) or value.numel() != self.B:
            raise ValueError(f"logits must be [{self.B},{NMOVES}] and value [{self.B}]")
        if not (logits.is_cuda and value.is_cuda and logits.is_contiguous() and value.is_contiguous()):
            raise ValueError("logits/value must be contiguous device tensors")
        return 1 if logits.dtype == torch.float16 else 0

    def step_logits(self, logits: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
        """Compact boundary: policy-head LOGITS in; the engine takes exp(log_softmax) of the legal ids itself."""
        self.gather_priors(logits, value)
        return self.step_compact(value)

    def expand_backup_logits(self, logits: torch.Tensor, value: torch.Tensor):
        self.gather_priors(logits, value)
        check(self.L.ccz_expand_backup_compact(self.h, self._stream(), _ptr(value)))

    def gather_priors(self, logits: torch.Tensor, value: torch.Tensor):
        """exp(log_softmax(logits)) of the pending leaf's legal ids -> the engine's [B,128] prior row."""
        f16 = self._check_logits(logits, value)
        check(self.L.ccz_gather_priors(self.h, self._stream(), _ptr(logits), f16))

    def expand_backup_compact(self, value: torch.Tensor | None):
        """``value`` None: the engine-owned leaf values of the planned boundary."""
        check(self.L.ccz_expand_backup_compact(self.h, self._stream(), _ptr(value)))

    def step_compact(self, value: torch.Tensor | None) -> torch.Tensor:
        """``value`` None: the engine-owned leaf values of the planned boundary (:meth:`gather_priors_planned`)."""
        check(self.L.ccz_step_compact(self.h, self._stream(), _ptr(value), _ptr(self.leaf_input)))
        return self.leaf_input

    # ------------------------------------------------------------------ wide search (include/cczero.h "Wide search")
    def set_width(self, width: int):
        """``width`` > 1: boards 0 .. B / width - 1 are searched and gather up to ``width`` leaves of their one tree per step, kept
        apart by virtual loss; slot ``r + j * A`` holds the j-th pending leaf of board r. 1: off, the sequential search. Call it
        with no leaf pending."""
        check(self.L.ccz_set_width(self.h, self._stream(), int(width)))
        self.width = int(width)
        self.A = self.B // self.width
        if not hasattr(self, "n_leaves_host"):
            self.n_leaves_host = torch.zeros((self.B,), dtype=torch.int32).pin_memory()   # written by the wide kernels: [A] leaves selected
            self._n_leaves_np = self.n_leaves_host.numpy()

    def select_wide(self) -> torch.Tensor:
        """Phase B alone (a move's first step): up to ``width`` leaves per searched board; the evaluator input of all ``B`` slots."""
        self._need_wide()
        check(self.L.ccz_select_wide(self.h, self._stream(), _ptr(self.leaf_input), C.c_void_p(self.n_leaves_host.data_ptr())))
        return self.leaf_input

    def step_wide(self, value: torch.Tensor | None) -> torch.Tensor:
        """Back the pending slots up from the engine's prior rows and ``value`` [B] (None: the engine-owned leaf values of the
        planned boundary), then select the next leaves: one launch. With every budget used up it is the move's last backup."""
        self._need_wide()
        check(self.L.ccz_step_wide(self.h, self._stream(), _ptr(value), _ptr(self.leaf_input), C.c_void_p(self.n_leaves_host.data_ptr())))
        return self.leaf_input

    def _need_wide(self):
        if getattr(self, "width", 1) <= 1:
            raise CczError("the width is 1: set_width(width > 1) turns the wide search on")

    def n_leaves(self) -> np.ndarray:
        """Wait for the stream; leaves selected per searched board by the last :meth:`select_wide` / :meth:`step_wide` (int32 [A])."""
        torch.cuda.current_stream(self.device).synchronize()
        return self._n_leaves_np[: self.A].copy()

    def wide_stats(self) -> dict:
        st = _lib.WideStats()
        check(self.L.ccz_get_wide_stats(self.h, self._stream(), C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    # ------------------------------------------------------------------ planned evaluator boundary (evaluation cache)
    def eval_plan(self):
        """Probe the evaluation cache for the pending leaves and plan the evaluator's batch: returns the device tensors
        ``(miss_rows int32 [B], n_miss int32 [1])`` -- the boards whose leaves still need the network (deduplicated, ascending)
        and their number. No host sync: the evaluator's kernels read the count on the device."""
        check(self.L.ccz_eval_plan(self.h, self._stream(), _ptr(self.miss_rows), _ptr(self.n_miss)))
        return self.miss_rows, self.n_miss

    # ------------------------------------------------------------------ leaf history planes (include/cczero.h ccz_set_leaf_history)
    def set_leaf_history(self, enabled: bool = True):
        """The evaluator input of a pending leaf shows the eight positions a training row shows (the game's recorded plies, the root,
        the selection path; clamped at the game's first position) instead of the leaf alone in groups 7 / 15, and the leaf's cache
        key becomes its history key, from the next select phase on. Call it between moves or before the first selection: a leaf that
        is pending keeps the row it has. A change drops what rested on the old setting: the evaluation cache is cleared, the leaf
        tensor is zeroed when the option goes off (the old path rewrites three groups only) and ``history_version`` moves -- a hipGraph
        of the step does not hold the new launch, and ``selfplay.GraphedStep`` captures again when it sees that. The evaluator must
        read all 17 groups (``boundary.need_history``). Not with scout slots, a width above 1 or ``reference_quirks``."""
        enabled = bool(enabled)
        if enabled == self.leaf_history:
            return
        check(self.L.ccz_set_leaf_history(self.h, self._stream(), int(enabled)))
        self.leaf_history = enabled
        self.history_version += 1
        self.clear_eval_cache()
        if not enabled:
            check(self.L.ccz_zero_leaf_input(self.h, self._stream(), _ptr(self.leaf_input)))

    def get_leaf_history(self) -> bool:
        """The setting as the engine holds it (``ccz_get_leaf_history``)."""
        v = C.c_int32(0)
        check(self.L.ccz_get_leaf_history(self.h, C.byref(v)))
        return bool(v.value)

    # ------------------------------------------------------------------ scouts (one game at a time: include/cczero.h ccz_scout)
    def set_scouts(self, n_scouts: int):
        """The last ``n_scouts`` boards become scout slots (no tree, no game): the simulator entry points then run on the first
        ``B - n_scouts`` boards only. Needs an evaluation cache."""
        check(self.L.ccz_set_scouts(self.h, int(n_scouts)))
        self.n_scouts = int(n_scouts)
        if not hasattr(self, "_plan_state_host"):
            self._plan_state_host = torch.zeros((self.B,), dtype=torch.int32).pin_memory()   # written by k_cache_plan_scouted

    def scout(self):
        """Hand every scout slot its pending leaf: the next unvisited sibling(s) of the pending leaf of the board it scouts for --
        what that board's next simulations through the same parent will ask for (mcts.py:47-48: first maximum = insertion order)."""
        check(self.L.ccz_scout(self.h, self._stream(), _ptr(self.leaf_input)))

    def plan_scouted_launch(self):
        """Probe the table for every slot and plan the step's evaluator call (``ccz_eval_plan_scouted``; launches only). The plan
        state of the searched boards is written straight into pinned HOST memory by the plan kernel (no copy node: capturable)."""
        check(self.L.ccz_eval_plan_scouted(self.h, self._stream(), _ptr(self.miss_rows), _ptr(self.n_miss),
                                           C.c_void_p(self._plan_state_host.data_ptr())))

    def scout_and_plan(self):
        """:meth:`scout` + :meth:`plan_scouted_launch` as one launch (``ccz_scout_and_plan``)."""
        check(self.L.ccz_scout_and_plan(self.h, self._stream(), _ptr(self.leaf_input), _ptr(self.miss_rows), _ptr(self.n_miss),
                                        C.c_void_p(self._plan_state_host.data_ptr())))

    def scouted_run_launch(self):
        """Simulations in ONE launch (``ccz_scouted_run``): step + scout + probe + plan repeated on the device while board 0's next
        leaf is in the table. How many at most, and how many the move has left, go through pinned host memory -- the launch is
        capturable; write them with :meth:`set_run` before the launch or a replay, read the outcome with :meth:`run_outcome`."""
        if not hasattr(self, "_run_host"):
            self.set_run(1, 1)
        check(self.L.ccz_scouted_run(self.h, self._stream(), _ptr(self.leaf_input), _ptr(self.miss_rows), _ptr(self.n_miss),
                                     C.c_void_p(self._plan_state_host.data_ptr()), C.c_void_p(self._run_host.data_ptr())))

    def set_run(self, budget: int, left: int):
        """``budget``: simulations the next scouted run may do at most; ``left``: simulations left in this move, the pending one included."""
        if budget < 1 or left < 1:
            raise ValueError("scouted run: budget and simulations left must be >= 1")
        if not hasattr(self, "_run_host"):
            self._run_host = torch.zeros((4,), dtype=torch.int32).pin_memory()
            self._run_np = self._run_host.numpy()
        self._run_np[0] = budget
        self._run_np[1] = left

    def run_outcome(self):
        """Wait for the stream; ``(simulations done by the last scouted run, whether board 0's leaf needs the evaluator now)``."""
        torch.cuda.current_stream(self.device).synchronize()
        return int(self._run_np[2]), bool(self._run_np[3])

    def plan_state_of_board0(self) -> int:
        """Wait for the stream and read board 0's plan state: 0 = its leaf needs the evaluator -- run it on ALL ``B`` rows of
        ``leaf_input`` and hand the result to :meth:`gather_priors_planned` --, 1 = table hit, 2 = no evaluation needed."""
        torch.cuda.current_stream(self.device).synchronize()
        return int(self._plan_state_host[0])

    def plan_states(self) -> np.ndarray:
        """Wait for the stream; the plan states of ALL searched boards (0 miss / 1 hit / 2 nothing to evaluate): the evaluator has to
        run iff any of them is 0 (the host loop of the package searches one board and reads :meth:`plan_state_of_board0`)."""
        torch.cuda.current_stream(self.device).synchronize()
        return self._plan_state_host[: self.B - self.n_scouts].numpy().copy()

    def gather_priors_planned(self, logits: torch.Tensor, value: torch.Tensor):
        """``logits`` [B,2086] / ``value`` [B] as the planned evaluator returns them: COMPACT, row i = board miss_rows[i]."""
        f16 = self._check_logits(logits, value)
        check(self.L.ccz_gather_priors_planned(self.h, self._stream(), _ptr(logits), f16, _ptr(value)))

    def step_planned(self, logits: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
        self.gather_priors_planned(logits, value)
        return self.step_compact(None)

    def expand_backup_planned(self, logits: torch.Tensor, value: torch.Tensor):
        self.gather_priors_planned(logits, value)
        check(self.L.ccz_expand_backup_compact(self.h, self._stream(), None))

    def clear_eval_cache(self):
        """Forget every cached evaluation (the evaluator's weights changed)."""
        check(self.L.ccz_eval_cache_clear(self.h, self._stream()))

    # ------------------------------------------------------------------ two evaluators on one engine (include/cczero.h ccz_set_routing)
    def set_routing(self, red_net, salts=(0, 0)):
        """``red_net`` [B] of 0 / 1: the evaluator that plays red on each board (black: the other one); None = routing off.
        ``salts`` = (salt0, salt1), different: XORed into each evaluator's cache keys. A board's evaluator for a move is the owner
        of the root's side to move (:meth:`eval_plan_routed`). Needs an evaluation cache and no scouts."""
        if red_net is None:
            check(self.L.ccz_set_routing(self.h, self._stream(), None, 0, 0))
            return
        rn = np.ascontiguousarray(red_net, dtype=np.uint8)
        if rn.shape != (self.B,):
            raise ValueError(f"red_net must have {self.B} entries")
        s0, s1 = (int(x) & (2**64 - 1) for x in salts)
        with torch.cuda.device(self.device):
            check(self.L.ccz_set_routing(self.h, self._stream(), _ptr(rn), s0, s1))
        if not hasattr(self, "miss_rows2"):
            self.miss_rows2 = torch.zeros((2 * self.B,), dtype=torch.int32, device=self.device)
            self.n_miss2 = torch.zeros((2,), dtype=torch.int32, device=self.device)

    def eval_plan_routed(self):
        """Probe + plan with the routing: ``(plan0, plan1)``, each ``(rows, n)`` device tensors for one evaluator's planned
        boundary (``evaluate_leaves_logits(leaf, plan=...)``): evaluator 0's rows are ``miss_rows2[:B]``, evaluator 1's
        ``miss_rows2[B:]``; the counts ``n_miss2[0:1]`` / ``n_miss2[1:2]`` stay on the device."""
        check(self.L.ccz_eval_plan_routed(self.h, self._stream(), _ptr(self.miss_rows2), _ptr(self.n_miss2)))
        B = self.B
        return (self.miss_rows2[:B], self.n_miss2[0:1]), (self.miss_rows2[B:], self.n_miss2[1:2])

    def gather_priors_routed(self, logits0, value0, logits1, value1):
        """Each board takes its priors / value from the COMPACT output of its own evaluator (row = its row in that segment)."""
        f16 = self._check_logits(logits0, value0)
        if self._check_logits(logits1, value1) != f16:
            raise TypeError("both evaluators must return logits of the same dtype")
        check(self.L.ccz_gather_priors_routed(self.h, self._stream(), _ptr(logits0), _ptr(logits1), f16, _ptr(value0), _ptr(value1)))

    def step_routed(self, logits0, value0, logits1, value1) -> torch.Tensor:
        self.gather_priors_routed(logits0, value0, logits1, value1)
        return self.step_compact(None)

    def expand_backup_routed(self, logits0, value0, logits1, value1):
        self.gather_priors_routed(logits0, value0, logits1, value1)
        check(self.L.ccz_expand_backup_compact(self.h, self._stream(), None))

    # ------------------------------------------------------------------ per-board simulation budgets (include/cczero.h ccz_set_budgets)
    def set_budgets(self, budgets=None, targets=None):
        """``budgets`` int32 [B] (>= 1; array or device tensor): the simulations board b searches per move from now on, however
        many lockstep steps the host runs -- a board that has used its budget selects nothing (``LEAF_SKIP``, no row in ``eval_plan``).
        ``targets`` uint8 [B] or None (all 1): 1 = this move's pi is a policy target; the byte is stored with the ply and comes
        back as the record header's ``REC_FAST`` flag. ``budgets`` None: budgets off (unlimited, every move a target), the state of
        a new engine. Device tensors are taken as they are, with no host sync; an array is copied to the device first (a blocking
        copy of B words). Not with scout slots."""
        if budgets is None:
            check(self.L.ccz_set_budgets(self.h, self._stream(), None, None))
            return
        b = self._to_dev(budgets, torch.int32, "budgets")
        t = None if targets is None else self._to_dev(targets, torch.uint8, "targets")
        check(self.L.ccz_set_budgets(self.h, self._stream(), _ptr(b), _ptr(t)))

    def draw_budgets(self, n_full: int, n_fast: int, p_full: float) -> torch.Tensor:
        """Playout-cap randomisation for the move about to be searched (``ccz_draw_budgets``): every board is a full search
        (``n_full`` simulations, policy target) with probability ``p_full``, else a fast one (``n_fast``, no target), drawn on the
        board's own Philox stream (counter word 0xffe: the Dirichlet and move streams are untouched). Returns the budgets, device
        int32 [B] (``self.budgets_out``, overwritten by the next draw). No host sync. Call it at a move boundary."""
        check(self.L.ccz_draw_budgets(self.h, self._stream(), int(n_full), int(n_fast), float(p_full), _ptr(self.budgets_out)))
        return self.budgets_out

    # ------------------------------------------------------------------ resignation (include/cczero.h ccz_set_resign)
    def set_resign(self, threshold, consecutive: int = 2, min_ply: int = 30, p_playon: float = 0.1):
        """Self-play resignation from the next :meth:`finish_move` on: the side to move resigns when the root value of its last
        ``consecutive`` full-search plies was below ``threshold`` (in [-1, 0]) and the game has at least ``min_ply`` plies; a
        fraction ``p_playon`` of such games is played on instead, for :meth:`resign_stats` to measure the false positives.
        ``consecutive`` 0: root values are recorded (``REC_VALUE``) and nothing resigns. ``threshold`` None: off, the state of a
        new engine. No host sync."""
        if threshold is None:
            check(self.L.ccz_set_resign(self.h, self._stream(), 0, 0.0, 0, 0, 0.0))
            return
        check(self.L.ccz_set_resign(self.h, self._stream(), 1, float(threshold), int(consecutive), int(min_ply), float(p_playon)))

    def resign_status(self) -> dict:
        """Per-board resignation state (syncs): ``state`` uint8 [B] (0, or ``RESIGN_RESIGNED`` / ``RESIGN_PLAYON`` | side), ``run``
        uint8 [B,2] (indexed by side: 1 red), ``fire_ply`` int32 [B] (-1: not fired), ``last_value`` float32 [B] (NaN: none)."""
        B = self.B
        state = np.zeros(B, np.uint8)
        run = np.zeros((B, 2), np.uint8)
        fire = np.zeros(B, np.int32)
        last = np.zeros(B, np.float32)
        check(self.L.ccz_resign_status(self.h, self._stream(), _ptr(state), _ptr(run), _ptr(fire), _ptr(last)))
        return {"state": state, "run": run, "fire_ply": fire, "last_value": last}

    def resign_stats(self) -> dict:
        """The calibration counters (``ccz_resign_stats``; syncs): the false-positive rate is ``playon_won / playon_games``."""
        s = _lib.ResignStats()
        check(self.L.ccz_get_resign_stats(self.h, self._stream(), C.byref(s)))
        return {f: int(getattr(s, f)) for f, _ in _lib.ResignStats._fields_}

    # ------------------------------------------------------------------ policy surprise weighting (include/cczero.h ccz_set_surprise)
    def set_surprise(self, alpha=0.5, cap: float = 8.0):
        """Policy surprise weighting from the next :meth:`finish_move` on: every policy-target ply stores KL(pi || prior), and
        :meth:`harvest_record_chunks` writes a sampling weight into the records (``REC_WEIGHT``, bytes 90..91): a share
        ``1 - alpha`` of a game's weight spread evenly, the share ``alpha`` (in [0, 1]) by surprise, no ply above ``cap`` (in
        [1, 15]). ``alpha`` None: off, the state of a new engine. Plies recorded before the call carry no surprise. Not with
        scout slots. No host sync."""
        if alpha is None:
            check(self.L.ccz_set_surprise(self.h, self._stream(), 0, 0.5, 8.0))
            return
        check(self.L.ccz_set_surprise(self.h, self._stream(), 1, float(alpha), float(cap)))

    def surprise_stats(self) -> dict:
        """Sums over boards in board order (``ccz_surprise_stats``; syncs): ``target_plies`` measured, ``surprise_sum`` (float) of
        their stored surprise and ``weights_clipped`` at the cap by the harvest."""
        s = _lib.SurpriseStats()
        check(self.L.ccz_get_surprise_stats(self.h, self._stream(), C.byref(s)))
        return {"target_plies": int(s.target_plies), "surprise_sum": float(s.surprise_sum), "weights_clipped": int(s.weights_clipped)}

    def ply_surprise(self):
        """``(kl float32 [B, max_plies], has uint8 [B, max_plies])``: the surprise stored with the plies of the boards' current
        games and whether a ply carries one; entries at or past a board's ply count are stale. Syncs (tests, reports)."""
        kl = np.zeros((self.B, self.max_plies), np.float32)
        has = np.zeros((self.B, self.max_plies), np.uint8)
        check(self.L.ccz_ply_surprise(self.h, self._stream(), _ptr(kl), _ptr(has)))
        return kl, has

    # ------------------------------------------------------------------ root exploration (include/cczero.h ccz_set_root_exploration)
    def set_root_exploration(self, eps, alpha: float | None = None, forced_k: float = 2.0, prune_targets: bool = True):
        """Exploration inside the search, on policy-target moves: Dirichlet(``alpha``) noise of weight ``eps`` in the ROOT's priors
        (nodes keep their raw priors), forced playouts (``forced_k``, KataGo's 2; 0 = none) and policy target pruning
        (``prune_targets``): pi is formed from the pruned visit counts and the move drawn from it without the sampler's mixing.
        ``alpha`` None: the engine's sampler alpha. ``eps`` None: off, the state of a new engine. Fast moves of playout-cap
        randomisation search and sample as without it. Not with scout slots. No host sync."""
        if eps is None:
            check(self.L.ccz_set_root_exploration(self.h, self._stream(), 0, 0.0, 1.0, 0.0, 0))
            return
        a = self.alpha if alpha is None else float(alpha)
        check(self.L.ccz_set_root_exploration(self.h, self._stream(), 1, float(eps), a, float(forced_k), 1 if prune_targets else 0))

    def exploration_stats(self) -> dict:
        """Sums over boards (``ccz_exploration_stats``; syncs): ``explored_moves``, ``forced_selections`` (root selections won by the
        forced-playout rule on a visited child), ``visits_pruned`` and ``children_pruned`` (taken out of the policy targets)."""
        s = _lib.ExplorationStats()
        check(self.L.ccz_get_exploration_stats(self.h, self._stream(), C.byref(s)))
        return {f: int(getattr(s, f)) for f, _ in _lib.ExplorationStats._fields_}

    def root_noise(self):
        """``(noise float32 [B,128], k int32 [B])``: the Dirichlet component of every root child for the move being searched, as the
        score used it (zero past k; k = 0 on a board without noise for its current move). Syncs (tests, diagnostics)."""
        noise = np.zeros((self.B, MAX_LEGAL), np.float32)
        k = np.zeros(self.B, np.int32)
        check(self.L.ccz_root_noise(self.h, self._stream(), _ptr(noise), _ptr(k)))
        return noise, k

    # ------------------------------------------------------------------ Gumbel root search (include/cczero.h ccz_set_gumbel)
    def set_gumbel(self, n_sims, max_considered: int = 16, c_visit: float = 50.0, c_scale: float = 1.0):
        """Gumbel root search (Danihelka et al. 2022) on every move of every board: one Gumbel draw per root child and move,
        sequential halving over the ``max_considered`` best of them within the move's simulations (the board's budget, else
        ``n_sims``), the winner is played and pi' = softmax(logit + sigma(completed Q)) is recorded as the policy target --
        fast moves of playout-cap randomisation included. Below the root the search is unchanged. ``n_sims`` None: off, the
        state of a new engine. Not with scout slots or root exploration. No host sync."""
        if n_sims is None:
            check(self.L.ccz_set_gumbel(self.h, self._stream(), 0, 1, 16, 50.0, 1.0))
            return
        check(self.L.ccz_set_gumbel(self.h, self._stream(), 1, int(n_sims), int(max_considered), float(c_visit), float(c_scale)))

    def gumbel_stats(self) -> dict:
        """Sums over boards (``ccz_gumbel_stats``; syncs): ``gumbel_moves``, ``considered_sum`` (sum of m over them) and
        ``offvisit_moves`` (plies whose played child is not the most visited one)."""
        s = _lib.GumbelStats()
        check(self.L.ccz_get_gumbel_stats(self.h, self._stream(), C.byref(s)))
        return {f: int(getattr(s, f)) for f, _ in _lib.GumbelStats._fields_}

    def gumbel_root(self):
        """``(g float64 [B,128], logit float64 [B,128], n0 int32 [B,128], k int32 [B], n_eff int32 [B])``: the Gumbel rows of the
        move being searched (zero past k; k = 0 on a board without a row for its current move). Syncs (tests, diagnostics)."""
        g = np.zeros((self.B, MAX_LEGAL), np.float64)
        logit = np.zeros((self.B, MAX_LEGAL), np.float64)
        n0 = np.zeros((self.B, MAX_LEGAL), np.int32)
        k = np.zeros(self.B, np.int32)
        n_eff = np.zeros(self.B, np.int32)
        check(self.L.ccz_gumbel_root(self.h, self._stream(), _ptr(g), _ptr(logit), _ptr(n0), _ptr(k), _ptr(n_eff)))
        return g, logit, n0, k, n_eff

    # ------------------------------------------------------------------ search parameters (include/cczero.h ccz_set_search)
    def set_search(self, enabled: bool = True, fpu_mode: int = 0, fpu_value: float = 0.0, fpu_root_mode: int | None = None,
                   fpu_root_value: float | None = None, c_base: float = 19652.0, c_factor: float = 0.0):
        """First-play urgency and the visit-scaled exploration constant. ``fpu_mode``: 0 an unvisited child scores +inf (the
        reference's rule), 1 reduction (the parent's value minus ``fpu_value`` * sqrt(visited prior mass), Lc0 / KataGo), 2 absolute
        (``fpu_value``, AlphaZero). ``fpu_root_mode`` / ``fpu_root_value``: the same at the root (None: the tree's setting).
        ``c_factor`` > 0: c_puct grows by ``c_factor * log((N + c_base + 1) / c_base)`` with the node's visits. ``enabled`` False or
        None: off, the state of a new engine; the other arguments are ignored. Not with scout slots. No host sync."""
        if not enabled:
            check(self.L.ccz_set_search(self.h, self._stream(), 0, 0, 0.0, 0, 0.0, 19652.0, 0.0))
            return
        rm = fpu_mode if fpu_root_mode is None else fpu_root_mode
        rv = (fpu_value if fpu_root_mode is None else 0.0) if fpu_root_value is None else fpu_root_value
        check(self.L.ccz_set_search(self.h, self._stream(), 1, int(fpu_mode), float(fpu_value), int(rm), float(rv), float(c_base),
                                    float(c_factor)))

    def search_settings(self) -> dict:
        """The search parameters as the kernels read them (``ccz_get_search``; syncs): ``enabled``, ``fpu_mode``, ``fpu_value``,
        ``fpu_root_mode``, ``fpu_root_value``, ``c_base``, ``c_factor``."""
        s = _lib.SearchCfg()
        check(self.L.ccz_get_search(self.h, self._stream(), C.byref(s)))
        out = {f: getattr(s, f) for f, _ in _lib.SearchCfg._fields_ if f != "reserved"}
        out["enabled"] = bool(out["enabled"])
        return out

    # ------------------------------------------------------------------ early stop per board (include/cczero.h ccz_set_early_stop)
    def set_early_stop(self, enabled: bool = True, single_reply: bool = False, gap_factor: float = 0.0, kld_interval: int = 0,
                       min_gain: float = 0.0, min_sims: int = 0, n_sims: int | None = None):
        """A board stops searching its move early and from then on selects nothing (``LEAF_SKIP``, no evaluator row), like one whose
        budget is spent: with one legal reply (``single_reply``), when the most visited root child leads the runner-up by more than
        the simulations left can make up (``gap_factor`` f >= 1: ``(N1 - N2) * f > n_b - s``; 0 off), or when the KL divergence
        between the root's visit distributions ``kld_interval`` simulations apart, per new visit, falls below ``min_gain``. No rule
        runs below ``min_sims`` simulations. ``n_sims``: the simulations of a move on a board without a budget (None: the engine's
        ``n_playout``). ``enabled`` False or None: off, the state of a new engine. Not with scout slots, a width above 1 or the
        Gumbel root. No host sync."""
        c = _lib.EarlyStopCfg()
        if enabled:
            c.enabled, c.single_reply, c.kld_interval, c.min_sims = 1, int(single_reply), int(kld_interval), int(min_sims)
            c.n_sims = self.n_playout if n_sims is None else int(n_sims)
            c.gap_factor, c.min_gain = float(gap_factor), float(min_gain)
        check(self.L.ccz_set_early_stop(self.h, self._stream(), C.byref(c)))

    def early_stop_settings(self) -> dict:
        """The early-stop settings as the kernels read them (``ccz_get_early_stop``; syncs): ``enabled``, ``single_reply``,
        ``gap_factor``, ``kld_interval``, ``min_gain``, ``min_sims``, ``n_sims``."""
        c = _lib.EarlyStopCfg()
        check(self.L.ccz_get_early_stop(self.h, self._stream(), C.byref(c)))
        return {"enabled": bool(c.enabled), "single_reply": bool(c.single_reply), "gap_factor": c.gap_factor,
                "kld_interval": c.kld_interval, "min_gain": c.min_gain, "min_sims": c.min_sims, "n_sims": c.n_sims}

    def early_stop_stats(self) -> dict:
        """Sums over boards (``ccz_get_early_stop_stats``; syncs): ``single_reply`` / ``visit_gap`` / ``kld_gain`` (stops by
        reason), ``sims_saved`` (simulations the stopped boards had left) and ``evaluations`` (KLD snapshots taken)."""
        s = _lib.EarlyStopStats()
        check(self.L.ccz_get_early_stop_stats(self.h, self._stream(), C.byref(s)))
        return {"single_reply": int(s.stops[1]), "visit_gap": int(s.stops[2]), "kld_gain": int(s.stops[3]),
                "sims_saved": int(s.sims_saved), "evaluations": int(s.evaluations)}

    def early_stop_status(self) -> dict:
        """Per board (``ccz_early_stop_status``; syncs): ``reason`` uint8 [B] (0: not stopped in its current move, 1 single reply,
        2 visit gap, 3 KLD gain) and ``sims`` int32 [B], the simulations its current move has backed up."""
        out = {"reason": np.zeros(self.B, np.uint8), "sims": np.zeros(self.B, np.int32)}
        check(self.L.ccz_early_stop_status(self.h, self._stream(), _ptr(out["reason"]), _ptr(out["sims"])))
        return out

    def searching(self) -> int:
        """How many searched boards would still select a leaf (``ccz_searching``; one small kernel and a 4-byte copy; syncs): the
        game running, the budget not spent, not stopped. 0: the rest of the move's steps would do nothing."""
        n = C.c_int32(0)
        check(self.L.ccz_searching(self.h, self._stream(), C.byref(n)))
        return int(n.value)

    # ------------------------------------------------------------------ MCTS-solver (include/cczero.h ccz_set_solver)
    def set_solver(self, enabled: bool = True):
        """Exact propagation of decided positions (Winands' MCTS-solver): a terminal leaf proves its node, a node with a lost child
        is won, a node whose children are all won is lost, and the descent stops at a proven node (``LEAF_WIN`` / ``LEAF_LOSS`` /
        ``LEAF_DRAW`` with k = 0: no move generation, no evaluator row). PUCT, N, Q and the move choice are untouched; a front-end
        forces the proven move with :func:`proof_move`. The first call that turns it on allocates one byte per tree node and may
        sync. Off (the state of a new engine): every output is what it is without the feature."""
        with torch.cuda.device(self.device):
            check(self.L.ccz_set_solver(self.h, self._stream(), 1 if enabled else 0))
        self.solver = bool(enabled)

    def root_proof(self) -> dict:
        """Proof bytes at the top of every tree (``ccz_root_proof``; syncs): ``state`` / ``dist`` uint8 [B] of the root,
        ``child_state`` / ``child_dist`` uint8 [B,128] aligned with ``root_children()['acts']`` (zero past k). States are
        ``PROOF_WIN`` / ``PROOF_LOSS`` / ``PROOF_DRAW`` in the view of the side to move AT THAT NODE (0: unknown); ``dist``: plies
        to the end, saturating at 63. All zeros while the solver is off."""
        B = self.B
        out = {"state": np.zeros(B, np.uint8), "dist": np.zeros(B, np.uint8),
               "child_state": np.zeros((B, MAX_LEGAL), np.uint8), "child_dist": np.zeros((B, MAX_LEGAL), np.uint8)}
        check(self.L.ccz_root_proof(self.h, self._stream(), _ptr(out["state"]), _ptr(out["dist"]), _ptr(out["child_state"]), _ptr(out["child_dist"])))
        return out

    def proof_moves(self) -> np.ndarray:
        """int32 [B]: :func:`proof_move` of every board (-1: its root is not decided, or the solver is off) -- what a front-end hands
        :meth:`finish_move` as ``forced_moves`` (-1 leaves the choice to the sampler). Syncs."""
        rp, rc = self.root_proof(), self.root_children()
        out = np.full(self.B, -1, np.int32)
        for b in np.nonzero(rp["state"])[0]:
            mv = proof_move(rp["state"][b], rp["dist"][b], rp["child_state"][b], rp["child_dist"][b], rc["acts"][b])
            if mv is not None:
                out[b] = mv
        return out

    def solver_stats(self) -> dict:
        """Sums over boards (``ccz_solver_stats``; syncs): ``nodes_proven``, ``proven_stops`` (simulations whose descent ended at a
        node proven earlier), ``roots_proven`` (searched boards whose game is running and whose root is proven now)."""
        s = _lib.SolverStats()
        check(self.L.ccz_get_solver_stats(self.h, self._stream(), C.byref(s)))
        return {f: int(getattr(s, f)) for f, _ in _lib.SolverStats._fields_}

    # ------------------------------------------------------------------ value spread and the LCB move (include/cczero.h ccz_set_value_stats)
    def set_value_stats(self, enabled: bool = True):
        """Every tree node also keeps S, the running sum of squared deviations of the values backed up through it (Welford, float32:
        ``S += (val - q) * (val - q_new)`` in the backup), which is what :meth:`lcb_moves` needs. S never feeds back into the search:
        N, Q, P, leaves, moves and records are bit for bit what they are without it. The first call that turns it on allocates four
        bytes per tree node and may sync; turning it on again starts from zeros. Off (the state of a new engine): every launch is
        what it is without the feature. Not with a width above 1, not on a ``value_f16`` engine, and no snapshot while it is on."""
        with torch.cuda.device(self.device):
            check(self.L.ccz_set_value_stats(self.h, self._stream(), 1 if enabled else 0))
        self.value_stats = bool(enabled)

    def get_value_stats(self) -> bool:
        """The setting as the engine holds it (``ccz_get_value_stats``)."""
        v = C.c_int32(0)
        check(self.L.ccz_get_value_stats(self.h, C.byref(v)))
        return bool(v.value)

    def root_value_stats(self) -> dict:
        """S at the top of every tree (``ccz_root_value_stats``; syncs): ``S`` float32 [B,128] of the root's children, aligned with
        ``root_children()['acts']`` (zero past k), and ``root_S`` float32 [B]. Zero rows for finished boards and scout slots. The
        sample variance of child i is ``max(S_i, 0) / (N_i - 1)``. Fails while the option is off."""
        out = {"S": np.zeros((self.B, MAX_LEGAL), np.float32), "root_S": np.zeros(self.B, np.float32)}
        check(self.L.ccz_root_value_stats(self.h, self._stream(), _ptr(out["S"]), _ptr(out["root_S"])))
        return out

    def lcb_moves(self, z: float, min_visit_ratio: float, min_visits: int, with_bounds: bool = False):
        """The lower-confidence-bound move of every board (``ccz_lcb_moves``; the rule in full is in include/cczero.h): among the
        root's children searched enough -- ``N >= max(2, min_visits)`` and ``N >= min_visit_ratio * N_max``, and always the most
        visited one -- the one of largest ``Q - z * sqrt(var / N)``. Returns ``moves`` int32 [B] on the device (-1: finished board,
        scout slot, nothing visited): what :meth:`finish_move` takes as ``forced_moves``. No host sync. ``with_bounds``: a dict
        ``moves`` / ``child`` int32 [B] and ``lcb`` float64 [B,128] (-inf: no bound; 0 past k), on the device."""
        if not hasattr(self, "_lcb_moves"):
            self._lcb_moves = torch.empty((self.B,), dtype=torch.int32, device=self.device)
            self._lcb_child = torch.empty((self.B,), dtype=torch.int32, device=self.device)
        lcb = torch.empty((self.B, MAX_LEGAL), dtype=torch.float64, device=self.device) if with_bounds else None
        check(self.L.ccz_lcb_moves(self.h, self._stream(), float(z), float(min_visit_ratio), int(min_visits), _ptr(self._lcb_moves),
                                   _ptr(self._lcb_child), _ptr(lcb)))
        if with_bounds:
            return {"moves": self._lcb_moves, "child": self._lcb_child, "lcb": lcb}
        return self._lcb_moves

    def mate_search(self, max_plies: int, node_budget: int, out=None) -> dict:
        """Forced mates by consecutive checks from every board's root (``ccz_mate_search``; the definition in full is in
        include/cczero.h): the side to move may only give check, the other side tries every reply, depth-first with iterative
        deepening 1, 3, ..., ``max_plies`` (odd, at most ``MATE_MAX_PLIES``), at most ``node_budget`` move generations per board
        (1 .. ``MATE_MAX_NODES``). No evaluator row, nothing of the engine changes. Returns NumPy int32 [B] arrays: ``state``
        (0 not searched: game over, parked, scout slot; 1 mate found; 2 none within ``max_plies``; 3 budget reached), ``dist`` (plies
        of the mate, else 0), ``move`` (the first mating move in ``legal_moves`` order, else -1), ``nodes``. ``out``: an int32 device
        tensor [4,B] to launch into (default: one kept by the engine). Syncs, for the copy."""
        if out is None:
            if not hasattr(self, "_mate_out"):
                self._mate_out = torch.empty((4, self.B), dtype=torch.int32, device=self.device)
            out = self._mate_out
        if out.dtype != torch.int32 or tuple(out.shape) != (4, self.B) or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous int32 tensor [4,{self.B}] on {self.device}")
        with torch.cuda.device(self.device):
            check(self.L.ccz_mate_search(self.h, self._stream(), int(max_plies), int(node_budget), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                         _ptr(out[3])))
        host = out.cpu().numpy()
        return {"state": host[0].copy(), "dist": host[1].copy(), "move": host[2].copy(), "nodes": host[3].copy()}

    def _to_dev(self, x, dtype, name):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype={torch.int32: np.int32, torch.uint8: np.uint8}[dtype]))
        t = t.to(device=self.device, dtype=dtype).contiguous()
        if tuple(t.shape) != (self.B,):
            raise ValueError(f"{name} must have {self.B} entries")
        return t

    # ------------------------------------------------------------------ once per move
    def finish_move(self, forced_moves=None, temps=None, keep_tree: bool = True) -> torch.Tensor:
        """Record pi, choose (or accept) the move, re-root, push, detect game end. Returns moves int32[B] (device)."""
        f = t = None
        if forced_moves is not None:
            self._forced.copy_(torch.as_tensor(np.asarray(forced_moves, dtype=np.int32)) if not isinstance(forced_moves, torch.Tensor) else forced_moves)
            f = self._forced
        if temps is not None:
            self._temps.copy_(torch.as_tensor(np.asarray(temps, dtype=np.float64)) if not isinstance(temps, torch.Tensor) else temps)
            t = self._temps
        check(self.L.ccz_finish_move(self.h, self._stream(), _ptr(f), _ptr(t), _ptr(self.moves_out), 1 if keep_tree else 0))
        return self.moves_out

    # ------------------------------------------------------------------ inspection (sync)
    def root_children(self):
        B = self.B
        k = np.zeros(B, np.int32)
        acts = np.zeros((B, MAX_LEGAL), np.uint16)
        visits = np.zeros((B, MAX_LEGAL), np.int32)
        q = np.zeros((B, MAX_LEGAL), np.float32)
        p = np.zeros((B, MAX_LEGAL), np.float32)
        rn = np.zeros(B, np.int32)
        check(self.L.ccz_root_children(self.h, self._stream(), _ptr(k), _ptr(acts), _ptr(visits), _ptr(q), _ptr(p), _ptr(rn)))
        return {"k": k, "acts": acts, "visits": visits, "q": q, "prior": p, "root_visits": rn}

    def principal_variations(self, multipv: int = 1, max_len: int = 32) -> dict:
        """The best lines of every live tree (``ccz_principal_variations``). Line r starts at the root child of rank r by visits
        (ties to the lower child index: line 0 starts with the arg-max move) and follows the first most-visited child while it
        has visits. Returns numpy arrays: ``moves`` uint16 [B,multipv,max_len], ``len`` int32 [B,multipv] (0: unused line),
        ``visits`` int32 [B,multipv,max_len] (N of every node on the line), ``q`` / ``prior`` float32 [B,multipv] (the first
        move's stored Q -- root side to move's view -- and P), ``root_visits`` int32 [B]. Boards that are over and scout slots
        have no lines. Syncs once, like :meth:`root_children`."""
        B, K, M = self.B, int(multipv), int(max_len)
        if not 1 <= K <= MAX_LEGAL or M < 1:
            raise ValueError(f"multipv must be 1..{MAX_LEGAL} and max_len >= 1")
        dev = self.device
        out = {"moves": torch.empty((B, K, M), dtype=torch.int16, device=dev), "len": torch.empty((B, K), dtype=torch.int32, device=dev),
               "visits": torch.empty((B, K, M), dtype=torch.int32, device=dev), "q": torch.empty((B, K), dtype=torch.float32, device=dev),
               "prior": torch.empty((B, K), dtype=torch.float32, device=dev), "root_visits": torch.empty((B,), dtype=torch.int32, device=dev)}
        check(self.L.ccz_principal_variations(self.h, self._stream(), K, M, _ptr(out["moves"]), _ptr(out["len"]), _ptr(out["visits"]),
                                              _ptr(out["q"]), _ptr(out["prior"]), _ptr(out["root_visits"])))
        host = {k: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k, v in out.items()}
        for k, v in out.items():
            host[k].copy_(v, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        res = {k: v.numpy().copy() for k, v in host.items()}
        res["moves"] = res["moves"].view(np.uint16)
        return res

    def root_pi(self, temps=None) -> np.ndarray:
        pi = np.zeros((self.B, MAX_LEGAL), np.float64)
        t = None if temps is None else np.ascontiguousarray(np.broadcast_to(np.asarray(temps, np.float64), (self.B,)))
        check(self.L.ccz_root_pi(self.h, self._stream(), _ptr(t), _ptr(pi)))
        return pi

    def move_distribution(self, temps=None):
        """What the next unforced :meth:`finish_move` samples from, without moving (syncs; tests): ``(gamma, mixed, u)`` with
        the raw Gamma(alpha) draws and ``(1-eps) pi + eps Dirichlet`` as float64 [B,128] aligned with ``root_children()['acts']``
        (zero past k) and the choice uniform float64 [B] (NaN where no move would be sampled). ``temps`` as for :meth:`root_pi`."""
        gamma = np.zeros((self.B, MAX_LEGAL), np.float64)
        mixed = np.zeros((self.B, MAX_LEGAL), np.float64)
        u = np.zeros(self.B, np.float64)
        t = None if temps is None else np.ascontiguousarray(np.broadcast_to(np.asarray(temps, np.float64), (self.B,)))
        check(self.L.ccz_move_distribution(self.h, self._stream(), _ptr(t), _ptr(gamma), _ptr(mixed), _ptr(u)))
        return gamma, mixed, u

    def game_status(self):
        B = self.B
        over = np.zeros(B, np.uint8)
        winner = np.zeros(B, np.int8)
        plies = np.zeros(B, np.int32)
        turn = np.zeros(B, np.uint8)
        check(self.L.ccz_game_status(self.h, self._stream(), _ptr(over), _ptr(winner), _ptr(plies), _ptr(turn)))
        return {"over": over, "winner": winner, "plies": plies, "turn": turn}

    def root_positions(self) -> np.ndarray:
        sq = np.zeros((self.B, SQ_STRIDE), np.uint8)
        check(self.L.ccz_root_positions(self.h, self._stream(), _ptr(sq)))
        return sq[:, :90].copy()

    def leaf_info(self):
        B = self.B
        status = np.zeros(B, np.uint8)
        k = np.zeros(B, np.int32)
        ids = np.zeros((B, MAX_LEGAL), np.uint16)
        depth = np.zeros(B, np.int32)
        check(self.L.ccz_leaf_info(self.h, self._stream(), _ptr(status), _ptr(k), _ptr(ids), _ptr(depth)))
        return {"status": status, "k": k, "ids": ids, "depth": depth}

    def leaf_priors(self, values: bool = True):
        """What the compact / planned boundary hands the tree for the pending leaves, after ``gather_priors[_planned]``:
        ``(prior float32 [B,128] aligned with leaf_info()['ids'], value float32 [B] or None)``; ``values`` needs an evaluation
        cache (engine-owned leaf values). Syncs (tests)."""
        pri = np.zeros((self.B, MAX_LEGAL), np.float32)
        val = np.zeros(self.B, np.float32) if values else None
        check(self.L.ccz_leaf_priors(self.h, self._stream(), _ptr(pri), _ptr(val)))
        return pri, val

    def leaf_keys(self):
        """(keys int64 [B], status uint8 [B]) of the pending leaves as device tensors (no sync): equal keys = equal evaluator
        input (position + side to move)."""
        keys = torch.empty((self.B,), dtype=torch.int64, device=self.device)
        status = torch.empty((self.B,), dtype=torch.uint8, device=self.device)
        check(self.L.ccz_leaf_keys(self.h, self._stream(), _ptr(keys), _ptr(status)))
        return keys, status

    def stats(self) -> dict:
        s = Stats()
        check(self.L.ccz_get_stats(self.h, self._stream(), C.byref(s)))
        d = {f: getattr(s, f) for f, _ in Stats._fields_ if f != "reserved"}
        if s.reserved:
            d["bounds_line"] = int(s.reserved)  # bounds-checked diagnostic build: where cczero_kernels.h indexed out of range
        return d

    def check_healthy(self):
        e = self.stats()["error_flags"]
        if e:
            msgs = [m for bit, m in _lib.ERR_BITS.items() if e & bit]
            raise CczError(f"engine error flags {e}: " + "; ".join(msgs) + (f" (cczero_kernels.h:{self.stats()['bounds_line']})" if e & 128 else ""))

    # ------------------------------------------------------------------ training tuples
    def harvest_chunks(self, max_rows: int = 1 << 19):
        """Yield (states fp16 [R,17,7,10,9], pi f32 [R,2086], z f32 [R]) chunks of at most ``max_rows`` rows until no
        finished game is left; harvested boards restart. (2^19 rows = 15.6 GB: many boards can reach the ply cap in
        the same move, so the rows of one harvest are bounded by the buffer, not by the number of finished games.)"""
        while True:
            rows = C.c_int64(0)
            check(self.L.ccz_harvest_rows(self.h, self._stream(), C.byref(rows)))
            total = int(rows.value)
            if total == 0:
                return
            cap = min(total, int(max_rows))
            while True:
                states = torch.empty((cap, 17, 7, 10, 9), dtype=torch.float16, device=self.device)
                pi = torch.empty((cap, NMOVES), dtype=torch.float32, device=self.device)
                z = torch.empty((cap,), dtype=torch.float32, device=self.device)
                got = C.c_int64(0)
                rc = self.L.ccz_harvest(self.h, self._stream(), _ptr(states), _ptr(pi), _ptr(z), cap, C.byref(got))
                if rc == -5 and cap < total:  # one single game is longer than the chunk: grow to fit it
                    cap = min(total, cap * 2)
                    continue
                check(rc)
                break
            R = int(got.value)
            yield states[:R], pi[:R], z[:R]

    def harvest(self, max_rows: int = 1 << 19):
        """Tuples of all finished games -> (states fp16 [R,17,7,10,9], pi f32 [R,2086], z f32 [R]); restarts those
        boards. Raises if more than ``max_rows`` rows are pending: iterate :meth:`harvest_chunks` instead."""
        rows = C.c_int64(0)
        check(self.L.ccz_harvest_rows(self.h, self._stream(), C.byref(rows)))
        if rows.value > max_rows:
            raise CczError(f"{rows.value} rows pending (> {max_rows}): use harvest_chunks() to bound device memory")
        chunks = list(self.harvest_chunks(max_rows))
        if not chunks:
            return (torch.empty((0, 17, 7, 10, 9), dtype=torch.float16, device=self.device),
                    torch.empty((0, NMOVES), dtype=torch.float32, device=self.device),
                    torch.empty((0,), dtype=torch.float32, device=self.device))
        if len(chunks) == 1:
            return chunks[0]
        return tuple(torch.cat([c[i] for c in chunks]) for i in range(3))


    def harvest_record_chunks(self, max_plies: int = 1 << 16):
        """Yield uint8 [P, 880] tensors of compact ply records (``include/cczero.h`` CCZ_REC_*: whole finished games, plies in
        order) of at most ``max_plies`` records until no finished game is left; harvested boards restart. The wire format of
        the multi-GPU exchange: :func:`expand_records` rebuilds from them, byte for byte, the rows :meth:`harvest_chunks` yields."""
        mul = 2 if self.mirror else 1
        while True:
            rows = C.c_int64(0)
            check(self.L.ccz_harvest_rows(self.h, self._stream(), C.byref(rows)))
            total = int(rows.value) // mul
            if total == 0:
                return
            cap = min(total, int(max_plies))
            while True:
                rec = torch.empty((cap, _lib.REC_BYTES), dtype=torch.uint8, device=self.device)
                got = C.c_int64(0)
                rc = self.L.ccz_harvest_records(self.h, self._stream(), _ptr(rec), cap, C.byref(got))
                if rc == -5 and cap < total:  # one single game is longer than the chunk: grow to fit it
                    cap = min(total, cap * 2)
                    continue
                check(rc)
                break
            yield rec[:int(got.value)]

    # ------------------------------------------------------------------ snapshots (include/cczero.h "Engine snapshots")
    def snapshot_size(self) -> int:
        """Bytes :meth:`save_state` would write now (``ccz_snapshot_size``; syncs)."""
        n = C.c_uint64(0)
        with torch.cuda.device(self.device):
            check(self.L.ccz_snapshot_size(self.h, self._stream(), C.byref(n)))
        return int(n.value)

    def save_state(self) -> torch.Tensor:
        """The engine's state as one uint8 device tensor of exactly the snapshot's size (``ccz_snapshot_save``): the live prefixes of
        the node pool and the record arrays and every per-board row, not the allocations (:mod:`chinesechesszero_amd.snapshot`).
        Call it at a MOVE BOUNDARY -- after :meth:`finish_move`, before or after the harvest, with no leaf pending; whether one is
        pending the engine cannot tell (``BatchedSelfPlay.state_dict`` checks it). The evaluation cache is not saved. Syncs."""
        blob = torch.empty((self.snapshot_size(),), dtype=torch.uint8, device=self.device)
        n = C.c_uint64(0)
        with torch.cuda.device(self.device):
            check(self.L.ccz_snapshot_save(self.h, self._stream(), _ptr(blob), blob.numel(), C.byref(n)))
        if int(n.value) != blob.numel():
            raise CczError(f"ccz_snapshot_save wrote {int(n.value)} bytes into a blob of {blob.numel()}")
        return blob

    def load_state(self, blob, keep_board_id_base: bool = False):
        """Continue from a snapshot: ``blob`` is what :meth:`save_state` returned (a device or CPU uint8 tensor) or the path of a
        ``torch.save``d one. STRICT: the engine must have been created with the same arguments and hold the same settings
        (resign, root exploration, Gumbel, search, early stop, solver, width); any difference raises :class:`CczError` naming the field
        and leaves the engine exactly as it was. ``keep_board_id_base``: the one override -- the engine keeps its own
        ``board_id_base``. The evaluation cache starts cold (the trees do not depend on it; the cache counters of :meth:`stats` do).
        Graphs captured before the load stay valid. Syncs."""
        if not isinstance(blob, torch.Tensor):
            blob = torch.load(blob, map_location="cpu")
        if not isinstance(blob, torch.Tensor) or blob.dtype != torch.uint8:
            raise TypeError("an engine snapshot is a uint8 tensor")
        t = blob.reshape(-1).to(self.device).contiguous()
        if t.data_ptr() % 16:        # (a view into a larger tensor)
            t = t.clone()
        with torch.cuda.device(self.device):
            check(self.L.ccz_snapshot_load(self.h, self._stream(), _ptr(t), t.numel(), 1 if keep_board_id_base else 0))

    def record_flags(self) -> int:
        """The ``flags`` :func:`expand_records` needs to reproduce this engine's :meth:`harvest` (quirk mode, mirror)."""
        return (_lib.FLAG_REFERENCE_QUIRKS if self.reference_quirks else 0) | (0 if self.mirror else _lib.FLAG_NO_MIRROR)


def rows_of_records(n_plies: int, flags: int = 0) -> int:
    return int(n_plies) * (1 if flags & _lib.FLAG_NO_MIRROR else 2)


def game_aligned_chunks(records: torch.Tensor, max_plies: int):
    """Split records uint8 [P, 880] (whole games) into views of at most ``max_plies`` records that hold whole games each
    (a single longer game becomes its own chunk). Reads one 2-byte header word per cut."""
    P, lo = int(records.shape[0]), 0
    while lo < P:
        hi = min(P, lo + int(max_plies))
        if hi < P:
            t = int(records[hi, _lib.REC_HDR:_lib.REC_HDR + 2].cpu().view(torch.int16).item()) & 0xffff  # ply index of record hi
            if hi - t > lo:
                hi -= t       # cut in front of the game that holds record hi
            else:             # the game starting at lo is longer than max_plies: take it whole (T at header bytes 2..3)
                T = int(records[lo, _lib.REC_HDR + 2:_lib.REC_HDR + 4].cpu().view(torch.int16).item()) & 0xffff
                hi = min(P, lo + max(T, 1))
        yield records[lo:hi]
        lo = hi


def _expand(records: torch.Tensor, flags, plane_of_type, dense, ring: int, head_row, bad, target, value):
    """One ``ccz_expand_records`` launch on the current stream. ``dense``: (states, pi, z) or None (the side-only mode);
    ``target`` / ``value``: the side outputs or None; ``ring``: the outputs' length if they are a ring, else 0."""
    if not (records.is_cuda and records.dtype == torch.uint8 and records.is_contiguous()):
        raise ValueError("records must be a contiguous uint8 device tensor")
    if records.numel() % _lib.REC_BYTES:
        raise ValueError("records must hold whole 880-byte ply records")
    dev = records.device
    pot = None if plane_of_type is None else (C.c_uint8 * 8)(*[int(x) for x in plane_of_type])
    states, pi, z = dense if dense is not None else (None, None, None)
    with torch.cuda.device(dev):
        check(_lib.lib().ccz_expand_records(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), _ptr(records), records.numel() // _lib.REC_BYTES,
                                            int(flags), pot, _ptr(states), _ptr(pi), _ptr(z), ring, int(head_row) if ring else 0, _ptr(bad),
                                            _ptr(target), _ptr(value)))


def _side_ring(name: str, t, dtype, dev, ring=None):
    """A side output of :func:`_expand` given by the caller: a 1-d ring on the records' device (of ``ring`` entries, if given)."""
    if not (t.is_contiguous() and t.dtype == dtype and t.dim() == 1 and t.device == dev):
        raise ValueError(f"{name} must be a contiguous {'uint8' if dtype == torch.uint8 else 'float32'} [N] tensor on the records' device")
    if ring is not None and int(t.shape[0]) != ring:
        raise ValueError(f"{name} must have the length of z ({ring})")
    return t


def expand_records(records: torch.Tensor, flags: int = 0, plane_of_type=None, out=None, head_row: int = 0, bad=None, targets=False, values=False):
    """Compact ply records (uint8 [P, 880] on the GPU, whole games) -> the dense training rows ``ccz_harvest`` would have
    written for those games: (states fp16 [R,17,7,10,9], pi f32 [R,2086], z f32 [R]), R = P x (1 or 2 with mirror images).
    Stateless (no engine: the records may come from another rank). ``out=(states, pi, z)`` writes into existing arrays as a
    ring: row i goes to (head_row + i) % len(z). ``bad``: int32 device tensor [1] counting records of cut games (skipped).
    ``targets`` / ``values``: also return, after ``z`` and in this order, the rows' policy-target bytes (uint8 [R]: 0 for a
    ``REC_FAST`` ply and for rows of cut games) and root values (float32 [R]: NaN for a ply without ``REC_VALUE`` and for rows of
    cut games), written by the same launch; the mirror row carries its ply's. With ``out`` they are no flags: the tuple may carry
    a 4th (targets) and 5th (values) ring tensor of the length of ``z``, written at the same ``head_row``.
    Asynchronous on the current stream. reference game.py:213-237 + collect.py:64-131 (preprocess, flip_data)."""
    R = rows_of_records(records.numel() // _lib.REC_BYTES, flags)
    dev = records.device
    if out is None:
        states = torch.empty((R, 17, 7, 10, 9), dtype=torch.float16, device=dev)
        pi = torch.empty((R, NMOVES), dtype=torch.float32, device=dev)
        z = torch.empty((R,), dtype=torch.float32, device=dev)
        target = torch.empty((R,), dtype=torch.uint8, device=dev) if targets else None
        value = torch.empty((R,), dtype=torch.float32, device=dev) if values else None
        ring = 0
    else:
        states, pi, z = out[:3]
        ring = int(z.shape[0])
        if not (states.is_contiguous() and pi.is_contiguous() and z.is_contiguous() and states.shape[0] == ring and pi.shape[0] == ring
                and states.dtype == torch.float16 and pi.dtype == torch.float32 and z.dtype == torch.float32):
            raise ValueError("out must be contiguous (states fp16 [N,17,7,10,9], pi f32 [N,2086], z f32 [N])")
        target = _side_ring("out[3]", out[3], torch.uint8, dev, ring) if len(out) > 3 and out[3] is not None else None
        value = _side_ring("out[4]", out[4], torch.float32, dev, ring) if len(out) > 4 and out[4] is not None else None
    _expand(records, flags, plane_of_type, (states, pi, z), ring, head_row, bad, target, value)
    return (states, pi, z) + ((target,) if target is not None else ()) + ((value,) if value is not None else ())


def expand_record_targets(records: torch.Tensor, flags: int = 0, out=None, head_row: int = 0) -> torch.Tensor:
    """The policy-target byte (1 = target, 0 = a ``REC_FAST`` ply) of every row :func:`expand_records` writes for ``records``
    (its ``targets`` output alone: the same launch without the rows): uint8 [R], the mirror row carries its ply's flag, rows of cut
    games get 0. ``out``: a uint8 ring [N] written at (head_row + i) % N, as :func:`expand_records` writes its ``out``.
    Asynchronous on the current stream."""
    if out is None:
        target = torch.zeros((rows_of_records(records.numel() // _lib.REC_BYTES, flags),), dtype=torch.uint8, device=records.device)
    else:
        target = _side_ring("out", out, torch.uint8, records.device)
    _expand(records, flags, None, None, 0 if out is None else int(target.shape[0]), head_row, None, target, None)
    return target


def expand_record_values(records: torch.Tensor, flags: int = 0, out=None, head_row: int = 0) -> torch.Tensor:
    """The root value (``REC_VALUE`` plies: record bytes 92..95, the side to move's view) of every row :func:`expand_records`
    writes for ``records`` (its ``values`` output alone): float32 [R], the mirror row carries its ply's value, NaN for a ply
    without a value and for rows of cut games. ``out``: a float32 ring [N] written at (head_row + i) % N. Asynchronous."""
    if out is None:
        value = torch.full((rows_of_records(records.numel() // _lib.REC_BYTES, flags),), float("nan"), dtype=torch.float32, device=records.device)
    else:
        value = _side_ring("out", out, torch.float32, records.device)
    _expand(records, flags, None, None, 0 if out is None else int(value.shape[0]), head_row, None, None, value)
    return value


# ---------------------------------------------------------------------- MCTS-solver helpers
def proof_move(state, dist, child_state, child_dist, acts):
    """The move a front-end should force on ONE board given :meth:`SelfPlayEngine.root_proof` (``state`` / ``dist`` of its root, the
    children's rows) and ``root_children()['acts']``: under a WIN root the LOSS child with the smallest distance (the fastest mate;
    the first in insertion order on ties), under a LOSS root the WIN child with the largest distance (the longest defence), else
    None. ``child_state`` / ``child_dist`` / ``acts`` may be whole 128-entry rows: entries past the children have state 0."""
    cs, cd = np.asarray(child_state, np.int64), np.asarray(child_dist, np.int64)
    st = int(state)
    if st == _lib.PROOF_WIN:
        idx = np.nonzero(cs == _lib.PROOF_LOSS)[0]
        if len(idx):
            return int(acts[int(idx[int(np.argmin(cd[idx]))])])
    elif st == _lib.PROOF_LOSS:
        idx = np.nonzero(cs == _lib.PROOF_WIN)[0]
        if len(idx):
            return int(acts[int(idx[int(np.argmax(cd[idx]))])])
    return None


def mate_score(child_state, child_dist):
    """``score mate N`` of a move whose child carries (``child_state``, ``child_dist``): N in moves, positive when the side that
    plays the move mates, negative when it is mated; None for an unproven or drawn child. The child is LOSS in d plies: the mover
    mates in (d + 1) plies; WIN in d: the mover is mated in d + 1."""
    st, d = int(child_state), int(child_dist) + 1
    if st == _lib.PROOF_LOSS:
        return (d + 1) // 2
    if st == _lib.PROOF_WIN:
        return -((d + 1) // 2)
    return None


def proof_combine(cases, device: int = 0) -> np.ndarray:
    """The solver's combine rule on the GPU (``ccz_proof_combine``, one wave per case): ``cases`` = lists of up to 128 proof bytes;
    returns the byte of each case's parent, uint8 [n]."""
    L = _lib.lib()
    dev = torch.device("cuda", device)
    n = len(cases)
    rows = np.zeros((n, MAX_LEGAL), np.uint8)
    counts = np.zeros(n, np.int32)
    for i, c in enumerate(cases):
        if len(c) > MAX_LEGAL:
            raise ValueError("a node has at most 128 children")
        rows[i, :len(c)] = np.asarray(c, np.uint8)
        counts[i] = len(c)
    d_rows, d_counts = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
    out = torch.zeros((n,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L.ccz_proof_combine(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), _ptr(d_rows), _ptr(d_counts), n, _ptr(out)))
    return out.cpu().numpy()


def snapshot_layout(n_nodes, ply, pi_used, sections: int = 2, device: int = 0) -> np.ndarray:
    """The snapshot's layout scan on the GPU (``ccz_snapshot_layout``): the exclusive scan, in 64 bits, of the section sizes of B
    boards with the given counts (arrays or device tensors); returns uint64 [B + 1], the last entry their sum. ``sections``:
    ``snapshot.SNAP_PROOF | snapshot.SNAP_VALUES``. Only the count and offset arrays are allocated."""
    L = _lib.lib()
    dev = torch.device("cuda", device)

    def dev_i32(x, np_dtype):
        if isinstance(x, torch.Tensor):
            return x.to(dev).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np_dtype).view(np.int32)).to(dev)
    d_n, d_p, d_u = dev_i32(n_nodes, np.int32), dev_i32(ply, np.int32), dev_i32(pi_used, np.uint32)
    B = int(d_n.numel())
    if B < 1 or d_p.numel() != B or d_u.numel() != B:
        raise ValueError("n_nodes, ply and pi_used must have the same length >= 1")
    off = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(L.ccz_snapshot_layout(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), B, _ptr(d_n), _ptr(d_p), _ptr(d_u), int(sections), _ptr(off)))
    return off.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------------- stateless batch rules
def legal_moves(squares, turn, halfmove=None, device: int = 0):
    """Legal-move bitmask / count / flags of n positions on the GPU (replaces cchess legal_moves).

    squares uint8 [n,90], turn [n]. Returns (mask bool [n,2086], count int32 [n], flags uint8 [n]).
    """
    L = _lib.lib()
    if not torch.cuda.is_available():
        raise CczError("no GPU visible to PyTorch-ROCm; the engine has no CPU fallback")
    dev = torch.device("cuda", device)
    sq = np.zeros((len(squares), SQ_STRIDE), np.uint8)
    sq[:, :90] = np.asarray(squares, np.uint8)
    n = sq.shape[0]
    d_sq = torch.from_numpy(sq).to(dev)
    d_turn = torch.from_numpy(np.ascontiguousarray(turn, dtype=np.uint8)).to(dev)
    d_half = None if halfmove is None else torch.from_numpy(np.ascontiguousarray(halfmove, dtype=np.int32)).to(dev)
    d_mask = torch.zeros((n, _lib.MASK_WORDS), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros((n,), dtype=torch.int32, device=dev)
    d_flags = torch.zeros((n,), dtype=torch.uint8, device=dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(L.ccz_legal_moves(s, n, _ptr(d_sq), _ptr(d_turn), _ptr(d_half), _ptr(d_mask), _ptr(d_cnt), _ptr(d_flags)))
    words = d_mask.cpu().numpy().view(np.uint32)
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :NMOVES].astype(bool)
    return bits, d_cnt.cpu().numpy(), d_flags.cpu().numpy()


def apply_moves(squares, turn, move_ids, device: int = 0):
    L = _lib.lib()
    dev = torch.device("cuda", device)
    sq = np.zeros((len(squares), SQ_STRIDE), np.uint8)
    sq[:, :90] = np.asarray(squares, np.uint8)
    n = sq.shape[0]
    d_sq = torch.from_numpy(sq).to(dev)
    d_turn = torch.from_numpy(np.ascontiguousarray(turn, dtype=np.uint8)).to(dev)
    d_ids = torch.from_numpy(np.ascontiguousarray(move_ids, dtype=np.int32)).to(dev)
    d_cap = torch.zeros((n,), dtype=torch.uint8, device=dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(L.ccz_apply_moves(s, n, _ptr(d_sq), _ptr(d_turn), _ptr(d_ids), _ptr(d_cap)))
    return d_sq.cpu().numpy()[:, :90], d_turn.cpu().numpy(), d_cap.cpu().numpy()
