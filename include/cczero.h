/*
 * cczero.h -- C ABI of libcczero.so: the MI355X (gfx950) lockstep self-play rollout engine.
 *
 * Drop-in boundary for the ONE hot path of Symb0x76/ChineseChessZero:
 * per-move MCTS select / expand / backup (reference mcts.py:101-178), the rules the reference
 * takes from `cchess` (move generation, make-move, game-end and draw predicates; call sites
 * mcts.py:111-126, net.py:154-157, game.py:201-216, tools.py:109-123), leaf encoding for the
 * evaluator (net.py:160-177, tools.py:74-106), pi / Dirichlet-mixed move choice
 * (mcts.py:163-166,216-224), tree reuse (mcts.py:168-178) and the self-play bookkeeping of
 * game.py:133-237 + collect.py:64-131 (training tuples, mirror augmentation).
 *
 * The reference is pure Python and has no FFI; what it has is a call surface
 * (policy_value_fn / MCTS_AI / Game.start_self_play / CollectPipeline). The Python mirror of
 * that surface (chinesechesszero_amd/{mcts,game,collect,net,tools}.py) binds these entry points
 * with ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - B boards advance in lockstep; one 64-lane wavefront owns one board.
 *   - every function returns 0 on success, <0 on error (ccz_last_error() has the text); nothing
 *     throws across the ABI.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all
 *     device work is enqueued on it; functions documented "syncs" wait for that stream.
 *   - pointers named *_dev are device pointers owned by the caller (torch tensors); *_host are
 *     host pointers. Everything else is owned by the engine.
 *   - single caller thread per engine, no re-entrancy (same as the reference).
 *   - there is NO CPU fallback: every entry point that computes fails if no gfx950 device is
 *     usable.
 */
#ifndef CCZERO_H
#define CCZERO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCZ_ABI_VERSION 9           /* ABI 9: ccz_expand_records / ccz_sample_records write target_dev / value_dev themselves; the four ccz_*_record_targets / _values calls are gone */
#define CCZ_NSQ 90
#define CCZ_SQ_STRIDE 96            /* mailbox row stride in bytes (90 squares + 6 pad)         */
#define CCZ_NMOVES 2086             /* action space, reference tools.py:172-272                 */
#define CCZ_MAX_LEGAL 128           /* upper bound on legal moves of one position               */
#define CCZ_MASK_WORDS 66           /* ceil(2086/32): legal-move bitmask words                  */
#define CCZ_PLANES 10710            /* 17*7*10*9 evaluator input elements, net.py:174-177       */

/* piece codes in the mailbox: 0 empty, red = type, black = type + 8;
 * types PAWN=1 CANNON=2 ROOK=3 KNIGHT=4 BISHOP=5 ADVISOR=6 KING=7 (the engine's own numbering; the plane
 * channel a type is encoded into is ccz_config.plane_of_type, default type-1 as tools.py:100 computes it)
 * colours as in cchess: RED = 1 (True), BLACK = 0 (False). square = file + 9*rank (tools.py:91). */

/* ccz_config.rule_flags: rule variants of the absent `cchess` module that cannot be checked here */
#define CCZ_RULE_PAWN_MOVE_RESETS_CLOCK 2u /* the sixty-move clock (and the repetition history with it) restarts on pawn
                                       moves as well as on captures -- python-chess's `is_zeroing`, which a port may have kept;
                                       default: captures only. A pawn never moves backwards, so no earlier position can recur */
#define CCZ_RULE_PERPETUAL_CHECK 1u /* a game that ends by fourfold repetition is examined for perpetual check: inside the
                                       repetition window (the positions after the EARLIEST occurrence of the repeated position,
                                       up to the current one) a side whose every move gave check, while not every move of the
                                       other side did, LOSES (winner = the other side); both or neither: draw, as without the
                                       flag. Changes outcome().winner only (game.py:210-216, z of the tuples): in the search
                                       the same leaf is `end and is_tie` -> 0.0 either way (mcts.py:120-122), visit counts do
                                       not depend on it. This build's statement of the rule: python-chinese-chess may apply
                                       one [unverified]; default off                                                    */

/* flags for ccz_config.flags */
#define CCZ_FLAG_REFERENCE_QUIRKS 1u /* harvest(): reproduce game.py:234-237 (all samples carry the
                                        final 8-ply history) and collect.py:78 (turn plane all ones) */
#define CCZ_FLAG_NO_MIRROR 2u        /* harvest(): do not append collect.py:112-131 mirror samples  */
#define CCZ_FLAG_VALUE_F16 4u        /* reference CUDA-path quirk: under autocast (net.py:178-189) the value reaches
                                        Node.update as a float16 ndarray and NumPy accumulates Node.value in float16
                                        (mcts.py:63-71 under NEP 50). With this flag the leaf value is rounded to float16
                                        and every operation of the incremental mean rounds to float16; default (off) is
                                        the float32 arithmetic of the reference's CPU path                              */

#define CCZ_FLAG_CACHE_VERIFY 8u     /* debug mode of the evaluation cache (ABI 5): one table hit in 128 is sent through the evaluator
                                        again and its fresh priors / value are compared, bit for bit, with what the table
                                        returned (ccz_stats.cache_verified / cache_verify_mismatches). Results are unchanged;
                                        the evaluator computes ~0.8 % of the hits again. Needs eval_cache_log2 > 0           */

#define CCZ_FLAG_STRICT 16u          /* parity mode (ABI 7): the two places where this engine silently departs from the reference become
                                        sticky error bits instead of counters -- a kept subtree that had to be pruned to fit the node
                                        pool (CCZ_ERR_PRUNED; the reference's tree is unbounded, mcts.py:31-39) and a game adjudicated
                                        at max_plies (CCZ_ERR_TRUNCATED; the reference's game ends by the rules only, game.py:155).
                                        The search results are what they are without the flag; MCTS_AI, the UCI loop and the parity
                                        tests run with it, the throughput paths (bench, collector) count and report instead          */

/* leaf status written by ccz_select_leaves */
#define CCZ_LEAF_EXPAND 0 /* non-terminal: children are created from the evaluator's priors */
#define CCZ_LEAF_DRAW 1   /* game over and is_tie(): leaf value 0.0   (mcts.py:120-122)   */
#define CCZ_LEAF_LOSS 2   /* side to move has no legal move: leaf value -1.0 (mcts.py:123-126) */
#define CCZ_LEAF_NONE 3   /* no pending leaf: board finished, simulation budget used up, leaf already backed up, or nothing selected yet */
#define CCZ_LEAF_WIN 4    /* MCTS-solver only (ccz_set_solver): the descent ended at a node proven won for its side to move: leaf value +1.0 */

typedef struct ccz_engine ccz_engine;

typedef struct ccz_config {
    int32_t n_boards;      /* B: concurrent boards on this GPU                                   */
    int32_t n_playout;     /* simulations per move (parameters.py:14 PLAYOUT; informational)    */
    float c_puct;          /* parameters.py:8  C_PUCT = 5                                        */
    float eps;             /* parameters.py:10 EPS   = 0.25 (Dirichlet mixing weight); must be in [0, 1] */
    float alpha;           /* parameters.py:12 ALPHA = 0.2; must be finite and > 0. The device widens the float to double
                              (0.2f = 0.20000000298...). A Gamma draw g = G(alpha+1) U^(1/alpha) is flushed to 0 when
                              log(U)/alpha < -708 (det_exp's cutoff), with probability ~exp(-708 alpha): 6e-10 at alpha 0.03,
                              0.09 % at 0.01, 49 % at 0.001 (measured on the twin); when all k draws of a board are 0 the
                              noise is pi itself (k = 2: 1.7 % at 0.003). Exact noise needs alpha >= 0.03 */
    float temp;            /* game.py:133 temp=1.0 ; schedule of game.py:159 applied per board; must be > 0 */
    int32_t max_nodes;     /* tree nodes per board per pool half (0 = 512 x (n_playout + 64))    */
    int32_t max_depth;     /* selection path capacity (0 = 512)                                  */
    int32_t max_plies;     /* recorded plies per game before adjudicating a draw (0 = 2048)      */
    uint32_t flags;        /* CCZ_FLAG_*                                                         */
    uint64_t seed;         /* device-mode sampling: Philox key                                   */
    uint64_t board_id_base;/* global id of board 0 (rank * n_boards): RNG streams independent of GPU count */
    int32_t device;        /* HIP device ordinal                                                 */
    int32_t reserve_nodes; /* pool nodes kept free at re-root time for the next move's expansions
                              (0 = min(128 x n_playout, max_nodes / 2)); the kept subtree is pruned
                              bottom-up to max_nodes - reserve_nodes                            */
    /* ---- the two choices the golden traces cannot pin, as run-time tables (ABI 2) ---------------------
     * move_rank_host: uint16 [2086] host array or NULL. The iteration order of `board.legal_moves`
     *   (net.py:154-157) decides the children's insertion order (mcts.py:37-39), hence which unvisited
     *   child is tried first and how PUCT ties break (mcts.py:47-48,59-61). Legal moves are listed in
     *   ascending move_rank_host[id]; NULL = ascending id (this build's canonical order). Must be a
     *   permutation of 0..2085. Copied at create.
     * type_rank: major sort key by the PIECE TYPE of the mover (index 1..7, entry 0 unused, values 0..7; all zero = no
     *   major key): legal moves are listed in ascending (type_rank[type], move_rank[id]). Bitboard libraries iterate
     *   piece sets, so their order is typically "these piece types first, squares in scan order within" -- e.g. the
     *   python-chess scheme (non-pawn moves by from-square and to-square descending, then pawn moves) is
     *   type_rank = {PAWN: 1, others: 0} with move_rank = the rank of (from, to) in descending order.
     * plane_of_type: channel (0..6) of piece type t = 1..7 inside a colour's 7-plane group, entry 0 unused;
     *   all zero = {-, 0,1,2,3,4,5,6}, i.e. `piece_type - 1` (tools.py:100) under this build's type numbering.
     *   With another cchess PIECE_TYPES numbering only this table changes (reference-trained weights see
     *   their own plane order). Must be a permutation of 0..6. */
    const uint16_t *move_rank_host;
    uint8_t plane_of_type[8];
    uint32_t rule_flags;   /* CCZ_RULE_*                                                         */
    uint32_t eval_cache_log2; /* 0 = none; n = an evaluation cache of 2^n entries of 528 B (ABI 3): see ccz_eval_plan */
    uint8_t type_rank[8];
} ccz_config;

typedef struct ccz_stats {
    int64_t sims;            /* playouts completed since create                                  */
    int64_t moves;           /* moves played                                                     */
    int64_t games;           /* games finished                                                   */
    int64_t truncated_games; /* games adjudicated at max_plies                                   */
    int64_t nodes_peak;      /* max nodes in use on any board                                    */
    int64_t depth_peak;      /* max selection depth seen                                         */
    int64_t sum_depth;       /* sum of leaf depths (for d-bar)                                   */
    int64_t sum_children;    /* sum of children created (for k-bar)                              */
    int64_t expansions;      /* leaves expanded                                                  */
    int64_t terminal_leaves; /* terminal leaves backed up                                        */
    int32_t error_flags;     /* sticky device error bits (CCZ_ERR_*), 0 = healthy                */
    int32_t reserved;        /* -DCCZ_BOUNDS diagnostic build: source line of the last stray index; 0 otherwise */
    int64_t hbm_bytes;       /* device memory held by the engine                                 */
    int64_t pruned_subtrees; /* nodes whose children were dropped at re-root time to keep the kept
                                subtree within the pool budget (0 in normal runs)                 */
    /* evaluation cache (ABI 3; all zero without one) */
    int64_t cache_probes;      /* leaves that needed an evaluation                                */
    int64_t cache_hits;        /* ... served from the cache                                       */
    int64_t cache_shared_rows; /* ... served by the evaluator row of another board of the same step (same position) */
    int64_t cache_stores;      /* entries written                                                 */
    /* CCZ_FLAG_CACHE_VERIFY (ABI 5; zero without it) */
    int64_t cache_verified;          /* table hits that were evaluated again                        */
    int64_t cache_verify_mismatches; /* ... whose fresh priors or value differ from the cached ones: must stay 0 (a colliding
                                        position, a non-deterministic evaluator, or weights changed without ccz_eval_cache_clear) */
} ccz_stats;

#define CCZ_ERR_NODE_POOL 1   /* a board ran out of tree nodes (raise max_nodes)                 */
#define CCZ_ERR_DEPTH 2       /* a selection path exceeded max_depth                             */
#define CCZ_ERR_CHAIN 64      /* more than 128 positions since the last capture (history chain)  */
#define CCZ_ERR_MOVES 4       /* more than CCZ_MAX_LEGAL legal moves / pseudo-move overflow       */
#define CCZ_ERR_RECORD 8      /* pi record arena overflow (game adjudicated)                     */
#define CCZ_ERR_BAD_MOVE 16   /* forced move id invalid / nothing searched and nothing forced    */
#define CCZ_ERR_NAN 32        /* NaN priors: no comparable child during selection                */
#define CCZ_ERR_BOUNDS 128    /* bounds-checked diagnostic build only (-DCCZ_BOUNDS): an index left its array      */
#define CCZ_ERR_PRUNED 256    /* CCZ_FLAG_STRICT: a kept subtree lost nodes at re-root time (raise max_nodes / lower reserve_nodes) */
#define CCZ_ERR_TRUNCATED 512 /* CCZ_FLAG_STRICT: a game reached max_plies and was adjudicated a draw (raise max_plies)            */
#define CCZ_ERR_BAD_TEMP 1024 /* a per-board temperature (ccz_finish_move temps_dev) that is NaN or <= 0: that board neither records nor moves */

/* ---- library ---------------------------------------------------------------------------- */
int ccz_abi_version(void);
const char *ccz_last_error(void);
/* number of usable gfx950 devices (0 if none); never initialises more than the runtime needs */
int ccz_device_count(void);

/* ---- action space (replaces reference tools.py:172-272 tables and tools.py:133-166 flip) - */
/* uci_out: 2086 x 5 bytes, NUL-terminated 4-char strings ("a0a1") */
int ccz_action_table(char *uci_out_host, uint8_t *from_out_host, uint8_t *to_out_host);
int ccz_flip_map(int32_t *flip_out_host); /* collect.py:118-123 */

/* ---- engine lifetime --------------------------------------------------------------------- */
int ccz_create(const ccz_config *cfg, ccz_engine **out);
int ccz_destroy(ccz_engine *e);
/* start new games (standard opening, fresh trees, empty records) on the boards whose mask byte is
 * non-zero; mask_host == NULL means all boards. Replaces cchess.Board() + reset_player()
 * (game.py:148, mcts.py:200-201). */
int ccz_reset(ccz_engine *e, void *stream, const uint8_t *mask_host);
/* set an arbitrary root position on one board (fresh tree, game record restarted); for tests and
 * match play. sq_host: 90 piece codes. */
int ccz_set_position(ccz_engine *e, void *stream, int32_t board, const uint8_t *sq_host,
                     int32_t turn, int32_t halfmove);
/* Load MANY boards, each with the moves that led to its position, in one launch (one wave per board) -- and with no host
 * sync when mask_host == NULL. All arrays are in device memory: sq_dev uint8 [B*96] (90 piece codes per board, 4-byte aligned),
 * turn_dev uint8 [B], halfmove_dev int32 [B] (NULL: 0), moves_dev int32 [B*max_moves] (move ids, applied to the given position in
 * order), n_moves_dev int32 [B] (NULL: no moves), status_dev int32 [B] (output). mask_host as in ccz_reset.
 * For every masked board the kernel validates the position (piece codes, exactly one king and at most 16 pieces per side, clock
 * >= 0), replays the moves with the engine's own rules -- every move must be in the legal-move set of the position it is played
 * in: the generator and rule tables (move_rank_host, type_rank, rule_flags) of the selection --, keeping key, turn, clock, history
 * chain and in-check bits exactly as ccz_finish_move does per ply (CCZ_RULE_PAWN_MOVE_RESETS_CLOCK and the chain restart on
 * captures included), and, if moves were played, runs ccz_finish_move's game-end test on the position reached (the positions on
 * the way are not tested). It finishes as a new game does: fresh root, empty record, ply 0, game number + 1, no pending leaf.
 * With no moves the board is left field for field as ccz_set_position leaves it. ccz_stats.moves / .games are not touched.
 *   status: 0 loaded; 1 + i: move i is not legal where it is played; -1: invalid position (also: a move count outside
 *   -1 .. max_moves); -2: more than 128 positions since the last capture (the history chain).
 * Bad input is the caller's mistake, not an engine fault: no sticky error bit is set, the board is PARKED. So is, on request, a
 * board whose n_moves entry is -1 (status 0). A parked board is over = 1, winner = -1, ply = 0, an empty mailbox and a root without
 * children: the simulator skips it (CCZ_LEAF_NONE: no evaluator row), ccz_harvest_rows counts nothing for it, ccz_harvest and
 * ccz_harvest_records emit nothing for it and leave it alone; it stays parked until ccz_reset, ccz_set_position or
 * ccz_set_positions loads it. (The harvest calls skip every finished board without a recorded ply: a loaded position that is
 * already decided is such a board as well.) */
int ccz_set_positions(ccz_engine *e, void *stream, const uint8_t *sq_dev, const uint8_t *turn_dev, const int32_t *halfmove_dev,
                      const int32_t *moves_dev, const int32_t *n_moves_dev, int32_t max_moves, const uint8_t *mask_host,
                      int32_t *status_dev);
/* fresh root `Node(None, 1.0)` on the boards whose mask byte is non-zero (NULL = all), keeping position,
 * history chain, game record and clocks: MCTS.update_with_move(-1) (mcts.py:176-178, what reset_player() and
 * the non-self-play branch of get_action call, mcts.py:200-201,228-229). The pending leaf is dropped. */
int ccz_reset_tree(ccz_engine *e, void *stream, const uint8_t *mask_host);

/* ---- one lockstep simulation = select -> (evaluator) -> expand+backup --------------------- */
/* Replaces the first half of MCTS.playout (mcts.py:101-111) + policy_value_fn's input building
 * (net.py:154-177) for all boards: PUCT descent from each root with make-move, legal-move
 * generation and game-end tests at the leaf, and the evaluator input written to
 * leaf_input_f16_dev [B,17,7,10,9] fp16. Only plane groups 7, 15 and 16 are ever non-zero on this
 * path (net.py:160-173); the engine rewrites those three and assumes the other 14 groups are zero
 * (ccz_zero_leaf_input zeroes the whole tensor once). ccz_set_leaf_history replaces this row by the eight-position row a
 * training sample holds. */
int ccz_select_leaves(ccz_engine *e, void *stream, void *leaf_input_f16_dev);
int ccz_zero_leaf_input(ccz_engine *e, void *stream, void *leaf_input_f16_dev);
/* Replaces the second half of MCTS.playout (mcts.py:113-129): Node.expand with priors
 * prob_dev[b, id] (float32 [B,2086] = exp(log_act_probs), net.py:202-203) for the leaf's legal ids
 * in ascending id order, leaf value value_dev[b] (float32 [B], side to move's view) or the terminal
 * value, and Node.update_recursive up the path. */
int ccz_expand_backup(ccz_engine *e, void *stream, const float *prob_dev, const float *value_dev);

/* Fused form of "ccz_expand_backup for the pending leaf, then ccz_select_leaves for the next
 * simulation" in ONE launch (one launch boundary and one tree-head re-read less per simulation).
 * A move of n simulations is: select, (evaluator, step) x (n-1), evaluator, expand_backup. */
int ccz_step(ccz_engine *e, void *stream, const float *prob_dev, const float *value_dev,
             void *leaf_input_f16_dev);

/* Compact evaluator boundary: the evaluator hands over the policy head's LOGITS (float32 or float16
 * [B,2086], before log_softmax). ccz_gather_priors computes exp(log_softmax(logits)) for the pending leaf's
 * legal ids only (net.py:202-205 use exactly those) in one pass per board into an engine-owned [B,128] row;
 * ccz_step_compact / ccz_expand_backup_compact are ccz_step / ccz_expand_backup reading that row. Two full
 * [B,2086] passes less on the evaluator side and no scattered prior gather inside the simulator kernel. */
int ccz_gather_priors(ccz_engine *e, void *stream, const void *logits_dev, int32_t logits_f16);
int ccz_step_compact(ccz_engine *e, void *stream, const float *value_dev, void *leaf_input_f16_dev);
int ccz_expand_backup_compact(ccz_engine *e, void *stream, const float *value_dev);

/* ---- scouts (round 6, ABI 7): the next leaves of a board, evaluated before it asks for them -------------------------------------
 * The reference's first-maximum rule (mcts.py:47-48,59-61: an unvisited child scores +inf and max() returns the first one) fixes the
 * order in which a node's children are first visited: the order of board.legal_moves. When a board's pending leaf is child i of a
 * node, the simulations that reach that node next will ask for children i + 1, i + 2, ... One game at a time (MCTS_AI, the UCI loop:
 * one 90-pixel row per evaluator call) therefore runs with SCOUT SLOTS: the last n_scouts boards of the engine have no tree and no
 * game; ccz_scout hands slot active + j * active + r the (i + 1 + j)-th child of board r's pending leaf's parent as its pending leaf
 * (position, legal moves, status, key, evaluator input row), ccz_eval_plan_scouted probes the evaluation cache for every slot and
 * plans ONE evaluator call of all n_boards rows (row b = slot b; *n_miss_dev = n_boards) iff a searched board misses, else none
 * (*n_miss_dev = 0; state_dev[r] = 0 miss / 1 hit / 2 no evaluation needed, for the host to branch on); ccz_gather_priors_planned
 * then stores the scouts' evaluations in the table, where board r finds them. The simulator entry points (select / step /
 * expand_backup / finish_move) run on boards 0 .. n_boards - n_scouts - 1 only. Same visit counts, bit for bit: the table returns
 * what the evaluator returns for the position, and the evaluator's result for a row does not depend on the batch it sits in. */
int ccz_set_scouts(ccz_engine *e, int32_t n_scouts);
int ccz_scout(ccz_engine *e, void *stream, void *leaf_input_f16_dev);
int ccz_eval_plan_scouted(ccz_engine *e, void *stream, int32_t *miss_rows_dev, int32_t *n_miss_dev, int32_t *state_dev);
/* ccz_scout + ccz_eval_plan_scouted as ONE launch (engines of up to 16 slots: one workgroup, one wave per slot; more: the three launches) */
int ccz_scout_and_plan(ccz_engine *e, void *stream, void *leaf_input_f16_dev, int32_t *miss_rows_dev, int32_t *n_miss_dev, int32_t *state_dev);
/* Simulations of a scouted engine (at most 16 slots) WITHOUT the host in between: ONE launch, one workgroup, repeats
 * { ccz_step_compact (expand + backup of the pending leaves from the engine's prior / value rows, next selection) ; ccz_scout_and_plan }
 * for as long as every searched board finds its next leaf in the table (or needs no evaluation). It returns to the host when the
 * evaluator has to run, after run_dev[0] simulations (a caller that reports progress), or when the move's last simulation -- which has
 * no next selection: ccz_expand_backup_compact -- is backed up. run_dev: four int32 the device can reach (device or pinned host memory):
 *   [0] in:  budget, >= 1            [1] in:  simulations left in this move, the pending one included, >= 1
 *   [2] out: simulations done here   [3] out: 1 = a searched board's leaf needs the evaluator now (the plan and state_dev are then what
 *                                            ccz_scout_and_plan would have left), 0 = budget or move exhausted
 * Call it where ccz_step_compact would be called: the pending leaves' priors and values are in place (ccz_gather_priors_planned, or a
 * table hit). Same phases in the same order on the same data as the separate launches: same trees, bit for bit
 * (tests/test_gpu_scouts.py). mcts.py:101-129 is the loop this runs; the reference's one-evaluation-per-playout is the path it skips. */
int ccz_scouted_run(ccz_engine *e, void *stream, void *leaf_input_f16_dev, int32_t *miss_rows_dev, int32_t *n_miss_dev, int32_t *state_dev,
                    int32_t *run_dev);

/* Evaluation cache (ccz_config.eval_cache_log2 > 0). On the search path the evaluator sees the leaf POSITION and the side to move
 * only (net.py:160-173: the history planes are zero; mcts.py:214 passes none), i.e. a function of the leaf's Zobrist key (with
 * ccz_set_leaf_history on: of the leaf's HISTORY KEY, which stands in for the Zobrist key in everything below). The
 * reference evaluates every leaf on its own (mcts.py:114); here a position that was evaluated before -- by this board (a
 * transposition), by another board (every restarted game walks through openings that earlier games searched), or by another
 * board in this very step -- is not sent through the network again. Results are unchanged bit for bit as long as the evaluator is
 * a deterministic function of the position that does not depend on the row it sits in (tests/test_gpu_evaluator_depth.py) --
 * up to key collisions: a hit needs the 64-bit key, the number of legal moves AND a 24-bit hash of the legal-move list (in the
 * order the priors are stored in) to agree, so a foreign position is served with probability < 2^-64 per probe (about 1e-9 per
 * day at 2 x 10^5 probes a second); CCZ_FLAG_CACHE_VERIFY re-evaluates a sample of the hits and counts disagreements.
 *   ccz_eval_plan: probes the direct-mapped table (2^n entries: key, value, the priors of the legal moves) for every pending
 *     leaf that needs an evaluation; hits receive their priors and value at once. The misses are deduplicated (boards with the
 *     same key share one row) and compacted: miss_rows_dev int32 [B] receives the board index of every row the evaluator has to
 *     compute, ascending; *n_miss_dev (int32 on the device) their number. No host sync.
 *   The evaluator then runs on those rows only: ccz_pack_live_planes_rows_f16 gathers them, the ccz_conv3x3_*_live entry points
 *     skip the tiles beyond the live rows; logits / values come back COMPACT: row i belongs to board miss_rows_dev[i].
 *   ccz_gather_priors_planned: ccz_gather_priors for the misses (each reads the row of its representative), and the fresh
 *     evaluations are stored in the table. Afterwards ccz_step_compact / ccz_expand_backup_compact with value_dev == NULL use
 *     the engine-owned leaf values (hits: from the table; misses: value_compact_dev[row]).
 *   ccz_eval_cache_clear: forget everything (the evaluator's weights changed). */
int ccz_eval_plan(ccz_engine *e, void *stream, int32_t *miss_rows_dev, int32_t *n_miss_dev);
int ccz_gather_priors_planned(ccz_engine *e, void *stream, const void *logits_compact_dev, int32_t logits_f16,
                              const float *value_compact_dev);
int ccz_eval_cache_clear(ccz_engine *e, void *stream);

/* ---- leaf history planes (additive to ABI 9) -------------------------------------------------------------------------------------
 * The rows the collector trains on (ccz_harvest, default mode) show eight positions; the search above shows the net one, in the
 * groups where a row holds the position of seven plies ago. With the option on, every select phase (ccz_select_leaves, ccz_step,
 * ccz_step_compact) is followed by one more launch that rewrites ALL 17 groups of the row of every board with a pending leaf to
 * evaluate (CCZ_LEAF_EXPAND; other boards' rows are unspecified, as before):
 *   p = the plies recorded in the board's current game, S_0 .. S_{p-1} = their root positions, S_p = the root, S_{p+1} .. S_{p+d} = the
 *   positions along the selection path to the leaf at depth d, te = p + d. History slot i (0..7) shows S_{max(te - i, 0)} -- the clamp
 *   of the rows (the reference's reset_states_history padding). Groups 0..7 hold the red pieces of slots 0..7, groups 8..15 the black
 *   ones, group 16 is all ones iff red is to move at the leaf; channels follow plane_of_type. That is, byte for byte, the state
 *   ccz_harvest writes (pass 0) for ply te of a game played along that path.
 * Cache key rule: "equal keys = equal evaluator input" must hold, and with history the input is no function of the leaf position. The
 * same launch therefore replaces the board's key by the HISTORY KEY
 *   mix64(leaf_key ^ h_7),  h_0 = 0x9E3779B97F4A7C15, h_i = mix64(h_{i-1} ^ P(slot i)),  i = 1..7,
 * P(S) = the XOR of the Zobrist words of S's pieces (no side to move), mix64 = the splitmix64 finaliser. The hash depends on the
 * positions shown, not on where they come from: a clamped prefix and a real repeat of the same positions hash alike, as their input
 * is alike. Every reader of the key (probe, plan, same-step sharing, the routing salts, verify mode, ccz_leaf_keys) sees the history
 * key and works unchanged; a transposition reached by another move order is now another input and misses.
 *   ccz_set_leaf_history: host-side, takes effect with the next select phase (`stream` is unused). Enabling fails with scout slots
 *     (ccz_set_scouts), with a width above 1 (ccz_set_width) and on CCZ_FLAG_REFERENCE_QUIRKS engines (their rows alias the final
 *     history, which no search sees); ccz_set_scouts(n > 0) and ccz_set_width(width > 1) fail while it is on. The select calls then
 *     need a non-null leaf input. After turning it OFF the caller must call ccz_zero_leaf_input once: the old path rewrites groups
 *     7, 15 and 16 only. A hipGraph captured before the call does not hold the new launch: capture again. Flush the evaluation cache
 *     when the setting changes (ccz_eval_cache_clear): keys of the two modes name different inputs.
 *   Positions loaded by ccz_set_position(s) start a game at ply 0: the moves that led there are no history, the clamp repeats the
 *     loaded position. */
int ccz_set_leaf_history(ccz_engine *e, void *stream, int32_t enabled);
int ccz_get_leaf_history(ccz_engine *e, int32_t *enabled_host);
/* The evaluator's side of it: ALL 119 planes of a row, where ccz_pack_live_planes_* keep the 21 of groups 7, 15 and 16.
 *   ccz_pack_planes128_f16 / _g16_f16 / _rows_f16: dense [B,17,7,10,9] fp16 -> NHWC rows of 128 channels (119 + 9 zeros), board-major /
 *     group-of-16 / planned rows: the three ccz_pack_live_planes* entry points with x128_dev [rows, 128] for x64_dev, the same rows /
 *     n_rows conventions; every byte of a written row is written (no pre-zeroed buffer is assumed).
 *   ccz_conv3x3_stem128_f16[_live]: ccz_conv3x3_stem_f16[_live] at cin = 128 -- the GENERAL tile forms (k_conv3x3_c256 with two 64-channel
 *     chunks, k_conv3x3_g16 with four 32-channel chunks under CCZ_CONV_G16), not the one-chunk stem form; weights [256, 3, 3, 128]
 *     (under CCZ_CONV_G16: packed by ccz_pack_conv_weights_g16_f16 with cin = 128). Flags: ReLU, tile order, CCZ_CONV_G16. There is no small-
 *     batch form and no G16C form at 128 channels: any batch runs the tile kernel, and a tower that follows runs on rows. */
int ccz_pack_planes128_f16(void *stream, const void *leaf_dev, void *x128_dev, int32_t n_boards);
int ccz_pack_planes128_g16_f16(void *stream, const void *leaf_dev, void *x128_dev, int32_t n_boards, const int32_t *rows_dev, const int32_t *n_rows_dev);
int ccz_pack_planes128_rows_f16(void *stream, const void *leaf_dev, void *x128_dev, int32_t n_boards, const int32_t *rows_dev, const int32_t *n_rows_dev);
int ccz_conv3x3_stem128_f16(void *stream, const void *x128_dev, const void *w_dev, const void *bias_f32_dev, void *y_dev, int64_t n_pixels, int32_t relu);
int ccz_conv3x3_stem128_f16_live(void *stream, const void *x128_dev, const void *w_dev, const void *bias_f32_dev, void *y_dev, int64_t n_pixels, int32_t relu,
                                 const int32_t *live_rows_dev, int32_t part, int32_t n_parts);

/* Two evaluators on one engine (an arena between two networks; needs the evaluation cache, no scout slots). The reference's
 * Game.start_play (game.py:77-130) with two MCTS_AI players: the player to move at the ROOT searches with its own network, which
 * evaluates every leaf of that search whoever is to move there; the tree is discarded after the move. So board b's evaluator is
 * fixed for a whole move: red_net[b] when red is to move at the root, 1 - red_net[b] when black is.
 *   ccz_set_routing: red_net_host uint8 [B] (0 or 1) = the evaluator that plays red on each board (NULL: routing off); salt0 /
 *     salt1 (must differ) are XORed into the cache key of each evaluator's entries -- slot and stored key alike -- so one table holds
 *     both networks' evaluations and never serves one network's to the other. New weights for one network: give it a new salt (its
 *     old entries can then never hit; the other network's stay valid).
 *   ccz_eval_plan_routed: ccz_eval_plan with the routing: miss_rows_dev int32 [2B], n_miss_dev int32 [2]. Rows are shared only
 *     between boards of the same evaluator; evaluator 0's rows are miss_rows_dev[0 .. n_miss_dev[0]), evaluator 1's
 *     miss_rows_dev[B .. B + n_miss_dev[1]), each ascending -- so each evaluator runs the planned boundary unchanged on
 *     (miss_rows_dev + e * B, n_miss_dev + e), and both base pointers are known on the host. CCZ_FLAG_CACHE_VERIFY rows land in
 *     their own evaluator's segment.
 *   ccz_gather_priors_routed: ccz_gather_priors_planned with each board reading the compact output (logits_e, value_e) of its own
 *     evaluator and storing under that evaluator's salt. Then ccz_step_compact / ccz_expand_backup_compact with value_dev == NULL. */
int ccz_set_routing(ccz_engine *e, void *stream, const uint8_t *red_net_host, uint64_t salt0, uint64_t salt1);
int ccz_eval_plan_routed(ccz_engine *e, void *stream, int32_t *miss_rows_dev, int32_t *n_miss_dev);
int ccz_gather_priors_routed(ccz_engine *e, void *stream, const void *logits0_dev, const void *logits1_dev, int32_t logits_f16,
                             const float *value0_dev, const float *value1_dev);

/* ---- per-board simulation budgets (additive to ABI 8) ---------------------------------------------------------------------------
 * Every board counts the simulations it has backed up since its last move boundary (ccz_finish_move on a live board, ccz_reset,
 * ccz_set_position(s), a harvest restart, ccz_reset_tree). With budgets on, a board whose count has reached its budget selects
 * nothing more: CCZ_LEAF_NONE, no evaluator row from ccz_eval_plan[_routed], no simulation counted -- exactly as a finished board.
 * A board therefore searches exactly budget[b] simulations per move however many lockstep steps the host runs, and its tree is,
 * bit for bit, the tree of an engine that runs budget[b] steps. Both calls are asynchronous on `stream` (no host sync) and take
 * effect with the next ccz_select_leaves / ccz_step*; both fail while scout slots are active, and ccz_set_scouts fails while
 * budgets are on. After ccz_create budgets are off.
 *   ccz_set_budgets: budgets_dev int32 [B] (an entry below 1 counts as 1), targets_dev uint8 [B] or NULL (all 1): 1 = this move's
 *     pi is a policy target. budgets_dev == NULL: budgets off (unlimited, every move a target; targets_dev is ignored).
 *   ccz_draw_budgets: playout-cap randomisation. Board b draws ua of uniform2(seed, board_id_base + b, its move counter, child
 *     0xffe, draw 0) -- the sampler's Philox stream, a counter word neither the Gamma draws (children 0..127) nor the choice uniform
 *     (0xfff) use: Dirichlet noise and moves are what they are without the call, and a board's budgets do not depend on the GPU
 *     count. ua < p_full: budget n_full, target 1; else budget n_fast, target 0. budgets_out_dev int32 [B] (may be NULL) receives
 *     the budgets. n_full, n_fast >= 1, p_full in [0, 1]. Call it at a move boundary (before the move's first selection).
 * ccz_finish_move stores the board's target byte with the ply; ccz_harvest_records writes it into the record header as
 * flags = target ? 0 : CCZ_REC_FAST. The dense-row calls (ccz_harvest, ccz_expand_records, ccz_sample_records) form a row for
 * every ply as before (a fast ply's pi is still a distribution, and its z a value target); the two calls below hand the flag
 * to the consumer, row-aligned with what their siblings write. */
#define CCZ_REC_FAST 1 /* record header flags: the ply was a fast move of playout-cap randomisation -- keep it out of the policy loss */
int ccz_set_budgets(ccz_engine *e, void *stream, const int32_t *budgets_dev, const uint8_t *targets_dev);
int ccz_draw_budgets(ccz_engine *e, void *stream, int32_t n_full, int32_t n_fast, double p_full, int32_t *budgets_out_dev);

/* ---- self-play resignation with play-on calibration (additive to ABI 8) -----------------------------------------------------------
 * AlphaZero-style: a side resigns when the search's root value stays below a threshold for a few of its moves in a row; a random
 * fraction of such games is played on so that the false-positive rate can be measured; the threshold is set from that
 * measurement. Off after ccz_create: ccz_finish_move then computes, records and counts exactly what it does without the feature
 * (record bytes 90..95 zero, none of the three flags below).
 *   ccz_set_resign: asynchronous on `stream`, takes effect with the next ccz_finish_move. enabled = 0: off (the other arguments are
 *     still validated). threshold finite and in [-1, 0]; consecutive 0..255 (0: values are recorded and the run counters kept, but
 *     nothing ever resigns); min_ply >= 0; p_playon in [0, 1].
 * With the feature on, ccz_finish_move does this on every live board that records a ply, in this order:
 *   1. root value v = sum_i N_i * (double)Q_i / sum_i N_i over the root's k children (what ccz_root_children returns: Q in the view
 *      of the root's side to move), accumulated in child order in float64; no visited child: 0.0. (float)v is stored with the ply.
 *   2. s = side to move. On a full-search ply (target byte 1): run[b][s] = v < (double)threshold ? min(run + 1, 255) : 0. A fast ply
 *      of playout-cap randomisation records v and leaves the counter alone.
 *   3. the rule fires when: full-search ply, consecutive > 0, run[b][s] >= consecutive, ply >= min_ply, no forced move on this board
 *      (a host that forces a move has decided), and the game has not drawn the play-on lot before.
 *   4. on firing, u = ua of uniform2(seed, board_id_base + b, move counter, child 0xffd, draw 0): a word no other draw uses (Gamma:
 *      0..127, budgets: 0xffe, move choice: 0xfff), so noise, moves and budgets are unchanged and the lot does not depend on the GPU
 *      count. u < p_playon: the game is marked CCZ_RESIGN_PLAYON | s with this fire ply, plays its normal move and can never
 *      resign. Otherwise the game ENDS here: the ply is recorded like any other (position, pi, v: the search was done), ply and
 *      move counter advance, no move is pushed (root position, key, clock, history stay), moves_out = -1, over = 1, winner = the
 *      other side, ccz_stats.games + 1, state CCZ_RESIGN_RESIGNED | s.
 *   5. when a play-on game ends (by the rules or at the ply cap) the calibration counters below are updated.
 * A board's state is cleared wherever a new game starts (harvest restart, ccz_reset, ccz_set_position(s)); ccz_reset_tree keeps it.
 * ccz_harvest_records writes CCZ_REC_RESIGNED / CCZ_REC_PLAYON on every ply of such a game, CCZ_REC_VALUE and the float32 value in
 * record bytes 92..95 on a ply that carries one (bytes 90..91 stay zero). The dense-row calls write what they always wrote. */
#define CCZ_REC_RESIGNED 2  /* record header flags: the game ended by resignation (of the side to move at its last ply)  */
#define CCZ_REC_PLAYON 4    /* ... the rule fired in this game and the game was played on                               */
#define CCZ_REC_VALUE 8     /* ... bytes 92..95 of this record hold the ply's root value, float32, side to move's view   */
#define CCZ_REC_VALUE_OFF 92
#define CCZ_RESIGN_RESIGNED 2 /* ccz_resign_status state: bit 0 = the side (1 RED, 0 BLACK) that resigned / would have resigned */
#define CCZ_RESIGN_PLAYON 4
typedef struct ccz_resign_stats {
    int64_t resigned_games;     /* games that ended by resignation                                                      */
    int64_t resigned_by_red;    /* ... in which red resigned                                                             */
    int64_t resigned_plies;     /* sum of their recorded plies T (the resign ply included)                               */
    int64_t playon_games;       /* FINISHED games that drew the play-on lot                                              */
    int64_t playon_won;         /* ... that the side which would have resigned won: the false positives                  */
    int64_t playon_drawn;       /* ... that were drawn (adjudications at the ply cap included)                           */
    int64_t playon_plies_after; /* sum of T - fire ply over them: the plies resignation would have saved                 */
} ccz_resign_stats;
int ccz_set_resign(ccz_engine *e, void *stream, int32_t enabled, float threshold, int32_t consecutive, int32_t min_ply, double p_playon);
int ccz_get_resign_stats(ccz_engine *e, void *stream, ccz_resign_stats *out); /* syncs */
/* per-board state (syncs): state_host uint8 [B] (0, or CCZ_RESIGN_* | side), run_host uint8 [B*2] (run[b][side]), fire_ply_host
 * int32 [B] (-1: the rule has not fired in this game), last_value_host float [B] (the last recorded ply's v; NaN: none in this
 * game); any pointer may be NULL. */
int ccz_resign_status(ccz_engine *e, void *stream, uint8_t *state_host, uint8_t *run_host, int32_t *fire_ply_host, float *last_value_host);

/* ---- policy surprise weighting (additive to ABI 9) -----------------------------------------------------------------------------------
 * KataGo's rule for how often a recorded ply is trained on: a share 1 - alpha of a game's sampling weight is spread evenly over its
 * plies, the share alpha goes to the policy-target plies in proportion to s = KL(search policy || network prior). Off after
 * ccz_create: ccz_finish_move and ccz_harvest_records then read one word of the settings and do exactly what they do without the
 * feature (record bytes 90..91 zero, no CCZ_REC_WEIGHT).
 *   ccz_set_surprise: asynchronous on `stream`, takes effect with the next ccz_finish_move / ccz_harvest_records. alpha in [0, 1],
 *     cap in [1, 15] (validated also with enabled = 0). Refused with scout slots. The call clears the has-bit of every stored ply: a
 *     ply recorded before it carries no surprise.
 * With the feature on, ccz_finish_move stores with every ply it records (a resigned ply is a ply like any other):
 *   target byte 1: s = sum_i pi_i * (det_log(pi_i) - det_log(max((double)P_i, 2^-100))) over the root's children with pi_i > 0, in child
 *     order in float64, a negative sum clamped to 0; (float)s and the has-bit 1. pi is the float64 distribution that is recorded
 *     (rounded to float32 only in the record): the visit softmax at the move's temperature, the pruned-count pi under root exploration,
 *     pi' under the Gumbel root. P_i is the child's stored prior (root noise is never stored).
 *   target byte 0 (a fast ply of playout-cap randomisation): 0 and the has-bit 0.
 * ccz_harvest_records, with the feature on, gives every ply of a harvested game CCZ_REC_WEIGHT and in record bytes 90..91 the uint16
 *   wq = floor(w * 4096 + 0.5), w = min(w', cap), where with F = the game's plies with the has-bit, n = |F| and S = the sum of their
 *   float32 s as doubles in ply order: w' = (1 - alpha) + alpha * n * s_t / S for t in F if S > 0, else 1. A ply with w' > cap counts
 *   in weights_clipped. The dense-row call ccz_harvest writes what it always wrote. */
#define CCZ_REC_WEIGHT 16     /* record header flags: bytes 90..91 of this record hold the ply's sampling weight, uint16 in 1/4096 */
#define CCZ_REC_WEIGHT_OFF 90
#define CCZ_REC_WEIGHT_ONE 4096
typedef struct ccz_surprise_stats { /* sums over boards, taken in board order */
    int64_t target_plies;    /* policy-target plies whose surprise was measured                   */
    double surprise_sum;     /* the sum of their stored float32 surprise                          */
    int64_t weights_clipped; /* harvested plies whose weight was cut to the cap                   */
} ccz_surprise_stats;
int ccz_set_surprise(ccz_engine *e, void *stream, int32_t enabled, double alpha, double cap);
int ccz_get_surprise_stats(ccz_engine *e, void *stream, ccz_surprise_stats *out); /* syncs */
/* the surprise stored with the plies of the boards' current games (syncs): kl_host float [B * max_plies], has_host uint8 [B * max_plies],
 * either may be NULL; entries at or past a board's ply count are stale. */
int ccz_ply_surprise(ccz_engine *e, void *stream, float *kl_host, uint8_t *has_host);

/* ---- root exploration in the search: root noise, forced playouts, policy target pruning (additive to ABI 8) ---------------------------
 * AlphaZero puts the Dirichlet noise into the root's PRIORS; KataGo adds forced playouts and policy target pruning, so that a move the
 * noise favours gets real visits and the visits spent on exploration are taken out of the policy target again. Off after ccz_create:
 * every kernel then computes, records and counts exactly what it does without the feature (the noise is mixed into pi by the sampler
 * after the search, mcts.py:216-224, and pi is the raw visit distribution).
 *   ccz_set_root_exploration: asynchronous on `stream`, takes effect with the next selection / ccz_finish_move. enabled = 0: off (the
 *     other arguments are still validated). eps in [0, 1]; alpha finite and > 0; forced_k finite and >= 0 (KataGo: 2; 0: no forced
 *     playouts); prune_targets 0 / 1. Fails while scout slots are active, and ccz_set_scouts(n > 0) fails while it is enabled.
 * It applies to a board whose current move is a policy-target move (target byte 1: every board unless ccz_set_budgets /
 * ccz_draw_budgets say otherwise); a fast move of playout-cap randomisation searches and samples as without the feature. On such a
 * board, k = number of root children, S = root.N - 1 (= the sum of the children's N while no kept subtree was pruned):
 *   1. noise: g_i = the board's Gamma(alpha) draw i of this move (the draws the sampler uses when the feature is off), G = sum g_i in
 *      index order in float64, dir_i = (float)(G > 0 ? g_i / G : P_i), P'_i = (float)((1 - eps) (double)P_i + eps (double)dir_i).
 *      The selection scores the ROOT's children with (double)(c_puct * P'_i) * sqrt(N_root) / (1 + N_i); nodes keep their raw P (a
 *      kept subtree never carries noise, the evaluation cache is untouched, ccz_root_children reports raw P). dir is computed once
 *      per move and board, at the first selection that finds the root expanded.
 *   2. forced playouts (forced_k > 0): a root child with N_i > 0 and (double)N_i < sqrt(forced_k * (double)P'_i * (double)S) scores
 *      +inf like an unvisited one; the first maximum in child order still wins.
 *   3. ccz_finish_move, policy target pruning (prune_targets): c* = the child of largest N (lowest index on ties) keeps N'_* = N_*.
 *      With E_i = (double)(c_puct * P'_i) * sqrt((double)N_root) and top = Q_* + E_* / (1 + N_*), every other child with N_i > 0 gets
 *      nf_i = ceil(sqrt(forced_k P'_i S)), gap = top - Q_i, need_i = gap > 0 ? max(0, ceil(E_i / gap - 1)) : N_i,
 *      N'_i = min(N_i, max(need_i, N_i - nf_i, 0)), and N'_i = 0 if N'_i < N_i and N'_i <= 1; all in float64. Without pruning N' = N.
 *      pi = the usual softmax chain on N'; that pi is recorded (also under a forced move) and the move is drawn from it on the usual
 *      choice word with NO Dirichlet mixing, whatever eps -- the call's or ccz_config's -- is: enabled alone decides. (So enabled = 1,
 *      eps = 0, forced_k = 0, prune_targets = 0 searches and records exactly like an engine without the call, and moves like one
 *      whose ccz_config.eps is 0.) ccz_move_distribution returns that pi as `mixed` and the unused Gamma draws.
 * The resignation value, ccz_root_children and ccz_principal_variations read the counts as searched. */
typedef struct ccz_exploration_stats { /* sums over boards */
    int64_t explored_moves;    /* plies recorded with root exploration                                                        */
    int64_t forced_selections; /* root selections in which the chosen child had N > 0 and won by the forced-playout rule       */
    int64_t visits_pruned;     /* sum of N_i - N'_i                                                                            */
    int64_t children_pruned;   /* children with N_i > 0 and N'_i = 0                                                           */
} ccz_exploration_stats;
int ccz_set_root_exploration(ccz_engine *e, void *stream, int32_t enabled, double eps, double alpha, double forced_k, int32_t prune_targets);
int ccz_get_exploration_stats(ccz_engine *e, void *stream, ccz_exploration_stats *out); /* syncs */
/* the noise of the move being searched (syncs; tests, diagnostics): noise_host float [B*128] = dir_i as the score used it, zero past
 * k; k_host int32 [B] = the root's child count the row was filled for, 0 on a board that has no row for its current move. */
int ccz_root_noise(ccz_engine *e, void *stream, float *noise_host, int32_t *k_host);

/* ---- Gumbel root search: sequential halving at the root, completed-Q policy targets (additive to ABI 9) ----------------------------
 * "Policy improvement by planning with Gumbel" (Danihelka et al., ICLR 2022) at the ROOT: one Gumbel draw per move, sequential halving
 * over the considered moves, the winner is played and pi' = softmax(logits + sigma(completed Q)) is the policy target -- a target that
 * improves on the prior at any simulation count, which the visit distribution of PUCT does not at the counts of a fast move. Below the
 * root the descent is the reference's PUCT with the first-maximum rule. Off after ccz_create: every output of every call is then bit
 * for bit what it is without the feature (the selection and ccz_finish_move each test one word).
 *   ccz_set_gumbel: asynchronous on `stream`, takes effect with the next selection / ccz_finish_move. enabled = 0: off (the other
 *     arguments are still validated). n_sims >= 1; max_considered in 2..128; c_visit and c_scale finite and >= 0 (the paper: 50, 1).
 *     Fails while scout slots are active or root exploration is enabled; ccz_set_scouts(n > 0) and ccz_set_root_exploration(enabled =
 *     1) fail while it is on. Every board's row (below) is invalidated.
 * It applies to EVERY move of a running board, fast moves of playout-cap randomisation included (the target byte is recorded as
 * before). Float64 unless said otherwise; all sums run in child index order on one lane; i = the root's children in insertion order,
 * k their number.
 *   1. row, filled once per move and board, at the first selection that finds the root expanded:
 *      g_i = -det_log(-det_log(ua)), ua = the first uniform of Philox word (seed, board_id_base + b, move counter, child i, draw
 *      0xfffff) -- the Gamma loop of child i stops below draw 0xffff2, so the Dirichlet draws, budgets, the resign lot and the choice
 *      uniform are what they are --; logit_i = det_log((double)P_i) of the raw stored prior (P_i = 0: what det_log returns for 0, a
 *      finite -709.09); N0_i = N_i at that moment (the kept subtree's visits; "move-visits" M_i = N_i - N0_i); n_b = the board's
 *      budget if it has one (ccz_set_budgets / ccz_draw_budgets; INT32_MAX counts as none), else n_sims; n_eff = max(1, n_b - the
 *      simulations of this move already backed up): n_b - 1 on a fresh root, n_b on a kept tree; m = min(max_considered, k).
 *      A selection that finds the root unexpanded (a fresh tree: reset, set position, a refused move) drops the board's row.
 *   2. seq(m, n), n entries: m <= 1: 0, 1, .., n - 1. Else L = ceil(log2 m), v = 0, c = m, and until n entries exist:
 *      x = max(1, floor(n / (L c))); x times: c copies of v, v += 1; then c = max(2, floor(c / 2)). Cut to n entries.
 *      ((4, 8): 0 0 0 0 1 1 2 2; (3, 7): 0 0 0 1 1 2 2.)
 *   3. completed Q: S = sum N_i; qt_i = ((double)Q_i + 1) / 2 for N_i > 0 (Q_i as stored: the view of the root's side to move);
 *      v0 = (-(double)Q_root + 1) / 2, the root's own running mean turned to its side to move;
 *      v_mix = (v0 + S * (sum_{N_i>0} (double)P_i qt_i) / (sum_{N_i>0} (double)P_i)) / (1 + S), v_mix = v0 when no child is visited;
 *      cq_i = qt_i if N_i > 0 else v_mix; sigma_i = (c_visit + max_j N_j) * c_scale * cq_i.
 *   4. root selection (depth 0, in place of PUCT): t = sum M_i; if t < n_eff the candidates are the children with M_i =
 *      seq(m, n_eff)[t]; if t >= n_eff or no child qualifies, the children with M_i = max_j M_j. The first maximum in child order
 *      of score_i = g_i + logit_i + sigma_i among the candidates wins; NaN on every candidate: CCZ_ERR_NAN. The solver's
 *      proven-stop rule applies to the chosen child as under PUCT.
 *   5. ccz_finish_move: pi'_i = det_exp(s_i - max s) / sum, s_i = logit_i + sigma_i over all k children, recorded as float32 (also
 *      under a forced move) and returned by ccz_move_distribution as `mixed` (gamma zero, u NaN). The temperature is not applied
 *      (a bad one still refuses the board). The move, unless forced, is the first maximum of score_i among the children with M_i =
 *      max_j M_j: no choice uniform, no Dirichlet mixing. A board whose current move has no row (the call came after the search)
 *      uses the row it would get now (M = 0 everywhere). Resignation, ccz_root_children, ccz_root_pi and
 *      ccz_principal_variations read the counts as searched. */
typedef struct ccz_gumbel_stats { /* sums over boards */
    int64_t gumbel_moves;   /* plies recorded under the Gumbel root rule                                     */
    int64_t considered_sum; /* sum of m over those plies                                                     */
    int64_t offvisit_moves; /* plies whose played child is not the first maximum of N                        */
} ccz_gumbel_stats;
int ccz_set_gumbel(ccz_engine *e, void *stream, int32_t enabled, int32_t n_sims, int32_t max_considered, double c_visit, double c_scale);
int ccz_get_gumbel_stats(ccz_engine *e, void *stream, ccz_gumbel_stats *out); /* syncs */
/* the rows of the move being searched (syncs; tests, diagnostics): g_host / logit_host double [B*128], n0_host int32 [B*128], zero
 * past k; k_host int32 [B] = the root's child count the row was filled for, 0 on a board that has no row for its current move;
 * n_eff_host int32 [B]. Any output but k_host may be NULL. */
int ccz_gumbel_root(ccz_engine *e, void *stream, double *g_host, double *logit_host, int32_t *n0_host, int32_t *k_host, int32_t *n_eff_host);
/* seq(m, n) of rule 2 written to seq_dev int32 [n], one wave. Stateless, asynchronous. */
int ccz_gumbel_sequence(void *stream, int32_t m, int32_t n, int32_t *seq_dev);

/* ---- Search parameters: first-play urgency and a visit-scaled exploration constant (additive to ABI 9) ----------------------------
 * In the reference's PUCT an unvisited child scores +inf (mcts.py:47-48): every simulation that reaches a node first walks through all
 * of its children in legal-move order. With first-play urgency (FPU) an unvisited child is scored from its parent's value instead --
 * the "reduction" form of Lc0 / KataGo, or an absolute value as in AlphaZero --, and c_puct may grow with the node's visits as in
 * AlphaZero. Off after ccz_create: every output of every call is then bit for bit what it is without the feature (the selection
 * tests one word).
 *   ccz_set_search: asynchronous on `stream`, takes effect with the next selection. enabled = 0: off; the other arguments are ignored
 *     and the defaults are stored (modes 0, values 0, c_base 19652, c_factor 0). enabled = 1: fpu_mode / fpu_root_mode in {0 off
 *     (+inf), 1 reduction, 2 absolute}; the value of a mode-1 pair finite and >= 0, of a mode-2 pair in [-1, 1], of a mode-0 pair
 *     ignored (stored as 0); c_base finite and > 0; c_factor finite and >= 0 (0: c_puct is constant). A refused call names the field
 *     in ccz_last_error and leaves the old settings in place. Fails while scout slots are active, and ccz_set_scouts(n > 0) fails
 *     while it is on: the scout scheme rests on "children are first visited in legal-move order", which R4 ends.
 *   ccz_get_search: syncs; what the kernels read.
 * A node X has children i = 0 .. k-1, each with N_i, Q_i and raw float32 prior P_i; its own N_X; and Q_X, its running mean as stored,
 * from the side that moved into X: -Q_X is X's value for its side to move (the sign convention of v0 in the Gumbel rule above).
 *   R1. Exploration constant. c_eff(X) = c_puct (the float32 of ccz_config) when c_factor == 0. Otherwise
 *       c_eff(X) = (float)((double)c_puct + c_factor * det_log(((double)N_X + c_base + 1.0) / c_base)). It enters the score exactly
 *       where c_puct does, as the float32 product c_eff * P, then float64.
 *   R2. Visited prior mass. M(X) is the float64 sum of (double)P_i over children with N_i > 0, in this order: lane l (0..63) forms
 *       m_l = a + b, where a = P_l if l < k and N_l > 0 else 0.0, and b is the same for child l + 64; then for s = 32, 16, 8, 4, 2, 1:
 *       m_l = m_l + m_{l xor s}. IEEE addition is commutative, so every lane ends with the same bits. M uses the RAW priors, also at
 *       an explored root (ccz_set_root_exploration): the noisy P' stays in the U term only.
 *   R3. Urgency. mode / value are the root pair at depth 0 and the tree pair below it. Mode 1: f(X) = (double)(-Q_X) - value *
 *       sqrt(M(X)). Mode 2: f(X) = value. Mode 0: +inf, the reference's rule. No clamping.
 *   R4. Score of an unvisited child: f(X) + (double)(c_eff * P_i) * sqrt((double)N_X) -- the visited formula with Q_i := f, N_i := 0
 *       (under mode 0: +inf). First maximum in child order wins, as without the feature.
 *   R5. What stays as it is. A visited root child short of its forced playouts still scores +inf; an unvisited root child of an
 *       explored root uses P'_i in R4. At a Gumbel root the candidates and scores are Gumbel's: the root pair is unused, and the tree
 *       pair applies from depth 1. The solver's stop at a proven chosen child, budgets and CCZ_LEAF_SKIP, NaN priors (CCZ_ERR_NAN: no
 *       comparable child) and the depth and pool limits meet the rule where they meet PUCT.
 *   R6. Target pruning (ccz_set_root_exploration, rule 3) uses c_eff(root) where it uses c_puct. With c_factor == 0 it is untouched.
 * Q_X is the running mean of X, not the raw network value of X (Lc0 uses the same); nothing new is stored per node. */
typedef struct ccz_search_cfg {
    int32_t enabled, fpu_mode, fpu_root_mode, reserved;
    double fpu_value, fpu_root_value, c_base, c_factor;
} ccz_search_cfg;
int ccz_set_search(ccz_engine *e, void *stream, int32_t enabled, int32_t fpu_mode, double fpu_value, int32_t fpu_root_mode,
                   double fpu_root_value, double c_base, double c_factor);
int ccz_get_search(ccz_engine *e, void *stream, ccz_search_cfg *out); /* syncs */

/* ---- Early stop per board: single reply, visit gap, KLD gain (additive to ABI 9) ----------------------------------------------------
 * A board whose budget is spent selects nothing for the rest of a lockstep move (ccz_set_budgets). With this feature a board also
 * stops when searching on cannot change its move -- one legal reply, or a leader the runner-up cannot catch with the simulations
 * left (Lc0's "smart pruning") -- or when its visit distribution has stopped moving (the KL-divergence gain per new visit, as in Lc0
 * and KataGo). Off after ccz_create: every output of every call is then bit for bit what it is without the feature (the selection
 * tests one prefetched word).
 *   ccz_set_early_stop: asynchronous on `stream`, takes effect with the next selection. cfg->enabled = 0: off; the other fields are
 *     ignored and zeros are stored. enabled = 1: single_reply in {0, 1}; gap_factor 0 (off) or finite and >= 1; kld_interval 0 (off)
 *     or >= 1; min_gain finite and >= 0; min_sims >= 0; n_sims >= 1; reserved 0. A refused call names the field in ccz_last_error and
 *     leaves the old settings in place. Every accepted call clears each board's stop and snapshot. Fails with scout slots, a width
 *     above 1 or the Gumbel root (whose sequential halving plans the whole budget), and ccz_set_scouts / ccz_set_width /
 *     ccz_set_gumbel fail while it is on. It works with budgets, routing, root exploration, ccz_set_search, the solver, resignation
 *     and the evaluation cache.
 *   ccz_get_early_stop: syncs; what the kernels read.
 * Per board, at a selection (ccz_select_leaves, the selection of ccz_step*): s = the simulations of the current move backed up so
 * far, this launch's backup included (what the budget test compares); n_b = the board's budget when budgets are on, else n_sims;
 * the root has children i = 0 .. k-1 with counts N_i as they stand after this launch's backup.
 *   S1. When. The rules run when the game is not over, s < n_b, the root is expanded (k >= 1), the board is not already stopped in
 *       this move, and s >= min_sims; in the order S2, S3, S4, and the first that fires wins.
 *   S2. Single reply (single_reply = 1): k == 1 fires with reason 1.
 *   S3. Visit gap (gap_factor f != 0): i1 = the first maximum of N_i in child order, N1 = N_{i1}, N2 = max_{i != i1} N_i (0 when
 *       k == 1). Fires with reason 2 if (double)(N1 - N2) * f > (double)(n_b - s). Both maxima run over children 0 .. 127.
 *   S4. KLD gain (kld_interval I > 0). Per board a snapshot p_i (int32 [128], zero past k) and snap_s, which is -1 at every move
 *       boundary. The rule is evaluated only if s > 0, s % I == 0 and s != snap_s (a selection repeated without a backup must not
 *       meet its own snapshot). If snap_s >= 0 and S_c = sum N_i > S_p = sum p_i: for p_i > 0, o = (double)p_i / (double)S_p,
 *       n = (double)N_i / (double)S_c, t_i = o * det_log(o / n), else t_i = 0.0; T = the butterfly sum of R2 above (lane l forms
 *       t_l + t_{l+64}, then m_l = m_l + m_{l xor s} for s = 32 .. 1); G = T / (double)(S_c - S_p); fires with reason 3 if
 *       G < min_gain (a NaN does not fire). Fired or not, the snapshot becomes N_i and snap_s = s (counted in `evaluations`).
 *   S5. Effect. stopped[b] = reason; this selection and every later one of the move treat the board exactly as a spent budget:
 *       CCZ_LEAF_SKIP, no evaluator row, no simulation counted. stops[reason] += 1 and sims_saved += n_b - s. stopped and snap_s
 *       are cleared wherever the move's simulation count is zeroed (ccz_finish_move on every running board, a fresh root:
 *       ccz_reset, ccz_reset_tree, ccz_set_position(s)). Everything else reads the counts as searched: pi, records, resignation,
 *       ccz_root_children, ccz_principal_variations.
 * Consequence: with f = 1, the solver and root exploration off, the first maximum of N at a root stopped by S3 is the first maximum
 * of the same search run to n_b (the leader gains nothing less than the runner-up can gain), and the stopped board is bit for bit
 * the board of an engine whose budget is s. */
typedef struct ccz_early_stop_cfg {
    int32_t enabled, single_reply, kld_interval, min_sims, n_sims, reserved;
    double gap_factor, min_gain;
} ccz_early_stop_cfg;
typedef struct ccz_early_stop_stats { /* sums over boards */
    int64_t stops[4];     /* by reason: [1] single reply, [2] visit gap, [3] KLD gain ([0] unused)          */
    int64_t sims_saved;   /* sum of n_b - s over the stops                                                  */
    int64_t evaluations;  /* snapshots taken by S4                                                          */
} ccz_early_stop_stats;
#define CCZ_STOP_SINGLE_REPLY 1
#define CCZ_STOP_VISIT_GAP 2
#define CCZ_STOP_KLD_GAIN 3
int ccz_set_early_stop(ccz_engine *e, void *stream, const ccz_early_stop_cfg *cfg);
int ccz_get_early_stop(ccz_engine *e, void *stream, ccz_early_stop_cfg *out);         /* syncs */
int ccz_get_early_stop_stats(ccz_engine *e, void *stream, ccz_early_stop_stats *out); /* syncs */
/* per board: the reason it stopped with in its current move (0: it has not; uint8 [B]) and the simulations its move has backed up
 * (int32 [B]). Either output may be NULL. Syncs. */
int ccz_early_stop_status(ccz_engine *e, void *stream, uint8_t *reason_host, int32_t *sims_host);
/* the number of searched boards that would still select a leaf: the game running, the budget not spent, not stopped. One small
 * kernel and a 4-byte copy; syncs. What a front end polls to end a move's loop early. */
int ccz_searching(ccz_engine *e, void *stream, int32_t *count_host);

/* ---- MCTS-solver: exact propagation of decided positions through the tree (additive to ABI 8) ----
 * One proof byte per tree node, in a device array of its own (uint8 [B][2][max_nodes], allocated and zeroed by the first
 * ccz_set_solver(enabled = 1), which may sync; never touched while the solver is off). Bits 0..1: the state in the view of the side
 * to move at the node -- 0 unknown, CCZ_PROOF_WIN, CCZ_PROOF_LOSS, CCZ_PROOF_DRAW --, bits 2..7: plies to the end, saturating at 63
 * (0 for a draw).
 *   combine(children of a node), in this order: a LOSS child -> WIN in 1 + the smallest such distance; else an unknown child ->
 *     unknown; else a DRAW child -> DRAW; else (all WIN) -> LOSS in 1 + the largest distance.
 *   backup: a simulation whose leaf is CCZ_LEAF_DRAW / CCZ_LEAF_LOSS / CCZ_LEAF_WIN sets the leaf's byte (rules-terminal: LOSS or
 *     DRAW, distance 0; a node proven earlier keeps its byte) and walks up the path: parent <- combine(its children), until a byte
 *     does not change. N and Q are backed up as without the solver (CCZ_LEAF_WIN: leaf value +1).
 *   selection: PUCT and the first-maximum rule are unchanged; a chosen child at depth >= 1 whose state is not 0 ends the descent
 *     there: status DRAW / LOSS / WIN by its state, k = 0, no move generation, no evaluator row. The root is never treated as
 *     decided: a proven root keeps descending, and its visits converge on the proving move by themselves.
 *   expansion zeroes the new children's bytes; the re-root of ccz_finish_move copies a kept node's byte with its records (the new
 *     root's byte is the chosen child's); a fresh root (ccz_reset, ccz_reset_tree, keep_tree = 0, ccz_set_position[s]) is unknown.
 * Off (the state of a new engine, and after ccz_set_solver(0)): every output of every call is what it is without the feature.
 * ccz_set_solver(1) after ccz_set_solver(0) starts from an all-unknown array. Works with scout slots and in ccz_scouted_run.
 * ccz_root_proof (syncs): state / distance of every root (uint8 [B]) and of its children (uint8 [B][128], aligned with
 * ccz_root_children's acts; zero past k); all zeros while the solver is off. Any output may be NULL.
 * ccz_get_solver_stats (syncs): sums over boards.
 * ccz_proof_combine: the combine rule on its own, one wave per case: bytes_dev uint8 [n_cases][128], counts_dev int32 [n_cases]
 * (0..128 children; 0 -> unknown), out_dev uint8 [n_cases]. Stateless, asynchronous. */
#define CCZ_PROOF_WIN 1
#define CCZ_PROOF_LOSS 2
#define CCZ_PROOF_DRAW 3
typedef struct ccz_solver_stats {
    int64_t nodes_proven;  /* nodes whose byte left "unknown"                                        */
    int64_t proven_stops;  /* simulations backed up whose descent ended at a node proven earlier     */
    int64_t roots_proven;  /* searched boards whose game is running and whose root is proven now (a state, not a running sum) */
} ccz_solver_stats;
int ccz_set_solver(ccz_engine *e, void *stream, int32_t enabled);
int ccz_root_proof(ccz_engine *e, void *stream, uint8_t *state_host, uint8_t *dist_host, uint8_t *child_state_host, uint8_t *child_dist_host);
int ccz_get_solver_stats(ccz_engine *e, void *stream, ccz_solver_stats *out);
int ccz_proof_combine(void *stream, const uint8_t *bytes_dev, const int32_t *counts_dev, int32_t n_cases, uint8_t *out_dev);

/* ---- Value spread and the LCB move: what decides the move a match player plays (additive to ABI 9) --------------------------------------
 * A node stores {N, Q, P, first_child}; with this option it also has S, the running sum of squared deviations of the values backed up
 * through it (Welford), in a device array of its own (float32 [B][2][max_nodes], indexed like the node records; allocated and zeroed
 * by the first ccz_set_value_stats(enabled = 1), which may sync; never touched while the option is off).
 *   backup: with val the value applied to a path node, q its Q and n = N + 1 as the backup forms them, all float32, no contraction:
 *       d0 = val - q;  qn = q + d0 / (float)n;        (the incremental mean, unchanged)
 *       S  = S + d0 * (val - qn);                     (one multiply, one add)
 *     in every stepping sequence (ccz_step[_compact], ccz_expand_backup[_compact], ccz_scouted_run with either loop).
 *   expansion writes S = 0 for the new children; the re-root of ccz_finish_move copies a kept node's S with its records, pruned or
 *     not (the new root's S is the chosen child's); a fresh root (ccz_reset, ccz_reset_tree, keep_tree = 0, ccz_set_position[s], a
 *     refused move) has S = 0. ccz_set_value_stats(1) after ccz_set_value_stats(0) starts from an all-zero array.
 * S never feeds back into the search: with the option on, N, Q, P, leaves, moves and records are bit for bit what they are with it
 * off. Works with scout slots (a scout slot has no tree) and with the solver.
 * Refused, in either call order: a width above 1 (a virtual loss is no value), a CCZ_FLAG_VALUE_F16 engine (the float16 running mean
 * has no stated S), ccz_snapshot_save / _load while the option is on (the array is no snapshot section yet).
 * ccz_get_value_stats: the host's word; no sync.
 * ccz_root_value_stats (syncs; fails while the option is off): S of every root's children (float32 [B][128], aligned with
 * ccz_root_children's acts, zero past k) and of the root (float32 [B]); zero rows for finished boards and scout slots. Either may be NULL.
 * ccz_lcb_moves (asynchronous; fails while the option is off): the lower-confidence-bound move of every board, one wave per board,
 * all arithmetic float64 with IEEE / and sqrt. For the root's child i with visits N_i, stored value Q_i (already in the view of the
 * root's side to move) and S_i:
 *     N_i >= 2:  var_i = max((double)S_i, 0) / (N_i - 1);   lcb_i = (double)Q_i - z * sqrt(var_i / N_i)
 *     N_i <  2:  lcb_i = -inf
 *   i* = the first index of maximal N (the move an arg-max player plays); i* is always eligible; another child is eligible iff
 *   N_i >= 2 and N_i >= min_visits and (double)N_i >= min_visit_ratio * (double)N_max. The move is the eligible child of maximal lcb,
 *   ties to the lowest index; if every eligible bound is -inf the move is i*. So z = 0 plays the eligible child of highest Q, and
 *   min_visit_ratio = 1 plays i* unless another child ties its visits.
 *   moves_out_dev int32 [B]: the move id; child_out_dev int32 [B] (or NULL): the child index; lcb_out_dev float64 [B][128] (or NULL):
 *   every child's bound, -inf where it has none, 0 past k. A finished board, a root without a visited child and a scout slot: -1 / -1
 *   (a finished board's and a scout slot's row of bounds is all zero).
 *   Arguments refused: z not finite or < 0, min_visit_ratio outside [0, 1], min_visits < 0. */
int ccz_set_value_stats(ccz_engine *e, void *stream, int32_t enabled);
int ccz_get_value_stats(ccz_engine *e, int32_t *enabled_out);
int ccz_root_value_stats(ccz_engine *e, void *stream, float *s_host, float *root_s_host);
int ccz_lcb_moves(ccz_engine *e, void *stream, double z, double min_visit_ratio, int32_t min_visits, int32_t *moves_out_dev,
                  int32_t *child_out_dev, double *lcb_out_dev);

/* ---- Mate search: forced mates by consecutive checks (additive to ABI 9) ---------------------------------------------------------------
 * A stateless query like ccz_lcb_moves: asynchronous, one wave per board, no evaluator row, no engine state changed (no tree node, no
 * board field, no counter, no error bit); it writes its four output arrays and nothing else, and keeps nothing for a snapshot.
 *
 * The definition. S, the side to move at a board's root position, is the attacker. Iterative deepening n = 1, 3, ..., max_plies:
 *   attacker node with r plies left (r odd): the legal moves in `legal_moves` order (the configured move rank: the order of the tree's
 *     children). A move after which the enemy king is not attacked is skipped; every other move leads to a defender node with r - 1
 *     plies left. The first child that succeeds makes the node succeed; with none it fails.
 *   defender node (the position after the attacker's move): with no legal move it is a mate and succeeds -- also at halfmove clock 120:
 *     the sixty-move rule requires a legal move. Otherwise it FAILS if it is blocked, and fails if r - 1 == 0. Else every reply, in
 *     order, leads to an attacker node with r - 2 left, and the first reply whose node fails makes the defender node fail.
 *   an attacker node below the root is tested for blocked before it generates: a blocked one fails, and is not counted as a node.
 *   blocked: the position (64-bit key, side to move included) equals an earlier position of the DFS path or one of the board's history
 *     chain; or the halfmove clock, kept as ccz_finish_move keeps it (CCZ_RULE_PAWN_MOVE_RESETS_CLOCK included), has reached 120; or
 *     the material is insufficient. This is stricter than the game's rules on purpose (ANY repeat blocks, not the fourth): a mate found
 *     is a forced win under the engine's own game-end rules, the perpetual-check rule included. The search may miss mates (it never
 *     looks at a quiet first move, nor past a repeat) and never invents one.
 *   A node is one position whose legal moves are generated. Nodes are counted over the whole call, every iteration's root included;
 *     the search stops the moment the count reaches node_budget.
 * Per board (all int32 [n_boards], device memory):
 *   state  0 not searched (the game is over, the board is parked, the slot lies past the active boards, or the history chain is full:
 *            128 keys since the last zeroing move, where any deeper leaf raises CCZ_ERR_CHAIN -- here no error bit is set),
 *          1 mate found, 2 no checking mate within max_plies, 3 the budget was reached;
 *   dist   the plies of the first iteration that succeeded (odd), else 0;
 *   move   the id of that iteration's succeeding root move -- the first such move in `legal_moves` order --, else -1;
 *   nodes  the nodes counted; == node_budget exactly in state 3; 0 in state 0.
 * Refused (an error with a message; no sticky bit): max_plies even or outside 1 .. CCZ_MATE_MAX_PLIES, node_budget outside
 * 1 .. CCZ_MATE_MAX_NODES, a null output. The budget bounds the kernel's one loop, so a launch always ends. */
#define CCZ_MATE_MAX_PLIES 31
#define CCZ_MATE_MAX_NODES 131072
#define CCZ_MATE_NONE 0
#define CCZ_MATE_FOUND 1
#define CCZ_MATE_NO_MATE 2
#define CCZ_MATE_BUDGET 3
int ccz_mate_search(ccz_engine *e, void *stream, int32_t max_plies, int32_t node_budget, int32_t *state_dev, int32_t *dist_dev,
                    int32_t *move_dev, int32_t *nodes_dev);

/* ---- Wide search: several pending leaves per board and step, with virtual loss (additive to ABI 9) -------------------------------------
 * Every board runs a strictly sequential MCTS by default: one leaf per board and lockstep step. That fills the chip at thousands of
 * boards and leaves it idle where boards are few (one game, a handful of analysed positions): the evaluator call costs the same for
 * one row as for 64. With a width W > 1 a board gathers up to W leaves of its ONE tree per step, as Lc0 / KataGo / AlphaGo do, kept
 * apart by virtual loss. Off (width 1: the state of a new engine): every output of every call is bit for bit what it is without the
 * feature; nothing of it is allocated or read.
 *
 * The rule ("wide PUCT"). An engine of n_boards = A * W slots has A searched boards, 0 .. A-1: trees and games exist only there (as
 * with scout slots). Slot s(r, j) = r + j * A, j = 0 .. W-1, holds the j-th pending leaf of board r in the per-board hand-over arrays
 * (path, depth, leaf ids, k, status, key, prior row, leaf value, evaluator input row): ccz_leaf_info, ccz_leaf_priors, ccz_leaf_keys,
 * ccz_eval_plan, ccz_gather_priors[_planned] and the evaluator see n_boards independent leaves, and share a row between slots with
 * one position. Every tree node has an in-flight count F: uint8, in an array of its own indexed like the node records, allocated and
 * zeroed by the first ccz_set_width(width > 1) (which may sync) and never touched while the width is 1.
 * A step on board r is two phases, both sequential in j:
 *   A. Backup. For j = 0 .. W-1, slot s = s(r, j) whose status is not CCZ_LEAF_NONE: F -= 1 on every node of the slot's path (depths
 *      0 .. d); an EXPAND leaf gets its k children from the slot's prior row and ids as in ccz_expand_backup_compact (node-pool
 *      accounting and CCZ_ERR_NODE_POOL included); the value value_dev[s] -- or the engine-owned leaf value of slot s when value_dev
 *      == NULL; DRAW: 0, LOSS: -1 -- is backed up along the path with the float32 incremental mean and alternating sign of
 *      ccz_expand_backup; the board's simulation count + 1 (ccz_stats counts as always); the slot's status becomes NONE.
 *   B. Select. t = 0. For j = 0 .. W-1: if the board is over, or its simulation count + t >= its budget (ccz_set_budgets), or the
 *      batch has ended (below), slot s(r, j) gets CCZ_LEAF_NONE, k = 0, depth 0. Otherwise descend from the root. At node X with
 *      children i: Ne = N_i + F_i; score_i = +inf if Ne == 0, else
 *          Qe + (double)(c_puct * P_i) * sqrt((double)(N_X + F_X)) / (double)(1 + Ne),
 *      Qe = (double)Q_i if F_i == 0, else ((double)N_i * (double)Q_i - (double)F_i) / (double)Ne: each in-flight visit counts as one
 *      loss for the side that moved into the child. Every operation is rounded on its own (the library is built -ffp-contract=off);
 *      the first maximum in child order wins. With all F = 0 this is the sequential search's expression, operation for operation.
 *      CCZ_ERR_NAN and CCZ_ERR_DEPTH arise where they do there: the slot gets NONE and the batch ends. The descent ends at the first
 *      node L without children. F[L] > 0 is a COLLISION: L is the pending leaf of an earlier slot of this step and the tree is
 *      unchanged, so every later descent would arrive there too: the slot gets NONE and the batch ends. Otherwise F += 1 on every
 *      node of the path (visible to the next descent), the path goes to the slot, t += 1, and the slot receives what
 *      ccz_select_leaves writes for a board: legal moves, game end, key, evaluator input row. A terminal node with F = 0 may be
 *      selected again in a later step, as in the sequential search. n_leaves_dev[r] = t.
 * Move boundary: ccz_finish_move, ccz_reset, ccz_reset_tree and ccz_set_position(s) drop pending leaves as always; at a width > 1
 * one extra launch in front of them takes the dropped slots' paths out of F and sets the slots to NONE. Between moves F is zero.
 * Budgets (ccz_set_budgets / ccz_draw_budgets) work and are what makes a move exactly n simulations; the evaluation cache (planned
 * boundary) and the unplanned compact boundary work unchanged; resignation, ccz_principal_variations, ccz_root_children and ccz_root_pi
 * read the counts as searched. Refused both ways, naming the other call in ccz_last_error and leaving every setting as it was: scout
 * slots, root exploration, the Gumbel root, the solver, ccz_set_search and routing. While the width is above 1 the sequential step
 * calls fail instead of silently using slot 0 of each board: ccz_select_leaves, ccz_step, ccz_step_compact, ccz_expand_backup,
 * ccz_expand_backup_compact, ccz_scout*. ccz_select_wide / ccz_step_wide in turn need a width above 1: at width 1 the sequential
 * calls ARE the search, and F does not exist.
 *   ccz_set_width: width 1 .. 64, a divisor of n_boards; call it with no leaf pending (at a move boundary). Width 1: off. A width
 *     above 1 sets every slot to CCZ_LEAF_NONE (the slots >= A, and whatever the sequential calls left pending on a searched board:
 *     such a leaf was never counted in F); going back to width 1 drops the pending leaves like a move boundary.
 *   ccz_select_wide: phase B alone, for a move's first step.
 *   ccz_step_wide: phases A then B in one launch, reading the engine's prior rows as ccz_step_compact does (value_dev == NULL: the
 *     engine-owned leaf values of the planned boundary). When every budget is used up it selects nothing: it is also the move's
 *     last backup. n_leaves_dev: int32 [A], device or pinned host memory.
 *   ccz_get_wide_stats (syncs): sums over boards; all zero while the width has never been above 1. */
typedef struct ccz_wide_stats {
    int64_t steps;        /* board-steps that selected at least one leaf                                                   */
    int64_t leaves;       /* leaves selected                                                                                */
    int64_t collisions;   /* batches ended by a collision                                                                   */
    int64_t inflight_now; /* sum of F over the live pool half: 0 between moves and after a finished search                  */
} ccz_wide_stats;
int ccz_set_width(ccz_engine *e, void *stream, int32_t width);
int ccz_select_wide(ccz_engine *e, void *stream, void *leaf_input_f16_dev, int32_t *n_leaves_dev);
int ccz_step_wide(ccz_engine *e, void *stream, const float *value_dev, void *leaf_input_f16_dev, int32_t *n_leaves_dev);
int ccz_get_wide_stats(ccz_engine *e, void *stream, ccz_wide_stats *out);

/* ---- once per move ------------------------------------------------------------------------ */
/* Replaces MCTS.get_move_probs' tail (mcts.py:162-166), MCTS_AI.get_action's choice
 * (mcts.py:216-224), MCTS.update_with_move (mcts.py:168-178) and the per-move part of
 * Game.start_self_play (game.py:159,188-237): pi from root visits at the board's temperature,
 * record (position, turn, pi), choose the move, re-root the tree on the chosen child (subtree
 * kept), make the move on the root position, detect the end of the game and its winner.
 *   forced_moves_dev: int32 [B] or NULL. entry >= 0: play that move id (host-exact numpy sampling
 *     or match play). It must be a LEGAL move of the root position: on a searched root one of its children (they are all of
 *     its legal moves), on a root never searched -- which then gives a fresh root, as update_with_move does (mcts.py:176-178) --
 *     a move the engine's generator lists, as ccz_set_positions checks per ply. Anything else (an id >= 2086, an empty
 *     from-square, the opponent's piece, a move through a blocker, a move that leaves the own king in check) sets
 *     CCZ_ERR_BAD_MOVE, as does a board with nothing forced and nothing searched. entry < 0 or NULL: sample on the device
 *     stream Philox(seed, board id).
 *   temps_dev: float64 [B] or NULL (NULL: schedule of game.py:159 from cfg.temp). An entry that is NaN or <= 0 sets
 *     CCZ_ERR_BAD_TEMP.
 *   A board REFUSED with CCZ_ERR_BAD_MOVE or CCZ_ERR_BAD_TEMP neither records nor moves: moves_out is -1; position, side to move,
 *     clock, history chain, ply, move counter (its Philox stream) and game record are kept. It loses its tree and its pending leaf:
 *     the tree is a fresh root of one node, and the board's node-pool accounting restarts there. The checks run in this order:
 *     finished board (skipped), bad id / nothing to move, bad temperature, the ply cap and the pi arena (the game is adjudicated
 *     a draw, records kept: CCZ_ERR_RECORD for the arena, CCZ_ERR_TRUNCATED for the ply cap in strict mode), forced-move legality.
 *   moves_out_dev: int32 [B] or NULL, receives the move played.
 *   keep_tree: 1 = self-play tree reuse (mcts.py:222-224); 0 = discard (mcts.py:228-229).
 * All live trees move to the other half of their node pool in this call (one flip for every board),
 * which is what lets the simulation kernel request a root's children before any load has returned. */
int ccz_finish_move(ccz_engine *e, void *stream, const int32_t *forced_moves_dev,
                    const double *temps_dev, int32_t *moves_out_dev, int32_t keep_tree);

/* root children of every board (syncs): k_host int32[B]; acts_host uint16[B*128];
 * visits_host int32[B*128]; q_host/prior_host float[B*128] (may be NULL); root_visits_host int32[B]
 * (may be NULL). What mcts.py:162-163 reads. */
int ccz_root_children(ccz_engine *e, void *stream, int32_t *k_host, uint16_t *acts_host,
                      int32_t *visits_host, float *q_host, float *prior_host, int32_t *root_visits_host);
/* The best lines of every live tree: asynchronous on the stream, device outputs only (one wave per board and line). Line r
 * (0 <= r < multipv, multipv 1..128) of board b starts at the root child of rank r -- by visits, descending, ties to the lower
 * child index: rank 0 is the first maximum, the move an arg-max player chooses (mcts.py:225-229); children with N = 0 start no
 * line -- and follows the first child of maximal N with N > 0 until an unexpanded node, a node without a visited child or max_len
 * (>= 1) moves. Outputs: moves_dev uint16 [B][multipv][max_len] move ids, len_dev int32 [B][multipv] (0: unused line),
 * visits_dev int32 [B][multipv][max_len] N of every node on the line, q_dev / prior_dev float32 [B][multipv] the first move's Q and
 * P as stored (Q from the view of the side that played the move: the root's side to move), root_visits_dev int32 [B]. Entries
 * past a line's length are 0. Boards that are over, and scout slots (ccz_set_scouts), get zero lines and root visits 0.
 * A chain of dependent loads, one round per level, like the descent of ccz_step: latency-bound. */
int ccz_principal_variations(ccz_engine *e, void *stream, int32_t multipv, int32_t max_len, uint16_t *moves_dev, int32_t *len_dev,
                             int32_t *visits_dev, float *q_dev, float *prior_dev, int32_t *root_visits_dev);
/* pi of the root at temperature temps_host[b] (float64 [B], or NULL for the schedule; entries must be > 0) without
 * moving: pi_host float64 [B*128] aligned with ccz_root_children's acts (syncs). */
int ccz_root_pi(ccz_engine *e, void *stream, const double *temps_host, double *pi_host);
/* what the next unforced ccz_finish_move samples from, without moving (syncs; tests): with the same temps_host as
 * ccz_root_pi, per board the raw Gamma(alpha) draws gamma_host float64 [B*128], the mixed vector (1-eps) pi + eps g/sum(g)
 * mixed_host float64 [B*128] (both aligned with ccz_root_children's acts, zero past k) and the choice uniform u_host
 * float64 [B]; the move is child searchsorted(cumsum(mixed) / sum(mixed), u, side="right"), at most k-1. A board that
 * would not be sampled (game over, no children) has zero rows and u = NaN. temps_host entries must be > 0. */
int ccz_move_distribution(ccz_engine *e, void *stream, const double *temps_host, double *gamma_host, double *mixed_host,
                          double *u_host);
/* per-board game state (syncs): over_host uint8[B] (1 = finished, waiting for harvest),
 * winner_host int8[B] (1 RED, 0 BLACK, -1 draw), plies_host int32[B], turn_host uint8[B];
 * any pointer may be NULL. */
int ccz_game_status(ccz_engine *e, void *stream, uint8_t *over_host, int8_t *winner_host,
                    int32_t *plies_host, uint8_t *turn_host);
/* root positions (syncs): sq_host uint8 [B*96] */
int ccz_root_positions(ccz_engine *e, void *stream, uint8_t *sq_host);
/* leaf bookkeeping of the last ccz_select_leaves / ccz_step (syncs; tests): status uint8[B] (CCZ_LEAF_*), k int32[B],
 * ids uint16[B*128], depth int32[B]; any pointer may be NULL. */
int ccz_leaf_info(ccz_engine *e, void *stream, uint8_t *status_host, int32_t *k_host,
                  uint16_t *ids_host, int32_t *depth_host);

/* What the compact / planned evaluator boundary hands the tree for the pending leaves, AFTER ccz_gather_priors[_planned] and
 * before ccz_step_compact / ccz_expand_backup_compact consume it (syncs; tests): prior_host float [B*128] = the engine-owned
 * prior rows, entry i of board b belongs to the i-th id of ccz_leaf_info (entries past k and rows of terminal leaves are
 * unspecified); value_host float [B] = the engine-owned leaf values of the planned boundary (table hits and fresh evaluations
 * alike; only with an evaluation cache, else pass NULL). Either may be NULL. This is the `(act_probs, leaf_value)` pair of
 * mcts.py:114 as the tree will see it: a sequential oracle fed these numbers must grow the same tree. */
int ccz_leaf_priors(ccz_engine *e, void *stream, float *prior_host, float *value_host);

/* Zobrist keys (pieces + side to move: everything the evaluator input of net.py:160-173 depends on) and CCZ_LEAF_* status of
 * the pending leaves, copied device-to-device on `stream` (no sync): keys_dev uint64 [B], status_dev uint8 [B], either may be
 * NULL. Equal keys = equal evaluator input: what a transposition / duplicate-leaf cache would key on (the reference
 * evaluates every leaf separately, mcts.py:114). With ccz_set_leaf_history on these are the HISTORY KEYS (see there): the leaf's
 * key mixed with a hash of the seven older positions shown, so the sentence above stays true. */
int ccz_leaf_keys(ccz_engine *e, void *stream, uint64_t *keys_dev, uint8_t *status_dev);

/* ---- training tuples ---------------------------------------------------------------------- */
/* number of tuple rows the finished games would produce (syncs). */
int ccz_harvest_rows(ccz_engine *e, void *stream, int64_t *rows_host);
/* Replaces game.py:208-237 (z assignment) + collect.py:64-131 (preprocess, flip_data) for every
 * finished board: writes rows (state fp16 [17,7,10,9], pi float32 [2086], z float32) into the
 * caller's device buffers, game by game (samples, then their mirror images), then starts a new
 * game on those boards. Finished boards are taken in index order while their rows fit capacity_rows;
 * the others stay finished for the next call (loop until ccz_harvest_rows reports 0). Syncs. */
int ccz_harvest(ccz_engine *e, void *stream, void *states_f16_dev, float *pi_dev, float *z_dev,
                int64_t capacity_rows, int64_t *rows_host);

/* ---- compact game records: the wire format of the multi-GPU exchange ------------------------------ */
/* One fixed-size record per PLY of a finished game, plies of a game contiguous and in order:
 *   bytes   0..89   position before the move (piece codes, square = file + 9*rank), 90..91 the sampling weight (uint16, 1/4096)
 *                   on a CCZ_REC_WEIGHT ply, else zero, 92..95 the root value (float32) on a CCZ_REC_VALUE ply, else zero
 *   bytes  96..111  header: uint16 t (ply index), uint16 T (plies of the game), int8 winner (1 RED, 0 BLACK, -1 draw),
 *                   uint8 turn (side to move), uint8 k (entries of pi), uint8 flags (CCZ_REC_*), uint32 board_id (global),
 *                   uint32 game_no
 *   bytes 112..367  uint16 ids[128]   move ids of the root's children (mcts.py:162), zero-padded
 *   bytes 368..879  float  pi[128]    visit distribution of the move (mcts.py:163-166), zero-padded
 * 880 B per ply stand for the TWO dense rows of 29,768 B (sample + mirror image) that ccz_harvest writes, so the
 * all-gather of finished games (replay.RecordGatherer) moves 1/67 of the bytes; ccz_expand_records rebuilds the rows
 * on the receiving side. What N reference collectors would append to data.h5 (collect.py:146-167). */
#define CCZ_REC_BYTES 880
#define CCZ_REC_HDR 96
#define CCZ_REC_IDS 112
#define CCZ_REC_PI 368
/* ccz_harvest with records as output: the finished boards (index order, while their plies fit capacity_plies; loop
 * until ccz_harvest_rows reports 0) are written to records_dev [capacity_plies x 880 B] and restarted. Syncs. */
int ccz_harvest_records(ccz_engine *e, void *stream, void *records_dev, int64_t capacity_plies, int64_t *plies_host);
/* Records -> dense rows, byte for byte what ccz_harvest writes for the same games (game.py:213-237, collect.py:64-131):
 * state fp16 [17,7,10,9], pi float32 [2086], z float32; per game T samples then (unless CCZ_FLAG_NO_MIRROR) their T mirror
 * images. Stateless: needs no engine (the receiving rank may never have played these games). records_dev must hold WHOLE
 * games (a record whose game is cut is skipped and counted in *bad_records_dev, int32 on the device, may be NULL).
 * flags: CCZ_FLAG_REFERENCE_QUIRKS | CCZ_FLAG_NO_MIRROR; plane_of_type_host: as ccz_config.plane_of_type or NULL.
 * Rows are written to row (head_row + i) % ring_rows of the output arrays (a replay ring resident in HBM);
 * ring_rows = 0: a plain array, row i. Asynchronous on `stream`.
 * target_dev uint8 / value_dev float32 (4-byte aligned), either may be NULL: one entry per row, written at the same index as z.
 * target: the policy-target byte (1 = target, 0 = a CCZ_REC_FAST ply); value: the ply's root value (record bytes 92..95), NaN
 * for a ply without CCZ_REC_VALUE. The sample and its mirror image carry their ply's byte and value. The rows of a buffer of
 * whole games that a cut game leaves unwritten -- (head_row + mul * p + q) % ring_rows for its records p, q < mul -- get 0 / NaN.
 * states_f16_dev, pi_dev and z_dev may be NULL all three together if a side output is given: then only the side outputs are
 * written (one launch of the same kernel, no row is formed). */
int ccz_expand_records(void *stream, const void *records_dev, int64_t n_plies, uint32_t flags,
                       const uint8_t *plane_of_type_host, void *states_f16_dev, float *pi_dev, float *z_dev,
                       int64_t ring_rows, int64_t head_row, int32_t *bad_records_dev, uint8_t *target_dev, float *value_dev);

/* ---- the replay ring of compact records ------------------------------------------------------------ */
/* A trainer-side ring that keeps finished games AS RECORDS (ring_dev: cap_plies x 880 B in HBM) and forms a dense row only
 * when a minibatch draws it: 1/67 of the bytes of a ring of rows, so the trainer sees hours of play, not seconds. Together the
 * two calls replace the reference's train.py:114-122 (DataLoader shuffle over everything convert.py wrote) + collect.py:64-131
 * (preprocess, flip_data) without the disk round trip. window_dev: int64 {tail, head} on the device, logical ply counters that
 * only grow (zero them once); physical slot = counter % cap_plies; [tail, head) holds whole games only. Both calls are
 * stateless (no engine) and asynchronous on `stream`.
 *
 * ccz_ring_retire: call after the records of logical plies [head_old, head_new) have been copied to their slots (an append of
 * at most cap_plies records, whole games): head = head_new, tail = max(tail, head_new - cap_plies), then tail moves on to the
 * next game start, so that the window advances by whole games only. Needs cap_plies >= 2 * max_game_plies; a game at the tail
 * longer than max_game_plies (or a header with t >= T) is counted in *bad_records_dev (int32, may be NULL) and skipped. */
int ccz_ring_retire(void *stream, const void *ring_dev, int64_t cap_plies, int64_t *window_dev, int64_t head_new,
                    int32_t max_game_plies, int32_t *bad_records_dev);
/* ccz_sample_records: draws_dev int64 [batch], non-negative. With live = (head - tail) * mul rows (mul = 1 under
 * CCZ_FLAG_NO_MIRROR, else 2) draw u means row r = u % live: ply tail + r / mul, pass r % mul (1 = the mirror image). Output
 * row j of states fp16 [batch,17,7,10,9], pi float32 [batch,2086], z float32 [batch] gets, byte for byte, what
 * ccz_expand_records writes for that ply and pass (flags, plane_of_type_host: as there). A drawn record that is not part of a
 * whole game inside the window, or an empty window, counts in *bad_records_dev and yields a row of zeros.
 * target_dev uint8 [batch] / value_dev float32 [batch] (4-byte aligned), either may be NULL: the drawn row's policy-target byte
 * and root value, as ccz_expand_records gives them for that ply (the mirror row carries its ply's); a bad draw gets 0 / NaN. */
int ccz_sample_records(void *stream, const void *ring_dev, int64_t cap_plies, const int64_t *window_dev,
                       const int64_t *draws_dev, int64_t batch, uint32_t flags, const uint8_t *plane_of_type_host,
                       void *states_f16_dev, float *pi_dev, float *z_dev, int32_t *bad_records_dev, uint8_t *target_dev,
                       float *value_dev);
/* ccz_sample_records_weighted: ccz_sample_records with the draws made on the device, by weight. seed_dev: one uint64 on the device
 * (8-byte aligned); cap_q: the cap on a weight in 1/4096, 4096 .. 61440; chosen_dev int64 [batch] (may be NULL) receives the draw u
 * every row took; *fallback_dev (int32, may be NULL) counts the rows that fell back. Row j is chosen by rejection: candidate (r, l),
 * r = 0..3, l = 0..63, takes the Philox4x32-10 words o of key *seed_dev and counter {hi = j, lo = 64 r + l}; u = (o0:o1) >> 2 (62
 * bits), a = ((o2:o3) >> 11) * 2^-53. Its ply is that of draw u in ccz_sample_records; wq = the uint16 at record byte 90 with
 * CCZ_REC_WEIGHT, else 4096. It is accepted iff the ply is part of a whole game inside the window and a * cap_q < wq; the first
 * accepted candidate in (r, l) order is the row's. None of the 256 accepted: the row takes candidate (0, 0) and counts in
 * *fallback_dev (weights at most cap_q / 4096 of mean m: a chance of (1 - m * 4096 / cap_q)^256 per row). Output row j, target and
 * value are byte for byte what ccz_sample_records writes for draw u, a bad row (candidate (0, 0) of a fallback that is no whole game,
 * or an empty window) included; candidates that lose count nowhere. The pass (mirror image or not) comes from u; both passes share
 * the ply's weight. Asynchronous, no host sync. */
int ccz_sample_records_weighted(void *stream, const void *ring_dev, int64_t cap_plies, const int64_t *window_dev,
                                const uint64_t *seed_dev, int32_t cap_q, int64_t *chosen_dev, int32_t *fallback_dev, int64_t batch,
                                uint32_t flags, const uint8_t *plane_of_type_host, void *states_f16_dev, float *pi_dev, float *z_dev,
                                int32_t *bad_records_dev, uint8_t *target_dev, float *value_dev);

int ccz_get_stats(ccz_engine *e, void *stream, ccz_stats *out); /* syncs */

/* ---- stateless batch rules (parity tests, perft; replaces cchess legal_moves / game-end) ---- */
/* n positions: sq_dev uint8 [n*96], turn_dev uint8 [n], halfmove_dev int32 [n] or NULL.
 * outputs (any may be NULL): mask_dev uint32 [n*66] legal-move bitmask over the 2086 ids,
 * count_dev int32 [n], flags_dev uint8 [n]: bit0 side to move in check, bit1 insufficient material,
 * bit2 sixty-move rule (needs halfmove_dev). */
int ccz_legal_moves(void *stream, int32_t n, const uint8_t *sq_dev, const uint8_t *turn_dev,
                    const int32_t *halfmove_dev, uint32_t *mask_dev, int32_t *count_dev,
                    uint8_t *flags_dev);
/* apply move ids to n positions in place (captures reported in captured_dev uint8[n], may be NULL);
 * replaces cchess.Board.push for batches. */
int ccz_apply_moves(void *stream, int32_t n, uint8_t *sq_dev, uint8_t *turn_dev,
                    const int32_t *move_ids_dev, uint8_t *captured_dev);

/* ---- evaluator epilogue (the net itself stays in PyTorch-ROCm / MIOpen) ------------------------ */
/* One-pass fused epilogue of a tower convolution on NHWC fp16 activations y [rows, channels]:
 * y = relu(y + bias[c])  or, with residual_dev != NULL,  y = relu(y + bias[c] + residual)  (reference
 * net.py:32-43: conv -> BN(folded into conv/bias) -> [+x] -> ReLU). Replaces three separate full-tensor
 * passes (bias, add, clamp) that PyTorch issues around an MIOpen convolution. 16-byte aligned pointers. */
int ccz_bias_act_f16(void *stream, void *y_dev, const void *bias_dev, const void *residual_dev,
                     int64_t rows, int32_t channels);

/* A whole tower convolution in one kernel (MFMA implicit GEMM, hand-written for gfx950): 3x3, padding 1,
 * 256 -> 256 channels over boards of 10 x 9, NHWC fp16 in and out, fp32 accumulate:
 *   y[p, co] = act( bias[co] + sum_{ky,kx,ci} w[co, ky, kx, ci] * x[p + 9*(ky-1) + (kx-1), ci] [+ residual[p, co]] )
 * with taps that leave the board contributing zero; relu is a flag word (CCZ_CONV_*): bit 0 = apply ReLU, bit 1 = process
 * the pixel tiles in descending order (same results; alternating the order from layer to layer reads first what the
 * previous layer wrote last), bit 6 = the activations are in the group-of-16 row layout (below) (reference net.py:20-43,
 * ResBlock conv -> BN(folded) -> [+x] -> ReLU; replaces F.conv2d + ccz_bias_act_f16 for these layers).
 * x, y, residual: [n_pixels, 256] fp16 (n_pixels = boards * 90); w: [256, 3, 3, 256] fp16 (the memory of a
 * channels-last [co, ci, 3, 3] tensor); bias: float32 [256]. y may alias residual, not x. At most 93,206 boards
 * per call (32-bit element offsets).
 * Row layouts. Default: NHWC, row = board * 90 + pos (pos = rank * 9 + file). CCZ_CONV_G16: row = (g * 90 + pos) * 16 + j
 * for board 16 g + j (n_pixels must then be a multiple of 1440 = 16 boards): sixteen consecutive rows are ONE board position
 * of sixteen boards, which lets the kernel skip the taps that leave the board instead of multiplying zeros, on tiles of two
 * whole ranks (csrc/cczero_conv_g16.h: the form the evaluator uses from 640 boards on). With CCZ_CONV_G16 the WEIGHTS
 * are packed too: w_dev is what ccz_pack_conv_weights_g16_f16 wrote (below). All kernels behind these entry points add their
 * products in the same order: a board's result is the same in either layout and at any batch size. */
#define CCZ_CONV_RELU 1
#define CCZ_CONV_DESCENDING 2
#define CCZ_CONV_FORCE_SMALL 16 /* A/B runs and tests: k_conv3x3_small whatever the batch size (default layout only) */
#define CCZ_CONV_FORCE_TILE 32  /* A/B runs and tests: the 256-pixel tile kernel whatever the batch size (default layout only) */
#define CCZ_CONV_G16 64
#define CCZ_CONV_G16_EDGE_TILES 128 /* with CCZ_CONV_G16 (round 4, opt-in): the middle launch (ranks 1..8, four two-rank tiles per group) followed
                                       by the edge-pair launch (ranks 0 and 9 of two groups per tile, six live taps instead of nine:
                                       csrc/cczero_conv_g16e.h) instead of ONE launch of five tiles per group whose edge tiles multiply
                                       zeroed ranks. Same values; -3 % per layer at 4096 boards in isolation; in the workload it pays only
                                       with three launch chains and from ~4096 boards on (+0.7...0.9 % sims/s), where the evaluator
                                       sets it (InferenceNet edge_tiles=auto); smaller launches lose (profiles/r04_conv_g16.json) */
#define CCZ_CONV_G16_ONE_LAUNCH 512 /* with CCZ_CONV_G16_EDGE_TILES (round 7): the middle tiles and the edge-pair tiles of a layer as ONE launch
                                       (csrc/cczero_conv_g16e.h k_conv3x3_g16_one): the two classes do not depend on each other, so a launch
                                       chain pays one dependent-launch tail per layer instead of two and the shorter edge tiles fill the
                                       last round of the middle ones. Same tiles, same values; the heads layer (ccz_conv3x3_c256_heads_f16)
                                       ignores it */
#define CCZ_CONV_G16_QUAD 65536     /* with CCZ_CONV_G16_EDGE_TILES (additive to ABI 8: bit 16, which ABI-8 libraries before it refuse with the retired
                                       persistent form's bits 16..27 -- an older library fails the call, it never ignores the flag): the middle
                                       tiles as FOUR ranks x 128 output channels instead of two ranks x 256 (csrc/cczero_conv_g16.h g5q_tile):
                                       as many tiles of as many rows x channels and the same MFMAs in the same order, but a tile streams half
                                       the layer's weights: -30 % LDS-DMA bytes per tile. Same values. Where the five-tile launch runs (no
                                       CCZ_CONV_G16_EDGE_TILES, or fewer than 32 boards) it has no effect; the heads layer
                                       (ccz_conv3x3_c256_heads_f16) ignores it: its epilogue needs all 256 channels of a row */
int ccz_conv3x3_c256_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev,
                         const void *residual_dev, void *y_dev, int64_t n_pixels, int32_t relu);
/* Weights for the CCZ_CONV_G16 form, once per weight set: w [256, 3, 3, cin] fp16 (cin = 256: tower, 64: stem) ->
 * wp [cin / 32][9][256][32] fp16, the four 16-byte chunks of every 64-byte row in the order of the kernel's LDS image: a
 * half-tile (32 input channels of one tap, all output channels) is then one contiguous 16 KB block. Not in place. */
int ccz_pack_conv_weights_g16_f16(void *stream, const void *w_dev, void *wp_dev, int32_t cin);

/* The stem convolution (reference net.py:59-66,86-88: conv3x3(119 -> 256) -> BN(folded) -> ReLU) with the same kernel,
 * one 64-channel chunk: x64 [n_pixels, 64] fp16 holds the 21 planes that can be non-zero on the search path in
 * channels 0..20 (ccz_pack_live_planes_f16) and zeros above; w: [256, 3, 3, 64] fp16 (input channels in the same
 * order, zero-padded); bias float32 [256]; y [n_pixels, 256] fp16. Exact: zero inputs contribute nothing. With
 * CCZ_CONV_G16 the kernel takes that at its word: channels 32..63 of x64 are NOT READ (one 32-channel chunk instead of two:
 * they hold zeros by this contract, and adding products of zeros changes no bit of an accumulator that starts at a bias). */
int ccz_conv3x3_stem_f16(void *stream, const void *x64_dev, const void *w_dev, const void *bias_f32_dev,
                         void *y_dev, int64_t n_pixels, int32_t relu);
/* Evaluator input [n_boards, 17, 7, 10, 9] fp16 (the layout ccz_select_leaves / ccz_step write, net.py:174-177)
 * -> NHWC rows of 64 channels: planes 49..55 (group 7), 105..118 (groups 15, 16), then zeros (net.py:160-173 leaves
 * every other group zero on the search path). */
int ccz_pack_live_planes_f16(void *stream, const void *leaf_dev, void *x64_dev, int32_t n_boards);
/* The same into the CCZ_CONV_G16 row layout; x64 must hold ceil(n_boards / 16) * 1440 rows (the rows of the boards that pad the
 * last group are left alone). rows_dev / n_rows_dev as for ccz_pack_live_planes_rows_f16 below, or both NULL. */
int ccz_pack_live_planes_g16_f16(void *stream, const void *leaf_dev, void *x64_dev, int32_t n_boards,
                                 const int32_t *rows_dev, const int32_t *n_rows_dev);

/* The same three for the planned evaluator boundary (ccz_eval_plan): the number of rows to compute is a DEVICE value, so that
 * no host sync stands between the plan and the evaluator. ccz_pack_live_planes_rows_f16: output row i = board rows_dev[i] for
 * i < *n_rows_dev (the rest is left alone). The planned forms (rows_dev != NULL, either layout) write channels 0..23 of a row
 * only: x64 must be a buffer whose channels 24..63 are ZERO (zeroed once and reused step after step: what the evaluator does). The *_live convolutions take the pointers of the WHOLE batch: the first *live_rows_dev
 * boards are live and are cut into n_parts equal ranges (multiples of 8 boards; of 16 with CCZ_CONV_G16) of which this launch
 * computes range `part` -- so that concurrent launch chains stay balanced whatever the live count is; n_pixels = the largest
 * range a launch may get (ceil(boards / n_parts) rounded up to 8 (16) boards, x 90): the grid is sized for it, tiles past the
 * live rows exit at once, the last live tile may be partial. */
int ccz_pack_live_planes_rows_f16(void *stream, const void *leaf_dev, void *x64_dev, int32_t n_boards,
                                  const int32_t *rows_dev, const int32_t *n_rows_dev);
int ccz_conv3x3_c256_f16_live(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev,
                              const void *residual_dev, void *y_dev, int64_t n_pixels, int32_t relu,
                              const int32_t *live_rows_dev, int32_t part, int32_t n_parts);
int ccz_conv3x3_stem_f16_live(void *stream, const void *x64_dev, const void *w_dev, const void *bias_f32_dev,
                              void *y_dev, int64_t n_pixels, int32_t relu, const int32_t *live_rows_dev,
                              int32_t part, int32_t n_parts);

/* ---- the evaluator's tail: head convolutions, fully connected layers, tanh (reference net.py:96-109) -------------------------
 * Hand-written like the tower so that (1) only the LIVE rows of a planned batch are computed, (2) the group-of-16 -> board
 * permutation, bias, ReLU and the policy / value split cost no passes of their own, and (3) a board's logits and value are the
 * same bits at every batch size (each output element is one fixed chain of MFMAs over k = 0, 32, 64, ...).
 *
 * ccz_heads_conv1x1_f16: both 1x1 head convolutions (policy_conv 256 -> 17, value_conv 256 -> 7, BatchNorm folded) + ReLU on the
 *   tower's output rows x [n_boards * 90, 256] fp16 (NHWC rows, or the group-of-16 row order with flags = CCZ_CONV_G16: n_boards
 *   a multiple of 16). w32: [32, 256] fp16, rows 0..16 = policy channels, 17..23 = value channels, 24..31 zero; bias32: float
 *   [32]. Outputs in BOARD order: pol [n_boards, 1536] fp16 = (pos, channel)-major 90 x 17 values + 6 pad elements that are
 *   never written (keep them zero), val [n_boards, 640] fp16 = 90 x 7 values + 10 pad. live_boards_dev: device int32 count of
 *   live boards (rows of boards past it are skipped) or NULL.
 * ccz_fc_f16: c[m, n] = act(bias[n] + sum_k a[m, k] * w[n, k]): a [m, lda] fp16, w [ceil(n / 128) * 128, k] fp16 with zero rows
 *   past n, bias float [ceil(n / 128) * 128], c [m, ldc] fp16; k a multiple of 64 (zero-pad the columns of w), n and ldc even;
 *   relu bit 0 applies ReLU (bits 1 / 2 force the 128 x 128-tile kernel / the 256 x 144-tile kernel, which otherwise serves m >= 2048
 *   with n >= 1024; m <= 16 -- one game at a time -- runs on a one-wave-per-16-columns kernel: the same bits from all three -- tests and A/B runs). policy_fc: a = pol, k = 1536, n = 2086; value_fc1: a = val,
 *   k = 640, n = 256, relu. The FC weights'
 *   input columns are in (pos, channel) order (the reference flattens (channel, pos): net.py:98,103).
 * ccz_value_out_f32: v[m] = tanh(fp16(b2 + sum_k h[m, k] * w2[k])), h [m, 256] fp16, w2 fp16 [256] (value_fc2 + tanh, net.py:107-109).
 * live_rows_dev as above (rows past *live_rows_dev are not computed) or NULL. Asynchronous on `stream`. */
#define CCZ_HEAD_POL_STRIDE 1536
#define CCZ_HEAD_VAL_STRIDE 640
int ccz_heads_conv1x1_f16(void *stream, const void *x_dev, const void *w32_dev, const void *bias32_f32_dev, void *pol_dev,
                          void *val_dev, int32_t n_boards, int32_t flags, const int32_t *live_boards_dev);
int ccz_fc_f16(void *stream, const void *a_dev, int32_t lda, const void *w_dev, const void *bias_f32_dev, void *c_dev, int32_t ldc,
               int32_t m, int32_t n, int32_t k, int32_t relu, const int32_t *live_rows_dev);
int ccz_value_out_f32(void *stream, const void *h_dev, const void *w2_dev, float b2, float *v_dev, int32_t m,
                      const int32_t *live_rows_dev);

/* ---- narrow towers: 64 and 128 channels (additive to ABI 9; csrc/cczero_conv_narrow.h) -------------------------------------------
 * The same chain as ccz_conv3x3_c256_f16 -- fp32 accumulator started at the bias, K in ascending chunks of 32 input channels x 9
 * taps, fp16(acc) [+ residual in fp16] [ReLU] -- for board-major rows x [n_pixels, cin] -> y [n_pixels, cout], cin and cout each 64
 * or 128 (towers 64 -> 64 and 128 -> 128; stems 64 -> 64 / 128 behind ccz_pack_live_planes_*_f16 and 128 -> 64 / 128 behind
 * ccz_pack_planes128_*). w: [cout, 3, 3, cin] fp16, unpacked; bias: float [cout]; residual: [n_pixels, cout] or NULL (y may alias it,
 * not x). relu: CCZ_CONV_RELU, CCZ_CONV_DESCENDING, CCZ_CONV_FORCE_SMALL / _TILE as on ccz_conv3x3_c256_f16; no group-of-16 form. Up
 * to 64 boards run on k_conv3x3_small, larger batches on k_conv3x3_narrow (256-pixel tiles): the same bits from both, so a board's
 * activations do not depend on its batch. A count that is not whole boards runs the tile form; the rows of its last board past
 * n_pixels read as zero. Any other (cin, cout), misaligned pointers, a bad part / n_parts or a NULL live count fail the call.
 * ccz_conv3x3_cn_f16_live: live_rows_dev / part / n_parts / n_pixels (the capacity of a range) as ccz_conv3x3_c256_f16_live on
 *   board-major rows: ranges of ceil(ceil(L / n_parts) / 8) * 8 boards, rows past the live boards are not written.
 * ccz_heads_conv1x1_cn_f16: ccz_heads_conv1x1_f16 on board-major rows of c_in = 64 or 128 channels (w32: [32, c_in]). */
int ccz_conv3x3_cn_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev,
                       void *y_dev, int64_t n_pixels, int32_t relu, int32_t cin, int32_t cout);
int ccz_conv3x3_cn_f16_live(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev,
                            void *y_dev, int64_t n_pixels, int32_t relu, int32_t cin, int32_t cout, const int32_t *live_rows_dev,
                            int32_t part, int32_t n_parts);
int ccz_heads_conv1x1_cn_f16(void *stream, const void *x_dev, const void *w32_dev, const void *bias32_f32_dev, void *pol_dev,
                             void *val_dev, int32_t n_boards, int32_t c_in, const int32_t *live_boards_dev);

/* The LAST residual layer of the tower with both head convolutions in its epilogue (group-of-16 rows only: flags must hold
 * CCZ_CONV_G16; bit 0 ReLU, CCZ_CONV_G16_EDGE_TILES as ccz_conv3x3_c256_f16): computes relu(conv3x3(x) + bias + residual) like
 * ccz_conv3x3_c256_f16 but does NOT store it -- each tile multiplies its finished rows with w32 while they are still in LDS and
 * writes pol / val exactly as ccz_heads_conv1x1_f16 would from the stored tensor (same operands, same MFMA chain: the same bits).
 * Saves one write and one read of the activation tensor (2 x 189 MB at 4096 boards). live_rows_dev == NULL: n_pixels rows at
 * x_dev / residual_dev, boards 0 .. n_pixels / 90 - 1 at pol_dev / val_dev (part / n_parts ignored). live_rows_dev != NULL: the
 * pointers of the WHOLE batch and part / n_parts as ccz_conv3x3_c256_f16_live; boards past *live_rows_dev are not written. */
int ccz_conv3x3_c256_heads_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev,
                               const void *residual_dev, const void *head_w32_dev, const void *head_bias32_f32_dev,
                               void *pol_dev, void *val_dev, int64_t n_pixels, int32_t flags,
                               const int32_t *live_rows_dev, int32_t part, int32_t n_parts);

/* ---- the chunk-major activation layout "G16C" (additive; csrc/cczero_conv_g16.h g16c_off) -------------------------------------
 * The same 16-board groups as CCZ_CONV_G16 and the same group stride (1440 rows x 512 B), but inside a group the bytes are
 * [chunk 0..7][row 0..1439][32 channels]: channel c of G16 row p of group g is at byte g * 737280 + (c / 32) * 92160 + p * 64 +
 * (c % 32) * 2. A tile's activation slab of one 32-channel chunk is then ONE contiguous run of whole cache lines (in CCZ_CONV_G16
 * rows it is 64-byte pieces 512 B apart, and every line crosses the L2 -> L1 path twice). Same tiles, same MFMAs in the same
 * order: the same values as the CCZ_CONV_G16 calls, permuted. The calls below take the arguments of their CCZ_CONV_G16 twins;
 * `relu` / `flags` must hold CCZ_CONV_G16. ccz_conv3x3_c256_g16c_f16(_live): x, residual, y in G16C; only the quad one-launch form
 * exists (CCZ_CONV_G16_EDGE_TILES | CCZ_CONV_G16_ONE_LAUNCH | CCZ_CONV_G16_QUAD must be set: anything else is refused; a single
 * group runs that form too). ccz_conv3x3_stem_g16c_f16(_live): x64 as for ccz_conv3x3_stem_f16 with CCZ_CONV_G16 (rows), y in G16C.
 * ccz_conv3x3_c256_heads_g16c_f16: x and residual in G16C (CCZ_CONV_G16_EDGE_TILES must be set: middle + edge-pair launches); pol / val in
 * board order as ever. */
int ccz_conv3x3_c256_g16c_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev,
                              const void *residual_dev, void *y_dev, int64_t n_pixels, int32_t relu);
int ccz_conv3x3_c256_g16c_f16_live(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev,
                                   const void *residual_dev, void *y_dev, int64_t n_pixels, int32_t relu,
                                   const int32_t *live_rows_dev, int32_t part, int32_t n_parts);
int ccz_conv3x3_stem_g16c_f16(void *stream, const void *x64_dev, const void *w_dev, const void *bias_f32_dev,
                              void *y_dev, int64_t n_pixels, int32_t relu);
int ccz_conv3x3_stem_g16c_f16_live(void *stream, const void *x64_dev, const void *w_dev, const void *bias_f32_dev,
                                   void *y_dev, int64_t n_pixels, int32_t relu, const int32_t *live_rows_dev,
                                   int32_t part, int32_t n_parts);
int ccz_conv3x3_c256_heads_g16c_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev,
                                    const void *residual_dev, const void *head_w32_dev, const void *head_bias32_f32_dev,
                                    void *pol_dev, void *val_dev, int64_t n_pixels, int32_t flags,
                                    const int32_t *live_rows_dev, int32_t part, int32_t n_parts);

/* ---- Engine snapshots: save a self-play run and resume it bit for bit (additive to ABI 9) -------------------------------------
 * A snapshot is one contiguous device blob that holds what decides what the engine does next and nothing else: of the node pool
 * ([B][2][cap] records) the first n_nodes nodes of every board's pool half -- the re-root's breadth-first copy leaves every kept tree
 * contiguous from node 0 --, of the record arrays the first `ply` plies and `pi_used` pi entries, and every per-board row (position,
 * history chain, check bits, budgets, resignation / exploration / Gumbel / early-stop state, all counters). The evaluation cache is
 * NOT saved: a loaded engine starts with a cold cache. The trees are the same with and without the cache; the cache counters of
 * ccz_stats (cache_probes, cache_hits, cache_shared_rows, cache_stores, cache_verified) go on from the saved sums and therefore
 * differ from those of an uninterrupted run.
 *   THE MOVE-BOUNDARY CONTRACT. ccz_snapshot_save and ccz_snapshot_load are called at a move boundary: after ccz_finish_move (before
 *     or after the harvest) or before the first selection, with NO LEAF PENDING on any board or slot. The selection path, the pending
 *     leaf, the cache plan, the compact prior rows and the wide search's in-flight counts are not saved; whether a leaf is pending is the
 *     caller's knowledge (BatchedSelfPlay.state_dict checks it), the engine cannot tell. A snapshot taken inside a move resumes from
 *     the tree as it stood, minus the pending simulation.
 *   The blob (csrc/cczero_snapshot.h, chinesechesszero_amd/snapshot.py): a 512-byte header -- magic, format version, the
 *     configuration that decides the layout and the arithmetic (B, cap, max_depth, max_plies, pi_cap, reserve, c_puct, eps, alpha, temp,
 *     flags, seed, board_id_base, rule_flags, the plane / type-rank packs, a hash of the move-rank table), the settings structs as the
 *     device holds them (resign, root exploration, Gumbel, search, early stop, solver on, width), the sticky error word --, the B + 1
 *     64-bit section offsets, the B meta records, and per board one section that starts on a 16-byte boundary.
 *   ccz_snapshot_size (syncs): the bytes a save would write now.
 *   ccz_snapshot_save (syncs): blob_dev is a device buffer of `capacity` bytes, 16-byte aligned; *bytes_host (may be NULL) = the bytes
 *     written, exactly ccz_snapshot_size's. A capacity below that: -1, *bytes_host says what is needed, nothing is written. Refused
 *     with scout slots (ccz_set_scouts). Changes nothing in the engine.
 *   ccz_snapshot_load (syncs): STRICT. The engine must have been created with the same configuration and hold the same settings;
 *     magic, version, total size, the offset table (monotone, inside `bytes`, every section as long as its board's counts say) and
 *     every board's counts (n_nodes <= cap, ply <= max_plies, pi_used <= pi_cap) are checked BEFORE anything is written: -1,
 *     ccz_last_error() names the field, the engine is exactly as it was. keep_board_id_base != 0: the one field a load may override
 *     -- the engine keeps its own board_id_base (the boards' Philox streams are those of ids board_id_base + b from here on);
 *     0: a different base is refused like any other field. Every tree lands in the pool half the engine's half word names; no
 *     pointer changes, so a hipGraph captured before the load stays valid. The load also restores what a move boundary guarantees:
 *     no pending leaf, zero in-flight counts, the evaluation cache cleared (ccz_eval_cache_clear). Growing cap, another B and loading a
 *     subset of the boards are not supported.
 *   ccz_snapshot_layout: the layout scan on its own: offsets_dev uint64 [B + 1] = the exclusive scan, in 64 bits, of the section sizes
 *     of B boards with the counts n_nodes_dev / ply_dev (int32 [B], negative counts as 0) / pi_used_dev (uint32 [B]);
 *     offsets_dev[B] = the sum. `sections`: CCZ_SNAP_PROOF (one proof byte per node) | CCZ_SNAP_VALUES (root value + flag per ply);
 *     an engine's own blobs have CCZ_SNAP_VALUES always and CCZ_SNAP_PROOF once ccz_set_solver(1) has allocated the bytes. With
 *     pad16(n) = n rounded up to 16, a section is CCZ_SNAP_FIXED_BYTES + 16 n_nodes + pad16(4 n_nodes) [+ pad16(n_nodes)] + 96 ply +
 *     pad16(4 ply) + 3 pad16(ply) [+ pad16(4 ply) + pad16(ply)] + pad16(2 pi_used) + pad16(4 pi_used) bytes. Any B >= 1; stateless,
 *     asynchronous. CCZ_SNAP_SURPRISE (the surprise and has-bit per ply and the board's counter row; in an engine's own blobs only
 *     while ccz_set_surprise is on, whose settings the header then holds in bytes 336..359, zero otherwise) adds pad16(4 ply) +
 *     pad16(ply) + 32 bytes behind the value arrays. */
#define CCZ_SNAP_PROOF 1u
#define CCZ_SNAP_VALUES 2u
#define CCZ_SNAP_SURPRISE 4u
#define CCZ_SNAP_HEADER_BYTES 512
#define CCZ_SNAP_FIXED_BYTES 5088
int ccz_snapshot_size(ccz_engine *e, void *stream, uint64_t *bytes_host);
int ccz_snapshot_save(ccz_engine *e, void *stream, void *blob_dev, uint64_t capacity, uint64_t *bytes_host);
int ccz_snapshot_load(ccz_engine *e, void *stream, const void *blob_dev, uint64_t bytes, int32_t keep_board_id_base);
int ccz_snapshot_layout(void *stream, int32_t B, const int32_t *n_nodes_dev, const int32_t *ply_dev, const uint32_t *pi_used_dev,
                        uint32_t sections, uint64_t *offsets_dev /* [B + 1] */);

#ifdef __cplusplus
}
#endif
#endif
