// cczero_kernels.h -- the gfx950 kernels of the lockstep self-play engine (one wave per board).
#pragma once
#include <type_traits>

#include "cczero_device.h"

namespace ccz {

constexpr uint16_t kHalfOne = 0x3C00; // fp16 1.0
constexpr int kMaxDepth = 512;     // selection path capacity (Dev.maxd <= kMaxDepth)

__device__ __forceinline__ void set_err(const Dev &D, int bit) { atomicOr(D.err, bit); }

// ------------------------------------------------------------------ new game / set position
// Start position: rank 0 = RNBAKABNR (red), rank 2 cannons b,h, rank 3 pawns a,c,e,g,i; black mirrored.
__device__ __forceinline__ int start_piece(int s)
{
    const int r = s / 9, f = s - 9 * r;
    const int rr = r <= 4 ? r : 9 - r; // distance from the own back rank
    const int add = r <= 4 ? 0 : 8;
    int t = 0;
    if (rr == 0) {
        const int ff = f <= 4 ? f : 8 - f;
        t = ff == 0 ? ROOK : ff == 1 ? KNIGHT : ff == 2 ? BISHOP : ff == 3 ? ADVISOR : KING;
    } else if (rr == 2) {
        t = (f == 1 || f == 7) ? CANNON : 0;
    } else if (rr == 3) {
        t = (f & 1) ? 0 : PAWN;
    }
    return t ? t + add : 0;
}

// Node(None, 1.0) (mcts.py:94) as the only node of board b's tree in pool half `half`, no pending leaf: what a new game
// (init_board) and MCTS.update_with_move(-1) (k_reset_tree) share. One lane.
__device__ __forceinline__ void fresh_root(const Dev &D, int b, int half)
{
    const size_t base = ((size_t)b * 2 + half) * (size_t)D.cap;
    D.nodeA[base] = NodeA{0, 0.0f, 1.0f, -1};
    D.nodeB[base] = 0u;
    const SolverCfg sv = *D.sv_cfg;
    if (sv.enabled) sv.proof[base] = 0; // a fresh root is unproven
    if (sv.spread) spread_array(D)[base] = 0.0f; // ... and has received no value
    D.path_len[b] = 0;
    D.leaf_status[b] = CCZ_LEAF_SKIP;
    D.move_sims[b] = 0; // a move boundary: the board's simulation budget (Dev.budget) starts over
    D.es_stopped[b] = 0; // ... and so does the early stop (S5): not stopped, no snapshot
    D.es_snap_s[b] = -1;
}

// A new game carries no resignation state: no run of low values, no play-on lot, no last value (the calibration counters in
// Dev.rs_stats are sums over games and stay). One lane. Called wherever a game starts; k_reset_tree keeps the state.
__device__ __forceinline__ void resign_clear(const Dev &D, int b)
{
    D.rs_state[b] = 0;
    D.rs_run[(size_t)b * 2] = 0;
    D.rs_run[(size_t)b * 2 + 1] = 0;
    D.rs_fire[b] = -1;
    D.rs_last[b] = __builtin_nanf("");
}

// A game that drew the play-on lot has ended with winner w after T plies: what resigning at the fire ply would have cost or saved
__device__ __forceinline__ void playon_count(const Dev &D, int b, int state, int winner, int T)
{
    ResignBoardStats &rs = D.rs_stats[b];
    rs.playon += 1;
    if (winner < 0) rs.playon_drawn += 1;
    else if (winner == (state & 1)) rs.playon_won += 1; // the side that would have resigned won: a false positive
    rs.playon_after += (unsigned long long)(T - D.rs_fire[b]);
}

// (re)initialise board b from D.root_sq[b] / the given turn+halfmove: key, chain, fresh tree, empty record
__device__ inline void init_board(const Dev &D, int b, int lane, int turn, int halfmove, bool new_game_no)
{
    const uint8_t *sq = D.root_sq + (size_t)b * 96;
    uint64_t k = 0;
    for (int s = lane; s < 90; s += 64) {
        const int pc = sq[s];
        if (pc) k ^= zob(pc, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k ^= __shfl_xor(k, o);
    if (turn) k ^= kTurnKey;
    if (lane == 0) {
        BoardMeta m = D.meta[b];
        m.key = k;
        m.halfmove = halfmove;
        m.chain_len = 1;
        m.ply = 0;
        m.n_nodes = 1;
        m.turn = (uint8_t)turn;
        m.over = 0;
        m.winner = -1;
        m.pi_used = 0;
        if (new_game_no) m.game_no += 1;
        m.half = (uint8_t)*D.half;
        D.meta[b] = m;
        D.chain[(size_t)b * kChainCap] = k;
        D.chain_chk[(size_t)b * 2] = 0ull; // (the first position of a chain never lies inside a repetition window)
        D.chain_chk[(size_t)b * 2 + 1] = 0ull;
        fresh_root(D, b, m.half);
        resign_clear(D, b);
    }
}

__global__ __launch_bounds__(64) void k_reset(Dev D, const uint8_t *mask)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[b]) return;
    uint8_t *sq = D.root_sq + (size_t)b * 96;
    for (int s = lane; s < 96; s += 64) sq[s] = s < 90 ? (uint8_t)start_piece(s) : 0;
    __syncthreads();
    init_board(D, b, lane, 1, 0, true);
}

// MCTS.update_with_move(-1) (mcts.py:176-178): a fresh root on the live pool half; position, history and record stay
__global__ void k_reset_tree(Dev D, const uint8_t *mask)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= D.B || (mask && !mask[b])) return;
    const int half = *D.half;
    fresh_root(D, b, half);
    D.meta[b].n_nodes = 1;
    D.meta[b].half = (uint8_t)half;
}

__global__ __launch_bounds__(64) void k_set_position(Dev D, int b, const uint8_t *sq_in, int turn, int halfmove)
{
    const int lane = threadIdx.x;
    uint8_t *sq = D.root_sq + (size_t)b * 96;
    for (int s = lane; s < 96; s += 64) sq[s] = s < 90 ? sq_in[s] : 0;
    __syncthreads();
    init_board(D, b, lane, turn, halfmove, true);
}

// ------------------------------------------------------------------ leaf evaluation shared by select and finish_move
struct LeafEval {
    int n_legal;
    int status; // CCZ_LEAF_*
    bool tie;
    bool insufficient;
    int rep;       // occurrences of the current position in the history chain (incl. itself)
    int first_occ; // chain index of its earliest occurrence
    int ksq;       // king square of the side to move
};

// s_chain[0..chain_len) holds the keys since the last capture incl. the current position (last)
__device__ inline LeafEval eval_position(const uint8_t *s_sq, int turn, int halfmove, uint64_t key,
                                         const uint64_t *s_chain, int chain_len, GenScratch &S,
                                         uint16_t *ids_out, int lane, bool &overflow, unsigned long long *sp = nullptr,
                                         const uint16_t *rank = nullptr, const uint16_t *unrank = nullptr, uint32_t trankpack = 0u)
{
    const GenResult g = gen_legal(s_sq, turn, S, ids_out, lane, sp, rank, unrank, trankpack);
    overflow = g.overflow;
    int rep = 0, first_occ = -1;
    for (int i0 = 0; i0 < chain_len; i0 += 64) {
        const int i = i0 + lane;
        const uint64_t hit = __ballot(i < chain_len && s_chain[i] == key);
        if (hit && first_occ < 0) first_occ = i0 + __ffsll((long long)hit) - 1;
        rep += __popcll(hit);
    }
    // tools.py:109-123 is_tie = insufficient material or fourfold repetition or sixty moves
    const bool sixty = halfmove >= 120 && g.n_legal > 0;
    LeafEval L;
    L.n_legal = g.n_legal;
    L.insufficient = g.insufficient;
    L.rep = rep;
    L.first_occ = first_occ;
    L.ksq = g.ksq;
    L.tie = g.insufficient || rep >= 4 || sixty;
    // mcts.py:116-126: not end and not tie -> expand ; end and tie -> 0.0 ; else side to move lost
    if (g.n_legal == 0) L.status = L.tie ? CCZ_LEAF_DRAW : CCZ_LEAF_LOSS;
    else L.status = L.tie ? CCZ_LEAF_DRAW : CCZ_LEAF_EXPAND;
    return L;
}

// ------------------------------------------------------------------ MCTS-solver: the proof byte of a node from its children's
// p0 / p1: the bytes of children `lane` and `64 + lane` of a node with nc <= 128 children (whatever a lane past nc passes is ignored).
// In this order: a child that is LOSS -> WIN in 1 + the smallest such distance; else an unknown child -> unknown; else a DRAW child
// -> DRAW; else every child is WIN -> LOSS in 1 + the largest distance. Distances saturate at 63. Two passes over the lanes (children
// 0..63, 64..127), the verdicts by ballot, the distances by a wave reduction. All 64 lanes call it; the result is wave-uniform.
__device__ __forceinline__ uint32_t proof_combine(uint32_t p0, uint32_t p1, int nc, int lane)
{
    if (nc <= 0) return 0u;
    bool anyL = false, anyU = false, anyD = false;
    int minL = 63, maxW = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bool in = 64 * h + lane < nc;
        const uint32_t p = h ? p1 : p0;
        const uint32_t st = p & 3u;
        const int ds = (int)((p >> 2) & 63u);
        anyL |= __ballot(in && st == kProofLoss) != 0ull;
        anyU |= __ballot(in && st == 0u) != 0ull;
        anyD |= __ballot(in && st == kProofDraw) != 0ull;
        if (in && st == kProofLoss && ds < minL) minL = ds;
        if (in && st == kProofWin && ds > maxW) maxW = ds;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(minL, o), c = __shfl_xor(maxW, o);
        minL = a < minL ? a : minL;
        maxW = c > maxW ? c : maxW;
    }
    if (anyL) return kProofWin | ((uint32_t)(minL < 62 ? minL + 1 : 63) << 2);
    if (anyU) return 0u;
    if (anyD) return kProofDraw;
    return kProofLoss | ((uint32_t)(maxW < 62 ? maxW + 1 : 63) << 2);
}

// ------------------------------------------------------------------ K1: select + make-move + movegen + terminal + encode
struct SelectShared {
    __align__(16) uint8_t sq[96];
    uint64_t chain[kChainCap];
    GenScratch S;
    union {
        __align__(16) uint32_t enc[948]; // staging of the 3 live plane groups (945 dwords); used after move generation
        struct {           // deferred make-move of the selection path; dead before move generation starts
            uint16_t mv[kMaxDepth];
            uint8_t from[kMaxDepth], to[kMaxDepth], pc[kMaxDepth], cap[kMaxDepth];
        } pm;
    };
};

// per-board state every phase needs, loaded in ONE round at the top of the kernel
struct Prefetch {
    BoardMeta m;
    uint32_t sqw;      // lane < 24: dword `lane` of the root mailbox
    uint64_t c0;       // chain key `lane` (keys 64.. are fetched on demand: > 64 plies without a capture is rare)
    int half;          // live pool half (one global word, the same for all boards)
    NodeA root;        // node 0 of the live half
    uint32_t rootw;
    NodeA kid;         // lane i: node 1 + i = child i of the root (the root's children always start at node 1)
    uint32_t kidw;
    int32_t budget;    // simulations the board may back up in this move (INT32_MAX: budgets off)
    int32_t move_sims; // ... and how many it has, as of the top of the kernel (this launch's backup is not in it)
    int32_t ex;        // root exploration (ccz_set_root_exploration) applies to the board's current move: on, and a policy-target move
    int32_t gm;        // Gumbel root search (ccz_set_gumbel) is on
    int32_t sr;        // search parameters (ccz_set_search) are on
    int32_t es;        // early stop per board (ccz_set_early_stop) is on
    SolverCfg sv;     // MCTS-solver (ccz_set_solver): on / off and where the proof bytes are
    uint32_t kidp;     // solver on: lane i: the proof byte of child i of the root (off: 0, nothing is read)
};

// what the expand+backup phase of this launch changed at the top of the tree (the prefetched root and
// root-children records predate those stores)
struct TopPatch {
    bool active;       // a backup ran
    bool root_expanded;// the root itself was the leaf and received children 1..k
    bool kid_expanded; // the depth-1 path node was the leaf and received children n0..n0+k
    int k, first_id, n0;
    int rootN;
    float rootQ;
    int node1, N1;     // path node at depth 1 (if depth >= 1) with its updated N, Q
    float Q1;
    bool has1;
    bool hasp1;        // solver: the backup rewrote the proof byte of node1 ...
    uint32_t p1;       // ... to this
};

// the solver's settings as a kernel reads them: once; `enabled` is tested wave-uniformly
__device__ __forceinline__ SolverCfg solver_cfg(const Dev &D)
{
    SolverCfg sv = *D.sv_cfg;
    sv.enabled = __builtin_amdgcn_readfirstlane(sv.enabled);
    sv.spread = __builtin_amdgcn_readfirstlane(sv.spread);
    return sv;
}

__device__ __forceinline__ Prefetch prefetch_board(const Dev &D, int b, int lane)
{
    Prefetch P;
    P.m = D.meta[b];
    P.sqw = lane < 24 ? ((const uint32_t *)(D.root_sq + (size_t)b * 96))[lane] : 0u;
    const uint64_t *ch = D.chain + (size_t)b * kChainCap;
    P.c0 = ch[lane];
    P.half = *D.half;
    const size_t base = ((size_t)b * 2 + P.half) * (size_t)D.cap;
    P.root = D.nodeA[base];
    P.rootw = D.nodeB[base];
    P.kid = D.nodeA[base + 1 + lane];
    P.kidw = D.nodeB[base + 1 + lane];
    P.budget = D.budget[b];
    P.move_sims = D.move_sims[b];
    P.ex = D.ex_cfg->enabled * (int32_t)D.target[b]; // (both words are requested with the rest: no load waits for the other)
    P.gm = D.gm_cfg->enabled;
    P.sr = D.sr_cfg->enabled;
    P.es = D.es_cfg->enabled;
    P.sv = solver_cfg(D); // (requested with the rest; off: no load waits for it)
    P.kidp = 0u;
    if (P.sv.enabled) P.kidp = P.sv.proof[base + 1 + lane];
    return P;
}

// The leaf end of a selection: the moves sh.pm.mv[0 .. depth) are made on the LDS board sh.sq (the root position), the Zobrist keys
// of the path extend the history chain sh.chain, then legal moves / game end (net.py:154-157, mcts.py:116-117) and the evaluator
// input of the leaf are written to the slots of board `b`. Shared by select_phase (b = the board searched) and k_scout (b = a scout
// slot: the leaf is a sibling of another board's pending leaf).
__device__ inline void leaf_tail(const Dev &D, int b, int lane, uint16_t *leaf_in, SelectShared &sh, int depth, int turn, int halfmove,
                                 int chain_len, uint64_t key, bool count_stats)
{
    uint8_t *s_sq = sh.sq;
    uint64_t *s_chain = sh.chain;
    CCZ_STAMP(D, b, lane, 4)
    // ---- replay the selection path on the LDS board: (1) table lookups in parallel, (2) the inherently
    // serial piece shuffling by one lane, (3) Zobrist deltas in parallel + XOR prefix scan
    if (depth > 0) {
        for (int j = lane; j < depth; j += 64) {
            const int mvj = sh.pm.mv[j];
            sh.pm.from[j] = c_tab.from[mvj];
            sh.pm.to[j] = c_tab.to[mvj];
        }
        wave_sync();
        int lastcap = -1;
        const bool pawn_zeroes = (D.rule_flags & 2u) != 0;
        if (lane == 0) {
            for (int j = 0; j < depth; ++j) {
                const int fr = sh.pm.from[j], to = sh.pm.to[j];
                const uint8_t pc = s_sq[fr], cp = s_sq[to];
                s_sq[to] = pc;
                s_sq[fr] = 0;
                sh.pm.pc[j] = pc;
                sh.pm.cap[j] = cp;
                if (cp || (pawn_zeroes && (pc & 7) == PAWN)) lastcap = j; // "lastcap" = last clock-resetting move
            }
        }
        lastcap = __builtin_amdgcn_readfirstlane(lastcap);
        wave_sync();
        // keys: key_j = root_key ^ XOR_{i<=j} delta_i ; a capture at move c restarts the chain at key_c
        const int first = lastcap >= 0 ? lastcap : 0;
        const int new_len = (lastcap >= 0 ? 0 : chain_len) + (depth - first);
        if (new_len > kChainCap) {
            set_err(D, 64);
            if (lane == 0) D.leaf_status[b] = CCZ_LEAF_SKIP;
            return;
        }
        uint64_t carry = key;
        const int off = lastcap >= 0 ? -first : chain_len; // chain slot of move j is off + j
        for (int j0 = 0; j0 < depth; j0 += 64) {
            const int j = j0 + lane;
            uint64_t dlt = 0;
            if (j < depth) {
                const int fr = sh.pm.from[j], to = sh.pm.to[j], pc = sh.pm.pc[j], cp = sh.pm.cap[j];
                dlt = zob(pc, fr) ^ zob(pc, to) ^ kTurnKey;
                if (cp) dlt ^= zob(cp, to);
            }
            dlt = wave_incl_xor64(dlt) ^ carry;
            if (j < depth && j >= first) s_chain[CCZ_IDX(D, off + j, kChainCap)] = dlt;
            carry = wave_readlane64(dlt, 63);
        }
        key = carry;
        halfmove = lastcap >= 0 ? depth - 1 - lastcap : halfmove + depth;
        chain_len = new_len;
        turn ^= depth & 1;
    }
    wave_sync();

    CCZ_STAMP(D, b, lane, 5)
    // ---- leaf: legal moves (net.py:154-157), game end (mcts.py:116-117)
    bool overflow;
#ifdef CCZ_STAMPS
    unsigned long long *sp = D.stamps + (size_t)b * 16;
#else
    unsigned long long *sp = nullptr;
#endif
    const LeafEval L = eval_position(s_sq, turn, halfmove, key, s_chain, chain_len, sh.S,
                                     D.leaf_ids + (size_t)b * kMaxLegal, lane, overflow, sp, D.rank, D.unrank, D.trankpack);
    if (overflow) set_err(D, 4);
    CCZ_STAMP(D, b, lane, 6)
    if (lane == 0) {
        D.path_len[b] = depth;
        D.leaf_key[b] = key;
        D.leaf_k[b] = L.n_legal > kMaxLegal ? kMaxLegal : L.n_legal;
        D.leaf_status[b] = (uint8_t)L.status;
        if (count_stats) {
            BoardStats &st = D.stats[b];
            st.sum_depth += (unsigned long long)depth;
            if (depth > st.depth_peak) st.depth_peak = depth;
        }
    }

    // ---- evaluator input (net.py:160-177): groups 7 (red now), 15 (black now), 16 (side to move).
    // Staged in LDS: fill (zeros / the turn plane), scatter one fp16 1.0 per piece, stream out as dwords.
    CCZ_STAMP(D, b, lane, 7)
    if (leaf_in) {
        uint32_t *enc = sh.enc;
        const uint32_t tv = turn ? 0x3C003C00u : 0u;
#pragma unroll
        for (int it = 0; it < 15; ++it) {
            const int i = lane + 64 * it;
            if (i < 945) enc[i] = i >= 630 ? tv : 0u;
        }
        wave_sync();
        {
            uint16_t *eh = (uint16_t *)enc;
            const int q0 = s_sq[lane];
            const int q1 = lane < 26 ? s_sq[64 + lane] : 0;
            if (q0) eh[(q0 >> 3) * 630 + plane_of(D, q0 & 7) * 90 + lane] = kHalfOne;
            if (q1) eh[(q1 >> 3) * 630 + plane_of(D, q1 & 7) * 90 + 64 + lane] = kHalfOne;
        }
        wave_sync();
        uint32_t *row = (uint32_t *)(leaf_in + (size_t)b * 10710);
#pragma unroll
        for (int it = 0; it < 15; ++it) {
            const int i = lane + 64 * it;
            if (i < 945) row[i + (i < 315 ? 2205 : (i < 630 ? 4725 - 315 : 5040 - 630))] = enc[i];
        }
    }
}

// ------------------------------------------------------------------ root exploration (ccz_set_root_exploration)
// The Dirichlet component of the root's children `lane` and `64 + lane` for the board's current move: dir_i = g_i / sum(g), g_i the
// board's Gamma(alpha) draws on Philox words 0..127 of (seed, board id, move counter) -- the draws the sampler mixes into pi when
// the feature is off --, summed in index order in float64 on lane 0 and stored as float32 in D.ex_dir. The row is filled once per
// move and board, under the wave-uniform stamp test; every later call reads it back. kids = the root's children; s_g = 128 doubles
// of LDS scratch. All 64 lanes call it.
__device__ inline void explore_dir(const Dev &D, const ExploreCfg &xc, int b, int lane, int k, uint32_t move_counter, const NodeA *kids,
                                   double *s_g, float &d0, float &d1)
{
    k = __builtin_amdgcn_readfirstlane(k); // (the same in every lane: say so, the tests below are scalar)
    move_counter = (uint32_t)__builtin_amdgcn_readfirstlane((int)move_counter);
    uint32_t *stp = D.ex_stamp + (size_t)b * 2;
    float *row = D.ex_dir + (size_t)b * kMaxLegal;
    const uint32_t st0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)stp[0]), st1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)stp[1]);
    if (st0 == move_counter + 1u && st1 == (uint32_t)k) {
        d0 = row[lane];
        d1 = row[64 + lane];
        return;
    }
    const uint64_t gid = D.board_id_base + (uint64_t)b;
    for (int i = lane; i < k; i += 64) s_g[i] = det_gamma(D.seed, gid, move_counter, (uint32_t)i, xc.alpha);
    wave_sync();
    double gs = 0.0;
    if (lane == 0) for (int i = 0; i < k; ++i) gs += s_g[i];
    gs = __shfl(gs, 0);
    d0 = 0.0f;
    d1 = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = 64 * h + lane;
        if (i < k) {
            const float f = (float)(gs > 0.0 ? s_g[i] / gs : (double)kids[CCZ_IDX(D, i, D.cap)].P);
            row[i] = f;
            if (h) d1 = f; else d0 = f;
        }
    }
    if (lane == 0) { stp[0] = move_counter + 1u; stp[1] = (uint32_t)k; }
    wave_sync();
}
// P'_i = (1 - eps) P_i + eps dir_i in float64, rounded to float32: what the root's score uses in place of the raw prior
__device__ __forceinline__ float explore_prior(const ExploreCfg &xc, float p, float dir)
{
    return (float)((1.0 - xc.eps) * (double)p + xc.eps * (double)dir);
}

// ------------------------------------------------------------------ Gumbel root search (ccz_set_gumbel, include/cczero.h)
// Entry t (0 <= t < n) of the considered-visits sequence seq(m, n): sequential halving over m moves with n simulations, written out
// as "how many move-visits the child to visit next has". Wave-uniform arguments give a wave-uniform loop of about 2 log2(m) rounds.
__device__ inline int gumbel_seq_at(int m, int n, int t)
{
    if (m <= 1) return t;
    int L = 0;
    while (L < 30 && (1 << L) < m) ++L;
    long long pos = 0, v = 0;
    int c = m;
    for (;;) {
        long long x = (long long)n / ((long long)L * c);
        if (x < 1) x = 1;
        const long long block = x * c;
        if ((long long)t < pos + block) return (int)(v + ((long long)t - pos) / c);
        pos += block;
        v += x;
        c = c / 2 > 2 ? c / 2 : 2;
    }
}

// lowest index among the root's children `lane` (s0, if c0) and `64 + lane` (s1, if c1) whose score is the maximum; -1: nothing
// comparable (no candidate, or NaN on every one). Wave-uniform result.
__device__ inline int gumbel_first_max(double s0, bool c0, double s1, bool c1, int lane)
{
    const double ninf = -__builtin_huge_val();
    const double a0 = (c0 && s0 == s0) ? s0 : ninf, a1 = (c1 && s1 == s1) ? s1 : ninf;
    const double top = wave_max_f64(a0 > a1 ? a0 : a1);
    const uint64_t h0 = __ballot(c0 && s0 == top), h1 = __ballot(c1 && s1 == top);
    if (h0) return __ffsll((long long)h0) - 1;
    if (h1) return 64 + __ffsll((long long)h1) - 1;
    return -1;
}
__device__ inline int wave_max_i32(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o); if (t > v) v = t; }
    return v;
}

// The row of the board's current move for the root's children `lane` ([0]) and `64 + lane` ([1]): Gumbel draw, logit of the raw
// prior, the visits the child had when the row was filled, and the move's n_eff and m. c[2]: those children's records as they stand.
// store (the selection): the row is filled once per move and board, under the wave-uniform stamp test, and read back afterwards.
// !store (k_finish_move, k_move_distribution): a board without a row gets one computed on the spot (N0 = N) and nothing is written.
struct GumbelRow { double g[2], logit[2]; int n0[2]; int n_eff, m; };
__device__ inline GumbelRow gumbel_row(const Dev &D, const GumbelCfg &gc, int b, int lane, int k, uint32_t move_counter, const NodeA *c,
                                       int sims_done, int budget, bool store)
{
    GumbelRow r;
    uint32_t *stp = D.gm_stamp + (size_t)b * 4;
    const size_t o = (size_t)b * kMaxLegal;
    const uint32_t st0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)stp[0]), st1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)stp[1]);
    if (st0 == move_counter + 1u && st1 == (uint32_t)k) {
        r.n_eff = __builtin_amdgcn_readfirstlane((int)stp[2]);
        r.m = __builtin_amdgcn_readfirstlane((int)stp[3]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = 64 * h + lane;
            r.g[h] = i < k ? D.gm_g[o + i] : 0.0;
            r.logit[h] = i < k ? D.gm_logit[o + i] : 0.0;
            r.n0[h] = i < k ? D.gm_n0[o + i] : 0;
        }
        return r;
    }
    const uint64_t gid = D.board_id_base + (uint64_t)b;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = 64 * h + lane;
        r.g[h] = 0.0; r.logit[h] = 0.0; r.n0[h] = 0;
        if (i < k) {
            double ua, ub;
            uniform2(D.seed, gid, move_counter, (uint32_t)i, 0xfffffu, ua, ub); // (the Gamma loop of child i stops below draw 0xffff2)
            r.g[h] = -det_log(-det_log(ua));
            r.logit[h] = det_log((double)c[h].P);
            r.n0[h] = c[h].N;
            if (store) { D.gm_g[o + i] = r.g[h]; D.gm_logit[o + i] = r.logit[h]; D.gm_n0[o + i] = r.n0[h]; }
        }
    }
    const int n_b = budget == 0x7fffffff ? gc.n_sims : budget;
    r.n_eff = n_b - sims_done > 1 ? n_b - sims_done : 1;
    r.m = gc.max_considered < k ? gc.max_considered : k;
    if (store && lane == 0) { stp[0] = move_counter + 1u; stp[1] = (uint32_t)k; stp[2] = (uint32_t)r.n_eff; stp[3] = (uint32_t)r.m; }
    return r;
}

// sigma_i = (c_visit + max_j N_j) * c_scale * cq_i for the children `lane` and `64 + lane` (c[2]), cq the completed Q in [0, 1]: the
// child's own (Q_i + 1) / 2 when visited, else v_mix, the prior-weighted mean of the visited children's mixed with the root's own
// mean. Float64; the two prior-weighted sums run in child order on lane 0. s_w: 128 doubles, s_p: 128 floats of LDS scratch.
__device__ inline void gumbel_sigma(const GumbelCfg &gc, int lane, int k, const NodeA *c, float rootQ, double *s_w, float *s_p, double *sig)
{
    double qt[2];
    int nsum = 0, nmax = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = 64 * h + lane;
        qt[h] = 0.0;
        if (i < k) {
            qt[h] = ((double)c[h].Q + 1.0) / 2.0;
            s_w[i] = (double)c[h].P * qt[h];
            s_p[i] = c[h].P;
            nsum += c[h].N;
            if (c[h].N > nmax) nmax = c[h].N;
        }
    }
    const uint64_t v0m = __ballot(lane < k && c[0].N > 0), v1m = __ballot(64 + lane < k && c[1].N > 0);
    wave_sync();
    const double S = (double)__builtin_amdgcn_readlane(wave_incl_scan(nsum, lane), 63);
    nmax = wave_max_i32(nmax);
    double vmix = (-(double)rootQ + 1.0) / 2.0;
    if (lane == 0 && (v0m | v1m)) {
        double wsum = 0.0, psum = 0.0;
        for (int i = 0; i < k; ++i)
            if (((i < 64 ? v0m : v1m) >> (i & 63)) & 1ull) { wsum += s_w[i]; psum += (double)s_p[i]; }
        vmix = (vmix + S * wsum / psum) / (1.0 + S);
    }
    vmix = __shfl(vmix, 0);
    wave_sync();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = 64 * h + lane;
        const double cq = (i < k && c[h].N > 0) ? qt[h] : vmix;
        sig[h] = (gc.c_visit + (double)nmax) * gc.c_scale * cq;
    }
}

// The root rule of the selection: which of the root's children are candidates (masks c0: children 0..63, c1: 64..127) and their
// scores g + logit + sigma (s0: child `lane`, s1: child `64 + lane`). kids = the root's children as they stand in memory.
struct GumbelPick { double s0, s1; uint64_t c0, c1; };
__device__ inline GumbelPick gumbel_select(const Dev &D, const GumbelCfg &gc, int b, int lane, int k, uint32_t move_counter, const NodeA *kids,
                                           float rootQ, int sims_done, int budget, double *s_w, float *s_p)
{
    k = __builtin_amdgcn_readfirstlane(k);
    move_counter = (uint32_t)__builtin_amdgcn_readfirstlane((int)move_counter);
    NodeA c[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) c[h] = 64 * h + lane < k ? kids[CCZ_IDX(D, 64 * h + lane, D.cap)] : NodeA{0, 0.0f, 0.0f, -1};
    const GumbelRow r = gumbel_row(D, gc, b, lane, k, move_counter, c, sims_done, budget, true);
    double sig[2];
    gumbel_sigma(gc, lane, k, c, rootQ, s_w, s_p, sig);
    const int M0 = c[0].N - r.n0[0], M1 = c[1].N - r.n0[1]; // (past k: 0 - 0)
    const int t = __builtin_amdgcn_readlane(wave_incl_scan(M0 + M1, lane), 63);
    const bool in0 = lane < k, in1 = 64 + lane < k;
    GumbelPick p;
    p.s0 = r.g[0] + r.logit[0] + sig[0];
    p.s1 = r.g[1] + r.logit[1] + sig[1];
    p.c0 = 0ull; p.c1 = 0ull;
    if (t < r.n_eff) {
        const int want = gumbel_seq_at(r.m, r.n_eff, t);
        p.c0 = __ballot(in0 && M0 == want);
        p.c1 = __ballot(in1 && M1 == want);
    }
    if ((p.c0 | p.c1) == 0ull) {
        const int a0 = in0 ? M0 : (int)0x80000000, a1 = in1 ? M1 : (int)0x80000000;
        const int mx = wave_max_i32(a0 > a1 ? a0 : a1);
        p.c0 = __ballot(in0 && M0 == mx);
        p.c1 = __ballot(in1 && M1 == mx);
    }
    return p;
}

// ------------------------------------------------------------------ search parameters (ccz_set_search, include/cczero.h)
// R1: the exploration constant of a node with N visits. c_factor == 0 (or the rule off): c_puct as it is, no logarithm.
__device__ __forceinline__ float search_c_eff(float c_puct, const SearchCfg &sr, int N)
{
    if (!sr.enabled || sr.c_factor == 0.0) return c_puct;
    return (float)((double)c_puct + sr.c_factor * det_log(((double)N + sr.c_base + 1.0) / sr.c_base));
}
// R2: the visited prior mass of a node, from lane l's children l (a) and 64 + l (b), each the child's raw prior when it exists and
// has visits, else 0.0: m_l = a + b, then m_l = m_l + m_{l xor s} for s = 32, 16, 8, 4, 2, 1. IEEE addition is commutative, so every
// lane ends with the same bits.
__device__ __forceinline__ double search_mass(double a, double b)
{
    double m = a + b;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = m + __shfl_xor(m, s);
    return m;
}
// R3: the value an unvisited child of a node takes for Q. q: the node's running mean as stored (the view of the side that moved into
// it), mass: R2.
__device__ __forceinline__ double search_fpu(int mode, double value, float q, double mass)
{
    if (mode == 1) return (double)(-q) - value * sqrt(mass);
    if (mode == 2) return value;
    return __builtin_huge_val();
}

// ------------------------------------------------------------------ early stop per board (ccz_set_early_stop, include/cczero.h)
// S1-S5 at one selection of board b: the reason the board is stopped (one it stopped with earlier in the move, or the rule that
// fires now: 1 single reply, 2 visit gap, 3 KLD gain), 0: it goes on searching. root / rootw: the root record with this launch's
// backup patched in. The counts of children 0..63 come from the prefetched records (P.kid + TopPatch), those of children 64..127
// from memory, where the fence in front of the selection made this launch's backup visible. All 64 lanes call it; everything it
// branches on is wave-uniform, and the state (Dev.es_*) is written by ordinary stores, the scalars from lane 0.
__device__ inline int early_stop(const Dev &D, int b, int lane, const Prefetch &P, const TopPatch &tp, const NodeA &root, uint32_t rootw,
                                 const NodeA *A)
{
    const int was = __builtin_amdgcn_readfirstlane((int)D.es_stopped[b]);
    if (was) return was; // S5: stopped earlier in this move
    int k = __builtin_amdgcn_readfirstlane((int)(rootw >> 16));
    if (k < 1) return 0;
    if (k > kMaxLegal) k = kMaxLegal;
    const StopCfg sc = *D.es_cfg;
    const int s = __builtin_amdgcn_readfirstlane(P.move_sims + (tp.active ? 1 : 0));
    const int n_b = __builtin_amdgcn_readfirstlane(P.budget == 0x7fffffff ? sc.n_sims : P.budget);
    if (s >= n_b || s < sc.min_sims) return 0; // S1
    const int fc = __builtin_amdgcn_readfirstlane(root.fc);
    const bool in0 = lane < k, in1 = 64 + lane < k;
    int n0 = 0, n1 = 0;
    if (in0) {
        if (fc == 1) {
            n0 = P.kid.N;
            if (tp.root_expanded) n0 = 0;
            else if (tp.has1 && 1 + lane == tp.node1) n0 = tp.N1;
        } else {
            n0 = A[CCZ_IDX(D, fc + lane, D.cap)].N;
        }
    }
    if (in1) n1 = A[CCZ_IDX(D, fc + 64 + lane, D.cap)].N;
    int reason = 0;
    if (sc.single_reply && k == 1) reason = 1; // S2
    if (!reason && sc.gap_factor != 0.0) {     // S3: the first maximum, then the best of the others (both over children 0..127)
        const int a0 = in0 ? n0 : -1, a1 = in1 ? n1 : -1;
        const int N1 = wave_max_i32(a0 > a1 ? a0 : a1);
        const uint64_t h0 = __ballot(a0 == N1), h1 = __ballot(a1 == N1);
        const int i1 = h0 ? __ffsll((long long)h0) - 1 : 64 + __ffsll((long long)h1) - 1;
        const int r0 = (in0 && lane != i1) ? n0 : 0, r1 = (in1 && 64 + lane != i1) ? n1 : 0;
        const int N2 = wave_max_i32(r0 > r1 ? r0 : r1);
        if ((double)(N1 - N2) * sc.gap_factor > (double)(n_b - s)) reason = 2;
    }
    if (!reason && sc.kld_interval > 0 && s > 0 && s % sc.kld_interval == 0) { // S4
        int32_t *snap = D.es_snap + (size_t)b * kMaxLegal;
        const int snap_s = __builtin_amdgcn_readfirstlane(D.es_snap_s[b]);
        if (s != snap_s) { // (a selection repeated without a backup finds its own snapshot)
            if (snap_s >= 0) {
                const int p0 = snap[lane], p1 = snap[64 + lane];
                const int Sc = __builtin_amdgcn_readlane(wave_incl_scan(n0 + n1, lane), 63);
                const int Sp = __builtin_amdgcn_readlane(wave_incl_scan(p0 + p1, lane), 63);
                if (Sc > Sp) {
                    double t0 = 0.0, t1 = 0.0;
                    if (p0 > 0) { const double o = (double)p0 / (double)Sp, n = (double)n0 / (double)Sc; t0 = o * det_log(o / n); }
                    if (p1 > 0) { const double o = (double)p1 / (double)Sp, n = (double)n1 / (double)Sc; t1 = o * det_log(o / n); }
                    const double G = search_mass(t0, t1) / (double)(Sc - Sp);
                    if (G < sc.min_gain) reason = 3; // (a NaN does not fire)
                }
            }
            snap[lane] = n0;
            snap[64 + lane] = n1;
            if (lane == 0) { D.es_snap_s[b] = s; D.es_stats[b].evaluations += 1; }
        }
    }
    if (reason && lane == 0) { // S5
        D.es_stopped[b] = (uint8_t)reason;
        StopBoardStats &st = D.es_stats[b];
        st.stops[reason] += 1;
        st.sims_saved += (unsigned long long)(n_b - s);
    }
    return reason;
}

// One wave: PUCT descent from the root of board b, leaf rules, evaluator input. Per tree level there is
// ONE dependent global load round (the children's 16-B NodeA records + their move/count words); the
// chosen child's own N / first_child / count are broadcast from the winning lane, not re-read.
// EX: the root exploration of ccz_set_root_exploration is compiled in (not in the scouted run: the two exclude each other).
template <bool EX>
__device__ inline void select_phase(const Dev &D, int b, int lane, uint16_t *leaf_in, SelectShared &sh, const Prefetch &P,
                                    const TopPatch &tp)
{
    uint8_t *s_sq = sh.sq;
    uint64_t *s_chain = sh.chain;
    const BoardMeta m = P.m;
    // a board whose move has used up its simulation budget selects nothing, like a finished one: no evaluator row, no simulation
    // counted (the prefetched count predates this launch's backup: tp.active adds it)
    if (m.over || P.move_sims + (tp.active ? 1 : 0) >= P.budget) {
        if (lane == 0) D.leaf_status[b] = CCZ_LEAF_SKIP;
        return;
    }
    const size_t base = ((size_t)b * 2 + P.half) * (size_t)D.cap;
    const NodeA *A = D.nodeA + base;
    const uint32_t *Bn = D.nodeB + base;
    // the root record was requested together with everything else at the top of the kernel; what this
    // launch's backup changed in it is patched in from registers
    NodeA pa = P.root;
    uint32_t nb = P.rootw;
    if (tp.active) {
        pa.N = tp.rootN;
        pa.Q = tp.rootQ;
        if (tp.root_expanded) { pa.fc = 1; nb = (nb & 0xffffu) | ((uint32_t)tp.k << 16); }
    }
    // ---- early stop per board (off: the one prefetched word tested here): a stopped board is a board whose budget is spent
    if (__builtin_amdgcn_readfirstlane(P.es) && early_stop(D, b, lane, P, tp, pa, nb, A) != 0) {
        if (lane == 0) D.leaf_status[b] = CCZ_LEAF_SKIP;
        return;
    }
    if (lane < 24) {
        uint32_t v = P.sqw;
        if (lane == 22) v &= 0x0000ffffu;
        if (lane == 23) v = 0u;
        ((uint32_t *)s_sq)[lane] = v;
    }
    s_chain[lane] = P.c0;
    if (m.chain_len > 64) s_chain[64 + lane] = D.chain[(size_t)b * kChainCap + 64 + lane];
    wave_sync();

    CCZ_STAMP(D, b, lane, 3)
    int32_t *path = D.path + (size_t)b * D.maxd;
    int depth = 0, turn = m.turn, halfmove = m.halfmove, chain_len = m.chain_len;
    uint64_t key = m.key;
    bool bad = false;
    if (lane == 0) path[0] = 0;
    const bool solver = P.sv.enabled != 0;
    const uint8_t *proof = P.sv.proof + base;
    uint32_t proven = 0u;

    // ---- root exploration: noisy priors and forced playouts at depth 0 (off: the one prefetched word tested here)
    bool ex = false;
    ExploreCfg xc;
    xc.enabled = 0; xc.prune = 0; xc.eps = 0.0; xc.alpha = 1.0; xc.forced_k = 0.0;
    float xd0 = 0.0f, xd1 = 0.0f;
    if (EX && __builtin_amdgcn_readfirstlane(P.ex) && (nb >> 16) != 0u) {
        ex = true;
        xc = *D.ex_cfg;
        explore_dir(D, xc, b, lane, (int)(nb >> 16), m.move_counter, A + pa.fc, (double *)sh.S.cand, xd0, xd1);
    }
    // ---- Gumbel root search: candidates and scores of the root's children (off: the one prefetched word tested here). The children
    // are read as they stand in memory: the fence in front of this phase made this launch's backup visible
    bool gm = false;
    GumbelPick gp;
    gp.s0 = 0.0; gp.s1 = 0.0; gp.c0 = 0ull; gp.c1 = 0ull;
    if (EX && __builtin_amdgcn_readfirstlane(P.gm) && (nb >> 16) == 0u) {
        // an unexpanded root is a fresh tree (reset, set position, a refused move): whatever row the board holds for this move counter
        // belonged to another tree
        if (lane == 0) D.gm_stamp[(size_t)b * 4] = 0u;
    } else if (EX && __builtin_amdgcn_readfirstlane(P.gm)) {
        gm = true;
        const GumbelCfg gc = *D.gm_cfg;
        gp = gumbel_select(D, gc, b, lane, (int)(nb >> 16), m.move_counter, A + pa.fc, pa.Q, P.move_sims + (tp.active ? 1 : 0), P.budget,
                           (double *)sh.S.cand, (float *)sh.S.list);
    }

    // ---- search parameters (ccz_set_search; off: the one prefetched word tested here)
    const bool srch = EX && __builtin_amdgcn_readfirstlane(P.sr) != 0;
    SearchCfg sr;
    sr.enabled = 0; sr.fpu_mode = 0; sr.fpu_root_mode = 0; sr.pad = 0;
    sr.fpu_value = 0.0; sr.fpu_root_value = 0.0; sr.c_base = 1.0; sr.c_factor = 0.0;
    if (srch) sr = *D.sr_cfg;

    // ---- PUCT descent (mcts.py:105-111, 41-61). Compiled twice, chosen by the wave-uniform solver word: with the solver off the
    // loop is the one it was (no proof byte in it); SV: std::true_type / std::false_type. Likewise GM, the Gumbel root, and SR, the
    // search parameters: off, no word of them is in the loop
    const auto descend = [&](auto SV, auto GM, auto SR) {
        constexpr bool SOLVER = decltype(SV)::value;
        constexpr bool GUMBEL = decltype(GM)::value;
        constexpr bool SEARCH = decltype(SR)::value;
        for (;;) {
            const int nc = (int)(nb >> 16);
            if (nc == 0) break;
            const double sqrtNp = sqrt((double)pa.N); // np.sqrt(parent.visits): float64
            double best = -__builtin_huge_val();
            int besti = 0x7fffffff, bN = 0, bfc = -1;
            float bQ = 0.0f;
            uint32_t bw = 0, bP = 0;
            bool bF = false;
            const bool exroot = EX && !GUMBEL && ex && depth == 0; // (the two exclude each other)
            const bool gmroot = GUMBEL && depth == 0;
            // the record, move / count word and proof byte (solver off: none) of child i = c0 + lane, in one load round. Root
            // children: prefetched (+ this launch's backup). The patch of a root expanded in this launch knows child 0's move only
            // (PUCT takes the first unvisited child): the Gumbel root reads the records as they stand in memory, and so does a root
            // under the search parameters, whose first choice is the first maximum of R4
            const auto load = [&](int c0, int i, NodeA &c, uint32_t &w, uint32_t &pb) {
                if (depth == 0 && c0 == 0 && pa.fc == 1 && !gmroot && !(SEARCH && tp.root_expanded)) {
                    c = P.kid;
                    w = P.kidw;
                    if (SOLVER) pb = P.kidp;
                    if (tp.root_expanded) { c.N = 0; c.Q = 0.0f; c.fc = -1; w = (uint32_t)tp.first_id; pb = 0u; }
                    else if (tp.has1 && 1 + i == tp.node1) {
                        c.N = tp.N1;
                        c.Q = tp.Q1;
                        if (tp.kid_expanded) { c.fc = tp.n0; w = (w & 0xffffu) | ((uint32_t)tp.k << 16); }
                        if (SOLVER && tp.hasp1) pb = tp.p1;
                    }
                } else {
                    c = A[CCZ_IDX(D, pa.fc + i, D.cap)];
                    w = Bn[CCZ_IDX(D, pa.fc + i, D.cap)];
                    if (SOLVER) pb = proof[CCZ_IDX(D, pa.fc + i, D.cap)];
                }
            };
            // search parameters, once per level: the children (a node has at most 128) are loaded ahead of the scoring pass, which
            // takes them from registers; the mass of the visited ones (R2), the urgency (R3) and the exploration constant (R1)
            NodeA kc[2];
            uint32_t kw[2], kp[2];
            double fpu = __builtin_huge_val();
            float ceff = D.c_puct;
            if (SEARCH) {
                double pm[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    kc[h] = NodeA{0, 0.0f, 0.0f, -1};
                    kw[h] = 0u;
                    kp[h] = 0u;
                    if (64 * h + lane < nc) load(64 * h, 64 * h + lane, kc[h], kw[h], kp[h]);
                    pm[h] = kc[h].N > 0 ? (double)kc[h].P : 0.0; // (past nc: N = 0)
                }
                const double mass = search_mass(pm[0], pm[1]);
                fpu = search_fpu(depth == 0 ? sr.fpu_root_mode : sr.fpu_mode, depth == 0 ? sr.fpu_root_value : sr.fpu_value, pa.Q, mass);
                ceff = search_c_eff(D.c_puct, sr, pa.N);
            }
            for (int c0 = 0; c0 < nc; c0 += 64) {
                const int i = c0 + lane;
                if (i < nc) {
                    NodeA c;
                    uint32_t w, pb = 0u; // pb: the candidate's proof byte, loaded in the round of its record (solver off: none)
                    if (SEARCH && c0 < 128) { c = kc[c0 >> 6]; w = kw[c0 >> 6]; pb = kp[c0 >> 6]; }
                    else load(c0, i, c, w, pb);
                    // value + c_puct*prob*sqrt(N_parent)/(1+N): float32 product, float64 elsewhere; inf if unvisited
                    float pp = c.P;
                    bool fsel = false;
                    if (exroot) { // P' for P, and a visited child short of its forced playouts scores like an unvisited one
                        pp = explore_prior(xc, c.P, c0 ? xd1 : xd0);
                        fsel = xc.forced_k > 0.0 && c.N > 0 && (double)c.N < sqrt(xc.forced_k * (double)pp * (double)(pa.N - 1));
                    }
                    double sc;
                    if (SEARCH) // R4: an unvisited child scores like a visited one with Q = the urgency (+inf under mode 0) and N = 0
                        sc = (fsel || (c.N == 0 && fpu == __builtin_huge_val()))
                                 ? __builtin_huge_val()
                                 : (c.N == 0 ? fpu : (double)c.Q) + (double)(ceff * pp) * sqrtNp / (double)(1 + c.N);
                    else
                        sc = (c.N == 0 || fsel) ? __builtin_huge_val()
                                                : (double)c.Q + (double)(D.c_puct * pp) * sqrtNp / (double)(1 + c.N);
                    // Gumbel root: g + logit + sigma of a candidate; every other child is out of the comparison (like a NaN score)
                    if (gmroot) sc = (((c0 ? gp.c1 : gp.c0) >> lane) & 1ull) ? (c0 ? gp.s1 : gp.s0) : __builtin_nan("");
                    if (sc > best) { best = sc; besti = i; bN = c.N; bQ = c.Q; bfc = c.fc; bw = w; bF = fsel; if (SOLVER) bP = pb; }
                }
            }
            // first maximum in insertion order wins (Python max()): wave max of the score, then the lowest index
            // holding it (a lane's running best is its lowest-index maximum; indices < 64 precede the second pass)
            const double top = wave_max_f64(best);
            const bool hit = best == top && besti < nc;
            const uint64_t h0 = __ballot(hit && besti < 64), h1 = __ballot(hit);
            if (h1 == 0ull) { bad = true; set_err(D, 32); break; } // NaN priors: no comparable child
            const int owner = __builtin_amdgcn_readfirstlane((h0 ? __ffsll((long long)h0) : __ffsll((long long)h1)) - 1);
            besti = __builtin_amdgcn_readlane(besti, owner);
            if (exroot && __builtin_amdgcn_readlane((int)bF, owner) && lane == 0) D.ex_stats[b].forced += 1;
            const int child = pa.fc + besti;
            pa.N = __builtin_amdgcn_readlane(bN, owner);
            pa.Q = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bQ), owner));
            pa.fc = __builtin_amdgcn_readlane(bfc, owner);
            nb = (uint32_t)__builtin_amdgcn_readlane((int)bw, owner);
            const int mv = (int)(nb & 0xffffu);
            // board.push(move) (mcts.py:111) is DEFERRED: only the move id is noted here, so that a tree level costs
            // one global load round plus the arg-max and nothing else sits on the critical path
            if (lane == 0) sh.pm.mv[depth] = (uint16_t)mv;
            ++depth;
            if (depth >= D.maxd) { bad = true; set_err(D, 2); break; }
            if (lane == 0) path[CCZ_IDX(D, depth, D.maxd)] = child;
            // MCTS-solver: a chosen child (depth >= 1: never the root) whose result is proven ends the descent
            if (SOLVER) {
                proven = (uint32_t)__builtin_amdgcn_readlane((int)bP, owner) & 3u;
                if (proven) break;
            }
        }
    };
    const std::true_type on{};
    const std::false_type off{};
    if (EX && srch) {
        if (gm) { if (solver) descend(on, on, on); else descend(off, on, on); }
        else if (solver) descend(on, off, on);
        else descend(off, off, on);
    } else if (EX && gm) {
        if (solver) descend(on, on, off);
        else descend(off, on, off);
    } else if (solver) descend(on, off, off);
    else descend(off, off, off);
    wave_sync();
    if (bad) {
        if (lane == 0) D.leaf_status[b] = CCZ_LEAF_SKIP;
        return;
    }
    if (proven) { // the leaf is that node: no pushes, no move generation, no evaluator row; the backup takes the value from the status
        if (lane == 0) {
            D.path_len[b] = depth;
            D.leaf_k[b] = 0;
            D.leaf_status[b] = (uint8_t)(proven == kProofWin ? CCZ_LEAF_WIN : proven == kProofLoss ? CCZ_LEAF_LOSS : CCZ_LEAF_DRAW);
            BoardStats &st = D.stats[b];
            st.sum_depth += (unsigned long long)depth;
            if (depth > st.depth_peak) st.depth_peak = depth;
        }
        return;
    }

    leaf_tail(D, b, lane, leaf_in, sh, depth, turn, halfmove, chain_len, key, true);
}

__global__ __launch_bounds__(64) void k_select(Dev D, uint16_t *leaf_in)
{
    __shared__ SelectShared sh;
    const Prefetch P = prefetch_board(D, blockIdx.x, threadIdx.x);
    TopPatch none;
    none.active = false; none.root_expanded = false; none.kid_expanded = false; none.k = 0; none.first_id = 0; none.n0 = 0;
    none.rootN = 0; none.rootQ = 0.0f; none.node1 = -1; none.N1 = 0; none.Q1 = 0.0f; none.has1 = false; none.hasp1 = false; none.p1 = 0u;
    select_phase<true>(D, blockIdx.x, threadIdx.x, leaf_in, sh, P, none);
}

// ------------------------------------------------------------------ scouts: the NEXT leaves of a board, before it asks for them
// The reference's first-maximum rule (mcts.py:47-48,59-61: an unvisited child scores +inf, max() returns the first one) makes the
// order in which a node's children are first visited the order of board.legal_moves: after child i of a node X has been expanded,
// the next simulations that reach X expand children i + 1, i + 2, ... So when board r's pending leaf is child i of X, scout slot
// (active + j * active + r) is handed child i + 1 + j of X as ITS pending leaf -- position, legal moves, status, key and evaluator
// input, exactly what the selection writes for a leaf -- and goes through the evaluation cache's plan with it: one evaluator call of
// `1 + scouts` rows answers the leaf AND its next siblings, which board r then finds in the table (ccz_scout, round 6: one game at a
// time -- MCTS_AI, the UCI loop -- is one 90-pixel row per evaluator call, the worst shape for the chip). Scout slots have no tree
// and no game of their own (the simulator kernels run on boards 0 .. active - 1 only); they read board r's root, chain and path.
// Results are unchanged: the table returns what the evaluator returns for the position (tests/test_gpu_scouts.py).
__device__ inline void scout_wave(const Dev &D, uint16_t *leaf_in, int active, int q, int lane, SelectShared &sh)
{
    const int b = active + q;                           // the scout slot
    const int r = q % active;                           // the board it scouts for
    const int ahead = 1 + q / active;                   // how many children past that board's pending leaf
    const Prefetch P = prefetch_board(D, r, lane);
    const int d = D.path_len[r];
    const int st_r = D.leaf_status[r];
    const int32_t *path = D.path + (size_t)r * D.maxd;
    const int pj = path[lane < D.maxd ? lane : 0];      // path nodes 0 .. 63 (deeper paths are not scouted)
    bool none = P.m.over || d < 1 || d >= 64 || st_r == CCZ_LEAF_SKIP || st_r == CCZ_LEAF_NONE;
    const size_t base = ((size_t)r * 2 + P.half) * (size_t)D.cap;
    const NodeA *A = D.nodeA + base;
    const uint32_t *Bn = D.nodeB + base;
    int sib = -1;
    if (!none) {
        const int leaf = __builtin_amdgcn_readlane(pj, __builtin_amdgcn_readfirstlane(d));
        const int par = __builtin_amdgcn_readlane(pj, __builtin_amdgcn_readfirstlane(d - 1));
        const NodeA X = A[CCZ_IDX(D, par, D.cap)];
        const int nc = (int)(Bn[CCZ_IDX(D, par, D.cap)] >> 16);
        sib = leaf + ahead;
        // the sibling exists, and nobody has been there: an expanded or visited child already has its evaluation (or needs none)
        none = X.fc < 0 || leaf < X.fc || sib >= X.fc + nc;
        if (!none) {
            const NodeA S = A[CCZ_IDX(D, sib, D.cap)];
            none = S.fc >= 0 || S.N != 0;
        }
    }
    if (none) {
        if (lane == 0) { D.leaf_status[b] = CCZ_LEAF_NONE; D.leaf_k[b] = 0; D.path_len[b] = 0; }
        return;
    }
    // the LDS board and chain of board r (as select_phase sets them up), the moves down to X, then the sibling's move
    if (lane < 24) {
        uint32_t v = P.sqw;
        if (lane == 22) v &= 0x0000ffffu;
        if (lane == 23) v = 0u;
        ((uint32_t *)sh.sq)[lane] = v;
    }
    sh.chain[lane] = P.c0;
    if (P.m.chain_len > 64) sh.chain[64 + lane] = D.chain[(size_t)r * kChainCap + 64 + lane];
    if (lane >= 1 && lane < d) sh.pm.mv[lane - 1] = (uint16_t)(Bn[CCZ_IDX(D, pj, D.cap)] & 0xffffu);
    if (lane == 0) sh.pm.mv[d - 1] = (uint16_t)(Bn[CCZ_IDX(D, sib, D.cap)] & 0xffffu);
    wave_sync();
    leaf_tail(D, b, lane, leaf_in, sh, d, P.m.turn, P.m.halfmove, P.m.chain_len, P.m.key, false);
}

__global__ __launch_bounds__(64) void k_scout(Dev D, uint16_t *leaf_in, int active)
{
    __shared__ SelectShared sh;
    scout_wave(D, leaf_in, active, blockIdx.x, threadIdx.x, sh);
}

// ------------------------------------------------------------------ MCTS-solver: the backup of a decided simulation
// Wave-uniform and sequential: the leaf's byte, then from its parent up to the root byte <- proof_combine(children) until a byte does
// not change. The path nodes' child ranges and stored bytes come in one round (lane j: path node j = pj), then one round per level
// walked: the children's bytes -- the child just rewritten is taken from registers, not read back. proof / A / Bn: the board's live
// pool half; leaf = path node d if d < 64. Returns the new byte of the depth-1 path node | 0x100 if it was rewritten (TopPatch).
// Runs on terminal simulations only: kept out of line, so that the simulator kernels carry its registers only across the call.
__device__ __attribute__((noinline)) uint32_t proof_backup(const Dev &D, uint8_t *proof, const NodeA *A, const uint32_t *Bn, const int32_t *path,
                                                           SolverBoardStats *stats, int pj, int d, int status, int leaf, int lane)
{
    uint32_t top = 0u;
    int fcl = -1, ncl = 0;
    uint32_t pl = 0u;
    if (lane <= d && lane < 64) {
        const int node = (int)CCZ_IDX(D, pj, D.cap);
        fcl = A[node].fc;
        ncl = (int)(Bn[node] >> 16);
        pl = proof[node];
    }
    int childn = (int)CCZ_IDX(D, d < 64 ? leaf : path[CCZ_IDX(D, d, D.maxd)], D.cap);
    uint32_t cur = d < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)pl, __builtin_amdgcn_readfirstlane(d < 64 ? d : 0)) : (uint32_t)proof[childn];
    const bool stopped = (cur & 3u) != 0u; // the descent ended at a node proven earlier: its byte stays
    int newly = 0;
    bool walk = true;
    if (!stopped) {
        if (status == CCZ_LEAF_WIN) walk = false; // (no such leaf: a WIN status comes from a proven byte)
        else {
            cur = status == CCZ_LEAF_DRAW ? kProofDraw : kProofLoss; // decided by the rules: distance 0
            if (lane == 0) proof[childn] = (uint8_t)cur;
            newly = 1;
        }
    }
    if (walk && d == 1) top = 0x100u | cur;
    for (int j = d - 1; walk && j >= 0; --j) {
        int node, fc, nc;
        uint32_t stored;
        if (j < 64) {
            const int js = __builtin_amdgcn_readfirstlane(j);
            node = (int)CCZ_IDX(D, __builtin_amdgcn_readlane(pj, js), D.cap);
            fc = __builtin_amdgcn_readlane(fcl, js);
            nc = __builtin_amdgcn_readlane(ncl, js);
            stored = (uint32_t)__builtin_amdgcn_readlane((int)pl, js);
        } else {
            node = (int)CCZ_IDX(D, path[CCZ_IDX(D, j, D.maxd)], D.cap);
            fc = A[node].fc;
            nc = (int)(Bn[node] >> 16);
            stored = proof[node];
        }
        if (nc > kMaxLegal) nc = kMaxLegal;
        uint32_t p0 = 0u, p1 = 0u;
        if (lane < nc) p0 = proof[CCZ_IDX(D, fc + lane, D.cap)];
        if (64 + lane < nc) p1 = proof[CCZ_IDX(D, fc + 64 + lane, D.cap)];
        if (fc + lane == childn) p0 = cur;
        if (fc + 64 + lane == childn) p1 = cur;
        const uint32_t nw = proof_combine(p0, p1, nc, lane);
        if (nw == stored) break;
        if (lane == 0) proof[node] = (uint8_t)nw;
        newly += ((stored & 3u) == 0u && (nw & 3u) != 0u) ? 1 : 0;
        if (j == 1) top = 0x100u | nw;
        cur = nw;
        childn = node;
    }
    if (lane == 0) {
        stats->proven += (unsigned long long)newly;
        stats->stops += stopped ? 1ull : 0ull;
    }
    return top;
}

// ------------------------------------------------------------------ K2: expand + backup
// prob: dense [B][2086] priors (compact == false) or compact [B][128] priors aligned with leaf_ids (compact == true)
// r: the board whose tree, node pool and counters are updated; b: the slot holding the pending leaf (path, ids, status, priors, value).
// r == b everywhere but in the wide search (k_wide), where slot r + j * A holds the j-th pending leaf of board r.
template <bool COMPACT>
__device__ inline TopPatch expand_backup_phase(const Dev &D, int r, int b, int lane, const float *prob, const float *value,
                                               const BoardMeta &m0, int half, const SolverCfg &sv)
{
    TopPatch tp;
    tp.active = false; tp.root_expanded = false; tp.kid_expanded = false; tp.k = 0; tp.first_id = 0; tp.n0 = 0; tp.rootN = 0;
    tp.rootQ = 0.0f; tp.node1 = -1; tp.N1 = 0; tp.Q1 = 0.0f; tp.has1 = false; tp.hasp1 = false; tp.p1 = 0u;
    const bool solver = sv.enabled != 0;
    const bool spread = sv.spread != 0; // value spread (ccz_set_value_stats): wave-uniform; off: no S is read or written, nor its pointer
    // everything that does not depend on another load is requested first
    const int status = D.leaf_status[b];
    const int d = D.path_len[b];
    const int k_leaf = D.leaf_k[b];
    const float v_net = value ? value[b] : D.vleaf[b]; // value == nullptr: the engine-owned leaf values of the planned evaluator boundary
    const int32_t *path = D.path + (size_t)b * D.maxd;
    const uint16_t *ids = D.leaf_ids + (size_t)b * kMaxLegal;
    const int id0 = ids[lane], id1 = ids[64 + lane];
    // compact priors need no second, id-dependent load round: they are requested here with everything else
    float cp0 = 0.0f, cp1 = 0.0f;
    if (COMPACT) { cp0 = prob[(size_t)b * kMaxLegal + lane]; cp1 = prob[(size_t)b * kMaxLegal + 64 + lane]; }
    const int pj = path[lane < D.maxd ? lane : 0];
    if (status == CCZ_LEAF_SKIP) return tp;
    CCZ_STAMP(D, b, lane, 8)
    BoardMeta *mp = D.meta + r;
    const size_t base = ((size_t)r * 2 + half) * (size_t)D.cap;
    NodeA *A = D.nodeA + base;
    uint32_t *Bn = D.nodeB + base;
    const int leaf = __builtin_amdgcn_readlane(pj, __builtin_amdgcn_readfirstlane(d < 64 ? d : 0));
    float v;
    if (status == CCZ_LEAF_EXPAND) {
        // Node.expand (mcts.py:31-39): one child per legal id, ascending id order
        const int k = k_leaf;
        const int n0 = m0.n_nodes;
        v = v_net;
        if (n0 + k > D.cap) {
            set_err(D, 1); // pool exhausted: the leaf stays unexpanded, the value is still backed up
        } else {
            const float *pr = prob + (size_t)b * kNMoves;
            if (lane < k) {
                A[CCZ_IDX(D, n0 + lane, D.cap)] = NodeA{0, 0.0f, COMPACT ? cp0 : pr[COMPACT ? 0 : CCZ_IDX(D, id0, kNMoves)], -1};
                Bn[CCZ_IDX(D, n0 + lane, D.cap)] = (uint32_t)id0;
            }
            if (64 + lane < k) {
                A[CCZ_IDX(D, n0 + 64 + lane, D.cap)] = NodeA{0, 0.0f, COMPACT ? cp1 : pr[COMPACT ? 0 : CCZ_IDX(D, id1, kNMoves)], -1};
                Bn[CCZ_IDX(D, n0 + 64 + lane, D.cap)] = (uint32_t)id1;
            }
            if (solver) { // pool slots are reused across moves: the new children are unproven
                uint8_t *proof = sv.proof + base;
                if (lane < k) proof[CCZ_IDX(D, n0 + lane, D.cap)] = 0;
                if (64 + lane < k) proof[CCZ_IDX(D, n0 + 64 + lane, D.cap)] = 0;
            }
            if (spread) { // ... and have received no value
                float *S = spread_array(D) + base;
                if (lane < k) S[CCZ_IDX(D, n0 + lane, D.cap)] = 0.0f;
                if (64 + lane < k) S[CCZ_IDX(D, n0 + 64 + lane, D.cap)] = 0.0f;
            }
            tp.root_expanded = d == 0;
            tp.kid_expanded = d == 1;
            tp.n0 = n0;
            tp.k = k;
            tp.first_id = __builtin_amdgcn_readlane(id0, 0);
            if (lane == 0) {
                const int leaf0 = (int)CCZ_IDX(D, d < 64 ? leaf : path[CCZ_IDX(D, d, D.maxd)], D.cap);
                A[leaf0].fc = n0;
                Bn[leaf0] = (Bn[leaf0] & 0xffffu) | ((uint32_t)k << 16);
                mp->n_nodes = n0 + k;
                BoardStats &st = D.stats[r];
                st.sum_children += (unsigned long long)k;
                st.expansions += 1;
                if (n0 + k > st.nodes_peak) st.nodes_peak = n0 + k;
            }
        }
    } else {
        v = status == CCZ_LEAF_DRAW ? 0.0f : status == CCZ_LEAF_WIN ? 1.0f : -1.0f; // mcts.py:120-126; WIN: a node proven won (solver)
        if (lane == 0) D.stats[r].terminal += 1;
    }
    if (lane == 0) {
        D.stats[r].sims += 1;
        D.move_sims[r] += 1;
        D.leaf_status[b] = CCZ_LEAF_SKIP; // consumed: a repeated call must not back the same leaf up twice
    }
    // Node.update_recursive(-leaf_value) (mcts.py:73-78,129): leaf gets -v, its parent +v, ...
    CCZ_STAMP(D, b, lane, 15)
    int myN = 0;
    float myQ = 0.0f;
    for (int j = lane; j <= d; j += 64) {
        const int node = (int)CCZ_IDX(D, j < 64 ? pj : path[CCZ_IDX(D, j, D.maxd)], D.cap);
        const float val = ((d - j) & 1) ? v : -v;
        const int n = A[node].N + 1;
        const float q = A[node].Q;
        // value spread (wave-uniform; off: nothing is read): the node's S is requested in the round of its N and Q
        float *Sn = nullptr;
        float s_old = 0.0f;
        if (spread) { Sn = spread_array(D) + base + node; s_old = *Sn; }
        // visits += 1 ; value += 1.0*(leaf_value - value)/visits   in float32 (mcts.py:68-71)
        float qn;
        if (D.flags & 4u) {
            // CCZ_FLAG_VALUE_F16: the same expression on a float16 value (reference CUDA path). Every operation is done
            // in float32 and rounded once to float16, which is what NumPy's half loops do (and equals IEEE binary16
            // arithmetic: 24 >= 2*11 + 2); `visits` is a weak Python int, i.e. converted to float16 as well.
            const float vh = (float)(_Float16)val, qh = (float)(_Float16)q;
            float dh = (float)(_Float16)(vh - qh);
            dh = (float)(_Float16)(dh / (float)(_Float16)(float)n);
            qn = (float)(_Float16)(qh + dh);
        } else {
            const float d0 = val - q;
            const float delta = d0 / (float)n;
            qn = q + delta;
            // value spread: S <- S + (val - q) * (val - qn), Welford's sum of squared deviations, float32, no contraction; the node's
            // S is its lane's, like N and Q, and is stored with them (a CCZ_FLAG_VALUE_F16 engine refuses the option)
            if (spread) {
                const float d1 = val - qn;
                const float prod = d0 * d1;
                *Sn = s_old + prod;
            }
        }
        A[node].N = n;
        A[node].Q = qn;
        if (j < 64) { myN = n; myQ = qn; }
    }
    tp.active = true;
    tp.rootN = __builtin_amdgcn_readlane(myN, 0);
    tp.rootQ = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(myQ), 0));
    tp.has1 = d >= 1;
    tp.node1 = __builtin_amdgcn_readlane(pj, 1);
    tp.N1 = __builtin_amdgcn_readlane(myN, 1);
    tp.Q1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(myQ), 1));
    // ---- MCTS-solver: a simulation that ended in a decided position proves what it can of its path (off, or an expansion: nothing)
    if (solver && status != CCZ_LEAF_EXPAND) {
        const uint32_t top = proof_backup(D, sv.proof + base, A, Bn, path, D.sv_stats + r, pj, d, status, leaf, lane);
        tp.hasp1 = (top & 0x100u) != 0u;
        tp.p1 = top & 0xffu;
    }
    return tp;
}

template <bool COMPACT>
__global__ __launch_bounds__(64) void k_expand_backup(Dev D, const float *prob, const float *value)
{
    const BoardMeta m0 = D.meta[blockIdx.x];
    const SolverCfg sv = solver_cfg(D);
    (void)expand_backup_phase<COMPACT>(D, blockIdx.x, blockIdx.x, threadIdx.x, prob, value, m0, *D.half, sv);
}

// ------------------------------------------------------------------ fused step: expand+backup of the pending leaf, then the next select
// Saves one launch boundary and the re-read of the board's tree head per simulation. The phases
// touch the same nodes from different lanes, so a workgroup barrier (one wave) separates them.
template <bool COMPACT>
__global__ __launch_bounds__(64) void k_step(Dev D, const float *prob, const float *value, uint16_t *leaf_in)
{
    __shared__ SelectShared sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    CCZ_STAMP(D, b, lane, 0)
    const Prefetch P = prefetch_board(D, b, lane); // root board, chain and meta: untouched by the expand phase
    const TopPatch tp = expand_backup_phase<COMPACT>(D, b, b, lane, prob, value, P.m, P.half, P.sv);
    CCZ_STAMP(D, b, lane, 1)
    __threadfence_block();
    __syncthreads();
    CCZ_STAMP(D, b, lane, 2)
    select_phase<true>(D, b, lane, leaf_in, sh, P, tp);
    CCZ_STAMP(D, b, lane, 9)
}

// What a cache entry is checked against besides its 64-bit key: the number of legal moves (8 bits) and a 24-bit hash of the
// legal-move LIST in the order the priors are stored in. The list is derived from the position, not from the key: a position that
// collides with another one on all 64 key bits (2^-40 per probe of an occupied slot, i.e. once in days at 2 x 10^5 probes a
// second) would also have to have the same legal moves in the same order to be served the other position's priors; a list that
// differs in any entry passes with probability 2^-24. Residual per probe: < 2^-64.
__device__ __forceinline__ uint32_t cache_tag(int id0, int id1, int k, int lane)
{
    uint64_t h = 0;
    if (lane < k) h ^= mix64(((uint64_t)(uint32_t)id0 << 8 | (uint32_t)lane) + 0x9E3779B97F4A7C15ull);
    if (64 + lane < k) h ^= mix64(((uint64_t)(uint32_t)id1 << 8 | (uint32_t)(64 + lane)) + 0x9E3779B97F4A7C15ull);
    h = wave_readlane64(wave_incl_xor64(h), 63);
    return ((uint32_t)(h >> 40) << 8) | (uint32_t)(k & 0xff);
}

// ------------------------------------------------------------------ compact evaluator boundary: logits -> priors of the legal moves
// exp(log_softmax(logits))[legal ids] (net.py:202-205) for every board in one pass: the wave reads its 2086
// logits once (coalesced), reduces max and sum on the DPP network, and writes only the <= 128 priors the
// expansion will use, aligned with leaf_ids. Replaces two full [B,2086] torch passes (log_softmax, exp) and
// turns the expansion's scattered 4-byte gather (one 64-B line per legal move) into one coalesced 512-B read.
// PLANNED: the evaluator ran on the compact rows of k_cache_plan; board b's logits sit in row row_of[b] of `logits`, its value in
// vcompact[row_of[b]]; cache hits already hold their priors and value (k_cache_probe); a fresh evaluation whose board won the
// slot's claim is stored in the cache.
// `salt` is XORed into the key an entry is stored under (ccz_set_routing: one table, two evaluators; 0 = the plain key).
template <typename T, bool PLANNED>
__device__ __forceinline__ void softmax_gather_board(const Dev &D, int b, int lane, float *row, const T *logits, const float *vcompact,
                                                     uint64_t salt)
{
    // everything the wave needs to know about its board is requested at once (one memory round trip instead of a chain of four:
    // status -> state -> row -> logits); a board that turns out to have nothing to do leaves after it
    const int status = D.leaf_status[b];
    int cst = 0, src = b;
    if (PLANNED) {
        cst = D.cstate[b];
        src = D.row_of[b];
    }
    const int k = D.leaf_k[b];
    const uint16_t *ids = D.leaf_ids + (size_t)b * kMaxLegal;
    const int id0 = ids[lane], id1 = ids[64 + lane];
    if (status != CCZ_LEAF_EXPAND || cst != 0) return; // (cst != 0: a hit -- prior128 / vleaf were filled by the probe)
    const T *srcrow = logits + (size_t)src * kNMoves;
    float mx = -__builtin_huge_valf();
    float sum = 0.0f;
    if constexpr (sizeof(T) == 2) {
        // fp16 logits: a row is 1043 dwords (4-byte aligned: 2086 is even), two logits per load -- half the loads, LDS writes and
        // loop trips of the element-wise form. A lane adds its exponentials in ascending element order (2j, 2j + 1, 2j + 128, ...).
        static_assert(kNMoves % 2 == 0, "dword rows");
        const uint32_t *src32 = (const uint32_t *)srcrow;
        constexpr int kIt = (kNMoves / 2 + 63) / 64;
        uint32_t wreg[kIt]; // the whole row in flight before the first use
#pragma unroll
        for (int i = 0; i < kIt; ++i) {
            const int j = lane + 64 * i;
            wreg[i] = j < kNMoves / 2 ? src32[j] : 0u;
        }
#pragma unroll
        for (int i = 0; i < kIt; ++i) {
            const int j = lane + 64 * i;
            if (j < kNMoves / 2) {
                const uint32_t w = wreg[i];
                const float x0 = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
                const float x1 = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
                *(float2 *)(row + 2 * j) = make_float2(x0, x1);
                mx = fmaxf(mx, fmaxf(x0, x1));
            }
        }
        mx = wave_max_f32(mx);
        for (int j = lane; j < kNMoves / 2; j += 64) {
            const float2 x = *(const float2 *)(row + 2 * j);
            sum += __expf(x.x - mx);
            sum += __expf(x.y - mx);
        }
    } else {
        for (int i = lane; i < kNMoves; i += 64) {
            const float x = (float)srcrow[i];
            row[i] = x;
            mx = fmaxf(mx, x);
        }
        mx = wave_max_f32(mx);
        for (int i = lane; i < kNMoves; i += 64) sum += __expf(row[i] - mx);
    }
    sum = wave_sum_f32(sum);
    wave_sync();
    float *out = D.prior128 + (size_t)b * kMaxLegal;
    const float p0 = lane < k ? __expf(row[id0] - mx) / sum : 0.0f;
    const float p1 = 64 + lane < k ? __expf(row[id1] - mx) / sum : 0.0f;
    if (PLANNED) {
        const float v = vcompact[src];
        if (D.cver[b]) {
            // CCZ_FLAG_CACHE_VERIFY: this leaf HIT the table (the probe left the cached priors / value in prior128 / vleaf) and was
            // sent through the evaluator all the same: the fresh numbers must be the cached ones, bit for bit
            const bool d0 = lane < k && __float_as_uint(out[lane]) != __float_as_uint(p0);
            const bool d1 = 64 + lane < k && __float_as_uint(out[64 + lane]) != __float_as_uint(p1);
            const bool dv = __float_as_uint(D.vleaf[b]) != __float_as_uint(v);
            const bool bad = __ballot(d0 || d1 || dv) != 0ull;
            if (lane == 0) {
                D.stats[b].cache_verified += 1u;
                if (bad) D.stats[b].cache_mismatch += 1u;
            }
        }
        if (lane < k) out[lane] = p0;
        if (64 + lane < k) out[64 + lane] = p1;
        const uint32_t slot = D.cslot[b];
        if (lane == 0) {
            D.vleaf[b] = v;
            D.claim[slot] = 0x7fffffff; // (every board that missed on the slot resets it: idempotent)
        }
        if (D.cins[b]) { // the slot's claim winner stores its evaluation (nobody reads the table before the next launch)
            CacheEntry *e = D.cache + slot;
            const uint32_t tag = cache_tag(id0, id1, k, lane);
            e->pri[lane] = p0;
            e->pri[64 + lane] = p1;
            if (lane == 0) { e->v = v; e->k = tag; e->key = D.leaf_key[b] ^ salt; D.stats[b].cache_stores += 1u; }
        }
    } else {
        if (lane < k) out[lane] = p0;
        if (64 + lane < k) out[64 + lane] = p1;
    }
}

template <typename T, bool PLANNED>
__global__ __launch_bounds__(64) void k_softmax_gather(Dev D, const T *logits, const float *vcompact)
{
    __shared__ __attribute__((aligned(16))) float row[kNMoves + 2];
    softmax_gather_board<T, PLANNED>(D, blockIdx.x, threadIdx.x, row, logits, vcompact, 0ull);
}

// ROUTED (ccz_gather_priors_routed): board b's leaf was planned for evaluator net[b] (k_cache_probe_routed); its logits / value sit
// in that evaluator's compact output, row row_of[b] of its segment, and a fresh evaluation is stored under that evaluator's salt.
template <typename T>
__global__ __launch_bounds__(64) void k_softmax_gather_routed(Dev D, const uint8_t *net, const T *logits0, const T *logits1,
                                                              const float *v0, const float *v1, uint64_t salt0, uint64_t salt1)
{
    __shared__ __attribute__((aligned(16))) float row[kNMoves + 2];
    const int b = blockIdx.x;
    const int n = net[b];
    softmax_gather_board<T, true>(D, b, threadIdx.x, row, n ? logits1 : logits0, n ? v1 : v0, n ? salt1 : salt0);
}

// ------------------------------------------------------------------ evaluation cache: probe, plan
__device__ __forceinline__ uint32_t cache_slot(uint64_t key, uint32_t mask) { return (uint32_t)(key ^ (key >> 29)) & mask; }

// One wave per board: look the pending leaf up. Hit: its priors and value go straight to prior128 / vleaf. Miss: the board
// bids for the slot (lowest board index wins: deterministic) -- the winner's evaluation will be stored there, and boards that
// missed with the SAME key in this step share the winner's evaluator row (k_cache_plan).
// `salt`: XORed into the key before the slot is chosen and the entry compared (ccz_set_routing; 0 = the plain key).
__device__ inline int cache_probe_wave(const Dev &D, int b, int lane, uint64_t salt = 0) // returns the board's plan state (wave-uniform): 0 miss, 1 hit, 2 nothing to evaluate
{
    const int status = D.leaf_status[b];
    const uint64_t key = D.leaf_key[b] ^ salt; // (requested together with the status: one round trip less in front of the table access)
    if (status != CCZ_LEAF_EXPAND) {
        if (lane == 0) D.cstate[b] = 2;
        return 2;
    }
    const uint32_t slot = cache_slot(key, D.cache_mask);
    const CacheEntry *e = D.cache + slot;
    const uint64_t ekey = e->key;
    const uint32_t ek = e->k;
    const float ev = e->v, q0 = e->pri[lane], q1 = e->pri[64 + lane];
    const uint16_t *ids = D.leaf_ids + (size_t)b * kMaxLegal;
    const uint32_t tag = cache_tag(ids[lane], ids[64 + lane], D.leaf_k[b], lane);
    const bool hit = ekey == key && ek == tag;
    if (hit) {
        float *out = D.prior128 + (size_t)b * kMaxLegal;
        out[lane] = q0;
        out[64 + lane] = q1;
    }
    // CCZ_FLAG_CACHE_VERIFY: one hit in 128 (chosen by the key, the board and the board's probe count) is ALSO planned as an evaluator row;
    // k_softmax_gather compares its fresh priors / value with what the table just returned. It does not bid for the slot.
    BoardStats &st = D.stats[b];
    const bool verify = hit && (D.flags & 8u) && (mix64(key + 0x632BE59BD9B4E019ull * (uint64_t)st.cache_probes + 0xD1342543DE82EF95ull * (uint64_t)b) & 127ull) == 0ull;
    if (lane == 0) {
        D.cslot[b] = slot;
        D.ctag[b] = tag;
        D.cstate[b] = hit && !verify ? 1 : 0;
        D.cver[b] = verify ? 1 : 0;
        if (hit) D.vleaf[b] = ev;
        else atomicMin(D.claim + slot, b);
        st.cache_probes += 1u;
        if (hit && !verify) st.cache_hits += 1u;
    }
    return hit && !verify ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_cache_probe(Dev D) { (void)cache_probe_wave(D, blockIdx.x, threadIdx.x); }

// Routed probe (ccz_set_routing): the search on board b belongs to the evaluator that owns the ROOT's side to move -- red_net[b] on
// a red move, the other one on a black move (game.py:77-130 with two MCTS_AI players: the player to move searches with its own
// net, whoever is to move at the leaf). net_out[b] <- that evaluator; the board probes under that evaluator's salted key.
__global__ __launch_bounds__(64) void k_cache_probe_routed(Dev D, const uint8_t *red_net, uint8_t *net_out, uint64_t salt0, uint64_t salt1)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = D.meta[b].turn ? red_net[b] : 1 - red_net[b];
    if (lane == 0) net_out[b] = (uint8_t)n;
    (void)cache_probe_wave(D, b, lane, n ? salt1 : salt0);
}

// One workgroup: representatives and the compaction plan. A miss whose slot was won by a board with the same key uses that
// board's row; every other miss is its own representative (a different key on the same slot is evaluated but not stored).
// miss_rows[0 .. n_miss) = the representatives in ascending board order: the rows the evaluator computes.
// ROUTED (ccz_eval_plan_routed): every board belongs to evaluator net[b] (k_cache_probe_routed) and its key is salted with that
// evaluator's salt; a row is shared only between boards of the same evaluator, and the representatives are compacted into one
// segment per evaluator: evaluator 0 at miss_rows[0 .. n_miss[0]), evaluator 1 at miss_rows[B .. B + n_miss[1]); row_of[b] is the
// row within the board's own segment.
template <bool ROUTED>
__device__ __forceinline__ void cache_plan_block(const Dev &D, int32_t *miss_rows, int32_t *n_miss, const uint8_t *net, uint64_t salt0,
                                                 uint64_t salt1, int (&s_wave)[2][16], int (&s_base)[2])
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_base[0] = s_base[1] = 0;
    __syncthreads();
    // 4096 boards per pass: a thread looks after boards b0 + tid + 1024 i, i = 0..3. The three dependent load rounds (state / slot /
    // key -> claim -> the claimant's state and key) are issued for all four boards before any is used, so a pass costs three memory
    // round trips instead of twelve (this kernel is one workgroup: nothing else hides its latency)
    for (int b0 = 0; b0 < D.B; b0 += 4096) {
        int st[4], w[4], rep[4], nt[4];
        uint32_t slot[4], tag[4];
        uint64_t key[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + i * 1024 + tid;
            st[i] = 3;
            slot[i] = 0;
            tag[i] = 0;
            key[i] = 0;
            nt[i] = 0;
            if (b < D.B) {
                st[i] = D.cstate[b]; slot[i] = D.cslot[b]; key[i] = D.leaf_key[b]; tag[i] = D.ctag[b];
                if (ROUTED) nt[i] = net[b];
            }
            if (ROUTED) key[i] ^= nt[i] ? salt1 : salt0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = st[i] == 0 ? D.claim[slot[i]] : -1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + i * 1024 + tid;
            rep[i] = b;
            // (w < b: a bidder's claim winner is never above it; a CACHE_VERIFY board did not bid, and must not take the row of a
            // higher board -- possibly of a later pass, not assigned yet -- on a full 64-bit key collision)
            if (st[i] == 0 && w[i] >= 0 && w[i] < b) {
                // the same position = the same 64-bit key AND the same legal-move list (count + 24-bit hash of the list in prior order):
                // what a table hit is checked against (k_cache_probe), now also between two leaves of one step (round 6)
                bool same = D.cstate[w[i]] == 0 && D.ctag[w[i]] == tag[i];
                if (ROUTED) {   // (the claim winner of a slot may be the other evaluator's board: never share its row)
                    const int nw = net[w[i]];
                    same = same && nw == nt[i] && (D.leaf_key[w[i]] ^ (nw ? salt1 : salt0)) == key[i];
                } else {
                    same = same && D.leaf_key[w[i]] == key[i];
                }
                rep[i] = same ? w[i] : b;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + i * 1024 + tid;
            int isrep = 0;
            if (st[i] == 0) {
                D.crep[b] = rep[i];
                D.cins[b] = (uint8_t)(w[i] == b);
                isrep = rep[i] == b;
                if (!isrep) D.stats[b].cache_shared += 1u;
            }
            // exclusive position of every representative in its segment: ballot inside the wave, 16 wave totals through LDS
            const uint64_t m0 = __ballot(isrep && nt[i] == 0);
            const uint64_t m1 = ROUTED ? __ballot(isrep && nt[i] == 1) : 0ull;
            const int in_wave = __popcll((nt[i] ? m1 : m0) & lanemask_lt(lane));
            if (lane == 0) {
                s_wave[0][wv] = __popcll(m0);
                if (ROUTED) s_wave[1][wv] = __popcll(m1);
            }
            __syncthreads();
            int before = 0, total0 = 0, total1 = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int t0 = s_wave[0][j], t1 = ROUTED ? s_wave[1][j] : 0;
                before += j < wv ? (nt[i] ? t1 : t0) : 0;
                total0 += t0;
                total1 += t1;
            }
            const int base0 = s_base[0], base1 = ROUTED ? s_base[1] : 0;
            if (isrep) {
                const int pos = (nt[i] ? base1 : base0) + before + in_wave;
                D.row_of[b] = pos;
                miss_rows[(nt[i] ? D.B : 0) + pos] = b;
            }
            __syncthreads();
            if (tid == 0) {
                s_base[0] = base0 + total0;
                if (ROUTED) s_base[1] = base1 + total1;
            }
            __syncthreads();
        }
        // boards that use another board's row: the representative is the slot's claim winner, i.e. a LOWER board index -- its row
        // was assigned above, in this pass or an earlier one (straight from the registers of this pass: one load round)
        __threadfence_block();
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + i * 1024 + tid;
            if (st[i] == 0 && rep[i] != b) // (read past this CU's L1: the row was written a moment ago by another wave)
                D.row_of[b] = __hip_atomic_load(D.row_of + rep[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (tid == 0) {
        n_miss[0] = s_base[0];
        if (ROUTED) n_miss[1] = s_base[1];
    }
}

__global__ __launch_bounds__(1024) void k_cache_plan(Dev D, int32_t *miss_rows, int32_t *n_miss)
{
    __shared__ int s_wave[2][16];
    __shared__ int s_base[2];
    cache_plan_block<false>(D, miss_rows, n_miss, nullptr, 0ull, 0ull, s_wave, s_base);
}

__global__ __launch_bounds__(1024) void k_cache_plan_routed(Dev D, int32_t *miss_rows, int32_t *n_miss, const uint8_t *net, uint64_t salt0,
                                                            uint64_t salt1)
{
    __shared__ int s_wave[2][16];
    __shared__ int s_base[2];
    cache_plan_block<true>(D, miss_rows, n_miss, net, salt0, salt1, s_wave, s_base);
}

// The plan of a step with scouts (ccz_eval_plan_scouted): the evaluator runs -- on ALL slots, row b = slot b, a fixed small batch --
// only when a board that is really searched misses; the scouts of a board that hit (or whose leaf needs no evaluation) are dropped
// for this step: their next siblings are asked for again when the board next misses. No row sharing here (a duplicate position
// costs a row of a batch that is latency-bound anyway). state_out[r] = cstate of real board r (0 = its leaf needs the evaluator).
__device__ inline void plan_scouted_block(const Dev &D, int active, int32_t *miss_rows, int32_t *n_miss, int32_t *state_out, int tid, int nt, int &s_any)
{
    if (tid == 0) s_any = 0;
    __syncthreads();
    for (int b = tid; b < D.B; b += nt) {
        const int st = D.cstate[b];
        if (b < active) {
            if (st == 0) atomicOr(&s_any, 1);
            if (state_out) state_out[b] = st;
        }
    }
    __syncthreads();
    for (int b = tid; b < D.B; b += nt) {
        const int st = D.cstate[b];
        const uint32_t slot = D.cslot[b];
        const int r = b < active ? b : (b - active) % active;
        const bool keep = st == 0 && (b < active || D.cstate[r] == 0);
        if (st == 0) {
            const int w = D.claim[slot];
            if (!keep) {
                if (w == b) D.claim[slot] = 0x7fffffff; // a dropped scout that won its slot gives it back (nobody stores there this step)
            } else {
                D.crep[b] = b;
                D.row_of[b] = b;
                D.cins[b] = (uint8_t)(w == b);
            }
        }
        miss_rows[b] = b;
    }
    __syncthreads();
    // (second pass: cstate of the scouts is rewritten only after every thread has read what it needed of it)
    for (int b = active + tid; b < D.B; b += nt) {
        const int r = (b - active) % active;
        if (D.cstate[b] == 0 && D.cstate[r] != 0) D.cstate[b] = 2;
    }
    if (tid == 0) *n_miss = s_any ? D.B : 0;
}

__global__ __launch_bounds__(256) void k_cache_plan_scouted(Dev D, int active, int32_t *miss_rows, int32_t *n_miss, int32_t *state_out)
{
    __shared__ int s_any;
    plan_scouted_block(D, active, miss_rows, n_miss, state_out, threadIdx.x, 256, s_any);
}

// scout + probe + plan of an engine of up to 16 slots as ONE workgroup (one wave per slot): what a scouted simulation launches behind
// ccz_step_compact -- two launches per simulation instead of four (the step is a chain of small launches: every one costs ~5 us)
constexpr int kScoutFusedMax = 16;
__global__ __launch_bounds__(1024) void k_scout_probe_plan(Dev D, uint16_t *leaf_in, int active, int32_t *miss_rows, int32_t *n_miss, int32_t *state_out)
{
    __shared__ SelectShared sh[kScoutFusedMax];
    __shared__ int s_any;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (w >= active && w < D.B) scout_wave(D, leaf_in, active, w - active, lane, sh[w]);
    __threadfence_block();      // the scout's leaf slots (global memory, written by this wave) are read back by its own probe
    if (w < D.B) (void)cache_probe_wave(D, w, lane);
    __threadfence();            // cstate / cslot / claim of every slot are read by other waves of this workgroup in the plan
    __syncthreads();
    plan_scouted_block(D, active, miss_rows, n_miss, state_out, tid, (int)blockDim.x, s_any);
}

// Simulations of a scouted engine WITHOUT the host in between (ccz_scouted_run): what the host loop launches per simulation -- the
// fused step (expand + backup of the pending leaf, next selection) and scout + probe + plan -- repeated by ONE workgroup (one wave per
// slot, <= 16 slots) for as long as every searched board finds its next leaf in the table. A simulation that hits costs the
// latency chains of its phases instead of two launches, a graph replay and a stream synchronisation (~46 us,
// profiles/r06_single_board.json); the host comes back only when the evaluator has to run, when `budget` simulations are done (a
// caller that reports progress) or when the move's last simulation -- which has no next selection -- is backed up.
//   * the scouts of a board that hit are dropped by the plan (plan_scouted_block), so while the searched boards hit, the scout waves
//     do nothing at all: a searched board's wave expands, backs up, selects and probes ITS leaf; the scouts are handed their leaves
//     only once, for the step that leaves the loop with a miss -- and what that step's plan leaves behind is what k_scout_probe_plan
//     would have left (a dropped scout gives back the slot it claimed: the same table state as never having claimed it).
//   * run[0] = budget (>= 1), run[1] = simulations left in this move including the pending one (>= 1); run[2] <- simulations done
//     here, run[3] <- 1 if a searched board's leaf needs the evaluator now.
// Same phases, same order, same device functions as the separate launches; all hand-offs between waves stay inside the workgroup
// (one CU, one L1): workgroup-scope fences and barriers, as in k_step and k_scout_probe_plan.
template <int MAXW> // 12: engines of up to 12 slots (168 registers per lane: no spills; the default 1 + 10 scouts), 16: up to 16
__global__ __launch_bounds__(64 * MAXW) void k_scouted_run(Dev D, uint16_t *leaf_in, int active, int32_t *miss_rows, int32_t *n_miss, int32_t *state_out,
                                                        int32_t *run)
{
    __shared__ SelectShared sh[MAXW];
    __shared__ int s_any, s_state[MAXW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool real = w < active;
    int budget = __hip_atomic_load(run + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    int left = __hip_atomic_load(run + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    budget = budget < 1 ? 1 : (budget > (1 << 20) ? (1 << 20) : budget); // whatever the caller left in the run block, the loop ends
    int done = 0, need = 0;
    for (;;) {
        Prefetch P;
        TopPatch tp;
        if (real) {
            P = prefetch_board(D, w, lane);
            tp = expand_backup_phase<true>(D, w, w, lane, D.prior128, nullptr, P.m, P.half, P.sv);
            __threadfence_block();      // (k_step: the phases touch the same nodes from different lanes of the wave)
            __builtin_amdgcn_wave_barrier();
        }
        ++done;
        if (--left <= 0) break;         // the move's last simulation: nothing is selected behind it (ccz_expand_backup_compact)
        if (real) {
            select_phase<false>(D, w, lane, leaf_in, sh[w], P, tp);
            __threadfence_block();      // the leaf (global memory, written by this wave) is read back by its own probe
            const int st = cache_probe_wave(D, w, lane);
            if (lane == 0) s_state[w] = st;
        }
        __threadfence_block();          // the searched boards' leaves, paths, statuses and probe results: read by every wave from here on
        __syncthreads();
        need = 0;
        for (int r = 0; r < active; ++r) need |= s_state[r] == 0 ? 1 : 0;
        if (need || done >= budget) break;
        __syncthreads();                // (s_state is rewritten by the next pass)
    }
    if (left > 0) {
        // the plan of the step that leaves the loop. A miss: the scouts get their leaves and probe, then the plan of all slots; no
        // miss (budget used): the searched boards' states, no evaluator call -- plan_scouted_block with every scout dropped
        if (need) {
            if (!real) {
                scout_wave(D, leaf_in, active, w - active, lane, sh[w]);
                __threadfence_block();
                (void)cache_probe_wave(D, w, lane);
            }
            __threadfence_block();      // cstate / cslot / claim of every slot are read by other waves of this workgroup in the plan
            __syncthreads();
            plan_scouted_block(D, active, miss_rows, n_miss, state_out, tid, (int)blockDim.x, s_any);
        } else {
            if (tid < active) state_out[tid] = s_state[tid];
            if (tid == 0) *n_miss = 0;
        }
    }
    if (tid == 0) {
        run[2] = done;
        run[3] = need;
    }
}

// ------------------------------------------------------------------ pi from root visits (mcts.py:162-166)
// s_vis[k] -> s_pi[k] ; softmax(1/temp * log(N + 1e-10)) with the deterministic log/exp; the
// normalising sum is accumulated sequentially (index order) to match the CPU twin bit for bit.
__device__ __forceinline__ void root_pi(const int32_t *s_vis, double *s_pi, int k, double temp, int lane)
{
    const double it = 1.0 / temp;
    double mx = -__builtin_huge_val();
    for (int i = lane; i < k; i += 64) {
        const double x = it * det_log((double)s_vis[i] + 1e-10);
        s_pi[i] = x;
        if (x > mx) mx = x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(mx, o); if (t > mx) mx = t; }
    for (int i = lane; i < k; i += 64) s_pi[i] = det_exp(s_pi[i] - mx);
    wave_sync();
    double sum = 0.0;
    if (lane == 0) for (int i = 0; i < k; ++i) sum += s_pi[i];
    sum = __shfl(sum, 0);
    wave_sync();
    for (int i = lane; i < k; i += 64) s_pi[i] = s_pi[i] / sum;
    wave_sync();
}

// move ~ Categorical((1-EPS)*pi + EPS*Dirichlet(ALPHA)) on the board's Philox stream (mcts.py:216-224), s_pi[k] -> *choice
// (lane 0). s_g[k] is scratch (the Gamma draws, then the cdf). k_finish_move passes null outputs; k_move_distribution passes
// g_out / mixed_out (float64 [k]) and u_out to read what the sampler drew -- the same instructions, written out on lane 0.
__device__ __forceinline__ void sample_move(const Dev &D, uint64_t gid, uint64_t move_no, const double *s_pi, double *s_g, int k,
                                            int lane, int *choice, double *g_out, double *mixed_out, double *u_out, bool mix = true)
{
    // mix == false (a move searched with root exploration: the noise has acted in the search): the move is drawn from pi itself on the
    // same choice word; the Gamma draws are made only for a caller that reads them
    if (mix || g_out) for (int i = lane; i < k; i += 64) s_g[i] = det_gamma(D.seed, gid, move_no, (uint32_t)i, D.alpha);
    __syncthreads();
    if (lane == 0) {
        double gs = 0.0, acc = 0.0, ua, ub;
        if (mix) for (int i = 0; i < k; ++i) gs += s_g[i];
        for (int i = 0; i < k; ++i) {
            const double dir = gs > 0.0 ? s_g[i] / gs : s_pi[i];
            const double mx = mix ? (1.0 - D.eps) * s_pi[i] + D.eps * dir : s_pi[i];
            if (g_out) g_out[i] = s_g[i];
            if (mixed_out) mixed_out[i] = mx;
            acc += mx;
            s_g[i] = acc; // cdf
        }
        uniform2(D.seed, gid, move_no, 0xfffu, 0, ua, ub);
        if (u_out) *u_out = ua;
        int idx = 0;
        for (int i = 0; i < k; ++i) if (s_g[i] / acc <= ua) idx = i + 1; // searchsorted(side="right")
        *choice = idx < k ? idx : k - 1;
    }
}

// Policy target pruning of a move searched with root exploration (ccz_set_root_exploration, include/cczero.h): s_vis[k] -> s_vp[k],
// the visit counts pi is formed from. c* = the most visited child (lowest index on ties) keeps its count; every other visited child
// gives back the visits PUCT would not have made without its forced playouts: at most nf_i = ceil(sqrt(forced_k P'_i S)) of them, and
// no more than bring its score Q_i + E_i / (1 + N') up to c*'s; what would be left with at most one visit is dropped. All float64.
// s_q / s_pn [128] and s_g [128] are LDS scratch. All 64 lanes call it; count: the board's counters are updated (k_finish_move).
__device__ inline void explore_targets(const Dev &D, const ExploreCfg &xc, int b, int lane, int k, uint32_t move_counter, const NodeA &root,
                                       const NodeA *kids, const int32_t *s_vis, int32_t *s_vp, float *s_q, float *s_pn, double *s_g, bool count)
{
    float xd0, xd1;
    explore_dir(D, xc, b, lane, k, move_counter, kids, s_g, xd0, xd1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = 64 * h + lane;
        if (i < k) {
            const NodeA c = kids[CCZ_IDX(D, i, D.cap)];
            s_q[i] = c.Q;
            s_pn[i] = explore_prior(xc, c.P, h ? xd1 : xd0);
            s_vp[i] = s_vis[i];
        }
    }
    __syncthreads();
    int vp = 0, cp = 0;
    if (xc.prune) {
        int cs = 0; // every lane runs the same <= 128 terms on the same LDS words: wave-uniform without a broadcast
        for (int i = 1; i < k; ++i) if (s_vis[i] > s_vis[cs]) cs = i;
        const double sq = sqrt((double)root.N), S = (double)(root.N - 1);
        const float ce = search_c_eff(D.c_puct, *D.sr_cfg, root.N); // (ccz_set_search off, or c_factor 0: c_puct as it is)
        const double top = (double)s_q[cs] + (double)(ce * s_pn[cs]) * sq / (double)(1 + s_vis[cs]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = 64 * h + lane;
            if (i < k && i != cs && s_vis[i] > 0) {
                const int n = s_vis[i];
                const double E = (double)(ce * s_pn[i]) * sq;
                const double nf = ceil(sqrt(xc.forced_k * (double)s_pn[i] * S));
                const double gap = top - (double)s_q[i];
                double need = (double)n;
                if (gap > 0.0) { const double t = ceil(E / gap - 1.0); need = t > 0.0 ? t : 0.0; }
                double keep = (double)n - nf;
                keep = keep > need ? keep : need;
                int np = keep >= (double)n ? n : (keep > 0.0 ? (int)keep : 0);
                if (np < n && np <= 1) np = 0;
                s_vp[i] = np;
                vp += n - np;
                cp += np == 0 ? 1 : 0;
            }
        }
    }
    if (count) {
        vp = __builtin_amdgcn_readlane(wave_incl_scan(vp, lane), 63);
        cp = __builtin_amdgcn_readlane(wave_incl_scan(cp, lane), 63);
        if (lane == 0) {
            ExploreBoardStats &xs = D.ex_stats[b];
            xs.explored += 1;
            xs.visits_pruned += (unsigned long long)vp;
            xs.children_pruned += (unsigned long long)cp;
        }
    }
    __syncthreads();
}

// a per-board temperature the softmax of root_pi cannot take (1/temp of 0 or NaN): CCZ_ERR_BAD_TEMP, the board neither records nor moves
__device__ __forceinline__ bool bad_temp(double t) { return !(t > 0.0); }

__device__ __forceinline__ double board_temp(const Dev &D, const BoardMeta &m, const double *temps, int b)
{
    if (temps) return temps[b];
    // game.py:157-159: move_count = ply+1 ; temp if move_count <= 30 else max(0.1, temp*0.5)
    const double half = D.temp * 0.5;
    return (m.ply + 1) <= 30 ? D.temp : (half > 0.1 ? half : 0.1);
}

// ------------------------------------------------------------------ the move boundary: phases with one definition each
// What k_root_children, k_move_distribution, k_finish_move and k_set_positions are made of. Every phase
// works on the calling kernel's LDS arrays (it declares none), is called by all 64 lanes and returns wave-uniform results by value.
// the board's tree in the current pool half: node arrays and root record. The child count as stored is root_k(); what a count above
// kMaxLegal means is the caller's policy (k_root_children clamps, k_move_distribution reports nothing, k_finish_move raises error 16).
struct RootView { const NodeA *A; const uint32_t *Bn; NodeA root; int half; };

__device__ __forceinline__ RootView root_view(const Dev &D, int b)
{
    const int half = *D.half;
    const size_t base = ((size_t)b * 2 + half) * (size_t)D.cap;
    return RootView{D.nodeA + base, D.nodeB + base, D.nodeA[base], half};
}
__device__ __forceinline__ int root_k(const RootView &rv) { return (int)(rv.Bn[0] >> 16); }

// What the policy target and the drawn move are formed from: s_vis[k] (the counts as searched) -> s_pi[k]. A policy-target move
// searched with root exploration (ccz_set_root_exploration; off: one word read) takes pi from the pruned counts s_vp and is drawn
// from it without Dirichlet mixing: that is the `explored` returned, and the caller's sample_move gets mix = !explored. count: the
// board's exploration counters move (k_finish_move) or not (k_move_distribution). s_q / s_pn / s_g: scratch of explore_targets.
__device__ __forceinline__ bool move_target_pi(const Dev &D, int b, int lane, const RootView &rv, int k, uint32_t move_counter, int target,
                                               double temp, const int32_t *s_vis, int32_t *s_vp, float *s_q, float *s_pn, double *s_g,
                                               double *s_pi, bool count)
{
    const ExploreCfg xc = *D.ex_cfg;
    const bool explored = xc.enabled && target && k > 0;
    if (explored) explore_targets(D, xc, b, lane, k, move_counter, rv.root, rv.A + rv.root.fc, s_vis, s_vp, s_q, s_pn, s_g, count);
    if (k > 0) root_pi(explored ? s_vp : s_vis, s_pi, k, temp, lane);
    return explored;
}

// The move boundary of a board searched with the Gumbel root rule (ccz_set_gumbel): s_pi[k] = pi' = softmax(logit + sigma) with the
// deterministic exp, the sum in child order on lane 0; returns the child the rule plays: the first maximum of g + logit + sigma among
// the children of most move-visits (wave-uniform). played: the forced move's child, or -1. count: the board's counters move
// (k_finish_move) or not (k_move_distribution). s_w [128] doubles / s_p [128] floats: LDS scratch.
__device__ inline int gumbel_targets(const Dev &D, const GumbelCfg &gc, int b, int lane, int k, uint32_t move_counter, const RootView &rv,
                                     double *s_w, float *s_p, double *s_pi, int played, bool count)
{
    NodeA c[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) c[h] = 64 * h + lane < k ? rv.A[CCZ_IDX(D, rv.root.fc + 64 * h + lane, D.cap)] : NodeA{0, 0.0f, 0.0f, -1};
    const GumbelRow r = gumbel_row(D, gc, b, lane, k, move_counter, c, 0, D.budget[b], false);
    double sig[2];
    gumbel_sigma(gc, lane, k, c, rv.root.Q, s_w, s_p, sig);
    const bool in0 = lane < k, in1 = 64 + lane < k;
    const double ninf = -__builtin_huge_val();
    const double l0 = r.logit[0] + sig[0], l1 = r.logit[1] + sig[1];
    const double a0 = (in0 && l0 == l0) ? l0 : ninf, a1 = (in1 && l1 == l1) ? l1 : ninf;
    const double mx = wave_max_f64(a0 > a1 ? a0 : a1);
    if (in0) s_pi[lane] = det_exp(l0 - mx);
    if (in1) s_pi[64 + lane] = det_exp(l1 - mx);
    wave_sync();
    double sum = 0.0;
    if (lane == 0) for (int i = 0; i < k; ++i) sum += s_pi[i];
    sum = __shfl(sum, 0);
    wave_sync();
    if (in0) s_pi[lane] = s_pi[lane] / sum;
    if (in1) s_pi[64 + lane] = s_pi[64 + lane] / sum;
    wave_sync();
    const int M0 = c[0].N - r.n0[0], M1 = c[1].N - r.n0[1];
    const int b0 = in0 ? M0 : (int)0x80000000, b1 = in1 ? M1 : (int)0x80000000;
    const int mm = wave_max_i32(b0 > b1 ? b0 : b1);
    int choice = gumbel_first_max(r.g[0] + r.logit[0] + sig[0], in0 && M0 == mm, r.g[1] + r.logit[1] + sig[1], in1 && M1 == mm, lane);
    if (choice < 0) { set_err(D, 32); choice = 0; } // NaN priors: no comparable child
    if (count) {
        const int most = gumbel_first_max((double)c[0].N, in0, (double)c[1].N, in1, lane);
        if (lane == 0) {
            GumbelBoardStats &gs = D.gm_stats[b];
            gs.moves += 1;
            gs.considered += (unsigned long long)r.m;
            gs.offvisit += (played >= 0 ? played : choice) != most ? 1 : 0;
        }
    }
    return choice;
}

__global__ __launch_bounds__(64) void k_root_children(Dev D, int32_t *k_out, uint16_t *acts, int32_t *visits,
                                                        float *q, float *prior, int32_t *root_visits,
                                                        const double *temps, double *pi_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    __shared__ int32_t s_vis[kMaxLegal];
    __shared__ double s_pi[kMaxLegal];
    const BoardMeta m = D.meta[b];
    const RootView rv = root_view(D, b);
    int k = root_k(rv) > kMaxLegal ? kMaxLegal : root_k(rv);
    if (lane == 0) {
        if (k_out) k_out[b] = k;
        if (root_visits) root_visits[b] = rv.root.N;
    }
    for (int i = lane; i < kMaxLegal; i += 64) {
        NodeA c = NodeA{0, 0.0f, 0.0f, -1};
        uint32_t w = 0;
        if (i < k) { c = rv.A[rv.root.fc + i]; w = rv.Bn[rv.root.fc + i]; }
        s_vis[i] = c.N;
        const size_t o = (size_t)b * kMaxLegal + i;
        if (acts) acts[o] = (uint16_t)(w & 0xffffu);
        if (visits) visits[o] = c.N;
        if (q) q[o] = c.Q;
        if (prior) prior[o] = c.P;
    }
    __syncthreads();
    if (pi_out) {
        const double temp = board_temp(D, m, temps, b);
        if (bad_temp(temp)) { if (lane == 0) set_err(D, CCZ_ERR_BAD_TEMP); k = 0; }
        if (k > 0) root_pi(s_vis, s_pi, k, temp, lane);
        for (int i = lane; i < kMaxLegal; i += 64) pi_out[(size_t)b * kMaxLegal + i] = i < k ? s_pi[i] : 0.0;
    }
}

// ------------------------------------------------------------------ what the next unforced k_finish_move samples from
// Read-only (moves nothing, records nothing): move_target_pi and sample_move as k_finish_move calls them, on the same Philox counters.
// g_out / mixed_out float64 [B][128] (the raw Gamma draws, (1-eps) pi + eps Dirichlet; a move searched with root exploration: the
// draws as they would have been, mixed == pi of the pruned counts), u_out float64 [B] (the choice uniform).
// A board k_finish_move would not sample on (game over, no children, bad temperature) gets zero rows and u = NaN.
__global__ __launch_bounds__(64) void k_move_distribution(Dev D, const double *temps, double *g_out, double *mixed_out, double *u_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    __shared__ int32_t s_vis[kMaxLegal];
    __shared__ double s_pi[kMaxLegal];
    __shared__ double s_g[kMaxLegal];
    __shared__ int32_t s_vp[kMaxLegal];
    __shared__ float s_q[kMaxLegal], s_pn[kMaxLegal];
    __shared__ int s_choice;
    const BoardMeta m = D.meta[b];
    const RootView rv = root_view(D, b);
    int k = root_k(rv);
    const double temp = board_temp(D, m, temps, b);
    if (m.over || k > kMaxLegal || bad_temp(temp)) k = 0;
    double *g = g_out + (size_t)b * kMaxLegal, *mixed = mixed_out + (size_t)b * kMaxLegal;
    for (int i = lane; i < kMaxLegal; i += 64) if (i >= k) { g[i] = 0.0; mixed[i] = 0.0; }
    if (k == 0) { if (lane == 0) u_out[b] = __builtin_nan(""); return; }
    for (int i = lane; i < k; i += 64) s_vis[i] = rv.A[CCZ_IDX(D, rv.root.fc + i, D.cap)].N;
    __syncthreads();
    const GumbelCfg gc = *D.gm_cfg;
    if (gc.enabled) { // a Gumbel board draws nothing: mixed = pi', no Gamma draws, no choice uniform
        (void)gumbel_targets(D, gc, b, lane, k, m.move_counter, rv, s_g, s_pn, s_pi, -1, false);
        for (int i = lane; i < k; i += 64) { g[i] = 0.0; mixed[i] = s_pi[i]; }
        if (lane == 0) u_out[b] = __builtin_nan("");
        return;
    }
    const bool explored = move_target_pi(D, b, lane, rv, k, m.move_counter, D.target[b], temp, s_vis, s_vp, s_q, s_pn, s_g, s_pi, false);
    sample_move(D, D.board_id_base + (uint64_t)b, m.move_counter, s_pi, s_g, k, lane, &s_choice, g, mixed, u_out + b, !explored);
}

// CCZ_RULE_PERPETUAL_CHECK: the game ends by fourfold repetition; inside the repetition window --
// the positions after the earliest occurrence of the repeated position -- a side whose EVERY move gave check while the
// other side's did not loses. Only outcome().winner changes (game.py:210-216): in the search the same leaf is
// "end and is_tie" -> 0.0 either way (mcts.py:120-122), so visit counts do not depend on this flag.
// Returns the winner (1 RED / 0 BLACK) or -1. `turn` = the side to move in the position the chain ends with, chk0 / chk1 = the
// chain's in-check bits including that position's. Called by root_game_end. All 64 lanes call it.
__device__ __forceinline__ int perpetual_check_winner(uint32_t rule_flags, const LeafEval &L, int halfmove, int chain_len, uint64_t chk0,
                                                      uint64_t chk1, int turn, int lane)
{
    int perpetual_winner = -1;
    // (the host view and the reference order of checks, game.py:208-214: insufficient material, then the sixty-move rule, then the
    // repetition -- a game that the sixty-move rule ends at the same ply is a DRAW, whatever the repetition window holds)
    if ((rule_flags & 1u) && L.n_legal > 0 && !L.insufficient && !(halfmove >= 120) && L.rep >= 4) {
        const int last = chain_len - 1;
        bool miss_mover = false, miss_other = false, any_other = false; // mover = the side that just moved (turn ^ 1)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = h * 64 + lane;
            const bool in = i > L.first_occ && i <= last;
            const bool bit = ((h ? chk1 : chk0) >> lane) & 1ull;
            const bool by_mover = ((last - i) & 1) == 0;
            miss_mover |= __ballot(in && by_mover && !bit) != 0ull;
            miss_other |= __ballot(in && !by_mover && !bit) != 0ull;
            any_other |= __ballot(in && !by_mover) != 0ull;
        }
        const bool mover_all = !miss_mover, other_all = any_other && !miss_other;
        if (mover_all && !other_all) perpetual_winner = turn;          // the side that kept checking loses
        else if (other_all && !mover_all) perpetual_winner = turn ^ 1;
    }
    return perpetual_winner;
}

// ------------------------------------------------------------------ a move on the root (k_finish_move, k_set_positions)
// What it changes besides the squares: key, side to move, sixty-move clock, length of the history chain (the keys
// since the last zeroing move: s_chain) and the chain's in-check bits: the side to move stands in check at that chain position.
struct RootState { uint64_t key; int turn, halfmove, chain_len; uint64_t chk0, chk1; };

// board.push(move) on the root (game.py:201) and its history: squares, key, clock, and the chain -- restarted, with its check bits,
// by a zeroing move --, then the new key appended. True: the chain was full, its last key is overwritten and the caller reports it
// (k_finish_move: sticky bit 64, k_set_positions: status -2). sync(): the caller's own barrier, before and after lane 0's writes.
template <typename Sync>
__device__ __forceinline__ bool push_root_move(const Dev &D, int mv, uint8_t *s_sq, uint64_t *s_chain, RootState &st, int lane, Sync sync)
{
    const int from = c_tab.from[mv], to = c_tab.to[mv];
    const int pc = s_sq[from], cap = s_sq[to];
    sync();
    if (lane == 0) { s_sq[to] = (uint8_t)pc; s_sq[from] = 0; }
    st.key ^= zob(pc, from) ^ zob(pc, to) ^ kTurnKey;
    if (cap) st.key ^= zob(cap, to);
    st.turn ^= 1;
    const bool zeroing = cap || ((D.rule_flags & 2u) && (pc & 7) == PAWN); // CCZ_RULE_PAWN_MOVE_RESETS_CLOCK
    st.halfmove = zeroing ? 0 : st.halfmove + 1;
    if (zeroing) { st.chain_len = 0; st.chk0 = 0ull; st.chk1 = 0ull; }
    const bool full = st.chain_len >= kChainCap;
    if (full) st.chain_len = kChainCap - 1;
    if (lane == 0) s_chain[CCZ_IDX(D, st.chain_len, kChainCap)] = st.key;
    ++st.chain_len;
    sync();
    return full;
}

// the in-check bit of the chain's last position (st.turn to move there, its king on ksq)
__device__ __forceinline__ void mark_check(const uint8_t *s_sq, GenScratch &S, int ksq, RootState &st)
{
    const bool in_check = ksq >= 0 && king_attacked(s_sq, S, ksq, -1, -1, 0, st.turn);
    const int ci = st.chain_len - 1;
    if (in_check) { if (ci < 64) st.chk0 |= 1ull << ci; else st.chk1 |= 1ull << (ci - 64); }
}

// game end (game.py:208-219) of the position a push reached: is_game_over() or is_tie(); winner from outcome() (1 RED / 0 BLACK /
// -1: a draw, or not over); overflow: the move generator's lists overflowed. Marks the position's check bit in st.
struct GameEnd { bool over; int winner; bool overflow; };
__device__ __forceinline__ GameEnd root_game_end(uint32_t rule_flags, const uint8_t *s_sq, const uint64_t *s_chain, GenScratch &S, RootState &st, int lane)
{
    GameEnd e;
    const LeafEval L = eval_position(s_sq, st.turn, st.halfmove, st.key, s_chain, st.chain_len, S, nullptr, lane, e.overflow);
    mark_check(s_sq, S, L.ksq, st);
    const int pw = perpetual_check_winner(rule_flags, L, st.halfmove, st.chain_len, st.chk0, st.chk1, st.turn, lane);
    e.over = L.status != CCZ_LEAF_EXPAND;
    e.winner = !e.over ? -1 : L.n_legal == 0 ? (st.turn ^ 1) : pw; // no legal move: side to move loses
    return e;
}

// ------------------------------------------------------------------ K3: once per move
__global__ __launch_bounds__(64) void k_finish_move(Dev D, const int32_t *forced, const double *temps,
                                                      int32_t *moves_out, int keep_tree)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    __shared__ __align__(16) uint8_t s_sq[96];
    __shared__ uint64_t s_chain[kChainCap];
    __shared__ GenScratch S;
    __shared__ int32_t s_vis[kMaxLegal];
    __shared__ uint16_t s_act[kMaxLegal];
    __shared__ double s_pi[kMaxLegal];
    __shared__ double s_g[kMaxLegal];
    __shared__ int32_t s_src[64], s_dst[64], s_cnt[64];
    __shared__ int32_t s_vp[kMaxLegal];
    __shared__ float s_q[kMaxLegal], s_pn[kMaxLegal];
    __shared__ int s_choice;

    // ---- guards
    BoardMeta m = D.meta[b];
    if (moves_out && lane == 0) moves_out[b] = -1;
    if (m.over) return;
    if (lane == 0) { // a move boundary for every live board, whether or not it moves below
        D.move_sims[b] = 0;
        D.es_stopped[b] = 0; // (early stop, S5)
        D.es_snap_s[b] = -1;
    }
    const RootView rv = root_view(D, b);
    const int k = root_k(rv), nh = rv.half ^ 1; // every board moves to the other pool half (the host flips the word afterwards)
    const size_t baseNew = ((size_t)b * 2 + nh) * (size_t)D.cap;
    // MCTS-solver (off: this one word read): a kept node's proof byte moves with its records; a fresh root is unproven
    const SolverCfg sv = *D.sv_cfg;
    const uint8_t *PO = sv.proof + ((size_t)b * 2 + rv.half) * (size_t)D.cap;
    uint8_t *PN = sv.proof + baseNew;
    // value spread (off: the word that came with the solver's): a kept node's S moves with its records; a fresh root has S = 0
    const float *SO = nullptr;
    float *SN = nullptr;
    if (sv.spread) { float *S = spread_array(D); SO = S + ((size_t)b * 2 + rv.half) * (size_t)D.cap; SN = S + baseNew; }
    if (lane == 0) { D.nodeA[baseNew] = NodeA{0, 0.0f, 1.0f, -1}; D.nodeB[baseNew] = 0u; if (sv.enabled) PN[0] = 0; if (sv.spread) SN[0] = 0.0f; } // whatever happens below, the new half holds a valid (empty) tree
    const int want = forced ? forced[b] : -1;
    // A refused board neither records nor moves: position, clocks, history, ply and move counter stay. Its tree is the empty root just
    // written, so its pool accounting restarts with it (the host flips the half word for every board), and its pending leaf is dropped.
    const auto refuse = [&](int bit) {
        if (lane == 0) { set_err(D, bit); m.n_nodes = 1; m.half = (uint8_t)nh; D.meta[b] = m; D.leaf_status[b] = CCZ_LEAF_SKIP; }
    };
    // (k == 0 and no forced move: nothing searched, nothing to sample from)
    if (k > kMaxLegal || (k == 0 && want < 0) || want >= kNMoves) { refuse(16); return; }
    const double temp = board_temp(D, m, temps, b);
    if (bad_temp(temp)) { refuse(CCZ_ERR_BAD_TEMP); return; }

    load_board(s_sq, D.root_sq + (size_t)b * 96, lane);
    for (int i = lane; i < k; i += 64) {
        s_vis[i] = rv.A[CCZ_IDX(D, rv.root.fc + i, D.cap)].N;
        s_act[i] = (uint16_t)(rv.Bn[CCZ_IDX(D, rv.root.fc + i, D.cap)] & 0xffffu);
    }
    __syncthreads();

    // ---- the documented caps: the game is adjudicated a draw, its records so far stay valid
    if (m.ply >= D.max_plies || m.pi_used + (uint32_t)k > (uint32_t)D.pi_cap) {
        if (lane == 0) {
            if (m.ply < D.max_plies) set_err(D, 8);
            else if (D.flags & CCZ_FLAG_STRICT) set_err(D, CCZ_ERR_TRUNCATED); // the reference's game has no ply cap (game.py:155)
            m.over = 1; m.winner = -1;
            D.meta[b] = m;
            D.stats[b].truncated += 1;
            D.stats[b].games += 1;
            const int rstate = D.rs_state[b];
            if (rstate & kPlayOn) playon_count(D, b, rstate, -1, m.ply);
        }
        return;
    }

    // ---- a forced move must be a legal move of the root. A searched root's children are all of its legal moves (an expansion is
    // all or nothing, pruning drops whole child lists); an unsearched root asks the generator, as k_set_positions does per ply.
    // found: the forced move's child index, -1 on an unsearched root (a fresh root below, as MCTS.update_with_move does, mcts.py:176-178)
    int found = -1;
    if (want >= 0) {
        for (int i0 = 0; i0 < k; i0 += 64) {
            const int i = i0 + lane;
            const uint64_t hit = __ballot(i < k && s_act[i] == want);
            if (hit && found < 0) found = i0 + __ffsll((long long)hit) - 1;
        }
        bool legal = found >= 0;
        if (k == 0) {
            const GenResult g = gen_legal(s_sq, m.turn, S, nullptr, lane, nullptr, D.rank, D.unrank, D.trankpack);
            if (g.overflow) set_err(D, 4);
            const int bit = D.rank ? (int)D.rank[want] : want; // bit r of the mask = the move of rank r (gen_legal)
            legal = ((S.mask[bit >> 5] >> (bit & 31)) & 1u) != 0u;
        }
        if (!legal) { refuse(16); return; }
    }

    // ---- pi (mcts.py:162-166) and the training record. The resignation value below, ccz_root_children and the lines read the
    // counts as searched (s_vis), whatever pi is formed from.
    const int tgt = D.target[b];
    // Gumbel root search (ccz_set_gumbel; off: this one word read): pi' and the rule's move in place of the visit softmax and the draw
    const GumbelCfg gc = *D.gm_cfg;
    const bool gumbel = gc.enabled && k > 0;
    int gchoice = -1;
    bool explored = false;
    if (gumbel) gchoice = gumbel_targets(D, gc, b, lane, k, m.move_counter, rv, s_g, s_pn, s_pi, found, true);
    else explored = move_target_pi(D, b, lane, rv, k, m.move_counter, tgt, temp, s_vis, s_vp, s_q, s_pn, s_g, s_pi, true);
    const size_t r = (size_t)b * D.max_plies + CCZ_IDX(D, m.ply, D.max_plies);
    if (lane < 24) ((uint32_t *)(D.rec_sq + r * 96))[lane] = ((const uint32_t *)s_sq)[lane];
    if (lane == 0) { D.rec_turn[r] = m.turn; D.rec_k[r] = (uint8_t)k; D.rec_off[r] = m.pi_used; D.rec_target[r] = (uint8_t)tgt; D.rec_hasv[r] = 0; }
    for (int i = lane; i < k; i += 64) {
        const size_t o = (size_t)b * D.pi_cap + CCZ_IDX(D, m.pi_used + (uint32_t)i, D.pi_cap);
        D.rec_ids[o] = s_act[i];
        D.rec_pi[o] = (float)s_pi[i];
    }

    // ---- policy surprise weighting (ccz_set_surprise; off: this one word read). s = KL(pi || prior) of a policy-target ply: pi is s_pi
    // as just recorded, the prior the children's stored P (root noise is never stored). A lane forms the terms of its own children (the
    // two logarithms are the cost), then every lane adds the same <= 128 LDS words in child order in float64: s is wave-uniform without
    // a broadcast and is the sequential sum bit for bit (a term of pi_i = 0 is +0.0, which changes no sum). s_g is free until the
    // resignation's root value and sample_move.
    const SurpriseBlock *sp = surprise_block(D);
    if (sp->cfg.enabled) {
        double s = 0.0;
        if (tgt) {
            __syncthreads(); // s_pi and the scratch rows of the targets are complete
            for (int i = lane; i < k; i += 64) {
                const double p = s_pi[i];
                double term = 0.0;
                if (p > 0.0) {
                    double q = (double)rv.A[CCZ_IDX(D, rv.root.fc + i, D.cap)].P;
                    if (!(q >= 0x1p-100)) q = 0x1p-100;
                    term = p * (det_log(p) - det_log(q));
                }
                s_g[i] = term;
            }
            __syncthreads();
            for (int i = 0; i < k; ++i) s = s + s_g[i];
            if (!(s > 0.0)) s = 0.0;
            __syncthreads(); // every lane has read s_g before the code below writes it
        }
        if (lane == 0) {
            sp->rec_kl[r] = (float)s;
            sp->rec_hask[r] = tgt ? 1 : 0;
            if (tgt) {
                SurpriseBoardStats &ss = sp->sp_stats[b];
                ss.plies += 1;
                ss.sum = ss.sum + (double)(float)s;
            }
        }
    }

    // A ply is played by a move or by resigning: the record took k entries, the board's Philox move counter advances, and the board's
    // tree (n_nodes nodes) lies in the other pool half
    const auto ply_played = [&](int n_nodes) { m.ply += 1; m.move_counter += 1; m.n_nodes = n_nodes; m.half = (uint8_t)nh; m.pi_used += (uint32_t)k; };

    // ---- resignation (ccz_set_resign; off: one word read, nothing below runs). The root value is the visit-weighted mean of the
    // children's Q as stored (the view of the root's side to move), summed in child order in float64: every lane runs the same <= 128
    // terms on the same LDS words, so the decision is wave-uniform without a broadcast. s_g is free until sample_move.
    const ResignCfg rc = *D.rs_cfg;
    if (rc.enabled) {
        for (int i = lane; i < k; i += 64) s_g[i] = (double)rv.A[CCZ_IDX(D, rv.root.fc + i, D.cap)].Q;
        __syncthreads();
        double acc = 0.0;
        long long nsum = 0;
        for (int i = 0; i < k; ++i) { acc = acc + (double)s_vis[i] * s_g[i]; nsum += s_vis[i]; }
        const double v = nsum ? acc / (double)nsum : 0.0;
        const int s = m.turn;
        const int state = D.rs_state[b];
        int run = D.rs_run[(size_t)b * 2 + s];
        if (tgt) { run = v < (double)rc.threshold ? (run < 255 ? run + 1 : 255) : 0; } // a fast ply records v and leaves the run alone
        bool fire = tgt && rc.consecutive > 0 && run >= rc.consecutive && m.ply >= rc.min_ply && want < 0 && !(state & kPlayOn);
        bool playon = false;
        if (fire) { // the lot: word 0xffd of the board's Philox stream for this move (Gamma draws: 0..127, budgets: 0xffe, move choice: 0xfff)
            double ua, ub;
            uniform2(D.seed, D.board_id_base + (uint64_t)b, m.move_counter, 0xffdu, 0, ua, ub);
            playon = ua < rc.p_playon;
            fire = !playon;
        }
        __syncthreads(); // s_g is read above by every lane before sample_move writes it
        if (lane == 0) {
            D.rec_value[r] = (float)v;
            D.rec_hasv[r] = 1;
            D.rs_last[b] = (float)v;
            if (tgt) D.rs_run[(size_t)b * 2 + s] = (uint8_t)run;
            if (playon) { D.rs_state[b] = (uint8_t)(kPlayOn | s); D.rs_fire[b] = m.ply; }
        }
        if (fire) {
            // the side to move resigns: the ply is a sample like any other (the search was done), no move is pushed -- root position,
            // key, clock, history chain and check bits stay -- and the new pool half keeps the empty root written above
            if (lane == 0) {
                D.rs_state[b] = (uint8_t)(kResigned | s);
                D.rs_fire[b] = m.ply;
                ply_played(1);
                m.over = 1;
                m.winner = (int8_t)(s ^ 1);
                D.meta[b] = m;
                D.stats[b].games += 1;
                D.leaf_status[b] = CCZ_LEAF_SKIP;
                ResignBoardStats &rs = D.rs_stats[b];
                rs.resigned += 1;
                rs.resigned_red += (unsigned long long)s;
                rs.resigned_plies += (unsigned long long)m.ply;
            }
            return;
        }
    }

    // ---- move choice (mcts.py:216-229)
    if (want >= 0) {
        if (lane == 0) s_choice = found;
    } else if (gumbel) {
        if (lane == 0) s_choice = gchoice;
    } else {
        sample_move(D, D.board_id_base + (uint64_t)b, m.move_counter, s_pi, s_g, k, lane, &s_choice, nullptr, nullptr, nullptr, !explored);
    }
    __syncthreads();
    const int ci = s_choice;
    const int mv = ci >= 0 ? (int)s_act[ci] : want;
    if (moves_out && lane == 0) moves_out[b] = mv;

    // ---- MCTS.update_with_move (mcts.py:168-178): re-root on the chosen child, subtree copied breadth-first into the other pool
    // half (children of a node stay contiguous); a forced move that is no child of the root, or !keep_tree: a fresh root
    NodeA *NA = D.nodeA + baseNew;
    uint32_t *NB = D.nodeB + baseNew;
    int n_new = 1;
    if (ci < 0) keep_tree = 0;
    if (keep_tree) {
        if (lane == 0) {
            NA[0] = rv.A[CCZ_IDX(D, rv.root.fc + ci, D.cap)];
            NB[0] = rv.Bn[CCZ_IDX(D, rv.root.fc + ci, D.cap)];
            if (sv.enabled) PN[0] = PO[CCZ_IDX(D, rv.root.fc + ci, D.cap)];
            if (sv.spread) SN[0] = SO[CCZ_IDX(D, rv.root.fc + ci, D.cap)];
        }
        __syncthreads();
        int head = 0, pruned = 0;
        // The kept subtree may use the pool up to `budget`, leaving room for a whole move of new expansions.
        // Breadth-first order copies the tree level by level, so when the budget runs out it is the DEEPEST nodes
        // that lose their children (they become unexpanded leaves again, keeping N, Q, P): bounded memory with a
        // graceful loss at the bottom of very concentrated trees instead of failed expansions later (counted in
        // stats.pruned_subtrees; the reference's Python tree is unbounded, DESIGN.md "caps").
        const int budget = D.cap - D.reserve;
        while (head < n_new) {
            const int i = head + lane;
            const bool valid = i < n_new;
            NodeA rec = NodeA{0, 0.0f, 0.0f, -1};
            int nc = 0;
            if (valid) { rec = NA[CCZ_IDX(D, i, D.cap)]; nc = (int)(NB[CCZ_IDX(D, i, D.cap)] >> 16); }
            const int incl = wave_incl_scan(nc, lane);
            const bool keep_kids = nc > 0 && n_new + incl <= budget;   // a prefix of the lanes: incl is non-decreasing
            const bool drop = nc > 0 && !keep_kids;
            const uint64_t km = __ballot(keep_kids);
            const int total = km ? __builtin_amdgcn_readlane(incl, __builtin_amdgcn_readfirstlane(63 - __builtin_clzll(km))) : 0;
            const int dst = n_new + incl - nc;
            s_cnt[lane] = keep_kids ? nc : 0;
            if (keep_kids) { s_src[lane] = rec.fc; s_dst[lane] = dst; NA[i].fc = dst; }
            if (drop) { NA[i].fc = -1; NB[i] = NB[i] & 0xffffu; }
            pruned += __popcll(__ballot(drop));
            __syncthreads();
            uint64_t todo = km;
            while (todo) {
                const int L = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int src = s_src[L], dd = s_dst[L], cn = s_cnt[L];
                for (int j = lane; j < cn; j += 64) {
                    NA[CCZ_IDX(D, dd + j, D.cap)] = rv.A[CCZ_IDX(D, src + j, D.cap)];
                    NB[CCZ_IDX(D, dd + j, D.cap)] = rv.Bn[CCZ_IDX(D, src + j, D.cap)];
                    if (sv.enabled) PN[CCZ_IDX(D, dd + j, D.cap)] = PO[CCZ_IDX(D, src + j, D.cap)];
                    if (sv.spread) SN[CCZ_IDX(D, dd + j, D.cap)] = SO[CCZ_IDX(D, src + j, D.cap)];
                }
            }
            const int nbatch = n_new - head < 64 ? n_new - head : 64;
            head += nbatch;
            n_new += total;
            __syncthreads();
        }
        if (pruned && lane == 0) {
            D.stats[b].pruned += (unsigned long long)pruned;
            if (D.flags & CCZ_FLAG_STRICT) set_err(D, CCZ_ERR_PRUNED); // the reference's tree is unbounded (mcts.py:31-39)
        }
    }
    if (!keep_tree || n_new == 0) {
        if (lane == 0) { NA[0] = NodeA{0, 0.0f, 1.0f, -1}; NB[0] = 0u; if (sv.enabled) PN[0] = 0; if (sv.spread) SN[0] = 0.0f; }
        n_new = 1;
    }

    // ---- push on the root, its history (the chain comes from memory, the new key goes back), game end
    RootState st = {m.key, m.turn, m.halfmove, m.chain_len, D.chain_chk[(size_t)b * 2], D.chain_chk[(size_t)b * 2 + 1]};
    for (int i = lane; i < st.chain_len; i += 64) s_chain[i] = D.chain[(size_t)b * kChainCap + i];
    if (push_root_move(D, mv, s_sq, s_chain, st, lane, [] { __syncthreads(); })) set_err(D, 64);
    if (lane == 0) D.chain[(size_t)b * kChainCap + CCZ_IDX(D, st.chain_len - 1, kChainCap)] = st.key;
    if (lane < 24) ((uint32_t *)(D.root_sq + (size_t)b * 96))[lane] = ((const uint32_t *)s_sq)[lane];
    const GameEnd end = root_game_end(D.rule_flags, s_sq, s_chain, S, st, lane);
    if (end.overflow) set_err(D, 4);

    // ---- commit
    if (lane == 0) {
        D.chain_chk[(size_t)b * 2] = st.chk0;
        D.chain_chk[(size_t)b * 2 + 1] = st.chk1;
        m.key = st.key;
        m.halfmove = st.halfmove;
        m.chain_len = st.chain_len;
        m.turn = (uint8_t)st.turn;
        ply_played(n_new);
        BoardStats &bs = D.stats[b];
        bs.moves += 1;
        if (end.over) {
            m.over = 1;
            m.winner = (int8_t)end.winner;
            bs.games += 1;
            const int rstate = D.rs_state[b];
            if (rstate & kPlayOn) playon_count(D, b, rstate, m.winner, m.ply);
        }
        D.meta[b] = m;
        D.leaf_status[b] = CCZ_LEAF_SKIP;
    }
}

// ------------------------------------------------------------------ many positions with their move history, in one launch
// One wave per board (ccz_set_positions): validate the position, replay the board's moves with the engine's own rules -- every
// move must be in the legal-move set of the position it is played in (gen_legal with the engine's rank table: the generator of the
// selection) and is pushed by push_root_move, the check bit of the position before it set by mark_check --, call root_game_end on
// the position reached (only if moves were played: without moves the board is left exactly as k_set_position leaves it), and finish
// as init_board does. status: 0 loaded, 1 + i move i is not legal where it is played, -1 invalid position, -2 more than kChainCap
// positions since the last zeroing move. A board with a non-zero status, or with n_moves == -1, is PARKED: empty mailbox, over = 1,
// winner = -1, ply = 0, a root without children -- the simulator skips it (m.over), the harvest has nothing to emit for it. Bad input
// sets no sticky error bit. The replay is a chain of n dependent move generations (~ n x the leaf phase of k_step); the moves are
// fetched 64 at a time so that no load sits between two of them.
__global__ __launch_bounds__(64) void k_set_positions(Dev D, const uint8_t *mask, const uint8_t *sq_in, const uint8_t *turn_in,
                                                        const int32_t *halfmove_in, const int32_t *moves, const int32_t *n_moves,
                                                        int max_moves, int32_t *status_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[b]) return;
    __shared__ __align__(16) uint8_t s_sq[96];
    __shared__ uint64_t s_chain[kChainCap];
    __shared__ GenScratch S;
    const int n = n_moves ? n_moves[b] : 0;
    RootState st = {0ull, turn_in[b] ? 1 : 0, halfmove_in ? halfmove_in[b] : 0, 1, 0ull, 0ull};
    const uint8_t *src = sq_in + (size_t)b * 96;
    const int p0 = src[lane], p1 = lane < 26 ? src[64 + lane] : 0;
    const bool park = n == -1;
    int status = 0;
    if (!park) {
        // what ccz_set_position checks on the host: piece codes, one king per side, the clock; and at most 16 pieces per side
        // (the generator's piece list), a move count inside the row
        const bool badcode = p0 > 15 || p0 == 8 || p1 > 15 || p1 == 8;
        const int kr = __popcll(__ballot(p0 == KING)) + __popcll(__ballot(p1 == KING));
        const int kb = __popcll(__ballot(p0 == KING + 8)) + __popcll(__ballot(p1 == KING + 8));
        const int nr = __popcll(__ballot(p0 >= 1 && p0 <= 7)) + __popcll(__ballot(p1 >= 1 && p1 <= 7));
        const int nb = __popcll(__ballot(p0 >= 9 && p0 <= 15)) + __popcll(__ballot(p1 >= 9 && p1 <= 15));
        if (__ballot(badcode) != 0ull || kr != 1 || kb != 1 || nr > 16 || nb > 16 || st.halfmove < 0 || n < -1 || n > max_moves) status = -1;
    }
    GameEnd end = {false, -1, false};
    if (!park && status == 0) {
        s_sq[lane] = (uint8_t)p0;
        if (lane < 32) s_sq[64 + lane] = (uint8_t)p1; // (p1 == 0 for lanes 26..31: the mailbox pad)
        if (p0) st.key ^= zob(p0, lane);
        if (p1) st.key ^= zob(p1, 64 + lane);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) st.key ^= __shfl_xor(st.key, o);
        if (st.turn) st.key ^= kTurnKey;
        if (lane == 0) s_chain[0] = st.key;
        wave_sync();
        const int32_t *row = moves + (size_t)b * (size_t)max_moves;
        int mvreg = -1;
        for (int i = 0; i < n; ++i) {
            if ((i & 63) == 0) mvreg = i + lane < n ? row[i + lane] : -1;
            const int mv = __builtin_amdgcn_readlane(mvreg, __builtin_amdgcn_readfirstlane(i & 63));
            const GenResult g = gen_legal(s_sq, st.turn, S, nullptr, lane, nullptr, D.rank, D.unrank, D.trankpack);
            if (g.overflow) { status = -1; break; }
            if (i > 0) mark_check(s_sq, S, g.ksq, st); // the move before gave check
            bool legal = (unsigned)mv < (unsigned)kNMoves;
            if (legal) {
                const int bit = D.rank ? (int)D.rank[mv] : mv; // bit r of the mask = the move of rank r (gen_legal)
                legal = ((S.mask[bit >> 5] >> (bit & 31)) & 1u) != 0u;
            }
            if (!legal) { status = 1 + i; break; }
            if (push_root_move(D, mv, s_sq, s_chain, st, lane, [] { wave_sync(); })) { status = -2; break; }
        }
        if (status == 0 && n > 0) {
            end = root_game_end(D.rule_flags, s_sq, s_chain, S, st, lane);
            if (end.overflow) status = -1;
        }
        wave_sync();
    }
    const bool parked = park || status != 0;
    if (parked) { st = RootState{0ull, 1, 0, 1, 0ull, 0ull}; end.over = true; end.winner = -1; }
    if (lane < 24) ((uint32_t *)(D.root_sq + (size_t)b * 96))[lane] = parked ? 0u : ((const uint32_t *)s_sq)[lane];
    uint64_t *chain = D.chain + (size_t)b * kChainCap;
    if (parked) { if (lane == 0) chain[0] = 0ull; }
    else for (int i = lane; i < st.chain_len; i += 64) chain[i] = s_chain[i];
    if (lane == 0) {
        BoardMeta m = D.meta[b];
        m.key = st.key;
        m.halfmove = st.halfmove;
        m.chain_len = st.chain_len;
        m.ply = 0;
        m.n_nodes = 1;
        m.turn = (uint8_t)st.turn;
        m.over = (uint8_t)end.over;
        m.winner = (int8_t)end.winner;
        m.pi_used = 0;
        m.game_no += 1;
        m.half = (uint8_t)*D.half;
        D.meta[b] = m;
        D.chain_chk[(size_t)b * 2] = st.chk0;
        D.chain_chk[(size_t)b * 2 + 1] = st.chk1;
        fresh_root(D, b, m.half);
        resign_clear(D, b);
        status_out[b] = status;
    }
}

// ------------------------------------------------------------------ principal variations: the tree below the root
// One wave per (board, line) (ccz_principal_variations). Line r starts at the root child of rank r -- by visits, descending, ties
// to the lower child index, so rank 0 is the first maximum: the arg-max move (mcts.py:225-229) -- and follows the first child of
// maximal N while that N is > 0. Per level every lane loads its share of the <= 128 children (NodeA + move word) in one round,
// the first maximum is the selection's idiom (wave max on the DPP network, ballot, lowest index), and the winner's record is
// broadcast from its lane. Like the descent of k_step this is a chain of dependent loads, one round trip per level: latency-bound,
// microseconds per line, no bandwidth to speak of. Boards that are over or scout slots (b >= active) get zero lines.
struct PvCand {
    int32_t N, fc, idx;
    float Q, P;
    uint32_t w;
};

__device__ __forceinline__ PvCand pv_bcast(const PvCand &c, int owner)
{
    PvCand o;
    o.N = __builtin_amdgcn_readlane(c.N, owner);
    o.fc = __builtin_amdgcn_readlane(c.fc, owner);
    o.idx = __builtin_amdgcn_readlane(c.idx, owner);
    o.Q = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.Q), owner));
    o.P = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.P), owner));
    o.w = (uint32_t)__builtin_amdgcn_readlane((int)c.w, owner);
    return o;
}

__global__ __launch_bounds__(64) void k_principal_variations(Dev D, int active, int multipv, int max_len, uint16_t *moves_out,
                                                               int32_t *len_out, int32_t *visits_out, float *q_out, float *prior_out,
                                                               int32_t *root_visits)
{
    const int b = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const size_t line = (size_t)b * (size_t)multipv + (size_t)r;
    uint16_t *mv_o = moves_out + line * (size_t)max_len;
    int32_t *n_o = visits_out + line * (size_t)max_len;
    const BoardMeta m = D.meta[b];
    const size_t base = ((size_t)b * 2 + *D.half) * (size_t)D.cap;
    const NodeA *A = D.nodeA + base;
    const uint32_t *Bn = D.nodeB + base;
    const NodeA root = A[0];
    const bool live = b < active && !m.over;
    if (r == 0 && lane == 0) root_visits[b] = live ? root.N : 0;
    int len = 0;
    float q1 = 0.0f, p1 = 0.0f;
    int fc = root.fc, nc = (int)(Bn[0] >> 16);
    while (live && len < max_len) {
        if (nc > kMaxLegal) nc = kMaxLegal;
        if (nc <= 0 || fc < 0 || fc + nc > D.cap) break; // unexpanded node (or a record no tree of this engine holds: nothing is read)
        // every lane's share of the children: i = lane and 64 + lane
        PvCand c0 = PvCand{-1, -1, lane, 0.0f, 0.0f, 0u}, c1 = PvCand{-1, -1, 64 + lane, 0.0f, 0.0f, 0u};
        if (lane < nc) {
            const NodeA c = A[CCZ_IDX(D, fc + lane, D.cap)];
            c0.N = c.N; c0.fc = c.fc; c0.Q = c.Q; c0.P = c.P;
            c0.w = Bn[CCZ_IDX(D, fc + lane, D.cap)];
        }
        if (64 + lane < nc) {
            const NodeA c = A[CCZ_IDX(D, fc + 64 + lane, D.cap)];
            c1.N = c.N; c1.fc = c.fc; c1.Q = c.Q; c1.P = c.P;
            c1.w = Bn[CCZ_IDX(D, fc + 64 + lane, D.cap)];
        }
        PvCand mine;
        bool hit;
        if (len == 0 && r > 0) {
            // the root child of rank r: a child's rank = the children with more visits + the earlier ones with as many
            int rk0 = 0, rk1 = 0;
            for (int j = 0; j < nc; ++j) {
                const int js = __builtin_amdgcn_readfirstlane(j & 63);
                const int nj = j < 64 ? __builtin_amdgcn_readlane(c0.N, js) : __builtin_amdgcn_readlane(c1.N, js);
                rk0 += (nj > c0.N || (nj == c0.N && j < lane)) ? 1 : 0;
                rk1 += (nj > c1.N || (nj == c1.N && j < 64 + lane)) ? 1 : 0;
            }
            const bool s1 = 64 + lane < nc && rk1 == r;
            mine = s1 ? c1 : c0;
            hit = (s1 || (lane < nc && rk0 == r)) && mine.N > 0;
        } else {
            // first maximum of N (a lane's own best is its lower index unless the upper one is larger), N > 0
            mine = c1.N > c0.N ? c1 : c0;
            const double top = wave_max_f64((double)mine.N);
            hit = top > 0.0 && (double)mine.N == top && mine.idx < nc;
        }
        const uint64_t h0 = __ballot(hit && mine.idx < 64), h1 = __ballot(hit);
        if (h1 == 0ull) break; // no visited child (or fewer than r + 1 visited root children)
        const int owner = __builtin_amdgcn_readfirstlane((h0 ? __ffsll((long long)h0) : __ffsll((long long)h1)) - 1);
        const PvCand ch = pv_bcast(mine, owner);
        if (lane == 0) {
            mv_o[len] = (uint16_t)(ch.w & 0xffffu);
            n_o[len] = ch.N;
        }
        if (len == 0) { q1 = ch.Q; p1 = ch.P; }
        ++len;
        fc = ch.fc;
        nc = (int)(ch.w >> 16);
    }
    if (lane == 0) {
        len_out[line] = len;
        q_out[line] = q1;
        prior_out[line] = p1;
    }
    for (int j = len + lane; j < max_len; j += 64) { mv_o[j] = 0; n_o[j] = 0; }
}

// ------------------------------------------------------------------ harvest: finished games -> training rows
// rows of board b start at row_base[b] (< 0: board not harvested). Per game: T samples then, unless
// CCZ_FLAG_NO_MIRROR, their T mirror images (collect.py:112-131: data + data_flip). Grid = (boards, kHarvestSlices):
// only a few dozen games end per move, so the plies of a game are spread over kHarvestSlices blocks (one 256-thread
// block per game left the chip nearly empty: 1.8 ms for 28 k rows; the blocks of boards that are not harvested exit at once).
constexpr int kHarvestSlices = 32;
// One dense training row (game.py:213-237 z and history, collect.py:64-131 preprocess + flip_data): the 17 x 7 x 10 x 9 fp16
// planes, the sparse -> dense pi scatter and z; pass 0 = the sample, pass 1 = its mirror image. The ONE place where a row is
// formed: k_harvest, k_expand_records and k_sample_records all call it, so what they write is equal by construction. They
// differ only in where a ply is read from, which `src` says (HarvestPly: the engine's arrays; RecordPly: a record and its
// staged history): sq(i, s) = the piece on square s of the position i plies back (game.py:23-44), turn(), winner(), k(),
// pi_id(i) (< 0: skip the entry) and pi_val(i). All 256 threads of the block call it together.
template <class Src>
__device__ __forceinline__ void form_row(const Src &src, int pass, int turn_plane, uint32_t typepack, uint16_t *states, float *pi, float *z,
                                         long long row)
{
    const int tid = threadIdx.x;
    uint32_t *srow = (uint32_t *)(states + (size_t)row * 10710);
    for (int i = tid; i < 5355; i += 256) {
        uint32_t v = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = 2 * i + h;
            const int g = e / 630, w = e - g * 630;
            bool on;
            if (g == 16) on = turn_plane != 0;
            else {
                const int ch = w / 90, s = w - 90 * ch;
                const int ss = pass ? (s - s % 9) + (8 - s % 9) : s; // np.flip(axis=2): file mirror
                on = src.sq(g & 7, ss) == (int)((typepack >> (3 * ch)) & 7u) + 1 + (g >= 8 ? 8 : 0);
            }
            if (on) v |= (uint32_t)kHalfOne << (16 * h);
        }
        srow[i] = v;
    }
    float *prow = pi + (size_t)row * kNMoves;
    for (int i = tid; i < kNMoves; i += 256) prow[i] = 0.0f;
    __syncthreads();
    const int k = src.k();
    for (int i = tid; i < k; i += 256) {
        const int id = src.pi_id(i);
        if (id >= 0) prow[pass ? c_tab.flip[id] : id] = src.pi_val(i); // mcts_prob[flip_map]
    }
    if (tid == 0) { // game.py:213-219
        const int8_t w = src.winner();
        z[row] = w < 0 ? 0.0f : (src.turn() == (uint8_t)w ? 1.0f : -1.0f);
    }
    __syncthreads();
}

// ply t of board b's finished game, where k_harvest reads it: D.rec_sq / rec_turn / rec_k / rec_off / rec_ids / rec_pi in global memory
struct HarvestPly {
    const Dev &D;
    const BoardMeta &m;
    int b, te; // te: the ply whose history the row shows
    size_t r;
    const uint8_t *rsq; // the board's recorded positions
    __device__ __forceinline__ int sq(int back, int ss) const
    {
        int tp = te - back;
        if (tp < 0) tp = 0;
        return rsq[(size_t)CCZ_IDX(D, tp, D.max_plies) * 96 + CCZ_IDX(D, ss, 90)];
    }
    __device__ __forceinline__ uint8_t turn() const { return D.rec_turn[r]; }
    __device__ __forceinline__ int8_t winner() const { return m.winner; }
    __device__ __forceinline__ int k() const { return D.rec_k[r]; }
    __device__ __forceinline__ int pi_id(int i) const
    {
        return (int)CCZ_IDX(D, D.rec_ids[(size_t)b * D.pi_cap + CCZ_IDX(D, D.rec_off[r] + (uint32_t)i, D.pi_cap)], kNMoves);
    }
    __device__ __forceinline__ float pi_val(int i) const { return D.rec_pi[(size_t)b * D.pi_cap + D.rec_off[r] + i]; }
};

__global__ __launch_bounds__(256) void k_harvest(Dev D, const long long *row_base, uint16_t *states, float *pi, float *z)
{
    const int b = blockIdx.x;
    const long long rb = row_base[b];
    if (rb < 0) return;
    const BoardMeta m = D.meta[b];
    const int T = m.ply;
    const bool quirks = (D.flags & 1u) != 0, mirror = (D.flags & 2u) == 0;
    const uint8_t *rsq = D.rec_sq + (size_t)b * D.max_plies * 96;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        // reference quirk: every sample aliases the history at the LAST recorded ply
        const HarvestPly src{D, m, b, quirks ? T - 1 : t, (size_t)b * D.max_plies + t, rsq};
        const int turn_plane = quirks ? 1 : src.turn(); // collect.py:78 reads a board that never advances
        for (int pass = 0; pass < (mirror ? 2 : 1); ++pass) form_row(src, pass, turn_plane, D.typepack, states, pi, z, rb + (pass ? T : 0) + t);
    }
}

// ------------------------------------------------------------------ compact game records (the multi-GPU wire format)
// One fixed-size record per PLY of a finished game (include/cczero.h: CCZ_REC_*): position before the move, 16-byte
// header, sparse pi (ids + float32, zero-padded to 128). The plies of a game are contiguous and in order, so a record
// finds its game's first record at (index - t) and the two dense rows it stands for (the sample and its mirror image)
// at 2 * first + t and 2 * first + T + t: expansion needs no prefix sum and no engine state. 880 B per ply against
// 2 x 29,768 B of dense rows: what the all-gather moves (k_expand_records rebuilds the rows on the receiving side).
constexpr int kRecBytes = 880, kRecHdr = 96, kRecIds = 112, kRecPi = 368;
constexpr uint8_t kRecFast = 1; // PlyHeader.flags (CCZ_REC_FAST): a fast move of playout-cap randomisation, its pi is no policy target
constexpr uint8_t kRecValue = 8; // PlyHeader.flags (CCZ_REC_VALUE): bytes 92..95 of the record hold the ply's root value (float32)
constexpr uint8_t kRecWeight = 16; // PlyHeader.flags (CCZ_REC_WEIGHT): bytes 90..91 of the record hold the ply's sampling weight (uint16, 1/4096)
constexpr int kRecWeightOff = 90;
constexpr int kRecValueOff = 92; // (flags 2 and 4, CCZ_REC_RESIGNED / CCZ_REC_PLAYON on every ply of such a game, are kResigned / kPlayOn)
struct __align__(4) PlyHeader {
    uint16_t t, T;      // ply index inside its game, plies of the game
    int8_t winner;      // 1 RED, 0 BLACK, -1 draw
    uint8_t turn, k, flags;
    uint32_t board_id;  // global board id (low 32 bits)
    uint32_t game_no;
};
static_assert(sizeof(PlyHeader) == 16, "ply header is 16 bytes");

// rec_base[b]: index of the first record of board b's game in `out` (< 0: board not harvested)
__global__ __launch_bounds__(256) void k_harvest_records(Dev D, const long long *rec_base, uint8_t *out)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long rb = rec_base[b];
    if (rb < 0) return;
    const BoardMeta m = D.meta[b];
    const int T = m.ply;
    // policy surprise weighting (ccz_set_surprise; off: this one word read): the game's n plies that carry a surprise and their sum S, the
    // float32 values added as doubles in ply order -- by every block of the game in the same order, so no block waits for another
    const SurpriseBlock *sp = surprise_block(D);
    const bool weigh = sp->cfg.enabled != 0;
    double sp_alpha = 0.0, sp_cap = 0.0, S = 0.0;
    const float *rec_kl = nullptr;
    const uint8_t *rec_hask = nullptr;
    int n = 0;
    if (weigh) {
        sp_alpha = sp->cfg.alpha;
        sp_cap = sp->cfg.cap;
        rec_kl = sp->rec_kl;
        rec_hask = sp->rec_hask;
        for (int t = 0; t < T; ++t) {
            const size_t r = (size_t)b * D.max_plies + t;
            if (rec_hask[r]) { S = S + (double)rec_kl[r]; n += 1; }
        }
    }
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const size_t r = (size_t)b * D.max_plies + t;
        uint32_t *rec = (uint32_t *)(out + (size_t)(rb + t) * kRecBytes);
        const int k = D.rec_k[r];
        const size_t po = (size_t)b * D.pi_cap + D.rec_off[r];
        if (tid < 24) {
            uint32_t v = ((const uint32_t *)(D.rec_sq + r * 96))[tid];
            if (tid == 22) {
                v &= 0x0000ffffu;
                if (weigh) { // bytes 90..91: the ply's sampling weight in 1/4096 (CCZ_REC_WEIGHT)
                    double w = 1.0;
                    if (rec_hask[r] && S > 0.0) w = (1.0 - sp_alpha) + sp_alpha * (double)n * (double)rec_kl[r] / S;
                    if (w > sp_cap) { w = sp_cap; atomicAdd(&sp->sp_stats[b].clipped, 1ull); }
                    v |= (uint32_t)(uint16_t)floor(w * 4096.0 + 0.5) << 16;
                }
            }
            if (tid == 23) v = D.rec_hasv[r] ? __float_as_uint(D.rec_value[r]) : 0u; // bytes 92..95: the ply's root value (CCZ_REC_VALUE)
            rec[tid] = v;
        } else if (tid == 24) {
            PlyHeader h;
            h.t = (uint16_t)t; h.T = (uint16_t)T; h.winner = m.winner; h.turn = D.rec_turn[r]; h.k = (uint8_t)k;
            h.flags = (uint8_t)((D.rec_target[r] ? 0 : kRecFast) | (D.rs_state[b] & (kResigned | kPlayOn)) | (D.rec_hasv[r] ? kRecValue : 0) | (weigh ? kRecWeight : 0));
            h.board_id = (uint32_t)(D.board_id_base + (uint64_t)b); h.game_no = m.game_no;
            *(PlyHeader *)(rec + kRecHdr / 4) = h;
        }
        if (tid < 64) { // ids: 128 x u16 = 64 dwords
            const int i0 = 2 * tid, i1 = 2 * tid + 1;
            const uint32_t lo = i0 < k ? D.rec_ids[po + i0] : 0u, hi = i1 < k ? D.rec_ids[po + i1] : 0u;
            rec[kRecIds / 4 + tid] = lo | (hi << 16);
        } else if (tid < 192) {
            const int i = tid - 64;
            ((float *)rec)[kRecPi / 4 + i] = i < k ? D.rec_pi[po + i] : 0.0f;
        }
    }
}

// the policy-target byte of a ply (0: a fast move of playout-cap randomisation) and its root value (NaN: the record carries none)
__device__ __forceinline__ uint8_t rec_target(const PlyHeader &h) { return (h.flags & kRecFast) ? 0 : 1; }
__device__ __forceinline__ float rec_value(const uint8_t *rec, const PlyHeader &h)
{
    return (h.flags & kRecValue) ? *(const float *)(rec + kRecValueOff) : __builtin_nanf("");
}
// the side outputs of one row (either may be null), written by one thread next to z
__device__ __forceinline__ void write_side(uint8_t *target, float *value, long long row, uint8_t tg, float v)
{
    if (target) target[row] = tg;
    if (value) value[row] = v;
}

// a ply where the record kernels read it: its own record and the 8-deep history stage_history put into LDS
struct RecordPly {
    const uint8_t (*hist)[96];
    const uint8_t *rec;
    const PlyHeader &h;
    __device__ __forceinline__ int sq(int back, int ss) const { return hist[back][ss]; }
    __device__ __forceinline__ uint8_t turn() const { return h.turn; }
    __device__ __forceinline__ int8_t winner() const { return h.winner; }
    __device__ __forceinline__ int k() const { return h.k; }
    __device__ __forceinline__ int pi_id(int i) const
    {
        const int id = ((const uint16_t *)(rec + kRecIds))[i];
        return id < kNMoves ? id : -1;
    }
    __device__ __forceinline__ float pi_val(int i) const { return ((const float *)(rec + kRecPi))[i]; }
};

// The 8-deep history of game.py:23-44 of ply h.t of the game whose first record is record `first`: index i = the position i
// plies back, the first one before that (game.py:234-237, quirk mode: every sample aliases the history at the LAST recorded
// ply). slot_of(record index) = where that record lies in `recs`. Ends with a barrier: all 256 threads call it together.
template <class SlotOf>
__device__ __forceinline__ void stage_history(uint8_t (*hist)[96], const uint8_t *recs, long long first, const PlyHeader &h, bool quirks, SlotOf slot_of)
{
    const int tid = threadIdx.x, te = quirks ? h.T - 1 : h.t;
    if (tid < 192) {
        const int i = tid / 24, w = tid - 24 * i;
        int tp = te - i;
        if (tp < 0) tp = 0;
        ((uint32_t *)hist[i])[w] = ((const uint32_t *)(recs + (size_t)slot_of(first + tp) * kRecBytes))[w];
    }
    __syncthreads();
}

// Record p of a buffer of n_plies records, as k_expand_records sees it: its header, the first record of its game, whether the
// game is whole in the buffer, and row(q), q < mul: the dense row of pass q -- for a record whose game is cut, the q-th of the
// rows it would have stood for in a buffer of whole games, (head + mul * p + q) % ring_rows: exactly the rows the whole games
// leave out.
struct ExpandPly {
    PlyHeader h;
    long long p, first, mul, ring_rows, head;
    bool whole; // else nothing of the game may be read: its records may lie outside the buffer
    __device__ __forceinline__ long long row(int q) const
    {
        const long long i = head + (whole ? mul * first + (q ? h.T : 0) + h.t : mul * p + q);
        return ring_rows > 0 ? i % ring_rows : i;
    }
};
__device__ __forceinline__ ExpandPly locate_expand_ply(const uint8_t *recs, long long p, long long n_plies, uint32_t flags, long long ring_rows,
                                                       long long head)
{
    ExpandPly e;
    e.h = *(const PlyHeader *)(recs + (size_t)p * kRecBytes + kRecHdr);
    e.p = p;
    e.first = p - e.h.t;
    e.mul = (flags & 2u) ? 1 : 2;
    e.ring_rows = ring_rows;
    e.head = head;
    e.whole = !(e.first < 0 || e.h.t >= e.h.T || e.first + e.h.T > n_plies || e.h.k > kMaxLegal);
    return e;
}

// Records -> dense training rows, exactly what k_harvest writes for the same games (form_row). One block per ply record; rows
// go to a ring of ring_rows rows starting at row `head` (head = 0 and ring_rows >= rows: a plain array). flags:
// CCZ_FLAG_REFERENCE_QUIRKS / CCZ_FLAG_NO_MIRROR; typepack: 3 bits per plane channel = piece type - 1 encoded there
// (ccz_config.plane_of_type inverted). target / value (either may be null): the policy-target byte and the root value of every
// row, the mirror row carrying its ply's; the rows a cut game leaves unwritten get 0 / NaN, and the record counts in *bad.
// Side-only mode: states == nullptr (then pi and z are null too) stages no history and forms no row; only target / value are
// written. It serves callers that want the side outputs alone and is no faster than it looks: one thread per block works.
__global__ __launch_bounds__(256) void k_expand_records(const uint8_t *recs, long long n_plies, uint32_t flags, uint32_t typepack,
                                                          uint16_t *states, float *pi, float *z, long long ring_rows, long long head,
                                                          int32_t *bad, uint8_t *target, float *value)
{
    const long long p = blockIdx.x;
    const int tid = threadIdx.x;
    if (p >= n_plies) return;
    __shared__ __align__(16) uint8_t hist[8][96];
    const uint8_t *rec = recs + (size_t)p * kRecBytes;
    const ExpandPly e = locate_expand_ply(recs, p, n_plies, flags, ring_rows, head);
    const int passes = (int)e.mul;
    const long long row[2] = {e.row(0), e.row(passes - 1)};
    if (tid == 0) {
        if (!e.whole && bad) atomicAdd(bad, 1);
        for (int q = 0; q < passes; ++q) write_side(target, value, row[q], e.whole ? rec_target(e.h) : 0, e.whole ? rec_value(rec, e.h) : __builtin_nanf(""));
    }
    if (!e.whole || !states) return;
    const bool quirks = (flags & 1u) != 0;
    stage_history(hist, recs, e.first, e.h, quirks, [](long long q) { return q; });
    const RecordPly src{hist, rec, e.h};
    const int turn_plane = quirks ? 1 : e.h.turn; // collect.py:78 reads a board that never advances
    for (int pass = 0; pass < passes; ++pass) form_row(src, pass, turn_plane, typepack, states, pi, z, row[pass]);
}

// ------------------------------------------------------------------ the replay ring of compact records
// The ring keeps what the exchange delivers -- 880 B per ply instead of the 2 x 29,768 B of dense rows -- and a row is
// formed only when a minibatch draws it (train.py:114-122: the DataLoader's shuffle over everything convert.py wrote;
// collect.py:64-131: what it wrote). window = {tail, head}: logical ply counters that only grow, physical slot =
// counter % cap_plies; [tail, head) holds whole games only (k_ring_retire), so a game may wrap around the physical end
// of the ring but is never cut by it.
#ifdef CCZ_BOUNDS
// the stateless ring kernels have no Dev: a stray index adds 65536 to the launch's *bad (tests ask for bad == 0) and goes to element 0
__device__ __forceinline__ long long ring_checked(int32_t *bad, long long i, long long n)
{
    if (i < 0 || i >= n) { if (bad) atomicAdd(bad, 65536); return 0; }
    return i;
}
#define CCZ_RING_IDX(bad_, i_, n_) ring_checked((bad_), (long long)(i_), (long long)(n_))
#else
#define CCZ_RING_IDX(bad_, i_, n_) (i_)
#endif

// Draw u of a window {tail, head}, as k_sample_records sees it: r = u % live (live = (head - tail) * mul rows, mul = 1 without
// mirror images), ply p = tail + r / mul, pass = r % mul. ok: the window and the draw are sane and the record is part of a
// whole game inside the window; else nothing more may be read. Nothing outside the ring is read either way.
struct SampledPly {
    bool ok;
    long long p, first;
    int pass;
    const uint8_t *rec;
    PlyHeader h;
};
__device__ __forceinline__ SampledPly locate_sampled_ply(const uint8_t *ring, long long cap_plies, const long long *window, long long u, long long mul,
                                                         int32_t *bad)
{
    SampledPly s = {};
    const long long tail = window[0], head = window[1];
    if (!(tail >= 0 && head > tail && head - tail <= cap_plies && u >= 0)) return s;
    const long long r = u % ((head - tail) * mul);
    s.p = tail + r / mul;
    s.pass = (int)(r % mul);
    s.rec = ring + (size_t)CCZ_RING_IDX(bad, s.p % cap_plies, cap_plies) * kRecBytes;
    s.h = *(const PlyHeader *)(s.rec + kRecHdr);
    s.first = s.p - s.h.t;
    s.ok = s.h.t < s.h.T && s.h.k <= kMaxLegal && s.first >= tail && s.first + s.h.T <= head; // a whole game inside the window
    return s;
}

// Output row j of a located draw, by the 256 threads of a block (s is block-uniform): exactly the bytes k_expand_records writes for
// that ply and pass (form_row), and in target / value (either may be null) the ply's policy-target byte and root value. A bad draw
// counts in *bad and its row is zeros, 0 and NaN. The ONE tail of k_sample_records and k_sample_records_weighted.
__device__ __forceinline__ void write_sampled_row(const uint8_t *ring, long long cap_plies, const SampledPly &s, long long j, uint32_t flags,
                                                  uint32_t typepack, uint8_t (*hist)[96], uint16_t *states, float *pi, float *z, int32_t *bad,
                                                  uint8_t *target, float *value)
{
    const int tid = threadIdx.x;
    const bool quirks = (flags & 1u) != 0;
    if (!s.ok) {
        uint32_t *srow = (uint32_t *)(states + (size_t)j * 10710);
        for (int i = tid; i < 5355; i += 256) srow[i] = 0u;
        for (int i = tid; i < kNMoves; i += 256) pi[(size_t)j * kNMoves + i] = 0.0f;
        if (tid == 0) {
            z[j] = 0.0f;
            write_side(target, value, j, 0, __builtin_nanf(""));
            if (bad) atomicAdd(bad, 1);
        }
        return;
    }
    // the game may wrap around the physical end of the ring
    stage_history(hist, ring, s.first, s.h, quirks, [&](long long q) { return CCZ_RING_IDX(bad, q % cap_plies, cap_plies); });
    form_row(RecordPly{hist, s.rec, s.h}, s.pass, quirks ? 1 : s.h.turn, typepack, states, pi, z, j);
    if (tid == 0) write_side(target, value, j, rec_target(s.h), rec_value(s.rec, s.h));
}

// One block per drawn row (locate_sampled_ply, write_sampled_row): output row blockIdx.x is that of draw draws[blockIdx.x].
// HBM-write-bound: 29.8 KB out, <= 1.6 KB in.
__global__ __launch_bounds__(256) void k_sample_records(const uint8_t *ring, long long cap_plies, const long long *window, const long long *draws,
                                                          long long batch, uint32_t flags, uint32_t typepack, uint16_t *states, float *pi,
                                                          float *z, int32_t *bad, uint8_t *target, float *value)
{
    const long long j = blockIdx.x;
    if (j >= batch) return;
    __shared__ __align__(16) uint8_t hist[8][96];
    const SampledPly s = locate_sampled_ply(ring, cap_plies, window, draws[j], (flags & 2u) ? 1 : 2, bad); // (block-uniform)
    write_sampled_row(ring, cap_plies, s, j, flags, typepack, hist, states, pi, z, bad, target, value);
}

// The ring draws by weight (include/cczero.h "policy surprise weighting"): one block per output row j, as above, but the block draws
// its own u by rejection. In round r = 0..3, lane l of the first wave takes the Philox4x32-10 words o of (key *seed, counter {hi = j,
// lo = 64 r + l}): candidate u = (o0:o1) >> 2 (62 bits), a = ((o2:o3) >> 11) * 2^-53 in [0, 1). It locates u (locate_sampled_ply),
// reads the ply's weight wq (uint16 at byte 90 of a CCZ_REC_WEIGHT record, else 4096 = 1.0) and accepts iff the candidate is ok and
// a * cap_q < wq. The lowest accepting (round, lane) wins by ballot; later rounds are not run. Nothing accepted in 256 candidates: the
// row takes candidate (0, 0) and *fallback counts it. The chosen u goes through LDS to the whole block and to chosen[j]; from there the
// row is what k_sample_records writes for draw u. Candidates that lose are counted nowhere, ok or not.
__global__ __launch_bounds__(256) void k_sample_records_weighted(const uint8_t *ring, long long cap_plies, const long long *window,
                                                                   const uint64_t *seed, int cap_q, long long *chosen, int32_t *fallback,
                                                                   long long batch, uint32_t flags, uint32_t typepack, uint16_t *states,
                                                                   float *pi, float *z, int32_t *bad, uint8_t *target, float *value)
{
    const long long j = blockIdx.x;
    const int tid = threadIdx.x;
    if (j >= batch) return;
    __shared__ __align__(16) uint8_t hist[8][96];
    __shared__ long long s_u;
    const long long mul = (flags & 2u) ? 1 : 2;
    if (tid < 64) {
        const uint64_t key = *seed;
        long long u00 = 0;
        bool found = false;
        for (int r = 0; r < 4 && !found; ++r) {
            uint32_t o[4];
            philox4x32(key, (uint64_t)j, (uint64_t)(r * 64 + tid), o);
            const long long u = (long long)((((uint64_t)o[0] << 32) | o[1]) >> 2);
            const double a = (double)((((uint64_t)o[2] << 32) | o[3]) >> 11) * 0x1p-53;
            if (r == 0) u00 = u; // (lane 0's is candidate (0, 0))
            const SampledPly c = locate_sampled_ply(ring, cap_plies, window, u, mul, bad);
            int wq = 4096;
            if (c.ok && (c.h.flags & kRecWeight)) wq = *(const uint16_t *)(c.rec + kRecWeightOff);
            const uint64_t hit = __ballot(c.ok && a * (double)cap_q < (double)wq);
            if (hit) {
                if (tid == __ffsll((long long)hit) - 1) s_u = u;
                found = true; // (wave-uniform: the ballot is)
            }
        }
        if (!found && tid == 0) {
            s_u = u00;
            if (fallback) atomicAdd(fallback, 1);
        }
    }
    __syncthreads();
    const long long u = s_u;
    if (tid == 0 && chosen) chosen[j] = u;
    const SampledPly s = locate_sampled_ply(ring, cap_plies, window, u, mul, bad); // (block-uniform)
    write_sampled_row(ring, cap_plies, s, j, flags, typepack, hist, states, pi, z, bad, target, value);
}

// After an append of logical plies [head_old, head_new) has been copied into the ring (it overwrote the slots of
// [head_old - cap, head_new - cap)): head = head_new, tail = max(tail, head_new - cap), and a tail that landed inside a
// game moves on to the start of the next one, so the window advances by WHOLE GAMES only. The record at tail is one the
// copy did not overwrite (tail >= head_new - cap), so this is race-free in stream order and needs no host sync. A game
// at the tail with more than max_game_plies plies is counted in *bad and skipped; so is a header that cannot be one
// (t >= T: the window is emptied). One thread; tail and head are written with ordinary vector stores.
__global__ void k_ring_retire(const uint8_t *ring, long long cap_plies, long long *window, long long head_new, int max_game_plies, int32_t *bad)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long tail = window[0];
    if (tail < head_new - cap_plies) tail = head_new - cap_plies;
    if (tail < 0) tail = 0;
    int nbad = 0;
    while (tail < head_new) {
        const PlyHeader h = *(const PlyHeader *)(ring + (size_t)CCZ_RING_IDX(bad, tail % cap_plies, cap_plies) * kRecBytes + kRecHdr);
        const int t = h.t, T = h.T;
        if (t >= T) { // not a ply header
            ++nbad;
            tail = head_new;
            break;
        }
        if (T > max_game_plies) ++nbad;
        else if (t == 0) break;
        tail += T - t; // to the start of the next game
    }
    if (tail > head_new) tail = head_new;
    if (nbad && bad) atomicAdd(bad, nbad);
    window[0] = tail;
    window[1] = head_new;
}

// ------------------------------------------------------------------ per-board simulation budgets
// budgets == nullptr: budgets off (unlimited, every move a policy target). An entry below 1 counts as 1: a board always searches.
__global__ void k_set_budgets(Dev D, int n, const int32_t *budgets, const uint8_t *targets)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    int v = 0x7fffffff;
    if (budgets) { v = budgets[b]; if (v < 1) v = 1; }
    D.budget[b] = v;
    D.target[b] = (budgets && targets) ? (uint8_t)(targets[b] != 0) : (uint8_t)1;
}

// Playout-cap randomisation: the move board b is about to search is a full one (n_full simulations, a policy target) with
// probability p_full, else a fast one (n_fast, no target). The uniform is word 0xffe of the board's Philox stream for this move:
// the Gamma draws use children 0..127 and the choice uniform 0xfff (sample_move), so the Dirichlet and move streams are untouched,
// and the draw is a function of (seed, global board id, move counter): independent of the GPU count.
__global__ void k_draw_budgets(Dev D, int n, int n_full, int n_fast, double p_full, int32_t *budgets_out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    double ua, ub;
    uniform2(D.seed, D.board_id_base + (uint64_t)b, D.meta[b].move_counter, 0xffeu, 0, ua, ub);
    const bool full = ua < p_full;
    const int v = full ? n_full : n_fast;
    D.budget[b] = v;
    D.target[b] = full ? 1 : 0;
    if (budgets_out) budgets_out[b] = v;
}

// ccz_set_resign: the settings reach the device in stream order, so they hold from the next k_finish_move on
__global__ void k_set_resign(ResignCfg *cfg, ResignCfg v)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *cfg = v;
}

// ccz_set_surprise: the settings reach the device in stream order; the has-bits of all n plies are cleared, so a ply recorded before the
// call carries no surprise whatever an earlier game left at its index
__global__ void k_set_surprise(SurpriseBlock *blk, SurpriseCfg v, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) blk->rec_hask[i] = 0;
    if (i == 0) blk->cfg = v;
}

// ccz_set_gumbel: the settings reach the device in stream order; every board's row is invalidated (n_eff and m may have changed)
__global__ void k_set_gumbel(GumbelCfg *cfg, GumbelCfg v, uint32_t *stamps, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stamps[i] = 0u;
    if (i == 0) *cfg = v;
}

// ccz_gumbel_sequence: seq(m, n) written out, one wave
__global__ __launch_bounds__(64) void k_gumbel_sequence(int m, int n, int32_t *seq)
{
    for (int t = threadIdx.x; t < n; t += 64) seq[t] = gumbel_seq_at(m, n, t);
}

// ccz_set_root_exploration: the settings reach the device in stream order; every board's noise row is invalidated (alpha may have changed)
__global__ void k_set_root_exploration(ExploreCfg *cfg, ExploreCfg v, uint32_t *stamps, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stamps[i] = 0u;
    if (i == 0) *cfg = v;
}

// ccz_set_search: the settings reach the device in stream order
__global__ void k_set_search(SearchCfg *cfg, SearchCfg v)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *cfg = v;
}

// ccz_set_early_stop: the settings reach the device in stream order; every board's stop and snapshot are dropped (the rules may have
// changed under them), so turning the feature on and off again leaves nothing behind
__global__ void k_set_early_stop(StopCfg *cfg, StopCfg v, uint8_t *stopped, int32_t *snap_s, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { stopped[i] = 0; snap_s[i] = -1; }
    if (i == 0) *cfg = v;
}

// ccz_searching: how many of the boards 0 .. n - 1 would still select a leaf -- the game running, the budget not spent, not stopped.
// One workgroup; the count is summed per wave and then over the waves in LDS.
__global__ __launch_bounds__(1024) void k_searching(Dev D, int n, int32_t *count)
{
    __shared__ int s_part[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool es = D.es_cfg->enabled != 0;
    int c = 0;
    for (int b = tid; b < n; b += 1024)
        c += (!D.meta[b].over && D.move_sims[b] < D.budget[b] && !(es && D.es_stopped[b])) ? 1 : 0;
    c = __builtin_amdgcn_readlane(wave_incl_scan(c, lane), 63);
    if (lane == 0) s_part[w] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int i = 0; i < 16; ++i) t += s_part[i];
        *count = t;
    }
}

// ------------------------------------------------------------------ MCTS-solver: settings, inspection, the combine rule on its own
// ccz_set_solver: the settings reach the device in stream order (the proof array is zeroed in front of this launch when it turns on)
__global__ void k_set_solver(SolverCfg *cfg, SolverCfg v)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *cfg = v;
}

// ccz_root_proof: the proof byte of every root and of its children, split into state and distance; zeros while the solver is off
__global__ __launch_bounds__(64) void k_root_proof(Dev D, uint8_t *state, uint8_t *dist, uint8_t *cstate, uint8_t *cdist)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const SolverCfg sv = *D.sv_cfg;
    const RootView rv = root_view(D, b);
    int k = root_k(rv) > kMaxLegal ? kMaxLegal : root_k(rv);
    if (!sv.enabled) k = 0;
    const uint8_t *proof = sv.proof + ((size_t)b * 2 + rv.half) * (size_t)D.cap;
    if (lane == 0) {
        const uint32_t p = sv.enabled ? proof[0] : 0u;
        state[b] = (uint8_t)(p & 3u);
        dist[b] = (uint8_t)(p >> 2);
    }
    for (int i = lane; i < kMaxLegal; i += 64) {
        const uint32_t p = i < k ? proof[CCZ_IDX(D, rv.root.fc + i, D.cap)] : 0u;
        cstate[(size_t)b * kMaxLegal + i] = (uint8_t)(p & 3u);
        cdist[(size_t)b * kMaxLegal + i] = (uint8_t)(p >> 2);
    }
}

// ------------------------------------------------------------------ value spread: settings, inspection, the LCB move
// ccz_set_value_stats: the word and the array's pointer reach the device in stream order (the array is zeroed in front of this launch
// when the option turns on). The solver's two members of the block are not touched; k_set_solver writes the word back as the host knows it.
__global__ void k_set_value_stats(SolverBlock *blk, int32_t spread, float *S)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { blk->cfg.spread = spread; blk->S = S; }
}

// ccz_root_value_stats: S of the root's children, aligned with k_root_children's acts (zero past k), and of the root; zero rows for
// a finished board and a slot past `active`
__global__ __launch_bounds__(64) void k_root_value_stats(Dev D, int active, float *s_out, float *root_s)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const BoardMeta m = D.meta[b];
    const SolverCfg sv = *D.sv_cfg;
    const RootView rv = root_view(D, b);
    int k = root_k(rv) > kMaxLegal ? kMaxLegal : root_k(rv);
    const bool live = sv.spread && !m.over && b < active;
    if (!live) k = 0;
    const float *S = live ? spread_array(D) + ((size_t)b * 2 + rv.half) * (size_t)D.cap : nullptr;
    if (lane == 0) root_s[b] = live ? S[0] : 0.0f;
    for (int i = lane; i < kMaxLegal; i += 64) s_out[(size_t)b * kMaxLegal + i] = i < k ? S[CCZ_IDX(D, rv.root.fc + i, D.cap)] : 0.0f;
}

// ccz_lcb_moves (the rule in full: include/cczero.h, "Value spread and the LCB move"): one wave per board, children `lane` and
// `64 + lane`; all arithmetic float64. moves / child: -1 for a finished board, a slot past `active`, a root without a visited child.
__global__ __launch_bounds__(64) void k_lcb_moves(Dev D, int active, double z, double min_ratio, int min_visits, int32_t *moves_out,
                                                    int32_t *child_out, double *lcb_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const BoardMeta m = D.meta[b];
    const SolverCfg sv = *D.sv_cfg;
    const RootView rv = root_view(D, b);
    int k = root_k(rv) > kMaxLegal ? kMaxLegal : root_k(rv);
    const bool live = sv.spread && !m.over && b < active;
    if (!live) k = 0;
    const float *S = live ? spread_array(D) + ((size_t)b * 2 + rv.half) * (size_t)D.cap : nullptr;
    const double ninf = -__builtin_huge_val();
    int N[2];
    double lcb[2];
    bool in[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = 64 * h + lane;
        in[h] = i < k;
        N[h] = 0;
        lcb[h] = ninf;
        if (in[h]) {
            const NodeA c = rv.A[CCZ_IDX(D, rv.root.fc + i, D.cap)];
            const double s = (double)S[CCZ_IDX(D, rv.root.fc + i, D.cap)];
            N[h] = c.N;
            if (c.N >= 2) {
                const double var = (s > 0.0 ? s : 0.0) / (double)(c.N - 1);
                const double se = sqrt(var / (double)c.N);
                const double zs = z * se;
                lcb[h] = (double)c.Q - zs;
            }
        }
        if (lcb_out) lcb_out[(size_t)b * kMaxLegal + i] = in[h] ? lcb[h] : 0.0;
    }
    const int best = gumbel_first_max((double)N[0], in[0], (double)N[1], in[1], lane); // i*: the first index of maximal N
    const int nmax = wave_max_i32(N[0] > N[1] ? N[0] : N[1]);
    int choice = -1;
    if (best >= 0 && nmax > 0) {
        bool el[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double need = min_ratio * (double)nmax;
            el[h] = in[h] && (64 * h + lane == best || (N[h] >= 2 && N[h] >= min_visits && (double)N[h] >= need));
            el[h] = el[h] && lcb[h] > ninf; // a bound of -inf is never chosen over i*: if nothing is left, i* it is
        }
        choice = gumbel_first_max(lcb[0], el[0], lcb[1], el[1], lane);
        if (choice < 0) choice = best;
    }
    if (lane == 0) {
        moves_out[b] = choice >= 0 ? (int32_t)(rv.Bn[CCZ_IDX(D, rv.root.fc + choice, D.cap)] & 0xffffu) : -1;
        if (child_out) child_out[b] = choice;
    }
}

// ccz_proof_combine: one wave per case, proof_combine on bytes[case][0 .. counts[case])
__global__ __launch_bounds__(64) void k_proof_combine(const uint8_t *bytes, const int32_t *counts, int n, uint8_t *out)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= n) return;
    int nc = counts[c];
    nc = nc < 0 ? 0 : (nc > kMaxLegal ? kMaxLegal : nc);
    const uint8_t *row = bytes + (size_t)c * kMaxLegal;
    const uint32_t p0 = lane < nc ? row[lane] : 0u, p1 = 64 + lane < nc ? row[64 + lane] : 0u;
    const uint32_t r = proof_combine(p0, p1, nc, lane);
    if (lane == 0) out[c] = (uint8_t)r;
}

// ------------------------------------------------------------------ stateless batch rules
__global__ __launch_bounds__(64) void k_legal_moves(int n, const uint8_t *sq, const uint8_t *turn, const int32_t *halfmove,
                                                      uint32_t *mask, int32_t *count, uint8_t *flags)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= n) return;
    __shared__ __align__(16) uint8_t s_sq[96];
    __shared__ GenScratch S;
    load_board(s_sq, sq + (size_t)b * 96, lane);
    __syncthreads();
    const int t = turn[b] ? 1 : 0;
    const GenResult g = gen_legal(s_sq, t, S, nullptr, lane);
    __syncthreads();
    if (mask) for (int w = lane; w < kMaskWords; w += 64) mask[(size_t)b * kMaskWords + w] = S.mask[w];
    if (lane == 0) {
        if (count) count[b] = g.n_legal;
        if (flags) {
            uint8_t f = 0;
            if (g.ksq >= 0 && king_attacked(s_sq, S, g.ksq, -1, -1, 0, t)) f |= 1;
            if (g.insufficient) f |= 2;
            if (halfmove && halfmove[b] >= 120 && g.n_legal > 0) f |= 4;
            if (g.overflow) f |= 128;
            flags[b] = f;
        }
    }
}

__global__ void k_apply_moves(int n, uint8_t *sq, uint8_t *turn, const int32_t *ids, uint8_t *captured)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    if (id < 0 || id >= kNMoves) return;
    uint8_t *s = sq + (size_t)i * 96;
    const int from = c_tab.from[id], to = c_tab.to[id];
    if (captured) captured[i] = s[to];
    s[to] = s[from];
    s[from] = 0;
    turn[i] ^= 1;
}

} // namespace ccz

namespace ccz {
// one thread, after k_finish_move: all live trees now sit in the other pool half

// ------------------------------------------------------------------ wide search: several leaves per board and step, with virtual loss
// (ccz_set_width / ccz_select_wide / ccz_step_wide; the rule is stated in cczero.h). One workgroup per searched board r. Wave 0 runs
// the cheap, inherently serial part -- phase A, the backups of the board's pending slots in slot order, then phase B's descents, each
// seeing the in-flight counts F the earlier ones left -- with one dependent load round per tree level, as select_phase has. The
// expensive part of a selection (replaying the path, move generation, game end, key, evaluator input row: leaf_tail) does not touch
// the tree, so the workgroup's NW waves then run the selected slots' tails side by side, each in its own SelectShared, like the scout
// waves of k_scouted_run. All hand-offs stay inside the workgroup (one CU, one L1): workgroup-scope fences and barriers.
// The options the wide search excludes (root exploration, Gumbel, solver, search parameters) are refused on the host: none is read.

// one descent under wide PUCT from the root of board r; returns the depth of the node it ends at (its path is written to `path`), or
// -1 after CCZ_ERR_NAN / CCZ_ERR_DEPTH. leafF <- the in-flight count of that node. All 64 lanes call it.
__device__ inline int wide_descend(const Dev &D, const NodeA *A, const uint32_t *Bn, const uint8_t *F, int32_t *path, int lane, int &leafF)
{
    NodeA pa = A[0];
    uint32_t nb = Bn[0];
    int pF = F[0];
    int depth = 0;
    if (lane == 0) path[0] = 0;
    for (;;) {
        const int nc = (int)(nb >> 16);
        if (nc == 0) break;
        const double sqrtNp = sqrt((double)(pa.N + pF));
        double best = -__builtin_huge_val();
        int besti = 0x7fffffff, bN = 0, bfc = -1, bFl = 0;
        float bQ = 0.0f;
        uint32_t bw = 0;
        for (int c0 = 0; c0 < nc; c0 += 64) {
            const int i = c0 + lane;
            if (i < nc) {
                const NodeA c = A[CCZ_IDX(D, pa.fc + i, D.cap)];
                const uint32_t w = Bn[CCZ_IDX(D, pa.fc + i, D.cap)];
                const int f = F[CCZ_IDX(D, pa.fc + i, D.cap)];
                const int ne = c.N + f;
                // every in-flight visit counts as one loss for the side that moved into the child; F = 0: the expression of select_phase
                double qe = (double)c.Q;
                if (f != 0) qe = ((double)c.N * (double)c.Q - (double)f) / (double)ne;
                const double sc = ne == 0 ? __builtin_huge_val() : qe + (double)(D.c_puct * c.P) * sqrtNp / (double)(1 + ne);
                if (sc > best) { best = sc; besti = i; bN = c.N; bQ = c.Q; bfc = c.fc; bw = w; bFl = f; }
            }
        }
        const double top = wave_max_f64(best);
        const bool hit = best == top && besti < nc;
        const uint64_t h0 = __ballot(hit && besti < 64), h1 = __ballot(hit);
        if (h1 == 0ull) { set_err(D, 32); return -1; } // NaN priors: no comparable child
        const int owner = __builtin_amdgcn_readfirstlane((h0 ? __ffsll((long long)h0) : __ffsll((long long)h1)) - 1);
        besti = __builtin_amdgcn_readlane(besti, owner);
        const int child = pa.fc + besti;
        pa.N = __builtin_amdgcn_readlane(bN, owner);
        pa.Q = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bQ), owner));
        pa.fc = __builtin_amdgcn_readlane(bfc, owner);
        nb = (uint32_t)__builtin_amdgcn_readlane((int)bw, owner);
        pF = __builtin_amdgcn_readlane(bFl, owner);
        ++depth;
        if (depth >= D.maxd) { set_err(D, 2); return -1; }
        if (lane == 0) path[CCZ_IDX(D, depth, D.maxd)] = child;
    }
    leafF = pF;
    return depth;
}

// F += delta on the nodes path[0 .. d] (distinct nodes: one lane each)
__device__ __forceinline__ void wide_count(const Dev &D, uint8_t *F, const int32_t *path, int d, int delta, int lane)
{
    for (int j = lane; j <= d; j += 64) {
        const int node = (int)CCZ_IDX(D, path[CCZ_IDX(D, j, D.maxd)], D.cap);
        F[node] = (uint8_t)((int)F[node] + delta);
    }
}

// what one wave hands the next phase of the same wave through global memory
__device__ __forceinline__ void wide_fence()
{
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_wide(Dev D, WideArgs wa, const float *value, uint16_t *leaf_in, int32_t *n_leaves, int backup)
{
    __shared__ SelectShared sh[NW];
    __shared__ int s_depth[64]; // slot j of this step: the depth of its selected leaf, -1: nothing selected
    __shared__ int s_undo[64];  // ... its tail refused the leaf (CCZ_ERR_CHAIN): the path leaves F again
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int A = wa.A, W = wa.W;
    const int half = *D.half;
    const size_t base = ((size_t)r * 2 + half) * (size_t)D.cap;
    uint8_t *F = wa.F + base;
    const BoardMeta m = D.meta[r];
    if (w == 0) {
        if (lane < 64) { s_depth[lane] = -1; s_undo[lane] = 0; }
        SolverCfg sv;
        sv.enabled = 0; sv.spread = 0; sv.proof = nullptr; // (both refuse a width above 1)
        int sims = D.move_sims[r];
        // ---- phase A: the pending slots are backed up in slot order
        if (backup) {
            BoardMeta mm = m;
            for (int j = 0; j < W; ++j) {
                const int s = r + j * A;
                const int d = D.path_len[s]; // (read before the backup: the slot's status decides whether it counts)
                const TopPatch tp = expand_backup_phase<true>(D, r, s, lane, D.prior128, value, mm, half, sv);
                if (tp.active) {
                    wide_count(D, F, D.path + (size_t)s * D.maxd, d, -1, lane);
                    if (tp.k > 0) mm.n_nodes = tp.n0 + tp.k;
                    ++sims;
                    wide_fence(); // the next slot's backup reads N, Q and F of shared path nodes from other lanes
                }
            }
        }
        // ---- phase B: up to W descents, each seeing the in-flight counts of the earlier ones
        const int budget = D.budget[r];
        const NodeA *An = D.nodeA + base;
        const uint32_t *Bn = D.nodeB + base;
        int t = 0;
        bool ended = m.over != 0;
        bool collided = false;
        for (int j = 0; j < W; ++j) {
            const int s = r + j * A;
            int32_t *path = D.path + (size_t)s * D.maxd;
            int d = -1;
            if (!ended && sims + t < budget) {
                int leafF = 0;
                d = wide_descend(D, An, Bn, F, path, lane, leafF);
                if (d < 0) ended = true; // (the slot gets SKIP below: the same byte as NONE)
                else if (leafF > 0) { ended = true; collided = true; d = -1; }
            }
            if (d < 0) {
                if (lane == 0) { D.leaf_status[s] = CCZ_LEAF_NONE; D.leaf_k[s] = 0; D.path_len[s] = 0; }
                continue;
            }
            wide_fence();                 // the path (lane 0's stores) is read by every lane
            wide_count(D, F, path, d, +1, lane);
            wide_fence();                 // ... and the counts by the next descent
            if (lane == 0) s_depth[j] = d;
            ++t;
        }
        if (lane == 0) {
            n_leaves[r] = t;
            WideBoardStats &ws = wa.stats[r];
            if (t > 0) ws.steps += 1;
            ws.leaves += (unsigned long long)t;
            if (collided) ws.collisions += 1;
        }
    }
    __threadfence_block(); // the selected slots' paths and the tree as backed up: read by every wave from here on
    __syncthreads();
    // ---- the leaf tails of the selected slots, one wave per slot (slots NW apart share a wave)
    for (int j = w; j < W; j += NW) {
        const int d = s_depth[j];
        if (d < 0) continue;
        const int s = r + j * A;
        SelectShared &S = sh[w];
        const int32_t *path = D.path + (size_t)s * D.maxd;
        const uint32_t *Bn = D.nodeB + base;
        if (lane < 24) {
            uint32_t v = ((const uint32_t *)(D.root_sq + (size_t)r * 96))[lane];
            if (lane == 22) v &= 0x0000ffffu;
            if (lane == 23) v = 0u;
            ((uint32_t *)S.sq)[lane] = v;
        }
        S.chain[lane] = D.chain[(size_t)r * kChainCap + lane];
        if (m.chain_len > 64) S.chain[64 + lane] = D.chain[(size_t)r * kChainCap + 64 + lane];
        for (int i = 1 + lane; i <= d; i += 64)
            S.pm.mv[i - 1] = (uint16_t)(Bn[CCZ_IDX(D, path[CCZ_IDX(D, i, D.maxd)], D.cap)] & 0xffffu);
        wave_sync();
        leaf_tail(D, s, lane, leaf_in, S, d, m.turn, m.halfmove, m.chain_len, m.key, true);
        if (lane == 0 && D.leaf_status[s] == CCZ_LEAF_SKIP) s_undo[j] = 1; // (lane 0 wrote the status itself)
        wave_sync(); // the next slot of this wave reuses the LDS block
    }
    __syncthreads();
    if (w == 0) {
        for (int j = 0; j < W; ++j)
            if (s_undo[j]) {
                const int s = r + j * A;
                wide_count(D, F, D.path + (size_t)s * D.maxd, s_depth[j], -1, lane);
                if (lane == 0) D.path_len[s] = 0;
                wide_fence();
            }
    }
}

// The move boundary of a wide engine: the pending leaves of board r's slots are dropped -- their paths leave F, the slots get
// CCZ_LEAF_NONE. Launched in front of the kernel that resets, re-roots or reloads the trees (between moves F is zero everywhere).
// only >= 0: that board alone; mask: as in k_reset. One thread per board: the slots of a board share path nodes.
__global__ void k_wide_drop(Dev D, WideArgs wa, const uint8_t *mask, int only)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= wa.A || (only >= 0 && r != only) || (mask && !mask[r])) return;
    uint8_t *F = wa.F + ((size_t)r * 2 + *D.half) * (size_t)D.cap;
    for (int j = 0; j < wa.W; ++j) {
        const int s = r + j * wa.A;
        if (D.leaf_status[s] != CCZ_LEAF_NONE) {
            const int32_t *path = D.path + (size_t)s * D.maxd;
            const int d = D.path_len[s];
            for (int i = 0; i <= d && i < D.maxd; ++i) {
                const int node = (int)CCZ_IDX(D, path[i], D.cap);
                F[node] = (uint8_t)(F[node] - 1);
            }
        }
        D.leaf_status[s] = CCZ_LEAF_NONE;
        D.leaf_k[s] = 0;
        D.path_len[s] = 0;
    }
}

// slots A .. B - 1 of an engine whose width was just set (ccz_set_width passes A = 0: every slot): no pending leaf
__global__ void k_wide_clear_slots(Dev D, int A)
{
    const int s = A + blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= D.B) return;
    D.leaf_status[s] = CCZ_LEAF_NONE;
    D.leaf_k[s] = 0;
    D.path_len[s] = 0;
}

// sum of F over the live pool half of the searched boards (ccz_get_wide_stats.inflight_now); *out is zeroed by the caller
__global__ __launch_bounds__(256) void k_wide_inflight(Dev D, WideArgs wa, unsigned long long *out)
{
    const uint8_t *F = wa.F + ((size_t)blockIdx.x * 2 + *D.half) * (size_t)D.cap;
    unsigned long long sum = 0;
    for (int i = threadIdx.x; i < D.cap; i += 256) sum += F[i];
    if (sum) atomicAdd(out, sum);
}

__global__ void k_flip_half(Dev D) { *D.half ^= 1; }
} // namespace ccz
