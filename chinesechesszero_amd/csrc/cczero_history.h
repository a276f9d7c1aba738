// cczero_history.h -- leaf history planes (ccz_set_leaf_history): the evaluator input a training row holds, at the leaf of the search.
//
// k_select / k_step write plane groups 7, 15 and 16 of a leaf's row (the reference's search passes no history, mcts.py:214); the rows
// the collector trains on (form_row, pass 0, default mode) show eight positions. With the option on the host launches k_leaf_history
// after every select phase: it rewrites the whole row of each board with a pending leaf to evaluate, and the board's cache key with
// it. The kernel reads what the select phase left (path, path_len, leaf_status, leaf_key) and the game record; it touches neither the
// trees nor any other kernel, and with the option off it is never launched.
#pragma once
#include "cczero_kernels.h"
#include "cczero_netops.h"

namespace ccz {

// 64-bit hash of the seven older history slots, oldest last: h_0 = kHistSeed, h_i = mix64(h_{i-1} ^ P(slot i)), P = the XOR of
// zob(piece, square) over the position's pieces (no side to move: it follows from the leaf's). The history key of a leaf is
// mix64(leaf_key ^ h_7). tests/leaf_history_model.py restates both.
constexpr uint64_t kHistSeed = 0x9E3779B97F4A7C15ull;

struct HistoryShared {
    __align__(16) uint32_t enc[5356];   // the whole row, 17 x 630 fp16 = 5355 dwords
    __align__(16) uint8_t ring[8][96];  // position S_idx lives in ring[idx & 7]
    __align__(16) uint8_t cur[96];      // the position the replay stands at
    uint8_t from[kMaxDepth], to[kMaxDepth];
};

// One wave per board. S_0 .. S_{p-1}: the recorded root positions of the board's game (p = meta.ply), S_p: the root, S_{p+1} ..
// S_{p+d}: the positions along the selection path (d = path_len). With te = p + d, slot i shows S_{max(te - i, 0)} (HarvestPly::sq's
// clamp); red pieces of slot i go to group i, black ones to group 8 + i, group 16 is the side to move at the leaf.
__global__ __launch_bounds__(64) void k_leaf_history(Dev D, uint16_t *leaf_in)
{
    __shared__ HistoryShared sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    // boards without a pending leaf to evaluate (terminal, proven, finished, stopped, budget spent) keep their row and key
    if (__builtin_amdgcn_readfirstlane((int)D.leaf_status[b]) != CCZ_LEAF_EXPAND) return;
    const BoardMeta m = D.meta[b];
    const int d = __builtin_amdgcn_readfirstlane(D.path_len[b]), p = __builtin_amdgcn_readfirstlane(m.ply);
    if (d < 0 || d >= D.maxd || p < 0 || p > D.max_plies) return; // (never: the select phase and k_finish_move keep both in range)
    const int te = p + d, lo = te > 7 ? te - 7 : 0;

    // ---- one load round: the root mailbox, the path's move ids, the recorded positions lo .. p - 1 (at most seven)
    if (lane < 24) {
        uint32_t v = ((const uint32_t *)(D.root_sq + (size_t)b * 96))[lane];
        if (lane == 22) v &= 0x0000ffffu;
        if (lane == 23) v = 0u;
        ((uint32_t *)sh.cur)[lane] = v;
    }
    {
        const size_t base = ((size_t)b * 2 + *D.half) * (size_t)D.cap;
        const int32_t *path = D.path + (size_t)b * D.maxd;
        for (int j = lane; j < d; j += 64) {
            int node = path[j + 1];
            node = node < 0 ? 0 : (node >= D.cap ? D.cap - 1 : node);
            int mv = (int)(D.nodeB[base + node] & 0xffffu);
            if (mv >= kNMoves) mv = 0;
            sh.from[j] = c_tab.from[mv];
            sh.to[j] = c_tab.to[mv];
        }
    }
    for (int idx = lo; idx < p; ++idx)
        if (lane < 24) ((uint32_t *)sh.ring[idx & 7])[lane] = ((const uint32_t *)(D.rec_sq + ((size_t)b * D.max_plies + idx) * 96))[lane];
    wave_sync();

    // ---- replay: the moves in front of the first position that is shown by one lane in one go, then position by position
    const int j0 = lo > p ? lo - p : 0;
    if (lane == 0) {
        for (int j = 0; j < j0; ++j) {
            const int fr = sh.from[j], to = sh.to[j];
            sh.cur[to] = sh.cur[fr];
            sh.cur[fr] = 0;
        }
    }
    wave_sync();
    for (int j = j0; j <= d; ++j) { // at most eight rounds
        if (lane < 24) ((uint32_t *)sh.ring[(p + j) & 7])[lane] = ((const uint32_t *)sh.cur)[lane];
        wave_sync();
        if (j < d && lane == 0) {
            const int fr = sh.from[j], to = sh.to[j];
            sh.cur[to] = sh.cur[fr];
            sh.cur[fr] = 0;
        }
        wave_sync();
    }

    // ---- the history key: the evaluator input is a function of the leaf's key and of slots 1..7, and so is the cache key
    uint64_t h = kHistSeed;
#pragma unroll 1
    for (int i = 1; i < 8; ++i) {
        const uint8_t *r = sh.ring[(te - i > 0 ? te - i : 0) & 7];
        const int q0 = r[lane], q1 = lane < 26 ? r[64 + lane] : 0;
        uint64_t x = 0;
        if (q0 & 7) x ^= zob(q0 & 15, lane);
        if (q1 & 7) x ^= zob(q1 & 15, 64 + lane);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
        h = mix64(h ^ x);
    }
    if (lane == 0) D.leaf_key[b] = mix64(D.leaf_key[b] ^ h);

    // ---- the row, staged in LDS: fill (zeros / the turn plane), one fp16 1.0 per piece and slot, stream out as dwords
    const int turn = (int)m.turn ^ (d & 1);
    const uint32_t tv = turn ? 0x3C003C00u : 0u;
    for (int i = lane; i < 5355; i += 64) sh.enc[i] = i >= 5040 ? tv : 0u;
    wave_sync();
    {
        uint16_t *eh = (uint16_t *)sh.enc;
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            const uint8_t *r = sh.ring[(te - i > 0 ? te - i : 0) & 7];
            const int q0 = r[lane], q1 = lane < 26 ? r[64 + lane] : 0;
            if (q0 & 7) eh[(((q0 >> 3) & 1) * 8 + i) * 630 + plane_of(D, q0 & 7) * 90 + lane] = kHalfOne;
            if (q1 & 7) eh[(((q1 >> 3) & 1) * 8 + i) * 630 + plane_of(D, q1 & 7) * 90 + 64 + lane] = kHalfOne;
        }
    }
    wave_sync();
    uint32_t *row = (uint32_t *)(leaf_in + (size_t)b * 10710);
    for (int i = lane; i < 5355; i += 64) row[i] = sh.enc[i];
}

// ---- the evaluator's side: all 119 planes of a row as NHWC rows of 128 channels (119 + 9 zeros), the input of the 128-channel stem.
// k_pack_live_planes with every plane: one wave per board, the board's 21,420 B staged in LDS with dword loads and transposed from
// there, 16 chunks of 16 bytes per pixel. rows / n_rows / flags bit 0 (group-of-16 rows) as there; every chunk is always written.
__global__ __launch_bounds__(kPackThreads) void k_pack_planes128(const _Float16 *__restrict__ leaf, half8_t *__restrict__ out, int n_boards,
                                                                 const int *__restrict__ rows, const int *__restrict__ n_rows, int flags)
{
    __shared__ uint32_t s_w[5356];
    const long b = blockIdx.x;
    const int lane = threadIdx.x;
    long sb = b;
    if (rows) {
        const int nr = *n_rows;
        sb = rows[b];
        if (b >= nr) return;
        if (sb < 0 || sb >= n_boards) return; // (never: the plan names boards of the batch)
    }
    const uint32_t *src = (const uint32_t *)(leaf + sb * (119 * 90));
    for (int i = lane; i < 5355; i += kPackThreads) s_w[i] = src[i];
    __syncthreads(); // (one wave: only the wait for the LDS writes)
    const _Float16 *s_h = (const _Float16 *)s_w; // channel ch (0..118), pixel p at s_h[ch * 90 + p]
    const bool g16 = flags & 1;
    for (int i = lane; i < 90 * 16; i += kPackThreads) {
        const int p = i >> 4, cpos = i & 15;
        half8_t o = (half8_t)(_Float16)0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ch = cpos * 8 + e;
            if (ch < 119) o[e] = s_h[ch * 90 + p];
        }
        const long row = g16 ? ((b >> 4) * 90 + p) * 16 + (b & 15) : b * 90 + p;
        out[row * 16 + cpos] = o;
    }
}

} // namespace ccz
