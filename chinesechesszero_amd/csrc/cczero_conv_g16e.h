// cczero_conv_g16e.h -- the EDGE tiles of the group-of-16 tower convolution (round 4).
//
// k_conv3x3_g16 (cczero_conv_g16.h) cuts a 16-board group into five tiles of two ranks. The first tile has no rank above its first
// rank, the last none below its second: there the wave row that owns the edge rank multiplies zeroed slab rows in three of the nine
// taps -- 6.7 % of all MFMAs -- and nothing cheap removes them: which wave it is, is a run-time property (tile class x wave row), a
// branch around the MFMAs costs the kernel its register allocation (256 of 256, no slack), and hidden in inline asm it is 34 %
// slower (profiles/r04_conv_g16.json). This kernel makes the dead taps a COMPILE-TIME property of a tile instead:
//
//   * an edge tile = the SAME edge rank (rank 0, or rank 9) of TWO groups: wave row 0 owns it for group A, wave row 1 for group B.
//     Both wave rows then lose the same three taps (rank 0: dy = -1, rank 9: dy = +1): a chunk is SIX half-steps -- six weight
//     half-tiles, six barriers, 192-208 MFMAs per wave -- instead of nine, and no slab row is ever zeroed.
//   * top and bottom run the same code: the slab of a wave row holds ITS group's two ranks next to the edge (ranks 0, 1 resp. 8, 9)
//     as sub-ranks 0 and 1; the six live taps read sub-rank 0 in their first three half-steps and sub-rank 1 in the last three
//     (top: dy = 0 then +1; bottom: dy = -1 then 0 -- ascending tap order either way: each accumulator adds the same products in
//     the same order as in the other kernels); what differs is a run-time tap offset into the packed weights and the row offsets.
//   * the other eight ranks of a group are four ordinary two-rank tiles of k_conv3x3_g16 (mode 1: ranks 1-2, 3-4, 5-6, 7-8, every
//     neighbour rank exists). Per pair of groups: 8 + 2 tiles where there were 10, the two edge tiles ~30 % shorter.
//   * it is a second kernel (its own register allocation: 256 VGPRs, no spill) and therefore a second launch per layer, right behind
//     the middle launch in the same stream (csrc/cczero.hip conv3x3_launch: no gap between the two in the kernel trace).
//
// Everything else -- ring of five weight half-tiles three ahead, one raw s_barrier per half-step with counted vmcnt, pixel fragments
// shared by the three dx taps of a dy and refilled in place, LDS-transposed epilogue -- is k_conv3x3_g16's. The next chunk's slab
// is staged in half-steps 0-2 (2 + 2 + 1 pieces) instead of taps 1-5: its first fragments are read in half-step 5.
// The DMA goes through k_conv3x3_g16's buffer descriptors; past the last chunk the prefetches are issued against zero records.
#pragma once
#include "cczero_conv_g16.h"

namespace ccz {

__host__ __device__ constexpr int g5e_nslab(int h) { return h == 0 ? 2 : h == 1 ? 2 : h == 2 ? 1 : 0; } // slab pieces issued in half-step h
// DMA loads younger than the weight half-tile the NEXT half-step reads (issue order per half-step: slab pieces, 2 weight loads)
__host__ __device__ constexpr int g5e_dma(int h) { return 2 + g5e_nslab(h); } // DMA loads a thread issues in half-step h, past the last chunk as well
__host__ __device__ constexpr int g5e_vmcnt(int h) { return g5e_dma(h) + g5e_dma((h + 5) % 6); }
static_assert(g5e_vmcnt(0) == 6 && g5e_vmcnt(1) == 8 && g5e_vmcnt(2) == 7 && g5e_vmcnt(3) == 5 && g5e_vmcnt(4) == 4 && g5e_vmcnt(5) == 4, "g5e_vmcnt table");
static_assert(g5e_dma(0) == 4 && g5e_dma(1) == 4 && g5e_dma(2) == 3 && g5e_dma(3) == 2 && g5e_dma(4) == 2 && g5e_dma(5) == 2,
              "17 DMA loads per chunk and thread: 5 slab pieces + 6 x 2 weight pieces");

// One half-step of an edge tile: live tap H = J % 6 of a 32-channel chunk (tap index H + toff in the packed weights), J = its
// index inside the unrolled pair of chunks (A register set = J & 1, slab buffer = J / 6). vb[BUF] = this lane's fragment base of
// the wave row's sub-rank 0 in slab buffer BUF; sub-rank d = H / 3 is at + 9 * 1024 d.
template <int J, bool CM = false>
__device__ __forceinline__ void g5e_step(const G5Ctx &c, cv_f32x4 (&acc)[4][9], int chunk, int &ring_rd, int &ring_wr,
                                          cv_half8 (&a0)[4], cv_half8 (&a1)[4], cv_half8 (&b)[9], int toff)
{
    constexpr int H = J % 6, BUF = J / 6;
    constexpr int Hn = (H + 1) % 6, BUFn = (H == 5) ? 1 - BUF : BUF;
    cv_half8 (&acur)[4] = (J & 1) ? a1 : a0;
    cv_half8 (&anxt)[4] = (J & 1) ? a0 : a1;
    unsigned char *const lds = c.lds;
    // as in g5_step: the nine fragments of a sub-rank serve its three dx taps (cell N multiplies b[N + dx]) and are refilled in
    // place for the next sub-rank during the dx = +1 tap; the order is pinned, one scheduling region per cell
#define G5_REFILL(N) ((Hn / 3) * 9 + N)
    constexpr int H2 = (H + kG5Ahead) % 6;
    // past the last chunk: as in g5_step, the loads are issued against descriptors of zero records and fetch nothing
    const int chunk2 = chunk + (H + kG5Ahead >= 6 ? 1 : 0);
    G5_CELLS(H, 0, 1)
    if constexpr (g5e_dma(H) > 2) { // the next chunk's slab: passes 0,1 | 2,3 | 4 in half-steps 0 | 1 | 2
        constexpr int p0 = H * 2;
        const unsigned so = (unsigned)((chunk + 1) * (CM ? kG16CChunk : 64));
        const unsigned live = chunk < c.cmask ? (p0 < 4 ? c.xbytes : c.xbytes_part) : 0u;
        cv_blds16(c.X, live, c.xoff[p0], so,
                  lds + (p0 < 4 ? kG5AOff + (1 - BUF) * kG5SlabBytes + p0 * 8192 + c.wave_dst : c.wave_dst_part + (1 - BUF) * c.wave_step_part));
        if constexpr (g5e_dma(H) > 3)
            cv_blds16(c.X, live, c.xoff[p0 + 1], so, lds + kG5AOff + (1 - BUF) * kG5SlabBytes + ((p0 + 1) * 8192 + c.wave_dst));
        __builtin_amdgcn_sched_barrier(0);
    }
    G5_CELLS(H, 1, 2)
    {
        const unsigned wlive = chunk2 <= c.cmask ? c.wbytes : 0u;
        const unsigned so = (unsigned)((H2 + toff + 9 * chunk2) * (2 * 8192)); // half-tile (chunk2, tap H2 + toff): one contiguous 16 KB block
        unsigned char *const d = lds + ring_wr * kG5WBytes + c.wave_dst;
        cv_blds16(c.W, wlive, c.woff, so, d);
        __builtin_amdgcn_sched_barrier(0);
        G5_CELLS(H, 2, 3)
        cv_blds16(c.W, wlive, c.woff, so + 8192u, d + 8192);
        __builtin_amdgcn_sched_barrier(0);
    }
    G5_CELLS(H, 3, kG5Split)

    ring_rd = ring_rd + 1 == kG5Ring ? 0 : ring_rd + 1;
    cv_wait_vm<g5e_vmcnt(H)>();
    g5_barrier();

    {
        const unsigned char *wa = lds + (ring_rd * kG5WBytes + c.a_off);
#pragma unroll
        for (int i = 0; i < 4; ++i) anxt[i] = *(const cv_half8 *)(wa + i * 1024);
        __builtin_amdgcn_sched_barrier(0);
    }
    G5_CELLS(H, kG5Split, 9)
    ring_wr = ring_wr + 1 == kG5Ring ? 0 : ring_wr + 1;
#undef G5_REFILL
}

// X, Y, R: rows in the group-of-16 layout, M rows (a multiple of 1440); W packed (k_pack_conv_weights_g16). grid = 2 * ceil(groups
// / 2): workgroup e = pair e / 2 of groups, side e & 1 (0: rank 0, 1: rank 9). live_rows / row0: as k_conv3x3_g16 (planned boundary).
// `lds`, `blk`: the workgroup's LDS and edge-tile slot (as g5_tile).
template <bool RES, bool HEADS, bool CM = false>
__device__ __forceinline__ void g5e_tile(unsigned char *lds, int blk, const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                         const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                         int relu, int cin, const int *live_rows, int row0, const G5Heads &ha)
{
    [[maybe_unused]] long first_board = 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q4 = lane >> 4;
    const int wm = w & 3, wn = w >> 2;
    int groups = M / 1440;
    if (live_rows) { // the same cut of the live groups into n_parts equal ranges as k_conv3x3_g16
        int first;
        groups = g5_live_groups(live_rows, row0, groups, first);
        g5_live_part<RES, HEADS>(first, cin, X, R, Y, first_board);
    }
    const int e = __builtin_amdgcn_readfirstlane(blk);
    if (e >= 2 * ((groups + 1) >> 1)) return;
    const int side = e & 1, gA = (e >> 1) * 2;
    const bool dup = gA + 1 >= groups;                       // an odd group count: the last pair is one group twice (wave row 1 stores nothing)
    const int gB = dup ? gA : gA + 1;
    const int toff = __builtin_amdgcn_readfirstlane(side ? 0 : 3); // bottom: taps 0..5 (dy = -1, 0); top: taps 3..8 (dy = 0, +1)
    const long srcA = (long)gA * 1440 + (side ? 8 : 0) * 144;      // the two ranks next to the edge: slab sub-ranks 0, 1
    const long srcB = (long)gB * 1440 + (side ? 8 : 0) * 144;
    const long outA = (long)gA * 1440 + (side ? 9 : 0) * 144;      // the edge rank itself
    const long outB = (long)gB * 1440 + (side ? 9 : 0) * 144;
    relu &= 1;

    G5Ctx c;
    g5_ctx_common(c, lds, X, W, w, (unsigned)groups * (1440u * 2u) * (unsigned)cin, cin, cin >> 5);
    c.wave_dst_part = w < 4 ? kG5AOff + 4 * 8192 + w * 1024 : kG5Dump + w * 1024;
    c.wave_step_part = w < 4 ? kG5SlabBytes : 0;
    c.xbytes_part = w < 4 ? c.xbytes : 0u;
    {
        // slab row sr: 0..287 = group A's rows srcA + sr, 288..575 = group B's; 64-byte rows, position pos of row sr holds source
        // chunk pos ^ f(sr), f = (-(sr >> 2)) & 3 (the swizzle of k_conv3x3_g16)
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const int piece = (it < 4 || w < 4) ? it * 512 + tid : 3 * 512 + tid; // (waves 4-7 in pass 4: any offset, xbytes_part = 0)
            const int sr = piece >> 2, pos = piece & 3;
            const int schunk = pos ^ ((0 - (sr >> 2)) & 3);
            const long p = sr < 288 ? srcA + sr : srcB + (sr - 288);
            if constexpr (CM) c.xoff[it] = g16c_off(p) + (unsigned)(schunk * 16);
            else c.xoff[it] = (unsigned)(p * cin + schunk * 8) * 2u;
        }
        c.woff = (unsigned)(tid * 16);
    }
    // ---- prologue: slab of chunk 0, weight half-tiles of the first three live taps
#pragma unroll
    for (int it = 0; it < 5; ++it)
        cv_blds16(X, it < 4 ? c.xbytes : c.xbytes_part, c.xoff[it], 0u, lds + (it < 4 ? kG5AOff + it * 8192 + c.wave_dst : c.wave_dst_part));
#pragma unroll
    for (int u = 0; u < kG5Ahead; ++u) {
        unsigned char *d = lds + u * kG5WBytes + c.wave_dst;
        cv_blds16(W, c.wbytes, c.woff, (unsigned)((u + toff) * 2 * 8192), d);
        cv_blds16(W, c.wbytes, c.woff, (unsigned)((u + toff) * 2 * 8192 + 8192), d + 8192);
    }
    g5_ctx_frags(c, r, q4, wm, wn * 18, kG5AOff, kG5SlabBytes); // slab cell 18 wn + 9 d + n

    cv_f32x4 acc[4][9];
#pragma unroll
    for (int i = 0; i < 4; ++i) g5_acc_row_from_bias(acc[i], bias + wm * 64 + i * 16 + 4 * q4);

    cv_wait_vm<4>();
    g5_barrier();

    int ring_rd = 0, ring_wr = kG5Ahead;
    cv_half8 a0[4], a1[4], b[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) a0[i] = *(const cv_half8 *)(lds + c.a_off + i * 1024);
#pragma unroll
    for (int n = 0; n < 9; ++n) b[n] = *(const cv_half8 *)(lds + c.vb[0] + n * 1024); // sub-rank 0
    for (int chunk = 0; chunk <= c.cmask; chunk += 2) {
#define G5E_S(j) g5e_step<j, CM>(c, acc, chunk + (j) / 6, ring_rd, ring_wr, a0, a1, b, toff)
        G5E_S(0); G5E_S(1); G5E_S(2); G5E_S(3); G5E_S(4); G5E_S(5);
        G5E_S(6); G5E_S(7); G5E_S(8); G5E_S(9); G5E_S(10); G5E_S(11);
#undef G5E_S
    }
    cv_wait_vm<0>(); // the out-of-range DMA loads (zeros) must have landed before the LDS is reused / released

    // ---- epilogue (k_conv3x3_g16's): the [row][channel] image in LDS, rows 0..143 = group A's edge rank, 144..287 = group B's;
    // wave w owns image rows 36 w .. 36 w + 35 and moves whole 512-byte rows (residual in, output out). The rows go out under the
    // store predicate in this tile's own copy of g5_rows_out (cczero_conv_g16.h: why)
    g5_barrier();
    g5_image_store<kG5ERow>(lds, acc, wm, wn, r, q4);
    const int prow = lane >> 5, piece = lane & 31;
    const long pbase = (w < 4 ? outA : outB) + (w & 3) * 36 + prow;
    const bool store = !(dup && w >= 4);
    cv_half8 rv[18];
    if constexpr (CM) { // wave w owns chunk w of the 18 cells (g5c_rows_out): cells 0..8 group A's edge rank, 9..17 group B's
        const int erow = g16c_lane_row(lane), ep = lane & 3;
        const size_t yoA = (size_t)g16c_off(outA + erow) + (size_t)(w * kG16CChunk + ep * 16);
        const size_t yoB = (size_t)g16c_off(outB + erow) + (size_t)(w * kG16CChunk + ep * 16);
        if (RES) {
#pragma unroll
            for (int it = 0; it < 18; ++it) rv[it] = *(const cv_half8 *)((const unsigned char *)R + (it < 9 ? yoA + it * 1024 : yoB + (it - 9) * 1024));
        }
        g5_barrier<true>();
        const cv_half8 zero = (cv_half8)(_Float16)0;
        unsigned char *eb = lds + erow * kG5ERow + w * 64 + ep * 16;
#pragma unroll
        for (int it = 0; it < 18; ++it) {
            if (it < 9 || !dup) {                                            // (wave-uniform: with `dup` group B is group A again)
                cv_half8 v = *(const cv_half8 *)(eb + it * 16 * kG5ERow);
                if (RES) v = v + rv[it];
                if (relu) v = __builtin_elementwise_max(v, zero);
                if constexpr (HEADS) *(cv_half8 *)(eb + it * 16 * kG5ERow) = v;
                else *(cv_half8 *)((unsigned char *)Y + (it < 9 ? yoA + it * 1024 : yoB + (it - 9) * 1024)) = v;
            }
        }
    } else {
        if (RES) {
#pragma unroll
            for (int it = 0; it < 18; ++it) rv[it] = *(const cv_half8 *)(R + (pbase + it * 2) * kCvC + piece * 8);
        }
        g5_barrier<true>();
        if (store) {
            const cv_half8 zero = (cv_half8)(_Float16)0;
            unsigned char *eb = lds + (w * 36 + prow) * kG5ERow + piece * 16;
#pragma unroll
            for (int it = 0; it < 18; ++it) {
                cv_half8 v = *(const cv_half8 *)(eb + it * 2 * kG5ERow);
                if (RES) v = v + rv[it];
                if (relu) v = __builtin_elementwise_max(v, zero);
                if constexpr (HEADS) *(cv_half8 *)(eb + it * 2 * kG5ERow) = v;   // the finished row stays in the image; Y is not written
                else *(cv_half8 *)(Y + (pbase + it * 2) * kCvC + piece * 8) = v;
            }
        }
    }
    if constexpr (HEADS) { // the heads on the finished rows (cczero_conv_g16.h g5_heads_phase): image rows 0..143 group A's edge rank, 144..287 group B's
        g5_barrier<true>();
        const long board0[2] = {first_board + (long)gA * 16, first_board + (long)gB * 16};
        const int pos0[2] = {side ? 81 : 0, side ? 81 : 0};
        g5_heads_phase(lds, w, lane, ha, board0, pos0, dup);
    }
}

template <bool RES>
__global__ __launch_bounds__(512) void k_conv3x3_g16_edge(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                            const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                                            int relu, int cin, const int *live_rows, int row0)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    g5e_tile<RES, false>(lds, blockIdx.x, X, W, bias, R, Y, M, relu, cin, live_rows, row0, G5Heads{});
}

__global__ __launch_bounds__(512) void k_conv3x3_g16_edge_heads(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                                  const float *__restrict__ bias, const _Float16 *R, _Float16 *Y,
                                                                  int M, int relu, int cin, const int *live_rows, int row0, G5Heads ha)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    if (live_rows) ha.nb = *live_rows; // planned boundary: the pointers are the whole batch's, M only the capacity of this part
    g5e_tile<true, true>(lds, blockIdx.x, X, W, bias, R, Y, M, relu, cin, live_rows, row0, ha);
}

// CCZ_CONV_G16_ONE_LAUNCH: the middle tiles AND the edge-pair tiles of a layer in ONE launch. The two classes are independent (the
// middle tiles write ranks 1..8, the edge tiles ranks 0 and 9, both read only the layer's input and their own residual rows), so
// nothing orders them inside a layer; as two launches in a chain's stream the edge launch waited for the middle launch's last tile,
// and every chain-layer paid two dependent-launch tails instead of one. Slots [0, 4 g) are the middle tiles of the g live groups
// (k_conv3x3_g16 flag bit 2, same XCD-aware order), slots [4 g, 4 g + 2 ceil(g / 2)) the edge pairs: they are dispatched last, and
// being ~24 % shorter they fill the launch's last round. Each tile is the same code as in its own kernel (the branch is taken once,
// before either body starts): the same values. grid = 4 groups + 2 ceil(groups / 2) of the capacity; slots past the live ones leave.
// Not for the last layer: with the heads in the epilogue both bodies in one kernel spill (one VGPR); it stays two launches.
template <bool RES, bool QUAD, bool CM = false>
__device__ __forceinline__ void g5_one_launch(unsigned char *lds, const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                              const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                              int relu, int cin, const int *live_rows, int row0)
{
    int groups = M / 1440;
    if (live_rows) {
        int first;
        groups = g5_live_groups(live_rows, row0, groups, first);
    }
    const int mid = groups * 4, blk = blockIdx.x;
    if (blk < mid) {
        if constexpr (QUAD) g5q_tile<RES, CM>(lds, blk, mid, X, W, bias, R, Y, M, relu, cin, live_rows, row0);
        else g5_tile<RES, false>(lds, blk, mid, X, W, bias, R, Y, M, relu | 4, cin, live_rows, row0, G5Heads{});
    } else g5e_tile<RES, false, CM>(lds, blk - mid, X, W, bias, R, Y, M, relu, cin, live_rows, row0, G5Heads{});
}

template <bool RES>
__global__ __launch_bounds__(512) void k_conv3x3_g16_one(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                           const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                                           int relu, int cin, const int *live_rows, int row0)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    g5_one_launch<RES, false>(lds, X, W, bias, R, Y, M, relu, cin, live_rows, row0);
}

// The same with the middle slots as QUAD tiles (CCZ_CONV_G16_QUAD, cczero_conv_g16.h g5q_tile): slot t of group g = quad t >> 1, channel half t & 1
template <bool RES>
__global__ __launch_bounds__(512) void k_conv3x3_g16_one_quad(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                                const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                                                int relu, int cin, const int *live_rows, int row0)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    g5_one_launch<RES, true>(lds, X, W, bias, R, Y, M, relu, cin, live_rows, row0);
}

// The G16C forms (cczero_conv_g16.h g16c_off): every activation tensor of the layer chunk-major
template <bool RES>
__global__ __launch_bounds__(512) void k_conv3x3_g16c_one_quad(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                                 const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                                                 int relu, int cin, const int *live_rows, int row0)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    g5_one_launch<RES, true, true>(lds, X, W, bias, R, Y, M, relu, cin, live_rows, row0);
}

__global__ __launch_bounds__(512) void k_conv3x3_g16c_edge_heads(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                                   const float *__restrict__ bias, const _Float16 *R, _Float16 *Y,
                                                                   int M, int relu, int cin, const int *live_rows, int row0, G5Heads ha)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    if (live_rows) ha.nb = *live_rows;
    g5e_tile<true, true, true>(lds, blockIdx.x, X, W, bias, R, Y, M, relu, cin, live_rows, row0, ha);
}

#undef G5_CELLS
#undef G5_CELL

} // namespace ccz
