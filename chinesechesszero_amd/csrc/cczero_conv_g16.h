// cczero_conv_g16.h -- the tower convolution for LARGE batches: group-of-16 activation layout, whole-rank tiles.
//
//   y[p, co] = relu( bias[co] + sum_{tap, ci} w[co, tap, ci] * x[p + 9*dy + dx, ci]  [+ res[p, co]] )
//
// (reference net.py:20-43: conv3x3 -> BN -> [+x] -> ReLU with BN folded into w / bias.) k_conv3x3_c256 (cczero_conv.h) works on
// NHWC rows in board order; 110 of the 810 (pixel, tap) pairs of a 10 x 9 board point off the board and it multiplies a zero row
// for them, because 16 consecutive pixels of ONE board never have the same tap off the board. This kernel changes what the
// 16 columns of an MFMA block are:
//
//   * layout "G16" (CCZ_CONV_G16): activation row = (g * 90 + pos) * 16 + j for board 16 g + j -- 16 consecutive rows = one
//     board position ("cell") of 16 boards = one 16-column MFMA block: a tap is on the board for all 16 columns or for none.
//   * tile = 2 whole ranks of one 16-board group = 18 cells = 288 rows x all 256 output channels; 5 tiles per group,
//     4096 boards = 1280 tiles = 5.0 rounds on 256 CUs (k_conv3x3_c256: 1440 tiles of 256 rows = 5.6 rounds).
//   * 8 waves = 4 (64 output channels) x 2 (one rank = 9 cells each): 4 x 9 accumulator tiles per wave (144 VGPRs). The file
//     of a cell is a compile-time constant of the accumulator tile: a tap with dx = -1 skips cell 0, dx = +1 skips cell 8 --
//     32 instead of 36 MFMAs in six of nine taps, the same for every wave, so nothing of it is lost at the barrier (-7.4 %
//     MFMAs). The slab rows of the ranks above rank 0 and below rank 9 are zeroed once per chunk by the threads that staged
//     them, so dy needs no test. No per-lane validity flags, no v_cndmask, no per-tap address arithmetic: every LDS address
//     in the loop is a lane constant + an immediate.
//   * weights come PACKED (k_pack_conv_weights_g16 / ccz_pack_conv_weights_g16_f16, once per weight set): [ci / 32][tap][co][32]
//     with the LDS swizzle already applied, so that a half-tile is one contiguous 16 KB block.
//   * K order = chunks of 32 input channels x 9 taps (one MFMA k-step each; all three convolution kernels add in this order,
//     so their results are the same values -- up to the sign of a zero, where this one skips a product of zeros): 72
//     half-steps per tower layer, one weight half-tile (256 output channels x 32 k, 16 KB) per half-step through a ring of
//     five (three ahead, one barrier per half-step, LDS-DMA with counted vmcnt, as in k_conv3x3_c256). The slab of a chunk
//     = the tile's 2 ranks + one rank either side = 36 cells = 576 rows of 64 B, double-buffered; ring + slabs = 152 KB.
//   * pixel fragments: the three taps of one dy read the SAME nine cells of slab rank (rank + dy) -- cell N needs cell N + dx, and
//     N + dx = -1 / 9 are exactly the skipped pairs -- so the nine fragments of a rank stay in registers for three half-steps and
//     are refilled once per dy, IN PLACE, during the dx = +1 tap (b[N] is dead as soon as cell N - 1 has issued its MFMAs there):
//     27 fragment reads per chunk and wave instead of 78, one register set. The order is pinned (one scheduling region per
//     cell): left to the scheduler the refills move up and the kernel spills.
//   * the DMA goes through two buffer descriptors built in the kernel -- the launch part's activation rows, this layer's packed
//     weights -- as buffer_load_dwordx4 ... offen lds (cv_blds16): per-lane byte offset in one VGPR, everything wave-uniform (chunk,
//     tap, half-tile) in the scalar offset, no VALU add in the loop. The counted waits need every half-step to issue the same loads
//     in every chunk, so past the last chunk the loop still issues the next chunk's slab pieces and the weight half-tiles three
//     ahead -- but against a descriptor of ZERO records (a scalar select of the num_records word): the range check fails, vmcnt
//     counts the load, nothing is fetched, zeros land in LDS that nobody reads. The same for staging pass 4 of waves 4-7 (2,304
//     pieces over 512 threads: pass 4 has work for half of them; their zeros go to the wave's dump area). Before, those loads
//     wrapped around to chunk 0 and re-read valid memory: 40 KB of slab + 48 KB of weights per tile and 4 KB per chunk, 120 KB
//     on top of the 1,440 KB a middle tile needs (8.3 %; an edge-pair tile 11 %; a stem tile more than its useful stream), and
//     the epilogue waited for them to land. Measured: profiles/r08_tile_stream_ab.json, CHANGELOG.
//   * QUAD middle tiles (CCZ_CONV_G16_QUAD; g5q_tile below; what the evaluator runs on ranks 1..8 from 4096 boards on): the same wave body
//     on 4 ranks x 128 output channels -- as many tiles of as many rows x channels and MFMAs, but a tile streams half the layer's
//     weights: 1,032 instead of 1,475 KB of LDS-DMA per tile, 16 instead of 23 DMA instructions per thread and chunk. Same bits.
//     Measured (profiles/r09_quad_tiles_ab.json, CHANGELOG): 200.2-200.8 k -> 202.8-203.3 k sims/s. The two-rank tile stays for the
//     five-tile mode, the stem and the heads layer (its 1x1 epilogue needs all 256 channels of a row in one workgroup).
//   * ONE skeleton for the three tile forms (g5_tile and g5q_tile here, g5e_tile in cczero_conv_g16e.h): a form keeps its geometry, its
//     staging passes, its zeroing and dump-area rules, its step loop; the rest is shared -- g5_live_part (a launch part's pointers),
//     g5_xcd_tile (tile order), g5_ctx_common / g5_ctx_frags (G5Ctx), g5_acc_row_from_bias, g5_image_store / g5_rows_out (epilogue),
//     g5_barrier, and the cell macros G5_CELL / G5_CELLS of both step functions. What stayed per form, and what the compiler did with
//     the forms that were tried: CHANGELOG, "one prologue and epilogue for the three g16 tile forms".
//   * XCD-aware tile order: workgroup b runs on XCD b % 8 and the five tiles of a group read each other's ranks as halo, so XCD x
//     takes the x-th contiguous eighth of the tiles (HBM traffic per launch 398 MB -> 283-288 MB = algorithmic).
//
// Measured (profiles/r03_conv_g16.json; 4096 boards, one layer in isolation, interleaved on one device): 310-316 us against
// 355-363 us for k_conv3x3_c256; in the workload 301 us per layer (58 % of the dense fp16 peak), 22.14 against 23.69 ms per step
// on one box. The loop is power-limited like its predecessor's (DESIGN.md sections 2 and 10): 3 / 5 / 7 cells in front of the
// barrier and the weight DMA behind it all measure the same; what paid, step by step, was removing work -- the MFMAs of the
// off-board taps (-3...-5 %), the halo fetches (-2.4 %), 46 % of the LDS fragment reads (-3 %), the scattered weight reads (-2.2 %),
// half of the zero stores (-0.9 %). Not everything that removes LDS traffic pays: an epilogue straight from registers (v_permlane16_swap
// pairs two tiles so that a lane stores 16 contiguous bytes; no LDS image, no barrier) is bit-identical and 5 % slower -- its stores
// are sixteen 64-byte segments per instruction instead of whole 512-byte rows. Nor does hiding the prologue: a persistent form (round 6,
// a fixed number of workgroups walking tile lists, the next tile's first slab and weights staged while the epilogue drains) was
// bit-identical and -4.3 % per layer in isolation at exactly five tiles per workgroup, but lost or tied in the workload -- 183.4 k against
// 193.3-194.0 k sims/s, cache off 176.3 k against 181.4 k, 1024 boards 175.1 k against 180.2 k (profiles/r06_persistent_tower.json): the
// launch chains buy more at every layer boundary than it hides. It was removed after round 7.
#pragma once
#include "cczero_conv.h"

namespace ccz {

constexpr int kG5Rows = 288;                               // rows per tile (18 cells x 16 boards)
constexpr int kG5SlabRows = 576;                           // 36 cells
constexpr int kG5SlabBytes = kG5SlabRows * 64;             // 36,864 B per 32-channel chunk
constexpr int kG5WBytes = 256 * 64;                        // one half-step of weights
constexpr int kG5Ring = 5, kG5Ahead = 3;
constexpr int kG5AOff = kG5Ring * kG5WBytes;               // LDS: [weight ring | slab 0 | slab 1]
constexpr int kG5Dump = kG5AOff + 2 * kG5SlabBytes;        // 8 x 1 KB: where a wave's zero stores go when it has no row to zero
constexpr int kG5Lds = kG5Dump + 8 * 1024;                 // 163,840 B = all of it
constexpr int kG5ERow = 528;                               // epilogue image: bytes per row (512 + pad)
static_assert(kG5Rows * kG5ERow <= kG5Dump, "epilogue image must fit the operand buffers");
// the QUAD middle tile (g5q_tile below): 4 ranks x 128 output channels -- weight half-tiles of 8 KB, slabs of 6 ranks
constexpr int kG5QRows = 576;                              // rows per tile (36 cells x 16 boards)
constexpr int kG5QSlabRows = 864;                          // 54 cells
constexpr int kG5QSlabBytes = kG5QSlabRows * 64;           // 55,296 B per 32-channel chunk: six staging passes of 8 KB + one of 6 KB
constexpr int kG5QWBytes = 128 * 64;                       // one half-step of weights: 128 output channels
// CCZ_G5Q_PAIR (A/B switch; 1 = what ships): the quad tile meets at ONE workgroup barrier per TWO half-steps -- a ring of six weight
// slots, four ahead (g5_step, "the two-step ring"). 0 builds the body with a ring of five, three ahead, one barrier per half-step.
#ifndef CCZ_G5Q_PAIR
#define CCZ_G5Q_PAIR 1
#endif
constexpr bool kG5QPair = CCZ_G5Q_PAIR != 0;
constexpr int kG5QRing = kG5QPair ? 6 : kG5Ring, kG5QAhead = kG5QPair ? 4 : kG5Ahead;
constexpr int kG5QAOff = kG5QRing * kG5QWBytes;            // LDS: [weight ring | slab 0 | slab 1 | dump]
constexpr int kG5QDump = kG5QAOff + 2 * kG5QSlabBytes;     // where waves 6-7 aim staging pass 6, which has no piece for them: 1 KB each
constexpr int kG5QDumpWave0 = kG5QPair ? 6 : 0;            // (ring of five: a KB for each of the eight waves, six of them unused)
constexpr int kG5QLds = kG5QDump + (8 - kG5QDumpWave0) * 1024;
constexpr int kG5QERow = 272;                              // epilogue image: bytes per row (256 + pad)
static_assert(kG5QLds == (kG5QPair ? 161792 : 159744) && kG5QLds <= kG5Lds, "quad tile: ring + two slabs + dump must fit the workgroup's LDS");
static_assert(kG5QRows * kG5QERow == 156672 && kG5QRows * kG5QERow <= kG5QLds,
              "quad tile: the epilogue image covers the operand buffers (ring of five: and most of the dump area), free once every DMA has landed");

// Layout "G16C" (the CM forms): inside each 16-board group the rows are chunk-major -- [chunk 0..7][row 0..1439][32 channels], row
// stride 64 B, chunk stride 92,160 B, the group stride (737,280 B) as in G16 -- so that a chunk's slab is one contiguous run of whole
// 128-byte lines. Byte offset of chunk 0 of G16 row p:
constexpr int kG16CChunk = 1440 * 64;
__device__ __forceinline__ unsigned g16c_off(long p)
{
    const long g = p / 1440;
    return (unsigned)(g * (1440 * 512) + (p - g * 1440) * 64);
}

struct G5Ctx {
    unsigned char *lds;
    const _Float16 *X, *W;   // uniform bases of the two buffer descriptors: every DMA is descriptor + 32-bit byte offset (one VGPR) + scalar offset
    unsigned xbytes, wbytes; // SCALAR: bytes of the launch part's activation rows / of this layer's packed weights (the descriptors' num_records)
    unsigned xbytes_part;        // SCALAR: xbytes for waves 0-3, 0 for waves 4-7 -- staging pass 4 has 256 pieces, theirs fetch nothing
    unsigned xoff[5];        // per staging pass: byte offset of this thread's 16-byte source in X (chunk 0), row clamped into the tensor
                             // (quad tile: xoff[0] alone -- nothing is clamped, pass `it` is + it * xstep in the scalar offset)
    unsigned xstep, whalf;   // SCALAR (quad tile): bytes between two staging passes (128 rows); byte offset of the tile's channel half in a half-tile
    unsigned woff;           // byte offset of this thread's 16-byte weight source in W (row pass 0, tap 0, chunk 0)
    int zo[2], zd[2];        // SCALAR: where this wave's two zero stores go for slab 0, and the step to slab 1 (0 for the dump area)
    int wave_dst;            // w * 1024
    int lane16;              // (lane & 63) * 16 (the two-rank tile alone: g5_zero_ranks)
    int wave_dst_part, wave_step_part; // SCALAR: LDS offset of this wave's piece of staging pass 4 in slab 0 and the step to slab 1 (waves 4-7: their
                             // 1 KB of the dump area, step 0 -- the zeros of their out-of-range loads land where nothing is read)
    int a_off;               // weight fragment offset inside a ring slot (tile 0; tile i: + 1024 i)
    int vb[2];               // this lane's pixel-fragment base in slab 0 / 1 (cell 0 of the wave's rank at tap offset 0 = + 9 * 1024)
    int cin, cmask;          // input channels; number of 32-channel chunks - 1
#ifdef CCZ_STAMPS
    mutable unsigned long long st_vm, st_bar, st_n; // SCALAR, diagnostic build (G5Q_STAMP_ADD): cycles in the vmcnt waits / in the barriers, their count
#endif
};

__host__ __device__ constexpr bool g5_slab_tap(int t) { return t >= 1 && t <= 5; }
// DMA loads younger than the weight half-tile the NEXT half-step reads (issue order per half-step: slab piece, 2 weight loads)
constexpr int kG5Split = 7; // cells in front of the barrier (3 / 5 / 7 and the weight DMA behind the barrier: 344-351 us, noise)
// DMA loads a thread issues in half-step t, past the last chunk as well (g5_step: its slab piece `if constexpr (g5_dma(T) > 2)`, then
// the two weight pieces); the wait of half-step t leaves this half-step's and the previous one's in flight
__host__ __device__ constexpr int g5_dma(int t) { return 2 + (g5_slab_tap(t) ? 1 : 0); }
__host__ __device__ constexpr int g5_vmcnt(int t) { return g5_dma(t) + g5_dma(t - 1); }
// the counted waits rest on every half-step issuing the same loads in every chunk, the last included: pinned
static_assert(g5_vmcnt(0) == 4 && g5_vmcnt(1) == 5 && g5_vmcnt(2) == 6 && g5_vmcnt(3) == 6 && g5_vmcnt(4) == 6 && g5_vmcnt(5) == 6 &&
              g5_vmcnt(6) == 5 && g5_vmcnt(7) == 4 && g5_vmcnt(8) == 4, "g5_vmcnt table");
static_assert(g5_dma(0) == 2 && g5_dma(1) == 3 && g5_dma(2) == 3 && g5_dma(3) == 3 && g5_dma(4) == 3 && g5_dma(5) == 3 && g5_dma(6) == 2 &&
              g5_dma(7) == 2 && g5_dma(8) == 2, "23 DMA loads per chunk and thread: 5 slab pieces + 9 x 2 weight pieces");
// The quad tile: ONE weight piece per half-step (8 KB over 512 threads) and seven slab pieces per chunk. The next chunk's slab is first
// read in half-step 8 (the refill for dy = -1), published by the barrier of half-step 7, whose wait leaves the loads of half-steps 6
// and 7 in flight: the pieces go into half-steps 0..5 -- passes 0 and 1 in half-step 0, pass t + 1 in half-step t.
__host__ __device__ constexpr int g5q_nslab(int t) { return t == 0 ? 2 : t <= 5 ? 1 : 0; }
__host__ __device__ constexpr int g5q_dma(int t) { return 1 + g5q_nslab(t); }
__host__ __device__ constexpr int g5q_vmcnt(int t) { return g5q_dma(t) + g5q_dma((t + 8) % 9); }
static_assert(g5q_vmcnt(0) == 4 && g5q_vmcnt(1) == 5 && g5q_vmcnt(2) == 4 && g5q_vmcnt(3) == 4 && g5q_vmcnt(4) == 4 && g5q_vmcnt(5) == 4 &&
              g5q_vmcnt(6) == 3 && g5q_vmcnt(7) == 2 && g5q_vmcnt(8) == 2, "g5q_vmcnt table");
static_assert(g5q_dma(0) == 3 && g5q_dma(1) == 2 && g5q_dma(2) == 2 && g5q_dma(3) == 2 && g5q_dma(4) == 2 && g5q_dma(5) == 2 && g5q_dma(6) == 1 &&
              g5q_dma(7) == 1 && g5q_dma(8) == 1, "16 DMA loads per chunk and thread: 7 slab pieces + 9 weight pieces");

// The two-step ring (kG5QPair): the barrier stands in the ODD half-steps J of the unrolled pair of chunks and publishes the slots of
// half-steps J + 1 and J + 2; its wait still leaves the loads of half-steps J and J - 1 in flight, and with the weights four ahead
// those are the pieces of half-steps J + 4 and J + 3. A chunk is nine half-steps, so in the second chunk (J = 9..17) the barrier in
// front of the first slab read (half-step 8 of the chunk, J = 17) is the one of its half-step 6 (J = 15), not 7: there the seven slab
// pieces go into half-steps 0..4 -- passes 0, 1 | 2, 3 | 4 | 5 | 6 -- and in the first chunk they stay where the ring of five has them.
__host__ __device__ constexpr int g5q2_nslab(int j) { return j < 9 ? g5q_nslab(j) : j - 9 <= 1 ? 2 : j - 9 <= 4 ? 1 : 0; }
__host__ __device__ constexpr int g5q2_pass(int j) { return j % 9 == 0 ? 0 : g5q2_pass(j - 1) + g5q2_nslab(j - 1); } // first staging pass of half-step j
__host__ __device__ constexpr int g5q2_dma(int j) { return 1 + g5q2_nslab(j); }
__host__ __device__ constexpr int g5q2_vmcnt(int j) { return g5q2_dma(j) + g5q2_dma((j + 17) % 18); }
__host__ __device__ constexpr bool g5q2_barrier(int j) { return (j & 1) != 0; }
static_assert(g5q2_vmcnt(1) == 5 && g5q2_vmcnt(3) == 4 && g5q2_vmcnt(5) == 4 && g5q2_vmcnt(7) == 2 && g5q2_vmcnt(9) == 4 && g5q2_vmcnt(11) == 5 &&
              g5q2_vmcnt(13) == 4 && g5q2_vmcnt(15) == 2 && g5q2_vmcnt(17) == 2, "g5q2_vmcnt table (the odd half-steps wait)");
static_assert(g5q2_pass(8) == 7 && g5q2_pass(17) == 7 && g5q2_pass(5) == 6 && g5q2_pass(13) == 6 && g5q2_nslab(6) == 0 && g5q2_nslab(14) == 0,
              "seven slab pieces per chunk; the last one is issued in J = 5 resp. 13, two half-steps in front of the barriers of J = 7 resp. 15");
static_assert(18 % kG5QRing == 0 || !kG5QPair, "the slot of a half-step is a compile-time function of J");

template <int T, int N> __host__ __device__ constexpr bool g5_on_board() // is tap T of the cell with file N on the board (dx only)
{
    return !((T % 3 == 0 && N == 0) || (T % 3 == 2 && N == 8));
}

// The workgroup barrier of these kernels: a raw s_barrier fenced on both sides, so that nothing is scheduled across it.
// LDS_DONE: this wave's own LDS stores and loads have completed first (lgkmcnt(0)).
template <bool LDS_DONE = false> __device__ __forceinline__ void g5_barrier()
{
    if constexpr (LDS_DONE) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// Diagnostic build (-DCCZ_STAMPS, profiles/conv_quad_stamps.py; the shipped kernels hold no stamp): what the quad tile's meeting point
// costs a wave -- cycles in the counted vmcnt wait and in the barrier, summed over the tile's half-steps in scalar registers.
#ifdef CCZ_STAMPS
__device__ unsigned long long g_g5q_stamps[4096 * 8 * 8]; // [workgroup][wave]: vm wait, barrier, loop, real time of the loop, meetings
#define G5Q_STAMP(s_) const unsigned long long s_ = cv_stamp();
#define G5Q_STAMP_ADD(c_, s0_, s1_, s2_) (c_).st_vm += s1_ - s0_; (c_).st_bar += s2_ - s1_; (c_).st_n += 1;
#else
#define G5Q_STAMP(s_)
#define G5Q_STAMP_ADD(c_, s0_, s1_, s2_)
#endif

// The rank above rank 0 (tiles with k = 0) and the rank below rank 9 (k = 4) do not exist: their slab rows were staged from
// clamped addresses (the DMA count stays static) and are overwritten with zeros by the thread that staged them, after its DMA has
// landed and before the barrier that publishes the slab. Rows 0..143 / 432..575 = whole 16-row pieces, so the tests are
// wave-uniform -- and there are no tests in the loop: the two stores always execute, a wave that has nothing to zero aims
// them at its 1 KB dump area behind the slabs (a branch here splits the loop body and costs the register allocation 90 spills).
__device__ __forceinline__ void g5_zero_ranks(const G5Ctx &c, int buf)
{
    int l16 = c.lane16, zero = 0;
    asm volatile("" : "+v"(l16), "+v"(zero)); // formed here: as loop invariants the four addresses and the zero vector hold 8 registers
    typedef int g5_int4 __attribute__((ext_vector_type(4)));
    const g5_int4 z = {zero, zero, zero, zero};
#pragma unroll
    for (int j = 0; j < 2; ++j) *(g5_int4 *)(c.lds + (l16 + (c.zo[j] + buf * c.zd[j]))) = z;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// The cells of one half-step (g5_step here, g5e_step in cczero_conv_g16e.h): G5_CELLS(TAP, LO, HI) runs cells LO..HI-1 of tap TAP inside a
// step function that has `lds`, `c`, `acc`, `acur`, `b`, `BUFn` in scope and defines G5_REFILL(N) = the slab cell that b[N] is refilled
// from during a dx = +1 tap. The order is pinned, one scheduling region per cell (see g5_step). Both macros end with cczero_conv_g16e.h.
#define G5_CELL(TAP, N)                                                                                                   \
    {                                                                                                                     \
        if constexpr (TAP % 3 == 2)                                                                                       \
            b[N] = *(const cv_half8 *)(lds + c.vb[BUFn] + G5_REFILL(N) * 1024);                                           \
        if constexpr (g5_on_board<TAP, N>()) {                                                                            \
            constexpr int NB = N + TAP % 3 - 1;                                                                           \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                 \
                acc[i][N] = __builtin_amdgcn_mfma_f32_16x16x32_f16(acur[i], b[NB], acc[i][N], 0, 0, 0);                   \
        }                                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                                \
    }
#define G5_CELLS(TAP, LO, HI)                                                                                             \
    if constexpr (LO <= 0 && 0 < HI) G5_CELL(TAP, 0) if constexpr (LO <= 1 && 1 < HI) G5_CELL(TAP, 1) if constexpr (LO <= 2 && 2 < HI) G5_CELL(TAP, 2) \
    if constexpr (LO <= 3 && 3 < HI) G5_CELL(TAP, 3) if constexpr (LO <= 4 && 4 < HI) G5_CELL(TAP, 4) if constexpr (LO <= 5 && 5 < HI) G5_CELL(TAP, 5) \
    if constexpr (LO <= 6 && 6 < HI) G5_CELL(TAP, 6) if constexpr (LO <= 7 && 7 < HI) G5_CELL(TAP, 7) if constexpr (LO <= 8 && 8 < HI) G5_CELL(TAP, 8)

// One half-step = tap T of a 32-channel chunk; J = its index inside the unrolled pair of chunks (parity of the A register
// set = J & 1, slab buffer = J / 9). Q: the quad tile's staging (8 KB ring slots, slabs of six ranks, g5q_dma) around the SAME cells.
template <int J, bool Q = false, bool CM = false>
__device__ __forceinline__ void g5_step(const G5Ctx &c, cv_f32x4 (&acc)[4][9], int chunk, int &ring_rd, int &ring_wr,
                                         cv_half8 (&a0)[4], cv_half8 (&a1)[4], cv_half8 (&b)[9])
{
    constexpr int T = J % 9, BUF = J / 9;
    constexpr int Tn = (T + 1) % 9, BUFn = (T == 8) ? 1 - BUF : BUF;
    constexpr int kWB = Q ? kG5QWBytes : kG5WBytes, kAOff = Q ? kG5QAOff : kG5AOff, kSlab = Q ? kG5QSlabBytes : kG5SlabBytes;
    cv_half8 (&acur)[4] = (J & 1) ? a1 : a0;
    cv_half8 (&anxt)[4] = (J & 1) ? a0 : a1;
    unsigned char *const lds = c.lds;

    // the order below is pinned (one scheduling region per cell): a fragment register is refilled right AFTER the MFMAs that read
    // it -- left to the scheduler the refills move up and every fragment needs a second register
    // The three taps of one dy read the SAME nine cells of slab rank (rank + dy): cell N needs cell N + dx. So b[] holds the nine
    // fragments of that rank for three half-steps (cell N multiplies b[N + dx]; N + dx = -1 and 9 are exactly the skipped,
    // off-board pairs) and is refilled once per dy, during the dx = +1 tap: b[N] is dead as soon as cell N - 1 has issued its
    // MFMAs there, so it is reloaded for the next dy right in front of cell N's MFMAs -- 27 fragment reads per chunk instead of 78.
#define G5_REFILL(N) (9 + N + 9 * (Tn / 3 - 1))
    constexpr bool P = Q && kG5QPair;           // the two-step ring: a barrier in the odd half-steps only, slots by J (g5q2_vmcnt)
    constexpr int kAhead = Q ? kG5QAhead : kG5Ahead;
    constexpr int T2 = (T + kAhead) % 9;
    // Past the last chunk there is nothing left to prefetch, but every load is still ISSUED (the vmcnt counts stay static): its
    // descriptor then has zero records, the range check fails and nothing is fetched (cv_blds16)
    const int chunk2 = chunk + (T + kAhead >= 9 ? 1 : 0);
    constexpr int nslab = !Q ? 0 : P ? g5q2_nslab(J) : g5q_nslab(T);
    G5_CELLS(T, 0, 1)
    if constexpr (nslab > 0) { // the next chunk's slab: 7 pieces per thread, passes 0, 1 | 2 | .. | 6 in taps 0 | 1 | .. | 5 (P, second chunk: g5q2_nslab)
        constexpr int pass = P ? g5q2_pass(J) : T == 0 ? 0 : T + 1;
        const unsigned so = (unsigned)((chunk + 1) * (CM ? kG16CChunk : 64));
        const unsigned live = chunk < c.cmask ? (pass < 6 ? c.xbytes : c.xbytes_part) : 0u;
        cv_blds16(c.X, live, c.xoff[0], so + pass * c.xstep,
                  lds + (pass < 6 ? kAOff + (1 - BUF) * kSlab + pass * 8192 + c.wave_dst : c.wave_dst_part + (1 - BUF) * c.wave_step_part));
        if constexpr (nslab > 1) cv_blds16(c.X, live, c.xoff[0], so + (pass + 1) * c.xstep, lds + kAOff + (1 - BUF) * kSlab + ((pass + 1) * 8192 + c.wave_dst));
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (!Q && g5_dma(T) > 2) { // the next chunk's slab: 5 pieces per thread, in taps 1..5
        constexpr int pass = T - 1;
        const unsigned live = pass < 4 ? c.xbytes : c.xbytes_part;
        cv_blds16(c.X, chunk < c.cmask ? live : 0u, c.xoff[pass], (unsigned)((chunk + 1) * (CM ? kG16CChunk : 64)),
                  lds + (pass < 4 ? kG5AOff + (1 - BUF) * kG5SlabBytes + pass * 8192 + c.wave_dst : c.wave_dst_part + (1 - BUF) * c.wave_step_part));
        __builtin_amdgcn_sched_barrier(0);
    }
    G5_CELLS(T, 1, 2)
    if constexpr (Q) { // this tile's half (8 KB: rows 128 h .. 128 h + 127) of half-tile (chunk2, T2): one piece per thread
        if constexpr (P) cv_blds16(c.W, chunk2 <= c.cmask ? c.wbytes : 0u, c.woff, (unsigned)((T2 + 9 * chunk2) * (2 * 8192)) + c.whalf, lds + ((J + kAhead) % kG5QRing) * kWB + c.wave_dst);
        else cv_blds16(c.W, chunk2 <= c.cmask ? c.wbytes : 0u, c.woff, (unsigned)((T2 + 9 * chunk2) * (2 * 8192)) + c.whalf, lds + ring_wr * kWB + c.wave_dst);
        __builtin_amdgcn_sched_barrier(0);
        G5_CELLS(T, 2, 3)
    } else {
        const unsigned wlive = chunk2 <= c.cmask ? c.wbytes : 0u;
        const unsigned so = (unsigned)((T2 + 9 * chunk2) * (2 * 8192)); // half-tile (chunk2, T2): one contiguous 16 KB block, a scalar offset
        unsigned char *const d = lds + ring_wr * kG5WBytes + c.wave_dst;
        cv_blds16(c.W, wlive, c.woff, so, d);
        __builtin_amdgcn_sched_barrier(0);
        G5_CELLS(T, 2, 3)
        cv_blds16(c.W, wlive, c.woff, so + 8192u, d + 8192);            // its rows 128..255
        __builtin_amdgcn_sched_barrier(0);
    }
    G5_CELLS(T, 3, kG5Split)

    if constexpr (P) {
        // The two-step ring. An odd half-step waits for this thread's pieces of the slots of J + 1 and J + 2 (and, J = 7 and 15, of the
        // next chunk's slab) and meets the other waves; an even one does neither: slot J + 1, which it reads below, was published by the
        // barrier of J - 1. What a DMA of half-step J overwrites is slot J + 4 = J - 2 (mod 6): its readers loaded their fragments in
        // J - 3 and spent them in the MFMAs of J - 2, in front of the last barrier this wave has passed (J - 1 or J - 2).
        if constexpr (g5q2_barrier(J)) {
            G5Q_STAMP(s0)
            cv_wait_vm<g5q2_vmcnt(J)>();
            G5Q_STAMP(s1)
            g5_barrier();
            G5Q_STAMP(s2)
            G5Q_STAMP_ADD(c, s0, s1, s2)
        } else __builtin_amdgcn_sched_barrier(0);
        const unsigned char *wa = lds + (((J + 1) % kG5QRing) * kWB + c.a_off);
#pragma unroll
        for (int i = 0; i < 4; ++i) anxt[i] = *(const cv_half8 *)(wa + i * 1024);
        __builtin_amdgcn_sched_barrier(0);
        G5_CELLS(T, kG5Split, 9)
    } else {
        ring_rd = ring_rd + 1 == kG5Ring ? 0 : ring_rd + 1;
        if constexpr (Q) { G5Q_STAMP(s0) cv_wait_vm<g5q_vmcnt(T)>(); G5Q_STAMP(s1) g5_barrier(); G5Q_STAMP(s2) G5Q_STAMP_ADD(c, s0, s1, s2) }
        else {
            cv_wait_vm<g5_vmcnt(T)>();
            if constexpr (T == 7) g5_zero_ranks(c, 1 - BUF); // this thread's slab pieces of the next chunk have landed (all but the youngest weight loads)
            g5_barrier();
        }

        {
            const unsigned char *wa = lds + (ring_rd * kWB + c.a_off);
#pragma unroll
            for (int i = 0; i < 4; ++i) anxt[i] = *(const cv_half8 *)(wa + i * 1024);
            __builtin_amdgcn_sched_barrier(0);
        }
        G5_CELLS(T, kG5Split, 9)
        ring_wr = ring_wr + 1 == kG5Ring ? 0 : ring_wr + 1;
    }
#undef G5_REFILL
}

// ---- the heads fused into the LAST tower layer (round 4) ------------------------------------------------------------------------------
// The tower's last layer writes 170 MB of activations that only the two 1x1 head convolutions read (k_head_conv1x1: 46 us, HBM-bound).
// In the HEADS instantiation the layer's epilogue keeps its finished rows (conv + bias + residual, ReLU) in the LDS image instead of
// storing them, and the workgroup multiplies them with the 24 head channels right there: per 16-row cell 16 MFMAs against the 72 x 36
// of the tile's own loop. The output tensor of the layer is never written; the head outputs leave in board order exactly as
// k_head_conv1x1 writes them (cczero_heads.h) -- same operands, same chain of MFMAs over k = 0, 32, ...: the same bits.
struct G5Heads {
    const _Float16 *w32; // [32][256]: rows 0..16 policy, 17..23 value, 24..31 zero
    const float *b32;    // [32]
    _Float16 *pol, *val; // [boards][1536], [boards][640] (cczero_heads.h kHdPolStride / kHdValStride)
    int nb;              // boards that hold rows (compact live count or the batch size): stores past it are skipped
};

// `board0[wnr]` / `pos0[wnr]`: first board (group * 16) and first position (rank * 9) of image rows 144 wnr .. 144 wnr + 143 (wnr = 0, 1);
// `skip1`: image rows 144..287 are a duplicate (edge kernel, odd group count). Called by every wave after the barrier that publishes the
// image of FINISHED rows.
__device__ __forceinline__ void g5_heads_phase(const unsigned char *lds, int w, int lane, const G5Heads &ha, const long (&board0)[2],
                                               const int (&pos0)[2], bool skip1)
{
    const int r = lane & 15, q4 = lane >> 4;
    cv_half8 a[2][8];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int s = 0; s < 8; ++s) a[m][s] = *(const cv_half8 *)(ha.w32 + (m * 16 + r) * 256 + s * 32 + q4 * 8);
    const float4 b0 = *(const float4 *)(ha.b32 + 4 * q4), b1 = *(const float4 *)(ha.b32 + 16 + 4 * q4);
    for (int cell = w; cell < 18; cell += 8) { // 18 cells of 16 rows over 8 waves
        const unsigned char *row = lds + (cell * 16 + r) * kG5ERow + q4 * 16;
        cv_f32x4 acc0, acc1;
        acc0[0] = b0.x; acc0[1] = b0.y; acc0[2] = b0.z; acc0[3] = b0.w;
        acc1[0] = b1.x; acc1[1] = b1.y; acc1[2] = b1.z; acc1[3] = b1.w;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const cv_half8 b = *(const cv_half8 *)(row + s * 64);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0][s], b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[1][s], b, acc1, 0, 0, 0);
        }
        const int wnr = cell >= 9 ? 1 : 0, n = cell - 9 * wnr;
        const long board = board0[wnr] + r;
        if (board < ha.nb && !(skip1 && wnr)) {
            const int pos = pos0[wnr] + n;
            _Float16 *po = ha.pol + board * 1536 + pos * 17;
            _Float16 *vo = ha.val + board * 640 + pos * 7;
#pragma unroll
            for (int e = 0; e < 4; ++e) po[4 * q4 + e] = (_Float16)fmaxf(acc0[e], 0.0f);
            if (q4 == 0) {
                po[16] = (_Float16)fmaxf(acc1[0], 0.0f);
                vo[0] = (_Float16)fmaxf(acc1[1], 0.0f);
                vo[1] = (_Float16)fmaxf(acc1[2], 0.0f);
                vo[2] = (_Float16)fmaxf(acc1[3], 0.0f);
            } else if (q4 == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) vo[3 + e] = (_Float16)fmaxf(acc1[e], 0.0f);
            }
        }
    }
}

// ONE: only the first 32 input channels of a row can be non-zero (the stem: 21 live planes in rows of 64 channels) -- the tile runs the
// nine half-steps of chunk 0 and stops; the second chunk would add products of zeros to accumulators that are never -0 (they start at
// a bias): the same bits (the board-major and small-batch kernels run both chunks; tests compare them bit for bit).
// Planned evaluator boundary (ccz_eval_plan): only the first *live_rows boards hold rows to compute, a number that stays on the
// device. Their 16-board groups are cut into n_parts EQUAL ranges; a launch is range `part` of them (row0 carries part | n_parts << 16)
// and finds its groups itself: returns how many of them are live (at most `cap`, the groups the launch was sized for) and sets `first`
// to the first. Workgroups beyond the live tiles leave at once.
__device__ __forceinline__ int g5_live_groups(const int *live_rows, int row0, int cap, int &first)
{
    const int part = row0 & 0xffff, n_parts = row0 >> 16;
    const int G = (*live_rows + 15) >> 4;
    const int per = (G + n_parts - 1) / n_parts;
    first = part * per;
    int live = G - first;
    live = live < 0 ? 0 : (live > per ? per : live);
    return live > cap ? cap : live;
}

// A launch part's pointers moved to its first live group `first` (g5_live_groups); `first_board` = that group's global board
// index for the heads. HEADS: there is no output tensor, Y stays.
template <bool RES, bool HEADS>
__device__ __forceinline__ void g5_live_part(int first, int cin, const _Float16 *__restrict__ &X, const _Float16 *&R, _Float16 *&Y, long &first_board)
{
    const long off = (long)first * 1440 * kCvC;
    X += (long)first * 1440 * cin;
    if (!HEADS) Y += off;
    if (RES) R += off;
    first_board = (long)first * 16;
}

// XCD-aware order: workgroup b runs on XCD b % 8 (round-robin dispatch), and the five tiles of a group read each other's
// ranks as halo -- so XCD x takes the x-th CONTIGUOUS eighth of the tiles, in order: a halo rank is then in that XCD's L2
// (with tile = b: 398 MB fetched per half-batch launch against 283 MB algorithmic, profiles/pmc_summary.json).
// flags bit 1: tiles in descending order (the tiles written last by the previous layer are then read first)
__device__ __forceinline__ int g5_xcd_tile(int blk, int tiles, int flags)
{
    const int b = blk, x = b & 7, per = tiles >> 3, rem = tiles & 7;
    const int tile = x * per + (x < rem ? x : rem) + (b >> 3);
    return __builtin_amdgcn_readfirstlane((flags & 2) ? tiles - 1 - tile : tile);
}

// The G5Ctx fields that every tile form sets the same way. `xbytes`: bytes of the launch part's activation rows; `chunks`: 32-channel
// chunks to run. (`woff` is as common but stays behind each form's `xoff`: set here, in front of them, the loop of
// k_conv3x3_g16<no residual> compiles to other instructions; `lane16` is the two-rank tile's alone, for g5_zero_ranks.)
__device__ __forceinline__ void g5_ctx_common(G5Ctx &c, unsigned char *lds, const _Float16 *X, const _Float16 *W, int w, unsigned xbytes, int cin, int chunks)
{
    c.lds = lds;
    c.X = X;
    c.W = W;
    c.wave_dst = w * 1024;
    c.cin = cin;
    c.cmask = chunks - 1;
    c.xbytes = xbytes;
    c.wbytes = 9u * 256u * (unsigned)cin * 2u;
}

// This lane's fragment addresses: weight rows 64 wm + 16 i + r of a ring slot, and row r of slab cell `cell0` (+ n, + the tap's offset)
// in the slabs at `aoff`, `slab` bytes apart -- both through the swizzle of the 64-byte rows
__device__ __forceinline__ void g5_ctx_frags(G5Ctx &c, int r, int q4, int wm, int cell0, int aoff, int slab)
{
    const int lane1 = r * 64 + ((q4 ^ ((0 - (r >> 2)) & 3)) << 4);
    c.a_off = wm * 4096 + lane1;
    c.vb[0] = aoff + cell0 * 1024 + lane1;
    c.vb[1] = c.vb[0] + slab;
}

// Epilogue, part 1: the wave's 64 channels x 144 rows (wave row `wn`, channels from 64 wm) as fp16 into the [row][channel] image in
// LDS, EROW bytes per image row. `r`, `q4`: lane & 15, lane >> 4.
template <int EROW>
__device__ __forceinline__ void g5_image_store(unsigned char *lds, cv_f32x4 (&acc)[4][9], int wm, int wn, int r, int q4)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = wm * 64 + i * 16 + 4 * q4;
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            cv_half4 o;
            o[0] = (_Float16)acc[i][n][0];
            o[1] = (_Float16)acc[i][n][1];
            o[2] = (_Float16)acc[i][n][2];
            o[3] = (_Float16)acc[i][n][3];
            *(cv_half4 *)(lds + ((wn * 9 + n) * 16 + r) * EROW + col * 2) = o;
        }
    }
}

// Epilogue, part 2, behind the barrier that publishes the image: a lane moves 18 16-byte pieces, STEP image rows apart -- image row
// `irow` + STEP it, piece `piece` of it = tensor row `pbase` + STEP it, channels `gcol` .. + 7. Image + residual `rv` (loaded by the
// caller in front of that barrier) (+ ReLU) out to Y -- or (HEADS) back into the image: the finished row stays there, Y is not written.
// The two-rank and the quad tile; the edge pair keeps its own copy under its store predicate (cczero_conv_g16e.h: in
// k_conv3x3_g16_one* the compiler folds two bodies' identical store tails into one, and the kernels' instruction counts move).
template <int EROW, int STEP, bool RES, bool HEADS>
__device__ __forceinline__ void g5_rows_out(unsigned char *lds, int irow, int piece, long pbase, int gcol, _Float16 *Y, int relu, const cv_half8 (&rv)[18])
{
    const cv_half8 zero = (cv_half8)(_Float16)0;
    unsigned char *eb = lds + irow * EROW + piece * 16;
#pragma unroll
    for (int it = 0; it < 18; ++it) {
        cv_half8 v = *(const cv_half8 *)(eb + it * STEP * EROW);
        if (RES) v = v + rv[it];
        if (relu) v = __builtin_elementwise_max(v, zero);
        if constexpr (HEADS) *(cv_half8 *)(eb + it * STEP * EROW) = v;
        else *(cv_half8 *)(Y + (pbase + it * STEP) * kCvC + gcol) = v;
    }
}

// Epilogue, part 2, of the G16C forms: one wave instruction moves 16 rows x 64 B of ONE chunk -- 1 KB contiguous in memory, whole lines.
// A wave owns one chunk of the image and 18 cells of it, one per iteration (cell = 16 image rows, 1 KB of tensor). Within an
// instruction a lane takes 16-byte piece lane & 3 of the row g16c_lane_row(lane): ds_read_b128 serves the lanes in four fixed groups
// of four quads ({0,3,5,6}, {1,2,4,7}, {8,11,13,14}, {9,10,12,15}), an image row is 16 (mod 256) bytes after the one before (EROW =
// 272, 528), so the four rows of a group must lie four rows apart (0, 4, 8, 12 + k) for their 64-byte pieces to cover the 64 banks
// once; and the four quads 4 q .. 4 q + 3 are given two PAIRS of neighbouring rows, so that each quarter-wave still covers two whole
// 128-byte lines of the tensor. The image and the accumulator stores into it are untouched.
__device__ __forceinline__ int g16c_lane_row(int lane) { return (int)((0xFEAB6732DC894510ull >> (4 * (lane >> 2))) & 15); }

// `img`: this lane's byte offset in the image at iteration 0 (iteration it: + it * 16 * EROW); `yoff`: its byte offset in the tensor
// (iteration it: + it * 1024). `rv`: the residual pieces, loaded by the caller from the same offsets.
template <int EROW, bool RES, bool HEADS>
__device__ __forceinline__ void g5c_rows_out(unsigned char *lds, int img, size_t yoff, _Float16 *Y, int relu, const cv_half8 (&rv)[18])
{
    const cv_half8 zero = (cv_half8)(_Float16)0;
    unsigned char *eb = lds + img;
#pragma unroll
    for (int it = 0; it < 18; ++it) {
        cv_half8 v = *(const cv_half8 *)(eb + it * 16 * EROW);
        if (RES) v = v + rv[it];
        if (relu) v = __builtin_elementwise_max(v, zero);
        if constexpr (HEADS) *(cv_half8 *)(eb + it * 16 * EROW) = v;
        else *(cv_half8 *)((unsigned char *)Y + yoff + it * 1024) = v;
    }
}

// The accumulators start at the bias: the nine tiles of one accumulator row, from the four bias values at `bias4`. One row per call, the
// loop over the four rows is the caller's: with it in here (acc[4][9] by reference) k_conv3x3_g16_quad<residual> and
// k_conv3x3_g16_one_quad<residual> spill 16 VGPRs and the loops of the other kernels change (CHANGELOG).
__device__ __forceinline__ void g5_acc_row_from_bias(cv_f32x4 (&row)[9], const float *bias4)
{
    const float4 bv = *(const float4 *)bias4;
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        row[n][0] = bv.x; row[n][1] = bv.y; row[n][2] = bv.z; row[n][3] = bv.w;
    }
}

// One two-rank tile. `lds`: the workgroup's kG5Lds bytes (declared by the kernel, so that one kernel can hold two tile classes);
// `blk`: this workgroup's tile slot, `grid`: the launch's tile count (without a live-row count; with one, the tiles of the live groups).
// CM: the layer's tensors are in the chunk-major G16C layout -- X and R where they are read (not the stem's packed planes: ONE), Y.
template <bool RES, bool HEADS, bool ONE = false, bool CM = false>
__device__ __forceinline__ void g5_tile(unsigned char *lds, int blk, int grid, const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                        const float *__restrict__ bias, const _Float16 *R,
                                        _Float16 *Y, int M, int relu, int cin, const int *live_rows, int row0, const G5Heads &ha)
{
    [[maybe_unused]] long first_board = 0; // (HEADS) global index of this launch's first board: the live parts offset their pointers
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q4 = lane >> 4;
    const int wm = w & 3, wn = w >> 2; // the two waves of a SIMD share their weight fragments' rows
    int tiles = grid;
    if (live_rows) {
        int first;
        const int live = g5_live_groups(live_rows, row0, M / 1440, first);
        M = live * 1440;
        tiles = live * ((relu & 4) ? 4 : 5);
        if (blk >= tiles) return;
        g5_live_part<RES, HEADS>(first, cin, X, R, Y, first_board);
    }
    const int tile = g5_xcd_tile(blk, tiles, relu);
    // flags bit 2 ("middle" mode, round 4): the launch covers ranks 1..8 only, four tiles per group (ranks 1-2, 3-4, 5-6, 7-8: every
    // neighbour rank exists, nothing is zeroed); ranks 0 and 9 are k_conv3x3_g16_edge's (cczero_conv_g16e.h)
    const int mid = relu & 4;
    const int k = mid ? 2 : tile % 5;        // ranks 2k, 2k + 1 of the tile's group (middle mode: any k without an edge)
    const long p0 = mid ? (long)(tile >> 2) * 1440 + 144 + (long)(tile & 3) * kG5Rows
                        : (long)tile * kG5Rows;    // = (group * 90 + 18 k) * 16
    relu &= 1;

    G5Ctx c;
    {
        // rows 0..143 (k = 0) = pass 0 of every wave + pass 1 of wave 0; rows 432..575 (k = 4) = pass 3 of waves 3..7 + pass 4 of
        // waves 0..3: two stores per wave cover either (wave 0 resp. wave 3 need both of theirs); anything else goes to the dump area
        const int piece[2] = {k == 0 ? 0 : k == 4 ? (w >= 3 ? 3 : 4) : -1, (k == 0 && w == 0) ? 1 : (k == 4 && w == 3) ? 4 : -1};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            c.zo[j] = __builtin_amdgcn_readfirstlane(piece[j] >= 0 ? kG5AOff + piece[j] * 8192 + w * 1024 : kG5Dump + w * 1024);
            c.zd[j] = __builtin_amdgcn_readfirstlane(piece[j] >= 0 ? kG5SlabBytes : 0);
        }
    }
    g5_ctx_common(c, lds, X, W, w, (unsigned)M * (unsigned)cin * 2u, cin, ONE ? 1 : cin >> 5);
    c.lane16 = lane * 16; // (g5_zero_ranks)
    c.wave_dst_part = w < 4 ? kG5AOff + 4 * 8192 + w * 1024 : kG5Dump + w * 1024;
    c.wave_step_part = w < 4 ? kG5SlabBytes : 0;
    c.xbytes_part = w < 4 ? c.xbytes : 0u;
    {
        // slab row sr (0..575) = tensor row p0 - 144 + sr: rank 2k - 1 + sr / 144 of the group; 64-byte rows, position pos of
        // row sr holds source chunk pos ^ f(sr), f = (-(sr >> 2)) & 3 (conflict-free for the 16 rows x 4 chunks one ds_read_b128
        // of this MFMA shape covers)
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const int piece = (it < 4 || w < 4) ? it * 512 + tid : 3 * 512 + tid; // (waves 4-7 in pass 4: any offset, xbytes_part = 0)
            const int sr = piece >> 2, pos = piece & 3;
            const int schunk = pos ^ ((0 - (sr >> 2)) & 3);
            long p = p0 - 144 + sr;
            p = p < 0 ? 0 : (p > (long)M - 1 ? (long)M - 1 : p);
            if constexpr (CM && !ONE) c.xoff[it] = g16c_off(p) + (unsigned)(schunk * 16);
            else c.xoff[it] = (unsigned)(p * cin + schunk * 8) * 2u;
        }
        c.woff = (unsigned)(tid * 16); // packed weights (k_pack_conv_weights_g16): a half-tile is the LDS image itself, read linearly
    }
    // ---- prologue: slab of chunk 0, weight half-tiles 0..2; the per-lane setup below runs while the DMA is in flight
#pragma unroll
    for (int it = 0; it < 5; ++it)
        cv_blds16(X, it < 4 ? c.xbytes : c.xbytes_part, c.xoff[it], 0u, lds + (it < 4 ? kG5AOff + it * 8192 + c.wave_dst : c.wave_dst_part));
#pragma unroll
    for (int u = 0; u < kG5Ahead; ++u) {
        unsigned char *d = lds + u * kG5WBytes + c.wave_dst;
        cv_blds16(W, c.wbytes, c.woff, (unsigned)(u * 2 * 8192), d);
        cv_blds16(W, c.wbytes, c.woff, (unsigned)(u * 2 * 8192 + 8192), d + 8192);
    }
    g5_ctx_frags(c, r, q4, wm, wn * 9, kG5AOff, kG5SlabBytes); // slab cell 9 wn + n + 9 + delta

    cv_f32x4 acc[4][9];
#pragma unroll
    for (int i = 0; i < 4; ++i) g5_acc_row_from_bias(acc[i], bias + wm * 64 + i * 16 + 4 * q4);

    cv_wait_vm<4>();
    g5_zero_ranks(c, 0);
    g5_barrier<true>();

    int ring_rd = 0, ring_wr = kG5Ahead;
    cv_half8 a0[4], a1[4], b[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) a0[i] = *(const cv_half8 *)(lds + c.a_off + i * 1024);
#pragma unroll
    for (int n = 0; n < 9; ++n) b[n] = *(const cv_half8 *)(lds + c.vb[0] + (9 + n - 9) * 1024); // the rank above this wave's: dy = -1
#define G5_S(j) g5_step<j, false, CM && !ONE>(c, acc, chunk + (j) / 9, ring_rd, ring_wr, a0, a1, b)
    if constexpr (ONE) {
        const int chunk = 0; // (one chunk: every next-chunk prefetch is issued against an empty descriptor and fetches nothing)
        G5_S(0); G5_S(1); G5_S(2); G5_S(3); G5_S(4); G5_S(5); G5_S(6); G5_S(7); G5_S(8);
    } else {
        for (int chunk = 0; chunk <= c.cmask; chunk += 2) {
            G5_S(0); G5_S(1); G5_S(2); G5_S(3); G5_S(4); G5_S(5); G5_S(6); G5_S(7); G5_S(8);
            G5_S(9); G5_S(10); G5_S(11); G5_S(12); G5_S(13); G5_S(14); G5_S(15); G5_S(16); G5_S(17);
        }
    }
#undef G5_S
    cv_wait_vm<0>(); // the out-of-range DMA loads (zeros) must have landed before the LDS is reused / released

    // ---- epilogue: every wave writes its 64 channels x 144 rows into the [row][channel] image in LDS; then wave w owns
    // rows 36 w .. 36 w + 35 and moves whole 512-byte rows (residual in, output out)
    g5_barrier(); // every wave is done reading the slabs and the ring
    // the lane index is formed again here (v_mbcnt): carried through the loop it is the 257th register of the heads instantiation
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int re = lane_e & 15, q4e = lane_e >> 4;
    const int prow = lane_e >> 5, piece = lane_e & 31;
    const long pbase = p0 + w * 36 + prow;
    cv_half8 rv[18];
    g5_image_store<kG5ERow>(lds, acc, wm, wn, re, q4e);
    if constexpr (CM) { // wave w owns chunk w of the 18 cells (g5c_rows_out)
        const int erow = g16c_lane_row(lane_e), ep = lane_e & 3;
        const size_t yo = (size_t)g16c_off(p0 + erow) + (size_t)(w * kG16CChunk + ep * 16);
        if (RES) {
#pragma unroll
            for (int it = 0; it < 18; ++it) rv[it] = *(const cv_half8 *)((const unsigned char *)R + yo + it * 1024);
        }
        g5_barrier<true>();
        g5c_rows_out<kG5ERow, RES, HEADS>(lds, erow * kG5ERow + w * 64 + ep * 16, yo, Y, relu, rv);
    } else {
        if (RES) {
#pragma unroll
            for (int it = 0; it < 18; ++it) rv[it] = *(const cv_half8 *)(R + (pbase + it * 2) * kCvC + piece * 8);
        }
        g5_barrier<true>();
        g5_rows_out<kG5ERow, 2, RES, HEADS>(lds, w * 36 + prow, piece, pbase, piece * 8, Y, relu, rv);
    }
    if constexpr (HEADS) {
        g5_barrier<true>(); // every finished row is in the image
        // image rows 0..143 = the tile's first rank, 144..287 = its second: tensor row p0 + i = (group * 90 + 9 * rank + cell) * 16 + board
        const long grp = p0 / 1440;
        const int rank0 = (int)((p0 - grp * 1440) / 144);
        const long board0[2] = {first_board + grp * 16, first_board + grp * 16};
        const int pos0[2] = {rank0 * 9, rank0 * 9 + 9};
        g5_heads_phase(lds, w, lane_e, ha, board0, pos0, false);
    }
}

// ---- the QUAD middle tile (CCZ_CONV_G16_QUAD): four ranks x 128 output channels ----------------------------------------------------
// A two-rank middle tile streams the WHOLE layer's weights (72 x 16 KB = 1,180 KB) for 288 rows: 80 % of its 1,475 KB of DMA. The quad
// tile runs the same MFMAs -- a wave is still 64 output channels x one rank, the same cells in the same order (g5_step), the same K
// order: the same bits -- on ranks 1-4 or 5-8 of a group x ONE HALF of the output channels: 72 x 8 KB of weights + 8 x 55,296 B of
// slab (six ranks) = 1,032 KB per tile, -30 % DMA bytes per MFMA, 16 DMA instructions per thread and chunk instead of 23.
//   * waves: wm = w & 1 (64 of the tile's 128 channels), wn = w >> 1 (rank of the quad).
//   * tile slot t of a group (four, as in middle mode): quad t >> 1, channel half h = t & 1 -- the two halves of a quad are neighbours
//     in the XCD-aware order: they run on the same XCD at about the same time and the second finds the slab in that L2.
//   * a middle tile's slab never leaves its group's 1,440 rows: nothing is clamped, nothing is zeroed, and staging pass `it` is the
//     thread's pass-0 offset + it * 128 rows in the SCALAR offset (one VGPR instead of five). Pass 6 has 384 pieces: waves 6-7 issue
//     theirs against the zero-record descriptor into their KB of the dump area.
//   * epilogue image: 576 rows x 272 B; wave w owns rows 72 w .. 72 w + 71 and moves 256-byte row segments (channels 128 h ..).
template <bool RES, bool CM = false>
__device__ __forceinline__ void g5q_tile(unsigned char *lds, int blk, int grid, const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                         const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M, int relu, int cin,
                                         const int *live_rows, int row0)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q4 = lane >> 4;
    const int wm = w & 1, wn = w >> 1;
    int tiles = grid;
    if (live_rows) {
        int first;
        const int live = g5_live_groups(live_rows, row0, M / 1440, first);
        M = live * 1440;
        tiles = live * 4;
        if (blk >= tiles) return;
        long first_board;
        g5_live_part<RES, false>(first, cin, X, R, Y, first_board);
    }
    const int tile = g5_xcd_tile(blk, tiles, relu);
    const int h = tile & 1;                                                              // output channels 128 h .. 128 h + 127
    const long p0 = (long)(tile >> 2) * 1440 + 144 + (long)((tile >> 1) & 1) * kG5QRows; // = (group * 90 + 9 * (1 or 5)) * 16
    relu &= 1;

    G5Ctx c;
    g5_ctx_common(c, lds, X, W, w, (unsigned)M * (unsigned)cin * 2u, cin, cin >> 5);
    c.wave_dst_part = w < 6 ? kG5QAOff + 6 * 8192 + w * 1024 : kG5QDump + (w - kG5QDumpWave0) * 1024;
    c.wave_step_part = w < 6 ? kG5QSlabBytes : 0;
    c.xbytes_part = w < 6 ? c.xbytes : 0u;
    c.xstep = CM ? 128u * 64u : 128u * (unsigned)cin * 2u;
    c.whalf = (unsigned)h * 8192u;
    {
        // slab row sr (0..863) = tensor row p0 - 144 + sr: rank (1 or 5) - 1 + sr / 144 of the group; piece it * 512 + tid is row
        // it * 128 + (tid >> 2), and the swizzle f(sr) = (-(sr >> 2)) & 3 does not depend on `it`
        const int sr = tid >> 2, pos = tid & 3;
        const int schunk = pos ^ ((0 - (sr >> 2)) & 3);
        if constexpr (CM) c.xoff[0] = g16c_off(p0 - 144 + sr) + (unsigned)(schunk * 16); // a wave's 16 rows x 64 B: 1 KB of whole lines
        else c.xoff[0] = (unsigned)((p0 - 144 + sr) * cin + schunk * 8) * 2u;
        c.woff = (unsigned)(tid * 16);
    }
    // ---- prologue: slab of chunk 0, this half's weight blocks of the first kG5QAhead taps
#pragma unroll
    for (int it = 0; it < 7; ++it)
        cv_blds16(X, it < 6 ? c.xbytes : c.xbytes_part, c.xoff[0], it * c.xstep, lds + (it < 6 ? kG5QAOff + it * 8192 + c.wave_dst : c.wave_dst_part));
#pragma unroll
    for (int u = 0; u < kG5QAhead; ++u) cv_blds16(W, c.wbytes, c.woff, (unsigned)(u * 2 * 8192) + c.whalf, lds + u * kG5QWBytes + c.wave_dst);
    g5_ctx_frags(c, r, q4, wm, wn * 9, kG5QAOff, kG5QSlabBytes); // weight rows 128 h + 64 wm + ..; slab cell 9 wn + n + 9 + delta

    cv_f32x4 acc[4][9];
#pragma unroll
    for (int i = 0; i < 4; ++i) g5_acc_row_from_bias(acc[i], bias + h * 128 + wm * 64 + i * 16 + 4 * q4);

    cv_wait_vm<2>(); // all but the weight blocks of the last two taps (two-step ring: slots 0 AND 1 are published here, half-step 0 has no barrier)
    g5_barrier();

    int ring_rd = 0, ring_wr = kG5QAhead; // (two-step ring: unused, a half-step's slots are functions of J)
    cv_half8 a0[4], a1[4], b[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) a0[i] = *(const cv_half8 *)(lds + c.a_off + i * 1024);
#pragma unroll
    for (int n = 0; n < 9; ++n) b[n] = *(const cv_half8 *)(lds + c.vb[0] + n * 1024); // the rank above this wave's: dy = -1
#ifdef CCZ_STAMPS
    c.st_vm = c.st_bar = c.st_n = 0;
    const unsigned long long st_loop0 = cv_stamp(), st_real0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
    for (int chunk = 0; chunk <= c.cmask; chunk += 2) {
#define G5Q_S(j) g5_step<j, true, CM>(c, acc, chunk + (j) / 9, ring_rd, ring_wr, a0, a1, b)
        G5Q_S(0); G5Q_S(1); G5Q_S(2); G5Q_S(3); G5Q_S(4); G5Q_S(5); G5Q_S(6); G5Q_S(7); G5Q_S(8);
        G5Q_S(9); G5Q_S(10); G5Q_S(11); G5Q_S(12); G5Q_S(13); G5Q_S(14); G5Q_S(15); G5Q_S(16); G5Q_S(17);
#undef G5Q_S
    }
#ifdef CCZ_STAMPS
    {
        const unsigned long long st_loop1 = cv_stamp(), st_real1 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        if (blk < 4096 && lane == 0) { // a buffer of the stamps' own: nothing in the kernel reads it
            unsigned long long *o = g_g5q_stamps + ((size_t)blk * 8 + w) * 8;
            o[0] = c.st_vm; o[1] = c.st_bar; o[2] = st_loop1 - st_loop0; o[3] = st_real1 - st_real0; o[4] = c.st_n;
        }
    }
#endif
    cv_wait_vm<0>(); // the out-of-range DMA loads (zeros) must have landed before the image below is written over the operand buffers

    // ---- epilogue: every wave writes its 64 channels x 144 rows into the [row][channel] image; then wave w owns rows 72 w .. 72 w + 71
    g5_barrier(); // every wave is done reading the slabs and the ring
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); // formed again, as in g5_tile
    const int re = lane_e & 15, q4e = lane_e >> 4;
    const int prow = lane_e >> 4, piece = lane_e & 15;
    const long pbase = p0 + w * 72 + prow;
    const int gcol = h * 128 + piece * 8;
    cv_half8 rv[18];
    g5_image_store<kG5QERow>(lds, acc, wm, wn, re, q4e);
    if constexpr (CM) { // wave w owns chunk 4 h + (w & 3), cells 18 (w >> 2) .. + 17 of the tile's 36 (g5c_rows_out)
        const int erow = g16c_lane_row(lane_e), ep = lane_e & 3, ch = w & 3, irow = (w >> 2) * 288 + erow;
        const size_t yo = (size_t)g16c_off(p0 + irow) + (size_t)((h * 4 + ch) * kG16CChunk + ep * 16);
        if (RES) {
#pragma unroll
            for (int it = 0; it < 18; ++it) rv[it] = *(const cv_half8 *)((const unsigned char *)R + yo + it * 1024);
        }
        g5_barrier<true>();
        g5c_rows_out<kG5QERow, RES, false>(lds, irow * kG5QERow + ch * 64 + ep * 16, yo, Y, relu, rv);
    } else {
        if (RES) {
#pragma unroll
            for (int it = 0; it < 18; ++it) rv[it] = *(const cv_half8 *)(R + (pbase + it * 4) * kCvC + gcol);
        }
        g5_barrier<true>();
        g5_rows_out<kG5QERow, 4, RES, false>(lds, w * 72 + prow, piece, pbase, gcol, Y, relu, rv);
    }
}

template <bool RES>
__global__ __launch_bounds__(512) void k_conv3x3_g16(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                         const float *__restrict__ bias, const _Float16 *R,
                                                         _Float16 *Y, int M, int relu, int cin, const int *live_rows, int row0)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    g5_tile<RES, false>(lds, blockIdx.x, gridDim.x, X, W, bias, R, Y, M, relu, cin, live_rows, row0, G5Heads{});
}

// The middle launch of quad tiles (CCZ_CONV_G16_QUAD without CCZ_CONV_G16_ONE_LAUNCH): grid = 4 tiles per group, ranks 1..8
template <bool RES>
__global__ __launch_bounds__(512) void k_conv3x3_g16_quad(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                            const float *__restrict__ bias, const _Float16 *R,
                                                            _Float16 *Y, int M, int relu, int cin, const int *live_rows, int row0)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    g5q_tile<RES>(lds, blockIdx.x, gridDim.x, X, W, bias, R, Y, M, relu, cin, live_rows, row0);
}

// The stem (ccz_conv3x3_stem_f16 with CCZ_CONV_G16): rows of 64 channels of which only 0..31 can be non-zero, one chunk (g5_tile ONE)
__global__ __launch_bounds__(512) void k_conv3x3_g16_stem(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                            const float *__restrict__ bias, _Float16 *Y, int M, int relu, int cin,
                                                            const int *live_rows, int row0)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    g5_tile<false, false, true>(lds, blockIdx.x, gridDim.x, X, W, bias, nullptr, Y, M, relu, cin, live_rows, row0, G5Heads{});
}

// The last layer of the tower with the heads in its epilogue (always with residual; Y may be null: nothing is stored to it).
__global__ __launch_bounds__(512) void k_conv3x3_g16_heads(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                             const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                                             int relu, int cin, const int *live_rows, int row0, G5Heads ha)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    if (live_rows) ha.nb = *live_rows; // planned boundary: the pointers are the whole batch's, M only the capacity of this part
    g5_tile<true, true>(lds, blockIdx.x, gridDim.x, X, W, bias, R, Y, M, relu, cin, live_rows, row0, ha);
}

// The G16C forms of the stem (writes chunk-major rows; its input stays the packed planes) and of the heads layer (reads them)
__global__ __launch_bounds__(512) void k_conv3x3_g16c_stem(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                             const float *__restrict__ bias, _Float16 *Y, int M, int relu, int cin,
                                                             const int *live_rows, int row0)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    g5_tile<false, false, true, true>(lds, blockIdx.x, gridDim.x, X, W, bias, nullptr, Y, M, relu, cin, live_rows, row0, G5Heads{});
}

__global__ __launch_bounds__(512) void k_conv3x3_g16c_heads(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                              const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                                              int relu, int cin, const int *live_rows, int row0, G5Heads ha)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[kG5Lds];
    if (live_rows) ha.nb = *live_rows;
    g5_tile<true, true, false, true>(lds, blockIdx.x, gridDim.x, X, W, bias, R, Y, M, relu, cin, live_rows, row0, ha);
}

// Weights for k_conv3x3_g16: [co][tap][ci] (the memory of a channels-last [co, ci, 3, 3] tensor) -> [ci / 32][tap][co][32], each
// 64-byte row stored with its four 16-byte chunks in the swizzled order the LDS image uses (position pos of row co holds chunk
// pos ^ ((-(co >> 2)) & 3)): a half-tile (32 input channels of one tap, all 256 output channels) becomes ONE contiguous 16 KB
// block that the DMA copies linearly -- whole 128-byte lines instead of 256 scattered 64-byte pieces 4.6 KB apart (-2.7 % per
// layer). One thread per 16-byte piece.
__global__ __launch_bounds__(256) void k_pack_conv_weights_g16(const cv_half8 *__restrict__ w, cv_half8 *__restrict__ wp, int cin)
{
    const int n = 256 * 9 * (cin >> 3);
    const int i = blockIdx.x * 256 + threadIdx.x;   // destination piece: ((c32 * 9 + tap) * 256 + co) * 4 + pos
    if (i >= n) return;
    const int pos = i & 3, co = (i >> 2) & 255, h = i >> 10, tap = h % 9, c32 = h / 9;
    const int chunk = pos ^ ((0 - (co >> 2)) & 3);
    wp[i] = w[(co * 9 + tap) * (cin >> 3) + c32 * 4 + chunk];
}

} // namespace ccz
