// cczero_conv_narrow.h -- the tower convolution for NARROW towers: 3x3 on the 10 x 9 board, 64 or 128 channels in and out, board-major
// NHWC fp16 rows, fp32 accumulate, + bias [+ residual] + ReLU in the epilogue. The chain is the one of cczero_conv.h:
//
//   a[p, co] = bias[co] + sum_{tap, ci} w[co, tap, ci] * x[p + 9*dy + dx, ci]      fp32 accumulator, started at the bias
//   y[p, co] = relu?( fp16( fp16(a[p, co]) + res[p, co] ) )                            with a residual: two roundings, the add in fp16
//   y[p, co] = relu?( fp16(a[p, co]) )                                                 without
//
// Two forms, the same bits from both (tests/test_gpu_narrow_f64.py):
//
//   * up to 64 boards: k_conv3x3_small<RES, CIN, COUT> (cczero_conv_small.h), which is generic in both widths;
//   * above: k_conv3x3_narrow<RES, CIN, COUT> below. One workgroup = 256 consecutive pixels x ALL COUT output channels, 8 waves of 32
//     pixels (two 16-pixel MFMA tiles) x COUT / 16 weight tiles each. v_mfma_f32_16x16x32_f16, weights = A operand (row lane & 15,
//     k-chunk lane >> 4), pixels = B operand; K order = ascending chunks of 32 input channels x 9 taps; every output element is ONE
//     dependent chain of CIN / 32 * 9 MFMAs whose operands and lane positions are those of the small kernel: K is never split, and
//     neither the tile nor the batch size enters the arithmetic.
//   * the slab (the tile's 256 pixels + the 10-pixel halo either side, all CIN channels: 69 KB at 128) is staged ONCE with plain loads
//     into XOR-swizzled rows (the small kernel's image) and read at the nine row offsets; a tap that leaves the board reads a zero row
//     (per-lane 9-bit mask, no arithmetic on the data). Rows past the tensor are clamped on load and never stored.
//   * the weights are staged per chunk of 32 input channels (9 taps x COUT rows x 64 B = 72 KB at 128 output channels) as lane-linear
//     1 KB MFMA fragments: conflict-free reads. The next chunk's weights are requested into registers BEFORE the current chunk's
//     MFMAs and written to the one LDS buffer behind them, between two barriers: 2 x (CIN / 32 - 1) + 1 barriers per tile.
//   * a whole layer's weights (288 KB at 128 -> 128) do not fit LDS next to the slab, so every workgroup re-reads them from L2: what
//     bounds the tile at large batches is this restaging (288 KB per 256 pixels), not the MFMAs.
//   * the _live form is the planned boundary of k_conv3x3_c256: *live_rows boards cut into n_parts equal ranges of whole 8 boards, this
//     launch computes range `part` (row0 = part | n_parts << 16); workgroups past the live tiles leave at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cczero_conv.h"

namespace ccz {

constexpr int kNwBM = 256;                        // pixels per workgroup (8 waves x 32)
constexpr int kNwRows = kNwBM + 2 * kCvHalo;      // slab rows
__host__ __device__ constexpr int nw_lds_bytes(int cin, int cout) { return 9 * (cout / 16) * 1024 + (kNwRows + 1) * cin * 2; }

// LDS: [weights of one chunk: fragment (tap, m) of 1 KB, lane-linear | slab rows of CIN fp16, 16-byte chunk c of row r at position
// (c & ~swz) | ((c ^ r) & swz) | one zero row]
template <bool RES, int CIN, int COUT>
__global__ __launch_bounds__(512) void k_conv3x3_narrow(const _Float16 *__restrict__ X, const _Float16 *__restrict__ W,
                                                          const float *__restrict__ bias, const _Float16 *R, _Float16 *Y, int M,
                                                          int relu, const int *live_rows, int row0)
{
    constexpr int MT = COUT / 16, NC = CIN / 32;             // weight tiles per wave, chunks of 32 input channels
    constexpr int row_bytes = CIN * 2, cpr = CIN >> 3;        // bytes and 16-byte chunks per slab row
    constexpr int swz = cpr >= 16 ? 15 : 7;
    constexpr int w_bytes = 9 * MT * 1024, slab_off = w_bytes, zero_off = slab_off + kNwRows * row_bytes;
    constexpr int kWPieces = 9 * MT * 64, kWIters = (kWPieces + 511) / 512;     // 16-byte weight pieces of a chunk, per thread: 9 / 5
    constexpr int kSPieces = kNwRows * cpr, kSIters = (kSPieces + 511) / 512;   // slab pieces, per thread: 9 / 5
    __shared__ __attribute__((aligned(16))) unsigned char lds[nw_lds_bytes(CIN, COUT)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q4 = lane >> 4;
    int tiles = gridDim.x;
    if (live_rows) { // the planned boundary, as in k_conv3x3_c256
        const int part = row0 & 0xffff, n_parts = row0 >> 16;
        const int L = *live_rows;
        const int per = ((L + n_parts - 1) / n_parts + 7) / 8 * 8;
        const int first = part * per;
        int live = L - first;
        live = live < 0 ? 0 : (live > per ? per : live);
        live = live > M / 90 ? M / 90 : live;
        M = live * 90;
        tiles = (M + kNwBM - 1) / kNwBM;
        if ((int)blockIdx.x >= tiles) return;
        X += (long)first * 90 * CIN;
        Y += (long)first * 90 * COUT;
        if (RES) R += (long)first * 90 * COUT;
    }
    // flags bit 1: tiles in descending order (the tiles written last by the previous layer are then read first)
    const long p0 = (long)((relu & 2) ? tiles - 1 - (int)blockIdx.x : (int)blockIdx.x) * kNwBM;
    relu &= 1;

    // ---- staging. No guards: a thread without a piece of its own in the last pass repeats the last piece (same bytes, same address)
    cv_half8 wreg[kWIters];
    auto get_w = [&](int c32) { // fragment f = tap * MT + m, lane l = row l & 15, k-chunk l >> 4 -> LDS f * 1024 + l * 16
#pragma unroll
        for (int j = 0; j < kWIters; ++j) {
            int i = j * 512 + tid;
            i = i < kWPieces ? i : kWPieces - 1;
            const int f = i >> 6, l = i & 63, tap = f / MT, m = f - tap * MT;
            wreg[j] = *(const cv_half8 *)(W + (long)(m * 16 + (l & 15)) * (9 * CIN) + tap * CIN + c32 * 32 + (l >> 4) * 8);
        }
    };
    auto put_w = [&]() {
#pragma unroll
        for (int j = 0; j < kWIters; ++j) {
            int i = j * 512 + tid;
            i = i < kWPieces ? i : kWPieces - 1;
            *(cv_half8 *)(lds + i * 16) = wreg[j];
        }
    };
    get_w(0);
    {
        cv_half8 sreg[kSIters];
#pragma unroll
        for (int j = 0; j < kSIters; ++j) { // rows p0 - 10 .. p0 + 256 + 10, clamped into the tensor: a clamped row is only ever read by a masked tap
            int i = j * 512 + tid;
            i = i < kSPieces ? i : kSPieces - 1;
            const int row = i / cpr, c = i - row * cpr;
            long p = p0 - kCvHalo + row;
            p = p < 0 ? 0 : (p > (long)M - 1 ? (long)M - 1 : p);
            sreg[j] = *(const cv_half8 *)(X + p * CIN + c * 8);
        }
        put_w();
#pragma unroll
        for (int j = 0; j < kSIters; ++j) {
            int i = j * 512 + tid;
            i = i < kSPieces ? i : kSPieces - 1;
            const int row = i / cpr, c = i - row * cpr;
            *(cv_half8 *)(lds + slab_off + row * row_bytes + (((c & ~swz) | ((c ^ row) & swz)) << 4)) = sreg[j];
        }
    }
    if (tid < row_bytes / 4) *(uint32_t *)(lds + zero_off + tid * 4) = 0u;

    // validity of the nine taps for this lane's two pixels: on the board, and inside the tensor (a count that is not whole boards:
    // the rows of the last board past it read as zero)
    unsigned vmask[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const long pix = p0 + wv * 32 + n * 16 + r;
        const int pos = (int)(pix % 90), rank = pos / 9, file = pos - rank * 9;
        unsigned m = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            if (rank + dy >= 0 && rank + dy <= 9 && file + dx >= 0 && file + dx <= 8 && pix + 9 * dy + dx < M) m |= 1u << t;
        }
        vmask[n] = m;
    }

    // the accumulators start at the bias
    cv_f32x4 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const float4 bv = *(const float4 *)(bias + m * 16 + 4 * q4);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            acc[m][n][0] = bv.x; acc[m][n][1] = bv.y; acc[m][n][2] = bv.z; acc[m][n][3] = bv.w;
        }
    }
    const bool idle = p0 + wv * 32 >= M; // this wave's pixels lie past the tensor: it helps with the staging and the barriers only
    auto publish = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    publish();

    // ---- K loop: chunk of 32 input channels (outer) x tap (inner); per tap MT weight fragments, two pixel fragments, 2 MT MFMAs
#pragma unroll
    for (int c32 = 0; c32 < NC; ++c32) {
        if (c32 + 1 < NC) get_w(c32 + 1); // in flight behind this chunk's MFMAs
        if (!idle) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int delta = 9 * (tap / 3 - 1) + (tap % 3 - 1);
                const int c = c32 * 4 + q4; // 16-byte chunk of this lane's k-range inside the slab row
                cv_half8 b[2];
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const int row = kCvHalo + wv * 32 + n * 16 + r + delta;
                    const bool ok = (vmask[n] >> tap) & 1u;
                    const int off = ok ? slab_off + row * row_bytes + (((c & ~swz) | ((c ^ row) & swz)) << 4) : zero_off;
                    b[n] = *(const cv_half8 *)(lds + off);
                }
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const cv_half8 a = *(const cv_half8 *)(lds + (tap * MT + m) * 1024 + lane * 16);
#pragma unroll
                    for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b[n], acc[m][n], 0, 0, 0);
                }
            }
        }
        if (c32 + 1 < NC) {
            publish(); // every wave has read this chunk's weights
            put_w();
            publish();
        }
    }
    if (idle) return;

    // ---- epilogue: lane holds output channels 16 m + 4 q4 .. + 3 of pixels p0 + 32 wv + 16 n + r
    const cv_half4 zero = (cv_half4)(_Float16)0;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const long pix = p0 + wv * 32 + n * 16 + r;
        if (pix >= M) continue;
        cv_half4 res[MT];
        if constexpr (RES) {
#pragma unroll
            for (int m = 0; m < MT; ++m) res[m] = *(const cv_half4 *)(R + pix * COUT + m * 16 + 4 * q4);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            cv_half4 o;
            o[0] = (_Float16)acc[m][n][0];
            o[1] = (_Float16)acc[m][n][1];
            o[2] = (_Float16)acc[m][n][2];
            o[3] = (_Float16)acc[m][n][3];
            if constexpr (RES) o = o + res[m];
            if (relu) o = __builtin_elementwise_max(o, zero);
            *(cv_half4 *)(Y + pix * COUT + m * 16 + 4 * q4) = o;
        }
    }
}

} // namespace ccz
