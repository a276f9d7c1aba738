// cczero_snapshot.h -- engine snapshots (include/cczero.h "Engine snapshots"): the layout scan and the pack / unpack kernels.
//
// A snapshot is taken at a move boundary. What is live in the node pool and in the record arrays then is a per-board prefix: n_nodes
// nodes of the board's pool half, ply plies, pi_used pi entries. The kernels here move exactly those prefixes, and the fixed-size rows
// of every board, between the engine's arrays and one contiguous blob. The job is plain bandwidth: one workgroup per board, 16-byte
// accesses wherever both sides are 16-byte aligned (the blob side always is), no atomics.
//
// The blob (all little-endian; chinesechesszero_amd/snapshot.py parses it on the host):
//   [0, 512)                 header (ccz_snapshot_save in cczero.hip writes it; SnapHeader below)
//   [512, 512 + 8 (B + 1))   uint64 offsets[B + 1]: the exclusive scan of the section sizes; offsets[B] = their sum
//   then                     BoardMeta meta[B] (40 bytes each)
//   sections_start           = the above rounded up to 16; board b's section is [sections_start + offsets[b], sections_start + offsets[b + 1])
// A section: the fixed rows (kSnapFixed bytes, the table below), then nodeA [n_nodes][16], nodeB [n_nodes][4], proof [n_nodes] (with
// kSnapProof), rec_sq [ply][96], rec_off [ply][4], rec_turn / rec_k / rec_target [ply], rec_value [ply][4] and rec_hasv [ply] (with
// kSnapValues), rec_kl [ply][4], rec_hask [ply] and the board's SurpriseBoardStats row (with kSnapSurprise: only while ccz_set_surprise is
// on), rec_ids [pi_used][2], rec_pi [pi_used][4] -- every array rounded up to 16 bytes with zeros.
#pragma once
#include "cczero_device.h"

namespace ccz {

constexpr uint32_t kSnapProof = 1u, kSnapValues = 2u, kSnapSurprise = 4u; // CCZ_SNAP_PROOF / CCZ_SNAP_VALUES / CCZ_SNAP_SURPRISE
constexpr uint64_t kSnapMagic = 0x0050414E535A4343ull; // "CCZSNAP\0"
constexpr uint32_t kSnapVersion = 1u;
constexpr int kSnapHeader = 512;

// the fixed rows of a section: byte offsets (16-byte rows first, then 8, 4, 1)
constexpr int kSnapRootSq = 0;          // uint8 [96]
constexpr int kSnapChain = 96;          // uint64 [128]
constexpr int kSnapChainChk = 1120;     // uint64 [2]
constexpr int kSnapGmG = 1136;          // double [128]
constexpr int kSnapGmLogit = 2160;      // double [128]
constexpr int kSnapGmN0 = 3184;         // int32 [128]
constexpr int kSnapExDir = 3696;        // float [128]
constexpr int kSnapEsSnap = 4208;       // int32 [128]
constexpr int kSnapGmStamp = 4720;      // uint32 [4]
constexpr int kSnapStats = 4736;        // BoardStats (104)
constexpr int kSnapRsStats = 4840;      // ResignBoardStats (56)
constexpr int kSnapExStats = 4896;      // ExploreBoardStats (32)
constexpr int kSnapSvStats = 4928;      // SolverBoardStats (16)
constexpr int kSnapGmStats = 4944;      // GumbelBoardStats (24)
constexpr int kSnapEsStats = 4968;      // StopBoardStats (48)
constexpr int kSnapWideStats = 5016;    // WideBoardStats (24; zeros while the wide search never was on)
constexpr int kSnapExStamp = 5040;      // uint32 [2]
constexpr int kSnapBudget = 5048;       // int32
constexpr int kSnapMoveSims = 5052;     // int32
constexpr int kSnapRsFire = 5056;       // int32
constexpr int kSnapRsLast = 5060;       // float
constexpr int kSnapEsSnapS = 5064;      // int32
constexpr int kSnapTarget = 5068;       // uint8
constexpr int kSnapRsState = 5069;      // uint8
constexpr int kSnapRsRun = 5070;        // uint8 [2]
constexpr int kSnapEsStopped = 5072;    // uint8
constexpr int kSnapFixedUsed = 5073;
constexpr int kSnapFixed = 5088;        // rounded up to 16
static_assert(sizeof(BoardMeta) == 40 && sizeof(NodeA) == 16, "the snapshot's meta / node records");
static_assert(sizeof(BoardStats) == 104 && sizeof(ResignBoardStats) == 56 && sizeof(ExploreBoardStats) == 32 && sizeof(SolverBoardStats) == 16 &&
                  sizeof(GumbelBoardStats) == 24 && sizeof(StopBoardStats) == 48 && sizeof(WideBoardStats) == 24,
              "the snapshot's per-board counter rows");
static_assert(sizeof(ResignCfg) == 24 && sizeof(ExploreCfg) == 32 && sizeof(GumbelCfg) == 32 && sizeof(SearchCfg) == 48 && sizeof(StopCfg) == 40,
              "the snapshot's settings structs");

// The header as ccz_snapshot_save writes it. Everything that decides the layout and the arithmetic of the engine that saved.
struct SnapHeader {
    uint64_t magic;
    uint32_t version, header_bytes;
    uint64_t total_bytes, sections_start;
    int32_t B, cap, maxd, max_plies, pi_cap, reserve;
    float c_puct;
    uint32_t flags;
    double eps, alpha, temp;
    uint64_t seed, board_id_base;
    uint32_t rule_flags, chanpack, typepack, trankpack;
    uint64_t rank_hash;       // FNV-1a over the move-rank table (0: none, ascending id)
    uint32_t sections;        // kSnapProof | kSnapValues
    int32_t width, solver_enabled, budgets_on;
    int32_t err, half;        // the sticky error word; the pool half word when saved (informational: a load lands in the receiver's)
    uint32_t fixed_bytes, meta_bytes;
    ResignCfg resign;
    ExploreCfg explore;
    GumbelCfg gumbel;
    SearchCfg search;
    StopCfg stop;
    SurpriseCfg surprise;     // (zeros while ccz_set_surprise never was on: the bytes a header without the field has there)
    uint8_t pad[kSnapHeader - 360];
};
static_assert(sizeof(SnapHeader) == kSnapHeader, "the snapshot header is 512 bytes");
static_assert(offsetof(SnapHeader, resign) == 160 && offsetof(SnapHeader, stop) == 296 && offsetof(SnapHeader, surprise) == 336,
              "snapshot.py reads the settings at these offsets");
static_assert(sizeof(SurpriseCfg) == 24 && sizeof(SurpriseBoardStats) == 24, "the snapshot's surprise settings and counter row");

__host__ __device__ __forceinline__ uint64_t snap_pad16(uint64_t n) { return (n + 15ull) & ~15ull; }

// bytes of one board's section: the documented formula (snapshot.py: section_bytes)
__host__ __device__ __forceinline__ uint64_t snap_section_bytes(uint32_t sections, uint64_t n_nodes, uint64_t ply, uint64_t pi_used)
{
    uint64_t s = (uint64_t)kSnapFixed + n_nodes * 16ull + snap_pad16(n_nodes * 4ull);
    if (sections & kSnapProof) s += snap_pad16(n_nodes);
    s += ply * 96ull + snap_pad16(ply * 4ull) + 3ull * snap_pad16(ply);
    if (sections & kSnapValues) s += snap_pad16(ply * 4ull) + snap_pad16(ply);
    if (sections & kSnapSurprise) s += snap_pad16(ply * 4ull) + snap_pad16(ply) + snap_pad16(sizeof(SurpriseBoardStats));
    s += snap_pad16(pi_used * 2ull) + snap_pad16(pi_used * 4ull);
    return s;
}

// ------------------------------------------------------------------ the layout: an exclusive scan of the section sizes in 64 bits
// One workgroup of 1024 threads walks the boards 1024 at a time (any B); the carry between rounds is the round's last inclusive sum.
// The counts come with a stride in words: 1 for caller-supplied arrays (ccz_snapshot_layout), sizeof(BoardMeta) / 4 for the fields of
// the engine's own meta records. Negative counts count as 0.
__global__ __launch_bounds__(1024) void k_snapshot_layout(int B, const int32_t *n_nodes, const int32_t *ply, const uint32_t *pi_used, int stride,
                                                            uint32_t sections, uint64_t *offsets)
{
    __shared__ uint64_t s_scan[1024];
    const int t = threadIdx.x;
    uint64_t carry = 0;
    for (int b0 = 0; b0 < B; b0 += 1024) {
        const int b = b0 + t;
        uint64_t v = 0;
        if (b < B) {
            const size_t i = (size_t)b * (size_t)stride;
            const int nn = n_nodes[i], pl = ply[i];
            v = snap_section_bytes(sections, (uint64_t)(nn > 0 ? nn : 0), (uint64_t)(pl > 0 ? pl : 0), (uint64_t)pi_used[i]);
        }
        s_scan[t] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const uint64_t a = t >= o ? s_scan[t - o] : 0ull;
            __syncthreads();
            s_scan[t] += a;
            __syncthreads();
        }
        if (b < B) offsets[b] = carry + s_scan[t] - v;
        carry += s_scan[1023];
        __syncthreads(); // s_scan[1023] is read by every thread before the next round writes it
    }
    if (t == 0) offsets[B] = carry;
}

// ------------------------------------------------------------------ moving bytes
// n bytes between two arrays that do not overlap, by the nt threads of a workgroup: 16 bytes per access where both sides are 16-byte
// aligned, else 4, else 1; the tail in bytes. Nothing past n is read or written on either side.
__device__ __forceinline__ void snap_copy(uint8_t *dst, const uint8_t *src, size_t n, int t, int nt)
{
    const uintptr_t a = (uintptr_t)dst | (uintptr_t)src;
    size_t done = 0;
    if (!(a & 15u)) {
        const size_t q = n >> 4;
        for (size_t i = (size_t)t; i < q; i += (size_t)nt) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
        done = q << 4;
    } else if (!(a & 3u)) {
        const size_t q = n >> 2;
        for (size_t i = (size_t)t; i < q; i += (size_t)nt) ((uint32_t *)dst)[i] = ((const uint32_t *)src)[i];
        done = q << 2;
    }
    for (size_t i = done + (size_t)t; i < n; i += (size_t)nt) dst[i] = src[i];
}

// One array of a section: `n` live bytes at blob + p, and the padding up to the next 16 bytes. PACK: engine -> blob, the padding zeroed;
// else blob -> engine, the padding skipped. `eng` null: the engine has no such array (PACK: zeros; else: nothing is written).
// Returns the section offset behind the array.
template <bool PACK> __device__ __forceinline__ uint64_t snap_array(uint8_t *blob, uint64_t p, void *eng, size_t n, int t, int nt)
{
    uint8_t *o = blob + p;
    const size_t padded = (size_t)snap_pad16(n);
    if (PACK) {
        if (eng) snap_copy(o, (const uint8_t *)eng, n, t, nt);
        for (size_t i = (eng ? n : 0) + (size_t)t; i < padded; i += (size_t)nt) o[i] = 0;
    } else if (eng) {
        snap_copy((uint8_t *)eng, o, n, t, nt);
    }
    return p + padded;
}

// Every byte of board b's section, in the order of the layout. m: the board's meta record (PACK: the engine's; else the blob's, already
// validated against cap / max_plies / pi_cap on the host); half: the pool half the tree is read from / lands in.
template <bool PACK> __device__ __forceinline__ void snap_section(const Dev &D, int b, const BoardMeta &m, int half, uint8_t *o, uint32_t sections,
                                                                  uint8_t *proof, WideBoardStats *wide, int t, int nt)
{
    const size_t sb = (size_t)b;
#define SNAP_ROW(OFF_, PTR_, BYTES_) (void)snap_array<PACK>(o, (uint64_t)(OFF_), (void *)(PTR_), (size_t)(BYTES_), t, nt)
    SNAP_ROW(kSnapRootSq, D.root_sq + sb * 96, 96);
    SNAP_ROW(kSnapChain, D.chain + sb * kChainCap, kChainCap * 8);
    SNAP_ROW(kSnapChainChk, D.chain_chk + sb * 2, 16);
    SNAP_ROW(kSnapGmG, D.gm_g + sb * kMaxLegal, kMaxLegal * 8);
    SNAP_ROW(kSnapGmLogit, D.gm_logit + sb * kMaxLegal, kMaxLegal * 8);
    SNAP_ROW(kSnapGmN0, D.gm_n0 + sb * kMaxLegal, kMaxLegal * 4);
    SNAP_ROW(kSnapExDir, D.ex_dir + sb * kMaxLegal, kMaxLegal * 4);
    SNAP_ROW(kSnapEsSnap, D.es_snap + sb * kMaxLegal, kMaxLegal * 4);
    SNAP_ROW(kSnapGmStamp, D.gm_stamp + sb * 4, 16);
#undef SNAP_ROW
    // the rows that are no multiple of 16 bytes: moved without padding (the row behind starts inside the same 16 bytes)
#define SNAP_SMALL(OFF_, PTR_, BYTES_)                                                        \
    do {                                                                                      \
        if (PACK) snap_copy(o + (OFF_), (const uint8_t *)(PTR_), (size_t)(BYTES_), t, nt);    \
        else snap_copy((uint8_t *)(PTR_), o + (OFF_), (size_t)(BYTES_), t, nt);               \
    } while (0)
    SNAP_SMALL(kSnapStats, D.stats + sb, sizeof(BoardStats));
    SNAP_SMALL(kSnapRsStats, D.rs_stats + sb, sizeof(ResignBoardStats));
    SNAP_SMALL(kSnapExStats, D.ex_stats + sb, sizeof(ExploreBoardStats));
    SNAP_SMALL(kSnapSvStats, D.sv_stats + sb, sizeof(SolverBoardStats));
    SNAP_SMALL(kSnapGmStats, D.gm_stats + sb, sizeof(GumbelBoardStats));
    SNAP_SMALL(kSnapEsStats, D.es_stats + sb, sizeof(StopBoardStats));
    if (wide) SNAP_SMALL(kSnapWideStats, wide + sb, sizeof(WideBoardStats));
    else if (PACK) for (int i = t; i < (int)sizeof(WideBoardStats); i += nt) o[kSnapWideStats + i] = 0;
    SNAP_SMALL(kSnapExStamp, D.ex_stamp + sb * 2, 8);
    SNAP_SMALL(kSnapBudget, D.budget + sb, 4);
    SNAP_SMALL(kSnapMoveSims, D.move_sims + sb, 4);
    SNAP_SMALL(kSnapRsFire, D.rs_fire + sb, 4);
    SNAP_SMALL(kSnapRsLast, D.rs_last + sb, 4);
    SNAP_SMALL(kSnapEsSnapS, D.es_snap_s + sb, 4);
    SNAP_SMALL(kSnapTarget, D.target + sb, 1);
    SNAP_SMALL(kSnapRsState, D.rs_state + sb, 1);
    SNAP_SMALL(kSnapRsRun, D.rs_run + sb * 2, 2);
    SNAP_SMALL(kSnapEsStopped, D.es_stopped + sb, 1);
#undef SNAP_SMALL
    if (PACK) for (int i = kSnapFixedUsed + t; i < kSnapFixed; i += nt) o[i] = 0;

    // the three prefixes
    const size_t nn = (size_t)m.n_nodes, pl = (size_t)m.ply, pu = (size_t)m.pi_used;
    const size_t nbase = (sb * 2 + (size_t)half) * (size_t)D.cap, rbase = sb * (size_t)D.max_plies, pbase = sb * (size_t)D.pi_cap;
    uint64_t p = (uint64_t)kSnapFixed;
    p = snap_array<PACK>(o, p, D.nodeA + nbase, nn * 16, t, nt);
    p = snap_array<PACK>(o, p, D.nodeB + nbase, nn * 4, t, nt);
    if (sections & kSnapProof) p = snap_array<PACK>(o, p, proof ? proof + nbase : nullptr, nn, t, nt);
    else if (!PACK && proof) for (size_t i = (size_t)t; i < nn; i += (size_t)nt) proof[nbase + i] = 0; // saved without proof bytes: all unknown
    p = snap_array<PACK>(o, p, D.rec_sq + rbase * 96, pl * 96, t, nt);
    p = snap_array<PACK>(o, p, D.rec_off + rbase, pl * 4, t, nt);
    p = snap_array<PACK>(o, p, D.rec_turn + rbase, pl, t, nt);
    p = snap_array<PACK>(o, p, D.rec_k + rbase, pl, t, nt);
    p = snap_array<PACK>(o, p, D.rec_target + rbase, pl, t, nt);
    if (sections & kSnapValues) {
        p = snap_array<PACK>(o, p, D.rec_value + rbase, pl * 4, t, nt);
        p = snap_array<PACK>(o, p, D.rec_hasv + rbase, pl, t, nt);
    }
    if (sections & kSnapSurprise) {
        const SurpriseBlock *sp = surprise_block(D);
        p = snap_array<PACK>(o, p, sp->rec_kl + rbase, pl * 4, t, nt);
        p = snap_array<PACK>(o, p, sp->rec_hask + rbase, pl, t, nt);
        p = snap_array<PACK>(o, p, sp->sp_stats + sb, sizeof(SurpriseBoardStats), t, nt);
    }
    p = snap_array<PACK>(o, p, D.rec_ids + pbase, pu * 2, t, nt);
    p = snap_array<PACK>(o, p, D.rec_pi + pbase, pu * 4, t, nt);
}

// One workgroup per board: the engine's live bytes -> the board's section. The tree is read from the board's own pool half (a board
// that is over was left behind when the halves flipped: meta.half says where its n_nodes nodes are).
__global__ __launch_bounds__(256) void k_snapshot_pack(Dev D, const uint64_t *offsets, uint8_t *sections_base, uint32_t sections, uint8_t *proof,
                                                         WideBoardStats *wide)
{
    const int b = blockIdx.x;
    const BoardMeta m = D.meta[b];
    snap_section<true>(D, b, m, (int)(m.half & 1), sections_base + offsets[b], sections, proof, wide, (int)threadIdx.x, (int)blockDim.x);
}

// One workgroup per board: the board's section -> the engine's arrays. Every tree lands in the pool half the engine's half word names
// (the word is not written: no pointer and no word a captured graph holds changes), and meta.half is set to it. What a move boundary
// guarantees is restored with it: no pending leaf, an empty selection path.
__global__ __launch_bounds__(256) void k_snapshot_unpack(Dev D, const uint64_t *offsets, const BoardMeta *meta, uint8_t *sections_base, uint32_t sections,
                                                           uint8_t *proof, WideBoardStats *wide)
{
    const int b = blockIdx.x;
    BoardMeta m = meta[b];
    const int half = *D.half & 1;
    snap_section<false>(D, b, m, half, sections_base + offsets[b], sections, proof, wide, (int)threadIdx.x, (int)blockDim.x);
    if (threadIdx.x == 0) {
        m.half = (uint8_t)half;
        D.meta[b] = m;
        D.leaf_status[b] = CCZ_LEAF_SKIP;
        D.leaf_k[b] = 0;
        D.path_len[b] = 0;
    }
}

} // namespace ccz
