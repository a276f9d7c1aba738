// cczero.hip -- C ABI (include/cczero.h) of the gfx950 lockstep self-play rollout engine.
//
// Host side: memory layout in HBM, launches on the caller's stream, error reporting. There is no
// CPU fallback anywhere in this file: without a usable HIP device every compute entry point fails.
#include "../../include/cczero.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

#include "cczero_kernels.h"
#include "cczero_history.h"
#include "cczero_mate.h"
#include "cczero_netops.h"
#include "cczero_conv.h"
#include "cczero_conv_small.h"
#include "cczero_conv_narrow.h"
#include "cczero_conv_g16.h"
#include "cczero_conv_g16e.h"
#include "cczero_heads.h"
#include "cczero_snapshot.h"

using namespace ccz;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) return fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

constexpr Tables h_tab = make_tables();

template <typename T>
hipError_t dalloc(T **p, size_t n, std::vector<void *> &owned, size_t &total)
{
    void *q = nullptr;
    const size_t bytes = n * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
    if (e != hipSuccess) return e;
    e = hipMemset(q, 0, bytes ? bytes : 16);
    if (e != hipSuccess) return e;
    owned.push_back(q);
    total += bytes;
    *p = (T *)q;
    return hipSuccess;
}

} // namespace

struct ccz_engine {
    ccz_config cfg;
    Dev d;
    std::vector<void *> owned;
    size_t bytes = 0;
    // staging (device) for the sync'ing accessors
    int32_t *st_k = nullptr, *st_visits = nullptr, *st_rootn = nullptr;
    uint16_t *st_acts = nullptr;
    float *st_q = nullptr, *st_p = nullptr;
    double *st_pi = nullptr, *st_temps = nullptr;
    double *st_g = nullptr, *st_u = nullptr; // ccz_move_distribution (allocated at its first call)
    long long *st_rowbase = nullptr;
    uint8_t *st_mask = nullptr, *st_sq = nullptr;
    std::vector<BoardMeta> h_meta;
    int active = 0; // boards 0 .. active - 1 are searched; the rest are scout slots (ccz_set_scouts); 0 = all
    // two evaluators on one engine (ccz_set_routing): which one plays red on each board, which one owns each board's pending search
    bool routed = false;
    uint8_t *route_red = nullptr;  // [B] device
    uint8_t *route_net = nullptr;  // [B] device: written by k_cache_probe_routed, read by the plan and the gather
    uint64_t salt[2] = {0, 0};
    bool budgets_on = false;       // ccz_set_budgets / ccz_draw_budgets (off: every budget INT32_MAX, every target 1)
    bool explore_on = false;       // ccz_set_root_exploration(enabled): the host's shadow of ExploreCfg.enabled (scouts are refused with it)
    bool search_on = false;        // ccz_set_search(enabled): the host's shadow of SearchCfg.enabled (scouts are refused with it)
    bool stop_on = false;          // ccz_set_early_stop(enabled): the host's shadow of StopCfg.enabled (scouts, a width above 1 and the Gumbel root are refused with it)
    int32_t *st_count = nullptr;   // ccz_searching: the count on the device
    bool gumbel_on = false;        // ccz_set_gumbel(enabled): the host's shadow of GumbelCfg.enabled (scouts and root exploration are refused with it)
    SurpriseBlock *sp_block = nullptr; // device: the surprise settings and array pointers, behind the resignation settings (BoundaryCfg)
    SurpriseBlock sp_host = {};        // the host's copy of the pointers (cfg stays zero here: the device's is the truth)
    bool surprise_on = false;      // ccz_set_surprise(enabled): the host's shadow of SurpriseCfg.enabled (scouts are refused with it; a snapshot gets its section)
    bool history_on = false;       // ccz_set_leaf_history(enabled): every select phase is followed by k_leaf_history (scouts and a width above 1 are refused with it)
    // MCTS-solver (ccz_set_solver): the proof bytes [B][2][cap] (allocated by the first call that turns it on), the host's shadow of
    // SolverCfg.enabled, staging of ccz_root_proof (state [B], dist [B], child state [B][128], child dist [B][128])
    uint8_t *proof = nullptr, *st_proof = nullptr;
    bool solver_on = false;
    // value spread (ccz_set_value_stats): S [B][2][cap] floats (allocated by the first call that turns it on), the host's shadow of
    // SolverCfg.spread, staging of ccz_root_value_stats (children [B][128], root [B])
    float *spread_S = nullptr, *st_spread = nullptr;
    bool spread_on = false;
    // wide search (ccz_set_width): slots per board (1: off; above 1 `active` = n_boards / width), the in-flight counts F [B][2][cap] and
    // the per-board counters (both allocated by the first call that turns it on), staging of ccz_get_wide_stats
    int width = 1;
    uint8_t *wide_F = nullptr;
    WideBoardStats *wide_stats = nullptr;
    unsigned long long *st_wide = nullptr;
    // engine snapshots (ccz_snapshot_*): a hash of the move-rank table (0: none), the section offsets on the device [B + 1] (allocated at
    // the first call), and the host's side of a save / load: the header and the directory (offsets, then meta)
    uint64_t rank_hash = 0;
    uint64_t *snap_off = nullptr;
    SnapHeader snap_hdr;
    std::vector<uint64_t> snap_dir;
};

#define ACTIVE(e) ((unsigned)((e)->active > 0 ? (e)->active : (e)->d.B))
#define SCOUTS(e) ((e)->active > 0 && (e)->width == 1) // the slots past `active` are scout slots (not the leaves of a wide search)
#define WIDE(e) ((e)->width > 1)
// the sequential step calls of a wide engine would silently use slot 0 of each board
#define NOT_WIDE(e) do { if (WIDE(e)) return fail(-1, "%s: not while the width is %d (ccz_set_width): a wide engine steps with ccz_select_wide / ccz_step_wide", __func__, (e)->width); } while (0)
static WideArgs wide_args(const ccz_engine *e) { return WideArgs{e->active, e->width, e->wide_F, e->wide_stats}; }

// one record of counters per board, read back for the caller to sum (syncs)
template <typename T> static int fetch_board_stats(ccz_engine *e, hipStream_t s, const T *dev, std::vector<T> &st)
{
    st.resize((size_t)e->d.B);
    HIP_TRY(hipMemcpyAsync(st.data(), dev, st.size() * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// ---- the launches of the group-of-16 tower kernels (cczero_conv_g16.h, cczero_conv_g16e.h) ----
// ccz_set_search off: what ccz_create writes and ccz_get_search reads back (c_base: AlphaZero's; it is idle while c_factor is 0)
static SearchCfg search_defaults()
{
    SearchCfg v;
    v.enabled = 0; v.fpu_mode = 0; v.fpu_root_mode = 0; v.pad = 0;
    v.fpu_value = 0.0; v.fpu_root_value = 0.0; v.c_base = 19652.0; v.c_factor = 0.0;
    return v;
}

static bool g16_bad_part(int32_t part, int32_t n_parts) { return n_parts < 1 || n_parts > 256 || part < 0 || part >= n_parts; }

// The launch shape of a layer of `groups` 16-board groups. Without CCZ_CONV_G16_EDGE_TILES (or below two groups): `mid` = five two-rank
// tiles per group, no edge tiles. With it: `mid` = four middle tiles per group (ranks 1..8; two-rank or quad), `edge` = one edge-pair
// tile per side and pair of groups (ranks 0 and 9, cczero_conv_g16e.h) -- in their own launch or, CCZ_CONV_G16_ONE_LAUNCH, as slots
// [mid, mid + edge) of the same.
struct G16Shape {
    unsigned mid, edge;
};
static G16Shape g16_shape(int groups, int flags)
{
    const bool split = (flags & CCZ_CONV_G16_EDGE_TILES) && groups >= 2;
    return {(unsigned)(groups * (split ? 4 : 5)), split ? 2u * (unsigned)((groups + 1) / 2) : 0u};
}

// What every tower kernel of a layer is launched with; one launch = `grid` tile slots of 512 threads. `tail`: the heads kernels' G5Heads.
struct G16Args {
    const _Float16 *x, *w;
    const float *bias;
    const _Float16 *res;
    _Float16 *y;
    int n_pixels, cin;
    const int *live_rows;
    int row0;
};
template <typename Kernel, typename... Tail> static void g16_launch(Kernel kernel, unsigned grid, hipStream_t s, const G16Args &a, int flags, Tail... tail)
{
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(512), 0, s, a.x, a.w, a.bias, a.res, a.y, a.n_pixels, flags, a.cin, a.live_rows, a.row0, tail...);
}
// (a kernel with and without the residual read: two instantiations)
#define CCZ_G16_RES(KERNEL_, RES_) ((RES_) ? KERNEL_<true> : KERNEL_<false>)

extern "C" {

int ccz_abi_version(void) { return CCZ_ABI_VERSION; }
const char *ccz_last_error(void) { return g_err; }

int ccz_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ccz_action_table(char *uci, uint8_t *from, uint8_t *to)
{
    for (int i = 0; i < kNMoves; ++i) {
        const int fr = h_tab.from[i], t = h_tab.to[i];
        if (uci) {
            uci[i * 5 + 0] = (char)('a' + fr % 9);
            uci[i * 5 + 1] = (char)('0' + fr / 9);
            uci[i * 5 + 2] = (char)('a' + t % 9);
            uci[i * 5 + 3] = (char)('0' + t / 9);
            uci[i * 5 + 4] = 0;
        }
        if (from) from[i] = (uint8_t)fr;
        if (to) to[i] = (uint8_t)t;
    }
    return 0;
}

int ccz_flip_map(int32_t *flip)
{
    if (!flip) return fail(-1, "ccz_flip_map: null output");
    for (int i = 0; i < kNMoves; ++i) flip[i] = h_tab.flip[i];
    return 0;
}

int ccz_create(const ccz_config *cfg, ccz_engine **out)
{
    if (!cfg || !out) return fail(-1, "ccz_create: null argument");
    if (cfg->n_boards <= 0) return fail(-1, "ccz_create: n_boards must be > 0");
    // the sampler's parameters, checked before any device work: out of range, the noise and pi are NaN or meaningless
    if (!(cfg->eps >= 0.0f && cfg->eps <= 1.0f)) return fail(-1, "ccz_create: eps %g must be in [0, 1]", (double)cfg->eps);
    if (!(cfg->alpha > 0.0f && std::isfinite(cfg->alpha))) return fail(-1, "ccz_create: alpha %g must be finite and > 0", (double)cfg->alpha);
    if (!(cfg->temp > 0.0f)) return fail(-1, "ccz_create: temp %g must be > 0", (double)cfg->temp);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(-3, "ccz_create: no HIP device available (the engine has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(-1, "ccz_create: device %d out of range (%d devices)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));
    ccz_engine *e = new (std::nothrow) ccz_engine();
    if (!e) return fail(-4, "ccz_create: out of host memory");
    e->cfg = *cfg;
    Dev &d = e->d;
    d.B = cfg->n_boards;
    // nodes per pool half: every playout creates <= ~k children; the retained subtree adds to it
    const int n_play = cfg->n_playout > 0 ? cfg->n_playout : 400;
    // nodes per pool half: a move adds <= n_playout expansions of ~40 children; the subtree kept across moves adds to
    // it (concentrated searches keep most of the tree: 97 k nodes were seen after 45 moves at 400 sims). Sized for
    // the HBM at hand (288 GB): 512 nodes per simulation of a move, 39 GB at 4096 boards x 400 sims.
    d.cap = cfg->max_nodes > 0 ? cfg->max_nodes : (n_play + 64) * 512;
    if (d.cap < 130) d.cap = 130; // root + one full expansion (the root's children are prefetched unconditionally)
    d.reserve = n_play * 128 < d.cap / 2 ? n_play * 128 : d.cap / 2;
    if (cfg->reserve_nodes > 0) d.reserve = cfg->reserve_nodes < d.cap - 129 ? cfg->reserve_nodes : d.cap - 129;
    d.maxd = cfg->max_depth > 0 ? cfg->max_depth : kMaxDepth;
    if (d.maxd > kMaxDepth) { delete e; return fail(-1, "ccz_create: max_depth %d exceeds the compiled limit %d", d.maxd, kMaxDepth); }
    if (d.maxd < 64) { delete e; return fail(-1, "ccz_create: max_depth must be >= 64"); }
    d.max_plies = cfg->max_plies > 0 ? cfg->max_plies : 2048;
    d.pi_cap = d.max_plies * 80; // sparse pi entries: opening positions have 44 legal moves, open middlegames 50-70
    d.c_puct = cfg->c_puct;
    d.eps = (double)cfg->eps;
    d.alpha = (double)cfg->alpha;
    d.temp = (double)cfg->temp;
    d.flags = cfg->flags;
    d.seed = cfg->seed;
    d.board_id_base = cfg->board_id_base;
    // ---- run-time rule tables (ABI 2)
    if ((cfg->flags & CCZ_FLAG_CACHE_VERIFY) && !cfg->eval_cache_log2) { delete e; return fail(-1, "ccz_create: CCZ_FLAG_CACHE_VERIFY without an evaluation cache (eval_cache_log2)"); }
    if (cfg->flags & ~(CCZ_FLAG_REFERENCE_QUIRKS | CCZ_FLAG_NO_MIRROR | CCZ_FLAG_VALUE_F16 | CCZ_FLAG_CACHE_VERIFY | CCZ_FLAG_STRICT)) { delete e; return fail(-1, "ccz_create: unknown flags 0x%x", cfg->flags); }
    if (cfg->eval_cache_log2 && (cfg->eval_cache_log2 < 10 || cfg->eval_cache_log2 > 28)) { delete e; return fail(-1, "ccz_create: eval_cache_log2 must be 0 (no cache) or 10..28"); }
    if (cfg->rule_flags & ~(CCZ_RULE_PERPETUAL_CHECK | CCZ_RULE_PAWN_MOVE_RESETS_CLOCK)) { delete e; return fail(-1, "ccz_create: unknown rule_flags 0x%x", cfg->rule_flags); }
    d.rule_flags = cfg->rule_flags;
    {
        uint8_t pot[8] = {0, 0, 1, 2, 3, 4, 5, 6};
        bool all_zero = true;
        for (int t = 0; t < 8; ++t) all_zero = all_zero && cfg->plane_of_type[t] == 0;
        if (!all_zero) {
            unsigned seen = 0;
            for (int t = 1; t <= 7; ++t) {
                const int c = cfg->plane_of_type[t];
                if (c > 6 || (seen >> c & 1u)) { delete e; return fail(-1, "ccz_create: plane_of_type[1..7] must be a permutation of 0..6"); }
                seen |= 1u << c;
                pot[t] = (uint8_t)c;
            }
        }
        d.chanpack = d.typepack = 0;
        for (int t = 1; t <= 7; ++t) {
            d.chanpack |= (uint32_t)pot[t] << (3 * t);
            d.typepack |= (uint32_t)(t - 1) << (3 * pot[t]);
        }
    }
    d.trankpack = 0;
    for (int t = 1; t <= 7; ++t) {
        if (cfg->type_rank[t] > 7) { delete e; return fail(-1, "ccz_create: type_rank[%d] must be 0..7", t); }
        d.trankpack |= (uint32_t)cfg->type_rank[t] << (3 * t);
    }
    std::vector<uint16_t> h_rank, h_unrank;
    if (cfg->move_rank_host) {
        h_rank.assign(cfg->move_rank_host, cfg->move_rank_host + kNMoves);
        h_unrank.assign(kNMoves, 0xffff);
        for (int i = 0; i < kNMoves; ++i) {
            if (h_rank[i] >= kNMoves || h_unrank[h_rank[i]] != 0xffff) { delete e; return fail(-1, "ccz_create: move_rank_host must be a permutation of 0..2085 (entry %d)", i); }
            h_unrank[h_rank[i]] = (uint16_t)i;
        }
        e->rank_hash = 0xcbf29ce484222325ull; // FNV-1a over the table's entries: what a snapshot's header says of it
        for (int i = 0; i < kNMoves; ++i) e->rank_hash = (e->rank_hash ^ (uint64_t)h_rank[i]) * 0x100000001b3ull;
    }
    const size_t B = (size_t)d.B;
    hipError_t he = hipSuccess;
#define ALLOC(ptr, n)                                                        \
    if (he == hipSuccess) he = dalloc(&(ptr), (size_t)(n), e->owned, e->bytes)
    ALLOC(d.nodeA, B * 2 * d.cap);
    ALLOC(d.nodeB, B * 2 * d.cap);
    ALLOC(d.meta, B);
    ALLOC(d.root_sq, B * 96);
    ALLOC(d.chain, B * kChainCap);
    ALLOC(d.chain_chk, B * 2);
    ALLOC(d.path, B * d.maxd);
    ALLOC(d.path_len, B);
    ALLOC(d.leaf_ids, B * kMaxLegal);
    ALLOC(d.leaf_k, B);
    ALLOC(d.leaf_status, B);
    ALLOC(d.leaf_key, B);
    d.cache = nullptr;
    d.cache_mask = 0;
    if (cfg->eval_cache_log2) {
        const size_t slots = (size_t)1 << cfg->eval_cache_log2;
        d.cache_mask = (uint32_t)(slots - 1);
        ALLOC(d.cache, slots);
        ALLOC(d.claim, slots);
        ALLOC(d.cslot, B);
        ALLOC(d.ctag, B);
        ALLOC(d.cstate, B);
        ALLOC(d.cins, B);
        ALLOC(d.cver, B);
        ALLOC(d.crep, B);
        ALLOC(d.row_of, B);
        ALLOC(d.vleaf, B);
        if (he == hipSuccess) he = hipMemset(d.claim, 0x7f, slots * 4);
    }
    ALLOC(d.rec_sq, B * d.max_plies * 96);
    ALLOC(d.rec_turn, B * d.max_plies);
    ALLOC(d.rec_k, B * d.max_plies);
    ALLOC(d.rec_off, B * d.max_plies);
    ALLOC(d.rec_target, B * d.max_plies);
    ALLOC(d.budget, B);
    ALLOC(d.move_sims, B);
    ALLOC(d.target, B);
    BoundaryCfg *bd_cfg = nullptr;
    ALLOC(bd_cfg, 1); // zeroed: resignation off, policy surprise weighting off (its array pointers are written below)
    d.rs_cfg = bd_cfg ? &bd_cfg->resign : nullptr;
    e->sp_block = bd_cfg ? &bd_cfg->surprise : nullptr;
    ALLOC(d.rs_state, B);
    ALLOC(d.rs_run, B * 2);
    ALLOC(d.rs_fire, B);
    ALLOC(d.rs_last, B);
    ALLOC(d.rec_value, B * d.max_plies);
    ALLOC(d.rec_hasv, B * d.max_plies);
    ALLOC(d.rs_stats, B);
    ExploreCfg *ex_cfg = nullptr;
    ALLOC(ex_cfg, 1); // zeroed: root exploration off
    d.ex_cfg = ex_cfg;
    ALLOC(d.ex_dir, B * kMaxLegal);
    ALLOC(d.ex_stamp, B * 2);
    ALLOC(d.ex_stats, B);
    SolverBlock *sv_block = nullptr;
    ALLOC(sv_block, 1); // zeroed: solver off, no proof array; value spread off, no S array
    d.sv_cfg = &sv_block->cfg;
    ALLOC(d.sv_stats, B);
    GumbelCfg *gm_cfg = nullptr;
    ALLOC(gm_cfg, 1); // zeroed: Gumbel root search off
    d.gm_cfg = gm_cfg;
    ALLOC(d.gm_g, B * kMaxLegal);
    ALLOC(d.gm_logit, B * kMaxLegal);
    ALLOC(d.gm_n0, B * kMaxLegal);
    ALLOC(d.gm_stamp, B * 4);
    ALLOC(d.gm_stats, B);
    SearchCfg *sr_cfg = nullptr;
    ALLOC(sr_cfg, 1); // off; the defaults are written below
    d.sr_cfg = sr_cfg;
    {
        const SearchCfg off = search_defaults();
        if (he == hipSuccess) he = hipMemcpy(sr_cfg, &off, sizeof off, hipMemcpyHostToDevice);
    }
    StopCfg *es_cfg = nullptr;
    ALLOC(es_cfg, 1); // zeroed: early stop off
    d.es_cfg = es_cfg;
    ALLOC(d.es_stopped, B);
    ALLOC(d.es_snap_s, B); // (k_reset below writes the -1 of "no snapshot")
    ALLOC(d.es_snap, B * kMaxLegal);
    ALLOC(d.es_stats, B);
    ALLOC(e->sp_host.rec_kl, B * d.max_plies);
    ALLOC(e->sp_host.rec_hask, B * d.max_plies);
    ALLOC(e->sp_host.sp_stats, B);
    if (he == hipSuccess) he = hipMemcpy(e->sp_block, &e->sp_host, sizeof e->sp_host, hipMemcpyHostToDevice); // (cfg zeros: off)
    ALLOC(e->st_count, 4);
    ALLOC(d.rec_ids, B * d.pi_cap);
    ALLOC(d.rec_pi, B * d.pi_cap);
    ALLOC(d.stats, B);
    ALLOC(d.err, 4);
    ALLOC(d.half, 4);
    ALLOC(d.prior128, B * kMaxLegal);
    ALLOC(d.stamps, B * 16);
    ALLOC(e->st_k, B);
    ALLOC(e->st_visits, B * kMaxLegal);
    ALLOC(e->st_rootn, B);
    ALLOC(e->st_acts, B * kMaxLegal);
    ALLOC(e->st_q, B * kMaxLegal);
    ALLOC(e->st_p, B * kMaxLegal);
    ALLOC(e->st_pi, B * kMaxLegal);
    ALLOC(e->st_temps, B);
    ALLOC(e->st_rowbase, B);
    ALLOC(e->st_mask, B);
    ALLOC(e->st_sq, 96);
    uint16_t *d_rank = nullptr, *d_unrank = nullptr;
    if (!h_rank.empty()) {
        ALLOC(d_rank, kNMoves);
        ALLOC(d_unrank, kNMoves);
        if (he == hipSuccess) he = hipMemcpy(d_rank, h_rank.data(), kNMoves * 2, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipMemcpy(d_unrank, h_unrank.data(), kNMoves * 2, hipMemcpyHostToDevice);
    }
    d.rank = d_rank;
    d.unrank = d_unrank;
#undef ALLOC
    if (he != hipSuccess) {
        for (void *p : e->owned) (void)hipFree(p);
        const size_t got = e->bytes;
        delete e;
        return fail(-2, "ccz_create: device allocation failed after %zu bytes: %s", got, hipGetErrorString(he));
    }
    e->h_meta.resize(B);
    hipLaunchKernelGGL(k_set_budgets, dim3((d.B + 255) / 256), dim3(256), 0, 0, d, d.B, (const int32_t *)nullptr, (const uint8_t *)nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_reset, dim3(d.B), dim3(64), 0, 0, d, (const uint8_t *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    *out = e;
    return 0;
}

int ccz_destroy(ccz_engine *e)
{
    if (!e) return 0;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    for (void *p : e->owned) (void)hipFree(p);
    delete e;
    return 0;
}

#define NEED(e) do { if (!(e)) return fail(-1, "%s: null engine", __func__); } while (0)

// the caller's host mask on the device: *mask = st_mask, null without one. st_mask is reused by the next call, so a caller that passed a
// mask syncs after its launch
static int stage_mask(ccz_engine *e, hipStream_t s, const uint8_t *mask_host, const uint8_t **mask)
{
    if (mask_host) HIP_TRY(hipMemcpyAsync(e->st_mask, mask_host, (size_t)e->d.B, hipMemcpyHostToDevice, s));
    *mask = mask_host ? e->st_mask : nullptr;
    return 0;
}

// The move boundary of a wide engine (width > 1 only: one extra launch): the pending leaves of the boards about to be reset, reloaded or
// moved leave the in-flight counts, their slots get CCZ_LEAF_NONE. mask: the staged device mask or null; only >= 0: that board alone
static int wide_drop(ccz_engine *e, hipStream_t s, const uint8_t *mask, int only)
{
    if (!WIDE(e)) return 0;
    hipLaunchKernelGGL(k_wide_drop, dim3((unsigned)((e->active + 63) / 64)), dim3(64), 0, s, e->d, wide_args(e), mask, only);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_reset(ccz_engine *e, void *stream, const uint8_t *mask_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *mask;
    if (const int rc = stage_mask(e, s, mask_host, &mask)) return rc;
    if (const int rc = wide_drop(e, s, mask, -1)) return rc;
    hipLaunchKernelGGL(k_reset, dim3(e->d.B), dim3(64), 0, s, e->d, mask);
    HIP_TRY(hipGetLastError());
    if (mask_host) HIP_TRY(hipStreamSynchronize(s)); // st_mask is reused by the next call
    return 0;
}

int ccz_set_position(ccz_engine *e, void *stream, int32_t board, const uint8_t *sq_host, int32_t turn, int32_t halfmove)
{
    NEED(e);
    if (board < 0 || board >= e->d.B || !sq_host) return fail(-1, "ccz_set_position: bad board index or null squares");
    int kings[2] = {0, 0};
    for (int i = 0; i < 90; ++i) {
        const int pc = sq_host[i];
        if (pc > 15 || pc == 8) return fail(-1, "ccz_set_position: bad piece code %d on square %d", pc, i);
        if ((pc & 7) == KING && pc) kings[pc >> 3]++;
    }
    if (kings[0] != 1 || kings[1] != 1) return fail(-1, "ccz_set_position: each side needs exactly one king");
    if (halfmove < 0) return fail(-1, "ccz_set_position: negative halfmove clock");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(e->st_sq, sq_host, 90, hipMemcpyHostToDevice, s));
    if (const int rc = wide_drop(e, s, nullptr, board)) return rc;
    hipLaunchKernelGGL(k_set_position, dim3(1), dim3(64), 0, s, e->d, board, (const uint8_t *)e->st_sq, turn ? 1 : 0, halfmove);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_set_positions(ccz_engine *e, void *stream, const uint8_t *sq_dev, const uint8_t *turn_dev, const int32_t *halfmove_dev,
                      const int32_t *moves_dev, const int32_t *n_moves_dev, int32_t max_moves, const uint8_t *mask_host, int32_t *status_dev)
{
    NEED(e);
    if (!sq_dev || !turn_dev || !status_dev) return fail(-1, "ccz_set_positions: null squares / turn / status");
    if (((uintptr_t)sq_dev) & 3) return fail(-1, "ccz_set_positions: the squares must be 4-byte aligned");
    if (max_moves < 0) return fail(-1, "ccz_set_positions: negative max_moves");
    if (n_moves_dev && !moves_dev && max_moves > 0) return fail(-1, "ccz_set_positions: n_moves without moves");
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *mask;
    if (const int rc = stage_mask(e, s, mask_host, &mask)) return rc;
    if (const int rc = wide_drop(e, s, mask, -1)) return rc;
    hipLaunchKernelGGL(k_set_positions, dim3(e->d.B), dim3(64), 0, s, e->d, mask, sq_dev, turn_dev, halfmove_dev, moves_dev, n_moves_dev,
                       (int)max_moves, status_dev);
    HIP_TRY(hipGetLastError());
    if (mask_host) HIP_TRY(hipStreamSynchronize(s)); // st_mask is reused by the next call
    return 0;
}

int ccz_reset_tree(ccz_engine *e, void *stream, const uint8_t *mask_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *mask;
    if (const int rc = stage_mask(e, s, mask_host, &mask)) return rc;
    if (const int rc = wide_drop(e, s, mask, -1)) return rc;
    hipLaunchKernelGGL(k_reset_tree, dim3((e->d.B + 255) / 256), dim3(256), 0, s, e->d, mask);
    HIP_TRY(hipGetLastError());
    if (mask_host) HIP_TRY(hipStreamSynchronize(s)); // st_mask is reused by the next call
    return 0;
}

int ccz_zero_leaf_input(ccz_engine *e, void *stream, void *leaf_input_f16_dev)
{
    NEED(e);
    if (!leaf_input_f16_dev) return fail(-1, "ccz_zero_leaf_input: null buffer");
    HIP_TRY(hipMemsetAsync(leaf_input_f16_dev, 0, (size_t)e->d.B * CCZ_PLANES * 2, (hipStream_t)stream));
    return 0;
}

// ccz_set_leaf_history on: the rows and keys of the select phase just launched are rewritten with the boards' histories (off: no launch)
static int leaf_history(ccz_engine *e, hipStream_t s, void *leaf_input_f16_dev)
{
    if (!e->history_on) return 0;
    if (!leaf_input_f16_dev) return fail(-1, "leaf history is on (ccz_set_leaf_history): the select phase needs a leaf input tensor");
    hipLaunchKernelGGL(k_leaf_history, dim3(ACTIVE(e)), dim3(64), 0, s, e->d, (uint16_t *)leaf_input_f16_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_set_leaf_history(ccz_engine *e, void *stream, int32_t enabled)
{
    NEED(e);
    (void)stream; // the setting lives on the host: it decides which launches the next select phase is made of
    if (enabled) {
        if (SCOUTS(e)) return fail(-1, "ccz_set_leaf_history: not with scout slots (ccz_set_scouts): a scout's leaf has no path of its own to replay");
        if (WIDE(e)) return fail(-1, "ccz_set_leaf_history: not while the width is %d (ccz_set_width)", e->width);
        if (e->d.flags & CCZ_FLAG_REFERENCE_QUIRKS)
            return fail(-1, "ccz_set_leaf_history: not on a CCZ_FLAG_REFERENCE_QUIRKS engine: its training rows alias the final history, which no search sees");
    }
    e->history_on = enabled != 0;
    return 0;
}

int ccz_get_leaf_history(ccz_engine *e, int32_t *enabled_host)
{
    NEED(e);
    if (!enabled_host) return fail(-1, "ccz_get_leaf_history: null output");
    *enabled_host = e->history_on ? 1 : 0;
    return 0;
}

int ccz_select_leaves(ccz_engine *e, void *stream, void *leaf_input_f16_dev)
{
    NEED(e);
    NOT_WIDE(e);
    hipLaunchKernelGGL(k_select, dim3(ACTIVE(e)), dim3(64), 0, (hipStream_t)stream, e->d, (uint16_t *)leaf_input_f16_dev);
    HIP_TRY(hipGetLastError());
    return leaf_history(e, (hipStream_t)stream, leaf_input_f16_dev);
}

int ccz_expand_backup(ccz_engine *e, void *stream, const float *prob_dev, const float *value_dev)
{
    NEED(e);
    NOT_WIDE(e);
    if (!prob_dev || !value_dev) return fail(-1, "ccz_expand_backup: null prob/value");
    hipLaunchKernelGGL(k_expand_backup<false>, dim3(ACTIVE(e)), dim3(64), 0, (hipStream_t)stream, e->d, prob_dev, value_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_step(ccz_engine *e, void *stream, const float *prob_dev, const float *value_dev, void *leaf_input_f16_dev)
{
    NEED(e);
    NOT_WIDE(e);
    if (!prob_dev || !value_dev) return fail(-1, "ccz_step: null prob/value");
    hipLaunchKernelGGL(k_step<false>, dim3(ACTIVE(e)), dim3(64), 0, (hipStream_t)stream, e->d, prob_dev, value_dev,
                       (uint16_t *)leaf_input_f16_dev);
    HIP_TRY(hipGetLastError());
    return leaf_history(e, (hipStream_t)stream, leaf_input_f16_dev);
}

int ccz_gather_priors(ccz_engine *e, void *stream, const void *logits_dev, int32_t logits_f16)
{
    NEED(e);
    if (!logits_dev) return fail(-1, "ccz_gather_priors: null logits");
    hipStream_t s = (hipStream_t)stream;
    if (logits_f16)
        hipLaunchKernelGGL((k_softmax_gather<_Float16, false>), dim3(e->d.B), dim3(64), 0, s, e->d, (const _Float16 *)logits_dev, (const float *)nullptr);
    else
        hipLaunchKernelGGL((k_softmax_gather<float, false>), dim3(e->d.B), dim3(64), 0, s, e->d, (const float *)logits_dev, (const float *)nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_eval_plan(ccz_engine *e, void *stream, int32_t *miss_rows_dev, int32_t *n_miss_dev)
{
    NEED(e);
    if (!e->d.cache) return fail(-1, "ccz_eval_plan: the engine was created without an evaluation cache (ccz_config.eval_cache_log2)");
    if (!miss_rows_dev || !n_miss_dev) return fail(-1, "ccz_eval_plan: null output");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cache_probe, dim3(e->d.B), dim3(64), 0, s, e->d);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cache_plan, dim3(1), dim3(1024), 0, s, e->d, miss_rows_dev, n_miss_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_set_scouts(ccz_engine *e, int32_t n_scouts)
{
    NEED(e);
    if (n_scouts < 0 || n_scouts >= e->d.B) return fail(-1, "ccz_set_scouts: n_scouts must be in 0 .. n_boards - 1 (got %d of %d boards)", n_scouts, e->d.B);
    if (WIDE(e)) return fail(-1, "ccz_set_scouts: not while the width is %d (ccz_set_width): the slots past the searched boards hold the boards' own leaves", e->width);
    if (n_scouts && !e->d.cache) return fail(-1, "ccz_set_scouts: scouts work through the evaluation cache (ccz_config.eval_cache_log2)");
    if (n_scouts && e->budgets_on) return fail(-1, "ccz_set_scouts: not while simulation budgets are on (ccz_set_budgets(NULL) turns them off)");
    if (n_scouts && e->explore_on) return fail(-1, "ccz_set_scouts: not while root exploration is on (ccz_set_root_exploration)");
    if (n_scouts && e->gumbel_on) return fail(-1, "ccz_set_scouts: not while the Gumbel root search is on (ccz_set_gumbel)");
    if (n_scouts && e->history_on) return fail(-1, "ccz_set_scouts: not while leaf history is on (ccz_set_leaf_history)");
    if (n_scouts && e->surprise_on) return fail(-1, "ccz_set_scouts: not while policy surprise weighting is on (ccz_set_surprise)");
    if (n_scouts && e->stop_on) return fail(-1, "ccz_set_scouts: not while the early stop is on (ccz_set_early_stop)");
    if (n_scouts && e->search_on) return fail(-1, "ccz_set_scouts: not while the search parameters are on (ccz_set_search): scouts rest on children being first visited in legal-move order");
    e->active = n_scouts ? e->d.B - n_scouts : 0;
    return 0;
}

int ccz_scout(ccz_engine *e, void *stream, void *leaf_input_f16_dev)
{
    NEED(e);
    NOT_WIDE(e);
    if (e->active <= 0) return fail(-1, "ccz_scout: no scout slots (ccz_set_scouts)");
    if (!leaf_input_f16_dev) return fail(-1, "ccz_scout: null leaf input");
    hipLaunchKernelGGL(k_scout, dim3((unsigned)(e->d.B - e->active)), dim3(64), 0, (hipStream_t)stream, e->d, (uint16_t *)leaf_input_f16_dev, e->active);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_eval_plan_scouted(ccz_engine *e, void *stream, int32_t *miss_rows_dev, int32_t *n_miss_dev, int32_t *state_dev)
{
    NEED(e);
    NOT_WIDE(e);
    if (!e->d.cache) return fail(-1, "ccz_eval_plan_scouted: the engine was created without an evaluation cache (ccz_config.eval_cache_log2)");
    if (e->active <= 0) return fail(-1, "ccz_eval_plan_scouted: no scout slots (ccz_set_scouts)");
    if (!miss_rows_dev || !n_miss_dev) return fail(-1, "ccz_eval_plan_scouted: null output");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cache_probe, dim3(e->d.B), dim3(64), 0, s, e->d);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cache_plan_scouted, dim3(1), dim3(256), 0, s, e->d, e->active, miss_rows_dev, n_miss_dev, state_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_scout_and_plan(ccz_engine *e, void *stream, void *leaf_input_f16_dev, int32_t *miss_rows_dev, int32_t *n_miss_dev, int32_t *state_dev)
{
    NEED(e);
    NOT_WIDE(e);
    if (!e->d.cache || e->active <= 0) return fail(-1, "ccz_scout_and_plan: needs an evaluation cache and scout slots (ccz_set_scouts)");
    if (!leaf_input_f16_dev || !miss_rows_dev || !n_miss_dev) return fail(-1, "ccz_scout_and_plan: null leaf input / output");
    if (e->d.B > kScoutFusedMax) {     // more slots than one workgroup has waves: the three launches
        const int rc = ccz_scout(e, stream, leaf_input_f16_dev);
        return rc ? rc : ccz_eval_plan_scouted(e, stream, miss_rows_dev, n_miss_dev, state_dev);
    }
    hipLaunchKernelGGL(k_scout_probe_plan, dim3(1), dim3((unsigned)(64 * e->d.B)), 0, (hipStream_t)stream, e->d, (uint16_t *)leaf_input_f16_dev, e->active,
                       miss_rows_dev, n_miss_dev, state_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_scouted_run(ccz_engine *e, void *stream, void *leaf_input_f16_dev, int32_t *miss_rows_dev, int32_t *n_miss_dev, int32_t *state_dev, int32_t *run_dev)
{
    NEED(e);
    NOT_WIDE(e);
    if (!e->d.cache || e->active <= 0 || e->active == e->d.B) return fail(-1, "ccz_scouted_run: needs an evaluation cache and scout slots (ccz_set_scouts)");
    if (e->d.B > kScoutFusedMax) return fail(-1, "ccz_scouted_run: at most %d slots (one workgroup, one wave per slot); this engine has %d", kScoutFusedMax, e->d.B);
    if (!leaf_input_f16_dev || !miss_rows_dev || !n_miss_dev || !state_dev || !run_dev) return fail(-1, "ccz_scouted_run: null leaf input / output / run block");
    if (e->d.B <= 12)
        hipLaunchKernelGGL(k_scouted_run<12>, dim3(1), dim3((unsigned)(64 * e->d.B)), 0, (hipStream_t)stream, e->d, (uint16_t *)leaf_input_f16_dev, e->active,
                           miss_rows_dev, n_miss_dev, state_dev, run_dev);
    else
        hipLaunchKernelGGL(k_scouted_run<kScoutFusedMax>, dim3(1), dim3((unsigned)(64 * e->d.B)), 0, (hipStream_t)stream, e->d, (uint16_t *)leaf_input_f16_dev,
                           e->active, miss_rows_dev, n_miss_dev, state_dev, run_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_gather_priors_planned(ccz_engine *e, void *stream, const void *logits_compact_dev, int32_t logits_f16, const float *value_compact_dev)
{
    NEED(e);
    if (!e->d.cache) return fail(-1, "ccz_gather_priors_planned: the engine was created without an evaluation cache");
    if (!logits_compact_dev || !value_compact_dev) return fail(-1, "ccz_gather_priors_planned: null logits / value");
    hipStream_t s = (hipStream_t)stream;
    if (logits_f16)
        hipLaunchKernelGGL((k_softmax_gather<_Float16, true>), dim3(e->d.B), dim3(64), 0, s, e->d, (const _Float16 *)logits_compact_dev, value_compact_dev);
    else
        hipLaunchKernelGGL((k_softmax_gather<float, true>), dim3(e->d.B), dim3(64), 0, s, e->d, (const float *)logits_compact_dev, value_compact_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_set_routing(ccz_engine *e, void *stream, const uint8_t *red_net_host, uint64_t salt0, uint64_t salt1)
{
    NEED(e);
    if (!red_net_host) {
        e->routed = false;
        return 0;
    }
    if (WIDE(e)) return fail(-1, "ccz_set_routing: not while the width is %d (ccz_set_width)", e->width);
    if (!e->d.cache) return fail(-1, "ccz_set_routing: routing works through the evaluation cache (ccz_config.eval_cache_log2)");
    if (SCOUTS(e)) return fail(-1, "ccz_set_routing: not with scout slots (ccz_set_scouts)");
    if (salt0 == salt1) return fail(-1, "ccz_set_routing: the two evaluators need different salts (one would be served the other's evaluations)");
    for (int b = 0; b < e->d.B; ++b)
        if (red_net_host[b] > 1) return fail(-1, "ccz_set_routing: red_net[%d] = %d (must be 0 or 1)", b, (int)red_net_host[b]);
    hipError_t he = hipSuccess;
    if (!e->route_red) {
        he = dalloc(&e->route_red, (size_t)e->d.B, e->owned, e->bytes);
        if (he == hipSuccess) he = dalloc(&e->route_net, (size_t)e->d.B, e->owned, e->bytes);
    }
    HIP_TRY(he);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(e->route_red, red_net_host, (size_t)e->d.B, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s)); // (the host array may go away after the call)
    e->salt[0] = salt0;
    e->salt[1] = salt1;
    e->routed = true;
    return 0;
}

int ccz_eval_plan_routed(ccz_engine *e, void *stream, int32_t *miss_rows_dev, int32_t *n_miss_dev)
{
    NEED(e);
    if (!e->routed) return fail(-1, "ccz_eval_plan_routed: no routing set (ccz_set_routing)");
    if (!e->d.cache) return fail(-1, "ccz_eval_plan_routed: the engine was created without an evaluation cache");
    if (SCOUTS(e)) return fail(-1, "ccz_eval_plan_routed: not with scout slots (ccz_set_scouts)");
    if (!miss_rows_dev || !n_miss_dev) return fail(-1, "ccz_eval_plan_routed: null output");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cache_probe_routed, dim3(e->d.B), dim3(64), 0, s, e->d, (const uint8_t *)e->route_red, e->route_net, e->salt[0], e->salt[1]);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cache_plan_routed, dim3(1), dim3(1024), 0, s, e->d, miss_rows_dev, n_miss_dev, (const uint8_t *)e->route_net,
                       e->salt[0], e->salt[1]);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_gather_priors_routed(ccz_engine *e, void *stream, const void *logits0_dev, const void *logits1_dev, int32_t logits_f16,
                             const float *value0_dev, const float *value1_dev)
{
    NEED(e);
    if (!e->routed) return fail(-1, "ccz_gather_priors_routed: no routing set (ccz_set_routing)");
    if (!e->d.cache) return fail(-1, "ccz_gather_priors_routed: the engine was created without an evaluation cache");
    if (SCOUTS(e)) return fail(-1, "ccz_gather_priors_routed: not with scout slots (ccz_set_scouts)");
    if (!logits0_dev || !logits1_dev || !value0_dev || !value1_dev) return fail(-1, "ccz_gather_priors_routed: null logits / value");
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *net = e->route_net;
    if (logits_f16)
        hipLaunchKernelGGL(k_softmax_gather_routed<_Float16>, dim3(e->d.B), dim3(64), 0, s, e->d, net, (const _Float16 *)logits0_dev,
                           (const _Float16 *)logits1_dev, value0_dev, value1_dev, e->salt[0], e->salt[1]);
    else
        hipLaunchKernelGGL(k_softmax_gather_routed<float>, dim3(e->d.B), dim3(64), 0, s, e->d, net, (const float *)logits0_dev,
                           (const float *)logits1_dev, value0_dev, value1_dev, e->salt[0], e->salt[1]);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_set_budgets(ccz_engine *e, void *stream, const int32_t *budgets_dev, const uint8_t *targets_dev)
{
    NEED(e);
    if (SCOUTS(e)) return fail(-1, "ccz_set_budgets: not with scout slots (ccz_set_scouts)");
    hipLaunchKernelGGL(k_set_budgets, dim3((e->d.B + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->d, e->d.B, budgets_dev, targets_dev);
    HIP_TRY(hipGetLastError());
    e->budgets_on = budgets_dev != nullptr;
    return 0;
}

int ccz_draw_budgets(ccz_engine *e, void *stream, int32_t n_full, int32_t n_fast, double p_full, int32_t *budgets_out_dev)
{
    NEED(e);
    if (SCOUTS(e)) return fail(-1, "ccz_draw_budgets: not with scout slots (ccz_set_scouts)");
    if (n_full < 1 || n_fast < 1) return fail(-1, "ccz_draw_budgets: n_full and n_fast must be >= 1 (got %d, %d)", n_full, n_fast);
    if (!(p_full >= 0.0 && p_full <= 1.0)) return fail(-1, "ccz_draw_budgets: p_full %g must be in [0, 1]", p_full);
    hipLaunchKernelGGL(k_draw_budgets, dim3((e->d.B + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->d, e->d.B, (int)n_full, (int)n_fast, p_full,
                       budgets_out_dev);
    HIP_TRY(hipGetLastError());
    e->budgets_on = true;
    return 0;
}

int ccz_set_resign(ccz_engine *e, void *stream, int32_t enabled, float threshold, int32_t consecutive, int32_t min_ply, double p_playon)
{
    NEED(e);
    if (!(std::isfinite(threshold) && threshold >= -1.0f && threshold <= 0.0f)) return fail(-1, "ccz_set_resign: threshold %g must be finite and in [-1, 0]", (double)threshold);
    if (consecutive < 0 || consecutive > 255) return fail(-1, "ccz_set_resign: consecutive %d must be 0..255", consecutive);
    if (min_ply < 0) return fail(-1, "ccz_set_resign: negative min_ply %d", min_ply);
    if (!(p_playon >= 0.0 && p_playon <= 1.0)) return fail(-1, "ccz_set_resign: p_playon %g must be in [0, 1]", p_playon);
    ResignCfg v;
    v.enabled = enabled ? 1 : 0;
    v.consecutive = consecutive;
    v.min_ply = min_ply;
    v.threshold = threshold;
    v.p_playon = p_playon;
    hipLaunchKernelGGL(k_set_resign, dim3(1), dim3(1), 0, (hipStream_t)stream, const_cast<ResignCfg *>(e->d.rs_cfg), v);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_get_resign_stats(ccz_engine *e, void *stream, ccz_resign_stats *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_resign_stats: null output");
    std::vector<ResignBoardStats> st;
    if (const int rc = fetch_board_stats(e, (hipStream_t)stream, e->d.rs_stats, st)) return rc;
    memset(out, 0, sizeof *out);
    for (const ResignBoardStats &b : st) {
        out->resigned_games += (int64_t)b.resigned;
        out->resigned_by_red += (int64_t)b.resigned_red;
        out->resigned_plies += (int64_t)b.resigned_plies;
        out->playon_games += (int64_t)b.playon;
        out->playon_won += (int64_t)b.playon_won;
        out->playon_drawn += (int64_t)b.playon_drawn;
        out->playon_plies_after += (int64_t)b.playon_after;
    }
    return 0;
}

int ccz_set_surprise(ccz_engine *e, void *stream, int32_t enabled, double alpha, double cap)
{
    NEED(e);
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(-1, "ccz_set_surprise: alpha %g must be in [0, 1]", alpha);
    if (!(cap >= 1.0 && cap <= 15.0)) return fail(-1, "ccz_set_surprise: cap %g must be in [1, 15]", cap);
    if (enabled && SCOUTS(e)) return fail(-1, "ccz_set_surprise: not with scout slots (ccz_set_scouts): the one-game path records no game");
    SurpriseCfg v;
    v.enabled = enabled ? 1 : 0;
    v.pad = 0;
    v.alpha = alpha;
    v.cap = cap;
    const size_t n = (size_t)e->d.B * (size_t)e->d.max_plies;
    hipLaunchKernelGGL(k_set_surprise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e->sp_block, v, n);
    HIP_TRY(hipGetLastError());
    e->surprise_on = enabled != 0;
    return 0;
}

int ccz_get_surprise_stats(ccz_engine *e, void *stream, ccz_surprise_stats *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_surprise_stats: null output");
    std::vector<SurpriseBoardStats> st;
    if (const int rc = fetch_board_stats(e, (hipStream_t)stream, e->sp_host.sp_stats, st)) return rc;
    memset(out, 0, sizeof *out);
    for (const SurpriseBoardStats &b : st) { // in board order: the float64 total is the same on every run
        out->target_plies += (int64_t)b.plies;
        out->surprise_sum = out->surprise_sum + b.sum;
        out->weights_clipped += (int64_t)b.clipped;
    }
    return 0;
}

int ccz_ply_surprise(ccz_engine *e, void *stream, float *kl_host, uint8_t *has_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)e->d.B * (size_t)e->d.max_plies;
    if (kl_host) HIP_TRY(hipMemcpyAsync(kl_host, e->sp_host.rec_kl, n * 4, hipMemcpyDeviceToHost, s));
    if (has_host) HIP_TRY(hipMemcpyAsync(has_host, e->sp_host.rec_hask, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_resign_status(ccz_engine *e, void *stream, uint8_t *state_host, uint8_t *run_host, int32_t *fire_ply_host, float *last_value_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    if (state_host) HIP_TRY(hipMemcpyAsync(state_host, e->d.rs_state, B, hipMemcpyDeviceToHost, s));
    if (run_host) HIP_TRY(hipMemcpyAsync(run_host, e->d.rs_run, B * 2, hipMemcpyDeviceToHost, s));
    if (fire_ply_host) HIP_TRY(hipMemcpyAsync(fire_ply_host, e->d.rs_fire, B * 4, hipMemcpyDeviceToHost, s));
    if (last_value_host) HIP_TRY(hipMemcpyAsync(last_value_host, e->d.rs_last, B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_set_root_exploration(ccz_engine *e, void *stream, int32_t enabled, double eps, double alpha, double forced_k, int32_t prune_targets)
{
    NEED(e);
    if (!(eps >= 0.0 && eps <= 1.0)) return fail(-1, "ccz_set_root_exploration: eps %g must be in [0, 1]", eps);
    if (!(alpha > 0.0 && std::isfinite(alpha))) return fail(-1, "ccz_set_root_exploration: alpha %g must be finite and > 0", alpha);
    if (!(forced_k >= 0.0 && std::isfinite(forced_k))) return fail(-1, "ccz_set_root_exploration: forced_k %g must be finite and >= 0", forced_k);
    if (enabled && WIDE(e)) return fail(-1, "ccz_set_root_exploration: not while the width is %d (ccz_set_width): the wide search has the plain PUCT rule only", e->width);
    if (enabled && SCOUTS(e)) return fail(-1, "ccz_set_root_exploration: not with scout slots (ccz_set_scouts): the one-game path keeps the reference's search");
    if (enabled && e->gumbel_on) return fail(-1, "ccz_set_root_exploration: not while the Gumbel root search is on (ccz_set_gumbel): it has its own root rule");
    ExploreCfg v;
    v.enabled = enabled ? 1 : 0;
    v.prune = prune_targets ? 1 : 0;
    v.eps = eps;
    v.alpha = alpha;
    v.forced_k = forced_k;
    const int n = 2 * e->d.B;
    hipLaunchKernelGGL(k_set_root_exploration, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, const_cast<ExploreCfg *>(e->d.ex_cfg), v, e->d.ex_stamp, n);
    HIP_TRY(hipGetLastError());
    e->explore_on = enabled != 0;
    return 0;
}

int ccz_get_exploration_stats(ccz_engine *e, void *stream, ccz_exploration_stats *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_exploration_stats: null output");
    std::vector<ExploreBoardStats> st;
    if (const int rc = fetch_board_stats(e, (hipStream_t)stream, e->d.ex_stats, st)) return rc;
    memset(out, 0, sizeof *out);
    for (const ExploreBoardStats &b : st) {
        out->explored_moves += (int64_t)b.explored;
        out->forced_selections += (int64_t)b.forced;
        out->visits_pruned += (int64_t)b.visits_pruned;
        out->children_pruned += (int64_t)b.children_pruned;
    }
    return 0;
}

int ccz_set_gumbel(ccz_engine *e, void *stream, int32_t enabled, int32_t n_sims, int32_t max_considered, double c_visit, double c_scale)
{
    NEED(e);
    if (n_sims < 1) return fail(-1, "ccz_set_gumbel: n_sims %d must be >= 1", n_sims);
    if (max_considered < 2 || max_considered > kMaxLegal) return fail(-1, "ccz_set_gumbel: max_considered %d must be in 2..%d", max_considered, kMaxLegal);
    if (!(c_visit >= 0.0 && std::isfinite(c_visit))) return fail(-1, "ccz_set_gumbel: c_visit %g must be finite and >= 0", c_visit);
    if (!(c_scale >= 0.0 && std::isfinite(c_scale))) return fail(-1, "ccz_set_gumbel: c_scale %g must be finite and >= 0", c_scale);
    if (enabled && WIDE(e)) return fail(-1, "ccz_set_gumbel: not while the width is %d (ccz_set_width): the wide search has the plain PUCT rule only", e->width);
    if (enabled && SCOUTS(e)) return fail(-1, "ccz_set_gumbel: not with scout slots (ccz_set_scouts): the one-game path keeps the reference's search");
    if (enabled && e->explore_on) return fail(-1, "ccz_set_gumbel: not while root exploration is on (ccz_set_root_exploration)");
    if (enabled && e->stop_on) return fail(-1, "ccz_set_gumbel: not while the early stop is on (ccz_set_early_stop): sequential halving plans the whole budget");
    GumbelCfg v;
    v.enabled = enabled ? 1 : 0;
    v.n_sims = n_sims;
    v.max_considered = max_considered;
    v.pad = 0;
    v.c_visit = c_visit;
    v.c_scale = c_scale;
    const int n = 4 * e->d.B;
    hipLaunchKernelGGL(k_set_gumbel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, const_cast<GumbelCfg *>(e->d.gm_cfg), v, e->d.gm_stamp, n);
    HIP_TRY(hipGetLastError());
    e->gumbel_on = enabled != 0;
    return 0;
}

int ccz_get_gumbel_stats(ccz_engine *e, void *stream, ccz_gumbel_stats *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_gumbel_stats: null output");
    std::vector<GumbelBoardStats> st;
    if (const int rc = fetch_board_stats(e, (hipStream_t)stream, e->d.gm_stats, st)) return rc;
    memset(out, 0, sizeof *out);
    for (const GumbelBoardStats &b : st) {
        out->gumbel_moves += (int64_t)b.moves;
        out->considered_sum += (int64_t)b.considered;
        out->offvisit_moves += (int64_t)b.offvisit;
    }
    return 0;
}

static int fetch_meta(ccz_engine *e, hipStream_t s);

int ccz_gumbel_root(ccz_engine *e, void *stream, double *g_host, double *logit_host, int32_t *n0_host, int32_t *k_host, int32_t *n_eff_host)
{
    NEED(e);
    if (!k_host) return fail(-1, "ccz_gumbel_root: null k output");
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    std::vector<uint32_t> stamp(B * 4);
    if (g_host) HIP_TRY(hipMemcpyAsync(g_host, e->d.gm_g, B * kMaxLegal * 8, hipMemcpyDeviceToHost, s));
    if (logit_host) HIP_TRY(hipMemcpyAsync(logit_host, e->d.gm_logit, B * kMaxLegal * 8, hipMemcpyDeviceToHost, s));
    if (n0_host) HIP_TRY(hipMemcpyAsync(n0_host, e->d.gm_n0, B * kMaxLegal * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(stamp.data(), e->d.gm_stamp, B * 16, hipMemcpyDeviceToHost, s));
    const int rc = fetch_meta(e, s); // syncs
    if (rc) return rc;
    for (size_t b = 0; b < B; ++b) { // a row filled for an earlier move (or never) is no row of this one: k = 0, zeros
        const bool live = stamp[4 * b] == e->h_meta[b].move_counter + 1u && stamp[4 * b + 1] <= (uint32_t)kMaxLegal;
        const int k = live ? (int)stamp[4 * b + 1] : 0;
        k_host[b] = k;
        if (n_eff_host) n_eff_host[b] = live ? (int32_t)stamp[4 * b + 2] : 0;
        for (int i = k; i < kMaxLegal; ++i) {
            if (g_host) g_host[b * kMaxLegal + i] = 0.0;
            if (logit_host) logit_host[b * kMaxLegal + i] = 0.0;
            if (n0_host) n0_host[b * kMaxLegal + i] = 0;
        }
    }
    return 0;
}

int ccz_gumbel_sequence(void *stream, int32_t m, int32_t n, int32_t *seq_dev)
{
    if (m < 0 || n < 0 || !seq_dev) return fail(-1, "ccz_gumbel_sequence: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_gumbel_sequence, dim3(1), dim3(64), 0, (hipStream_t)stream, (int)m, (int)n, seq_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// one urgency pair of ccz_set_search: nullptr, or what is wrong with it
static const char *bad_fpu(int32_t mode, double value)
{
    if (mode < 0 || mode > 2) return "must be 0 (off), 1 (reduction) or 2 (absolute)";
    if (mode == 1 && !(value >= 0.0 && std::isfinite(value))) return "is a reduction: its value must be finite and >= 0";
    if (mode == 2 && !(value >= -1.0 && value <= 1.0)) return "is absolute: its value must be in [-1, 1]";
    return nullptr;
}

int ccz_set_search(ccz_engine *e, void *stream, int32_t enabled, int32_t fpu_mode, double fpu_value, int32_t fpu_root_mode,
                   double fpu_root_value, double c_base, double c_factor)
{
    NEED(e);
    SearchCfg v = search_defaults(); // enabled = 0: the other arguments are ignored
    if (enabled) {
        if (const char *why = bad_fpu(fpu_mode, fpu_value)) return fail(-1, "ccz_set_search: fpu_mode %d / fpu_value %g: the mode %s", fpu_mode, fpu_value, why);
        if (const char *why = bad_fpu(fpu_root_mode, fpu_root_value))
            return fail(-1, "ccz_set_search: fpu_root_mode %d / fpu_root_value %g: the mode %s", fpu_root_mode, fpu_root_value, why);
        if (!(c_base > 0.0 && std::isfinite(c_base))) return fail(-1, "ccz_set_search: c_base %g must be finite and > 0", c_base);
        if (!(c_factor >= 0.0 && std::isfinite(c_factor))) return fail(-1, "ccz_set_search: c_factor %g must be finite and >= 0", c_factor);
        if (WIDE(e)) return fail(-1, "ccz_set_search: not while the width is %d (ccz_set_width): the wide search has the plain PUCT rule only", e->width);
        if (SCOUTS(e)) return fail(-1, "ccz_set_search: not with scout slots (ccz_set_scouts): the one-game path keeps the reference's search");
        v.enabled = 1;
        v.fpu_mode = fpu_mode;
        v.fpu_root_mode = fpu_root_mode;
        v.fpu_value = fpu_mode ? fpu_value : 0.0; // (a mode that is off has no value)
        v.fpu_root_value = fpu_root_mode ? fpu_root_value : 0.0;
        v.c_base = c_base;
        v.c_factor = c_factor;
    }
    hipLaunchKernelGGL(k_set_search, dim3(1), dim3(1), 0, (hipStream_t)stream, const_cast<SearchCfg *>(e->d.sr_cfg), v);
    HIP_TRY(hipGetLastError());
    e->search_on = enabled != 0;
    return 0;
}

int ccz_get_search(ccz_engine *e, void *stream, ccz_search_cfg *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_search: null output");
    hipStream_t s = (hipStream_t)stream;
    SearchCfg v;
    HIP_TRY(hipMemcpyAsync(&v, e->d.sr_cfg, sizeof v, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->enabled = v.enabled;
    out->fpu_mode = v.fpu_mode;
    out->fpu_root_mode = v.fpu_root_mode;
    out->reserved = 0;
    out->fpu_value = v.fpu_value;
    out->fpu_root_value = v.fpu_root_value;
    out->c_base = v.c_base;
    out->c_factor = v.c_factor;
    return 0;
}

// ---- early stop per board (cczero.h: "Early stop per board")
int ccz_set_early_stop(ccz_engine *e, void *stream, const ccz_early_stop_cfg *cfg)
{
    NEED(e);
    if (!cfg) return fail(-1, "ccz_set_early_stop: null settings");
    StopCfg v;
    memset(&v, 0, sizeof v); // enabled = 0: the other fields are ignored
    if (cfg->enabled != 0 && cfg->enabled != 1) return fail(-1, "ccz_set_early_stop: enabled %d must be 0 or 1", cfg->enabled);
    if (cfg->enabled) {
        if (cfg->single_reply != 0 && cfg->single_reply != 1) return fail(-1, "ccz_set_early_stop: single_reply %d must be 0 or 1", cfg->single_reply);
        if (cfg->kld_interval < 0) return fail(-1, "ccz_set_early_stop: kld_interval %d must be 0 (off) or >= 1", cfg->kld_interval);
        if (cfg->min_sims < 0) return fail(-1, "ccz_set_early_stop: negative min_sims %d", cfg->min_sims);
        if (cfg->n_sims < 1) return fail(-1, "ccz_set_early_stop: n_sims %d must be >= 1", cfg->n_sims);
        if (cfg->reserved != 0) return fail(-1, "ccz_set_early_stop: reserved %d must be 0", cfg->reserved);
        if (!(cfg->gap_factor == 0.0 || (cfg->gap_factor >= 1.0 && std::isfinite(cfg->gap_factor))))
            return fail(-1, "ccz_set_early_stop: gap_factor %g must be 0 (off) or finite and >= 1", cfg->gap_factor);
        if (!(cfg->min_gain >= 0.0 && std::isfinite(cfg->min_gain))) return fail(-1, "ccz_set_early_stop: min_gain %g must be finite and >= 0", cfg->min_gain);
        if (SCOUTS(e)) return fail(-1, "ccz_set_early_stop: not with scout slots (ccz_set_scouts): the one-game path keeps the reference's search");
        if (WIDE(e)) return fail(-1, "ccz_set_early_stop: not while the width is %d (ccz_set_width): the wide search has its own budget test", e->width);
        if (e->gumbel_on) return fail(-1, "ccz_set_early_stop: not while the Gumbel root search is on (ccz_set_gumbel): sequential halving plans the whole budget");
        v.enabled = 1;
        v.single_reply = cfg->single_reply;
        v.kld_interval = cfg->kld_interval;
        v.min_sims = cfg->min_sims;
        v.n_sims = cfg->n_sims;
        v.gap_factor = cfg->gap_factor;
        v.min_gain = cfg->min_gain;
    }
    const int n = e->d.B;
    hipLaunchKernelGGL(k_set_early_stop, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, const_cast<StopCfg *>(e->d.es_cfg), v, e->d.es_stopped,
                       e->d.es_snap_s, n);
    HIP_TRY(hipGetLastError());
    e->stop_on = v.enabled != 0;
    return 0;
}

int ccz_get_early_stop(ccz_engine *e, void *stream, ccz_early_stop_cfg *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_early_stop: null output");
    hipStream_t s = (hipStream_t)stream;
    StopCfg v;
    HIP_TRY(hipMemcpyAsync(&v, e->d.es_cfg, sizeof v, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->enabled = v.enabled;
    out->single_reply = v.single_reply;
    out->kld_interval = v.kld_interval;
    out->min_sims = v.min_sims;
    out->n_sims = v.n_sims;
    out->reserved = 0;
    out->gap_factor = v.gap_factor;
    out->min_gain = v.min_gain;
    return 0;
}

int ccz_get_early_stop_stats(ccz_engine *e, void *stream, ccz_early_stop_stats *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_early_stop_stats: null output");
    std::vector<StopBoardStats> st;
    if (const int rc = fetch_board_stats(e, (hipStream_t)stream, e->d.es_stats, st)) return rc;
    memset(out, 0, sizeof *out);
    for (const StopBoardStats &b : st) {
        for (int r = 0; r < 4; ++r) out->stops[r] += (int64_t)b.stops[r];
        out->sims_saved += (int64_t)b.sims_saved;
        out->evaluations += (int64_t)b.evaluations;
    }
    return 0;
}

int ccz_early_stop_status(ccz_engine *e, void *stream, uint8_t *reason_host, int32_t *sims_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    if (reason_host) HIP_TRY(hipMemcpyAsync(reason_host, e->d.es_stopped, B, hipMemcpyDeviceToHost, s));
    if (sims_host) HIP_TRY(hipMemcpyAsync(sims_host, e->d.move_sims, B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_searching(ccz_engine *e, void *stream, int32_t *count_host)
{
    NEED(e);
    if (!count_host) return fail(-1, "ccz_searching: null output");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_searching, dim3(1), dim3(1024), 0, s, e->d, (int)ACTIVE(e), e->st_count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(count_host, e->st_count, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_set_solver(ccz_engine *e, void *stream, int32_t enabled)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    if (enabled && WIDE(e)) return fail(-1, "ccz_set_solver: not while the width is %d (ccz_set_width): the wide search has the plain PUCT rule only", e->width);
    const size_t n = (size_t)e->d.B * 2 * (size_t)e->d.cap;
    if (enabled && !e->proof) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(dalloc(&e->proof, n, e->owned, e->bytes)); // (zeroed; may sync)
    } else if (enabled && !e->solver_on) {
        HIP_TRY(hipMemsetAsync(e->proof, 0, n, s)); // nothing kept the bytes up to date while it was off
    }
    SolverCfg v;
    v.enabled = enabled ? 1 : 0;
    v.spread = e->spread_on ? 1 : 0;
    v.proof = e->proof;
    hipLaunchKernelGGL(k_set_solver, dim3(1), dim3(1), 0, s, const_cast<SolverCfg *>(e->d.sv_cfg), v);
    HIP_TRY(hipGetLastError());
    e->solver_on = enabled != 0;
    return 0;
}

// ---- value spread and the LCB move (cczero.h: "Value spread and the LCB move")
int ccz_set_value_stats(ccz_engine *e, void *stream, int32_t enabled)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    if (enabled && WIDE(e)) return fail(-1, "ccz_set_value_stats: not while the width is %d (ccz_set_width): a virtual loss is no value", e->width);
    if (enabled && (e->d.flags & CCZ_FLAG_VALUE_F16)) return fail(-1, "ccz_set_value_stats: not on a CCZ_FLAG_VALUE_F16 engine: the float16 running mean has no stated S");
    const size_t n = (size_t)e->d.B * 2 * (size_t)e->d.cap;
    if (enabled && !e->spread_S) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(dalloc(&e->spread_S, n, e->owned, e->bytes)); // (zeroed; may sync)
    } else if (enabled && !e->spread_on) {
        HIP_TRY(hipMemsetAsync(e->spread_S, 0, n * sizeof(float), s)); // nothing kept the sums up to date while it was off
    }
    SolverBlock *blk = reinterpret_cast<SolverBlock *>(const_cast<SolverCfg *>(e->d.sv_cfg));
    hipLaunchKernelGGL(k_set_value_stats, dim3(1), dim3(1), 0, s, blk, enabled ? 1 : 0, e->spread_S);
    HIP_TRY(hipGetLastError());
    e->spread_on = enabled != 0;
    return 0;
}

int ccz_get_value_stats(ccz_engine *e, int32_t *enabled_out)
{
    NEED(e);
    if (!enabled_out) return fail(-1, "ccz_get_value_stats: null output");
    *enabled_out = e->spread_on ? 1 : 0;
    return 0;
}

int ccz_root_value_stats(ccz_engine *e, void *stream, float *s_host, float *root_s_host)
{
    NEED(e);
    if (!e->spread_on) return fail(-1, "ccz_root_value_stats: the value spread is off (ccz_set_value_stats)");
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    if (!e->st_spread) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(dalloc(&e->st_spread, B * (kMaxLegal + 1), e->owned, e->bytes));
    }
    float *p = e->st_spread;
    hipLaunchKernelGGL(k_root_value_stats, dim3(e->d.B), dim3(64), 0, s, e->d, (int)ACTIVE(e), p, p + B * kMaxLegal);
    HIP_TRY(hipGetLastError());
    if (s_host) HIP_TRY(hipMemcpyAsync(s_host, p, B * kMaxLegal * sizeof(float), hipMemcpyDeviceToHost, s));
    if (root_s_host) HIP_TRY(hipMemcpyAsync(root_s_host, p + B * kMaxLegal, B * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_lcb_moves(ccz_engine *e, void *stream, double z, double min_visit_ratio, int32_t min_visits, int32_t *moves_out_dev,
                  int32_t *child_out_dev, double *lcb_out_dev)
{
    NEED(e);
    if (!e->spread_on) return fail(-1, "ccz_lcb_moves: the value spread is off (ccz_set_value_stats)");
    if (!moves_out_dev) return fail(-1, "ccz_lcb_moves: null moves_out");
    if (!(z >= 0.0) || z > 1.7976931348623157e308) return fail(-1, "ccz_lcb_moves: z %g must be finite and >= 0", z);
    if (!(min_visit_ratio >= 0.0 && min_visit_ratio <= 1.0)) return fail(-1, "ccz_lcb_moves: min_visit_ratio %g must be in [0, 1]", min_visit_ratio);
    if (min_visits < 0) return fail(-1, "ccz_lcb_moves: min_visits %d must be >= 0", min_visits);
    hipLaunchKernelGGL(k_lcb_moves, dim3(e->d.B), dim3(64), 0, (hipStream_t)stream, e->d, (int)ACTIVE(e), z, min_visit_ratio, (int)min_visits,
                       moves_out_dev, child_out_dev, lcb_out_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_mate_search(ccz_engine *e, void *stream, int32_t max_plies, int32_t node_budget, int32_t *state_dev, int32_t *dist_dev,
                    int32_t *move_dev, int32_t *nodes_dev)
{
    NEED(e);
    if (!state_dev || !dist_dev || !move_dev || !nodes_dev) return fail(-1, "ccz_mate_search: null output");
    if (max_plies < 1 || max_plies > CCZ_MATE_MAX_PLIES || !(max_plies & 1))
        return fail(-1, "ccz_mate_search: max_plies %d must be odd and in 1..%d", max_plies, CCZ_MATE_MAX_PLIES);
    if (node_budget < 1 || node_budget > CCZ_MATE_MAX_NODES)
        return fail(-1, "ccz_mate_search: node_budget %d must be in 1..%d", node_budget, CCZ_MATE_MAX_NODES);
    hipLaunchKernelGGL(k_mate_search, dim3(e->d.B), dim3(64), 0, (hipStream_t)stream, e->d, (int)ACTIVE(e), (int)max_plies, (int)node_budget,
                       state_dev, dist_dev, move_dev, nodes_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// k_root_proof into the staging block (allocated at the first call); the caller copies what it wants and syncs
static int stage_root_proof(ccz_engine *e, hipStream_t s)
{
    const size_t B = (size_t)e->d.B;
    if (!e->st_proof) HIP_TRY(dalloc(&e->st_proof, B * (2 + 2 * kMaxLegal), e->owned, e->bytes));
    uint8_t *p = e->st_proof;
    hipLaunchKernelGGL(k_root_proof, dim3(e->d.B), dim3(64), 0, s, e->d, p, p + B, p + 2 * B, p + 2 * B + B * kMaxLegal);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_root_proof(ccz_engine *e, void *stream, uint8_t *state_host, uint8_t *dist_host, uint8_t *child_state_host, uint8_t *child_dist_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    if (const int rc = stage_root_proof(e, s)) return rc;
    const uint8_t *p = e->st_proof;
    if (state_host) HIP_TRY(hipMemcpyAsync(state_host, p, B, hipMemcpyDeviceToHost, s));
    if (dist_host) HIP_TRY(hipMemcpyAsync(dist_host, p + B, B, hipMemcpyDeviceToHost, s));
    if (child_state_host) HIP_TRY(hipMemcpyAsync(child_state_host, p + 2 * B, B * kMaxLegal, hipMemcpyDeviceToHost, s));
    if (child_dist_host) HIP_TRY(hipMemcpyAsync(child_dist_host, p + 2 * B + B * kMaxLegal, B * kMaxLegal, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

static int fetch_meta(ccz_engine *e, hipStream_t s);

int ccz_get_solver_stats(ccz_engine *e, void *stream, ccz_solver_stats *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_solver_stats: null output");
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = stage_root_proof(e, s)) return rc;
    std::vector<uint8_t> root((size_t)e->d.B);
    HIP_TRY(hipMemcpyAsync(root.data(), e->st_proof, root.size(), hipMemcpyDeviceToHost, s));
    std::vector<SolverBoardStats> st;
    if (const int rc = fetch_board_stats(e, s, e->d.sv_stats, st)) return rc; // syncs
    memset(out, 0, sizeof *out);
    for (const SolverBoardStats &b : st) {
        out->nodes_proven += (int64_t)b.proven;
        out->proven_stops += (int64_t)b.stops;
    }
    // a finished board is searched no more, and k_finish_move leaves it behind when the pool halves flip: what lies at its tree top is
    // an older move's tree, not a root
    if (const int rc = fetch_meta(e, s)) return rc;
    for (unsigned b = 0; b < ACTIVE(e); ++b) out->roots_proven += (root[b] && !e->h_meta[b].over) ? 1 : 0;
    return 0;
}

int ccz_proof_combine(void *stream, const uint8_t *bytes_dev, const int32_t *counts_dev, int32_t n_cases, uint8_t *out_dev)
{
    if (n_cases < 0 || !bytes_dev || !counts_dev || !out_dev) return fail(-1, "ccz_proof_combine: bad arguments");
    if (n_cases == 0) return 0;
    hipLaunchKernelGGL(k_proof_combine, dim3((unsigned)n_cases), dim3(64), 0, (hipStream_t)stream, bytes_dev, counts_dev, (int)n_cases, out_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int fetch_meta(ccz_engine *e, hipStream_t s);

int ccz_root_noise(ccz_engine *e, void *stream, float *noise_host, int32_t *k_host)
{
    NEED(e);
    if (!noise_host || !k_host) return fail(-1, "ccz_root_noise: null output");
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    std::vector<uint32_t> stamp(B * 2);
    HIP_TRY(hipMemcpyAsync(noise_host, e->d.ex_dir, B * kMaxLegal * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(stamp.data(), e->d.ex_stamp, B * 8, hipMemcpyDeviceToHost, s));
    const int rc = fetch_meta(e, s); // syncs
    if (rc) return rc;
    for (size_t b = 0; b < B; ++b) { // a row filled for an earlier move (or never) is no noise of this one: k = 0, zeros
        const bool live = stamp[2 * b] == e->h_meta[b].move_counter + 1u && stamp[2 * b + 1] <= (uint32_t)kMaxLegal;
        const int k = live ? (int)stamp[2 * b + 1] : 0;
        k_host[b] = k;
        for (int i = k; i < kMaxLegal; ++i) noise_host[b * kMaxLegal + i] = 0.0f;
    }
    return 0;
}

int ccz_eval_cache_clear(ccz_engine *e, void *stream)
{
    NEED(e);
    if (!e->d.cache) return 0;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(e->d.cache, 0, ((size_t)e->d.cache_mask + 1) * sizeof(CacheEntry), s));
    HIP_TRY(hipMemsetAsync(e->d.claim, 0x7f, ((size_t)e->d.cache_mask + 1) * 4, s));
    return 0;
}

int ccz_step_compact(ccz_engine *e, void *stream, const float *value_dev, void *leaf_input_f16_dev)
{
    NEED(e);
    NOT_WIDE(e);
    if (!value_dev && !e->d.cache) return fail(-1, "ccz_step_compact: null value (engine-owned leaf values exist only with an evaluation cache)");
    hipLaunchKernelGGL(k_step<true>, dim3(ACTIVE(e)), dim3(64), 0, (hipStream_t)stream, e->d, (const float *)e->d.prior128, value_dev,
                       (uint16_t *)leaf_input_f16_dev);
    HIP_TRY(hipGetLastError());
    return leaf_history(e, (hipStream_t)stream, leaf_input_f16_dev);
}

int ccz_expand_backup_compact(ccz_engine *e, void *stream, const float *value_dev)
{
    NEED(e);
    NOT_WIDE(e);
    if (!value_dev && !e->d.cache) return fail(-1, "ccz_expand_backup_compact: null value (engine-owned leaf values exist only with an evaluation cache)");
    hipLaunchKernelGGL(k_expand_backup<true>, dim3(ACTIVE(e)), dim3(64), 0, (hipStream_t)stream, e->d, (const float *)e->d.prior128,
                       value_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- wide search (cczero.h: "Wide search")
int ccz_set_width(ccz_engine *e, void *stream, int32_t width)
{
    NEED(e);
    if (width < 1 || width > 64) return fail(-1, "ccz_set_width: width %d must be in 1 .. 64", width);
    if (e->d.B % width) return fail(-1, "ccz_set_width: width %d does not divide n_boards %d", width, e->d.B);
    if (width > 1) {
        if (SCOUTS(e)) return fail(-1, "ccz_set_width: not with scout slots (ccz_set_scouts)");
        if (e->explore_on) return fail(-1, "ccz_set_width: not while root exploration is on (ccz_set_root_exploration)");
        if (e->gumbel_on) return fail(-1, "ccz_set_width: not while the Gumbel root search is on (ccz_set_gumbel)");
        if (e->solver_on) return fail(-1, "ccz_set_width: not while the solver is on (ccz_set_solver)");
        if (e->search_on) return fail(-1, "ccz_set_width: not while the search parameters are on (ccz_set_search)");
        if (e->stop_on) return fail(-1, "ccz_set_width: not while the early stop is on (ccz_set_early_stop)");
        if (e->routed) return fail(-1, "ccz_set_width: not while routing is on (ccz_set_routing)");
        if (e->history_on) return fail(-1, "ccz_set_width: not while leaf history is on (ccz_set_leaf_history)");
        if (e->spread_on) return fail(-1, "ccz_set_width: not while the value spread is on (ccz_set_value_stats): a virtual loss is no value");
    }
    hipStream_t s = (hipStream_t)stream;
    if (width == 1) {
        if (WIDE(e)) {
            if (const int rc = wide_drop(e, s, nullptr, -1)) return rc; // (the contract says none is pending: this keeps F zero anyway)
            e->active = 0;
        }
        e->width = 1;
        return 0;
    }
    const size_t n = (size_t)e->d.B * 2 * (size_t)e->d.cap;
    if (!e->wide_F) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(dalloc(&e->wide_F, n, e->owned, e->bytes)); // (zeroed; may sync)
        HIP_TRY(dalloc(&e->wide_stats, (size_t)e->d.B, e->owned, e->bytes));
        HIP_TRY(dalloc(&e->st_wide, 1, e->owned, e->bytes));
    } else {
        HIP_TRY(hipMemsetAsync(e->wide_F, 0, n, s)); // no leaf is pending: all counts are zero
    }
    e->width = width;
    e->active = e->d.B / width;
    // every slot, not only those past the searched boards: a leaf left pending by the sequential calls (the contract says there is
    // none) was never counted in F and must not be taken out of it at the next move boundary
    hipLaunchKernelGGL(k_wide_clear_slots, dim3((unsigned)((e->d.B + 255) / 256)), dim3(256), 0, s, e->d, 0);
    HIP_TRY(hipGetLastError());
    return 0;
}

// waves of a board's workgroup: one per slot up to 16 (CCZ_WIDE_TAIL_WAVES: an A/B knob of the measurements, 1 = one wave does everything)
static int wide_waves(int width)
{
    static const int forced = [] { const char *v = getenv("CCZ_WIDE_TAIL_WAVES"); return v ? atoi(v) : 0; }();
    const int want = forced > 0 ? forced : width;
    return want <= 1 ? 1 : want <= 2 ? 2 : want <= 4 ? 4 : want <= 8 ? 8 : 16;
}

static int wide_launch(ccz_engine *e, hipStream_t s, const float *value_dev, void *leaf_in, int32_t *n_leaves_dev, int backup)
{
    const dim3 grid((unsigned)e->active);
    const WideArgs wa = wide_args(e);
    uint16_t *li = (uint16_t *)leaf_in;
    switch (wide_waves(e->width)) {
    case 1: hipLaunchKernelGGL(k_wide<1>, grid, dim3(64), 0, s, e->d, wa, value_dev, li, n_leaves_dev, backup); break;
    case 2: hipLaunchKernelGGL(k_wide<2>, grid, dim3(128), 0, s, e->d, wa, value_dev, li, n_leaves_dev, backup); break;
    case 4: hipLaunchKernelGGL(k_wide<4>, grid, dim3(256), 0, s, e->d, wa, value_dev, li, n_leaves_dev, backup); break;
    case 8: hipLaunchKernelGGL(k_wide<8>, grid, dim3(512), 0, s, e->d, wa, value_dev, li, n_leaves_dev, backup); break;
    default: hipLaunchKernelGGL(k_wide<16>, grid, dim3(1024), 0, s, e->d, wa, value_dev, li, n_leaves_dev, backup); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_select_wide(ccz_engine *e, void *stream, void *leaf_input_f16_dev, int32_t *n_leaves_dev)
{
    NEED(e);
    if (!WIDE(e)) return fail(-1, "ccz_select_wide: the width is 1 (ccz_set_width): the sequential search selects with ccz_select_leaves");
    if (!n_leaves_dev) return fail(-1, "ccz_select_wide: null n_leaves");
    return wide_launch(e, (hipStream_t)stream, nullptr, leaf_input_f16_dev, n_leaves_dev, 0);
}

int ccz_step_wide(ccz_engine *e, void *stream, const float *value_dev, void *leaf_input_f16_dev, int32_t *n_leaves_dev)
{
    NEED(e);
    if (!WIDE(e)) return fail(-1, "ccz_step_wide: the width is 1 (ccz_set_width): the sequential search steps with ccz_step_compact");
    if (!n_leaves_dev) return fail(-1, "ccz_step_wide: null n_leaves");
    if (!value_dev && !e->d.cache) return fail(-1, "ccz_step_wide: null value (engine-owned leaf values exist only with an evaluation cache)");
    return wide_launch(e, (hipStream_t)stream, value_dev, leaf_input_f16_dev, n_leaves_dev, 1);
}

int ccz_get_wide_stats(ccz_engine *e, void *stream, ccz_wide_stats *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_wide_stats: null output");
    memset(out, 0, sizeof *out);
    if (!e->wide_F) return 0;
    hipStream_t s = (hipStream_t)stream;
    std::vector<WideBoardStats> st;
    if (const int rc = fetch_board_stats(e, s, e->wide_stats, st)) return rc;
    for (const WideBoardStats &b : st) {
        out->steps += (int64_t)b.steps;
        out->leaves += (int64_t)b.leaves;
        out->collisions += (int64_t)b.collisions;
    }
    unsigned long long sum = 0;
    HIP_TRY(hipMemsetAsync(e->st_wide, 0, sizeof sum, s));
    hipLaunchKernelGGL(k_wide_inflight, dim3(ACTIVE(e)), dim3(256), 0, s, e->d, wide_args(e), e->st_wide);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&sum, e->st_wide, sizeof sum, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->inflight_now = (int64_t)sum;
    return 0;
}

int ccz_finish_move(ccz_engine *e, void *stream, const int32_t *forced_moves_dev, const double *temps_dev,
                    int32_t *moves_out_dev, int32_t keep_tree)
{
    NEED(e);
    if (const int rc = wide_drop(e, (hipStream_t)stream, nullptr, -1)) return rc;
    hipLaunchKernelGGL(k_finish_move, dim3(ACTIVE(e)), dim3(64), 0, (hipStream_t)stream, e->d, forced_moves_dev, temps_dev,
                       moves_out_dev, keep_tree ? 1 : 0);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_flip_half, dim3(1), dim3(1), 0, (hipStream_t)stream, e->d);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_root_children(ccz_engine *e, void *stream, int32_t *k_host, uint16_t *acts_host, int32_t *visits_host,
                      float *q_host, float *prior_host, int32_t *root_visits_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    hipLaunchKernelGGL(k_root_children, dim3(e->d.B), dim3(64), 0, s, e->d, e->st_k, e->st_acts, e->st_visits, e->st_q, e->st_p,
                       e->st_rootn, (const double *)nullptr, (double *)nullptr);
    HIP_TRY(hipGetLastError());
    if (k_host) HIP_TRY(hipMemcpyAsync(k_host, e->st_k, B * 4, hipMemcpyDeviceToHost, s));
    if (acts_host) HIP_TRY(hipMemcpyAsync(acts_host, e->st_acts, B * kMaxLegal * 2, hipMemcpyDeviceToHost, s));
    if (visits_host) HIP_TRY(hipMemcpyAsync(visits_host, e->st_visits, B * kMaxLegal * 4, hipMemcpyDeviceToHost, s));
    if (q_host) HIP_TRY(hipMemcpyAsync(q_host, e->st_q, B * kMaxLegal * 4, hipMemcpyDeviceToHost, s));
    if (prior_host) HIP_TRY(hipMemcpyAsync(prior_host, e->st_p, B * kMaxLegal * 4, hipMemcpyDeviceToHost, s));
    if (root_visits_host) HIP_TRY(hipMemcpyAsync(root_visits_host, e->st_rootn, B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_principal_variations(ccz_engine *e, void *stream, int32_t multipv, int32_t max_len, uint16_t *moves_dev, int32_t *len_dev,
                             int32_t *visits_dev, float *q_dev, float *prior_dev, int32_t *root_visits_dev)
{
    NEED(e);
    if (multipv < 1 || multipv > kMaxLegal) return fail(-1, "ccz_principal_variations: multipv must be 1..%d (got %d)", kMaxLegal, multipv);
    if (max_len < 1) return fail(-1, "ccz_principal_variations: max_len must be >= 1 (got %d)", max_len);
    if (!moves_dev || !len_dev || !visits_dev || !q_dev || !prior_dev || !root_visits_dev) return fail(-1, "ccz_principal_variations: null output");
    hipLaunchKernelGGL(k_principal_variations, dim3(e->d.B, (unsigned)multipv), dim3(64), 0, (hipStream_t)stream, e->d, (int)ACTIVE(e), (int)multipv,
                       (int)max_len, moves_dev, len_dev, visits_dev, q_dev, prior_dev, root_visits_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// per-board temperatures of the caller `fn`, checked and copied to st_temps: *temps is the device pointer, null without temperatures
static int stage_temps(ccz_engine *e, hipStream_t s, const double *temps_host, const char *fn, const double **temps)
{
    for (int b = 0; temps_host && b < e->d.B; ++b)
        if (!(temps_host[b] > 0.0)) return fail(-1, "%s: temps[%d] = %g must be > 0", fn, b, temps_host[b]);
    if (temps_host) HIP_TRY(hipMemcpyAsync(e->st_temps, temps_host, (size_t)e->d.B * 8, hipMemcpyHostToDevice, s));
    *temps = temps_host ? e->st_temps : nullptr;
    return 0;
}

int ccz_move_distribution(ccz_engine *e, void *stream, const double *temps_host, double *gamma_host, double *mixed_host,
                          double *u_host)
{
    NEED(e);
    if (!gamma_host || !mixed_host || !u_host) return fail(-1, "ccz_move_distribution: null output");
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    const double *temps;
    if (const int rc = stage_temps(e, s, temps_host, "ccz_move_distribution", &temps)) return rc;
    if (!e->st_g) {
        HIP_TRY(hipMalloc(&e->st_g, B * kMaxLegal * 8));
        e->owned.push_back(e->st_g);
        HIP_TRY(hipMalloc(&e->st_u, B * 8));
        e->owned.push_back(e->st_u);
    }
    // boards past ACTIVE (scout slots) are not sampled by ccz_finish_move either: zero rows, u = NaN
    HIP_TRY(hipMemsetAsync(e->st_g, 0, B * kMaxLegal * 8, s));
    HIP_TRY(hipMemsetAsync(e->st_pi, 0, B * kMaxLegal * 8, s));
    HIP_TRY(hipMemsetAsync(e->st_u, 0xff, B * 8, s));
    hipLaunchKernelGGL(k_move_distribution, dim3(ACTIVE(e)), dim3(64), 0, s, e->d, temps, e->st_g, e->st_pi, e->st_u);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(gamma_host, e->st_g, B * kMaxLegal * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(mixed_host, e->st_pi, B * kMaxLegal * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(u_host, e->st_u, B * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_root_pi(ccz_engine *e, void *stream, const double *temps_host, double *pi_host)
{
    NEED(e);
    if (!pi_host) return fail(-1, "ccz_root_pi: null output");
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    const double *temps;
    if (const int rc = stage_temps(e, s, temps_host, "ccz_root_pi", &temps)) return rc;
    hipLaunchKernelGGL(k_root_children, dim3(e->d.B), dim3(64), 0, s, e->d, (int32_t *)nullptr, (uint16_t *)nullptr,
                       (int32_t *)nullptr, (float *)nullptr, (float *)nullptr, (int32_t *)nullptr, temps, e->st_pi);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(pi_host, e->st_pi, B * kMaxLegal * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

static int fetch_meta(ccz_engine *e, hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(e->h_meta.data(), e->d.meta, (size_t)e->d.B * sizeof(BoardMeta), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_game_status(ccz_engine *e, void *stream, uint8_t *over_host, int8_t *winner_host, int32_t *plies_host, uint8_t *turn_host)
{
    NEED(e);
    const int rc = fetch_meta(e, (hipStream_t)stream);
    if (rc) return rc;
    for (int b = 0; b < e->d.B; ++b) {
        const BoardMeta &m = e->h_meta[b];
        if (over_host) over_host[b] = m.over;
        if (winner_host) winner_host[b] = m.winner;
        if (plies_host) plies_host[b] = m.ply;
        if (turn_host) turn_host[b] = m.turn;
    }
    return 0;
}

int ccz_root_positions(ccz_engine *e, void *stream, uint8_t *sq_host)
{
    NEED(e);
    if (!sq_host) return fail(-1, "ccz_root_positions: null output");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(sq_host, e->d.root_sq, (size_t)e->d.B * 96, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_leaf_info(ccz_engine *e, void *stream, uint8_t *status_host, int32_t *k_host, uint16_t *ids_host, int32_t *depth_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    if (status_host) HIP_TRY(hipMemcpyAsync(status_host, e->d.leaf_status, B, hipMemcpyDeviceToHost, s));
    if (k_host) HIP_TRY(hipMemcpyAsync(k_host, e->d.leaf_k, B * 4, hipMemcpyDeviceToHost, s));
    if (ids_host) HIP_TRY(hipMemcpyAsync(ids_host, e->d.leaf_ids, B * kMaxLegal * 2, hipMemcpyDeviceToHost, s));
    if (depth_host) HIP_TRY(hipMemcpyAsync(depth_host, e->d.path_len, B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_leaf_priors(ccz_engine *e, void *stream, float *prior_host, float *value_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->d.B;
    if (value_host && !e->d.cache) return fail(-1, "ccz_leaf_priors: engine-owned leaf values exist only with an evaluation cache (pass value_host = NULL)");
    if (prior_host) HIP_TRY(hipMemcpyAsync(prior_host, e->d.prior128, B * kMaxLegal * 4, hipMemcpyDeviceToHost, s));
    if (value_host) HIP_TRY(hipMemcpyAsync(value_host, e->d.vleaf, B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_leaf_keys(ccz_engine *e, void *stream, uint64_t *keys_dev, uint8_t *status_dev)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    if (keys_dev) HIP_TRY(hipMemcpyAsync(keys_dev, e->d.leaf_key, (size_t)e->d.B * 8, hipMemcpyDeviceToDevice, s));
    if (status_dev) HIP_TRY(hipMemcpyAsync(status_dev, e->d.leaf_status, (size_t)e->d.B, hipMemcpyDeviceToDevice, s));
    return 0;
}

int ccz_harvest_rows(ccz_engine *e, void *stream, int64_t *rows_host)
{
    NEED(e);
    if (!rows_host) return fail(-1, "ccz_harvest_rows: null output");
    const int rc = fetch_meta(e, (hipStream_t)stream);
    if (rc) return rc;
    const int mul = (e->d.flags & CCZ_FLAG_NO_MIRROR) ? 1 : 2;
    int64_t rows = 0;
    for (int b = 0; b < e->d.B; ++b)
        if (e->h_meta[b].over) rows += (int64_t)e->h_meta[b].ply * mul;
    *rows_host = rows;
    return 0;
}

// The finished boards one harvest call takes, in units of `mul` per ply (rows or plies): in index order while they fit the caller's
// capacity; the rest stay finished and are picked up by the next call (many boards can reach the ply cap in the same move). base[b] =
// where board b's game starts in the output (-1: not taken). The first game must fit: else -5 with the caller's text `first_fmt`.
struct HarvestPlan {
    std::vector<long long> base;
    std::vector<uint8_t> mask;
    int64_t total = 0;
    bool any = false;
};

static int plan_harvest(ccz_engine *e, hipStream_t s, int mul, int64_t capacity, const char *first_fmt, HarvestPlan &p)
{
    const int rc = fetch_meta(e, s);
    if (rc) return rc;
    const int B = e->d.B;
    p.base.assign((size_t)B, -1);
    p.mask.assign((size_t)B, 0);
    for (int b = 0; b < B; ++b)
        if (e->h_meta[b].over && e->h_meta[b].ply > 0) { // (over with no ply: a parked board, ccz_set_positions -- nothing to emit, stays parked)
            const int64_t add = (int64_t)e->h_meta[b].ply * mul;
            if (p.total + add > capacity) {
                if (!p.any) return fail(-5, first_fmt, (long long)add, (long long)capacity);
                break;
            }
            p.base[b] = p.total;
            p.mask[b] = 1;
            p.any = true;
            p.total += add;
        }
    return 0;
}

// a new game on every board the plan took (syncs: st_mask and the plan's arrays are free afterwards)
static int restart_harvested(ccz_engine *e, hipStream_t s, const HarvestPlan &p)
{
    HIP_TRY(hipMemcpyAsync(e->st_mask, p.mask.data(), (size_t)e->d.B, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_reset, dim3(e->d.B), dim3(64), 0, s, e->d, (const uint8_t *)e->st_mask);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_harvest(ccz_engine *e, void *stream, void *states_f16_dev, float *pi_dev, float *z_dev, int64_t capacity_rows,
                int64_t *rows_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    HarvestPlan p;
    const int rc = plan_harvest(e, s, (e->d.flags & CCZ_FLAG_NO_MIRROR) ? 1 : 2, capacity_rows,
                                "ccz_harvest: the first finished game needs %lld rows, capacity %lld", p);
    if (rc) return rc;
    if (rows_host) *rows_host = p.total;
    if (!p.any) return 0;
    if (p.total > 0) {
        if (!states_f16_dev || !pi_dev || !z_dev) return fail(-1, "ccz_harvest: null output buffer");
        HIP_TRY(hipMemcpyAsync(e->st_rowbase, p.base.data(), (size_t)e->d.B * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_harvest, dim3(e->d.B, kHarvestSlices), dim3(256), 0, s, e->d, (const long long *)e->st_rowbase,
                           (uint16_t *)states_f16_dev, pi_dev, z_dev);
        HIP_TRY(hipGetLastError());
    }
    return restart_harvested(e, s, p);
}

int ccz_harvest_records(ccz_engine *e, void *stream, void *records_dev, int64_t capacity_plies, int64_t *plies_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    HarvestPlan p;
    if (const int rc = plan_harvest(e, s, 1, capacity_plies, "ccz_harvest_records: the first finished game has %lld plies, capacity %lld", p)) return rc;
    if (plies_host) *plies_host = p.total;
    if (!p.any) return 0;
    if (p.total > 0) {
        if (!records_dev) return fail(-1, "ccz_harvest_records: null output buffer");
        HIP_TRY(hipMemcpyAsync(e->st_rowbase, p.base.data(), (size_t)e->d.B * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_harvest_records, dim3(e->d.B, kHarvestSlices), dim3(256), 0, s, e->d, (const long long *)e->st_rowbase, (uint8_t *)records_dev);
        HIP_TRY(hipGetLastError());
    }
    return restart_harvested(e, s, p);
}

// plane_of_type_host (as ccz_config.plane_of_type, NULL or all zero = the reference's order) -> typepack of the record kernels
static int typepack_of(const char *who, const uint8_t *plane_of_type_host, uint32_t *typepack)
{
    uint8_t pot[8] = {0, 0, 1, 2, 3, 4, 5, 6};
    if (plane_of_type_host) {
        bool all_zero = true;
        for (int t = 0; t < 8; ++t) all_zero = all_zero && plane_of_type_host[t] == 0;
        if (!all_zero) {
            unsigned seen = 0;
            for (int t = 1; t <= 7; ++t) {
                const int c = plane_of_type_host[t];
                if (c > 6 || (seen >> c & 1u)) return fail(-1, "%s: plane_of_type[1..7] must be a permutation of 0..6", who);
                seen |= 1u << c;
                pot[t] = (uint8_t)c;
            }
        }
    }
    *typepack = 0;
    for (int t = 1; t <= 7; ++t) *typepack |= (uint32_t)(t - 1) << (3 * pot[t]);
    return 0;
}

// the argument checks of the two record -> row call families: what may be NULL is the caller's business, the rest is here
static int check_expand_args(const char *who, const void *records_dev, int64_t n_plies, uint32_t flags, const void *states_f16_dev, const float *value_dev,
                             int64_t ring_rows, int64_t head_row)
{
    if (!records_dev) return fail(-1, "%s: null buffer", who);
    if (((uintptr_t)records_dev | (uintptr_t)states_f16_dev) & 3) return fail(-1, "%s: buffers must be 4-byte aligned", who);
    if ((uintptr_t)value_dev & 3) return fail(-1, "%s: the values must be 4-byte aligned", who);
    if (n_plies > (int64_t)INT32_MAX) return fail(-1, "%s: too many records for one launch", who);
    const int64_t rows = n_plies * ((flags & CCZ_FLAG_NO_MIRROR) ? 1 : 2);
    if (ring_rows > 0 && rows > ring_rows) return fail(-1, "%s: %lld rows do not fit a ring of %lld", who, (long long)rows, (long long)ring_rows);
    if (ring_rows == 0 && head_row != 0) return fail(-1, "%s: head_row needs ring_rows", who);
    return 0;
}

static int check_sample_args(const char *who, const void *ring_dev, const int64_t *window_dev, const int64_t *draws_dev, int64_t batch,
                             const void *states_f16_dev, const float *pi_dev, const float *z_dev, const float *value_dev)
{
    if (!ring_dev || !window_dev || !draws_dev || !states_f16_dev || !pi_dev || !z_dev) return fail(-1, "%s: null buffer", who);
    if (((uintptr_t)ring_dev | (uintptr_t)states_f16_dev) & 3) return fail(-1, "%s: buffers must be 4-byte aligned", who);
    if ((uintptr_t)value_dev & 3) return fail(-1, "%s: the values must be 4-byte aligned", who);
    if (((uintptr_t)window_dev | (uintptr_t)draws_dev) & 7) return fail(-1, "%s: window and draws must be 8-byte aligned", who);
    if (batch > (int64_t)INT32_MAX) return fail(-1, "%s: too many rows for one launch", who);
    return 0;
}

int ccz_expand_records(void *stream, const void *records_dev, int64_t n_plies, uint32_t flags, const uint8_t *plane_of_type_host,
                       void *states_f16_dev, float *pi_dev, float *z_dev, int64_t ring_rows, int64_t head_row, int32_t *bad_records_dev,
                       uint8_t *target_dev, float *value_dev)
{
    const char *who = "ccz_expand_records";
    if (n_plies < 0 || ring_rows < 0 || head_row < 0) return fail(-1, "%s: negative size", who);
    if (n_plies == 0) return 0;
    const int dense = (states_f16_dev != nullptr) + (pi_dev != nullptr) + (z_dev != nullptr);
    // all three dense outputs, or none of them and a side output: the side-only mode of k_expand_records
    if (dense != 3 && !(dense == 0 && (target_dev || value_dev))) return fail(-1, "%s: null buffer", who);
    if (const int rc = check_expand_args(who, records_dev, n_plies, flags, states_f16_dev, value_dev, ring_rows, head_row)) return rc;
    uint32_t typepack = 0;
    if (const int rc = typepack_of(who, plane_of_type_host, &typepack)) return rc;
    hipLaunchKernelGGL(k_expand_records, dim3((unsigned)n_plies), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)records_dev, (long long)n_plies,
                       flags & (CCZ_FLAG_REFERENCE_QUIRKS | CCZ_FLAG_NO_MIRROR), typepack, (uint16_t *)states_f16_dev, pi_dev, z_dev,
                       (long long)ring_rows, (long long)head_row, bad_records_dev, target_dev, value_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_ring_retire(void *stream, const void *ring_dev, int64_t cap_plies, int64_t *window_dev, int64_t head_new, int32_t max_game_plies,
                    int32_t *bad_records_dev)
{
    if (cap_plies <= 0 || head_new < 0) return fail(-1, "ccz_ring_retire: capacity must be positive and head_new non-negative");
    if (max_game_plies <= 0 || max_game_plies > 65535) return fail(-1, "ccz_ring_retire: max_game_plies must be 1..65535 (the header's T is 16 bits)");
    if (cap_plies < 2 * (int64_t)max_game_plies) return fail(-1, "ccz_ring_retire: a ring of %lld plies is smaller than two games of %d", (long long)cap_plies, max_game_plies);
    if (!ring_dev || !window_dev) return fail(-1, "ccz_ring_retire: null buffer");
    if (((uintptr_t)ring_dev & 3) || ((uintptr_t)window_dev & 7)) return fail(-1, "ccz_ring_retire: the ring must be 4-byte, the window 8-byte aligned");
    hipLaunchKernelGGL(k_ring_retire, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint8_t *)ring_dev, (long long)cap_plies,
                       (long long *)window_dev, (long long)head_new, (int)max_game_plies, bad_records_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_sample_records(void *stream, const void *ring_dev, int64_t cap_plies, const int64_t *window_dev, const int64_t *draws_dev, int64_t batch,
                       uint32_t flags, const uint8_t *plane_of_type_host, void *states_f16_dev, float *pi_dev, float *z_dev, int32_t *bad_records_dev,
                       uint8_t *target_dev, float *value_dev)
{
    const char *who = "ccz_sample_records";
    if (cap_plies <= 0 || batch < 0) return fail(-1, "%s: capacity must be positive and batch non-negative", who);
    if (batch == 0) return 0;
    if (const int rc = check_sample_args(who, ring_dev, window_dev, draws_dev, batch, states_f16_dev, pi_dev, z_dev, value_dev)) return rc;
    uint32_t typepack = 0;
    if (const int rc = typepack_of(who, plane_of_type_host, &typepack)) return rc;
    hipLaunchKernelGGL(k_sample_records, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)ring_dev, (long long)cap_plies,
                       (const long long *)window_dev, (const long long *)draws_dev, (long long)batch,
                       flags & (CCZ_FLAG_REFERENCE_QUIRKS | CCZ_FLAG_NO_MIRROR), typepack, (uint16_t *)states_f16_dev, pi_dev, z_dev, bad_records_dev,
                       target_dev, value_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_sample_records_weighted(void *stream, const void *ring_dev, int64_t cap_plies, const int64_t *window_dev, const uint64_t *seed_dev, int32_t cap_q,
                                int64_t *chosen_dev, int32_t *fallback_dev, int64_t batch, uint32_t flags, const uint8_t *plane_of_type_host,
                                void *states_f16_dev, float *pi_dev, float *z_dev, int32_t *bad_records_dev, uint8_t *target_dev, float *value_dev)
{
    const char *who = "ccz_sample_records_weighted";
    if (cap_plies <= 0 || batch < 0) return fail(-1, "%s: capacity must be positive and batch non-negative", who);
    if (cap_q < 4096 || cap_q > 15 * 4096) return fail(-1, "%s: cap_q %d must be in 4096 .. 61440 (a cap of 1 .. 15 in 1/4096)", who, cap_q);
    if (batch == 0) return 0;
    if (const int rc = check_sample_args(who, ring_dev, window_dev, (const int64_t *)seed_dev, batch, states_f16_dev, pi_dev, z_dev, value_dev)) return rc;
    if ((uintptr_t)chosen_dev & 7) return fail(-1, "%s: chosen must be 8-byte aligned", who);
    if ((uintptr_t)fallback_dev & 3) return fail(-1, "%s: the fallback counter must be 4-byte aligned", who);
    uint32_t typepack = 0;
    if (const int rc = typepack_of(who, plane_of_type_host, &typepack)) return rc;
    hipLaunchKernelGGL(k_sample_records_weighted, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)ring_dev, (long long)cap_plies,
                       (const long long *)window_dev, seed_dev, (int)cap_q, (long long *)chosen_dev, fallback_dev, (long long)batch,
                       flags & (CCZ_FLAG_REFERENCE_QUIRKS | CCZ_FLAG_NO_MIRROR), typepack, (uint16_t *)states_f16_dev, pi_dev, z_dev, bad_records_dev,
                       target_dev, value_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- engine snapshots (cczero.h: "Engine snapshots"; the kernels and the blob's layout: cczero_snapshot.h)
static uint32_t snap_sections(const ccz_engine *e) { return (e->proof ? kSnapProof : 0u) | kSnapValues | (e->surprise_on ? kSnapSurprise : 0u); }
static size_t snap_dir_bytes(int B) { return ((size_t)B + 1) * 8 + (size_t)B * sizeof(BoardMeta); }
static uint64_t snap_sections_start(int B) { return snap_pad16((uint64_t)kSnapHeader + snap_dir_bytes(B)); }

// the settings as the device holds them, the sticky error word and the half word -> h (syncs)
static int snap_read_settings(ccz_engine *e, hipStream_t s, SnapHeader &h)
{
    SolverCfg sv;
    HIP_TRY(hipMemcpyAsync(&h.resign, e->d.rs_cfg, sizeof h.resign, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.explore, e->d.ex_cfg, sizeof h.explore, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.gumbel, e->d.gm_cfg, sizeof h.gumbel, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.search, e->d.sr_cfg, sizeof h.search, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.stop, e->d.es_cfg, sizeof h.stop, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.surprise, &e->sp_block->cfg, sizeof h.surprise, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&sv, e->d.sv_cfg, sizeof sv, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.err, e->d.err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.half, e->d.half, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    h.solver_enabled = sv.enabled;
    h.width = e->width;
    return 0;
}

// the header of a snapshot of this engine as it stands (without the total) and the section offsets on the device (e->snap_off), checked
// against the host's own sum over the meta records; *total = the snapshot's bytes. Syncs.
static int snap_prepare(ccz_engine *e, hipStream_t s, const char *who, uint64_t *total)
{
    const Dev &d = e->d;
    const int B = d.B;
    if (!e->snap_off) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(dalloc(&e->snap_off, (size_t)B + 1, e->owned, e->bytes));
    }
    const uint32_t sections = snap_sections(e);
    const BoardMeta *m0 = d.meta;
    hipLaunchKernelGGL(k_snapshot_layout, dim3(1), dim3(1024), 0, s, B, &m0->n_nodes, &m0->ply, &m0->pi_used, (int)(sizeof(BoardMeta) / 4), sections,
                       e->snap_off);
    HIP_TRY(hipGetLastError());
    uint64_t sum_dev = 0;
    HIP_TRY(hipMemcpyAsync(&sum_dev, e->snap_off + B, 8, hipMemcpyDeviceToHost, s));
    SnapHeader &h = e->snap_hdr;
    memset(&h, 0, sizeof h);
    if (const int rc = snap_read_settings(e, s, h)) return rc;
    if (const int rc = fetch_meta(e, s)) return rc;
    uint64_t sum = 0;
    for (int b = 0; b < B; ++b) {
        const BoardMeta &m = e->h_meta[(size_t)b];
        if (m.n_nodes < 0 || m.n_nodes > d.cap || m.ply < 0 || m.ply > d.max_plies || m.pi_used > (uint32_t)d.pi_cap)
            return fail(-1, "%s: board %d holds counts outside the engine's arrays (n_nodes %d, ply %d, pi_used %u)", who, b, m.n_nodes, m.ply, m.pi_used);
        sum += snap_section_bytes(sections, (uint64_t)m.n_nodes, (uint64_t)m.ply, (uint64_t)m.pi_used);
    }
    if (sum != sum_dev) return fail(-2, "%s: the layout kernel's total %llu differs from the host's %llu", who, (unsigned long long)sum_dev, (unsigned long long)sum);
    h.magic = kSnapMagic;
    h.version = kSnapVersion;
    h.header_bytes = (uint32_t)kSnapHeader;
    h.sections_start = snap_sections_start(B);
    h.total_bytes = h.sections_start + sum;
    h.B = d.B; h.cap = d.cap; h.maxd = d.maxd; h.max_plies = d.max_plies; h.pi_cap = d.pi_cap; h.reserve = d.reserve;
    h.c_puct = d.c_puct; h.flags = d.flags;
    h.eps = d.eps; h.alpha = d.alpha; h.temp = d.temp;
    h.seed = d.seed; h.board_id_base = d.board_id_base;
    h.rule_flags = d.rule_flags; h.chanpack = d.chanpack; h.typepack = d.typepack; h.trankpack = d.trankpack;
    h.rank_hash = e->rank_hash;
    h.sections = sections;
    h.budgets_on = e->budgets_on ? 1 : 0;
    h.fixed_bytes = (uint32_t)kSnapFixed;
    h.meta_bytes = (uint32_t)sizeof(BoardMeta);
    *total = h.total_bytes;
    return 0;
}

int ccz_snapshot_size(ccz_engine *e, void *stream, uint64_t *bytes_host)
{
    NEED(e);
    if (!bytes_host) return fail(-1, "ccz_snapshot_size: null output");
    return snap_prepare(e, (hipStream_t)stream, "ccz_snapshot_size", bytes_host);
}

int ccz_snapshot_save(ccz_engine *e, void *stream, void *blob_dev, uint64_t capacity, uint64_t *bytes_host)
{
    NEED(e);
    if (!blob_dev) return fail(-1, "ccz_snapshot_save: null blob");
    if ((uintptr_t)blob_dev & 15) return fail(-1, "ccz_snapshot_save: the blob must be 16-byte aligned");
    if (SCOUTS(e)) return fail(-1, "ccz_snapshot_save: not with scout slots (ccz_set_scouts): a scout slot has no game and no tree");
    if (e->spread_on) return fail(-1, "ccz_snapshot_save: not while the value spread is on (ccz_set_value_stats): its array is no snapshot section yet");
    hipStream_t s = (hipStream_t)stream;
    uint64_t total = 0;
    if (const int rc = snap_prepare(e, s, "ccz_snapshot_save", &total)) return rc;
    if (bytes_host) *bytes_host = total;
    if (capacity < total)
        return fail(-1, "ccz_snapshot_save: capacity %llu is below the snapshot's %llu bytes (nothing was written)", (unsigned long long)capacity,
                    (unsigned long long)total);
    const int B = e->d.B;
    uint8_t *blob = (uint8_t *)blob_dev;
    const size_t dir_end = (size_t)kSnapHeader + snap_dir_bytes(B);
    HIP_TRY(hipMemcpyAsync(blob, &e->snap_hdr, sizeof e->snap_hdr, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(blob + kSnapHeader, e->snap_off, ((size_t)B + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(blob + kSnapHeader + ((size_t)B + 1) * 8, e->d.meta, (size_t)B * sizeof(BoardMeta), hipMemcpyDeviceToDevice, s));
    if (e->snap_hdr.sections_start > dir_end) HIP_TRY(hipMemsetAsync(blob + dir_end, 0, (size_t)e->snap_hdr.sections_start - dir_end, s));
    hipLaunchKernelGGL(k_snapshot_pack, dim3((unsigned)B), dim3(256), 0, s, e->d, (const uint64_t *)e->snap_off, blob + e->snap_hdr.sections_start,
                       e->snap_hdr.sections, e->proof, e->wide_stats);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s)); // (the header travels from the engine's own host copy)
    return 0;
}

int ccz_snapshot_load(ccz_engine *e, void *stream, const void *blob_dev, uint64_t bytes, int32_t keep_board_id_base)
{
    NEED(e);
    if (!blob_dev) return fail(-1, "ccz_snapshot_load: null blob");
    if ((uintptr_t)blob_dev & 15) return fail(-1, "ccz_snapshot_load: the blob must be 16-byte aligned");
    if (SCOUTS(e)) return fail(-1, "ccz_snapshot_load: not with scout slots (ccz_set_scouts)");
    if (e->spread_on) return fail(-1, "ccz_snapshot_load: not while the value spread is on (ccz_set_value_stats): its array is no snapshot section yet");
    hipStream_t s = (hipStream_t)stream;
    const Dev &d = e->d;
    const int B = d.B;
    const uint8_t *blob = (const uint8_t *)blob_dev;
    if (bytes < (uint64_t)kSnapHeader) return fail(-1, "ccz_snapshot_load: truncated: %llu bytes are less than the header's %d", (unsigned long long)bytes, kSnapHeader);
    // ---- everything below up to the unpack launch only reads: a refused blob leaves the engine exactly as it was
    SnapHeader &h = e->snap_hdr;
    HIP_TRY(hipMemcpyAsync(&h, blob, sizeof h, hipMemcpyDeviceToHost, s));
    SnapHeader mine;
    memset(&mine, 0, sizeof mine);
    if (const int rc = snap_read_settings(e, s, mine)) return rc; // syncs
    if (h.magic != kSnapMagic) return fail(-1, "ccz_snapshot_load: bad magic 0x%016llx (not an engine snapshot)", (unsigned long long)h.magic);
    if (h.version != kSnapVersion) return fail(-1, "ccz_snapshot_load: format version %u, this library reads %u", h.version, kSnapVersion);
    if (h.header_bytes != (uint32_t)kSnapHeader || h.fixed_bytes != (uint32_t)kSnapFixed || h.meta_bytes != (uint32_t)sizeof(BoardMeta))
        return fail(-1, "ccz_snapshot_load: header_bytes / fixed_bytes / meta_bytes %u / %u / %u, this library reads %d / %d / %d", h.header_bytes,
                    h.fixed_bytes, h.meta_bytes, kSnapHeader, kSnapFixed, (int)sizeof(BoardMeta));
#define SNAP_SAME(NAME_, FMT_, CAST_, A_, B_)                                                                                           \
    if ((A_) != (B_)) return fail(-1, "ccz_snapshot_load: " NAME_ " differs: the snapshot has " FMT_ ", the engine " FMT_, (CAST_)(A_), (CAST_)(B_))
    SNAP_SAME("B (n_boards)", "%d", int, h.B, d.B);
    SNAP_SAME("cap (max_nodes)", "%d", int, h.cap, d.cap);
    SNAP_SAME("maxd (max_depth)", "%d", int, h.maxd, d.maxd);
    SNAP_SAME("max_plies", "%d", int, h.max_plies, d.max_plies);
    SNAP_SAME("pi_cap", "%d", int, h.pi_cap, d.pi_cap);
    SNAP_SAME("reserve (reserve_nodes)", "%d", int, h.reserve, d.reserve);
    SNAP_SAME("c_puct", "%.9g", double, h.c_puct, d.c_puct);
    SNAP_SAME("eps", "%.17g", double, h.eps, d.eps);
    SNAP_SAME("alpha", "%.17g", double, h.alpha, d.alpha);
    SNAP_SAME("temp", "%.17g", double, h.temp, d.temp);
    SNAP_SAME("flags", "0x%x", unsigned, h.flags, d.flags);
    SNAP_SAME("seed", "%llu", unsigned long long, h.seed, d.seed);
    if (!keep_board_id_base && h.board_id_base != d.board_id_base)
        return fail(-1, "ccz_snapshot_load: board_id_base differs: the snapshot has %llu, the engine %llu (keep_board_id_base = 1 keeps the engine's)",
                    (unsigned long long)h.board_id_base, (unsigned long long)d.board_id_base);
    SNAP_SAME("rule_flags", "0x%x", unsigned, h.rule_flags, d.rule_flags);
    SNAP_SAME("chanpack (plane_of_type)", "0x%x", unsigned, h.chanpack, d.chanpack);
    SNAP_SAME("typepack (plane_of_type)", "0x%x", unsigned, h.typepack, d.typepack);
    SNAP_SAME("trankpack (type_rank)", "0x%x", unsigned, h.trankpack, d.trankpack);
    SNAP_SAME("the move-rank table's hash", "0x%016llx", unsigned long long, h.rank_hash, e->rank_hash);
    SNAP_SAME("width (ccz_set_width)", "%d", int, h.width, mine.width);
    SNAP_SAME("solver enabled (ccz_set_solver)", "%d", int, h.solver_enabled, mine.solver_enabled);
    SNAP_SAME("resign.enabled", "%d", int, h.resign.enabled, mine.resign.enabled);
    SNAP_SAME("resign.consecutive", "%d", int, h.resign.consecutive, mine.resign.consecutive);
    SNAP_SAME("resign.min_ply", "%d", int, h.resign.min_ply, mine.resign.min_ply);
    SNAP_SAME("resign.threshold", "%.9g", double, h.resign.threshold, mine.resign.threshold);
    SNAP_SAME("resign.p_playon", "%.17g", double, h.resign.p_playon, mine.resign.p_playon);
    SNAP_SAME("root_exploration.enabled", "%d", int, h.explore.enabled, mine.explore.enabled);
    SNAP_SAME("root_exploration.prune", "%d", int, h.explore.prune, mine.explore.prune);
    SNAP_SAME("root_exploration.eps", "%.17g", double, h.explore.eps, mine.explore.eps);
    SNAP_SAME("root_exploration.alpha", "%.17g", double, h.explore.alpha, mine.explore.alpha);
    SNAP_SAME("root_exploration.forced_k", "%.17g", double, h.explore.forced_k, mine.explore.forced_k);
    SNAP_SAME("gumbel.enabled", "%d", int, h.gumbel.enabled, mine.gumbel.enabled);
    SNAP_SAME("gumbel.n_sims", "%d", int, h.gumbel.n_sims, mine.gumbel.n_sims);
    SNAP_SAME("gumbel.max_considered", "%d", int, h.gumbel.max_considered, mine.gumbel.max_considered);
    SNAP_SAME("gumbel.c_visit", "%.17g", double, h.gumbel.c_visit, mine.gumbel.c_visit);
    SNAP_SAME("gumbel.c_scale", "%.17g", double, h.gumbel.c_scale, mine.gumbel.c_scale);
    SNAP_SAME("search.enabled", "%d", int, h.search.enabled, mine.search.enabled);
    SNAP_SAME("search.fpu_mode", "%d", int, h.search.fpu_mode, mine.search.fpu_mode);
    SNAP_SAME("search.fpu_root_mode", "%d", int, h.search.fpu_root_mode, mine.search.fpu_root_mode);
    SNAP_SAME("search.fpu_value", "%.17g", double, h.search.fpu_value, mine.search.fpu_value);
    SNAP_SAME("search.fpu_root_value", "%.17g", double, h.search.fpu_root_value, mine.search.fpu_root_value);
    SNAP_SAME("search.c_base", "%.17g", double, h.search.c_base, mine.search.c_base);
    SNAP_SAME("search.c_factor", "%.17g", double, h.search.c_factor, mine.search.c_factor);
    SNAP_SAME("early_stop.enabled", "%d", int, h.stop.enabled, mine.stop.enabled);
    SNAP_SAME("early_stop.single_reply", "%d", int, h.stop.single_reply, mine.stop.single_reply);
    SNAP_SAME("early_stop.kld_interval", "%d", int, h.stop.kld_interval, mine.stop.kld_interval);
    SNAP_SAME("early_stop.min_sims", "%d", int, h.stop.min_sims, mine.stop.min_sims);
    SNAP_SAME("early_stop.n_sims", "%d", int, h.stop.n_sims, mine.stop.n_sims);
    SNAP_SAME("early_stop.gap_factor", "%.17g", double, h.stop.gap_factor, mine.stop.gap_factor);
    SNAP_SAME("early_stop.min_gain", "%.17g", double, h.stop.min_gain, mine.stop.min_gain);
    SNAP_SAME("surprise.enabled", "%d", int, h.surprise.enabled, mine.surprise.enabled);
    SNAP_SAME("surprise.alpha", "%.17g", double, h.surprise.alpha, mine.surprise.alpha);
    SNAP_SAME("surprise.cap", "%.17g", double, h.surprise.cap, mine.surprise.cap);
#undef SNAP_SAME
    if (h.sections & ~(kSnapProof | kSnapValues | kSnapSurprise)) return fail(-1, "ccz_snapshot_load: unknown sections bits 0x%x", h.sections);
    if (h.total_bytes != bytes)
        return fail(-1, "ccz_snapshot_load: total size: the header says %llu bytes, the caller passes %llu (a truncated or padded blob)",
                    (unsigned long long)h.total_bytes, (unsigned long long)bytes);
    const uint64_t start = snap_sections_start(B);
    if (h.sections_start != start || bytes < start)
        return fail(-1, "ccz_snapshot_load: sections_start %llu, expected %llu within %llu bytes", (unsigned long long)h.sections_start,
                    (unsigned long long)start, (unsigned long long)bytes);
    // ---- the directory: offsets monotone and inside the blob, every board's counts inside the engine's arrays, every section as long
    // as its counts say
    e->snap_dir.resize((snap_dir_bytes(B) + 7) / 8);
    HIP_TRY(hipMemcpyAsync(e->snap_dir.data(), blob + kSnapHeader, snap_dir_bytes(B), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t *off = e->snap_dir.data();
    const uint8_t *metab = (const uint8_t *)(off + B + 1);
    if (off[0] != 0) return fail(-1, "ccz_snapshot_load: offsets[0] is %llu, not 0", (unsigned long long)off[0]);
    for (int b = 0; b < B; ++b)
        if (off[b + 1] < off[b] || off[b + 1] > bytes - start)
            return fail(-1, "ccz_snapshot_load: offsets[%d] = %llu after %llu: the offset table is not monotone inside the blob's %llu section bytes", b + 1,
                        (unsigned long long)off[b + 1], (unsigned long long)off[b], (unsigned long long)(bytes - start));
    for (int b = 0; b < B; ++b) {
        BoardMeta m;
        memcpy(&m, metab + (size_t)b * sizeof(BoardMeta), sizeof m);
        if (m.n_nodes < 1 || m.n_nodes > d.cap) return fail(-1, "ccz_snapshot_load: board %d: n_nodes %d outside 1 .. cap %d", b, m.n_nodes, d.cap);
        if (m.ply < 0 || m.ply > d.max_plies) return fail(-1, "ccz_snapshot_load: board %d: ply %d outside 0 .. max_plies %d", b, m.ply, d.max_plies);
        if (m.pi_used > (uint32_t)d.pi_cap) return fail(-1, "ccz_snapshot_load: board %d: pi_used %u above pi_cap %d", b, m.pi_used, d.pi_cap);
        if (m.chain_len < 1 || m.chain_len > kChainCap) return fail(-1, "ccz_snapshot_load: board %d: chain_len %d outside 1 .. %d", b, m.chain_len, kChainCap);
        const uint64_t want = snap_section_bytes(h.sections, (uint64_t)m.n_nodes, (uint64_t)m.ply, (uint64_t)m.pi_used);
        if (off[b + 1] - off[b] != want)
            return fail(-1, "ccz_snapshot_load: offsets[%d] .. offsets[%d] span %llu bytes, board %d's counts need %llu", b, b + 1,
                        (unsigned long long)(off[b + 1] - off[b]), b, (unsigned long long)want);
    }
    if (start + off[B] != bytes)
        return fail(-1, "ccz_snapshot_load: offsets[%d] = %llu ends the sections at %llu of %llu bytes", B, (unsigned long long)off[B],
                    (unsigned long long)(start + off[B]), (unsigned long long)bytes);
    // ---- the writes
    hipLaunchKernelGGL(k_snapshot_unpack, dim3((unsigned)B), dim3(256), 0, s, e->d, (const uint64_t *)(blob + kSnapHeader),
                       (const BoardMeta *)(blob + kSnapHeader + ((size_t)B + 1) * 8), const_cast<uint8_t *>(blob) + start, h.sections, e->proof, e->wide_stats);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(e->d.err, &h.err, 4, hipMemcpyHostToDevice, s));
    if (const int rc = ccz_eval_cache_clear(e, stream)) return rc; // a cold cache: claim refilled with it
    if (e->wide_F) { // a move boundary: no leaf in flight, on any slot
        HIP_TRY(hipMemsetAsync(e->wide_F, 0, (size_t)B * 2 * (size_t)d.cap, s));
        hipLaunchKernelGGL(k_wide_clear_slots, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, e->d, 0);
        HIP_TRY(hipGetLastError());
    }
    e->budgets_on = h.budgets_on != 0;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int ccz_snapshot_layout(void *stream, int32_t B, const int32_t *n_nodes_dev, const int32_t *ply_dev, const uint32_t *pi_used_dev, uint32_t sections,
                        uint64_t *offsets_dev)
{
    if (B < 1 || !n_nodes_dev || !ply_dev || !pi_used_dev || !offsets_dev) return fail(-1, "ccz_snapshot_layout: bad arguments");
    if (sections & ~(kSnapProof | kSnapValues | kSnapSurprise)) return fail(-1, "ccz_snapshot_layout: unknown sections bits 0x%x", sections);
    hipLaunchKernelGGL(k_snapshot_layout, dim3(1), dim3(1024), 0, (hipStream_t)stream, (int)B, n_nodes_dev, ply_dev, pi_used_dev, 1, sections, offsets_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_get_stats(ccz_engine *e, void *stream, ccz_stats *out)
{
    NEED(e);
    if (!out) return fail(-1, "ccz_get_stats: null output");
    hipStream_t s = (hipStream_t)stream;
    std::vector<BoardStats> st((size_t)e->d.B);
    int32_t err[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(st.data(), e->d.stats, st.size() * sizeof(BoardStats), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(err, e->d.err, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    for (const BoardStats &b : st) {
        out->sims += (int64_t)b.sims;
        out->moves += (int64_t)b.moves;
        out->games += (int64_t)b.games;
        out->truncated_games += (int64_t)b.truncated;
        out->sum_depth += (int64_t)b.sum_depth;
        out->sum_children += (int64_t)b.sum_children;
        out->expansions += (int64_t)b.expansions;
        out->terminal_leaves += (int64_t)b.terminal;
        out->pruned_subtrees += (int64_t)b.pruned;
        out->cache_probes += (int64_t)b.cache_probes;
        out->cache_hits += (int64_t)b.cache_hits;
        out->cache_shared_rows += (int64_t)b.cache_shared;
        out->cache_stores += (int64_t)b.cache_stores;
        out->cache_verified += (int64_t)b.cache_verified;
        out->cache_verify_mismatches += (int64_t)b.cache_mismatch;
        if (b.nodes_peak > out->nodes_peak) out->nodes_peak = b.nodes_peak;
        if (b.depth_peak > out->depth_peak) out->depth_peak = b.depth_peak;
    }
    out->error_flags = err[0];
    out->reserved = err[1]; // bounds-checked diagnostic build: source line of the stray index (0 otherwise)
    out->hbm_bytes = (int64_t)e->bytes;
    return 0;
}

int ccz_legal_moves(void *stream, int32_t n, const uint8_t *sq_dev, const uint8_t *turn_dev, const int32_t *halfmove_dev,
                    uint32_t *mask_dev, int32_t *count_dev, uint8_t *flags_dev)
{
    if (n < 0 || !sq_dev || !turn_dev) return fail(-1, "ccz_legal_moves: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_legal_moves, dim3(n), dim3(64), 0, (hipStream_t)stream, n, sq_dev, turn_dev, halfmove_dev, mask_dev,
                       count_dev, flags_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_apply_moves(void *stream, int32_t n, uint8_t *sq_dev, uint8_t *turn_dev, const int32_t *move_ids_dev, uint8_t *captured_dev)
{
    if (n < 0 || !sq_dev || !turn_dev || !move_ids_dev) return fail(-1, "ccz_apply_moves: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_apply_moves, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, sq_dev, turn_dev, move_ids_dev,
                       captured_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_bias_act_f16(void *stream, void *y_dev, const void *bias_dev, const void *residual_dev, int64_t rows, int32_t channels)
{
    if (!y_dev || !bias_dev || rows < 0 || channels <= 0 || (channels & 7)) return fail(-1, "ccz_bias_act_f16: bad arguments (channels must be a multiple of 8)");
    if ((((uintptr_t)y_dev) | ((uintptr_t)bias_dev) | ((uintptr_t)residual_dev)) & 15) return fail(-1, "ccz_bias_act_f16: pointers must be 16-byte aligned");
    const long n_vec = rows * (long)(channels / 8);
    if (n_vec == 0) return 0;
    long blocks = (n_vec + 255) / 256;
    if (blocks > 4096) blocks = 4096; // grid-stride: 16 resident blocks per CU
    if (residual_dev)
        hipLaunchKernelGGL(k_bias_act<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (half8_t *)y_dev, (const half8_t *)bias_dev,
                           (const half8_t *)residual_dev, n_vec, channels / 8);
    else
        hipLaunchKernelGGL(k_bias_act<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (half8_t *)y_dev, (const half8_t *)bias_dev,
                           (const half8_t *)nullptr, n_vec, channels / 8);
    HIP_TRY(hipGetLastError());
    return 0;
}

static_assert(((int64_t)INT32_MAX / kCvC) * kCvC * 2 <= (int64_t)UINT32_MAX, "the largest accepted activation tensor must fit 32-bit byte offsets / num_records");
constexpr int64_t kSmallMaxPixels = 64 * 90; // up to 64 boards (profiles/r03_single_board.json: crossover with the tile kernel)

static int conv3x3_launch(const char *who, void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev, void *y_dev,
                          int64_t n_pixels, int32_t relu, int cin, const int32_t *live_rows_dev = nullptr, int32_t row0 = 0, bool g16c = false)
{
    if (!x_dev || !w_dev || !bias_f32_dev || !y_dev || n_pixels < 0 || n_pixels % 90 || n_pixels > (int64_t)INT32_MAX / kCvC) /* 32-bit BYTE offsets and a 32-bit num_records in the kernels: n_pixels * kCvC * 2 < 2^32, see the static_assert below */
        return fail(-1, "%s: bad arguments (n_pixels must be boards * 90, at most 93206 boards per call)", who);
    if ((((uintptr_t)x_dev) | ((uintptr_t)w_dev) | ((uintptr_t)bias_f32_dev) | ((uintptr_t)residual_dev) | ((uintptr_t)y_dev)) & 15)
        return fail(-1, "%s: pointers must be 16-byte aligned", who);
    if (x_dev == y_dev) return fail(-1, "%s: the output may alias the residual but not the input", who);
    if (n_pixels == 0) return 0;
    if (relu & CCZ_CONV_G16) { // rows in the group-of-16 layout: whole-rank tiles, off-board taps skipped (cczero_conv_g16.h)
        if (relu & (256 | (0xffe << 16))) // the persistent form's flag and workgroup count (round 6; removed in ABI 8): refused, not ignored
            return fail(-1, "%s: flag 256 / bits 17..27 were CCZ_CONV_G16_PERSISTENT, retired in ABI 8", who); // (bit 16 is CCZ_CONV_G16_QUAD now)
        if (n_pixels % 1440) return fail(-1, "%s: CCZ_CONV_G16 needs a multiple of 16 boards", who);
        const int groups = (int)(n_pixels / 1440);
        const int fl = relu & 3;
        hipStream_t s = (hipStream_t)stream;
        const G16Shape shape = g16_shape(groups, relu);
        const G16Args a = {(const _Float16 *)x_dev, (const _Float16 *)w_dev, (const float *)bias_f32_dev, (const _Float16 *)residual_dev, (_Float16 *)y_dev,
                           (int)n_pixels, cin, (const int *)live_rows_dev, (int)row0};
        const bool res = residual_dev != nullptr;
        if (g16c) { // the chunk-major G16C layout (cczero_conv_g16.h g16c_off): the stem, and the quad one-launch form of a tower layer
            if (cin == 64) {
                hipLaunchKernelGGL(k_conv3x3_g16c_stem, dim3((unsigned)(groups * 5)), dim3(512), 0, s, (const _Float16 *)x_dev, (const _Float16 *)w_dev,
                                   (const float *)bias_f32_dev, (_Float16 *)y_dev, (int)n_pixels, (int)fl, cin, (const int *)live_rows_dev, (int)row0);
                HIP_TRY(hipGetLastError());
                return 0;
            }
            const int need = CCZ_CONV_G16_EDGE_TILES | CCZ_CONV_G16_ONE_LAUNCH | CCZ_CONV_G16_QUAD;
            if ((relu & need) != need)
                return fail(-1, "%s: the G16C layout runs the quad one-launch form only (CCZ_CONV_G16_EDGE_TILES | _ONE_LAUNCH | _QUAD)", who);
            // (a single group too: its edge pair is that group twice, as for an odd live count)
            g16_launch(CCZ_G16_RES(k_conv3x3_g16c_one_quad, res), (unsigned)(groups * 4 + 2 * ((groups + 1) / 2)), s, a, fl);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        // Without the flag: ONE launch of five two-rank tiles per group. CCZ_CONV_G16_EDGE_TILES (flag bit 7, round 4): the edge ranks (0
        // and 9) of two groups at a time are their own tiles on their own kernel (six live taps instead of nine, cczero_conv_g16e.h) and
        // the middle launch covers ranks 1..8 with four two-rank tiles per group -- two ordinary launches back to back in the caller's
        // stream (no gap between them in the kernel trace). Same values. Measured (profiles/r04_conv_g16.json): -3 % per layer at 4096
        // boards in isolation (1024 middle tiles = four full rounds of 256 CUs, 256 edge tiles = one round ~24 % shorter); in the
        // workload +0.7 % on the step with two launch chains (the extra launch boundary per layer and chain costs more than the six
        // taps save) but -0.7...-0.9 % with three: the evaluator sets the flag from 4096 boards on and runs three chains then. (The
        // edge launch on a helper stream beside the middle one put two event packets per layer on the main stream -- a 12.7 us gap
        // between layers; hipExtAnyOrderLaunch is ignored on gfx9: the trace shows the kernels one after the other.)
        if (cin == 64) { // the stem: the packed live planes sit in channels 0..20 of 64: ONE 32-channel chunk (k_conv3x3_g16_stem), one launch
            hipLaunchKernelGGL(k_conv3x3_g16_stem, dim3((unsigned)(groups * 5)), dim3(512), 0, s, (const _Float16 *)x_dev, (const _Float16 *)w_dev,
                               (const float *)bias_f32_dev, (_Float16 *)y_dev, (int)n_pixels, (int)fl, cin, (const int *)live_rows_dev, (int)row0);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        if (!shape.edge) {
            g16_launch(CCZ_G16_RES(k_conv3x3_g16, res), shape.mid, s, a, fl);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        // CCZ_CONV_G16_QUAD: the middle slots as four-rank x 128-channel tiles (cczero_conv_g16.h g5q_tile) -- as many, as large, half the weight stream
        const bool quad = (relu & CCZ_CONV_G16_QUAD) != 0;
        if (relu & CCZ_CONV_G16_ONE_LAUNCH) { // both tile classes in one launch (cczero_conv_g16e.h k_conv3x3_g16_one)
            g16_launch(quad ? CCZ_G16_RES(k_conv3x3_g16_one_quad, res) : CCZ_G16_RES(k_conv3x3_g16_one, res), shape.mid + shape.edge, s, a, fl);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        if (quad) g16_launch(CCZ_G16_RES(k_conv3x3_g16_quad, res), shape.mid, s, a, fl);
        else g16_launch(CCZ_G16_RES(k_conv3x3_g16, res), shape.mid, s, a, fl | 4);   // (edge launch first: measured the same, 194.4 / 194.3 k against 194.8 / 194.0 k sims/s)
        HIP_TRY(hipGetLastError());
        g16_launch(CCZ_G16_RES(k_conv3x3_g16_edge, res), shape.edge, s, a, fl);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // Small batches (one game at a time; up to kSmallMaxPixels): the 16-channel x 64-pixel-block kernel spreads them over the chip
    // instead of filling a few 256-pixel tiles. Same operations in the same order: bit-identical results (cczero_conv_small.h).
    // flags bit 4 forces it, bit 5 forces the tile kernel (A/B runs, tests).
    if (cin != 128 && !live_rows_dev && !(relu & 32) && ((relu & 16) || n_pixels <= kSmallMaxPixels)) { // (128, the history stem: the tile kernel at any size)
        const dim3 grid((unsigned)((n_pixels + kSmPix - 1) / kSmPix), 16);
        const int rl = relu & 1;
#define CCZ_SMALL(RES_, CIN_)                                                                                                  \
        hipLaunchKernelGGL((k_conv3x3_small<RES_, CIN_, kCvC>), grid, dim3(256), 0, (hipStream_t)stream, (const _Float16 *)x_dev, (const _Float16 *)w_dev, \
                           (const float *)bias_f32_dev, (const _Float16 *)residual_dev, (_Float16 *)y_dev, (int)n_pixels, rl)
        if (cin == 64) CCZ_SMALL(false, 64);
        else if (residual_dev) CCZ_SMALL(true, 256);
        else CCZ_SMALL(false, 256);
#undef CCZ_SMALL
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const unsigned tiles = (unsigned)((n_pixels + kCvBM - 1) / kCvBM);
#ifndef CCZ_STAMPS
    relu &= 3; // bit 0: ReLU, bit 1: descending tile order; the diagnostic build passes ablation switches in bits 8.. (profiles/conv_microbench.py)
#endif
    if (residual_dev)
        hipLaunchKernelGGL(k_conv3x3_c256<true>, dim3(tiles), dim3(512), 0, (hipStream_t)stream, (const _Float16 *)x_dev, (const _Float16 *)w_dev,
                           (const float *)bias_f32_dev, (const _Float16 *)residual_dev, (_Float16 *)y_dev, (int)n_pixels, (int)relu, cin, (const int *)live_rows_dev, (int)row0);
    else
        hipLaunchKernelGGL(k_conv3x3_c256<false>, dim3(tiles), dim3(512), 0, (hipStream_t)stream, (const _Float16 *)x_dev, (const _Float16 *)w_dev,
                           (const float *)bias_f32_dev, (const _Float16 *)nullptr, (_Float16 *)y_dev, (int)n_pixels, (int)relu, cin, (const int *)live_rows_dev, (int)row0);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_conv3x3_c256_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev, void *y_dev,
                         int64_t n_pixels, int32_t relu)
{
    return conv3x3_launch("ccz_conv3x3_c256_f16", stream, x_dev, w_dev, bias_f32_dev, residual_dev, y_dev, n_pixels, relu, 256);
}

// ---- the chunk-major "G16C" activation layout (cczero_conv_g16.h g16c_off): additive twins of the CCZ_CONV_G16 calls ----
int ccz_conv3x3_c256_g16c_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev, void *y_dev,
                              int64_t n_pixels, int32_t relu)
{
    if (!(relu & CCZ_CONV_G16)) return fail(-1, "ccz_conv3x3_c256_g16c_f16: CCZ_CONV_G16 must be set");
    return conv3x3_launch("ccz_conv3x3_c256_g16c_f16", stream, x_dev, w_dev, bias_f32_dev, residual_dev, y_dev, n_pixels, relu, 256, nullptr, 0, true);
}

int ccz_conv3x3_c256_g16c_f16_live(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev, void *y_dev,
                                   int64_t n_pixels, int32_t relu, const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    if (!(relu & CCZ_CONV_G16)) return fail(-1, "ccz_conv3x3_c256_g16c_f16_live: CCZ_CONV_G16 must be set");
    if (!live_rows_dev || g16_bad_part(part, n_parts)) return fail(-1, "ccz_conv3x3_c256_g16c_f16_live: null live-row count or bad part / n_parts");
    return conv3x3_launch("ccz_conv3x3_c256_g16c_f16_live", stream, x_dev, w_dev, bias_f32_dev, residual_dev, y_dev, n_pixels, relu, 256, live_rows_dev,
                          part | (n_parts << 16), true);
}

int ccz_conv3x3_stem_g16c_f16(void *stream, const void *x64_dev, const void *w_dev, const void *bias_f32_dev, void *y_dev, int64_t n_pixels, int32_t relu)
{
    if (!(relu & CCZ_CONV_G16)) return fail(-1, "ccz_conv3x3_stem_g16c_f16: CCZ_CONV_G16 must be set");
    return conv3x3_launch("ccz_conv3x3_stem_g16c_f16", stream, x64_dev, w_dev, bias_f32_dev, nullptr, y_dev, n_pixels, relu, 64, nullptr, 0, true);
}

int ccz_conv3x3_stem_g16c_f16_live(void *stream, const void *x64_dev, const void *w_dev, const void *bias_f32_dev, void *y_dev, int64_t n_pixels, int32_t relu,
                                   const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    if (!(relu & CCZ_CONV_G16)) return fail(-1, "ccz_conv3x3_stem_g16c_f16_live: CCZ_CONV_G16 must be set");
    if (!live_rows_dev || g16_bad_part(part, n_parts)) return fail(-1, "ccz_conv3x3_stem_g16c_f16_live: null live-row count or bad part / n_parts");
    return conv3x3_launch("ccz_conv3x3_stem_g16c_f16_live", stream, x64_dev, w_dev, bias_f32_dev, nullptr, y_dev, n_pixels, relu, 64, live_rows_dev,
                          part | (n_parts << 16), true);
}

static int heads_layer_launch(const char *who, bool g16c, void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev,
                              const void *head_w32_dev, const void *head_b32_dev, void *pol_dev, void *val_dev, int64_t n_pixels, int32_t flags,
                              const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    if (!x_dev || !w_dev || !bias_f32_dev || !residual_dev || !head_w32_dev || !head_b32_dev || !pol_dev || !val_dev || n_pixels < 0 || n_pixels % 1440 ||
        n_pixels > (int64_t)INT32_MAX / kCvC)
        return fail(-1, "%s: bad arguments (n_pixels must be a multiple of 16 boards * 90, at most 93200 boards per call)", who);
    if (!(flags & CCZ_CONV_G16)) return fail(-1, "%s: rows must be in the group-of-16 layout (CCZ_CONV_G16)", who);
    if ((((uintptr_t)x_dev) | ((uintptr_t)w_dev) | ((uintptr_t)bias_f32_dev) | ((uintptr_t)residual_dev) | ((uintptr_t)head_w32_dev) | ((uintptr_t)head_b32_dev)) & 15)
        return fail(-1, "%s: pointers must be 16-byte aligned", who);
    if ((((uintptr_t)pol_dev) | ((uintptr_t)val_dev)) & 1) return fail(-1, "%s: outputs must be 2-byte aligned", who);
    if (live_rows_dev && g16_bad_part(part, n_parts)) return fail(-1, "%s: bad part / n_parts", who);
    if (n_pixels == 0) return 0;
    const G16Shape shape = g16_shape((int)(n_pixels / 1440), flags);
    const int fl = flags & 3;
    const G16Args a = {(const _Float16 *)x_dev, (const _Float16 *)w_dev, (const float *)bias_f32_dev, (const _Float16 *)residual_dev, nullptr,
                       (int)n_pixels, 256, (const int *)live_rows_dev, live_rows_dev ? (part | (n_parts << 16)) : 0};
    G5Heads ha;
    ha.w32 = (const _Float16 *)head_w32_dev;
    ha.b32 = (const float *)head_b32_dev;
    ha.pol = (_Float16 *)pol_dev;
    ha.val = (_Float16 *)val_dev;
    ha.nb = (int)(n_pixels / 90);
    hipStream_t s = (hipStream_t)stream;
    if (g16c) { // middle + edge-pair launches whatever the group count (a single group: its edge pair is that group twice)
        if (!(flags & CCZ_CONV_G16_EDGE_TILES)) return fail(-1, "%s: the G16C layout needs CCZ_CONV_G16_EDGE_TILES", who);
        const int groups = (int)(n_pixels / 1440);
        g16_launch(k_conv3x3_g16c_heads, (unsigned)(groups * 4), s, a, fl | 4, ha);
        HIP_TRY(hipGetLastError());
        g16_launch(k_conv3x3_g16c_edge_heads, 2u * (unsigned)((groups + 1) / 2), s, a, fl, ha);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    g16_launch(k_conv3x3_g16_heads, shape.mid, s, a, shape.edge ? fl | 4 : fl, ha);
    HIP_TRY(hipGetLastError());
    if (!shape.edge) return 0;
    g16_launch(k_conv3x3_g16_edge_heads, shape.edge, s, a, fl, ha);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_conv3x3_c256_heads_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev,
                               const void *head_w32_dev, const void *head_b32_dev, void *pol_dev, void *val_dev, int64_t n_pixels, int32_t flags,
                               const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    return heads_layer_launch("ccz_conv3x3_c256_heads_f16", false, stream, x_dev, w_dev, bias_f32_dev, residual_dev, head_w32_dev, head_b32_dev, pol_dev, val_dev,
                              n_pixels, flags, live_rows_dev, part, n_parts);
}

int ccz_conv3x3_c256_heads_g16c_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev,
                                    const void *head_w32_dev, const void *head_b32_dev, void *pol_dev, void *val_dev, int64_t n_pixels, int32_t flags,
                                    const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    return heads_layer_launch("ccz_conv3x3_c256_heads_g16c_f16", true, stream, x_dev, w_dev, bias_f32_dev, residual_dev, head_w32_dev, head_b32_dev, pol_dev, val_dev,
                              n_pixels, flags, live_rows_dev, part, n_parts);
}

int ccz_conv3x3_stem_f16(void *stream, const void *x64_dev, const void *w_dev, const void *bias_f32_dev, void *y_dev, int64_t n_pixels, int32_t relu)
{
    return conv3x3_launch("ccz_conv3x3_stem_f16", stream, x64_dev, w_dev, bias_f32_dev, nullptr, y_dev, n_pixels, relu, 64);
}

int ccz_conv3x3_c256_f16_live(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev, void *y_dev,
                              int64_t n_pixels, int32_t relu, const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    if (!live_rows_dev || g16_bad_part(part, n_parts)) return fail(-1, "ccz_conv3x3_c256_f16_live: null live-row count or bad part / n_parts");
    return conv3x3_launch("ccz_conv3x3_c256_f16_live", stream, x_dev, w_dev, bias_f32_dev, residual_dev, y_dev, n_pixels, relu, 256, live_rows_dev, part | (n_parts << 16));
}

int ccz_conv3x3_stem_f16_live(void *stream, const void *x64_dev, const void *w_dev, const void *bias_f32_dev, void *y_dev, int64_t n_pixels, int32_t relu,
                              const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    if (!live_rows_dev || g16_bad_part(part, n_parts)) return fail(-1, "ccz_conv3x3_stem_f16_live: null live-row count or bad part / n_parts");
    return conv3x3_launch("ccz_conv3x3_stem_f16_live", stream, x64_dev, w_dev, bias_f32_dev, nullptr, y_dev, n_pixels, relu, 64, live_rows_dev, part | (n_parts << 16));
}

int ccz_pack_live_planes_rows_f16(void *stream, const void *leaf_dev, void *x64_dev, int32_t n_boards, const int32_t *rows_dev, const int32_t *n_rows_dev)
{
    if (!leaf_dev || !x64_dev || n_boards < 0 || !rows_dev || !n_rows_dev) return fail(-1, "ccz_pack_live_planes_rows_f16: bad arguments");
    if ((uintptr_t)x64_dev & 15) return fail(-1, "ccz_pack_live_planes_rows_f16: output must be 16-byte aligned");
    if (n_boards == 0) return 0;
    hipLaunchKernelGGL(k_pack_live_planes, dim3((unsigned)n_boards), dim3(kPackThreads), 0, (hipStream_t)stream, (const _Float16 *)leaf_dev, (half8_t *)x64_dev, (int)n_boards,
                       (const int *)rows_dev, (const int *)n_rows_dev, 2); // planned form: only the chunks that can be non-zero are written
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_pack_conv_weights_g16_f16(void *stream, const void *w_dev, void *wp_dev, int32_t cin)
{
    if (!w_dev || !wp_dev || w_dev == wp_dev || (cin != 64 && cin != 128 && cin != 256)) return fail(-1, "ccz_pack_conv_weights_g16_f16: bad arguments (cin must be 64, 128 or 256, not in place)");
    if ((((uintptr_t)w_dev) | ((uintptr_t)wp_dev)) & 15) return fail(-1, "ccz_pack_conv_weights_g16_f16: pointers must be 16-byte aligned");
    const int n = 256 * 9 * (cin >> 3);
    hipLaunchKernelGGL(k_pack_conv_weights_g16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const cv_half8 *)w_dev, (cv_half8 *)wp_dev, (int)cin);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_pack_live_planes_g16_f16(void *stream, const void *leaf_dev, void *x64_dev, int32_t n_boards, const int32_t *rows_dev, const int32_t *n_rows_dev)
{
    if (!leaf_dev || !x64_dev || n_boards < 0 || (!rows_dev) != (!n_rows_dev)) return fail(-1, "ccz_pack_live_planes_g16_f16: bad arguments");
    if ((uintptr_t)x64_dev & 15) return fail(-1, "ccz_pack_live_planes_g16_f16: output must be 16-byte aligned");
    if (n_boards == 0) return 0;
    hipLaunchKernelGGL(k_pack_live_planes, dim3((unsigned)n_boards), dim3(kPackThreads), 0, (hipStream_t)stream, (const _Float16 *)leaf_dev, (half8_t *)x64_dev, (int)n_boards,
                       (const int *)rows_dev, (const int *)n_rows_dev, rows_dev ? 3 : 1); // planned form: as ccz_pack_live_planes_rows_f16
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the 128-channel stem of the leaf history planes (cczero.h "leaf history planes"): the general tile forms at cin = 128
static int pack_planes128(const char *who, void *stream, const void *leaf_dev, void *x128_dev, int32_t n_boards, const int32_t *rows_dev, const int32_t *n_rows_dev, int flags)
{
    if (!leaf_dev || !x128_dev || n_boards < 0 || (!rows_dev) != (!n_rows_dev)) return fail(-1, "%s: bad arguments", who);
    if ((uintptr_t)x128_dev & 15) return fail(-1, "%s: output must be 16-byte aligned", who);
    if (n_boards == 0) return 0;
    hipLaunchKernelGGL(k_pack_planes128, dim3((unsigned)n_boards), dim3(kPackThreads), 0, (hipStream_t)stream, (const _Float16 *)leaf_dev, (half8_t *)x128_dev, (int)n_boards,
                       (const int *)rows_dev, (const int *)n_rows_dev, flags);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_pack_planes128_f16(void *stream, const void *leaf_dev, void *x128_dev, int32_t n_boards)
{
    return pack_planes128("ccz_pack_planes128_f16", stream, leaf_dev, x128_dev, n_boards, nullptr, nullptr, 0);
}

int ccz_pack_planes128_g16_f16(void *stream, const void *leaf_dev, void *x128_dev, int32_t n_boards, const int32_t *rows_dev, const int32_t *n_rows_dev)
{
    return pack_planes128("ccz_pack_planes128_g16_f16", stream, leaf_dev, x128_dev, n_boards, rows_dev, n_rows_dev, 1);
}

int ccz_pack_planes128_rows_f16(void *stream, const void *leaf_dev, void *x128_dev, int32_t n_boards, const int32_t *rows_dev, const int32_t *n_rows_dev)
{
    if (!rows_dev || !n_rows_dev) return fail(-1, "ccz_pack_planes128_rows_f16: bad arguments");
    return pack_planes128("ccz_pack_planes128_rows_f16", stream, leaf_dev, x128_dev, n_boards, rows_dev, n_rows_dev, 0);
}

int ccz_conv3x3_stem128_f16(void *stream, const void *x128_dev, const void *w_dev, const void *bias_f32_dev, void *y_dev, int64_t n_pixels, int32_t relu)
{
    if (relu & ~(3 | CCZ_CONV_G16)) return fail(-1, "ccz_conv3x3_stem128_f16: flags are ReLU (1), tile order (2) and CCZ_CONV_G16");
    return conv3x3_launch("ccz_conv3x3_stem128_f16", stream, x128_dev, w_dev, bias_f32_dev, nullptr, y_dev, n_pixels, relu, 128);
}

int ccz_conv3x3_stem128_f16_live(void *stream, const void *x128_dev, const void *w_dev, const void *bias_f32_dev, void *y_dev, int64_t n_pixels, int32_t relu,
                                 const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    if (relu & ~(3 | CCZ_CONV_G16)) return fail(-1, "ccz_conv3x3_stem128_f16_live: flags are ReLU (1), tile order (2) and CCZ_CONV_G16");
    if (!live_rows_dev || g16_bad_part(part, n_parts)) return fail(-1, "ccz_conv3x3_stem128_f16_live: null live-row count or bad part / n_parts");
    return conv3x3_launch("ccz_conv3x3_stem128_f16_live", stream, x128_dev, w_dev, bias_f32_dev, nullptr, y_dev, n_pixels, relu, 128, live_rows_dev, part | (n_parts << 16));
}

int ccz_pack_live_planes_f16(void *stream, const void *leaf_dev, void *x64_dev, int32_t n_boards)
{
    if (!leaf_dev || !x64_dev || n_boards < 0) return fail(-1, "ccz_pack_live_planes_f16: bad arguments");
    if ((uintptr_t)x64_dev & 15) return fail(-1, "ccz_pack_live_planes_f16: output must be 16-byte aligned");
    if (n_boards == 0) return 0;
    hipLaunchKernelGGL(k_pack_live_planes, dim3((unsigned)n_boards), dim3(kPackThreads), 0, (hipStream_t)stream, (const _Float16 *)leaf_dev, (half8_t *)x64_dev, (int)n_boards,
                       (const int *)nullptr, (const int *)nullptr, 0);
    HIP_TRY(hipGetLastError());
    return 0;
}

#ifdef CCZ_STAMPS
// diagnostic build only: cycle stamps of the last ccz_conv3x3_c256_f16 launch (uint64 [2048][2][16])
int ccz_debug_conv_stamps(unsigned long long *out_host)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_cv_stamps), sizeof(unsigned long long) * 2048 * 2 * 16));
    return 0;
}
// diagnostic build only: wait / barrier cycle sums of the last launch with quad tiles (uint64 [4096][8][8], cczero_conv_g16.h g_g5q_stamps)
int ccz_debug_g5q_stamps(unsigned long long *out_host, int clear)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_g5q_stamps), sizeof(unsigned long long) * 4096 * 8 * 8));
    if (clear) {
        void *p = nullptr;
        HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(g_g5q_stamps)));
        HIP_TRY(hipMemset(p, 0, sizeof(unsigned long long) * 4096 * 8 * 8));
    }
    return 0;
}
// diagnostic build only: per-board s_memtime stamps of the last k_step launch (uint64 [B*16])
int ccz_debug_stamps(ccz_engine *e, void *stream, unsigned long long *out_host)
{
    NEED(e);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(out_host, e->d.stamps, (size_t)e->d.B * 16 * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
#endif

int ccz_heads_conv1x1_f16(void *stream, const void *x_dev, const void *w32_dev, const void *bias32_f32_dev, void *pol_dev, void *val_dev,
                          int32_t n_boards, int32_t flags, const int32_t *live_boards_dev)
{
    if (!x_dev || !w32_dev || !bias32_f32_dev || !pol_dev || !val_dev || n_boards < 0) return fail(-1, "ccz_heads_conv1x1_f16: bad arguments");
    if ((((uintptr_t)x_dev) | ((uintptr_t)w32_dev) | ((uintptr_t)bias32_f32_dev)) & 15) return fail(-1, "ccz_heads_conv1x1_f16: x, weights and bias must be 16-byte aligned");
    if (flags & ~CCZ_CONV_G16) return fail(-1, "ccz_heads_conv1x1_f16: unknown flags 0x%x", flags);
    const bool g16 = (flags & CCZ_CONV_G16) != 0;
    if (g16 && (n_boards & 15)) return fail(-1, "ccz_heads_conv1x1_f16: the group-of-16 layout holds whole groups of 16 boards (n_boards = %d)", n_boards);
    if (n_boards == 0) return 0;
    const long cells = ((long)n_boards * 90 + 15) / 16;
    const unsigned blocks = (unsigned)((cells + 3) / 4 < 768 ? (cells + 3) / 4 : 768); // 768 x 4 waves = 3 per SIMD on 256 CUs: all resident, one round
    if (g16)
        hipLaunchKernelGGL(k_head_conv1x1<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const _Float16 *)x_dev, (const _Float16 *)w32_dev,
                           (const float *)bias32_f32_dev, (_Float16 *)pol_dev, (_Float16 *)val_dev, (int)n_boards, (const int *)live_boards_dev);
    else
        hipLaunchKernelGGL(k_head_conv1x1<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const _Float16 *)x_dev, (const _Float16 *)w32_dev,
                           (const float *)bias32_f32_dev, (_Float16 *)pol_dev, (_Float16 *)val_dev, (int)n_boards, (const int *)live_boards_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- narrow towers (64 / 128 channels, board-major rows; cczero_conv_narrow.h): additive to ABI 9 ----
static int conv3x3_cn_launch(const char *who, void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev, void *y_dev,
                             int64_t n_pixels, int32_t relu, int32_t cin, int32_t cout, const int32_t *live_rows_dev, int32_t row0)
{
    if ((cin != 64 && cin != 128) || (cout != 64 && cout != 128))
        return fail(-1, "%s: unsupported shape %d -> %d channels (cin and cout must be 64 or 128; 256-wide towers: ccz_conv3x3_c256_f16)", who, cin, cout);
    if (!x_dev || !w_dev || !bias_f32_dev || !y_dev || n_pixels < 0 || n_pixels > (int64_t)INT32_MAX / 256)
        return fail(-1, "%s: bad arguments (null pointer, or n_pixels outside 0 .. 2^31 / 256)", who);
    if ((((uintptr_t)x_dev) | ((uintptr_t)w_dev) | ((uintptr_t)bias_f32_dev) | ((uintptr_t)residual_dev) | ((uintptr_t)y_dev)) & 15)
        return fail(-1, "%s: pointers must be 16-byte aligned", who);
    if (x_dev == y_dev) return fail(-1, "%s: the output may alias the residual but not the input", who);
    if (relu & ~(CCZ_CONV_RELU | CCZ_CONV_DESCENDING | CCZ_CONV_FORCE_SMALL | CCZ_CONV_FORCE_TILE))
        return fail(-1, "%s: flags are ReLU, tile order and the two force bits (board-major rows only)", who);
    const bool whole = n_pixels % 90 == 0;
    if (live_rows_dev && !whole) return fail(-1, "%s: the live form takes whole boards (n_pixels = boards * 90)", who);
    if ((relu & CCZ_CONV_FORCE_SMALL) && (relu & CCZ_CONV_FORCE_TILE)) return fail(-1, "%s: both force bits set", who);
    if ((relu & CCZ_CONV_FORCE_SMALL) && (live_rows_dev || !whole)) return fail(-1, "%s: the small form takes whole boards and no live count", who);
    if (n_pixels == 0) return 0;
    const bool res = residual_dev != nullptr;
    const bool small = whole && !live_rows_dev && !(relu & CCZ_CONV_FORCE_TILE) && ((relu & CCZ_CONV_FORCE_SMALL) || n_pixels <= kSmallMaxPixels);
#define CCZ_CN_SMALL(RES_, CIN_, COUT_)                                                                                                         \
    hipLaunchKernelGGL((k_conv3x3_small<RES_, CIN_, COUT_>), dim3((unsigned)((n_pixels + kSmPix - 1) / kSmPix), COUT_ / 16), dim3(256), 0, (hipStream_t)stream, \
                       (const _Float16 *)x_dev, (const _Float16 *)w_dev, (const float *)bias_f32_dev, (const _Float16 *)residual_dev, (_Float16 *)y_dev, \
                       (int)n_pixels, (int)(relu & 1))
#define CCZ_CN_TILE(RES_, CIN_, COUT_)                                                                                                          \
    hipLaunchKernelGGL((k_conv3x3_narrow<RES_, CIN_, COUT_>), dim3((unsigned)((n_pixels + kNwBM - 1) / kNwBM)), dim3(512), 0, (hipStream_t)stream, \
                       (const _Float16 *)x_dev, (const _Float16 *)w_dev, (const float *)bias_f32_dev, (const _Float16 *)residual_dev, (_Float16 *)y_dev, \
                       (int)n_pixels, (int)(relu & 3), (const int *)live_rows_dev, (int)row0)
#define CCZ_CN_FORM(RES_, CIN_, COUT_) do { if (small) CCZ_CN_SMALL(RES_, CIN_, COUT_); else CCZ_CN_TILE(RES_, CIN_, COUT_); } while (0)
#define CCZ_CN_RES(CIN_, COUT_) do { if (res) CCZ_CN_FORM(true, CIN_, COUT_); else CCZ_CN_FORM(false, CIN_, COUT_); } while (0)
    if (cin == 64 && cout == 64) CCZ_CN_RES(64, 64);
    else if (cin == 64) CCZ_CN_RES(64, 128);
    else if (cout == 64) CCZ_CN_RES(128, 64);
    else CCZ_CN_RES(128, 128);
#undef CCZ_CN_RES
#undef CCZ_CN_FORM
#undef CCZ_CN_TILE
#undef CCZ_CN_SMALL
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_conv3x3_cn_f16(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev, void *y_dev,
                       int64_t n_pixels, int32_t relu, int32_t cin, int32_t cout)
{
    return conv3x3_cn_launch("ccz_conv3x3_cn_f16", stream, x_dev, w_dev, bias_f32_dev, residual_dev, y_dev, n_pixels, relu, cin, cout, nullptr, 0);
}

int ccz_conv3x3_cn_f16_live(void *stream, const void *x_dev, const void *w_dev, const void *bias_f32_dev, const void *residual_dev, void *y_dev,
                            int64_t n_pixels, int32_t relu, int32_t cin, int32_t cout, const int32_t *live_rows_dev, int32_t part, int32_t n_parts)
{
    if (!live_rows_dev || g16_bad_part(part, n_parts)) return fail(-1, "ccz_conv3x3_cn_f16_live: null live-row count or bad part / n_parts");
    return conv3x3_cn_launch("ccz_conv3x3_cn_f16_live", stream, x_dev, w_dev, bias_f32_dev, residual_dev, y_dev, n_pixels, relu, cin, cout, live_rows_dev,
                             part | (n_parts << 16));
}

int ccz_heads_conv1x1_cn_f16(void *stream, const void *x_dev, const void *w32_dev, const void *bias32_f32_dev, void *pol_dev, void *val_dev,
                             int32_t n_boards, int32_t c_in, const int32_t *live_boards_dev)
{
    if (c_in != 64 && c_in != 128) return fail(-1, "ccz_heads_conv1x1_cn_f16: unsupported width %d (64 or 128; 256: ccz_heads_conv1x1_f16)", c_in);
    if (!x_dev || !w32_dev || !bias32_f32_dev || !pol_dev || !val_dev || n_boards < 0) return fail(-1, "ccz_heads_conv1x1_cn_f16: bad arguments");
    if ((((uintptr_t)x_dev) | ((uintptr_t)w32_dev) | ((uintptr_t)bias32_f32_dev)) & 15) return fail(-1, "ccz_heads_conv1x1_cn_f16: x, weights and bias must be 16-byte aligned");
    if ((((uintptr_t)pol_dev) | ((uintptr_t)val_dev)) & 1) return fail(-1, "ccz_heads_conv1x1_cn_f16: outputs must be 2-byte aligned");
    if (n_boards == 0) return 0;
    const long cells = ((long)n_boards * 90 + 15) / 16;
    const unsigned blocks = (unsigned)((cells + 3) / 4 < 768 ? (cells + 3) / 4 : 768); // as ccz_heads_conv1x1_f16
    if (c_in == 64)
        hipLaunchKernelGGL((k_head_conv1x1<false, 64>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const _Float16 *)x_dev, (const _Float16 *)w32_dev,
                           (const float *)bias32_f32_dev, (_Float16 *)pol_dev, (_Float16 *)val_dev, (int)n_boards, (const int *)live_boards_dev);
    else
        hipLaunchKernelGGL((k_head_conv1x1<false, 128>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const _Float16 *)x_dev, (const _Float16 *)w32_dev,
                           (const float *)bias32_f32_dev, (_Float16 *)pol_dev, (_Float16 *)val_dev, (int)n_boards, (const int *)live_boards_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_fc_f16(void *stream, const void *a_dev, int32_t lda, const void *w_dev, const void *bias_f32_dev, void *c_dev, int32_t ldc,
               int32_t m, int32_t n, int32_t k, int32_t relu, const int32_t *live_rows_dev)
{
    if (!a_dev || !w_dev || !bias_f32_dev || !c_dev || m < 0 || n <= 0 || k <= 0) return fail(-1, "ccz_fc_f16: bad arguments");
    if ((k & 63) || (lda & 7) || lda < k || (n & 1) || (ldc & 1) || ldc < n) return fail(-1, "ccz_fc_f16: k must be a multiple of 64, lda a multiple of 8 and >= k, n and ldc even, ldc >= n");
    if ((((uintptr_t)a_dev) | ((uintptr_t)w_dev) | ((uintptr_t)bias_f32_dev)) & 15 || ((uintptr_t)c_dev & 3)) return fail(-1, "ccz_fc_f16: a, w, bias must be 16-byte aligned, c 4-byte aligned");
    if (m == 0) return 0;
    // many rows x thousands of columns (the policy layer of a big batch): the 256 x 144 tile kernel; relu bit 1 forces the 128 x 128 kernel,
    // bit 2 the wide one (tests, A/B) -- same bits from either
    // (policy shape on one box, us: M 4096: 31.8 against 53.4; 3712: 31.6 / 41.5; 2048: 27.1 / 29.3; 1024: 25.9 / 22.1 -- profiles/r04_fc_microbench_wide.json)
    if (!(relu & 2) && ((relu & 4) || (m >= 2048 && n >= 1024))) {
        const int wtiles = ((n + kFwBN - 1) / kFwBN) * ((m + kFwBM - 1) / kFwBM);
        const dim3 wgrid((unsigned)(8 * ((wtiles + 7) / 8)));
        if (relu & 1)
            hipLaunchKernelGGL(k_fc_wide_f16<true>, wgrid, dim3(512), 0, (hipStream_t)stream, (const _Float16 *)a_dev, (int)lda, (const _Float16 *)w_dev,
                               (const float *)bias_f32_dev, (_Float16 *)c_dev, (int)ldc, (int)m, (int)n, (int)k, (const int *)live_rows_dev, (int)(relu >> 8));
        else
            hipLaunchKernelGGL(k_fc_wide_f16<false>, wgrid, dim3(512), 0, (hipStream_t)stream, (const _Float16 *)a_dev, (int)lda, (const _Float16 *)w_dev,
                               (const float *)bias_f32_dev, (_Float16 *)c_dev, (int)ldc, (int)m, (int)n, (int)k, (const int *)live_rows_dev, (int)(relu >> 8));
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // a handful of rows (one game at a time: 1 + 10 scout rows): one wave per 16 columns, operands straight from memory -- same bits
    if (m <= 16 && !(relu & 6)) {
        const dim3 sgrid((unsigned)((n + 15) / 16));
        if (relu & 1)
            hipLaunchKernelGGL(k_fc_skinny_f16<true>, sgrid, dim3(64), 0, (hipStream_t)stream, (const _Float16 *)a_dev, (int)lda, (const _Float16 *)w_dev,
                               (const float *)bias_f32_dev, (_Float16 *)c_dev, (int)ldc, (int)m, (int)n, (int)k, (const int *)live_rows_dev);
        else
            hipLaunchKernelGGL(k_fc_skinny_f16<false>, sgrid, dim3(64), 0, (hipStream_t)stream, (const _Float16 *)a_dev, (int)lda, (const _Float16 *)w_dev,
                               (const float *)bias_f32_dev, (_Float16 *)c_dev, (int)ldc, (int)m, (int)n, (int)k, (const int *)live_rows_dev);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const int tiles = ((n + kFcBN - 1) / kFcBN) * ((m + kFcBM - 1) / kFcBM);
    const dim3 grid((unsigned)(8 * ((tiles + 7) / 8))); // XCD x = block mod 8 takes the x-th contiguous eighth of the tile order: see k_fc_f16
    if (relu & 1)
        hipLaunchKernelGGL(k_fc_f16<true>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16 *)a_dev, (int)lda, (const _Float16 *)w_dev,
                           (const float *)bias_f32_dev, (_Float16 *)c_dev, (int)ldc, (int)m, (int)n, (int)k, (const int *)live_rows_dev, (int)(relu >> 8));
    else
        hipLaunchKernelGGL(k_fc_f16<false>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16 *)a_dev, (int)lda, (const _Float16 *)w_dev,
                           (const float *)bias_f32_dev, (_Float16 *)c_dev, (int)ldc, (int)m, (int)n, (int)k, (const int *)live_rows_dev, (int)(relu >> 8));
    HIP_TRY(hipGetLastError());
    return 0;
}

int ccz_value_out_f32(void *stream, const void *h_dev, const void *w2_dev, float b2, float *v_dev, int32_t m, const int32_t *live_rows_dev)
{
    if (!h_dev || !w2_dev || !v_dev || m < 0) return fail(-1, "ccz_value_out_f32: bad arguments");
    if ((((uintptr_t)h_dev) | ((uintptr_t)w2_dev)) & 7) return fail(-1, "ccz_value_out_f32: h and w2 must be 8-byte aligned");
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_value_out, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const _Float16 *)h_dev, (const _Float16 *)w2_dev, b2, v_dev,
                       (int)m, (const int *)live_rows_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // extern "C"
