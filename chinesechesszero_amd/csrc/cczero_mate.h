// cczero_mate.h -- ccz_mate_search: forced mates by consecutive checks, one wave per board.
//
// The definition (include/cczero.h "Mate search"; tests/mate_model.py restates it sequentially). S, the side to
// move at a board's root, is the attacker. Iterative deepening n = 1, 3, ..., max_plies, depth-first:
//   attacker node, r plies left (r odd): the legal moves in `legal_moves` order; a move after which the enemy king is not attacked
//     is skipped, the others lead to a defender node with r - 1 left; the first child that succeeds makes the node succeed.
//   defender node: no legal move -> mate, it succeeds (also at clock 120: the sixty-move rule needs a legal move). Otherwise it
//     FAILS if it is blocked, or if r - 1 == 0; else every reply, in order, must lead to an attacker node (r - 2 left) that succeeds.
//   an attacker node below the root is tested for blocked before it generates (a blocked one is no node: nothing is generated).
//   blocked: the position's key equals an earlier key of the DFS path or of the board's history chain; or the clock (kept as
//     push_root_move keeps it) has reached 120; or the material is insufficient.
// A node is a position whose legal moves are generated; nodes are counted over the whole call, every iteration's root included, and the
// search stops the moment the count reaches the budget (state 3, nodes == budget).
//
// The kernel reads engine state and writes its four output arrays, nothing else. Everything indexed by depth lives in LDS (no private
// array is indexed dynamically); the control flow is wave-uniform: one while loop over an explicit stack, gen_legal called by all 64
// lanes, the check test of move j on lane j in two passes of 64, the next checking move from the ballot's bits.
#pragma once
#include "cczero_kernels.h"

namespace ccz {

constexpr int kMatePlies = CCZ_MATE_MAX_PLIES;  // deepest iteration; depths 0 .. kMatePlies are positions on the stack
constexpr int kMateFrames = kMatePlies + 1;

struct MateFrame {
    uint16_t ids[kMaxLegal]; // the node's legal moves in `legal_moves` order
    uint64_t todo[2];        // attacker: the checking moves not yet tried (bit j of word j / 64); defender: unused
    int32_t n;               // number of legal moves (<= kMaxLegal)
    int32_t it;              // defender: the next reply; attacker: the move tried last
    int32_t halfmove;        // the clock of this position
    uint8_t from, to, cap, pad; // the move made from this node: undo data (the clock before it is `halfmove`)
};

struct MateShared {
    __align__(16) uint8_t sq[96];
    GenScratch S;
    uint64_t chain[kChainCap];
    uint64_t key[kMateFrames]; // key[d]: the position at depth d (key[0]: the root)
    MateFrame f[kMateFrames];
};

// no rook, cannon, knight or pawn of either colour is left (gen_legal's test, without a generation)
__device__ __forceinline__ bool mate_insufficient(const uint8_t *sq, int lane)
{
    const int p0 = sq[lane], p1 = lane < 26 ? sq[64 + lane] : 0;
    const int t0 = p0 & 7, t1 = p1 & 7;
    const bool a0 = p0 != 0 && t0 >= PAWN && t0 <= KNIGHT, a1 = p1 != 0 && t1 >= PAWN && t1 <= KNIGHT;
    return (__ballot(a0) | __ballot(a1)) == 0ull;
}

// the key of depth d equals one of the path above it or of the history chain
__device__ __forceinline__ bool mate_repeated(const MateShared &sh, int d, int chain_len, int lane)
{
    const uint64_t k = sh.key[d];
    bool hit = lane < d && sh.key[lane] == k; // (d <= kMatePlies < 64)
    hit |= lane < chain_len && sh.chain[lane] == k;
    hit |= 64 + lane < chain_len && sh.chain[64 + lane] == k;
    return __ballot(hit) != 0ull;
}

__global__ __launch_bounds__(64) void k_mate_search(Dev D, int active, int max_plies, int budget, int32_t *state_out, int32_t *dist_out,
                                                      int32_t *move_out, int32_t *nodes_out)
{
    __shared__ MateShared sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    const BoardMeta m = D.meta[b];
    const int chain_len = __builtin_amdgcn_readfirstlane(m.chain_len);
    int state = 0, dist = 0, move = -1, nodes = 0;
    // not searched: a finished or parked board, a slot past the active boards, a history chain that is full (the next push would
    // overflow it: what leaf_tail flags) or out of range
    const bool live = b < active && !m.over && chain_len >= 1 && chain_len < kChainCap;
    if (live) {
        load_board(sh.sq, D.root_sq + (size_t)b * 96, lane);
        const uint64_t *ch = D.chain + (size_t)b * kChainCap;
        for (int i = lane; i < chain_len; i += 64) sh.chain[i] = ch[i];
        if (lane == 0) { sh.key[0] = m.key; sh.f[0].halfmove = m.halfmove; }
        wave_sync();
        const int root_turn = m.turn ? 1 : 0;
        const bool pawn_zeroes = (D.rule_flags & 2u) != 0;
        state = 2;
        for (int n = 1; n <= max_plies && state == 2; n += 2) {
            int d = 0;            // the position on sh.sq is the one at depth d
            int mode = 0;         // 0 enter the node at d, 1 take its next move, 2 return `ok` from it
            bool ok = false;
            while (true) {
                MateFrame &F = sh.f[d];
                const int turn = root_turn ^ (d & 1);
                if (mode == 0) {
                    if (d > 0 && !(d & 1)) { // an attacker node below the root: blocked -> it fails, and is no node
                        const int hm = __builtin_amdgcn_readfirstlane(F.halfmove);
                        if (hm >= 120 || mate_insufficient(sh.sq, lane) || mate_repeated(sh, d, chain_len, lane)) { ok = false; mode = 2; continue; }
                    }
                    if (++nodes >= budget) { state = 3; break; }
                    const GenResult g = gen_legal(sh.sq, turn, sh.S, F.ids, lane, nullptr, D.rank, D.unrank, D.trankpack);
                    const int nl = g.n_legal < kMaxLegal ? g.n_legal : kMaxLegal;
                    wave_sync();
                    if (d & 1) {
                        if (nl == 0) { ok = true; mode = 2; continue; } // mate: the move that led here gave check
                        const int hm = __builtin_amdgcn_readfirstlane(F.halfmove);
                        if (hm >= 120 || g.insufficient || mate_repeated(sh, d, chain_len, lane) || n - d == 0) { ok = false; mode = 2; continue; }
                        if (lane == 0) { F.n = nl; F.it = 0; }
                    } else {
                        // which moves give check: move j on lane j, two passes. The enemy king's square from a ballot
                        const int ek = turn ? KING + 8 : KING;
                        const uint64_t k0 = __ballot(sh.sq[lane] == ek), k1 = __ballot(lane < 26 && sh.sq[64 + lane] == ek);
                        const int eksq = k0 ? (__ffsll((long long)k0) - 1) : (k1 ? 64 + (__ffsll((long long)k1) - 1) : -1);
                        uint64_t w[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int j = 64 * h + lane;
                            bool chk = false;
                            if (j < nl && eksq >= 0) {
                                int id = F.ids[j];
                                if (id >= kNMoves) id = 0;
                                const int fr = c_tab.from[id], to = c_tab.to[id];
                                chk = to != eksq && king_attacked(sh.sq, sh.S, eksq, fr, to, sh.sq[fr], turn ^ 1);
                            }
                            w[h] = __ballot(chk);
                        }
                        if (lane == 0) { F.n = nl; F.todo[0] = w[0]; F.todo[1] = w[1]; }
                    }
                    wave_sync();
                    mode = 1;
                    continue;
                }
                if (mode == 1) {
                    int j;
                    if (d & 1) {
                        j = __builtin_amdgcn_readfirstlane(F.it);
                        if (j >= __builtin_amdgcn_readfirstlane(F.n)) { ok = true; mode = 2; continue; } // every reply is answered
                    } else {
                        const uint64_t w0 = wave_readlane64(F.todo[0], 0), w1 = wave_readlane64(F.todo[1], 0);
                        if (!(w0 | w1)) { ok = false; mode = 2; continue; } // no checking move is left
                        j = w0 ? __ffsll((long long)w0) - 1 : 64 + __ffsll((long long)w1) - 1;
                    }
                    // make move j: squares by lane 0, the key and the clock of depth d + 1 (push_root_move's rules)
                    int id = sh.f[d].ids[j & (kMaxLegal - 1)];
                    id = __builtin_amdgcn_readfirstlane(id);
                    if (id >= kNMoves) id = 0;
                    const int fr = c_tab.from[id], to = c_tab.to[id];
                    const int pc = __builtin_amdgcn_readfirstlane((int)sh.sq[fr]), cap = __builtin_amdgcn_readfirstlane((int)sh.sq[to]);
                    const int hm = __builtin_amdgcn_readfirstlane(F.halfmove);
                    uint64_t key = sh.key[d] ^ zob(pc, fr) ^ zob(pc, to) ^ kTurnKey;
                    if (cap) key ^= zob(cap, to);
                    const bool zeroing = cap || (pawn_zeroes && (pc & 7) == PAWN);
                    wave_sync();
                    if (lane == 0) {
                        if (d & 1) F.it = j + 1;
                        else { F.it = j; if (j < 64) F.todo[0] &= ~(1ull << j); else F.todo[1] &= ~(1ull << (j - 64)); }
                        F.from = (uint8_t)fr; F.to = (uint8_t)to; F.cap = (uint8_t)cap;
                        sh.sq[to] = (uint8_t)pc;
                        sh.sq[fr] = 0;
                        sh.key[d + 1] = key;
                        sh.f[d + 1].halfmove = zeroing ? 0 : hm + 1;
                    }
                    wave_sync();
                    ++d; // (d + 1 <= kMatePlies: a defender at depth n fails before it takes a move, and n <= kMatePlies)
                    mode = 0;
                    continue;
                }
                // mode 2: the node at depth d returns `ok`
                if (d == 0) break;
                --d;
                {
                    MateFrame &P = sh.f[d];
                    wave_sync();
                    if (lane == 0) { sh.sq[P.from] = sh.sq[P.to]; sh.sq[P.to] = P.cap; }
                    wave_sync();
                }
                if (d & 1) { if (!ok) { mode = 2; continue; } mode = 1; }  // defender: the first failing reply fails it
                else { if (ok) { mode = 2; continue; } mode = 1; }         // attacker: the first succeeding move succeeds
            }
            if (state == 3) break;
            if (ok) {
                state = 1;
                dist = n;
                const int j = __builtin_amdgcn_readfirstlane(sh.f[0].it);
                move = __builtin_amdgcn_readfirstlane((int)sh.f[0].ids[j & (kMaxLegal - 1)]);
            }
        }
    }
    if (lane == 0) { state_out[b] = state; dist_out[b] = dist; move_out[b] = move; nodes_out[b] = nodes; }
}

} // namespace ccz
