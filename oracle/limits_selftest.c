/*
 * limits_selftest.c -- CPU ORACLE (test infrastructure, NOT the product): a stand-alone program that walks the host twins of
 * ccz_ref.c into every limit they model -- node pool, path capacity, NaN priors, pi arena, ply cap, the move-boundary guards -- and
 * checks the sticky bits and the counts that follow from the rules by hand. `make -C oracle limits_selftest_asan` builds it with
 * the oracle sources under ASan/UBSan (a program of its own: nothing is loaded into an interpreter); tests/test_cpu_engine_limits.py
 * builds and runs it. Exit status 0 and "limits_selftest: ok" = every check held and the sanitizers had nothing to say.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cczero.h"
#include "xq_oracle.h"

typedef struct ccz_ref_engine ccz_ref_engine;
int ccz_ref_create(const ccz_config *cfg, ccz_ref_engine **out);
int ccz_ref_destroy(ccz_ref_engine *e);
int ccz_ref_set_position(ccz_ref_engine *e, void *stream, int32_t board, const uint8_t *sq_host, int32_t turn, int32_t halfmove);
int ccz_ref_reset_tree(ccz_ref_engine *e, void *stream, const uint8_t *mask_host);
int ccz_ref_select_leaves(ccz_ref_engine *e, void *stream, void *leaf_input_f16_host);
int ccz_ref_expand_backup(ccz_ref_engine *e, void *stream, const float *prob_host, const float *value_host);
int ccz_ref_finish_move(ccz_ref_engine *e, void *stream, const int32_t *forced, const double *temps, int32_t *moves_out, int32_t keep_tree);
int ccz_ref_root_children(ccz_ref_engine *e, void *stream, int32_t *k, uint16_t *acts, int32_t *visits, float *q, float *prior, int32_t *root_visits);
int ccz_ref_game_status(ccz_ref_engine *e, void *stream, uint8_t *over, int8_t *winner, int32_t *plies, uint8_t *turn);
int ccz_ref_leaf_info(ccz_ref_engine *e, void *stream, uint8_t *status, int32_t *k, uint16_t *ids, int32_t *depth);
int32_t ccz_ref_error_flags(const ccz_ref_engine *e);
int ccz_ref_usage(const ccz_ref_engine *e, int32_t *n_nodes, int32_t *pi_used, int32_t *board_err, int64_t *counts);

#define B 2
static int failures;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "limits_selftest: line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static float P[B * XQ_NMOVES], V[B];
static uint16_t planes[B * XQ_PLANES];

/* one lockstep simulation. kind 0: uniform priors; 1: all mass but 3 % on one legal move chosen by a hash of the legal-move list (one
   long line); 2: NaN priors */
static void simulate(ccz_ref_engine *e, const int *kind)
{
    uint8_t status[B];
    int32_t k[B], depth[B];
    uint16_t ids[B * XQ_MAX_LEGAL];
    int b, i;
    CHECK(ccz_ref_select_leaves(e, NULL, planes) == 0);
    CHECK(ccz_ref_leaf_info(e, NULL, status, k, ids, depth) == 0);
    memset(P, 0, sizeof P);
    for (b = 0; b < B; b++) {
        uint32_t h = 2166136261u;
        V[b] = 0.0f;
        for (i = 0; i < k[b]; i++) h = (h ^ ids[b * XQ_MAX_LEGAL + i]) * 16777619u;
        h = k[b] ? (h >> 7) % (uint32_t)k[b] : 0u;
        for (i = 0; i < k[b]; i++) {
            const int id = ids[b * XQ_MAX_LEGAL + i];
            P[b * XQ_NMOVES + id] = kind[b] == 2 ? NAN : kind[b] == 1 ? ((uint32_t)i == h ? 0.97f : 0.03f / (float)k[b]) : 1.0f / (float)k[b];
        }
    }
    CHECK(ccz_ref_expand_backup(e, NULL, P, V) == 0);
}

static ccz_ref_engine *create(int max_nodes, int max_depth, int max_plies, int reserve)
{
    ccz_config cfg;
    ccz_ref_engine *e = NULL;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_boards = B; cfg.n_playout = 16; cfg.c_puct = 5.0f; cfg.eps = 0.25f; cfg.alpha = 0.2f; cfg.temp = 1.0f;
    cfg.max_nodes = max_nodes; cfg.max_depth = max_depth; cfg.max_plies = max_plies; cfg.reserve_nodes = reserve; cfg.seed = 9;
    if (ccz_ref_create(&cfg, &e) != 0) return NULL;
    return e;
}

int main(void)
{
    const int uniform[B] = {0, 0}, line[B] = {1, 0}, nans[B] = {2, 0};
    int32_t n_nodes[B], pi_used[B], berr[B], moves[B], k[B], rv[B], visits[B * XQ_MAX_LEGAL], forced[B];
    int64_t counts[3];
    uint8_t over[B];
    ccz_ref_engine *e;
    int i;

    /* create refuses a path capacity outside 64 .. 512 */
    CHECK(create(0, 63, 0, 0) == NULL);
    CHECK(create(0, 513, 0, 0) == NULL);

    /* pool: 200 nodes = the start position's root and three children's expansions (1 + 44 + the three replies' widths); the fifth is refused, its simulation counts */
    e = create(200, 0, 0, 70);
    CHECK(e != NULL);
    if (!e) return 2;
    for (i = 0; i < 20; i++) simulate(e, uniform);
    CHECK(ccz_ref_usage(e, n_nodes, pi_used, berr, counts) == 0);
    {
        /* uniform priors visit the root's children in order: the root and its first three children expand, a fourth does not fit */
        xq_board r, c;
        uint16_t ids[XQ_MAX_LEGAL], cids[XQ_MAX_LEGAL];
        int want = 1, fourth;
        xq_board_init(&r);
        CHECK(xq_legal_ids(&r, ids) == 44);
        want += 44;
        for (i = 0; i < 3; i++) { c = r; xq_push(&c, xq_move_from(ids[i]), xq_move_to(ids[i])); want += xq_legal_ids(&c, cids); }
        c = r; xq_push(&c, xq_move_from(ids[3]), xq_move_to(ids[3])); fourth = xq_legal_ids(&c, cids);
        CHECK(want <= 200 && want + fourth > 200);
        CHECK(n_nodes[0] == want && n_nodes[1] == want && berr[0] == CCZ_ERR_NODE_POOL && counts[0] == 40 && counts[2] == want);
    }
    CHECK(ccz_ref_root_children(e, NULL, k, NULL, visits, NULL, NULL, rv) == 0);
    CHECK(k[0] == 44 && rv[0] == 20 && visits[18] == 1 && visits[19] == 0);
    CHECK(ccz_ref_error_flags(e) == CCZ_ERR_NODE_POOL);
    /* the move boundary: 2086 is no move id, a0a5 (id 4) jumps the pawn on a3; both boards stay where they are with a one-node tree */
    forced[0] = XQ_NMOVES; forced[1] = xq_move_id(0, 45);
    CHECK(ccz_ref_finish_move(e, NULL, forced, NULL, moves, 1) == 0);
    CHECK(ccz_ref_usage(e, n_nodes, pi_used, berr, counts) == 0);
    CHECK(moves[0] == -1 && moves[1] == -1 && n_nodes[0] == 1 && n_nodes[1] == 1 && pi_used[0] == 0 && (berr[1] & CCZ_ERR_BAD_MOVE));
    /* nothing searched, nothing forced */
    CHECK(ccz_ref_finish_move(e, NULL, NULL, NULL, moves, 1) == 0 && moves[0] == -1);
    /* a legal forced move on an unsearched root, and a bad temperature next to it */
    {
        const double temps[B] = {1.0, -1.0};
        forced[0] = 0; forced[1] = 0;
        CHECK(ccz_ref_finish_move(e, NULL, forced, temps, moves, 1) == 0 && moves[0] == 0 && moves[1] == -1);
        CHECK(ccz_ref_error_flags(e) == (CCZ_ERR_NODE_POOL | CCZ_ERR_BAD_MOVE | CCZ_ERR_BAD_TEMP));
    }
    ccz_ref_destroy(e);

    /* depth and NaN: a line dug by one sharp prior reaches 64 path entries; all-NaN priors freeze a board after root + children */
    e = create(0, 64, 0, 0);
    CHECK(e != NULL);
    if (!e) return 2;
    {
        /* kings and five pawns each: pawn pushes are irreversible, so a long line does not die of repetition early */
        static const struct { int sq, pc; } men[] = {{3, 7}, {27, 1}, {29, 1}, {31, 1}, {33, 1}, {35, 1}, {86, 15}, {54, 9}, {56, 9}, {58, 9}, {60, 9}, {62, 9}};
        uint8_t sq[XQ_NSQ] = {0};
        for (i = 0; i < (int)(sizeof men / sizeof men[0]); i++) sq[men[i].sq] = (uint8_t)men[i].pc;
        CHECK(ccz_ref_set_position(e, NULL, 0, sq, 1, 0) == 0);
    }
    for (i = 0; i < 4000 && !(ccz_ref_error_flags(e) & CCZ_ERR_DEPTH); i++) simulate(e, line);
    CHECK(ccz_ref_error_flags(e) == CCZ_ERR_DEPTH);
    CHECK(ccz_ref_usage(e, n_nodes, pi_used, berr, counts) == 0);
    CHECK(berr[0] == CCZ_ERR_DEPTH && berr[1] == 0);
    CHECK(ccz_ref_reset_tree(e, NULL, NULL) == 0);
    for (i = 0; i < 50; i++) simulate(e, nans);
    CHECK(ccz_ref_root_children(e, NULL, k, NULL, visits, NULL, NULL, rv) == 0);
    CHECK(rv[0] == 1 + k[0] && k[0] > 0 && visits[k[0] - 1] == 1 && rv[1] == 50); /* board 0: the root and one visit per child */
    CHECK(ccz_ref_error_flags(e) == (CCZ_ERR_DEPTH | CCZ_ERR_NAN));
    ccz_ref_destroy(e);

    /* the ply cap: with max_plies = 1 the second move adjudicates the game, ply 0 (44 pi entries) stays recorded */
    e = create(0, 0, 1, 0);
    CHECK(e != NULL);
    if (!e) return 2;
    simulate(e, uniform);
    CHECK(ccz_ref_finish_move(e, NULL, NULL, NULL, moves, 1) == 0 && moves[0] >= 0);
    simulate(e, uniform);
    CHECK(ccz_ref_finish_move(e, NULL, NULL, NULL, moves, 1) == 0 && moves[0] == -1);
    CHECK(ccz_ref_game_status(e, NULL, over, NULL, NULL, NULL) == 0 && over[0] == 1 && over[1] == 1);
    CHECK(ccz_ref_usage(e, n_nodes, pi_used, berr, counts) == 0 && pi_used[0] == 44 && counts[1] == 2);
    CHECK(ccz_ref_error_flags(e) == 0); /* at the ply cap the game is adjudicated without a bit (not strict) */
    ccz_ref_destroy(e);

    if (failures) return 1;
    puts("limits_selftest: ok");
    return 0;
}
