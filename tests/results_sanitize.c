/* results_sanitize.c -- a stand-alone program (its own main) for AddressSanitizer and UBSan: pagk_sequence_results_layout over
 * the caps of the tests and the restated id rule (tests/results_ref.c) over the hand-written five-frame example and seeded
 * runs, every array in a heap block of exactly its size.  Linked against the library for the layout function only (which
 * needs no device); nothing here touches a GPU. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pagk.h"

int32_t results_ref_frame(int32_t cap, int32_t n_live, const int32_t *index_in_last, const int64_t *id_last,
                          const int32_t *age_last, int64_t *next_id, int64_t *id, int32_t *age);
void results_ref_run(int32_t nf, int32_t cap, const int32_t *n_live, const int32_t *index_in_last, int64_t *id, int32_t *age,
                     int32_t *n_new, int64_t *next_id);

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                     \
        }                                                                 \
    } while (0)

/* the example of tests/test_sequence_results_cpu.py: cap 6, five frames */
static const int32_t EX_LIVE[5] = {3, 4, 2, 0, 5};
static const int32_t EX_INDEX[5][6] = {
    {-1, -1, -1, -1, -1, -1},   /* the start: three new rows */
    {0, -1, 2, -1, -1, -1},     /* a new row between two survivors, one behind them */
    {-1, -1, -1, -1, -1, -1},   /* no survivor: two new rows */
    {-1, -1, -1, -1, -1, -1},   /* no live row */
    {-1, -1, -1, -1, -1, -1},   /* refilled */
};
static const int64_t EX_ID[5][6] = {
    {0, 1, 2, -1, -1, -1}, {0, 3, 2, 4, -1, -1}, {5, 6, -1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1}, {7, 8, 9, 10, 11, -1}};
static const int32_t EX_AGE[5][6] = {{0, 0, 0, 0, 0, 0}, {1, 0, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
static const int32_t EX_NEW[5] = {3, 2, 2, 0, 5};
static const int64_t EX_NEXT[5] = {3, 5, 7, 7, 12};

static int layouts(void)
{
    static const int32_t caps[] = {1, 4, 12, 33, 40, 70, 2200, PAGK_LK_MAX_ROWS};
    for (size_t c = 0; c < sizeof caps / sizeof caps[0]; c++)
        for (int32_t sensor = 0; sensor < 2; sensor++) {
            pagk_results_layout *l = malloc(sizeof *l);
            CHECK(l && pagk_sequence_results_layout(caps[c], sensor, l) == PAGK_OK);
            const int64_t off[16] = {l->header, l->state, l->info, l->keys, l->keys_un, l->keys_normal, l->index_in_last, l->live,
                                     l->track_id, l->age, l->velocity, l->status, l->pt_predict, l->pt_predict_un, l->err, l->bytes};
            CHECK(off[0] == 0 && l->cap == caps[c] && l->sensor == sensor);
            for (int k = 0; k < 15; k++) CHECK(off[k] % 256 == 0 && off[k + 1] > off[k]);
            CHECK(off[15] % 256 == 0);
            free(l);
        }
    pagk_results_layout l;
    CHECK(pagk_sequence_results_layout(0, 0, &l) == PAGK_E_ARG && pagk_sequence_results_layout(PAGK_LK_MAX_ROWS + 1, 0, &l) == PAGK_E_ARG);
    CHECK(pagk_sequence_results_layout(4, 0, NULL) == PAGK_E_ARG && pagk_sequence_results_layout(-1, 1, &l) == PAGK_E_ARG);
    return 0;
}

static int run(int32_t nf, int32_t cap, const int32_t *live, const int32_t *index, int64_t **id_out, int32_t **age_out,
               int32_t **new_out, int64_t **next_out)
{
    const size_t rows = (size_t)nf * cap;
    int32_t *n_live = malloc(nf * sizeof *n_live), *idx = malloc(rows * sizeof *idx);
    int64_t *id = malloc(rows * sizeof *id), *next = malloc(nf * sizeof *next);
    int32_t *age = malloc(rows * sizeof *age), *n_new = malloc(nf * sizeof *n_new);
    CHECK(n_live && idx && id && next && age && n_new);
    memcpy(n_live, live, nf * sizeof *n_live);
    memcpy(idx, index, rows * sizeof *idx);
    results_ref_run(nf, cap, n_live, idx, id, age, n_new, next);
    free(n_live), free(idx);
    *id_out = id, *age_out = age, *new_out = n_new, *next_out = next;
    return 0;
}

int main(void)
{
    if (layouts()) return 1;
    int64_t *id, *next;
    int32_t *age, *n_new;
    if (run(5, 6, EX_LIVE, &EX_INDEX[0][0], &id, &age, &n_new, &next)) return 1;
    CHECK(memcmp(id, EX_ID, sizeof EX_ID) == 0 && memcmp(age, EX_AGE, sizeof EX_AGE) == 0);
    CHECK(memcmp(n_new, EX_NEW, sizeof EX_NEW) == 0 && memcmp(next, EX_NEXT, sizeof EX_NEXT) == 0);
    free(id), free(age), free(n_new), free(next);
    /* seeded runs: every row of frame 0 is new; later a live row survives (any row of the last frame's live ones) or is new */
    int runs = 1;
    uint64_t s = 0x5EED0A10u;
    static const int32_t caps[] = {1, 4, 33, 70, 2200};
    for (size_t c = 0; c < sizeof caps / sizeof caps[0]; c++, runs++) {
        const int32_t cap = caps[c], nf = 6;
        int32_t *live = malloc(nf * sizeof *live), *idx = malloc((size_t)nf * cap * sizeof *idx);
        CHECK(live && idx);
        for (int32_t f = 0; f < nf; f++) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            live[f] = f == 3 ? 0 : (int32_t)((s >> 33) % (uint64_t)(cap + 1));
            for (int32_t j = 0; j < cap; j++) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const int32_t last = f ? live[f - 1] : 0;
                idx[(size_t)f * cap + j] = (j < live[f] && last > 0 && ((s >> 40) & 3)) ? (int32_t)((s >> 20) % (uint64_t)last) : -1;
            }
        }
        if (run(nf, cap, live, idx, &id, &age, &n_new, &next)) return 1;
        int64_t issued = 0;
        for (int32_t f = 0; f < nf; f++) {
            int32_t fresh = 0;
            for (int32_t j = 0; j < cap; j++) {
                const int64_t v = id[(size_t)f * cap + j];
                CHECK(j < live[f] ? (v >= 0 && v < next[f]) : v == -1);
                fresh += j < live[f] && idx[(size_t)f * cap + j] < 0;
            }
            issued += fresh;
            CHECK(n_new[f] == fresh && next[f] == issued);
        }
        free(live), free(idx), free(id), free(age), free(n_new), free(next);
    }
    printf("%d runs clean\n", runs);
    return 0;
}
