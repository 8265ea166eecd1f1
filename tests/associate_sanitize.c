/* associate_sanitize.c -- a stand-alone driver over tests/associate_ref.c for AddressSanitizer and UBSan: seeded neighbour
 * lists and point sets, every array in a heap block of exactly its size (a read or write outside it is an error), over-long
 * lists, indices out of range, NaN and infinite scores and coordinates, empty inputs.
 * Build: gcc -std=c99 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all associate_sanitize.c associate_ref.c -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int assoc_ref_match(int32_t n, int32_t m, int32_t cap, const int32_t *count, const int32_t *nbr_idx, const float *nbr_dist,
                    const float *nbr_ncc, int32_t use_ncc, float th_high, float th_low, float th_ratio,
                    const float *keys_cur_un, const float *pt_predict_un, int32_t *match_query, int32_t *match_train,
                    float *match_dist, float *match_ncc, float *flows_err, int32_t *info);
int assoc_ref_klt(int32_t cap, int32_t n, int32_t m, const uint8_t *status, const float *pt_lk, const float *pt_ref,
                  const float *keys_cur, float max_distance, double ratio, double factor, int32_t *match_query,
                  int32_t *match_train, float *match_dist, double *disparity, double *stats, int32_t *info);

static uint32_t lcg(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }
static float unit(uint32_t *s) { return (float)(lcg(s) >> 8) / 16777216.0f; }
static float odd(uint32_t *s, float v) { const uint32_t r = lcg(s) >> 27; return r == 0 ? NAN : r == 1 ? INFINITY : r == 2 ? -INFINITY : v; }

static int run_match(int n, int m, int cap, int use_ncc, uint32_t seed)
{
    const size_t nn = (size_t)(n ? n : 1), mm = (size_t)(m ? m : 1), lc = nn * (size_t)cap;
    int32_t *count = malloc(nn * 4), *idx = malloc(lc * 4), *q = malloc(nn * 4), *t = malloc(nn * 4), info[8];
    float *dist = malloc(lc * 4), *ncc = malloc(lc * 4), *md = malloc(nn * 4), *mc = malloc(nn * 4);
    float *cur = malloc(mm * 8), *pred = malloc(nn * 8), *flows = malloc(nn * 8);
    int k, again;
    if (!count || !idx || !q || !t || !dist || !ncc || !md || !mc || !cur || !pred || !flows) return 1;
    for (int i = 0; i < n; i++) {
        count[i] = (int32_t)(lcg(&seed) >> 16) % (cap + 3) - 1;              /* -1 .. cap + 1: negative and over-long too */
        pred[2 * i] = odd(&seed, 100 * unit(&seed)), pred[2 * i + 1] = 100 * unit(&seed);
        for (int c = 0; c < cap; c++) {
            idx[i * cap + c] = (int32_t)(lcg(&seed) >> 16) % (m + 2) - 1;    /* -1 .. m: out of range at both ends */
            dist[i * cap + c] = odd(&seed, 20 * unit(&seed));
            ncc[i * cap + c] = odd(&seed, unit(&seed));
        }
    }
    for (int j = 0; j < m; j++) cur[2 * j] = 100 * unit(&seed), cur[2 * j + 1] = odd(&seed, 100 * unit(&seed));
    k = assoc_ref_match(n, m, cap, count, idx, dist, ncc, use_ncc, 0.6f, 0.3f, 0.75f, cur, pred, q, t, md, mc, flows, info);
    again = assoc_ref_match(n, m, cap, count, idx, dist, ncc, use_ncc, 0.6f, 0.3f, 0.75f, NULL, NULL, q, t, NULL, NULL, NULL, info);
    printf("match n %d m %d cap %d mode %d: %d matches, info %d %d %d %d %d\n", n, m, cap, use_ncc, k, info[0], info[1], info[2],
           info[3], info[4]);
    free(count), free(idx), free(q), free(t), free(dist), free(ncc), free(md), free(mc), free(cur), free(pred), free(flows);
    return k < 0 || k != again || k != info[4];
}

static int run_klt(int cap, int n, int m, uint32_t seed)
{
    const size_t cc = (size_t)(cap ? cap : 1), mm = (size_t)(m ? m : 1);
    uint8_t *status = malloc(cc);
    float *lk = malloc(cc * 8), *ref = malloc(cc * 8), *cur = malloc(mm * 8), *md = malloc(cc * 4);
    int32_t *q = malloc(cc * 4), *t = malloc(cc * 4), info[8];
    double *disp = malloc(cc * 8), stats[8];
    int k;
    if (!status || !lk || !ref || !cur || !md || !q || !t || !disp) return 1;
    for (int i = 0; i < cap; i++) {
        status[i] = (uint8_t)((lcg(&seed) >> 20) % 4 != 0);
        lk[2 * i] = odd(&seed, (float)((lcg(&seed) >> 16) % 40) * 0.5f), lk[2 * i + 1] = (float)((lcg(&seed) >> 16) % 40) * 0.5f;
        ref[2 * i] = lk[2 * i] - 1.5f, ref[2 * i + 1] = odd(&seed, lk[2 * i + 1] + 0.75f);
    }
    for (int j = 0; j < m; j++)   /* a coarse grid: equal distances, distance 0 and crowded keypoints are common */
        cur[2 * j] = (float)((lcg(&seed) >> 16) % 40) * 0.5f, cur[2 * j + 1] = odd(&seed, (float)((lcg(&seed) >> 16) % 40) * 0.5f);
    k = assoc_ref_klt(cap, n, m, status, lk, ref, cur, 4.0f, 0.7, 1.5, q, t, md, disp, stats, info);
    printf("klt cap %d n %d m %d: %d matches, info %d %d %d %d %d %d %d %d\n", cap, n, m, k, info[0], info[1], info[2], info[3],
           info[4], info[5], info[6], info[7]);
    k = k < 0 || k != info[7] || assoc_ref_klt(cap, n, m, status, lk, ref, cur, 4.0f, 0.7, 1.5, q, t, NULL, disp, NULL, info) != info[7];
    free(status), free(lk), free(ref), free(cur), free(md), free(q), free(t), free(disp);
    return k;
}

int main(void)
{
    int bad = 0, runs = 0;
    for (int mode = 0; mode < 2; mode++) {
        bad |= run_match(0, 0, 1, mode, 1u), runs++;
        bad |= run_match(1, 1, 1, mode, 2u), runs++;
        bad |= run_match(300, 3, 2, mode, 3u), runs++;
        bad |= run_match(257, 17, 8, mode, 4u), runs++;
    }
    bad |= run_klt(1, 0, 0, 5u), runs++;
    bad |= run_klt(64, 64, 0, 6u), runs++;
    bad |= run_klt(200, 150, 90, 7u), runs++;
    bad |= run_klt(130, 400, 700, 8u), runs++;
    printf("%d runs\n", runs);
    return bad;
}
