/* lk_sanitize.c -- a stand-alone driver over tests/lk_ref.c for AddressSanitizer and UBSan: seeded image pairs, each in a heap
 * block of exactly its size (a read outside it is an error), features on and beyond every border, a NaN and huge coordinates.
 * Build: gcc -std=c99 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all lk_sanitize.c lk_ref.c -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int lk_ref_track(const uint8_t *ref, const uint8_t *cur, int32_t w, int32_t h, int64_t step_ref, int64_t step_cur,
                 int32_t half_patch, int32_t max_level, int32_t max_count, double epsilon, double min_eig_threshold,
                 float err_threshold, int32_t n, int32_t cap, const float *pt_ref, float *pt_out, uint8_t *status,
                 uint8_t *status_raw, float *err, float *flow, int32_t *info, int32_t *iters, uint8_t *why);

static uint32_t lcg(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }

static int run(int w, int h, int half_patch, int max_level, uint32_t seed)
{
    enum { N = 96 };
    const int win = 2 * half_patch + 1;
    uint8_t *a = (uint8_t *)malloc((size_t)w * h), *b = (uint8_t *)malloc((size_t)w * h);
    float *pts = (float *)malloc(sizeof(float) * 2 * N), *out = (float *)malloc(sizeof(float) * 2 * N);
    float *flow = (float *)malloc(sizeof(float) * 2 * N), *err = (float *)malloc(sizeof(float) * N);
    uint8_t *st = (uint8_t *)malloc(N), *raw = (uint8_t *)malloc(N);
    int32_t info[8], *iters = (int32_t *)malloc(sizeof(int32_t) * N);
    uint8_t *why = (uint8_t *)malloc(8 * N);   /* exactly cap x 8 bytes */
    int left[7] = {0};
    if (!a || !b || !pts || !out || !flow || !err || !st || !raw || !iters || !why) return 1;
    for (int y = 0; y < h; y++)   /* smooth enough to track, one pixel apart */
        for (int x = 0; x < w; x++) {
            a[y * w + x] = (uint8_t)(128 + 60 * sin(0.35 * x + 0.1 * y) + 50 * cos(0.27 * y - 0.05 * x) + (int)(lcg(&seed) >> 29));
            b[y * w + x] = (uint8_t)(128 + 60 * sin(0.35 * (x - 1) + 0.1 * y) + 50 * cos(0.27 * y - 0.05 * (x - 1)) + (int)(lcg(&seed) >> 29));
        }
    for (int k = 0; k < N; k++) {   /* from win + 2 pixels outside to win + 2 pixels outside, quarter-pixel positions */
        pts[2 * k] = (float)((int)(lcg(&seed) >> 8) % (4 * (w + 2 * win + 4))) * 0.25f - (float)(win + 2);
        pts[2 * k + 1] = (float)((int)(lcg(&seed) >> 8) % (4 * (h + 2 * win + 4))) * 0.25f - (float)(win + 2);
    }
    pts[0] = NAN, pts[3] = NAN, pts[4] = 1e9f, pts[7] = -1e9f, pts[8] = INFINITY, pts[11] = -INFINITY, pts[12] = 3e38f;
    pts[14] = (float)(-win) + (float)half_patch, pts[16] = (float)(w - 1 + half_patch), pts[19] = (float)(h - 1 + half_patch);
    int rc = lk_ref_track(a, b, w, h, w, w, half_patch, max_level, 30, 0.01, 1e-4, 12.0f, N - 1, N, pts, out, st, raw, err,
                          flow, info, iters, why);
    for (int i = 0; i < 8 * N; i++) {
        if (why[i] > 6) return 1;
        left[why[i]]++;
    }
    printf("%d x %d, win %d: rc %d, info %d %d %d %d %d %d, why %d %d %d %d %d %d %d\n", w, h, win, rc, info[0], info[1], info[2],
           info[3], info[4], info[5], left[0], left[1], left[2], left[3], left[4], left[5], left[6]);
    /* once more without the optional outputs */
    rc |= lk_ref_track(a, b, w, h, w, w, half_patch, max_level, 2, 0.0, 0.0, 0.0f, N - 1, N, pts, out, st, raw, err, flow, info, NULL,
                       NULL);
    free(a), free(b), free(pts), free(out), free(flow), free(err), free(st), free(raw), free(iters), free(why);
    return rc;
}

int main(void)
{
    int bad = 0, images = 0;
    bad |= run(48, 36, 2, 2, 1u), images++;
    bad |= run(33, 31, 1, 7, 2u), images++;
    bad |= run(40, 24, 10, 2, 3u), images++;
    bad |= run(70, 66, 15, 2, 4u), images++;
    printf("%d images\n", images);
    return bad;
}
