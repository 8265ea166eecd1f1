/* lk_flow_sanitize.c -- a stand-alone driver over tests/lk_flow_ref.c for AddressSanitizer and UBSan on the shapes of the flow
 * edge table (tests/lk_flow_ref_util.py): every window at both ends of each kernel's range, on its smallest legal frame and
 * on a frame of three levels; seeded image pairs, each array in a heap block of exactly its size (a read outside it is an
 * error); initial points on the reference point, a sub-pixel and a negative step away, several windows away, infinite and NaN;
 * a mix of status_in values; a count below the capacity; cameras with four and five coefficients and with k1 == 0.
 * Build: gcc -std=c99 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all lk_flow_sanitize.c
 *        lk_flow_ref.c -lm */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int lk_flow_ref_track(const uint8_t *ref, const uint8_t *cur, int32_t w, int32_t h, int64_t step_ref, int64_t step_cur,
                      int32_t half_patch, int32_t max_level, int32_t max_count, double epsilon, double min_eig_threshold,
                      float err_threshold, const float *cam, int32_t n_dist_coef, int32_t n, int32_t cap, const float *pt_ref,
                      const float *pt_init, const uint8_t *status_in, float *pt_out, float *pt_out_dist, uint8_t *status,
                      uint8_t *status_raw, float *err, float *flow, int32_t *info, int32_t *iters, uint8_t *why);

static uint32_t lcg(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }

static int run(int w, int h, int half_patch, int max_level, int camera, uint32_t seed)
{
    enum { CAP = 48, N = 43 };
    const int win = 2 * half_patch + 1;
    uint8_t *a = (uint8_t *)malloc((size_t)w * h), *b = (uint8_t *)malloc((size_t)w * h);
    float *pts = (float *)malloc(sizeof(float) * 2 * CAP), *init = (float *)malloc(sizeof(float) * 2 * CAP);
    float *out = (float *)malloc(sizeof(float) * 2 * CAP), *dist = (float *)malloc(sizeof(float) * 2 * CAP);
    float *flow = (float *)malloc(sizeof(float) * 2 * CAP), *err = (float *)malloc(sizeof(float) * CAP);
    uint8_t *live = (uint8_t *)malloc(CAP), *st = (uint8_t *)malloc(CAP), *raw = (uint8_t *)malloc(CAP);
    int32_t *info = (int32_t *)malloc(sizeof(int32_t) * 8), *iters = (int32_t *)malloc(sizeof(int32_t) * CAP);
    uint8_t *why = (uint8_t *)malloc(8 * CAP);
    float *cam = (float *)malloc(sizeof(float) * 9);
    if (!a || !b || !pts || !init || !out || !dist || !flow || !err || !live || !st || !raw || !info || !iters || !why || !cam) return 1;
    for (int y = 0; y < h; y++)   /* smooth enough to track, one pixel apart */
        for (int x = 0; x < w; x++) {
            a[y * w + x] = (uint8_t)(128 + 60 * sin(0.35 * x + 0.1 * y) + 50 * cos(0.27 * y - 0.05 * x) + (int)(lcg(&seed) >> 29));
            b[y * w + x] = (uint8_t)(128 + 60 * sin(0.35 * (x - 1) + 0.1 * y) + 50 * cos(0.27 * y - 0.05 * (x - 1)) + (int)(lcg(&seed) >> 29));
        }
    for (int k = 0; k < CAP; k++) {   /* from win + 2 pixels outside to win + 2 pixels outside, quarter-pixel positions */
        pts[2 * k] = (float)((int)(lcg(&seed) >> 8) % (4 * (w + 2 * win + 4))) * 0.25f - (float)(win + 2);
        pts[2 * k + 1] = (float)((int)(lcg(&seed) >> 8) % (4 * (h + 2 * win + 4))) * 0.25f - (float)(win + 2);
        if (k % 2) pts[2 * k] = (float)(k % w), pts[2 * k + 1] = (float)(k % h) + 0.5f;   /* every other one inside */
        float dx = 0.f, dy = 0.f;
        switch (k % 6) {
            case 1: dx = 0.3125f, dy = -0.4375f; break;
            case 2: dx = -1.75f, dy = -2.5f; break;
            case 3: dx = 3.f * (float)win + 0.5f, dy = 2.f * (float)win; break;
            case 4: dx = INFINITY; break;
            case 5: dy = NAN; break;
            default: break;
        }
        init[2 * k] = pts[2 * k] + dx, init[2 * k + 1] = pts[2 * k + 1] + dy;
        live[k] = (uint8_t)((lcg(&seed) >> 30) != 0 ? 1 + (k & 1) * 200 : 0);
    }
    pts[0] = NAN, pts[5] = 1e9f, pts[8] = INFINITY, pts[13] = -3e38f;
    init[14] = 3e38f, init[17] = -INFINITY;
    cam[0] = 61.5f, cam[1] = 59.25f, cam[2] = (float)w * 0.5f, cam[3] = (float)h * 0.5f;
    cam[4] = camera == 2 ? 0.f : -0.2834f, cam[5] = 0.0739f, cam[6] = 0.00019f, cam[7] = 1.76e-5f, cam[8] = -0.0112f;
    int rc = lk_flow_ref_track(a, b, w, h, w, w, half_patch, max_level, 30, 0.01, 1e-4, 12.0f, cam, camera == 0 ? 4 : 5, N, CAP, pts,
                               init, live, out, dist, st, raw, err, flow, info, iters, why);
    int left[7] = {0};
    for (int i = 0; i < 8 * CAP; i++) {
        if (why[i] > 6) return 1;
        left[why[i]]++;
    }
    for (int k = N; k < CAP; k++)
        if (out[2 * k] != 0.f || dist[2 * k + 1] != 0.f || st[k] || raw[k] || err[k] != 0.f || flow[2 * k] != 0.f) return 1;
    printf("%d x %d, win %d, camera %d: rc %d, info %d %d %d %d %d %d %d, why %d %d %d %d %d %d %d\n", w, h, win, camera, rc, info[0],
           info[1], info[2], info[3], info[4], info[5], info[6], left[0], left[1], left[2], left[3], left[4], left[5], left[6]);
    /* once more without the optional inputs and outputs */
    rc |= lk_flow_ref_track(a, b, w, h, w, w, half_patch, max_level, 2, 0.0, 0.0, 0.0f, NULL, 4, N, CAP, pts, NULL, NULL, out, NULL, st,
                            raw, err, flow, info, NULL, NULL);
    free(a), free(b), free(pts), free(init), free(out), free(dist), free(flow), free(err), free(live), free(st), free(raw);
    free(info), free(iters), free(why), free(cam);
    return rc;
}

int main(void)
{
    static const int wins[10] = {3, 7, 9, 11, 13, 15, 17, 21, 23, 31};
    int bad = 0, frames = 0;
    for (int i = 0; i < 10; i++) {
        const int win = wins[i], w3 = 4 * win + 9 < 160 ? 4 * win + 9 : 160, h3 = 4 * win + 6 < 128 ? 4 * win + 6 : 128;
        bad |= run(win + 1, win + 1, win / 2, 0, i % 3, 10u + (uint32_t)i), frames++;
        bad |= run(w3, h3, win / 2, 2, (i + 1) % 3, 30u + (uint32_t)i), frames++;
    }
    printf("%d frames\n", frames);
    return bad;
}
