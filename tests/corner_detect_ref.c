/* corner_detect_ref.c -- plain-C restatement of the corner detector defined in include/pagk.h (pagk_detect_corners):
 * the reference's cv::goodFeaturesToTrack(mGray, corners_un, n_new, 0.005, 20, mMask, 3, true, 0.04)
 * (reference src/frame.cpp:181-184) with the Harris response, as that header defines it step by step.
 *   cdr_response    Sobel, 3 x 3 block sums, R = (float)((a*c - b*b) - k * (a + c)^2)
 *   cdr_raw_bound   ceil((W-2)/2) * ceil((H-2)/2)
 *   cdr_detect      threshold against Rmax under the mask, the 3 x 3 non-maximum test with the raster-order tie rule,
 *                   descending order of (bits(R), pixel index), greedy minimum distance, the info words
 * Sequential loops over whole-image arrays.  Shares no code with the kernels (csrc/pagk_detect_kernel.h).
 * Build: gcc -std=c99 -O2 -ffp-contract=off (one rounding per operation). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* index -1 is 1, index n is n - 2 */
static int cdr_reflect(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

static int cdr_pixel(const uint8_t *img, int64_t step, int w, int h, int x, int y)
{
    return img[(int64_t)cdr_reflect(y, h) * step + cdr_reflect(x, w)];
}

/* R: w * h floats.  Returns 0, or -1 when memory ran out. */
int32_t cdr_response(const uint8_t *img, int32_t w, int32_t h, int64_t step, double k, float *R)
{
    const size_t px = (size_t)w * h;
    int32_t *dx = (int32_t *)malloc(px * sizeof(int32_t)), *dy = (int32_t *)malloc(px * sizeof(int32_t));
    int x, y, u, v;
    if (!dx || !dy) {
        free(dx);
        free(dy);
        return -1;
    }
    for (y = 0; y < h; y++)
        for (x = 0; x < w; x++) {
            dx[(size_t)y * w + x] = (cdr_pixel(img, step, w, h, x + 1, y - 1) + 2 * cdr_pixel(img, step, w, h, x + 1, y) +
                                     cdr_pixel(img, step, w, h, x + 1, y + 1)) -
                                    (cdr_pixel(img, step, w, h, x - 1, y - 1) + 2 * cdr_pixel(img, step, w, h, x - 1, y) +
                                     cdr_pixel(img, step, w, h, x - 1, y + 1));
            dy[(size_t)y * w + x] = (cdr_pixel(img, step, w, h, x - 1, y + 1) + 2 * cdr_pixel(img, step, w, h, x, y + 1) +
                                     cdr_pixel(img, step, w, h, x + 1, y + 1)) -
                                    (cdr_pixel(img, step, w, h, x - 1, y - 1) + 2 * cdr_pixel(img, step, w, h, x, y - 1) +
                                     cdr_pixel(img, step, w, h, x + 1, y - 1));
        }
    for (y = 0; y < h; y++)
        for (x = 0; x < w; x++) {
            int32_t a = 0, b = 0, c = 0;
            double da, db, dc, det, tr, r64;
            for (v = -1; v <= 1; v++)
                for (u = -1; u <= 1; u++) { /* the product maps, reflected like the image */
                    const size_t q = (size_t)cdr_reflect(y + v, h) * w + cdr_reflect(x + u, w);
                    a += dx[q] * dx[q];
                    b += dx[q] * dy[q];
                    c += dy[q] * dy[q];
                }
            da = (double)a, db = (double)b, dc = (double)c;
            det = da * dc - db * db; /* exact: integers below 2^53 */
            tr = da + dc;
            r64 = det - k * (tr * tr); /* two roundings (-ffp-contract=off: no FMA) */
            R[(size_t)y * w + x] = (float)r64;
        }
    free(dx);
    free(dy);
    return 0;
}

int64_t cdr_raw_bound(int32_t w, int32_t h) { return (int64_t)((w - 2 + 1) / 2) * ((h - 2 + 1) / 2); }

static int cdr_key_desc(const void *pa, const void *pb)
{
    const uint64_t a = *(const uint64_t *)pa, b = *(const uint64_t *)pb;
    return a < b ? 1 : (a > b ? -1 : 0);
}

/* mask: w * h bytes or NULL.  raw_cap 0 = the bound.  corners: cap x 2 floats, all written; the limit is
 * min(cap, max(0, max_corners)).  info: 8 words.  R_out (w * h floats) may be NULL.  Returns 0, or -1 out of memory. */
int32_t cdr_detect(const uint8_t *img, int32_t w, int32_t h, int64_t step, const uint8_t *mask, double quality_level,
                   double min_distance, double k, int32_t raw_cap, int32_t max_corners, int32_t cap, float *corners,
                   int32_t *info, float *R_out)
{
    const size_t px = (size_t)w * h;
    float *R = (float *)malloc(px * sizeof(float));
    uint64_t *keys = (uint64_t *)malloc((px / 4 + 1) * sizeof(uint64_t)); /* >= the bound */
    int32_t *acc_x = (int32_t *)malloc(((size_t)cap + 1) * sizeof(int32_t)), *acc_y = (int32_t *)malloc(((size_t)cap + 1) * sizeof(int32_t));
    int64_t n_raw = 0, i;
    int32_t n_acc = 0, visited = 0, limit, overflow = 0, have_max = 0, x, y, j;
    float rmax = 0.0f;
    uint32_t rmax_bits = 0;
    memset(corners, 0, (size_t)cap * 2 * sizeof(float));
    memset(info, 0, 8 * sizeof(int32_t));
    if (!R || !keys || !acc_x || !acc_y || cdr_response(img, w, h, step, k, R)) {
        free(R), free(keys), free(acc_x), free(acc_y);
        return -1;
    }
    if (R_out) memcpy(R_out, R, px * sizeof(float));
    if (raw_cap <= 0) raw_cap = (int32_t)cdr_raw_bound(w, h);
    limit = max_corners < 0 ? 0 : (max_corners > cap ? cap : max_corners);
    for (i = 0; i < (int64_t)px; i++) /* Rmax over the unmasked pixels, the outer ring included */
        if (!mask || mask[i]) {
            if (!have_max || R[i] > rmax) rmax = R[i];
            have_max = 1;
        }
    if (have_max && rmax > 0.0f) {
        const double thr = quality_level * (double)rmax;
        memcpy(&rmax_bits, &rmax, 4);
        for (y = 1; y <= h - 2; y++)
            for (x = 1; x <= w - 2; x++) {
                const size_t p = (size_t)y * w + x;
                const float r = R[p];
                uint32_t bits;
                if (mask && !mask[p]) continue;
                if (!((double)r > thr)) continue;
                /* >= the neighbours in front in raster order, > the ones behind */
                if (!(r >= R[p - w - 1] && r >= R[p - w] && r >= R[p - w + 1] && r >= R[p - 1])) continue;
                if (!(r > R[p + 1] && r > R[p + w - 1] && r > R[p + w] && r > R[p + w + 1])) continue;
                memcpy(&bits, &r, 4);
                keys[n_raw++] = ((uint64_t)bits << 32) | (uint64_t)p;
            }
        if (n_raw > raw_cap) {
            overflow = 1; /* which candidates a buffer of raw_cap would hold is undefined: no corners */
        } else {
            const double d2 = min_distance * min_distance;
            qsort(keys, (size_t)n_raw, sizeof(uint64_t), cdr_key_desc);
            for (i = 0; i < n_raw; i++) {
                int near = 0;
                if (n_acc >= limit) break;
                visited++;
                y = (int32_t)((keys[i] & 0xffffffffu) / (uint32_t)w);
                x = (int32_t)((keys[i] & 0xffffffffu) % (uint32_t)w);
                if (min_distance >= 1.0)
                    for (j = 0; j < n_acc && !near; j++) {
                        const int64_t ddx = x - acc_x[j], ddy = y - acc_y[j];
                        near = (double)(ddx * ddx + ddy * ddy) < d2;
                    }
                if (near) continue;
                acc_x[n_acc] = x, acc_y[n_acc] = y;
                corners[2 * n_acc] = (float)x, corners[2 * n_acc + 1] = (float)y;
                n_acc++;
            }
        }
    }
    info[0] = n_acc;
    info[1] = (int32_t)n_raw;
    info[2] = overflow;
    info[3] = (int32_t)rmax_bits;
    info[4] = visited;
    free(R), free(keys), free(acc_x), free(acc_y);
    return 0;
}
