/* orb_ref.c -- the definition "ORB descriptors and matching" of include/pagk.h restated in plain C: the Q8 separable blur,
 * IC_Angle with the restated fastAtan2, the steering pair by the stated f64 algorithm, the rBRIEF comparisons, and the
 * brute-force Hamming matcher with its distance filter.  The device result is held to this, byte for byte.
 * Build: gcc -std=c99 -O2 -ffp-contract=off -shared -fPIC orb_ref.c -lm */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define EDGE 19
#define HALF_PATCH 15
#define INFO_WORDS 8

static const int UMAX[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

static int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

/* out: h rows of w bytes.  tmp holds the horizontal pass. */
int orb_ref_blur(const uint8_t *img, int32_t w, int32_t h, int64_t step, const int32_t *wt, uint8_t *out)
{
    if (w < 4 || h < 4) return -1;
    int32_t *tmp = (int32_t *)malloc((size_t)w * h * sizeof(int32_t));
    if (!tmp) return -2;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int32_t s = 0;
            for (int k = -3; k <= 3; k++) s += wt[abs(k)] * img[(int64_t)y * step + reflect101(x + k, w)];
            tmp[(size_t)y * w + x] = s;
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int32_t s = 0;
            for (int k = -3; k <= 3; k++) s += wt[abs(k)] * tmp[(size_t)reflect101(y + k, h) * w + x];
            out[(size_t)y * w + x] = (uint8_t)((s + 32768) >> 16);
        }
    free(tmp);
    return 0;
}

float orb_ref_fast_atan2(float y, float x)
{
    const float p1 = 0x1.ca44dep+5f, p3 = -0x1.2aaddcp+4f, p5 = 0x1.1d3f7ep+3f, p7 = -0x1.4515b2p+1f;
    const float eps = 0x1p-52f; /* (float)DBL_EPSILON */
    float ax = fabsf(x), ay = fabsf(y), a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + eps);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + eps);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

void orb_ref_cos_sin(float r, float *a, float *b)
{
    static const double S[6] = {-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
                                2.75573137070700676789e-06,  -2.50507602534068634195e-08, 1.58969099521155010221e-10};
    static const double C[6] = {4.16666666666666019037e-02,  -1.38888888888741095749e-03, 2.48015872894767294178e-05,
                                -2.75573143513906633035e-07, 2.08757232129817482790e-09,  -1.13596475577881948265e-11};
    double x = (double)r;
    int k = (int)(x * 0x1.45f306dc9c883p-1 + 0.5);
    double t = (x - k * 0x1.921fb544p+0) - k * 0x1.0b4611a626331p-34;
    double z = t * t, ps = S[5], pc = C[5];
    for (int i = 4; i >= 0; i--) {
        ps = S[i] + z * ps;
        pc = C[i] + z * pc;
    }
    double s = t + t * (z * ps);
    double c = 1.0 - z * (0.5 - z * pc);
    double co, si;
    switch (k & 3) {
    case 0: co = c, si = s; break;
    case 1: co = -s, si = c; break;
    case 2: co = -c, si = -s; break;
    default: co = s, si = -c; break;
    }
    *a = (float)co;
    *b = (float)si;
}

/* m[0] = m10, m[1] = m01 of a centre inside the border: the disc row by row */
void orb_ref_moments(const uint8_t *img, int64_t step, int cx, int cy, int32_t *m)
{
    int32_t m10 = 0, m01 = 0;
    for (int v = -HALF_PATCH; v <= HALF_PATCH; v++) {
        const uint8_t *row = img + (int64_t)(cy + v) * step + cx;
        const int d = UMAX[abs(v)];
        int32_t row_sum = 0, row_moment = 0;
        for (int u = -d; u <= d; u++) {
            row_sum += row[u];
            row_moment += u * row[u];
        }
        m10 += row_moment;
        m01 += v * row_sum;
    }
    m[0] = m10;
    m[1] = m01;
}

/* keypoints cap x 2, angle cap (or NULL), desc cap x 32, info INFO_WORDS; blurred (or NULL): h x w bytes out */
int orb_ref_describe(const uint8_t *img, int32_t w, int32_t h, int64_t step, const int32_t *wt, const int32_t *pattern,
                     int32_t n, int32_t cap, const float *keypoints, float *angle, uint8_t *desc, int32_t *info,
                     uint8_t *blurred)
{
    if (n < 0) n = 0;
    if (n > cap) n = cap;
    uint8_t *bl = (uint8_t *)malloc((size_t)w * h);
    if (!bl) return -2;
    int rc = orb_ref_blur(img, w, h, step, wt, bl);
    if (rc) {
        free(bl);
        return rc;
    }
    memset(info, 0, INFO_WORDS * sizeof(int32_t));
    memset(desc, 0, (size_t)cap * 32);
    if (angle) memset(angle, 0, (size_t)cap * sizeof(float));
    for (int k = 0; k < n; k++) {
        float fx = rintf(keypoints[2 * k]), fy = rintf(keypoints[2 * k + 1]);
        if (!(fx >= EDGE && fx < (float)(w - EDGE) && fy >= EDGE && fy < (float)(h - EDGE))) {
            if (angle) angle[k] = -1.f;
            info[1]++;
            continue;
        }
        int cx = (int)fx, cy = (int)fy;
        int32_t m[2];
        orb_ref_moments(img, step, cx, cy, m);
        float ang = orb_ref_fast_atan2((float)m[1], (float)m[0]);
        float r = ang * 0x1.1df46ap-6f, a, b;
        orb_ref_cos_sin(r, &a, &b);
        const uint8_t *center = bl + (size_t)cy * w + cx;
        const int32_t *pt = pattern;
        for (int i = 0; i < 32; i++, pt += 32) {
            int val = 0;
            for (int j = 0; j < 8; j++) {
                float x0 = (float)pt[4 * j], y0 = (float)pt[4 * j + 1], x1 = (float)pt[4 * j + 2], y1 = (float)pt[4 * j + 3];
                int t0 = center[(int)rintf(x0 * b + y0 * a) * w + (int)rintf(x0 * a - y0 * b)];
                int t1 = center[(int)rintf(x1 * b + y1 * a) * w + (int)rintf(x1 * a - y1 * b)];
                val |= (t0 < t1) << j;
            }
            desc[(size_t)k * 32 + i] = (uint8_t)val;
        }
        if (angle) angle[k] = ang;
        info[0]++;
    }
    if (blurred) memcpy(blurred, bl, (size_t)w * h);
    free(bl);
    return 0;
}

static int hamming256(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) {
        unsigned x = (unsigned)(a[i] ^ b[i]);
        while (x) {
            d += (int)(x & 1u);
            x >>= 1;
        }
    }
    return d;
}

/* train_idx, distance, keep: cap_q entries; info INFO_WORDS */
int orb_ref_match(int32_t nq, int32_t cap_q, const uint8_t *desc_q, int32_t nt, const uint8_t *desc_t, int32_t match_floor,
                  int32_t *train_idx, int32_t *distance, uint8_t *keep, int32_t *info)
{
    if (nq < 0) nq = 0;
    if (nq > cap_q) nq = cap_q;
    if (nt < 0) nt = 0;
    int matches = nt > 0 ? nq : 0, min_dist = 257, max_dist = 0, kept = 0;
    for (int q = 0; q < cap_q; q++) train_idx[q] = -1, distance[q] = 257, keep[q] = 0;
    for (int q = 0; q < matches; q++) {
        for (int t = 0; t < nt; t++) {
            int d = hamming256(desc_q + (size_t)q * 32, desc_t + (size_t)t * 32);
            if (d < distance[q]) distance[q] = d, train_idx[q] = t; /* strictly: the lowest index keeps a tie */
        }
        if (distance[q] < min_dist) min_dist = distance[q];
        if (distance[q] > max_dist) max_dist = distance[q];
    }
    if (!matches) min_dist = 0;
    int threshold = 2 * min_dist > match_floor ? 2 * min_dist : match_floor;
    for (int q = 0; q < matches; q++) {
        keep[q] = (uint8_t)(distance[q] <= threshold);
        kept += keep[q];
    }
    memset(info, 0, INFO_WORDS * sizeof(int32_t));
    info[0] = nq, info[1] = matches, info[2] = kept, info[3] = min_dist, info[4] = max_dist, info[5] = threshold;
    return 0;
}
