/* "ORB over a scale pyramid" of include/pagk.h restated in plain C: the level table, the resize, the per-level loop, the
 * packing and the mask variant of the reference's ORBextractor (src/ORBextractor.cc).  Compiled TOGETHER with
 * tests/fast_detect_ref.c (fdr_*: the one-level detector) and tests/orb_ref.c (orb_ref_*: blur, orientation, descriptors),
 * which stay as they are.  Sequential, no attempt at speed. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAX_LEVELS 8
#define INFO_WORDS 32

int fdr_bounds(int w, int h, int n_features, int *raw_bound, int *out_bound);
int fdr_detect(const uint8_t *img, int w, int h, int64_t step, const uint8_t *mask, int t_ini, int t_min, int n_features, int cap,
               float *kp, float *resp, int *info, int *stats, int reverse_tie);
int orb_ref_describe(const uint8_t *img, int32_t w, int32_t h, int64_t step, const int32_t *wt, const int32_t *pattern,
                     int32_t n, int32_t cap, const float *keypoints, float *angle, uint8_t *desc, int32_t *info,
                     uint8_t *blurred);

static int cv_round(float v) { return (int)lrintf(v); } /* ties to even */

/* The constructor (src/ORBextractor.cc:434-470) and the level sizes of ComputePyramid (:1211-1212).  Arrays of MAX_LEVELS
 * entries.  -1 where the definition refuses. */
int olr_levels(int n_features, float scale_factor, int n_levels, int W, int H, int *lw, int *lh, float *sc, int *quota,
               int *size, int *out_bound)
{
    if (n_levels < 1 || n_levels > MAX_LEVELS || !(scale_factor > 1.0f) || !(scale_factor <= 1.5f) || n_features < 1 ||
        n_features > (1 << 24) || W < 1 || H < 1)
        return -1;
    float inv[MAX_LEVELS];
    sc[0] = 1.0f, inv[0] = 1.0f; /* :446-455 */
    for (int l = 1; l < n_levels; l++) {
        sc[l] = sc[l - 1] * scale_factor;
        inv[l] = 1.0f / sc[l];
    }
    const float factor = 1.0f / scale_factor; /* :459 */
    double p = 1.0;
    for (int l = 0; l < n_levels; l++) p *= (double)factor; /* the library's rule in place of pow (:460) */
    const float num = (float)n_features * (1.0f - factor), den = 1.0f - (float)p;
    float nd = num / den;
    int sum = 0;
    for (int l = 0; l < n_levels - 1; l++) { /* :463-468 */
        quota[l] = cv_round(nd);
        sum += quota[l];
        nd *= factor;
    }
    quota[n_levels - 1] = n_features - sum > 0 ? n_features - sum : 0; /* :469 */
    int total = 0;
    for (int l = 0; l < n_levels; l++) {
        lw[l] = cv_round((float)W * inv[l]), lh[l] = cv_round((float)H * inv[l]); /* :1211-1212 */
        size[l] = (int)(31.0f * sc[l]);                                            /* :860 */
        int rb, ob;
        if (fdr_bounds(lw[l], lh[l], quota[l] > 1 ? quota[l] : 1, &rb, &ob)) return -1;
        total += ob;
    }
    *out_bound = total;
    return 0;
}

/* cv::resize(src, dst, sz, 0, 0, INTER_LINEAR) of :1220 for 8-bit images, as include/pagk.h writes it out */
int olr_resize(const uint8_t *src, int sw, int sh, int64_t sstep, uint8_t *dst, int dw, int dh, int64_t dstep)
{
    if (!src || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1 || sstep < sw || dstep < dw) return -1;
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int b0 = cv_round((1.f - fy) * 2048.f), b1 = cv_round(fy * 2048.f);
        const int y0 = sy < 0 ? 0 : (sy < sh ? sy : sh - 1);
        const int y1 = sy + 1 < 0 ? 0 : (sy + 1 < sh ? sy + 1 : sh - 1);
        const uint8_t *r0 = src + (int64_t)y0 * sstep, *r1 = src + (int64_t)y1 * sstep;
        for (int dx = 0; dx < dw; dx++) {
            float fx = (float)((dx + 0.5) * scale_x - 0.5);
            int sx = (int)floorf(fx);
            fx -= (float)sx;
            int single = 0;
            if (sx < 0) fx = 0, sx = 0;
            if (sx + 1 >= sw) {
                single = 1;
                if (sx >= sw - 1) fx = 0, sx = sw - 1;
            }
            const int a0 = cv_round((1.f - fx) * 2048.f), a1 = cv_round(fx * 2048.f);
            int S0, S1;
            if (single) {
                S0 = r0[sx] * 2048, S1 = r1[sx] * 2048;
            } else {
                S0 = r0[sx] * a0 + r0[sx + 1] * a1, S1 = r1[sx] * a0 + r1[sx + 1] * a1;
            }
            dst[(int64_t)dy * dstep + dx] = (uint8_t)(((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2) & 255);
        }
    }
    return 0;
}

/* ORBextractor::operator() (:1066-1146; pattern != NULL) or DetectFeatures (:1148-1205; pattern == NULL, mask or NULL).
 * kp cap x 2, octave cap, resp cap, angle cap and desc cap x 32 (both or NULL), info INFO_WORDS; levels (or NULL): the
 * level images one after the other, rows of lw[l] bytes. */
int olr_extract(const uint8_t *img, int W, int H, int64_t step, int n_features, float scale_factor, int n_levels, int t_ini,
                int t_min, const int32_t *wt, const int32_t *pattern, const uint8_t *mask, int cap, float *kp, int32_t *octave,
                float *resp, float *angle, uint8_t *desc, int32_t *info, uint8_t *levels)
{
    int lw[MAX_LEVELS], lh[MAX_LEVELS], quota[MAX_LEVELS], size[MAX_LEVELS], out_bound;
    float sc[MAX_LEVELS];
    if (olr_levels(n_features, scale_factor, n_levels, W, H, lw, lh, sc, quota, size, &out_bound) || cap < out_bound) return -1;
    memset(info, 0, sizeof(int32_t) * INFO_WORDS);
    memset(kp, 0, sizeof(float) * 2 * (size_t)cap), memset(octave, 0, sizeof(int32_t) * (size_t)cap);
    memset(resp, 0, sizeof(float) * (size_t)cap);
    if (angle) memset(angle, 0, sizeof(float) * (size_t)cap);
    if (desc) memset(desc, 0, (size_t)cap * 32);
    uint8_t *prev = NULL;
    int n_out = 0, rc = 0;
    size_t level_off = 0;
    for (int l = 0; l < n_levels && !rc; l++) {
        /* ComputePyramid (:1207-1230): level l from level l - 1 */
        const int w = lw[l], h = lh[l];
        uint8_t *cur = malloc((size_t)w * h);
        if (l == 0)
            for (int y = 0; y < h; y++) memcpy(cur + (size_t)y * w, img + (int64_t)y * step, (size_t)w);
        else
            rc = olr_resize(prev, lw[l - 1], lh[l - 1], lw[l - 1], cur, w, h, w);
        if (levels) memcpy(levels + level_off, cur, (size_t)w * h);
        level_off += (size_t)w * h;
        /* ComputeKeyPointsOctTree for the level (:789-871) with N = max(quota, 1) and no mask */
        const int N = quota[l] > 1 ? quota[l] : 1;
        int rb, ob, finfo[8];
        fdr_bounds(w, h, N, &rb, &ob);
        float *lkp = malloc(sizeof(float) * 2 * (size_t)ob), *lresp = malloc(sizeof(float) * (size_t)ob);
        float *lang = malloc(sizeof(float) * (size_t)ob);
        uint8_t *ldesc = malloc((size_t)ob * 32);
        int32_t oinfo[8] = {0};
        if (!rc) rc = fdr_detect(cur, w, h, w, NULL, t_ini, t_min, N, ob, lkp, lresp, finfo, NULL, 0);
        const int n = rc ? 0 : finfo[0];
        /* computeOrientation on the level (:873-875), blur and descriptors on the blurred level (:1123-1128) */
        if (!rc && pattern) rc = orb_ref_describe(cur, w, h, w, wt, pattern, n, ob, lkp, lang, ldesc, oinfo, NULL);
        int kept = 0;
        for (int k = 0; k < n && !rc; k++) {
            float x = lkp[2 * k], y = lkp[2 * k + 1];
            if (l != 0) x = x * sc[l], y = y * sc[l]; /* :1132-1139, :1189-1196 */
            if (mask) {                                /* :1199-1203 */
                const int ix = (int)x, iy = (int)y;
                if (ix < 0 || ix >= W || iy < 0 || iy >= H || mask[(int64_t)iy * W + ix] == 0) continue;
            }
            kp[2 * n_out] = x, kp[2 * n_out + 1] = y;
            octave[n_out] = l; /* :869 */
            resp[n_out] = lresp[k];
            if (angle) angle[n_out] = pattern ? lang[k] : 0.0f;
            if (desc && pattern) memcpy(desc + (size_t)n_out * 32, ldesc + (size_t)k * 32, 32);
            n_out++, kept++;
        }
        if (!rc) {
            info[1] += oinfo[1];
            info[8 + l] = kept, info[16 + l] = finfo[1], info[24 + l] = quota[l];
        }
        free(lkp), free(lresp), free(lang), free(ldesc);
        free(prev);
        prev = cur;
    }
    free(prev);
    info[0] = n_out, info[2] = n_levels;
    return rc;
}
