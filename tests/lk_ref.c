/* lk_ref.c -- the definition "Pyramidal Lucas-Kanade" of include/pagk.h restated in plain C: the 5 x 5 pyrDown levels, the
 * Scharr derivatives with their zero border, the Q14 bilinear template, the exact 64-bit sums, the f32 tail with one
 * rounding per operation, and the reference's error filter.  The device result is held to this, byte for byte.
 * Build: gcc -std=c99 -O2 -ffp-contract=off -shared -fPIC lk_ref.c -lm */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define INFO_WORDS 8
#define MAX_LEVELS 8

static int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

/* the effective top level, or -1 when level 0 is not larger than the window */
int lk_ref_levels(int32_t w, int32_t h, int32_t half_patch, int32_t max_level)
{
    const int win = 2 * half_patch + 1;
    if (w <= win || h <= win) return -1;
    int top = 0;
    while (top < max_level) {
        w = (w + 1) / 2, h = (h + 1) / 2;
        if (w <= win || h <= win) break;
        top++;
    }
    return top;
}

/* dst: (h + 1) / 2 rows of (w + 1) / 2 bytes */
void lk_ref_pyrdown(const uint8_t *src, int32_t w, int32_t h, int64_t step, uint8_t *dst)
{
    static const int wt[5] = {1, 4, 6, 4, 1};
    const int dw = (w + 1) / 2, dh = (h + 1) / 2;
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            int s = 0;
            for (int j = 0; j < 5; j++)
                for (int i = 0; i < 5; i++)
                    s += wt[i] * wt[j] * src[(int64_t)reflect101(2 * y + j - 2, h) * step + reflect101(2 * x + i - 2, w)];
            dst[(size_t)y * dw + x] = (uint8_t)((s + 128) >> 8);
        }
}

typedef struct {
    const uint8_t *p;
    int w, h;
    int64_t step;
} plane;

static int gray(const plane *m, int x, int y) { return m->p[(int64_t)reflect101(y, m->h) * m->step + reflect101(x, m->w)]; }

static int t0(const plane *m, int x, int y) { return 3 * (gray(m, x, y - 1) + gray(m, x, y + 1)) + 10 * gray(m, x, y); }
static int t1(const plane *m, int x, int y) { return gray(m, x, y + 1) - gray(m, x, y - 1); }

/* the Scharr pair at (x, y); 0 outside the level */
static void deriv(const plane *m, int x, int y, int *dx, int *dy)
{
    if (x < 0 || x >= m->w || y < 0 || y >= m->h) {
        *dx = *dy = 0;
        return;
    }
    *dx = t0(m, x + 1, y) - t0(m, x - 1, y);
    *dy = 3 * (t1(m, x - 1, y) + t1(m, x + 1, y)) + 10 * t1(m, x, y);
}

/* both derivative planes of an image (h rows of w int16 each), for the hand-checkable cases */
void lk_ref_scharr(const uint8_t *img, int32_t w, int32_t h, int64_t step, int16_t *dx, int16_t *dy)
{
    const plane m = {img, w, h, step};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int a, b;
            deriv(&m, x, y, &a, &b);
            dx[(size_t)y * w + x] = (int16_t)a, dy[(size_t)y * w + x] = (int16_t)b;
        }
}

/* step 2: the range test on the floored f32 coordinates, before any conversion */
static int out_of_range(float fx, float fy, int win, int w, int h)
{
    if (!isfinite(fx) || !isfinite(fy)) return 1;
    return fx < (float)-win || fx >= (float)w || fy < (float)-win || fy >= (float)h;
}

/* step 3 */
static void weights(float a, float b, int iw[4])
{
    iw[0] = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
    iw[1] = (int)rintf(a * (1.f - b) * 16384.f);
    iw[2] = (int)rintf((1.f - a) * b * 16384.f);
    iw[3] = 16384 - iw[0] - iw[1] - iw[2];
}

static int sample(const plane *m, int x, int y, const int iw[4])
{
    return (gray(m, x, y) * iw[0] + gray(m, x + 1, y) * iw[1] + gray(m, x, y + 1) * iw[2] + gray(m, x + 1, y + 1) * iw[3] + 256) >> 9;
}

typedef struct {
    uint8_t *lv[MAX_LEVELS];
    plane m[MAX_LEVELS];
} pyramid;

static int build(pyramid *p, const uint8_t *img, int w, int h, int64_t step, int top)
{
    memset(p, 0, sizeof(*p));
    p->m[0].p = img, p->m[0].w = w, p->m[0].h = h, p->m[0].step = step;
    for (int l = 1; l <= top; l++) {
        const plane *s = &p->m[l - 1];
        const int dw = (s->w + 1) / 2, dh = (s->h + 1) / 2;
        p->lv[l] = (uint8_t *)malloc((size_t)dw * dh);
        if (!p->lv[l]) return -1;
        lk_ref_pyrdown(s->p, s->w, s->h, s->step, p->lv[l]);
        p->m[l].p = p->lv[l], p->m[l].w = dw, p->m[l].h = dh, p->m[l].step = dw;
    }
    return 0;
}

static void drop(pyramid *p)
{
    for (int l = 0; l < MAX_LEVELS; l++) free(p->lv[l]);
}

/* level `level` (1 .. top) of an image's pyramid into dst (tight rows); returns 0, or -1 for a level that does not exist */
int lk_ref_level(const uint8_t *img, int32_t w, int32_t h, int64_t step, int32_t half_patch, int32_t max_level, int32_t level,
                 uint8_t *dst)
{
    const int top = lk_ref_levels(w, h, half_patch, max_level);
    pyramid p;
    if (top < 0 || level < 1 || level > top || build(&p, img, w, h, step, top)) return -1;
    memcpy(dst, p.lv[level], (size_t)p.m[level].w * p.m[level].h);
    drop(&p);
    return 0;
}

/* why a feature left a level (the optional record `why` of lk_ref_track) */
enum {
    WHY_NOT_VISITED = 0,   /* the level is above the effective top level, or the feature was done */
    WHY_TEMPLATE = 1,      /* step 2: the template is out of range */
    WHY_MIN_EIG = 2,       /* step 5: the min-eigenvalue or the determinant test failed */
    WHY_RANGE = 3,         /* step 6: out of range inside the iteration */
    WHY_EPSILON = 4,       /* step 6: stopped by epsilon */
    WHY_OSCILLATION = 5,   /* step 6: stopped by the oscillation rule */
    WHY_COUNT = 6          /* step 6: the iteration count was used up */
};

/* The tracker.  pt_ref, pt_out, flow: cap x 2; status, status_raw: cap bytes; err: cap; info: INFO_WORDS; iters (or NULL):
 * cap int32, the iterations run at level 0; why (or NULL): cap x MAX_LEVELS bytes, byte [k][l] says why feature k left level
 * l (the WHY_ codes above).  Rows at or beyond n (clamped to [0, cap]) are zeroed. */
int lk_ref_track(const uint8_t *ref, const uint8_t *cur, int32_t w, int32_t h, int64_t step_ref, int64_t step_cur,
                 int32_t half_patch, int32_t max_level, int32_t max_count, double epsilon, double min_eig_threshold,
                 float err_threshold, int32_t n, int32_t cap, const float *pt_ref, float *pt_out, uint8_t *status,
                 uint8_t *status_raw, float *err, float *flow, int32_t *info, int32_t *iters, uint8_t *why)
{
    const int win = 2 * half_patch + 1;
    const int top = lk_ref_levels(w, h, half_patch, max_level);
    if (top < 0 || top >= MAX_LEVELS) return -1;
    pyramid pi, pj;
    if (build(&pi, ref, w, h, step_ref, top) || build(&pj, cur, w, h, step_cur, top)) return -2;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    int *tI = (int *)malloc(sizeof(int) * 3 * win * win), *tx = tI + win * win, *ty = tx + win * win;
    if (!tI) return -2;
    memset(info, 0, INFO_WORDS * sizeof(int32_t));
    info[0] = n, info[3] = top;
    const float half = (float)(win - 1) * 0.5f;
    for (int k = 0; k < cap; k++) {
        pt_out[2 * k] = pt_out[2 * k + 1] = flow[2 * k] = flow[2 * k + 1] = err[k] = 0.f;
        status[k] = status_raw[k] = 0;
        if (iters) iters[k] = 0;
        if (why) memset(why + (size_t)k * MAX_LEVELS, WHY_NOT_VISITED, MAX_LEVELS);
        if (k >= n) continue;
        uint8_t *const left = why ? why + (size_t)k * MAX_LEVELS : NULL;
        int st = 1;
        float e = 0.f, nx = 0.f, ny = 0.f;
        for (int l = top; l >= 0; l--) {
            const plane *I = &pi.m[l], *J = &pj.m[l];
            const float sc = (float)(1.0 / (double)(1 << l));
            const float px = pt_ref[2 * k] * sc - half, py = pt_ref[2 * k + 1] * sc - half;   /* prev - half */
            if (l == top)
                nx = pt_ref[2 * k] * sc, ny = pt_ref[2 * k + 1] * sc;
            else
                nx = 2.f * nx, ny = 2.f * ny;
            const float fx = floorf(px), fy = floorf(py);
            if (out_of_range(fx, fy, win, I->w, I->h)) {
                if (l == 0) st = 0, e = 0.f, info[5]++;
                if (left) left[l] = WHY_TEMPLATE;
                continue;
            }
            const int ipx = (int)fx, ipy = (int)fy;
            int iw[4];
            weights(px - fx, py - fy, iw);
            int64_t S11 = 0, S12 = 0, S22 = 0;
            for (int y = 0; y < win; y++)
                for (int x = 0; x < win; x++) {
                    int dx[4], dy[4];
                    deriv(I, ipx + x, ipy + y, &dx[0], &dy[0]);
                    deriv(I, ipx + x + 1, ipy + y, &dx[1], &dy[1]);
                    deriv(I, ipx + x, ipy + y + 1, &dx[2], &dy[2]);
                    deriv(I, ipx + x + 1, ipy + y + 1, &dx[3], &dy[3]);
                    const int ix = (dx[0] * iw[0] + dx[1] * iw[1] + dx[2] * iw[2] + dx[3] * iw[3] + 8192) >> 14;
                    const int iy = (dy[0] * iw[0] + dy[1] * iw[1] + dy[2] * iw[2] + dy[3] * iw[3] + 8192) >> 14;
                    tI[y * win + x] = sample(I, ipx + x, ipy + y, iw);
                    tx[y * win + x] = ix, ty[y * win + x] = iy;
                    S11 += (int64_t)ix * ix, S12 += (int64_t)ix * iy, S22 += (int64_t)iy * iy;
                }
            const float A11 = (float)S11 * 0x1p-20f, A12 = (float)S12 * 0x1p-20f, A22 = (float)S22 * 0x1p-20f;
            float D = A11 * A22 - A12 * A12;
            const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
            if ((double)minEig < min_eig_threshold || D < FLT_EPSILON) {
                if (l == 0) st = 0, info[4]++;
                if (left) left[l] = WHY_MIN_EIG;
                continue;
            }
            D = 1.f / D;
            float qx = nx - half, qy = ny - half, pdx = 0.f, pdy = 0.f;
            int code = WHY_COUNT;
            for (int j = 0; j < max_count; j++) {
                const float gx = floorf(qx), gy = floorf(qy);
                if (out_of_range(gx, gy, win, J->w, J->h)) {
                    if (l == 0) st = 0, info[5]++;
                    code = WHY_RANGE;
                    break;
                }
                if (l == 0 && iters) iters[k] = j + 1;
                const int iqx = (int)gx, iqy = (int)gy;
                weights(qx - gx, qy - gy, iw);
                int64_t B1 = 0, B2 = 0;
                for (int y = 0; y < win; y++)
                    for (int x = 0; x < win; x++) {
                        const int diff = sample(J, iqx + x, iqy + y, iw) - tI[y * win + x];
                        B1 += (int64_t)diff * tx[y * win + x], B2 += (int64_t)diff * ty[y * win + x];
                    }
                const float b1 = (float)B1 * 0x1p-20f, b2 = (float)B2 * 0x1p-20f;
                const float ddx = (A12 * b2 - A22 * b1) * D, ddy = (A12 * b1 - A11 * b2) * D;
                qx += ddx, qy += ddy;
                nx = qx + half, ny = qy + half;
                if ((double)ddx * ddx + (double)ddy * ddy <= epsilon * epsilon) {
                    code = WHY_EPSILON;
                    break;
                }
                if (j > 0 && (double)fabsf(ddx + pdx) < 0.01 && (double)fabsf(ddy + pdy) < 0.01) {
                    nx -= ddx * 0.5f, ny -= ddy * 0.5f;
                    code = WHY_OSCILLATION;
                    break;
                }
                pdx = ddx, pdy = ddy;
            }
            if (left) left[l] = (uint8_t)code;
            if (l == 0 && st) {
                const float ex = nx - half, ey = ny - half, gx = floorf(ex), gy = floorf(ey);
                if (out_of_range(gx, gy, win, J->w, J->h)) {
                    st = 0, info[5]++;
                } else {
                    const int iex = (int)gx, iey = (int)gy;
                    weights(ex - gx, ey - gy, iw);
                    int64_t E = 0;
                    for (int y = 0; y < win; y++)
                        for (int x = 0; x < win; x++) E += llabs((long long)(sample(J, iex + x, iey + y, iw) - tI[y * win + x]));
                    e = (float)E / (float)(32 * win * win);
                }
            }
        }
        pt_out[2 * k] = nx, pt_out[2 * k + 1] = ny;
        err[k] = e;
        status_raw[k] = (uint8_t)st;
        status[k] = (uint8_t)(st && !(e >= err_threshold));
        flow[2 * k] = nx - pt_ref[2 * k], flow[2 * k + 1] = ny - pt_ref[2 * k + 1];
        info[1] += st, info[2] += status[k];
    }
    free(tI);
    drop(&pi), drop(&pj);
    return 0;
}
