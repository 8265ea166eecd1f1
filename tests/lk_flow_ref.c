/* lk_flow_ref.c -- the addendum "the flow form" of the definition "Pyramidal Lucas-Kanade" (include/pagk.h) restated in plain
 * C with its own per-feature loop: Lucas-Kanade started from an initial point (OpenCV 3.4's OPTFLOW_USE_INITIAL_FLOW branch),
 * rows switched off by status_in written as zeros and counted in info[6], and pt_out_dist = DistortVecPoints(pt_out)
 * (reference src/utils.cpp:49-76).  Written apart from tests/lk_ref.c (which stays the restatement of flags = 0): whole
 * derivative planes per level, one function per feature.  pagk_lk_track_flow is held to this, byte for byte.
 * Build: gcc -std=c99 -O2 -ffp-contract=off -shared -fPIC lk_flow_ref.c -lm */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define INFO_WORDS 8
#define MAX_LEVELS 8

enum { WHY_NOT_VISITED = 0, WHY_TEMPLATE = 1, WHY_MIN_EIG = 2, WHY_RANGE = 3, WHY_EPSILON = 4, WHY_OSCILLATION = 5, WHY_COUNT = 6 };

static int r101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

typedef struct {
    uint8_t *own;        /* the level's pixels when this file allocated them (levels above 0) */
    const uint8_t *pix;
    int16_t *dx, *dy;    /* the Scharr planes of the level, h rows of w (the reference image alone has them) */
    int w, h;
    int64_t step;
} level;

static int px(const level *m, int x, int y) { return m->pix[(int64_t)r101(y, m->h) * m->step + r101(x, m->w)]; }

/* derivative plane `d` at (x, y): zero outside the level (the constant border of derivI) */
static int at(const level *m, const int16_t *d, int x, int y)
{
    return (x < 0 || x >= m->w || y < 0 || y >= m->h) ? 0 : d[(size_t)y * m->w + x];
}

static int scharr(level *m)
{
    m->dx = (int16_t *)malloc(sizeof(int16_t) * (size_t)m->w * m->h);
    m->dy = (int16_t *)malloc(sizeof(int16_t) * (size_t)m->w * m->h);
    if (!m->dx || !m->dy) return -1;
    for (int y = 0; y < m->h; y++)
        for (int x = 0; x < m->w; x++) {
            /* t0 = 3 (I(x, y - 1) + I(x, y + 1)) + 10 I(x, y) and t1 = I(x, y + 1) - I(x, y - 1) at x - 1, x, x + 1 */
            int t0[3], t1[3];
            for (int i = 0; i < 3; i++) {
                t0[i] = 3 * (px(m, x + i - 1, y - 1) + px(m, x + i - 1, y + 1)) + 10 * px(m, x + i - 1, y);
                t1[i] = px(m, x + i - 1, y + 1) - px(m, x + i - 1, y - 1);
            }
            m->dx[(size_t)y * m->w + x] = (int16_t)(t0[2] - t0[0]);
            m->dy[(size_t)y * m->w + x] = (int16_t)(3 * (t1[0] + t1[2]) + 10 * t1[1]);
        }
    return 0;
}

static int top_level(int w, int h, int win, int max_level)
{
    if (w <= win || h <= win) return -1;
    int top = 0;
    while (top < max_level && (w + 1) / 2 > win && (h + 1) / 2 > win) w = (w + 1) / 2, h = (h + 1) / 2, top++;
    return top;
}

static int pyramid(level *lv, const uint8_t *img, int w, int h, int64_t step, int top, int with_derivatives)
{
    static const int k5[5] = {1, 4, 6, 4, 1};
    memset(lv, 0, sizeof(level) * MAX_LEVELS);
    lv[0].pix = img, lv[0].w = w, lv[0].h = h, lv[0].step = step;
    for (int l = 1; l <= top; l++) {
        const level *s = &lv[l - 1];
        level *d = &lv[l];
        d->w = (s->w + 1) / 2, d->h = (s->h + 1) / 2, d->step = d->w;
        d->own = (uint8_t *)malloc((size_t)d->w * d->h);
        if (!d->own) return -1;
        d->pix = d->own;
        for (int y = 0; y < d->h; y++)
            for (int x = 0; x < d->w; x++) {
                int acc = 128;
                for (int j = 0; j < 5; j++) {
                    int row = 0;
                    for (int i = 0; i < 5; i++) row += k5[i] * px(s, 2 * x + i - 2, 2 * y + j - 2);
                    acc += k5[j] * row;
                }
                d->own[(size_t)y * d->w + x] = (uint8_t)(acc >> 8);
            }
    }
    if (with_derivatives)
        for (int l = 0; l <= top; l++)
            if (scharr(&lv[l])) return -1;
    return 0;
}

static void release(level *lv)
{
    for (int l = 0; l < MAX_LEVELS; l++) free(lv[l].own), free(lv[l].dx), free(lv[l].dy);
}

static int outside(float fx, float fy, int win, const level *m)
{
    if (!isfinite(fx) || !isfinite(fy)) return 1;
    return fx < (float)-win || fx >= (float)m->w || fy < (float)-win || fy >= (float)m->h;
}

typedef struct { int w00, w01, w10, w11; } q14;

static q14 weights(float a, float b)
{
    q14 w;
    w.w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
    w.w01 = (int)rintf(a * (1.f - b) * 16384.f);
    w.w10 = (int)rintf((1.f - a) * b * 16384.f);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

static int gray_q5(const level *m, int x, int y, q14 w)
{
    return (px(m, x, y) * w.w00 + px(m, x + 1, y) * w.w01 + px(m, x, y + 1) * w.w10 + px(m, x + 1, y + 1) * w.w11 + 256) >> 9;
}

static int deriv_q5(const level *m, const int16_t *d, int x, int y, q14 w)
{
    return (at(m, d, x, y) * w.w00 + at(m, d, x + 1, y) * w.w01 + at(m, d, x, y + 1) * w.w10 + at(m, d, x + 1, y + 1) * w.w11 + 8192) >> 14;
}

typedef struct {
    int win, top, max_count;
    double eps2, min_eig;
    const level *I, *J;
    int *tI, *tx, *ty;   /* win x win each */
} setup;

typedef struct {
    float x, y, err;
    int status, lost_eig, lost_range, iters;
} tracked;

/* one feature: the template around `ref`, the search started at `init` on the top level */
static tracked feature(const setup *s, const float ref[2], const float init[2], uint8_t *why)
{
    const int win = s->win;
    const float half = (float)(win - 1) * 0.5f;
    tracked t = {0.f, 0.f, 0.f, 1, 0, 0, 0};
    for (int l = s->top; l >= 0; l--) {
        const level *I = &s->I[l], *J = &s->J[l];
        const float sc = ldexpf(1.f, -l);
        if (l == s->top)
            t.x = init[0] * sc, t.y = init[1] * sc;   /* OPTFLOW_USE_INITIAL_FLOW: nextPts scaled like prevPts */
        else
            t.x = 2.f * t.x, t.y = 2.f * t.y;
        const float tpx = ref[0] * sc - half, tpy = ref[1] * sc - half;
        const float tfx = floorf(tpx), tfy = floorf(tpy);
        if (outside(tfx, tfy, win, I)) {
            if (l == 0) t.status = 0, t.err = 0.f, t.lost_range++;
            if (why) why[l] = WHY_TEMPLATE;
            continue;
        }
        const int ix0 = (int)tfx, iy0 = (int)tfy;
        q14 w = weights(tpx - tfx, tpy - tfy);
        int64_t S11 = 0, S12 = 0, S22 = 0;
        for (int i = 0; i < win * win; i++) {
            const int x = ix0 + i % win, y = iy0 + i / win;
            s->tI[i] = gray_q5(I, x, y, w);
            s->tx[i] = deriv_q5(I, I->dx, x, y, w);
            s->ty[i] = deriv_q5(I, I->dy, x, y, w);
            S11 += (int64_t)s->tx[i] * s->tx[i], S12 += (int64_t)s->tx[i] * s->ty[i], S22 += (int64_t)s->ty[i] * s->ty[i];
        }
        const float A11 = (float)S11 * 0x1p-20f, A12 = (float)S12 * 0x1p-20f, A22 = (float)S22 * 0x1p-20f;
        float D = A11 * A22 - A12 * A12;
        const float min_eig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
        if ((double)min_eig < s->min_eig || D < FLT_EPSILON) {
            if (l == 0) t.status = 0, t.lost_eig++;
            if (why) why[l] = WHY_MIN_EIG;
            continue;
        }
        D = 1.f / D;
        float qx = t.x - half, qy = t.y - half, lastx = 0.f, lasty = 0.f;
        int code = WHY_COUNT;
        for (int j = 0; j < s->max_count; j++) {
            const float fx = floorf(qx), fy = floorf(qy);
            if (outside(fx, fy, win, J)) {
                if (l == 0) t.status = 0, t.lost_range++;
                code = WHY_RANGE;
                break;
            }
            if (l == 0) t.iters = j + 1;
            w = weights(qx - fx, qy - fy);
            int64_t B1 = 0, B2 = 0;
            for (int i = 0; i < win * win; i++) {
                const int diff = gray_q5(J, (int)fx + i % win, (int)fy + i / win, w) - s->tI[i];
                B1 += (int64_t)diff * s->tx[i], B2 += (int64_t)diff * s->ty[i];
            }
            const float b1 = (float)B1 * 0x1p-20f, b2 = (float)B2 * 0x1p-20f;
            const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
            qx += dx, qy += dy;
            t.x = qx + half, t.y = qy + half;
            if ((double)dx * dx + (double)dy * dy <= s->eps2) {
                code = WHY_EPSILON;
                break;
            }
            if (j > 0 && (double)fabsf(dx + lastx) < 0.01 && (double)fabsf(dy + lasty) < 0.01) {
                t.x -= dx * 0.5f, t.y -= dy * 0.5f;
                code = WHY_OSCILLATION;
                break;
            }
            lastx = dx, lasty = dy;
        }
        if (why) why[l] = (uint8_t)code;
        if (l == 0 && t.status) {
            const float ex = t.x - half, ey = t.y - half, fx = floorf(ex), fy = floorf(ey);
            if (outside(fx, fy, win, J)) {
                t.status = 0, t.lost_range++;
            } else {
                w = weights(ex - fx, ey - fy);
                int64_t E = 0;
                for (int i = 0; i < win * win; i++) {
                    const int diff = gray_q5(J, (int)fx + i % win, (int)fy + i / win, w) - s->tI[i];
                    E += diff < 0 ? -diff : diff;
                }
                t.err = (float)E / (float)(32 * win * win);
            }
        }
    }
    return t;
}

/* DistortVecPoints, reference src/utils.cpp:49-76, one point; cam = fx fy cx cy k1 k2 p1 p2 k3 (k3 read with five
 * coefficients only); a copy when k1 == 0 */
static void distort(const float *cam, int n_coef, float ux, float uy, float *out)
{
    const float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    const float k1 = cam[4], k2 = cam[5], p1 = cam[6], p2 = cam[7], k3 = n_coef == 5 ? cam[8] : 0.f;
    if (k1 == 0.f) {
        out[0] = ux, out[1] = uy;
        return;
    }
    const float fx_inv = (float)(1.0 / (double)fx), fy_inv = (float)(1.0 / (double)fy);
    const float x = (ux - cx) * fx_inv, y = (uy - cy) * fy_inv;
    const float r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const float xd = x * (1 + k1 * r2 + k2 * r4 + k3 * r6) + 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
    const float yd = y * (1 + k1 * r2 + k2 * r4 + k3 * r6) + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
    out[0] = fx * xd + cx, out[1] = fy * yd + cy;
}

/* The flow form.  pt_ref, pt_out, flow: cap x 2; pt_init: cap x 2 or NULL for pt_ref; status_in: cap bytes or NULL for all 1;
 * cam: nine floats (above) or NULL, and then pt_out_dist (cap x 2) is not written; status, status_raw: cap bytes; err: cap;
 * info: INFO_WORDS; iters (or NULL): cap int32; why (or NULL): cap x MAX_LEVELS bytes, as in tests/lk_ref.c.  Rows at or
 * beyond n (clamped to [0, cap]) and rows with status_in == 0 are zeroed; the latter are counted in info[6]. */
int lk_flow_ref_track(const uint8_t *ref, const uint8_t *cur, int32_t w, int32_t h, int64_t step_ref, int64_t step_cur,
                      int32_t half_patch, int32_t max_level, int32_t max_count, double epsilon, double min_eig_threshold,
                      float err_threshold, const float *cam, int32_t n_dist_coef, int32_t n, int32_t cap, const float *pt_ref,
                      const float *pt_init, const uint8_t *status_in, float *pt_out, float *pt_out_dist, uint8_t *status,
                      uint8_t *status_raw, float *err, float *flow, int32_t *info, int32_t *iters, uint8_t *why)
{
    const int win = 2 * half_patch + 1;
    const int top = top_level(w, h, win, max_level);
    if (top < 0 || top >= MAX_LEVELS) return -1;
    level I[MAX_LEVELS], J[MAX_LEVELS];
    int *t = (int *)malloc(sizeof(int) * 3 * (size_t)win * win);
    int rc = pyramid(I, ref, w, h, step_ref, top, 1);
    if (!rc) rc = pyramid(J, cur, w, h, step_cur, top, 0);
    else memset(J, 0, sizeof J);
    if (rc || !t) {
        release(I), release(J), free(t);
        return -2;
    }
    const setup s = {win, top, max_count, epsilon * epsilon, min_eig_threshold, I, J, t, t + win * win, t + 2 * win * win};
    n = n < 0 ? 0 : (n > cap ? cap : n);
    memset(info, 0, INFO_WORDS * sizeof(int32_t));
    info[0] = n, info[3] = top;
    for (int k = 0; k < cap; k++) {
        uint8_t *left = why ? why + (size_t)k * MAX_LEVELS : NULL;
        if (left) memset(left, WHY_NOT_VISITED, MAX_LEVELS);
        const int live = k < n && (!status_in || status_in[k] != 0);
        if (!live) {
            pt_out[2 * k] = pt_out[2 * k + 1] = flow[2 * k] = flow[2 * k + 1] = err[k] = 0.f;
            status[k] = status_raw[k] = 0;
            if (cam) pt_out_dist[2 * k] = pt_out_dist[2 * k + 1] = 0.f;
            if (iters) iters[k] = 0;
            if (k < n) info[6]++;
            continue;
        }
        const tracked r = feature(&s, pt_ref + 2 * k, (pt_init ? pt_init : pt_ref) + 2 * k, left);
        pt_out[2 * k] = r.x, pt_out[2 * k + 1] = r.y;
        err[k] = r.err;
        status_raw[k] = (uint8_t)r.status;
        status[k] = (uint8_t)(r.status && !(r.err >= err_threshold));
        flow[2 * k] = r.x - pt_ref[2 * k], flow[2 * k + 1] = r.y - pt_ref[2 * k + 1];
        if (cam) distort(cam, n_dist_coef, r.x, r.y, pt_out_dist + 2 * k);
        if (iters) iters[k] = r.iters;
        info[1] += r.status, info[2] += status[k], info[4] += r.lost_eig, info[5] += r.lost_range;
    }
    release(I), release(J), free(t);
    return 0;
}
