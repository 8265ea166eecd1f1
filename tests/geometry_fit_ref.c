/* geometry_fit_ref.c -- plain-C restatement of the device RANSAC fit (csrc/pagk_fit_kernel.h, include/pagk.h
 * pagk_geometry_fit).  Test infrastructure: the GPU result must equal this one byte for byte.  Built by the tests with
 * gcc -O2 -ffp-contract=off (one IEEE rounding per operation, like the library) and loaded with ctypes.
 *
 * Every step is written in the order the kernels evaluate it; the reductions restate the kernels' fixed tree (256
 * per-lane partial sums over a stride of 256, a shuffle tree inside each 64-lane wave, then (w0 + w1) + (w2 + w3)). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct gfr_params { /* the layout of pagk_fit_params */
    uint64_t seed;
    int32_t iters_H, iters_F;
    double thresh_H, thresh_F;
    double conf_H, conf_F;
} gfr_params;

enum { MAX_DRAWS = 64, LANES = 256, INFO_WORDS = 12 };

static uint64_t sm64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

uint64_t gfr_splitmix64(uint64_t x) { return sm64(x); }

/* index of draw `draw` of hypothesis `hyp` of model `model` (0 = H, 1 = F) among m points */
uint32_t gfr_draw(uint64_t seed, int model, uint32_t hyp, uint32_t draw, uint32_t m)
{
    const uint64_t z = sm64(seed ^ sm64(((uint64_t)model << 56) | ((uint64_t)hyp << 8) | (uint64_t)draw));
    return (uint32_t)(((z >> 32) * (uint64_t)m) >> 32);
}

/* the sample of one hypothesis: 4 (H) or 8 (F) distinct indices; 0 when MAX_DRAWS draws did not find them */
int gfr_sample(uint64_t seed, int model, uint32_t hyp, uint32_t m, int32_t *idx)
{
    const int s = model ? 8 : 4;
    uint32_t d = 0;
    for (int j = 0; j < s; j++) idx[j] = -1;
    for (int j = 0; j < s; j++) {
        for (;;) {
            if (d >= MAX_DRAWS) {
                for (int k = 0; k < s; k++) idx[k] = -1;
                return 0;
            }
            const int32_t c = (int32_t)gfr_draw(seed, model, hyp, d, m);
            d++;
            int dup = 0;
            for (int k = 0; k < j; k++) dup |= idx[k] == c;
            if (!dup) {
                idx[j] = c;
                break;
            }
        }
    }
    return 1;
}

static int finite9(const double *h)
{
    for (int k = 0; k < 9; k++)
        if (!isfinite(h[k])) return 0;
    return 1;
}

static void mat3_mul(const double *a, const double *b, double *c)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

/* normalisation from the sums of a point set: centroid to the origin, RMS distance sqrt(2).  0 when degenerate. */
static int norm_from_sums(double c, double sx, double sy, double sq, double *cx, double *cy, double *sc)
{
    *cx = sx / c;
    *cy = sy / c;
    const double mq = sq / c;
    const double var = mq - (*cx * *cx + *cy * *cy);
    if (!(var > 1e-12 * mq)) return 0;
    *sc = sqrt(2.0 / var);
    return 1;
}

/* T2^-1 * Mn * T1 (homography) or T2^T * Mn * T1 (fundamental) */
static void denormalise(int model, const double *mn, double cx1, double cy1, double s1, double cx2, double cy2, double s2,
                        double *out)
{
    const double T1[9] = {s1, 0.0, -s1 * cx1, 0.0, s1, -s1 * cy1, 0.0, 0.0, 1.0};
    double L[9];
    if (model == 0) {
        const double Ti[9] = {1.0 / s2, 0.0, cx2, 0.0, 1.0 / s2, cy2, 0.0, 0.0, 1.0};
        memcpy(L, Ti, sizeof L);
    } else {
        const double Tt[9] = {s2, 0.0, 0.0, 0.0, s2, 0.0, -s2 * cx2, -s2 * cy2, 1.0};
        memcpy(L, Tt, sizeof L);
    }
    double tmp[9];
    mat3_mul(mn, T1, tmp);
    mat3_mul(L, tmp, out);
}

/* rows of the linear systems, normalised coordinates (x, y) in image 1 -> (u, v) in image 2 */
static void h_rows(double x, double y, double u, double v, double *r1, double *r2)
{
    r1[0] = x, r1[1] = y, r1[2] = 1.0, r1[3] = 0.0, r1[4] = 0.0, r1[5] = 0.0, r1[6] = -(u * x), r1[7] = -(u * y), r1[8] = -u;
    r2[0] = 0.0, r2[1] = 0.0, r2[2] = 0.0, r2[3] = x, r2[4] = y, r2[5] = 1.0, r2[6] = -(v * x), r2[7] = -(v * y), r2[8] = -v;
}
static void f_row(double x, double y, double u, double v, double *r)
{
    r[0] = u * x, r[1] = u * y, r[2] = u, r[3] = v * x, r[4] = v * y, r[5] = v, r[6] = x, r[7] = y, r[8] = 1.0;
}

/* null vector of an 8x9 system (h[8] = 1) by Gaussian elimination with partial pivoting; 0 on a pivot at or below
 * 1e-6 of the largest |entry| */
static int null8x9(double *A, double *h)
{
    double mx = 0.0;
    for (int k = 0; k < 72; k++) mx = fabs(A[k]) > mx ? fabs(A[k]) : mx;
    for (int j = 0; j < 8; j++) {
        int p = j;
        double best = fabs(A[9 * j + j]);
        for (int r = j + 1; r < 8; r++)
            if (fabs(A[9 * r + j]) > best) best = fabs(A[9 * r + j]), p = r;
        if (!(best > 1e-6 * mx)) return 0;
        if (p != j)
            for (int c = 0; c < 9; c++) {
                const double t = A[9 * j + c];
                A[9 * j + c] = A[9 * p + c];
                A[9 * p + c] = t;
            }
        for (int r = j + 1; r < 8; r++) {
            const double f = A[9 * r + j] / A[9 * j + j];
            for (int c = j + 1; c < 9; c++) A[9 * r + c] = A[9 * r + c] - f * A[9 * j + c];
        }
    }
    h[8] = 1.0;
    for (int j = 7; j >= 0; j--) {
        double s = A[9 * j + 8];
        for (int c = j + 1; c < 8; c++) s = s + A[9 * j + c] * h[c];
        h[j] = -s / A[9 * j + j];
    }
    return 1;
}

/* three of the points a, b, c collinear: sin^2 of the angle at a <= 1e-6 (also: two of them equal) */
static int collinear(const double *a, const double *b, const double *c)
{
    const double bx = b[0] - a[0], by = b[1] - a[1], cx = c[0] - a[0], cy = c[1] - a[1];
    const double cr = bx * cy - by * cx;
    return cr * cr <= 1e-6 * ((bx * bx + by * by) * (cx * cx + cy * cy));
}

/* the minimal solve of one hypothesis: 1 and the (denormalised) model, or 0 = invalid */
int gfr_hypothesis(int model, uint64_t seed, uint32_t hyp, int32_t m, const float *p1, const float *p2, double *out)
{
    const int s = model ? 8 : 4;
    int32_t idx[8];
    if (!gfr_sample(seed, model, hyp, (uint32_t)m, idx)) return 0;
    double a[8][2], b[8][2];
    for (int j = 0; j < s; j++) {
        a[j][0] = (double)p1[2 * idx[j]], a[j][1] = (double)p1[2 * idx[j] + 1];
        b[j][0] = (double)p2[2 * idx[j]], b[j][1] = (double)p2[2 * idx[j] + 1];
    }
    if (model == 0) {
        static const int tri[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
        for (int t = 0; t < 4; t++)
            if (collinear(a[tri[t][0]], a[tri[t][1]], a[tri[t][2]])) return 0;
        for (int t = 0; t < 4; t++)
            if (collinear(b[tri[t][0]], b[tri[t][1]], b[tri[t][2]])) return 0;
    }
    double sx1 = 0.0, sy1 = 0.0, sq1 = 0.0, sx2 = 0.0, sy2 = 0.0, sq2 = 0.0;
    for (int j = 0; j < s; j++) {
        sx1 = sx1 + a[j][0], sy1 = sy1 + a[j][1], sq1 = sq1 + (a[j][0] * a[j][0] + a[j][1] * a[j][1]);
        sx2 = sx2 + b[j][0], sy2 = sy2 + b[j][1], sq2 = sq2 + (b[j][0] * b[j][0] + b[j][1] * b[j][1]);
    }
    double cx1, cy1, s1, cx2, cy2, s2;
    if (!norm_from_sums((double)s, sx1, sy1, sq1, &cx1, &cy1, &s1) ||
        !norm_from_sums((double)s, sx2, sy2, sq2, &cx2, &cy2, &s2))
        return 0;
    double A[72];
    for (int j = 0; j < s; j++) {
        const double x = (a[j][0] - cx1) * s1, y = (a[j][1] - cy1) * s1;
        const double u = (b[j][0] - cx2) * s2, v = (b[j][1] - cy2) * s2;
        if (model == 0)
            h_rows(x, y, u, v, A + 18 * j, A + 18 * j + 9);
        else
            f_row(x, y, u, v, A + 9 * j);
    }
    double hn[9];
    if (!null8x9(A, hn)) return 0;
    denormalise(model, hn, cx1, cy1, s1, cx2, cy2, s2, out);
    return finite9(out);
}

/* the consensus tests (squared threshold t2) */
static int h_inlier(const double *h, float fu1, float fv1, float fu2, float fv2, double t2)
{
    const double u1 = fu1, v1 = fv1, u2 = fu2, v2 = fv2;
    const double w = h[6] * u1 + h[7] * v1 + h[8];
    const double ex = u2 * w - (h[0] * u1 + h[1] * v1 + h[2]);
    const double ey = v2 * w - (h[3] * u1 + h[4] * v1 + h[5]);
    return ex * ex + ey * ey <= t2 * (w * w);
}
static int f_inlier(const double *f, float fu1, float fv1, float fu2, float fv2, double t2)
{
    const double u1 = fu1, v1 = fv1, u2 = fu2, v2 = fv2;
    const double a2 = f[0] * u1 + f[1] * v1 + f[2], b2 = f[3] * u1 + f[4] * v1 + f[5], c2 = f[6] * u1 + f[7] * v1 + f[8];
    const double n2 = a2 * u2 + b2 * v2 + c2;
    const double a1 = u2 * f[0] + v2 * f[3] + f[6], b1 = u2 * f[1] + v2 * f[4] + f[7], c1 = u2 * f[2] + v2 * f[5] + f[8];
    const double n1 = a1 * u1 + b1 * v1 + c1;
    return n2 * n2 <= t2 * (a2 * a2 + b2 * b2) && n1 * n1 <= t2 * (a1 * a1 + b1 * b1);
}
static int inlier(int model, const double *mdl, const float *p1, const float *p2, int k, double t2)
{
    return model == 0 ? h_inlier(mdl, p1[2 * k], p1[2 * k + 1], p2[2 * k], p2[2 * k + 1], t2)
                      : f_inlier(mdl, p1[2 * k], p1[2 * k + 1], p2[2 * k], p2[2 * k + 1], t2);
}

/* the kernels' fixed reduction tree over 256 lane partials (destroys p) */
static double tree256(double *p)
{
    for (int w = 0; w < 4; w++)
        for (int off = 32; off >= 1; off >>= 1)
            for (int l = 0; l < off; l++) p[64 * w + l] = p[64 * w + l] + p[64 * w + l + off];
    return (p[0] + p[64]) + (p[128] + p[192]);
}

/* log(x) for 0 < x < 1 with + - * / only (the same bits on every IEEE machine) */
double gfr_log(double x)
{
    int e = 0;
    double m = x;
    for (int k = 0; k < 1100 && m < 0.7071067811865476; k++) m = m * 2.0, e--;
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double term = s, sum = 0.0;
    for (int k = 0; k < 24; k++) {
        sum = sum + term / (double)(2 * k + 1);
        term = term * s2;
    }
    return (double)e * 0.6931471805599453 + 2.0 * sum;
}

/* ceil(log(1 - conf) / log(1 - w^s)), w = count / m */
int32_t gfr_adaptive(int32_t count, int32_t m, int s, double conf)
{
    if (count <= 0) return 0;
    const double w = (double)count / (double)m;
    double p = w;
    for (int k = 1; k < s; k++) p = p * w;
    const double den = 1.0 - p;
    if (!(den > 0.0)) return 1;
    if (!(den < 1.0)) return 2147483647;
    const double r = ceil(gfr_log(1.0 - conf) / gfr_log(den));
    if (!(r < 2147483647.0)) return 2147483647;
    return r < 1.0 ? 1 : (int32_t)r;
}

/* smallest eigenvector of the symmetric 9x9 M (upper triangle, 45 entries row by row) by inverse iteration on
 * M + 1e-12 tr(M) I: Cholesky, 10 steps from x_i = 1 / (i + 1), each normalised to unit length.  0 on failure. */
static int smallest_eigvec(const double *mu, double *x)
{
    double B[81], L[81];
    int k = 0;
    for (int i = 0; i < 9; i++)
        for (int j = i; j < 9; j++) B[9 * i + j] = B[9 * j + i] = mu[k++];
    double tr = 0.0;
    for (int i = 0; i < 9; i++) tr = tr + B[10 * i];
    if (!(tr > 0.0) || !isfinite(tr)) return 0;
    const double dl = 1e-12 * tr;
    for (int i = 0; i < 9; i++) B[10 * i] = B[10 * i] + dl;
    memset(L, 0, sizeof L);
    for (int j = 0; j < 9; j++) {
        double d = B[10 * j];
        for (int c = 0; c < j; c++) d = d - L[9 * j + c] * L[9 * j + c];
        if (!(d > 0.0)) return 0;
        L[10 * j] = sqrt(d);
        for (int i = j + 1; i < 9; i++) {
            double t = B[9 * i + j];
            for (int c = 0; c < j; c++) t = t - L[9 * i + c] * L[9 * j + c];
            L[9 * i + j] = t / L[10 * j];
        }
    }
    for (int i = 0; i < 9; i++) x[i] = 1.0 / (double)(i + 1);
    for (int it = 0; it < 10; it++) {
        double y[9];
        for (int i = 0; i < 9; i++) {
            double t = x[i];
            for (int c = 0; c < i; c++) t = t - L[9 * i + c] * y[c];
            y[i] = t / L[10 * i];
        }
        for (int i = 8; i >= 0; i--) {
            double t = y[i];
            for (int c = i + 1; c < 9; c++) t = t - L[9 * c + i] * x[c];
            x[i] = t / L[10 * i];
        }
        double nn = 0.0;
        for (int i = 0; i < 9; i++) nn = nn + x[i] * x[i];
        const double r = sqrt(nn);
        for (int i = 0; i < 9; i++) x[i] = x[i] / r;
    }
    return finite9(x);
}

/* F := F - (F v) v^T, v = the eigenvector of F^T F with the smallest eigenvalue (cyclic Jacobi, 10 sweeps) */
static void rank2(double *f)
{
    double G[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) G[3 * i + j] = f[i] * f[j] + f[3 + i] * f[3 + j] + f[6 + i] * f[6 + j];
    static const int pq[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int sw = 0; sw < 10; sw++)
        for (int r = 0; r < 3; r++) {
            const int p = pq[r][0], q = pq[r][1];
            if (G[3 * p + q] == 0.0) continue;
            const double th = (G[3 * q + q] - G[3 * p + p]) / (2.0 * G[3 * p + q]);
            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; k++) {
                const double gp = G[3 * k + p], gq = G[3 * k + q];
                G[3 * k + p] = c * gp - s * gq;
                G[3 * k + q] = s * gp + c * gq;
            }
            for (int k = 0; k < 3; k++) {
                const double gp = G[3 * p + k], gq = G[3 * q + k];
                G[3 * p + k] = c * gp - s * gq;
                G[3 * q + k] = s * gp + c * gq;
            }
            for (int k = 0; k < 3; k++) {
                const double vp = V[3 * k + p], vq = V[3 * k + q];
                V[3 * k + p] = c * vp - s * vq;
                V[3 * k + q] = s * vp + c * vq;
            }
        }
    int mi = 0;
    for (int i = 1; i < 3; i++)
        if (G[4 * i] < G[4 * mi]) mi = i;
    const double v[3] = {V[mi], V[3 + mi], V[6 + mi]};
    for (int r = 0; r < 3; r++) {
        const double w = f[3 * r] * v[0] + f[3 * r + 1] * v[1] + f[3 * r + 2] * v[2];
        for (int c = 0; c < 3; c++) f[3 * r + c] = f[3 * r + c] - w * v[c];
    }
}

/* scale to m[8] = 1; F falls back to the largest |entry| (first in row-major order) when |f33| <= 1e-12 max |entry|.
 * 0 when H cannot be scaled. */
static int scale_model(int model, double *h)
{
    double mx = 0.0;
    int im = 0;
    for (int k = 0; k < 9; k++)
        if (fabs(h[k]) > mx) mx = fabs(h[k]), im = k;
    int piv = 8;
    if (!(fabs(h[8]) > 1e-12 * mx)) {
        if (model == 0) return 0;
        piv = im;
    }
    const double d = h[piv];
    for (int k = 0; k < 9; k++) h[k] = h[k] / d;
    return finite9(h);
}

static int invert3(const double *h, double *o)
{
    const double c00 = h[4] * h[8] - h[5] * h[7], c01 = h[5] * h[6] - h[3] * h[8], c02 = h[3] * h[7] - h[4] * h[6];
    const double det = h[0] * c00 + h[1] * c01 + h[2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return 0;
    o[0] = c00 / det, o[1] = (h[2] * h[7] - h[1] * h[8]) / det, o[2] = (h[1] * h[5] - h[2] * h[4]) / det;
    o[3] = c01 / det, o[4] = (h[0] * h[8] - h[2] * h[6]) / det, o[5] = (h[2] * h[3] - h[0] * h[5]) / det;
    o[6] = c02 / det, o[7] = (h[1] * h[6] - h[0] * h[7]) / det, o[8] = (h[0] * h[4] - h[1] * h[3]) / det;
    return finite9(o);
}

/* refit of one model on the inliers of hypothesis `hm`; 1 and out (and for H: out + 9 = inverse) or 0 */
static int refit(int model, const double *hm, int32_t m, const float *p1, const float *p2, double t2, double *out)
{
    static double part[7][LANES];
    int32_t cnt = 0;
    memset(part, 0, sizeof part);
    for (int l = 0; l < LANES; l++)
        for (int k = l; k < m; k += LANES)
            if (inlier(model, hm, p1, p2, k, t2)) {
                const double x1 = p1[2 * k], y1 = p1[2 * k + 1], x2 = p2[2 * k], y2 = p2[2 * k + 1];
                cnt++;
                part[0][l] = part[0][l] + x1, part[1][l] = part[1][l] + y1, part[2][l] = part[2][l] + (x1 * x1 + y1 * y1);
                part[3][l] = part[3][l] + x2, part[4][l] = part[4][l] + y2, part[5][l] = part[5][l] + (x2 * x2 + y2 * y2);
            }
    if (cnt < (model ? 8 : 4)) return 0;
    double S[6];
    for (int k = 0; k < 6; k++) S[k] = tree256(part[k]);
    double cx1, cy1, s1, cx2, cy2, s2;
    if (!norm_from_sums((double)cnt, S[0], S[1], S[2], &cx1, &cy1, &s1) ||
        !norm_from_sums((double)cnt, S[3], S[4], S[5], &cx2, &cy2, &s2))
        return 0;
    static double mp[45][LANES];
    memset(mp, 0, sizeof mp);
    for (int l = 0; l < LANES; l++)
        for (int k = l; k < m; k += LANES)
            if (inlier(model, hm, p1, p2, k, t2)) {
                const double x = ((double)p1[2 * k] - cx1) * s1, y = ((double)p1[2 * k + 1] - cy1) * s1;
                const double u = ((double)p2[2 * k] - cx2) * s2, v = ((double)p2[2 * k + 1] - cy2) * s2;
                double r1[9], r2[9];
                if (model == 0)
                    h_rows(x, y, u, v, r1, r2);
                else
                    f_row(x, y, u, v, r1);
                int e = 0;
                for (int i = 0; i < 9; i++)
                    for (int j = i; j < 9; j++, e++) {
                        mp[e][l] = mp[e][l] + r1[i] * r1[j];
                        if (model == 0) mp[e][l] = mp[e][l] + r2[i] * r2[j];
                    }
            }
    double M[45], x[9];
    for (int e = 0; e < 45; e++) M[e] = tree256(mp[e]);
    if (!smallest_eigvec(M, x)) return 0;
    if (model == 1) rank2(x);
    denormalise(model, x, cx1, cy1, s1, cx2, cy2, s2, out);
    if (!finite9(out) || !scale_model(model, out)) return 0;
    if (model == 0 && !invert3(out, out + 9)) return 0;
    return 1;
}

/* the whole fit.  models: H21 | H12 | F21 (27 doubles); masks: n each (may be NULL); info: 12 words; hyp_counts:
 * iters_H + iters_F (may be NULL).  status may be NULL (every point takes part). */
int gfr_fit(const gfr_params *P, int32_t n, const float *pts1, const float *pts2, const uint8_t *status, double *models,
            uint8_t *mask_H, uint8_t *mask_F, int32_t *info, int32_t *hyp_counts)
{
    float *p1 = malloc(sizeof(float) * 2 * (size_t)(n > 0 ? n : 1)), *p2 = malloc(sizeof(float) * 2 * (size_t)(n > 0 ? n : 1));
    int32_t *idx = malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    int32_t m = 0;
    for (int i = 0; i < n; i++) {
        if (mask_H) mask_H[i] = 0;
        if (mask_F) mask_F[i] = 0;
        if (status && !status[i]) continue;
        p1[2 * m] = pts1[2 * i], p1[2 * m + 1] = pts1[2 * i + 1];
        p2[2 * m] = pts2[2 * i], p2[2 * m + 1] = pts2[2 * i + 1];
        idx[m++] = i;
    }
    memset(models, 0, 27 * sizeof(double));
    for (int k = 0; k < INFO_WORDS; k++) info[k] = 0;
    info[1] = info[7] = -1;
    for (int model = 0; model < 2; model++) {
        const int iters = model ? P->iters_F : P->iters_H, s = model ? 8 : 4;
        const double th = model ? P->thresh_F : P->thresh_H, t2 = th * th;
        int32_t *ci = info + 6 * model;
        int32_t *hc = hyp_counts ? hyp_counts + (model ? P->iters_H : 0) : NULL;
        if (m <= 8) {
            if (hc)
                for (int h = 0; h < iters; h++) hc[h] = -1;
            continue;
        }
        double best_m[9], hm[9];
        int32_t best = -1, best_c = -1, valid = 0;
        for (int h = 0; h < iters; h++) {
            int32_t c = -1;
            if (gfr_hypothesis(model, P->seed, (uint32_t)h, m, p1, p2, hm)) {
                c = 0;
                for (int k = 0; k < m; k++) c += inlier(model, hm, p1, p2, k, t2);
                valid++;
                if (c > best_c) best_c = c, best = h, memcpy(best_m, hm, sizeof hm);
            }
            if (hc) hc[h] = c;
        }
        ci[1] = best, ci[2] = best < 0 ? 0 : best_c, ci[4] = valid;
        ci[5] = best < 0 ? 0 : gfr_adaptive(best_c, m, s, model ? P->conf_F : P->conf_H);
        if (best < 0) continue;
        double out[18];
        if (!refit(model, best_m, m, p1, p2, t2, out)) continue;
        int32_t rc = 0;
        uint8_t *mk = model ? mask_F : mask_H;
        for (int k = 0; k < m; k++) {
            const int in = inlier(model, out, p1, p2, k, t2);
            rc += in;
            if (mk) mk[idx[k]] = (uint8_t)in;
        }
        ci[0] = 1, ci[3] = rc;
        if (model == 0)
            memcpy(models, out, 18 * sizeof(double));
        else
            memcpy(models + 18, out, 9 * sizeof(double));
    }
    free(p1), free(p2), free(idx);
    return m;
}
