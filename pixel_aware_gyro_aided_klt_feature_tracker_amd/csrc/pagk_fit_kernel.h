// pagk_fit_kernel.h -- the RANSAC fits in front of GyroAidedTracker::GeometryValidation's scoring loops (reference
// src/gyro_aided_tracker.cpp:429-480, 589-768): cv::findHomography(vPts1, vPts2, cv::RANSAC, 3) (:597) and
// cv::findFundamentalMat(vPts1, vPts2, CV_FM_RANSAC, 3., 0.99) (:691), restated as a DETERMINISTIC fit.  OpenCV's
// random generator, minimal solvers and Levenberg-Marquardt refinement are not reproduced (include/pagk.h); what the
// kernels promise is the bits of the plain-C restatement in tests/geometry_fit_ref.c for the same seed and inputs.
// All model arithmetic is f64, one IEEE rounding per operation (-ffp-contract=off), with f64 `/` and sqrt correctly
// rounded; every reduction below has a fixed order, restated in that file.
//
// Launch sequence of one fit (all on the context stream, no host synchronisation, graph-capturable):
//   k_fit_compact   1 x 1024   status-true correspondences, in index order (ballot scan), -> m; resets the per-model
//                              best keys / valid counters, the models, the info words and the caller's masks
//   k_fit_hyp       ceil(iters_H / 16) + ceil(iters_F / 16) x 256
//                              four hypotheses per wave: lanes 0-3 draw and solve one each (model -> LDS and the
//                              hypothesis array), then the wave streams all m correspondences once per hypothesis and
//                              reduces the integer count; lane 0 stores it and atomicMax'es (count << 32) | ~index
//   k_fit_refit     2 x 256    one workgroup per model: re-test the best hypothesis, sums for the normalisation, the
//                              9x9 normal matrix (per-lane partials over a stride of 256, a shuffle tree inside each
//                              wave, then (w0 + w1) + (w2 + w3)), lane 0 solves it, every lane writes the final masks
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pagk {

constexpr int kFitHypPerWave = 4;                     // hypotheses one wave solves (lanes 0-3) and then counts
constexpr int kFitHypPerBlock = 4 * kFitHypPerWave;   // four waves per workgroup
constexpr int kFitMaxDraws = 64;                      // draws per hypothesis before its sample is given up
constexpr int kFitInfoWords = 12;                     // PAGK_FIT_INFO_WORDS

struct FitHdr {                   // device header of a fit (workspace)
    int32_t m;                    // correspondences that take part
    int32_t valid[2];             // valid hypotheses per model
    int32_t pad;
    unsigned long long key[2];    // best (count << 32) | ~index per model; 0 = none valid
};

struct FitArgs {
    const float *p1, *p2;         // compacted correspondences, m x 2
    const int32_t *idx;           // their original indices
    FitHdr *hdr;
    double *hyp_models;           // (iters_H + iters_F) x 9
    int32_t *hyp_counts;          // iters_H + iters_F
    double *models;               // H21 | H12 | F21
    int32_t *info;                // kFitInfoWords
    uint8_t *mask_H, *mask_F;     // original indexing, may be null
    unsigned long long seed;
    int32_t iters[2];
    int32_t nblk_H;               // workgroups of k_fit_hyp that serve the homography
    double t2[2];                 // squared thresholds
    double conf[2];
};

__device__ __forceinline__ unsigned long long fit_sm64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ int32_t fit_draw(unsigned long long seed, int model, uint32_t hyp, uint32_t draw, uint32_t m)
{
    const unsigned long long z =
        fit_sm64(seed ^ fit_sm64(((unsigned long long)model << 56) | ((unsigned long long)hyp << 8) | draw));
    return (int32_t)(((z >> 32) * (unsigned long long)m) >> 32);
}

__device__ __forceinline__ int fit_sample_size(int model) { return model == 2 ? 5 : model ? 8 : 4; }

// s = 4 (H), 8 (F) or 5 (E, model 2: pagk_pose_kernel.h) distinct indices; false (and -1s) when kFitMaxDraws draws did not
// find them
__device__ bool fit_sample(unsigned long long seed, int model, uint32_t hyp, uint32_t m, int32_t *idx)
{
    const int s = fit_sample_size(model);
    uint32_t d = 0;
    for (int j = 0; j < 8; j++) idx[j] = -1;
    for (int j = 0; j < s; j++) {
        for (;;) {
            if (d >= (uint32_t)kFitMaxDraws) {
                for (int k = 0; k < 8; k++) idx[k] = -1;
                return false;
            }
            const int32_t c = fit_draw(seed, model, hyp, d, m);
            d++;
            bool dup = false;
            for (int k = 0; k < j; k++) dup |= idx[k] == c;
            if (!dup) {
                idx[j] = c;
                break;
            }
        }
    }
    return true;
}

__device__ __forceinline__ bool fit_finite9(const double *h)
{
    bool ok = true;
    for (int k = 0; k < 9; k++) ok &= isfinite(h[k]);
    return ok;
}

__device__ __forceinline__ void fit_mat3_mul(const double *a, const double *b, double *c)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// centroid to the origin, RMS distance sqrt(2), from the sums of a point set
__device__ __forceinline__ bool fit_norm(double c, double sx, double sy, double sq, double &cx, double &cy, double &sc)
{
    cx = sx / c;
    cy = sy / c;
    const double mq = sq / c;
    const double var = mq - (cx * cx + cy * cy);
    if (!(var > 1e-12 * mq)) return false;
    sc = sqrt(2.0 / var);
    return true;
}

__device__ void fit_denormalise(int model, const double *mn, double cx1, double cy1, double s1, double cx2, double cy2,
                                double s2, double *out)
{
    const double T1[9] = {s1, 0.0, -s1 * cx1, 0.0, s1, -s1 * cy1, 0.0, 0.0, 1.0};
    double L[9];
    if (model == 0) {
        const double i2 = 1.0 / s2;
        L[0] = i2, L[1] = 0.0, L[2] = cx2, L[3] = 0.0, L[4] = i2, L[5] = cy2, L[6] = 0.0, L[7] = 0.0, L[8] = 1.0;
    } else {
        L[0] = s2, L[1] = 0.0, L[2] = 0.0, L[3] = 0.0, L[4] = s2, L[5] = 0.0, L[6] = -s2 * cx2, L[7] = -s2 * cy2, L[8] = 1.0;
    }
    double tmp[9];
    fit_mat3_mul(mn, T1, tmp);
    fit_mat3_mul(L, tmp, out);
}

__device__ __forceinline__ void fit_h_rows(double x, double y, double u, double v, double *r1, double *r2)
{
    r1[0] = x, r1[1] = y, r1[2] = 1.0, r1[3] = 0.0, r1[4] = 0.0, r1[5] = 0.0, r1[6] = -(u * x), r1[7] = -(u * y), r1[8] = -u;
    r2[0] = 0.0, r2[1] = 0.0, r2[2] = 0.0, r2[3] = x, r2[4] = y, r2[5] = 1.0, r2[6] = -(v * x), r2[7] = -(v * y), r2[8] = -v;
}
__device__ __forceinline__ void fit_f_row(double x, double y, double u, double v, double *r)
{
    r[0] = u * x, r[1] = u * y, r[2] = u, r[3] = v * x, r[4] = v * y, r[5] = v, r[6] = x, r[7] = y, r[8] = 1.0;
}

// null vector (h[8] = 1) of an 8x9 system, Gaussian elimination with partial pivoting; false on a pivot at or below
// 1e-6 of the largest |entry|
__device__ bool fit_null8x9(double *A, double *h)
{
    double mx = 0.0;
    for (int k = 0; k < 72; k++) mx = fabs(A[k]) > mx ? fabs(A[k]) : mx;
    for (int j = 0; j < 8; j++) {
        int p = j;
        double best = fabs(A[9 * j + j]);
        for (int r = j + 1; r < 8; r++)
            if (fabs(A[9 * r + j]) > best) best = fabs(A[9 * r + j]), p = r;
        if (!(best > 1e-6 * mx)) return false;
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
    return true;
}

// sin^2 of the angle at a <= 1e-6 (two of the points equal included)
__device__ __forceinline__ bool fit_collinear(const double *a, const double *b, const double *c)
{
    const double bx = b[0] - a[0], by = b[1] - a[1], cx = c[0] - a[0], cy = c[1] - a[1];
    const double cr = bx * cy - by * cx;
    return cr * cr <= 1e-6 * ((bx * bx + by * by) * (cx * cx + cy * cy));
}

// the minimal solve of one hypothesis (denormalised model), false = invalid
__device__ bool fit_hypothesis(int model, unsigned long long seed, uint32_t hyp, int32_t m, const float *p1,
                               const float *p2, double *out)
{
    const int s = model ? 8 : 4;
    int32_t idx[8];
    if (!fit_sample(seed, model, hyp, (uint32_t)m, idx)) return false;
    double a[8][2], b[8][2];
    for (int j = 0; j < s; j++) {
        a[j][0] = (double)p1[2 * idx[j]], a[j][1] = (double)p1[2 * idx[j] + 1];
        b[j][0] = (double)p2[2 * idx[j]], b[j][1] = (double)p2[2 * idx[j] + 1];
    }
    if (model == 0) {
        const int tri[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
        for (int t = 0; t < 4; t++)
            if (fit_collinear(a[tri[t][0]], a[tri[t][1]], a[tri[t][2]])) return false;
        for (int t = 0; t < 4; t++)
            if (fit_collinear(b[tri[t][0]], b[tri[t][1]], b[tri[t][2]])) return false;
    }
    double sx1 = 0.0, sy1 = 0.0, sq1 = 0.0, sx2 = 0.0, sy2 = 0.0, sq2 = 0.0;
    for (int j = 0; j < s; j++) {
        sx1 = sx1 + a[j][0], sy1 = sy1 + a[j][1], sq1 = sq1 + (a[j][0] * a[j][0] + a[j][1] * a[j][1]);
        sx2 = sx2 + b[j][0], sy2 = sy2 + b[j][1], sq2 = sq2 + (b[j][0] * b[j][0] + b[j][1] * b[j][1]);
    }
    double cx1, cy1, s1, cx2, cy2, s2;
    if (!fit_norm((double)s, sx1, sy1, sq1, cx1, cy1, s1) || !fit_norm((double)s, sx2, sy2, sq2, cx2, cy2, s2))
        return false;
    double A[72];
    for (int j = 0; j < s; j++) {
        const double x = (a[j][0] - cx1) * s1, y = (a[j][1] - cy1) * s1;
        const double u = (b[j][0] - cx2) * s2, v = (b[j][1] - cy2) * s2;
        if (model == 0)
            fit_h_rows(x, y, u, v, A + 18 * j, A + 18 * j + 9);
        else
            fit_f_row(x, y, u, v, A + 9 * j);
    }
    double hn[9];
    if (!fit_null8x9(A, hn)) return false;
    fit_denormalise(model, hn, cx1, cy1, s1, cx2, cy2, s2, out);
    return fit_finite9(out);
}

// consensus: H |p2 w - H p1|^2 <= t2 w^2 (w = third row . p1: the squared transfer error without its division);
// F both squared point-to-epipolar-line distances, num^2 <= t2 (a^2 + b^2)
__device__ __forceinline__ bool fit_inlier(int model, const double *f, float fu1, float fv1, float fu2, float fv2, double t2)
{
    const double u1 = fu1, v1 = fv1, u2 = fu2, v2 = fv2;
    if (model == 0) {
        const double w = f[6] * u1 + f[7] * v1 + f[8];
        const double ex = u2 * w - (f[0] * u1 + f[1] * v1 + f[2]);
        const double ey = v2 * w - (f[3] * u1 + f[4] * v1 + f[5]);
        return ex * ex + ey * ey <= t2 * (w * w);
    }
    const double a2 = f[0] * u1 + f[1] * v1 + f[2], b2 = f[3] * u1 + f[4] * v1 + f[5], c2 = f[6] * u1 + f[7] * v1 + f[8];
    const double n2 = a2 * u2 + b2 * v2 + c2;
    const double a1 = u2 * f[0] + v2 * f[3] + f[6], b1 = u2 * f[1] + v2 * f[4] + f[7], c1 = u2 * f[2] + v2 * f[5] + f[8];
    const double n1 = a1 * u1 + b1 * v1 + c1;
    return n2 * n2 <= t2 * (a2 * a2 + b2 * b2) && n1 * n1 <= t2 * (a1 * a1 + b1 * b1);
}

// log(x), 0 < x < 1, with + - * / only
__device__ double fit_log(double x)
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

// OpenCV's adaptive iteration count ceil(log(1 - conf) / log(1 - w^s)), w = count / m
__device__ int32_t fit_adaptive(int32_t count, int32_t m, int s, double conf)
{
    if (count <= 0) return 0;
    const double w = (double)count / (double)m;
    double p = w;
    for (int k = 1; k < s; k++) p = p * w;
    const double den = 1.0 - p;
    if (!(den > 0.0)) return 1;
    if (!(den < 1.0)) return 2147483647;
    const double r = ceil(fit_log(1.0 - conf) / fit_log(den));
    if (!(r < 2147483647.0)) return 2147483647;
    return r < 1.0 ? 1 : (int32_t)r;
}

// smallest eigenvector of the symmetric 9x9 (upper triangle, 45 entries row by row): inverse iteration on
// M + 1e-12 tr(M) I, Cholesky, 10 steps from x_i = 1 / (i + 1), each normalised
__device__ bool fit_smallest_eigvec(const double *mu, double *x)
{
    double B[81], L[81];
    int k = 0;
    for (int i = 0; i < 9; i++)
        for (int j = i; j < 9; j++) B[9 * i + j] = B[9 * j + i] = mu[k++];
    double tr = 0.0;
    for (int i = 0; i < 9; i++) tr = tr + B[10 * i];
    if (!(tr > 0.0) || !isfinite(tr)) return false;
    const double dl = 1e-12 * tr;
    for (int i = 0; i < 9; i++) B[10 * i] = B[10 * i] + dl;
    for (int i = 0; i < 81; i++) L[i] = 0.0;
    for (int j = 0; j < 9; j++) {
        double d = B[10 * j];
        for (int c = 0; c < j; c++) d = d - L[9 * j + c] * L[9 * j + c];
        if (!(d > 0.0)) return false;
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
    return fit_finite9(x);
}

// rank 2: F := F - (F v) v^T, v = eigenvector of F^T F with the smallest eigenvalue (cyclic Jacobi, 10 sweeps)
__device__ void fit_rank2(double *f)
{
    double G[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) G[3 * i + j] = f[i] * f[j] + f[3 + i] * f[3 + j] + f[6 + i] * f[6 + j];
    for (int sw = 0; sw < 10; sw++)
        for (int r = 0; r < 3; r++) {
            const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2;
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

// m[8] = 1; F falls back to the largest |entry| (first in row-major order) when |f33| <= 1e-12 max |entry|
__device__ bool fit_scale(int model, double *h)
{
    double mx = 0.0;
    int im = 0;
    for (int k = 0; k < 9; k++)
        if (fabs(h[k]) > mx) mx = fabs(h[k]), im = k;
    int piv = 8;
    if (!(fabs(h[8]) > 1e-12 * mx)) {
        if (model == 0) return false;
        piv = im;
    }
    const double d = h[piv];
    for (int k = 0; k < 9; k++) h[k] = h[k] / d;
    return fit_finite9(h);
}

__device__ bool fit_invert3(const double *h, double *o)
{
    const double c00 = h[4] * h[8] - h[5] * h[7], c01 = h[5] * h[6] - h[3] * h[8], c02 = h[3] * h[7] - h[4] * h[6];
    const double det = h[0] * c00 + h[1] * c01 + h[2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return false;
    o[0] = c00 / det, o[1] = (h[2] * h[7] - h[1] * h[8]) / det, o[2] = (h[1] * h[5] - h[2] * h[4]) / det;
    o[3] = c01 / det, o[4] = (h[0] * h[8] - h[2] * h[6]) / det, o[5] = (h[2] * h[3] - h[0] * h[5]) / det;
    o[6] = c02 / det, o[7] = (h[1] * h[6] - h[0] * h[7]) / det, o[8] = (h[0] * h[4] - h[1] * h[3]) / det;
    return fit_finite9(o);
}

// the fixed tree inside a wave: p[l] += p[l + off] for off = 32 .. 1; lane 0 holds the result
__device__ __forceinline__ double fit_wave_sum(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ int fit_wave_isum(int v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---- kernels ------------------------------------------------------------------------------------------------------
// k_fit_compact: one workgroup of 1024; n may be 0.  status may be null.
__device__ __forceinline__ void fit_compact_body(int32_t n, const float *pts1, const float *pts2, const uint8_t *status,
                                                 float *p1, float *p2, int32_t *idx, FitHdr *hdr, double *models,
                                                 int32_t *info, uint8_t *mask_H, uint8_t *mask_F)
{
    __shared__ int32_t wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 27) models[tid] = 0.0;
    if (tid < kFitInfoWords) info[tid] = (tid == 1 || tid == 7) ? -1 : 0;
    if (tid < 2) hdr->key[tid] = 0ull, hdr->valid[tid] = 0;
    int32_t base = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + tid;
        const bool take = i < n && (!status || status[i] != 0);
        if (i < n) {
            if (mask_H) mask_H[i] = 0;
            if (mask_F) mask_F[i] = 0;
        }
        const unsigned long long bal = __ballot(take);
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int32_t off = base, tot = 0;
        for (int w = 0; w < 16; w++) {
            off += w < wave ? wtot[w] : 0;
            tot += wtot[w];
        }
        __syncthreads();
        if (take) {
            const int32_t o = off + __popcll(bal & ((1ull << lane) - 1ull));
            p1[2 * o] = pts1[2 * i], p1[2 * o + 1] = pts1[2 * i + 1];
            p2[2 * o] = pts2[2 * i], p2[2 * o + 1] = pts2[2 * i + 1];
            idx[o] = i;
        }
        base += tot;
    }
    if (tid == 0) hdr->m = base;
}

__global__ void __launch_bounds__(1024) k_fit_compact(int32_t n, const float *pts1, const float *pts2,
                                                      const uint8_t *status, float *p1, float *p2, int32_t *idx,
                                                      FitHdr *hdr, double *models, int32_t *info, uint8_t *mask_H,
                                                      uint8_t *mask_F)
{
    fit_compact_body(n, pts1, pts2, status, p1, p2, idx, hdr, models, info, mask_H, mask_F);
}

// (workgroup blockIdx.x of a fit's hypotheses: the same numbering in k_fit_hyp and in every camera of its batched form)
__device__ __forceinline__ void fit_hyp_body(const FitArgs &a)
{
    __shared__ double mdl[kFitHypPerBlock][9];
    __shared__ int32_t ok[kFitHypPerBlock];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int model = (int)blockIdx.x < a.nblk_H ? 0 : 1;
    const int first = (model ? (int)blockIdx.x - a.nblk_H : (int)blockIdx.x) * kFitHypPerBlock + wave * kFitHypPerWave;
    const int iters = a.iters[model], hoff = model ? a.iters[0] : 0;
    const int32_t m = a.hdr->m;
    if (m <= 8) {  // nothing is fitted (:445)
        if (lane < kFitHypPerWave && first + lane < iters) a.hyp_counts[hoff + first + lane] = -1;
        return;
    }
    if (lane < kFitHypPerWave) {
        const int h = first + lane;
        double out[9];
        bool v = false;
        if (h < iters) v = fit_hypothesis(model, a.seed, (uint32_t)h, m, a.p1, a.p2, out);
        ok[wave * kFitHypPerWave + lane] = v;
        if (v)
            for (int k = 0; k < 9; k++) {
                mdl[wave * kFitHypPerWave + lane][k] = out[k];
                a.hyp_models[9 * (size_t)(hoff + h) + k] = out[k];
            }
    }
    __syncthreads();
    const double t2 = a.t2[model];
    for (int j = 0; j < kFitHypPerWave; j++) {
        const int h = first + j;
        if (h >= iters) break;
        if (!ok[wave * kFitHypPerWave + j]) {
            if (lane == 0) a.hyp_counts[hoff + h] = -1;
            continue;
        }
        double f[9];
        for (int k = 0; k < 9; k++) f[k] = mdl[wave * kFitHypPerWave + j][k];
        int c = 0;
        for (int k = lane; k < m; k += 64)
            c += fit_inlier(model, f, a.p1[2 * k], a.p1[2 * k + 1], a.p2[2 * k], a.p2[2 * k + 1], t2) ? 1 : 0;
        c = fit_wave_isum(c);
        if (lane == 0) {
            a.hyp_counts[hoff + h] = c;
            atomicMax(&a.hdr->key[model], ((unsigned long long)(uint32_t)c << 32) | (unsigned long long)(~(uint32_t)h));
            atomicAdd(&a.hdr->valid[model], 1);
        }
    }
}

__global__ void __launch_bounds__(256) k_fit_hyp(FitArgs a) { fit_hyp_body(a); }

__device__ __forceinline__ void fit_refit_body(const FitArgs &a)
{
    __shared__ double red[4][45];
    __shared__ int32_t ired[4];
    __shared__ double res[18];
    __shared__ int32_t res_ok;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int model = blockIdx.x, s = model ? 8 : 4;
    const int32_t m = a.hdr->m;
    int32_t *info = a.info + 6 * model;
    if (m <= 8) return;  // k_fit_compact left "no model"
    const unsigned long long key = a.hdr->key[model];
    const int32_t best = key ? (int32_t)~(uint32_t)(key & 0xffffffffull) : -1;
    const int32_t bc = key ? (int32_t)(key >> 32) : 0;
    if (tid == 0) {
        info[1] = best, info[2] = bc, info[4] = a.hdr->valid[model];
        info[5] = best < 0 ? 0 : fit_adaptive(bc, m, s, a.conf[model]);
    }
    if (best < 0) return;
    const double t2 = a.t2[model];
    double hm[9];
    const int hoff = model ? a.iters[0] : 0;
    for (int k = 0; k < 9; k++) hm[k] = a.hyp_models[9 * (size_t)(hoff + best) + k];
    // pass A: the inliers' sums for the normalisation
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    for (int k = tid; k < m; k += 256) {
        const float fx1 = a.p1[2 * k], fy1 = a.p1[2 * k + 1], fx2 = a.p2[2 * k], fy2 = a.p2[2 * k + 1];
        if (fit_inlier(model, hm, fx1, fy1, fx2, fy2, t2)) {
            const double x1 = fx1, y1 = fy1, x2 = fx2, y2 = fy2;
            cnt++;
            S[0] = S[0] + x1, S[1] = S[1] + y1, S[2] = S[2] + (x1 * x1 + y1 * y1);
            S[3] = S[3] + x2, S[4] = S[4] + y2, S[5] = S[5] + (x2 * x2 + y2 * y2);
        }
    }
    for (int e = 0; e < 6; e++) {
        const double v = fit_wave_sum(S[e]);
        if (lane == 0) red[wave][e] = v;
    }
    cnt = fit_wave_isum(cnt);
    if (lane == 0) ired[wave] = cnt;
    __syncthreads();
    cnt = ired[0] + ired[1] + ired[2] + ired[3];
    for (int e = 0; e < 6; e++) S[e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    double cx1, cy1, s1, cx2, cy2, s2;
    if (cnt < s || !fit_norm((double)cnt, S[0], S[1], S[2], cx1, cy1, s1) ||
        !fit_norm((double)cnt, S[3], S[4], S[5], cx2, cy2, s2))
        return;  // uniform: every lane read the same sums
    __syncthreads();  // red[] is reused below
    // pass B: the normal matrix (upper triangle, 45 entries row by row)
    double M[45];
    for (int e = 0; e < 45; e++) M[e] = 0.0;
    for (int k = tid; k < m; k += 256) {
        const float fx1 = a.p1[2 * k], fy1 = a.p1[2 * k + 1], fx2 = a.p2[2 * k], fy2 = a.p2[2 * k + 1];
        if (!fit_inlier(model, hm, fx1, fy1, fx2, fy2, t2)) continue;
        const double x = ((double)fx1 - cx1) * s1, y = ((double)fy1 - cy1) * s1;
        const double u = ((double)fx2 - cx2) * s2, v = ((double)fy2 - cy2) * s2;
        double r1[9], r2[9];
        if (model == 0)
            fit_h_rows(x, y, u, v, r1, r2);
        else
            fit_f_row(x, y, u, v, r1);
        int e = 0;
        for (int i = 0; i < 9; i++)
            for (int j = i; j < 9; j++, e++) {
                M[e] = M[e] + r1[i] * r1[j];
                if (model == 0) M[e] = M[e] + r2[i] * r2[j];
            }
    }
    for (int e = 0; e < 45; e++) {
        const double v = fit_wave_sum(M[e]);
        if (lane == 0) red[wave][e] = v;
    }
    __syncthreads();
    if (tid == 0) {
        for (int e = 0; e < 45; e++) M[e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
        double x[9], out[18];
        bool good = fit_smallest_eigvec(M, x);
        if (good) {
            if (model == 1) fit_rank2(x);
            fit_denormalise(model, x, cx1, cy1, s1, cx2, cy2, s2, out);
            good = fit_finite9(out) && fit_scale(model, out);
            if (good && model == 0) good = fit_invert3(out, out + 9);
        }
        res_ok = good;
        if (good)
            for (int k = 0; k < 18; k++) res[k] = out[k];
    }
    __syncthreads();
    if (!res_ok) return;
    double f[9];
    for (int k = 0; k < 9; k++) f[k] = res[k];
    uint8_t *mk = model ? a.mask_F : a.mask_H;
    int rc = 0;
    for (int k = tid; k < m; k += 256) {
        const bool in = fit_inlier(model, f, a.p1[2 * k], a.p1[2 * k + 1], a.p2[2 * k], a.p2[2 * k + 1], t2);
        rc += in ? 1 : 0;
        if (mk) mk[a.idx[k]] = in ? 1 : 0;
    }
    rc = fit_wave_isum(rc);
    __syncthreads();  // ired[] of pass A has been read by every lane
    if (lane == 0) ired[wave] = rc;
    __syncthreads();
    if (tid == 0) {
        info[0] = 1;
        info[3] = ired[0] + ired[1] + ired[2] + ired[3];
    }
    if (tid < (model ? 9 : 18)) a.models[(model ? 18 : 0) + tid] = res[tid];
}

__global__ void __launch_bounds__(256) k_fit_refit(FitArgs a) { fit_refit_body(a); }

// the drawn index sets of hypotheses [first, first + count) (pagk_selftest_fit_samples)
__global__ void __launch_bounds__(256) k_fit_samples(unsigned long long seed, int model, int32_t m, int32_t first,
                                                     int32_t count, int32_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int s = fit_sample_size(model);
    int32_t idx[8];
    fit_sample(seed, model, (uint32_t)(first + i), (uint32_t)m, idx);
    for (int j = 0; j < s; j++) out[(size_t)s * i + j] = idx[j];
}

// the device end of GeometryValidation (:462-480) after k_geometry_scores_fit: model choice (pagk_geometry_select), the
// chosen model's outliers cleared in the caller's status, cnt_inlier and the chosen score.  Nothing happens unless
// m > 8 and at least one model was fitted.
__device__ __forceinline__ void fit_select_body(const FitHdr *hdr, const int32_t *info, const float *scores,
                                                const uint8_t *inl_H, const uint8_t *inl_F, const int32_t *idx,
                                                uint8_t *status, int32_t *d_cnt, float *d_score)
{
    __shared__ int32_t part[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t m = hdr->m;
    if (m <= 8 || (info[0] == 0 && info[6] == 0)) {
        if (tid == 0) *d_cnt = 0, *d_score = 0.0f;  // :447
        return;
    }
    const float sH = scores[0], sF = scores[1];
    const float RH = sH / (sF + sH);
    const bool useH = RH > 0.45;
    const uint8_t *in = useH ? inl_H : inl_F;
    int c = 0;
    for (int k = tid; k < m; k += 1024) {
        if (!in[k])
            status[idx[k]] = 0;
        else
            c++;
    }
    c = fit_wave_isum(c);
    if (lane == 0) part[wave] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < 16; w++) t += part[w];
        *d_cnt = t;
        *d_score = useH ? sH : sF;
    }
}

__global__ void __launch_bounds__(1024) k_fit_select(const FitHdr *hdr, const int32_t *info, const float *scores,
                                                     const uint8_t *inl_H, const uint8_t *inl_F, const int32_t *idx,
                                                     uint8_t *status, int32_t *d_cnt, float *d_score)
{
    fit_select_body(hdr, info, scores, inl_H, inl_F, idx, status, d_cnt, d_score);
}

}  // namespace pagk
