// pagk_pose_kernel.h -- ORBDetectAndDespMatcher::PoseEstimation2d2d (reference src/ORBDetectAndDespMatcher.cpp:93-105): the
// essential matrix of cv::findEssentialMat(points1, points2, f, pp, cv::RANSAC) and the pose of cv::recoverPose, restated
// as a DETERMINISTIC five-point RANSAC and a cheirality test.  OpenCV's random generator, its SVD-based solver and
// triangulatePoints are not reproduced (include/pagk.h "Two-view pose"); what the kernels promise is the bits of the
// plain-C restatement in tests/pose_ref.c for the same seed and inputs.  All model arithmetic is f64, one IEEE rounding per
// operation (-ffp-contract=off), + - * / sqrt and comparisons only; the only reductions are integer counts.  The H and F of
// the same call are the kernels of pagk_fit_kernel.h, unchanged; they also compact the correspondences for this file.
//
// Launch sequence behind the fit's (all on the context stream, no host synchronisation, graph-capturable):
//   k_pose_prep     ceil(n / 256) x 256   normalised correspondences q = ((u - cx) / f, (v - cy) / f) of the m compacted
//                              points, f64; resets the best key, the counters, E | R | t, the info words and the masks
//   k_pose_hyp      ceil(iters_E / 4) x 256   one hypothesis per wave: lane 0 draws the sample and solves it up to the Sturm
//                              chain out of the wave's LDS workspace (the solver's matrices and polynomials, 3440 B; nothing
//                              of it is a lane-private array), lane r isolates root r and forms its candidate, then the wave
//                              streams the m points once per candidate and reduces the
//                              integer count; lane 0 keeps the hypothesis' best candidate, stores its E in the hypothesis
//                              array and atomicMax'es (count << 32) | ~(16 h + root)
//   k_pose_recover  1 x 256    re-tests the winner (mask_E), decomposes it (thread 0, Horn's closed form), counts the good
//                              points of the four poses with ballots and one integer LDS atomic per wave and pose, chooses,
//                              writes mask_pose, R, t and the info words
//   k_pose_gather   ceil(cap_q / 256) x 256   in front of all that for pagk_pose_from_matches_device: the matched keypoint
//                              pairs of pagk_orb_match_device as correspondences with a status
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pagk_fit_kernel.h"

namespace pagk {

constexpr int kPoseInfoWords = 16;   // PAGK_POSE_INFO_WORDS
constexpr int kPoseModel = 2;        // the sampler's model id of the five-point samples
constexpr int kPoseHypPerBlock = 4;  // one hypothesis per wave, four waves per workgroup
constexpr int kPoseHalvings = 64, kPoseNewton = 6;
// the solver's workspace, in doubles: the 5 x 9 system, the basis X | Y | Z | W, E E^T (six entries) and its trace, the
// three cofactors of the determinant, the 10 x 20 constraint matrix, the three rows of B(z).  What is dead is reused: the
// minors, the roots and the division's remainder over the system, the Sturm chain over E E^T, the sample's points and later
// the candidates over the constraint matrix.
enum { kWsA = 0, kWsB = 45, kWsG = 81, kWsT = 141, kWsC = 151, kWsM = 181, kWsBp = 381, kWsSize = 420,
       kWsP = 0, kWsRoot = 10, kWsTmp = 20, kWsSt = 81, kWsE = 181 };
enum { kWiPerm = 0, kWiDeg = 9, kWiIdx = 20, kWiSize = 28,
       kWiNch = 20, kWiVlo = 21, kWiD = 22 };   // (over the sample's indices, dead once its points are read)

struct PoseHdr {                  // device header of a pose estimation (workspace)
    unsigned long long key;       // best (count << 32) | ~(16 h + root); 0 = no valid candidate
    int32_t valid_samples, valid_candidates;
};

struct PoseArgs {
    const float *p1, *p2;         // the fit's compacted correspondences, m x 2
    const int32_t *idx;           // their original indices
    const FitHdr *fit_hdr;        // m
    PoseHdr *hdr;
    double *qn;                   // normalised correspondences, m x 4
    double *hyp_E;                // iters x 9: the best candidate of every hypothesis
    int32_t *cand_counts;         // iters x 10 or null
    double *pose;                 // E | R | t
    int32_t *info;                // kPoseInfoWords
    uint8_t *mask_E, *mask_pose;  // original indexing, may be null
    unsigned long long seed;
    int32_t n, iters;
    double f, cx, cy;
    double t2;                    // (thresh_E / f)^2
    double conf, max_depth;
};

// monomials.  Linear: x y z 1.  Quadratic: x2 y2 xy xz x yz y z2 z 1.  Cubic, Nister's order: x3 y3 x2y xy2 x2z x2 y2z y2
// xyz xy | xz2 xz x yz2 yz y z3 z2 z 1.  kPoseLL / kPoseQL: where the product of two monomials lands.
__device__ const int8_t kPoseLL[4][4] = {{0, 2, 3, 4}, {2, 1, 5, 6}, {3, 5, 7, 8}, {4, 6, 8, 9}};
__device__ const int8_t kPoseQL[10][4] = {{0, 2, 4, 5},     {3, 1, 6, 7},     {2, 3, 8, 9},     {4, 8, 10, 11},   {5, 9, 11, 12},
                                          {8, 6, 13, 14},   {9, 7, 14, 15},   {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
__device__ const int8_t kPoseSym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};

// entry e of E = x X + y Y + z Z + W is the linear polynomial (bs[e], bs[9 + e], bs[18 + e], bs[27 + e])
__device__ void pose_mul_ll(double *out, const double *bs, int e1, int e2, bool neg)
{
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) {
            const double p = bs[9 * a + e1] * bs[9 * b + e2];
            const int k = kPoseLL[a][b];
            out[k] = neg ? out[k] - p : out[k] + p;
        }
}
__device__ void pose_mul_ql(double *out, const double *q, const double *bs, int e)
{
    for (int a = 0; a < 10; a++)
        for (int b = 0; b < 4; b++) {
            const int k = kPoseQL[a][b];
            out[k] = out[k] + q[a] * bs[9 * b + e];
        }
}

__device__ double pose_horner(const double *p, int deg, double x)
{
    double v = p[deg];
    for (int k = deg - 1; k >= 0; k--) v = v * x + p[k];
    return v;
}

// out[a + b] +-= pa[a] * pb[b]
__device__ void pose_conv(double *out, const double *pa, int na, const double *pb, int nb, bool neg)
{
    for (int a = 0; a < na; a++)
        for (int b = 0; b < nb; b++) {
            const double p = pa[a] * pb[b];
            out[a + b] = neg ? out[a + b] - p : out[a + b] + p;
        }
}

__device__ __forceinline__ int pose_st_off(int k) { return 11 * k - k * (k - 1) / 2; }

// sign variations of the Sturm chain at x (zeros and NaNs are skipped)
__device__ int pose_variations(const double *st, const int32_t *deg, int nch, double x)
{
    int prev = 0, cnt = 0;
    for (int k = 0; k < nch; k++) {
        const double v = pose_horner(st + pose_st_off(k), deg[k], x);
        const int s = v > 0.0 ? 1 : v < 0.0 ? -1 : 0;
        if (s != 0) {
            if (prev != 0 && s != prev) cnt++;
            prev = s;
        }
    }
    return cnt;
}

// The minimal solve up to the Sturm chain.  q: 5 x (x1, y1, x2, y2), normalised (it may lie in the constraint matrix'
// place).  Returns the number of real roots (0 .. 10), or -1 for an invalid sample, and leaves the basis, B(z), the chain,
// its degrees, Cauchy's bound and V(-R) in the workspace for pose_solve5_root.
__device__ int pose_solve5_chain(const double *q, double *ws, int32_t *wi)
{
    double *A = ws + kWsA, *bs = ws + kWsB, *G = ws + kWsG, *T = ws + kWsT, *Cq = ws + kWsC, *M = ws + kWsM, *Bp = ws + kWsBp;
    int32_t *perm = wi + kWiPerm, *deg = wi + kWiDeg;
    // the epipolar system
    for (int j = 0; j < 5; j++) {
        const double x = q[4 * j], y = q[4 * j + 1], u = q[4 * j + 2], v = q[4 * j + 3];
        double *r = A + 9 * j;
        r[0] = u * x, r[1] = u * y, r[2] = u, r[3] = v * x, r[4] = v * y, r[5] = v, r[6] = x, r[7] = y, r[8] = 1.0;
    }
    // null space: Gauss-Jordan with full pivoting
    double mx = 0.0;
    for (int k = 0; k < 45; k++) mx = fabs(A[k]) > mx ? fabs(A[k]) : mx;
    for (int c = 0; c < 9; c++) perm[c] = c;
    for (int j = 0; j < 5; j++) {
        int pr = j, pc = j;
        double best = fabs(A[9 * j + j]);
        for (int r = j; r < 5; r++)
            for (int c = j; c < 9; c++)
                if (fabs(A[9 * r + c]) > best) best = fabs(A[9 * r + c]), pr = r, pc = c;
        if (!(best > 1e-8 * mx)) return -1;
        if (pr != j)
            for (int c = 0; c < 9; c++) {
                const double t = A[9 * j + c];
                A[9 * j + c] = A[9 * pr + c];
                A[9 * pr + c] = t;
            }
        if (pc != j) {
            for (int r = 0; r < 5; r++) {
                const double t = A[9 * r + j];
                A[9 * r + j] = A[9 * r + pc];
                A[9 * r + pc] = t;
            }
            const int32_t t = perm[j];
            perm[j] = perm[pc];
            perm[pc] = t;
        }
        const double piv = A[9 * j + j];
        for (int c = j; c < 9; c++) A[9 * j + c] = A[9 * j + c] / piv;
        for (int r = 0; r < 5; r++) {
            if (r == j) continue;
            const double f = A[9 * r + j];
            for (int c = j + 1; c < 9; c++) A[9 * r + c] = A[9 * r + c] - f * A[9 * j + c];
            A[9 * r + j] = 0.0;
        }
    }
    for (int t = 0; t < 4; t++) {
        for (int e = 0; e < 9; e++) bs[9 * t + e] = 0.0;
        bs[9 * t + perm[5 + t]] = 1.0;
        for (int i = 0; i < 5; i++) bs[9 * t + perm[i]] = -A[9 * i + 5 + t];
    }
    // modified Gram-Schmidt, in index order
    for (int t = 0; t < 4; t++) {
        for (int j = 0; j < t; j++) {
            double d = 0.0;
            for (int e = 0; e < 9; e++) d = d + bs[9 * j + e] * bs[9 * t + e];
            for (int e = 0; e < 9; e++) bs[9 * t + e] = bs[9 * t + e] - d * bs[9 * j + e];
        }
        double nn = 0.0;
        for (int e = 0; e < 9; e++) nn = nn + bs[9 * t + e] * bs[9 * t + e];
        const double nr = sqrt(nn);
        for (int e = 0; e < 9; e++) bs[9 * t + e] = bs[9 * t + e] / nr;
    }
    // the constraints: rows 0 .. 8 (E E^T - 1/2 tr(E E^T) I) E, row 9 det E
    for (int k = 0; k < 200; k++) M[k] = 0.0;
    for (int k = 0; k < 30; k++) Cq[k] = 0.0;
    pose_mul_ll(Cq, bs, 4, 8, false), pose_mul_ll(Cq, bs, 5, 7, true);
    pose_mul_ll(Cq + 10, bs, 5, 6, false), pose_mul_ll(Cq + 10, bs, 3, 8, true);
    pose_mul_ll(Cq + 20, bs, 3, 7, false), pose_mul_ll(Cq + 20, bs, 4, 6, true);
    for (int k = 0; k < 3; k++) pose_mul_ql(M + 180, Cq + 10 * k, bs, k);
    for (int k = 0; k < 60; k++) G[k] = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++)
            for (int k = 0; k < 3; k++) pose_mul_ll(G + 10 * kPoseSym[i][j], bs, 3 * i + k, 3 * j + k, false);
    for (int k = 0; k < 10; k++) T[k] = (G[k] + G[30 + k]) + G[50 + k];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 10; k++) G[10 * kPoseSym[i][i] + k] = G[10 * kPoseSym[i][i] + k] - 0.5 * T[k];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) pose_mul_ql(M + 20 * (3 * i + j), G + 10 * kPoseSym[i][k], bs, 3 * k + j);
    // Gauss-Jordan with partial pivoting on the first ten columns; rows 0 .. 3 are not needed after their own step
    for (int j = 0; j < 10; j++) {
        int p = j;
        double best = fabs(M[20 * j + j]);
        for (int r = j + 1; r < 10; r++)
            if (fabs(M[20 * r + j]) > best) best = fabs(M[20 * r + j]), p = r;
        if (!(best > 0.0)) return -1;
        if (p != j)
            for (int c = 0; c < 20; c++) {
                const double t = M[20 * j + c];
                M[20 * j + c] = M[20 * p + c];
                M[20 * p + c] = t;
            }
        const double piv = M[20 * j + j];
        for (int c = j; c < 20; c++) M[20 * j + c] = M[20 * j + c] / piv;
        for (int r = 0; r < 10; r++) {
            if (r == j || (r < j && r < 4)) continue;
            const double f = M[20 * r + j];
            for (int c = j + 1; c < 20; c++) M[20 * r + c] = M[20 * r + c] - f * M[20 * j + c];
            M[20 * r + j] = 0.0;
        }
    }
    // B(z): rows e - z f, g - z h, i - z j; columns x (degree 3), y (degree 3), 1 (degree 4), ascending powers
    for (int r = 0; r < 3; r++) {
        const double *e = M + 20 * (4 + 2 * r), *f = M + 20 * (5 + 2 * r);
        double *o = Bp + 13 * r;
        for (int s = 0; s < 2; s++) {
            const int cb = 10 + 3 * s;
            o[4 * s] = e[cb + 2], o[4 * s + 1] = e[cb + 1] - f[cb + 2], o[4 * s + 2] = e[cb] - f[cb + 1], o[4 * s + 3] = -f[cb];
        }
        o[8] = e[19], o[9] = e[18] - f[19], o[10] = e[17] - f[18], o[11] = e[16] - f[17], o[12] = -f[16];
    }
    // det B(z), degree 10: expansion along the third column
    double *P = ws + kWsP, *st = ws + kWsSt, *tmp = ws + kWsTmp;
    for (int k = 0; k < 11; k++) st[k] = 0.0;
    for (int r = 0; r < 3; r++) {
        const int a = r == 0 ? 1 : 0, b = r == 2 ? 1 : 2;
        for (int k = 0; k < 7; k++) P[k] = 0.0;
        pose_conv(P, Bp + 13 * a, 4, Bp + 13 * b + 4, 4, false);
        pose_conv(P, Bp + 13 * b, 4, Bp + 13 * a + 4, 4, true);
        pose_conv(st, Bp + 13 * r + 8, 5, P, 7, r == 1);
    }
    // scaled to largest |coefficient| 1; its degree
    mx = 0.0;
    for (int k = 0; k < 11; k++) {
        if (!isfinite(st[k])) return -1;
        mx = fabs(st[k]) > mx ? fabs(st[k]) : mx;
    }
    if (!(mx > 0.0)) return -1;
    for (int k = 0; k < 11; k++) st[k] = st[k] / mx;
    int d = 10;
    while (d > 0 && st[d] == 0.0) d--;
    if (d < 1) return -1;
    // Cauchy's bound
    double R = 0.0;
    for (int k = 0; k < d; k++) {
        const double t = fabs(st[k] / st[d]);
        R = t > R ? t : R;
    }
    R = R + 1.0;
    if (!isfinite(R)) return -1;
    // the Sturm chain: p, p', then the negated remainders, each scaled to largest |coefficient| 1
    deg[0] = d, deg[1] = d - 1;
    for (int k = 1; k <= d; k++) st[11 + k - 1] = (double)k * st[k];
    int nch = 2;
    while (deg[nch - 1] > 0) {
        const double *pa = st + pose_st_off(nch - 2), *pb = st + pose_st_off(nch - 1);
        const int da = deg[nch - 2], db = deg[nch - 1];
        for (int k = 0; k <= da; k++) tmp[k] = pa[k];
        for (int i = da; i >= db; i--) {
            const double f = tmp[i] / pb[db];
            for (int j = 0; j < db; j++) tmp[i - db + j] = tmp[i - db + j] - f * pb[j];
        }
        int dr = db - 1;
        double rm = 0.0;
        for (int k = 0; k <= dr; k++) {
            if (!isfinite(tmp[k])) return -1;
            rm = fabs(tmp[k]) > rm ? fabs(tmp[k]) : rm;
        }
        if (!(rm > 0.0)) break;
        while (dr > 0 && tmp[dr] == 0.0) dr--;
        double *pn = st + pose_st_off(nch);
        for (int k = 0; k <= dr; k++) pn[k] = -(tmp[k] / rm);
        deg[nch] = dr;
        nch++;
    }
    const int vlo = pose_variations(st, deg, nch, -R);
    int nroot = vlo - pose_variations(st, deg, nch, R);
    nroot = nroot < 0 ? 0 : nroot > 10 ? 10 : nroot;
    tmp[0] = R;
    wi[kWiNch] = nch, wi[kWiVlo] = vlo, wi[kWiD] = d;
    return nroot;
}

// Root r (0-based, in increasing order) of the chain pose_solve5_chain left, and its candidate ws[kWsE + 9 r ..]; true when
// the candidate is finite.  The roots are independent of each other: in k_pose_hyp lane r finds root r.  From here on the
// constraint matrix is dead: the candidates take its place.
__device__ bool pose_solve5_root(int r, double *ws, const int32_t *wi)
{
    const double *bs = ws + kWsB, *Bp = ws + kWsBp, *st = ws + kWsSt;
    const int32_t *deg = wi + kWiDeg;
    const int nch = wi[kWiNch], vlo = wi[kWiVlo], d = wi[kWiD];
    const double R = ws[kWsTmp];
    double z;
    {
        // root r + 1 in increasing order lies in (lo, hi]
        double lo = -R, hi = R;
        for (int it = 0; it < kPoseHalvings; it++) {
            const double mid = 0.5 * (lo + hi);
            if (vlo - pose_variations(st, deg, nch, mid) >= r + 1)
                hi = mid;
            else
                lo = mid;
        }
        double x = 0.5 * (lo + hi);
        for (int it = 0; it < kPoseNewton; it++) {
            const double xn = x - pose_horner(st, d, x) / pose_horner(st + 11, d - 1, x);
            if (!(xn >= lo && xn <= hi)) break;
            x = xn;
        }
        ws[kWsRoot + r] = z = x;
    }
    // back-substitution
    double *Es = ws + kWsE;
    bool fin = true;
    {
        const double bx0 = pose_horner(Bp, 3, z), by0 = pose_horner(Bp + 4, 3, z), bc0 = pose_horner(Bp + 8, 4, z);
        const double bx1 = pose_horner(Bp + 13, 3, z), by1 = pose_horner(Bp + 17, 3, z), bc1 = pose_horner(Bp + 21, 4, z);
        const double bx2 = pose_horner(Bp + 26, 3, z), by2 = pose_horner(Bp + 30, 3, z), bc2 = pose_horner(Bp + 34, 4, z);
        const double d01 = bx0 * by1 - bx1 * by0, d02 = bx0 * by2 - bx2 * by0, d12 = bx1 * by2 - bx2 * by1;
        double dd = d01, xa = bx0, ya = by0, ca = bc0, xb = bx1, yb = by1, cb = bc1;
        if (fabs(d02) > fabs(dd)) dd = d02, xb = bx2, yb = by2, cb = bc2;
        if (fabs(d12) > fabs(dd)) dd = d12, xa = bx1, ya = by1, ca = bc1, xb = bx2, yb = by2, cb = bc2;
        const double x = (ya * cb - yb * ca) / dd, y = (xb * ca - xa * cb) / dd;
        double *E = Es + 9 * r;
        double nn = 0.0;
        for (int e = 0; e < 9; e++) {
            E[e] = ((x * bs[e] + y * bs[9 + e]) + z * bs[18 + e]) + bs[27 + e];
            nn = nn + E[e] * E[e];
        }
        const double nr = sqrt(nn);
        for (int e = 0; e < 9; e++) {
            E[e] = E[e] / nr;
            fin &= isfinite(E[e]);
        }
    }
    return fin;
}

// the Sampson distance without its division: (q2^T E q1)^2 <= t2 (a^2 + b^2 + c^2 + d^2)
__device__ __forceinline__ bool pose_inlier(const double *E, double x1, double y1, double x2, double y2, double t2)
{
    const double a = (E[0] * x1 + E[1] * y1) + E[2], b = (E[3] * x1 + E[4] * y1) + E[5], c = (E[6] * x1 + E[7] * y1) + E[8];
    const double d1 = (E[0] * x2 + E[3] * y2) + E[6], d2 = (E[1] * x2 + E[4] * y2) + E[7];
    const double r = (x2 * a + y2 * b) + c;
    return r * r <= t2 * (((a * a + b * b) + d1 * d1) + d2 * d2);
}

// Horn's closed form: b b^T = 1/2 tr(E E^T) I - E E^T, (b.b) R = cof(E) -+ [b]x E; rt: R1 | R2 | t
__device__ void pose_decompose(const double *E, double *rt)
{
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[3 * i + j] = (E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2];
    const double h = 0.5 * ((G[0] + G[4]) + G[8]);
    const double D0 = h - G[0], D1 = h - G[4], D2 = h - G[8];
    int im = 0;
    double Dm = D0;
    if (D1 > Dm) im = 1, Dm = D1;
    if (D2 > Dm) im = 2, Dm = D2;
    const double sd = sqrt(Dm);
    // row im of b b^T, without a runtime-indexed array
    const double r0 = im == 0 ? Dm : im == 1 ? -G[3] : -G[6];
    const double r1 = im == 1 ? Dm : im == 0 ? -G[1] : -G[7];
    const double r2 = im == 2 ? Dm : im == 0 ? -G[2] : -G[5];
    const double b0 = r0 / sd, b1 = r1 / sd, b2 = r2 / sd;
    const double bb = (b0 * b0 + b1 * b1) + b2 * b2;
    const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                           E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                           E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double be[3] = {b1 * E[6 + j] - b2 * E[3 + j], b2 * E[j] - b0 * E[6 + j], b0 * E[3 + j] - b1 * E[j]};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            rt[3 * i + j] = (cof[3 * i + j] - be[i]) / bb;
            rt[9 + 3 * i + j] = (cof[3 * i + j] + be[i]) / bb;
        }
    }
    const double nb = sqrt(bb);
    rt[18] = b0 / nb, rt[19] = b1 / nb, rt[20] = b2 / nb;
}

// both depths of lambda2 q2 = lambda1 R q1 + t from the 2 x 2 normal equations
__device__ __forceinline__ bool pose_good_depth(const double *R, double t0, double t1, double t2, double x1, double y1,
                                                double x2, double y2, double max_depth)
{
    const double a0 = (R[0] * x1 + R[1] * y1) + R[2], a1 = (R[3] * x1 + R[4] * y1) + R[5], a2 = (R[6] * x1 + R[7] * y1) + R[8];
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2, qq = (x2 * x2 + y2 * y2) + 1.0, aq = (a0 * x2 + a1 * y2) + a2;
    const double at = (a0 * t0 + a1 * t1) + a2 * t2, qt = (x2 * t0 + y2 * t1) + t2;
    const double det = aa * qq - aq * aq;
    const double l1 = (aq * qt - at * qq) / det, l2 = (aa * qt - aq * at) / det;
    return l1 > 0.0 && l1 < max_depth && l2 > 0.0 && l2 < max_depth;
}

// ---- kernels ------------------------------------------------------------------------------------------------------
// k_pose_prep: behind k_fit_compact.  The grid covers n (one workgroup when n is 0).
__global__ void __launch_bounds__(256) k_pose_prep(PoseArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int32_t m = a.fit_hdr->m;
    if (i < a.n) {
        if (a.mask_E) a.mask_E[i] = 0;
        if (a.mask_pose) a.mask_pose[i] = 0;
    }
    if (i < m) {
        a.qn[4 * (size_t)i] = ((double)a.p1[2 * i] - a.cx) / a.f;
        a.qn[4 * (size_t)i + 1] = ((double)a.p1[2 * i + 1] - a.cy) / a.f;
        a.qn[4 * (size_t)i + 2] = ((double)a.p2[2 * i] - a.cx) / a.f;
        a.qn[4 * (size_t)i + 3] = ((double)a.p2[2 * i + 1] - a.cy) / a.f;
    }
    if (i < 21) a.pose[i] = 0.0;
    if (i < kPoseInfoWords) a.info[i] = i == 1 ? m : (i == 2 || i == 3) ? -1 : 0;
    if (i == 0) a.hdr->key = 0ull, a.hdr->valid_samples = 0, a.hdr->valid_candidates = 0;
}

__global__ void __launch_bounds__(256) k_pose_hyp(PoseArgs a)
{
    __shared__ double ws[kPoseHypPerBlock][kWsSize];
    __shared__ int32_t wi[kPoseHypPerBlock][kWiSize];
    __shared__ int32_t res[kPoseHypPerBlock];   // number of roots (-1: invalid sample)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = (int)blockIdx.x * kPoseHypPerBlock + wave;
    const int32_t m = a.fit_hdr->m;
    const bool live = h < a.iters && m >= 5;
    if (lane == 0) {
        int n = -1;
        if (live && fit_sample(a.seed, kPoseModel, (uint32_t)h, (uint32_t)m, wi[wave] + kWiIdx)) {
            double *q = ws[wave] + kWsM;
            for (int j = 0; j < 5; j++)
                for (int k = 0; k < 4; k++) q[4 * j + k] = a.qn[4 * (size_t)wi[wave][kWiIdx + j] + k];
            n = pose_solve5_chain(q, ws[wave], wi[wave]);
        }
        res[wave] = n;
    }
    __syncthreads();
    const int nr = res[wave];   // -1 also when fewer than 5 points take part
    // the roots are independent: lane r isolates root r and forms its candidate (the same operations in the same order)
    const bool fin = lane < nr && pose_solve5_root(lane, ws[wave], wi[wave]);
    const uint32_t ok = (uint32_t)__ballot(fin);
    __syncthreads();
    if (h >= a.iters) return;
    if (nr < 0) {
        if (a.cand_counts && lane < 10) a.cand_counts[10 * (size_t)h + lane] = -1;
        return;
    }
    // the consensus: the wave streams the points once per candidate
    int best_c = -1, best_r = -1, valid = 0, mine = -1;   // mine: lane r keeps candidate r's count
    for (int r = 0; r < nr; r++) {
        if (!(ok >> r & 1)) continue;
        double E[9];
#pragma unroll
        for (int k = 0; k < 9; k++) E[k] = ws[wave][kWsE + 9 * r + k];
        int c = 0;
        for (int k = lane; k < m; k += 64) {
            const double4 p = *reinterpret_cast<const double4 *>(a.qn + 4 * (size_t)k);
            c += pose_inlier(E, p.x, p.y, p.z, p.w, a.t2) ? 1 : 0;
        }
        c = __shfl(fit_wave_isum(c), 0, 64);
        valid++;
        if (c > best_c) best_c = c, best_r = r;
        if (lane == r) mine = c;
    }
    if (a.cand_counts && lane < 10) a.cand_counts[10 * (size_t)h + lane] = mine;
    if (lane == 0) {
        atomicAdd(&a.hdr->valid_samples, 1);
        if (best_r >= 0) {
            for (int k = 0; k < 9; k++) a.hyp_E[9 * (size_t)h + k] = ws[wave][kWsE + 9 * best_r + k];
            atomicAdd(&a.hdr->valid_candidates, valid);
            atomicMax(&a.hdr->key, ((unsigned long long)(uint32_t)best_c << 32) |
                                       (unsigned long long)(~(uint32_t)(16 * h + best_r)));
        }
    }
}

__global__ void __launch_bounds__(256) k_pose_recover(PoseArgs a)
{
    __shared__ double rt[21];
    __shared__ int32_t good[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int32_t m = a.fit_hdr->m;
    const unsigned long long key = a.hdr->key;
    if (!key) {  // k_pose_prep left "no model"
        if (tid == 0) a.info[5] = a.hdr->valid_samples, a.info[6] = a.hdr->valid_candidates;
        return;
    }
    const int32_t num = (int32_t)~(uint32_t)(key & 0xffffffffull), bc = (int32_t)(key >> 32);
    const int32_t bh = num >> 4;
    if (tid == 0) {
        a.info[2] = bh, a.info[3] = num & 15, a.info[4] = bc;
        a.info[5] = a.hdr->valid_samples, a.info[6] = a.hdr->valid_candidates;
        a.info[7] = fit_adaptive(bc, m, 5, a.conf);
    }
    if (bc < 5) return;
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = a.hyp_E[9 * (size_t)bh + k];
    if (tid == 0) pose_decompose(E, rt);
    if (tid < 4) good[tid] = 0;
    __syncthreads();
    double R1[9], R2[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R1[k] = rt[k], R2[k] = rt[9 + k];
    const double t0 = rt[18], t1 = rt[19], t2 = rt[20];
    int g0 = 0, g1 = 0, g2 = 0, g3 = 0;   // lane 0: the wave's counts
    for (int k0 = 0; k0 < m; k0 += 256) {
        const int k = k0 + tid;
        bool in = false, p0 = false, p1 = false, p2 = false, p3 = false;
        if (k < m) {
            const double4 p = *reinterpret_cast<const double4 *>(a.qn + 4 * (size_t)k);
            in = pose_inlier(E, p.x, p.y, p.z, p.w, a.t2);
            p0 = pose_good_depth(R1, t0, t1, t2, p.x, p.y, p.z, p.w, a.max_depth);
            p1 = pose_good_depth(R2, t0, t1, t2, p.x, p.y, p.z, p.w, a.max_depth);
            p2 = pose_good_depth(R1, -t0, -t1, -t2, p.x, p.y, p.z, p.w, a.max_depth);
            p3 = pose_good_depth(R2, -t0, -t1, -t2, p.x, p.y, p.z, p.w, a.max_depth);
            if (a.mask_E) a.mask_E[a.idx[k]] = in ? 1 : 0;
        }
        g0 += __popcll(__ballot(p0)), g1 += __popcll(__ballot(p1)), g2 += __popcll(__ballot(p2)), g3 += __popcll(__ballot(p3));
    }
    if (lane == 0) atomicAdd(&good[0], g0), atomicAdd(&good[1], g1), atomicAdd(&good[2], g2), atomicAdd(&good[3], g3);
    __syncthreads();
    const int c0 = good[0], c1 = good[1], c2 = good[2], c3 = good[3];
    int bp = 0, bg = c0;
    if (c1 > bg) bp = 1, bg = c1;
    if (c2 > bg) bp = 2, bg = c2;
    if (c3 > bg) bp = 3, bg = c3;
    const double sg = (bp & 2) ? -1.0 : 1.0;
    if (a.mask_pose)
        for (int k = tid; k < m; k += 256) {
            const double4 p = *reinterpret_cast<const double4 *>(a.qn + 4 * (size_t)k);
            const bool g = (bp & 1) ? pose_good_depth(R2, sg * t0, sg * t1, sg * t2, p.x, p.y, p.z, p.w, a.max_depth)
                                    : pose_good_depth(R1, sg * t0, sg * t1, sg * t2, p.x, p.y, p.z, p.w, a.max_depth);
            a.mask_pose[a.idx[k]] = g ? 1 : 0;
        }
    if (tid < 9) a.pose[tid] = a.hyp_E[9 * (size_t)bh + tid];
    if (tid < 9) a.pose[9 + tid] = rt[((bp & 1) ? 9 : 0) + tid];
    if (tid < 3) a.pose[18 + tid] = sg * rt[18 + tid];
    if (tid == 0) {
        a.info[0] = 1, a.info[8] = bp;
        a.info[9] = c0, a.info[10] = c1, a.info[11] = c2, a.info[12] = c3;
    }
}

// the input of PoseEstimation2d2d (:86-91) from what pagk_detect_fast_device and pagk_orb_match_device wrote: for query row q
// pts1[q] = kp_ref[q], pts2[q] = kp_cur[train_idx[q]], status[q] = q < nq && keep[q] && 0 <= train_idx[q] < nt
__global__ void __launch_bounds__(256) k_pose_gather(int32_t cap_q, const float *kp_ref, const int32_t *d_nq, int32_t cap_t,
                                                     const float *kp_cur, const int32_t *d_nt, const int32_t *train_idx,
                                                     const uint8_t *keep, float *pts1, float *pts2, uint8_t *status)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= cap_q) return;
    int32_t nq = *d_nq, nt = *d_nt;
    nq = nq < 0 ? 0 : nq > cap_q ? cap_q : nq;
    nt = nt < 0 ? 0 : nt > cap_t ? cap_t : nt;
    const int32_t tr = train_idx[q];
    const bool row = q < nq, live = row && keep[q] != 0 && tr >= 0 && tr < nt;
    pts1[2 * q] = row ? kp_ref[2 * q] : 0.0f, pts1[2 * q + 1] = row ? kp_ref[2 * q + 1] : 0.0f;
    pts2[2 * q] = live ? kp_cur[2 * tr] : 0.0f, pts2[2 * q + 1] = live ? kp_cur[2 * tr + 1] : 0.0f;
    status[q] = live ? 1 : 0;
}

}  // namespace pagk
