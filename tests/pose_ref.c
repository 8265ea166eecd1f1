/* pose_ref.c -- plain-C restatement of the two-view pose (csrc/pagk_pose_kernel.h, include/pagk.h "Two-view pose"):
 * the essential matrix by a deterministic five-point RANSAC, the rotation and the translation direction by the
 * cheirality test.  Test infrastructure: the GPU result must equal this one byte for byte.  Built by the tests with
 * gcc -O2 -ffp-contract=off (one IEEE rounding per operation, like the library) and loaded with ctypes.
 *
 * Every step is written in the order the kernels evaluate it.  The only reductions are integer counts. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct pr_fit_params { /* the layout of pagk_fit_params */
    uint64_t seed;
    int32_t iters_H, iters_F;
    double thresh_H, thresh_F;
    double conf_H, conf_F;
} pr_fit_params;

typedef struct pr_params { /* the layout of pagk_pose_params */
    uint64_t seed;
    int32_t iters_E;
    int32_t reserved;
    double thresh_E, conf_E, max_depth;
    pr_fit_params fit;
} pr_params;

enum { MAX_DRAWS = 64, INFO_WORDS = 16, MODEL_E = 2 };
/* the solver's workspace, in doubles: the 5 x 9 system, the basis X | Y | Z | W, E E^T (six entries) and its trace, the
 * three cofactors of the determinant, the 10 x 20 constraint matrix, the three rows of B(z).  What is dead is reused: the
 * minors, the roots and the division's remainder over the system, the Sturm chain over E E^T, the candidates over the
 * constraint matrix. */
enum { WS_A = 0, WS_B = 45, WS_G = 81, WS_T = 141, WS_C = 151, WS_M = 181, WS_BP = 381, WS_SIZE = 420,
       WS_P = 0, WS_ROOT = 10, WS_TMP = 20, WS_ST = 81, WS_E = 181 };
enum { WI_PERM = 0, WI_DEG = 9, WI_SIZE = 20 };
enum { HALVINGS = 64, NEWTON = 6 };

static uint64_t sm64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static uint32_t draw_index(uint64_t seed, int model, uint32_t hyp, uint32_t draw, uint32_t m)
{
    const uint64_t z = sm64(seed ^ sm64(((uint64_t)model << 56) | ((uint64_t)hyp << 8) | (uint64_t)draw));
    return (uint32_t)(((z >> 32) * (uint64_t)m) >> 32);
}

/* the sample of hypothesis `hyp` of model 2: 5 distinct indices; 0 when MAX_DRAWS draws did not find them */
int pr_sample(uint64_t seed, uint32_t hyp, uint32_t m, int32_t *idx)
{
    uint32_t d = 0;
    for (int j = 0; j < 5; j++) idx[j] = -1;
    for (int j = 0; j < 5; j++) {
        for (;;) {
            if (d >= MAX_DRAWS) {
                for (int k = 0; k < 5; k++) idx[k] = -1;
                return 0;
            }
            const int32_t c = (int32_t)draw_index(seed, MODEL_E, hyp, d, m);
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

/* monomials.  Linear: x y z 1.  Quadratic: x2 y2 xy xz x yz y z2 z 1.  Cubic, Nister's order: x3 y3 x2y xy2 x2z x2 y2z
 * y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1.  LL / QL: where the product of two monomials lands. */
static const int8_t LL[4][4] = {{0, 2, 3, 4}, {2, 1, 5, 6}, {3, 5, 7, 8}, {4, 6, 8, 9}};
static const int8_t QL[10][4] = {{0, 2, 4, 5},     {3, 1, 6, 7},     {2, 3, 8, 9},     {4, 8, 10, 11},   {5, 9, 11, 12},
                                 {8, 6, 13, 14},   {9, 7, 14, 15},   {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
static const int8_t SYM[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};

/* entry e of E = x X + y Y + z Z + W is the linear polynomial (bs[e], bs[9 + e], bs[18 + e], bs[27 + e]) */
static void mul_ll(double *out, const double *bs, int e1, int e2, int neg)
{
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) {
            const double p = bs[9 * a + e1] * bs[9 * b + e2];
            const int k = LL[a][b];
            out[k] = neg ? out[k] - p : out[k] + p;
        }
}
static void mul_ql(double *out, const double *q, const double *bs, int e)
{
    for (int a = 0; a < 10; a++)
        for (int b = 0; b < 4; b++) {
            const int k = QL[a][b];
            out[k] = out[k] + q[a] * bs[9 * b + e];
        }
}

static double horner(const double *p, int deg, double x)
{
    double v = p[deg];
    for (int k = deg - 1; k >= 0; k--) v = v * x + p[k];
    return v;
}

/* out[a + b] +-= pa[a] * pb[b] */
static void conv(double *out, const double *pa, int na, const double *pb, int nb, int neg)
{
    for (int a = 0; a < na; a++)
        for (int b = 0; b < nb; b++) {
            const double p = pa[a] * pb[b];
            out[a + b] = neg ? out[a + b] - p : out[a + b] + p;
        }
}

static int st_off(int k) { return 11 * k - k * (k - 1) / 2; }

/* sign variations of the Sturm chain at x (zeros and NaNs are skipped) */
static int variations(const double *st, const int32_t *deg, int nch, double x)
{
    int prev = 0, cnt = 0;
    for (int k = 0; k < nch; k++) {
        const double v = horner(st + st_off(k), deg[k], x);
        const int s = v > 0.0 ? 1 : v < 0.0 ? -1 : 0;
        if (s != 0) {
            if (prev != 0 && s != prev) cnt++;
            prev = s;
        }
    }
    return cnt;
}

/* The minimal solve.  q: 5 x (x1, y1, x2, y2), normalised.  Returns the number of real roots (0 .. 10), or -1 for an invalid
 * sample; candidate r is ws[WS_E + 9 r ..], bit r of *ok says that it is finite; ws[WS_ROOT + r] is its root.  When
 * `detp` is not NULL it receives the 11 coefficients of the scaled determinant polynomial (ascending). */
static int solve5(const double *q, double *ws, int32_t *wi, uint32_t *ok, double *detp)
{
    double *A = ws + WS_A, *bs = ws + WS_B, *G = ws + WS_G, *T = ws + WS_T, *Cq = ws + WS_C, *M = ws + WS_M,
           *Bp = ws + WS_BP;
    int32_t *perm = wi + WI_PERM, *deg = wi + WI_DEG;
    *ok = 0;
    /* the epipolar system */
    for (int j = 0; j < 5; j++) {
        const double x = q[4 * j], y = q[4 * j + 1], u = q[4 * j + 2], v = q[4 * j + 3];
        double *r = A + 9 * j;
        r[0] = u * x, r[1] = u * y, r[2] = u, r[3] = v * x, r[4] = v * y, r[5] = v, r[6] = x, r[7] = y, r[8] = 1.0;
    }
    /* null space: Gauss-Jordan with full pivoting */
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
    /* modified Gram-Schmidt, in index order */
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
    /* the constraints: rows 0 .. 8 (E E^T - 1/2 tr(E E^T) I) E, row 9 det E */
    for (int k = 0; k < 200; k++) M[k] = 0.0;
    for (int k = 0; k < 30; k++) Cq[k] = 0.0;
    mul_ll(Cq, bs, 4, 8, 0), mul_ll(Cq, bs, 5, 7, 1);
    mul_ll(Cq + 10, bs, 5, 6, 0), mul_ll(Cq + 10, bs, 3, 8, 1);
    mul_ll(Cq + 20, bs, 3, 7, 0), mul_ll(Cq + 20, bs, 4, 6, 1);
    for (int k = 0; k < 3; k++) mul_ql(M + 180, Cq + 10 * k, bs, k);
    for (int k = 0; k < 60; k++) G[k] = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++)
            for (int k = 0; k < 3; k++) mul_ll(G + 10 * SYM[i][j], bs, 3 * i + k, 3 * j + k, 0);
    for (int k = 0; k < 10; k++) T[k] = (G[k] + G[30 + k]) + G[50 + k];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 10; k++) G[10 * SYM[i][i] + k] = G[10 * SYM[i][i] + k] - 0.5 * T[k];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) mul_ql(M + 20 * (3 * i + j), G + 10 * SYM[i][k], bs, 3 * k + j);
    /* Gauss-Jordan with partial pivoting on the first ten columns; rows 0 .. 3 are not needed after their own step */
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
    /* B(z): rows e - z f, g - z h, i - z j; columns x (degree 3), y (degree 3), 1 (degree 4), ascending powers */
    for (int r = 0; r < 3; r++) {
        const double *e = M + 20 * (4 + 2 * r), *f = M + 20 * (5 + 2 * r);
        double *o = Bp + 13 * r;
        for (int s = 0; s < 2; s++) {
            const int cb = 10 + 3 * s;
            o[4 * s] = e[cb + 2], o[4 * s + 1] = e[cb + 1] - f[cb + 2], o[4 * s + 2] = e[cb] - f[cb + 1], o[4 * s + 3] = -f[cb];
        }
        o[8] = e[19], o[9] = e[18] - f[19], o[10] = e[17] - f[18], o[11] = e[16] - f[17], o[12] = -f[16];
    }
    /* det B(z), degree 10: expansion along the third column */
    double *P = ws + WS_P, *st = ws + WS_ST, *root = ws + WS_ROOT, *tmp = ws + WS_TMP;
    for (int k = 0; k < 11; k++) st[k] = 0.0;
    for (int r = 0; r < 3; r++) {
        const int a = r == 0 ? 1 : 0, b = r == 2 ? 1 : 2;
        for (int k = 0; k < 7; k++) P[k] = 0.0;
        conv(P, Bp + 13 * a, 4, Bp + 13 * b + 4, 4, 0);
        conv(P, Bp + 13 * b, 4, Bp + 13 * a + 4, 4, 1);
        conv(st, Bp + 13 * r + 8, 5, P, 7, r == 1);
    }
    /* scaled to largest |coefficient| 1; its degree */
    mx = 0.0;
    for (int k = 0; k < 11; k++) {
        if (!isfinite(st[k])) return -1;
        mx = fabs(st[k]) > mx ? fabs(st[k]) : mx;
    }
    if (!(mx > 0.0)) return -1;
    for (int k = 0; k < 11; k++) st[k] = st[k] / mx;
    if (detp)
        for (int k = 0; k < 11; k++) detp[k] = st[k];
    int d = 10;
    while (d > 0 && st[d] == 0.0) d--;
    if (d < 1) return -1;
    /* Cauchy's bound */
    double R = 0.0;
    for (int k = 0; k < d; k++) {
        const double t = fabs(st[k] / st[d]);
        R = t > R ? t : R;
    }
    R = R + 1.0;
    if (!isfinite(R)) return -1;
    /* the Sturm chain: p, p', then the negated remainders, each scaled to largest |coefficient| 1 */
    deg[0] = d, deg[1] = d - 1;
    for (int k = 1; k <= d; k++) st[11 + k - 1] = (double)k * st[k];
    int nch = 2;
    while (deg[nch - 1] > 0) {
        const double *pa = st + st_off(nch - 2), *pb = st + st_off(nch - 1);
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
        double *pn = st + st_off(nch);
        for (int k = 0; k <= dr; k++) pn[k] = -(tmp[k] / rm);
        deg[nch] = dr;
        nch++;
    }
    const int vlo = variations(st, deg, nch, -R);
    int nroot = vlo - variations(st, deg, nch, R);
    nroot = nroot < 0 ? 0 : nroot > 10 ? 10 : nroot;
    for (int r = 0; r < nroot; r++) {
        /* root r + 1 in increasing order lies in (lo, hi] */
        double lo = -R, hi = R;
        for (int it = 0; it < HALVINGS; it++) {
            const double mid = 0.5 * (lo + hi);
            if (vlo - variations(st, deg, nch, mid) >= r + 1)
                hi = mid;
            else
                lo = mid;
        }
        double x = 0.5 * (lo + hi);
        for (int it = 0; it < NEWTON; it++) {
            const double xn = x - horner(st, d, x) / horner(st + 11, d - 1, x);
            if (!(xn >= lo && xn <= hi)) break;
            x = xn;
        }
        root[r] = x;
    }
    /* back-substitution.  From here on the constraint matrix is dead: the candidates take its place. */
    double *Es = ws + WS_E;
    for (int r = 0; r < nroot; r++) {
        const double z = root[r];
        double bx[3], by[3], bc[3];
        for (int i = 0; i < 3; i++) {
            bx[i] = horner(Bp + 13 * i, 3, z);
            by[i] = horner(Bp + 13 * i + 4, 3, z);
            bc[i] = horner(Bp + 13 * i + 8, 4, z);
        }
        const double d01 = bx[0] * by[1] - bx[1] * by[0], d02 = bx[0] * by[2] - bx[2] * by[0],
                     d12 = bx[1] * by[2] - bx[2] * by[1];
        double dd = d01, xa = bx[0], ya = by[0], ca = bc[0], xb = bx[1], yb = by[1], cb = bc[1];
        if (fabs(d02) > fabs(dd)) dd = d02, xb = bx[2], yb = by[2], cb = bc[2];
        if (fabs(d12) > fabs(dd)) dd = d12, xa = bx[1], ya = by[1], ca = bc[1], xb = bx[2], yb = by[2], cb = bc[2];
        const double x = (ya * cb - yb * ca) / dd, y = (xb * ca - xa * cb) / dd;
        double *E = Es + 9 * r;
        double nn = 0.0;
        for (int e = 0; e < 9; e++) {
            E[e] = ((x * bs[e] + y * bs[9 + e]) + z * bs[18 + e]) + bs[27 + e];
            nn = nn + E[e] * E[e];
        }
        const double nr = sqrt(nn);
        int fin = 1;
        for (int e = 0; e < 9; e++) {
            E[e] = E[e] / nr;
            fin &= isfinite(E[e]) != 0;
        }
        if (fin) *ok |= 1u << r;
    }
    return nroot;
}

/* the Sampson distance without its division: (q2^T E q1)^2 <= t2 (a^2 + b^2 + c^2 + d^2) */
static int inlier(const double *E, const double *q, double t2)
{
    const double x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
    const double a = (E[0] * x1 + E[1] * y1) + E[2], b = (E[3] * x1 + E[4] * y1) + E[5], c = (E[6] * x1 + E[7] * y1) + E[8];
    const double d1 = (E[0] * x2 + E[3] * y2) + E[6], d2 = (E[1] * x2 + E[4] * y2) + E[7];
    const double r = (x2 * a + y2 * b) + c;
    return r * r <= t2 * (((a * a + b * b) + d1 * d1) + d2 * d2);
}

static double flog(double x)
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

static int32_t adaptive(int32_t count, int32_t m, int s, double conf)
{
    if (count <= 0) return 0;
    const double w = (double)count / (double)m;
    double p = w;
    for (int k = 1; k < s; k++) p = p * w;
    const double den = 1.0 - p;
    if (!(den > 0.0)) return 1;
    if (!(den < 1.0)) return 2147483647;
    const double r = ceil(flog(1.0 - conf) / flog(den));
    if (!(r < 2147483647.0)) return 2147483647;
    return r < 1.0 ? 1 : (int32_t)r;
}

/* Horn's closed form: b b^T = 1/2 tr(E E^T) I - E E^T, (b.b) R = cof(E) -+ [b]x E; rt: R1 | R2 | t */
static void decompose(const double *E, double *rt)
{
    double G[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) G[3 * i + j] = (E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2];
    const double h = 0.5 * ((G[0] + G[4]) + G[8]);
    const double D[3] = {h - G[0], h - G[4], h - G[8]};
    int im = 0;
    if (D[1] > D[im]) im = 1;
    if (D[2] > D[im]) im = 2;
    const double sd = sqrt(D[im]);
    double b[3];
    for (int j = 0; j < 3; j++) b[j] = (j == im ? D[im] : -G[3 * im + j]) / sd;
    const double bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                           E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                           E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
    for (int j = 0; j < 3; j++) {
        const double be[3] = {b[1] * E[6 + j] - b[2] * E[3 + j], b[2] * E[j] - b[0] * E[6 + j], b[0] * E[3 + j] - b[1] * E[j]};
        for (int i = 0; i < 3; i++) {
            rt[3 * i + j] = (cof[3 * i + j] - be[i]) / bb;
            rt[9 + 3 * i + j] = (cof[3 * i + j] + be[i]) / bb;
        }
    }
    const double nb = sqrt(bb);
    for (int j = 0; j < 3; j++) rt[18 + j] = b[j] / nb;
}

/* both depths of lambda2 q2 = lambda1 R q1 + t from the 2 x 2 normal equations; pose 0 .. 3 = (R1, t) (R2, t) (R1, -t) (R2, -t) */
static int good_depth(const double *rt, int pose, const double *q, double max_depth)
{
    const double *R = rt + ((pose & 1) ? 9 : 0);
    const double x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
    const double t0 = (pose & 2) ? -rt[18] : rt[18], t1 = (pose & 2) ? -rt[19] : rt[19], t2 = (pose & 2) ? -rt[20] : rt[20];
    const double a0 = (R[0] * x1 + R[1] * y1) + R[2], a1 = (R[3] * x1 + R[4] * y1) + R[5], a2 = (R[6] * x1 + R[7] * y1) + R[8];
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2, qq = (x2 * x2 + y2 * y2) + 1.0, aq = (a0 * x2 + a1 * y2) + a2;
    const double at = (a0 * t0 + a1 * t1) + a2 * t2, qt = (x2 * t0 + y2 * t1) + t2;
    const double det = aa * qq - aq * aq;
    const double l1 = (aq * qt - at * qq) / det, l2 = (aa * qt - aq * at) / det;
    return l1 > 0.0 && l1 < max_depth && l2 > 0.0 && l2 < max_depth;
}

/* ---- exported pieces ------------------------------------------------------------------------------------------------ */
/* the minimal solve of 5 normalised correspondences q (5 x 4 doubles): E 10 x 9, roots 10, detp 11, *okmask.  Returns the
 * number of roots or -1. */
int pr_solve5(const double *q, double *E, double *roots, double *detp, uint32_t *okmask)
{
    double ws[WS_SIZE];
    int32_t wi[WI_SIZE];
    memset(E, 0, 90 * sizeof(double));
    memset(roots, 0, 10 * sizeof(double));
    memset(detp, 0, 11 * sizeof(double));
    const int nr = solve5(q, ws, wi, okmask, detp);
    for (int r = 0; r < nr; r++) {
        roots[r] = ws[WS_ROOT + r];
        memcpy(E + 9 * r, ws + WS_E + 9 * r, 9 * sizeof(double));
    }
    return nr;
}

void pr_decompose(const double *E, double *rt) { decompose(E, rt); }
int pr_good_depth(const double *rt, int pose, const double *q, double max_depth) { return good_depth(rt, pose, q, max_depth); }
int pr_inlier(const double *E, const double *q, double t2) { return inlier(E, q, t2); }

/* the consensus counts of hypothesis h's candidates (counts[10], -1 = no such candidate or not finite); returns the
 * number of roots or -1.  qn: m x 4 normalised correspondences. */
static int hypothesis(uint64_t seed, uint32_t h, int32_t m, const double *qn, double t2, double *ws, int32_t *wi,
                      int32_t *counts)
{
    int32_t idx[5];
    uint32_t ok;
    double q[20];
    for (int r = 0; r < 10; r++) counts[r] = -1;
    if (!pr_sample(seed, h, (uint32_t)m, idx)) return -1;
    for (int j = 0; j < 5; j++)
        for (int k = 0; k < 4; k++) q[4 * j + k] = qn[4 * (size_t)idx[j] + k];
    const int nr = solve5(q, ws, wi, &ok, NULL);
    for (int r = 0; r < nr; r++) {
        if (!(ok >> r & 1)) continue;
        int32_t c = 0;
        for (int k = 0; k < m; k++) c += inlier(ws + WS_E + 9 * r, qn + 4 * (size_t)k, t2);
        counts[r] = c;
    }
    return nr;
}

/* the whole E and pose half of pagk_pose_2d2d.  pose: E | R | t (21 doubles); masks: n each (may be NULL); info: 16 words;
 * cand_counts: iters_E x 10 (may be NULL).  status may be NULL.  Returns m. */
int pr_pose(const pr_params *P, double f, double cx, double cy, int32_t n, const float *pts1, const float *pts2,
            const uint8_t *status, double *pose, uint8_t *mask_E, uint8_t *mask_pose, int32_t *info, int32_t *cand_counts)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    double *qn = malloc(sizeof(double) * 4 * nn);
    int32_t *idx = malloc(sizeof(int32_t) * nn);
    int32_t m = 0;
    for (int i = 0; i < n; i++) {
        if (mask_E) mask_E[i] = 0;
        if (mask_pose) mask_pose[i] = 0;
        if (status && !status[i]) continue;
        qn[4 * m] = ((double)pts1[2 * i] - cx) / f, qn[4 * m + 1] = ((double)pts1[2 * i + 1] - cy) / f;
        qn[4 * m + 2] = ((double)pts2[2 * i] - cx) / f, qn[4 * m + 3] = ((double)pts2[2 * i + 1] - cy) / f;
        idx[m++] = i;
    }
    memset(pose, 0, 21 * sizeof(double));
    for (int k = 0; k < INFO_WORDS; k++) info[k] = 0;
    info[1] = m, info[2] = info[3] = -1;
    if (cand_counts)
        for (int k = 0; k < 10 * P->iters_E; k++) cand_counts[k] = -1;
    const double tn = P->thresh_E / f, t2 = tn * tn;
    double ws[WS_SIZE], bestE[9];
    int32_t wi[WI_SIZE];
    int32_t best_h = -1, best_r = -1, best_c = -1, valid_s = 0, valid_c = 0;
    if (m >= 5)
        for (int h = 0; h < P->iters_E; h++) {
            int32_t counts[10];
            const int nr = hypothesis(P->seed, (uint32_t)h, m, qn, t2, ws, wi, counts);
            if (nr < 0) continue;
            valid_s++;
            for (int r = 0; r < nr; r++) {
                if (cand_counts) cand_counts[10 * h + r] = counts[r];
                if (counts[r] < 0) continue;
                valid_c++;
                if (counts[r] > best_c) best_c = counts[r], best_h = h, best_r = r, memcpy(bestE, ws + WS_E + 9 * r, sizeof bestE);
            }
        }
    info[5] = valid_s, info[6] = valid_c;
    if (best_h >= 0) {
        info[2] = best_h, info[3] = best_r, info[4] = best_c;
        info[7] = adaptive(best_c, m, 5, P->conf_E);
    }
    if (best_h >= 0 && best_c >= 5) {
        info[0] = 1;
        memcpy(pose, bestE, sizeof bestE);
        double rt[21];
        decompose(bestE, rt);
        int32_t good[4] = {0, 0, 0, 0};
        for (int k = 0; k < m; k++) {
            if (mask_E) mask_E[idx[k]] = (uint8_t)inlier(bestE, qn + 4 * (size_t)k, t2);
            for (int p = 0; p < 4; p++) good[p] += good_depth(rt, p, qn + 4 * (size_t)k, P->max_depth);
        }
        int bp = 0;
        for (int p = 1; p < 4; p++)
            if (good[p] > good[bp]) bp = p;
        info[8] = bp;
        for (int p = 0; p < 4; p++) info[9 + p] = good[p];
        memcpy(pose + 9, rt + ((bp & 1) ? 9 : 0), 9 * sizeof(double));
        for (int j = 0; j < 3; j++) pose[18 + j] = (bp & 2) ? -rt[18 + j] : rt[18 + j];
        if (mask_pose)
            for (int k = 0; k < m; k++) mask_pose[idx[k]] = (uint8_t)good_depth(rt, bp, qn + 4 * (size_t)k, P->max_depth);
    }
    free(qn), free(idx);
    return m;
}
