/*
 * inverse_ref.c -- the template-Jacobian mode (pagk_params::inverse == PAGK_INVERSE_TEMPLATE, include/pagk.h) in plain
 * sequential C: what every entry point of the library must return, bit for bit.
 *
 * TEST INFRASTRUCTURE ONLY.  The sampler, the pyramid, the 4 x 4 solve and the software log are the oracle library's
 * exported functions (one source for each); everything else -- the level loop, the set-up, the sums and their order, the
 * penalty, the termination rules, NCC, the distortion and the outputs -- is restated here.
 *
 * Build: gcc -O2 -ffp-contract=off -fno-fast-math (one IEEE rounding per operation), like the oracle and the library.
 * "file:line" citations are relative to the reference checkout, as in oracle/pagk_oracle.c.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/pagk_oracle.h"

int inverse_ref_track_pyr(const pagk_params *p, int32_t n_levels, const pagk_image *ref_levels, const pagk_image *cur_levels,
                          int32_t n, const float *pt_ref, const float *pt_init, const float *affine, const uint8_t *status_in,
                          const pagk_outputs *out);
int inverse_ref_track(const pagk_params *p, const pagk_image *ref, const pagk_image *cur, int32_t n, const float *pt_ref,
                      const float *pt_init, const float *affine, const uint8_t *status_in, const pagk_outputs *out);
double inverse_ref_sum_f64(const double *term, int32_t count);
float inverse_ref_sum_f32(const float *term, int32_t count);

/* ---- the order of every sum over the patch -------------------------------------------------------------------------------
 * term k belongs to slot k mod 64; a slot starts at +0.0 and adds its terms in ascending k; then six steps
 * v[s] = v[s] + v[s ^ m] over all slots at once, m = 1, 2, 4, 8, 16, 32; the sum is v[0]. */
double inverse_ref_sum_f64(const double *term, int32_t count)
{
    double v[64], w[64];
    for (int s = 0; s < 64; s++) v[s] = 0.0;
    for (int32_t k = 0; k < count; k++) v[k % 64] = v[k % 64] + term[k];
    for (int m = 1; m < 64; m *= 2) {
        for (int s = 0; s < 64; s++) w[s] = v[s] + v[s ^ m];
        memcpy(v, w, sizeof v);
    }
    return v[0];
}

float inverse_ref_sum_f32(const float *term, int32_t count)
{
    float v[64], w[64];
    for (int s = 0; s < 64; s++) v[s] = 0.0f;
    for (int32_t k = 0; k < count; k++) v[k % 64] = v[k % 64] + term[k];
    for (int m = 1; m < 64; m *= 2) {
        for (int s = 0; s < 64; s++) w[s] = v[s] + v[s ^ m];
        memcpy(v, w, sizeof v);
    }
    return v[0];
}

/* PatchMatch::NCC, src/patch_match.cpp:433-469: x outer, y inner (:438-439), float sums in that order. */
static float ncc_patch(int h, const pagk_image *ref, const pagk_image *cur, float rx, float ry, float cx, float cy,
                       const float *A, float *xy, float *vr, float *vc)
{
    const int P = (2 * h + 1) * (2 * h + 1);
    int k = 0;
    for (int x = -h; x <= h; x++)
        for (int y = -h; y <= h; y++, k++) {
            xy[2 * k] = rx + x;
            xy[2 * k + 1] = ry + y;
        }
    pagk_oracle_sample(ref, P, xy, vr);
    k = 0;
    for (int x = -h; x <= h; x++)
        for (int y = -h; y <= h; y++, k++) {
            if (!A) {
                xy[2 * k] = cx + x;
                xy[2 * k + 1] = cy + y;
            } else {
                float wx = A[0] * x + A[1] * y;
                float wy = A[2] * x + A[3] * y;
                xy[2 * k] = cx + wx;
                xy[2 * k + 1] = cy + wy;
            }
        }
    pagk_oracle_sample(cur, P, xy, vc);
    float mean_ref = 0.0f, mean_cur = 0.0f;
    for (int i = 0; i < P; i++) {
        mean_ref += vr[i];
        mean_cur += vc[i];
    }
    mean_ref /= (float)P;
    mean_cur /= (float)P;
    float numerator = 0, den1 = 0, den2 = 0;
    for (int i = 0; i < P; i++) {
        numerator += ((vr[i] - mean_ref) * (vc[i] - mean_cur));
        den1 += (vr[i] - mean_ref) * (vr[i] - mean_ref);
        den2 += (vc[i] - mean_cur) * (vc[i] - mean_cur);
    }
    return (float)((double)numerator / sqrt((double)(den1 * den2) + 1e-10)); /* :468 */
}

/* DistortVecPoints, src/utils.cpp:49-76, one point (src/patch_match.cpp:409-416). */
static void distort_point(const pagk_params *p, float ux, float uy, float *ox, float *oy)
{
    if (p->dist_coef[0] == 0.0) { /* :410 */
        *ox = ux;
        *oy = uy;
        return;
    }
    float mfx = p->fx, mfy = p->fy, mcx = p->cx, mcy = p->cy;
    float mfx_inv = (float)(1.0 / (double)mfx), mfy_inv = (float)(1.0 / (double)mfy);
    float K1 = p->dist_coef[0], K2 = p->dist_coef[1], mp1 = p->dist_coef[2], mp2 = p->dist_coef[3];
    float K3 = p->n_dist_coef == 5 ? p->dist_coef[4] : 0;
    float x = (ux - mcx) * mfx_inv;
    float y = (uy - mcy) * mfy_inv;
    float r2 = x * x + y * y;
    float r4 = r2 * r2;
    float r6 = r4 * r2;
    float x_distort = x * (1 + K1 * r2 + K2 * r4 + K3 * r6) + 2 * mp1 * x * y + mp2 * (r2 + 2 * x * x);
    float y_distort = y * (1 + K1 * r2 + K2 * r4 + K3 * r6) + mp1 * (r2 + 2 * y * y) + 2 * mp2 * x * y;
    *ox = mfx * x_distort + mcx;
    *oy = mfy * y_distort + mcy;
}

typedef struct {
    float *xy, *T, *e, *t32, *wx, *wy, *s5; /* P pairs, P, P, P, P, P, 5 P */
    double (*J)[4];                         /* P */
    double *t64;                            /* P */
} scratch_t;

/* One feature on one level: the loop of include/pagk.h, "Template-Jacobian mode".  Returns the iterations executed. */
static int one_level(const pagk_params *p, float inv_log_max_dist, const pagk_image *img1, const pagk_image *img2, float ptx,
                     float pty, const float *A, float *dx_io, float *dy_io, int *succ_out, float *last_cost_out, scratch_t *s)
{
    const int h = p->half_patch, W = 2 * h + 1, P = W * W;
    float dx = *dx_io, dy = *dy_io, dg = 0.0f, db = 0.0f; /* :186-191 */
    float lastCost = 0.0f;
    int succ = 1, iters = 0;

    /* ---- set-up, once: T, Ix, Iy from the reference image, J, Hp ---- */
    int k = 0;
    for (int y = -h; y <= h; y++)       /* :233 */
        for (int x = -h; x <= h; x++) { /* :234 */
            const float X = ptx + x, Y = pty + y;
            float *q = s->xy + 10 * k;
            q[0] = X, q[1] = Y;
            q[2] = X + 1, q[3] = Y;
            q[4] = X - 1, q[5] = Y;
            q[6] = X, q[7] = Y + 1;
            q[8] = X, q[9] = Y - 1;
            /* :203-204 warp_patch; without the warp (wx, wy) = (x, y) (:235) */
            s->wx[k] = A ? A[0] * x + A[1] * y : (float)x;
            s->wy[k] = A ? A[2] * x + A[3] * y : (float)y;
            k++;
        }
    pagk_oracle_sample(img1, 5 * P, s->xy, s->s5);
    float c;
    {
        const float centre[2] = {ptx, pty};
        pagk_oracle_sample(img1, 1, centre, &c); /* :263: the patch CENTRE */
    }
    for (k = 0; k < P; k++) {
        const float *v = s->s5 + 5 * k;
        s->T[k] = v[0];
        const float Ix = (float)(0.5 * (double)(v[1] - v[2])); /* :269-270 */
        const float Iy = (float)(0.5 * (double)(v[3] - v[4])); /* :271-272 */
        s->J[k][0] = Ix;                                       /* :273-274 */
        s->J[k][1] = Iy;
        s->J[k][2] = -c;
        s->J[k][3] = 1;
    }
    double Hp[4][4];
    for (int r = 0; r < 4; r++)
        for (int cc = 0; cc <= r; cc++) {
            for (k = 0; k < P; k++) s->t64[k] = s->J[k][r] * s->J[k][cc]; /* exact */
            Hp[r][cc] = Hp[cc][r] = inverse_ref_sum_f64(s->t64, P);
        }

    for (int iter = 0; iter < p->iterations; iter++) { /* :215 */
        iters++;
        for (k = 0; k < P; k++) {
            s->xy[2 * k] = ptx + dx + s->wx[k];
            s->xy[2 * k + 1] = pty + dy + s->wy[k];
        }
        pagk_oracle_sample(img2, P, s->xy, s->e);
        for (k = 0; k < P; k++) s->e[k] = s->e[k] + db - (1.0f + dg) * s->T[k]; /* :252-253 */

        double H[4][4], b[4];
        for (int r = 0; r < 4; r++) {
            for (k = 0; k < P; k++) s->t64[k] = (-s->J[k][r]) * (double)s->e[k]; /* :293, exact */
            b[r] = inverse_ref_sum_f64(s->t64, P);
        }
        for (k = 0; k < P; k++) s->t32[k] = s->e[k] * s->e[k]; /* :294 float */
        float cost = inverse_ref_sum_f32(s->t32, P);
        memcpy(H, Hp, sizeof H);

        if (p->regularization_penalty) { /* :302-314, on the fresh copy of H */
            double d = (double)sqrtf(dx * dx + dy * dy);
            double e_penalty = (double)(p->lambda * inv_log_max_dist) * pagk_oracle_log((double)p->alpha * d + 1);
            double jpx = (double)(p->lambda * inv_log_max_dist * p->alpha) / ((double)p->alpha * d + 1) * ((double)dx / d);
            double jpy = (double)(p->lambda * inv_log_max_dist * p->alpha) / ((double)p->alpha * d + 1) * ((double)dy / d);
            double JP[4] = {jpx, jpy, 0, 0};
            for (int r = 0; r < 4; r++)
                for (int cc = 0; cc < 4; cc++) H[r][cc] += JP[r] * JP[cc];
            for (int r = 0; r < 4; r++) b[r] += JP[r] * e_penalty;
            cost = (float)((double)cost + e_penalty * e_penalty);
        }

        double update[4];
        double unorm = pagk_oracle_llt_solve4(&H[0][0], b, update); /* :319 */
        if (isnan(update[0])) {                                    /* :322-326 */
            succ = 0;
            break;
        }
        if (iter > 0 && cost > lastCost) break; /* :328-329 */
        dx = (float)((double)dx + update[0]);   /* :332 */
        dy = (float)((double)dy + update[1]);
        if (p->consider_illumination) { /* :334-337 */
            dg = (float)((double)dg + update[2]);
            db = (float)((double)db + update[3]);
        }
        lastCost = cost;
        succ = 1;
        if (unorm < 1e-2) break; /* :343 */
    }
    *dx_io = dx;
    *dy_io = dy;
    *succ_out = succ;
    *last_cost_out = lastCost;
    return iters;
}

int inverse_ref_track_pyr(const pagk_params *p, int32_t n_levels, const pagk_image *l1, const pagk_image *l2, int32_t n,
                          const float *pt_ref, const float *pt_init, const float *affine, const uint8_t *status_in,
                          const pagk_outputs *out)
{
    if (!p || p->half_patch < 1 || p->half_patch > PAGK_MAX_HALF_PATCH || p->iterations < 0 || n_levels < 1 ||
        n_levels > PAGK_MAX_PYRAMIDS || n_levels != p->pyramids || !l1 || !l2)
        return PAGK_E_ARG;
    if (n < 0 || !out || !out->pt_un || !out->status) return PAGK_E_ARG;
    if (n > 0 && (!pt_ref || !status_in)) return PAGK_E_ARG;
    if (n > 0 && p->has_gyro_predict_initial && !pt_init) return PAGK_E_ARG;
    if (n > 0 && p->consider_affine && !affine) return PAGK_E_ARG;

    const int h = p->half_patch, P = (2 * h + 1) * (2 * h + 1);
    float scales[PAGK_MAX_PYRAMIDS];
    for (int l = 0; l < n_levels; l++) scales[l] = l == 0 ? 1.0f : (float)((double)scales[l - 1] * 0.5); /* :66, :73 */
    float inv_log = p->inv_log_max_dist;
    if (inv_log == 0.0f) { /* :51 */
        float arg = p->alpha * (float)p->max_distance + 1;
        inv_log = (float)(1.0 / (double)logf(arg));
    }
    const double win_size_inv = (double)(1.0f / (2.0f * h + 1.0f) / (2.0f * h + 1.0f)); /* :57 */

    scratch_t s;
    s.xy = (float *)malloc(sizeof(float) * 10 * (size_t)P);
    s.T = (float *)malloc(sizeof(float) * (size_t)P);
    s.e = (float *)malloc(sizeof(float) * (size_t)P);
    s.t32 = (float *)malloc(sizeof(float) * (size_t)P);
    s.wx = (float *)malloc(sizeof(float) * (size_t)P);
    s.wy = (float *)malloc(sizeof(float) * (size_t)P);
    s.s5 = (float *)malloc(sizeof(float) * 5 * (size_t)P);
    s.J = (double(*)[4])malloc(sizeof(double) * 4 * (size_t)P);
    s.t64 = (double *)malloc(sizeof(double) * (size_t)P);

    for (int i = 0; i < n; i++) {
        const float *init = p->has_gyro_predict_initial ? pt_init : pt_ref; /* :83-90 */
        float p2x = init[2 * i], p2y = init[2 * i + 1];
        int succ = 0, iters = 0, ran = 0;
        float lastCost = 0.0f, ncc = 0.0f;
        if (status_in[i]) { /* :173 */
            const float *A = p->consider_affine ? affine + 4 * (size_t)i : NULL;
            for (int level = n_levels - 1; level >= 0; level--) { /* :98 */
                float ptx = pt_ref[2 * i] * scales[level], pty = pt_ref[2 * i + 1] * scales[level]; /* :177 */
                float nx, ny;
                if (level == n_levels - 1) { /* :180 */
                    nx = p2x * scales[level];
                    ny = p2y * scales[level];
                } else { /* :182 */
                    nx = (float)((double)(p2x * 1.0f) / 0.5);
                    ny = (float)((double)(p2y * 1.0f) / 0.5);
                }
                float dx = nx - ptx, dy = ny - pty;
                iters += one_level(p, inv_log, &l1[level], &l2[level], ptx, pty, A, &dx, &dy, &succ, &lastCost, &s);
                p2x = ptx + dx; /* :348 */
                p2y = pty + dy;
            }
            ran = 1;
            ncc = 1; /* :365 */
            if (p->calculate_ncc) /* :356-363, on the level-0 images */
                ncc = ncc_patch(h, &l1[0], &l2[0], pt_ref[2 * i], pt_ref[2 * i + 1], p2x, p2y, A, s.xy, s.s5, s.s5 + P);
        }
        out->pt_un[2 * i] = p2x;
        out->pt_un[2 * i + 1] = p2y;
        out->status[i] = (uint8_t)(ran ? succ : 0);                                             /* :351, :381 */
        if (out->pix_err) out->pix_err[i] = ran ? sqrt((double)lastCost * win_size_inv) : 0.0; /* :352 */
        if (out->dist_pred) {                                                                   /* :384-385 */
            const float *pred = pt_init ? pt_init : pt_ref;
            float ddx = pred[2 * i] - p2x, ddy = pred[2 * i + 1] - p2y;
            out->dist_pred[i] = (double)sqrtf(ddx * ddx + ddy * ddy);
        }
        if (out->pt_dist) distort_point(p, p2x, p2y, &out->pt_dist[2 * i], &out->pt_dist[2 * i + 1]); /* :116 */
        if (out->ncc) out->ncc[i] = ncc;
        if (out->iters) out->iters[i] = iters;
    }
    free(s.xy);
    free(s.T);
    free(s.e);
    free(s.t32);
    free(s.wx);
    free(s.wy);
    free(s.s5);
    free(s.J);
    free(s.t64);
    return PAGK_OK;
}

/* PatchMatch::CreatePyramids, src/patch_match.cpp:61-76: every level in a heap block of exactly its size. */
int inverse_ref_track(const pagk_params *p, const pagk_image *ref, const pagk_image *cur, int32_t n, const float *pt_ref,
                      const float *pt_init, const float *affine, const uint8_t *status_in, const pagk_outputs *out)
{
    if (!p || p->pyramids < 1 || p->pyramids > PAGK_MAX_PYRAMIDS || !ref || !cur || !ref->data || !cur->data) return PAGK_E_ARG;
    if (ref->width != cur->width || ref->height != cur->height) return PAGK_E_ARG;
    pagk_image lv[2][PAGK_MAX_PYRAMIDS];
    uint8_t *own[2][PAGK_MAX_PYRAMIDS];
    memset(own, 0, sizeof own);
    int rc = PAGK_OK;
    for (int k = 0; k < 2 && !rc; k++) {
        lv[k][0] = k == 0 ? *ref : *cur;
        for (int l = 1; l < p->pyramids && !rc; l++) {
            const pagk_image *pv = &lv[k][l - 1];
            const int dw = (int)(pv->width * 0.5), dh = (int)(pv->height * 0.5); /* :69 */
            if (pv->width < 2 || pv->height < 2 || dw < 1 || dh < 1) {
                rc = PAGK_E_ARG;
                break;
            }
            own[k][l] = (uint8_t *)malloc((size_t)dw * (size_t)dh);
            rc = pagk_oracle_pyr_down(pv->data, pv->width, pv->height, pv->step, own[k][l]);
            lv[k][l].data = own[k][l];
            lv[k][l].width = dw;
            lv[k][l].height = dh;
            lv[k][l].step = dw;
        }
    }
    if (!rc) rc = inverse_ref_track_pyr(p, p->pyramids, lv[0], lv[1], n, pt_ref, pt_init, affine, status_in, out);
    for (int k = 0; k < 2; k++)
        for (int l = 0; l < PAGK_MAX_PYRAMIDS; l++) free(own[k][l]);
    return rc;
}
