/* gyro_integrate_ref.c -- the "Gyro integration" section of include/pagk.h restated in plain C: the window checks, the
 * window-to-rotation arithmetic (reference src/gyro_aided_tracker.cpp:511-587) and the flow velocity of the sensor sequence
 * (src/frame.cpp:139-143).  Sequential, one rounding per operation (build with -ffp-contract=off); no libm call but sqrtf,
 * which IEEE 754 rounds correctly.  tests/gyro_integrate_ref_util.py builds it against oracle/libpagk_oracle.so and loads it. */
#include <math.h>
#include <stdint.h>

#include "../oracle/pagk_oracle.h"

#define GI_MAX_SAMPLES 64

/* The f64 sine and cosine, the 3x3 f32 product (f32 factors, an f64 accumulator starting at 0, k ascending, one rounding to
 * f32) and the f64 cofactor inverse are defined once, in oracle/pagk_oracle.c: the stand-in cv::Mat under the reference's own
 * src/gyro_aided_tracker.cpp (oracle/ref_shim) calls the same functions. */
#define gi_sin_cos pagk_oracle_sin_cos
#define gi_inv3 pagk_oracle_mat_inv3
static void gi_mul3(const float *a, const float *b, float *o) { pagk_oracle_mat_mul(3, 3, 3, a, b, o); }

static void gi_transpose(const float *a, float *o)
{
    float m[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[c * 3 + r] = a[r * 3 + c];
    for (int k = 0; k < 9; k++) o[k] = m[k];
}

/* IntegrateOneGyroMeasurement (:564-587) */
void gyro_ref_one_step(const float gyro[3], const float bias[3], float tstep, float R[9])
{
    const float x = (float)((double)(gyro[0] - bias[0]) * (double)tstep);
    const float y = (float)((double)(gyro[1] - bias[1]) * (double)tstep);
    const float z = (float)((double)(gyro[2] - bias[2]) * (double)tstep);
    const float d2 = x * x + y * y + z * z;
    const float d = sqrtf(d2);
    const float w[9] = {0.0f, -z, y, z, 0.0f, -x, -y, x, 0.0f};
    const float eye[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if ((double)d < 1e-4) {
        for (int k = 0; k < 9; k++) R[k] = eye[k] + w[k];
        return;
    }
    float ww[9];
    gi_mul3(w, w, ww);
    double sn, cs;
    gi_sin_cos((double)d, &sn, &cs);
    const double s = (double)(float)sn;                 /* std::sin(float) returns float */
    const double c = (double)(1.0f - (float)cs);        /* 1.0f - std::cos(float): an f32 difference */
    for (int k = 0; k < 9; k++)
        R[k] = (float)(((double)eye[k] + (double)w[k] * s / (double)d) + (double)ww[k] * c / (double)d2);
}

/* 0 if the window may be integrated, -1 (PAGK_E_ARG) otherwise */
int gyro_ref_window_check(double t_ref, double t_cur, int32_t n, const double *t, const float *w, const float bias[3],
                          int32_t imu_cap)
{
    if (imu_cap < 1 || imu_cap > GI_MAX_SAMPLES || n < 0 || n > imu_cap || !bias) return -1;
    if (!isfinite(t_ref) || !isfinite(t_cur) || !(t_cur > t_ref)) return -1;
    if (n > 0 && (!t || !w)) return -1;
    for (int k = 0; k < 3; k++)
        if (!isfinite(bias[k])) return -1;
    for (int32_t i = 0; i < n; i++) {
        if (!isfinite(t[i]) || !isfinite(w[3 * i]) || !isfinite(w[3 * i + 1]) || !isfinite(w[3 * i + 2])) return -1;
        if (i > 0 && !(t[i] > t[i - 1])) return -1;
    }
    return 0;
}

/* IntegrateGyroMeasurements and SetRcl (:511-562): Rcl, and rot9 = rows 0 and 1 of K Rcl K^-1, then the third row of Rcl */
int gyro_ref_integrate(const float Rbc[9], float fx, float fy, float cx, float cy, double t_ref, double t_cur, int32_t n_samples,
                       const double *t, const float *w, const float bias[3], float Rcl[9], float rot9[9])
{
    if (gyro_ref_window_check(t_ref, t_cur, n_samples, t, w, bias, GI_MAX_SAMPLES)) return -1;
    float dR[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    const int n = n_samples - 1;
    for (int i = 0; i < n; i++) {
        const float *w0 = w + 3 * i, *w1 = w + 3 * (i + 1);
        const double t0 = t[i], t1 = t[i + 1];
        float tstep = 0.0f, av[3] = {0.0f, 0.0f, 0.0f};
        if (i == 0 && i < n - 1) {
            const float tab = (float)(t1 - t0), tini = (float)(t0 - t_ref), r = tini / tab;
            for (int k = 0; k < 3; k++) av[k] = ((w0[k] + w1[k]) - (w1[k] - w0[k]) * r) * 0.5f;
            tstep = (float)(t1 - t_ref);
        } else if (i < n - 1) {
            for (int k = 0; k < 3; k++) av[k] = (w0[k] + w1[k]) * 0.5f;
            tstep = (float)(t1 - t0);
        } else if (i > 0 && i == n - 1) {
            const float tab = (float)(t1 - t0), tend = (float)(t1 - t_cur), r = tend / tab;
            for (int k = 0; k < 3; k++) av[k] = ((w0[k] + w1[k]) - (w1[k] - w0[k]) * r) * 0.5f;
            tstep = (float)(t_cur - t0);
        } else {   /* i == 0 && i == n - 1 */
            for (int k = 0; k < 3; k++) av[k] = w0[k];
            tstep = (float)(t_cur - t_ref);
        }
        float R[9];
        gyro_ref_one_step(av, bias, tstep, R);
        gi_mul3(dR, R, dR);
    }
    float RbcT[9], dRT[9], m[9];
    gi_transpose(Rbc, RbcT);
    gi_transpose(dR, dRT);
    gi_mul3(RbcT, dRT, m);
    gi_mul3(m, Rbc, Rcl);
    const float K[9] = {fx, 0.0f, cx, 0.0f, fy, cy, 0.0f, 0.0f, 1.0f};
    float Kinv[9], KR[9], KRK[9];
    gi_inv3(K, Kinv);
    gi_mul3(K, Rcl, KR);
    gi_mul3(KR, Kinv, KRK);
    for (int k = 0; k < 6; k++) rot9[k] = KRK[k];
    for (int k = 0; k < 3; k++) rot9[6 + k] = Rcl[6 + k];
    return 0;
}

/* mvFlowVelocityInNormalPlane (src/frame.cpp:139-143) over `cap` rows: Point2f / double */
void gyro_ref_flow_velocity(int32_t cap, int32_t live, const float *normal_cur, const float *normal_last,
                            const int32_t *index_in_last, double t_cur, double t_last, float *v)
{
    const double dt = t_cur - t_last;
    for (int32_t j = 0; j < cap; j++) {
        const int32_t i = index_in_last[j];
        if (j >= live || i < 0 || i >= cap) {
            v[2 * j] = v[2 * j + 1] = 0.0f;
            continue;
        }
        const float dx = normal_cur[2 * j] - normal_last[2 * i], dy = normal_cur[2 * j + 1] - normal_last[2 * i + 1];
        v[2 * j] = (float)((double)dx / dt);
        v[2 * j + 1] = (float)((double)dy / dt);
    }
}
