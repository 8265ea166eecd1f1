// pagk_gyro_kernel.h -- the IMU window of a frame pair on the device (include/pagk.h "Gyro integration"):
//   k_gyro_integrate  GyroAidedTracker::IntegrateGyroMeasurements, IntegrateOneGyroMeasurement and SetRcl (reference
//                     src/gyro_aided_tracker.cpp:511-587): the window's samples -> Rcl and the nine floats the prediction
//                     reads (rows 0 and 1 of K Rcl K^-1, then the third row of Rcl)
//   k_flow_velocity   mvFlowVelocityInNormalPlane (src/frame.cpp:139-143) behind the hand-over
// tests/gyro_integrate_ref.c restates both in plain C; the kernels return its bits.
//
// k_gyro_integrate is one launch of one wavefront.  Lane i computes the rotation of step i (at most 63 steps) into the LDS;
// every 3 x 3 product that follows is taken by the whole wave at once, lane l holding element l % 9 of the running matrix
// and fetching the row it needs from its neighbours with a cross-lane read: the products keep the defined order (f64
// accumulator from 0, k ascending, one rounding to f32), and there is no barrier but the one behind the per-step phase.
// Plain HIP C++, vector stores only, no atomics.  The window lies in device memory (a part of the sequence's input block,
// or of the host form's staging block), so a captured graph replays with the window of its frame.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pagk {

constexpr int kImuMaxSamples = 64;   // PAGK_IMU_MAX_SAMPLES
// The window as the device reads it: t_ref, t_cur (f64) | n (int32) | bias[3] (f32) | pad to 64 | t[64] (f64) | w[64][3] (f32)
constexpr size_t kImuOffN = 16, kImuOffBias = 20, kImuOffT = 64, kImuOffW = kImuOffT + kImuMaxSamples * 8;
constexpr size_t kImuWindowBytes = kImuOffW + kImuMaxSamples * 12;   // 1344

struct GyroArgs {
    const uint8_t *win;   // kImuWindowBytes, checked by the host (pagk_imu_window_check)
    float Rbc[9];
    float fx, fy, cx, cy;
    float *Rcl;           // 9
    float *rot9;          // 9
};

// the f64 sine and cosine of include/pagk.h's ORB "steering" paragraph for x >= 0: f64 + - * only
__device__ __forceinline__ void gyro_sin_cos(double x, double *sn, double *cs)
{
    constexpr double two_over_pi = 0x1.45f306dc9c883p-1, pio2_hi = 0x1.921fb544p+0, pio2_lo = 0x1.0b4611a626331p-34;
    constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                     S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                     C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    double v = x * two_over_pi + 0.5;
    if (!(v < 2147483647.0)) v = 2147483647.0;   // the conversion saturates
    const int k = (int)v;
    const double kd = (double)k;
    const double t = (x - kd * pio2_hi) - kd * pio2_lo;
    const double z = t * t;
    const double s = t + t * (z * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))))));
    const double c = 1.0 - z * (0.5 - z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))))));
    const int q = k & 3;
    *cs = q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
    *sn = q == 0 ? s : (q == 1 ? c : (q == 2 ? -s : -c));
}

// IntegrateOneGyroMeasurement (:564-587); R is a register array (every index is a constant after unrolling)
__device__ __forceinline__ void gyro_one_step(float gx, float gy, float gz, const float *bias, float tstep, float (&R)[9])
{
    const float x = (float)((double)(gx - bias[0]) * (double)tstep);
    const float y = (float)((double)(gy - bias[1]) * (double)tstep);
    const float z = (float)((double)(gz - bias[2]) * (double)tstep);
    const float d2 = x * x + y * y + z * z;
    const float d = __fsqrt_rn(d2);
    const float w[9] = {0.0f, -z, y, z, 0.0f, -x, -y, x, 0.0f};
    const float eye[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if ((double)d < 1e-4) {
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = eye[k] + w[k];
        return;
    }
    double sn, cs;
    gyro_sin_cos((double)d, &sn, &cs);
    const double s = (double)(float)sn;            // std::sin(float) returns float
    const double c = (double)(1.0f - (float)cs);   // 1.0f - std::cos(float): an f32 difference
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) acc += (double)w[r * 3 + k] * (double)w[k * 3 + q];
            const float ww = (float)acc;
            R[r * 3 + q] = (float)(((double)eye[r * 3 + q] + (double)w[r * 3 + q] * s / (double)d) + (double)ww * c / (double)d2);
        }
}

// element (r, c) of A B with row r of A in a0..a2 and column c of B in b0..b2
__device__ __forceinline__ float gyro_dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    double s = 0.0;
    s += (double)a0 * (double)b0;
    s += (double)a1 * (double)b1;
    s += (double)a2 * (double)b2;
    return (float)s;
}

// (the body is a function of its own so that pagk_group_sensor_kernel.h can run it for one of several cameras per launch)
__device__ __forceinline__ void gyro_integrate_body(const GyroArgs &a)
{
    __shared__ float s_delta[kImuMaxSamples * 9];
    __shared__ float s_mat[3 * 9];   // Rbc | K | K^-1
    const int lane = (int)threadIdx.x;
    const double t_ref = *reinterpret_cast<const double *>(a.win), t_cur = *reinterpret_cast<const double *>(a.win + 8);
    int ns = *reinterpret_cast<const int32_t *>(a.win + kImuOffN);
    ns = min(max(ns, 0), kImuMaxSamples);   // (the host has checked the window; nothing reads beyond the block either way)
    const int n = ns - 1;
    const float *bias = reinterpret_cast<const float *>(a.win + kImuOffBias);
    const double *t = reinterpret_cast<const double *>(a.win + kImuOffT);
    const float *w = reinterpret_cast<const float *>(a.win + kImuOffW);

    {   // the constant matrices into the LDS, every index a compile-time constant
        const float K[9] = {a.fx, 0.0f, a.cx, 0.0f, a.fy, a.cy, 0.0f, 0.0f, 1.0f};
        double m[3][3];
#pragma unroll
        for (int k = 0; k < 9; k++) m[k / 3][k % 3] = (double)K[k];
        const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
        const double d = det != 0.0 ? 1.0 / det : 0.0;
        const float Ki[9] = {(float)((m[1][1] * m[2][2] - m[1][2] * m[2][1]) * d), (float)((m[0][2] * m[2][1] - m[0][1] * m[2][2]) * d),
                             (float)((m[0][1] * m[1][2] - m[0][2] * m[1][1]) * d), (float)((m[1][2] * m[2][0] - m[1][0] * m[2][2]) * d),
                             (float)((m[0][0] * m[2][2] - m[0][2] * m[2][0]) * d), (float)((m[0][2] * m[1][0] - m[0][0] * m[1][2]) * d),
                             (float)((m[1][0] * m[2][1] - m[1][1] * m[2][0]) * d), (float)((m[0][1] * m[2][0] - m[0][0] * m[2][1]) * d),
                             (float)((m[0][0] * m[1][1] - m[0][1] * m[1][0]) * d)};
#pragma unroll
        for (int k = 0; k < 9; k++)
            if (lane == k) s_mat[k] = a.Rbc[k], s_mat[9 + k] = K[k], s_mat[18 + k] = Ki[k];
    }

    if (lane < n) {   // step `lane` (:530-555, the four cases in the reference's order)
        const int i = lane;
        const float w0x = w[3 * i], w0y = w[3 * i + 1], w0z = w[3 * i + 2];
        const float w1x = w[3 * i + 3], w1y = w[3 * i + 4], w1z = w[3 * i + 5];
        const double t0 = t[i], t1 = t[i + 1];
        float tstep, ax, ay, az;
        if (i == 0 && i < n - 1) {
            const float tab = (float)(t1 - t0), tini = (float)(t0 - t_ref), r = __fdiv_rn(tini, tab);
            ax = ((w0x + w1x) - (w1x - w0x) * r) * 0.5f, ay = ((w0y + w1y) - (w1y - w0y) * r) * 0.5f;
            az = ((w0z + w1z) - (w1z - w0z) * r) * 0.5f;
            tstep = (float)(t1 - t_ref);
        } else if (i < n - 1) {
            ax = (w0x + w1x) * 0.5f, ay = (w0y + w1y) * 0.5f, az = (w0z + w1z) * 0.5f;
            tstep = (float)(t1 - t0);
        } else if (i > 0) {   // && i == n - 1
            const float tab = (float)(t1 - t0), tend = (float)(t1 - t_cur), r = __fdiv_rn(tend, tab);
            ax = ((w0x + w1x) - (w1x - w0x) * r) * 0.5f, ay = ((w0y + w1y) - (w1y - w0y) * r) * 0.5f;
            az = ((w0z + w1z) - (w1z - w0z) * r) * 0.5f;
            tstep = (float)(t_cur - t0);
        } else {              // i == 0 && i == n - 1
            ax = w0x, ay = w0y, az = w0z;
            tstep = (float)(t_cur - t_ref);
        }
        float R[9];
        gyro_one_step(ax, ay, az, bias, tstep, R);
#pragma unroll
        for (int k = 0; k < 9; k++) s_delta[i * 9 + k] = R[k];
    }
    __syncthreads();

    // lane l holds element e = l % 9 of the running matrix (the lanes from 9 on repeat the first nine: every lane takes
    // part in the cross-lane reads)
    const int e = lane % 9, r = e / 3, c = e % 3;
    float v = r == c ? 1.0f : 0.0f;   // dR = I
    for (int i = 0; i < n; i++) {     // dR = dR * deltaR_i, left to right
        const float a0 = __shfl(v, r * 3), a1 = __shfl(v, r * 3 + 1), a2 = __shfl(v, r * 3 + 2);
        v = gyro_dot3(a0, a1, a2, s_delta[i * 9 + c], s_delta[i * 9 + 3 + c], s_delta[i * 9 + 6 + c]);
    }
    {   // m = Rbc^T dR^T: m[r][c] = sum_k Rbc[k][r] dR[c][k]
        const float b0 = __shfl(v, c * 3), b1 = __shfl(v, c * 3 + 1), b2 = __shfl(v, c * 3 + 2);
        v = gyro_dot3(s_mat[r], s_mat[3 + r], s_mat[6 + r], b0, b1, b2);
    }
    {   // Rcl = m Rbc (:560)
        const float a0 = __shfl(v, r * 3), a1 = __shfl(v, r * 3 + 1), a2 = __shfl(v, r * 3 + 2);
        v = gyro_dot3(a0, a1, a2, s_mat[c], s_mat[3 + c], s_mat[6 + c]);
    }
    const float rcl = v;
    {   // K Rcl (:518)
        const float b0 = __shfl(v, c), b1 = __shfl(v, 3 + c), b2 = __shfl(v, 6 + c);
        v = gyro_dot3(s_mat[9 + r * 3], s_mat[9 + r * 3 + 1], s_mat[9 + r * 3 + 2], b0, b1, b2);
    }
    {   // (K Rcl) K^-1
        const float a0 = __shfl(v, r * 3), a1 = __shfl(v, r * 3 + 1), a2 = __shfl(v, r * 3 + 2);
        v = gyro_dot3(a0, a1, a2, s_mat[18 + c], s_mat[18 + 3 + c], s_mat[18 + 6 + c]);
    }
    if (lane < 9) {
        a.Rcl[lane] = rcl;
        a.rot9[lane] = lane < 6 ? v : rcl;   // rows 0 and 1 of K Rcl K^-1, then the third row of Rcl
    }
}

__global__ void __launch_bounds__(64) k_gyro_integrate(GyroArgs a) { gyro_integrate_body(a); }

struct FlowVelocityArgs {
    const float *normal_cur, *normal_last;   // cap x 2
    const int32_t *index_in_last;            // cap
    const int32_t *state;                    // [0]: the live count of the new key set
    const uint8_t *win;                      // t_ref (the last frame's time) and t_cur
    float *v;                                // cap x 2
    int32_t cap;
};

// Row j of the new key set: ((normal_cur[j] - normal_last[i]) in f32) / (t_cur - t_last) as Point2f / double divides (an f64
// quotient rounded once); (0, 0) for a row the top-up added and for rows at or beyond the live count.
__device__ __forceinline__ void flow_velocity_body(const FlowVelocityArgs &a)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= a.cap) return;
    const double dt = *reinterpret_cast<const double *>(a.win + 8) - *reinterpret_cast<const double *>(a.win);
    const int live = a.state[0], i = a.index_in_last[j];
    float2 o = make_float2(0.0f, 0.0f);
    if (j < live && i >= 0 && i < a.cap) {
        const float2 cur = reinterpret_cast<const float2 *>(a.normal_cur)[j], last = reinterpret_cast<const float2 *>(a.normal_last)[i];
        const float dx = cur.x - last.x, dy = cur.y - last.y;
        o.x = (float)((double)dx / dt), o.y = (float)((double)dy / dt);
    }
    reinterpret_cast<float2 *>(a.v)[j] = o;
}

__global__ void __launch_bounds__(256) k_flow_velocity(FlowVelocityArgs a) { flow_velocity_body(a); }

}  // namespace pagk
