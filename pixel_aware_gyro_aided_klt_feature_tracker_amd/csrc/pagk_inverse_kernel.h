// pagk_inverse_kernel.h -- k_inv_wave: PAGK_INVERSE_TEMPLATE (pagk_params::inverse == 2), one wavefront per feature.
//
// The mode include/pagk.h defines under "Template-Jacobian mode": the Jacobian J_k = (Ix_k, Iy_k, -c, 1) is taken from the
// REFERENCE image once per level and kept per pixel, Hp = sum J J^T is reduced once per level, and an iteration is one img2
// sample per pixel, the residual, b = sum (-J) e, cost = sum e e, H = Hp (+ penalty), the solve and the update.  Level loop,
// initial points, warp, sampler, residual association, penalty, solver_variant, termination rules, NCC and outputs are the
// forward path's (pagk_wave_kernel.h), line for line.
//
// Lane l owns the pixels l, l + 64, ... (row-major, y outer) and keeps their T, Ix, Iy in registers for the level.  Nothing
// leaves the wave: no LDS inside the Gauss-Newton loop, no barrier, no flag, no atomic, no workspace.
//
// The sums.  Every sum over the patch (ten of Hp, four of b, the cost) is taken in ONE order that depends on half_patch alone:
//   1. pixel k belongs to lane k mod 64; a lane starts at +0.0 and adds its pixels in ascending k;
//   2. six steps v = v + v[lane ^ m], m = 1, 2, 4, 8, 16, 32; lane 0's value is the sum (every lane ends with the same bits:
//      IEEE addition commutes).
// Steps m = 1, 2 are quad permutes; m = 4 and m = 8 read the mirrored lane of the half row / the row, which after the steps
// before holds the bits of lane ^ m; m = 16 and 32 add the four rows' values as (r0 + r1) + (r2 + r3) -- what both steps give
// in every lane.  tests/inverse_ref.c restates the order sequentially.
#pragma once
#include <type_traits>
#include "pagk_chain_asm.h"
#include "pagk_device.h"

namespace pagk {

__device__ __forceinline__ void write_outputs(const TrackArgs &a, int i, float p2x, float p2y, int succ,
                                              float lastCost, int level0_ran, float ncc, int iters);
__device__ __forceinline__ uint32_t lds_off(const void *p);
__host__ __device__ inline int track_block_pp(int half);

// LDS: the NCC epilogue's five f32 arrays of PP and its five partial results; nothing without NCC.
__host__ __device__ inline size_t inv_wave_lds_bytes(int half, bool calc_ncc)
{
    return calc_ncc ? ((size_t)5 * track_block_pp(half) + 32 + 8) * 4 : 0;  // (a chain may read one block past its array)
}

template <int CTRL>
__device__ __forceinline__ float inv_dpp_f32(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ double inv_dpp_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float inv_row_value(float v, int row)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16 * row));
}
__device__ __forceinline__ double inv_row_value(double v, int row) { return lane_bcast(v, 16 * row); }

// The wave's sum of the lanes' partial sums, in the order of the header (all 64 lanes active).
template <class T>
__device__ __forceinline__ T inv_wave_sum(T v)
{
    if constexpr (std::is_same<T, float>::value) {
        v = v + inv_dpp_f32<0xB1>(v);   // quad_perm:[1,0,3,2]   lane ^ 1
        v = v + inv_dpp_f32<0x4E>(v);   // quad_perm:[2,3,0,1]   lane ^ 2
        v = v + inv_dpp_f32<0x141>(v);  // row_half_mirror       the other quad of the half row: lane ^ 4's bits
        v = v + inv_dpp_f32<0x140>(v);  // row_mirror            the other half row: lane ^ 8's bits
    } else {
        v = v + inv_dpp_f64<0xB1>(v);
        v = v + inv_dpp_f64<0x4E>(v);
        v = v + inv_dpp_f64<0x141>(v);
        v = v + inv_dpp_f64<0x140>(v);
    }
    const T r0 = inv_row_value(v, 0), r1 = inv_row_value(v, 1), r2 = inv_row_value(v, 2), r3 = inv_row_value(v, 3);
    return (r0 + r1) + (r2 + r3);      // lane ^ 16, then lane ^ 32
}

// Waves per SIMD the register allocation targets: the most at which the compiler spills nothing.  A wave keeps six registers
// per pixel it owns (T, Ix, Iy, wx, wy, the packed x and y); the generic build adds the penalty's and the solver switches' f64
// temporaries.  The common sizes (h <= 10) get three or four waves per SIMD, the rest two.
constexpr int inv_wave_occ(int nr, bool lean) { return lean ? (nr <= 6 ? 4 : (nr <= 7 ? 3 : 2)) : (nr <= 2 ? 4 : (nr <= 7 ? 3 : 2)); }

// NR: chunks of 64 pixels; TAIL: P mod 32 (the NCC epilogue's ordered chains); LEAN: no penalty, solver_variant 0.
template <int NR, int TAIL, bool LEAN = false>
__global__ void __launch_bounds__(64, inv_wave_occ(NR, LEAN)) k_inv_wave(TrackArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int i = blockIdx.x;
    const int lane = threadIdx.x;
    const int h = a.half, Wd = 2 * h + 1, P = Wd * Wd, PP = track_block_pp(h);
    const int nfull = P / 32;

    const float *init = a.has_gyro ? a.pt_init : a.pt_ref;  // :85-89
    float p2x = init[2 * i], p2y = init[2 * i + 1];
    if (!a.status_in[i]) {  // :173
        if (lane == 0) write_outputs(a, i, p2x, p2y, 0, 0.0f, 0, 0.0f, 0);
        return;
    }
    float A00 = 1, A01 = 0, A10 = 0, A11 = 1;
    if (a.use_affine) {
        A00 = a.affine[4 * i], A01 = a.affine[4 * i + 1], A10 = a.affine[4 * i + 2], A11 = a.affine[4 * i + 3];
    }
    const float refx = a.pt_ref[2 * i], refy = a.pt_ref[2 * i + 1];

    // lane -> pixels p = lane + 64 r, row-major (y outer, :233-234); slots past the patch shadow the last pixel and add nothing
    float wx[NR], wy[NR];
    int pxy[NR];  // x and y packed (two int16)
#pragma unroll
    for (int r = 0; r < NR; r++) {
        int p = lane + 64 * r;
        p = p < P ? p : P - 1;
        const int yy = p / Wd, xx = p - yy * Wd;
        const int x = xx - h, y = yy - h;
        pxy[r] = (x & 0xffff) | (y << 16);
        // :203-204; without the warp A is the identity, and 1 * x + 0 * y is x (and 0 * x + 1 * y is y) bit for bit for these integers
        wx[r] = A00 * (float)x + A01 * (float)y;
        wy[r] = A10 * (float)x + A11 * (float)y;
        asm volatile("" : "+v"(wx[r]), "+v"(wy[r]), "+v"(pxy[r]));
    }
    const float fh = (float)h;
    const float ext_x = fabsf(A00) * fh + fabsf(A01) * fh + 2.0f;
    const float ext_y = fabsf(A10) * fh + fabsf(A11) * fh + 2.0f;

    int succ = 1, iters = 0;
    float lastCost = 0.0f;

    for (int level = a.n_levels - 1; level >= 0; level--) {
        const DevLevel &L1 = a.l1[level];
        const DevLevel L2 = pin_level(a.l2[level]);
        const float ptx = refx * a.scales[level], pty = refy * a.scales[level];  // :177
        float nx, ny;
        if (level == a.n_levels - 1) {  // :180
            nx = p2x * a.scales[level];
            ny = p2y * a.scales[level];
        } else {  // :182
            nx = (float)((double)(p2x * 1.0f) / 0.5);
            ny = (float)((double)(p2y * 1.0f) / 0.5);
        }
        float dx = nx - ptx, dy = ny - pty, dg = 0.0f, db = 0.0f;  // :186-191
        lastCost = 0.0f;
        succ = 1;

        // ---- set-up: template, its derivatives, Hp -- once per level -------------------------------------
        const float c = sample<true>(L1, ptx, pty);  // :263 (the patch centre)
        const double jc = (double)(-c);
        float T[NR], Ix[NR], Iy[NR];
        double hp[10];  // lower triangle, row by row: 00 | 10 11 | 20 21 22 | 30 31 32 33
#pragma unroll
        for (int q = 0; q < 10; q++) hp[q] = 0.0;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const float X = ptx + (float)(short)(pxy[r] & 0xffff), Y = pty + (float)(pxy[r] >> 16);
            const OneTap t0 = sample_issue<true>(L1, X, Y);
            const OneTap t1 = sample_issue<true>(L1, X + 1.0f, Y), t2 = sample_issue<true>(L1, X - 1.0f, Y);
            const OneTap t3 = sample_issue<true>(L1, X, Y + 1.0f), t4 = sample_issue<true>(L1, X, Y - 1.0f);
            T[r] = sample_finish(t0);                                     // :253
            Ix[r] = 0.5f * (sample_finish(t1) - sample_finish(t2));      // :269-270
            Iy[r] = 0.5f * (sample_finish(t3) - sample_finish(t4));      // :271-272
            asm volatile("" : "+v"(T[r]), "+v"(Ix[r]), "+v"(Iy[r]));     // three registers a pixel from here on, not its taps
            if (r < NR - 1 || lane + 64 * r < P) {  // (NR = ceil(P / 64): only the last chunk is partial)
                const double jx = (double)Ix[r], jy = (double)Iy[r];     // :273-274; every product below is exact
                hp[0] += jx * jx;
                hp[1] += jy * jx;
                hp[2] += jy * jy;
                hp[3] += jc * jx;
                hp[4] += jc * jy;
                hp[5] += jc * jc;
                hp[6] += jx;
                hp[7] += jy;
                hp[8] += jc;
                hp[9] += 1.0;
            }
            __builtin_amdgcn_sched_barrier(0);  // one pixel's five gathers in flight, not the whole set-up's: registers
        }
#pragma unroll
        for (int q = 0; q < 10; q++) hp[q] = inv_wave_sum(hp[q]);

        for (int iter = 0; iter < a.iterations; iter++) {  // :215
            iters++;
            // ---- 1. one img2 sample per pixel, the residual, the lane's partial sums --------------------------
            const float bx = ptx + dx, by = pty + dy;
            const float gain = 1.0f + dg;
            const bool interior = (bx - ext_x >= 0.0f) && (bx + ext_x < L2.fcols_m1) &&
                                  (by - ext_y >= 0.0f) && (by + ext_y < L2.frows_m1);
            double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
            float cs = 0.0f;
            auto sampling = [&](auto clamp_tag) {
                constexpr bool CLAMP = decltype(clamp_tag)::value;
                constexpr int kU = NR < 8 ? NR : 8;  // gathers in flight
#pragma unroll
                for (int r0 = 0; r0 < NR; r0 += kU) {
                    OneTap taps[kU];
#pragma unroll
                    for (int u = 0; u < kU; u++) {
                        const int r = r0 + u;
                        if (r < NR) taps[u] = sample_issue<CLAMP>(L2, bx + wx[r], by + wy[r]);
                    }
#pragma unroll
                    for (int u = 0; u < kU; u++) {
                        const int r = r0 + u;
                        if (r < NR) {
                            const float e = sample_finish(taps[u]) + db - gain * T[r];  // :252-253
                            if (r < NR - 1 || lane + 64 * r < P) {  // (NR = ceil(P / 64): only the last chunk is partial)
                                const double ed = (double)e;
                                // (widened here, every iteration: hoisted out of the loop the f64 copies cost four registers a pixel)
                                float ix = Ix[r], iy = Iy[r];
                                asm volatile("" : "+v"(ix), "+v"(iy));
                                b0 += (double)(-ix) * ed;  // :293  b += -J * e
                                b1 += (double)(-iy) * ed;
                                b2 += (double)c * ed;
                                b3 += -ed;
                                cs += e * e;                  // :294  float
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);  // kU gathers in flight
                }
            };
            if (interior)
                sampling(std::false_type{});
            else
                sampling(std::true_type{});
            // ---- 2. the five sums ----------------------------------------------------------------------------
            double H[4][4], b[4], upd[4];
            b[0] = inv_wave_sum(b0);
            b[1] = inv_wave_sum(b1);
            b[2] = inv_wave_sum(b2);
            b[3] = inv_wave_sum(b3);
            float cost = inv_wave_sum(cs);
            __builtin_amdgcn_sched_barrier(0);
            // ---- 3. H = Hp, penalty, solve (:302-319): every lane, on the same bits ---------------------------
            H[0][0] = hp[0];
            H[1][0] = hp[1], H[1][1] = hp[2];
            H[2][0] = hp[3], H[2][1] = hp[4], H[2][2] = hp[5];
            H[3][0] = hp[6], H[3][1] = hp[7], H[3][2] = hp[8], H[3][3] = hp[9];
            if constexpr (!LEAN) {
                if (a.penalty) add_penalty(a, dx, dy, H, b, cost);
            }
            // lanes 0..3 share the divides of each Cholesky column (pagk_device.h); every lane ends with the result
            const double unorm = llt4_solve_nsq_lanes(H, b, lane, upd, LEAN ? 0u : a.solver);  // update.squaredNorm()
            // ---- 4. update + termination (:322-344) ----------------------------------------------------------
            if (upd[0] != upd[0]) {  // :322
                succ = 0;
                break;
            }
            if (iter > 0 && cost > lastCost) break;  // :328
            dx = (float)((double)dx + upd[0]);       // :332
            dy = (float)((double)dy + upd[1]);
            if (a.illum) {  // :334-337
                dg = (float)((double)dg + upd[2]);
                db = (float)((double)db + upd[3]);
            }
            lastCost = cost;
            succ = 1;
            if (unorm < kNormSqConverged) break;  // :343  update.norm() < 1e-2
        }
        p2x = ptx + dx;  // :348
        p2y = pty + dy;
    }

    float ncc = 1.0f;  // :365
    if (a.calc_ncc) {
        // PatchMatch::NCC (:433-469) as k_track_wave has it: x outer / y inner order, ordered f32 sums through LDS
        float *vref = reinterpret_cast<float *>(lds_raw), *vcur = vref + PP, *tnum = vcur + PP, *td1 = tnum + PP, *td2 = td1 + PP;
        float *sh_f = td2 + PP + 32;
        const DevLevel &R0 = a.l1[0], &C0 = a.l2[0];
        float vr[NR], vc[NR];
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));  // the epilogue's coordinates are computed here, not carried through the loops in registers
#pragma unroll
        for (int r = 0; r < NR; r++) {
            int k = lane_e + 64 * r;
            k = k < P ? k : P - 1;
            int xi = k / Wd - h, yi = k - (k / Wd) * Wd - h;
            vr[r] = sample<true>(R0, refx + xi, refy + yi);
            if (a.use_affine) {
                float wxx = A00 * xi + A01 * yi, wyy = A10 * xi + A11 * yi;
                vc[r] = sample<true>(C0, p2x + wxx, p2y + wyy);
            } else {
                vc[r] = sample<true>(C0, p2x + xi, p2y + yi);
            }
            asm volatile("" : "+v"(vr[r]), "+v"(vc[r]));
            if (lane + 64 * r < P) {
                vref[lane + 64 * r] = vr[r];
                vcur[lane + 64 * r] = vc[r];
            }
        }
        __syncthreads();
        const int row = lane >> 4, lr = lane & 15;
        {
            float m = chain_rows_f32<TAIL>(lds_off(row == 1 ? vcur : vref) + 8u * lr, 128u, nfull);
            if (lr == 0 && row < 2) sh_f[row] = m;
        }
        __syncthreads();
        const float mean_ref = sh_f[0] / (float)P, mean_cur = sh_f[1] / (float)P;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            int k = lane + 64 * r;
            if (k < P) {
                float dr = vr[r] - mean_ref, dc = vc[r] - mean_cur;
                tnum[k] = dr * dc;
                td1[k] = dr * dr;
                td2[k] = dc * dc;
            }
        }
        __syncthreads();
        {
            const float *src = row == 0 ? tnum : (row == 1 ? td1 : td2);
            float v = chain_rows_f32<TAIL>(lds_off(src) + 8u * lr, 128u, nfull);
            if (lr == 0 && row < 3) sh_f[2 + row] = v;
        }
        __syncthreads();
        ncc = (float)((double)sh_f[2] / sqrt((double)(sh_f[3] * sh_f[4]) + 1e-10));
    }
    if (lane == 0) write_outputs(a, i, p2x, p2y, succ, lastCost, 1, ncc, iters);
}

}  // namespace pagk
