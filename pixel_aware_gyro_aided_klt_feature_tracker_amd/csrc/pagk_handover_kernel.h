// pagk_handover_kernel.h -- what lies between two frame pairs of a tracker's loop, on the device (include/pagk.h:
// pagk_post_filter_device, pagk_frame_handover_device):
//   k_post_filter      GyroAidedTracker::GyroPredictFeaturesAndOpticalFlowRefined Step 3 (reference
//                      src/gyro_aided_tracker.cpp:289-341), bit-identical to the host function pagk_post_filter
//   k_handover_fill    Frame::mMask = ones (src/frame.cpp:89)
//   k_handover_holes   the 14 x 14 block of zeros around every surviving track (src/frame.cpp:147-151)
//   k_handover_keys    GyroAidedTracker::SetBackToFrame (:97-111) + Frame::SetPredictKeyPointsAndMask (src/frame.cpp:
//                      115-153, the key arrays) + the top-up rule of Frame::DetectKeyPoints / LoadDetectedKeypointFromFile
//                      (:156-218, :244-281) on a candidate list
// Plain HIP C++, vector stores only.  No lane returns or branches around a barrier: the loops that hold one are bounded
// by kernel arguments and by counts every lane reads from the same address.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pagk {

constexpr int kHandoverStateWords = 8;   // PAGK_HANDOVER_STATE_WORDS
constexpr int kHandoverHalf = 7;         // half_path_size of Frame::SetPredictKeyPointsAndMask (src/frame.cpp:117)

// One workgroup of 1024.  Phase 1, in rounds of 2048 entries: every thread loads two entries of the NEXT round (coalesced;
// a status-false entry, and the padding behind n, becomes +0.0) and counts its status-true ones, wave 0 meanwhile adds
// the entries of THIS round from LDS in index order, one rounding per add, then the loaded values go into the other LDS
// buffer and a barrier ends the round.  So the global loads of a round hide behind the chain of the round before, and the
// chain touches LDS only: it reads the entries back as broadcasts (every lane the same address, 16 bytes = two entries per
// read, the next 16 entries on their way while 16 are added), its operand is a plain vector register and its critical
// path one dependent v_add_f64 per entry; every lane of wave 0 computes the same sum.  +0.0 is an identity of this
// running sum: it starts at +0.0 and can therefore never be -0.0; NaN stays NaN.
// Phase 2, behind the last barrier (status_out may alias status_pm: every read of phase 1 is over): the mask, the
// survivors' points, the count.
constexpr int kPfRound = 2048;

// s + b[0] + b[1] + ... + b[255], in order
__device__ __forceinline__ double pf_chain256(double s, const double2 *b)
{
    // 16 blocks of 16 entries, two register sets in turn: the block behind is read while this one is added.  The
    // scheduling barriers keep the compiler from moving the reads down to their uses (it would wait for each)
    double2 A[8], B[8];
#pragma unroll
    for (int j = 0; j < 8; j++) A[j] = b[j];
    for (int k = 0; k < 128; k += 16) {
#pragma unroll
        for (int j = 0; j < 8; j++) B[j] = b[k + 8 + j];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            s = s + A[j].x;
            s = s + A[j].y;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 8; j++) A[j] = b[(k + 16 + j) & 127];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            s = s + B[j].x;
            s = s + B[j].y;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    return s;
}

// (the body of k_post_filter, and of one camera's workgroup of its batched form in pagk_group_kernel.h)
__device__ __forceinline__ void post_filter_body(int32_t n, int32_t half_patch, const uint8_t *status_pm,
                                                 const double *pix_err, const double *dist_pred, const float *pt_pm,
                                                 const float *pt_pm_un, uint8_t *status_out, float *pt_predict,
                                                 float *pt_predict_un, int32_t *kept_out, double *thresholds)
{
    __shared__ double s_sum;
    __shared__ __align__(16) double s_stage[2][kPfRound];
    __shared__ int32_t s_cnt[16], s_kept[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t cnt = 0;
    double s = 0.0;
    // round r's entries r * 2048 + tid and r * 2048 + 1024 + tid are this thread's
    auto load = [&](int i, int32_t &c) -> double {
        if (i >= n) return 0.0;
        const double v = pix_err[i];
        const bool on = status_pm[i] != 0;
        c += on ? 1 : 0;
        return on ? v : 0.0;
    };
    double v0 = load(tid, cnt), v1 = load(1024 + tid, cnt);
    s_stage[0][tid] = v0, s_stage[0][1024 + tid] = v1;
    __syncthreads();
    for (int r0 = 0, g = 0; r0 < n; r0 += kPfRound, g ^= 1) {   // (n is a kernel argument: every wave runs the same rounds)
        v0 = load(r0 + kPfRound + tid, cnt), v1 = load(r0 + kPfRound + 1024 + tid, cnt);
        if (wave == 0) {
            const int left = n - r0;   // groups of 256 that hold entries of this round
            const int groups = left >= kPfRound ? kPfRound / 256 : (left + 255) / 256;
            for (int q = 0; q < groups; q++) s = pf_chain256(s, reinterpret_cast<const double2 *>(&s_stage[g][q * 256]));
        }
        s_stage[g ^ 1][tid] = v0, s_stage[g ^ 1][1024 + tid] = v1;
        __syncthreads();
    }
    if (tid == 0) s_sum = s;
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    int32_t total = 0;
    for (int w = 0; w < 16; w++) total += s_cnt[w];
    const double avg = s_sum / (double)total;                                                // :305
    const double th_pix = 4.0 * avg > (double)half_patch ? 4.0 * avg : (double)half_patch;  // :308
    const double th_dist = (double)half_patch * 4.0;                                         // :312
    int32_t kept = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {   // :318
        const int i = c0 + tid;
        if (i < n) {
            const bool ok = status_pm[i] && pix_err[i] < th_pix && dist_pred[i] < th_dist;
            status_out[i] = ok ? 1 : 0;
            if (ok) {
                if (pt_predict && pt_pm) pt_predict[2 * i] = pt_pm[2 * i], pt_predict[2 * i + 1] = pt_pm[2 * i + 1];
                if (pt_predict_un && pt_pm_un)
                    pt_predict_un[2 * i] = pt_pm_un[2 * i], pt_predict_un[2 * i + 1] = pt_pm_un[2 * i + 1];
                kept++;
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) kept += __shfl_down(kept, off, 64);
    if (lane == 0) s_kept[wave] = kept;
    __syncthreads();
    if (tid == 0) {
        int32_t k = 0;
        for (int w = 0; w < 16; w++) k += s_kept[w];
        *kept_out = k;
        if (thresholds) thresholds[0] = th_pix, thresholds[1] = th_dist;
    }
}

__global__ void __launch_bounds__(1024) k_post_filter(int32_t n, int32_t half_patch, const uint8_t *status_pm,
                                                      const double *pix_err, const double *dist_pred, const float *pt_pm,
                                                      const float *pt_pm_un, uint8_t *status_out, float *pt_predict,
                                                      float *pt_predict_un, int32_t *kept_out, double *thresholds)
{
    post_filter_body(n, half_patch, status_pm, pix_err, dist_pred, pt_pm, pt_pm_un, status_out, pt_predict, pt_predict_un,
                     kept_out, thresholds);
}

// ---- frame hand-over -----------------------------------------------------------------------------------------------
struct HandoverArgs {
    int32_t cap, cand_cap, width, height, target_n;
    double new_point_threshold;   // mThresholdOfPredictNewKeyPoint (src/frame.cpp:79)
    float fx, fy, cx, cy, fx_inv, fy_inv, k1, k2, p1, p2, k3;
    int32_t distort_on;
    const uint8_t *status;
    const float *pt_predict, *pt_predict_un;
    const int32_t *n_cand;
    const float *cand_un;
    float *keys, *keys_un, *keys_normal;
    int32_t *index_in_last;
    uint8_t *live, *mask;
    int32_t *state;
    // the tracking launches' per-slot hints (pagk_prio.h), compacted IN PLACE with the survivors; nullptr / 0: none
    int32_t *prio_hint;
    int32_t prio_hint_n;
};

// mMask = ones: 16 bytes per store; `bytes` is a multiple of 16 (the buffer is padded), the tail is stored bytewise
// when the caller's own mask is not
__device__ __forceinline__ void handover_fill_body(uint8_t *mask, int64_t bytes)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, o = t * 16;
    if (o + 16 <= bytes) {
        if ((reinterpret_cast<uintptr_t>(mask) & 15) == 0) {
            *reinterpret_cast<uint4 *>(mask + o) = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
        } else {
            for (int k = 0; k < 16; k++) mask[o + k] = 1;
        }
    } else {
        for (int64_t k = o; k < bytes; k++) mask[k] = 1;
    }
}

__global__ void __launch_bounds__(256) k_handover_fill(uint8_t *mask, int64_t bytes) { handover_fill_body(mask, bytes); }

// int(x) - 7 clamped so that the 14-wide block lies in the image (src/frame.cpp:148-149)
__device__ __forceinline__ int handover_hole_origin(float x, int extent)
{
    const int a = (int)x - kHandoverHalf;
    const int b = a > 0 ? a : 0;
    const int hi = extent - 2 * kHandoverHalf;
    return b < hi ? b : hi;
}

// one thread per (feature, row of its hole): 14 zero bytes.  Holes overlap; every writer stores 0.
__device__ __forceinline__ void handover_holes_body(int32_t cap, int32_t width, int32_t height, const uint8_t *status,
                                                    const float *pt_predict_un, uint8_t *mask)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t / (2 * kHandoverHalf), r = t - i * (2 * kHandoverHalf);
    if (i >= cap || !status[i]) return;
    const int x0 = handover_hole_origin(pt_predict_un[2 * i], width);
    const int y0 = handover_hole_origin(pt_predict_un[2 * i + 1], height);
    uint8_t *row = mask + (int64_t)(y0 + r) * width + x0;
    for (int k = 0; k < 2 * kHandoverHalf; k++) row[k] = 0;
}

__global__ void __launch_bounds__(256) k_handover_holes(int32_t cap, int32_t width, int32_t height, const uint8_t *status,
                                                        const float *pt_predict_un, uint8_t *mask)
{
    handover_holes_body(cap, width, height, status, pt_predict_un, mask);
}

// exclusive rank of this lane's `take` among the workgroup's 1024 in thread order, and the workgroup's total
__device__ __forceinline__ int32_t handover_scan(bool take, int32_t *wtot, int lane, int wave, int32_t &tot)
{
    const unsigned long long bal = __ballot(take);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int32_t off = 0;
    tot = 0;
    for (int w = 0; w < 16; w++) {
        off += w < wave ? wtot[w] : 0;
        tot += wtot[w];
    }
    __syncthreads();
    return off + __popcll(bal & ((1ull << lane) - 1ull));
}

// the acceptance test of one candidate (src/frame.cpp:253); outside the image: rejected
__device__ __forceinline__ bool handover_accepts(const HandoverArgs &a, float x, float y)
{
    // int() truncates toward zero: exactly the x in (-1, width) land on a column of the image
    if (!(x > -1.0f && x < (float)a.width && y > -1.0f && y < (float)a.height)) return false;
    return a.mask[(int64_t)(int)y * a.width + (int)x] != 0;
}

// One workgroup of 1024, behind k_handover_fill and k_handover_holes on the stream: two stable compactions (ballot
// scans over coalesced groups of 1024 entries), the survivors' and the accepted candidates'.
__device__ __forceinline__ void handover_keys_body(const HandoverArgs &a)
{
    __shared__ int32_t wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // survivors (src/frame.cpp:120-135)
    int32_t m = 0;
    for (int c0 = 0; c0 < a.cap; c0 += 1024) {
        const int i = c0 + tid;
        const bool take = i < a.cap && a.status[i] != 0;
        // (in place: a group's hints are read in front of the scan's barriers and stored behind them, to slots o <= i that no
        // later group reads)
        const int32_t hint = (take && i < a.prio_hint_n) ? a.prio_hint[i] : 0;
        int32_t tot;
        const int32_t o = m + handover_scan(take, wtot, lane, wave, tot);
        if (take) {
            const float xu = a.pt_predict_un[2 * i], yu = a.pt_predict_un[2 * i + 1];
            a.keys[2 * o] = a.pt_predict[2 * i], a.keys[2 * o + 1] = a.pt_predict[2 * i + 1];
            a.keys_un[2 * o] = xu, a.keys_un[2 * o + 1] = yu;
            if (a.keys_normal) a.keys_normal[2 * o] = (xu - a.cx) * a.fx_inv, a.keys_normal[2 * o + 1] = (yu - a.cy) * a.fy_inv;  // :128-129
            a.index_in_last[o] = i;
            if (o < a.prio_hint_n) a.prio_hint[o] = hint;
        }
        m += tot;
    }
    // the top-up (:164-215, :248-266).  reach_flag is read by every lane in front of the barrier below, lane 0 rewrites
    // it behind it.
    const int32_t reach = a.state[1];
    int32_t n_cand = *a.n_cand;
    n_cand = n_cand < 0 ? 0 : (n_cand > a.cand_cap ? a.cand_cap : n_cand);
    __syncthreads();
    const int32_t n_new = a.target_n - m;                                                    // :168
    const bool topup = ((double)m < a.new_point_threshold || !reach) && n_new > 0;           // :164, :169
    int32_t seen = 0;   // acceptable candidates in front of the running group
    for (int c0 = 0; c0 < n_cand; c0 += 1024) {   // (n_cand: the same value in every lane)
        const int j = c0 + tid;
        float x = 0.0f, y = 0.0f;
        if (j < n_cand) x = a.cand_un[2 * j], y = a.cand_un[2 * j + 1];
        const bool ok = j < n_cand && handover_accepts(a, x, y);
        int32_t tot;
        const int32_t r = seen + handover_scan(ok, wtot, lane, wave, tot);
        if (topup && ok && r < n_new) {   // :263-265
            const int32_t q = m + r;
            a.keys_un[2 * q] = x, a.keys_un[2 * q + 1] = y;
            const float xn = (x - a.cx) * a.fx_inv, yn = (y - a.cy) * a.fy_inv;               // :259-260
            if (a.keys_normal) a.keys_normal[2 * q] = xn, a.keys_normal[2 * q + 1] = yn;
            float ox = x, oy = y;
            if (a.distort_on) {   // DistortVecPoints, src/utils.cpp:63-72
                const float r2 = xn * xn + yn * yn;
                const float r4 = r2 * r2;
                const float r6 = r4 * r2;
                const float xd = xn * (1 + a.k1 * r2 + a.k2 * r4 + a.k3 * r6) + 2 * a.p1 * xn * yn + a.p2 * (r2 + 2 * xn * xn);
                const float yd = yn * (1 + a.k1 * r2 + a.k2 * r4 + a.k3 * r6) + a.p1 * (r2 + 2 * yn * yn) + 2 * a.p2 * xn * yn;
                ox = a.fx * xd + a.cx;
                oy = a.fy * yd + a.cy;
            }
            a.keys[2 * q] = ox, a.keys[2 * q + 1] = oy;
            a.index_in_last[q] = -1;                                                         // :258
        }
        seen += tot;
    }
    const int32_t added = topup ? (seen < n_new ? seen : n_new) : 0;
    const int32_t total = m + added;
    for (int i = tid; i < a.cap; i += 1024) {
        if (i >= m && i < a.prio_hint_n) a.prio_hint[i] = 0;   // topped-up and unused slots: no forecast
        a.live[i] = i < total ? 1 : 0;
        if (i >= total) {
            a.keys[2 * i] = a.keys[2 * i + 1] = 0.0f;
            a.keys_un[2 * i] = a.keys_un[2 * i + 1] = 0.0f;
            if (a.keys_normal) a.keys_normal[2 * i] = a.keys_normal[2 * i + 1] = 0.0f;
            a.index_in_last[i] = -1;
        }
    }
    if (tid == 0) {
        a.state[0] = total;
        a.state[1] = topup ? (total == a.target_n ? 1 : 0) : reach;                          // :214
        a.state[2] = m;
        a.state[3] = added;
        a.state[4] = n_cand - seen;
        a.state[5] = a.state[6] = a.state[7] = 0;
    }
}

__global__ void __launch_bounds__(1024) k_handover_keys(HandoverArgs a) { handover_keys_body(a); }

}  // namespace pagk
