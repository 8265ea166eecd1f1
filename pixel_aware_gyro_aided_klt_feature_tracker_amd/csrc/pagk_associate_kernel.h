// pagk_associate_kernel.h -- track-to-detection association: what ties a tracked point to a keypoint that was detected
// independently in the current frame (include/pagk.h, "Track-to-detection association"; tests/associate_ref.c restates
// it sequentially):
//   k_match_choose   GyroAidedTracker::MatchFeatures, the choice rule (reference src/gyro_aided_tracker.cpp:955-990): one
//                    thread per feature, an integer atomicAdd per claim
//   k_match_compact  ... its uniqueness rule (:993-1007) and the flow error of SearchByGyroPredict (:928-933).  A current
//                    keypoint enters sFoundInCurPts at its first claim, every later claim erases all matches to it and it
//                    is never admitted again: feature i keeps its choice t iff exactly one feature chose t, in increasing
//                    i.  A count and a stable compaction.
//   k_radius_top2    cv::BFMatcher::radiusMatch of SearchByOpencvKLT (:1059-1087) for 2-D points, and its ratio test: one
//                    thread per query, the current keypoints staged through LDS, an atomicMin per claim
//   k_klt_finish     ... its first-come uniqueness (:1089-1105: the lowest claiming index wins) and the mean-disparity
//                    filter (:1108-1130): two stable compactions around an ordered f64 sum
// Sums of integer atomics and minima do not depend on the order in which workgroups run; everything else is a function of
// one feature or runs in one workgroup.  Plain HIP C++, vector stores only.  No lane returns or branches around a barrier.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pagk_handover_kernel.h"

namespace pagk {

constexpr int kAssocInfoWords = 8;    // PAGK_ASSOC_INFO_WORDS
constexpr int kAssocStatsWords = 8;   // PAGK_ASSOC_STATS_WORDS
// what k_match_choose / k_radius_top2 leave in choice[i] when feature i chose nothing
constexpr int32_t kNoChoice = -1;     // no neighbour, or the rule rejected
constexpr int32_t kOverlong = -2;     // count[i] > cap (match) / the ratio test rejected (KLT)
constexpr int32_t kBadIndex = -3;     // train index outside [0, m) (match) / the query is not live (KLT)
constexpr int kRadiusTile = 1024;     // current keypoints per LDS tile of k_radius_top2: 8 KB

struct MatchArgs {
    int32_t n, m, cap, use_ncc;
    float th_high, th_low, th_ratio;
    const int32_t *count, *nbr_idx;   // n, n x cap
    const float *nbr_dist, *nbr_ncc;  // n x cap
    int32_t *choice;                  // n (workspace)
    int32_t *claims;                  // m (workspace), zero before k_match_choose
    const float *keys_cur_un, *pt_pred;   // the flow error's operands, or nullptr with flows
    int32_t *match_query, *match_train;   // n
    float *match_dist, *match_ncc;        // n, or nullptr
    int32_t *n_matches;
    float *flows;                         // n x 2, or nullptr
    int32_t *info;                        // kAssocInfoWords
    const int32_t *gate;                  // info[5] = *gate < gate_below (read before n_matches is written), or nullptr: 0
    int32_t gate_below;
};

__global__ void __launch_bounds__(256) k_match_choose(MatchArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int32_t c = a.count[i];
    int32_t pick = kNoChoice;
    if (c > a.cap) {
        pick = kOverlong;
    } else if (c > 0) {   // :955
        const size_t b = (size_t)i * a.cap;
        bool take = true;
        if (a.use_ncc) {  // :959-975
            const float n0 = a.nbr_ncc[b];
            if (!(n0 > a.th_high)) {
                if (c > 1) {
                    if (n0 < a.th_low) take = false;
                    else if (!(a.nbr_ncc[b + 1] < n0 * a.th_ratio)) take = false;   // the two best are too similar
                } else
                    take = false;
            }
        } else if (c > 1 && !(a.nbr_dist[b] < a.nbr_dist[b + 1] * a.th_ratio)) {  // :977-989
            take = false;
        }
        if (take) {
            const int32_t t = a.nbr_idx[b];
            pick = (t >= 0 && t < a.m) ? t : kBadIndex;
        }
    }
    a.choice[i] = pick;
    if (pick >= 0) atomicAdd(&a.claims[pick], 1);
}

// adds v of every thread into *slot (LDS, zero before the first add): a wave's sum by shuffles, then one integer atomic per
// wave.  The sum is read behind a barrier.
__device__ __forceinline__ void assoc_add(int32_t v, int32_t *slot, int lane)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) atomicAdd(slot, v);
}

// One workgroup of 1024, behind k_match_choose on the stream.
__global__ void __launch_bounds__(1024) k_match_compact(MatchArgs a)
{
    __shared__ int32_t wtot[16], acc[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t ran2 = a.gate ? (*a.gate < a.gate_below ? 1 : 0) : 0;
    if (tid < 4) acc[tid] = 0;
    __syncthreads();
    int32_t chosen = 0, overlong = 0, bad = 0, k = 0;
    for (int c0 = 0; c0 < a.n; c0 += 1024) {   // (n is a kernel argument: every wave runs the same groups)
        const int i = c0 + tid;
        const int32_t t = i < a.n ? a.choice[i] : kNoChoice;
        chosen += t >= 0, overlong += t == kOverlong, bad += t == kBadIndex;
        const bool keep = t >= 0 && a.claims[t] == 1;
        int32_t tot;
        const int32_t o = k + handover_scan(keep, wtot, lane, wave, tot);
        if (keep) {
            const size_t b = (size_t)i * a.cap;
            a.match_query[o] = i, a.match_train[o] = t;
            if (a.match_dist) a.match_dist[o] = a.nbr_dist[b];
            if (a.match_ncc) a.match_ncc[o] = a.nbr_ncc[b];
        }
        if (a.flows && i < a.n) {   // :928-933
            float fx = 0.0f, fy = 0.0f;
            if (keep) fx = a.keys_cur_un[2 * t] - a.pt_pred[2 * i], fy = a.keys_cur_un[2 * t + 1] - a.pt_pred[2 * i + 1];
            a.flows[2 * i] = fx, a.flows[2 * i + 1] = fy;
        }
        k += tot;
    }
    for (int o = k + tid; o < a.n; o += 1024) {   // rows at or beyond the count
        a.match_query[o] = -1, a.match_train[o] = -1;
        if (a.match_dist) a.match_dist[o] = 0.0f;
        if (a.match_ncc) a.match_ncc[o] = 0.0f;
    }
    int32_t multi = 0;
    for (int j = tid; j < a.m; j += 1024) multi += a.claims[j] > 1;
    assoc_add(chosen, &acc[0], lane), assoc_add(overlong, &acc[1], lane), assoc_add(bad, &acc[2], lane);
    assoc_add(multi, &acc[3], lane);
    __syncthreads();
    if (tid == 0) {
        *a.n_matches = k;
        a.info[0] = acc[0], a.info[1] = acc[1], a.info[2] = acc[2], a.info[3] = acc[3], a.info[4] = k, a.info[5] = ran2;
        a.info[6] = a.info[7] = 0;
    }
}

struct KltArgs {
    int32_t cap, m;
    const int32_t *d_n, *d_m;      // device counts, or nullptr: cap, m
    const uint8_t *status;         // cap: after the err filter
    const float *pt_lk;            // cap x 2: the tracked points (the queries)
    const float *pt_ref;           // cap x 2: the reference keypoints
    const float *keys_cur;         // m x 2: the detected keypoints
    float max_distance;
    double ratio, factor;
    int32_t *choice, *nnb;         // cap (workspace): the choice, the true number of neighbours
    float *dist0;                  // cap (workspace): distance of the best neighbour
    int32_t *owner;                // m (workspace), INT_MAX before k_radius_top2
    int32_t *match_query, *match_train;   // cap
    float *match_dist;                    // cap, or nullptr
    double *disparity;                    // cap
    int32_t *n_matches;
    double *stats;                        // kAssocStatsWords
    int32_t *info;                        // kAssocInfoWords
};

__device__ __forceinline__ int32_t assoc_live(const int32_t *d, int32_t cap)
{
    if (!d) return cap;
    const int32_t v = *d;
    return v < 0 ? 0 : (v > cap ? cap : v);
}

__global__ void __launch_bounds__(256) k_radius_top2(KltArgs a)
{
    __shared__ float2 tile[kRadiusTile];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const int32_t n_live = assoc_live(a.d_n, a.cap), m_live = assoc_live(a.d_m, a.m);
    const bool row = i < a.cap, live = row && i < n_live && a.status[i] != 0;
    float qx = 0.0f, qy = 0.0f;
    if (live) qx = a.pt_lk[2 * i], qy = a.pt_lk[2 * i + 1];
    int32_t cnt = 0, j0 = -1;
    float d0 = 0.0f, d1 = 0.0f;
    // sqrtf is monotone: a sum of squares beyond this bound has a root beyond max_distance (the bound is seven parts in ten
    // million above max_distance^2, an ulp of the root is at most 1.2 parts), so the root is formed for the few candidates
    // at or under it only, and the test on the root itself decides.  NaN fails both tests.
    const float bound = a.max_distance * a.max_distance * 1.000001f + 1.17549435e-38f;
    for (int base = 0; base < m_live; base += kRadiusTile) {   // (m_live: the same value in every thread)
        const int len = m_live - base < kRadiusTile ? m_live - base : kRadiusTile;
        const int padded = (len + 7) & ~7;                     // NaN points fill the last group of eight
        for (int k = tid; k < padded; k += 256)
            tile[k] = k < len ? make_float2(a.keys_cur[2 * (base + k)], a.keys_cur[2 * (base + k) + 1])
                              : make_float2(__builtin_nanf(""), __builtin_nanf(""));
        __syncthreads();
        if (live) {
            for (int k0 = 0; k0 < padded; k0 += 8) {   // index order; every thread reads the same addresses, eight reads in flight
                float2 t[8];
                float s[8];
#pragma unroll
                for (int u = 0; u < 8; u++) t[u] = tile[k0 + u];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const float dx = qx - t[u].x, dy = qy - t[u].y;
                    s[u] = dx * dx + dy * dy;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    if (s[u] <= bound) {
                        const float d = sqrtf(s[u]);
                        if (d <= a.max_distance) {    // (NaN: not a neighbour)
                            const int j = base + k0 + u;
                            if (cnt == 0) {
                                d0 = d, j0 = j;
                            } else if (d < d0) {      // strict: equal distances keep the lower train index in front
                                d1 = d0, d0 = d, j0 = j;
                            } else if (cnt == 1 || d < d1) {
                                d1 = d;
                            }
                            cnt++;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!row) return;   // (behind the last barrier)
    int32_t pick = kBadIndex;
    if (live) {
        if (cnt == 0) pick = kNoChoice;
        else if (cnt == 1) pick = j0;                                         // :1076
        else pick = ((double)(d0 / d1) < a.ratio) ? j0 : kOverlong;          // :1080-1084, f32 division then widened
    }
    a.choice[i] = pick, a.nnb[i] = cnt, a.dist0[i] = d0;
    if (pick >= 0) atomicMin(&a.owner[pick], i);
}

// s + v[0] + ... + v[k - 1] in order, one rounding per add, v in global memory: staged through LDS in rounds of 1024, wave 0
// adds a round from LDS (every lane the same address, eight entries per step), as k_post_filter forms its ordered sum.
// +0.0 pads the last round: an identity of a sum that starts at +0.0.
__device__ __forceinline__ double assoc_ordered_sum(const double *v, int32_t k, double *stage, double *out, int tid, int wave)
{
    double s = 0.0;
    for (int r0 = 0; r0 < k; r0 += 1024) {   // (k: the same value in every thread)
        __syncthreads();
        stage[tid] = r0 + tid < k ? v[r0 + tid] : 0.0;
        __syncthreads();
        if (wave == 0) {
            const int left = k - r0 < 1024 ? k - r0 : 1024;
            const double2 *b = reinterpret_cast<const double2 *>(stage);
#pragma unroll 2
            for (int j = 0; j < (left + 7) / 8 * 4; j += 4) {
                const double2 a0 = b[j], a1 = b[j + 1], a2 = b[j + 2], a3 = b[j + 3];
                s = s + a0.x, s = s + a0.y, s = s + a1.x, s = s + a1.y;
                s = s + a2.x, s = s + a2.y, s = s + a3.x, s = s + a3.y;
            }
        }
    }
    __syncthreads();
    if (tid == 0) *out = s;
    __syncthreads();
    return *out;
}

// max(0, the non-NaN values) -- what `m = v > m ? v : m` from m = 0 leaves, in any order -- of every thread's v >= +0.0 into
// *slot (LDS, zero before the first use).  Doubles that are not negative order as their bit patterns do.
__device__ __forceinline__ void assoc_max(double v, unsigned long long *slot, int lane)
{
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    if (lane == 0) atomicMax(slot, (unsigned long long)__double_as_longlong(v));
}

// One workgroup of 1024, behind k_radius_top2 on the stream.
__global__ void __launch_bounds__(1024) k_klt_finish(KltArgs a)
{
    __shared__ int32_t wtot[16], acc[6];
    __shared__ unsigned long long top[2];
    __shared__ double s_out;
    __shared__ __align__(16) double stage[1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t liveq = 0, nb0 = 0, nb1 = 0, nb2 = 0, ratio_rej = 0, lost = 0, k1 = 0;
    double max1 = 0.0;
    if (tid < 6) acc[tid] = 0;
    if (tid < 2) top[tid] = 0ull;
    __syncthreads();
    // first-come uniqueness (:1089-1105) and the disparities (:1096-1102)
    for (int c0 = 0; c0 < a.cap; c0 += 1024) {
        const int i = c0 + tid;
        int32_t t = kBadIndex, nb = 0;
        if (i < a.cap) t = a.choice[i], nb = a.nnb[i];
        const bool isq = t != kBadIndex;
        liveq += isq, nb0 += isq && nb == 0, nb1 += isq && nb == 1, nb2 += isq && nb >= 2, ratio_rej += t == kOverlong;
        const bool win = t >= 0 && a.owner[t] == i;
        lost += t >= 0 && !win;
        int32_t tot;
        const int32_t o = k1 + handover_scan(win, wtot, lane, wave, tot);
        if (win) {
            const float rx = a.pt_ref[2 * i], ry = a.pt_ref[2 * i + 1], cx = a.keys_cur[2 * t], cy = a.keys_cur[2 * t + 1];
            const double disp = (double)sqrtf((rx - cx) * (rx - cx) + (ry - cy) * (ry - cy));   // :1099, the f32 overload
            a.match_query[o] = i, a.match_train[o] = t, a.disparity[o] = disp;
            if (a.match_dist) a.match_dist[o] = a.dist0[i];
            max1 = disp > max1 ? disp : max1;
        }
        k1 += tot;
    }
    assoc_add(liveq, &acc[0], lane), assoc_add(nb0, &acc[1], lane), assoc_add(nb1, &acc[2], lane);
    assoc_add(nb2, &acc[3], lane), assoc_add(ratio_rej, &acc[4], lane), assoc_add(lost, &acc[5], lane);
    assoc_max(max1, &top[0], lane);
    const double sum1 = assoc_ordered_sum(a.disparity, k1, stage, &s_out, tid, wave);   // (its first barrier orders the stores above)
    const double avg1 = sum1 / (double)k1;   // :1109; k1 == 0: NaN, nothing is dropped
    const double th = avg1 * a.factor;       // :1116
    if (tid == 0) {
        for (int w = 0; w < 6; w++) a.info[w] = acc[w];   // (assoc_ordered_sum's barriers lie behind the adds)
        a.stats[0] = avg1, a.stats[2] = __longlong_as_double((long long)top[0]), a.stats[4] = th, a.stats[5] = sum1;
    }
    // the disparity filter (:1117-1129), in place: a group is read before the scan's barrier and written behind it, to rows
    // at or in front of the rows read
    int32_t k2 = 0;
    double max2 = 0.0;
    for (int c0 = 0; c0 < k1; c0 += 1024) {
        const int r = c0 + tid;
        int32_t q = 0, t = 0;
        float d = 0.0f;
        double disp = 0.0;
        if (r < k1) {
            q = a.match_query[r], t = a.match_train[r], disp = a.disparity[r];
            if (a.match_dist) d = a.match_dist[r];
        }
        const bool keep = r < k1 && !(disp > th);
        int32_t tot;
        const int32_t o = k2 + handover_scan(keep, wtot, lane, wave, tot);
        if (keep) {
            a.match_query[o] = q, a.match_train[o] = t, a.disparity[o] = disp;
            if (a.match_dist) a.match_dist[o] = d;
            max2 = disp > max2 ? disp : max2;
        }
        k2 += tot;
    }
    const double sum2 = assoc_ordered_sum(a.disparity, k2, stage, &s_out, tid, wave);
    const double avg2 = sum2 / (double)k2;   // :1130
    assoc_max(max2, &top[1], lane);
    __syncthreads();
    for (int o = k2 + tid; o < a.cap; o += 1024) {   // rows at or beyond the count
        a.match_query[o] = -1, a.match_train[o] = -1, a.disparity[o] = 0.0;
        if (a.match_dist) a.match_dist[o] = 0.0f;
    }
    if (tid == 0) {
        *a.n_matches = k2;
        a.info[6] = k1 - k2, a.info[7] = k2;
        a.stats[1] = avg2, a.stats[3] = __longlong_as_double((long long)top[1]), a.stats[6] = sum2, a.stats[7] = 0.0;
    }
}

}  // namespace pagk
