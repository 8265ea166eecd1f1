// pagk_group_lk_kernel.h -- the Lucas-Kanade stages of a sequence's frame for k cameras at once (include/pagk.h: Lucas-Kanade in
// the sequence groups, pagk_sequence_group_create_lk).  A frame of one Lucas-Kanade camera enqueues a copy of its level 0, one
// k_lk_pyrdown per pyramid level, a clear of its info words and k_lk_flow, which is one wavefront per feature: 250 workgroups
// at 1000 keypoints, a latency chain that leaves most of the device idle.  Here, as in pagk_group_kernel.h, the camera is a
// dimension of the grid: one launch per stage for the whole rig, and the flow launch of eight cameras is 2000 workgroups.
//
// A workgroup reads its camera's LkGroupRec from a third table the lead owns (record [parity * k + camera]) through the scalar
// cache; every pointer of a record is rebuilt as a global one (group_global, pagk_group_kernel.h), so the loads stay what they
// are in the single-camera kernels, where the pointers are kernel arguments.
//   k_group_lk_copy     every camera's frame in its input block into its parity copy of level 0, 16 bytes per thread
//   k_group_lk_clear    every camera's info words, in front of the flow launch (also when no pyramid launch exists)
//   k_group_lk_pyrdown  level l of every camera from its level l - 1: lk_pyrdown_body, the camera is blockIdx.z
//   k_group_lk_flow     the text of pagk_lk_body.h a third time, the camera is blockIdx.y.  The level descriptors stay in the
//                       record and are read inside the level loop, one level at a time.
// Plain HIP C++, vector stores only, no barrier.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pagk_lk_kernel.h"
#include "pagk_group_kernel.h"

namespace pagk {

// One camera's frame of one parity: the arguments its own copy, pyrDown launches, clear and k_lk_flow would carry.  Every
// pointer is fixed while the group's tables stand (the sequence's block, the frame slots' level 0, the LK_PYR buffers).
struct LkGroupRec {
    LkFlowArgs flow;                    // k_lk_flow of (slot 1 - parity, slot parity)
    LkPyrArgs pyr[kLkMaxLevels - 1];    // k_lk_pyrdown of slot `parity`: entry l - 1 builds level l
    const uint8_t *copy_src;            // the frame in the input block, or nullptr: level 0 is rectified in place
    uint8_t *copy_dst;                  // the parity's copy of level 0
    long long copy_bytes;
};

// what pagk_lk_body.h names `a.lv`: level l of the record, its two image pointers rebuilt as global ones
struct LkGroupLevels {
    const LkLevel *lv;
    __device__ __forceinline__ LkLevel operator[](int l) const
    {
        LkLevel L = lv[l];
        L.I = group_global(L.I), L.J = group_global(L.J);
        return L;
    }
};

// what pagk_lk_body.h names `a`: LkTrackArgs with the levels left in memory
struct LkGroupTrack {
    LkGroupLevels lv;
    const float *pt_ref;
    const int32_t *n;
    float *pt_out;
    uint8_t *status, *status_raw;
    float *err, *flow;
    int32_t *info;
    double eps2, min_eig;
    float err_threshold;
    int cap, win, top, max_count;
};

__global__ void __launch_bounds__(256) k_group_lk_copy(const LkGroupRec *__restrict__ table)
{
    const LkGroupRec &r = group_global(table)[blockIdx.y];
    const uint8_t *src = group_global(r.copy_src);
    uint8_t *dst = group_global(r.copy_dst);
    const long long bytes = r.copy_bytes, i = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i + 16 <= bytes && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(src + i);
    } else {
        for (long long j = i; j < min(i + 16, bytes); j++) dst[j] = src[j];
    }
}

__global__ void __launch_bounds__(64) k_group_lk_clear(const LkGroupRec *__restrict__ table)
{
    int32_t *info = group_global(group_global(table)[blockIdx.y].flow.t.info);
    if (threadIdx.x < kLkInfoWords) info[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(256) k_group_lk_pyrdown(const LkGroupRec *__restrict__ table, int level)
{
    const LkPyrArgs &a = group_global(table)[blockIdx.z].pyr[level - 1];
    lk_pyrdown_body(group_global(a.src), a.spitch, group_global(a.dst), a.sw, a.sh, a.dw, a.dh);
}

template <int NPIX>
__global__ void __launch_bounds__(256) k_group_lk_flow(const LkGroupRec *__restrict__ table)
{
    const LkFlowArgs &rec = group_global(table)[blockIdx.y].flow;
    LkFlowArgs f;   // (f.t is never read: the body takes the tracker's arguments from `a`)
    f.pt_init = group_global(rec.pt_init), f.status_in = group_global(rec.status_in), f.pt_out_dist = group_global(rec.pt_out_dist);
    f.fx = rec.fx, f.fy = rec.fy, f.cx = rec.cx, f.cy = rec.cy, f.fx_inv = rec.fx_inv, f.fy_inv = rec.fy_inv;
    f.k1 = rec.k1, f.k2 = rec.k2, f.p1 = rec.p1, f.p2 = rec.p2, f.k3 = rec.k3, f.distort_on = rec.distort_on;
    const LkTrackArgs &t = rec.t;
    const LkGroupTrack a = {{t.lv}, group_global(t.pt_ref), group_global(t.n), group_global(t.pt_out), group_global(t.status),
                            group_global(t.status_raw), group_global(t.err), group_global(t.flow), group_global(t.info), t.eps2,
                            t.min_eig, t.err_threshold, t.cap, t.win, t.top, t.max_count};
#define PAGK_LK_FLOW 1
#include "pagk_lk_body.h"
#undef PAGK_LK_FLOW
}

}  // namespace pagk
