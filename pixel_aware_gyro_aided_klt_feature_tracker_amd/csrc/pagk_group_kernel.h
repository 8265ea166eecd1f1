// pagk_group_kernel.h -- the small kernels of a sequence's frame for k cameras at once (include/pagk.h: the sequence group,
// pagk_sequence_group_step).  One frame of one camera enqueues ten kernels of one or two workgroups between and behind its
// pyramid and tracking launches: the prediction, Step 3, the five of the validation and the three of the hand-over.  Their
// cost is launch and dependent-load latency, and k cameras stepped one after another pay it k times.  Here the camera is
// blockIdx.y: one launch per stage for the whole rig.
//
// A workgroup reads its camera's argument record from a table in device memory.  The table is written once per group by a
// host copy that is over before the first launch, and the address table + blockIdx.y is the same in every lane: the record
// arrives through the scalar cache into scalar registers, as a kernel argument does.  Everything a workgroup then runs is
// the body of its camera's own launch (the *_body functions next to the single-camera kernels), on the same arguments,
// with blockIdx.x, blockDim and threadIdx as in that launch: the same arithmetic in the same order, the same bytes.
//
// An exit is a whole workgroup's -- a camera without live features, with fewer than nine correspondences, without a valid
// hypothesis -- and the barriers of a body are those of one workgroup: no camera waits for another one's.  The 1024-thread
// bodies (Step 3, the two compactions, the selection) hold a CU's sixteen wave slots of one SIMD row each: k of them run on
// k compute units side by side.
// Plain HIP C++, vector stores only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pagk_kernels.h"

namespace pagk {

// One camera's frame of one parity: every pointer is fixed from pagk_sequence_group_create on (the sequence's block, the
// context's fit workspace, its hand-over mask, its hints), every number is the group's common parameter.
struct GroupRec {
    PredictArgs predict;         // k_gyro_predict: d_rot is the camera's rot9 in its input block, live the reference set's mask
    // Step 3 (k_post_filter)
    int32_t n, half_patch;
    const uint8_t *pf_status_pm;
    const double *pf_pix_err, *pf_dist_pred;
    const float *pf_pt_pm, *pf_pt_pm_un;
    uint8_t *pf_status_out;
    float *pf_pt_predict, *pf_pt_predict_un;
    int32_t *pf_kept;
    double *pf_thresholds;
    // validation (k_fit_compact, k_fit_hyp, k_fit_refit, k_geometry_scores_fit, k_fit_select)
    const float *fit_pts1, *fit_pts2;
    uint8_t *fit_status;
    float *fit_p1, *fit_p2;      // the workspace's compacted correspondences, as k_fit_compact writes them
    int32_t *fit_idx;
    FitArgs fit;
    float sigma;
    uint8_t *inl_H, *inl_F;
    float *scores;
    int32_t *val_cnt;
    float *val_score;
    // hand-over (k_handover_fill, k_handover_holes, k_handover_keys)
    HandoverArgs hand;
    int64_t mask_bytes;
};

// A pointer that was read from the table is a generic one to the compiler, and a load through a generic pointer counts as
// divergent (it could address a lane's scratch): the bodies would lose their scalar loads and uniform branches.  Every
// pointer of a record addresses global memory, where a generic address is the global one: rebuilt from its bits as a pointer
// into the global address space it says so, and after inlining the bodies load as they do in the single-camera kernels,
// where the pointers are kernel arguments.  (A plain cast there and back is folded away.)
template <class T>
__device__ __forceinline__ T *group_global(T *p)
{
    typedef __attribute__((address_space(1))) T G;
    return (T *)(G *)(uintptr_t)p;
}
#define PAGK_GROUP_GLOBAL(x) x = group_global(x)

__device__ __forceinline__ FitArgs group_fit_args(const GroupRec *__restrict__ table)
{
    FitArgs a = group_global(table)[blockIdx.y].fit;
    PAGK_GROUP_GLOBAL(a.p1), PAGK_GROUP_GLOBAL(a.p2), PAGK_GROUP_GLOBAL(a.idx), PAGK_GROUP_GLOBAL(a.hdr);
    PAGK_GROUP_GLOBAL(a.hyp_models), PAGK_GROUP_GLOBAL(a.hyp_counts), PAGK_GROUP_GLOBAL(a.models), PAGK_GROUP_GLOBAL(a.info);
    PAGK_GROUP_GLOBAL(a.mask_H), PAGK_GROUP_GLOBAL(a.mask_F);
    return a;
}

__global__ void __launch_bounds__(256) k_group_gyro_predict(const GroupRec *__restrict__ table)
{
    PredictArgs a = group_global(table)[blockIdx.y].predict;
    PAGK_GROUP_GLOBAL(a.pt_ref), PAGK_GROUP_GLOBAL(a.pt_un), PAGK_GROUP_GLOBAL(a.pt_dist), PAGK_GROUP_GLOBAL(a.affine);
    PAGK_GROUP_GLOBAL(a.status), PAGK_GROUP_GLOBAL(a.d_rot), PAGK_GROUP_GLOBAL(a.live);
    gyro_predict_body(a, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ void __launch_bounds__(1024) k_group_post_filter(const GroupRec *__restrict__ table)
{
    const GroupRec &r = group_global(table)[blockIdx.y];
    post_filter_body(r.n, r.half_patch, group_global(r.pf_status_pm), group_global(r.pf_pix_err), group_global(r.pf_dist_pred),
                     group_global(r.pf_pt_pm), group_global(r.pf_pt_pm_un), group_global(r.pf_status_out),
                     group_global(r.pf_pt_predict), group_global(r.pf_pt_predict_un), group_global(r.pf_kept),
                     group_global(r.pf_thresholds));
}

__global__ void __launch_bounds__(1024) k_group_fit_compact(const GroupRec *__restrict__ table)
{
    const GroupRec &r = group_global(table)[blockIdx.y];
    fit_compact_body(r.n, group_global(r.fit_pts1), group_global(r.fit_pts2), group_global(r.fit_status), group_global(r.fit_p1),
                     group_global(r.fit_p2), group_global(r.fit_idx), group_global(r.fit.hdr), group_global(r.fit.models),
                     group_global(r.fit.info), nullptr, nullptr);
}

__global__ void __launch_bounds__(256) k_group_fit_hyp(const GroupRec *__restrict__ table)
{
    const FitArgs a = group_fit_args(table);
    fit_hyp_body(a);
}

__global__ void __launch_bounds__(256) k_group_fit_refit(const GroupRec *__restrict__ table)
{
    const FitArgs a = group_fit_args(table);
    fit_refit_body(a);
}

__global__ void __launch_bounds__(256) k_group_scores_fit(const GroupRec *__restrict__ table)
{
    const GroupRec &r = group_global(table)[blockIdx.y];
    FitHdr *hdr = group_global(r.fit.hdr);
    // (the chain's trip count is a scalar operand of its assembly: the count from the workspace, made one explicitly)
    geometry_scores_fit_body(group_global(r.fit.models), group_global(r.fit.info), __builtin_amdgcn_readfirstlane(hdr->m), group_global(r.fit_p1),
                             group_global(r.fit_p2), r.sigma, group_global(r.inl_H), group_global(r.inl_F), group_global(r.scores));
}

__global__ void __launch_bounds__(1024) k_group_fit_select(const GroupRec *__restrict__ table)
{
    const GroupRec &r = group_global(table)[blockIdx.y];
    fit_select_body(group_global(r.fit.hdr), group_global(r.fit.info), group_global(r.scores), group_global(r.inl_H),
                    group_global(r.inl_F), group_global(r.fit_idx), group_global(r.fit_status), group_global(r.val_cnt),
                    group_global(r.val_score));
}

__global__ void __launch_bounds__(256) k_group_handover_fill(const GroupRec *__restrict__ table)
{
    const GroupRec &r = group_global(table)[blockIdx.y];
    handover_fill_body(group_global(r.hand.mask), r.mask_bytes);
}

__global__ void __launch_bounds__(256) k_group_handover_holes(const GroupRec *__restrict__ table)
{
    const GroupRec &r = group_global(table)[blockIdx.y];
    handover_holes_body(r.hand.cap, r.hand.width, r.hand.height, group_global(r.hand.status), group_global(r.hand.pt_predict_un),
                        group_global(r.hand.mask));
}

__global__ void __launch_bounds__(1024) k_group_handover_keys(const GroupRec *__restrict__ table)
{
    HandoverArgs a = group_global(table)[blockIdx.y].hand;
    PAGK_GROUP_GLOBAL(a.status), PAGK_GROUP_GLOBAL(a.pt_predict), PAGK_GROUP_GLOBAL(a.pt_predict_un), PAGK_GROUP_GLOBAL(a.n_cand);
    PAGK_GROUP_GLOBAL(a.cand_un), PAGK_GROUP_GLOBAL(a.keys), PAGK_GROUP_GLOBAL(a.keys_un), PAGK_GROUP_GLOBAL(a.keys_normal);
    PAGK_GROUP_GLOBAL(a.index_in_last), PAGK_GROUP_GLOBAL(a.live), PAGK_GROUP_GLOBAL(a.mask), PAGK_GROUP_GLOBAL(a.state);
    PAGK_GROUP_GLOBAL(a.prio_hint);
    handover_keys_body(a);
}

#undef PAGK_GROUP_GLOBAL

}  // namespace pagk
