/*
 * pagk.h -- C ABI of the MI355X-native pyramidal patch-based KLT refinement.
 *
 * This is the drop-in boundary for ONE path of the reference tracker: the body of
 * PatchMatch::OpticalFlowMultiLevel() (reference src/patch_match.cpp:79-142) and
 * everything it calls.  Plain pointers and sizes only; no C++/torch types.
 *
 * Every entry point cites the reference interface it replaces.  All buffers are
 * caller-owned; the library owns only its pagk_ctx (device buffers, stream).
 *
 * Conventions
 *   - points are interleaved (x, y) float32 pairs, n of them  (cv::Point2f layout)
 *   - affine is n x 4 float32, row-major 2x2 per feature      (cv::Mat CV_32F 2x2,
 *     reference src/gyro_aided_tracker.cpp:166-168)
 *   - status bytes are 0 / 1                                   (std::vector<uchar>)
 *   - an image given as data, width, height and step (a pagk_image, or the d_data / d_next / d_raw of the *_device
 *     calls) is (height - 1) * step + width bytes long (d_raw: src_width * channels in place of width): the bytes of a
 *     row beyond its last pixel and everything after the last row's last pixel are not part of it: they are
 *     never written and no result depends on them
 *   - return value: 0 = PAGK_OK, negative = error (never throws, never aborts)
 */
#ifndef PAGK_H
#define PAGK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAGK_VERSION 303 /* 0.3.3: + pagk_priority_threshold (the fits, pagk_post_filter_device, pagk_frame_handover[_device] and pagk_gyro_predict_device_live came later under the same number: ask for a symbol, not for the number); 0.3.2: + pagk_frame_set_device_batch; 0.3.1: pipelined 4-wave kernel, pagk_track_device_batch, pagk_check_launch, pagk_selftest_repeat_sum */

#define PAGK_MAX_PYRAMIDS 8
#define PAGK_MAX_HALF_PATCH 15 /* (2h+1)^2 <= 961 pixels */

enum {
    PAGK_OK = 0,
    PAGK_E_ARG = -1,         /* null pointer / out-of-range parameter                     */
    PAGK_E_HIP = -2,         /* a HIP runtime call failed (see pagk_last_error)           */
    PAGK_E_NOMEM = -3,       /* device or host allocation failed                          */
    PAGK_E_UNSUPPORTED = -4, /* pagk_params::inverse other than 0 and PAGK_INVERSE_TEMPLATE (1 is the reference's
                                bInverse_: "not support yet"); a variant or mode this build does not carry */
    PAGK_E_NODEVICE = -5,    /* no HIP device / HIP library could not initialise          */
    PAGK_E_NCCL = -6,        /* an RCCL call of the sharded path failed (see pagk_last_error) */
    PAGK_E_CAPACITY = -7     /* a caller-sized output array is too small (neighbour lists)  */
};

/* 8-bit single-channel image view.  Mirrors the fields of cv::Mat (CV_8UC1) the
 * reference reads: data, cols, rows, step (src/patch_match.cpp:396-403). */
typedef struct pagk_image {
    const uint8_t *data;
    int32_t width;  /* cv::Mat::cols */
    int32_t height; /* cv::Mat::rows */
    int64_t step;   /* cv::Mat::step, bytes per row, >= width */
} pagk_image;

/* Arguments of PatchMatch::PatchMatch (include/patch_match.h:44-49) plus the
 * constants its constructor hard-codes (src/patch_match.cpp:48-57) and the camera
 * model DistortPoints() reads from the tracker (src/patch_match.cpp:409-416,
 * src/utils.cpp:49-76). Fill with pagk_params_default() and override. */
typedef struct pagk_params {
    int32_t half_patch; /* halfPatchSize_  (reference apps: 5; BASELINE: 10)             */
    int32_t iterations; /* iterations_     (reference call site: 10; BASELINE: 30)       */
    int32_t pyramids;   /* pyramids_       (reference call site: 3)                      */
    uint8_t has_gyro_predict_initial; /* bHasGyroPredictInitial_: 0 => pt_init ignored   */
    uint8_t inverse;                  /* 0 = forward mode (the reference's path).  1 = bInverse_, the reference's own
                                         branch: PAGK_E_UNSUPPORTED, as there.  2 = PAGK_INVERSE_TEMPLATE, the library's
                                         template-Jacobian mode defined below.  Others: PAGK_E_UNSUPPORTED.          */
    uint8_t consider_illumination;    /* bConsiderIllumination_                           */
    uint8_t consider_affine;          /* bConsiderAffineDeformation_                      */
    uint8_t regularization_penalty;   /* bRegularizationPenalty_                          */
    uint8_t calculate_ncc;            /* bCalculateNCC_                                   */
    uint8_t predict_method;           /* pagk_gyro_predict_device only: 0 or 1 = PIXEL_AWARE_PREDICTION, 2 =
                                         SINGLE_HOMOGRAPHY (ePredictMethod, include/gyro_aided_tracker.h:66-69)   */
    uint8_t solver_variant;           /* 0 = Eigen 3.3 with SSE2 packets, as restated in oracle/README.md.  Bits select
                                         the association another Eigen version / build uses in H.llt().solve(b) and
                                         update.norm() (src/patch_match.cpp:319,343):  1 lower solve row 3 as
                                         (c0+c1)+c2;  2 upper solve row 0 as c0+(c1+c2);  4 squaredNorm sequential
                                         (EIGEN_DONT_VECTORIZE);  8 LLT column scaling by the reciprocal (Eigen <= 3.2);
                                         32 4th pivot's squaredNorm as a0+(a1+a2).  Same bits as
                                         pagk_oracle_set_alternatives.  Others: PAGK_E_ARG.                         */
    float lambda;            /* mLambda      = 1.0f  (:48) */
    float alpha;             /* mAlpha       = 0.5f  (:49) */
    int32_t max_distance;    /* mMaxDistance = 25    (:50) */
    float inv_log_max_dist;  /* mInvLogMaxDist (:51); 0 => computed by the library       */
    /* camera model used only by the distortion epilogue */
    float fx, fy, cx, cy;    /* mK(0,0), mK(1,1), mK(0,2), mK(1,2)                        */
    float dist_coef[5];      /* k1 k2 p1 p2 k3                                            */
    int32_t n_dist_coef;     /* 4 or 5 (mDistCoef.total()); k3 ignored unless 5           */
} pagk_params;

/* ---- Template-Jacobian mode: pagk_params::inverse == PAGK_INVERSE_TEMPLATE ---------------------------------------------
 * The Gauss-Newton loop with the Jacobian taken from the REFERENCE image, once per pyramid level: what the reference's
 * bInverse_ branch (src/patch_match.cpp:216-222, :265-275, :286-297) sets out to do and refuses ("not support yet", :220).
 * Everything around the loop is the forward path unchanged: the level loop and its initial points (:177-183), dg = db = 0
 * per level, warp_patch (:198-209), the member GetPixelValue, the residual (:252-253) with its association, the penalty
 * (:302-314), solver_variant, the termination rules (:319-344), :348-353, NCC (:356-366), DistortPoints and SetMatcher.
 *
 * Per feature and level, with pt the reference point at the level, h = half_patch, pixel k = (y + h)(2h + 1) + (x + h) for
 * y (outer) and x in -h .. h, I1 / I2 = GetPixelValue on the level of the reference / current image:
 *   set-up, once, before iteration 0:
 *     T_k  = I1(pt.x + x, pt.y + y)
 *     Ix_k = (float)(0.5 * (I1(pt.x + x + 1, pt.y + y) - I1(pt.x + x - 1, pt.y + y)))      (:269-270)
 *     Iy_k = (float)(0.5 * (I1(pt.x + x, pt.y + y + 1) - I1(pt.x + x, pt.y + y - 1)))      (:271-272)
 *            coordinate sums left to right in f32; the f32 difference is widened, halved and narrowed
 *     c    = I1(pt.x, pt.y);   J_k = (Ix_k, Iy_k, -c, 1) widened to f64                    (:273-274)
 *     Hp   = sum_k J_k J_k^T:  ten f64 sums of exact products
 *   every iteration:
 *     e_k  = I2(pt.x + dx + wx_k, pt.y + dy + wy_k) + db - (1 + dg) * T_k                  (:252-253, (wx, wy) = warp_patch)
 *     b    = sum_k (-J_k) (double)e_k      cost = sum_k e_k * e_k in f32      H = Hp
 *     then the penalty (if set) on this fresh H, b and cost, the solve, and :319-344, as in the forward path.
 * The sums.  Each of the fifteen sums over the patch is taken in one order that depends on half_patch alone -- not on the
 * launch size, the entry point or any hardware state: pixel k belongs to slot k mod 64; a slot starts at +0.0 and adds its
 * pixels in ascending k (a slot without pixels stays +0.0); then six steps v[s] = v[s] + v[s ^ m] over all 64 slots at
 * once, m = 1, 2, 4, 8, 16, 32; the sum is v[0].  Accumulators are f64 for Hp and b, f32 for the cost.
 * tests/inverse_ref.c restates the mode sequentially; every entry point returns its bits.
 *
 * Departures from the reference's branch: (1) the Jacobians are kept per pixel (the reference overwrites vJ[i] with an unset
 * local from iteration 1 on and accumulates with the last pixel's Jacobian); (2) H is rebuilt from Hp in every iteration, so
 * the penalty term does not pile up as :295-297 with :311 would have it; (3) the summation order is the library's own.
 * Kept on purpose: -I1(pt), the patch CENTRE, as the gain column -- in exact arithmetic a singular H, as in the forward
 * mode -- so that both modes fit the same model.
 *
 * A launch of this mode runs one kernel (csrc/pagk_inverse_kernel.h; every half_patch 1 .. 15) and pagk_last_variant reports
 * 8 after it; pagk_has_variant(8) == 1.  pagk_set_kernel (1, 3, 5 and 7 included), the issue-priority hint, the dispatch
 * order and the hand-over do not apply to such a launch.  pagk_track_device_fused runs pyramid and tracking as two launches,
 * pagk_track_device_batch as k launches.  Accuracy is claimed where the coarsest level holds the patch (DESIGN.md,
 * "Template-Jacobian mode"); the results are defined and reproducible everywhere. */
#define PAGK_INVERSE_TEMPLATE 2

/* check of a pagk_params as every tracking entry point applies it: PAGK_OK, PAGK_E_ARG (NULL, half_patch outside
 * 1 .. PAGK_MAX_HALF_PATCH, iterations < 0, pyramids outside 1 .. PAGK_MAX_PYRAMIDS, an unknown solver_variant bit) or
 * PAGK_E_UNSUPPORTED (inverse other than 0 and PAGK_INVERSE_TEMPLATE).  Needs no device. */
int pagk_params_check(const pagk_params *params);

/* Outputs == the six vectors PatchMatch::SetMatcher fills on the tracker
 * (src/patch_match.cpp:370-388, include/gyro_aided_tracker.h:214-219) plus an
 * optional diagnostic. Any pointer except pt_un/status may be NULL. */
typedef struct pagk_outputs {
    float *pt_un;      /* n x 2  mvPtPredictAfterPatchMatchedUn                           */
    float *pt_dist;    /* n x 2  mvPtPredictAfterPatchMatched (distorted)                 */
    uint8_t *status;   /* n      mvStatusAfterPatchMatched                                */
    double *pix_err;   /* n      mvPixelErrorsOfPatchMatched                              */
    double *dist_pred; /* n      mvDistanceBetweenPredictedAndPatchMatched                */
    float *ncc;        /* n      mvNccAfterPatchMatched                                   */
    int32_t *iters;    /* n      diagnostic: Gauss-Newton iterations executed, summed
                                 over levels (not in the reference)                       */
} pagk_outputs;

typedef struct pagk_ctx pagk_ctx;

/* ---- library / context ------------------------------------------------------ */
int pagk_version(void);
const char *pagk_strerror(int code);
/* Text of the last HIP failure on this context (empty string if none). */
const char *pagk_last_error(const pagk_ctx *ctx);

/* Defaults == reference call site src/gyro_aided_tracker.cpp:276-282 with
 * eType GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED_CONSIDER_ILLUMINATION_DEFORMATION
 * (:402-408): h=5, 10 iterations, 3 levels, gyro init, illumination + affine. */
void pagk_params_default(pagk_params *p);
/* mInvLogMaxDist exactly as src/patch_match.cpp:51 computes it. */
float pagk_inv_log_max_dist(float alpha, int32_t max_distance);

/* One context per host thread / GPU (reference: one PatchMatch per tracker, not
 * re-entrant because of the shared mLevel, src/patch_match.cpp:99). */
int pagk_create(pagk_ctx **out, int device);
void pagk_destroy(pagk_ctx *ctx);

/* ---- the hot path, host buffers (drop-in for OpticalFlowMultiLevel) -------- */
/* Replaces PatchMatch::OpticalFlowMultiLevel() src/patch_match.cpp:79-142:
 * CreatePyramids (:61-76) + per-level per-feature GN loop (:167-367) +
 * DistortPoints (:409-416) + SetMatcher (:370-388).  Synchronous.
 *   pt_ref_un  = mvKeysRefUn[i].pt        pt_init_un = mvPtPredictUn[i]
 *   affine     = mvAffineDeformationMatrix[i] (may be NULL iff !consider_affine)
 *   status_in  = mvStatus[i] snapshot (mvGyroPredictStatus, :58)                */
int pagk_track(pagk_ctx *ctx, const pagk_params *params, const pagk_image *ref,
               const pagk_image *cur, int32_t n, const float *pt_ref_un,
               const float *pt_init_un, const float *affine, const uint8_t *status_in,
               const pagk_outputs *out);

/* Same, but with caller-built pyramids (levels[0] = full resolution), so a host
 * that links real OpenCV can hand over cv::resize output (:69-70) verbatim. */
int pagk_track_pyr(pagk_ctx *ctx, const pagk_params *params, int32_t n_levels,
                   const pagk_image *ref_levels, const pagk_image *cur_levels, int32_t n,
                   const float *pt_ref_un, const float *pt_init_un, const float *affine,
                   const uint8_t *status_in, const pagk_outputs *out);

/* ---- the hot path, device-resident (streams of frame pairs, benchmarks) ---- */
/* Upload a frame into one of the context's frame slots and build its pyramid on
 * the device (CreatePyramids :61-76). In a sequence, cur of pair t is ref of pair
 * t+1, so each frame is uploaded once. slot in [0, 4).  Returns after img->data has been read (the caller may
 * reuse the buffer at once, also when it is pinned memory); the pyramid kernels may still be running. */
int pagk_frame_upload(pagk_ctx *ctx, int32_t slot, const pagk_image *img, int32_t pyramids);
/* The same for a frame in PINNED host memory (a camera ring buffer): asynchronous on the context's stream and
 * capturable -- inside pagk_graph_begin / pagk_graph_end the host -> device copy becomes a graph node, so a live loop
 * (Examples/Demo/RealSenseD435i.cpp:199-321: grab, track) replays [copy the frame -> pyramid -> PatchMatch] with one
 * pagk_graph_launch per frame.  The memory must stay pinned, and unchanged until the enqueued work has run. */
int pagk_frame_upload_pinned(pagk_ctx *ctx, int32_t slot, const pagk_image *img, int32_t pyramids);
/* Same for an image that already lives in device memory (d_data: device pointer,
 * rows of `step` bytes). Asynchronous on the context stream. */
int pagk_frame_set_device(pagk_ctx *ctx, int32_t slot, const void *d_data, int32_t width,
                          int32_t height, int64_t step, int32_t pyramids);
/* pagk_frame_set_device for the frames of k contexts that share one device, as ONE launch: PatchMatch::CreatePyramids
 * (src/patch_match.cpp:61-76) of k trackers that are stepped together (BASELINE configs[4], "batched multi-camera ...
 * shared pyramid upload"); the producer side of pagk_track_device_batch.  Frame j (device image d_data[j], width[j] x
 * height[j], rows step[j] bytes apart) goes into slot[j] of ctxs[j]; per frame the same bytes as pagk_frame_set_device.
 * The launch is issued on ctxs[0]'s stream and ordered against the other contexts' streams like pagk_track_device_batch;
 * its frame descriptors follow the same rules inside a capture (issue the call once directly first; at most four batched
 * calls of either kind per capture).  Frames the single-launch kernel does not serve (a parent level with an odd
 * dimension, more than four levels) make the call k per-context launches.  k <= 64. */
int pagk_frame_set_device_batch(pagk_ctx *const *ctxs, int32_t k, const int32_t *slot, const void *const *d_data,
                                const int32_t *width, const int32_t *height, const int64_t *step, int32_t pyramids);
/* Copy one pyramid level of a slot back to the host (tests: pyramid parity).  Level 0 is the image the pyramid was built
 * from: the slot's own copy, or the caller's device image where the slot reads it in place. */
int pagk_frame_download_level(pagk_ctx *ctx, int32_t slot, int32_t level, uint8_t *dst,
                              int32_t *width, int32_t *height);

/* Track with every per-feature array in DEVICE memory (all pointers are device
 * pointers; same layouts as pagk_track). Asynchronous on the context stream;
 * call pagk_sync before reading results on the host.  Every array is n elements (n x 2, n x 4) long: nothing is
 * written beyond it and no result depends on what lies beyond it.  n = 0 is valid and leaves every output untouched. */
int pagk_track_device(pagk_ctx *ctx, const pagk_params *params, int32_t slot_ref,
                      int32_t slot_cur, int32_t n, const float *d_pt_ref_un,
                      const float *d_pt_init_un, const float *d_affine,
                      const uint8_t *d_status_in, const pagk_outputs *d_out);
/* pagk_track_device for the pair (slot_ref, slot_cur) AND CreatePyramids (src/patch_match.cpp:61-76) of another
 * frame -- device image d_next, built into slot_next -- in ONE launch: when the 4-wave kernel is the one
 * selected, the pyramid is computed by trailing workgroups of the tracking launch and costs no launch of its
 * own; otherwise it is launched separately.  Results are those of pagk_frame_set_device(slot_next, ...) plus
 * pagk_track_device(...).  For pipelines that hold frame k+1 while pair (k-1, k) is tracked (replays, or a
 * camera loop that accepts one frame of latency).  slot_next must differ from slot_ref and slot_cur. */
int pagk_track_device_fused(pagk_ctx *ctx, const pagk_params *params, int32_t slot_ref, int32_t slot_cur, int32_t n,
                            const float *d_pt_ref_un, const float *d_pt_init_un, const float *d_affine,
                            const uint8_t *d_status_in, const pagk_outputs *d_out, int32_t slot_next,
                            const void *d_next, int32_t width, int32_t height, int64_t step, int32_t pyramids);
/* pagk_track_device for k camera streams that share one device, as ONE launch (BASELINE configs[4]: "batched
 * multi-camera").  The reference builds one PatchMatch per tracker (src/gyro_aided_tracker.cpp:276-283); this is k of those
 * calls at once: stream j is context ctxs[j] (its frame slots slot_ref[j] / slot_cur[j] hold the pyramids), n[j] features
 * in the device arrays d_pt_ref_un[j], d_pt_init_un[j], d_affine[j], d_status_in[j], results to d_out[j]; `params` is
 * common to all (the trackers of one application are configured alike).  Results per stream are bit-identical to its own
 * pagk_track_device.  From 6000 features in total (or pagk_set_kernel(ctxs[0], 7)) the streams are served by one launch
 * of variant 7 whose four-feature groups carry their stream; smaller batches, calculate_ncc, one-level pyramids and
 * inverse == PAGK_INVERSE_TEMPLATE run as k launches.  The launch is issued on ctxs[0]'s stream: it waits for what the other contexts' streams have enqueued
 * so far, and their later work waits for it (contexts switched to one common stream with pagk_set_stream need neither,
 * and can be captured together: pagk_graph_begin(ctxs[0]) ... pagk_graph_end -- after the same call has been issued once
 * directly, at most four batched calls (of this kind and of pagk_frame_set_device_batch together) per capture: the stream descriptors a captured launch reads are buffers that
 * pagk_graph_begin reserves and the graph owns, so that no later call can rewrite them under a replay; a direct call's are
 * not reused before that launch is over).  Pointer arrays are host arrays of device pointers, read during the call;
 * d_pt_init_un / d_affine may be NULL when the flags do not use them.  k <= 64, all contexts on one device. */
int pagk_track_device_batch(pagk_ctx *const *ctxs, int32_t k, const pagk_params *params, const int32_t *slot_ref,
                            const int32_t *slot_cur, const int32_t *n, const float *const *d_pt_ref_un,
                            const float *const *d_pt_init_un, const float *const *d_affine,
                            const uint8_t *const *d_status_in, const pagk_outputs *d_out);
int pagk_sync(pagk_ctx *ctx);
/* For callers that synchronise the stream themselves (pagk_set_stream: a torch stream, the host application's own) and
 * so never pass through pagk_sync: the error state pagk_sync would have returned, without synchronising.  Call it after
 * your own synchronisation.  PAGK_E_HIP (once) when a wave of a level-by-level launch (kernel 7) gave up its bounded
 * wait -- never expected; such a launch also clears its status array, so nothing stale can pass for a tracked point. */
int pagk_check_launch(pagk_ctx *ctx);
/* Use an external HIP stream (e.g. torch's current stream) instead of the
 * context's own; pass NULL to restore. */
int pagk_set_stream(pagk_ctx *ctx, void *hip_stream);

/* Kernel selection.  0 = automatic (default): by launch size (thresholds measured on MI355X at half_patch 10), one of
 *   - 4-wave workgroup per feature, DPP-row ordered accumulation  (lowest latency; < 6000 features)
 *   - one wavefront per feature, f32 streams + MFMA chain  (= 3; calculate_ncc launches from 6000 features, and 6000 to
 *     6999 features in total when the device is shared)
 *   - four features per wavefront, one pyramid level per wavefront  (= 7; from 6000 features, context alone on the device)
 *   - four features per wavefront  (= 5; from 7000 features in total when pagk_set_concurrency says the device is shared)
 * Selected explicitly only:
 *   - 2-wave workgroup per feature, ordered accumulation as a v_mfma_f64_4x4x4f64 chain  (= 2)
 * 1 = reference-shaped one-thread-per-feature kernel (debug / cross-check).  2 and 3 force a variant
 * (half_patch 5, 7 or 10; other sizes fall back to the 4-wave kernel).  Every variant 0-3 produces
 * bit-identical results.
 * 4 = EXPERIMENT, never chosen automatically: the 4-wave kernel with the reference's summation order
 *     given up (strided partial sums + tree instead of the 441-step ordered chains).  Not parity-exact:
 *     it exists to measure what the ordered accumulation costs.
 * 5 = four features per wavefront (block q of the f64 MFMA, row q of the cost chain and lane = feature solve shared
 *     by four features): a throughput variant for very large launches; bit-identical like 0-3.
 *     A launch of this variant that would end with an exposed tail (0.45 to 1.25 rounds of resident waves, the
 *     context alone on the device, not inside a graph capture) hands the features that have run 20 iterations to the
 *     4-wave latency kernel, which runs beside it on the context's auxiliary stream; results are the same bits.
 * 6 = 5 with the four rows of a wave independent (each row runs its own feature at its own level and takes the next
 *     feature from a work queue when it is done; a resident grid): bit-identical like 0-3.
 * 7 = 5 with one pyramid LEVEL per wavefront: pyramids x ceil(n / 4) wavefronts, each a third (a quarter) of the
 *     lifetime of a whole-feature wavefront, a quad handed from its level to the next through device memory (the
 *     waiting wavefront always waits for one that started earlier; the wait is bounded all the same and a launch in
 *     which one ran out reports PAGK_E_HIP at the next synchronisation).  For launches of about one to two rounds of
 *     resident wavefronts, which otherwise end with most of the device idle.  Bit-identical like 0-3.  With one
 *     pyramid level, or calc_ncc, it is 5. */
int pagk_set_kernel(pagk_ctx *ctx, int32_t which);
/* Variants 2 and 6 no longer win at any launch size and nothing selects them automatically; the product's build leaves
 * them out (pagk_set_kernel returns PAGK_E_UNSUPPORTED for them) and a library compiled with -DPAGK_ALL_VARIANTS carries
 * them for cross-checks.  1 = `which` can be selected in this build; also for 8, the kernel of PAGK_INVERSE_TEMPLATE, which
 * the parameters select and pagk_set_kernel does not. */
int pagk_has_variant(int32_t which);
/* The variant (numbering above; 0 = the 4-wave kernel; 8 = the kernel of PAGK_INVERSE_TEMPLATE) the last tracking launch
 * of this context actually used; -1 before the first launch. */
int pagk_last_variant(const pagk_ctx *ctx);

/* Number of features the last tracking launch of this context handed from the throughput kernel to the latency
 * kernel (variant 5, see above); 0 when the launch did not use the hand-over.  Synchronises the context's stream. */
int pagk_last_handover(pagk_ctx *ctx);

/* Diagnostic: the threshold K the next launch of the 4-wave kernels will use for its issue priorities (a workgroup that has used more
 * than K iterations per pyramid level entered outranks its neighbours; csrc/pagk_prio.h -- no arithmetic effect).  4 by default;
 * PAGK_PRIO_K in the environment of pagk_create fixes another value (0 = off) or, as "auto", lets K follow the mean number of
 * iterations per feature and level the context's launches have run.  No counterpart in the reference.  Synchronises the context's stream. */
int pagk_priority_threshold(pagk_ctx *ctx);

/* The hint of the same priorities (csrc/pagk_prio.h -- no arithmetic effect).  Every launch of the 4-wave kernels stores, per feature
 * SLOT (index into the arrays of the call), the iterations the feature ran; in the context's next launch a slot whose count exceeded
 * the threshold outranks its neighbours from its first iteration -- a tracker follows the same patch frame after frame, and last
 * frame's straggler is the best forecast of this frame's.  The forecast holds only while index i still means the same feature:
 *   - the host-buffer calls (pagk_track, pagk_track_pyr, pagk_track_sharded) install new arrays: they clear the hints, read none and
 *     store none;
 *   - a caller of the *_device calls that writes NEW features into its device arrays calls pagk_prio_hint_reset (stream order,
 *     capturable); one that keeps a feature at its index from frame to frame (status_in = 0 for the lost ones) calls nothing.
 * A stale or wrong hint costs issue order, never a bit of a result.  PAGK_PRIO_HINT in the environment of pagk_create sets the
 * threshold (a whole number; 0 = off; 14 by default).  It is stated for three pyramid levels: a launch of L levels compares with
 * threshold * L / 3, rounded up; a launch of no more workgroups than the device has CUs stores its counts and boosts nobody.  _get / _set copy the first n hints to / from HOST memory and synchronise (diagnostics, tests).
 * The array grows with the largest launch, and it may not grow inside a capture or while a graph of the context is alive: run the
 * largest *_device launch once directly BEFORE capturing (as for the other workspaces) -- a launch that meets too small an array
 * there is not refused, it runs without reading or storing hints.  A launch that selects another kernel than the 4-wave one at four
 * workgroups per CU (1025-1280 and 2500+ features, the other variants) leaves the array as it was: the next 4-wave launch reads older counts.
 * No counterpart in the reference. */
int pagk_prio_hint_threshold(pagk_ctx *ctx);
int pagk_prio_hint_reset(pagk_ctx *ctx);
int pagk_prio_hint_get(pagk_ctx *ctx, int32_t n, int32_t *hints);
int pagk_prio_hint_set(pagk_ctx *ctx, int32_t n, const int32_t *hints);

/* The dispatch order of the 4-wave kernels (csrc/pagk_order.h): workgroup b of a launch runs the feature with the b-th largest
 * hint -- a stable counting sort of the hints clamped to [0, 127], descending, ties in index order -- so that the features that
 * ran longest last time start first and on different compute units.  It decides when a feature runs and beside whom, never a bit
 * of a result.  The array is built on the device by one extra workgroup of the pyramid launch (pagk_frame_set_device,
 * pagk_frame_upload*, pagk_frame_rectify*) that precedes the tracking launch on the same stream, for the n of the context's last
 * *_device 4-wave launch (or of pagk_prio_hint_set), when that n is above the device's CU count and at most 8192.  A launch uses
 * it only when such a build for exactly its n was enqueued on its stream since the last 4-wave launch or hint write; otherwise --
 * hints cleared, host-buffer calls, another stream, a pyramid built by pagk_track_device_fused or pagk_frame_set_device_batch, an
 * array that could not grow under a live graph -- it runs in index order.  The array is bound to the stream of its last build,
 * reader or graph replay until the host has waited for that stream (pagk_sync, pagk_graph_destroy, the _get calls): pyramids and
 * launches on other streams meanwhile leave it alone.  Inside pagk_graph_begin's capture the decision is recorded with the graph; a
 * replayed [pagk_frame_set_device -> pagk_track_device] graph rebuilds and uses the order on every replay, and a replay on another
 * stream than the one the array is bound to waits for the device first.  Any other capture of the stream neither builds nor uses it.
 * PAGK_DISPATCH_ORDER=0 in the environment of pagk_create switches it off (_enabled: 1 / 0).  _get copies the first n entries of
 * the array as it is on the device to HOST memory and synchronises (diagnostics, tests; not capturable; entries the array does
 * not hold read as the identity); *in_force (may be NULL) is 1 when a 4-wave *_device launch of n features enqueued next on the
 * current stream would use the array.  No counterpart in the reference. */
int pagk_dispatch_order_enabled(pagk_ctx *ctx);
int pagk_dispatch_order_get(pagk_ctx *ctx, int32_t n, int32_t *order, int32_t *in_force);

/* Concurrency hint for the automatic selection: the caller runs `streams` contexts like this one at the same time on
 * this device (one PatchMatch per camera stream, BASELINE configs[4]: src/patch_match.cpp:79-142 called from several
 * threads).  The launch-size thresholds above are then applied to streams * n: a launch that would get a latency
 * variant on an empty device gets the throughput variant when the device is shared -- measured with eight concurrent
 * 1280x720 x 4000 streams: 26-29 instead of 17.6 Mfeat/s in aggregate (profiles/r02_ab_runs.md).  Results do not
 * depend on the variant.  streams = 1 (default) .. 64. */
int pagk_set_concurrency(pagk_ctx *ctx, int32_t streams);

/* Milliseconds spent in the tracking kernel(s) of the last pagk_track*_ call,
 * measured with HIP events on the stream the kernels ran on. Synchronises. */
int pagk_last_kernel_ms(pagk_ctx *ctx, float *track_ms, float *pyramid_ms);

/* ---- producer / consumer rows next to the path ----------------------------- */
/* GyroAidedTracker::GyroPredictFeatures + GyroPredictOnePixel (src/gyro_aided_tracker.cpp:118-185,194-256), both
 * prediction methods (params->predict_method: PIXEL_AWARE_PREDICTION :212-231, or SINGLE_HOMOGRAPHY :233-253, the
 * same with lambda = 1), on the device: predicted point (un-distorted and
 * distorted), border status and the 2x2 affine A = C B^T (B B^T)^-1 from the four predicted patch corners.
 * Produces exactly the arrays pagk_track_device consumes, so prediction -> tracking needs no host
 * round trip.  All pointers are device pointers; camera model from params (fx fy cx cy dist_coef);
 * KRKinv = mK * mRcl * mK^-1 (3x3 row-major, :518), r3 = third row of mRcl.  Where a prediction leaves
 * the image the outputs keep the tracker's initial state: status 0, points (0,0), affine untouched.
 * d_affine may be NULL.  Asynchronous on the context stream. */
int pagk_gyro_predict_device(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                             const float *KRKinv, const float *r3, int32_t n, const float *d_pt_ref_un,
                             float *d_pt_predict_un, float *d_pt_predict, uint8_t *d_status, float *d_affine);
/* The same with the rotation in DEVICE memory: d_rot = 9 floats, rows 0 and 1 of KRKinv followed by r3.
 * For graph capture: kernel arguments are frozen into a captured graph, device memory is not, so a graph
 * holding upload -> pyramid -> prediction -> tracking replays every frame with that frame's rotation. */
int pagk_gyro_predict_device_rot(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                                 const float *d_rot, int32_t n, const float *d_pt_ref_un, float *d_pt_predict_un,
                                 float *d_pt_predict, uint8_t *d_status, float *d_affine);

/* Tracker-side post-filter, GyroAidedTracker::GyroPredictFeaturesAndOpticalFlowRefined
 * Step 3 (src/gyro_aided_tracker.cpp:289-341): thresholds from the mean pixel
 * error, final inlier mask, survivors' points copied into pt_predict(_un).
 * Host-side; returns the number of survivors (>= 0) or a negative error. */
int pagk_post_filter(int32_t n, int32_t half_patch, const uint8_t *status_pm,
                     const double *pix_err, const double *dist_pred, const float *pt_pm,
                     const float *pt_pm_un, uint8_t *status_out, float *pt_predict,
                     float *pt_predict_un);
/* The same on the device: all pointers are device pointers, asynchronous on the context stream, capturable.  Results
 * are bit-identical to pagk_post_filter on the same arrays: `sum` (:298-303) is the f64 sum of d_pix_err[i] over the
 * status-true i in index order, one rounding per add (one wavefront walks the array as an ordered lane-to-lane chain;
 * a status-false entry enters as +0.0, an identity of this running sum); avg = sum / cnt, NaN for cnt == 0, and the
 * threshold then falls back to half_patch (:305-308).  Survivors' points are copied, other entries of
 * d_pt_predict(_un) are left untouched.  d_kept (1 int32) receives what pagk_post_filter returns, d_thresholds (2
 * doubles, or NULL) th_pix and th_dist.  d_status_out may alias d_status_pm (the mask then feeds
 * pagk_geometry_validation_device in place): every read of the input status is over before the first write.
 * d_pt_pm / d_pt_predict and d_pt_pm_un / d_pt_predict_un may be NULL pairwise, as in the host function. */
int pagk_post_filter_device(pagk_ctx *ctx, int32_t n, int32_t half_patch, const uint8_t *d_status_pm,
                            const double *d_pix_err, const double *d_dist_pred, const float *d_pt_pm,
                            const float *d_pt_pm_un, uint8_t *d_status_out, float *d_pt_predict,
                            float *d_pt_predict_un, int32_t *d_kept, double *d_thresholds /* 2, or NULL */);

/* pagk_gyro_predict_device_rot with a live mask: a feature with d_live[i] == 0 takes the outcome of a prediction that
 * leaves the image (status 0, points (0,0), affine untouched); with d_live all ones the same bytes as _rot.  This is
 * what lets every launch of a frame be sized by a fixed capacity inside a graph: a dead slot reaches the tracking
 * kernels as status_in = 0 and returns at once.  (With has_gyro_predict_initial == 0 there is no prediction: pass
 * d_live as d_status_in.) */
int pagk_gyro_predict_device_live(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                                  const float *d_rot, int32_t n, const float *d_pt_ref_un, const uint8_t *d_live,
                                  float *d_pt_predict_un, float *d_pt_predict, uint8_t *d_status, float *d_affine);

/* ---- frame hand-over: the results of pair (k-1, k) become the keypoints of pair (k, k+1) ---------------------- */
/* GyroAidedTracker::SetBackToFrame (src/gyro_aided_tracker.cpp:97-111), Frame::SetPredictKeyPointsAndMask
 * (src/frame.cpp:115-153) and the top-up rule all three detectors of the reference end in (Frame::DetectKeyPoints
 * :156-218, Frame::LoadDetectedKeypointFromFile :222-281, ORBextractor.cc:1199-1203), on the device.  The detector
 * stays the application's here: it delivers a candidate list (undistorted points) in device memory (SuperPoint, a file; for
 * the reference's own two detectors see pagk_frame_handover_fast_device and pagk_frame_handover_detect_device below).  In the reference's order:
 *   survivors  for i in index order with d_status[i] != 0 (cap entries): keys[m] = pt_predict[i], keys_un[m] =
 *              pt_predict_un[i], keys_normal[m] = ((x_un - cx) * fx_inv, (y_un - cy) * fy_inv) in f32 with fx_inv =
 *              (float)(1.0 / fx) (src/frame.cpp:70, :128-129), index_in_last[m] = i  (a stable compaction).
 *   mask       width x height bytes, all 1 (:89), then for every survivor a 14 x 14 block of 0 starting at
 *              _x = min(max(0, int(x_un) - 7), width - 14), _y likewise with height (:148-151); int() truncates toward
 *              zero.  d_mask NULL: the context owns the buffer (sized by a call outside a capture).
 *   top-up     num_predicted = m.  Runs only if (num_predicted < new_point_threshold || !reach_flag) and n_new =
 *              target_n - num_predicted > 0 (:164-169).  Candidates j = 0 .. *d_n_cand - 1 (clamped to [0, cand_cap])
 *              are taken in list order; one is accepted iff mask[int(y) * width + int(x)] != 0, until n_new are accepted
 *              (:252-266).  A candidate whose truncated coordinates fall outside the image is REJECTED: the reference
 *              would read out of bounds there, so this is the library's definition.  Accepted candidates do not change
 *              the mask.  Each appends keys_un = cand, keys = DistortVecPoints(cand) (src/utils.cpp:49-76; a copy when
 *              dist_coef[0] == 0, like the tracking epilogue), keys_normal as above, index_in_last = -1.  Then
 *              reach_flag = (total == target_n) (:214); when the top-up did not run the flag keeps its value.
 *   outputs    d_live[i] = i < total for all cap entries; entries of the key arrays at and beyond total are zeroed
 *              (index_in_last: -1).  d_state, PAGK_HANDOVER_STATE_WORDS int32: [0] total (the next pair's live count),
 *              [1] reach_flag -- it persists between calls (the reference's `static bool`): zero the block once --,
 *              [2] survivors, [3] added, [4] the candidates j < *d_n_cand that fail the acceptance test (mask 0 or
 *              outside the image), counted over the whole list on every call; the rest reserved, written 0.
 * target_n = Frame::mN, new_point_threshold = mThresholdOfPredictNewKeyPoint = mN * th (:79).  cap >= target_n
 * (PAGK_E_ARG otherwise); total <= cap whenever cap >= max(target_n, previous live count).  width, height >= 14.  A call
 * with an all-zero d_status is the reference's first-frame detection (Examples/Demo/RealSenseD435i.cpp:221-235): the
 * first target_n in-image candidates.  The output key arrays must not alias the inputs (the caller ping-pongs two
 * sets).  Device pointers, asynchronous, capturable; no count is read on the host: every launch is sized by cap /
 * cand_cap.  camera model from params (fx fy cx cy dist_coef).  mvFlowVelocityInNormalPlane (:139-143) is not computed. */
#define PAGK_HANDOVER_STATE_WORDS 8
int pagk_frame_handover_device(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                               int32_t target_n, double new_point_threshold, const uint8_t *d_status,
                               const float *d_pt_predict, const float *d_pt_predict_un, int32_t cand_cap,
                               const int32_t *d_n_cand, const float *d_cand_un, float *d_keys, float *d_keys_un,
                               float *d_keys_normal /* or NULL */, int32_t *d_index_in_last, uint8_t *d_live,
                               uint8_t *d_mask /* width * height, or NULL */, int32_t *d_state);
/* The same with host buffers, synchronous (C hosts, tests).  state is read (reach_flag) and written; keys_normal and
 * mask may be NULL. */
int pagk_frame_handover(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                        int32_t target_n, double new_point_threshold, const uint8_t *status, const float *pt_predict,
                        const float *pt_predict_un, int32_t cand_cap, const int32_t *n_cand, const float *cand_un,
                        float *keys, float *keys_un, float *keys_normal, int32_t *index_in_last, uint8_t *live,
                        uint8_t *mask, int32_t *state);

/* ---- corner detection on the device: the reference's goodFeaturesToTrack call ------------------------------------- */
/* Frame::DetectKeyPoints (src/frame.cpp:156-218) tops a frame up with
 *     cv::goodFeaturesToTrack(mGray, corners_un, n_new, 0.005, 20, mMask, 3, true, 0.04)               (:181-184)
 * OpenCV's SIMD paths fix no operation order, so NO parity with OpenCV's arithmetic is claimed.  The contract is this
 * definition, bit for bit (restated in plain C in tests/corner_detect_ref.c); it follows goodFeaturesToTrack with
 * useHarrisDetector = true step by step, and says where it is the library's own choice.
 *   input      an 8-bit image W x H (level 0 of a frame slot), W, H >= 14 as for the hand-over; an optional byte mask
 *              W x H, rows W bytes apart (the hand-over's layout), NULL = all ones.
 *   gradients  3 x 3 Sobel dx, dy in integers, unscaled; pixels outside the image by reflection without repeating the
 *              edge (index -1 is 1, index W is W - 2).
 *   block sums a = sum dx*dx, b = sum dx*dy, c = sum dy*dy over the 3 x 3 block around the pixel, in integers; the
 *              product maps are indexed with the same reflection.  |dx|, |dy| <= 1020: every sum <= 9 363 600 < 2^24.
 *   response   R64 = (a*c - b*b) - k * ((a + c) * (a + c)) in f64: a*c, b*b, their difference and (a + c)^2 are exact,
 *              so R64 has exactly two roundings (the product with k, the subtraction), never contracted into an FMA;
 *              R = (float)R64.  OpenCV's scale factor is left out (library's choice: a positive constant, and every
 *              later test compares responses with each other).
 *   threshold  Rmax = the largest R over the pixels with mask != 0, the outer ring included.  No unmasked pixel, or
 *              Rmax <= 0: no corners.  A pixel passes if (double)R > quality_level * (double)Rmax.
 *   non-max    only 1 <= x <= W - 2, 1 <= y <= H - 2 with mask != 0 can be corners.  The pixel must be >= its four
 *              neighbours that come earlier in raster order (NW, N, NE, W) and > the four that come later; the
 *              neighbours' responses count whatever their mask says.  This tie rule is the library's own (OpenCV keeps
 *              both pixels of an exact tie and lets the minimum distance drop one).  At most one pixel of any 2 x 2
 *              block survives: never more than ceil((W-2)/2) * ceil((H-2)/2) raw candidates.
 *   order      descending by the 64-bit key (bits(R) << 32) | (y * W + x); R > 0 here, so its bits order like its value;
 *              a tie goes to the higher pixel index, in agreement with the non-maximum rule.
 *   distance   the candidates are walked in that order; one is accepted unless an already accepted corner lies at
 *              (double)(ddx*ddx + ddy*ddy) < min_distance * min_distance, in integer pixel coordinates; the walk stops
 *              once max_corners are accepted.  min_distance < 1 switches the test off.
 *   output     the accepted corners as (float)x, (float)y in acceptance order, and their number; entries beyond the
 *              number are zeroed.  No sub-pixel step (goodFeaturesToTrack has none either).
 *   overflow   the caller sizes the raw-candidate buffer (raw_cap).  If more raw candidates exist than fit, which of
 *              them were stored is a matter of timing: the call then returns NO corners and sets the overflow word, never
 *              a result that depends on timing.  raw_cap = 0: the context owns a buffer of the bound above (sized by a
 *              call outside a capture, like d_mask == NULL in the hand-over).
 * Block size 3 and aperture 3 are fixed; cornerMinEigenVal (useHarrisDetector = false) is not provided.  This is the `else`
 * branch of Frame::DetectKeyPoints; the branch the shipped front-ends take (ORBextractor) is pagk_detect_fast_device below.
 * quality_level, min_distance >= 0 and finite, harris_k finite, raw_cap >= 0 (PAGK_E_ARG otherwise).
 * info, PAGK_DETECT_INFO_WORDS int32: [0] corners returned, [1] raw candidates found (the true number, also on
 * overflow), [2] overflow, [3] the bits of Rmax (0 if there is none or Rmax <= 0), [4] the candidates the distance walk
 * visited (the index of the last accepted one + 1 when it stopped at the limit), the rest 0. */
typedef struct pagk_detect_params {
    double quality_level; /* qualityLevel  0.005 (src/frame.cpp:183) */
    double min_distance;  /* minDistance   20                         */
    double harris_k;      /* k             0.04  (:184)               */
    int32_t raw_cap;      /* raw-candidate buffer; 0 = the bound, owned by the context */
} pagk_detect_params;
#define PAGK_DETECT_INFO_WORDS 8
/* 0.005, 20, 0.04, 0: the arguments at src/frame.cpp:181-184 */
void pagk_detect_params_default(pagk_detect_params *p);
/* Frame::DetectKeyPoints' detector call (src/frame.cpp:156-218, the call at :181-184) on level 0 of frame slot `slot`
 * (pagk_frame_set_device, its batch form and pagk_track_device_fused read the caller's image in place: detection on a slot
 * is defined only until the caller rewrites the buffer the slot was set from, not merely until the slot is set again --
 * a loop that feeds every frame through one buffer can detect on the slot of the current frame only).  d_mask: W * H bytes or NULL.
 * d_corners: cap x 2 float, d_info: PAGK_DETECT_INFO_WORDS int32.  The effective limit is min(cap, max(0,
 * *d_max_corners)); d_max_corners NULL = cap.  Device pointers, asynchronous on the context stream, capturable; no count
 * is read on the host: every launch is sized by W, H, raw_cap and cap.  Run it once outside a capture first (workspace). */
int pagk_detect_corners_device(pagk_ctx *ctx, const pagk_detect_params *det, int32_t slot, const uint8_t *d_mask,
                               int32_t cap, const int32_t *d_max_corners, float *d_corners, int32_t *d_info);
/* The same with host buffers, synchronous (src/frame.cpp:156-218): corners holds max_corners x 2 floats, mask (or NULL)
 * img->width * img->height bytes, info (or NULL) PAGK_DETECT_INFO_WORDS words.  max_corners >= 0. */
int pagk_detect_corners(pagk_ctx *ctx, const pagk_detect_params *det, const pagk_image *img, const uint8_t *mask,
                        int32_t max_corners, float *corners, int32_t *info);
/* pagk_frame_handover_device with the reference's own detector as the source of the candidates (Frame::DetectKeyPoints,
 * src/frame.cpp:156-218, in one call): its result is BY DEFINITION what pagk_frame_handover_device returns when the
 * candidate list is detect(level 0 of `slot`, the mask this call builds, max_corners = n_new) -- the mask of THIS frame,
 * as the reference passes it (:158, :184), not last frame's.  `slot` is the frame just tracked INTO (the current image).
 * The list is empty when the top-up does not run (:164-169): the detector's kernels then return early on a device-side
 * flag and d_info is all zero.  State words [0]-[4] keep their meaning; [4] is 0 by construction (a detected corner lies
 * on an unmasked pixel of the image).  A call with an all-zero d_status detects the first frame's target_n keypoints.
 * d_info: PAGK_DETECT_INFO_WORDS int32.  Otherwise the arguments and rules of pagk_frame_handover_device. */
int pagk_frame_handover_detect_device(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                                      int32_t cap, int32_t target_n, double new_point_threshold, const uint8_t *d_status,
                                      const float *d_pt_predict, const float *d_pt_predict_un,
                                      const pagk_detect_params *det, int32_t slot, float *d_keys, float *d_keys_un,
                                      float *d_keys_normal /* or NULL */, int32_t *d_index_in_last, uint8_t *d_live,
                                      uint8_t *d_mask /* width * height, or NULL */, int32_t *d_state, int32_t *d_info);
/* The same with host buffers, synchronous (src/frame.cpp:156-218); the current image comes as a pagk_image of
 * width x height.  state is read (reach_flag) and written; keys_normal, mask and info may be NULL. */
int pagk_frame_handover_detect(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                               int32_t target_n, double new_point_threshold, const uint8_t *status,
                               const float *pt_predict, const float *pt_predict_un, const pagk_detect_params *det,
                               const pagk_image *img, float *keys, float *keys_un, float *keys_normal,
                               int32_t *index_in_last, uint8_t *live, uint8_t *mask, int32_t *state, int32_t *info);
/* Diagnostic: the response map R alone (img->width * img->height floats, harris_k = 0.04), host buffers: localises a
 * mismatch to the first stage of the detector (src/frame.cpp:156-218 has no counterpart: OpenCV keeps the map inside). */
int pagk_selftest_corner_response(pagk_ctx *ctx, const pagk_image *img, float *R);

/* ---- the detector the reference's front-ends run: FAST in cells, then the quadtree ---------------------------------- */
/* Both shipped front-ends construct an ORBextractor(nFeatures, 1.2, nLevels = 1, iniThFAST = 20, minThFAST = 7)
 * (Examples/Demo/RealSenseD435i.cpp:184-190, Examples/ROS/.../feature_tracker.cpp:367-371), so Frame::DetectKeyPoints
 * (src/frame.cpp:156-218) takes its first branch, pORBextractor->DetectFeatures(mGray, mMask, keypoints) (:172-179):
 * ORBextractor::DetectFeatures (src/ORBextractor.cc:1148-1205), ComputeKeyPointsOctTree (:789-871), DistributeOctTree
 * (:563-787), ExtractorNode::DivideNode (:505-561).  This section is that branch for nlevels = 1.  What is pinned: every
 * statement of the reference this section reads -- the cell arithmetic, both skips, the fall-back pass, DistributeOctTree and
 * DivideNode -- against the reference's own src/ORBextractor.cc, compiled unchanged (oracle/_ref/ref_orb, oracle/README.md),
 * through the plain-C restatement tests/fast_detect_ref.c and on the device, bit for bit.  What remains a definition: cv::FAST
 * itself (m(p), the score, the suppression below; it cannot be built here, is integer arithmetic throughout, and a host with
 * OpenCV can pin it), and the order of nodes of equal size in the sort of :708, which the reference takes from their addresses
 * (the "creation number" rule below is that order under an allocator whose addresses ascend).  More than one
 * level is "ORB over a scale pyramid" below (pagk_orb_extractor); computeOrientation / IC_Angle (DetectKeyPoints reads key.pt only) and the
 * descriptors are pagk_orb_describe_device below ("ORB descriptors and matching").
 *   input      an 8-bit image W x H (level 0 of a frame slot, read through its pitch).  At level 0 without orientation
 *              every FAST window lies inside the image: the border image of ComputePyramid is never read.  EDGE_THRESHOLD
 *              = 19: minBorder = 16, maxBorderX = W - 16, maxBorderY = H - 16.
 *   cells      (:805-830) width = maxBorderX - 16, height = maxBorderY - 16 as floats; nCols = int(width / 30), nRows =
 *              int(height / 30); wCell = ceil(width / nCols), hCell = ceil(height / nRows).  Cell (i, j) is the sub-image
 *              rows [iniY, maxY) x columns [iniX, maxX): iniY = 16 + i * hCell, maxY = min(iniY + hCell + 6, maxBorderY),
 *              the row is skipped if iniY >= maxBorderY - 3; iniX = 16 + j * wCell, maxX = min(iniX + wCell + 6,
 *              maxBorderX), the cell is skipped if iniX >= maxBorderX - 6 (3 for rows, 6 for columns: the reference's).
 *              62 <= W, H <= 32767 and nIni >= 1 (below): PAGK_E_ARG otherwise -- the reference divides by zero there; the
 *              upper limit is the library's own (16-bit key coordinates).
 *   FAST-9/16  the ring is the 16 offsets of the Bresenham circle of radius 3 (OpenCV's order from (0, 3); only the cyclic
 *              order matters).  For a pixel p whose ring lies inside the cell's sub-image (local x in [3, w - 3), y in
 *              [3, h - 3)): m(p) = the maximum, over the 16 arcs of 9 consecutive ring pixels and both polarities, of the
 *              minimum over the arc of ring - centre (or centre - ring).  p is a corner at threshold t iff m(p) > t; its
 *              score is m(p) - 1, the largest t at which it still is one (cv::FAST's response).  S_t(p) = m(p) - 1 for a
 *              corner at t, 0 otherwise and 0 outside the detection region of the CELL.
 *   non-max    p is kept iff S_t(p) > S_t of all eight neighbours, strictly: both pixels of a tie go.  A neighbouring
 *              cell's scores are not seen (FAST on a sub-matrix).  At most one pixel of any 2 x 2 block is kept: a cell
 *              yields at most ceil(wCell / 2) * ceil(hCell / 2) keypoints, and has a fixed segment of that size.
 *   fall-back  pass 1 uses t = ini_threshold; a cell that keeps NO keypoint runs pass 2 with t = min_threshold (:833-840).
 *              A cell's keypoints come from exactly one pass.
 *   raw list   cells in loop order (i outer, j inner), raster order inside a cell; coordinates (x_local + j * wCell,
 *              y_local + i * hCell) as floats relative to minBorder (:846-847).
 *   target     N = n_features (mnFeaturesPerLevel[0] = nfeatures for one level, :459-470).  The tree distributes over the
 *              whole image and does not see the mask; the mask is applied after it (the reference's order: it changes
 *              which points are returned).
 *   quadtree   (:563-787) nIni = round((float)(maxX - minX) / (maxY - minY)), half away from zero; hX = (float)(maxX -
 *              minX) / nIni; initial node i spans x in [int(hX * i), int(hX * (i + 1))); a key goes to node int(pt.x /
 *              hX).  Empty nodes are erased; a node with one key is final.  An outer round walks the list front to back
 *              and splits every node that is not final (DivideNode: half sizes ceil(float(extent) / 2), child test x <
 *              n1.UR.x, y < n1.BR.y, keys keep their order inside a child); the non-empty children are pushed to the
 *              FRONT in the order n1, n2, n3, n4 and the parent is erased.  After a round: finished if size >= N or size
 *              == prevSize; otherwise, if size + 3 * nToExpand > N (nToExpand: children of the round with more than one
 *              key), the inner loop takes over: the children of the previous pass that have more than one key are sorted
 *              ascending and walked from the back, each split the same way, and the walk BREAKS as soon as size >= N;
 *              then the same finish test.
 *   tie rule   the reference sorts pair<int, ExtractorNode*>: nodes of equal size are ordered by heap address, the one
 *              place where it is not a function of its input.  The library's rule: every node gets a creation number when
 *              it is pushed into the list (initial nodes in order, then children in push order); the sort key is (size,
 *              creation number).
 *   result     one keypoint per node in list order, front to back: the key with the largest response, the first one on a
 *              tie (:768-784).  The list can be longer than N: at most max(N + 2, 4 * nIni) nodes (a full round runs
 *              only while size + 3 * nToExpand <= N, except the first, which starts from at most nIni nodes; the inner
 *              loop adds at most 3 per split before its break).  minBorder is added to both coordinates (:866-867), then
 *              every keypoint with mask[int(y) * W + int(x)] == 0 is dropped (:1199-1203; mask NULL = all ones) and the
 *              rest goes out in list order as (float x, float y) plus, optionally, the response; entries beyond the count
 *              are zeroed.  The trimming to n_new is the hand-over's (src/frame.cpp:176-179), not the detector's.
 * info, PAGK_DETECT_INFO_WORDS int32: [0] keypoints returned, [1] raw FAST keypoints, [2] cells whose first pass was empty,
 * [3] cells empty after both passes, [4] nodes at the end (the count before the mask), [5] splitting passes run (outer
 * rounds plus inner passes; 1 for an image without keypoints), the rest 0 ([7] would be -1, with no keypoints returned, if a
 * list ever outgrew the bound above: the kernel then stops instead of writing past a buffer). */
typedef struct pagk_fast_params {
    int32_t ini_threshold; /* iniThFAST 20 */
    int32_t min_threshold; /* minThFAST 7  */
    int32_t n_features;    /* nfeatures; 0 = the call's target_n (fused form), PAGK_E_ARG in the stand-alone forms */
    int32_t n_levels;      /* nlevels: must be 1 (PAGK_E_UNSUPPORTED otherwise) */
} pagk_fast_params;
/* 20, 7, 0, 1: the constructor arguments of both front-ends that src/ORBextractor.cc:1148-1205 runs with */
void pagk_fast_params_default(pagk_fast_params *p);
/* PAGK_OK if *p can be run by the entry points below (src/ORBextractor.cc:1148-1205 with one level): thresholds in
 * [0, 255], n_features >= 0 (PAGK_E_ARG otherwise), n_levels == 1 (PAGK_E_UNSUPPORTED otherwise).  Needs no device. */
int pagk_fast_params_check(const pagk_fast_params *p);
/* The sizes a caller needs for src/ORBextractor.cc:1148-1205 on a width x height image with n_features >= 1: *raw_bound =
 * nRows * nCols * ceil(wCell / 2) * ceil(hCell / 2) raw keypoints at most, *out_bound = max(n_features + 2, 4 * nIni)
 * keypoints returned at most.  PAGK_E_ARG for a size the definition excludes.  Needs no device; either pointer may be NULL. */
int pagk_detect_fast_bounds(int32_t width, int32_t height, int32_t n_features, int32_t *raw_bound, int32_t *out_bound);
/* ORBextractor::DetectFeatures (src/ORBextractor.cc:1148-1205) on level 0 of frame slot `slot` (for how long a slot can
 * be detected on see pagk_detect_corners_device).  d_mask: W * H bytes or NULL.  d_keypoints: cap x 2 float, d_response:
 * cap float or NULL, d_info: PAGK_DETECT_INFO_WORDS int32.  cap >= out_bound (PAGK_E_ARG otherwise).  Device pointers,
 * asynchronous on the context stream, capturable; no count is read on the host: every launch is sized by W, H and the
 * bounds.  Run it once outside a capture first (workspace). */
int pagk_detect_fast_device(pagk_ctx *ctx, const pagk_fast_params *params, int32_t slot, const uint8_t *d_mask, int32_t cap,
                            float *d_keypoints, float *d_response /* or NULL */, int32_t *d_info);
/* The same with host buffers, synchronous (src/ORBextractor.cc:1148-1205): keypoints holds cap x 2 floats, response (or
 * NULL) cap floats, mask (or NULL) img->width * img->height bytes, info (or NULL) PAGK_DETECT_INFO_WORDS words. */
int pagk_detect_fast(pagk_ctx *ctx, const pagk_fast_params *params, const pagk_image *img, const uint8_t *mask, int32_t cap,
                     float *keypoints, float *response, int32_t *info);
/* pagk_frame_handover_device with src/ORBextractor.cc:1148-1205 as the source of the candidates (the first branch of
 * Frame::DetectKeyPoints, src/frame.cpp:172-179, in one call): its result is BY DEFINITION what pagk_frame_handover_device
 * returns when the candidate list is the detector's output on level 0 of `slot` with NO mask, N = fast->n_features (0:
 * target_n), cand_cap = out_bound and *d_n_cand = the detector's count.  The hand-over's own acceptance test, against the
 * mask this call builds, is the reference's mask test (:1199-1203), and its "first n_new accepted" is src/frame.cpp:176-179.
 * State word [4] is meaningful here: the candidates the mask rejects.  When the top-up does not run (:164-169) the
 * detector's kernels return early on a device-side flag and d_info is all zero.  d_info: PAGK_DETECT_INFO_WORDS int32.
 * Otherwise the arguments and rules of pagk_frame_handover_detect_device. */
int pagk_frame_handover_fast_device(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                                    int32_t target_n, double new_point_threshold, const uint8_t *d_status,
                                    const float *d_pt_predict, const float *d_pt_predict_un, const pagk_fast_params *fast,
                                    int32_t slot, float *d_keys, float *d_keys_un, float *d_keys_normal /* or NULL */,
                                    int32_t *d_index_in_last, uint8_t *d_live, uint8_t *d_mask /* width * height, or NULL */,
                                    int32_t *d_state, int32_t *d_info);
/* The same with host buffers, synchronous (src/ORBextractor.cc:1148-1205 inside src/frame.cpp:156-218); the current image
 * comes as a pagk_image of width x height.  state is read (reach_flag) and written; keys_normal, mask and info may be NULL. */
int pagk_frame_handover_fast(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                             int32_t target_n, double new_point_threshold, const uint8_t *status, const float *pt_predict,
                             const float *pt_predict_un, const pagk_fast_params *fast, const pagk_image *img, float *keys,
                             float *keys_un, float *keys_normal, int32_t *index_in_last, uint8_t *live, uint8_t *mask,
                             int32_t *state, int32_t *info);
/* Diagnostic: the raw list alone (the FAST stage of src/ORBextractor.cc:1148-1205, before the tree), in its defined order,
 * host buffers: raw_xy raw_bound x 2 floats relative to minBorder, raw_score raw_bound int32, *n the count.  Localises a
 * mismatch to FAST or to the tree.  n_features is not read. */
int pagk_selftest_fast_cells(pagk_ctx *ctx, const pagk_fast_params *params, const pagk_image *img, float *raw_xy,
                             int32_t *raw_score, int32_t *n);

/* ---- rectification: a raw camera frame into a frame slot ------------------------------------------------------------ */
/* Both front-ends of the reference rectify every frame with
 *     cv::remap(image_cur_distort, image_cur, M1, M2, cv::INTER_LINEAR)
 * (Examples/Demo/RealSenseD435i.cpp:202, Examples/ROS/.../feature_tracker.cpp:137; M1, M2 = the CV_32F planes of
 * cv::initUndistortRectifyMap, include/imu_types.h:60-65) and Frame::Frame turns a 3- or 4-channel image into mGray
 * (src/frame.cpp:81-87).  These entry points do both on the device, in one pass.
 * Parity contract: OpenCV is third-party and its SIMD paths are not restated here, so parity with OpenCV's bytes is NOT
 * pinned.  The contract is this definition, bit for bit (restated in plain C in tests/rectify_ref.c).  It follows OpenCV
 * 3.4's remap for 8-bit images, INTER_LINEAR, planar CV_32FC1 maps, BORDER_CONSTANT with value 0, and its 8-bit RGB2GRAY,
 * step by step, and says where it is the library's own rule.  After one exact float step everything is integer arithmetic.
 * For destination pixel (r, c) of a W x H map pair and a source of Ws x Hs pixels with cn interleaved channels:
 *   fixed point  sx = rne(map_x[r][c] * 32), sy = rne(map_y[r][c] * 32): the float product is exact (a power of two), rne
 *                is round to nearest, ties to even (cvRound).
 *   split        ix = sat_i16(sx >> 5), fx = sx & 31, likewise iy, fy: the shift is arithmetic and the mask acts on the
 *                two's-complement value, so negative coordinates floor (-0.25 is ix = -1, fx = 24).
 *   taps         (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1); a tap outside [0, Ws) x [0, Hs) is 0.
 *   interpolate  per channel v = (p00 (32-fx)(32-fy) + p01 fx (32-fy) + p10 (32-fx) fy + p11 fx fy + 512) >> 10.  This is
 *                OpenCV's table form (sum of p * w * 32 + (1 << 14)) >> 15 with w the four products above; the one weight
 *                OpenCV saturates to 16 bits (32768 -> 32767, at fx = fy = 0) gives the same byte for every p <= 255
 *                ((p * 32767 + 16384) >> 15 = p), so the two forms agree on every input.
 *   no pixel     a non-finite map value, or one with |map * 32| >= 2^31, gives pixel 0 (the library's own rule: cvRound
 *                of such a value is undefined).
 *   limits       Ws, Hs <= 32767 (16-bit tap coordinates); larger: PAGK_E_ARG.
 *   gray         cn == 1: the byte is v.  cn == 3 or 4: the remap runs first, per channel, and the conversion follows it,
 *                as in the reference: gray = (v0 w0 + v1 w1 + v2 w2 + (1 << (shift - 1))) >> shift; channel 3 is ignored.
 * pagk_rectify_params carries the last step.  The defaults are 4899, 9617, 1868 and 14: CV_RGB2GRAY on channel order R, G,
 * B in OpenCV 3.4 (a BGR frame passes them reversed).  A host built against another OpenCV passes its own weights -- the
 * same idea as pagk_params::solver_variant.  For channels 3 and 4 the weights must be non-negative and sum to 1 << shift
 * with 1 <= shift <= 15 (the gray byte then never exceeds 255); channels == 1 does not read them.  Others: PAGK_E_ARG. */
typedef struct pagk_rectify_params {
    int32_t channels;       /* cn: 1, 3 or 4 interleaved bytes per source pixel */
    int32_t gray_weight[3]; /* w0 w1 w2, applied to channels 0 1 2              */
    int32_t gray_shift;     /* shift                                            */
} pagk_rectify_params;
/* channels 1; 4899, 9617, 1868; 14 */
void pagk_rectify_params_default(pagk_rectify_params *p);
/* PAGK_OK if the rules above hold for *p, PAGK_E_ARG otherwise (needs no device). */
int pagk_rectify_params_check(const pagk_rectify_params *p);
/* The maps: host pointers to two float planes of width x height, rows step_bytes apart (M1, M2 of the reference, or the
 * planes pagk_undistort_maps fills).  Converted ONCE into a packed entry per pixel (ix, iy, fx, fy: 8 bytes) in device
 * memory the context owns.  Synchronous; PAGK_E_ARG inside a capture.  Maps of another size can only be set while no
 * graph of the context is alive (its nodes hold the old pointer). */
int pagk_rectify_set_maps(pagk_ctx *ctx, const float *map_x, const float *map_y, int32_t width, int32_t height,
                          int64_t step_bytes);
/* The raw frame d_raw (DEVICE memory: src_height rows of src_step bytes, src_width pixels of params->channels bytes)
 * is rectified into frame slot `slot`, then the slot's pyramid is built as pagk_frame_upload builds it.  The rectified
 * image goes into the slot's own level-0 buffer: from then on the slot cannot be told from one filled by pagk_frame_upload
 * of the rectified image (a continuous image of the maps' size), and -- unlike a slot set with pagk_frame_set_device -- it
 * does not depend on the caller's buffer any longer, so pagk_detect_corners_device may run on it at any time.
 * Asynchronous on the context stream, capturable (run the same call once before capturing).  PAGK_E_ARG, with a text in
 * pagk_last_error: no maps set; the slot holds a frame of another size than the maps; channels not 1, 3 or 4 (or bad
 * weights); src_step < src_width * channels; a source dimension beyond 32767. */
int pagk_frame_rectify_device(pagk_ctx *ctx, int32_t slot, const pagk_rectify_params *params, const void *d_raw,
                              int32_t src_width, int32_t src_height, int64_t src_step, int32_t pyramids);
/* The same for a raw frame in PINNED host memory (a camera ring buffer): it is copied into a staging buffer the context
 * owns (sized by a call outside a capture), then rectified.  Asynchronous and capturable like pagk_frame_upload_pinned. */
int pagk_frame_rectify_pinned(pagk_ctx *ctx, int32_t slot, const pagk_rectify_params *params, const void *raw,
                              int32_t src_width, int32_t src_height, int64_t src_step, int32_t pyramids);
/* Host buffers, synchronous: the rectified gray image (the maps' size, rows dst_step bytes apart) into dst. */
int pagk_rectify(pagk_ctx *ctx, const pagk_rectify_params *params, const void *raw, int32_t src_width, int32_t src_height,
                 int64_t src_step, uint8_t *dst, int64_t dst_step);
/* Host helper, run once: the maps of cv::initUndistortRectifyMap(K, dist, R = I, newK, size, CV_32FC1) for the Brown-Conrady
 * model (dist_coef = k1 k2 p1 p2 [k3], n_dist_coef 0, 4 or 5).  This is the library's OWN definition -- an application
 * with OpenCV passes its M1 / M2 to pagk_rectify_set_maps --: a closed form per pixel in f64 (OpenCV walks running sums),
 * one rounding per operation, in this order, for pixel (r, c):
 *   x = (c - new_cx) / new_fx, y = (r - new_cy) / new_fy, x2 = x x, y2 = y y, r2 = x2 + y2, xy2 = (2 x) y,
 *   kr = 1 + ((k3 r2 + k2) r2 + k1) r2, xd = (x kr + p1 xy2) + p2 (r2 + 2 x2), yd = (y kr + p1 (r2 + 2 y2)) + p2 xy2,
 *   map_x = (float)(fx xd + cx), map_y = (float)(fy yd + cy).
 * map_x, map_y: width * height floats each, dense.  No device needed. */
int pagk_undistort_maps(double fx, double fy, double cx, double cy, const double *dist_coef, int32_t n_dist_coef,
                        double new_fx, double new_fy, double new_cx, double new_cy, int32_t width, int32_t height,
                        float *map_x, float *map_y);

/* ---- ORB descriptors and matching: the comparison arm of the reference's front-ends, one level ---------------------- */
/* Both front-ends run ORBDetectAndDespMatcher::FindFeatureMatches (src/ORBDetectAndDespMatcher.cpp:55-91) on every frame
 * pair (Examples/Demo/RealSenseD435i.cpp:282, Examples/ROS/.../feature_tracker.cpp:272): ORBextractor::operator() on both
 * images -- ComputeKeyPointsOctTree, computeOrientation / IC_Angle (src/ORBextractor.cc:101-128, 496-503), a 7 x 7 Gaussian
 * blur and the steered rBRIEF descriptors (:131-171, 1057-1064, 1113-1130) --, then BruteForce-Hamming matching and a
 * distance filter.  The detector half is pagk_detect_fast_device with mask = NULL (ComputeKeyPointsOctTree for the one
 * level the front-ends construct); this section is the describe and the match half, for nlevels = 1 (more
 * levels: "ORB over a scale pyramid" below, which runs this section's definition on every level).
 * Parity contract: IC_Angle and computeOrbDescriptor (:101-171) are pinned to the reference's own src/ORBextractor.cc,
 * compiled unchanged (oracle/_ref/ref_orb, oracle/README.md), through the plain-C restatement tests/orb_ref.c and on the
 * device, bit for bit.  OpenCV's own arithmetic under them (GaussianBlur, fastAtan2, cvRound), the sine and cosine of a
 * float, and BFMatcher remain this definition (they cannot be built here); it follows OpenCV 3.4's scalar code paths step by
 * step and says where it is the library's own rule.  The matcher and its filter (FindFeatureMatches) are not pinned.
 *   pattern    the 512 sampling points of bit_pattern_31_ (:174) are the host's: 1024 int32, x then y per point, pair q of
 *              the descriptor = points 2q and 2q + 1.  Every coordinate lies in [-13, 13] (the reference's table spans
 *              [-13, 12], largest radius 18.38): every rotated tap then rounds to at most 18 < EDGE_THRESHOLD = 19.
 *   blur       (:1123-1124) a separable 7-tap kernel in Q8, w[0..3] for offsets 0, +-1, +-2, +-3, w >= 0 and
 *              w0 + 2 (w1 + w2 + w3) == 256.  Border index r(i) = -i below 0 and 2 (n - 1) - i at or above n
 *              (BORDER_REFLECT_101); 4 <= W, H <= 32767.  Horizontal pass, exact integers: Hx = sum_k w[|k|] src[y][r(x + k)]
 *              (at most 65280); vertical pass: out = (sum_k w[|k|] Hx[r(y + k)][x] + 32768) >> 16, never above 255.  The
 *              defaults 54, 49, 34, 18 are exp(-k^2 / 8) normalised, times 256 (55.32, 48.82, 33.56, 17.96), rounded to
 *              nearest with the centre absorbing the remainder: the library's own fixed-point kernel, not OpenCV's.
 *   centre     cx = rintf(x), cy = rintf(y), ties to even (cvRound).  A keypoint with cx outside [19, W - 19) or cy outside
 *              [19, H - 19) (a NaN included) gets an all-zero descriptor and angle -1 and is counted in info[1]: the
 *              reference would read out of bounds there.
 *   angle      (:101-128) on the UNBLURRED image: m10 = sum u I(cx + u, cy + v), m01 = sum v I(cx + u, cy + v) in int32
 *              over the disc |v| <= 15, |u| <= umax[|v|], umax = 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3 (what :478-493
 *              evaluates to; 749 pixels).  angle = fastAtan2((float)m01, (float)m10) in degrees, OpenCV's scalar polynomial
 *              restated in f32 with one rounding per operation: ax = |x|, ay = |y|; if ax >= ay: c = ay / (ax + e),
 *              a = (((p7 c2 + p5) c2 + p3) c2 + p1) c with c2 = c c; else c = ax / (ay + e), a = 90 - that polynomial;
 *              x < 0: a = 180 - a; then y < 0: a = 360 - a.  e = (float)DBL_EPSILON = 0x1p-52f; the coefficients are
 *              OpenCV's times (float)(180 / pi) in f32: p1 = 0x1.ca44dep+5f (57.283627), p3 = -0x1.2aaddcp+4f (-18.667446),
 *              p5 = 0x1.1d3f7ep+3f (8.9140005), p7 = -0x1.4515b2p+1f (-2.5397246).  fastAtan2(0, 0) = 0.
 *   steering   (:136-137) r = angle * 0x1.1df46ap-6f in f32 ((float)(CV_PI / 180.f)); a = (float)cos(r), b = (float)sin(r)
 *              with the f64 cosine and sine computed by THIS algorithm on both sides (not by a library's cos / sin, which
 *              differ in the last place so that a tap could flip); only f64 + - * and comparisons, absolute error <= 2^-45:
 *                x = (double)r; k = (int)(x * 0x1.45f306dc9c883p-1 + 0.5); t = (x - k * 0x1.921fb544p+0)
 *                - k * 0x1.0b4611a626331p-34 (Cody-Waite by pi / 2 in two parts: the first product is exact); z = t t;
 *                s = t + t (z (S1 + z (S2 + z (S3 + z (S4 + z (S5 + z S6)))))),
 *                c = 1 - z (0.5 - z (C1 + z (C2 + z (C3 + z (C4 + z (C5 + z C6)))))) with
 *                S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
 *                S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10,
 *                C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
 *                C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
 *                (cos, sin) = (c, s), (-s, c), (-c, -s), (s, -c) for k & 3 = 0, 1, 2, 3.
 *   descriptor (:139-168) on the BLURRED image: tap of point (px, py) at row cy + rintf(px b + py a), column
 *              cx + rintf(px a - py b), f32 arithmetic with one rounding per operation (no contraction).  Bit j of byte i is
 *              tap(point 16 i + 2 j) < tap(point 16 i + 2 j + 1), strictly.
 *   match      (src/ORBDetectAndDespMatcher.cpp:61-65; BruteForce-Hamming, no cross-check) for each query row q < nq the
 *              train row with the smallest popcount of the 256-bit XOR; on a tie the LOWEST index (the library's stated
 *              rule).  nt == 0: no matches; every row gets train_idx -1, distance 257, keep 0.
 *   filter     (:67-81) min_dist, max_dist over all matches; threshold = max(2 min_dist, match_floor); keep[q] =
 *              distance[q] <= threshold.  Without a match (nq == 0 or nt == 0): min_dist = max_dist = 0, threshold =
 *              match_floor (the library's rule: the reference's 10000 / 0 start values are never used there).
 * Describe info, PAGK_ORB_INFO_WORDS int32: [0] keypoints described, [1] keypoints outside the border, the rest 0.
 * Match info: [0] nq, [1] matches, [2] kept (the three counts the reference logs per frame, :84-89), [3] min_dist,
 * [4] max_dist, [5] threshold, the rest 0. */
typedef struct pagk_orb_params {
    int32_t blur_weights[4]; /* Q8 taps for offsets 0, +-1, +-2, +-3: 54 49 34 18 (a host that has pinned OpenCV's passes its own) */
    int32_t match_floor;     /* experiment_value 30 (src/ORBDetectAndDespMatcher.cpp:76); 0 .. 256 */
    int32_t n_levels;        /* nlevels: must be 1 (PAGK_E_UNSUPPORTED otherwise) */
} pagk_orb_params;
#define PAGK_ORB_INFO_WORDS 8
#define PAGK_ORB_MAX_ROWS 1048576
/* 54, 49, 34, 18; 30; 1: the blur of src/ORBextractor.cc:1123-1124 in the library's fixed point and experiment_value of
 * src/ORBDetectAndDespMatcher.cpp:76 */
void pagk_orb_params_default(pagk_orb_params *p);
/* PAGK_OK if *p can be run by the entry points below (src/ORBextractor.cc:1113-1130 with one level): weights >= 0 with
 * w0 + 2 (w1 + w2 + w3) == 256, 0 <= match_floor <= 256 (PAGK_E_ARG otherwise), n_levels == 1 (PAGK_E_UNSUPPORTED
 * otherwise).  Needs no device. */
int pagk_orb_params_check(const pagk_orb_params *p);
/* PAGK_OK if every one of the 1024 coordinates of a sampling pattern (bit_pattern_31_, src/ORBextractor.cc:174) lies in
 * [-13, 13], PAGK_E_ARG otherwise or for NULL.  Needs no device. */
int pagk_orb_pattern_check(const int32_t pattern[1024]);
/* The sampling pattern (src/ORBextractor.cc:174, copied into `pattern` by the constructor, :442-445): a host pointer to
 * 1024 int32, uploaded ONCE into device memory the context owns, as pagk_rectify_set_maps does with M1 / M2.  The table
 * itself is the reference's and is not part of this library: INTEGRATION.md section 11 has the one line a host built against
 * the reference writes.  Synchronous; PAGK_E_ARG inside a capture or for a pattern pagk_orb_pattern_check refuses. */
int pagk_orb_set_pattern(pagk_ctx *ctx, const int32_t pattern[1024]);
/* computeOrientation and computeDescriptors of ORBextractor::operator() (src/ORBextractor.cc:101-171, 1113-1130) for the
 * keypoints of level 0 of frame slot `slot`, read through its pitch (for how long a slot can be read see
 * pagk_detect_corners_device).  d_keypoints: cap x 2 float and d_n: a device count (clamped to [0, cap]) -- the layout
 * pagk_detect_fast_device writes (its d_keypoints and d_info).  d_angle: cap float or NULL, d_desc: cap x 32 bytes on a
 * 16-byte boundary, d_info: PAGK_ORB_INFO_WORDS int32.  Rows at or beyond the count are zeroed.  1 <= cap <=
 * PAGK_ORB_MAX_ROWS.  Device pointers, asynchronous on the context stream, capturable; no count is read on the host.  Run
 * it once outside a capture first (the blurred image is a buffer of the context).  PAGK_E_ARG without a pattern. */
int pagk_orb_describe_device(pagk_ctx *ctx, const pagk_orb_params *params, int32_t slot, int32_t cap,
                             const float *d_keypoints, const int32_t *d_n, float *d_angle /* or NULL */, uint8_t *d_desc,
                             int32_t *d_info);
/* The same with host buffers, synchronous (src/ORBextractor.cc:101-171, 1113-1130): keypoints n x 2 floats, angle (or
 * NULL) n floats, desc n x 32 bytes, info (or NULL) PAGK_ORB_INFO_WORDS words.  0 <= n <= PAGK_ORB_MAX_ROWS. */
int pagk_orb_describe(pagk_ctx *ctx, const pagk_orb_params *params, const pagk_image *img, int32_t n,
                      const float *keypoints, float *angle, uint8_t *desc, int32_t *info);
/* matcher->match and the distance filter of FindFeatureMatches (src/ORBDetectAndDespMatcher.cpp:61-81).  d_desc_q: cap_q x
 * 32 bytes, d_desc_t: cap_t x 32 bytes, both on a 16-byte boundary; d_nq, d_nt: device counts (clamped to [0, cap]);
 * d_train_idx, d_distance: cap_q int32 each, d_keep: cap_q bytes, d_info: PAGK_ORB_INFO_WORDS int32.  Rows at or beyond nq
 * get -1 / 257 / 0.  1 <= cap_q, cap_t <= PAGK_ORB_MAX_ROWS.  The result does not depend on the order in which the
 * workgroups run.  Device pointers, asynchronous on the context stream, capturable; nothing is read on the host.  Run it
 * once outside a capture first (the match keys are a buffer of the context). */
int pagk_orb_match_device(pagk_ctx *ctx, const pagk_orb_params *params, int32_t cap_q, const uint8_t *d_desc_q,
                          const int32_t *d_nq, int32_t cap_t, const uint8_t *d_desc_t, const int32_t *d_nt,
                          int32_t *d_train_idx, int32_t *d_distance, uint8_t *d_keep, int32_t *d_info);
/* The same with host buffers, synchronous (src/ORBDetectAndDespMatcher.cpp:61-81): desc_q nq x 32 bytes, desc_t nt x 32
 * bytes, train_idx / distance nq int32, keep nq bytes, info (or NULL) PAGK_ORB_INFO_WORDS words.  0 <= nq, nt <=
 * PAGK_ORB_MAX_ROWS. */
int pagk_orb_match(pagk_ctx *ctx, const pagk_orb_params *params, int32_t nq, const uint8_t *desc_q, int32_t nt,
                   const uint8_t *desc_t, int32_t *train_idx, int32_t *distance, uint8_t *keep, int32_t *info);

/* ---- ORB over a scale pyramid ----------------------------------------------------------------------------------------- */
/* ORBextractor is general in nlevels (src/ORBextractor.cc:434-470 the constructor, :1207-1230 ComputePyramid, :789-875
 * ComputeKeyPointsOctTree, :1066-1146 operator(), :1148-1205 DetectFeatures); both front-ends write the alternative next to
 * the value they ship ("int nLevels = 1;    // 8", Examples/Demo/RealSenseD435i.cpp:187).  This section is the extractor for
 * 1 <= nlevels <= PAGK_ORB_MAX_LEVELS.  The two n_levels fields of pagk_fast_params and pagk_orb_params describe the
 * one-level calls above and keep refusing anything but 1; the levels of this section come from pagk_orb_extractor.
 * Parity contract: the constructor's tables, ComputePyramid's sizes, the per-level loop, the packing and the mask test are
 * pinned to the reference's own src/ORBextractor.cc, compiled unchanged (oracle/_ref/ref_orb, oracle/README.md), through the
 * plain-C restatement tests/orb_levels_ref.c (on top of tests/fast_detect_ref.c and tests/orb_ref.c) and on the device, bit
 * for bit.  OpenCV under them (cv::resize, cv::FAST, GaussianBlur, copyMakeBorder) and pow remain this definition; no output
 * depends on the border copyMakeBorder writes, on any level.
 *   scales     (:439-455) sc[0] = 1.0f, sc[l] = sc[l - 1] * scale_factor (one f32 rounding per level), inv[l] = 1.0f / sc[l].
 *   sizes      (:1211-1212) W_l = cvRound((float)W * inv[l]), H_l = cvRound((float)H * inv[l]), ties to even; W and H are
 *              always the ORIGINAL image's.  Every level must be a legal input of the one-level detector: 62 <= W_l, H_l <=
 *              32767 and nIni >= 1 (PAGK_E_ARG otherwise: the reference divides by zero there).
 *   quotas     (:459-470) factor = 1.0f / scale_factor; nd = ((float)n_features * (1.0f - factor)) / (1.0f - (float)p), one
 *              f32 rounding per operation, where p is (double)factor multiplied n_levels times, starting from 1.0, in f64
 *              (the library's stated rule in place of pow).  quota[l] = cvRound(nd), then nd *= factor, for l < n_levels - 1;
 *              the last level gets max(n_features - sum, 0).  A quota of 0 is legal and reachable (10 features over 8 levels:
 *              2 2 2 1 1 1 1 0; one feature over 3 levels: 0 0 1).  The tree of a level with quota 0 runs with N = 1, which is
 *              identical to the reference's N = 0: the first splitting round runs unconditionally (:618-689), and the finish
 *              test size >= N || size == prevSize (:693) is then true for both values.
 *   pyramid    (:1207-1230) level 0 is the image, level l is the resize of level l - 1 to W_l x H_l: OpenCV 3.4's 8-bit
 *              INTER_LINEAR restated.  With src, dst the two extents of an axis: scale = 1 / ((double)dst / src); for
 *              destination index d: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s.  Columns: s < 0 gives
 *              (f, s) = (0, 0); s + 1 >= src makes the column a single tap S = 2048 I[s], and s >= src - 1 first gives
 *              (f, s) = (0, src - 1).  Rows: the two rows s and s + 1 are each clipped into [0, src - 1]; f stays.
 *              Coefficients in Q11 by cvRound: a0 = rne((1.f - fx) * 2048.f), a1 = rne(fx * 2048.f), b0, b1 likewise from
 *              fy.  Horizontal pass in int: S = I[s] a0 + I[s + 1] a1 per row.  Vertical pass: the low byte of
 *              (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.  Since scale_factor <= 1.5 a level is never
 *              exactly half its parent: at that ratio OpenCV switches to another kernel, which is not restated here.  The
 *              border image of copyMakeBorder (:1222-1228) is never read: the FAST windows and the orientation disc lie
 *              inside the level, as the one-level sections argue (cells start at minBorder = 16 with a ring of 3; the disc
 *              of radius 15 and the taps of reach 18 are only used for centres in [19, W_l - 19) x [19, H_l - 19)).
 *   per level  (:789-875) the one-level definition ("FAST in cells, then the quadtree") runs unchanged on the level image
 *              with N = max(quota[l], 1) and no mask.  Orientation runs on the unblurred level, the blur and the descriptor
 *              on the blurred level ("ORB descriptors and matching").  The centre rule [19, W_l - 19) x [19, H_l - 19) uses
 *              the LEVEL's size; a keypoint outside it gets a zero descriptor and angle -1, and is counted.
 *   packing    (:1113-1142) levels in ascending order, inside a level the tree's list order.  pt = pt_level * sc[l], one f32
 *              multiplication per coordinate, for l != 0; octave = l; the keypoint size size_l = (int)(31 * sc[l]) comes
 *              from the level table, not per keypoint.  Entries beyond the count are zeroed.
 *   detect     DetectFeatures (:1148-1205) is the same without orientation and descriptors, and a keypoint is dropped when
 *              mask[int(y) * W + int(x)] == 0 at the SCALED coordinates, W x H bytes of the original image (NULL: all ones;
 *              a scaled coordinate lies inside the image, because x_level <= W_l - 17 and W_l <= W inv[l] + 0.5).
 *              operator() never reads its mask (:1066-1146): the extract form has none.
 * Info, PAGK_ORB_LEVELS_INFO_WORDS int32: [0] keypoints returned, [1] keypoints outside the descriptor border, [2] levels,
 * [8 + l] keypoints of level l, [16 + l] raw FAST keypoints of level l, [24 + l] quota of level l, the rest 0.
 * None of the entry points takes an array in device memory from the caller: the device form works on a frame slot and
 * writes a keypoint set the context owns for that slot (the number of keypoints depends on the data and spans levels); the
 * results are read with the synchronous host-buffer calls. */
#define PAGK_ORB_MAX_LEVELS 8
#define PAGK_ORB_LEVELS_INFO_WORDS 32
typedef struct pagk_orb_extractor {
    int32_t n_features;    /* nfeatures 1000 */
    float scale_factor;    /* scaleFactor 1.2; 1 < scale_factor <= 1.5 */
    int32_t n_levels;      /* nlevels 8; 1 .. PAGK_ORB_MAX_LEVELS */
    int32_t ini_threshold; /* iniThFAST 20 */
    int32_t min_threshold; /* minThFAST 7 */
} pagk_orb_extractor;
/* 1000, 1.2f, 8, 20, 7: the five constructor arguments (src/ORBextractor.cc:434-437) as ORB is normally run */
void pagk_orb_extractor_default(pagk_orb_extractor *ex);
/* PAGK_OK if *ex can be run by the entry points below (the constructor, src/ORBextractor.cc:434-470): 1 <= n_levels <=
 * PAGK_ORB_MAX_LEVELS, 1 < scale_factor <= 1.5, thresholds in [0, 255], 1 <= n_features <= 1 << 24; PAGK_E_ARG otherwise or
 * for NULL.  Needs no device. */
int pagk_orb_extractor_check(const pagk_orb_extractor *ex);
/* The level table of a width x height image (src/ORBextractor.cc:439-470, 1211-1212): per level its size, sc[l], quota and
 * keypoint size; *out_bound = the sum over the levels of the one-level out_bound (pagk_detect_fast_bounds) with N =
 * max(quota[l], 1): the rows a keypoint set can hold.  Host arrays of PAGK_ORB_MAX_LEVELS entries (entries at or beyond
 * n_levels are zeroed); any pointer may be NULL.  PAGK_E_ARG for parameters the check refuses or a level the definition
 * excludes.  Needs no device. */
int pagk_orb_extractor_levels(const pagk_orb_extractor *ex, int32_t width, int32_t height, int32_t *level_width,
                              int32_t *level_height, float *scale, int32_t *quota, int32_t *size, int32_t *out_bound);
/* ORBextractor::operator() (src/ORBextractor.cc:1066-1146) on level 0 of frame slot `slot` (for how long a slot can be read
 * see pagk_detect_corners_device): pyramid, per-level detection, orientation, blur, descriptors, packing.  The result goes
 * into the keypoint set the context owns for that slot.  Asynchronous on the context stream, capturable; nothing is read on
 * the host.  Run it once outside a capture first (the pyramid, the set and the workspace are buffers of the context).
 * PAGK_E_ARG without a pattern, for an empty slot, for a size the level table refuses, or where a buffer would have to grow
 * inside a capture or under a live graph.  orb->n_levels stays 1: it describes the one-level calls; the levels are
 * ex->n_levels. */
int pagk_orb_extract_slot(pagk_ctx *ctx, const pagk_orb_extractor *ex, const pagk_orb_params *orb, int32_t slot);
/* The keypoint set of `slot` (what src/ORBextractor.cc:1113-1142 packs) into host arrays, synchronous: keypoints cap x 2
 * floats, octave cap int32, response cap floats, angle cap floats, desc cap x 32 bytes, info PAGK_ORB_LEVELS_INFO_WORDS
 * words; any array but keypoints may be NULL.  cap >= out_bound of the call that wrote the set (PAGK_E_ARG otherwise, or
 * for a slot without a set). */
int pagk_orb_slot_read(pagk_ctx *ctx, int32_t slot, int32_t cap, float *keypoints, int32_t *octave, float *response,
                       float *angle, uint8_t *desc, int32_t *info);
/* matcher->match and the distance filter of FindFeatureMatches (src/ORBDetectAndDespMatcher.cpp:61-81) between the sets of
 * slot_q (query) and slot_t (train), both written by pagk_orb_extract_slot: the launches of pagk_orb_match_device on the
 * context's own arrays and counts, the result kept by the context for slot_q.  Asynchronous on the context stream,
 * capturable; run it once outside a capture first.  Two pagk_orb_extract_slot calls and one pagk_orb_match_slots call are
 * FindFeatureMatches as one capturable chain. */
int pagk_orb_match_slots(pagk_ctx *ctx, const pagk_orb_params *orb, int32_t slot_q, int32_t slot_t);
/* The result of the last pagk_orb_match_slots with slot_q as the query (src/ORBDetectAndDespMatcher.cpp:61-81), synchronous:
 * train_idx, distance cap int32 each, keep cap bytes, info (or NULL) PAGK_ORB_INFO_WORDS words (the match info).  cap >= the
 * query set's out_bound; rows at or beyond the query count hold -1 / 257 / 0. */
int pagk_orb_match_slots_read(pagk_ctx *ctx, int32_t slot_q, int32_t cap, int32_t *train_idx, int32_t *distance,
                              uint8_t *keep, int32_t *info);
/* ORBextractor::operator() with host buffers, synchronous (src/ORBextractor.cc:1066-1146): the image is uploaded into a
 * scratch slot, pagk_orb_extract_slot's launches run, the set is read back as by pagk_orb_slot_read. */
int pagk_orb_extract_levels(pagk_ctx *ctx, const pagk_orb_extractor *ex, const pagk_orb_params *orb, const pagk_image *img,
                            int32_t cap, float *keypoints, int32_t *octave, float *response, float *angle, uint8_t *desc,
                            int32_t *info);
/* ORBextractor::DetectFeatures with host buffers, synchronous (src/ORBextractor.cc:1148-1205): mask (or NULL)
 * img->width * img->height bytes; keypoints cap x 2 floats, octave (or NULL) cap int32, response (or NULL) cap floats, info
 * (or NULL) PAGK_ORB_LEVELS_INFO_WORDS words ([1] is 0).  The output is a candidate list in the reference's order: an
 * application copies it into the candidate array of pagk_frame_handover_device. */
int pagk_orb_detect_levels(pagk_ctx *ctx, const pagk_orb_extractor *ex, const pagk_image *img, const uint8_t *mask,
                           int32_t cap, float *keypoints, int32_t *octave, float *response, int32_t *info);
/* Diagnostic, never on the per-frame path: level `level` (0 .. n_levels - 1) of the scale pyramid that the last
 * pagk_orb_extract_slot built for `slot` (ComputePyramid, src/ORBextractor.cc:1207-1230), into dst with rows of `pitch`
 * bytes.  Host pointer, synchronous, not between pagk_graph_begin and pagk_graph_end.  Localises a mismatch to the resize. */
int pagk_selftest_orb_level(pagk_ctx *ctx, int32_t slot, int32_t level, uint8_t *dst, int64_t pitch);

/* ---- Pyramidal Lucas-Kanade: tracker type 0, the image-only baseline of the reference's comparison ------------------ */
/* GyroAidedTracker::TrackFeatures with mType == OPENCV_OPTICAL_FLOW_PYR_LK (src/gyro_aided_tracker.cpp:353-380) calls
 * cv::calcOpticalFlowPyrLK on the two gray images with winSize = 2 half_patch + 1, maxLevel = 2,
 * TermCriteria(COUNT + EPS, 30, 0.01), flags = 0, minEigThreshold = 1e-4, clears the status of features with err >= 12
 * (:371-375) and forms the flow.  This section is that call for 8-bit one-channel images.
 * Parity contract: parity with OpenCV is NOT claimed (it cannot be built here); the contract is this definition, bit for
 * bit (restated in plain C in tests/lk_ref.c).  It follows OpenCV 3.4's scalar code path step by step and says where it is
 * the library's own rule.  win = 2 h + 1; r(i) = -i below 0 and 2 (n - 1) - i at or above n (BORDER_REFLECT_101, the r of
 * the ORB section).
 *   pyramid    level 0 is level 0 of the frame slot.  Level l + 1 has size ((W_l + 1) / 2, (H_l + 1) / 2); its pixel (x, y)
 *              is (sum_{i, j = 0..4} w_i w_j src(r(2 x + i - 2), r(2 y + j - 2)) + 128) >> 8 with w = 1 4 6 4 1: exact
 *              integers.  The effective top level is the largest L <= max_level such that every level 1 .. L has W_l > win
 *              and H_l > win (buildOpticalFlowPyramid's stop rule); level 0 itself must have W, H > win (PAGK_E_ARG
 *              otherwise).  These are NOT the slot's cv::resize levels (CreatePyramids, src/patch_match.cpp:61-76), which
 *              stay as they are.
 *   reads      gray values at any coordinate in [-win, W + win) x [-win, H + win) are read through r(); no read goes
 *              further.  Derivatives outside [0, W) x [0, H) are 0 (the constant border of derivI).
 *   derivative Scharr as calcSharrDeriv computes it, int arithmetic, neighbours through r():
 *              t0(x, y) = 3 (I(x, y - 1) + I(x, y + 1)) + 10 I(x, y), t1(x, y) = I(x, y + 1) - I(x, y - 1),
 *              dx = t0(x + 1, y) - t0(x - 1, y), dy = 3 (t1(x - 1, y) + t1(x + 1, y)) + 10 t1(x, y); both in [-4080, 4080].
 *   per feature, from the top level L down to 0; status starts at 1, err at 0:
 *   1 start    prev = pt_ref 2^-l (an exact f32 scaling).  At the top level next = prev, otherwise next = 2.f next of the
 *              level above.  next is stored before any test.  half = (win - 1) 0.5f.
 *   2 template p = prev - half, ip = floorf(p).  Out of range: ip.x < -win, ip.x >= W_l, ip.y < -win or ip.y >= H_l; a
 *              non-finite coordinate counts as out of range (the library's rule: decided in f32 before any conversion to
 *              int).  Out of range at level 0: status = 0, err = 0, the feature is done; at a higher level: on to the next
 *              level.
 *   3 weights  a = p.x - ip.x, b = p.y - ip.y; iw00 = rintf((1.f - a) (1.f - b) 16384.f), iw01 = rintf(a (1.f - b) 16384.f),
 *              iw10 = rintf((1.f - a) b 16384.f), iw11 = 16384 - iw00 - iw01 - iw10; f32 with one rounding per operation,
 *              no contraction; rintf rounds ties to even (cvRound).
 *   4 sums     for every window pixel Ival = (sum I iw + 256) >> 9 (0 .. 8160) over the four neighbours (x, y), (x + 1, y),
 *              (x, y + 1), (x + 1, y + 1) with iw00, iw01, iw10, iw11; ix, iy = (sum d iw + 8192) >> 14, arithmetic shifts.
 *              S11 = sum ix ix, S12 = sum ix iy, S22 = sum iy iy.  The library's rule: these sums, B1, B2 and the error sum
 *              below are EXACT integers in 64 bits, each converted to f32 once, round to nearest even (OpenCV accumulates
 *              in f32 in an order that differs between its scalar and SIMD builds; an exact sum is a function of the input
 *              and of nothing else, and needs no ordered chain on the device).  A11 = (float)S11 0x1p-20f, likewise A12, A22.
 *   5 test     D = A11 A22 - A12 A12; minEig = (A22 + A11 - sqrtf((A11 - A22) (A11 - A22) + 4.f A12 A12)) /
 *              (float)(2 win win): f32, one rounding per operation, left to right as written, correctly rounded sqrtf and
 *              division.  If (double)minEig < min_eig_threshold or D < FLT_EPSILON: status = 0 at level 0; on to the next
 *              level.  Otherwise D = 1.f / D.
 *   6 iterate  q = next - half; at most max_count times: iq = floorf(q), range as in step 2 (out of range at level 0:
 *              status = 0; either way leave the loop); weights from q as in step 3; diff = ((sum J iw + 256) >> 9) - Ival;
 *              B1 = sum diff ix, B2 = sum diff iy (exact); b1 = (float)B1 0x1p-20f, likewise b2;
 *              delta = ((A12 b2 - A22 b1) D, (A12 b1 - A11 b2) D) in f32; q += delta; next = q + half.  Stop if
 *              (double)delta.x delta.x + (double)delta.y delta.y <= epsilon epsilon (f64, left to right, no contraction).
 *              From the second iteration on: if (double)fabsf(delta.x + previous delta.x) < 0.01 and the same for y, then
 *              next -= delta 0.5f and stop.
 *   7 error    at level 0 with status still 1: e = next - half, range as in step 2 (out of range: status = 0); otherwise
 *              weights from e and err = (float)(sum |diff|) / (float)(32 win win).  err stays 0 wherever it is not written.
 *   filter     (:371-375) kept = status_raw && !(err >= err_threshold); flow = pt_out - pt_ref.
 * Info, PAGK_LK_INFO_WORDS int32: [0] n, [1] features with raw status 1, [2] kept, [3] the effective top level, [4] lost to
 * the min-eigenvalue test at level 0, [5] lost out of range at level 0, the rest 0.
 * Not provided: OPTFLOW_LK_GET_MIN_EIGENVALS, images with more than one channel.  OPTFLOW_USE_INITIAL_FLOW is provided by
 * pagk_lk_track_flow (the addendum below); pagk_lk_track_device and pagk_lk_track are flags = 0.
 *
 * Addendum: the flow form (pagk_lk_track_flow; kernel k_lk_flow, restated in plain C in tests/lk_flow_ref.c).  The reference
 * carries the flag as its own open experiment ("TODO: test OPTFLOW_USE_INITIAL_FLOW", "int flags = 0;
 * //cv::OPTFLOW_USE_INITIAL_FLOW;", src/gyro_aided_tracker.cpp:364-365).  Everything above holds; the changes are:
 *   1 start    at the top level next = pt_init 2^-L, the same exact f32 scaling as prev, in place of next = prev (OpenCV 3.4's
 *              OPTFLOW_USE_INITIAL_FLOW branch).  prev, the template, the tests, the iteration and the error are unchanged;
 *              flow = pt_out - pt_ref.  pt_init may be non-finite or far outside the image: the range rule of step 6 decides.
 *   status_in  the library's own rule: a row k below the count with status_in[k] == 0 is not tracked and is written like a row
 *              at or beyond the count: point, distorted point, err and flow 0, status and raw status 0.  It is counted in info
 *              [6] and in none of [1], [2], [4], [5]; [0] stays the count.  With the flag OpenCV would track such a row from
 *              whatever nextPts holds, which after GyroPredictFeatures is (0, 0) for a prediction that left the image
 *              (src/gyro_aided_tracker.cpp:131-139): a search started in the image's corner, which this rule leaves out.
 *   distorted  pt_out_dist = DistortVecPoints(pt_out) (src/utils.cpp:49-76; mvPtPredict = DistortVecPoints(mvPtPredictUn),
 *              src/gyro_aided_tracker.cpp:379) with the camera of a pagk_params: x = (u - cx) (float)(1.0 / fx), y likewise,
 *              r2 = x x + y y, r4 = r2 r2, r6 = r4 r2, xd = x (1 + k1 r2 + k2 r4 + k3 r6) + 2 p1 x y + p2 (r2 + 2 x x),
 *              yd = y (1 + k1 r2 + k2 r4 + k3 r6) + p1 (r2 + 2 y y) + 2 p2 x y, out = (fx xd + cx, fy yd + cy): f32, left to
 *              right, one rounding per operation, no contraction.  With dist_coef[0] == 0 it is a copy, as in the PatchMatch
 *              epilogue and the frame hand-over.  It is written for every tracked row whatever its status (:379 distorts all
 *              of them); zeroed rows get (0, 0).
 *   identity   with pt_init bit-equal to pt_ref (or NULL) and every status_in set (or NULL), every output equals
 *              pagk_lk_track's byte for byte.
 * Info word [6]: rows below the count that status_in switched off (0 from pagk_lk_track_device and pagk_lk_track). */
typedef struct pagk_lk_params {
    int32_t half_patch;        /* mHalfPatchSize: 10; winSize = 2 half_patch + 1 (:361) */
    int32_t max_level;         /* maxLevel 2 (:362) */
    int32_t max_count;         /* TermCriteria count 30 (:363) */
    double epsilon;            /* TermCriteria epsilon 0.01 (:363) */
    double min_eig_threshold;  /* 1e-4 (:366) */
    float err_threshold;       /* 12 (:372) */
} pagk_lk_params;
#define PAGK_LK_INFO_WORDS 8
#define PAGK_LK_MAX_ROWS 16777216
/* 10, 2, 30, 0.01, 1e-4, 12: the constants of src/gyro_aided_tracker.cpp:353-380 */
void pagk_lk_params_default(pagk_lk_params *p);
/* PAGK_OK if *p can be run by the entry points below (src/gyro_aided_tracker.cpp:353-380): 1 <= half_patch <=
 * PAGK_MAX_HALF_PATCH, 0 <= max_level < PAGK_MAX_PYRAMIDS, max_count >= 1, epsilon, min_eig_threshold and err_threshold
 * finite and >= 0; PAGK_E_ARG otherwise or for NULL.  Needs no device. */
int pagk_lk_params_check(const pagk_lk_params *p);
/* The effective top level of a width x height image under *params (the stop rule of the pyramid that
 * src/gyro_aided_tracker.cpp:353-380 has calcOpticalFlowPyrLK build), 0 .. max_level, or PAGK_E_ARG for parameters the check
 * refuses or a level 0 that is not larger than the window in both directions.  Needs no device. */
int pagk_lk_levels(int32_t width, int32_t height, const pagk_lk_params *params);
/* The pyrDown levels 1 .. top of frame slot `slot` (the pyramid cv::calcOpticalFlowPyrLK builds for each image,
 * src/gyro_aided_tracker.cpp:353-380) into a buffer the context owns for that slot; level 0 is read from the slot itself
 * (for how long a slot can be read see pagk_detect_corners_device).  Call it again whenever the slot's image has changed.
 * Asynchronous on the context stream, capturable.  Run it once outside a capture first (the buffer is the context's). */
int pagk_lk_pyramid_device(pagk_ctx *ctx, const pagk_lk_params *params, int32_t slot);
/* cv::calcOpticalFlowPyrLK and the error filter of src/gyro_aided_tracker.cpp:353-380 from slot_ref to slot_cur, which
 * have the same size and whose pyramids pagk_lk_pyramid_device has built for at least the top level of *params.
 * d_pt_ref, d_pt_out: cap x 2 float; d_n: a device count (clamped to [0, cap]) or NULL for cap; d_status: cap bytes (after
 * the filter); d_status_raw: cap bytes or NULL (before it); d_err: cap float; d_flow: cap x 2 float or NULL; d_info:
 * PAGK_LK_INFO_WORDS int32.  Rows at or beyond the count are zeroed.  1 <= cap <= PAGK_LK_MAX_ROWS.  The result does not
 * depend on the order in which the workgroups run.  Device pointers, asynchronous on the context stream, capturable;
 * nothing is read on the host. */
int pagk_lk_track_device(pagk_ctx *ctx, const pagk_lk_params *params, int32_t slot_ref, int32_t slot_cur, int32_t cap,
                         const float *d_pt_ref, const int32_t *d_n /* or NULL: cap */, float *d_pt_out, uint8_t *d_status,
                         uint8_t *d_status_raw /* or NULL */, float *d_err, float *d_flow /* or NULL */, int32_t *d_info);
/* The same with host buffers, synchronous (src/gyro_aided_tracker.cpp:353-380): both images are uploaded and their
 * pyramids built; pt_ref, pt_out n x 2 floats, status n bytes, status_raw (or NULL) n bytes, err n floats, flow (or NULL)
 * n x 2 floats, info (or NULL) PAGK_LK_INFO_WORDS words.  0 <= n <= PAGK_LK_MAX_ROWS. */
int pagk_lk_track(pagk_ctx *ctx, const pagk_lk_params *params, const pagk_image *ref, const pagk_image *cur, int32_t n,
                  const float *pt_ref, float *pt_out, uint8_t *status, uint8_t *status_raw, float *err, float *flow,
                  int32_t *info);
/* The flow form of the addendum above with host buffers, synchronous (src/gyro_aided_tracker.cpp:353-380 with the flag of
 * :364-365 and the distortion of :379): both images are uploaded and their pyramids built.  cam (or NULL: no pt_out_dist)
 * must pass pagk_params_check; only its camera model is read.  pt_ref, pt_out n x 2 floats; pt_init n x 2 floats or NULL for
 * pt_ref; status_in n bytes or NULL for all 1; pt_out_dist (or NULL) n x 2 floats; status n bytes; status_raw (or NULL) n
 * bytes; err n floats; flow (or NULL) n x 2 floats; info (or NULL) PAGK_LK_INFO_WORDS words.  0 <= n <= PAGK_LK_MAX_ROWS.  Not
 * between pagk_graph_begin and pagk_graph_end. */
int pagk_lk_track_flow(pagk_ctx *ctx, const pagk_lk_params *params, const pagk_params *cam /* or NULL: no pt_out_dist */,
                       const pagk_image *ref, const pagk_image *cur, int32_t n, const float *pt_ref,
                       const float *pt_init /* or NULL: pt_ref */, const uint8_t *status_in /* or NULL: all 1 */,
                       float *pt_out, float *pt_out_dist /* or NULL */, uint8_t *status, uint8_t *status_raw /* or NULL */,
                       float *err, float *flow /* or NULL */, int32_t *info /* or NULL */);
/* Diagnostic, never on the tracking path: level `level` (1 .. the top level built) of the pyramid that
 * pagk_lk_pyramid_device built for `slot` (the pyrDown levels behind src/gyro_aided_tracker.cpp:353-380), into dst with
 * rows of `pitch` bytes.  Host pointer, synchronous, not between pagk_graph_begin and pagk_graph_end. */
int pagk_selftest_lk_level(pagk_ctx *ctx, int32_t slot, int32_t level, uint8_t *dst, int64_t pitch);

/* Diagnostics (never on the tracking path): the arithmetic of H.llt().solve(b) / update.norm()
 * (src/patch_match.cpp:319,343) on the caller's operands, so that a host can check on its own device -- and, with
 * Eigen at hand, against its own Eigen -- what pagk_params::solver_variant selects.
 * pagk_selftest_divide: per item i, q_plain[i] = num[i] / den[i] (the compiler's correctly rounded division),
 * q_prepared[i] = the same quotient through the prepared-denominator form the kernels use, root[i] = sqrt(num[i]),
 * root_lean[i] = the same root through the solve's ten-instruction form (plain where num[i] is outside its range).
 * pagk_selftest_solve: per 4x4 system (H row-major, lower triangle read; b) the update x and its norm from the
 * one-lane form (x_serial, norm_serial = sqrt of the squared norm) and from the four-lane form (x_lanes, nsq_lanes =
 * the squared norm the kernels compare with the threshold equivalent to `norm < 1e-2`).  Host pointers. */
int pagk_selftest_divide(pagk_ctx *ctx, int32_t n, const double *num, const double *den, double *q_plain,
                         double *q_prepared, double *root, double *root_lean);
int pagk_selftest_solve(pagk_ctx *ctx, int32_t n, const double *H, const double *b, uint32_t solver_variant,
                        double *x_serial, double *norm_serial, double *x_lanes, double *nsq_lanes);
/* pagk_selftest_repeat_sum: H(2,2) of src/patch_match.cpp:296 is the ordered sum of `count` = (2h+1)^2 copies of c * c
 * (J[2] = de_dg = c is constant over the patch, :263).  The pipelined 4-wave kernel (half_patch 8, 9, 10) computes it in
 * closed form -- binade by binade, ~100 instructions -- instead of as a `count`-step chain; per item i this returns the
 * closed form (closed[i]) beside the loop s = fma(c, c, s) (loop[i]) for the caller's c[i].  57 < count <= 480.
 * Host pointers. */
int pagk_selftest_repeat_sum(pagk_ctx *ctx, int32_t n, const float *c, int32_t count, double *closed, double *loop);
/* pagk_selftest_sample: the bilinear sampler every tracking kernel shares (PatchMatch::GetPixelValue,
 * src/patch_match.cpp:391-406) on level `level` of a built slot, at the caller's n coordinates xy = (x, y) pairs: one thread
 * per coordinate reads the level's own packed taps.  mode 0: the clamped sampler, out = n floats.  mode 1: the clamp-free
 * sampler the kernels use for a patch that lies inside the image, n floats.  mode 2: the five clamped samples of one
 * Gauss-Newton pixel, out = 5 n floats (x, y), (x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1), the +-1 formed in float.
 * mode 3: the same five clamp-free.  The clamped modes take any float (NaN samples column / row 0).  The clamp-free modes
 * read without a test, so the call checks every coordinate first and returns PAGK_E_ARG, launching nothing, unless
 * 0 <= x < cols - 1 and 0 <= y < rows - 1 (mode 1) or 1 <= x < cols - 2 and 1 <= y < rows - 2 (mode 3) hold for all of them
 * (NaN fails).  Host pointers, synchronous, not between pagk_graph_begin and pagk_graph_end. */
int pagk_selftest_sample(pagk_ctx *ctx, int32_t slot, int32_t level, int32_t mode, int32_t n, const float *xy, float *out);
/* Selftest: overwrite the scratch this context owns with the 32-bit `word`, on the context's stream (the call waits for the
 * context's queued work first): every workspace and staging buffer the library has allocated for this context so far, the
 * row queue, the Lucas-Kanade pyramids of all slots and the blocks of all frame slots.  Afterwards NO frame slot is valid
 * and no slot has a Lucas-Kanade pyramid: the caller uploads its frames (and calls pagk_lk_pyramid_device) again before the
 * next call that reads them, and pagk_last_handover returns 0 until the next launch.  A sequence of the context
 * (pagk_sequence_create) is invalid until the next pagk_sequence_start, as frame slots are.  Left as they are: what has set / reset
 * calls of its own (the maps of pagk_rectify_set_maps, the pattern of pagk_orb_set_pattern, the priority hints and the
 * dispatch order) and the descriptors of the batched launches.
 * also_new != 0: from now on every block the library allocates for this context is filled with `word` before its first
 * use; also_new == 0 switches that off again.
 * PAGK_E_ARG inside a graph capture and while a graph of this context is alive.  No result of the library may depend on
 * `word`: that is what the call is for (tests/test_workspace_content_gpu.py). */
int pagk_selftest_fill_workspaces(pagk_ctx *ctx, uint32_t word, int32_t also_new);

/* hipGraph capture of the per-frame work (BASELINE configs[4], "hipGraph-captured iterate").  A camera
 * stream issues the same launches on the same device pointers every frame; between pagk_graph_begin and
 * pagk_graph_end the *_device entry points (pagk_frame_set_device, pagk_gyro_predict_device[_rot],
 * pagk_gyro_predict_device_live, pagk_track_device, pagk_post_filter_device, pagk_geometry_scores_device,
 * pagk_geometry_fit_device, pagk_geometry_validation_device, pagk_frame_handover_device, pagk_detect_corners_device,
 * pagk_frame_handover_detect_device, pagk_detect_fast_device,
 * pagk_frame_handover_fast_device, pagk_frame_rectify_device, pagk_orb_describe_device, pagk_orb_match_device,
 * pagk_orb_extract_slot, pagk_orb_match_slots, pagk_lk_pyramid_device, pagk_lk_track_device, pagk_match_features_device, pagk_search_gyro_predict_device,
 * pagk_search_klt_device; and the
 * pinned-memory forms pagk_frame_upload_pinned,
 * pagk_frame_rectify_pinned) are recorded on the context stream instead of executed,
 * pagk_graph_launch replays them with one hipGraphLaunch.  Rules: run the same calls once before capturing
 * (nothing may allocate during capture); host-buffer and synchronising entry points return PAGK_E_ARG while
 * capturing; the context stream must not be the legacy default stream; the kernel timers
 * (pagk_last_kernel_ms) do not see replays.  Up to 8 graphs per context.  The reference has no counterpart:
 * its per-frame loop is Examples/Demo/RealSenseD435i.cpp:199-321.
 * A captured pagk_track_device that hands its stragglers to the latency kernel (kernels 5 / 7 on large launches) is
 * replayed in SEGMENTS: HIP replays the parallel branches of one graph one after the other, and that kernel has to run
 * beside the throughput kernel, so the capture is closed in front of it, the finisher becomes a plain launch on the
 * context's auxiliary stream, and the capture reopens -- pagk_graph_launch then issues graph, finisher, graph, graph.
 * Same results, and the replayed step is as fast as the direct one (BASELINE configs[3]: 0.57 ms either way).  Such a
 * capture must not have forked other streams into itself at that point. */
int pagk_graph_begin(pagk_ctx *ctx);
int pagk_graph_end(pagk_ctx *ctx, int32_t *graph_id);
int pagk_graph_launch(pagk_ctx *ctx, int32_t graph_id);
int pagk_graph_destroy(pagk_ctx *ctx, int32_t graph_id);

/* Geometry validation, the consumer after the post-filter:
 * the per-correspondence scoring loops of GyroAidedTracker::CheckHomography
 * (src/gyro_aided_tracker.cpp:620-676) and ::CheckFundamental (:704-768) on models the caller fitted
 * (cv::findHomography / cv::findFundamentalMat, :596, :699, and H21.inv(), :597 -- or pagk_geometry_fit
 * below), passed as 3x3 matrices (row-major double, the layout of a CV_64F cv::Mat).  One launch scores both models (the reference runs them on two
 * threads, :455-460); inlier flags and the float scores, accumulated in index order, are
 * bit-identical to the reference loops.  pts1 / pts2: n x 2 float (mvKeysRefUn[i].pt, mvPtPredictUn[i]
 * of the status-true features, :434-440).
 *   pagk_geometry_scores_device: device pointers (d_scores: 2 floats, [0] = H, [1] = F),
 *                                asynchronous on the context stream;
 *   pagk_geometry_scores:        host buffers, synchronous. */
int pagk_geometry_scores_device(pagk_ctx *ctx, const double *H21, const double *H12, const double *F21,
                                int32_t n, const float *d_pts1, const float *d_pts2, float sigma,
                                uint8_t *d_inliers_H, uint8_t *d_inliers_F, float *d_scores);
int pagk_geometry_scores(pagk_ctx *ctx, const double *H21, const double *H12, const double *F21, int32_t n,
                         const float *pts1, const float *pts2, float sigma, uint8_t *inliers_H,
                         uint8_t *inliers_F, float *score_H, float *score_F);
/* Model choice of GeometryValidation (:462-470): 1 = homography (RH = score_H / (score_F + score_H)
 * > 0.45), 0 = fundamental. */
int pagk_geometry_select(float score_H, float score_F);
/* GyroAidedTracker::GeometryValidation (:429-480) around the fits: compacts the status-true
 * correspondences (:434-440), does nothing unless more than 8 remain (:445), scores both models on the
 * device, clears the status of the chosen model's outliers (:472-480).  status: n flags, updated in
 * place; track_score (may be NULL) receives the chosen model's score.  Host buffers, synchronous.
 * Returns cnt_inlier (>= 0; 0 when nothing was validated) or a negative error. */
int pagk_geometry_validation(pagk_ctx *ctx, const double *H21, const double *H12, const double *F21,
                             int32_t n, const float *pt_ref_un, const float *pt_predict_un,
                             uint8_t *status, float sigma, float *track_score);

/* ---- the RANSAC fits of GeometryValidation, on the device (src/gyro_aided_tracker.cpp:429-480, 589-768) ------ */
/* The reference fits H21 with cv::findHomography(vPts1, vPts2, cv::RANSAC, 3) (:597) and F21 with
 * cv::findFundamentalMat(vPts1, vPts2, CV_FM_RANSAC, 3., 0.99) (:691).  These entry points fit both models with a
 * DETERMINISTIC RANSAC instead.  Parity contract: NO parity with OpenCV is claimed (its random generator, minimal
 * solvers and Levenberg-Marquardt refinement are third-party and randomised); for a given seed and input the result is
 * bit-identical to the plain-C restatement in tests/geometry_fit_ref.c, and on clean two-view scenes the fits recover
 * the true models and inlier sets.  An application that needs OpenCV's own models keeps its fitter
 * (GyroAidedTracker::SetModelFitter, pagk_geometry_validation).
 *
 * The algorithm (m = the status-true correspondences, compacted in index order; all model arithmetic f64):
 *   sampling   hypothesis h of model k (0 = H, 4 points; 1 = F, 8 points): draw d = 0, 1, ... (at most 64) gives
 *              index ((z >> 32) * m) >> 32 with z = SplitMix64(seed ^ SplitMix64((k << 56) | (h << 8) | d)); a
 *              repeated index is redrawn; 64 draws without a full sample make the hypothesis invalid.
 *   degenerate H samples with three of the four points collinear in either image (sin^2 of the angle <= 1e-6) are
 *              invalid.
 *   solve      each image's sample is normalised (centroid to the origin, RMS distance sqrt(2), from the sums
 *              x, y, x^2 + y^2 taken in sample order); H: 4-point DLT, F: 8-point linear system; the null vector of the
 *              8x9 system (h9 = 1) by Gaussian elimination with partial pivoting -- a pivot at or below 1e-6 of the
 *              largest |entry|, a degenerate normalisation or a non-finite model make the hypothesis invalid
 *              (count -1, never chosen); the model is denormalised (H = T2^-1 Hn T1, F = T2^T Fn T1).
 *   consensus  H: |p2 w - H p1|^2 <= thresh_H^2 w^2 with w = (H p1)_3 (the squared forward transfer error, without its
 *              division); F: both squared point-to-epipolar-line distances <= thresh_F^2, compared as
 *              num^2 <= thresh^2 (a^2 + b^2).  Highest count wins, the lowest index on a tie.
 *   refit      once, on the best hypothesis' inliers: normalisation from their sums, the 9x9 normal matrix of the linear
 *              system (each sum: 256 partials over a stride of 256, a fixed tree), its smallest eigenvector by 10 steps
 *              of inverse iteration on M + 1e-12 tr(M) I (Cholesky); F is made rank 2 by F - (F v) v^T, v from a
 *              10-sweep cyclic Jacobi on F^T F; no Levenberg-Marquardt refinement (cv::findHomography has one).
 *              H21 is scaled to h33 = 1 (no model when |h33| <= 1e-12 max |h|), H12 is its inverse (cofactors / det),
 *              F21 is scaled to f33 = 1, or -- when |f33| <= 1e-12 max |f| -- to its largest |entry| = 1.  The masks are
 *              the refit models' inliers under the same tests.  No valid hypothesis, fewer inliers than a sample, or a
 *              non-finite refit: "no model" (info status 0, the model's doubles 0, its mask all 0).
 *   m <= 8     nothing is fitted (:445): no model, every hypothesis count -1.
 * Info words, PAGK_FIT_INFO_WORDS int32, six per model (H at 0, F at 6): status (1 = model, 0 = no model), the best
 * hypothesis (-1: none), its count, the refit model's inlier count, the number of valid hypotheses, and OpenCV's adaptive
 * iteration count ceil(log(1 - conf) / log(1 - w^s)) for w = best count / m (log restated with + - * /; 0 without a
 * valid hypothesis) -- more than iters_* means the budget was short of the confidence asked for. */
#define PAGK_FIT_INFO_WORDS 12
#define PAGK_FIT_MAX_ITERS 1048576
typedef struct pagk_fit_params {
    uint64_t seed;
    int32_t iters_H;   /* hypotheses of the homography, default 2000 (findHomography's maxIters), 1 .. PAGK_FIT_MAX_ITERS */
    int32_t iters_F;   /* hypotheses of the fundamental matrix, default 1000                                         */
    double thresh_H;   /* px, default 3 (:597 ransacReprojThreshold)                                                  */
    double thresh_F;   /* px, default 3 (:691 param1)                                                                 */
    double conf_H;     /* default 0.995, reported adaptive count only                                                 */
    double conf_F;     /* default 0.99 (:691 param2), reported adaptive count only                                    */
} pagk_fit_params;
void pagk_fit_params_default(pagk_fit_params *p);
/* Device pointers, asynchronous on the context stream, capturable (run the same call once before capturing: the
 * workspace is sized for n and the budgets by a call outside a capture).  d_status may be NULL (every point takes
 * part); d_models: 27 doubles H21 | H12 | F21 (row-major); d_mask_H / d_mask_F: n flags each, or NULL; d_info:
 * PAGK_FIT_INFO_WORDS; d_hyp_counts: iters_H + iters_F consensus counts (-1 = invalid), or NULL. */
int pagk_geometry_fit_device(pagk_ctx *ctx, const pagk_fit_params *params, int32_t n, const float *d_pts1,
                             const float *d_pts2, const uint8_t *d_status, double *d_models, uint8_t *d_mask_H,
                             uint8_t *d_mask_F, int32_t *d_info, int32_t *d_hyp_counts);
/* The same with host buffers, synchronous.  status, mask_H, mask_F and hyp_counts may be NULL. */
int pagk_geometry_fit(pagk_ctx *ctx, const pagk_fit_params *params, int32_t n, const float *pts1, const float *pts2,
                      const uint8_t *status, double *models, uint8_t *mask_H, uint8_t *mask_F, int32_t *info,
                      int32_t *hyp_counts);
/* GyroAidedTracker::GeometryValidation (:429-480) with the fits above, entirely on the device: compaction of the
 * status-true correspondences, the fits, the scoring loops of pagk_geometry_scores on the fitted models (read from
 * device memory), the choice of pagk_geometry_select, the chosen model's outliers cleared in d_status (in place).
 * d_cnt (1 int32) receives cnt_inlier, d_score (1 float) the chosen model's score.  Nothing changes in d_status (and
 * both outputs are 0) when at most 8 points take part or neither model could be fitted; a model that could not be
 * fitted scores 0 with no inliers.  Device pointers, asynchronous, capturable like pagk_geometry_fit_device. */
int pagk_geometry_validation_device(pagk_ctx *ctx, const pagk_fit_params *params, int32_t n, const float *d_pt_ref_un,
                                    const float *d_pt_predict_un, uint8_t *d_status, float sigma, int32_t *d_cnt,
                                    float *d_score);
/* pagk_geometry_validation without models: host buffers, synchronous; returns cnt_inlier (>= 0) or a negative
 * error.  Equal to pagk_geometry_validation fed with the models of pagk_geometry_fit. */
int pagk_geometry_validation_fit(pagk_ctx *ctx, const pagk_fit_params *params, int32_t n, const float *pt_ref_un,
                                 const float *pt_predict_un, uint8_t *status, float sigma, float *track_score);
/* Diagnostic: the drawn index sets of hypotheses first .. first + count - 1 of model (0 = H: 4 indices each, 1 = F: 8,
 * 2 = E: 5, the section below) among m points, -1s for a hypothesis whose draws ran out.  Host buffer idx, synchronous. */
int pagk_selftest_fit_samples(pagk_ctx *ctx, uint64_t seed, int32_t model, int32_t m, int32_t first, int32_t count,
                              int32_t *idx);

/* ---- Two-view pose: the essential matrix, R and t of a frame pair, on the device ------------------------------------ */
/* ORBDetectAndDespMatcher::PoseEstimation2d2d (src/ORBDetectAndDespMatcher.cpp:84-108), what both front-ends call behind
 * FindFeatureMatches (Examples/Demo/RealSenseD435i.cpp:282-284): cv::findFundamentalMat(points1, points2, cv::RANSAC) (:93),
 * cv::findEssentialMat(points1, points2, (mfx + mfy) / 2, cv::Point2d(mcx, mcy), cv::RANSAC) (:97), cv::findHomography(points1,
 * points2, cv::RANSAC, 3) (:101) and cv::recoverPose(mE, points1, points2, mR, mt, focal, pp) (:105).  H and F are the fits of
 * the section above (pagk_geometry_fit_device, bit for bit, its "more than 8 points" rule included); E, R and t are defined
 * here.  Parity contract: NO parity with OpenCV is claimed -- its random generator, its SVD-based five-point solver and
 * triangulatePoints are third-party.  The contract is this text, bit for bit, restated in plain C in tests/pose_ref.c.  Every
 * rule below that is not Nister's method or the reference's call is the library's own.  All model arithmetic is f64, one IEEE
 * rounding per operation, + - * / sqrt and comparisons only (no library call), every loop and sum in the stated order, sums
 * left to right.
 *
 *   points     the m status-true correspondences in index order (all n when status is NULL); a point takes part whatever the
 *              masks of H and F say (recoverPose is called without a mask, :105).
 *   normalise  q = ((u - cx) / f, (v - cy) / f, 1) for both images, u and v widened from f32; the pixel threshold becomes
 *              t = thresh_E / f.
 *   sampling   hypothesis h draws 5 distinct indices by the rule of the section above with model id k = 2 (the draws of H and F
 *              do not change); 64 draws without a full sample make the hypothesis invalid.
 *   null space the 5 x 9 system with rows (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1) is reduced by Gauss-Jordan with full
 *              pivoting: step j takes the largest |entry| of rows j.. and columns j.. (the first in row-major order on a tie),
 *              swaps it to (j, j), divides row j by it and subtracts f * row j from every other row.  A pivot at or below 1e-8
 *              of the system's largest |entry| makes the sample invalid.  Null vector k = 0 .. 3 has 1 at the k-th free column,
 *              minus column k of the reduced system at the pivot columns, 0 elsewhere.  The four vectors are orthonormalised by
 *              modified Gram-Schmidt in index order (dot products over the 9 entries in order): X, Y, Z, W.
 *   constraints  E = x X + y Y + z Z + W.  The 10 x 20 coefficient matrix, columns in Nister's order x3 y3 x2y xy2 x2z x2 y2z y2
 *              xyz xy | xz2 xz x yz2 yz y z3 z2 z 1: rows 0 .. 8 are the entries of (E E^T - 1/2 tr(E E^T) I) E in row-major
 *              order, row 9 is det E = e0 (e4 e8 - e5 e7) + e1 (e5 e6 - e3 e8) + e2 (e3 e7 - e4 e6).  Polynomial products
 *              accumulate term by term in monomial order (linear: x y z 1; quadratic: x2 y2 xy xz x yz y z2 z 1): of two
 *              linear factors the left one's monomials run in the outer loop, of a quadratic and a linear factor the
 *              quadratic's (the 2 x 2 cofactors of det E, the entries of E E^T - 1/2 tr I); a difference of two products adds
 *              the first and then subtracts the second, term by term; sums over the inner index k = 0, 1, 2 in order.  Gauss-Jordan with partial pivoting on the first
 *              ten columns (largest |entry| of the column from the diagonal down, the first on a tie; a pivot that is not > 0
 *              makes the sample invalid); rows 0 .. 3 are not updated after their own step.
 *   B(z)       rows 4 .. 9 are e (x2z), f (x2), g (y2z), h (y2), i (xyz), j (xy).  The rows e - z f, g - z h, i - z j form the
 *              3 x 3 matrix B(z) with columns x (degree 3), y (degree 3), 1 (degree 4); p(z) = det B(z), degree 10, by expansion
 *              along the third column (c0 (x1 y2 - x2 y1) - c1 (x0 y2 - x2 y0) + c2 (x0 y1 - x1 y0)), then divided by its
 *              largest |coefficient|.  A non-finite coefficient, p = 0 or a degree below 1 (after dropping exactly-zero leading
 *              coefficients) makes the sample invalid.
 *   real roots (the library's own algorithm) Cauchy's bound R = 1 + max |c_k / c_d|; the Sturm chain p, p', then the negated
 *              remainders of the polynomial division, each divided by its largest |coefficient|, exactly-zero leading
 *              coefficients dropped, ending at a zero remainder or degree 0; every polynomial is evaluated by Horner's rule.
 *              N = V(-R) - V(R) sign variations (zeros skipped), clamped to 0 .. 10.  Root r = 1 .. N in increasing order: the
 *              bracket (lo, hi] = (-R, R] is halved 64 times (mid = 0.5 (lo + hi); hi = mid when V(-R) - V(mid) >= r, else
 *              lo = mid); then x = 0.5 (lo + hi) takes up to 6 Newton steps x - p(x) / p'(x), stopping at the first step that
 *              leaves [lo, hi] or is not a number.  A companion-matrix eigen solver is not used.
 *   candidates per root z: of the three row pairs (0,1), (0,2), (1,2) of B(z) the one with the largest |2 x 2 determinant| of its
 *              x and y columns (the first on a tie) gives x and y by Cramer's rule; E = ((x X + y Y) + z Z) + W is divided by
 *              its Frobenius norm (sum of squares in index order).  A non-finite candidate is invalid.
 *   consensus  the Sampson distance without its division: with (a, b, c) = E q1, (d1, d2, .) = E^T q2, r = q2 . (E q1):
 *              r^2 <= t^2 (((a^2 + b^2) + d1^2) + d2^2).  Candidates are numbered 16 h + root; the highest integer count wins,
 *              the lowest number on a tie.  The winner is E: there is no refit (findEssentialMat has none).  mask_E holds its
 *              inliers.
 *   no model   fewer than 5 points, no valid candidate, or a best count below 5: E, R, t and both masks are 0, status 0.
 *   pose       Horn's closed form (no SVD, no Jacobi): G = E E^T, D_i = 1/2 tr G - G_ii; with i the largest D_i (the first on a
 *              tie) b = row i of (1/2 tr G I - G) / sqrt(D_i); (b . b) R1 = cof(E) - [b]x E, (b . b) R2 = cof(E) + [b]x E with
 *              cof the cofactor matrix; t = b / sqrt(b . b).  For E of Frobenius norm 1 D_i >= 1/6 up to rounding, so the
 *              division is defined.  det R = +1 and |t| = 1 as far as E satisfies its constraints.
 *   cheirality for each of (R1, t), (R2, t), (R1, -t), (R2, -t), in that order, and every point: a = R q1, the depths of
 *              lambda2 q2 = lambda1 a + t from the normal equations, det = (a.a)(q2.q2) - (a.q2)^2, lambda1 = ((a.q2)(q2.t) -
 *              (a.t)(q2.q2)) / det, lambda2 = ((a.a)(q2.t) - (a.q2)(a.t)) / det; the point is good when 0 < lambda1 < max_depth
 *              and 0 < lambda2 < max_depth (depths in units of |t|; a NaN is not good).  The pose with the most good points
 *              wins, the first on a tie; mask_pose holds its good points.
 * Info words, PAGK_POSE_INFO_WORDS int32: [0] status (1 = E, R, t; 0 = no model), [1] m, [2] the best hypothesis and [3] its
 * root (-1, -1: no valid candidate), [4] its count, [5] valid samples, [6] valid (finite) candidates, [7] OpenCV's adaptive
 * iteration count for w = best count / m, s = 5 and conf_E, as in the section above, [8] the chosen pose 0 .. 3, [9] .. [12]
 * the good counts of the four poses, the rest 0. */
#define PAGK_POSE_INFO_WORDS 16
typedef struct pagk_pose_params {
    uint64_t seed;
    int32_t iters_E;      /* hypotheses of the essential matrix, default 1000, 1 .. PAGK_FIT_MAX_ITERS                       */
    int32_t reserved;     /* 0                                                                                              */
    double thresh_E;      /* px, default 1 (findEssentialMat's threshold argument)                                          */
    double conf_E;        /* default 0.999 (its prob argument), reported adaptive count only                                 */
    double max_depth;     /* default 50: the distance threshold of OpenCV 3.4's recoverPose, a parameter so that a host can pin it */
    pagk_fit_params fit;  /* the H and F of the same call                                                                    */
} pagk_pose_params;
void pagk_pose_params_default(pagk_pose_params *p);
/* PAGK_OK if *p can be run by the entry points below (src/ORBDetectAndDespMatcher.cpp:84-108): iters_E in range, thresh_E and
 * max_depth finite and > 0, 0 < conf_E < 1, and a `fit` that pagk_geometry_fit_device accepts; PAGK_E_ARG otherwise or for
 * NULL.  Needs no device. */
int pagk_pose_params_check(const pagk_pose_params *p);
/* PoseEstimation2d2d (src/ORBDetectAndDespMatcher.cpp:93-105) on device correspondences.  f > 0, cx, cy: the calibration the
 * reference passes, (mfx + mfy) / 2 and (mcx, mcy).  d_pts1 / d_pts2: n x 2 float, d_status: n bytes or NULL; d_models: 27
 * doubles H21 | H12 | F21 and d_fit_info: PAGK_FIT_INFO_WORDS, as pagk_geometry_fit_device writes them; d_pose: 21 doubles
 * E | R | t (row-major); the four masks: n bytes each or NULL; d_pose_info: PAGK_POSE_INFO_WORDS; d_cand_counts: iters_E x 10
 * consensus counts (-1: no such root, or not finite) or NULL.  Device pointers, asynchronous on the context stream,
 * capturable; no count is read on the host (run the same call once before capturing: the workspaces are sized for n and
 * the budgets by a call outside a capture).  The result does not depend on the order in which the workgroups run. */
int pagk_pose_2d2d_device(pagk_ctx *ctx, const pagk_pose_params *params, double f, double cx, double cy, int32_t n,
                          const float *d_pts1, const float *d_pts2, const uint8_t *d_status /* or NULL */, double *d_models,
                          double *d_pose, uint8_t *d_mask_H, uint8_t *d_mask_F, uint8_t *d_mask_E, uint8_t *d_mask_pose,
                          int32_t *d_fit_info, int32_t *d_pose_info, int32_t *d_cand_counts /* or NULL */);
/* The input of PoseEstimation2d2d (src/ORBDetectAndDespMatcher.cpp:86-91) gathered on the device in front of the call above,
 * from what pagk_detect_fast_device and pagk_orb_match_device wrote: for query row q < cap_q, pts1[q] = d_kp_ref[q], pts2[q]
 * = d_kp_cur[d_train_idx[q]], status[q] = q < nq && d_keep[q] && 0 <= d_train_idx[q] < nt, with the device counts *d_nq and
 * *d_nt clamped to [0, cap_q] and [0, cap_t].  n = cap_q, and the masks (cap_q bytes each or NULL) are indexed by query row.
 * Device pointers, asynchronous on the context stream, capturable. */
int pagk_pose_from_matches_device(pagk_ctx *ctx, const pagk_pose_params *params, double f, double cx, double cy, int32_t cap_q,
                                  const float *d_kp_ref, const int32_t *d_nq, int32_t cap_t, const float *d_kp_cur,
                                  const int32_t *d_nt, const int32_t *d_train_idx, const uint8_t *d_keep, double *d_models,
                                  double *d_pose, uint8_t *d_mask_H, uint8_t *d_mask_F, uint8_t *d_mask_E, uint8_t *d_mask_pose,
                                  int32_t *d_fit_info, int32_t *d_pose_info);
/* pagk_pose_2d2d_device with host buffers, synchronous.  status, the masks and cand_counts may be NULL. */
int pagk_pose_2d2d(pagk_ctx *ctx, const pagk_pose_params *params, double f, double cx, double cy, int32_t n, const float *pts1,
                   const float *pts2, const uint8_t *status, double *models, double *pose, uint8_t *mask_H, uint8_t *mask_F,
                   uint8_t *mask_E, uint8_t *mask_pose, int32_t *fit_info, int32_t *pose_info, int32_t *cand_counts);

/* ---- NCC nearest-neighbour matching ------------------------------ */
/* GyroAidedTracker::FindAndSortNearNeighbor (src/gyro_aided_tracker.cpp:788-851) for all n reference keypoints
 * (the reference's cv::parallel_for_ over [0, mN), :912): for every feature with status 1 and no neighbours yet,
 * the current keypoints j whose undistorted position lies within level * radius_unit of the predicted point in
 * both coordinates (:811-815), each scored with the free NCC (src/utils.cpp:110-148) of the reference patch
 * around mvKeysRef[i].pt against the patch around mvKeysCur[j].pt warped by the feature's affine A -- sampled
 * with the free GetPixelValue of include/utils.h:32-46 (`>` clamp, four-term formula), not with
 * PatchMatch::GetPixelValue -- and sorted by the two-stack insertion of :825-842 (best first; equal keys: the
 * later index first).
 *   keys_ref      n x 2  mvKeysRef[i].pt           pt_predict_un  n x 2  mvPtPredictUn[i]
 *   status        n      mvStatus[i]               affine         n x 4  mvAffineDeformationMatrix[i]; NULL = empty Mat
 *   keys_cur      m x 2  mvKeysCur[j].pt           keys_cur_un    m x 2  mvKeysCurUn[j].pt
 *   level                1 or 2 (:912, :922)       radius_unit           mRadiusForFindNearNeighbor (= 2 * h, :62)
 *   use_ncc              mbNCC (:60: true); 0 sorts by distance, nearest first
 *   count         n      IN/OUT: mvvNearNeighbors[i].size(); features with count > 0 are skipped (:793), so a
 *                        second call with level 2 only fills the features the first left empty.  Zero it first.
 *   nbr_idx/dist/ncc  n x cap  sMatch::trainIdx / distance / ncc of the sorted lists (queryIdx = i, level = level)
 * pagk_near_neighbors_device: frames in slots (level 0 is used), device pointers, asynchronous on the context
 * stream; a list longer than cap leaves only its true size in d_count[i].  pagk_find_near_neighbors: host
 * buffers, synchronous; returns PAGK_E_CAPACITY when a list did not fit (count[] then holds the sizes needed). */
int pagk_near_neighbors_device(pagk_ctx *ctx, int32_t slot_ref, int32_t slot_cur, int32_t half_patch, int32_t n,
                               const float *d_keys_ref, const float *d_pt_predict_un, const uint8_t *d_status,
                               const float *d_affine, int32_t m, const float *d_keys_cur, const float *d_keys_cur_un,
                               int32_t level, float radius_unit, int32_t use_ncc, int32_t cap, int32_t *d_count,
                               int32_t *d_nbr_idx, float *d_nbr_dist, float *d_nbr_ncc);
int pagk_find_near_neighbors(pagk_ctx *ctx, const pagk_image *ref, const pagk_image *cur, int32_t half_patch, int32_t n,
                             const float *keys_ref, const float *pt_predict_un, const uint8_t *status,
                             const float *affine, int32_t m, const float *keys_cur, const float *keys_cur_un,
                             int32_t level, float radius_unit, int32_t use_ncc, int32_t cap, int32_t *count,
                             int32_t *nbr_idx, float *nbr_dist, float *nbr_ncc);
/* The free NCC(halfPatchSize, ref, cur, pt_ref, pt_cur, warp_mat) of src/utils.cpp:166-200 for n point pairs
 * (affine: n x 4 or NULL = empty warp_mat).  Host buffers, synchronous. */
int pagk_ncc_free(pagk_ctx *ctx, const pagk_image *ref, const pagk_image *cur, int32_t half_patch, int32_t n,
                  const float *pt_ref, const float *pt_cur, const float *affine, float *ncc);
/* GyroAidedTracker::MatchFeatures (src/gyro_aided_tracker.cpp:949-1008) on the lists above: thresholds
 * TH_NCC_HIGH 0.6, TH_NCC_LOW 0.3, TH_RATIO 0.75 (:7-9), one match per current keypoint -- a keypoint claimed
 * twice loses every match and stays banned (:991-1005).  Host-side, written as the reference's sequential pass; the result
 * is a count and a stable compaction, which pagk_match_features_device computes on the device.  match_*: capacity n
 * (match_dist / match_ncc may be NULL).  Returns mvMatches.size() or a negative error. */
int pagk_match_features(int32_t n, int32_t cap, const int32_t *count, const int32_t *nbr_idx, const float *nbr_dist,
                        const float *nbr_ncc, int32_t use_ncc, int32_t *match_query, int32_t *match_train,
                        float *match_dist, float *match_ncc);

/* ---- Track-to-detection association: which detected keypoint a tracked point belongs to -------------------------------- */
/* The two public methods of GyroAidedTracker that tie a tracked point to a keypoint detected independently in the current
 * frame: SearchByGyroPredict (src/gyro_aided_tracker.cpp:859-939) and SearchByOpencvKLT (:1017-1136), behind a finished
 * prediction / PatchMatch and behind pyramidal Lucas-Kanade.  Everything runs on the device, the "fewer than 100 matches"
 * retry (:921) and both filters included; nothing is read on the host.  The contract is this definition, bit for bit,
 * restated sequentially in plain C in tests/associate_ref.c (the std::set and erase loop of :949-1008 and the iterator loop
 * of :1111-1129, literally).  f32 arithmetic has one rounding per operation, no contraction.
 *
 * MatchFeatures (:949-1008) on the lists of the section above, n features, m current keypoints, lists of capacity cap:
 *   choice     feature i with c = count[i], its two best entries (ncc0, ncc1), (dist0, dist1) and t = nbr_idx[i][0] (:955-990):
 *              c <= 0: none.  use_ncc: ncc0 > th_ncc_high takes t; otherwise, with c > 1: ncc0 < th_ncc_low: none;
 *              ncc1 < ncc0 * th_ratio takes t; otherwise none.  Distance mode: c == 1 takes t; c > 1: dist0 < dist1 * th_ratio
 *              takes t.  The comparisons are written as pagk_match_features writes them (NaN falls the same way).
 *   own rules  the treatment of over-long lists and bad indices is the library's own: c > cap: none, counted in info[1]
 *              (pagk_match_features returns PAGK_E_CAPACITY instead); a taken t outside [0, m): none, counted in info[2]
 *              (the reference has no such index).
 *   uniqueness a current keypoint enters sFoundInCurPts at its first claim, every later claim erases all matches to it, and
 *              it is never admitted again (:993-1007).  So feature i keeps its choice t if and only if exactly one feature
 *              chose t, and the matches stand in increasing i: a count and a stable compaction, no sequential pass.
 *   outputs    match_query, match_train, match_dist (= dist0), match_ncc (= ncc0) in match order, the count in *d_n_matches;
 *              rows at or beyond the count: -1, -1, 0, 0.  With the default thresholds equal to pagk_match_features byte for
 *              byte whenever no list exceeds cap.
 *   flow error (:928-933) flows_err[i] = keys_cur_un[t] - pt_predict_un[i] (f32) for a kept feature, (0, 0) for every other.
 *   info       PAGK_ASSOC_INFO_WORDS int32: [0] features with a choice, [1] lists longer than cap, [2] train indices out of
 *              range, [3] current keypoints claimed more than once, [4] matches, [5] 1 if the level-2 search ran, the rest 0.
 *
 * SearchByOpencvKLT (:1017-1136) behind Lucas-Kanade (the section "Pyramidal Lucas-Kanade"), cap rows, m detected keypoints.
 * Parity with OpenCV's BFMatcher is NOT claimed; where a rule is the library's own it says so:
 *   queries    row i is live iff i < n (the device count clamped to [0, cap]) and status[i] != 0 after the err filter
 *              (:1047-1057); its query point q is Lucas-Kanade's pt_out[i].
 *   neighbours radiusMatch (:1067): the detected keypoints j < m (the device count clamped to [0, m]) in index order,
 *              d = sqrtf(dx*dx + dy*dy) with dx = q.x - t.x, dy = q.y - t.y, f32, left to right, correctly rounded sqrtf;
 *              j is a neighbour iff d <= klt_max_distance (`<=` at the radius: the library's own rule; NaN is no neighbour).
 *              The best and the second best are kept, replacement under strict `<`: equal distances keep the lower index in
 *              front (tie order of equal distances: the library's own rule, std::sort in OpenCV is unstable there).
 *   choice     (:1076-1087) exactly one neighbour: it.  Two or more: (double)(d0 / d1) < klt_ratio takes the best, an f32
 *              division then widened (:1080); 0 / 0 is NaN and rejects.  None: no choice.
 *   uniqueness (:1089-1105) first come: of the queries that chose t the lowest index keeps it, the others are dropped.
 *   disparity  (:1096-1102) disp = (double)sqrtf((rx-cx)*(rx-cx) + (ry-cy)*(ry-cy)), r = keys_ref[i], c = keys_cur[t]: the
 *              detected keypoint, not the tracked point; std::sqrt of a float is the f32 overload.
 *   filter     (:1108-1130) sum1 = the f64 sum of disp in match order, one rounding per add; avg1 = sum1 / (double)k (k == 0:
 *              NaN, nothing is dropped); th = avg1 * klt_disparity_factor; matches with disp > th are dropped, the order of
 *              the others stays.
 *   outputs    match_query, match_train, match_dist (= d0), disparity (f64) in match order, the count; rows at or beyond
 *              the count: -1, -1, 0, 0.  stats, PAGK_ASSOC_STATS_WORDS doubles: [0] avg1, [1] avg2 (:1130), [2], [3] the
 *              largest disparity before and after the filter (from 0; NaN never replaces), [4] th, [5] sum1, [6] sum2, [7] 0.
 *   info       PAGK_ASSOC_INFO_WORDS int32: [0] live queries, [1] / [2] / [3] queries with 0 / 1 / 2 or more neighbours,
 *              [4] ratio rejects, [5] lost to an earlier claimer, [6] dropped by the disparity filter, [7] matches.
 * Workspaces belong to the context: run a call once with its sizes outside a capture first.  The results do not depend on
 * the order in which workgroups run (the only atomics are integer adds and minima). */
typedef struct pagk_assoc_params {
    float th_ncc_high;            /* TH_NCC_HIGH 0.6 (:7) */
    float th_ncc_low;             /* TH_NCC_LOW 0.3 (:8) */
    float th_ratio;               /* TH_RATIO 0.75 (:9) */
    int32_t use_ncc;              /* mbNCC: 1 (:60) */
    int32_t min_matches;          /* 100 (:921): fewer matches than this and the search is repeated at twice the radius */
    float klt_max_distance;       /* maxDistance 4 (:1066) */
    double klt_ratio;             /* 0.7 (:1081) */
    double klt_disparity_factor;  /* filterOutFactor 1.5 (:1115) */
} pagk_assoc_params;
#define PAGK_ASSOC_INFO_WORDS 8
#define PAGK_ASSOC_STATS_WORDS 8
/* 0.6, 0.3, 0.75, 1, 100, 4, 0.7, 1.5: the constants of src/gyro_aided_tracker.cpp:7-9, :60, :921, :1066, :1081, :1115 */
void pagk_assoc_params_default(pagk_assoc_params *p);
/* PAGK_OK if *p can be run by the entry points below (src/gyro_aided_tracker.cpp:859-939, :1017-1136): every threshold
 * finite and >= 0, use_ncc 0 or 1, min_matches >= 0; PAGK_E_ARG otherwise or for NULL.  Needs no device. */
int pagk_assoc_params_check(const pagk_assoc_params *p);
/* MatchFeatures (src/gyro_aided_tracker.cpp:949-1008) on device lists, as defined above: d_count n, d_nbr_* n x cap,
 * d_match_* n rows (d_match_dist / d_match_ncc may be NULL), d_n_matches one int32, d_info PAGK_ASSOC_INFO_WORDS.  n, m >= 0,
 * cap >= 1.  Device pointers, asynchronous on the context stream, capturable; nothing is read on the host. */
int pagk_match_features_device(pagk_ctx *ctx, const pagk_assoc_params *params, int32_t n, int32_t m, int32_t cap,
                               const int32_t *d_count, const int32_t *d_nbr_idx, const float *d_nbr_dist,
                               const float *d_nbr_ncc, int32_t *d_match_query, int32_t *d_match_train,
                               float *d_match_dist /* or NULL */, float *d_match_ncc /* or NULL */, int32_t *d_n_matches,
                               int32_t *d_info);
/* Steps 2 and 3 of SearchByGyroPredict (src/gyro_aided_tracker.cpp:909-938) behind a finished prediction or PatchMatch;
 * the arguments of pagk_near_neighbors_device without `level` (use_ncc comes from *params).  The call zeroes d_count, then:
 * the neighbour search at level 1; choose and compact; the search at level 2 -- every workgroup of it returns at once
 * unless *d_n_matches < min_matches, and it fills only the empty lists (:793); choose and compact again (the same result
 * when level 2 did not run).  d_m: a device count of the live current keypoints (clamped to [0, m]) or NULL for m;
 * d_flows_err: n x 2 float or NULL.  A list longer than cap leaves its true size in d_count[i] and is counted in info[1].
 * Device pointers, asynchronous on the context stream, capturable: the retry is decided on the device at every replay. */
int pagk_search_gyro_predict_device(pagk_ctx *ctx, const pagk_assoc_params *params, int32_t slot_ref, int32_t slot_cur,
                                    int32_t half_patch, int32_t n, const float *d_keys_ref, const float *d_pt_predict_un,
                                    const uint8_t *d_status, const float *d_affine, int32_t m, const float *d_keys_cur,
                                    const float *d_keys_cur_un, const int32_t *d_m /* or NULL: m */, float radius_unit,
                                    int32_t cap, int32_t *d_count, int32_t *d_nbr_idx, float *d_nbr_dist, float *d_nbr_ncc,
                                    int32_t *d_match_query, int32_t *d_match_train, float *d_match_dist /* or NULL */,
                                    float *d_match_ncc /* or NULL */, int32_t *d_n_matches, float *d_flows_err /* or NULL */,
                                    int32_t *d_info);
/* The same with host buffers, synchronous (src/gyro_aided_tracker.cpp:909-938): both images are uploaded.  Returns
 * mvMatches.size(), or PAGK_E_CAPACITY when info[1] is not zero (count[] then holds the sizes needed, as in
 * pagk_find_near_neighbors; the device form only reports the word), or another negative error.  info may be NULL. */
int pagk_search_gyro_predict(pagk_ctx *ctx, const pagk_assoc_params *params, const pagk_image *ref, const pagk_image *cur,
                             int32_t half_patch, int32_t n, const float *keys_ref, const float *pt_predict_un,
                             const uint8_t *status, const float *affine, int32_t m, const float *keys_cur,
                             const float *keys_cur_un, float radius_unit, int32_t cap, int32_t *count, int32_t *nbr_idx,
                             float *nbr_dist, float *nbr_ncc, int32_t *match_query, int32_t *match_train, float *match_dist,
                             float *match_ncc, float *flows_err, int32_t *info);
/* SearchByOpencvKLT (src/gyro_aided_tracker.cpp:1017-1136): pagk_lk_track_device from slot_ref to slot_cur (whose pyramids
 * pagk_lk_pyramid_device has built), then the association defined above.  d_keys_ref, d_pt_out cap x 2 float; d_n, d_m device
 * counts or NULL for cap, m; d_keys_cur m x 2 float; d_status cap bytes, d_err cap float (Lucas-Kanade's, after the err
 * filter); d_match_query, d_match_train cap int32, d_match_dist cap float or NULL, d_disparity cap double, d_n_matches one
 * int32, d_stats PAGK_ASSOC_STATS_WORDS double, d_info PAGK_ASSOC_INFO_WORDS and d_lk_info PAGK_LK_INFO_WORDS int32.
 * Device pointers, asynchronous on the context stream, capturable; nothing is read on the host. */
int pagk_search_klt_device(pagk_ctx *ctx, const pagk_lk_params *lk_params, const pagk_assoc_params *assoc_params,
                           int32_t slot_ref, int32_t slot_cur, int32_t cap, const float *d_keys_ref,
                           const int32_t *d_n /* or NULL: cap */, int32_t m, const float *d_keys_cur,
                           const int32_t *d_m /* or NULL: m */, float *d_pt_out, uint8_t *d_status, float *d_err,
                           int32_t *d_match_query, int32_t *d_match_train, float *d_match_dist /* or NULL */,
                           double *d_disparity, int32_t *d_n_matches, double *d_stats, int32_t *d_info, int32_t *d_lk_info);
/* The same with host buffers, synchronous (src/gyro_aided_tracker.cpp:1017-1136): both images are uploaded and their
 * pyramids built.  Returns mvMatches.size() or a negative error.  match_dist, stats, info and lk_info may be NULL. */
int pagk_search_klt(pagk_ctx *ctx, const pagk_lk_params *lk_params, const pagk_assoc_params *assoc_params,
                    const pagk_image *ref, const pagk_image *cur, int32_t n, const float *keys_ref, int32_t m,
                    const float *keys_cur, float *pt_out, uint8_t *status, float *err, int32_t *match_query,
                    int32_t *match_train, float *match_dist, double *disparity, double *stats, int32_t *info,
                    int32_t *lk_info);

/* ---- the path sharded over the GPUs of one node ---------------------- */
/* Features are independent units (the cv::parallel_for_ of src/patch_match.cpp:103), so the path shards by
 * contiguous index blocks of ceil(n / G) features: rank r owns [r * ceil(n/G), min(n, (r+1) * ceil(n/G))).  Every
 * GPU holds both pyramids; the only exchange is ONE all-gather (RCCL ncclAllGather over xGMI) of the packed
 * per-rank result slice, after which every rank holds every result and the tracker's global post-filter
 * (src/gyro_aided_tracker.cpp:289-341) runs on them in index order.  The library owns the RCCL communicator
 * (loaded with dlopen on first use); failures of RCCL calls return PAGK_E_NCCL. */
typedef struct pagk_multi pagk_multi;
/* One process driving n_devices GPUs (a C++ GyroAidedTracker host): one context and one RCCL rank per device
 * (ncclCommInitAll).  n_devices = 1 is a valid group. */
int pagk_multi_create(pagk_multi **out, const int32_t *devices, int32_t n_devices);
/* One process per GPU (e.g. under torchrun): rank 0 calls pagk_multi_unique_id, the host application hands the 128
 * bytes to every rank through its own channel, each rank joins with its device (ncclCommInitRank). */
int pagk_multi_unique_id(uint8_t id[128]);
int pagk_multi_create_rank(pagk_multi **out, const uint8_t id[128], int32_t rank, int32_t world, int32_t device);
void pagk_multi_destroy(pagk_multi *pm);
int32_t pagk_multi_world(const pagk_multi *pm);  /* ranks of the group                        */
int32_t pagk_multi_local(const pagk_multi *pm);  /* ranks driven by this process              */
int32_t pagk_multi_comm_count(const pagk_multi *pm); /* ncclCommCount of the group's communicator: the ranks RCCL itself
                                                        reports (a benchmark line's proof that the gather spans N GPUs);
                                                        negative when unavailable */
pagk_ctx *pagk_multi_ctx(pagk_multi *pm, int32_t local_index);  /* owned by the group; do not pagk_destroy */
const char *pagk_multi_last_error(const pagk_multi *pm);
/* The partition and the layout of a rank's packed result slice for m = ceil(n / G) features: seven SoA blocks in
 * SetMatcher order (pt_un, pt_dist, status, pix_err, dist_pred, ncc, iters), each padded to 8 bytes; returns the
 * slice size in bytes. */
void pagk_shard_range(int32_t n, int32_t rank, int32_t world, int32_t *lo, int32_t *hi);
size_t pagk_shard_layout(int32_t m, size_t offsets[7]);
/* The exchange: every local member k contributes `bytes` bytes at d_send[k] and receives world * bytes at
 * d_recv[k], in rank order, on its context's stream (hip_streams: NULL, or one stream per local member).
 * Asynchronous; ordered on the stream after the tracking launch that produced the slice. */
int pagk_multi_allgather(pagk_multi *pm, const void *const *d_send, void *const *d_recv, size_t bytes,
                         void *const *hip_streams);
/* pagk_track with the feature loop split over the group (single-process groups): same arguments, same results
 * bit for bit.  Every GPU uploads both frames and builds both pyramids, tracks its block, the packed slices are
 * all-gathered, the host reads the gathered result from member 0.  Synchronous. */
int pagk_track_sharded(pagk_multi *pm, const pagk_params *params, const pagk_image *ref, const pagk_image *cur,
                       int32_t n, const float *pt_ref_un, const float *pt_init_un, const float *affine,
                       const uint8_t *status_in, const pagk_outputs *out);

/* ---- Gyro integration: the IMU window of a frame pair -> Rcl and K Rcl K^-1 ------------------------------------------- */
/* GyroAidedTracker::IntegrateGyroMeasurements, IntegrateOneGyroMeasurement and SetRcl (src/gyro_aided_tracker.cpp:511-587)
 * turn the gyroscope samples between two frames into the rotation Rcl and into K Rcl K^-1.  Parity contract: parity with
 * OpenCV's MatExpr evaluation and with a C library's sin / cos is NOT claimed (neither can be pinned here); the contract is
 * this definition, bit for bit, restated in plain C in tests/gyro_integrate_ref.c.  It follows the reference's expressions
 * step by step; f32 and f64 operations round once each (no contraction).
 *   window     samples (t_i, w_i), i = 0 .. samples - 1: f64 time stamps, f32 rates in rad/s; t_ref and t_cur are the two
 *              frames' time stamps, bias the gyroscope bias.  n = samples - 1 steps; 0 or 1 samples give dR = I.
 *   time steps every time difference is the f64 difference of two time stamps, rounded once to f32 (tab, tini, tend, tstep).
 *   step i     (:530-555, the four cases in the reference's order; w0 = w_i, w1 = w_(i+1), per component in f32)
 *              i == 0 and i < n - 1:  tab = t1 - t0, tini = t0 - t_ref, angVel = ((w0 + w1) - (w1 - w0) * (tini / tab)) * 0.5f,
 *                                     tstep = t1 - t_ref
 *              else i < n - 1:        angVel = (w0 + w1) * 0.5f, tstep = t1 - t0
 *              else i > 0 (the last): tab = t1 - t0, tend = t1 - t_cur, angVel = ((w0 + w1) - (w1 - w0) * (tend / tab)) * 0.5f,
 *                                     tstep = t_cur - t0
 *              else (n == 1):         angVel = w0, tstep = t_cur - t_ref
 *   deltaR     (IntegrateOneGyroMeasurement, :564-587) x = (float)((double)(angVel.x - bias.x) * (double)tstep), y and z alike;
 *              d2 = x * x + y * y + z * z in f32, left to right; d = sqrtf(d2), correctly rounded; W = the skew matrix
 *              0 -z y / z 0 -x / -y x 0.  If (double)d < 1e-4: R = I + W in f32.  Otherwise WW = W * W (a product as below),
 *              s = (double)(float)sin, c = (double)(1.0f - (float)cos) -- the reference's std::sin(float) and
 *              std::cos(float) return float, so each result is rounded once to f32, and 1.0f - cos is an f32 difference --
 *              with sin and cos the f64 ALGORITHM of the ORB "steering" paragraph above applied to (double)d (no library
 *              sin or cos is called; its k = (int)v saturates at 2147483647), and
 *              R[k] = (float)(((double)I[k] + (double)W[k] * s / (double)d) + (double)WW[k] * c / (double)d2).
 *   products   every 3 x 3 product: f32 factors, an f64 accumulator starting at 0, k ascending, one rounding to f32.
 *              dR = dR * deltaR_i for i = 0 .. n - 1, left to right from dR = I; Rcl = (Rbc^T * dR^T) * Rbc (:560);
 *              KRKinv = (K * Rcl) * inv3(K) (:518) with K = fx 0 cx / 0 fy cy / 0 0 1 and inv3 the f64 cofactor inverse:
 *              det expanded along the first row, each cofactor times (det != 0 ? 1 / det : 0), rounded once to f32.
 *   output     Rcl (9 floats, row-major) and rot9: rows 0 and 1 of KRKinv followed by the third row of Rcl, exactly what
 *              pagk_gyro_predict_device_rot reads.
 * A window is refused on the host with PAGK_E_ARG and never reaches the device when it has more than imu_cap samples, a
 * non-finite time, rate or bias, sample times that do not increase strictly, or t_cur <= t_ref. */
#define PAGK_IMU_MAX_SAMPLES 64
typedef struct pagk_imu_window {
    double t_ref, t_cur; /* mTimeStampRef, mTimeStamp: the two frames' time stamps, t_cur > t_ref */
    int32_t n;           /* samples (mvImuFromLastFrame.size()), 0 .. imu_cap                    */
    const double *t;     /* host: n time stamps, strictly increasing                             */
    const float *w;      /* host: n x 3 angular rates, rad/s                                     */
    float bias[3];       /* mBias                                                                */
} pagk_imu_window;
/* The window checks above (src/gyro_aided_tracker.cpp:521-562 makes none): PAGK_OK, or PAGK_E_ARG for NULL, imu_cap outside
 * 1 .. PAGK_IMU_MAX_SAMPLES, or a window the list above refuses.  Needs no device. */
int pagk_imu_window_check(const pagk_imu_window *window, int32_t imu_cap);
/* The definition above on the device (src/gyro_aided_tracker.cpp:511-587; one launch of one wavefront, csrc/pagk_gyro_kernel.h),
 * host buffers, synchronous: Rbc = the top-left 3 x 3 of Tbc, row-major; camera: fx, fy, cx, cy are read; Rcl and rot9: 9
 * floats each, either may be NULL.  PAGK_E_ARG for a window the check refuses (imu_cap = PAGK_IMU_MAX_SAMPLES) and inside a
 * capture. */
int pagk_gyro_integrate(pagk_ctx *ctx, const float Rbc[9], const pagk_params *camera, const pagk_imu_window *window,
                        float *Rcl, float *rot9);

/* ---- The sequence the context owns: the frame loop behind the C ABI --------------------------------------------------- */
/* The reference's main loop (Examples/Demo/RealSenseD435i.cpp:199-321: grab a frame and the gyro rotation, track, hand the
 * result over to the next pair) with everything between two frames on the device and every buffer owned by the context:
 * the caller hands in host frames and nine rotation floats and reads host arrays back.  One sequence per context.  The
 * tracker is PatchMatch behind the gyro prediction (tracker type 4, src/gyro_aided_tracker.cpp:381-392), pyramidal
 * Lucas-Kanade (type 0, :353-380), or Lucas-Kanade started from the gyro prediction (the flow form of the section
 * "Pyramidal Lucas-Kanade", the reference's open experiment at :364-365).
 * A step enqueues on the context stream, in the reference's order (the copy of the inputs into the fixed input block of the
 * sequence stands in front of it, outside the graph):
 *   PatchMatch  frame -> pyramid (pagk_frame_set_device); pagk_gyro_predict_device_live when has_gyro_predict_initial;
 *               pagk_track_device; pagk_post_filter_device (Step 3, :289-341); pagk_geometry_validation_device when
 *               `validate`; the hand-over of the chosen detector (:97-111, src/frame.cpp:115-218).
 *   LK          frame -> pyramid -> pagk_lk_pyramid_device (the other slot's was built one frame earlier); with
 *               lk_initial_flow pagk_gyro_predict_device_live, whose pt_predict_un becomes pt_init and whose status becomes
 *               status_in; the flow kernel with the live count on the device (its status_in is the live mask otherwise);
 *               pagk_geometry_validation_device on Lucas-Kanade's status when `validate`; the hand-over.  There is no
 *               Step-3 post-filter: it belongs to GyroPredictFeaturesAndOpticalFlowRefined, which type 0 does not enter.
 * With PAGK_SEQ_GRAPH the first step of each parity runs directly (allocations happen outside a capture), the next one of
 * that parity is captured, and later steps replay one of the two graphs; the context stream must then not be the legacy
 * default stream (pagk_graph_begin).  Every sequence call returns PAGK_E_ARG between pagk_graph_begin and pagk_graph_end.
 * After pagk_selftest_fill_workspaces a sequence is invalid until the next pagk_sequence_start, as frame slots are.
 * Out of scope: raw-frame rectification, gyro integration and mvFlowVelocityInNormalPlane in a sequence made by
 * pagk_sequence_create (they are what "The sensor form of the sequence" below adds); in both forms: k cameras batched,
 * sharding, tracker type GYRO_PREDICT, the C++ shell classes. */
#define PAGK_SEQ_PATCHMATCH 0
#define PAGK_SEQ_LK 1
#define PAGK_SEQ_GRAPH 0
#define PAGK_SEQ_DIRECT 1
#define PAGK_SEQ_STATUS_WORDS 4
typedef struct pagk_sequence_params {
    pagk_params track;           /* the PatchMatch configuration and the camera model (both trackers read the camera) */
    pagk_lk_params lk;           /* PAGK_SEQ_LK: the constants of src/gyro_aided_tracker.cpp:353-380 */
    pagk_fit_params fit;         /* the fits of the geometry validation (:429-480), read when `validate` */
    pagk_detect_params harris;   /* detector 1: src/frame.cpp:181-184 */
    pagk_fast_params fast;       /* detector 2: src/ORBextractor.cc:1148-1205 */
    double new_point_threshold;  /* mThresholdOfPredictNewKeyPoint = mN * th (src/frame.cpp:79) */
    int32_t tracker;             /* PAGK_SEQ_PATCHMATCH or PAGK_SEQ_LK */
    int32_t lk_initial_flow;     /* PAGK_SEQ_LK: 0 = flags 0, 1 = started from the gyro prediction */
    int32_t width, height;       /* of every frame */
    int32_t cap;                 /* rows of every key array; >= target_n */
    int32_t target_n;            /* Frame::mN */
    int32_t detector;            /* 0 the caller's candidate list, 1 Harris (goodFeaturesToTrack), 2 FAST cells and quadtree */
    int32_t cand_cap;            /* detector 0: the longest candidate list, >= 1 */
    int32_t validate;            /* 0 or 1: GeometryValidation behind the tracker */
    float sigma;                 /* its sigma (1.0 in the reference) */
} pagk_sequence_params;
/* The reference's demo configuration (Examples/Demo/RealSenseD435i.cpp:199-321): pagk_params_default, pagk_lk_params_default,
 * pagk_fit_params_default, both detectors' defaults, PatchMatch, 640 x 480, cap 448, target_n 400, threshold 320, the
 * caller's candidate list (cand_cap 1024), validation on, sigma 1. */
void pagk_sequence_params_default(pagk_sequence_params *p);
/* PAGK_OK if pagk_sequence_create accepts *p (Examples/Demo/RealSenseD435i.cpp:199-321): each nested block passes its own
 * check; tracker, lk_initial_flow, validate in {0, 1}; detector in {0, 1, 2}; width, height >= 14; cap >= target_n >= 1,
 * cap <= PAGK_LK_MAX_ROWS; cand_cap >= 1 for detector 0; new_point_threshold and sigma finite, sigma > 0; for PAGK_SEQ_LK
 * a frame larger than the window (pagk_lk_levels).  PAGK_E_ARG (or the nested check's code) otherwise.  Needs no device. */
int pagk_sequence_params_check(const pagk_sequence_params *p);
/* The sequence of this context (Examples/Demo/RealSenseD435i.cpp:199-321, the objects the loop keeps between frames):
 * reserves two key sets, the work arrays, the state and info words and the fixed input block in one buffer of the
 * context, and a ring of four pinned input blocks.  PAGK_E_ARG for a second sequence, inside a capture, or for parameters
 * the check refuses.  pagk_destroy destroys a live sequence. */
int pagk_sequence_create(pagk_ctx *ctx, const pagk_sequence_params *params);
/* Ends the sequence (Examples/Demo/RealSenseD435i.cpp:199-321, leaving the loop): waits for its queued work, destroys its
 * graphs, frees its blocks.  PAGK_E_ARG without a sequence or inside a capture. */
int pagk_sequence_destroy(pagk_ctx *ctx);
/* The first frame (Examples/Demo/RealSenseD435i.cpp:221-235): its pyramid into slot 0 and the first-frame hand-over, an
 * all-zero status, into key set 0.  frame: a host image of the sequence's size.  cand: host, n_cand x 2 floats
 * (0 <= n_cand <= cand_cap), required for detector 0 (non-NULL also when n_cand is 0) and refused (non-NULL or n_cand != 0) otherwise.  Runs directly, never
 * as a graph; may be called again to restart (graphs are kept).  Invalid after pagk_selftest_fill_workspaces until called. */
int pagk_sequence_start(pagk_ctx *ctx, const pagk_image *frame, const float *cand, int32_t n_cand);
/* Frame k >= 1 (Examples/Demo/RealSenseD435i.cpp:237-321): tracks pair (k - 1, k) and hands over to pair (k, k + 1).  rot9:
 * nine host floats, rows 0 and 1 of K R K^-1 followed by the third row of R, as pagk_gyro_predict_device_rot defines them
 * (NULL: nine zeros are NOT substituted -- PAGK_E_ARG when the tracker predicts).  mode: PAGK_SEQ_GRAPH or PAGK_SEQ_DIRECT.
 * Nothing is synchronised except the flow control of the pinned ring (a block is rewritten only after the copy that read
 * it, four frames earlier, has run).  PAGK_E_ARG before pagk_sequence_start. */
int pagk_sequence_step(pagk_ctx *ctx, const pagk_image *frame, const float *rot9, const float *cand, int32_t n_cand,
                       int32_t mode);
/* The current key set (Examples/Demo/RealSenseD435i.cpp:199-321, what the next pair starts from), synchronous: the first
 * `cap` rows (1 <= cap <= the sequence's cap) of keys, keys_un, keys_normal (x 2 floats), index_in_last (int32), live
 * (bytes); state: PAGK_HANDOVER_STATE_WORDS int32; info: PAGK_DETECT_INFO_WORDS int32 of the detector (zeros for detector
 * 0).  Any array but keys_un may be NULL. */
int pagk_sequence_read(pagk_ctx *ctx, int32_t cap, float *keys, float *keys_un, float *keys_normal, int32_t *index_in_last,
                       uint8_t *live, int32_t *state, int32_t *info);
/* What SetBackToFrame (src/gyro_aided_tracker.cpp:97-111; Examples/Demo/RealSenseD435i.cpp:199-321) hands over for the last
 * pair, synchronous: status (the mask after validation), pt_predict, pt_predict_un (x 2 floats), err (Lucas-Kanade's error;
 * 0 for PatchMatch), the first `cap` rows each.  Any array may be NULL.  PAGK_E_ARG before the first pagk_sequence_step. */
int pagk_sequence_read_pair(pagk_ctx *ctx, int32_t cap, uint8_t *status, float *pt_predict, float *pt_predict_un, float *err);
/* Host-side words, nothing synchronised (Examples/Demo/RealSenseD435i.cpp:199-321 has no counterpart), PAGK_SEQ_STATUS_WORDS
 * int32: [0] frames handed in, [1] 1 if the last step was a graph replay, [2] graphs held, [3] the depth of the result
 * ring (pagk_sequence_results_create), 0 without one. */
int pagk_sequence_status(pagk_ctx *ctx, int32_t *words);

/* ---- The sensor form of the sequence: raw frames and the IMU window in, tracked features out --------------------------- */
/* What a camera and an IMU deliver, instead of a rectified gray frame and nine rotation floats: both front-ends of the
 * reference remap every frame (Examples/Demo/RealSenseD435i.cpp:202), convert it to gray (src/frame.cpp:81-87) and integrate
 * the gyroscope samples between two frames (src/gyro_aided_tracker.cpp:511-587).  A sensor sequence does the three inside
 * the step.  The raw frame's rows, the window (times, rates, bias, t_ref, t_cur, n) and the candidates go into the pinned
 * ring block and with one asynchronous copy into the fixed input block; the issue order behind it is: rectification into
 * the parity's frame slot and its pyramid ("Rectification" above; Lucas-Kanade reads the rectified level 0 of the slot),
 * k_gyro_integrate ("Gyro integration" above) writing the nine floats the prediction reads, the chain of the chosen tracker
 * as for a plain sequence, then k_flow_velocity.  Graph mode follows the plain sequence's rule; so does everything the plain
 * section says about captures and pagk_selftest_fill_workspaces.  pagk_sequence_read, pagk_sequence_read_pair,
 * pagk_sequence_status and pagk_sequence_destroy serve both kinds; pagk_sequence_start and pagk_sequence_step return
 * PAGK_E_ARG on a sensor sequence, the _sensor calls on a plain one.  The results are those of a plain sequence fed the
 * rectified frames (pagk_rectify) and the rot9 of the window (pagk_gyro_integrate), bit for bit.
 *   flow velocity  (mvFlowVelocityInNormalPlane, src/frame.cpp:139-143) row j of the new key set with i = index_in_last[j] >= 0:
 *                  ((keys_normal_cur[j] - keys_normal_last[i]) in f32) / (t_cur - t_last), the divisor the f64 difference of
 *                  the two time stamps, the division as OpenCV's Point2f / double: an f64 quotient rounded once to f32.
 *                  Rows with index_in_last < 0 and rows at or beyond the live count get (0, 0); so does every row of the
 *                  first frame.  The reference indexes this vector by the compacted count (:143): that is row j. */
typedef struct pagk_sequence_sensor {
    pagk_rectify_params rectify; /* raw = 1: the gray step of the raw frames; raw = 0: channels must be 1        */
    int32_t raw;                 /* 0: frames arrive gray, at the sequence's size; 1: raw, through the context's maps */
    int32_t src_width, src_height; /* raw = 1: the size of a raw frame, 1 .. 32767 each                           */
    int32_t imu_cap;             /* the longest window, 1 .. PAGK_IMU_MAX_SAMPLES                                 */
    float Rbc[9];                /* the top-left 3 x 3 of Tbc (mRbc), row-major                                   */
    int32_t flow_velocity;       /* 0 or 1: mvFlowVelocityInNormalPlane behind the hand-over                      */
} pagk_sequence_sensor;
/* pagk_rectify_params_default, frames that arrive gray, imu_cap PAGK_IMU_MAX_SAMPLES, Rbc = I, flow_velocity 1
 * (src/frame.cpp:139-143 always computes it). */
void pagk_sequence_sensor_default(pagk_sequence_sensor *s);
/* PAGK_OK if pagk_sequence_create_sensor accepts *s (Examples/Demo/RealSenseD435i.cpp:199-321): the rectify block passes
 * its check; raw, flow_velocity in {0, 1}; the sizes and imu_cap in the ranges above; Rbc finite.  PAGK_E_ARG otherwise or for
 * NULL.  Needs no device. */
int pagk_sequence_sensor_check(const pagk_sequence_sensor *s);
/* pagk_sequence_create for a sensor sequence (Examples/Demo/RealSenseD435i.cpp:199-321): the same block with the window in
 * the input block and the sensor parts (rot9, Rcl, velocities) behind it; a plain sequence's layout does not change.  With
 * raw = 1 the maps must have been set (pagk_rectify_set_maps) with the sequence's width x height: PAGK_E_ARG otherwise, with
 * a text in pagk_last_error. */
int pagk_sequence_create_sensor(pagk_ctx *ctx, const pagk_sequence_params *params, const pagk_sequence_sensor *sensor);
/* pagk_sequence_start for a sensor sequence (Examples/Demo/RealSenseD435i.cpp:221-235).  raw: a host image; with raw = 1
 * width and height are the raw frame's, in pixels of `channels` bytes, and step >= width * channels.  t: the frame's time
 * stamp, finite. */
int pagk_sequence_start_sensor(pagk_ctx *ctx, const pagk_image *raw, double t, const float *cand, int32_t n_cand);
/* pagk_sequence_step for a sensor sequence (Examples/Demo/RealSenseD435i.cpp:237-321).  window: the samples between the
 * previous frame and this one; PAGK_E_ARG, with nothing enqueued, for a window pagk_imu_window_check refuses with the
 * sequence's imu_cap and for a t_ref that is not the previous frame's time (t of the start, t_cur of the last step). */
int pagk_sequence_step_sensor(pagk_ctx *ctx, const pagk_image *raw, const pagk_imu_window *window, const float *cand,
                              int32_t n_cand, int32_t mode);
/* The flow velocities of the current key set (src/frame.cpp:139-143), synchronous: the first `cap` rows x 2 floats.
 * PAGK_E_ARG on a plain sequence, with flow_velocity = 0, or before pagk_sequence_start_sensor. */
int pagk_sequence_read_velocity(pagk_ctx *ctx, int32_t cap, float *v);

/* ---- The sequence group: k cameras stepped together -------------------------------------------------------------------- */
/* A rig runs the reference's loop (Examples/Demo/RealSenseD435i.cpp:199-321) once per camera.  A sequence group is k contexts
 * on one device, each holding a plain sequence made by pagk_sequence_create, stepped together: it lifts the first item of
 * the plain section's "Out of scope" list, k cameras batched.  Per camera the results are, byte for byte, those of the same
 * sequence stepped alone with the same frames, rot9 and candidates.
 * A frame of one camera is twelve launches, ten of them kernels of one or two workgroups whose cost is launch and
 * dependent-load latency.  A group step issues every stage ONCE for all cameras, on the stream of ctxs[0], the lead:
 *   1. the lead's stream waits for what every member's stream has enqueued;
 *   2. every member's inputs go into the next block of its own pinned ring and from there, one asynchronous copy per member,
 *      into its own fixed input block (these copies stand in front of the graph; each ring keeps its own flow control);
 *   3. pagk_frame_set_device_batch; the prediction when has_gyro_predict_initial; pagk_track_device_batch (which keeps its
 *      rule: small totals run as k launches); Step 3; the five kernels of the validation when `validate`; the three of the
 *      hand-over -- each a launch with the camera as the grid's second dimension, reading its camera's arguments from a table
 *      the lead owns;
 *   4. every member's stream waits for the last launch, so that a member's synchronous reads see the step.
 * The first step after pagk_sequence_group_create runs member by member (every member's workspaces get their final size),
 * the next one as batched launches outside a capture (so do the lead's); from then on graph mode follows the plain
 * sequence's rule per parity: the first step of a parity runs directly, the next is captured, later ones replay one of the
 * group's two graphs.  A captured group step is one linear chain of nodes on the lead's stream, which must not be the
 * legacy default stream.
 * The group serves PatchMatch with the caller's candidate lists (tracker PAGK_SEQ_PATCHMATCH, detector 0), with or without
 * the gyro prediction and the validation.  Out of scope of the group: Lucas-Kanade, the Harris and FAST detectors, sensor
 * sequences (pagk_sequence_create_sensor), cameras that are configured differently, contexts on different devices.
 * (Lucas-Kanade has a group call of its own: "Lucas-Kanade in the sequence groups", pagk_sequence_group_create_lk.) */
/* PAGK_OK iff pagk_sequence_group_create accepts sequences of these parameters (Examples/Demo/RealSenseD435i.cpp:199-321, one
 * loop per camera): pagk_sequence_params_check passes, tracker == PAGK_SEQ_PATCHMATCH and detector == 0; validate and
 * track.has_gyro_predict_initial may each be 0 or 1.  PAGK_E_ARG (or the nested check's code) otherwise.  Needs no device. */
int pagk_sequence_group_check(const pagk_sequence_params *p);
/* Makes ctxs[0 .. k-1] a group (Examples/Demo/RealSenseD435i.cpp:199-321, the objects k loops keep between frames); ctxs[0]
 * is the lead and owns it.  PAGK_E_ARG, with a text in pagk_last_error(ctxs[0]), for NULL arguments, k outside 1 .. 64,
 * contexts on different devices, a context listed twice, a context without a sequence, with a sensor sequence or in a
 * group already, a call inside a capture, parameters that are not byte-equal across the members (the trackers of one
 * application are configured alike, as for pagk_track_device_batch) or that pagk_sequence_group_check refuses.  While
 * grouped a member's own pagk_sequence_start, pagk_sequence_step and pagk_sequence_destroy return PAGK_E_ARG;
 * pagk_sequence_read, pagk_sequence_read_pair and pagk_sequence_status keep working and see the group's results.  Other
 * calls on a member that make its fit workspace, its hand-over mask or its hints grow invalidate the group's table: the
 * next step returns PAGK_E_ARG and the group has to be destroyed. */
int pagk_sequence_group_create(pagk_ctx *const *ctxs, int32_t k);
/* Ends the group (Examples/Demo/RealSenseD435i.cpp:199-321, leaving the loops): waits for the queued work of every member,
 * destroys the group's graphs and table, and leaves every member an ordinary sequence that can be stepped alone from where
 * it stands.  pagk_destroy of the lead destroys the group first; pagk_destroy of another member dissolves it first.
 * PAGK_E_ARG when `lead` leads no group or inside a capture. */
int pagk_sequence_group_destroy(pagk_ctx *lead);
/* The k first frames (Examples/Demo/RealSenseD435i.cpp:221-235): k times pagk_sequence_start, frames[j], cand[j] and
 * n_cand[j] being camera j's; not a hot path.  Checks every camera's inputs first: PAGK_E_ARG with nothing enqueued if one
 * would be refused.  May be called again to restart; the group's graphs are kept. */
int pagk_sequence_group_start(pagk_ctx *lead, const pagk_image *frames, const float *const *cand, const int32_t *n_cand);
/* Frame k >= 1 of every camera (Examples/Demo/RealSenseD435i.cpp:237-321), in the issue order above.  frames: k host images;
 * rot9: k x 9 host floats, camera j's at rot9 + 9 j (NULL only when nothing predicts); cand, n_cand: k host lists and their
 * lengths; mode: PAGK_SEQ_GRAPH or PAGK_SEQ_DIRECT.  PAGK_E_ARG, with nothing enqueued, if any camera's frame, list or
 * rot9 would be refused by pagk_sequence_step, before pagk_sequence_group_start, or when the members do not stand at the
 * same frame. */
int pagk_sequence_group_step(pagk_ctx *lead, const pagk_image *frames, const float *rot9, const float *const *cand,
                             const int32_t *n_cand, int32_t mode);
/* Host-side words, nothing synchronised (Examples/Demo/RealSenseD435i.cpp:199-321 has no counterpart), PAGK_SEQ_STATUS_WORDS
 * int32: [0] frames handed in per camera, [1] 1 if the last step was a graph replay, [2] graphs held by the group, [3] k. */
int pagk_sequence_group_status(pagk_ctx *lead, int32_t *words);

/* ---- The sensor form of the sequence group: k raw frames and k IMU windows in ------------------------------------------ */
/* What a rig's cameras and IMU deliver.  Every front-end of the reference remaps and grays its frame
 * (Examples/Demo/RealSenseD435i.cpp:202, src/frame.cpp:81-87), integrates the gyro window (src/gyro_aided_tracker.cpp:511-587)
 * and tops up with ORBextractor::DetectFeatures (src/frame.cpp:172-179).  A sensor group is k contexts on one device, each
 * holding a sensor sequence made by pagk_sequence_create_sensor, stepped together: it lifts two items of the plain group's
 * "Out of scope" list, sensor sequences and the FAST detector.  Per camera every array of pagk_sequence_read,
 * pagk_sequence_read_pair and pagk_sequence_read_velocity is, after every frame, byte for byte that of the same sensor
 * sequence stepped alone with the same raw frames, windows and lists.
 * The stages a sensor step adds are launches of one or a few workgroups, and a group step issues each of them ONCE for all
 * cameras, the camera being the grid's second dimension, from a second table the lead owns.  The issue order on the lead's
 * stream is that of one sensor sequence, stage by stage:
 *   1. the lead's stream waits for what every member's stream has enqueued;
 *   2. every member's raw rows, window and list go into its own pinned ring block and, one asynchronous copy per member,
 *      into its own fixed input block;
 *   3. with raw = 1 the rectification of all cameras, each through its own maps into its own frame slot; then
 *      pagk_frame_set_device_batch on the slots' own level 0 (with raw = 0 on the input blocks);
 *   4. the gyro integration of all windows (always, also when nothing predicts), each with its camera's Rbc; the
 *      prediction when has_gyro_predict_initial; pagk_track_device_batch; Step 3; the validation when `validate`;
 *   5. the hand-over: fill and holes; with detector 2 the plan and the four kernels of the FAST detector, every camera under
 *      its own skip word (in one step the top-up may run for one camera and not for another); the keys;
 *   6. the flow velocities when flow_velocity; then every member's stream waits for the last launch.
 * Graph mode follows the plain group's rule: the first step runs member by member (that sizes every member's FAST
 * workspace), the second as batched launches outside a capture, then a parity is captured at its next step once it has run
 * directly, and replayed afterwards; a captured step is one linear chain.
 * The sensor group serves PatchMatch with the caller's candidate lists (detector 0) or the FAST detector (detector 2), with
 * or without the prediction, the validation, raw frames and the flow velocities.  What stays out: the Harris detector,
 * Lucas-Kanade, cameras whose parameters differ (anything but Rbc and the maps), contexts on different devices.
 * (Lucas-Kanade has a group call of its own: "Lucas-Kanade in the sequence groups", pagk_sequence_group_create_lk.) */
/* PAGK_OK iff pagk_sequence_group_create_sensor accepts sensor sequences of these blocks (Examples/Demo/RealSenseD435i.cpp:
 * 199-321, one loop per camera): pagk_sequence_params_check and pagk_sequence_sensor_check pass, tracker ==
 * PAGK_SEQ_PATCHMATCH and detector is 0 or 2; validate, track.has_gyro_predict_initial, raw and flow_velocity may each be 0
 * or 1.  PAGK_E_ARG (or the nested check's code) otherwise, so for the Harris detector and Lucas-Kanade.  Needs no device. */
int pagk_sequence_group_sensor_check(const pagk_sequence_params *p, const pagk_sequence_sensor *s);
/* pagk_sequence_group_create for sensor sequences (Examples/Demo/RealSenseD435i.cpp:199-321, the objects k loops keep between
 * frames); ctxs[0] is the lead.  Refuses, with a text in pagk_last_error(ctxs[0]), everything pagk_sequence_group_create
 * refuses, a plain sequence among the members, pagk_sequence_params that are not byte-equal, and pagk_sequence_sensor
 * blocks that differ in anything but Rbc (every camera has its own extrinsic rotation).  Every member keeps its own maps
 * (pagk_rectify_set_maps: every camera has its own lens).  pagk_sequence_group_status, pagk_sequence_group_destroy and
 * pagk_destroy of a member serve both kinds of group; pagk_sequence_group_start and pagk_sequence_group_step return
 * PAGK_E_ARG on a sensor group, the _sensor calls on a plain one.  While grouped a member's own
 * pagk_sequence_start_sensor, pagk_sequence_step_sensor and pagk_sequence_destroy return PAGK_E_ARG; its
 * pagk_sequence_read, pagk_sequence_read_pair, pagk_sequence_read_velocity and pagk_sequence_status keep working.  Calls
 * outside the group that move a member's FAST workspace, its map entries, its frame slots or its sequence invalidate
 * the tables like those the plain group names. */
int pagk_sequence_group_create_sensor(pagk_ctx *const *ctxs, int32_t k);
/* The k first raw frames (Examples/Demo/RealSenseD435i.cpp:221-235): k times pagk_sequence_start_sensor, raws[j], t[j],
 * cand[j] and n_cand[j] being camera j's (cand and n_cand NULL with detector 2).  All inputs are checked first: PAGK_E_ARG
 * with nothing enqueued if one is refused.  May be called again to restart; the group's graphs are kept. */
int pagk_sequence_group_start_sensor(pagk_ctx *lead, const pagk_image *raws, const double *t, const float *const *cand,
                                     const int32_t *n_cand);
/* Raw frame k >= 1 of every camera with its window (Examples/Demo/RealSenseD435i.cpp:237-321), in the issue order above.
 * raws: k host images; windows: k windows, camera j's the samples between its previous frame and this one; cand, n_cand: k
 * host lists and their lengths, both NULL with detector 2; mode: PAGK_SEQ_GRAPH or PAGK_SEQ_DIRECT.  Every camera's window
 * is checked on the host (pagk_imu_window_check with the sequence's imu_cap; t_ref must equal that camera's previous time)
 * before anything is enqueued: a refusal of any camera's frame, window or list returns PAGK_E_ARG and changes nothing. */
int pagk_sequence_group_step_sensor(pagk_ctx *lead, const pagk_image *raws, const pagk_imu_window *windows,
                                    const float *const *cand, const int32_t *n_cand, int32_t mode);

/* ---- The result ring of a sequence: every frame's results through pinned blocks, with track ids ------------------------ */
/* The output half of the loop (no counterpart in the reference, whose loop reads its Frame objects on the host:
 * Examples/Demo/RealSenseD435i.cpp:237-321).  pagk_sequence_read, pagk_sequence_read_pair and pagk_sequence_read_velocity
 * synchronise the stream and see the last frame handed in only.  A sequence with a result ring packs, as the last launch of
 * every frame (inside the captured chain), everything those three calls deliver plus a persistent track id and an age per
 * row into ONE record on the device; behind the step (behind the graph launch, outside any capture) one asynchronous copy
 * puts the record of frame f into pinned block f % depth and records that block's event -- the mirror image of the input
 * copy in front of the step.  pagk_sequence_fetch(f) waits for that copy only, while later frames are in flight.
 * Opt-in: a sequence without a ring issues exactly the launches it issued before the ring existed.
 * The record of frame f (frame 0 is the start): a header (frame, cap, n_live = state[0], n_new, next_id, t), the state and
 * info words, key set f on all `cap` rows (keys, keys_un, keys_normal, index_in_last, live, track_id, age, velocity) and
 * pair (f - 1, f) over the rows of key set f - 1 (status, pt_predict, pt_predict_un, err; all zero for frame 0).  Every array
 * is byte for byte what the three read calls return when called in lock-step after frame f; velocity is zeros unless this is
 * a sensor sequence with flow_velocity; t is the frame's time stamp for a sensor sequence and 0 for a plain one.
 *   track ids  (the library's own definition; the reference has only mvPtIndexInLastFrame, src/frame.cpp:135,192,
 *              include/frame.h:80)  At a start next_id = 0.  For row j of the new key set, with i = index_in_last[j]:
 *                j >= n_live:  track_id = -1, age = 0;
 *                i >= 0:       track_id = track_id_last[i], age = age_last[i] + 1;
 *                otherwise:    track_id = next_id + (the number of rows j' < j with j' < n_live and index_in_last[j'] < 0),
 *                              age = 0.
 *              n_new is the number of rows below n_live with index_in_last < 0; after the frame next_id += n_new, and the
 *              header carries that value.  The rank is a count in row order: new rows need not follow the survivors.  A
 *              restart (pagk_sequence_start called again) begins at 0 again and empties the ring.
 * Groups: the members of a group either all have a ring of one depth or none has; a group step then packs every camera's
 * record in one launch (the camera is the grid's second dimension, from a third table the lead owns) and enqueues one copy
 * and one event per member behind the graph, in front of the event the members' streams wait for.  pagk_sequence_fetch and
 * pagk_sequence_poll on a member keep working while it is grouped.
 * Out of scope: one contiguous record for a whole rig, ids that survive a restart, releasing blocks explicitly,
 * Lucas-Kanade's info words. */
typedef struct pagk_results_layout {
    int64_t header, state, info;                                   /* byte offsets of the parts of a record, in this order, ... */
    int64_t keys, keys_un, keys_normal, index_in_last, live, track_id, age, velocity;
    int64_t status, pt_predict, pt_predict_un, err;                /* ... each a multiple of 256 */
    int64_t bytes;                                                 /* the record's size: the last part's end, rounded up to 256 */
    int32_t cap, sensor;                                           /* what it was asked for */
} pagk_results_layout;
typedef struct pagk_sequence_result {
    int32_t frame, cap, n_live, n_new;   /* the header: the frame's number, the rows of every array, state[0], new tracks */
    int64_t next_id;                     /* the id the next new track gets */
    double t;                            /* sensor sequence: the frame's time stamp; 0 otherwise */
    const int32_t *state, *info;         /* PAGK_HANDOVER_STATE_WORDS and PAGK_DETECT_INFO_WORDS int32 */
    const float *keys, *keys_un, *keys_normal;   /* cap x 2 floats each */
    const int32_t *index_in_last;        /* cap int32 */
    const uint8_t *live;                 /* cap bytes */
    const int64_t *track_id;             /* cap int64: -1 at and beyond n_live */
    const int32_t *age;                  /* cap int32: frames since the track was new */
    const float *velocity;               /* cap x 2 floats */
    const uint8_t *status;               /* pair (frame - 1, frame): cap bytes, ... */
    const float *pt_predict, *pt_predict_un, *err;   /* ... cap x 2, cap x 2 and cap floats */
} pagk_sequence_result;
/* Where the parts of a record lie (no counterpart in the reference: Examples/Demo/RealSenseD435i.cpp:237-321 keeps Frame
 * objects): header | state | info | keys | keys_un | keys_normal | index_in_last | live | track_id | age | velocity | status
 * | pt_predict | pt_predict_un | err, every part on a multiple of 256 bytes.  The header part starts with int32 frame, cap,
 * n_live, n_new, int64 next_id, f64 t.  `sensor` (0 or 1) changes what velocity and t mean, not an offset.  PAGK_E_ARG for
 * cap outside 1 .. PAGK_LK_MAX_ROWS, a sensor flag that is neither, or a NULL layout.  Needs no device. */
int pagk_sequence_results_layout(int32_t cap, int32_t sensor, pagk_results_layout *layout);
/* Gives the context's sequence a result ring of `depth` (2 .. 8) pinned blocks and events (no counterpart in the reference:
 * Examples/Demo/RealSenseD435i.cpp:199-321 has no device to copy from).  Called after pagk_sequence_create[_sensor] and
 * before the first pagk_sequence_start[_sensor].  The parts on the device -- one record, track_id[2][cap] (int64) and
 * age[2][cap] (int32) by parity, next_id -- are a buffer of the context of their own, state and not scratch
 * (pagk_selftest_fill_workspaces leaves them alone); the layout of the sequence's own block does not change.  PAGK_E_ARG with
 * a text in pagk_last_error: without a sequence, for a second call, after a start, while grouped, inside a capture, for a
 * depth out of range.  pagk_sequence_destroy and pagk_destroy free the ring. */
int pagk_sequence_results_create(pagk_ctx *ctx, int32_t depth);
/* The record of frame `frame` (no counterpart in the reference: Examples/Demo/RealSenseD435i.cpp:237-321 reads the Frame it
 * just made): waits for the copy of that frame only, never for the stream, and fills *result with the header's scalars and
 * const views into the pinned block (zero copy).  Valid frames: frames handed in - depth <= frame < frames handed in, frame
 * 0 being the start; PAGK_E_ARG with a text for every other frame, for a frame from before a restart and for a sequence
 * without a ring.  The views stay valid until the call that hands in frame `frame + depth` (which rewrites the block), a
 * restart, or pagk_sequence_destroy.  Works on a member of a group.  Returns the launch-error word as the read calls do. */
int pagk_sequence_fetch(pagk_ctx *ctx, int32_t frame, pagk_sequence_result *result);
/* 1 if the copy of frame `frame` has completed, 0 if not yet (no counterpart in the reference:
 * Examples/Demo/RealSenseD435i.cpp:237-321 is synchronous); nothing is waited for.  PAGK_E_ARG as pagk_sequence_fetch. */
int pagk_sequence_poll(pagk_ctx *ctx, int32_t frame);

/* ---- Lucas-Kanade in the sequence groups: tracker type 0 for k cameras ------------------------------------------------ */
/* The image-only baseline the reference exists to be compared against (tracker type 0, OPENCV_OPTICAL_FLOW_PYR_LK,
 * src/gyro_aided_tracker.cpp:353-380) and its open experiment, Lucas-Kanade started from the gyro prediction (:364-365), for a
 * rig: k contexts on one device, each holding a Lucas-Kanade sequence (tracker PAGK_SEQ_LK), all plain
 * (pagk_sequence_create) or all sensor sequences (pagk_sequence_create_sensor), stepped together.  It lifts Lucas-Kanade from
 * the "Out of scope" list of the plain group and from the "What stays out" list of the sensor group: both arms of the
 * comparison then run through the same machinery.  Per camera, after every frame, every array of pagk_sequence_read and
 * pagk_sequence_read_pair (err included), every array of pagk_sequence_read_velocity of a sensor member and every record of
 * a result ring is byte for byte that of the same sequence stepped alone with the same inputs, in PAGK_SEQ_GRAPH and in
 * PAGK_SEQ_DIRECT.
 * A frame of one Lucas-Kanade camera enqueues a copy of its level 0, one pyrDown launch per pyramid level, a clear of the
 * info words and the flow kernel, which is one wavefront per feature (250 workgroups at 1000 keypoints: a latency chain).  A
 * group step issues each of them ONCE for all cameras, the camera being a dimension of the grid, from a table of its own the
 * lead owns.  The issue order on the lead's stream is that of one Lucas-Kanade sequence, stage by stage:
 *   1. with raw = 1 the rectification of all cameras into their frame slots; otherwise one launch that copies every camera's
 *      frame into its parity copy of level 0 (Lucas-Kanade reads level 0 in place for a whole pair);
 *   2. pagk_frame_set_device_batch on the slots' level 0; the pyrDown levels 1 .. top, one launch per level;
 *   3. for sensor members the gyro integration (always, also when nothing predicts); the prediction when lk_initial_flow;
 *   4. the clear of every camera's info words, then the flow kernel of the rig: one launch of k x ceil(cap / 4) workgroups;
 *   5. the validation on Lucas-Kanade's status when `validate`; the hand-over (with detector 2 the plan and the FAST
 *      detector, every camera under its own skip word); the flow velocities when flow_velocity; the pack of the result
 *      records when the members have rings.  No Step 3 runs: type 0 never enters it.
 * Graph mode follows the groups' rule: the first step runs member by member (that sizes every member's pyramid buffers and,
 * with FAST, its detector workspace), the second as batched launches outside a capture, then each parity is captured at its
 * next step and replayed; a captured step is one linear chain on the lead's stream.
 * pagk_sequence_group_start and pagk_sequence_group_step drive a Lucas-Kanade group of plain members,
 * pagk_sequence_group_start_sensor and pagk_sequence_group_step_sensor one of sensor members, under every rule of those
 * calls (rot9 == NULL only when lk_initial_flow == 0); pagk_sequence_group_status, pagk_sequence_group_destroy and
 * pagk_destroy of a member serve it as they serve the other groups.  What stays out: PatchMatch (the two other group calls
 * serve it), the Harris detector, a mixture of plain and sensor members, cameras whose parameters differ, contexts on
 * different devices. */
/* PAGK_OK iff pagk_sequence_group_create_lk accepts sequences of these blocks (Examples/Demo/RealSenseD435i.cpp:199-321, one
 * loop per camera, with the tracker of src/gyro_aided_tracker.cpp:353-380); s: the sensor block of sensor members, NULL for
 * plain sequences.  pagk_sequence_params_check passes and, with s, pagk_sequence_sensor_check; tracker == PAGK_SEQ_LK,
 * lk_initial_flow 0 or 1; detector == 0 for plain sequences, 0 or 2 (FAST) for sensor sequences; validate, raw and
 * flow_velocity may each be 0 or 1.  PAGK_E_ARG (or the nested check's code) otherwise, so for PatchMatch and the Harris
 * detector.  Needs no device. */
int pagk_sequence_group_lk_check(const pagk_sequence_params *p, const pagk_sequence_sensor *s);
/* Makes ctxs[0 .. k-1] a group of Lucas-Kanade sequences (Examples/Demo/RealSenseD435i.cpp:199-321, the objects k loops keep
 * between frames; src/gyro_aided_tracker.cpp:353-380 is their tracker); ctxs[0] is the lead, and the kind of the group, plain
 * or sensor, follows from the members.  Refuses, with a text in pagk_last_error(ctxs[0]), everything
 * pagk_sequence_group_create refuses but the sensor sequence (parameters that are not byte-equal, sensor blocks that differ
 * in anything but Rbc and result rings of different depths among them), a mixture of plain and sensor members, and
 * parameters that pagk_sequence_group_lk_check refuses.  While grouped a member's own start, step and destroy calls return
 * PAGK_E_ARG and its read calls keep working.  Calls outside the group that move a member's pyramid buffers
 * (pagk_lk_pyramid_device with a deeper max_level on slot 0 or 1), its frame slots or its sequence invalidate the tables
 * like those the other groups name: the next step returns PAGK_E_ARG and the group has to be destroyed. */
int pagk_sequence_group_create_lk(pagk_ctx *const *ctxs, int32_t k);

#ifdef __cplusplus
}
#endif
#endif /* PAGK_H */
