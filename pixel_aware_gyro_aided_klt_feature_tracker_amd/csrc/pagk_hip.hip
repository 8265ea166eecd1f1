// pagk_hip.hip -- C ABI (include/pagk.h) over the gfx950 kernels.  Host side of the boundary.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared  (see __graft_entry__.py)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/pagk.h"
#include "pagk_kernels.h"
#include "pagk_inverse_kernel.h"
#include "pagk_associate_kernel.h"
#include "pagk_pose_kernel.h"
#include "pagk_orb_levels_kernel.h"
#include "pagk_gyro_kernel.h"
#include "pagk_group_kernel.h"
#include "pagk_group_sensor_kernel.h"
#include "pagk_group_lk_kernel.h"
#include "pagk_results_kernel.h"
#include "pagk_layout.h"
#include "pagk_select.h"
#include "pagk_prio_env.h"
#include "pagk_order.h"

using namespace pagk;

namespace {

constexpr int kSlots = 6;        // 0..3 for the caller, 4/5 = scratch pair of the host-buffer path
constexpr int kUserSlots = 4;

// A device buffer the library owns: it only ever grows, through reserve(), and is freed by pagk_destroy.
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    void *host = nullptr;   // `mirrored` buffers: pinned host memory of the same size (one copy in, one copy out)
    bool mirrored = false;
    bool state = false;     // holds state with set / reset calls of its own, not scratch: pagk_selftest_fill_workspaces leaves it alone
};

struct FrameSlot {
    int w = 0, h = 0, L = 0;
    int wrap0 = 1;                   // level-0 source was continuous (step == cols)
    int pad0 = 0;                    // min(step - cols, 2) of the level-0 source (free GetPixelValue, x == cols)
    uint8_t *u8[kMaxLevels] = {};    // u8[0] is our contiguous copy of level 0 (pitch = w)
    uint32_t *quad[kMaxLevels] = {};
    const uint8_t *img0 = nullptr;   // level 0 where the pyramid was built from (our copy, or the caller's device image
    int64_t pitch0 = 0;              // read in place): what the corner detector reads (pagk_detect_kernel.h)
    DevBuf block;                    // one allocation for everything above
    bool valid = false;
};

// The sequence a context owns (pagk_sequence_*): its parameters, typed views into buf[SEQ], the pinned input ring and where
// the loop stands.  Everything the steps launch on is in buf[SEQ]; the pointers below are fixed from create to destroy.
struct SeqState {
    pagk_sequence_params p;
    size_t in_bytes = 0, off_rot = 0, off_ncand = 0, off_cand = 0;   // the input block: image | rot9 | n_cand | candidates
    uint8_t *in = nullptr;        // the fixed device input block
    uint8_t *img[2] = {};         // Lucas-Kanade: each parity's own copy of its frame (level 0 is read in place)
    struct KeySet {
        float *keys, *keys_un, *keys_normal;
        int32_t *index_in_last;
        uint8_t *live;
    } set[2] = {};
    uint8_t *work = nullptr;      // the work arrays, zeroed by start
    size_t work_bytes = 0;
    float *pu = nullptr, *pd = nullptr, *aff = nullptr, *pt_un = nullptr, *pt_dist = nullptr, *pp = nullptr, *ppu = nullptr;
    float *score = nullptr, *lk_err = nullptr;
    uint8_t *st_in = nullptr, *status = nullptr, *st = nullptr, *zero = nullptr;
    double *pix_err = nullptr, *dist_pred = nullptr, *th = nullptr;
    int32_t *kept = nullptr, *cnt = nullptr, *state = nullptr, *info = nullptr, *lk_info = nullptr;
    static constexpr int kRing = 4;   // pinned input blocks: one is rewritten only after the copy that read it has run
    void *pinned[kRing] = {};
    hipEvent_t read_done[kRing] = {};
    bool recorded[kRing] = {};
    int turn = 0, frames = 0;
    bool started = false, stepped = false, last_graph = false, direct_done[2] = {};
    int graph[2] = {-1, -1};
    // the sensor form (pagk_sequence_create_sensor): raw frames and the IMU window are parts of the input block
    bool sensor = false;
    pagk_sequence_sensor s = {};
    size_t row_bytes = 0;         // bytes of a frame row in the input block (raw: src_width * channels), and ...
    int rows = 0;                 // ... its rows
    size_t off_win = 0;           // the window in the input block (kImuWindowBytes)
    const float *rot = nullptr;   // what the prediction reads: the caller's nine floats in the input block, or k_gyro_integrate's
    float *rot_out = nullptr, *rcl = nullptr, *vel = nullptr;   // sensor parts: rot9 | Rcl, the flow velocities
    double t_last = 0.0;          // the previous frame's time
    // the result ring (pagk_sequence_results_create; depth 0: none): the device parts lie in buf[RESULTS], the blocks are pinned
    struct Results {
        static constexpr int kMaxDepth = 8;
        int depth = 0;
        size_t bytes = 0;             // of a record
        uint8_t *rec = nullptr;       // the record the pack writes
        int64_t *id[2] = {}, *next[2] = {};   // by parity: track ids, next_id
        int32_t *age[2] = {};
        void *pinned[kMaxDepth] = {};
        hipEvent_t copied[kMaxDepth] = {};
        int frame_of[kMaxDepth] = {};   // the frame whose copy the block's event stands behind (-1: none)
    } res;
    bool ever_started = false;
};

// The sequence group of k contexts (pagk_sequence_group_*): every member's ctx->group points here, members[0] is the lead and
// owns it -- its stream carries the steps, its graph slots hold the group's two graphs, its buf[GROUP] the argument table of
// the batched small kernels (pagk_group_kernel.h): record [parity * k + camera].
struct GroupState {
    std::vector<pagk_ctx *> members;
    bool members_done = false;   // one step has run member by member: every member's workspaces have their final size
    bool batched_done = false;   // one step has run as batched launches outside a capture: so have the lead's
    bool direct_done[2] = {}, last_graph = false, table_built = false;
    int graph[2] = {-1, -1};
    // The group's kind: k sensor sequences (pagk_sequence_group_create_sensor).  The lead's buf[GROUP_SENSOR] then holds a
    // second table, of the stages a sensor step adds (pagk_group_sensor_kernel.h): record [parity * k + camera].
    bool sensor = false;
    // every member has a result ring (of one depth): the lead's buf[GROUP_RESULTS] holds a third table, of k_group_results_pack
    bool rings = false;
    // every member tracks with Lucas-Kanade (pagk_sequence_group_create_lk; plain or sensor members): the lead's buf[GROUP_LK]
    // holds the table of the Lucas-Kanade stages (pagk_group_lk_kernel.h): record [parity * k + camera]
    bool lk = false;
    int n_cells = 0;             // (detector 2) the cells of the FAST grid, the same for every member
    // what the tables were built from, per member: a workspace that moved since then invalidates them
    struct Held {
        const void *fit, *hand, *hint;
        size_t hint_bytes;
        // the sensor group's: the FAST workspace, the map entries, both frame slots' level 0, the sequence's block
        const void *fast, *entries, *level0[2], *seq;
        int rect_w, rect_h, rect_wp;
        const void *results;   // with result rings: the member's buf[RESULTS] and its sequence's block (the third table)
        const void *results_seq;
        // the Lucas-Kanade group's: the pyrDown levels of slots 0 and 1 (the parity copies of level 0 lie in the sequence's
        // block, the rectified ones in the frame slots: `seq` and `level0`)
        const void *lk_pyr[2];
        size_t lk_pyr_bytes[2];
    };
    std::vector<Held> held;
};

}  // namespace

struct pagk_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    FrameSlot slots[kSlots];
    // Every buffer that grows with the calls (DESIGN.md section 2 has the table: what sizes it, when it may grow).
    // pagk_destroy frees them in one loop: a new one is a new name in front of kBufs.
    enum Buf {
        FEAT,          // the per-feature arrays of the host-buffer tracking path, and their pinned mirror
        SCORE,         // scratch of the host-buffer geometry scoring and neighbour paths
        FIT,           // workspace of the device RANSAC fits (pagk_fit_kernel.h): sized for fit_n correspondences and fit_iters hypotheses
        FITIO,         // scratch of the host-buffer fit / validation entry points
        HAND,          // the frame hand-over's own mask (pagk_handover_kernel.h)
        HANDIO,        // scratch of the host-buffer hand-over
        DET,           // workspace of the corner detector (pagk_detect_kernel.h)
        FAST,          // workspace of the FAST detector (pagk_fast_kernel.h): sized by W, H and n_features
        RECT_ENTRIES,  // rectification (pagk_rectify_kernel.h): the packed map entries of pagk_rectify_set_maps
        RECT_STAGE,    // ... and the staging buffer of a raw frame that arrives from the host
        ORB_PATTERN,   // ORB (pagk_orb_kernel.h): the sampling pattern of pagk_orb_set_pattern, 1024 int32
        ORB_BLUR,      // ... the blurred image of the slot being described: sized by W and H
        ORB_KEYS,      // ... the matcher's best-match keys: sized by cap_q
        LK_PYR,        // Lucas-Kanade (pagk_lk_kernel.h): the pyrDown levels of slot 0 ...
        LK_PYR_LAST = LK_PYR + kSlots - 1,   // ... to slot kSlots - 1, each sized by W, H and the top level
        ORBL_WS,       // ORB over a scale pyramid (pagk_orb_levels_kernel.h): a slice per level -- the FAST workspace, the blurred level, the level's keypoint segment
        ORBL_PYR,      // ... the resized levels 1 .. of slot 0 ...
        ORBL_PYR_LAST = ORBL_PYR + kSlots - 1,   // ... to slot kSlots - 1, each sized by the level table
        ORBL_SET,      // ... the packed keypoint set of slot 0 ...
        ORBL_SET_LAST = ORBL_SET + kSlots - 1,   // ... to slot kSlots - 1, each sized by the table's out_bound
        ORBL_MATCH,    // ... the match result of query slot 0 ...
        ORBL_MATCH_LAST = ORBL_MATCH + kSlots - 1,   // ... to slot kSlots - 1, each sized by the query set's capacity
        ASSOC,         // track-to-detection association (pagk_associate_kernel.h): choices and claims, sized by n and m
        POSE,          // workspace of the two-view pose (pagk_pose_kernel.h): sized for pose_n correspondences and pose_iters hypotheses
        POSEIO,        // scratch of the host-buffer pose entry point
        QUAD_WS,       // k_track_quad: iteration-invariant img1 samples, 4 * NCH * 64 floats per wave
        SUSP,          // continuation buffers: int count (256 B) | int list[n] | SuspState state[n]
        LV,            // one-level-per-wave launches: levels_layout (pagk_layout.h)
        PRIO_HINT,     // the 4-wave kernels' hint (pagk_prio.h): one int32 per feature slot of the largest launch so far
        DISPATCH_ORDER,  // ... and their dispatch order (pagk_order.h): one int32 per feature slot, beside the hints
        SEQ,           // the sequence the context owns (pagk_sequence_*): input block, two key sets, work arrays, state and info words
        GROUP,         // the sequence group this context leads (pagk_sequence_group_*): the argument table of its batched kernels, 2 k records
        GROUP_SENSOR,  // ... of k sensor sequences (pagk_sequence_group_*_sensor): the table of the stages they add, 2 k records
        RESULTS,       // the result ring of the sequence (pagk_sequence_results_create): one record, track ids and ages by parity, next_id
        GROUP_RESULTS, // ... of a group whose members have rings: the table of k_group_results_pack, 2 k records
        GROUP_LK,      // ... of a group of Lucas-Kanade sequences (pagk_sequence_group_create_lk): the table of pagk_group_lk_kernel.h, 2 k records
        kBufs
    };
    DevBuf buf[kBufs];
    int fit_n = 0, fit_iters = 0;  // what buf[FIT]'s layout was computed for
    int pose_n = 0, pose_iters = 0;  // ... and buf[POSE]'s
    int rect_w = 0, rect_h = 0, rect_wp = 0;
    bool orb_pattern_set = false;
    struct LkPyr { int w = 0, h = 0, top = -1; } lk_pyr[kSlots];   // what buf[LK_PYR + slot] holds (top -1: nothing)
    // what buf[ORBL_PYR + slot], buf[ORBL_SET + slot] and buf[ORBL_MATCH + slot] hold (n_levels 0, cap 0: nothing)
    struct OrbLevelsSlot {
        int w = 0, h = 0, n_levels = 0;
        int lw[kOrbMaxLevels] = {}, lh[kOrbMaxLevels] = {};
        int cap = 0;             // rows of the keypoint set
        bool described = false;  // the set has angles and descriptors (pagk_orb_extract_slot, not the detect form)
        int match_cap = 0;       // rows of the match result with this slot as the query
    } orbl[kSlots];
    void *queue = nullptr;    // k_track_rows: the work-queue counter (256 B)
    // per half patch (0 = not asked yet), the resident waves (occupancy x CUs) on this device of ...
    int quad_capacity[PAGK_MAX_HALF_PATCH + 1] = {};  // ... the generic whole-feature k_track_quad: the hand-over rule's "round"
    int rows_capacity[PAGK_MAX_HALF_PATCH + 1] = {};  // ... k_track_rows
    int rows_waves_cap = 0;            // PAGK_ROWS_WAVES: upper bound of that grid (tests: a small grid, a long queue)
    int *susp_count_dev = nullptr;  // the hand-over count of the last launch that used one (in buf[SUSP] or in buf[LV])
    // pagk_track_device_batch (lead context): the BatchStream array of a launch and its pinned source.  The copy to the
    // device is asynchronous, and a captured copy is replayed long after the call: a pair is therefore never rewritten
    // while something may still read it.  Direct launches take the pairs of a ring in turn (a pair is reused six calls
    // later, after waiting for the launch that used it); a capture takes pairs that pagk_graph_begin reserved for it and
    // that belong to the graph from then on (freed by pagk_graph_destroy).  Every pair holds the maximum of 64 streams.
    struct BatchDesc {
        void *host = nullptr, *dev = nullptr;
        hipEvent_t used = nullptr;   // recorded behind the launch that read `dev`
        bool recorded = false;
    };
    static constexpr int kBatchRing = 6, kBatchPerCapture = 4, kBatchMaxStreams = 64;
    BatchDesc batch_ring[kBatchRing];
    int batch_turn = 0;
    bool batch_seen = false;                 // this context has led a batched launch: captures reserve pairs
    std::vector<BatchDesc> cap_batch;        // reserved for the running capture
    int cap_batch_used = 0;
    hipEvent_t ev_batch = nullptr;  // orders a batched launch against the streams of the contexts it serves
    int *lv_error = nullptr;  // mapped host memory: a wave of such a launch gave up waiting (never expected; checked at syncs)
    int *lv_error_dev = nullptr;  // ... as the device addresses it
    hipStream_t aux_stream = nullptr;  // the live finisher's stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int susp_lone = 1;        // PAGK_SUSPEND_LONE=0: hand every feature over at the budget, not only the last of a wave
    int finisher_wgs = 16;    // PAGK_FINISHER_WGS: workgroups of the live finisher (0: sweep only)
    int finisher_polls = 20000;  // PAGK_FINISHER_POLLS: bounded wait of a finisher workgroup (~2 us per look: ~35 ms,
                                 // an order of magnitude beyond the longest launch the hand-over rule admits)
    int level_polls = 300000;  // PAGK_LEVEL_POLLS: bounded wait of a one-level-per-wave item for its ready-list entry (~1 s: far beyond any launch, also on a time-sliced device)
    int quad_budget = -1;     // iterations a feature may run in the four-features-per-wave kernel before it is handed to
                              // the latency kernel; 0: never; -1 (default): chosen per launch, see quad_budget_for().
                              // PAGK_QUAD_BUDGET overrides.
    int cus = 0;              // compute units of the device
    // hipGraph capture of the per-frame work (pagk_graph_*): while capturing, nothing may allocate and the
    // timing events are left out (an event recorded into a graph cannot be read back)
    bool capturing = false;
    // pagk_selftest_fill_workspaces(word, also_new != 0): every block allocated from now on starts as `fill_word`
    bool fill_new = false;
    uint32_t fill_word = 0;
    static constexpr int kGraphs = 8;
    hipGraph_t graphs[kGraphs] = {};
    hipGraphExec_t graph_execs[kGraphs] = {};
    // A captured step that contains a launch with the LIVE finisher is replayed in segments (round 4): HIP replays the
    // parallel branches of one graph one after the other, so the finisher -- which must run BESIDE the throughput kernel --
    // is not a node: the capture is closed in front of that kernel, the finisher is remembered as a plain launch on the
    // auxiliary stream, the capture reopens.  graph_execs[k] is the LAST segment; pre_segs[k] what runs before it.
    struct GraphSeg {
        enum Kind { GRAPH, FINISHER, JOIN } kind = GRAPH;
        hipGraph_t g = nullptr;
        hipGraphExec_t ex = nullptr;
        const void *fn = nullptr;   // FINISHER: k_track_resume_live<..>, its arguments and launch shape
        TrackArgs args;
        int grid = 0;
        size_t lds = 0;
    };
    std::vector<GraphSeg> pre_segs[kGraphs];
    std::vector<BatchDesc> graph_batch[kGraphs];   // the descriptor pairs graph k's batched launches read
    std::vector<GraphSeg> cap_segs;   // segments closed so far in the capture that is open
    hipEvent_t ev_trk[2] = {}, ev_pyr[2] = {};
    bool trk_timed = false, pyr_timed = false;
    int kernel = 0;
    bool last_handover = false;  // the last tracking launch used the hand-over (pagk_last_handover)
    int concurrency = 1;    // pagk_set_concurrency: contexts like this one running at the same time on the device
    int last_variant = -1;  // variant the last tracking launch used (pagk_last_variant)
    // auto-selection thresholds (the rule that applies them: select_variant in pagk_select.h, as a table in DESIGN.md
    // section 4.3), measured on MI355X at h = 10 (tools/sweep_n.py, profiles/r03_sweep_n.log): after round
    // 3's instruction diet the 4-wave DPP kernel is the fastest up to ~5000 features (it used to lose to the 2-wave MFMA
    // variant from 2500; that variant no longer wins at any size and is selected explicitly only), one wave per feature
    // wins between ~5000 and ~7000, four features per wave from there.  Later in round 3: four features per wave with
    // one pyramid level per wave (variant 7) is the fastest from ~6000 features for a context alone on the device
    // (profiles/r03_levels_sweep.log); contexts that share the device (pagk_set_concurrency) keep the sequence above.
    int mfma_min_features = 0x7fffffff;  // PAGK_MFMA_MIN
    int wave_min_features = 6000;        // PAGK_WAVE_MIN (5000 until the 4-wave kernel had its build for five workgroups per CU)
    int quad_min_features = 7000;        // PAGK_QUAD_MIN: four features per wave (pagk_quad_kernel.h)
    int block5_min_features = 2500;      // PAGK_BLOCK5_MIN: the 4-wave kernel in its five-workgroups-per-CU build (h = 10)
    int prio_k = 4;                      // PAGK_PRIO_K: iterations per pyramid level beyond which a 4-wave workgroup counts as behind (pagk_prio.h); 0 = rule off
    unsigned long long *prio_stats = nullptr;  // PAGK_PRIO_K=auto: device block [iterations, feature-levels (u64 each), K (int)]
    int prio_hint_t = kPrioHintDefault;  // PAGK_PRIO_HINT: a feature slot whose previous launch ran more iterations than this starts behind (pagk_prio.h); 0 = hint off
    bool graph_order[kGraphs] = {};      // graph k holds a build or a reader of the dispatch order (pagk_order.h: its replays bind the array)
    OrderState order;                    // PAGK_DISPATCH_ORDER: the 4-wave launches' dispatch order, and when a launch may use it (pagk_order.h)
    bool block5_window = true;           // ... also for launches that only five workgroups per CU hold in one round (off when PAGK_BLOCK5_MIN is set)
    int levels_min_features = 6000;      // PAGK_LEVELS_MIN: ... one level per wave (a context alone on the device)
    int levels_shift = 0;                // PAGK_LEVELS_XCD_SHIFT (tests): waves start with another XCD's ticket sequence
    bool levels_shared = false;          // PAGK_LEVELS_SHARED=1 (measurement): ... also for contexts that share the device
    bool unfused_pyramid = false;  // PAGK_UNFUSED_PYRAMID=1: level-by-level launches (cross-check)
    SeqState *seq = nullptr;       // pagk_sequence_create .. pagk_sequence_destroy
    GroupState *group = nullptr;   // pagk_sequence_group_create .. pagk_sequence_group_destroy: the group this context is a member of
    char err[256] = {0};
};

namespace {

#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s:%d %s -> %s", __FILE__, __LINE__, #call,     \
                     hipGetErrorString(e_));                                                           \
            return e_ == hipErrorOutOfMemory ? PAGK_E_NOMEM : PAGK_E_HIP;                              \
        }                                                                                              \
    } while (0)

// Entry points that copy from / to host memory or synchronise cannot be part of a graph capture.
#define NOT_WHILE_CAPTURING(ctx, what)                                                                 \
    do {                                                                                               \
        if ((ctx)->capturing) {                                                                        \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s is not capturable: use the *_device entry points between pagk_graph_begin and pagk_graph_end", what); \
            return PAGK_E_ARG;                                                                         \
        }                                                                                              \
    } while (0)

int level_dims(int w, int h, int L, int *lw, int *lh)
{
    lw[0] = w;
    lh[0] = h;
    for (int l = 1; l < L; l++) {
        // src/patch_match.cpp:69  cv::Size(cols * 0.5, rows * 0.5)
        lw[l] = (int)(lw[l - 1] * 0.5);
        lh[l] = (int)(lh[l - 1] * 0.5);
        if (lw[l] < 1 || lh[l] < 1) return PAGK_E_ARG;
    }
    return PAGK_OK;
}

// Is this context's work being recorded rather than executed?  Its own capture (pagk_graph_begin), or a capture of
// the stream it was switched to by somebody else -- another context of a batch (pagk_track_device_batch), the host
// application's own hipStreamBeginCapture.  Nothing may allocate then, and timing events are left out.
bool in_capture(pagk_ctx *ctx)
{
    if (ctx->capturing) return true;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(ctx->stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone;
}

// Library-owned device buffers that captured graphs point into may only be reallocated while no instantiated graph of
// this context is alive: the caller destroys its graphs (pagk_graph_destroy), or does what `hint` says BEFORE capturing,
// as include/pagk.h asks.
int no_live_graphs(pagk_ctx *ctx, const char *what, const char *hint)
{
    for (int k = 0; k < pagk_ctx::kGraphs; k++)
        if (ctx->graph_execs[k]) {
            snprintf(ctx->err, sizeof(ctx->err), "%s would have to grow while graph %d of this context is alive (its nodes hold the old "
                     "pointers): destroy the graph first, or %s", what, k, hint);
            return PAGK_E_ARG;
        }
    return PAGK_OK;
}

// When a buffer may grow.  One that the nodes of a captured graph point into (memsets, kernel arguments) must not move
// under that graph: nothing allocates while a capture records, and replaying a graph after its buffers moved would write
// freed memory.  GROW_FREELY is for the scratch of host-buffer entry points, which NOT_WHILE_CAPTURING keeps out of
// captures and which no graph can therefore point into.
enum GrowPolicy {
    GROW_FREELY = 0,
    NOT_IN_CAPTURE = 1,     // PAGK_E_ARG inside a capture
    NOT_UNDER_GRAPH = 2,    // PAGK_E_ARG while a graph of this context is alive
    NOT_IN_CAPTURE_NOR_UNDER_GRAPH = NOT_IN_CAPTURE | NOT_UNDER_GRAPH,
};

int release(pagk_ctx *ctx, DevBuf &b)
{
    if (b.ptr) HIPCHK(ctx, hipFree(b.ptr));
    if (b.host) HIPCHK(ctx, hipHostFree(b.host));
    b.ptr = b.host = nullptr;
    b.bytes = 0;
    return PAGK_OK;
}

// `bytes` at p become the 32-bit `word` (a tail that is no whole word: its low byte), in stream order
int fill_words(pagk_ctx *ctx, void *p, size_t bytes, uint32_t word)
{
    const size_t words = bytes / 4, tail = bytes % 4;
    if (p && words) HIPCHK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)word, words, ctx->stream));
    if (p && tail) HIPCHK(ctx, hipMemsetAsync(static_cast<uint8_t *>(p) + 4 * words, (int)(word & 0xff), tail, ctx->stream));
    return PAGK_OK;
}
// ... and of a pinned mirror, by the host (nothing is queued on a mirror when this is called)
void fill_words_host(void *p, size_t bytes, uint32_t word)
{
    uint8_t *b = static_cast<uint8_t *>(p);
    for (size_t i = 0; p && i < bytes; i++) b[i] = i < bytes / 4 * 4 ? (uint8_t)(word >> (8 * (i % 4))) : (uint8_t)word;
}

// Room for `bytes` in `b`: a buffer that is too small is freed and allocated anew (its content is scratch), and is left
// empty when that fails.  `what` names the buffer in ctx->err, `hint` is what the caller does instead of growing it here.
int reserve(pagk_ctx *ctx, DevBuf &b, size_t bytes, GrowPolicy policy, const char *what, const char *hint = "")
{
    if (bytes <= b.bytes) return PAGK_OK;
    if ((policy & NOT_IN_CAPTURE) && in_capture(ctx)) {
        snprintf(ctx->err, sizeof(ctx->err), "%s would have to grow inside a graph capture: %s", what, hint);
        return PAGK_E_ARG;
    }
    int rc = (policy & NOT_UNDER_GRAPH) ? no_live_graphs(ctx, what, hint) : PAGK_OK;
    if (rc || (rc = release(ctx, b))) return rc;
    HIPCHK(ctx, hipMalloc(&b.ptr, bytes));
    if (b.mirrored) HIPCHK(ctx, hipHostMalloc(&b.host, bytes, hipHostMallocDefault));
    b.bytes = bytes;
    if (ctx->fill_new) {   // (selftest only: the new block does not start as the allocator left it)
        fill_words_host(b.host, bytes, ctx->fill_word);
        return fill_words(ctx, b.ptr, bytes, ctx->fill_word);
    }
    return PAGK_OK;
}

// One synchronous host-buffer call: a device block carved into N parts, inputs copied in, the device form's launches,
// outputs copied out, one synchronisation.  The block is a context buffer (`keep`, grown freely) or the call's own, freed
// with the object.  The host side of a queued copy is a caller's array or a local of the entry point, so no path returns
// with a copy pending: an object that dies with copies queued and finish() not reached synchronises first.  Declare the
// locals that copies read or write in front of the object.
template <int N>
class Staged {
public:
    Staged(pagk_ctx *ctx, const size_t (&sizes)[N]) : ctx_(ctx), lay_(sizes) {}
    Staged(const Staged &) = delete;
    Staged &operator=(const Staged &) = delete;
    ~Staged()
    {
        if (pending_) (void)hipStreamSynchronize(ctx_->stream);
        if (own_) (void)hipFree(own_);
    }
    int open(DevBuf *keep, const char *what)
    {
        if (keep) {
            int rc = reserve(ctx_, *keep, lay_.total, GROW_FREELY, what);
            base_ = keep->ptr;
            return rc;
        }
        HIPCHK(ctx_, hipMalloc(&own_, lay_.total));
        base_ = own_;
        return ctx_->fill_new ? fill_words(ctx_, own_, lay_.total, ctx_->fill_word) : PAGK_OK;
    }
    template <class T>
    T *at(int k) const { return lay_.template at<T>(base_, k); }
    // queue a copy into / out of part k; nothing when the host array is NULL or there are no bytes
    int in(int k, const void *src, size_t bytes) { return copy(at<void>(k), src, bytes, hipMemcpyHostToDevice); }
    int out(int k, void *dst, size_t bytes) { return copy(dst, at<void>(k), bytes, hipMemcpyDeviceToHost); }
    int finish()
    {
        pending_ = false;
        HIPCHK(ctx_, hipStreamSynchronize(ctx_->stream));
        return PAGK_OK;
    }

private:
    int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
    {
        if (!dst || !src || !bytes) return PAGK_OK;
        pending_ = true;
        HIPCHK(ctx_, hipMemcpyAsync(dst, src, bytes, kind, ctx_->stream));
        return PAGK_OK;
    }
    pagk_ctx *ctx_;
    Layout<N> lay_;
    void *base_ = nullptr, *own_ = nullptr;
    bool pending_ = false;
};

// Close the open capture segment of pagk_graph_begin (what was recorded so far becomes one instantiated graph in
// ctx->cap_segs) and open the next one.  Used around a launch whose finisher must not be a graph node.
int capture_split(pagk_ctx *ctx)
{
    hipGraph_t g = nullptr;
    HIPCHK(ctx, hipStreamEndCapture(ctx->stream, &g));
    if (g) {
        pagk_ctx::GraphSeg seg;
        hipError_t e = hipGraphInstantiate(&seg.ex, g, nullptr, nullptr, 0);
        if (e != hipSuccess) {
            (void)hipGraphDestroy(g);
            ctx->capturing = false;
            (void)ctx->order.capture_ended();
            snprintf(ctx->err, sizeof(ctx->err), "hipGraphInstantiate (segment) -> %s", hipGetErrorString(e));
            return PAGK_E_HIP;
        }
        seg.g = g;
        ctx->cap_segs.push_back(seg);
    }
    hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
        ctx->capturing = false;
        (void)ctx->order.capture_ended();
        snprintf(ctx->err, sizeof(ctx->err), "hipStreamBeginCapture (next segment) -> %s", hipGetErrorString(e));
        return PAGK_E_HIP;
    }
    return PAGK_OK;
}
void destroy_segs(std::vector<pagk_ctx::GraphSeg> &v)
{
    for (auto &sg : v) {
        if (sg.ex) (void)hipGraphExecDestroy(sg.ex);
        if (sg.g) (void)hipGraphDestroy(sg.g);
    }
    v.clear();
}

int batch_desc_alloc(pagk_ctx *ctx, pagk_ctx::BatchDesc &d)
{
    // (one size for both users: the BatchStream array of a tracking launch, the PyrBatchEntry array of a pyramid launch)
    static_assert(sizeof(PyrBatchEntry) <= sizeof(BatchStream), "a descriptor pair is sized by the larger record");
    const size_t bytes = (size_t)pagk_ctx::kBatchMaxStreams * sizeof(BatchStream);
    HIPCHK(ctx, hipMalloc(&d.dev, bytes));
    HIPCHK(ctx, hipHostMalloc(&d.host, bytes, hipHostMallocDefault));
    HIPCHK(ctx, hipEventCreateWithFlags(&d.used, hipEventDisableTiming));
    d.recorded = false;
    return PAGK_OK;
}
void batch_desc_free(pagk_ctx::BatchDesc &d)
{
    if (d.dev) (void)hipFree(d.dev);
    if (d.host) (void)hipHostFree(d.host);
    if (d.used) (void)hipEventDestroy(d.used);
    d = pagk_ctx::BatchDesc();
}
void batch_desc_free(std::vector<pagk_ctx::BatchDesc> &v)
{
    for (auto &d : v) batch_desc_free(d);
    v.clear();
}

// The descriptor pair of the batched launch `lead` is about to issue: the next of the ring (after waiting for the launch
// that used it last), or -- inside lead's own capture -- the next of those pagk_graph_begin reserved.  nullptr: *rc, lead->err.
pagk_ctx::BatchDesc *batch_desc_take(pagk_ctx *lead, int *rc)
{
    *rc = PAGK_OK;
    if (in_capture(lead)) {
        if (!lead->capturing || lead->cap_batch_used >= (int)lead->cap_batch.size()) {
            snprintf(lead->err, sizeof(lead->err), "a batched launch inside a graph capture needs descriptor buffers reserved by pagk_graph_begin of "
                     "ctxs[0]: issue the batched call once before capturing, capture through pagk_graph_begin(ctxs[0]), at most %d batched calls per capture",
                     pagk_ctx::kBatchPerCapture);
            *rc = PAGK_E_ARG;
            return nullptr;
        }
        return &lead->cap_batch[lead->cap_batch_used++];
    }
    pagk_ctx::BatchDesc *desc = &lead->batch_ring[lead->batch_turn];
    lead->batch_turn = (lead->batch_turn + 1) % pagk_ctx::kBatchRing;
    if (!desc->dev) {
        if ((*rc = batch_desc_alloc(lead, *desc)) != PAGK_OK) {
            batch_desc_free(*desc);
            return nullptr;
        }
    } else if (desc->recorded) {
        if (hipEventSynchronize(desc->used) != hipSuccess) {   // (the launch a ring's length ago)
            snprintf(lead->err, sizeof(lead->err), "hipEventSynchronize of a batch descriptor's last user failed");
            *rc = PAGK_E_HIP;
            return nullptr;
        }
    }
    lead->batch_seen = true;
    return desc;
}
// ... and behind that launch: from here on the pair is busy until the launch is over
int batch_desc_used(pagk_ctx *lead, pagk_ctx::BatchDesc *desc)
{
    if (in_capture(lead)) return PAGK_OK;   // (the graph owns it)
    HIPCHK(lead, hipEventRecord(desc->used, lead->stream));
    desc->recorded = true;
    return PAGK_OK;
}

// A slot's block for levels of lw[l] x lh[l] pixels: the u8 levels, then their packed taps
int slot_alloc(pagk_ctx *ctx, FrameSlot &s, const int *lw, const int *lh, int L, GrowPolicy policy)
{
    size_t sizes[2 * kMaxLevels];
    for (int l = 0; l < L; l++) {
        sizes[l] = (size_t)lw[l] * lh[l];
        sizes[L + l] = sizes[l] * 4;
    }
    const Layout<2 * kMaxLevels> lay(sizes, 2 * L);
    int rc = reserve(ctx, s.block, lay.total, policy, "the frame slot", "run the same calls once before pagk_graph_begin");
    if (rc) return rc;
    for (int l = 0; l < L; l++) {
        s.u8[l] = lay.at<uint8_t>(s.block.ptr, l);
        s.quad[l] = lay.at<uint32_t>(s.block.ptr, L + l);
    }
    s.w = lw[0];
    s.h = lh[0];
    s.L = L;
    return PAGK_OK;
}

int slot_reserve(pagk_ctx *ctx, FrameSlot &s, int w, int h, int L)
{
    int lw[kMaxLevels], lh[kMaxLevels];
    int rc = level_dims(w, h, L, lw, lh);
    return rc ? rc : slot_alloc(ctx, s, lw, lh, L, NOT_IN_CAPTURE);
}

// How a launch that is about to be enqueued is recorded, for the order's rule: 0 executed, 1 into pagk_graph_begin's capture (the
// graph dies in pagk_graph_destroy), 2 into somebody else's capture of the stream (nobody tells us when that graph dies).
int capture_kind(pagk_ctx *ctx) { return ctx->capturing ? 1 : (in_capture(ctx) ? 2 : 0); }

// The order workgroup of the pyramid launch that is about to be enqueued on ctx->stream: n = 0 for none.
OrderArgs order_build_args(pagk_ctx *ctx)
{
    const DevBuf &hb = ctx->buf[pagk_ctx::PRIO_HINT], &ob = ctx->buf[pagk_ctx::DISPATCH_ORDER];
    const int n = ctx->order.build_n(ctx->stream, ctx->cus, (long long)(hb.bytes / sizeof(int32_t)), (long long)(ob.bytes / sizeof(int32_t)), capture_kind(ctx));
    return {static_cast<const int *>(hb.ptr), static_cast<int *>(ob.ptr), n};
}

// Arguments of the single-launch pyramid (k_pyramid_fused / the trailing blocks of k_track_block_pyr) for a
// reserved slot with at most 4 levels and even parents; returns the number of 256-thread blocks.
int make_pyr_args(const FrameSlot &s, const uint8_t *src0, int64_t pitch0, int wrap0, PyrArgs *out)
{
    int lw[kMaxLevels], lh[kMaxLevels];
    level_dims(s.w, s.h, s.L, lw, lh);
    PyrArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.src = src0;
    pa.pitch = pitch0;
    pa.wrap0 = wrap0;
    pa.n_levels = s.L;
    int nb = 0;
    for (int l = 0; l < 4; l++) {
        pa.first_block[l] = nb;
        if (l < s.L) {
            pa.cols[l] = lw[l];
            pa.rows[l] = lh[l];
            pa.u8[l] = s.u8[l];
            pa.quad[l] = s.quad[l];
            nb += (lw[l] * lh[l] + 255) / 256;
        }
    }
    pa.first_block[4] = nb;
    for (int l = s.L; l < 4; l++) pa.first_block[l] = nb;  // empty ranges for absent levels
    *out = pa;
    return nb;
}

bool pyramid_fusable(const FrameSlot &s)
{
    int lw[kMaxLevels], lh[kMaxLevels];
    level_dims(s.w, s.h, s.L, lw, lh);
    bool all_even = s.L <= 4;
    for (int l = 0; l + 1 < s.L; l++) all_even = all_even && !(lw[l] & 1) && !(lh[l] & 1);
    return all_even;
}

// CreatePyramids (src/patch_match.cpp:61-76) + tap packing, from a level-0 image that is
// already on the device at (src0, pitch0).
int slot_build(pagk_ctx *ctx, FrameSlot &s, const uint8_t *src0, int64_t pitch0, int wrap0)
{
    s.pad0 = wrap0 ? 0 : 2;  // callers that know the source's step refine this (frame_upload_any, pagk_frame_set_device)
    s.img0 = src0, s.pitch0 = pitch0;
    int lw[kMaxLevels], lh[kMaxLevels];
    level_dims(s.w, s.h, s.L, lw, lh);
    dim3 blk(32, 8);
    if (ctx->ev_pyr[0] && !in_capture(ctx)) HIPCHK(ctx, hipEventRecord(ctx->ev_pyr[0], ctx->stream));
    // the fused kernel re-derives every level from level 0 by nested 2x2 means: valid while every parent is
    // even in both dimensions (the exact-2x case of cv::resize); otherwise level by level
    bool all_even = true;
    for (int l = 0; l + 1 < s.L; l++) all_even = all_even && !(lw[l] & 1) && !(lh[l] & 1);
    if (s.L <= 4 && !ctx->unfused_pyramid && all_even) {
        PyrArgs pa;
        const int nb = make_pyr_args(s, src0, pitch0, wrap0, &pa);
        // ... with the next tracking launch's dispatch order as one leading workgroup, where one is due (pagk_order.h)
        const OrderArgs oa = order_build_args(ctx);
        hipLaunchKernelGGL(k_pyramid_fused, dim3(nb + (oa.n > 0 ? 1 : 0)), dim3(256), order_lds_bytes(oa.n), ctx->stream, pa, oa);
        HIPCHK(ctx, hipGetLastError());
        if (oa.n > 0) ctx->order.built(oa.n, ctx->stream, capture_kind(ctx));
        if (ctx->ev_pyr[1] && !in_capture(ctx)) HIPCHK(ctx, hipEventRecord(ctx->ev_pyr[1], ctx->stream));
        if (!in_capture(ctx)) ctx->pyr_timed = true;
        s.wrap0 = wrap0;
        s.valid = true;
        return PAGK_OK;
    }
    const uint8_t *src = src0;
    int64_t pitch = pitch0;
    for (int l = 0; l < s.L; l++) {
        if (l > 0) {
            dim3 grd((lw[l] + 31) / 32, (lh[l] + 7) / 8);
            if (!(lw[l - 1] & 1) && !(lh[l - 1] & 1))
                hipLaunchKernelGGL(k_pyr_down, grd, blk, 0, ctx->stream, src, pitch, lw[l], lh[l], s.u8[l]);
            else
                hipLaunchKernelGGL(k_pyr_down_linear, grd, blk, 0, ctx->stream, src, pitch, lw[l - 1], lh[l - 1], lw[l],
                                   lh[l], 1. / ((double)lw[l] / lw[l - 1]), 1. / ((double)lh[l] / lh[l - 1]), s.u8[l]);
            src = s.u8[l];
            pitch = lw[l];
        }
        dim3 grd((lw[l] + 31) / 32, (lh[l] + 7) / 8);
        hipLaunchKernelGGL(k_build_quads, grd, blk, 0, ctx->stream, src, pitch, lw[l], lh[l], l == 0 ? wrap0 : 1,
                           s.quad[l]);
    }
    HIPCHK(ctx, hipGetLastError());
    if (ctx->ev_pyr[1] && !in_capture(ctx)) HIPCHK(ctx, hipEventRecord(ctx->ev_pyr[1], ctx->stream));
    if (!in_capture(ctx)) ctx->pyr_timed = true;
    s.wrap0 = wrap0;
    s.valid = true;
    return PAGK_OK;
}

int check_params(const pagk_params *p)
{
    if (!p) return PAGK_E_ARG;
    if (p->half_patch < 1 || p->half_patch > PAGK_MAX_HALF_PATCH) return PAGK_E_ARG;
    if (p->iterations < 0 || p->pyramids < 1 || p->pyramids > PAGK_MAX_PYRAMIDS) return PAGK_E_ARG;
    // 1 is the reference's own bInverse_ (src/patch_match.cpp:220 "not support yet"); 2 the library's template-Jacobian mode
    if (p->inverse != 0 && p->inverse != PAGK_INVERSE_TEMPLATE) return PAGK_E_UNSUPPORTED;
    if (p->solver_variant & ~(SV_LOWER_SEQ | SV_UPPER_TREE | SV_NORM_SEQ | SV_LLT_RECIP | SV_PIVOT_TREE)) return PAGK_E_ARG;
    return PAGK_OK;
}

void fill_level(DevLevel &d, const FrameSlot &s, int l)
{
    int w = s.w, h = s.h;
    for (int k = 0; k < l; k++) {
        w = (int)(w * 0.5);
        h = (int)(h * 0.5);
    }
    d.quad = s.quad[l];
    d.cols = w;
    d.rows = h;
    d.fcols = (float)w;
    d.frows = (float)h;
    d.fcols_m1 = (float)(w - 1);
    d.frows_m1 = (float)(h - 1);
}

// A wave of a one-level-per-wave launch that gave up waiting for the level above (never expected: the wait is on a wave
// that started earlier), or a solving wave of the pipelined 4-wave body that gave up waiting for the other chain wave's
// sums, leaves results that must not be used.
int lv_check(pagk_ctx *ctx)
{
    if (ctx->lv_error && *static_cast<volatile int *>(ctx->lv_error) != 0) {
        *static_cast<volatile int *>(ctx->lv_error) = 0;
        snprintf(ctx->err, sizeof(ctx->err), "a wave of a tracking launch gave up waiting (for the level above, or for the other chain wave's sums)");
        return PAGK_E_HIP;
    }
    return PAGK_OK;
}

// The tracking kernels of one half patch, [lean] where a kernel has both forms: LEAN for the reference's defaults (no
// regularisation penalty, solver_variant 0 -- both compile-time facts there), generic for everything else.  Null where
// a kernel is not instantiated for the patch size: all but the 4-wave kernel exist for the common sizes only
// (pagk_select.h), block5 for h = 10, mfma and rows in a -DPAGK_ALL_VARIANTS build.
using TrackFn = void (*)(TrackArgs);
struct TrackKernels {
    TrackFn block[2] = {}, block5 = nullptr;         // 4-wave workgroup per feature; its build for five workgroups per CU
    void (*block_pyr[2])(TrackArgs, PyrArgs) = {};   // ... with another frame's pyramid built by trailing workgroups
    TrackFn resume[2] = {}, resume_live[2] = {};     // the hand-over's sweep and live finisher
    TrackFn wave[2] = {};                            // one wave per feature
    TrackFn quad[2] = {}, levels[2] = {}, batch[2] = {};  // four features per wave: whole features, one level per wave, ... of k streams
    TrackFn relaxed = nullptr;                       // relaxed-order experiment
    TrackFn mfma[2] = {}, rows = nullptr;            // 2-wave workgroup; four independent rows per wave
};

template <int H>
constexpr TrackKernels track_kernels()
{
    constexpr PatchShape s = patch_shape(H);
    TrackKernels k;
    k.block[0] = k_track_block<s.nr, s.tail>;
    k.block[1] = k_track_block<s.nr, s.tail, 4, false, false, true>;
    if constexpr (H == 10) k.block5 = k_track_block5<s.nr, s.tail, true>;
    if constexpr (common_patch(H)) {
        k.block_pyr[0] = k_track_block_pyr<s.nr, s.tail>;
        k.block_pyr[1] = k_track_block_pyr<s.nr, s.tail, true>;
        k.resume[0] = k_track_resume<s.nr, s.tail>;
        k.resume[1] = k_track_resume<s.nr, s.tail, true>;
        k.resume_live[0] = k_track_resume_live<s.nr, s.tail>;
        k.resume_live[1] = k_track_resume_live<s.nr, s.tail, true>;
        k.wave[0] = k_track_wave<s.nch, s.tail>;
        k.wave[1] = k_track_wave<s.nch, s.tail, true>;
        k.quad[0] = k_track_quad<s.nch>;
        k.quad[1] = k_track_quad<s.nch, true>;
        k.levels[0] = k_track_quad<s.nch, false, true>;
        k.levels[1] = k_track_quad<s.nch, true, true>;
        k.batch[0] = k_track_quad<s.nch, false, true, true>;
        k.batch[1] = k_track_quad<s.nch, true, true, true>;
        k.relaxed = k_track_block<s.nr, s.tail, 4, false, true>;
#ifdef PAGK_ALL_VARIANTS
        k.mfma[0] = k_track_block<s.mfma_nr, s.tail, 2, true>;
        k.mfma[1] = k_track_block<s.mfma_nr, s.tail, 2, true, false, true>;
        k.rows = k_track_rows<s.nch>;
#endif
    }
    return k;
}

template <int... H0>
constexpr std::array<TrackKernels, sizeof...(H0)> track_table(std::integer_sequence<int, H0...>)
{
    return {track_kernels<H0 + 1>()...};
}
constexpr auto kTrackTable = track_table(std::make_integer_sequence<int, PAGK_MAX_HALF_PATCH>{});
const TrackKernels &track_kernels_of(int half) { return kTrackTable[(size_t)half - 1]; }   // half: 1..15 (check_params)

// PAGK_INVERSE_TEMPLATE (pagk_inverse_kernel.h): one kernel, instantiated for every half patch, [lean] as above.
struct InverseKernels {
    TrackFn wave[2] = {};
};
template <int H>
constexpr InverseKernels inverse_kernels()
{
    constexpr PatchShape s = patch_shape(H);
    InverseKernels k;
    k.wave[0] = k_inv_wave<s.nch, s.tail>;
    k.wave[1] = k_inv_wave<s.nch, s.tail, true>;
    return k;
}
template <int... H0>
constexpr std::array<InverseKernels, sizeof...(H0)> inverse_table(std::integer_sequence<int, H0...>)
{
    return {inverse_kernels<H0 + 1>()...};
}
constexpr auto kInverseTable = inverse_table(std::make_integer_sequence<int, PAGK_MAX_HALF_PATCH>{});

#ifdef PAGK_ALL_VARIANTS
constexpr bool kAllVariants = true;
#else
constexpr bool kAllVariants = false;   // variants 2 and 6 are not in this build (pagk_has_variant)
#endif

// One launch of a tracking kernel; a kernel the table does not have for this patch size is an error, not a crash.
hipError_t launch(TrackFn kern, int grid, int block, size_t lds, hipStream_t stream, const TrackArgs &a)
{
    if (!kern) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, stream, a);
    return hipGetLastError();
}

// What select_variant (pagk_select.h) reads of a context and its parameters, for a launch of n features.
SelectIn select_in(const pagk_ctx *ctx, const pagk_params *p, long long n)
{
    return {ctx->kernel, p->half_patch, p->calculate_ncc != 0, p->pyramids, p->iterations, n, ctx->concurrency,
            ctx->lv_error != nullptr, ctx->levels_shared, ctx->mfma_min_features, ctx->wave_min_features,
            ctx->quad_min_features, ctx->levels_min_features, kAllVariants};
}

// Resident waves of k_track_quad<NCH> on this device: the kernel's own occupancy (registers, its 10000 B of LDS) times
// the CU count, asked once per context and patch size.
int quad_capacity(pagk_ctx *ctx, int half)
{
    if (ctx->quad_capacity[half] == 0) {
        int per_cu = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, track_kernels_of(half).quad[0], 64, 0);
        if (e != hipSuccess || per_cu <= 0) per_cu = 16;
        ctx->quad_capacity[half] = per_cu * (ctx->cus > 0 ? ctx->cus : 256);
    }
    return ctx->quad_capacity[half];
}

// Hand-over budget of a four-features-per-wave launch of `waves` wavefronts.  The hand-over pays where the launch ends
// with an exposed tail -- between half a round and 1.25 rounds of resident waves (quad_capacity: the kernel's occupancy
// on this device x its CU count; 16 x 256 on MI355X): a handful of features
// with 3-5x the mean iteration count would otherwise each keep a wave alive long after the rest has finished
// (configs[3], 20000 features: -6 %; 8000: -4 %).  With a fuller second round the first round's stragglers are already
// hidden behind it and the finisher only displaces throughput waves (30000: +8 %), and a context that shares the device
// (pagk_set_concurrency) has other launches to fill its tail.  profiles/r02_ab_runs.md.
int quad_budget_for(pagk_ctx *ctx, int waves, int iterations, int levels, int half)
{
    if (ctx->quad_budget >= 0) return ctx->quad_budget;
    // a feature can run iterations x levels iterations at most: with the reference's own call site (10 x 3) nothing
    // runs long enough past the budget for the hand-over to pay for its list reset, finisher launch and sweep
    if (iterations * levels < 60) return 0;
    const long long cap = quad_capacity(ctx, half);  // one "round" of resident waves
    // (beyond 1.25 rounds it loses, also when restricted to the launch's drain phase -- "a feature may leave only once
    // every wave has been dispatched": +8 % at 30000 features, +5 % at 60000, profiles/r03_finisher_sweep_drain_rule.log)
    const bool exposed_tail = 100ll * waves > 45 * cap && 100ll * waves <= 125 * cap;
    // (not inside a graph capture: the replayed graph runs its two branches one after the other, measured, and a
    // finisher that starts after the throughput kernel is the plain sweep: +13 %)
    // (not inside a capture of the stream that is not ours -- the host application's own hipStreamBeginCapture: a replayed
    // graph runs a finisher branch AFTER the throughput kernel, +13 %.  pagk_graph_begin's capture is replayed in
    // segments with the finisher beside the kernel, like a direct launch)
    if (ctx->concurrency != 1 || !exposed_tail || (in_capture(ctx) && !ctx->capturing)) return 0;
    return 20;
}

// The same for a one-level-per-wave launch (variant 7) of `quads` four-feature groups.  Its waves are short, so what
// the hand-over removes is not an idle tail but the critical path itself: the launch cannot end before its slowest
// feature has run its levels one after the other at the throughput kernel's ~11 us per iteration.  Measured with
// budgets 0 / 14 / 20 / 26 (profiles/r03_levels_handover.log): 20 gains 30 % at 10000-12000 features of configs[3],
// 13-20 % at 16000-24000, 3-7 % on the easier 752x480 pair, nothing from 30000 on (no loss either), and costs 3-6 %
// at 6000; 14 hands over ten times as many features and loses everywhere.  On from 0.45 rounds of resident waves.
// Inside a graph capture (the replayed graph runs a finisher branch AFTER the throughput kernel) the hand-over is
// the sweep alone -- `*live` false: the stragglers leave the throughput waves early and are finished by the 4-wave
// kernel behind them.  That still pays while the launch is chain-bound (12000 features of configs[3] 577 us instead of
// 714, 20000 features 699 instead of 769) and costs from about 1.3 rounds on (30000 features: +7.5 %,
// profiles/r03_levels_sweep_only.log): in a capture, up to 1.25 rounds.
int levels_budget_for(pagk_ctx *ctx, int quads, int iterations, int levels, int half, bool *live)
{
    // a capture of the stream that is not pagk_graph_begin's (the host application's own): its replay runs a finisher
    // branch after the kernel, so there the hand-over is the sweep alone, up to 1.25 rounds.  Our own capture is replayed
    // in segments with the finisher beside the kernel (launch_track): the direct launch's rule.
    const bool foreign = in_capture(ctx) && !ctx->capturing;
    *live = !foreign || ctx->quad_budget >= 0;   // (a forced budget keeps the parallel branch: tests)
    if (ctx->quad_budget >= 0) return ctx->quad_budget;
    if (iterations * levels < 60 || ctx->concurrency != 1) return 0;
    const long long cap = quad_capacity(ctx, half);
    if (100ll * quads <= 45 * cap) return 0;
    if (foreign && 100ll * quads > 125 * cap) return 0;
    return 20;
}

// What a launch takes from pagk_params: the constructor's constants (src/patch_match.cpp:48-57) and the camera model.
void fill_param_args(TrackArgs &a, const pagk_params *p)
{
    a.half = p->half_patch;
    a.iterations = p->iterations;
    a.has_gyro = p->has_gyro_predict_initial;
    a.illum = p->consider_illumination;
    a.use_affine = p->consider_affine;
    a.penalty = p->regularization_penalty;
    a.calc_ncc = p->calculate_ncc;
    a.solver = p->solver_variant;
    float invlog = p->inv_log_max_dist != 0.0f ? p->inv_log_max_dist
                                               : pagk_inv_log_max_dist(p->alpha, p->max_distance);
    a.lam_invlog = p->lambda * invlog;           // :305  mLambda * mInvLogMaxDist (float)
    a.lam_invlog_alpha = a.lam_invlog * p->alpha; // :307  ... * mAlpha (float)
    a.alpha = p->alpha;
    // :57  1.0f / (2.0f*h + 1.0f) / (2.0f*h + 1.0f), float, stored in a double
    a.win_size_inv = (double)(1.0f / (2.0f * p->half_patch + 1.0f) / (2.0f * p->half_patch + 1.0f));
    a.distort_on = p->dist_coef[0] != 0.0f;  // :410
    a.fx = p->fx, a.fy = p->fy, a.cx = p->cx, a.cy = p->cy;
    a.fx_inv = (float)(1.0 / (double)p->fx);  // src/utils.cpp:53
    a.fy_inv = (float)(1.0 / (double)p->fy);
    a.k1 = p->dist_coef[0], a.k2 = p->dist_coef[1], a.p1 = p->dist_coef[2], a.p2 = p->dist_coef[3];
    a.k3 = p->n_dist_coef == 5 ? p->dist_coef[4] : 0.0f;
}

constexpr const char *kLargestLaunchFirst = "run the largest launch once before capturing";
static_assert(sizeof(SuspState) == kSuspStateBytes, "levels_layout (pagk_layout.h) carves SuspState records");

// The workspaces of a four-features-per-wave launch: `need` bytes of img1 samples and, for one level per wave (lvl), the
// level workspace, whose base is returned in *lb.
int quad_workspace(pagk_ctx *ctx, size_t need, const LevelsLayout *lvl, TrackArgs *a, uint8_t **lb)
{
    const char *what = "the quad kernel's workspace";
    DevBuf &ws = ctx->buf[pagk_ctx::QUAD_WS], &lv = ctx->buf[pagk_ctx::LV];
    int rc = reserve(ctx, ws, need, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, what, kLargestLaunchFirst);
    if (rc || (rc = reserve(ctx, lv, lvl ? lvl->total : 0, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, what, kLargestLaunchFirst))) return rc;
    a->ws = static_cast<float *>(ws.ptr);
    if (!lvl) return PAGK_OK;
    *lb = static_cast<uint8_t *>(lv.ptr);
    a->queue = reinterpret_cast<int *>(*lb);
    a->lv_ready = reinterpret_cast<int *>(*lb + lvl->ready);
    a->lv_state = reinterpret_cast<float *>(*lb + lvl->state);
    a->lv_error = ctx->lv_error_dev;
    a->lv_polls = ctx->level_polls;
    a->lv_shift = ctx->levels_shift;
    return PAGK_OK;
}

// Variant 6 (pagk_rows_kernel.h): four features per wave with the four rows of a wave independent + a work queue.
int launch_rows(pagk_ctx *ctx, const TrackKernels &k, int n, TrackArgs &a)
{
    int &capacity = ctx->rows_capacity[a.half];
    if (capacity == 0) {
        int per_cu = 0, cus = 0;
        HIPCHK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.rows, 64, 0));
        HIPCHK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        capacity = per_cu * cus > 0 ? per_cu * cus : 1024;
    }
    // a resident grid: every wave starts at once, rows pull the features past 4 * grid from the queue
    int waves = (n + 3) / 4 < capacity ? (n + 3) / 4 : capacity;
    if (ctx->rows_waves_cap > 0 && waves > ctx->rows_waves_cap) waves = ctx->rows_waves_cap;
    const size_t need = (size_t)waves * 4 * patch_shape(a.half).nch * 64 * sizeof(float);
    if (int gr = reserve(ctx, ctx->buf[pagk_ctx::QUAD_WS], need, NOT_IN_CAPTURE_NOR_UNDER_GRAPH,
                         "the row kernel's workspace", kLargestLaunchFirst)) return gr;
    a.ws = static_cast<float *>(ctx->buf[pagk_ctx::QUAD_WS].ptr);
    a.queue = static_cast<int *>(ctx->queue);
    HIPCHK(ctx, hipMemsetAsync(a.queue, 0, 4, ctx->stream));
    HIPCHK(ctx, launch(k.rows, waves, 64, 0, ctx->stream, a));
    return PAGK_OK;
}

// Variants 5 and 7 (pagk_quad_kernel.h): four features per wave -- whole features per wave, or (use_levels) one pyramid
// level per wave (pyramids x ceil(n / 4) waves) -- with the hand-over of long features to the 4-wave kernel.
int launch_quad(pagk_ctx *ctx, const pagk_params *p, const TrackKernels &k, bool lean, bool use_levels, int n, TrackArgs &a)
{
    const int nch = patch_shape(a.half).nch, nq = (n + 3) / 4, waves = use_levels ? nq * p->pyramids : nq;
    const size_t need = (size_t)waves * 4 * nch * 64 * sizeof(float);
    const LevelsLayout lvl = levels_layout((size_t)n, (size_t)nq, p->pyramids);
    uint8_t *lb = nullptr;
    if (int gr = quad_workspace(ctx, need, use_levels ? &lvl : nullptr, &a, &lb)) return gr;
    a.susp_polls = ctx->finisher_polls;
    // continuation buffers; the hand-over needs the 4-wave kernel's LDS (<= 48 KB at these patch sizes)
    bool live_ok = true;
    const int budget = use_levels ? levels_budget_for(ctx, nq, p->iterations, p->pyramids, a.half, &live_ok)
                                  : quad_budget_for(ctx, nq, p->iterations, p->pyramids, a.half);
    const bool handover = budget > 0;
    ctx->last_handover = handover;
    if (handover) {
        // the continuation buffers: inside the level workspace, or -- whole features per wave -- a block of their own
        if (use_levels) {
            a.susp_count = reinterpret_cast<int *>(lb + lvl.susp_count);
            a.susp_list = reinterpret_cast<int *>(lb + lvl.susp_list);
            a.susp_state = reinterpret_cast<SuspState *>(lb + lvl.susp_state);
        } else {
            const size_t sizes[3] = {kSuspCountBytes, (size_t)n * 4, (size_t)n * sizeof(SuspState)};
            const Layout<3> lay(sizes);
            DevBuf &susp = ctx->buf[pagk_ctx::SUSP];
            if (int gr = reserve(ctx, susp, lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the continuation buffers",
                                 kLargestLaunchFirst)) return gr;
            a.susp_count = lay.at<int>(susp.ptr, 0);
            a.susp_list = lay.at<int>(susp.ptr, 1);
            a.susp_state = lay.at<SuspState>(susp.ptr, 2);
        }
        a.iter_budget = budget;
        a.susp_waves = nq;   // the waves that report their end: a quad's last-level wave / all of them
        a.susp_lone = ctx->susp_lone;
        ctx->susp_count_dev = a.susp_count;
    }
    // what must be zero before the launch: counters and ready lists, the hand-over's count and list
    if (use_levels)
        HIPCHK(ctx, hipMemsetAsync(lb, 0, handover ? lvl.susp_list + (size_t)n * 4 : lvl.susp_count, ctx->stream));
    else if (handover)
        HIPCHK(ctx, hipMemsetAsync(a.susp_count, 0, kSuspCountBytes + (size_t)n * 4, ctx->stream));
    // the live finisher runs beside the throughput kernel, on the context's auxiliary stream (inside a graph
    // capture the auxiliary stream joins the capture through the fork event: a parallel branch of the graph)
    const bool live = handover && live_ok && ctx->finisher_wgs > 0 && ctx->aux_stream;
    // inside pagk_graph_begin's capture the finisher is not a node of the graph but a launch of its own between
    // two segments of it (see pagk_ctx::GraphSeg); PAGK_GRAPH_BRANCH=1 keeps the old parallel-branch form (tests)
    const bool segmented = live && ctx->capturing && !getenv("PAGK_GRAPH_BRANCH");
    int fin_seg = -1;
    if (segmented) {
        if (int sr = capture_split(ctx)) return sr;
        ctx->cap_segs.emplace_back();
        ctx->cap_segs.back().kind = pagk_ctx::GraphSeg::FINISHER;   // (filled in below, once its arguments exist)
        fin_seg = (int)ctx->cap_segs.size() - 1;
    } else if (live) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->ev_fork, 0));
    }
    HIPCHK(ctx, launch(use_levels ? k.levels[lean] : k.quad[lean], waves, 64, 0, ctx->stream, a));
    TrackArgs af = a;   // what the latency kernels get
#ifdef PAGK_STAMPS
    if (af.dbg) af.dbg += (size_t)16 * (waves - nq);  // (diagnostic build: their records follow the throughput waves')
#endif
    const size_t lds = track_block_lds_bytes(a.half);
    if (live) {
        if (segmented) {   // remembered, not launched: pagk_graph_launch issues it beside the kernel's segment
            pagk_ctx::GraphSeg &fs = ctx->cap_segs[(size_t)fin_seg];
            fs.fn = reinterpret_cast<const void *>(k.resume_live[lean]);
            fs.args = af;
            fs.grid = ctx->finisher_wgs;
            fs.lds = lds;
            // the kernel's own segment ends here; what follows (the sweep, whatever the caller records next) waits
            // for the finisher at replay
            if (int sr = capture_split(ctx)) return sr;
            ctx->cap_segs.emplace_back();
            ctx->cap_segs.back().kind = pagk_ctx::GraphSeg::JOIN;
        } else {
            HIPCHK(ctx, launch(k.resume_live[lean], ctx->finisher_wgs, kBlock, lds, ctx->aux_stream, af));
            HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->aux_stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        }
    }
    // the sweep: the latency kernel finishes what is still waiting in the list (a fixed grid walks it)
    if (handover) HIPCHK(ctx, launch(k.resume[lean], live ? 64 : (n < 1024 ? n : 1024), kBlock, lds, ctx->stream, af));
    return PAGK_OK;
}

// Variant 0: the 4-wave workgroup per feature, for every patch size.  pyr / pyr_blocks / pyr_done: see launch_track.
int launch_block(pagk_ctx *ctx, const TrackKernels &k, bool lean, int n, const TrackArgs &a, const PyrArgs *pyr,
                 int pyr_blocks, bool *pyr_done)
{
    const size_t lds = track_block_lds_bytes(a.half);
    if (pyr && pyr_blocks > 0 && k.block_pyr[lean] && lds <= 48 * 1024) {
        hipLaunchKernelGGL(k.block_pyr[lean], dim3(n + pyr_blocks), dim3(kBlock), lds, ctx->stream, a, *pyr);
        HIPCHK(ctx, hipGetLastError());
        if (pyr_done) *pyr_done = true;
        return PAGK_OK;
    }
    // h = 10, lean, several rounds of workgroups: the build for five workgroups per CU
    // ... and a launch that five workgroups per CU hold at once but four do not (1025..1280 features on 256 CUs:
    // one round instead of two, 104 -> 97 us at 1100 features; from 1300 on the pipelined kernel is
    // equal or faster again, profiles/r04_block5_sweep_1100_3000.log)
    const bool five = lean && k.block5 && select_block5(n, ctx->block5_min_features, ctx->block5_window, ctx->cus);
    const TrackFn kern = five ? k.block5 : k.block[lean];
    if (lds > 48 * 1024) {
        // more than 48 KB of dynamic LDS (h >= 14) needs the attribute; set it once per kernel and device
        static thread_local bool configured[PAGK_MAX_HALF_PATCH + 1][2][16] = {};
        bool &done = configured[a.half][lean][ctx->device & 15];
        if (!done) {
            HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            done = true;
        }
    }
    HIPCHK(ctx, launch(kern, n, kBlock, lds, ctx->stream, a));
    return PAGK_OK;
}

// Room for the dispatch order of n features (pagk_order.h), beside the hints and under the same terms: where the buffer may not grow
// the launches run the identity.
int order_reserve(pagk_ctx *ctx, int n)
{
    DevBuf &ob = ctx->buf[pagk_ctx::DISPATCH_ORDER];
    if (!ctx->order.on || !order_serves(n, ctx->cus) || (size_t)n * sizeof(int32_t) <= ob.bytes || in_capture(ctx)) return PAGK_OK;
    for (int k = 0; k < pagk_ctx::kGraphs; k++)
        if (ctx->graph_execs[k]) return PAGK_OK;
    ctx->order.array_replaced();
    return reserve(ctx, ob, (size_t)n * sizeof(int32_t), NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the dispatch order", kLargestLaunchFirst);
}

// The hint array of the 4-wave kernels (pagk_prio.h): one int32 per feature slot, what the slot's feature ran in the previous
// launch.  It grows -- zeroed: no forecast -- with the largest launch; where it may not grow (inside a capture, under a live
// graph whose nodes hold the old pointer) the launch runs without a hint, which costs it issue order and nothing else.
int prio_hint_attach(pagk_ctx *ctx, int n, TrackArgs *a)
{
    DevBuf &hb = ctx->buf[pagk_ctx::PRIO_HINT];
    const size_t need = (size_t)n * sizeof(int32_t);
    if (int rc = order_reserve(ctx, n)) return rc;
    if (need > hb.bytes) {
        if (in_capture(ctx)) return PAGK_OK;
        for (int k = 0; k < pagk_ctx::kGraphs; k++)
            if (ctx->graph_execs[k]) return PAGK_OK;
        if (int rc = reserve(ctx, hb, need, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the priority hints", kLargestLaunchFirst)) return rc;
        HIPCHK(ctx, hipMemsetAsync(hb.ptr, 0, hb.bytes, ctx->stream));
    }
    a->prio_hint_in = a->prio_hint_out = static_cast<int *>(hb.ptr);
    return PAGK_OK;
}

// New features in the slots: what the slots' previous features ran says nothing about them (stream order).
int prio_hint_clear(pagk_ctx *ctx)
{
    DevBuf &hb = ctx->buf[pagk_ctx::PRIO_HINT];
    if (hb.ptr) HIPCHK(ctx, hipMemsetAsync(hb.ptr, 0, hb.bytes, ctx->stream));
    ctx->order.hints_cleared();   // all counts equal: the order they give is the identity, and no launch is handed an older one
    return PAGK_OK;
}

// pyr / pyr_blocks / pyr_done: optionally, another slot's pyramid to be built by trailing workgroups of the
// tracking launch (k_track_block_pyr).  Honoured when the 4-wave kernel is the one selected; *pyr_done tells the
// caller whether it was (otherwise the caller launches the pyramid itself).
int launch_track(pagk_ctx *ctx, const pagk_params *p, const FrameSlot &sr, const FrameSlot &sc, int n,
                 const float *d_pt_ref, const float *d_pt_init, const float *d_affine, const uint8_t *d_status,
                 const pagk_outputs *o, const PyrArgs *pyr = nullptr, int pyr_blocks = 0, bool *pyr_done = nullptr,
                 bool hinted = true)
{
    if (pyr_done) *pyr_done = false;
    TrackArgs a;
    memset(&a, 0, sizeof a);
    a.n_levels = p->pyramids;
    for (int l = 0; l < p->pyramids; l++) {
        fill_level(a.l1[l], sr, l);
        fill_level(a.l2[l], sc, l);
        // :66,:73  mvScales[i] = mvScales[i-1] * mPyramidScale  (float * double -> float)
        a.scales[l] = l == 0 ? 1.0f : (float)((double)a.scales[l - 1] * 0.5);
    }
    a.n = n;
    a.pt_ref = d_pt_ref;
    a.pt_init = d_pt_init;
    a.affine = d_affine;
    a.status_in = d_status;
    a.pt_un = o->pt_un;
    a.pt_dist = o->pt_dist;
    a.status = o->status;
    a.pix_err = o->pix_err;
    a.dist_pred = o->dist_pred;
    a.ncc = o->ncc;
    a.iters = o->iters;
#if defined(PAGK_STAMPS) || defined(PAGK_TIC)
    a.dbg = reinterpret_cast<unsigned long long *>(getenv("PAGK_DBG_PTR") ? strtoull(getenv("PAGK_DBG_PTR"), nullptr, 0) : 0ull);
#endif
    fill_param_args(a, p);
    a.prio_k = ctx->prio_k;
    a.prio_stats = ctx->prio_stats;
    a.prio_kbuf = ctx->prio_stats ? reinterpret_cast<const int *>(ctx->prio_stats + 2) : nullptr;
    a.lv_error = ctx->lv_error_dev;   // (the pipelined 4-wave body raises it too: a solve that gave up waiting for its sums)
    // ... and only where there is somebody to outrank: with a workgroup per CU or fewer, priority 3 throughout merely takes the
    // by-phase order away from the workgroup's own four waves (250 features: 55.1 -> 55.8 us).  The counts are stored all the same.
    // The threshold is stated for three pyramid levels, the shape it was chosen on; a feature's count grows with the levels it
    // runs -- K counts per level entered for the same reason -- so a launch of L levels compares with T L / 3, rounded up
    // (configs[2], four levels: 14 flags a third of the features, 1.3 per CU, and the boost is diluted; 19 flags 6 %).
    a.prio_hint_t = n > ctx->cus ? (int)(((long long)ctx->prio_hint_t * p->pyramids + 2) / 3) : 0;

    if (ctx->ev_trk[0] && !in_capture(ctx)) HIPCHK(ctx, hipEventRecord(ctx->ev_trk[0], ctx->stream));
    if (n > 0) {
        ctx->last_handover = false;
        // the reference's defaults (no regularisation penalty, solver_variant 0) run kernels in which both are
        // compile-time facts (LEAN); everything else runs the generic instantiations
        const bool lean = !a.penalty && a.solver == 0;
        const TrackKernels &k = track_kernels_of(a.half);
        // the template-Jacobian mode has one kernel: pagk_set_kernel, the priority hint, the dispatch order and the hand-over do
        // not apply to such a launch, and a pyramid offered for fusing is left to the caller (*pyr_done stays false)
        const int variant = ctx->last_variant = p->inverse == PAGK_INVERSE_TEMPLATE ? 8 : select_variant(select_in(ctx, p, n));
        int rc = PAGK_OK;
        hipError_t e = hipSuccess;
        switch (variant) {
            case 8:   // pagk_inverse_kernel.h
                e = launch(kInverseTable[(size_t)a.half - 1].wave[lean], n, 64, inv_wave_lds_bytes(a.half, a.calc_ncc != 0), ctx->stream, a);
                break;
            case 1: e = launch(k_track_thread, (n + 63) / 64, 64, 0, ctx->stream, a); break;
            case 2: e = launch(k.mfma[lean], n, 128, track_mfma_lds_bytes(a.half), ctx->stream, a); break;
            case 3: e = launch(k.wave[lean], n, 64, track_wave_lds_bytes(a.half), ctx->stream, a); break;   // pagk_wave_kernel.h
            // relaxed-order experiment (NOT parity-exact; never chosen automatically)
            case 4: e = launch(k.relaxed, n, kBlock, track_block_lds_bytes(a.half), ctx->stream, a); break;
            case 5:
            case 7: rc = launch_quad(ctx, p, k, lean, variant == 7, n, a); break;
            case 6: rc = launch_rows(ctx, k, n, a); break;
            default:
                // (hinted: false for the host-buffer calls -- their arrays are new features in a new order every call, a count
                // kept for them would forecast nothing, and they clear the array instead: prio_hint_clear)
                if (hinted && (rc = prio_hint_attach(ctx, n, &a))) break;
                // the dispatch order, by the conservative rule of pagk_order.h; frozen with the graph inside a capture, like the hint pointer
                if (a.prio_hint_in && ctx->order.usable(n, ctx->stream, ctx->cus, capture_kind(ctx)) &&
                    ctx->buf[pagk_ctx::DISPATCH_ORDER].bytes >= (size_t)n * sizeof(int32_t))
                    a.order = static_cast<const int *>(ctx->buf[pagk_ctx::DISPATCH_ORDER].ptr);
                rc = launch_block(ctx, k, lean, n, a, pyr, pyr_blocks, pyr_done);
                if (!rc && hinted) ctx->order.launched(a.prio_hint_out ? n : 0, ctx->stream, a.order != nullptr, capture_kind(ctx));
                break;
        }
        if (rc) return rc;
        HIPCHK(ctx, e);
        HIPCHK(ctx, hipGetLastError());
    }
    if (ctx->ev_trk[1] && !in_capture(ctx)) HIPCHK(ctx, hipEventRecord(ctx->ev_trk[1], ctx->stream));
    if (!in_capture(ctx)) ctx->trk_timed = true;
    return PAGK_OK;
}

// device staging for the host-buffer path: one block holding every per-feature array
struct FeatPtrs {
    float *pt_ref, *pt_init, *affine;
    uint8_t *status_in;
    pagk_outputs out;
    Layout<11> lay;    // the eleven arrays inside the block (and its pinned mirror)
    size_t in_bytes;   // [0, in_bytes) = the four input arrays; [in_bytes, lay.total) = the outputs
};

int feat_reserve(pagk_ctx *ctx, int n, FeatPtrs *fp)
{
    int cap = n < 1 ? 1 : n;
    // per feature: 8+8+16+1 in, 8+8+1+8+8+4+4 out; every array 256-aligned
    size_t sizes[11] = {8, 8, 16, 1, 8, 8, 1, 8, 8, 4, 4};
    for (size_t &sz : sizes) sz *= (size_t)cap;
    const Layout<11> lay(sizes);
    int rc = reserve(ctx, ctx->buf[pagk_ctx::FEAT], lay.total, GROW_FREELY, "the feature arrays");
    if (rc) return rc;
    void *b = ctx->buf[pagk_ctx::FEAT].ptr;
    fp->lay = lay;
    fp->in_bytes = lay.off[4];
    fp->pt_ref = lay.at<float>(b, 0);
    fp->pt_init = lay.at<float>(b, 1);
    fp->affine = lay.at<float>(b, 2);
    fp->status_in = lay.at<uint8_t>(b, 3);
    fp->out = {lay.at<float>(b, 4), lay.at<float>(b, 5), lay.at<uint8_t>(b, 6), lay.at<double>(b, 7),
               lay.at<double>(b, 8), lay.at<float>(b, 9), lay.at<int32_t>(b, 10)};
    return PAGK_OK;
}

int upload_level0(pagk_ctx *ctx, FrameSlot &s, const pagk_image *img)
{
    // straight from the caller's (pageable) memory: packing the rows into a pinned buffer first and shipping
    // one DMA measured the same (244 vs 238 us per pagk_track call, tools/host_path_time.py)
    HIPCHK(ctx, hipMemcpy2DAsync(s.u8[0], (size_t)s.w, img->data, (size_t)img->step, (size_t)s.w, (size_t)s.h,
                                 hipMemcpyHostToDevice, ctx->stream));
    return PAGK_OK;
}

int check_image(const pagk_image *im)
{
    if (!im || !im->data || im->width < 1 || im->height < 1 || im->step < im->width) return PAGK_E_ARG;
    // the samplers index with 24-bit multiplies and 32-bit element offsets
    if (im->width >= (1 << 24) || im->height >= (1 << 24) || (int64_t)im->width * im->height >= (1ll << 31)) return PAGK_E_ARG;
    return PAGK_OK;
}

int track_host_common(pagk_ctx *ctx, const pagk_params *p, int n, const float *pt_ref, const float *pt_init,
                      const float *affine, const uint8_t *status_in, const pagk_outputs *out, FrameSlot &sr,
                      FrameSlot &sc)
{
    if (n < 0 || !out || !out->pt_un || !out->status) return PAGK_E_ARG;
    if (n > 0 && (!pt_ref || !status_in)) return PAGK_E_ARG;
    if (n > 0 && p->has_gyro_predict_initial && !pt_init) return PAGK_E_ARG;
    if (n > 0 && p->consider_affine && !affine) return PAGK_E_ARG;
    FeatPtrs fp;
    int rc = feat_reserve(ctx, n, &fp);
    if (rc) return rc;
    const size_t *offs = fp.lay.off;
    uint8_t *hb = static_cast<uint8_t *>(ctx->buf[pagk_ctx::FEAT].host), *db = static_cast<uint8_t *>(ctx->buf[pagk_ctx::FEAT].ptr);
    if (n > 0) {
        // gather the (up to) four input arrays into the pinned mirror, ship them with ONE copy
        size_t nn = (size_t)n;
        memcpy(hb + offs[0], pt_ref, nn * 8);
        if (pt_init) memcpy(hb + offs[1], pt_init, nn * 8);
        if (affine) memcpy(hb + offs[2], affine, nn * 16);
        memcpy(hb + offs[3], status_in, nn);
        HIPCHK(ctx, hipMemcpyAsync(db, hb, fp.in_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = prio_hint_clear(ctx))) return rc;   // the arrays above are new features, whatever the slots held
    pagk_outputs dout = fp.out;
    if (!out->pt_dist) dout.pt_dist = nullptr;
    if (!out->pix_err) dout.pix_err = nullptr;
    if (!out->dist_pred) dout.dist_pred = nullptr;
    if (!out->ncc) dout.ncc = nullptr;
    if (!out->iters) dout.iters = nullptr;
    rc = launch_track(ctx, p, sr, sc, n, fp.pt_ref, pt_init ? fp.pt_init : nullptr, affine ? fp.affine : nullptr,
                      fp.status_in, &dout, nullptr, 0, nullptr, false);
    if (rc) return rc;
    if (n > 0)  // every output array with ONE copy into the pinned mirror, scattered to the caller after the sync
        HIPCHK(ctx, hipMemcpyAsync(hb + fp.in_bytes, db + fp.in_bytes, fp.lay.total - fp.in_bytes, hipMemcpyDeviceToHost,
                                   ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (int lr = lv_check(ctx)) return lr;
    if (n > 0) {
        size_t nn = (size_t)n;
        memcpy(out->pt_un, hb + offs[4], nn * 8);
        if (out->pt_dist) memcpy(out->pt_dist, hb + offs[5], nn * 8);
        memcpy(out->status, hb + offs[6], nn);
        if (out->pix_err) memcpy(out->pix_err, hb + offs[7], nn * 8);
        if (out->dist_pred) memcpy(out->dist_pred, hb + offs[8], nn * 8);
        if (out->ncc) memcpy(out->ncc, hb + offs[9], nn * 4);
        if (out->iters) memcpy(out->iters, hb + offs[10], nn * 4);
    }
    return PAGK_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

int pagk_version(void) { return PAGK_VERSION; }

const char *pagk_strerror(int code)
{
    switch (code) {
        case PAGK_OK: return "ok";
        case PAGK_E_ARG: return "invalid argument";
        case PAGK_E_HIP: return "HIP runtime error";
        case PAGK_E_NOMEM: return "out of memory";
        case PAGK_E_UNSUPPORTED: return "unsupported mode";
        case PAGK_E_NODEVICE: return "no HIP device";
        case PAGK_E_NCCL: return "RCCL error";
        case PAGK_E_CAPACITY: return "output capacity too small";
        default: return "unknown error";
    }
}

const char *pagk_last_error(const pagk_ctx *ctx) { return ctx ? ctx->err : ""; }

// Reference call site src/gyro_aided_tracker.cpp:276-282 and eType 4 (:402-408).
void pagk_params_default(pagk_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->half_patch = 5;
    p->iterations = 10;
    p->pyramids = 3;
    p->has_gyro_predict_initial = 1;
    p->inverse = 0;
    p->consider_illumination = 1;
    p->consider_affine = 1;
    p->regularization_penalty = 0;
    p->calculate_ncc = 0;
    p->lambda = 1.0f;      // src/patch_match.cpp:48
    p->alpha = 0.5f;       // :49
    p->max_distance = 25;  // :50
    p->inv_log_max_dist = 0.0f;
    p->fx = p->fy = 1.0f;
    p->n_dist_coef = 4;
}

// src/patch_match.cpp:51  mInvLogMaxDist = 1.0 / (std::log(mAlpha * mMaxDistance + 1));
// float * int -> float, + 1 -> float, std::log(float) -> float, 1.0 / float -> double -> float member.
float pagk_inv_log_max_dist(float alpha, int32_t max_distance)
{
    float arg = alpha * (float)max_distance + 1;
    float lg = std::log(arg);
    return (float)(1.0 / (double)lg);
}

int pagk_create(pagk_ctx **out, int device)
{
    if (!out) return PAGK_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PAGK_E_NODEVICE;
    if (device < 0 || device >= ndev) return PAGK_E_ARG;
    pagk_ctx *ctx = new (std::nothrow) pagk_ctx();
    if (!ctx) return PAGK_E_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return PAGK_E_HIP;
    }
    ctx->stream = ctx->own_stream;
    ctx->buf[pagk_ctx::FEAT].mirrored = true;
    for (int b : {pagk_ctx::RECT_ENTRIES, pagk_ctx::ORB_PATTERN, pagk_ctx::PRIO_HINT, pagk_ctx::DISPATCH_ORDER, pagk_ctx::GROUP,
                  pagk_ctx::RESULTS, pagk_ctx::GROUP_RESULTS, pagk_ctx::GROUP_LK, pagk_ctx::GROUP_SENSOR})
        ctx->buf[b].state = true;
    if (hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ctx->cus = 0;
    if (hipMalloc(&ctx->queue, 256) != hipSuccess) {
        pagk_destroy(ctx);
        return PAGK_E_NOMEM;
    }
    {   // the error word of the one-level-per-wave launches lives in mapped host memory: read at a sync without a copy
        void *hp = nullptr;
        void *dp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess) {
            memset(hp, 0, 64);
            if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess && dp) {
                ctx->lv_error = static_cast<int *>(hp);
                ctx->lv_error_dev = static_cast<int *>(dp);
            } else {
                (void)hipHostFree(hp);
            }
        }
    }
    // the selection thresholds were measured on 256 CUs; they are launch sizes relative to what the device holds at once,
    // so a device (or a partition of one) with another CU count gets them in proportion
    if (ctx->cus > 0 && ctx->cus != 256) {
        auto scaled = [&](int v) { return v >= 0x7fffffff / 2 ? v : (int)((long long)v * ctx->cus / 256); };
        ctx->wave_min_features = scaled(ctx->wave_min_features);
        ctx->quad_min_features = scaled(ctx->quad_min_features);
        ctx->levels_min_features = scaled(ctx->levels_min_features);
        ctx->block5_min_features = scaled(ctx->block5_min_features);
    }
    ctx->unfused_pyramid = getenv("PAGK_UNFUSED_PYRAMID") != nullptr;
    if (getenv("PAGK_MFMA_MIN")) ctx->mfma_min_features = atoi(getenv("PAGK_MFMA_MIN"));
    if (getenv("PAGK_WAVE_MIN")) ctx->wave_min_features = atoi(getenv("PAGK_WAVE_MIN"));
    if (getenv("PAGK_QUAD_MIN")) ctx->quad_min_features = atoi(getenv("PAGK_QUAD_MIN"));
    if (getenv("PAGK_BLOCK5_MIN")) ctx->block5_min_features = atoi(getenv("PAGK_BLOCK5_MIN")), ctx->block5_window = false;
    if (getenv("PAGK_LEVELS_MIN")) ctx->levels_min_features = atoi(getenv("PAGK_LEVELS_MIN"));
    if (getenv("PAGK_PRIO_K") && strcmp(getenv("PAGK_PRIO_K"), "auto") == 0) {
        // seeded with the BASELINE workloads' mean (3.5 iterations per feature and level: K = 4 until the context's own launches say otherwise)
        struct { unsigned long long st[2]; int k, pad; } seed = {{3500ull, 1000ull}, ctx->prio_k, 0};
        if (hipMalloc(reinterpret_cast<void **>(&ctx->prio_stats), sizeof seed) != hipSuccess ||
            hipMemcpy(ctx->prio_stats, &seed, sizeof seed, hipMemcpyHostToDevice) != hipSuccess) {
            if (ctx->prio_stats) (void)hipFree(ctx->prio_stats);
            ctx->prio_stats = nullptr;   // (the fixed threshold then)
            (void)hipGetLastError();
        }
    } else if (getenv("PAGK_PRIO_K")) {
        ctx->prio_k = atoi(getenv("PAGK_PRIO_K")) < 0 ? 0 : atoi(getenv("PAGK_PRIO_K"));
    }
    if (getenv("PAGK_PRIO_HINT")) ctx->prio_hint_t = prio_hint_parse(getenv("PAGK_PRIO_HINT"), ctx->prio_hint_t);
    if (getenv("PAGK_DISPATCH_ORDER")) ctx->order.on = atoi(getenv("PAGK_DISPATCH_ORDER")) != 0;
    if (getenv("PAGK_LEVELS_XCD_SHIFT")) ctx->levels_shift = atoi(getenv("PAGK_LEVELS_XCD_SHIFT")) & 7;
    if (getenv("PAGK_LEVELS_SHARED")) ctx->levels_shared = atoi(getenv("PAGK_LEVELS_SHARED")) != 0;
    if (getenv("PAGK_QUAD_BUDGET")) ctx->quad_budget = atoi(getenv("PAGK_QUAD_BUDGET"));
    if (getenv("PAGK_ROWS_WAVES")) ctx->rows_waves_cap = atoi(getenv("PAGK_ROWS_WAVES"));
    if (getenv("PAGK_FINISHER_WGS")) ctx->finisher_wgs = atoi(getenv("PAGK_FINISHER_WGS"));
    if (getenv("PAGK_SUSPEND_LONE")) ctx->susp_lone = atoi(getenv("PAGK_SUSPEND_LONE"));
    if (getenv("PAGK_FINISHER_POLLS")) ctx->finisher_polls = atoi(getenv("PAGK_FINISHER_POLLS"));
    if (getenv("PAGK_LEVEL_POLLS")) ctx->level_polls = atoi(getenv("PAGK_LEVEL_POLLS"));
    if (hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_batch, hipEventDisableTiming) != hipSuccess) {
        pagk_destroy(ctx);
        return PAGK_E_HIP;
    }
    for (int k = 0; k < 2; k++) {
        if (hipEventCreate(&ctx->ev_trk[k]) != hipSuccess || hipEventCreate(&ctx->ev_pyr[k]) != hipSuccess) {
            pagk_destroy(ctx);
            return PAGK_E_HIP;
        }
    }
    *out = ctx;
    return PAGK_OK;
}

void pagk_destroy(pagk_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->group) {   // a group goes with any of its members: the others stay ordinary sequences
        ctx->group->members[0]->capturing = false;
        (void)pagk_sequence_group_destroy(ctx->group->members[0]);
    }
    if (ctx->seq) {   // a live sequence goes with its context
        ctx->capturing = false;
        (void)pagk_sequence_destroy(ctx);
    }
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    if (ctx->aux_stream) {
        (void)hipStreamSynchronize(ctx->aux_stream);
        (void)hipStreamDestroy(ctx->aux_stream);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    for (int k = 0; k < pagk_ctx::kGraphs; k++) {
        if (ctx->graph_execs[k]) {
            (void)hipGraphExecDestroy(ctx->graph_execs[k]);
            (void)hipGraphDestroy(ctx->graphs[k]);
        }
        destroy_segs(ctx->pre_segs[k]);
    }
    destroy_segs(ctx->cap_segs);
    for (auto &s : ctx->slots) (void)release(ctx, s.block);
    for (auto &b : ctx->buf) (void)release(ctx, b);
    if (ctx->queue) (void)hipFree(ctx->queue);
    if (ctx->prio_stats) (void)hipFree(ctx->prio_stats);
    for (auto &d : ctx->batch_ring) batch_desc_free(d);
    batch_desc_free(ctx->cap_batch);
    for (int k = 0; k < pagk_ctx::kGraphs; k++) batch_desc_free(ctx->graph_batch[k]);
    if (ctx->ev_batch) (void)hipEventDestroy(ctx->ev_batch);
    if (ctx->lv_error) (void)hipHostFree(ctx->lv_error);
    for (int k = 0; k < 2; k++) {
        if (ctx->ev_trk[k]) (void)hipEventDestroy(ctx->ev_trk[k]);
        if (ctx->ev_pyr[k]) (void)hipEventDestroy(ctx->ev_pyr[k]);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int pagk_set_stream(pagk_ctx *ctx, void *hip_stream)
{
    if (!ctx) return PAGK_E_ARG;
    ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return PAGK_OK;
}

// Variants (b) (2-wave workgroup, f64 MFMA chain) and (e) (four independent rows per wave + work queue) win at no launch
// size any more ((b) since round 3's instruction diet of the 4-wave kernel, (e) only beyond 60000
// features) and nothing selects them automatically: they are compiled with -DPAGK_ALL_VARIANTS only (tools/ and the
// tests build that library when they want them), so the product's build and code object do not carry their fifteen
// instantiations.
int pagk_has_variant(int32_t which)
{
    if (which == 8) return 1;   // what pagk_last_variant reports after a PAGK_INVERSE_TEMPLATE launch; no pagk_set_kernel value
    return which >= 0 && which <= 7 && (kAllVariants || (which != 2 && which != 6));
}

int pagk_set_kernel(pagk_ctx *ctx, int32_t which)
{
    if (!ctx || which < 0 || which > 7) return PAGK_E_ARG;
    if (!pagk_has_variant(which)) {
        snprintf(ctx->err, sizeof(ctx->err), "variant %d is not in this build of libpagk_hip.so (compile with -DPAGK_ALL_VARIANTS)", which);
        return PAGK_E_UNSUPPORTED;
    }
    ctx->kernel = which;
    return PAGK_OK;
}

int pagk_params_check(const pagk_params *params) { return check_params(params); }

int pagk_last_variant(const pagk_ctx *ctx) { return ctx ? ctx->last_variant : PAGK_E_ARG; }

int pagk_last_handover(pagk_ctx *ctx)
{
    if (!ctx) return PAGK_E_ARG;
    if (!ctx->last_handover || !ctx->susp_count_dev) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int count = 0;
    HIPCHK(ctx, hipMemcpyAsync(&count, ctx->susp_count_dev, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (int lr = lv_check(ctx)) return lr;
    return count;
}

// The K the next launch of the 4-wave kernels will use (csrc/pagk_prio.h): the fixed one, or what the context's statistics say.
int pagk_priority_threshold(pagk_ctx *ctx)
{
    if (!ctx) return PAGK_E_ARG;
    if (!ctx->prio_stats) return ctx->prio_k;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int k = 0;
    HIPCHK(ctx, hipMemcpyAsync(&k, ctx->prio_stats + 2, sizeof k, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (int lr = lv_check(ctx)) return lr;
    return k;
}

// The hint threshold of the 4-wave kernels (csrc/pagk_prio.h; 0 = off).
int pagk_prio_hint_threshold(pagk_ctx *ctx) { return ctx ? ctx->prio_hint_t : PAGK_E_ARG; }

// The caller wrote NEW features into the device arrays it tracks with: forget what the slots' previous features ran.
// In stream order, capturable.  (The host-buffer entry points do this themselves.)
int pagk_prio_hint_reset(pagk_ctx *ctx)
{
    if (!ctx) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return prio_hint_clear(ctx);
}

// The first n hints to host memory (diagnostics, tests; synchronises).  Slots past the array's size read 0.
int pagk_prio_hint_get(pagk_ctx *ctx, int32_t n, int32_t *hints)
{
    if (!ctx || n < 0 || (n > 0 && !hints)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_prio_hint_get");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const DevBuf &hb = ctx->buf[pagk_ctx::PRIO_HINT];
    const size_t have = hb.bytes / sizeof(int32_t) < (size_t)n ? hb.bytes / sizeof(int32_t) : (size_t)n;
    memset(hints, 0, (size_t)n * sizeof(int32_t));
    if (have) HIPCHK(ctx, hipMemcpyAsync(hints, hb.ptr, have * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->order.stream_idle(ctx->stream);
    return PAGK_OK;
}

// The dispatch order of the 4-wave launches (csrc/pagk_order.h): 1 unless PAGK_DISPATCH_ORDER=0 was in the environment of pagk_create.
int pagk_dispatch_order_enabled(pagk_ctx *ctx) { return ctx ? (ctx->order.on ? 1 : 0) : PAGK_E_ARG; }

// The first n entries of the order array as they are on the device (diagnostics, tests; synchronises); entries past the array's size
// read as the identity.  *in_force (may be NULL): 1 when a hinted 4-wave launch of n features enqueued next on the current stream would
// be handed the array, 0 when it would run the identity.
int pagk_dispatch_order_get(pagk_ctx *ctx, int32_t n, int32_t *order, int32_t *in_force)
{
    if (!ctx || n < 0 || (n > 0 && !order)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_dispatch_order_get");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const DevBuf &ob = ctx->buf[pagk_ctx::DISPATCH_ORDER];
    const size_t have = ob.bytes / sizeof(int32_t) < (size_t)n ? ob.bytes / sizeof(int32_t) : (size_t)n;
    for (int32_t i = 0; i < n; i++) order[i] = i;
    if (have) HIPCHK(ctx, hipMemcpyAsync(order, ob.ptr, have * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->order.stream_idle(ctx->stream);
    if (in_force) *in_force = (have == (size_t)n && ctx->order.usable(n, ctx->stream, ctx->cus, 0)) ? 1 : 0;
    return PAGK_OK;
}

// Install n hints from host memory (tests, a host that keeps its own forecast; synchronises).  The array grows as a launch of n
// features would grow it; slots past n read 0.
int pagk_prio_hint_set(pagk_ctx *ctx, int32_t n, const int32_t *hints)
{
    if (!ctx || n < 0 || (n > 0 && !hints)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_prio_hint_set");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf &hb = ctx->buf[pagk_ctx::PRIO_HINT];
    if (int rc = reserve(ctx, hb, (size_t)n * sizeof(int32_t), NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the priority hints", kLargestLaunchFirst)) return rc;
    if (int rc = prio_hint_clear(ctx)) return rc;
    if (n) HIPCHK(ctx, hipMemcpyAsync(hb.ptr, hints, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = order_reserve(ctx, n)) return rc;
    ctx->order.stream_idle(ctx->stream);
    ctx->order.hints_set(n);   // a forecast for n slots: the next pyramid launch sorts it
    return PAGK_OK;
}

// The error word of the level-by-level launches without a synchronisation: for callers that synchronise the stream
// themselves (pagk_set_stream, a torch stream) and therefore never pass through pagk_sync.  Call it AFTER that
// synchronisation.  PAGK_OK, or PAGK_E_HIP once for a launch in which a wave gave up waiting.
int pagk_check_launch(pagk_ctx *ctx)
{
    if (!ctx) return PAGK_E_ARG;
    return lv_check(ctx);
}

int pagk_set_concurrency(pagk_ctx *ctx, int32_t streams)
{
    if (!ctx || streams < 1 || streams > 64) return PAGK_E_ARG;
    ctx->concurrency = streams;
    return PAGK_OK;
}

int pagk_sync(pagk_ctx *ctx)
{
    if (!ctx) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_sync");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->order.stream_idle(ctx->stream);
    return lv_check(ctx);
}

int pagk_last_kernel_ms(pagk_ctx *ctx, float *track_ms, float *pyramid_ms)
{
    if (!ctx) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_last_kernel_ms");
    if (track_ms) {
        *track_ms = 0.0f;
        if (ctx->trk_timed) {
            HIPCHK(ctx, hipEventSynchronize(ctx->ev_trk[1]));
            HIPCHK(ctx, hipEventElapsedTime(track_ms, ctx->ev_trk[0], ctx->ev_trk[1]));
        }
    }
    if (pyramid_ms) {
        *pyramid_ms = 0.0f;
        if (ctx->pyr_timed) {
            HIPCHK(ctx, hipEventSynchronize(ctx->ev_pyr[1]));
            HIPCHK(ctx, hipEventElapsedTime(pyramid_ms, ctx->ev_pyr[0], ctx->ev_pyr[1]));
        }
    }
    return PAGK_OK;
}

static int frame_upload_any(pagk_ctx *ctx, int32_t slot, const pagk_image *img, int32_t pyramids);

int pagk_frame_upload(pagk_ctx *ctx, int32_t slot, const pagk_image *img, int32_t pyramids)
{
    if (!ctx || slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_frame_upload");
    int rc = frame_upload_any(ctx, slot, img, pyramids);
    if (rc) return rc;
    // the copy reads img->data asynchronously when that memory is pinned (a camera ring buffer, a pinned tensor):
    // do not return before it has been read, or the caller could overwrite the frame while it is in flight
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PAGK_OK;
}

// The same for a frame in PINNED host memory (a camera driver's ring buffer, hipHostMalloc / hipHostRegister):
// asynchronous -- returns once the copy and the pyramid are enqueued on the context's stream -- and capturable: between
// pagk_graph_begin and pagk_graph_end the host -> device copy becomes a node of the graph, so a live loop replays
// [copy the frame the camera just wrote -> pyramid -> PatchMatch] with one pagk_graph_launch per frame.  The caller
// keeps the memory pinned, and unchanged from the call (or the replay) until that work has run.
int pagk_frame_upload_pinned(pagk_ctx *ctx, int32_t slot, const pagk_image *img, int32_t pyramids)
{
    if (!ctx || slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    return frame_upload_any(ctx, slot, img, pyramids);
}

static int frame_upload_any(pagk_ctx *ctx, int32_t slot, const pagk_image *img, int32_t pyramids)
{
    if (!ctx || slot < 0 || slot >= kSlots || pyramids < 1 || pyramids > PAGK_MAX_PYRAMIDS) return PAGK_E_ARG;
    int rc = check_image(img);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FrameSlot &s = ctx->slots[slot];
    s.valid = false;
    if ((rc = slot_reserve(ctx, s, img->width, img->height, pyramids))) return rc;
    if ((rc = upload_level0(ctx, s, img))) return rc;
    rc = slot_build(ctx, s, s.u8[0], s.w, img->step == img->width);
    s.pad0 = (int)(img->step - img->width > 2 ? 2 : img->step - img->width);
    return rc;
}

int pagk_frame_set_device(pagk_ctx *ctx, int32_t slot, const void *d_data, int32_t width, int32_t height,
                          int64_t step, int32_t pyramids)
{
    if (!ctx || slot < 0 || slot >= kUserSlots || pyramids < 1 || pyramids > PAGK_MAX_PYRAMIDS) return PAGK_E_ARG;
    if (!d_data || width < 1 || height < 1 || step < width) return PAGK_E_ARG;
    if (width >= (1 << 24) || height >= (1 << 24) || (int64_t)width * height >= (1ll << 31)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FrameSlot &s = ctx->slots[slot];
    s.valid = false;
    int rc = slot_reserve(ctx, s, width, height, pyramids);
    if (rc) return rc;
    // level 0 is read in place: no copy
    rc = slot_build(ctx, s, static_cast<const uint8_t *>(d_data), step, step == width);
    s.pad0 = (int)(step - width > 2 ? 2 : step - width);
    return rc;
}

// pagk_frame_set_device for the frames of k contexts that share a device, as ONE launch: the CreatePyramids
// (src/patch_match.cpp:61-76) of k trackers stepped together.  A pyramid kernel is a few microseconds of work behind a
// launch: eight of them in a row cost 50-125 us of a 0.85 ms batched step (tools/batch_breakdown.py).  Per frame the same
// bytes as its own launch (the same block body on the same arguments).
int pagk_frame_set_device_batch(pagk_ctx *const *ctxs, int32_t k, const int32_t *slot, const void *const *d_data,
                                const int32_t *width, const int32_t *height, const int64_t *step, int32_t pyramids)
{
    if (!ctxs || k < 1 || k > pagk_ctx::kBatchMaxStreams || !slot || !d_data || !width || !height || !step) return PAGK_E_ARG;
    if (pyramids < 1 || pyramids > PAGK_MAX_PYRAMIDS) return PAGK_E_ARG;
    for (int j = 0; j < k; j++) {
        if (!ctxs[j] || slot[j] < 0 || slot[j] >= kUserSlots || !d_data[j] || width[j] < 1 || height[j] < 1 || step[j] < width[j]) return PAGK_E_ARG;
        if (width[j] >= (1 << 24) || height[j] >= (1 << 24) || (int64_t)width[j] * height[j] >= (1ll << 31)) return PAGK_E_ARG;
        for (int i = 0; i < j; i++)
            if (ctxs[i] == ctxs[j] && slot[i] == slot[j]) return PAGK_E_ARG;   // (one frame per slot)
    }
    pagk_ctx *lead = ctxs[0];
    for (int j = 1; j < k; j++)
        if (ctxs[j]->device != lead->device) {
            snprintf(lead->err, sizeof(lead->err), "pagk_frame_set_device_batch: context %d lives on device %d, the first on %d", j, ctxs[j]->device, lead->device);
            return PAGK_E_ARG;
        }
    HIPCHK(lead, hipSetDevice(lead->device));
    // the slots first (allocation, level pointers); then: can every frame go through the single-launch kernel?
    bool fused = k > 1;
    for (int j = 0; j < k; j++) {
        pagk_ctx *c = ctxs[j];
        FrameSlot &s = c->slots[slot[j]];
        s.valid = false;
        int rc = slot_reserve(c, s, width[j], height[j], pyramids);
        if (rc) {
            if (c != lead) snprintf(lead->err, sizeof(lead->err), "stream %d: %s", j, c->err);
            return rc;
        }
        fused = fused && pyramid_fusable(s) && !c->unfused_pyramid;
    }
    if (!fused) {   // odd parents, more than four levels, a single frame: every frame as its own launch(es) on its own context
        for (int j = 0; j < k; j++) {
            pagk_ctx *c = ctxs[j];
            FrameSlot &s = c->slots[slot[j]];
            int rc = slot_build(c, s, static_cast<const uint8_t *>(d_data[j]), step[j], step[j] == width[j]);
            s.pad0 = (int)(step[j] - width[j] > 2 ? 2 : step[j] - width[j]);
            if (rc) {
                if (c != lead) snprintf(lead->err, sizeof(lead->err), "stream %d: %s", j, c->err);
                return rc;
            }
        }
        return PAGK_OK;
    }
    int rc = PAGK_OK;
    pagk_ctx::BatchDesc *desc = batch_desc_take(lead, &rc);
    if (!desc) return rc;
    PyrBatchEntry *he = static_cast<PyrBatchEntry *>(desc->host);
    int nb = 0;
    for (int j = 0; j < k; j++) {
        FrameSlot &s = ctxs[j]->slots[slot[j]];
        memset(&he[j], 0, sizeof he[j]);
        he[j].block_base = nb;
        nb += make_pyr_args(s, static_cast<const uint8_t *>(d_data[j]), step[j], step[j] == width[j], &he[j].a);
    }
    // the launch overwrites slots the other contexts' streams may still be reading, and reads images they may be writing ...
    for (int j = 1; j < k; j++)
        if (ctxs[j]->stream != lead->stream) {
            HIPCHK(lead, hipEventRecord(ctxs[j]->ev_batch, ctxs[j]->stream));
            HIPCHK(lead, hipStreamWaitEvent(lead->stream, ctxs[j]->ev_batch, 0));
        }
    HIPCHK(lead, hipMemcpyAsync(desc->dev, he, (size_t)k * sizeof(PyrBatchEntry), hipMemcpyHostToDevice, lead->stream));
    if (lead->ev_pyr[0] && !in_capture(lead)) HIPCHK(lead, hipEventRecord(lead->ev_pyr[0], lead->stream));
    hipLaunchKernelGGL(k_pyramid_fused_batch, dim3(nb), dim3(256), 0, lead->stream, static_cast<const PyrBatchEntry *>(desc->dev), (int)k);
    HIPCHK(lead, hipGetLastError());
    if (lead->ev_pyr[1] && !in_capture(lead)) HIPCHK(lead, hipEventRecord(lead->ev_pyr[1], lead->stream));
    if (!in_capture(lead)) lead->pyr_timed = true;
    if ((rc = batch_desc_used(lead, desc)) != PAGK_OK) return rc;
    // ... and what those streams do next sees the pyramids
    bool others = false;
    for (int j = 1; j < k; j++) others = others || ctxs[j]->stream != lead->stream;
    if (others) {
        HIPCHK(lead, hipEventRecord(lead->ev_batch, lead->stream));
        for (int j = 1; j < k; j++)
            if (ctxs[j]->stream != lead->stream) HIPCHK(lead, hipStreamWaitEvent(ctxs[j]->stream, lead->ev_batch, 0));
    }
    for (int j = 0; j < k; j++) {
        FrameSlot &s = ctxs[j]->slots[slot[j]];
        s.wrap0 = step[j] == width[j];
        s.pad0 = (int)(step[j] - width[j] > 2 ? 2 : step[j] - width[j]);
        s.img0 = static_cast<const uint8_t *>(d_data[j]), s.pitch0 = step[j];
        s.valid = true;
    }
    return PAGK_OK;
}

// ---- rectification: cv::remap + RGB-to-gray of a raw camera frame into a frame slot (include/pagk.h "rectification") ----
void pagk_rectify_params_default(pagk_rectify_params *p)
{
    if (!p) return;
    p->channels = 1;
    p->gray_weight[0] = 4899, p->gray_weight[1] = 9617, p->gray_weight[2] = 1868;   // CV_RGB2GRAY on R, G, B (OpenCV 3.4)
    p->gray_shift = 14;
}

int pagk_rectify_params_check(const pagk_rectify_params *p)
{
    if (!p) return PAGK_E_ARG;
    if (p->channels != 1 && p->channels != 3 && p->channels != 4) return PAGK_E_ARG;
    if (p->channels == 1) return PAGK_OK;   // (no gray step: the weights are not read)
    if (p->gray_shift < 1 || p->gray_shift > 15) return PAGK_E_ARG;
    int64_t sum = 0;
    for (int k = 0; k < 3; k++) {
        if (p->gray_weight[k] < 0) return PAGK_E_ARG;
        sum += p->gray_weight[k];
    }
    return sum == (int64_t)1 << p->gray_shift ? PAGK_OK : PAGK_E_ARG;
}

int pagk_undistort_maps(double fx, double fy, double cx, double cy, const double *dist_coef, int32_t n_dist_coef,
                        double new_fx, double new_fy, double new_cx, double new_cy, int32_t width, int32_t height,
                        float *map_x, float *map_y)
{
    if (!map_x || !map_y || width < 1 || height < 1 || (n_dist_coef != 0 && n_dist_coef != 4 && n_dist_coef != 5)) return PAGK_E_ARG;
    if (n_dist_coef > 0 && !dist_coef) return PAGK_E_ARG;
    if (!std::isfinite(new_fx) || !std::isfinite(new_fy) || new_fx == 0.0 || new_fy == 0.0) return PAGK_E_ARG;
    const double k1 = n_dist_coef >= 4 ? dist_coef[0] : 0.0, k2 = n_dist_coef >= 4 ? dist_coef[1] : 0.0;
    const double p1 = n_dist_coef >= 4 ? dist_coef[2] : 0.0, p2 = n_dist_coef >= 4 ? dist_coef[3] : 0.0;
    const double k3 = n_dist_coef >= 5 ? dist_coef[4] : 0.0;
    for (int32_t r = 0; r < height; r++)
        for (int32_t c = 0; c < width; c++) {
            // one rounding per operation, in exactly this order (the build never contracts a * b + c)
            const double x = ((double)c - new_cx) / new_fx, y = ((double)r - new_cy) / new_fy;
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = (2.0 * x) * y;
            const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
            const double xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
            const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
            map_x[(size_t)r * width + c] = (float)(fx * xd + cx);
            map_y[(size_t)r * width + c] = (float)(fy * yd + cy);
        }
    return PAGK_OK;
}

namespace {

// sx = rne(m * 32) of the definition -> *s; false = "no pixel" (non-finite, or |m * 32| >= 2^31)
bool rect_fixed(float m, int32_t *s)
{
    const float p = m * 32.0f;                       // exact (a power of two), or +-inf
    if (!(std::fabs(p) < 2147483648.0f)) return false;   // (NaN fails the comparison too)
    *s = (int32_t)std::nearbyintf(p);                // round to nearest, ties to even (the default rounding mode)
    return true;
}

inline int32_t sat_i16(int32_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

int rect_check_src(pagk_ctx *ctx, const pagk_rectify_params *params, int32_t sw, int32_t sh, int64_t sstep, const char *what)
{
    if (pagk_rectify_params_check(params) != PAGK_OK) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: channels must be 1, 3 or 4; for 3 and 4 the gray weights must be non-negative and sum to 1 << gray_shift, 1 <= gray_shift <= 15", what);
        return PAGK_E_ARG;
    }
    if (!ctx->buf[pagk_ctx::RECT_ENTRIES].ptr) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: no maps set (pagk_rectify_set_maps)", what);
        return PAGK_E_ARG;
    }
    if (sw < 1 || sh < 1 || sw > 32767 || sh > 32767) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: source %d x %d: both dimensions must be in 1 .. 32767 (16-bit tap coordinates)", what, sw, sh);
        return PAGK_E_ARG;
    }
    if (sstep < (int64_t)sw * params->channels) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: src_step %lld is less than src_width * channels = %lld", what, (long long)sstep, (long long)sw * params->channels);
        return PAGK_E_ARG;
    }
    return PAGK_OK;
}

// the kernel: d_raw -> dst (rect_w x rect_h bytes, pitch rect_w); arguments checked by the caller
RectArgs rect_args(pagk_ctx *ctx, const pagk_rectify_params *params, const void *d_raw, int32_t sw, int32_t sh, int64_t sstep,
                   uint8_t *dst)
{
    RectArgs a;
    memset(&a, 0, sizeof a);
    a.entries = static_cast<const RectEntry *>(ctx->buf[pagk_ctx::RECT_ENTRIES].ptr);
    a.src = static_cast<const uint8_t *>(d_raw);
    a.dst = dst;
    a.src_step = sstep;
    a.W = ctx->rect_w, a.H = ctx->rect_h, a.wp = ctx->rect_wp, a.Ws = sw, a.Hs = sh;
    a.gw0 = params->gray_weight[0], a.gw1 = params->gray_weight[1], a.gw2 = params->gray_weight[2], a.gshift = params->gray_shift;
    return a;
}

int rect_launch(pagk_ctx *ctx, const pagk_rectify_params *params, const void *d_raw, int32_t sw, int32_t sh, int64_t sstep,
                uint8_t *dst)
{
    const RectArgs a = rect_args(ctx, params, d_raw, sw, sh, sstep, dst);
    const long long threads = (long long)(a.wp >> 2) * a.H;
    const dim3 grd((unsigned)((threads + 255) / 256)), blk(256);
    const bool pair = sw >= 2;   // the two-taps-per-load form needs a second pixel in every source row
    if (params->channels == 1) {
        if (pair) hipLaunchKernelGGL((k_rectify<1, true>), grd, blk, 0, ctx->stream, a);
        else hipLaunchKernelGGL((k_rectify<1, false>), grd, blk, 0, ctx->stream, a);
    } else if (params->channels == 3) {
        if (pair) hipLaunchKernelGGL((k_rectify<3, true>), grd, blk, 0, ctx->stream, a);
        else hipLaunchKernelGGL((k_rectify<3, false>), grd, blk, 0, ctx->stream, a);
    } else {
        if (pair) hipLaunchKernelGGL((k_rectify<4, true>), grd, blk, 0, ctx->stream, a);
        else hipLaunchKernelGGL((k_rectify<4, false>), grd, blk, 0, ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

int rect_into_slot(pagk_ctx *ctx, int32_t slot, const pagk_rectify_params *params, const void *raw, bool raw_on_host,
                   int32_t sw, int32_t sh, int64_t sstep, int32_t pyramids, const char *what)
{
    if (!ctx || slot < 0 || slot >= kSlots || !raw || pyramids < 1 || pyramids > PAGK_MAX_PYRAMIDS) return PAGK_E_ARG;
    int rc = rect_check_src(ctx, params, sw, sh, sstep, what);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FrameSlot &s = ctx->slots[slot];
    // the maps decide the size: an unused slot takes it; one that holds a frame of another size is the caller's mistake
    // (two cameras' frames mixed up), not something to resize silently
    if (slot < kUserSlots && s.w && (s.w != ctx->rect_w || s.h != ctx->rect_h)) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: slot %d holds a %d x %d frame, the maps are %d x %d", what, slot, s.w, s.h, ctx->rect_w, ctx->rect_h);
        return PAGK_E_ARG;
    }
    s.valid = false;
    if ((rc = slot_reserve(ctx, s, ctx->rect_w, ctx->rect_h, pyramids))) return rc;
    if (raw_on_host) {
        const size_t row = (size_t)sw * params->channels;
        // the context's staging buffer for a raw frame that arrives from the host
        DevBuf &stage = ctx->buf[pagk_ctx::RECT_STAGE];
        if ((rc = reserve(ctx, stage, row * sh, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the raw frame's staging buffer",
                          "issue the same call once before capturing"))) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(stage.ptr, row, raw, (size_t)sstep, row, (size_t)sh, hipMemcpyHostToDevice, ctx->stream));
        raw = stage.ptr, sstep = (int64_t)row;
    }
    if ((rc = rect_launch(ctx, params, raw, sw, sh, sstep, s.u8[0]))) return rc;
    rc = slot_build(ctx, s, s.u8[0], s.w, 1);   // as frame_upload_any leaves a continuous image: wrap0 = 1 ...
    s.pad0 = 0;                                  // ... pad0 = 0
    return rc;
}

}  // namespace

int pagk_rectify_set_maps(pagk_ctx *ctx, const float *map_x, const float *map_y, int32_t width, int32_t height,
                          int64_t step_bytes)
{
    if (!ctx || !map_x || !map_y || width < 1 || height < 1 || step_bytes < (int64_t)width * 4) return PAGK_E_ARG;
    if (width >= (1 << 24) || height >= (1 << 24) || (int64_t)width * height >= (1ll << 31)) return PAGK_E_ARG;   // (check_image)
    NOT_WHILE_CAPTURING(ctx, "pagk_rectify_set_maps");
    if (in_capture(ctx)) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_rectify_set_maps allocates and synchronises: not inside a stream capture");
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int wp = (width + 3) & ~3;
    std::vector<RectEntry> e;
    try {
        e.assign((size_t)wp * height, RectEntry{kRectNoPixelLo, 0u});
    } catch (const std::bad_alloc &) {
        return PAGK_E_NOMEM;
    }
    for (int32_t r = 0; r < height; r++) {
        const float *mx = reinterpret_cast<const float *>(reinterpret_cast<const char *>(map_x) + (size_t)r * step_bytes);
        const float *my = reinterpret_cast<const float *>(reinterpret_cast<const char *>(map_y) + (size_t)r * step_bytes);
        for (int32_t c = 0; c < width; c++) {
            int32_t sx, sy;
            if (!rect_fixed(mx[c], &sx) || !rect_fixed(my[c], &sy)) continue;   // "no pixel"
            const int32_t ix = sat_i16(sx >> 5), iy = sat_i16(sy >> 5);         // arithmetic shifts: negative coordinates floor
            RectEntry &o = e[(size_t)r * wp + c];
            o.lo = ((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16);
            o.hi = (uint32_t)(sx & 31) | ((uint32_t)(sy & 31) << 8);
        }
    }
    const size_t bytes = e.size() * sizeof(RectEntry);
    DevBuf &entries = ctx->buf[pagk_ctx::RECT_ENTRIES];
    if (wp != ctx->rect_wp || height != ctx->rect_h || !entries.ptr) {   // keyed by the maps' size, not grow-only
        int rc = no_live_graphs(ctx, "the map entries (maps of another size)", "set maps of this size before capturing");
        if (rc) return rc;
        // nothing enqueued may still read the old entries
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if ((rc = release(ctx, entries))) return rc;
        ctx->rect_w = ctx->rect_h = ctx->rect_wp = 0;
        HIPCHK(ctx, hipMalloc(&entries.ptr, bytes));
        entries.bytes = bytes;
    }
    ctx->rect_w = width, ctx->rect_h = height, ctx->rect_wp = wp;
    HIPCHK(ctx, hipMemcpyAsync(entries.ptr, e.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (e goes out of scope)
    return PAGK_OK;
}

int pagk_frame_rectify_device(pagk_ctx *ctx, int32_t slot, const pagk_rectify_params *params, const void *d_raw,
                              int32_t src_width, int32_t src_height, int64_t src_step, int32_t pyramids)
{
    if (!ctx || slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    return rect_into_slot(ctx, slot, params, d_raw, false, src_width, src_height, src_step, pyramids, "pagk_frame_rectify_device");
}

int pagk_frame_rectify_pinned(pagk_ctx *ctx, int32_t slot, const pagk_rectify_params *params, const void *raw,
                              int32_t src_width, int32_t src_height, int64_t src_step, int32_t pyramids)
{
    if (!ctx || slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    return rect_into_slot(ctx, slot, params, raw, true, src_width, src_height, src_step, pyramids, "pagk_frame_rectify_pinned");
}

int pagk_rectify(pagk_ctx *ctx, const pagk_rectify_params *params, const void *raw, int32_t src_width, int32_t src_height,
                 int64_t src_step, uint8_t *dst, int64_t dst_step)
{
    if (!ctx || !raw || !dst) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_rectify");
    if (ctx->buf[pagk_ctx::RECT_ENTRIES].ptr && dst_step < ctx->rect_w) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_rectify: dst_step %lld is less than the maps' width %d", (long long)dst_step, ctx->rect_w);
        return PAGK_E_ARG;
    }
    int rc = rect_into_slot(ctx, 4, params, raw, true, src_width, src_height, src_step, 1, "pagk_rectify");
    if (rc) return rc;
    const FrameSlot &s = ctx->slots[4];
    HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)dst_step, s.u8[0], (size_t)s.w, (size_t)s.w, (size_t)s.h, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PAGK_OK;
}

int pagk_frame_download_level(pagk_ctx *ctx, int32_t slot, int32_t level, uint8_t *dst, int32_t *width,
                              int32_t *height)
{
    if (!ctx || slot < 0 || slot >= kUserSlots || !dst) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_frame_download_level");
    FrameSlot &s = ctx->slots[slot];
    if (!s.valid || level < 0 || level >= s.L || (level == 0 && !s.img0)) return PAGK_E_ARG;
    int lw[kMaxLevels], lh[kMaxLevels];
    level_dims(s.w, s.h, s.L, lw, lh);
    if (level == 0)   // where the pyramid was built from: the slot's own copy, or the caller's device image read in place
        HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)s.w, s.img0, (size_t)s.pitch0, (size_t)s.w, (size_t)s.h, hipMemcpyDeviceToHost, ctx->stream));
    else
        HIPCHK(ctx, hipMemcpyAsync(dst, s.u8[level], (size_t)lw[level] * lh[level], hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (width) *width = lw[level];
    if (height) *height = lh[level];
    return PAGK_OK;
}

int pagk_track_device(pagk_ctx *ctx, const pagk_params *params, int32_t slot_ref, int32_t slot_cur, int32_t n,
                      const float *d_pt_ref_un, const float *d_pt_init_un, const float *d_affine,
                      const uint8_t *d_status_in, const pagk_outputs *d_out)
{
    if (!ctx) return PAGK_E_ARG;
    int rc = check_params(params);
    if (rc) return rc;
    if (slot_ref < 0 || slot_ref >= kUserSlots || slot_cur < 0 || slot_cur >= kUserSlots) return PAGK_E_ARG;
    FrameSlot &sr = ctx->slots[slot_ref], &sc = ctx->slots[slot_cur];
    if (!sr.valid || !sc.valid || sr.L < params->pyramids || sc.L < params->pyramids) return PAGK_E_ARG;
    if (sr.w != sc.w || sr.h != sc.h) return PAGK_E_ARG;
    if (n < 0 || !d_out || !d_out->pt_un || !d_out->status) return PAGK_E_ARG;
    if (n > 0 && (!d_pt_ref_un || !d_status_in)) return PAGK_E_ARG;
    if (n > 0 && params->has_gyro_predict_initial && !d_pt_init_un) return PAGK_E_ARG;
    if (n > 0 && params->consider_affine && !d_affine) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return launch_track(ctx, params, sr, sc, n, d_pt_ref_un, d_pt_init_un, d_affine, d_status_in, d_out);
}

// One launch for k camera streams that share this device (BASELINE configs[4], "batched multi-camera").  The reference
// builds one PatchMatch per tracker (src/gyro_aided_tracker.cpp:276-283); k trackers' calls are k independent feature
// sets over k image pairs.  As k launches they are k launches of a few thousand features -- the latency variants' size,
// or the throughput variant run as k concurrent grids that hold each other's slots; as ONE launch of variant 7 (four
// features per wave, one pyramid level per wave; a quad carries its stream) they are a launch of several rounds of
// resident waves, which is where that variant is at its rate.  Per stream: the bits of its own pagk_track_device.
int pagk_track_device_batch(pagk_ctx *const *ctxs, int32_t k, const pagk_params *params, const int32_t *slot_ref,
                            const int32_t *slot_cur, const int32_t *n, const float *const *d_pt_ref_un,
                            const float *const *d_pt_init_un, const float *const *d_affine,
                            const uint8_t *const *d_status_in, const pagk_outputs *d_out)
{
    if (!ctxs || k < 1 || k > 64 || !slot_ref || !slot_cur || !n || !d_pt_ref_un || !d_status_in || !d_out) return PAGK_E_ARG;
    for (int j = 0; j < k; j++)
        if (!ctxs[j]) return PAGK_E_ARG;
    pagk_ctx *lead = ctxs[0];
    int rc = check_params(params);
    if (rc) return rc;
    long long total_n = 0;
    int total_q = 0;
    for (int j = 0; j < k; j++) {
        pagk_ctx *c = ctxs[j];
        if (c->device != lead->device) {
            snprintf(lead->err, sizeof(lead->err), "pagk_track_device_batch: context %d lives on device %d, the first on %d", j, c->device, lead->device);
            return PAGK_E_ARG;
        }
        if (slot_ref[j] < 0 || slot_ref[j] >= kUserSlots || slot_cur[j] < 0 || slot_cur[j] >= kUserSlots) return PAGK_E_ARG;
        const FrameSlot &sr = c->slots[slot_ref[j]], &sc = c->slots[slot_cur[j]];
        if (!sr.valid || !sc.valid || sr.L < params->pyramids || sc.L < params->pyramids || sr.w != sc.w || sr.h != sc.h) return PAGK_E_ARG;
        if (n[j] < 0 || !d_out[j].pt_un || !d_out[j].status) return PAGK_E_ARG;
        if (n[j] > 0 && (!d_pt_ref_un[j] || !d_status_in[j])) return PAGK_E_ARG;
        if (n[j] > 0 && params->has_gyro_predict_initial && (!d_pt_init_un || !d_pt_init_un[j])) return PAGK_E_ARG;
        if (n[j] > 0 && params->consider_affine && (!d_affine || !d_affine[j])) return PAGK_E_ARG;
        total_n += n[j];
        total_q += (n[j] + 3) / 4;
    }
    HIPCHK(lead, hipSetDevice(lead->device));
    // (the template-Jacobian mode has no batched kernel: k launches)
    const bool batched = params->inverse == 0 && select_batched(select_in(lead, params, 0), total_n, total_q);
    if (!batched) {
        // every stream as its own launch on its own context (small batches, NCC launches, a forced variant)
        for (int j = 0; j < k; j++) {
            pagk_ctx *c = ctxs[j];
            rc = launch_track(c, params, c->slots[slot_ref[j]], c->slots[slot_cur[j]], n[j], d_pt_ref_un[j],
                              d_pt_init_un ? d_pt_init_un[j] : nullptr, d_affine ? d_affine[j] : nullptr, d_status_in[j], &d_out[j]);
            if (rc) {
                if (c != lead) snprintf(lead->err, sizeof(lead->err), "stream %d: %s", j, c->err);
                return rc;
            }
        }
        return PAGK_OK;
    }
    TrackArgs a;
    memset(&a, 0, sizeof a);
    a.n_levels = params->pyramids;
    for (int l = 0; l < params->pyramids; l++) a.scales[l] = l == 0 ? 1.0f : (float)((double)a.scales[l - 1] * 0.5);  // :66,:73
    fill_param_args(a, params);
    a.n = 4 * total_q;   // features numbered through the batch, each stream padded to whole quads
    a.batch_k = k;
    // the stream descriptors: pinned source -> device.  The copy is asynchronous and, inside a capture, a node that is
    // replayed later: the pair it uses is this launch's alone until the launch is over (ring) / the graph's (capture)
    pagk_ctx::BatchDesc *desc = batch_desc_take(lead, &rc);
    if (!desc) return rc;
    BatchStream *hb = static_cast<BatchStream *>(desc->host);
    int qb = 0;
    for (int j = 0; j < k; j++) {
        pagk_ctx *c = ctxs[j];
        BatchStream &B = hb[j];
        memset(&B, 0, sizeof B);
        for (int l = 0; l < params->pyramids; l++) {
            fill_level(B.l1[l], c->slots[slot_ref[j]], l);
            fill_level(B.l2[l], c->slots[slot_cur[j]], l);
        }
        B.pt_ref = d_pt_ref_un[j];
        B.pt_init = d_pt_init_un ? d_pt_init_un[j] : nullptr;
        B.affine = d_affine ? d_affine[j] : nullptr;
        B.status_in = d_status_in[j];
        B.pt_un = d_out[j].pt_un, B.pt_dist = d_out[j].pt_dist, B.status = d_out[j].status;
        B.pix_err = d_out[j].pix_err, B.dist_pred = d_out[j].dist_pred, B.ncc = d_out[j].ncc, B.iters = d_out[j].iters;
        B.n = n[j];
        B.quad_base = qb;
        qb += (n[j] + 3) / 4;
    }
    // the launch reads what the other contexts' streams produced (their pyramids, their prediction kernels' outputs) ...
    for (int j = 1; j < k; j++)
        if (ctxs[j]->stream != lead->stream) {
            HIPCHK(lead, hipEventRecord(ctxs[j]->ev_batch, ctxs[j]->stream));
            HIPCHK(lead, hipStreamWaitEvent(lead->stream, ctxs[j]->ev_batch, 0));
        }
    HIPCHK(lead, hipMemcpyAsync(desc->dev, hb, (size_t)k * sizeof(BatchStream), hipMemcpyHostToDevice, lead->stream));
    a.batch = static_cast<const BatchStream *>(desc->dev);
    // workspaces of a one-level-per-wave launch (launch_track), for the batch's quads; no hand-over
    const int nch = patch_shape(a.half).nch, nq = total_q, waves = nq * params->pyramids;
    const size_t need = (size_t)waves * 4 * nch * 64 * sizeof(float);
    const LevelsLayout lvl = levels_layout((size_t)a.n, (size_t)nq, params->pyramids);
    uint8_t *lb = nullptr;
    if ((rc = quad_workspace(lead, need, &lvl, &a, &lb))) return rc;
    HIPCHK(lead, hipMemsetAsync(lb, 0, lvl.susp_count, lead->stream));
    if (lead->ev_trk[0] && !in_capture(lead)) HIPCHK(lead, hipEventRecord(lead->ev_trk[0], lead->stream));
    const bool lean = !a.penalty && a.solver == 0;
    HIPCHK(lead, launch(track_kernels_of(a.half).batch[lean], waves, 64, 0, lead->stream, a));
    if ((rc = batch_desc_used(lead, desc)) != PAGK_OK) return rc;
    if (lead->ev_trk[1] && !in_capture(lead)) HIPCHK(lead, hipEventRecord(lead->ev_trk[1], lead->stream));
    if (!in_capture(lead)) lead->trk_timed = true;
    // ... and whatever those streams do next sees its results
    bool others = false;
    for (int j = 1; j < k; j++) others = others || ctxs[j]->stream != lead->stream;
    if (others) {
        HIPCHK(lead, hipEventRecord(lead->ev_batch, lead->stream));
        for (int j = 1; j < k; j++)
            if (ctxs[j]->stream != lead->stream) HIPCHK(lead, hipStreamWaitEvent(ctxs[j]->stream, lead->ev_batch, 0));
    }
    for (int j = 0; j < k; j++) {
        ctxs[j]->last_variant = 7;
        ctxs[j]->last_handover = false;
    }
    return PAGK_OK;
}

// Tracking of (slot_ref, slot_cur) with the pyramid of ANOTHER frame (device image d_next) built into slot_next
// by the same launch when the 4-wave kernel is selected; otherwise two launches.  Same results as
// pagk_frame_set_device(slot_next, ...) followed by pagk_track_device(...).
int pagk_track_device_fused(pagk_ctx *ctx, const pagk_params *params, int32_t slot_ref, int32_t slot_cur, int32_t n,
                            const float *d_pt_ref_un, const float *d_pt_init_un, const float *d_affine,
                            const uint8_t *d_status_in, const pagk_outputs *d_out, int32_t slot_next,
                            const void *d_next, int32_t width, int32_t height, int64_t step, int32_t pyramids)
{
    if (!ctx || !d_next || slot_next < 0 || slot_next >= kUserSlots || slot_next == slot_ref || slot_next == slot_cur ||
        width < 1 || height < 1 || step < width || pyramids < 1 || pyramids > PAGK_MAX_PYRAMIDS)
        return PAGK_E_ARG;
    if (slot_ref < 0 || slot_ref >= kUserSlots || slot_cur < 0 || slot_cur >= kUserSlots) return PAGK_E_ARG;
    int rc = check_params(params);
    if (rc) return rc;
    FrameSlot &sr = ctx->slots[slot_ref], &sc = ctx->slots[slot_cur], &sn = ctx->slots[slot_next];
    if (!sr.valid || !sc.valid || sr.w != sc.w || sr.h != sc.h || sr.L < params->pyramids || sc.L < params->pyramids)
        return PAGK_E_ARG;
    if (n < 0 || !d_out || !d_out->pt_un || !d_out->status) return PAGK_E_ARG;
    if (n > 0 && (!d_pt_ref_un || !d_status_in)) return PAGK_E_ARG;
    if (n > 0 && params->has_gyro_predict_initial && !d_pt_init_un) return PAGK_E_ARG;
    if (n > 0 && params->consider_affine && !d_affine) return PAGK_E_ARG;
    pagk_image probe{static_cast<const uint8_t *>(d_next), width, height, step};
    if ((rc = check_image(&probe))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    sn.valid = false;
    if ((rc = slot_reserve(ctx, sn, width, height, pyramids))) return rc;
    const uint8_t *src0 = static_cast<const uint8_t *>(d_next);
    const int wrap0 = step == width;
    bool fused = false;
    if (n > 0 && pyramid_fusable(sn) && !ctx->unfused_pyramid) {
        PyrArgs pa;
        const int nb = make_pyr_args(sn, src0, step, wrap0, &pa);
        rc = launch_track(ctx, params, sr, sc, n, d_pt_ref_un, d_pt_init_un, d_affine, d_status_in, d_out, &pa, nb, &fused);
        if (rc) return rc;
        if (fused) {
            sn.wrap0 = wrap0;
            sn.pad0 = (int)(step - width > 2 ? 2 : step - width);
            sn.img0 = src0, sn.pitch0 = step;
            sn.valid = true;
            return PAGK_OK;
        }
    } else {
        rc = launch_track(ctx, params, sr, sc, n, d_pt_ref_un, d_pt_init_un, d_affine, d_status_in, d_out);
        if (rc) return rc;
    }
    rc = slot_build(ctx, sn, src0, step, wrap0);  // the launch selected another variant: pyramid on its own
    sn.pad0 = (int)(step - width > 2 ? 2 : step - width);
    return rc;
}

int pagk_track(pagk_ctx *ctx, const pagk_params *params, const pagk_image *ref, const pagk_image *cur, int32_t n,
               const float *pt_ref_un, const float *pt_init_un, const float *affine, const uint8_t *status_in,
               const pagk_outputs *out)
{
    if (!ctx) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_track");
    int rc = check_params(params);
    if (rc) return rc;
    if ((rc = check_image(ref)) || (rc = check_image(cur))) return rc;
    if (ref->width != cur->width || ref->height != cur->height) return PAGK_E_ARG;
    if ((rc = frame_upload_any(ctx, 4, ref, params->pyramids))) return rc;
    if ((rc = frame_upload_any(ctx, 5, cur, params->pyramids))) return rc;
    return track_host_common(ctx, params, n, pt_ref_un, pt_init_un, affine, status_in, out, ctx->slots[4],
                             ctx->slots[5]);
}

int pagk_track_pyr(pagk_ctx *ctx, const pagk_params *params, int32_t n_levels, const pagk_image *ref_levels,
                   const pagk_image *cur_levels, int32_t n, const float *pt_ref_un, const float *pt_init_un,
                   const float *affine, const uint8_t *status_in, const pagk_outputs *out)
{
    if (!ctx || !ref_levels || !cur_levels) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_track_pyr");
    int rc = check_params(params);
    if (rc) return rc;
    if (n_levels != params->pyramids) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // caller-built pyramids: every level is uploaded and packed as is; level sizes must be
    // the ones CreatePyramids would produce (int(cols*0.5)), but parents may be odd.
    FrameSlot *sl[2] = {&ctx->slots[4], &ctx->slots[5]};
    const pagk_image *lv[2] = {ref_levels, cur_levels};
    for (int k = 0; k < 2; k++) {
        for (int l = 0; l < n_levels; l++)
            if ((rc = check_image(&lv[k][l]))) return rc;
        int w = lv[k][0].width, h = lv[k][0].height;
        for (int l = 1; l < n_levels; l++) {
            w = (int)(w * 0.5);
            h = (int)(h * 0.5);
            if (lv[k][l].width != w || lv[k][l].height != h) return PAGK_E_ARG;
        }
        if (lv[k][0].width != lv[0][0].width || lv[k][0].height != lv[0][0].height) return PAGK_E_ARG;
        FrameSlot &s = *sl[k];
        s.valid = false;
        // reserve without the even-parent restriction
        int lw[kMaxLevels], lh[kMaxLevels];
        for (int l = 0; l < n_levels; l++) lw[l] = lv[k][l].width, lh[l] = lv[k][l].height;
        if ((rc = slot_alloc(ctx, s, lw, lh, n_levels, GROW_FREELY))) return rc;
        dim3 blk(32, 8);
        for (int l = 0; l < n_levels; l++) {
            const pagk_image &im = lv[k][l];
            HIPCHK(ctx, hipMemcpy2DAsync(s.u8[l], (size_t)im.width, im.data, (size_t)im.step, (size_t)im.width,
                                         (size_t)im.height, hipMemcpyHostToDevice, ctx->stream));
            dim3 grd((im.width + 31) / 32, (im.height + 7) / 8);
            hipLaunchKernelGGL(k_build_quads, grd, blk, 0, ctx->stream, (const uint8_t *)s.u8[l], (int64_t)im.width,
                               im.width, im.height, im.step == im.width ? 1 : 0, s.quad[l]);
        }
        HIPCHK(ctx, hipGetLastError());
        s.wrap0 = lv[k][0].step == lv[k][0].width;
        s.pad0 = (int)(lv[k][0].step - lv[k][0].width > 2 ? 2 : lv[k][0].step - lv[k][0].width);
        s.img0 = s.u8[0], s.pitch0 = s.w;
        s.valid = true;
    }
    return track_host_common(ctx, params, n, pt_ref_un, pt_init_un, affine, status_in, out, ctx->slots[4],
                             ctx->slots[5]);
}

// the arguments of k_gyro_predict: of one launch, or of one camera's record of a sequence group
static PredictArgs gyro_predict_args(const pagk_params *params, int32_t width, int32_t height, const float *KRKinv,
                                     const float *r3, const float *d_rot, int32_t n, const float *d_pt_ref_un,
                                     float *d_pt_predict_un, float *d_pt_predict, uint8_t *d_status, float *d_affine,
                                     const uint8_t *d_live)
{
    PredictArgs a;
    memset(&a, 0, sizeof a);
    a.n = n, a.width = width, a.height = height;
    a.half = (float)params->half_patch;
    a.single_homography = params->predict_method == 2;  // ePredictMethod SINGLE_HOMOGRAPHY
    a.fx = params->fx, a.fy = params->fy, a.cx = params->cx, a.cy = params->cy;
    a.fx_inv = (float)(1.0 / (double)params->fx);  // src/gyro_aided_tracker.cpp:66
    a.fy_inv = (float)(1.0 / (double)params->fy);
    a.k1 = params->dist_coef[0], a.k2 = params->dist_coef[1], a.p1 = params->dist_coef[2], a.p2 = params->dist_coef[3];
    a.k3 = params->n_dist_coef == 5 ? params->dist_coef[4] : 0.0f;
    if (d_rot) {
        a.d_rot = d_rot;
    } else {
        for (int k = 0; k < 6; k++) a.K[k] = KRKinv[k];
        a.r31 = r3[0], a.r32 = r3[1], a.r33 = r3[2];
    }
    // (B B^T)^-1 for B = +-h corners (:73-78): B B^T = diag(4h^2); cv::Mat::inv of a 2x2 goes through
    // the double determinant
    const float m00 = 4.0f * a.half * a.half;
    const double det = (double)m00 * m00, dinv = det != 0 ? 1. / det : 0;
    a.inv00 = (float)(m00 * dinv);
    a.inv01 = (float)(-0.0f * dinv);
    a.pt_ref = d_pt_ref_un;
    a.pt_un = d_pt_predict_un;
    a.pt_dist = d_pt_predict;
    a.status = d_status;
    a.affine = d_affine;
    a.live = d_live;
    return a;
}

static int gyro_predict_any(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                            const float *KRKinv, const float *r3, const float *d_rot, int32_t n,
                            const float *d_pt_ref_un, float *d_pt_predict_un, float *d_pt_predict, uint8_t *d_status,
                            float *d_affine, const uint8_t *d_live = nullptr)
{
    if (!ctx || !params || (!d_rot && (!KRKinv || !r3)) || n < 0 || width < 1 || height < 1) return PAGK_E_ARG;
    if (params->half_patch < 1 || params->half_patch > PAGK_MAX_HALF_PATCH) return PAGK_E_ARG;
    if (n > 0 && (!d_pt_ref_un || !d_pt_predict_un || !d_pt_predict || !d_status)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const PredictArgs a = gyro_predict_args(params, width, height, KRKinv, r3, d_rot, n, d_pt_ref_un, d_pt_predict_un,
                                            d_pt_predict, d_status, d_affine, d_live);
    if (n > 0) {
        hipLaunchKernelGGL(k_gyro_predict, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, a);
        HIPCHK(ctx, hipGetLastError());
    }
    return PAGK_OK;
}

int pagk_gyro_predict_device(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                             const float *KRKinv, const float *r3, int32_t n, const float *d_pt_ref_un,
                             float *d_pt_predict_un, float *d_pt_predict, uint8_t *d_status, float *d_affine)
{
    return gyro_predict_any(ctx, params, width, height, KRKinv, r3, nullptr, n, d_pt_ref_un, d_pt_predict_un,
                            d_pt_predict, d_status, d_affine);
}

int pagk_gyro_predict_device_rot(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                                 const float *d_rot, int32_t n, const float *d_pt_ref_un, float *d_pt_predict_un,
                                 float *d_pt_predict, uint8_t *d_status, float *d_affine)
{
    if (!d_rot) return PAGK_E_ARG;
    return gyro_predict_any(ctx, params, width, height, nullptr, nullptr, d_rot, n, d_pt_ref_un, d_pt_predict_un,
                            d_pt_predict, d_status, d_affine);
}

int pagk_gyro_predict_device_live(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                                  const float *d_rot, int32_t n, const float *d_pt_ref_un, const uint8_t *d_live,
                                  float *d_pt_predict_un, float *d_pt_predict, uint8_t *d_status, float *d_affine)
{
    if (!d_rot || (n > 0 && !d_live)) return PAGK_E_ARG;
    return gyro_predict_any(ctx, params, width, height, nullptr, nullptr, d_rot, n, d_pt_ref_un, d_pt_predict_un,
                            d_pt_predict, d_status, d_affine, d_live);
}

// GyroAidedTracker::GyroPredictFeaturesAndOpticalFlowRefined, Step 3,
// src/gyro_aided_tracker.cpp:289-341.  O(n) host arithmetic on the gathered results.
int pagk_post_filter(int32_t n, int32_t half_patch, const uint8_t *status_pm, const double *pix_err,
                     const double *dist_pred, const float *pt_pm, const float *pt_pm_un, uint8_t *status_out,
                     float *pt_predict, float *pt_predict_un)
{
    if (n < 0 || (n > 0 && (!status_pm || !pix_err || !dist_pred || !status_out))) return PAGK_E_ARG;
    double sum = 0;
    int cnt = 0;
    for (int i = 0; i < n; ++i)
        if (status_pm[i]) {  // :298
            sum += pix_err[i];
            cnt++;
        }
    const double avg = sum / cnt;  // :305 (cnt == 0 -> NaN -> threshold falls back to h)
    const double th_pix = 4.0 * avg > half_patch ? 4.0 * avg : half_patch;  // :308
    const double th_dist = half_patch * 4.0;                                // :312
    int kept = 0;
    for (int i = 0; i < n; i++) {  // :318
        const bool ok = status_pm[i] && pix_err[i] < th_pix && dist_pred[i] < th_dist;
        status_out[i] = ok ? 1 : 0;
        if (!ok) continue;
        if (pt_predict && pt_pm) {
            pt_predict[2 * i] = pt_pm[2 * i];
            pt_predict[2 * i + 1] = pt_pm[2 * i + 1];
        }
        if (pt_predict_un && pt_pm_un) {
            pt_predict_un[2 * i] = pt_pm_un[2 * i];
            pt_predict_un[2 * i + 1] = pt_pm_un[2 * i + 1];
        }
        kept++;
    }
    return kept;
}


// Step 3 on the device (k_post_filter): the same mask, points, count and thresholds as pagk_post_filter, bit for bit.
int pagk_post_filter_device(pagk_ctx *ctx, int32_t n, int32_t half_patch, const uint8_t *d_status_pm,
                            const double *d_pix_err, const double *d_dist_pred, const float *d_pt_pm,
                            const float *d_pt_pm_un, uint8_t *d_status_out, float *d_pt_predict,
                            float *d_pt_predict_un, int32_t *d_kept, double *d_thresholds)
{
    if (!ctx || n < 0 || !d_kept) return PAGK_E_ARG;
    if (n > 0 && (!d_status_pm || !d_pix_err || !d_dist_pred || !d_status_out)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_post_filter, dim3(1), dim3(1024), 0, ctx->stream, n, half_patch, d_status_pm, d_pix_err,
                       d_dist_pred, d_pt_pm, d_pt_pm_un, d_status_out, d_pt_predict, d_pt_predict_un, d_kept, d_thresholds);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

// ---- corner detection (pagk_detect_kernel.h) -------------------------------------------------------------------
namespace {

bool detect_params_ok(const pagk_detect_params *d)
{
    return d && std::isfinite(d->quality_level) && d->quality_level >= 0.0 && std::isfinite(d->min_distance) &&
           d->min_distance >= 0.0 && std::isfinite(d->harris_k) && d->raw_cap >= 0;
}

// at most one pixel of any 2 x 2 block passes the non-maximum test
int64_t detect_raw_bound(int w, int h) { return (int64_t)((w - 2 + 1) / 2) * ((h - 2 + 1) / 2); }

// The detector's workspace for one call: control words | response map | sort keys (a power of two, at least one sort
// block) | the fused call's candidate list | its plan's spare info | the distance grid when it does not fit the LDS.
struct DetectWs {
    int32_t *ctl = nullptr, *grid = nullptr;
    float *R = nullptr, *cand = nullptr;
    uint64_t *keys = nullptr;
    uint32_t key_slots = 0;
    int32_t raw_cap = 0, cell = 1, grid_w = 1, grid_h = 1, reach = 1;
};

int detect_workspace(pagk_ctx *ctx, const pagk_detect_params *det, int w, int h, int cap, DetectWs *ws)
{
    const int64_t bound = detect_raw_bound(w, h);
    const int64_t raw_cap = det->raw_cap > 0 ? det->raw_cap : bound;
    if (raw_cap > (1 << 30)) return PAGK_E_ARG;
    uint32_t slots = kDetSortBlock;
    while ((int64_t)slots < raw_cap) slots <<= 1;
    // cells of at most min_distance / sqrt(2) pixels: two pixels of one cell are closer than min_distance
    const double d = det->min_distance;
    int64_t cell = (int64_t)std::floor(d / std::sqrt(2.0));
    const int64_t longest = w > h ? w : h;
    cell = cell < 1 ? 1 : (cell > longest ? longest : cell);
    const int64_t gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
    int64_t reach = (int64_t)std::ceil(d / (double)cell);
    reach = reach > longest ? longest : reach;
    const bool grid_global = d >= 1.0 && gw * gh > kDetGridLds;
    const size_t px = (size_t)w * h;
    const size_t sizes[5] = {256, px * 4, (size_t)slots * 8, (size_t)cap * 8, grid_global ? (size_t)(gw * gh) * 4 : 0};
    const Layout<5> lay(sizes);
    int rc = reserve(ctx, ctx->buf[pagk_ctx::DET], lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the detector's workspace",
                     "run the call once with this image size, raw_cap, cap and min_distance before capturing");
    if (rc) return rc;
    void *b = ctx->buf[pagk_ctx::DET].ptr;
    ws->ctl = lay.at<int32_t>(b, 0);
    ws->R = lay.at<float>(b, 1);
    ws->keys = lay.at<uint64_t>(b, 2);
    ws->cand = lay.at<float>(b, 3);
    ws->grid = grid_global ? lay.at<int32_t>(b, 4) : nullptr;
    ws->key_slots = slots;
    ws->raw_cap = (int32_t)raw_cap;
    ws->cell = (int32_t)cell, ws->grid_w = (int32_t)gw, ws->grid_h = (int32_t)gh, ws->reach = (int32_t)reach;
    return PAGK_OK;
}

int detect_response_launch(pagk_ctx *ctx, const FrameSlot &s, const uint8_t *d_mask, double harris_k, const DetectWs &ws,
                           const int32_t *d_skip)
{
    hipLaunchKernelGGL(k_detect_response, dim3((s.w + kDetTileW - 1) / kDetTileW, (s.h + kDetTileH - 1) / kDetTileH), dim3(256),
                       0, ctx->stream, s.img0, s.pitch0, s.w, s.h, d_mask, harris_k, ws.R, ws.ctl, d_skip);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

// The detector's launches on frame slot `s`.  d_max_corners / d_skip: device words or NULL.  The first two control
// words (Rmax, the raw count) are cleared here; the fused call's plan (words 2, 3) is written in front of this.
int detect_launch(pagk_ctx *ctx, const pagk_detect_params *det, const FrameSlot &s, const uint8_t *d_mask, int32_t cap,
                  const int32_t *d_max_corners, const int32_t *d_skip, float *d_corners, int32_t *d_info, const DetectWs &ws)
{
    HIPCHK(ctx, hipMemsetAsync(ws.ctl, 0, 8, ctx->stream));
    int rc = detect_response_launch(ctx, s, d_mask, det->harris_k, ws, d_skip);
    if (rc) return rc;
    hipLaunchKernelGGL(k_detect_nms, dim3((s.w + 63) / 64, (s.h + 3) / 4), dim3(256), 0, ctx->stream, ws.R, s.w, s.h, d_mask,
                       det->quality_level, ws.ctl, ws.keys, ws.raw_cap, d_skip);
    HIPCHK(ctx, hipGetLastError());
    // bitonic network over key_slots: every launch is there whatever the count; the blocks that hold nothing return
    const uint32_t N = ws.key_slots;
    const size_t sort_lds = (size_t)kDetSortBlock * sizeof(uint64_t);   // 128 KiB: beyond the default limit of a launch
    if (!in_capture(ctx))   // (a capture follows a direct run of the same call, which has set it)
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_detect_sort_local),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds));
    hipLaunchKernelGGL(k_detect_sort_local, dim3(N / kDetSortBlock), dim3(1024), sort_lds, ctx->stream, ws.keys, ws.ctl,
                       ws.raw_cap, 0u, d_skip);
    for (uint32_t k = 2 * kDetSortBlock; k <= N; k <<= 1) {
        for (uint32_t j = k >> 1; j >= (uint32_t)kDetSortBlock; j >>= 1)
            hipLaunchKernelGGL(k_detect_sort_step, dim3(N / 2 / 256), dim3(256), 0, ctx->stream, ws.keys, ws.ctl, ws.raw_cap, k, j,
                               d_skip);
        hipLaunchKernelGGL(k_detect_sort_local, dim3(N / kDetSortBlock), dim3(1024), sort_lds, ctx->stream, ws.keys, ws.ctl,
                           ws.raw_cap, k, d_skip);
    }
    HIPCHK(ctx, hipGetLastError());
    DetectWalkArgs a;
    memset(&a, 0, sizeof a);
    a.keys = ws.keys, a.ctl = ws.ctl, a.max_corners = d_max_corners, a.skip = d_skip;
    a.raw_cap = ws.raw_cap, a.cap = cap, a.width = s.w, a.height = s.h;
    a.min_distance = det->min_distance;
    a.cell = ws.cell, a.grid_w = ws.grid_w, a.grid_h = ws.grid_h, a.reach = ws.reach, a.grid = ws.grid;
    a.corners = d_corners, a.info = d_info;
    hipLaunchKernelGGL(k_detect_walk, dim3(1), dim3(1024), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

bool detect_slot_ok(const FrameSlot &s) { return s.valid && s.img0 && s.w >= 14 && s.h >= 14; }

int detect_corners_slot(pagk_ctx *ctx, const pagk_detect_params *det, int32_t slot, const uint8_t *d_mask, int32_t cap,
                        const int32_t *d_max_corners, float *d_corners, int32_t *d_info)
{
    const FrameSlot &s = ctx->slots[slot];
    if (!detect_slot_ok(s)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DetectWs ws;
    int rc = detect_workspace(ctx, det, s.w, s.h, cap, &ws);
    if (rc) return rc;
    return detect_launch(ctx, det, s, d_mask, cap, d_max_corners, nullptr, d_corners, d_info, ws);
}

}  // namespace

void pagk_detect_params_default(pagk_detect_params *p)
{
    if (!p) return;
    p->quality_level = 0.005;   // src/frame.cpp:183
    p->min_distance = 20.0;
    p->harris_k = 0.04;         // :184
    p->raw_cap = 0;
}

int pagk_detect_corners_device(pagk_ctx *ctx, const pagk_detect_params *det, int32_t slot, const uint8_t *d_mask,
                               int32_t cap, const int32_t *d_max_corners, float *d_corners, int32_t *d_info)
{
    if (!ctx || !detect_params_ok(det) || slot < 0 || slot >= kUserSlots || cap < 1 || !d_corners || !d_info) return PAGK_E_ARG;
    return detect_corners_slot(ctx, det, slot, d_mask, cap, d_max_corners, d_corners, d_info);
}

int pagk_detect_corners(pagk_ctx *ctx, const pagk_detect_params *det, const pagk_image *img, const uint8_t *mask,
                        int32_t max_corners, float *corners, int32_t *info)
{
    if (!ctx || !detect_params_ok(det) || !img || max_corners < 0 || (max_corners > 0 && !corners)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_detect_corners");
    if (img->width < 14 || img->height < 14) return PAGK_E_ARG;
    int rc = frame_upload_any(ctx, 4, img, 1);
    if (rc) return rc;
    const size_t px = (size_t)img->width * img->height, cap = (size_t)(max_corners > 0 ? max_corners : 1);
    const size_t sizes[4] = {px, cap * 8, 256, 256};   // mask | corners | info | max_corners
    Staged<4> s(ctx, sizes);
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, mask, px)) || (rc = s.in(3, &max_corners, 4))) return rc;
    rc = detect_corners_slot(ctx, det, 4, mask ? s.at<uint8_t>(0) : nullptr, (int32_t)cap, s.at<int32_t>(3), s.at<float>(1),
                             s.at<int32_t>(2));
    if (rc || (rc = s.out(1, corners, (size_t)max_corners * 8)) || (rc = s.out(2, info, kDetectInfoWords * 4))) return rc;
    return s.finish();
}

int pagk_selftest_corner_response(pagk_ctx *ctx, const pagk_image *img, float *R)
{
    if (!ctx || !img || !R) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_corner_response");
    if (img->width < 14 || img->height < 14) return PAGK_E_ARG;
    int rc = frame_upload_any(ctx, 4, img, 1);
    if (rc) return rc;
    pagk_detect_params det;
    pagk_detect_params_default(&det);
    DetectWs ws;
    if ((rc = detect_workspace(ctx, &det, img->width, img->height, 1, &ws))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ws.ctl, 0, 8, ctx->stream));
    if ((rc = detect_response_launch(ctx, ctx->slots[4], nullptr, det.harris_k, ws, nullptr))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(R, ws.R, (size_t)img->width * img->height * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PAGK_OK;
}

// ---- the FAST detector: cells and quadtree (pagk_fast_kernel.h) --------------------------------------------------
namespace {

// The cell grid (src/ORBextractor.cc:805-830) and the initial nodes (:563-580) of a W x H image.  false where the
// reference would divide by zero (fewer than one cell, or no initial node), or where a coordinate leaves 15 bits.
bool fast_grid(int w, int h, FastGrid *g)
{
    if (w < 62 || h < 62 || w > 32767 || h > 32767) return false;
    g->W = w, g->H = h, g->max_bx = w - kFastBorder, g->max_by = h - kFastBorder;
    const float width = (float)(g->max_bx - kFastBorder), height = (float)(g->max_by - kFastBorder);
    g->n_cols = (int)(width / kFastCell), g->n_rows = (int)(height / kFastCell);
    if (g->n_cols < 1 || g->n_rows < 1) return false;
    g->w_cell = (int)std::ceil(width / g->n_cols), g->h_cell = (int)std::ceil(height / g->n_rows);
    g->seg = ((g->w_cell + 1) / 2) * ((g->h_cell + 1) / 2);   // at most one pixel of any 2 x 2 block survives
    g->n_ini = (int)std::round(width / height);               // half away from zero (:567)
    if (g->n_ini < 1) return false;
    g->hx = width / g->n_ini;
    return true;
}

int fast_params_check(const pagk_fast_params *p)
{
    if (!p || p->ini_threshold < 0 || p->ini_threshold > 255 || p->min_threshold < 0 || p->min_threshold > 255 ||
        p->n_features < 0 || p->n_features > (1 << 24))
        return PAGK_E_ARG;
    return p->n_levels == 1 ? PAGK_OK : PAGK_E_UNSUPPORTED;   // cv::resize at 1 / 1.2 is not restated
}

int64_t fast_raw_bound(const FastGrid &g) { return (int64_t)g.n_rows * g.n_cols * g.seg; }
int32_t fast_out_bound(const FastGrid &g, int32_t n_features) { return std::max(n_features + 2, 4 * g.n_ini); }

struct FastWs {
    int32_t *ctl = nullptr, *cell_cnt = nullptr, *cell_off = nullptr, *seg_score = nullptr, *kscore = nullptr, *knode = nullptr;
    int32_t *ncnt[2] = {}, *ncand[2] = {}, *cnt4 = nullptr, *cbase = nullptr, *split = nullptr;
    uint32_t *seg_xy = nullptr, *kxy = nullptr;
    int4 *box[2] = {};
    unsigned long long *sortk = nullptr, *best = nullptr;
    float *cand = nullptr;   // the fused call's candidate list, out_bound x 2
    uint32_t sort_slots = 0;
    int32_t raw_bound = 0, out_bound = 0, n_cells = 0;
};

// the parts of the detector's workspace for grid g and target n_features (false: a raw list beyond 2^30 keys)
constexpr int kFastWsParts = 20;
bool fast_ws_sizes(const FastGrid &g, int32_t n_features, size_t *sizes, uint32_t *sort_slots)
{
    const int64_t rb64 = fast_raw_bound(g);
    if (rb64 > (1 << 30)) return false;
    const size_t rb = (size_t)rb64, ob = (size_t)fast_out_bound(g, n_features), nc = (size_t)g.n_rows * g.n_cols;
    uint32_t slots = 2;
    while (slots < ob) slots <<= 1;
    const size_t v[kFastWsParts] = {256,    nc * 4, nc * 4, rb * 4, rb * 4, rb * 4, rb * 4,  rb * 4, ob * 16,           ob * 16,
                                    ob * 4, ob * 4, ob * 4, ob * 4, ob * 16, ob * 4, ob * 4, (size_t)slots * 8, ob * 8, ob * 8};
    std::copy(v, v + kFastWsParts, sizes);
    *sort_slots = slots;
    return true;
}

// ... and their addresses: part k of the workspace lies off[k] bytes into the block at b
void fast_ws_carve(const size_t *off, void *b, const FastGrid &g, int32_t n_features, uint32_t slots, FastWs *ws)
{
    auto part = [&](int k) { return static_cast<uint8_t *>(b) + off[k]; };
    auto i32 = [&](int k) { return reinterpret_cast<int32_t *>(part(k)); };
    ws->ctl = i32(0), ws->cell_cnt = i32(1), ws->cell_off = i32(2);
    ws->seg_xy = reinterpret_cast<uint32_t *>(part(3)), ws->seg_score = i32(4);
    ws->kxy = reinterpret_cast<uint32_t *>(part(5)), ws->kscore = i32(6), ws->knode = i32(7);
    ws->box[0] = reinterpret_cast<int4 *>(part(8)), ws->box[1] = reinterpret_cast<int4 *>(part(9));
    ws->ncnt[0] = i32(10), ws->ncnt[1] = i32(11), ws->ncand[0] = i32(12), ws->ncand[1] = i32(13);
    ws->cnt4 = i32(14), ws->cbase = i32(15), ws->split = i32(16);
    ws->sortk = reinterpret_cast<unsigned long long *>(part(17)), ws->best = reinterpret_cast<unsigned long long *>(part(18));
    ws->cand = reinterpret_cast<float *>(part(19));
    ws->sort_slots = slots, ws->raw_bound = (int32_t)fast_raw_bound(g), ws->out_bound = fast_out_bound(g, n_features);
    ws->n_cells = g.n_rows * g.n_cols;
}

int fast_workspace(pagk_ctx *ctx, const FastGrid &g, int32_t n_features, FastWs *ws)
{
    size_t sizes[kFastWsParts];
    uint32_t slots;
    if (!fast_ws_sizes(g, n_features, sizes, &slots)) return PAGK_E_ARG;
    const Layout<kFastWsParts> lay(sizes);
    int rc = reserve(ctx, ctx->buf[pagk_ctx::FAST], lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the FAST detector's workspace",
                     "run the call once with this image size and n_features before capturing");
    if (rc) return rc;
    fast_ws_carve(lay.off, ctx->buf[pagk_ctx::FAST].ptr, g, n_features, slots, ws);
    return PAGK_OK;
}

// FAST in cells and the raw list (step 3 of the definition) of frame slot `s`; d_skip: a device word or NULL.
FastCellArgs fast_cell_args(const pagk_fast_params *fp, const uint8_t *img, int64_t pitch, const FastGrid &g, const FastWs &ws,
                            const int32_t *d_skip)
{
    FastCellArgs c;
    memset(&c, 0, sizeof c);
    c.img = img, c.pitch = pitch, c.g = g, c.t_ini = fp->ini_threshold, c.t_min = fp->min_threshold;
    c.seg_xy = ws.seg_xy, c.seg_score = ws.seg_score, c.cell_cnt = ws.cell_cnt, c.skip = d_skip;
    return c;
}

FastTreeArgs fast_tree_args(int32_t n_features, const FastGrid &g, const uint8_t *d_mask, int32_t cap, float *d_keypoints,
                            float *d_response, int32_t *d_info, const int32_t *d_skip, const FastWs &ws)
{
    FastTreeArgs t;
    memset(&t, 0, sizeof t);
    t.g = g, t.n_features = n_features, t.cap = cap, t.out_bound = ws.out_bound, t.raw_bound = ws.raw_bound;
    t.sort_slots = ws.sort_slots, t.ctl = ws.ctl, t.kxy = ws.kxy, t.kscore = ws.kscore, t.knode = ws.knode;
    for (int k = 0; k < 2; k++) t.box[k] = ws.box[k], t.ncnt[k] = ws.ncnt[k], t.ncand[k] = ws.ncand[k];
    t.cnt4 = ws.cnt4, t.cbase = ws.cbase, t.split = ws.split, t.sortk = ws.sortk, t.best = ws.best;
    t.mask = d_mask, t.out_xy = d_keypoints, t.out_resp = d_response, t.info = d_info, t.skip = d_skip;
    return t;
}

int fast_cells_launch(pagk_ctx *ctx, const pagk_fast_params *fp, const FrameSlot &s, const FastGrid &g, const FastWs &ws,
                      const int32_t *d_skip)
{
    const FastCellArgs c = fast_cell_args(fp, s.img0, s.pitch0, g, ws, d_skip);
    hipLaunchKernelGGL(k_fast_cells, dim3(ws.n_cells), dim3(256), 0, ctx->stream, c);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fast_offsets, dim3(1), dim3(1024), 0, ctx->stream, ws.n_cells, (const int32_t *)ws.cell_cnt, ws.cell_off,
                       ws.ctl, d_skip);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fast_gather, dim3(ws.n_cells), dim3(256), 0, ctx->stream, g.seg, (const int32_t *)ws.cell_cnt,
                       (const int32_t *)ws.cell_off, (const uint32_t *)ws.seg_xy, (const int32_t *)ws.seg_score, ws.kxy, ws.kscore,
                       d_skip);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

// The detector's launches: cells -> raw list -> tree, best keys, mask, output.
int fast_launch(pagk_ctx *ctx, const pagk_fast_params *fp, int32_t n_features, const FrameSlot &s, const FastGrid &g,
                const uint8_t *d_mask, int32_t cap, float *d_keypoints, float *d_response, int32_t *d_info,
                const int32_t *d_skip, const FastWs &ws)
{
    int rc = fast_cells_launch(ctx, fp, s, g, ws, d_skip);
    if (rc) return rc;
    const FastTreeArgs t = fast_tree_args(n_features, g, d_mask, cap, d_keypoints, d_response, d_info, d_skip, ws);
    hipLaunchKernelGGL(k_fast_tree, dim3(1), dim3(1024), 0, ctx->stream, t);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

bool fast_slot_ok(const FrameSlot &s) { return s.valid && s.img0; }

}  // namespace

void pagk_fast_params_default(pagk_fast_params *p)
{
    if (!p) return;
    p->ini_threshold = 20;   // iniThFAST, Examples/Demo/RealSenseD435i.cpp:184-190
    p->min_threshold = 7;    // minThFAST
    p->n_features = 0;       // the call's target
    p->n_levels = 1;
}

int pagk_fast_params_check(const pagk_fast_params *p) { return fast_params_check(p); }

int pagk_detect_fast_bounds(int32_t width, int32_t height, int32_t n_features, int32_t *raw_bound, int32_t *out_bound)
{
    FastGrid g;
    if (n_features < 1 || n_features > (1 << 24) || !fast_grid(width, height, &g) || fast_raw_bound(g) > (1 << 30)) return PAGK_E_ARG;
    if (raw_bound) *raw_bound = (int32_t)fast_raw_bound(g);
    if (out_bound) *out_bound = fast_out_bound(g, n_features);
    return PAGK_OK;
}

// (slots 4 and 5 are the host-buffer forms' own)
static int detect_fast_slot(pagk_ctx *ctx, const pagk_fast_params *params, int32_t slot, const uint8_t *d_mask, int32_t cap,
                            float *d_keypoints, float *d_response, int32_t *d_info)
{
    if (!ctx) return PAGK_E_ARG;
    int rc = fast_params_check(params);
    if (rc) return rc;
    if (params->n_features < 1 || slot < 0 || slot >= kSlots || !d_keypoints || !d_info) return PAGK_E_ARG;
    const FrameSlot &s = ctx->slots[slot];
    FastGrid g;
    if (!fast_slot_ok(s) || !fast_grid(s.w, s.h, &g) || cap < fast_out_bound(g, params->n_features)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FastWs ws;
    if ((rc = fast_workspace(ctx, g, params->n_features, &ws))) return rc;
    return fast_launch(ctx, params, params->n_features, s, g, d_mask, cap, d_keypoints, d_response, d_info, nullptr, ws);
}

int pagk_detect_fast_device(pagk_ctx *ctx, const pagk_fast_params *params, int32_t slot, const uint8_t *d_mask, int32_t cap,
                            float *d_keypoints, float *d_response, int32_t *d_info)
{
    if (slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    return detect_fast_slot(ctx, params, slot, d_mask, cap, d_keypoints, d_response, d_info);
}

int pagk_detect_fast(pagk_ctx *ctx, const pagk_fast_params *params, const pagk_image *img, const uint8_t *mask, int32_t cap,
                     float *keypoints, float *response, int32_t *info)
{
    if (!ctx || !img) return PAGK_E_ARG;
    int rc = fast_params_check(params);
    if (rc) return rc;
    NOT_WHILE_CAPTURING(ctx, "pagk_detect_fast");
    FastGrid g;
    if (params->n_features < 1 || !keypoints || !fast_grid(img->width, img->height, &g) ||
        cap < fast_out_bound(g, params->n_features))
        return PAGK_E_ARG;
    if ((rc = frame_upload_any(ctx, 4, img, 1))) return rc;
    const size_t px = (size_t)img->width * img->height, nc = (size_t)cap;
    const size_t sizes[4] = {px, nc * 8, nc * 4, 256};   // mask | keypoints | response | info
    Staged<4> s(ctx, sizes);
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, mask, px))) return rc;
    rc = detect_fast_slot(ctx, params, 4, mask ? s.at<uint8_t>(0) : nullptr, cap, s.at<float>(1), s.at<float>(2), s.at<int32_t>(3));
    if (rc || (rc = s.out(1, keypoints, nc * 8)) || (rc = s.out(2, response, nc * 4)) || (rc = s.out(3, info, kDetectInfoWords * 4)))
        return rc;
    return s.finish();
}

int pagk_selftest_fast_cells(pagk_ctx *ctx, const pagk_fast_params *params, const pagk_image *img, float *raw_xy,
                             int32_t *raw_score, int32_t *n)
{
    if (!ctx || !img || !raw_xy || !raw_score || !n) return PAGK_E_ARG;
    int rc = fast_params_check(params);
    if (rc) return rc;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_fast_cells");
    FastGrid g;
    if (!fast_grid(img->width, img->height, &g)) return PAGK_E_ARG;
    if ((rc = frame_upload_any(ctx, 4, img, 1))) return rc;
    FastWs ws;
    if ((rc = fast_workspace(ctx, g, 1, &ws))) return rc;
    if ((rc = fast_cells_launch(ctx, params, ctx->slots[4], g, ws, nullptr))) return rc;
    int32_t cnt = 0;
    HIPCHK(ctx, hipMemcpyAsync(&cnt, ws.ctl + kFastCtlCount, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (cnt < 0 || cnt > ws.raw_bound) return PAGK_E_HIP;
    std::vector<uint32_t> xy((size_t)cnt);
    if (cnt) {
        HIPCHK(ctx, hipMemcpy(xy.data(), ws.kxy, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(raw_score, ws.kscore, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    }
    for (int32_t k = 0; k < cnt; k++) raw_xy[2 * k] = (float)(xy[k] & 0xffffu), raw_xy[2 * k + 1] = (float)(xy[k] >> 16);
    *n = cnt;
    return PAGK_OK;
}

// ---- frame hand-over (pagk_handover_kernel.h) ------------------------------------------------------------------
// Behind the two detectors, whose workspaces and launches it uses.
namespace {

// The hand-over's arrays: the device's for the check and the launch, the caller's for handover_host.  keys_normal may be
// NULL; without a mask the device forms use the context's own and the host forms copy none out.
struct HandoverArrays {
    const uint8_t *status = nullptr;
    const float *pt_predict = nullptr, *pt_predict_un = nullptr;
    float *keys = nullptr, *keys_un = nullptr, *keys_normal = nullptr;
    int32_t *index_in_last = nullptr;
    uint8_t *live = nullptr, *mask = nullptr;
    int32_t *state = nullptr;
};

// Where the candidates come from: the caller's list, or what a detector finds on level 0 of a frame slot and counts in info.
struct HandoverSource {
    enum Kind { GIVEN, CORNERS, FAST } kind = GIVEN;
    int32_t cand_cap = 0;                    // GIVEN
    const int32_t *n_cand = nullptr;
    const float *cand_un = nullptr;
    const pagk_detect_params *det = nullptr; // CORNERS
    const pagk_fast_params *fast = nullptr;  // FAST
    int32_t slot = 4;                        // CORNERS, FAST (the host forms detect on scratch slot 4)
    int32_t *info = nullptr;
};

bool handover_args_ok(const pagk_params *params, int32_t width, int32_t height, int32_t cap, int32_t target_n,
                      double new_point_threshold, int32_t cand_cap)
{
    // 14 = the mask's hole (src/frame.cpp:117-119): a smaller image has no place for one
    return params && width >= 14 && height >= 14 && (int64_t)width * height <= 0x7fffffff && cap >= 1 && target_n >= 0 &&
           cap >= target_n && cand_cap >= 0 && !std::isnan(new_point_threshold);
}

// What every form refuses first: the geometry, then the source's parameter block (whose code may be PAGK_E_UNSUPPORTED).
int handover_geometry_check(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                            int32_t target_n, double new_point_threshold, const HandoverSource &src)
{
    if (!ctx || !handover_args_ok(params, width, height, cap, target_n, new_point_threshold, src.cand_cap)) return PAGK_E_ARG;
    switch (src.kind) {
    case HandoverSource::GIVEN: return PAGK_OK;
    case HandoverSource::CORNERS: return detect_params_ok(src.det) ? PAGK_OK : PAGK_E_ARG;
    case HandoverSource::FAST: return fast_params_check(src.fast);
    }
    return PAGK_E_ARG;
}

// the arrays no form does without, the device's or the caller's
bool handover_required(const HandoverArrays &a, const HandoverSource &src)
{
    if (src.kind == HandoverSource::GIVEN && (!src.n_cand || (src.cand_cap > 0 && !src.cand_un))) return false;
    return a.status && a.pt_predict && a.pt_predict_un && a.keys && a.keys_un && a.index_in_last && a.live && a.state;
}

// Everything a device form refuses, in front of handover_launch.
int handover_check(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap, int32_t target_n,
                   double new_point_threshold, const HandoverArrays &a, const HandoverSource &src)
{
    const bool given = src.kind == HandoverSource::GIVEN;
    if (!given && (src.slot < 0 || src.slot >= kUserSlots)) return PAGK_E_ARG;   // (slots 4 and 5 are the host-buffer forms' own)
    int rc = handover_geometry_check(ctx, params, width, height, cap, target_n, new_point_threshold, src);
    if (rc) return rc;
    if (!handover_required(a, src) || (!given && !src.info)) return PAGK_E_ARG;
    if (a.keys == a.pt_predict || a.keys_un == a.pt_predict_un) return PAGK_E_ARG;  // the caller ping-pongs two sets
    if (given) return PAGK_OK;
    const FrameSlot &s = ctx->slots[src.slot];
    const bool slot_ok = src.kind == HandoverSource::CORNERS ? detect_slot_ok(s) : fast_slot_ok(s);
    return slot_ok && s.w == width && s.h == height ? PAGK_OK : PAGK_E_ARG;
}

// The tracking launches' hints (pagk_prio.h) are per feature SLOT: a survivor that moves to a new slot takes its hint along, a
// new or an unused slot has none.  The array as it stands when the hand-over is issued (none before the first launch).
void handover_hint_args(pagk_ctx *ctx, HandoverArgs *a)
{
    const DevBuf &hb = ctx->buf[pagk_ctx::PRIO_HINT];
    a->prio_hint = static_cast<int32_t *>(hb.ptr);
    a->prio_hint_n = (int32_t)(hb.bytes / sizeof(int32_t));
}

// the sizes, the rule's constants and the camera model of a hand-over; the pointers are the caller's to fill
void handover_fill_args(HandoverArgs *out, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                        int32_t target_n, double new_point_threshold)
{
    HandoverArgs a;
    memset(&a, 0, sizeof a);
    a.cap = cap, a.width = width, a.height = height, a.target_n = target_n;
    a.new_point_threshold = new_point_threshold;
    a.fx = params->fx, a.fy = params->fy, a.cx = params->cx, a.cy = params->cy;
    a.fx_inv = (float)(1.0 / (double)params->fx);  // src/frame.cpp:70
    a.fy_inv = (float)(1.0 / (double)params->fy);
    a.k1 = params->dist_coef[0], a.k2 = params->dist_coef[1], a.p1 = params->dist_coef[2], a.p2 = params->dist_coef[3];
    a.k3 = params->n_dist_coef == 5 ? params->dist_coef[4] : 0.0f;
    a.distort_on = params->dist_coef[0] != 0.0f;
    *out = a;
}

// The hand-over's launches on the context's stream: fill -> holes -> [plan -> detector] -> keys.  Without a.mask the
// context's own mask is used.  A detecting source's candidates are not the caller's but what its detector finds on the
// frame's slot, counted in info[0]: the corners under the mask the call has just built (at most n_new <= target_n <= cap),
// or the FAST keypoints of the whole frame (no mask: the acceptance test of k_handover_keys is the reference's mask test,
// src/ORBextractor.cc:1199-1203).
int handover_launch(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap, int32_t target_n,
                    double new_point_threshold, const HandoverArrays &a, const HandoverSource &src)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FastGrid g;
    int32_t n_features = 0;
    if (src.kind == HandoverSource::FAST) {   // (refused before anything is reserved)
        if (!fast_grid(width, height, &g)) return PAGK_E_ARG;
        n_features = src.fast->n_features ? src.fast->n_features : target_n;
        if (n_features < 1) return PAGK_E_ARG;
    }
    const int64_t bytes = (int64_t)width * height;
    DevBuf &hand = ctx->buf[pagk_ctx::HAND];   // the context's own mask, for a caller that passes none
    int rc = a.mask ? PAGK_OK
                    : reserve(ctx, hand, align_up((size_t)bytes, kPartAlign), NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the hand-over's mask",
                              "run the call once with this image size before capturing, or pass d_mask");
    if (rc) return rc;
    uint8_t *mask = a.mask ? a.mask : static_cast<uint8_t *>(hand.ptr);
    HandoverArgs k;
    handover_fill_args(&k, params, width, height, cap, target_n, new_point_threshold);
    DetectWs dws;
    FastWs fws;
    int32_t *plan = nullptr;   // the detector's control words, which k_handover_plan writes
    switch (src.kind) {
    case HandoverSource::GIVEN:
        k.cand_cap = src.cand_cap, k.n_cand = src.n_cand, k.cand_un = src.cand_un;
        break;
    case HandoverSource::CORNERS:
        if ((rc = detect_workspace(ctx, src.det, width, height, cap, &dws))) return rc;
        k.cand_cap = cap, k.n_cand = src.info, k.cand_un = dws.cand, plan = dws.ctl;
        break;
    case HandoverSource::FAST:
        if ((rc = fast_workspace(ctx, g, n_features, &fws))) return rc;
        k.cand_cap = fws.out_bound, k.n_cand = src.info, k.cand_un = fws.cand, plan = fws.ctl;
        break;
    }
    k.status = a.status, k.pt_predict = a.pt_predict, k.pt_predict_un = a.pt_predict_un;
    k.keys = a.keys, k.keys_un = a.keys_un, k.keys_normal = a.keys_normal;
    k.index_in_last = a.index_in_last, k.live = a.live, k.mask = mask, k.state = a.state;
    handover_hint_args(ctx, &k);
    hipLaunchKernelGGL(k_handover_fill, dim3((unsigned)((bytes + 4095) / 4096)), dim3(256), 0, ctx->stream, mask, bytes);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_handover_holes, dim3((unsigned)(((int64_t)cap * 14 + 255) / 256)), dim3(256), 0, ctx->stream, cap,
                       width, height, a.status, a.pt_predict_un, mask);
    HIPCHK(ctx, hipGetLastError());
    if (plan) {
        hipLaunchKernelGGL(k_handover_plan, dim3(1), dim3(1024), 0, ctx->stream, cap, target_n, new_point_threshold, a.status,
                           (const int32_t *)a.state, plan);
        HIPCHK(ctx, hipGetLastError());
        const FrameSlot &s = ctx->slots[src.slot];
        rc = src.kind == HandoverSource::CORNERS
                 ? detect_launch(ctx, src.det, s, mask, cap, dws.ctl + kDetCtlLimit, dws.ctl + kDetCtlSkip, dws.cand, src.info, dws)
                 : fast_launch(ctx, src.fast, n_features, s, g, nullptr, fws.out_bound, fws.cand, nullptr, src.info,
                               fws.ctl + kFastCtlSkip, fws);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_handover_keys, dim3(1), dim3(1024), 0, ctx->stream, k);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

// The host-buffer hand-overs: the caller's arrays `host` through one device block around handover_launch.  Of `src` the
// list, its count and info are the caller's too; the detecting sources find their candidates on `img`, uploaded into
// scratch slot 4.
int handover_host(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap, int32_t target_n,
                  double new_point_threshold, const HandoverArrays &host, const HandoverSource &src, const pagk_image *img)
{
    static const char *const kNames[] = {"pagk_frame_handover", "pagk_frame_handover_detect", "pagk_frame_handover_fast"};
    int rc = handover_geometry_check(ctx, params, width, height, cap, target_n, new_point_threshold, src);
    if (rc) return rc;
    NOT_WHILE_CAPTURING(ctx, kNames[src.kind]);
    const bool given = src.kind == HandoverSource::GIVEN;   // a count and a list go in, no info comes out
    if (!handover_required(host, src) || (!given && (!img || img->width != width || img->height != height))) return PAGK_E_ARG;
    if (given)
        HIPCHK(ctx, hipSetDevice(ctx->device));
    else if ((rc = frame_upload_any(ctx, 4, img, 1)))
        return rc;
    const size_t nc = (size_t)cap, cc = (size_t)(src.cand_cap > 0 ? src.cand_cap : 1), px = (size_t)width * height;
    enum { STATUS, PREDICT, PREDICT_UN, N_CAND, CAND, KEYS, KEYS_UN, KEYS_NORMAL, INDEX, LIVE, STATE, INFO, MASK, PARTS };
    const size_t sizes[PARTS] = {nc,     nc * 8, nc * 8, given ? 4 : 0u, given ? cc * 8 : 0u,     nc * 8,
                                 nc * 8, nc * 8, nc * 4, nc,             kHandoverStateWords * 4, given ? 0u : kDetectInfoWords * 4,
                                 px};
    Staged<PARTS> s(ctx, sizes);
    // (the form with the caller's candidates keeps its block in the context; the detecting forms take one per call)
    rc = s.open(given ? &ctx->buf[pagk_ctx::HANDIO] : nullptr, "the host-buffer hand-over's scratch");
    if (rc) return rc;
    const void *in[] = {host.status, host.pt_predict, host.pt_predict_un, src.n_cand, src.cand_cap > 0 ? src.cand_un : nullptr};
    for (int k = STATUS; k <= CAND; k++)
        if ((rc = s.in(k, in[k], sizes[k]))) return rc;
    if ((rc = s.in(STATE, host.state, sizes[STATE]))) return rc;   // reach_flag persists
    HandoverArrays d;
    d.status = s.at<uint8_t>(STATUS), d.pt_predict = s.at<float>(PREDICT), d.pt_predict_un = s.at<float>(PREDICT_UN);
    d.keys = s.at<float>(KEYS), d.keys_un = s.at<float>(KEYS_UN);
    d.keys_normal = host.keys_normal ? s.at<float>(KEYS_NORMAL) : nullptr;
    d.index_in_last = s.at<int32_t>(INDEX), d.live = s.at<uint8_t>(LIVE), d.mask = s.at<uint8_t>(MASK);
    d.state = s.at<int32_t>(STATE);
    HandoverSource dsrc = src;
    dsrc.n_cand = s.at<int32_t>(N_CAND), dsrc.cand_un = s.at<float>(CAND), dsrc.info = s.at<int32_t>(INFO);
    if ((rc = handover_launch(ctx, params, width, height, cap, target_n, new_point_threshold, d, dsrc))) return rc;
    void *out[] = {host.keys, host.keys_un, host.keys_normal, host.index_in_last, host.live, host.state, src.info, host.mask};
    for (int k = KEYS; k <= MASK; k++)
        if ((rc = s.out(k, out[k - KEYS], sizes[k]))) return rc;
    return s.finish();
}

}  // namespace

int pagk_frame_handover_device(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                               int32_t target_n, double new_point_threshold, const uint8_t *d_status,
                               const float *d_pt_predict, const float *d_pt_predict_un, int32_t cand_cap,
                               const int32_t *d_n_cand, const float *d_cand_un, float *d_keys, float *d_keys_un,
                               float *d_keys_normal, int32_t *d_index_in_last, uint8_t *d_live, uint8_t *d_mask,
                               int32_t *d_state)
{
    HandoverArrays a;
    a.status = d_status, a.pt_predict = d_pt_predict, a.pt_predict_un = d_pt_predict_un;
    a.keys = d_keys, a.keys_un = d_keys_un, a.keys_normal = d_keys_normal;
    a.index_in_last = d_index_in_last, a.live = d_live, a.mask = d_mask, a.state = d_state;
    HandoverSource src;
    src.cand_cap = cand_cap, src.n_cand = d_n_cand, src.cand_un = d_cand_un;
    int rc = handover_check(ctx, params, width, height, cap, target_n, new_point_threshold, a, src);
    return rc ? rc : handover_launch(ctx, params, width, height, cap, target_n, new_point_threshold, a, src);
}

int pagk_frame_handover(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                        int32_t target_n, double new_point_threshold, const uint8_t *status, const float *pt_predict,
                        const float *pt_predict_un, int32_t cand_cap, const int32_t *n_cand, const float *cand_un,
                        float *keys, float *keys_un, float *keys_normal, int32_t *index_in_last, uint8_t *live,
                        uint8_t *mask, int32_t *state)
{
    HandoverArrays a;
    a.status = status, a.pt_predict = pt_predict, a.pt_predict_un = pt_predict_un;
    a.keys = keys, a.keys_un = keys_un, a.keys_normal = keys_normal;
    a.index_in_last = index_in_last, a.live = live, a.mask = mask, a.state = state;
    HandoverSource src;
    src.cand_cap = cand_cap, src.n_cand = n_cand, src.cand_un = cand_un;
    return handover_host(ctx, params, width, height, cap, target_n, new_point_threshold, a, src, nullptr);
}

int pagk_frame_handover_detect_device(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height,
                                      int32_t cap, int32_t target_n, double new_point_threshold, const uint8_t *d_status,
                                      const float *d_pt_predict, const float *d_pt_predict_un,
                                      const pagk_detect_params *det, int32_t slot, float *d_keys, float *d_keys_un,
                                      float *d_keys_normal, int32_t *d_index_in_last, uint8_t *d_live, uint8_t *d_mask,
                                      int32_t *d_state, int32_t *d_info)
{
    HandoverArrays a;
    a.status = d_status, a.pt_predict = d_pt_predict, a.pt_predict_un = d_pt_predict_un;
    a.keys = d_keys, a.keys_un = d_keys_un, a.keys_normal = d_keys_normal;
    a.index_in_last = d_index_in_last, a.live = d_live, a.mask = d_mask, a.state = d_state;
    HandoverSource src;
    src.kind = HandoverSource::CORNERS, src.det = det, src.slot = slot, src.info = d_info;
    int rc = handover_check(ctx, params, width, height, cap, target_n, new_point_threshold, a, src);
    return rc ? rc : handover_launch(ctx, params, width, height, cap, target_n, new_point_threshold, a, src);
}

int pagk_frame_handover_detect(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                               int32_t target_n, double new_point_threshold, const uint8_t *status,
                               const float *pt_predict, const float *pt_predict_un, const pagk_detect_params *det,
                               const pagk_image *img, float *keys, float *keys_un, float *keys_normal,
                               int32_t *index_in_last, uint8_t *live, uint8_t *mask, int32_t *state, int32_t *info)
{
    HandoverArrays a;
    a.status = status, a.pt_predict = pt_predict, a.pt_predict_un = pt_predict_un;
    a.keys = keys, a.keys_un = keys_un, a.keys_normal = keys_normal;
    a.index_in_last = index_in_last, a.live = live, a.mask = mask, a.state = state;
    HandoverSource src;
    src.kind = HandoverSource::CORNERS, src.det = det, src.info = info;
    return handover_host(ctx, params, width, height, cap, target_n, new_point_threshold, a, src, img);
}

int pagk_frame_handover_fast_device(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                                    int32_t target_n, double new_point_threshold, const uint8_t *d_status,
                                    const float *d_pt_predict, const float *d_pt_predict_un, const pagk_fast_params *fast,
                                    int32_t slot, float *d_keys, float *d_keys_un, float *d_keys_normal,
                                    int32_t *d_index_in_last, uint8_t *d_live, uint8_t *d_mask, int32_t *d_state,
                                    int32_t *d_info)
{
    HandoverArrays a;
    a.status = d_status, a.pt_predict = d_pt_predict, a.pt_predict_un = d_pt_predict_un;
    a.keys = d_keys, a.keys_un = d_keys_un, a.keys_normal = d_keys_normal;
    a.index_in_last = d_index_in_last, a.live = d_live, a.mask = d_mask, a.state = d_state;
    HandoverSource src;
    src.kind = HandoverSource::FAST, src.fast = fast, src.slot = slot, src.info = d_info;
    int rc = handover_check(ctx, params, width, height, cap, target_n, new_point_threshold, a, src);
    return rc ? rc : handover_launch(ctx, params, width, height, cap, target_n, new_point_threshold, a, src);
}

int pagk_frame_handover_fast(pagk_ctx *ctx, const pagk_params *params, int32_t width, int32_t height, int32_t cap,
                             int32_t target_n, double new_point_threshold, const uint8_t *status, const float *pt_predict,
                             const float *pt_predict_un, const pagk_fast_params *fast, const pagk_image *img, float *keys,
                             float *keys_un, float *keys_normal, int32_t *index_in_last, uint8_t *live, uint8_t *mask,
                             int32_t *state, int32_t *info)
{
    HandoverArrays a;
    a.status = status, a.pt_predict = pt_predict, a.pt_predict_un = pt_predict_un;
    a.keys = keys, a.keys_un = keys_un, a.keys_normal = keys_normal;
    a.index_in_last = index_in_last, a.live = live, a.mask = mask, a.state = state;
    HandoverSource src;
    src.kind = HandoverSource::FAST, src.fast = fast, src.info = info;
    return handover_host(ctx, params, width, height, cap, target_n, new_point_threshold, a, src, img);
}

// ---- ORB descriptors and matching (pagk_orb_kernel.h) ----------------------------------------------------------
namespace {

int orb_params_check(const pagk_orb_params *p)
{
    if (!p) return PAGK_E_ARG;
    const int32_t *w = p->blur_weights;
    if (w[0] < 0 || w[1] < 0 || w[2] < 0 || w[3] < 0 || w[0] > 256 || w[1] > 128 || w[2] > 128 || w[3] > 128 ||
        w[0] + 2 * (w[1] + w[2] + w[3]) != 256 || p->match_floor < 0 || p->match_floor > 256)
        return PAGK_E_ARG;
    return p->n_levels == 1 ? PAGK_OK : PAGK_E_UNSUPPORTED;   // cv::resize at 1 / 1.2 is not restated
}

int orb_pattern_check(const int32_t *pattern)
{
    if (!pattern) return PAGK_E_ARG;
    for (int k = 0; k < kOrbPatternInts; k++)
        if (pattern[k] < -13 || pattern[k] > 13) return PAGK_E_ARG;
    return PAGK_OK;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// blur -> orientation and descriptors of the keypoints of slot `s`; arguments checked by the caller
int orb_describe_launch(pagk_ctx *ctx, const pagk_orb_params *params, const FrameSlot &s, int32_t cap, const float *d_keypoints,
                        const int32_t *d_n, float *d_angle, uint8_t *d_desc, int32_t *d_info)
{
    const int wp = (s.w + 3) & ~3;
    const size_t sizes[1] = {(size_t)wp * s.h};
    const Layout<1> lay(sizes);
    DevBuf &blur = ctx->buf[pagk_ctx::ORB_BLUR];
    int rc = reserve(ctx, blur, lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the blurred image of the ORB descriptors",
                     "run the call once with this image size before capturing");
    if (rc) return rc;
    OrbBlurArgs b;
    b.img = s.img0, b.pitch = s.pitch0, b.blur = lay.at<uint8_t>(blur.ptr, 0), b.info = d_info;
    b.W = s.w, b.H = s.h, b.wp = wp;
    b.w0 = params->blur_weights[0], b.w1 = params->blur_weights[1], b.w2 = params->blur_weights[2], b.w3 = params->blur_weights[3];
    hipLaunchKernelGGL(k_orb_blur, dim3((unsigned)((s.w + kOrbBlurTx - 1) / kOrbBlurTx), (unsigned)((s.h + kOrbBlurTy - 1) / kOrbBlurTy)),
                       dim3(256), 0, ctx->stream, b);
    HIPCHK(ctx, hipGetLastError());
    OrbDescArgs d;
    d.img = s.img0, d.pitch = s.pitch0, d.blur = b.blur;
    d.pattern = static_cast<const int32_t *>(ctx->buf[pagk_ctx::ORB_PATTERN].ptr);
    d.keypoints = d_keypoints, d.n = d_n, d.angle = d_angle, d.desc = d_desc, d.info = d_info;
    d.W = s.w, d.H = s.h, d.wp = wp, d.cap = cap;
    hipLaunchKernelGGL(k_orb_describe, dim3((unsigned)((cap + 3) / 4)), dim3(256), 0, ctx->stream, d);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

// (slots 4 and 5 are the host-buffer forms' own)
int orb_describe_slot(pagk_ctx *ctx, const pagk_orb_params *params, int32_t slot, int32_t cap, const float *d_keypoints,
                      const int32_t *d_n, float *d_angle, uint8_t *d_desc, int32_t *d_info)
{
    if (!ctx) return PAGK_E_ARG;
    int rc = orb_params_check(params);
    if (rc) return rc;
    if (slot < 0 || slot >= kSlots || cap < 1 || cap > kOrbMaxRows || !d_keypoints || !d_n || !d_desc || !d_info || !aligned16(d_desc))
        return PAGK_E_ARG;
    if (!ctx->orb_pattern_set) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_orb_describe: no sampling pattern set (pagk_orb_set_pattern)");
        return PAGK_E_ARG;
    }
    const FrameSlot &s = ctx->slots[slot];
    if (!fast_slot_ok(s) || s.w < 4 || s.h < 4 || s.w > 32767 || s.h > 32767) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return orb_describe_launch(ctx, params, s, cap, d_keypoints, d_n, d_angle, d_desc, d_info);
}

}  // namespace

void pagk_orb_params_default(pagk_orb_params *p)
{
    if (!p) return;
    p->blur_weights[0] = 54, p->blur_weights[1] = 49, p->blur_weights[2] = 34, p->blur_weights[3] = 18;
    p->match_floor = 30;   // experiment_value, src/ORBDetectAndDespMatcher.cpp:76
    p->n_levels = 1;
}

int pagk_orb_params_check(const pagk_orb_params *p) { return orb_params_check(p); }

int pagk_orb_pattern_check(const int32_t pattern[1024]) { return orb_pattern_check(pattern); }

int pagk_orb_set_pattern(pagk_ctx *ctx, const int32_t pattern[1024])
{
    if (!ctx || orb_pattern_check(pattern) != PAGK_OK) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_orb_set_pattern");
    if (in_capture(ctx)) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_orb_set_pattern allocates and synchronises: not inside a stream capture");
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf &pat = ctx->buf[pagk_ctx::ORB_PATTERN];   // grows once, to its only size: graphs keep pointing at it
    int rc = reserve(ctx, pat, kOrbPatternInts * sizeof(int32_t), NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the ORB sampling pattern",
                     "set a pattern before capturing");
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(pat.ptr, pattern, kOrbPatternInts * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->orb_pattern_set = true;
    return PAGK_OK;
}

int pagk_orb_describe_device(pagk_ctx *ctx, const pagk_orb_params *params, int32_t slot, int32_t cap,
                             const float *d_keypoints, const int32_t *d_n, float *d_angle, uint8_t *d_desc, int32_t *d_info)
{
    if (slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    return orb_describe_slot(ctx, params, slot, cap, d_keypoints, d_n, d_angle, d_desc, d_info);
}

int pagk_orb_describe(pagk_ctx *ctx, const pagk_orb_params *params, const pagk_image *img, int32_t n,
                      const float *keypoints, float *angle, uint8_t *desc, int32_t *info)
{
    if (!ctx || !img) return PAGK_E_ARG;
    int rc = orb_params_check(params);
    if (rc) return rc;
    NOT_WHILE_CAPTURING(ctx, "pagk_orb_describe");
    if (n < 0 || n > kOrbMaxRows || (n && (!keypoints || !desc))) return PAGK_E_ARG;
    if ((rc = frame_upload_any(ctx, 4, img, 1))) return rc;
    const size_t nc = (size_t)std::max(n, 1);
    const size_t sizes[5] = {nc * 8, 256, nc * 4, nc * 32, 256};   // keypoints | count | angle | descriptors | info
    Staged<5> s(ctx, sizes);
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, keypoints, (size_t)n * 8)) || (rc = s.in(1, &n, 4))) return rc;
    rc = orb_describe_slot(ctx, params, 4, (int32_t)nc, s.at<float>(0), s.at<int32_t>(1), s.at<float>(2), s.at<uint8_t>(3),
                           s.at<int32_t>(4));
    if (rc || (rc = s.out(2, angle, (size_t)n * 4)) || (rc = s.out(3, desc, (size_t)n * 32)) ||
        (rc = s.out(4, info, kOrbInfoWords * 4)))
        return rc;
    return s.finish();
}

int pagk_orb_match_device(pagk_ctx *ctx, const pagk_orb_params *params, int32_t cap_q, const uint8_t *d_desc_q,
                          const int32_t *d_nq, int32_t cap_t, const uint8_t *d_desc_t, const int32_t *d_nt,
                          int32_t *d_train_idx, int32_t *d_distance, uint8_t *d_keep, int32_t *d_info)
{
    if (!ctx) return PAGK_E_ARG;
    int rc = orb_params_check(params);
    if (rc) return rc;
    if (cap_q < 1 || cap_q > kOrbMaxRows || cap_t < 1 || cap_t > kOrbMaxRows || !d_desc_q || !d_nq || !d_desc_t || !d_nt ||
        !d_train_idx || !d_distance || !d_keep || !d_info || !aligned16(d_desc_q) || !aligned16(d_desc_t))
        return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t sizes[1] = {(size_t)cap_q * 4};
    const Layout<1> lay(sizes);
    DevBuf &keys = ctx->buf[pagk_ctx::ORB_KEYS];
    if ((rc = reserve(ctx, keys, lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the ORB matcher's keys",
                      "run the call once with this cap_q before capturing")))
        return rc;
    OrbMatchArgs a;
    a.desc_q = d_desc_q, a.desc_t = d_desc_t, a.nq = d_nq, a.nt = d_nt, a.keys = lay.at<uint32_t>(keys.ptr, 0);
    a.train_idx = d_train_idx, a.distance = d_distance, a.keep = d_keep, a.info = d_info;
    a.cap_q = cap_q, a.cap_t = cap_t, a.match_floor = params->match_floor;
    HIPCHK(ctx, hipMemsetAsync(a.keys, 0xff, sizes[0], ctx->stream));
    const unsigned groups = (unsigned)std::min((cap_t + kOrbMatchChunk - 1) / kOrbMatchChunk, kOrbMatchMaxChunkGroups);
    hipLaunchKernelGGL(k_orb_match, dim3((unsigned)((cap_q + 63) / 64), groups), dim3(64), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_orb_match_finish, dim3(1), dim3(1024), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

int pagk_orb_match(pagk_ctx *ctx, const pagk_orb_params *params, int32_t nq, const uint8_t *desc_q, int32_t nt,
                   const uint8_t *desc_t, int32_t *train_idx, int32_t *distance, uint8_t *keep, int32_t *info)
{
    if (!ctx) return PAGK_E_ARG;
    int rc = orb_params_check(params);
    if (rc) return rc;
    NOT_WHILE_CAPTURING(ctx, "pagk_orb_match");
    if (nq < 0 || nq > kOrbMaxRows || nt < 0 || nt > kOrbMaxRows || (nq && (!desc_q || !train_idx || !distance || !keep)) ||
        (nt && !desc_t))
        return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t cq = (size_t)std::max(nq, 1), ct = (size_t)std::max(nt, 1);
    const int32_t counts[2] = {nq, nt};
    // query rows | train rows | counts | train_idx | distance | keep | info
    const size_t sizes[7] = {cq * 32, ct * 32, 256, cq * 4, cq * 4, cq, 256};
    Staged<7> s(ctx, sizes);
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, desc_q, (size_t)nq * 32)) || (rc = s.in(1, desc_t, (size_t)nt * 32)) ||
        (rc = s.in(2, counts, 8)))
        return rc;
    rc = pagk_orb_match_device(ctx, params, (int32_t)cq, s.at<uint8_t>(0), s.at<int32_t>(2), (int32_t)ct, s.at<uint8_t>(1),
                               s.at<int32_t>(2) + 1, s.at<int32_t>(3), s.at<int32_t>(4), s.at<uint8_t>(5), s.at<int32_t>(6));
    if (rc || (rc = s.out(3, train_idx, (size_t)nq * 4)) || (rc = s.out(4, distance, (size_t)nq * 4)) ||
        (rc = s.out(5, keep, (size_t)nq)) || (rc = s.out(6, info, kOrbInfoWords * 4)))
        return rc;
    return s.finish();
}

// ---- ORB over a scale pyramid (pagk_orb_levels_kernel.h) ----------------------------------------------------------
namespace {

int orb_extractor_check(const pagk_orb_extractor *e)
{
    if (!e || e->n_levels < 1 || e->n_levels > kOrbMaxLevels || !(e->scale_factor > 1.0f) || !(e->scale_factor <= 1.5f) ||
        e->ini_threshold < 0 || e->ini_threshold > 255 || e->min_threshold < 0 || e->min_threshold > 255 || e->n_features < 1 ||
        e->n_features > (1 << 24))
        return PAGK_E_ARG;
    return PAGK_OK;
}

// The level table of src/ORBextractor.cc:439-470 and :1211-1212 for a W x H image.
struct OrbLevelTable {
    int L = 0;
    int w[kOrbMaxLevels], h[kOrbMaxLevels], quota[kOrbMaxLevels], N[kOrbMaxLevels], size[kOrbMaxLevels], ob[kOrbMaxLevels];
    float sc[kOrbMaxLevels], inv[kOrbMaxLevels];
    FastGrid g[kOrbMaxLevels];
    int64_t cap = 0;   // the sum of the levels' out_bound
};

int orb_level_table(const pagk_orb_extractor *e, int W, int H, OrbLevelTable *t)
{
    if (orb_extractor_check(e) || W < 1 || H < 1 || W > 32767 || H > 32767) return PAGK_E_ARG;
    const int L = t->L = e->n_levels;
    t->sc[0] = 1.0f, t->inv[0] = 1.0f;   // :446-455
    for (int l = 1; l < L; l++) t->sc[l] = t->sc[l - 1] * e->scale_factor, t->inv[l] = 1.0f / t->sc[l];
    const float factor = 1.0f / e->scale_factor;   // :459-470
    double p = 1.0;
    for (int l = 0; l < L; l++) p *= (double)factor;   // (the library's rule in place of pow)
    float nd = ((float)e->n_features * (1.0f - factor)) / (1.0f - (float)p);
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
        t->quota[l] = (int)std::lrint(nd);   // cvRound: ties to even
        sum += t->quota[l];
        nd *= factor;
    }
    t->quota[L - 1] = std::max(e->n_features - sum, 0);
    t->cap = 0;
    for (int l = 0; l < L; l++) {
        t->w[l] = (int)std::lrint((float)W * t->inv[l]), t->h[l] = (int)std::lrint((float)H * t->inv[l]);   // :1211-1212
        t->N[l] = std::max(t->quota[l], 1);
        t->size[l] = (int)(31.0f * t->sc[l]);
        if (!fast_grid(t->w[l], t->h[l], &t->g[l]) || fast_raw_bound(t->g[l]) > (1 << 30)) return PAGK_E_ARG;
        t->ob[l] = fast_out_bound(t->g[l], t->N[l]);
        t->cap += t->ob[l];
    }
    return t->cap > (1ll << 30) ? PAGK_E_ARG : PAGK_OK;
}

int orbl_pitch(int w) { return (w + 3) & ~3; }

// where the levels 1 .. L - 1 lie in buf[ORBL_PYR + slot] (part l - 1 is level l, rows of orbl_pitch(w[l]) bytes)
// (extern "C++": a class template cannot be returned with the C linkage of the block around these helpers)
extern "C++" Layout<kOrbMaxLevels> orbl_pyr_layout(const int *lw, const int *lh, int L)
{
    size_t sizes[kOrbMaxLevels] = {};
    for (int l = 1; l < L; l++) sizes[l - 1] = (size_t)orbl_pitch(lw[l]) * lh[l];
    return Layout<kOrbMaxLevels>(sizes, std::max(L - 1, 1));
}

// the keypoint set of a slot: keypoints | octave | response | angle | descriptors | info ([0] is the set's device count)
struct OrbSet {
    float *kp, *resp, *angle;
    int32_t *octave, *info;
    uint8_t *desc;
};
extern "C++" Layout<6> orbl_set_layout(size_t cap)
{
    const size_t sizes[6] = {cap * 8, cap * 4, cap * 4, cap * 4, cap * 32, kOrbLevelsInfoWords * sizeof(int32_t)};
    return Layout<6>(sizes);
}
OrbSet orbl_set_at(void *b, size_t cap)
{
    const Layout<6> lay = orbl_set_layout(cap);
    return {lay.at<float>(b, 0), lay.at<float>(b, 2), lay.at<float>(b, 3), lay.at<int32_t>(b, 1), lay.at<int32_t>(b, 5),
            lay.at<uint8_t>(b, 4)};
}

// the match result of a query slot: train_idx | distance | keep | info
extern "C++" Layout<4> orbl_match_layout(size_t cap)
{
    const size_t sizes[4] = {cap * 4, cap * 4, cap, kOrbInfoWords * sizeof(int32_t)};
    return Layout<4>(sizes);
}

// a level's slice of buf[ORBL_WS]: the detector's parts, then the blurred level | keypoints | response | angle | descriptors |
// the detector's info | the describer's info
constexpr int kOrblParts = kFastWsParts + 7;

// ORBextractor::operator() (orb != nullptr) or DetectFeatures (orb == nullptr, d_mask or nullptr) on frame slot `slot`, into
// the slot's keypoint set; arguments checked here.  (slots 4 and 5 are the host-buffer forms' own)
int orb_levels_slot(pagk_ctx *ctx, const pagk_orb_extractor *ex, const pagk_orb_params *orb, int32_t slot, const uint8_t *d_mask,
                    const char *what)
{
    if (!ctx || slot < 0 || slot >= kSlots) return PAGK_E_ARG;
    int rc = orb ? orb_params_check(orb) : PAGK_OK;
    if (rc) return rc;
    if (orb && !ctx->orb_pattern_set) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: no sampling pattern set (pagk_orb_set_pattern)", what);
        return PAGK_E_ARG;
    }
    const FrameSlot &s = ctx->slots[slot];
    if (!fast_slot_ok(s)) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: frame slot %d holds no image", what, slot);
        return PAGK_E_ARG;
    }
    OrbLevelTable t;
    if (orb_level_table(ex, s.w, s.h, &t)) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: the extractor's parameters, or a level of a %d x %d image, are outside the definition "
                 "(pagk_orb_extractor_levels)", what, s.w, s.h);
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int L = t.L;
    const char *hint = "run the call once with this image size and these parameters before capturing";
    // the three buffers: workspace, the slot's pyramid, the slot's set
    size_t sizes[kOrbMaxLevels * kOrblParts];
    uint32_t sort_slots[kOrbMaxLevels];
    for (int l = 0; l < L; l++) {
        size_t *z = sizes + l * kOrblParts;
        if (!fast_ws_sizes(t.g[l], t.N[l], z, &sort_slots[l])) return PAGK_E_ARG;
        const size_t ob = (size_t)t.ob[l];
        z[kFastWsParts + 0] = (size_t)orbl_pitch(t.w[l]) * t.h[l];
        z[kFastWsParts + 1] = ob * 8, z[kFastWsParts + 2] = ob * 4, z[kFastWsParts + 3] = ob * 4, z[kFastWsParts + 4] = ob * 32;
        z[kFastWsParts + 5] = 256, z[kFastWsParts + 6] = 256;
    }
    const Layout<kOrbMaxLevels * kOrblParts> wlay(sizes, L * kOrblParts);
    const Layout<kOrbMaxLevels> play = orbl_pyr_layout(t.w, t.h, L);
    const size_t cap = (size_t)t.cap;
    DevBuf &wsb = ctx->buf[pagk_ctx::ORBL_WS], &pyr = ctx->buf[pagk_ctx::ORBL_PYR + slot], &setb = ctx->buf[pagk_ctx::ORBL_SET + slot];
    pagk_ctx::OrbLevelsSlot &st = ctx->orbl[slot];
    if ((rc = reserve(ctx, wsb, wlay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the workspace of ORB over a scale pyramid", hint)))
        return rc;
    rc = reserve(ctx, pyr, play.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the ORB scale pyramid of a slot", hint);
    if (!rc) rc = reserve(ctx, setb, orbl_set_layout(cap).total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the ORB keypoint set of a slot", hint);
    if (rc) {
        if (!pyr.ptr) st.n_levels = 0;   // (a failed allocation left the buffer empty: the slot has no pyramid / no set)
        if (!setb.ptr) st.cap = 0;
        return rc;
    }
    st.n_levels = 0, st.cap = 0;   // nothing valid until everything has been enqueued
    // the pyramid (:1207-1230): level l from level l - 1
    const uint8_t *img[kOrbMaxLevels];
    long long pitch[kOrbMaxLevels];
    img[0] = s.img0, pitch[0] = (long long)s.pitch0;
    for (int l = 1; l < L; l++) {
        OrbResizeArgs r;
        r.src = img[l - 1], r.spitch = pitch[l - 1], r.dst = play.at<uint8_t>(pyr.ptr, l - 1);
        r.sw = t.w[l - 1], r.sh = t.h[l - 1], r.dw = t.w[l], r.dh = t.h[l], r.dpitch = orbl_pitch(t.w[l]);
        r.scale_x = 1.0 / ((double)r.dw / r.sw), r.scale_y = 1.0 / ((double)r.dh / r.sh);
        hipLaunchKernelGGL(k_orb_resize, dim3((unsigned)((r.dpitch / 4 + 63) / 64), (unsigned)((r.dh + 3) / 4)), dim3(256), 0,
                           ctx->stream, r);
        HIPCHK(ctx, hipGetLastError());
        img[l] = r.dst, pitch[l] = r.dpitch;
    }
    // the stages of the one-level definition, one launch each, the level as a grid dimension
    FastCellLevels cells;
    FastListLevels lists;
    FastTreeLevels trees;
    OrbBlurLevels blurs;
    OrbDescLevels descs;
    OrbPackArgs pk;
    memset(&cells, 0, sizeof cells), memset(&lists, 0, sizeof lists), memset(&trees, 0, sizeof trees);
    memset(&blurs, 0, sizeof blurs), memset(&descs, 0, sizeof descs), memset(&pk, 0, sizeof pk);
    int max_cells = 0, max_bx = 0, max_by = 0, max_db = 0;
    pagk_fast_params fp;
    fp.ini_threshold = ex->ini_threshold, fp.min_threshold = ex->min_threshold, fp.n_features = 0, fp.n_levels = 1;
    for (int l = 0; l < L; l++) {
        FastWs ws;
        fast_ws_carve(wlay.off + l * kOrblParts, wsb.ptr, t.g[l], t.N[l], sort_slots[l], &ws);
        const int first = l * kOrblParts + kFastWsParts;
        uint8_t *blur = wlay.at<uint8_t>(wsb.ptr, first);
        float *kp = wlay.at<float>(wsb.ptr, first + 1), *resp = wlay.at<float>(wsb.ptr, first + 2);
        float *angle = wlay.at<float>(wsb.ptr, first + 3);
        uint8_t *desc = wlay.at<uint8_t>(wsb.ptr, first + 4);
        int32_t *finfo = wlay.at<int32_t>(wsb.ptr, first + 5), *oinfo = wlay.at<int32_t>(wsb.ptr, first + 6);
        FastCellArgs &c = cells.a[l];
        c.img = img[l], c.pitch = pitch[l], c.g = t.g[l], c.t_ini = fp.ini_threshold, c.t_min = fp.min_threshold;
        c.seg_xy = ws.seg_xy, c.seg_score = ws.seg_score, c.cell_cnt = ws.cell_cnt, c.skip = nullptr;
        cells.n_cells[l] = ws.n_cells;
        max_cells = std::max(max_cells, ws.n_cells);
        FastListArgs &li = lists.a[l];
        li.n_cells = ws.n_cells, li.seg = t.g[l].seg, li.cell_cnt = ws.cell_cnt, li.cell_off = ws.cell_off, li.ctl = ws.ctl;
        li.seg_xy = ws.seg_xy, li.seg_score = ws.seg_score, li.kxy = ws.kxy, li.kscore = ws.kscore;
        FastTreeArgs &tr = trees.a[l];
        tr.g = t.g[l], tr.n_features = t.N[l], tr.cap = t.ob[l], tr.out_bound = ws.out_bound, tr.raw_bound = ws.raw_bound;
        tr.sort_slots = ws.sort_slots, tr.ctl = ws.ctl, tr.kxy = ws.kxy, tr.kscore = ws.kscore, tr.knode = ws.knode;
        for (int k = 0; k < 2; k++) tr.box[k] = ws.box[k], tr.ncnt[k] = ws.ncnt[k], tr.ncand[k] = ws.ncand[k];
        tr.cnt4 = ws.cnt4, tr.cbase = ws.cbase, tr.split = ws.split, tr.sortk = ws.sortk, tr.best = ws.best;
        tr.mask = nullptr, tr.out_xy = kp, tr.out_resp = resp, tr.info = finfo, tr.skip = nullptr;
        OrbBlurArgs &b = blurs.a[l];
        b.img = img[l], b.pitch = pitch[l], b.blur = blur, b.info = oinfo, b.W = t.w[l], b.H = t.h[l], b.wp = orbl_pitch(t.w[l]);
        if (orb) b.w0 = orb->blur_weights[0], b.w1 = orb->blur_weights[1], b.w2 = orb->blur_weights[2], b.w3 = orb->blur_weights[3];
        blurs.nbx[l] = (t.w[l] + kOrbBlurTx - 1) / kOrbBlurTx, blurs.nby[l] = (t.h[l] + kOrbBlurTy - 1) / kOrbBlurTy;
        max_bx = std::max(max_bx, blurs.nbx[l]), max_by = std::max(max_by, blurs.nby[l]);
        OrbDescArgs &d = descs.a[l];
        d.img = img[l], d.pitch = pitch[l], d.blur = blur;
        d.pattern = static_cast<const int32_t *>(ctx->buf[pagk_ctx::ORB_PATTERN].ptr);
        d.keypoints = kp, d.n = finfo, d.angle = angle, d.desc = desc, d.info = oinfo;
        d.W = t.w[l], d.H = t.h[l], d.wp = b.wp, d.cap = t.ob[l];
        descs.n_blocks[l] = (t.ob[l] + 3) / 4;
        max_db = std::max(max_db, descs.n_blocks[l]);
        OrbPackLevel &v = pk.lv[l];
        v.kp = kp, v.resp = resp, v.angle = orb ? angle : nullptr, v.desc = orb ? desc : nullptr, v.fast_info = finfo;
        v.orb_info = orb ? oinfo : nullptr, v.seg_cap = t.ob[l], v.quota = t.quota[l], v.scale = t.sc[l];
    }
    hipLaunchKernelGGL(k_fast_cells_levels, dim3((unsigned)max_cells, (unsigned)L), dim3(256), 0, ctx->stream, cells);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fast_offsets_levels, dim3((unsigned)L), dim3(1024), 0, ctx->stream, lists);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fast_gather_levels, dim3((unsigned)max_cells, (unsigned)L), dim3(256), 0, ctx->stream, lists);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fast_tree_levels, dim3((unsigned)L), dim3(1024), 0, ctx->stream, trees);
    HIPCHK(ctx, hipGetLastError());
    if (orb) {
        hipLaunchKernelGGL(k_orb_blur_levels, dim3((unsigned)max_bx, (unsigned)max_by, (unsigned)L), dim3(256), 0, ctx->stream, blurs);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_orb_describe_levels, dim3((unsigned)max_db, (unsigned)L), dim3(256), 0, ctx->stream, descs);
        HIPCHK(ctx, hipGetLastError());
    }
    const OrbSet set = orbl_set_at(setb.ptr, cap);
    pk.n_levels = L, pk.cap = (int32_t)cap, pk.W = s.w, pk.H = s.h, pk.mask = d_mask;
    pk.kp = set.kp, pk.octave = set.octave, pk.resp = set.resp, pk.angle = set.angle, pk.desc = set.desc, pk.info = set.info;
    hipLaunchKernelGGL(k_orb_pack, dim3(1), dim3(1024), 0, ctx->stream, pk);
    HIPCHK(ctx, hipGetLastError());
    st.w = s.w, st.h = s.h, st.n_levels = L, st.cap = (int)cap, st.described = orb != nullptr;
    std::copy(t.w, t.w + L, st.lw), std::copy(t.h, t.h + L, st.lh);
    return PAGK_OK;
}

// the slot's set into host arrays (cap rows each; rows at or beyond the set's capacity are zeroed here)
int orb_slot_read(pagk_ctx *ctx, int32_t slot, int32_t cap, float *keypoints, int32_t *octave, float *response, float *angle,
                  uint8_t *desc, int32_t *info)
{
    if (!ctx || slot < 0 || slot >= kSlots || !keypoints) return PAGK_E_ARG;
    const pagk_ctx::OrbLevelsSlot &st = ctx->orbl[slot];
    if (st.cap < 1 || cap < st.cap) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_orb_slot_read: slot %d has %s (cap %d)", slot,
                 st.cap < 1 ? "no keypoint set" : "a set of more rows than cap", cap);
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)st.cap, rest = (size_t)cap - n;
    const OrbSet set = orbl_set_at(ctx->buf[pagk_ctx::ORBL_SET + slot].ptr, n);
    hipStream_t q = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(keypoints, set.kp, n * 8, hipMemcpyDeviceToHost, q));
    if (octave) HIPCHK(ctx, hipMemcpyAsync(octave, set.octave, n * 4, hipMemcpyDeviceToHost, q));
    if (response) HIPCHK(ctx, hipMemcpyAsync(response, set.resp, n * 4, hipMemcpyDeviceToHost, q));
    if (angle && st.described) HIPCHK(ctx, hipMemcpyAsync(angle, set.angle, n * 4, hipMemcpyDeviceToHost, q));
    if (desc && st.described) HIPCHK(ctx, hipMemcpyAsync(desc, set.desc, n * 32, hipMemcpyDeviceToHost, q));
    if (info) HIPCHK(ctx, hipMemcpyAsync(info, set.info, kOrbLevelsInfoWords * sizeof(int32_t), hipMemcpyDeviceToHost, q));
    HIPCHK(ctx, hipStreamSynchronize(q));
    memset(keypoints + 2 * n, 0, rest * 8);
    if (octave) memset(octave + n, 0, rest * 4);
    if (response) memset(response + n, 0, rest * 4);
    if (angle) memset(angle + (st.described ? n : 0), 0, (st.described ? rest : (size_t)cap) * 4);
    if (desc) memset(desc + (st.described ? n * 32 : 0), 0, (st.described ? rest : (size_t)cap) * 32);
    return PAGK_OK;
}

}  // namespace

void pagk_orb_extractor_default(pagk_orb_extractor *e)
{
    if (!e) return;
    e->n_features = 1000;      // the arguments ORB is normally run with (src/ORBextractor.cc:434-437)
    e->scale_factor = 1.2f;
    e->n_levels = 8;           // "int nLevels = 1;    // 8", Examples/Demo/RealSenseD435i.cpp:187
    e->ini_threshold = 20;
    e->min_threshold = 7;
}

int pagk_orb_extractor_check(const pagk_orb_extractor *e) { return orb_extractor_check(e); }

int pagk_orb_extractor_levels(const pagk_orb_extractor *ex, int32_t width, int32_t height, int32_t *level_width,
                              int32_t *level_height, float *scale, int32_t *quota, int32_t *size, int32_t *out_bound)
{
    OrbLevelTable t;
    if (orb_level_table(ex, width, height, &t)) return PAGK_E_ARG;
    for (int l = 0; l < kOrbMaxLevels; l++) {
        const bool in = l < t.L;
        if (level_width) level_width[l] = in ? t.w[l] : 0;
        if (level_height) level_height[l] = in ? t.h[l] : 0;
        if (scale) scale[l] = in ? t.sc[l] : 0.0f;
        if (quota) quota[l] = in ? t.quota[l] : 0;
        if (size) size[l] = in ? t.size[l] : 0;
    }
    if (out_bound) *out_bound = (int32_t)t.cap;
    return PAGK_OK;
}

int pagk_orb_extract_slot(pagk_ctx *ctx, const pagk_orb_extractor *ex, const pagk_orb_params *orb, int32_t slot)
{
    if (!ctx || !orb || slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    return orb_levels_slot(ctx, ex, orb, slot, nullptr, "pagk_orb_extract_slot");
}

int pagk_orb_slot_read(pagk_ctx *ctx, int32_t slot, int32_t cap, float *keypoints, int32_t *octave, float *response,
                       float *angle, uint8_t *desc, int32_t *info)
{
    if (!ctx || slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_orb_slot_read");
    return orb_slot_read(ctx, slot, cap, keypoints, octave, response, angle, desc, info);
}

int pagk_orb_match_slots(pagk_ctx *ctx, const pagk_orb_params *orb, int32_t slot_q, int32_t slot_t)
{
    if (!ctx || slot_q < 0 || slot_q >= kUserSlots || slot_t < 0 || slot_t >= kUserSlots) return PAGK_E_ARG;
    int rc = orb_params_check(orb);
    if (rc) return rc;
    pagk_ctx::OrbLevelsSlot &q = ctx->orbl[slot_q];
    const pagk_ctx::OrbLevelsSlot &t = ctx->orbl[slot_t];
    if (q.cap < 1 || t.cap < 1 || !q.described || !t.described) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_orb_match_slots: slots %d and %d need a described keypoint set each "
                 "(pagk_orb_extract_slot)", slot_q, slot_t);
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf &mb = ctx->buf[pagk_ctx::ORBL_MATCH + slot_q];
    const Layout<4> lay = orbl_match_layout((size_t)q.cap);
    if ((rc = reserve(ctx, mb, lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the ORB match result of a slot",
                      "run the call once with these sets before capturing"))) {
        if (!mb.ptr) q.match_cap = 0;
        return rc;
    }
    q.match_cap = 0;
    const OrbSet sq = orbl_set_at(ctx->buf[pagk_ctx::ORBL_SET + slot_q].ptr, (size_t)q.cap);
    const OrbSet stt = orbl_set_at(ctx->buf[pagk_ctx::ORBL_SET + slot_t].ptr, (size_t)t.cap);
    rc = pagk_orb_match_device(ctx, orb, q.cap, sq.desc, sq.info, t.cap, stt.desc, stt.info, lay.at<int32_t>(mb.ptr, 0),
                               lay.at<int32_t>(mb.ptr, 1), lay.at<uint8_t>(mb.ptr, 2), lay.at<int32_t>(mb.ptr, 3));
    if (!rc) q.match_cap = q.cap;
    return rc;
}

int pagk_orb_match_slots_read(pagk_ctx *ctx, int32_t slot_q, int32_t cap, int32_t *train_idx, int32_t *distance, uint8_t *keep,
                              int32_t *info)
{
    if (!ctx || slot_q < 0 || slot_q >= kUserSlots || !train_idx || !distance || !keep) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_orb_match_slots_read");
    const pagk_ctx::OrbLevelsSlot &q = ctx->orbl[slot_q];
    if (q.match_cap < 1 || q.match_cap != q.cap || cap < q.match_cap) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_orb_match_slots_read: slot %d has no match result of at most cap = %d rows "
                 "(pagk_orb_match_slots)", slot_q, cap);
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)q.match_cap;
    const Layout<4> lay = orbl_match_layout(n);
    void *b = ctx->buf[pagk_ctx::ORBL_MATCH + slot_q].ptr;
    HIPCHK(ctx, hipMemcpyAsync(train_idx, lay.at<void>(b, 0), n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(distance, lay.at<void>(b, 1), n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(keep, lay.at<void>(b, 2), n, hipMemcpyDeviceToHost, ctx->stream));
    if (info) HIPCHK(ctx, hipMemcpyAsync(info, lay.at<void>(b, 3), kOrbInfoWords * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = n; i < (size_t)cap; i++) train_idx[i] = -1, distance[i] = 257, keep[i] = 0;   // as rows at or beyond nq
    return PAGK_OK;
}

int pagk_orb_extract_levels(pagk_ctx *ctx, const pagk_orb_extractor *ex, const pagk_orb_params *orb, const pagk_image *img,
                            int32_t cap, float *keypoints, int32_t *octave, float *response, float *angle, uint8_t *desc,
                            int32_t *info)
{
    if (!ctx || !img || !orb || !keypoints) return PAGK_E_ARG;
    int rc = orb_params_check(orb);
    if (rc) return rc;
    NOT_WHILE_CAPTURING(ctx, "pagk_orb_extract_levels");
    OrbLevelTable t;
    if (check_image(img) || orb_level_table(ex, img->width, img->height, &t) || cap < t.cap) return PAGK_E_ARG;
    if ((rc = frame_upload_any(ctx, 4, img, 1))) return rc;
    if ((rc = orb_levels_slot(ctx, ex, orb, 4, nullptr, "pagk_orb_extract_levels"))) return rc;
    return orb_slot_read(ctx, 4, cap, keypoints, octave, response, angle, desc, info);
}

int pagk_orb_detect_levels(pagk_ctx *ctx, const pagk_orb_extractor *ex, const pagk_image *img, const uint8_t *mask, int32_t cap,
                           float *keypoints, int32_t *octave, float *response, int32_t *info)
{
    if (!ctx || !img || !keypoints) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_orb_detect_levels");
    OrbLevelTable t;
    if (check_image(img) || orb_level_table(ex, img->width, img->height, &t) || cap < t.cap) return PAGK_E_ARG;
    int rc = frame_upload_any(ctx, 4, img, 1);
    if (rc) return rc;
    const size_t px = (size_t)img->width * img->height;
    const size_t sizes[1] = {px};
    Staged<1> s(ctx, sizes);
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, mask, px))) return rc;
    if ((rc = orb_levels_slot(ctx, ex, nullptr, 4, mask ? s.at<uint8_t>(0) : nullptr, "pagk_orb_detect_levels"))) return rc;
    if ((rc = orb_slot_read(ctx, 4, cap, keypoints, octave, response, nullptr, nullptr, info))) return rc;
    return s.finish();
}

int pagk_selftest_orb_level(pagk_ctx *ctx, int32_t slot, int32_t level, uint8_t *dst, int64_t pitch)
{
    if (!ctx || slot < 0 || slot >= kUserSlots || !dst) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_orb_level");
    const FrameSlot &s = ctx->slots[slot];
    const pagk_ctx::OrbLevelsSlot &st = ctx->orbl[slot];
    if (!fast_slot_ok(s) || st.n_levels < 1 || st.w != s.w || st.h != s.h || level < 0 || level >= st.n_levels ||
        pitch < st.lw[level])
        return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const Layout<kOrbMaxLevels> lay = orbl_pyr_layout(st.lw, st.lh, st.n_levels);
    const uint8_t *src = level ? lay.at<uint8_t>(ctx->buf[pagk_ctx::ORBL_PYR + slot].ptr, level - 1) : s.img0;
    const size_t spitch = level ? (size_t)orbl_pitch(st.lw[level]) : (size_t)s.pitch0;
    HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)pitch, src, spitch, (size_t)st.lw[level], (size_t)st.lh[level], hipMemcpyDeviceToHost,
                                 ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PAGK_OK;
}

// ---- pyramidal Lucas-Kanade, tracker type 0 (pagk_lk_kernel.h) ---------------------------------------------------
namespace {

int lk_params_check(const pagk_lk_params *p)
{
    if (!p || p->half_patch < 1 || p->half_patch > PAGK_MAX_HALF_PATCH || p->max_level < 0 || p->max_level >= PAGK_MAX_PYRAMIDS ||
        p->max_count < 1 || !std::isfinite(p->epsilon) || p->epsilon < 0.0 || !std::isfinite(p->min_eig_threshold) ||
        p->min_eig_threshold < 0.0 || !std::isfinite(p->err_threshold) || p->err_threshold < 0.0f)
        return PAGK_E_ARG;
    return PAGK_OK;
}

// sizes of levels 0 .. top and the top level itself (buildOpticalFlowPyramid's stop rule), or PAGK_E_ARG
int lk_levels(int w, int h, const pagk_lk_params *p, int *lw, int *lh)
{
    const int win = 2 * p->half_patch + 1;
    if (w <= win || h <= win) return PAGK_E_ARG;
    lw[0] = w, lh[0] = h;
    int top = 0;
    while (top < p->max_level) {
        const int nw = (lw[top] + 1) / 2, nh = (lh[top] + 1) / 2;
        if (nw <= win || nh <= win) break;
        top++;
        lw[top] = nw, lh[top] = nh;
    }
    return top;
}

// where the levels 1 .. top lie in buf[LK_PYR + slot] (part l - 1 is level l, rows of lw[l] bytes)
extern "C++" Layout<kLkMaxLevels> lk_layout(const int *lw, const int *lh, int top)
{
    size_t sizes[kLkMaxLevels] = {};
    for (int l = 1; l <= top; l++) sizes[l - 1] = (size_t)lw[l] * lh[l];
    return Layout<kLkMaxLevels>(sizes, std::max(top, 1));
}

bool lk_slot_ok(const FrameSlot &s) { return s.valid && s.img0; }

// the arguments of the pyrDown launch that builds level l (1 .. top) of slot s in `base` (of one launch, or of a group's record)
extern "C++" LkPyrArgs lk_pyr_args(const FrameSlot &s, const Layout<kLkMaxLevels> &lay, void *base, const int *lw, const int *lh, int l)
{
    LkPyrArgs a;
    a.src = l == 1 ? s.img0 : lay.at<uint8_t>(base, l - 2);
    a.spitch = l == 1 ? (long long)s.pitch0 : (long long)lw[l - 1];
    a.dst = lay.at<uint8_t>(base, l - 1);
    a.sw = lw[l - 1], a.sh = lh[l - 1], a.dw = lw[l], a.dh = lh[l];
    return a;
}

// (slots 4 and 5 are the host-buffer form's own)
int lk_pyramid_slot(pagk_ctx *ctx, const pagk_lk_params *params, int32_t slot)
{
    if (!ctx || lk_params_check(params) || slot < 0 || slot >= kSlots) return PAGK_E_ARG;
    const FrameSlot &s = ctx->slots[slot];
    if (!lk_slot_ok(s)) return PAGK_E_ARG;
    int lw[kLkMaxLevels], lh[kLkMaxLevels];
    const int top = lk_levels(s.w, s.h, params, lw, lh);
    if (top < 0) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const Layout<kLkMaxLevels> lay = lk_layout(lw, lh, top);
    DevBuf &pyr = ctx->buf[pagk_ctx::LK_PYR + slot];
    int rc = reserve(ctx, pyr, lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the Lucas-Kanade pyramid of a slot",
                     "run the call once with this image size and these parameters before capturing");
    if (rc) {
        if (!pyr.ptr) ctx->lk_pyr[slot].top = -1;   // (a failed allocation left the buffer empty: the slot has no pyramid)
        return rc;
    }
    ctx->lk_pyr[slot].top = -1;   // nothing valid until every level has been enqueued
    for (int l = 1; l <= top; l++) {
        const LkPyrArgs a = lk_pyr_args(s, lay, pyr.ptr, lw, lh, l);
        hipLaunchKernelGGL(k_lk_pyrdown, dim3((unsigned)((a.dw + 63) / 64), (unsigned)((a.dh + 3) / 4)), dim3(256), 0, ctx->stream, a);
        HIPCHK(ctx, hipGetLastError());
    }
    ctx->lk_pyr[slot].w = s.w, ctx->lk_pyr[slot].h = s.h, ctx->lk_pyr[slot].top = top;
    return PAGK_OK;
}

// What both trackers check and the launch arguments they share: the levels of both slots, the arrays, the constants.
int lk_track_args(pagk_ctx *ctx, const pagk_lk_params *params, int32_t slot_ref, int32_t slot_cur, int32_t cap,
                  const float *d_pt_ref, const int32_t *d_n, float *d_pt_out, uint8_t *d_status, uint8_t *d_status_raw,
                  float *d_err, float *d_flow, int32_t *d_info, LkTrackArgs *out)
{
    if (!ctx || lk_params_check(params) || slot_ref < 0 || slot_ref >= kSlots || slot_cur < 0 || slot_cur >= kSlots ||
        cap < 1 || cap > kLkMaxRows || !d_pt_ref || !d_pt_out || !d_status || !d_err || !d_info)
        return PAGK_E_ARG;
    const FrameSlot &r = ctx->slots[slot_ref], &c = ctx->slots[slot_cur];
    if (!lk_slot_ok(r) || !lk_slot_ok(c) || r.w != c.w || r.h != c.h) return PAGK_E_ARG;
    int lw[kLkMaxLevels], lh[kLkMaxLevels];
    const int top = lk_levels(r.w, r.h, params, lw, lh);
    if (top < 0) return PAGK_E_ARG;
    const int32_t both[2] = {slot_ref, slot_cur};
    for (int32_t slot : both) {
        const pagk_ctx::LkPyr &p = ctx->lk_pyr[slot];
        if (p.top < top || p.w != r.w || p.h != r.h) {
            snprintf(ctx->err, sizeof(ctx->err), "pagk_lk_track_device: slot %d has no Lucas-Kanade pyramid of %d x %d with top level %d "
                     "(pagk_lk_pyramid_device)", slot, r.w, r.h, top);
            return PAGK_E_ARG;
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LkTrackArgs a = {};
    for (int k = 0; k < 2; k++) {
        const FrameSlot &s = k ? c : r;
        // (a level's offset depends on the levels below it alone: the same whatever top level the buffer was carved for)
        const Layout<kLkMaxLevels> lay = lk_layout(lw, lh, top);
        void *base = ctx->buf[pagk_ctx::LK_PYR + both[k]].ptr;
        for (int l = 0; l <= top; l++) {
            const uint8_t *img = l ? lay.at<uint8_t>(base, l - 1) : s.img0;
            const long long pitch = l ? (long long)lw[l] : (long long)s.pitch0;
            if (k)
                a.lv[l].J = img, a.lv[l].pitch_j = pitch;
            else
                a.lv[l].I = img, a.lv[l].pitch_i = pitch;
            a.lv[l].w = lw[l], a.lv[l].h = lh[l];
        }
    }
    a.pt_ref = d_pt_ref, a.n = d_n, a.pt_out = d_pt_out, a.status = d_status, a.status_raw = d_status_raw, a.err = d_err;
    a.flow = d_flow, a.info = d_info;
    a.eps2 = params->epsilon * params->epsilon, a.min_eig = params->min_eig_threshold, a.err_threshold = params->err_threshold;
    a.cap = cap, a.win = 2 * params->half_patch + 1, a.top = top, a.max_count = params->max_count;
    *out = a;
    return PAGK_OK;
}

using LkKernel = void (*)(LkTrackArgs);
LkKernel lk_kernel(int win)
{
    switch (lk_npix(win)) {
        case 1: return k_lk_track<1>;
        case 2: return k_lk_track<2>;
        case 4: return k_lk_track<4>;
        case 8: return k_lk_track<8>;
        default: return k_lk_track<16>;
    }
}

int lk_track_slots(pagk_ctx *ctx, const pagk_lk_params *params, int32_t slot_ref, int32_t slot_cur, int32_t cap,
                   const float *d_pt_ref, const int32_t *d_n, float *d_pt_out, uint8_t *d_status, uint8_t *d_status_raw,
                   float *d_err, float *d_flow, int32_t *d_info)
{
    LkTrackArgs a;
    int rc = lk_track_args(ctx, params, slot_ref, slot_cur, cap, d_pt_ref, d_n, d_pt_out, d_status, d_status_raw, d_err, d_flow,
                           d_info, &a);
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(d_info, 0, kLkInfoWords * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(lk_kernel(a.win), dim3((unsigned)((cap + 3) / 4)), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

// Lucas-Kanade from an initial point, live rows only, with the distorted output (k_lk_flow): the chooser mirrors lk_kernel
using LkFlowKernel = void (*)(LkFlowArgs);
LkFlowKernel lk_flow_kernel(int win)
{
    switch (lk_npix(win)) {
        case 1: return k_lk_flow<1>;
        case 2: return k_lk_flow<2>;
        case 4: return k_lk_flow<4>;
        case 8: return k_lk_flow<8>;
        default: return k_lk_flow<16>;
    }
}

// ... and k_group_lk_flow (pagk_group_lk_kernel.h), every camera of a Lucas-Kanade group in one launch: the same chooser
using LkGroupFlowKernel = void (*)(const LkGroupRec *);
LkGroupFlowKernel lk_group_flow_kernel(int win)
{
    switch (lk_npix(win)) {
        case 1: return k_group_lk_flow<1>;
        case 2: return k_group_lk_flow<2>;
        case 4: return k_group_lk_flow<4>;
        case 8: return k_group_lk_flow<8>;
        default: return k_group_lk_flow<16>;
    }
}

// The arguments of k_lk_flow: of one launch, or of one camera's record of a Lucas-Kanade group.
// cam: the camera of d_pt_out_dist (required with it); d_pt_init, d_status_in, d_pt_out_dist may be nullptr
int lk_flow_args(pagk_ctx *ctx, const pagk_lk_params *params, const pagk_params *cam, int32_t slot_ref, int32_t slot_cur,
                 int32_t cap, const float *d_pt_ref, const float *d_pt_init, const uint8_t *d_status_in, const int32_t *d_n,
                 float *d_pt_out, float *d_pt_out_dist, uint8_t *d_status, uint8_t *d_status_raw, float *d_err, float *d_flow,
                 int32_t *d_info, LkFlowArgs *out)
{
    if (d_pt_out_dist && !cam) return PAGK_E_ARG;
    LkFlowArgs f = {};
    int rc = lk_track_args(ctx, params, slot_ref, slot_cur, cap, d_pt_ref, d_n, d_pt_out, d_status, d_status_raw, d_err, d_flow,
                           d_info, &f.t);
    if (rc) return rc;
    f.pt_init = d_pt_init, f.status_in = d_status_in, f.pt_out_dist = d_pt_out_dist;
    if (cam) {   // as fill_param_args takes the camera for the PatchMatch epilogue
        f.distort_on = cam->dist_coef[0] != 0.0f;
        f.fx = cam->fx, f.fy = cam->fy, f.cx = cam->cx, f.cy = cam->cy;
        f.fx_inv = (float)(1.0 / (double)cam->fx);  // src/utils.cpp:53
        f.fy_inv = (float)(1.0 / (double)cam->fy);
        f.k1 = cam->dist_coef[0], f.k2 = cam->dist_coef[1], f.p1 = cam->dist_coef[2], f.p2 = cam->dist_coef[3];
        f.k3 = cam->n_dist_coef == 5 ? cam->dist_coef[4] : 0.0f;
    }
    *out = f;
    return PAGK_OK;
}

int lk_flow_slots(pagk_ctx *ctx, const pagk_lk_params *params, const pagk_params *cam, int32_t slot_ref, int32_t slot_cur,
                  int32_t cap, const float *d_pt_ref, const float *d_pt_init, const uint8_t *d_status_in, const int32_t *d_n,
                  float *d_pt_out, float *d_pt_out_dist, uint8_t *d_status, uint8_t *d_status_raw, float *d_err, float *d_flow,
                  int32_t *d_info)
{
    LkFlowArgs f;
    int rc = lk_flow_args(ctx, params, cam, slot_ref, slot_cur, cap, d_pt_ref, d_pt_init, d_status_in, d_n, d_pt_out, d_pt_out_dist,
                          d_status, d_status_raw, d_err, d_flow, d_info, &f);
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(d_info, 0, kLkInfoWords * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(lk_flow_kernel(f.t.win), dim3((unsigned)((cap + 3) / 4)), dim3(256), 0, ctx->stream, f);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

}  // namespace

void pagk_lk_params_default(pagk_lk_params *p)
{
    if (!p) return;
    p->half_patch = 10;           // mHalfPatchSize of the reference's experiment
    p->max_level = 2;             // src/gyro_aided_tracker.cpp:362
    p->max_count = 30;            // :363
    p->epsilon = 0.01;            // :363
    p->min_eig_threshold = 1e-4;  // :366
    p->err_threshold = 12.0f;     // :372
}

int pagk_lk_params_check(const pagk_lk_params *p) { return lk_params_check(p); }

int pagk_lk_levels(int32_t width, int32_t height, const pagk_lk_params *params)
{
    if (lk_params_check(params) || width < 1 || height < 1) return PAGK_E_ARG;
    int lw[kLkMaxLevels], lh[kLkMaxLevels];
    return lk_levels(width, height, params, lw, lh);
}

int pagk_lk_pyramid_device(pagk_ctx *ctx, const pagk_lk_params *params, int32_t slot)
{
    if (slot < 0 || slot >= kUserSlots) return PAGK_E_ARG;
    return lk_pyramid_slot(ctx, params, slot);
}

int pagk_lk_track_device(pagk_ctx *ctx, const pagk_lk_params *params, int32_t slot_ref, int32_t slot_cur, int32_t cap,
                         const float *d_pt_ref, const int32_t *d_n, float *d_pt_out, uint8_t *d_status, uint8_t *d_status_raw,
                         float *d_err, float *d_flow, int32_t *d_info)
{
    if (slot_ref < 0 || slot_ref >= kUserSlots || slot_cur < 0 || slot_cur >= kUserSlots) return PAGK_E_ARG;
    return lk_track_slots(ctx, params, slot_ref, slot_cur, cap, d_pt_ref, d_n, d_pt_out, d_status, d_status_raw, d_err, d_flow,
                          d_info);
}

int pagk_lk_track(pagk_ctx *ctx, const pagk_lk_params *params, const pagk_image *ref, const pagk_image *cur, int32_t n,
                  const float *pt_ref, float *pt_out, uint8_t *status, uint8_t *status_raw, float *err, float *flow,
                  int32_t *info)
{
    if (!ctx || !ref || !cur || lk_params_check(params)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_lk_track");
    if (n < 0 || n > kLkMaxRows || (n && (!pt_ref || !pt_out || !status || !err))) return PAGK_E_ARG;
    if (ref->width != cur->width || ref->height != cur->height || pagk_lk_levels(ref->width, ref->height, params) < 0)
        return PAGK_E_ARG;
    int rc;
    if ((rc = frame_upload_any(ctx, 4, ref, 1)) || (rc = frame_upload_any(ctx, 5, cur, 1))) return rc;
    if ((rc = lk_pyramid_slot(ctx, params, 4)) || (rc = lk_pyramid_slot(ctx, params, 5))) return rc;
    const size_t nc = (size_t)std::max(n, 1);
    // points in | count | points out | status | raw status | err | flow | info
    const size_t sizes[8] = {nc * 8, 256, nc * 8, nc, nc, nc * 4, nc * 8, 256};
    const size_t nn = (size_t)n;
    Staged<8> s(ctx, sizes);
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, pt_ref, nn * 8)) || (rc = s.in(1, &n, 4))) return rc;
    rc = lk_track_slots(ctx, params, 4, 5, (int32_t)nc, s.at<float>(0), s.at<int32_t>(1), s.at<float>(2), s.at<uint8_t>(3),
                        s.at<uint8_t>(4), s.at<float>(5), s.at<float>(6), s.at<int32_t>(7));
    if (rc || (rc = s.out(2, pt_out, nn * 8)) || (rc = s.out(3, status, nn)) || (rc = s.out(4, status_raw, nn)) ||
        (rc = s.out(5, err, nn * 4)) || (rc = s.out(6, flow, nn * 8)) || (rc = s.out(7, info, kLkInfoWords * 4)))
        return rc;
    return s.finish();
}

int pagk_lk_track_flow(pagk_ctx *ctx, const pagk_lk_params *params, const pagk_params *cam, const pagk_image *ref,
                       const pagk_image *cur, int32_t n, const float *pt_ref, const float *pt_init, const uint8_t *status_in,
                       float *pt_out, float *pt_out_dist, uint8_t *status, uint8_t *status_raw, float *err, float *flow,
                       int32_t *info)
{
    if (!ctx || !ref || !cur || lk_params_check(params) || (cam && check_params(cam)) || (pt_out_dist && !cam)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_lk_track_flow");
    if (n < 0 || n > kLkMaxRows || (n && (!pt_ref || !pt_out || !status || !err))) return PAGK_E_ARG;
    if (ref->width != cur->width || ref->height != cur->height || pagk_lk_levels(ref->width, ref->height, params) < 0)
        return PAGK_E_ARG;
    int rc;
    if ((rc = frame_upload_any(ctx, 4, ref, 1)) || (rc = frame_upload_any(ctx, 5, cur, 1))) return rc;
    if ((rc = lk_pyramid_slot(ctx, params, 4)) || (rc = lk_pyramid_slot(ctx, params, 5))) return rc;
    const size_t nc = (size_t)std::max(n, 1);
    // points in | count | initial points | live mask | points out | distorted | status | raw status | err | flow | info
    const size_t sizes[11] = {nc * 8, 256, nc * 8, nc, nc * 8, nc * 8, nc, nc, nc * 4, nc * 8, 256};
    const size_t nn = (size_t)n;
    Staged<11> s(ctx, sizes);
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, pt_ref, nn * 8)) || (rc = s.in(1, &n, 4)) ||
        (rc = s.in(2, pt_init, nn * 8)) || (rc = s.in(3, status_in, nn)))
        return rc;
    rc = lk_flow_slots(ctx, params, cam, 4, 5, (int32_t)nc, s.at<float>(0), pt_init ? s.at<float>(2) : nullptr,
                       status_in ? s.at<uint8_t>(3) : nullptr, s.at<int32_t>(1), s.at<float>(4),
                       pt_out_dist ? s.at<float>(5) : nullptr, s.at<uint8_t>(6), s.at<uint8_t>(7), s.at<float>(8), s.at<float>(9),
                       s.at<int32_t>(10));
    if (rc || (rc = s.out(4, pt_out, nn * 8)) || (rc = s.out(5, pt_out_dist, nn * 8)) || (rc = s.out(6, status, nn)) ||
        (rc = s.out(7, status_raw, nn)) || (rc = s.out(8, err, nn * 4)) || (rc = s.out(9, flow, nn * 8)) ||
        (rc = s.out(10, info, kLkInfoWords * 4)))
        return rc;
    return s.finish();
}

int pagk_selftest_lk_level(pagk_ctx *ctx, int32_t slot, int32_t level, uint8_t *dst, int64_t pitch)
{
    if (!ctx || slot < 0 || slot >= kUserSlots || !dst) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_lk_level");
    const FrameSlot &s = ctx->slots[slot];
    const pagk_ctx::LkPyr &p = ctx->lk_pyr[slot];
    if (!lk_slot_ok(s) || p.top < 0 || p.w != s.w || p.h != s.h || level < 1 || level > p.top) return PAGK_E_ARG;
    int lw[kLkMaxLevels], lh[kLkMaxLevels];
    lw[0] = s.w, lh[0] = s.h;
    for (int l = 1; l <= p.top; l++) lw[l] = (lw[l - 1] + 1) / 2, lh[l] = (lh[l - 1] + 1) / 2;
    if (pitch < lw[level]) return PAGK_E_ARG;
    const Layout<kLkMaxLevels> lay = lk_layout(lw, lh, p.top);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)pitch, lay.at<uint8_t>(ctx->buf[pagk_ctx::LK_PYR + slot].ptr, level - 1),
                                 (size_t)lw[level], (size_t)lw[level], (size_t)lh[level], hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PAGK_OK;
}

// ---- hipGraph capture of the per-frame work ---------------------------------------------------
// BASELINE configs[4] ("hipGraph-captured iterate"): a camera stream issues the same launches with the same
// device pointers every frame (new frame written into a fixed device buffer -> pyramid -> prediction ->
// tracking -> scoring), so they are recorded once and replayed with one hipGraphLaunch.
int pagk_graph_begin(pagk_ctx *ctx)
{
    if (!ctx || ctx->capturing) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    destroy_segs(ctx->cap_segs);
    batch_desc_free(ctx->cap_batch);
    ctx->cap_batch_used = 0;
    if (ctx->batch_seen) {   // a context that leads batched launches: the capture's own descriptor pairs (no allocation inside a capture)
        ctx->cap_batch.resize(pagk_ctx::kBatchPerCapture);
        for (auto &d : ctx->cap_batch)
            if (int ar = batch_desc_alloc(ctx, d)) {
                batch_desc_free(ctx->cap_batch);
                return ar;
            }
    }
    HIPCHK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    ctx->capturing = true;
    return PAGK_OK;
}

int pagk_graph_end(pagk_ctx *ctx, int32_t *graph_id)
{
    if (!ctx || !ctx->capturing || !graph_id) return PAGK_E_ARG;
    ctx->capturing = false;
    const bool carries_order = ctx->order.capture_ended();
    hipGraph_t g = nullptr;
    HIPCHK(ctx, hipStreamEndCapture(ctx->stream, &g));
    int id = -1;
    for (int k = 0; k < pagk_ctx::kGraphs; k++)
        if (!ctx->graph_execs[k]) {
            id = k;
            break;
        }
    if (id < 0 || !g) {
        if (g) (void)hipGraphDestroy(g);
        destroy_segs(ctx->cap_segs);
        batch_desc_free(ctx->cap_batch);
        snprintf(ctx->err, sizeof(ctx->err), id < 0 ? "all %d graph slots are in use" : "capture produced no graph (%d)", pagk_ctx::kGraphs);
        return PAGK_E_ARG;
    }
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        destroy_segs(ctx->cap_segs);
        batch_desc_free(ctx->cap_batch);
        snprintf(ctx->err, sizeof(ctx->err), "hipGraphInstantiate -> %s", hipGetErrorString(e));
        return PAGK_E_HIP;
    }
    ctx->graphs[id] = g;
    ctx->graph_execs[id] = ex;
    ctx->graph_order[id] = carries_order;
    ctx->pre_segs[id] = std::move(ctx->cap_segs);   // (empty for a capture without a live finisher: one graph, as before)
    ctx->cap_segs.clear();
    batch_desc_free(ctx->graph_batch[id]);
    ctx->graph_batch[id] = std::move(ctx->cap_batch);   // (unused reserved pairs go with it: freed with the graph)
    ctx->cap_batch.clear();
    ctx->cap_batch_used = 0;
    *graph_id = id;
    return PAGK_OK;
}

int pagk_graph_launch(pagk_ctx *ctx, int32_t graph_id)
{
    if (!ctx || ctx->capturing || graph_id < 0 || graph_id >= pagk_ctx::kGraphs || !ctx->graph_execs[graph_id]) return PAGK_E_ARG;
    // a graph that builds or reads the dispatch order binds the array to the stream it is replayed on; bound to another stream, whose
    // work the host has not waited for, the array could be rewritten under a reader: wait first (rare: a stream switch without a sync)
    if (ctx->graph_order[graph_id] && ctx->order.replay(ctx->stream)) HIPCHK(ctx, hipDeviceSynchronize());
    for (pagk_ctx::GraphSeg &sg : ctx->pre_segs[graph_id]) {
        if (sg.kind == pagk_ctx::GraphSeg::GRAPH) {
            HIPCHK(ctx, hipGraphLaunch(sg.ex, ctx->stream));
        } else if (sg.kind == pagk_ctx::GraphSeg::FINISHER) {
            // the live finisher beside the throughput kernel of the next segment: the fork of a direct launch
            HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->ev_fork, 0));
            void *kargs[] = {&sg.args};
            HIPCHK(ctx, hipLaunchKernel(sg.fn, dim3(sg.grid), dim3(kBlock), kargs, sg.lds, ctx->aux_stream));
            HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->aux_stream));
        } else {
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        }
    }
    HIPCHK(ctx, hipGraphLaunch(ctx->graph_execs[graph_id], ctx->stream));
    return PAGK_OK;
}

int pagk_graph_destroy(pagk_ctx *ctx, int32_t graph_id)
{
    if (!ctx || graph_id < 0 || graph_id >= pagk_ctx::kGraphs || !ctx->graph_execs[graph_id]) return PAGK_E_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->aux_stream));
    (void)hipGraphExecDestroy(ctx->graph_execs[graph_id]);
    (void)hipGraphDestroy(ctx->graphs[graph_id]);
    destroy_segs(ctx->pre_segs[graph_id]);
    batch_desc_free(ctx->graph_batch[graph_id]);
    ctx->graph_execs[graph_id] = nullptr;
    ctx->graphs[graph_id] = nullptr;
    ctx->graph_order[graph_id] = false;
    ctx->order.stream_idle(ctx->stream);
    bool alive = false;
    for (int k = 0; k < pagk_ctx::kGraphs; k++) alive = alive || ctx->graph_execs[k];
    if (!alive) ctx->order.graphs_gone();
    return lv_check(ctx);
}

// ---- geometry validation scoring ----------------------------------
int pagk_geometry_scores_device(pagk_ctx *ctx, const double *H21, const double *H12, const double *F21,
                                int32_t n, const float *d_pts1, const float *d_pts2, float sigma,
                                uint8_t *d_inliers_H, uint8_t *d_inliers_F, float *d_scores)
{
    if (!ctx || !H21 || !H12 || !F21 || n < 0 || !d_scores) return PAGK_E_ARG;
    if (n > 0 && (!d_pts1 || !d_pts2 || !d_inliers_H || !d_inliers_F)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ScoreArgs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 9; k++) a.H21[k] = H21[k], a.H12[k] = H12[k], a.F21[k] = F21[k];
    a.pts1 = d_pts1, a.pts2 = d_pts2, a.n = n, a.sigma = sigma;
    a.inl_H = d_inliers_H, a.inl_F = d_inliers_F, a.scores = d_scores;
    hipLaunchKernelGGL(k_geometry_scores, dim3(2), dim3(256), 0, ctx->stream, a);  // n == 0: scores = 0
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

int pagk_geometry_scores(pagk_ctx *ctx, const double *H21, const double *H12, const double *F21, int32_t n,
                         const float *pts1, const float *pts2, float sigma, uint8_t *inliers_H,
                         uint8_t *inliers_F, float *score_H, float *score_F)
{
    if (!ctx || !H21 || !H12 || !F21 || n < 0 || !score_H || !score_F) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_geometry_scores");
    if (n > 0 && (!pts1 || !pts2 || !inliers_H || !inliers_F)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)(n < 1 ? 1 : n);
    const size_t sizes[5] = {nn * 8, nn * 8, nn, nn, 256};   // pts1 | pts2 | inliers_H | inliers_F | scores
    float sc[2];
    Staged<5> s(ctx, sizes);
    int rc;
    if ((rc = s.open(&ctx->buf[pagk_ctx::SCORE], "the geometry scores' scratch")) || (rc = s.in(0, pts1, (size_t)n * 8)) ||
        (rc = s.in(1, pts2, (size_t)n * 8)))
        return rc;
    rc = pagk_geometry_scores_device(ctx, H21, H12, F21, n, s.at<float>(0), s.at<float>(1), sigma, s.at<uint8_t>(2),
                                     s.at<uint8_t>(3), s.at<float>(4));
    if (rc || (rc = s.out(2, inliers_H, (size_t)n)) || (rc = s.out(3, inliers_F, (size_t)n)) || (rc = s.out(4, sc, 8)) ||
        (rc = s.finish()))
        return rc;
    *score_H = sc[0];
    *score_F = sc[1];
    return PAGK_OK;
}

// src/gyro_aided_tracker.cpp:462-465: `float RH = ...; if (RH > 0.45)` compares in double.
int pagk_geometry_select(float score_H, float score_F)
{
    const float RH = score_H / (score_F + score_H);
    return RH > 0.45 ? 1 : 0;
}

int pagk_geometry_validation(pagk_ctx *ctx, const double *H21, const double *H12, const double *F21,
                             int32_t n, const float *pt_ref_un, const float *pt_predict_un,
                             uint8_t *status, float sigma, float *track_score)
{
    if (!ctx || !H21 || !H12 || !F21 || n < 0) return PAGK_E_ARG;
    if (n > 0 && (!pt_ref_un || !pt_predict_un || !status)) return PAGK_E_ARG;
    if (track_score) *track_score = 0;  // :447
    try {
    std::vector<int> idx;               // :433-440
    std::vector<float> p1, p2;
    for (int i = 0; i < n; i++)
        if (status[i]) {
            idx.push_back(i);
            p1.push_back(pt_ref_un[2 * i]), p1.push_back(pt_ref_un[2 * i + 1]);
            p2.push_back(pt_predict_un[2 * i]), p2.push_back(pt_predict_un[2 * i + 1]);
        }
    const int m = (int)idx.size();
    if (m <= 8) return 0;  // :445
    std::vector<uint8_t> inH((size_t)m), inF((size_t)m);
    float sH = 0, sF = 0;
    int rc = pagk_geometry_scores(ctx, H21, H12, F21, m, p1.data(), p2.data(), sigma, inH.data(), inF.data(), &sH, &sF);
    if (rc) return rc;
    const bool useH = pagk_geometry_select(sH, sF) != 0;  // :462-470
    const std::vector<uint8_t> &in = useH ? inH : inF;
    if (track_score) *track_score = useH ? sH : sF;
    int cnt_inlier = 0;
    for (int k = 0; k < m; k++) {  // :472-480
        if (!in[k])
            status[idx[k]] = 0;
        else
            cnt_inlier++;
    }
    return cnt_inlier;
    } catch (const std::bad_alloc &) {  // nothing crosses the C ABI
        return PAGK_E_NOMEM;
    }
}

// ---- the RANSAC fits on the device (pagk_fit_kernel.h) ----------------------------------------------------------
void pagk_fit_params_default(pagk_fit_params *p)
{
    if (!p) return;
    p->seed = 0;
    p->iters_H = 2000;  // findHomography's default maxIters
    p->iters_F = 1000;
    p->thresh_H = 3.0;  // src/gyro_aided_tracker.cpp:597
    p->thresh_F = 3.0;  // :691
    p->conf_H = 0.995;
    p->conf_F = 0.99;   // :691
}

namespace {

bool fit_params_ok(const pagk_fit_params *p)
{
    return p && p->iters_H >= 1 && p->iters_H <= PAGK_FIT_MAX_ITERS && p->iters_F >= 1 &&
           p->iters_F <= PAGK_FIT_MAX_ITERS && std::isfinite(p->thresh_H) && p->thresh_H > 0 &&
           std::isfinite(p->thresh_F) && p->thresh_F > 0 && p->conf_H > 0 && p->conf_H < 1 && p->conf_F > 0 &&
           p->conf_F < 1;
}

// the fit workspace: FitHdr | p1 | p2 | idx | hypothesis models | hypothesis counts | models | info | scores |
// inl_H | inl_F (the last three for the validation path)
struct FitWs {
    FitHdr *hdr;
    float *p1, *p2;
    int32_t *idx;
    double *hyp_models;
    int32_t *hyp_counts;
    double *models;
    int32_t *info;
    float *scores;
    uint8_t *inl_H, *inl_F;
};

// Room for n correspondences and `iters` hypotheses; grows only outside a capture and while no graph of this context
// is alive (its nodes point into the workspace).
int fit_workspace(pagk_ctx *ctx, int32_t n, int32_t iters, FitWs *w)
{
    // the layout for the largest n and the largest iters seen so far: it grows in both, and so do its bytes
    const int32_t n2 = n > ctx->fit_n ? n : ctx->fit_n, it2 = iters > ctx->fit_iters ? iters : ctx->fit_iters;
    const size_t nn = (size_t)(n2 < 1 ? 1 : n2), hh = (size_t)it2;
    const size_t sizes[11] = {sizeof(FitHdr), nn * 8, nn * 8, nn * 4, hh * 72, hh * 4, 27 * 8, kFitInfoWords * 4, 8, nn, nn};
    const Layout<11> lay(sizes);
    char hint[128];
    snprintf(hint, sizeof hint, "run the call once with at least %d correspondences and %d hypotheses before capturing", n, iters);
    int rc = reserve(ctx, ctx->buf[pagk_ctx::FIT], lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the geometry fit's workspace", hint);
    if (rc) return rc;
    ctx->fit_n = n2, ctx->fit_iters = it2;
    void *b = ctx->buf[pagk_ctx::FIT].ptr;
    *w = FitWs{lay.at<FitHdr>(b, 0), lay.at<float>(b, 1), lay.at<float>(b, 2), lay.at<int32_t>(b, 3), lay.at<double>(b, 4),
               lay.at<int32_t>(b, 5), lay.at<double>(b, 6), lay.at<int32_t>(b, 7), lay.at<float>(b, 8), lay.at<uint8_t>(b, 9),
               lay.at<uint8_t>(b, 10)};   // (the workspace's parts in the order of FitWs' members)
    return PAGK_OK;
}

// the arguments of k_fit_hyp and k_fit_refit on workspace w (models, info: the caller's or the workspace's)
FitArgs fit_args(const pagk_fit_params *p, const FitWs &w, double *models, int32_t *info, int32_t *d_hyp_counts, uint8_t *d_mask_H,
                 uint8_t *d_mask_F)
{
    FitArgs a;
    memset(&a, 0, sizeof a);
    a.p1 = w.p1, a.p2 = w.p2, a.idx = w.idx, a.hdr = w.hdr, a.hyp_models = w.hyp_models;
    a.hyp_counts = d_hyp_counts ? d_hyp_counts : w.hyp_counts;
    a.models = models, a.info = info, a.mask_H = d_mask_H, a.mask_F = d_mask_F;
    a.seed = p->seed;
    a.iters[0] = p->iters_H, a.iters[1] = p->iters_F;
    a.nblk_H = (p->iters_H + kFitHypPerBlock - 1) / kFitHypPerBlock;
    a.t2[0] = p->thresh_H * p->thresh_H, a.t2[1] = p->thresh_F * p->thresh_F;
    a.conf[0] = p->conf_H, a.conf[1] = p->conf_F;
    return a;
}
// ... and the workgroups of k_fit_hyp
int fit_hyp_blocks(const pagk_fit_params *p)
{
    return (p->iters_H + kFitHypPerBlock - 1) / kFitHypPerBlock + (p->iters_F + kFitHypPerBlock - 1) / kFitHypPerBlock;
}

// compaction + hypotheses + refit on the context stream
int fit_launch(pagk_ctx *ctx, const pagk_fit_params *p, int32_t n, const float *d_pts1, const float *d_pts2,
               const uint8_t *d_status, double *d_models, uint8_t *d_mask_H, uint8_t *d_mask_F, int32_t *d_info,
               int32_t *d_hyp_counts, FitWs *w)
{
    int rc = fit_workspace(ctx, n, p->iters_H + p->iters_F, w);
    if (rc) return rc;
    double *models = d_models ? d_models : w->models;
    int32_t *info = d_info ? d_info : w->info;
    hipLaunchKernelGGL(k_fit_compact, dim3(1), dim3(1024), 0, ctx->stream, n, d_pts1, d_pts2, d_status, w->p1, w->p2,
                       w->idx, w->hdr, models, info, d_mask_H, d_mask_F);
    HIPCHK(ctx, hipGetLastError());
    const FitArgs a = fit_args(p, *w, models, info, d_hyp_counts, d_mask_H, d_mask_F);
    hipLaunchKernelGGL(k_fit_hyp, dim3(fit_hyp_blocks(p)), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fit_refit, dim3(2), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    w->models = models, w->info = info;
    return PAGK_OK;
}

}  // namespace

int pagk_geometry_fit_device(pagk_ctx *ctx, const pagk_fit_params *params, int32_t n, const float *d_pts1,
                             const float *d_pts2, const uint8_t *d_status, double *d_models, uint8_t *d_mask_H,
                             uint8_t *d_mask_F, int32_t *d_info, int32_t *d_hyp_counts)
{
    if (!ctx || !fit_params_ok(params) || n < 0 || !d_models || !d_info) return PAGK_E_ARG;
    if (n > 0 && (!d_pts1 || !d_pts2)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FitWs w;
    return fit_launch(ctx, params, n, d_pts1, d_pts2, d_status, d_models, d_mask_H, d_mask_F, d_info, d_hyp_counts, &w);
}

int pagk_geometry_fit(pagk_ctx *ctx, const pagk_fit_params *params, int32_t n, const float *pts1, const float *pts2,
                      const uint8_t *status, double *models, uint8_t *mask_H, uint8_t *mask_F, int32_t *info,
                      int32_t *hyp_counts)
{
    if (!ctx || !fit_params_ok(params) || n < 0 || !models || !info) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_geometry_fit");
    if (n > 0 && (!pts1 || !pts2)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)(n < 1 ? 1 : n), hh = (size_t)params->iters_H + (size_t)params->iters_F;
    // pts1 | pts2 | status | mask_H | mask_F | hyp_counts | models | info
    const size_t sizes[8] = {nn * 8, nn * 8, nn, nn, nn, hh * 4, 256, 256};
    Staged<8> s(ctx, sizes);
    int rc;
    if ((rc = s.open(&ctx->buf[pagk_ctx::FITIO], "the host-buffer fit's scratch")) || (rc = s.in(0, pts1, (size_t)n * 8)) ||
        (rc = s.in(1, pts2, (size_t)n * 8)) || (rc = s.in(2, status, (size_t)n)))
        return rc;
    FitWs w;
    rc = fit_launch(ctx, params, n, s.at<float>(0), s.at<float>(1), status ? s.at<uint8_t>(2) : nullptr, s.at<double>(6),
                    s.at<uint8_t>(3), s.at<uint8_t>(4), s.at<int32_t>(7), s.at<int32_t>(5), &w);
    if (rc || (rc = s.out(6, models, 27 * sizeof(double))) || (rc = s.out(7, info, PAGK_FIT_INFO_WORDS * sizeof(int32_t))) ||
        (rc = s.out(3, mask_H, (size_t)n)) || (rc = s.out(4, mask_F, (size_t)n)) || (rc = s.out(5, hyp_counts, hh * 4)))
        return rc;
    return s.finish();
}

int pagk_geometry_validation_device(pagk_ctx *ctx, const pagk_fit_params *params, int32_t n, const float *d_pt_ref_un,
                                    const float *d_pt_predict_un, uint8_t *d_status, float sigma, int32_t *d_cnt,
                                    float *d_score)
{
    if (!ctx || !fit_params_ok(params) || n < 0 || !d_cnt || !d_score) return PAGK_E_ARG;
    if (n > 0 && (!d_pt_ref_un || !d_pt_predict_un || !d_status)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FitWs w;
    int rc = fit_launch(ctx, params, n, d_pt_ref_un, d_pt_predict_un, d_status, nullptr, nullptr, nullptr, nullptr,
                        nullptr, &w);
    if (rc) return rc;
    hipLaunchKernelGGL(k_geometry_scores_fit, dim3(2), dim3(256), 0, ctx->stream, w.models, w.info, &w.hdr->m, w.p1,
                       w.p2, sigma, w.inl_H, w.inl_F, w.scores);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_fit_select, dim3(1), dim3(1024), 0, ctx->stream, w.hdr, w.info, w.scores, w.inl_H, w.inl_F,
                       w.idx, d_status, d_cnt, d_score);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

int pagk_geometry_validation_fit(pagk_ctx *ctx, const pagk_fit_params *params, int32_t n, const float *pt_ref_un,
                                 const float *pt_predict_un, uint8_t *status, float sigma, float *track_score)
{
    if (!ctx || !fit_params_ok(params) || n < 0) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_geometry_validation_fit");
    if (n > 0 && (!pt_ref_un || !pt_predict_un || !status)) return PAGK_E_ARG;
    if (track_score) *track_score = 0;  // :447
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)(n < 1 ? 1 : n);
    const size_t sizes[5] = {nn * 8, nn * 8, nn, 256, 256};   // pt_ref_un | pt_predict_un | status | count | score
    int32_t cnt = 0;
    float sc = 0;
    Staged<5> s(ctx, sizes);
    int rc;
    if ((rc = s.open(&ctx->buf[pagk_ctx::FITIO], "the host-buffer fit's scratch")) || (rc = s.in(0, pt_ref_un, (size_t)n * 8)) ||
        (rc = s.in(1, pt_predict_un, (size_t)n * 8)) || (rc = s.in(2, status, (size_t)n)))
        return rc;
    rc = pagk_geometry_validation_device(ctx, params, n, s.at<float>(0), s.at<float>(1), s.at<uint8_t>(2), sigma,
                                         s.at<int32_t>(3), s.at<float>(4));
    if (rc || (rc = s.out(2, status, (size_t)n)) || (rc = s.out(3, &cnt, 4)) || (rc = s.out(4, &sc, 4)) || (rc = s.finish()))
        return rc;
    if (track_score) *track_score = sc;
    return cnt;
}

// ---- the two-view pose on the device (pagk_pose_kernel.h) ---------------------------------------------------------
void pagk_pose_params_default(pagk_pose_params *p)
{
    if (!p) return;
    p->seed = 0;
    p->iters_E = 1000;
    p->reserved = 0;
    p->thresh_E = 1.0;    // findEssentialMat's default threshold
    p->conf_E = 0.999;    // ... and prob
    p->max_depth = 50.0;  // recoverPose's distance threshold
    pagk_fit_params_default(&p->fit);
}

int pagk_pose_params_check(const pagk_pose_params *p)
{
    const bool ok = p && p->iters_E >= 1 && p->iters_E <= PAGK_FIT_MAX_ITERS && std::isfinite(p->thresh_E) && p->thresh_E > 0 &&
                    p->conf_E > 0 && p->conf_E < 1 && std::isfinite(p->max_depth) && p->max_depth > 0 && fit_params_ok(&p->fit);
    return ok ? PAGK_OK : PAGK_E_ARG;
}

namespace {

bool pose_camera_ok(double f, double cx, double cy) { return std::isfinite(f) && f > 0 && std::isfinite(cx) && std::isfinite(cy); }

// the pose workspace: PoseHdr | normalised correspondences | the hypotheses' best candidates | E R t | info | and, for
// pagk_pose_from_matches_device, the gathered pts1 | pts2 | status
struct PoseWs {
    PoseHdr *hdr;
    double *qn, *hyp_E, *pose;
    int32_t *info;
    float *g1, *g2;
    uint8_t *gst;
};

// Room for n correspondences and `iters` hypotheses; grows like the fit's workspace, outside a capture only.
int pose_workspace(pagk_ctx *ctx, int32_t n, int32_t iters, PoseWs *w)
{
    const int32_t n2 = n > ctx->pose_n ? n : ctx->pose_n, it2 = iters > ctx->pose_iters ? iters : ctx->pose_iters;
    const size_t nn = (size_t)(n2 < 1 ? 1 : n2), hh = (size_t)it2;
    const size_t sizes[8] = {sizeof(PoseHdr), nn * 32, hh * 72, 21 * 8, kPoseInfoWords * 4, nn * 8, nn * 8, nn};
    const Layout<8> lay(sizes);
    char hint[128];
    snprintf(hint, sizeof hint, "run the call once with at least %d correspondences and %d hypotheses before capturing", n, iters);
    int rc = reserve(ctx, ctx->buf[pagk_ctx::POSE], lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the pose estimation's workspace", hint);
    if (rc) return rc;
    ctx->pose_n = n2, ctx->pose_iters = it2;
    void *b = ctx->buf[pagk_ctx::POSE].ptr;
    *w = PoseWs{lay.at<PoseHdr>(b, 0), lay.at<double>(b, 1), lay.at<double>(b, 2), lay.at<double>(b, 3), lay.at<int32_t>(b, 4),
                lay.at<float>(b, 5), lay.at<float>(b, 6), lay.at<uint8_t>(b, 7)};   // (in the order of PoseWs' members)
    return PAGK_OK;
}

// the fits of H and F (they compact the correspondences), then normalisation + hypotheses + recovery on the context stream
int pose_launch(pagk_ctx *ctx, const pagk_pose_params *p, double f, double cx, double cy, int32_t n, const float *d_pts1,
                const float *d_pts2, const uint8_t *d_status, double *d_models, double *d_pose, uint8_t *d_mask_H,
                uint8_t *d_mask_F, uint8_t *d_mask_E, uint8_t *d_mask_pose, int32_t *d_fit_info, int32_t *d_pose_info,
                int32_t *d_cand_counts, const PoseWs &w)
{
    FitWs fw;
    int rc = fit_launch(ctx, &p->fit, n, d_pts1, d_pts2, d_status, d_models, d_mask_H, d_mask_F, d_fit_info, nullptr, &fw);
    if (rc) return rc;
    PoseArgs a;
    memset(&a, 0, sizeof a);
    a.p1 = fw.p1, a.p2 = fw.p2, a.idx = fw.idx, a.fit_hdr = fw.hdr, a.hdr = w.hdr, a.qn = w.qn, a.hyp_E = w.hyp_E;
    a.cand_counts = d_cand_counts, a.pose = d_pose, a.info = d_pose_info, a.mask_E = d_mask_E, a.mask_pose = d_mask_pose;
    a.seed = p->seed, a.n = n, a.iters = p->iters_E;
    a.f = f, a.cx = cx, a.cy = cy;
    const double tn = p->thresh_E / f;
    a.t2 = tn * tn, a.conf = p->conf_E, a.max_depth = p->max_depth;
    hipLaunchKernelGGL(k_pose_prep, dim3(n > 0 ? (n + 255) / 256 : 1), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pose_hyp, dim3((p->iters_E + kPoseHypPerBlock - 1) / kPoseHypPerBlock), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pose_recover, dim3(1), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

}  // namespace

int pagk_pose_2d2d_device(pagk_ctx *ctx, const pagk_pose_params *params, double f, double cx, double cy, int32_t n,
                          const float *d_pts1, const float *d_pts2, const uint8_t *d_status, double *d_models, double *d_pose,
                          uint8_t *d_mask_H, uint8_t *d_mask_F, uint8_t *d_mask_E, uint8_t *d_mask_pose, int32_t *d_fit_info,
                          int32_t *d_pose_info, int32_t *d_cand_counts)
{
    if (!ctx || pagk_pose_params_check(params) || !pose_camera_ok(f, cx, cy) || n < 0) return PAGK_E_ARG;
    if (!d_models || !d_pose || !d_fit_info || !d_pose_info || (n > 0 && (!d_pts1 || !d_pts2))) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PoseWs w;
    int rc = pose_workspace(ctx, n, params->iters_E, &w);
    if (rc) return rc;
    return pose_launch(ctx, params, f, cx, cy, n, d_pts1, d_pts2, d_status, d_models, d_pose, d_mask_H, d_mask_F, d_mask_E,
                       d_mask_pose, d_fit_info, d_pose_info, d_cand_counts, w);
}

int pagk_pose_from_matches_device(pagk_ctx *ctx, const pagk_pose_params *params, double f, double cx, double cy, int32_t cap_q,
                                  const float *d_kp_ref, const int32_t *d_nq, int32_t cap_t, const float *d_kp_cur,
                                  const int32_t *d_nt, const int32_t *d_train_idx, const uint8_t *d_keep, double *d_models,
                                  double *d_pose, uint8_t *d_mask_H, uint8_t *d_mask_F, uint8_t *d_mask_E, uint8_t *d_mask_pose,
                                  int32_t *d_fit_info, int32_t *d_pose_info)
{
    if (!ctx || pagk_pose_params_check(params) || !pose_camera_ok(f, cx, cy) || cap_q < 1 || cap_t < 1) return PAGK_E_ARG;
    if (!d_kp_ref || !d_nq || !d_kp_cur || !d_nt || !d_train_idx || !d_keep || !d_models || !d_pose || !d_fit_info || !d_pose_info)
        return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PoseWs w;
    int rc = pose_workspace(ctx, cap_q, params->iters_E, &w);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pose_gather, dim3((cap_q + 255) / 256), dim3(256), 0, ctx->stream, cap_q, d_kp_ref, d_nq, cap_t, d_kp_cur,
                       d_nt, d_train_idx, d_keep, w.g1, w.g2, w.gst);
    HIPCHK(ctx, hipGetLastError());
    return pose_launch(ctx, params, f, cx, cy, cap_q, w.g1, w.g2, w.gst, d_models, d_pose, d_mask_H, d_mask_F, d_mask_E,
                       d_mask_pose, d_fit_info, d_pose_info, nullptr, w);
}

int pagk_pose_2d2d(pagk_ctx *ctx, const pagk_pose_params *params, double f, double cx, double cy, int32_t n, const float *pts1,
                   const float *pts2, const uint8_t *status, double *models, double *pose, uint8_t *mask_H, uint8_t *mask_F,
                   uint8_t *mask_E, uint8_t *mask_pose, int32_t *fit_info, int32_t *pose_info, int32_t *cand_counts)
{
    if (!ctx || pagk_pose_params_check(params) || !pose_camera_ok(f, cx, cy) || n < 0) return PAGK_E_ARG;
    if (!models || !pose || !fit_info || !pose_info || (n > 0 && (!pts1 || !pts2))) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_pose_2d2d");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)(n < 1 ? 1 : n), cc = (size_t)params->iters_E * 10 * sizeof(int32_t);
    // pts1 | pts2 | status | mask_H | mask_F | mask_E | mask_pose | models | pose | fit_info | pose_info | cand_counts
    const size_t sizes[12] = {nn * 8, nn * 8, nn, nn, nn, nn, nn, 27 * 8, 21 * 8, 256, 256, cand_counts ? cc : 4};
    Staged<12> s(ctx, sizes);
    int rc;
    if ((rc = s.open(&ctx->buf[pagk_ctx::POSEIO], "the host-buffer pose estimation's scratch")) ||
        (rc = s.in(0, pts1, (size_t)n * 8)) || (rc = s.in(1, pts2, (size_t)n * 8)) || (rc = s.in(2, status, (size_t)n)))
        return rc;
    rc = pagk_pose_2d2d_device(ctx, params, f, cx, cy, n, s.at<float>(0), s.at<float>(1), status ? s.at<uint8_t>(2) : nullptr,
                               s.at<double>(7), s.at<double>(8), s.at<uint8_t>(3), s.at<uint8_t>(4), s.at<uint8_t>(5),
                               s.at<uint8_t>(6), s.at<int32_t>(9), s.at<int32_t>(10), cand_counts ? s.at<int32_t>(11) : nullptr);
    if (rc || (rc = s.out(7, models, 27 * sizeof(double))) || (rc = s.out(8, pose, 21 * sizeof(double))) ||
        (rc = s.out(9, fit_info, PAGK_FIT_INFO_WORDS * sizeof(int32_t))) ||
        (rc = s.out(10, pose_info, PAGK_POSE_INFO_WORDS * sizeof(int32_t))) || (rc = s.out(3, mask_H, (size_t)n)) ||
        (rc = s.out(4, mask_F, (size_t)n)) || (rc = s.out(5, mask_E, (size_t)n)) || (rc = s.out(6, mask_pose, (size_t)n)) ||
        (rc = s.out(11, cand_counts, cc)))
        return rc;
    return s.finish();
}

// ---- NCC nearest-neighbour matching ---------------------------------
static int near_neighbors_launch(pagk_ctx *ctx, const FrameSlot &sr, const FrameSlot &sc, int32_t half_patch, int32_t n,
                                 const float *d_keys_ref, const float *d_pt_predict_un, const uint8_t *d_status,
                                 const float *d_affine, int32_t m, const float *d_keys_cur, const float *d_keys_cur_un,
                                 int32_t level, float radius_unit, int32_t use_ncc, int32_t pairs, int32_t cap,
                                 int32_t *d_count, int32_t *d_nbr_idx, float *d_nbr_dist, float *d_nbr_ncc,
                                 const int32_t *d_gate = nullptr, int32_t gate_below = 0, const int32_t *d_m = nullptr)
{
    NeighborArgs a;
    memset(&a, 0, sizeof a);
    fill_level(a.ref0, sr, 0);
    fill_level(a.cur0, sc, 0);
    a.pad_ref = sr.pad0;
    a.pad_cur = sc.pad0;
    a.half = half_patch, a.n = n, a.m = m, a.cap = cap, a.level = level, a.use_ncc = use_ncc, a.pairs = pairs;
    a.radius = (float)level * radius_unit;  // src/gyro_aided_tracker.cpp:811  int * float
    a.keys_ref = d_keys_ref, a.pt_pred = d_pt_predict_un, a.affine = d_affine, a.status = d_status;
    a.keys_cur = d_keys_cur, a.keys_cur_un = d_keys_cur_un;
    a.count = d_count, a.nbr_idx = d_nbr_idx, a.nbr_dist = d_nbr_dist, a.nbr_ncc = d_nbr_ncc;
    a.gate = d_gate, a.gate_below = gate_below, a.d_m = d_m;
    if (n <= 0) return PAGK_OK;
    const int P = (2 * half_patch + 1) * (2 * half_patch + 1);
    const int nr = (P + 255) / 256, tail = P % 32;
    const size_t lds = neighbor_lds_bytes(half_patch, cap);
    if (lds > 64 * 1024) {
        snprintf(ctx->err, sizeof(ctx->err), "neighbour capacity %d needs %zu bytes of LDS (limit 64 KiB)", cap, lds);
        return PAGK_E_ARG;
    }
    auto launch = [&](auto kern) -> hipError_t {
        hipLaunchKernelGGL(kern, dim3(n), dim3(256), lds, ctx->stream, a);
        return hipGetLastError();
    };
    hipError_t e = hipErrorInvalidValue;
    switch (nr * 100 + tail) {  // (NR, TAIL) as for k_track_block
        case 101: e = launch(k_near_neighbors<1, 1>); break;
        case 109: e = launch(k_near_neighbors<1, 9>); break;
        case 117: e = launch(k_near_neighbors<1, 17>); break;
        case 125: e = launch(k_near_neighbors<1, 25>); break;
        case 201: e = launch(k_near_neighbors<2, 1>); break;
        case 209: e = launch(k_near_neighbors<2, 9>); break;
        case 225: e = launch(k_near_neighbors<2, 25>); break;
        case 317: e = launch(k_near_neighbors<3, 17>); break;
        case 325: e = launch(k_near_neighbors<3, 25>); break;
        case 409: e = launch(k_near_neighbors<4, 9>); break;
        case 401: e = launch(k_near_neighbors<4, 1>); break;
        default: break;
    }
    HIPCHK(ctx, e);
    return PAGK_OK;
}

int pagk_near_neighbors_device(pagk_ctx *ctx, int32_t slot_ref, int32_t slot_cur, int32_t half_patch, int32_t n,
                               const float *d_keys_ref, const float *d_pt_predict_un, const uint8_t *d_status,
                               const float *d_affine, int32_t m, const float *d_keys_cur, const float *d_keys_cur_un,
                               int32_t level, float radius_unit, int32_t use_ncc, int32_t cap, int32_t *d_count,
                               int32_t *d_nbr_idx, float *d_nbr_dist, float *d_nbr_ncc)
{
    if (!ctx || slot_ref < 0 || slot_ref >= kUserSlots || slot_cur < 0 || slot_cur >= kUserSlots) return PAGK_E_ARG;
    if (half_patch < 1 || half_patch > PAGK_MAX_HALF_PATCH || n < 0 || m < 0 || cap < 1 || level < 0) return PAGK_E_ARG;
    if (n > 0 && (!d_keys_ref || !d_pt_predict_un || !d_status || !d_count || !d_nbr_idx || !d_nbr_dist || !d_nbr_ncc))
        return PAGK_E_ARG;
    if (n > 0 && m > 0 && (!d_keys_cur || !d_keys_cur_un)) return PAGK_E_ARG;
    const FrameSlot &sr = ctx->slots[slot_ref], &sc = ctx->slots[slot_cur];
    if (!sr.valid || !sc.valid) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return near_neighbors_launch(ctx, sr, sc, half_patch, n, d_keys_ref, d_pt_predict_un, d_status, d_affine, m, d_keys_cur,
                                 d_keys_cur_un, level, radius_unit, use_ncc, 0, cap, d_count, d_nbr_idx, d_nbr_dist,
                                 d_nbr_ncc);
}

// host-buffer forms: both frames go through the scratch slots (level 0 only), the per-feature arrays through one
// device block; synchronous
static int neighbors_host(pagk_ctx *ctx, const pagk_image *ref, const pagk_image *cur, int32_t half_patch, int32_t n,
                          const float *keys_ref, const float *pt_predict_un, const uint8_t *status, const float *affine,
                          int32_t m, const float *keys_cur, const float *keys_cur_un, int32_t level, float radius_unit,
                          int32_t use_ncc, int32_t pairs, int32_t cap, int32_t *count, int32_t *nbr_idx, float *nbr_dist,
                          float *nbr_ncc)
{
    int rc;
    if ((rc = check_image(ref)) || (rc = check_image(cur))) return rc;
    if ((rc = frame_upload_any(ctx, 4, ref, 1)) || (rc = frame_upload_any(ctx, 5, cur, 1))) return rc;
    const size_t nn = (size_t)(n < 1 ? 1 : n), mm = (size_t)(m < 1 ? 1 : m), cc = (size_t)cap;
    // keys_ref | pt_predict_un | status | affine | keys_cur | keys_cur_un | count | nbr_idx | nbr_dist | nbr_ncc
    const size_t sizes[10] = {nn * 8, nn * 8, nn, nn * 16, mm * 8, mm * 8, nn * 4, nn * cc * 4, nn * cc * 4, nn * cc * 4};
    const size_t fn = (size_t)n, fm = (size_t)m, list = fn * cc * 4;   // what is copied: the features, not the padded parts
    Staged<10> s(ctx, sizes);
    if ((rc = s.open(&ctx->buf[pagk_ctx::SCORE], "the neighbour search's scratch")) || (rc = s.in(0, keys_ref, fn * 8)) ||
        (rc = s.in(1, pt_predict_un, fn * 8)) || (rc = s.in(2, status, fn)) || (rc = s.in(3, affine, fn * 16)) ||
        (rc = s.in(6, count, fn * 4)) || (rc = s.in(4, keys_cur, fm * 8)) || (rc = s.in(5, keys_cur_un, fm * 8)))
        return rc;
    // the lists of skipped features (status 0, or already filled at a smaller radius) keep the caller's content
    if (!pairs && ((rc = s.in(7, nbr_idx, list)) || (rc = s.in(8, nbr_dist, list)) || (rc = s.in(9, nbr_ncc, list)))) return rc;
    rc = near_neighbors_launch(ctx, ctx->slots[4], ctx->slots[5], half_patch, n, s.at<float>(0), s.at<float>(1), s.at<uint8_t>(2),
                               affine ? s.at<float>(3) : nullptr, m, s.at<float>(4), s.at<float>(5), level, radius_unit, use_ncc,
                               pairs, cap, s.at<int32_t>(6), s.at<int32_t>(7), s.at<float>(8), s.at<float>(9));
    if (rc || (rc = s.out(6, count, fn * 4)) || (rc = s.out(7, nbr_idx, list)) || (rc = s.out(8, nbr_dist, list)) ||
        (rc = s.out(9, nbr_ncc, list)))
        return rc;
    return s.finish();
}

int pagk_find_near_neighbors(pagk_ctx *ctx, const pagk_image *ref, const pagk_image *cur, int32_t half_patch, int32_t n,
                             const float *keys_ref, const float *pt_predict_un, const uint8_t *status,
                             const float *affine, int32_t m, const float *keys_cur, const float *keys_cur_un,
                             int32_t level, float radius_unit, int32_t use_ncc, int32_t cap, int32_t *count,
                             int32_t *nbr_idx, float *nbr_dist, float *nbr_ncc)
{
    if (!ctx) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_find_near_neighbors");
    if (half_patch < 1 || half_patch > PAGK_MAX_HALF_PATCH || n < 0 || m < 0 || cap < 1 || level < 0) return PAGK_E_ARG;
    if (n > 0 && (!keys_ref || !pt_predict_un || !status || !count || !nbr_idx || !nbr_dist || !nbr_ncc)) return PAGK_E_ARG;
    if (n > 0 && m > 0 && (!keys_cur || !keys_cur_un)) return PAGK_E_ARG;
    int rc = neighbors_host(ctx, ref, cur, half_patch, n, keys_ref, pt_predict_un, status, affine, m, keys_cur, keys_cur_un,
                            level, radius_unit, use_ncc, 0, cap, count, nbr_idx, nbr_dist, nbr_ncc);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (count[i] > cap) {
            snprintf(ctx->err, sizeof(ctx->err), "feature %d has %d neighbours, capacity is %d", i, count[i], cap);
            return PAGK_E_CAPACITY;
        }
    return PAGK_OK;
}

int pagk_ncc_free(pagk_ctx *ctx, const pagk_image *ref, const pagk_image *cur, int32_t half_patch, int32_t n,
                  const float *pt_ref, const float *pt_cur, const float *affine, float *ncc)
{
    if (!ctx) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_ncc_free");
    if (half_patch < 1 || half_patch > PAGK_MAX_HALF_PATCH || n < 0) return PAGK_E_ARG;
    if (n > 0 && (!pt_ref || !pt_cur || !ncc)) return PAGK_E_ARG;
    if (n == 0) return PAGK_OK;
    try {
        std::vector<uint8_t> st((size_t)n, 1);
        std::vector<int32_t> cnt((size_t)n, 0);
        // pairs mode: feature i's only candidate is point i of pt_cur; capacity 1
        return neighbors_host(ctx, ref, cur, half_patch, n, pt_ref, pt_ref, st.data(), affine, n, pt_cur, pt_cur, 0, 0.0f, 1, 1,
                              1, cnt.data(), nullptr, nullptr, ncc);
    } catch (const std::bad_alloc &) {
        return PAGK_E_NOMEM;
    }
}

// ---- diagnostics: the solve's arithmetic on arbitrary operands (pagk_selftest_kernel.h) --------------------------

int pagk_selftest_divide(pagk_ctx *ctx, int32_t n, const double *num, const double *den, double *q_plain,
                         double *q_prepared, double *root, double *root_lean)
{
    if (!ctx || n < 0) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_divide");
    if (n == 0) return PAGK_OK;
    if (!num || !den || !q_plain || !q_prepared || !root || !root_lean) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)n * sizeof(double);
    const size_t sizes[6] = {nb, nb, nb, nb, nb, nb};   // num | den | q_plain | q_prepared | root | root_lean
    Staged<6> s(ctx, sizes);
    int rc;
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, num, nb)) || (rc = s.in(1, den, nb))) return rc;
    hipLaunchKernelGGL(k_selftest_divide, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, s.at<double>(0), s.at<double>(1),
                       s.at<double>(2), s.at<double>(3), s.at<double>(4), s.at<double>(5));
    HIPCHK(ctx, hipGetLastError());
    if ((rc = s.out(2, q_plain, nb)) || (rc = s.out(3, q_prepared, nb)) || (rc = s.out(4, root, nb)) || (rc = s.out(5, root_lean, nb)))
        return rc;
    return s.finish();
}

int pagk_selftest_fit_samples(pagk_ctx *ctx, uint64_t seed, int32_t model, int32_t m, int32_t first, int32_t count,
                              int32_t *idx)
{
    if (!ctx || model < 0 || model > 2 || m < 1 || first < 0 || count < 0 || !idx) return PAGK_E_ARG;
    if ((int64_t)first + count > (int64_t)PAGK_FIT_MAX_ITERS) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_fit_samples");
    if (count == 0) return PAGK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t sizes[1] = {(size_t)count * (model == 2 ? 5 : model ? 8 : 4) * sizeof(int32_t)};
    Staged<1> s(ctx, sizes);
    int rc = s.open(nullptr, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fit_samples, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, (unsigned long long)seed, model,
                       m, first, count, s.at<int32_t>(0));
    HIPCHK(ctx, hipGetLastError());
    if ((rc = s.out(0, idx, sizes[0]))) return rc;
    return s.finish();
}

int pagk_selftest_repeat_sum(pagk_ctx *ctx, int32_t n, const float *c, int32_t count, double *closed, double *loop)
{
    if (!ctx || n < 0 || count <= 57 || count > 480) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_repeat_sum");
    if (n == 0) return PAGK_OK;
    if (!c || !closed || !loop) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n;
    const size_t sizes[3] = {nn * sizeof(double), nn * sizeof(double), nn * sizeof(float)};   // closed | loop | c
    Staged<3> s(ctx, sizes);
    int rc;
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(2, c, sizes[2]))) return rc;
    hipLaunchKernelGGL(k_selftest_repeat_sum, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, s.at<float>(2), count,
                       s.at<double>(0), s.at<double>(1));
    HIPCHK(ctx, hipGetLastError());
    if ((rc = s.out(0, closed, sizes[0])) || (rc = s.out(1, loop, sizes[1]))) return rc;
    return s.finish();
}

int pagk_selftest_solve(pagk_ctx *ctx, int32_t n, const double *H, const double *b, uint32_t solver_variant,
                        double *x_serial, double *norm_serial, double *x_lanes, double *nsq_lanes)
{
    if (!ctx || n < 0) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_solve");
    if (solver_variant & ~(SV_LOWER_SEQ | SV_UPPER_TREE | SV_NORM_SEQ | SV_LLT_RECIP | SV_PIVOT_TREE)) return PAGK_E_ARG;
    if (n == 0) return PAGK_OK;
    if (!H || !b || !x_serial || !norm_serial || !x_lanes || !nsq_lanes) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)n * sizeof(double);
    const size_t sizes[6] = {16 * nb, 4 * nb, 4 * nb, nb, 4 * nb, nb};   // H | b | x_serial | norm_serial | x_lanes | nsq_lanes
    Staged<6> s(ctx, sizes);
    int rc;
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, H, sizes[0])) || (rc = s.in(1, b, sizes[1]))) return rc;
    hipLaunchKernelGGL(k_selftest_solve, dim3((n + 15) / 16), dim3(64), 0, ctx->stream, n, s.at<double>(0), s.at<double>(1),
                       solver_variant, s.at<double>(2), s.at<double>(3), s.at<double>(4), s.at<double>(5));
    HIPCHK(ctx, hipGetLastError());
    if ((rc = s.out(2, x_serial, sizes[2])) || (rc = s.out(3, norm_serial, sizes[3])) || (rc = s.out(4, x_lanes, sizes[4])) ||
        (rc = s.out(5, nsq_lanes, sizes[5])))
        return rc;
    return s.finish();
}

// The sampler of pagk_device.h on level `level` of a built slot.  A clamp-free sample reads the quad at (int(y), int(x)) with
// no test at all, so every coordinate of modes 1 and 3 is held against the domain first -- written so that NaN fails.
int pagk_selftest_sample(pagk_ctx *ctx, int32_t slot, int32_t level, int32_t mode, int32_t n, const float *xy, float *out)
{
    if (!ctx || slot < 0 || slot >= kUserSlots || mode < 0 || mode > 3 || n < 0) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_selftest_sample");
    const FrameSlot &s = ctx->slots[slot];
    if (!s.valid || level < 0 || level >= s.L) return PAGK_E_ARG;
    if (n == 0) return PAGK_OK;
    if (!xy || !out) return PAGK_E_ARG;
    DevLevel lv;
    fill_level(lv, s, level);
    const bool clamp = mode == 0 || mode == 2, five = mode >= 2;
    if (!clamp) {
        const float lo = five ? 1.0f : 0.0f;
        const float hx = (float)(lv.cols - (five ? 2 : 1)), hy = (float)(lv.rows - (five ? 2 : 1));
        for (int32_t i = 0; i < n; i++) {
            const float x = xy[2 * (size_t)i], y = xy[2 * (size_t)i + 1];
            if (!(x >= lo && x < hx && y >= lo && y < hy)) return PAGK_E_ARG;
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, per = five ? 5 : 1;
    const size_t sizes[2] = {2 * nn * sizeof(float), nn * per * sizeof(float)};   // xy | out
    Staged<2> st(ctx, sizes);
    int rc;
    if ((rc = st.open(nullptr, nullptr)) || (rc = st.in(0, xy, sizes[0]))) return rc;
    float *d_xy = st.at<float>(0), *d_out = st.at<float>(1);
    const dim3 grd((n + 255) / 256), blk(256);
    switch (mode) {
    case 0: hipLaunchKernelGGL((k_selftest_sample<true, false>), grd, blk, 0, ctx->stream, lv, n, d_xy, d_out); break;
    case 1: hipLaunchKernelGGL((k_selftest_sample<false, false>), grd, blk, 0, ctx->stream, lv, n, d_xy, d_out); break;
    case 2: hipLaunchKernelGGL((k_selftest_sample<true, true>), grd, blk, 0, ctx->stream, lv, n, d_xy, d_out); break;
    default: hipLaunchKernelGGL((k_selftest_sample<false, true>), grd, blk, 0, ctx->stream, lv, n, d_xy, d_out); break;
    }
    HIPCHK(ctx, hipGetLastError());
    if ((rc = st.out(1, out, sizes[1]))) return rc;
    return st.finish();
}

// What the context owns as scratch becomes `word`: every buf[] entry that is no state (DevBuf::state), the row queue, the
// Lucas-Kanade pyramids and the frame slots -- and what described their content is withdrawn (no slot is valid, no slot has a
// Lucas-Kanade pyramid, no hand-over count to read).  The descriptor ring of the batched launches is rewritten whole by
// every launch that uses it and stays as it is.
int pagk_selftest_fill_workspaces(pagk_ctx *ctx, uint32_t word, int32_t also_new)
{
    if (!ctx) return PAGK_E_ARG;
    if (in_capture(ctx)) {
        snprintf(ctx->err, sizeof(ctx->err), "the workspaces would have to be overwritten inside a graph capture: fill them before pagk_graph_begin");
        return PAGK_E_ARG;
    }
    for (int k = 0; k < pagk_ctx::kGraphs; k++)
        if (ctx->graph_execs[k]) {
            snprintf(ctx->err, sizeof(ctx->err), "the workspaces would have to be overwritten while graph %d of this context is alive (its nodes "
                     "read the slots and buffers as they were captured): destroy the graph first", k);
            return PAGK_E_ARG;
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // (the pinned mirror is written by the host)
    if (ctx->aux_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->aux_stream));
    ctx->fill_word = word;
    ctx->fill_new = also_new != 0;
    int rc = PAGK_OK;
    for (DevBuf &b : ctx->buf) {
        if (b.state) continue;
        fill_words_host(b.host, b.bytes, word);
        if ((rc = fill_words(ctx, b.ptr, b.bytes, word))) return rc;
    }
    if ((rc = fill_words(ctx, ctx->queue, 256, word))) return rc;
    for (auto &p : ctx->lk_pyr) p.top = -1;
    for (auto &o : ctx->orbl) o = pagk_ctx::OrbLevelsSlot();
    for (FrameSlot &s : ctx->slots) {
        s.valid = false;
        if ((rc = fill_words(ctx, s.block.ptr, s.block.bytes, word))) return rc;
    }
    ctx->last_handover = false;
    if (ctx->seq) ctx->seq->started = ctx->seq->stepped = false;   // (its key sets and work arrays are scratch too)
    return PAGK_OK;
}

// GyroAidedTracker::MatchFeatures, src/gyro_aided_tracker.cpp:949-1008, as the reference writes it: a sequential pass
// over a set and an erase loop.  Its result is a count and a stable compaction (feature i keeps its choice t iff exactly
// one feature chose t, in increasing i): pagk_match_features_device below computes the same bytes on device lists.
int pagk_match_features(int32_t n, int32_t cap, const int32_t *count, const int32_t *nbr_idx, const float *nbr_dist,
                        const float *nbr_ncc, int32_t use_ncc, int32_t *match_query, int32_t *match_train,
                        float *match_dist, float *match_ncc)
{
    if (n < 0 || cap < 1) return PAGK_E_ARG;
    if (n > 0 && (!count || !nbr_idx || !nbr_dist || !nbr_ncc || !match_query || !match_train)) return PAGK_E_ARG;
    const float TH_NCC_HIGH = 0.6f, TH_NCC_LOW = 0.3f, TH_RATIO = 0.75f;  // :7-9
    struct M {
        int q, t;
        float d, c;
    };
    try {
        std::vector<M> matches;
        std::vector<int> found;  // sFoundInCurPts (:951): indices stay in it after their matches are erased
        for (int i = 0; i < n; i++) {
            const int c = count[i];
            if (c <= 0) continue;  // :955
            if (c > cap) return PAGK_E_CAPACITY;
            const float *ncc = nbr_ncc + (size_t)i * cap, *dist = nbr_dist + (size_t)i * cap;
            if (use_ncc) {  // :959-975
                if (!(ncc[0] > TH_NCC_HIGH)) {
                    if (c > 1) {
                        if (ncc[0] < TH_NCC_LOW) continue;
                        if (!(ncc[1] < ncc[0] * TH_RATIO)) continue;  // the two best are too similar
                    } else
                        continue;
                }
            } else if (c > 1 && !(dist[0] < dist[1] * TH_RATIO)) {  // :977-989
                continue;
            }
            const M m{i, nbr_idx[(size_t)i * cap], dist[0], ncc[0]};
            bool seen = false;
            for (int t : found) seen = seen || t == m.t;
            if (!seen) {  // :991-994
                matches.push_back(m);
                found.push_back(m.t);
            } else {      // :995-1005
                size_t w = 0;
                for (size_t r = 0; r < matches.size(); r++)
                    if (matches[r].t != m.t) matches[w++] = matches[r];
                matches.resize(w);
            }
        }
        for (size_t k = 0; k < matches.size(); k++) {
            match_query[k] = matches[k].q;
            match_train[k] = matches[k].t;
            if (match_dist) match_dist[k] = matches[k].d;
            if (match_ncc) match_ncc[k] = matches[k].c;
        }
        return (int)matches.size();
    } catch (const std::bad_alloc &) {
        return PAGK_E_NOMEM;
    }
}

// ---- track-to-detection association (pagk_associate_kernel.h) --------------------------------------------------------
void pagk_assoc_params_default(pagk_assoc_params *p)
{
    if (!p) return;
    p->th_ncc_high = 0.6f, p->th_ncc_low = 0.3f, p->th_ratio = 0.75f;   // src/gyro_aided_tracker.cpp:7-9
    p->use_ncc = 1;                     // mbNCC, :60
    p->min_matches = 100;               // :921
    p->klt_max_distance = 4.0f;         // :1066
    p->klt_ratio = 0.7;                 // :1081
    p->klt_disparity_factor = 1.5;      // :1115
}

int pagk_assoc_params_check(const pagk_assoc_params *p)
{
    if (!p) return PAGK_E_ARG;
    auto ok = [](double v) { return std::isfinite(v) && v >= 0; };
    if (!ok(p->th_ncc_high) || !ok(p->th_ncc_low) || !ok(p->th_ratio) || !ok(p->klt_max_distance) || !ok(p->klt_ratio) ||
        !ok(p->klt_disparity_factor))
        return PAGK_E_ARG;
    if ((p->use_ncc != 0 && p->use_ncc != 1) || p->min_matches < 0) return PAGK_E_ARG;
    return PAGK_OK;
}

namespace {

// buf[ASSOC]: choice (rows) | neighbour counts (rows) | best distances (rows) | claims or owners (m)
struct AssocWs {
    int32_t *choice, *nnb, *claims;
    float *dist0;
    size_t claims_bytes;
};

int assoc_reserve(pagk_ctx *ctx, int32_t rows, int32_t m, AssocWs *w)
{
    const size_t rr = (size_t)std::max(rows, 1), mm = (size_t)std::max(m, 1);
    const size_t sizes[4] = {rr * 4, rr * 4, rr * 4, mm * 4};
    const Layout<4> lay(sizes);
    DevBuf &b = ctx->buf[pagk_ctx::ASSOC];
    int rc = reserve(ctx, b, lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the association's workspace",
                     "run the call once with these sizes before capturing");
    if (rc) return rc;
    w->choice = lay.at<int32_t>(b.ptr, 0), w->nnb = lay.at<int32_t>(b.ptr, 1), w->dist0 = lay.at<float>(b.ptr, 2);
    w->claims = lay.at<int32_t>(b.ptr, 3), w->claims_bytes = mm * 4;
    return PAGK_OK;
}

// choose and compact on device lists; `a` carries everything but the workspace
int match_launch(pagk_ctx *ctx, MatchArgs a, const AssocWs &w)
{
    a.choice = w.choice, a.claims = w.claims;
    HIPCHK(ctx, hipMemsetAsync(w.claims, 0, w.claims_bytes, ctx->stream));
    if (a.n > 0) {
        hipLaunchKernelGGL(k_match_choose, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, ctx->stream, a);
        HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_match_compact, dim3(1), dim3(1024), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

MatchArgs match_args(const pagk_assoc_params *p, int32_t n, int32_t m, int32_t cap, const int32_t *d_count,
                     const int32_t *d_nbr_idx, const float *d_nbr_dist, const float *d_nbr_ncc, int32_t *d_match_query,
                     int32_t *d_match_train, float *d_match_dist, float *d_match_ncc, int32_t *d_n_matches, int32_t *d_info)
{
    MatchArgs a = {};
    a.n = n, a.m = m, a.cap = cap, a.use_ncc = p->use_ncc;
    a.th_high = p->th_ncc_high, a.th_low = p->th_ncc_low, a.th_ratio = p->th_ratio;
    a.count = d_count, a.nbr_idx = d_nbr_idx, a.nbr_dist = d_nbr_dist, a.nbr_ncc = d_nbr_ncc;
    a.match_query = d_match_query, a.match_train = d_match_train, a.match_dist = d_match_dist, a.match_ncc = d_match_ncc;
    a.n_matches = d_n_matches, a.info = d_info;
    return a;
}

int search_gyro_slots(pagk_ctx *ctx, const pagk_assoc_params *p, const FrameSlot &sr, const FrameSlot &sc, int32_t half_patch,
                      int32_t n, const float *d_keys_ref, const float *d_pt_predict_un, const uint8_t *d_status,
                      const float *d_affine, int32_t m, const float *d_keys_cur, const float *d_keys_cur_un, const int32_t *d_m,
                      float radius_unit, int32_t cap, int32_t *d_count, int32_t *d_nbr_idx, float *d_nbr_dist, float *d_nbr_ncc,
                      int32_t *d_match_query, int32_t *d_match_train, float *d_match_dist, float *d_match_ncc,
                      int32_t *d_n_matches, float *d_flows_err, int32_t *d_info)
{
    AssocWs w;
    int rc = assoc_reserve(ctx, n, m, &w);
    if (rc) return rc;
    MatchArgs a = match_args(p, n, m, cap, d_count, d_nbr_idx, d_nbr_dist, d_nbr_ncc, d_match_query, d_match_train,
                             d_match_dist, d_match_ncc, d_n_matches, d_info);
    a.keys_cur_un = d_keys_cur_un, a.pt_pred = d_pt_predict_un, a.flows = d_flows_err;
    if (n > 0) HIPCHK(ctx, hipMemsetAsync(d_count, 0, (size_t)n * 4, ctx->stream));
    // Step 2.1 and 2.2 (:912-917)
    if ((rc = near_neighbors_launch(ctx, sr, sc, half_patch, n, d_keys_ref, d_pt_predict_un, d_status, d_affine, m, d_keys_cur,
                                    d_keys_cur_un, 1, radius_unit, p->use_ncc, 0, cap, d_count, d_nbr_idx, d_nbr_dist,
                                    d_nbr_ncc, nullptr, 0, d_m)) ||
        (rc = match_launch(ctx, a, w)))
        return rc;
    // the wider search, decided by the count on the device (:921-925): it fills only the lists that are empty (:793), and
    // choosing again on unchanged lists gives the same matches, so the second match needs no gate of its own
    if ((rc = near_neighbors_launch(ctx, sr, sc, half_patch, n, d_keys_ref, d_pt_predict_un, d_status, d_affine, m, d_keys_cur,
                                    d_keys_cur_un, 2, radius_unit, p->use_ncc, 0, cap, d_count, d_nbr_idx, d_nbr_dist,
                                    d_nbr_ncc, d_n_matches, p->min_matches, d_m)))
        return rc;
    a.gate = d_n_matches, a.gate_below = p->min_matches;
    return match_launch(ctx, a, w);
}

int search_klt_slots(pagk_ctx *ctx, const pagk_lk_params *lk, const pagk_assoc_params *p, int32_t slot_ref, int32_t slot_cur,
                     int32_t cap, const float *d_keys_ref, const int32_t *d_n, int32_t m, const float *d_keys_cur,
                     const int32_t *d_m, float *d_pt_out, uint8_t *d_status, float *d_err, int32_t *d_match_query,
                     int32_t *d_match_train, float *d_match_dist, double *d_disparity, int32_t *d_n_matches, double *d_stats,
                     int32_t *d_info, int32_t *d_lk_info)
{
    if (!ctx || pagk_assoc_params_check(p) || m < 0 || (m > 0 && !d_keys_cur) || !d_match_query || !d_match_train ||
        !d_disparity || !d_n_matches || !d_stats || !d_info || !d_lk_info)
        return PAGK_E_ARG;
    // calcOpticalFlowPyrLK and Step 1 (:1041-1057); it checks the rest of the arguments
    int rc = lk_track_slots(ctx, lk, slot_ref, slot_cur, cap, d_keys_ref, d_n, d_pt_out, d_status, nullptr, d_err, nullptr,
                            d_lk_info);
    if (rc) return rc;
    AssocWs w;
    if ((rc = assoc_reserve(ctx, cap, m, &w))) return rc;
    KltArgs a = {};
    a.cap = cap, a.m = m, a.d_n = d_n, a.d_m = d_m, a.status = d_status, a.pt_lk = d_pt_out, a.pt_ref = d_keys_ref;
    a.keys_cur = d_keys_cur, a.max_distance = p->klt_max_distance, a.ratio = p->klt_ratio, a.factor = p->klt_disparity_factor;
    a.choice = w.choice, a.nnb = w.nnb, a.dist0 = w.dist0, a.owner = w.claims;
    a.match_query = d_match_query, a.match_train = d_match_train, a.match_dist = d_match_dist, a.disparity = d_disparity;
    a.n_matches = d_n_matches, a.stats = d_stats, a.info = d_info;
    HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)w.claims, 0x7fffffff, w.claims_bytes / 4, ctx->stream));
    hipLaunchKernelGGL(k_radius_top2, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, ctx->stream, a);   // Step 2, :1059-1087
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_klt_finish, dim3(1), dim3(1024), 0, ctx->stream, a);                                // Steps 3 and 4
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

}  // namespace

int pagk_match_features_device(pagk_ctx *ctx, const pagk_assoc_params *params, int32_t n, int32_t m, int32_t cap,
                               const int32_t *d_count, const int32_t *d_nbr_idx, const float *d_nbr_dist,
                               const float *d_nbr_ncc, int32_t *d_match_query, int32_t *d_match_train, float *d_match_dist,
                               float *d_match_ncc, int32_t *d_n_matches, int32_t *d_info)
{
    if (!ctx || pagk_assoc_params_check(params) || n < 0 || m < 0 || cap < 1 || !d_n_matches || !d_info) return PAGK_E_ARG;
    if (n > 0 && (!d_count || !d_nbr_idx || !d_nbr_dist || !d_nbr_ncc || !d_match_query || !d_match_train)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AssocWs w;
    int rc = assoc_reserve(ctx, n, m, &w);
    if (rc) return rc;
    return match_launch(ctx, match_args(params, n, m, cap, d_count, d_nbr_idx, d_nbr_dist, d_nbr_ncc, d_match_query,
                                        d_match_train, d_match_dist, d_match_ncc, d_n_matches, d_info), w);
}

int pagk_search_gyro_predict_device(pagk_ctx *ctx, const pagk_assoc_params *params, int32_t slot_ref, int32_t slot_cur,
                                    int32_t half_patch, int32_t n, const float *d_keys_ref, const float *d_pt_predict_un,
                                    const uint8_t *d_status, const float *d_affine, int32_t m, const float *d_keys_cur,
                                    const float *d_keys_cur_un, const int32_t *d_m, float radius_unit, int32_t cap,
                                    int32_t *d_count, int32_t *d_nbr_idx, float *d_nbr_dist, float *d_nbr_ncc,
                                    int32_t *d_match_query, int32_t *d_match_train, float *d_match_dist, float *d_match_ncc,
                                    int32_t *d_n_matches, float *d_flows_err, int32_t *d_info)
{
    if (!ctx || pagk_assoc_params_check(params) || slot_ref < 0 || slot_ref >= kUserSlots || slot_cur < 0 || slot_cur >= kUserSlots)
        return PAGK_E_ARG;
    if (half_patch < 1 || half_patch > PAGK_MAX_HALF_PATCH || n < 0 || m < 0 || cap < 1 || !d_n_matches || !d_info) return PAGK_E_ARG;
    if (n > 0 && (!d_keys_ref || !d_pt_predict_un || !d_status || !d_count || !d_nbr_idx || !d_nbr_dist || !d_nbr_ncc ||
                  !d_match_query || !d_match_train))
        return PAGK_E_ARG;
    if (n > 0 && m > 0 && (!d_keys_cur || !d_keys_cur_un)) return PAGK_E_ARG;
    const FrameSlot &sr = ctx->slots[slot_ref], &sc = ctx->slots[slot_cur];
    if (!sr.valid || !sc.valid) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return search_gyro_slots(ctx, params, sr, sc, half_patch, n, d_keys_ref, d_pt_predict_un, d_status, d_affine, m, d_keys_cur,
                             d_keys_cur_un, d_m, radius_unit, cap, d_count, d_nbr_idx, d_nbr_dist, d_nbr_ncc, d_match_query,
                             d_match_train, d_match_dist, d_match_ncc, d_n_matches, d_flows_err, d_info);
}

int pagk_search_gyro_predict(pagk_ctx *ctx, const pagk_assoc_params *params, const pagk_image *ref, const pagk_image *cur,
                             int32_t half_patch, int32_t n, const float *keys_ref, const float *pt_predict_un,
                             const uint8_t *status, const float *affine, int32_t m, const float *keys_cur,
                             const float *keys_cur_un, float radius_unit, int32_t cap, int32_t *count, int32_t *nbr_idx,
                             float *nbr_dist, float *nbr_ncc, int32_t *match_query, int32_t *match_train, float *match_dist,
                             float *match_ncc, float *flows_err, int32_t *info)
{
    if (!ctx || pagk_assoc_params_check(params)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_search_gyro_predict");
    if (half_patch < 1 || half_patch > PAGK_MAX_HALF_PATCH || n < 0 || m < 0 || cap < 1) return PAGK_E_ARG;
    if (n > 0 && (!keys_ref || !pt_predict_un || !status || !count || !nbr_idx || !nbr_dist || !nbr_ncc || !match_query ||
                  !match_train))
        return PAGK_E_ARG;
    if (n > 0 && m > 0 && (!keys_cur || !keys_cur_un)) return PAGK_E_ARG;
    int rc;
    if ((rc = check_image(ref)) || (rc = check_image(cur))) return rc;
    if ((rc = frame_upload_any(ctx, 4, ref, 1)) || (rc = frame_upload_any(ctx, 5, cur, 1))) return rc;
    const size_t nn = (size_t)(n < 1 ? 1 : n), mm = (size_t)(m < 1 ? 1 : m), cc = (size_t)cap;
    // keys_ref | pt_predict_un | status | affine | keys_cur | keys_cur_un | count | nbr_idx | nbr_dist | nbr_ncc |
    // match_query | match_train | match_dist | match_ncc | flows_err | the count and the info words
    const size_t sizes[16] = {nn * 8, nn * 8, nn, nn * 16, mm * 8, mm * 8, nn * 4, nn * cc * 4, nn * cc * 4, nn * cc * 4,
                              nn * 4, nn * 4, nn * 4, nn * 4, nn * 8, 256};
    const size_t fn = (size_t)n, fm = (size_t)m, list = fn * cc * 4;
    int32_t tail[1 + kAssocInfoWords] = {};   // (in front of the object: copies write it)
    Staged<16> s(ctx, sizes);
    if ((rc = s.open(&ctx->buf[pagk_ctx::SCORE], "the neighbour search's scratch")) || (rc = s.in(0, keys_ref, fn * 8)) ||
        (rc = s.in(1, pt_predict_un, fn * 8)) || (rc = s.in(2, status, fn)) || (rc = s.in(3, affine, fn * 16)) ||
        (rc = s.in(4, keys_cur, fm * 8)) || (rc = s.in(5, keys_cur_un, fm * 8)) ||
        // the lists of features that stay empty keep the caller's content
        (rc = s.in(7, nbr_idx, list)) || (rc = s.in(8, nbr_dist, list)) || (rc = s.in(9, nbr_ncc, list)))
        return rc;
    int32_t *d_tail = s.at<int32_t>(15);
    rc = search_gyro_slots(ctx, params, ctx->slots[4], ctx->slots[5], half_patch, n, s.at<float>(0), s.at<float>(1),
                           s.at<uint8_t>(2), affine ? s.at<float>(3) : nullptr, m, s.at<float>(4), s.at<float>(5), nullptr,
                           radius_unit, cap, s.at<int32_t>(6), s.at<int32_t>(7), s.at<float>(8), s.at<float>(9),
                           s.at<int32_t>(10), s.at<int32_t>(11), s.at<float>(12), s.at<float>(13), d_tail,
                           flows_err ? s.at<float>(14) : nullptr, d_tail + 1);
    if (rc || (rc = s.out(6, count, fn * 4)) || (rc = s.out(7, nbr_idx, list)) || (rc = s.out(8, nbr_dist, list)) ||
        (rc = s.out(9, nbr_ncc, list)) || (rc = s.out(10, match_query, fn * 4)) || (rc = s.out(11, match_train, fn * 4)) ||
        (rc = s.out(12, match_dist, fn * 4)) || (rc = s.out(13, match_ncc, fn * 4)) || (rc = s.out(14, flows_err, fn * 8)) ||
        (rc = s.out(15, tail, sizeof tail)) || (rc = s.finish()))
        return rc;
    if (info) memcpy(info, tail + 1, kAssocInfoWords * sizeof(int32_t));
    if (tail[2]) {   // a list did not fit: count[] holds the sizes needed
        snprintf(ctx->err, sizeof(ctx->err), "%d neighbour lists are longer than the capacity %d", tail[2], cap);
        return PAGK_E_CAPACITY;
    }
    return tail[0];
}

int pagk_search_klt_device(pagk_ctx *ctx, const pagk_lk_params *lk_params, const pagk_assoc_params *assoc_params,
                           int32_t slot_ref, int32_t slot_cur, int32_t cap, const float *d_keys_ref, const int32_t *d_n,
                           int32_t m, const float *d_keys_cur, const int32_t *d_m, float *d_pt_out, uint8_t *d_status,
                           float *d_err, int32_t *d_match_query, int32_t *d_match_train, float *d_match_dist,
                           double *d_disparity, int32_t *d_n_matches, double *d_stats, int32_t *d_info, int32_t *d_lk_info)
{
    if (slot_ref < 0 || slot_ref >= kUserSlots || slot_cur < 0 || slot_cur >= kUserSlots) return PAGK_E_ARG;
    return search_klt_slots(ctx, lk_params, assoc_params, slot_ref, slot_cur, cap, d_keys_ref, d_n, m, d_keys_cur, d_m, d_pt_out,
                            d_status, d_err, d_match_query, d_match_train, d_match_dist, d_disparity, d_n_matches, d_stats,
                            d_info, d_lk_info);
}

int pagk_search_klt(pagk_ctx *ctx, const pagk_lk_params *lk_params, const pagk_assoc_params *assoc_params,
                    const pagk_image *ref, const pagk_image *cur, int32_t n, const float *keys_ref, int32_t m,
                    const float *keys_cur, float *pt_out, uint8_t *status, float *err, int32_t *match_query,
                    int32_t *match_train, float *match_dist, double *disparity, double *stats, int32_t *info, int32_t *lk_info)
{
    if (!ctx || !ref || !cur || lk_params_check(lk_params) || pagk_assoc_params_check(assoc_params)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_search_klt");
    if (n < 0 || n > kLkMaxRows || m < 0 || (n && (!keys_ref || !pt_out || !status || !err || !match_query || !match_train || !disparity)))
        return PAGK_E_ARG;
    if (m > 0 && !keys_cur) return PAGK_E_ARG;
    if (ref->width != cur->width || ref->height != cur->height || pagk_lk_levels(ref->width, ref->height, lk_params) < 0)
        return PAGK_E_ARG;
    int rc;
    if ((rc = frame_upload_any(ctx, 4, ref, 1)) || (rc = frame_upload_any(ctx, 5, cur, 1))) return rc;
    if ((rc = lk_pyramid_slot(ctx, lk_params, 4)) || (rc = lk_pyramid_slot(ctx, lk_params, 5))) return rc;
    const size_t nc = (size_t)std::max(n, 1), mm = (size_t)std::max(m, 1), nn = (size_t)n;
    // keys_ref | count | keys_cur | pt_out | status | err | match_query | match_train | match_dist | disparity | stats |
    // the match count, the info words and Lucas-Kanade's
    const size_t sizes[12] = {nc * 8, 256, mm * 8, nc * 8, nc, nc * 4, nc * 4, nc * 4, nc * 4, nc * 8, 256, 256};
    int32_t tail[1 + kAssocInfoWords + kLkInfoWords] = {};
    Staged<12> s(ctx, sizes);
    if ((rc = s.open(nullptr, nullptr)) || (rc = s.in(0, keys_ref, nn * 8)) || (rc = s.in(1, &n, 4)) ||
        (rc = s.in(2, keys_cur, (size_t)m * 8)))
        return rc;
    int32_t *d_tail = s.at<int32_t>(11);
    rc = search_klt_slots(ctx, lk_params, assoc_params, 4, 5, (int32_t)nc, s.at<float>(0), s.at<int32_t>(1), m, s.at<float>(2),
                          nullptr, s.at<float>(3), s.at<uint8_t>(4), s.at<float>(5), s.at<int32_t>(6), s.at<int32_t>(7),
                          s.at<float>(8), s.at<double>(9), d_tail, s.at<double>(10), d_tail + 1, d_tail + 1 + kAssocInfoWords);
    if (rc || (rc = s.out(3, pt_out, nn * 8)) || (rc = s.out(4, status, nn)) || (rc = s.out(5, err, nn * 4)) ||
        (rc = s.out(6, match_query, nn * 4)) || (rc = s.out(7, match_train, nn * 4)) || (rc = s.out(8, match_dist, nn * 4)) ||
        (rc = s.out(9, disparity, nn * 8)) || (rc = s.out(10, stats, kAssocStatsWords * sizeof(double))) ||
        (rc = s.out(11, tail, sizeof tail)) || (rc = s.finish()))
        return rc;
    if (info) memcpy(info, tail + 1, kAssocInfoWords * sizeof(int32_t));
    if (lk_info) memcpy(lk_info, tail + 1 + kAssocInfoWords, kLkInfoWords * sizeof(int32_t));
    return tail[0];
}

// ---- the sequence the context owns (Examples/Demo/RealSenseD435i.cpp:199-321) ---------------------------------------------
namespace {

constexpr int kSeqParts = 34;

// This frame's inputs into the next pinned block, then one asynchronous copy into the fixed device block.
// (a sensor sequence: the frame's rows as they arrive, and the IMU window -- `win`, or for the first frame t_ref = t_cur = t0
// and no sample)
int seq_feed(pagk_ctx *ctx, SeqState &q, const pagk_image *frame, const float *rot9, const float *cand, int32_t n_cand,
             const pagk_imu_window *win = nullptr, double t0 = 0.0)
{
    const int k = q.turn;
    q.turn = (k + 1) % SeqState::kRing;
    if (q.recorded[k]) HIPCHK(ctx, hipEventSynchronize(q.read_done[k]));   // flow control only: the copy four frames ago
    uint8_t *pin = static_cast<uint8_t *>(q.pinned[k]);
    for (int y = 0; y < q.rows; y++)
        memcpy(pin + (size_t)y * q.row_bytes, frame->data + (int64_t)y * frame->step, q.row_bytes);
    if (rot9) memcpy(pin + q.off_rot, rot9, 9 * sizeof(float));
    if (q.sensor) {
        uint8_t *w = pin + q.off_win;
        const double t_ref = win ? win->t_ref : t0, t_cur = win ? win->t_cur : t0;
        const int32_t n = win ? win->n : 0;
        memcpy(w, &t_ref, 8), memcpy(w + 8, &t_cur, 8), memcpy(w + kImuOffN, &n, 4);
        if (win) memcpy(w + kImuOffBias, win->bias, 12);
        if (n) memcpy(w + kImuOffT, win->t, (size_t)n * 8), memcpy(w + kImuOffW, win->w, (size_t)n * 12);
    }
    if (q.p.detector == 0) {
        memcpy(pin + q.off_ncand, &n_cand, sizeof n_cand);
        if (n_cand) memcpy(pin + q.off_cand, cand, (size_t)n_cand * 8);
    }
    if (q.res.depth) {   // what k_results_pack reads of the frame: its number and its time (spare bytes of the n_cand part)
        const int32_t frame_no = q.started ? q.frames : 0;
        const double t = win ? win->t_cur : t0;
        memcpy(pin + q.off_ncand + kResultsFrameOff, &frame_no, 4), memcpy(pin + q.off_ncand + kResultsTimeOff, &t, 8);
    }
    HIPCHK(ctx, hipMemcpyAsync(q.in, pin, q.in_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(q.read_done[k], ctx->stream));
    q.recorded[k] = true;
    return PAGK_OK;
}

// what every start / step checks of its frame and candidate list
int seq_inputs_check(const SeqState &q, const pagk_image *frame, const float *cand, int32_t n_cand)
{
    const bool raw = q.sensor && q.s.raw;   // a raw frame: src_width x src_height pixels of `channels` bytes
    if (!frame || !frame->data || frame->width != (raw ? q.s.src_width : q.p.width) ||
        frame->height != (raw ? q.s.src_height : q.p.height) || frame->step < (int64_t)q.row_bytes)
        return PAGK_E_ARG;
    if (q.p.detector == 0) return cand && n_cand >= 0 && n_cand <= q.p.cand_cap ? PAGK_OK : PAGK_E_ARG;   // (required, even when empty)
    return !cand && n_cand == 0 ? PAGK_OK : PAGK_E_ARG;   // a detecting sequence takes no list
}

// the frame in the input block into frame slot `slot` (Lucas-Kanade: through the parity's own copy, with its pyrDown levels)
int seq_frame(pagk_ctx *ctx, SeqState &q, int slot)
{
    const pagk_sequence_params &p = q.p;
    if (q.sensor && q.s.raw) {   // through the context's maps into the slot (Examples/Demo/RealSenseD435i.cpp:202, src/frame.cpp:81-87)
        if (ctx->rect_w != p.width || ctx->rect_h != p.height) {
            snprintf(ctx->err, sizeof(ctx->err), "the sequence is %d x %d, the maps are now %d x %d (pagk_rectify_set_maps)", p.width,
                     p.height, ctx->rect_w, ctx->rect_h);
            return PAGK_E_ARG;
        }
        int rc = rect_into_slot(ctx, slot, &q.s.rectify, q.in, false, q.s.src_width, q.s.src_height, (int64_t)q.row_bytes,
                                p.track.pyramids, "the sensor sequence");
        // Lucas-Kanade reads the rectified level 0 of the slot in place
        return rc || p.tracker != PAGK_SEQ_LK ? rc : lk_pyramid_slot(ctx, &p.lk, slot);
    }
    if (p.tracker != PAGK_SEQ_LK) return pagk_frame_set_device(ctx, slot, q.in, p.width, p.height, p.width, p.track.pyramids);
    HIPCHK(ctx, hipMemcpyAsync(q.img[slot], q.in, (size_t)p.width * p.height, hipMemcpyDeviceToDevice, ctx->stream));
    int rc = pagk_frame_set_device(ctx, slot, q.img[slot], p.width, p.height, p.width, p.track.pyramids);
    return rc ? rc : lk_pyramid_slot(ctx, &p.lk, slot);
}

int seq_handover(pagk_ctx *ctx, SeqState &q, const uint8_t *status, int slot)
{
    const pagk_sequence_params &p = q.p;
    const SeqState::KeySet &d = q.set[slot];
    if (p.detector == 2)
        return pagk_frame_handover_fast_device(ctx, &p.track, p.width, p.height, p.cap, p.target_n, p.new_point_threshold, status,
                                               q.pp, q.ppu, &p.fast, slot, d.keys, d.keys_un, d.keys_normal, d.index_in_last,
                                               d.live, nullptr, q.state, q.info);
    if (p.detector == 1)
        return pagk_frame_handover_detect_device(ctx, &p.track, p.width, p.height, p.cap, p.target_n, p.new_point_threshold,
                                                 status, q.pp, q.ppu, &p.harris, slot, d.keys, d.keys_un, d.keys_normal,
                                                 d.index_in_last, d.live, nullptr, q.state, q.info);
    return pagk_frame_handover_device(ctx, &p.track, p.width, p.height, p.cap, p.target_n, p.new_point_threshold, status, q.pp,
                                      q.ppu, p.cand_cap, reinterpret_cast<const int32_t *>(q.in + q.off_ncand),
                                      reinterpret_cast<const float *>(q.in + q.off_cand), d.keys, d.keys_un, d.keys_normal,
                                      d.index_in_last, d.live, nullptr, q.state);
}

// the arguments of a sensor sequence's own two kernels: the integration of the window in the input block ...
GyroArgs seq_gyro_args(const SeqState &q)
{
    const pagk_sequence_params &p = q.p;
    GyroArgs g;
    memset(&g, 0, sizeof g);
    g.win = q.in + q.off_win;
    memcpy(g.Rbc, q.s.Rbc, sizeof g.Rbc);
    g.fx = p.track.fx, g.fy = p.track.fy, g.cx = p.track.cx, g.cy = p.track.cy;
    g.Rcl = q.rcl, g.rot9 = q.rot_out;
    return g;
}

// ... and the flow velocities of key set c against set 1 - c
FlowVelocityArgs seq_flow_args(const SeqState &q, int c)
{
    FlowVelocityArgs f;
    memset(&f, 0, sizeof f);
    f.normal_cur = q.set[c].keys_normal, f.normal_last = q.set[1 - c].keys_normal, f.index_in_last = q.set[c].index_in_last;
    f.state = q.state, f.win = q.in + q.off_win, f.v = q.vel, f.cap = q.p.cap;
    return f;
}

// the arguments of the pack of a frame of parity c: key set c, the pair's arrays, the ids of parity 1 - c
ResultsArgs seq_results_args(const SeqState &q, int c)
{
    const SeqState::KeySet &s = q.set[c];
    ResultsArgs a;
    memset(&a, 0, sizeof a);
    a.words = q.in + q.off_ncand, a.state = q.state, a.info = q.info;
    a.keys = s.keys, a.keys_un = s.keys_un, a.keys_normal = s.keys_normal, a.index_in_last = s.index_in_last, a.live = s.live;
    a.velocity = q.sensor && q.s.flow_velocity ? q.vel : nullptr;
    a.status = q.st, a.pt_predict = q.pp, a.pt_predict_un = q.ppu, a.err = q.lk_err;
    a.id_last = q.res.id[1 - c], a.age_last = q.res.age[1 - c], a.next_last = q.res.next[1 - c];
    a.id_cur = q.res.id[c], a.age_cur = q.res.age[c], a.next_cur = q.res.next[c];
    a.rec = q.res.rec, a.cap = q.p.cap, a.sensor = q.sensor ? 1 : 0;
    return a;
}

unsigned results_blocks(int32_t cap) { return (unsigned)((cap + 1023) / 1024); }

// the last launch of a frame with a result ring: everything the read calls deliver, ids and ages, into the record
int seq_results_pack(pagk_ctx *ctx, SeqState &q, int c)
{
    const ResultsArgs a = seq_results_args(q, c);
    hipLaunchKernelGGL(k_results_pack, dim3(results_blocks(q.p.cap)), dim3(1024), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return PAGK_OK;
}

// Behind the step (the graph launch or the direct issue) and outside any capture: the record of frame `frame` into its pinned
// block, and the block's event.  The mirror image of seq_feed's input copy.
int seq_results_post(pagk_ctx *ctx, SeqState &q, int frame)
{
    if (!q.res.depth) return PAGK_OK;
    const int b = frame % q.res.depth;
    HIPCHK(ctx, hipMemcpyAsync(q.res.pinned[b], q.res.rec, q.res.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipEventRecord(q.res.copied[b], ctx->stream));
    q.res.frame_of[b] = frame;
    return PAGK_OK;
}

void seq_results_free(SeqState &q)
{
    for (int k = 0; k < SeqState::Results::kMaxDepth; k++) {
        if (q.res.pinned[k]) (void)hipHostFree(q.res.pinned[k]);
        if (q.res.copied[k]) (void)hipEventDestroy(q.res.copied[k]);
        q.res.pinned[k] = nullptr, q.res.copied[k] = nullptr;
    }
    q.res.depth = 0;
}

// The work of a frame of parity c: frame slot c is the current frame, slot 1 - c the reference; key set 1 - c holds the
// reference keypoints, set c receives the next pair's.
int seq_issue(pagk_ctx *ctx, SeqState &q, int c)
{
    const pagk_sequence_params &p = q.p;
    const SeqState::KeySet &ref = q.set[1 - c];
    const float *rot = q.rot;
    int rc = seq_frame(ctx, q, c);
    if (rc) return rc;
    if (q.sensor) {   // the window of this pair -> the nine floats the prediction reads (:511-587)
        const GyroArgs g = seq_gyro_args(q);
        hipLaunchKernelGGL(k_gyro_integrate, dim3(1), dim3(64), 0, ctx->stream, g);
        HIPCHK(ctx, hipGetLastError());
    }
    if (p.tracker == PAGK_SEQ_LK) {   // :353-380
        const float *init = nullptr;
        const uint8_t *live = ref.live;
        if (p.lk_initial_flow) {
            rc = pagk_gyro_predict_device_live(ctx, &p.track, p.width, p.height, rot, p.cap, ref.keys_un, ref.live, q.pu, q.pd,
                                               q.st_in, q.aff);
            if (rc) return rc;
            init = q.pu, live = q.st_in;
        }
        rc = lk_flow_slots(ctx, &p.lk, &p.track, 1 - c, c, p.cap, ref.keys_un, init, live, q.state, q.ppu, q.pp, q.st, nullptr,
                           q.lk_err, nullptr, q.lk_info);
        if (rc) return rc;
    } else {
        const pagk_outputs out = {q.pt_un, q.pt_dist, q.status, q.pix_err, q.dist_pred, nullptr, nullptr};
        if (p.track.has_gyro_predict_initial) {
            rc = pagk_gyro_predict_device_live(ctx, &p.track, p.width, p.height, rot, p.cap, ref.keys_un, ref.live, q.pu, q.pd,
                                               q.st_in, q.aff);
            if (!rc) rc = pagk_track_device(ctx, &p.track, 1 - c, c, p.cap, ref.keys_un, q.pu, q.aff, q.st_in, &out);
        } else {   // no prediction: the live mask is the tracking kernels' status_in
            rc = pagk_track_device(ctx, &p.track, 1 - c, c, p.cap, ref.keys_un, ref.keys_un, q.aff, ref.live, &out);
        }
        if (rc) return rc;
        rc = pagk_post_filter_device(ctx, p.cap, p.track.half_patch, q.status, q.pix_err, q.dist_pred, q.pt_dist, q.pt_un, q.st,
                                     q.pp, q.ppu, q.kept, q.th);
        if (rc) return rc;
    }
    if (p.validate) {
        rc = pagk_geometry_validation_device(ctx, &p.fit, p.cap, ref.keys_un, q.ppu, q.st, p.sigma, q.cnt, q.score);
        if (rc) return rc;
    }
    rc = seq_handover(ctx, q, q.st, c);
    if (rc) return rc;
    if (q.sensor && q.s.flow_velocity) {
        const FlowVelocityArgs f = seq_flow_args(q, c);   // src/frame.cpp:139-143, on the key set just written
        hipLaunchKernelGGL(k_flow_velocity, dim3((unsigned)((p.cap + 255) / 256)), dim3(256), 0, ctx->stream, f);
        HIPCHK(ctx, hipGetLastError());
    }
    return q.res.depth ? seq_results_pack(ctx, q, c) : PAGK_OK;
}

// the sequence of a call, or nullptr with the reason in ctx->err
SeqState *seq_of(pagk_ctx *ctx, const char *what)
{
    if (!ctx) return nullptr;
    if (ctx->capturing) {
        snprintf(ctx->err, sizeof(ctx->err), "%s between pagk_graph_begin and pagk_graph_end: the sequence captures its own graphs", what);
        return nullptr;
    }
    if (!ctx->seq) snprintf(ctx->err, sizeof(ctx->err), "%s: the context has no sequence (pagk_sequence_create)", what);
    return ctx->seq;
}

// a member of a sequence group is stepped, started and destroyed through its group only
bool seq_grouped(pagk_ctx *ctx, const char *what)
{
    if (!ctx->group) return false;
    snprintf(ctx->err, sizeof(ctx->err), "%s: the context is a member of a sequence group (pagk_sequence_group_step, pagk_sequence_group_destroy)", what);
    return true;
}

// what every sensor step checks of its window, on the host and before anything is enqueued; the text goes to `to`
int seq_window_check(pagk_ctx *to, const SeqState &q, const char *what, const pagk_imu_window *window)
{
    if (pagk_imu_window_check(window, q.s.imu_cap)) {
        snprintf(to->err, sizeof(to->err), "%s: the window fails pagk_imu_window_check (imu_cap %d)", what, q.s.imu_cap);
        return PAGK_E_ARG;
    }
    if (q.started && window->t_ref != q.t_last) {
        snprintf(to->err, sizeof(to->err), "%s: t_ref %.9f is not the previous frame's time %.9f", what, window->t_ref, q.t_last);
        return PAGK_E_ARG;
    }
    return PAGK_OK;
}

}  // namespace

void pagk_sequence_params_default(pagk_sequence_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    pagk_params_default(&p->track);
    pagk_lk_params_default(&p->lk);
    pagk_fit_params_default(&p->fit);
    pagk_detect_params_default(&p->harris);
    pagk_fast_params_default(&p->fast);
    p->tracker = PAGK_SEQ_PATCHMATCH, p->lk_initial_flow = 0;
    p->width = 640, p->height = 480, p->cap = 448, p->target_n = 400, p->new_point_threshold = 320.0;
    p->detector = 0, p->cand_cap = 1024, p->validate = 1, p->sigma = 1.0f;
}

int pagk_sequence_params_check(const pagk_sequence_params *p)
{
    if (!p) return PAGK_E_ARG;
    int rc = check_params(&p->track);
    if (rc || (rc = lk_params_check(&p->lk))) return rc;
    if (!fit_params_ok(&p->fit) || !detect_params_ok(&p->harris)) return PAGK_E_ARG;
    if ((rc = fast_params_check(&p->fast))) return rc;
    if ((p->tracker != PAGK_SEQ_PATCHMATCH && p->tracker != PAGK_SEQ_LK) || (p->lk_initial_flow & ~1) || (p->validate & ~1) ||
        p->detector < 0 || p->detector > 2 || p->width < 14 || p->height < 14 || p->target_n < 1 || p->cap < p->target_n ||
        p->cap > kLkMaxRows || (p->detector == 0 && p->cand_cap < 1) || p->cand_cap < 0 || p->cand_cap > kLkMaxRows ||
        !std::isfinite(p->new_point_threshold) || !std::isfinite(p->sigma) || !(p->sigma > 0.0f) ||
        (int64_t)p->width * p->height > (int64_t)1 << 28)
        return PAGK_E_ARG;
    if (p->tracker == PAGK_SEQ_LK && pagk_lk_levels(p->width, p->height, &p->lk) < 0) return PAGK_E_ARG;
    return PAGK_OK;
}

// (sensor: NULL for a plain sequence, whose block is carved exactly as before the sensor form existed)
static int seq_create(pagk_ctx *ctx, const pagk_sequence_params *params, const pagk_sequence_sensor *sensor)
{
    if (!ctx || pagk_sequence_params_check(params)) return PAGK_E_ARG;
    if (ctx->seq || in_capture(ctx)) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_sequence_create: %s", ctx->seq ? "the context has a sequence already" : "inside a graph capture");
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SeqState *q = new (std::nothrow) SeqState();
    if (!q) return PAGK_E_NOMEM;
    q->p = *params;
    const size_t n = (size_t)params->cap, px = (size_t)params->width * params->height;
    q->row_bytes = (size_t)params->width, q->rows = params->height;
    if (sensor) {
        q->sensor = true, q->s = *sensor;
        if (sensor->raw) q->row_bytes = (size_t)sensor->src_width * sensor->rectify.channels, q->rows = sensor->src_height;
    }
    q->off_rot = align_up(q->row_bytes * q->rows, kPartAlign);
    q->off_ncand = q->off_rot + kPartAlign;
    q->off_cand = q->off_ncand + kPartAlign;
    q->in_bytes = q->off_cand + align_up((size_t)(params->detector == 0 ? params->cand_cap : 0) * 8, kPartAlign);
    if (sensor) {   // the IMU window: one more part of the input block
        q->off_win = q->in_bytes;
        q->in_bytes += align_up(kImuWindowBytes, kPartAlign);
    }
    const bool lk = params->tracker == PAGK_SEQ_LK;
    // input | 2 frame copies (LK) | 2 x (keys keys_un keys_normal index_in_last live) | state | info | the work arrays:
    // pu pd aff pt_un pt_dist pp ppu score lk_err st_in status st zero pix_err dist_pred th kept cnt lk_info
    const size_t sizes[kSeqParts] = {q->in_bytes, lk ? px : 0, lk ? px : 0,
                                     n * 8, n * 8, n * 8, n * 4, n, n * 8, n * 8, n * 8, n * 4, n, 256, 256,
                                     n * 8, n * 8, n * 16, n * 8, n * 8, n * 8, n * 8, 256, n * 4, n, n, n, n, n * 8, n * 8, 256, 256,
                                     256, 256};
    const Layout<kSeqParts> lay(sizes);
    // the sensor parts lie behind the plain sequence's: rot9 and Rcl (k_gyro_integrate), the flow velocities
    const size_t sensor_sizes[2] = {256, n * 8};
    const Layout<2> slay(sensor_sizes);
    DevBuf &b = ctx->buf[pagk_ctx::SEQ];
    int rc = reserve(ctx, b, lay.total + (sensor ? slay.total : 0), NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the sequence's block",
                     "destroy the graphs first");
    for (int k = 0; !rc && k < SeqState::kRing; k++) {
        if (hipHostMalloc(&q->pinned[k], q->in_bytes, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&q->read_done[k], hipEventDisableTiming) != hipSuccess) {
            snprintf(ctx->err, sizeof(ctx->err), "pagk_sequence_create: no pinned input block of %zu bytes", q->in_bytes);
            rc = PAGK_E_NOMEM;
        } else {
            memset(q->pinned[k], 0, q->in_bytes);
        }
    }
    if (rc) {
        for (int k = 0; k < SeqState::kRing; k++) {
            if (q->pinned[k]) (void)hipHostFree(q->pinned[k]);
            if (q->read_done[k]) (void)hipEventDestroy(q->read_done[k]);
        }
        delete q;
        return rc;
    }
    int k = 0;
    void *base = b.ptr;
    q->in = lay.at<uint8_t>(base, k++);
    for (int s = 0; s < 2; s++) q->img[s] = lay.at<uint8_t>(base, k++);
    for (int s = 0; s < 2; s++) {
        q->set[s].keys = lay.at<float>(base, k++), q->set[s].keys_un = lay.at<float>(base, k++);
        q->set[s].keys_normal = lay.at<float>(base, k++), q->set[s].index_in_last = lay.at<int32_t>(base, k++);
        q->set[s].live = lay.at<uint8_t>(base, k++);
    }
    q->state = lay.at<int32_t>(base, k++), q->info = lay.at<int32_t>(base, k++);
    q->work = lay.at<uint8_t>(base, k);
    q->work_bytes = lay.total - lay.off[k];
    q->pu = lay.at<float>(base, k++), q->pd = lay.at<float>(base, k++), q->aff = lay.at<float>(base, k++);
    q->pt_un = lay.at<float>(base, k++), q->pt_dist = lay.at<float>(base, k++), q->pp = lay.at<float>(base, k++);
    q->ppu = lay.at<float>(base, k++), q->score = lay.at<float>(base, k++), q->lk_err = lay.at<float>(base, k++);
    q->st_in = lay.at<uint8_t>(base, k++), q->status = lay.at<uint8_t>(base, k++), q->st = lay.at<uint8_t>(base, k++);
    q->zero = lay.at<uint8_t>(base, k++), q->pix_err = lay.at<double>(base, k++), q->dist_pred = lay.at<double>(base, k++);
    q->th = lay.at<double>(base, k++), q->kept = lay.at<int32_t>(base, k++), q->cnt = lay.at<int32_t>(base, k++);
    q->lk_info = lay.at<int32_t>(base, k++);
    static_assert(kSeqParts == 34, "the carving above names every part");
    if (k != kSeqParts) {
        delete q;
        return PAGK_E_ARG;
    }
    q->rot = reinterpret_cast<const float *>(q->in + q->off_rot);
    if (sensor) {
        void *sbase = static_cast<uint8_t *>(base) + lay.total;
        q->rot_out = slay.at<float>(sbase, 0), q->rcl = q->rot_out + 16, q->vel = slay.at<float>(sbase, 1);
        q->rot = q->rot_out;
    }
    ctx->seq = q;
    return PAGK_OK;
}

int pagk_sequence_create(pagk_ctx *ctx, const pagk_sequence_params *params) { return seq_create(ctx, params, nullptr); }

void pagk_sequence_sensor_default(pagk_sequence_sensor *s)
{
    if (!s) return;
    memset(s, 0, sizeof *s);
    pagk_rectify_params_default(&s->rectify);
    s->raw = 0, s->src_width = s->src_height = 0, s->imu_cap = PAGK_IMU_MAX_SAMPLES;
    s->Rbc[0] = s->Rbc[4] = s->Rbc[8] = 1.0f;
    s->flow_velocity = 1;
}

int pagk_sequence_sensor_check(const pagk_sequence_sensor *s)
{
    if (!s || pagk_rectify_params_check(&s->rectify)) return PAGK_E_ARG;
    if ((s->raw & ~1) || (s->flow_velocity & ~1) || s->imu_cap < 1 || s->imu_cap > PAGK_IMU_MAX_SAMPLES) return PAGK_E_ARG;
    if (s->raw ? (s->src_width < 1 || s->src_height < 1 || s->src_width > 32767 || s->src_height > 32767)
               : (s->rectify.channels != 1)) return PAGK_E_ARG;   // (a frame that is not raw is gray)
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(s->Rbc[k])) return PAGK_E_ARG;
    return PAGK_OK;
}

int pagk_sequence_create_sensor(pagk_ctx *ctx, const pagk_sequence_params *params, const pagk_sequence_sensor *sensor)
{
    if (!ctx || pagk_sequence_params_check(params) || pagk_sequence_sensor_check(sensor)) return PAGK_E_ARG;
    if (sensor->raw && (!ctx->buf[pagk_ctx::RECT_ENTRIES].ptr || ctx->rect_w != params->width || ctx->rect_h != params->height)) {
        if (!ctx->buf[pagk_ctx::RECT_ENTRIES].ptr)
            snprintf(ctx->err, sizeof(ctx->err), "pagk_sequence_create_sensor: raw frames need maps (pagk_rectify_set_maps)");
        else
            snprintf(ctx->err, sizeof(ctx->err), "pagk_sequence_create_sensor: the maps are %d x %d, the sequence is %d x %d", ctx->rect_w,
                     ctx->rect_h, params->width, params->height);
        return PAGK_E_ARG;
    }
    return seq_create(ctx, params, sensor);
}

int pagk_sequence_destroy(pagk_ctx *ctx)
{
    SeqState *q = seq_of(ctx, "pagk_sequence_destroy");
    if (!q || seq_grouped(ctx, "pagk_sequence_destroy")) return PAGK_E_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (int &g : q->graph) {
        if (g >= 0) (void)pagk_graph_destroy(ctx, g);
        g = -1;
    }
    for (int k = 0; k < SeqState::kRing; k++) {
        if (q->pinned[k]) (void)hipHostFree(q->pinned[k]);
        if (q->read_done[k]) (void)hipEventDestroy(q->read_done[k]);
    }
    seq_results_free(*q);
    ctx->seq = nullptr;
    delete q;
    bool alive = false;
    for (int k = 0; k < pagk_ctx::kGraphs; k++) alive = alive || ctx->graph_execs[k];
    if (alive) return PAGK_OK;   // (a graph of the caller's cannot point into them, but stay safe)
    const int rc = release(ctx, ctx->buf[pagk_ctx::RESULTS]);
    return rc ? rc : release(ctx, ctx->buf[pagk_ctx::SEQ]);
}

// the sequence of a call of the plain (`sensor` false) or the sensor form; the other kind is refused with a text
static SeqState *seq_of_kind(pagk_ctx *ctx, const char *what, bool sensor)
{
    SeqState *q = seq_of(ctx, what);
    if (q && q->sensor != sensor) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: the context's sequence is %s", what,
                 q->sensor ? "a sensor sequence (pagk_sequence_start_sensor, pagk_sequence_step_sensor)"
                           : "a plain sequence (pagk_sequence_start, pagk_sequence_step)");
        return nullptr;
    }
    return q;
}

static int seq_start(pagk_ctx *ctx, SeqState *q, const pagk_image *frame, const float *cand, int32_t n_cand, double t0)
{
    if (seq_inputs_check(*q, frame, cand, n_cand)) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (q->sensor) {   // (the first frame has no pair: its velocities are zero)
        HIPCHK(ctx, hipMemsetAsync(q->rot_out, 0, 256, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(q->vel, 0, (size_t)q->p.cap * 8, ctx->stream));
    }
    const pagk_sequence_params &p = q->p;
    // what the loop reads before it has written it: the reach flag, the all-zero status, the identity affine
    HIPCHK(ctx, hipMemsetAsync(q->state, 0, 512, ctx->stream));   // (state and info: two parts of 256 bytes)
    HIPCHK(ctx, hipMemsetAsync(q->work, 0, q->work_bytes, ctx->stream));
    try {
        std::vector<float> eye((size_t)p.cap * 4);
        for (size_t i = 0; i < eye.size(); i += 4) eye[i] = 1.f, eye[i + 1] = 0.f, eye[i + 2] = 0.f, eye[i + 3] = 1.f;
        HIPCHK(ctx, hipMemcpyAsync(q->aff, eye.data(), eye.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (eye is a local)
    } catch (const std::bad_alloc &) {
        return PAGK_E_NOMEM;
    }
    q->started = q->stepped = false;
    q->ever_started = true;
    int rc = seq_feed(ctx, *q, frame, nullptr, cand, n_cand, nullptr, t0);
    if (rc || (rc = seq_frame(ctx, *q, 0)) || (rc = seq_handover(ctx, *q, q->zero, 0))) return rc;
    if (q->res.depth) {   // ids begin at 0 again, the ring is empty, frame 0 is the start's record
        HIPCHK(ctx, hipMemsetAsync(q->res.next[0], 0, 256, ctx->stream));
        for (int &f : q->res.frame_of) f = -1;
        if ((rc = seq_results_pack(ctx, *q, 0)) || (rc = seq_results_post(ctx, *q, 0))) return rc;
    }
    q->started = true, q->frames = 1, q->last_graph = false, q->t_last = t0;
    return PAGK_OK;
}

int pagk_sequence_start(pagk_ctx *ctx, const pagk_image *frame, const float *cand, int32_t n_cand)
{
    SeqState *q = seq_of_kind(ctx, "pagk_sequence_start", false);
    return q && !seq_grouped(ctx, "pagk_sequence_start") ? seq_start(ctx, q, frame, cand, n_cand, 0.0) : PAGK_E_ARG;
}

int pagk_sequence_start_sensor(pagk_ctx *ctx, const pagk_image *raw, double t, const float *cand, int32_t n_cand)
{
    SeqState *q = seq_of_kind(ctx, "pagk_sequence_start_sensor", true);
    if (!q || seq_grouped(ctx, "pagk_sequence_start_sensor") || !std::isfinite(t)) return PAGK_E_ARG;
    return seq_start(ctx, q, raw, cand, n_cand, t);
}

// rot9: the plain form's nine floats; win: the sensor form's window (checked by the caller)
static int seq_step(pagk_ctx *ctx, SeqState *q, const pagk_image *frame, const float *rot9, const pagk_imu_window *win,
                    const float *cand, int32_t n_cand, int32_t mode)
{
    if (seq_inputs_check(*q, frame, cand, n_cand) || (mode != PAGK_SEQ_GRAPH && mode != PAGK_SEQ_DIRECT)) return PAGK_E_ARG;
    const pagk_sequence_params &p = q->p;
    const bool predicts = p.tracker == PAGK_SEQ_LK ? p.lk_initial_flow != 0 : p.track.has_gyro_predict_initial != 0;
    if (!q->started || (predicts && !rot9 && !win)) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_sequence_step: %s", q->started ? "this tracker predicts: rot9 is required"
                                                                                  : "pagk_sequence_start hands in the first frame");
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int c = q->frames & 1;
    int rc = seq_feed(ctx, *q, frame, rot9, cand, n_cand, win);
    if (rc) return rc;
    if (win) q->t_last = win->t_cur;
    if (mode == PAGK_SEQ_GRAPH && q->direct_done[c]) {
        if (q->graph[c] < 0) {
            if ((rc = pagk_graph_begin(ctx))) return rc;
            rc = seq_issue(ctx, *q, c);
            int32_t id = -1;
            const int rc_end = pagk_graph_end(ctx, &id);
            if (rc || rc_end) {
                if (!rc_end && id >= 0) (void)pagk_graph_destroy(ctx, id);
                return rc ? rc : rc_end;
            }
            q->graph[c] = id;
        }
        if ((rc = pagk_graph_launch(ctx, q->graph[c]))) return rc;
        q->last_graph = true;
    } else {   // also the first step of each parity in graph mode: allocations happen outside a capture
        if ((rc = seq_issue(ctx, *q, c))) return rc;
        q->direct_done[c] = true;
        q->last_graph = false;
    }
    if ((rc = seq_results_post(ctx, *q, q->frames))) return rc;
    q->frames++;
    q->stepped = true;
    return PAGK_OK;
}

int pagk_sequence_step(pagk_ctx *ctx, const pagk_image *frame, const float *rot9, const float *cand, int32_t n_cand, int32_t mode)
{
    SeqState *q = seq_of_kind(ctx, "pagk_sequence_step", false);
    return q && !seq_grouped(ctx, "pagk_sequence_step") ? seq_step(ctx, q, frame, rot9, nullptr, cand, n_cand, mode) : PAGK_E_ARG;
}

int pagk_imu_window_check(const pagk_imu_window *w, int32_t imu_cap)
{
    if (!w || imu_cap < 1 || imu_cap > PAGK_IMU_MAX_SAMPLES || w->n < 0 || w->n > imu_cap) return PAGK_E_ARG;
    if (!std::isfinite(w->t_ref) || !std::isfinite(w->t_cur) || !(w->t_cur > w->t_ref)) return PAGK_E_ARG;
    if (w->n > 0 && (!w->t || !w->w)) return PAGK_E_ARG;
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(w->bias[k])) return PAGK_E_ARG;
    for (int32_t i = 0; i < w->n; i++) {
        if (!std::isfinite(w->t[i]) || !std::isfinite(w->w[3 * i]) || !std::isfinite(w->w[3 * i + 1]) || !std::isfinite(w->w[3 * i + 2]))
            return PAGK_E_ARG;
        if (i > 0 && !(w->t[i] > w->t[i - 1])) return PAGK_E_ARG;
    }
    return PAGK_OK;
}

int pagk_sequence_step_sensor(pagk_ctx *ctx, const pagk_image *raw, const pagk_imu_window *window, const float *cand,
                              int32_t n_cand, int32_t mode)
{
    SeqState *q = seq_of_kind(ctx, "pagk_sequence_step_sensor", true);
    if (!q || seq_grouped(ctx, "pagk_sequence_step_sensor") || seq_window_check(ctx, *q, "pagk_sequence_step_sensor", window)) return PAGK_E_ARG;
    return seq_step(ctx, q, raw, nullptr, window, cand, n_cand, mode);
}

int pagk_sequence_read_velocity(pagk_ctx *ctx, int32_t cap, float *v)
{
    SeqState *q = seq_of_kind(ctx, "pagk_sequence_read_velocity", true);
    if (!q || !q->started || !q->s.flow_velocity || !v || cap < 1 || cap > q->p.cap) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(v, q->vel, (size_t)cap * 8, hipMemcpyDeviceToHost));
    return lv_check(ctx);
}

int pagk_gyro_integrate(pagk_ctx *ctx, const float Rbc[9], const pagk_params *camera, const pagk_imu_window *window, float *Rcl,
                        float *rot9)
{
    if (!ctx || !Rbc || !camera || pagk_imu_window_check(window, PAGK_IMU_MAX_SAMPLES)) return PAGK_E_ARG;
    NOT_WHILE_CAPTURING(ctx, "pagk_gyro_integrate");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    alignas(8) uint8_t win[kImuWindowBytes] = {};   // (declared in front of the staging object: a queued copy reads it)
    memcpy(win, &window->t_ref, 8), memcpy(win + 8, &window->t_cur, 8), memcpy(win + kImuOffN, &window->n, 4);
    memcpy(win + kImuOffBias, window->bias, 12);
    if (window->n) {
        memcpy(win + kImuOffT, window->t, (size_t)window->n * 8);
        memcpy(win + kImuOffW, window->w, (size_t)window->n * 12);
    }
    const size_t sizes[3] = {kImuWindowBytes, 9 * sizeof(float), 9 * sizeof(float)};
    Staged<3> s(ctx, sizes);
    int rc = s.open(nullptr, "the staging block of pagk_gyro_integrate");
    if (rc || (rc = s.in(0, win, sizeof win))) return rc;
    GyroArgs g;
    g.win = s.at<uint8_t>(0);
    memcpy(g.Rbc, Rbc, sizeof g.Rbc);
    g.fx = camera->fx, g.fy = camera->fy, g.cx = camera->cx, g.cy = camera->cy;
    g.Rcl = s.at<float>(1), g.rot9 = s.at<float>(2);
    hipLaunchKernelGGL(k_gyro_integrate, dim3(1), dim3(64), 0, ctx->stream, g);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = s.out(1, Rcl, 9 * sizeof(float))) || (rc = s.out(2, rot9, 9 * sizeof(float)))) return rc;
    return s.finish();
}

int pagk_sequence_read(pagk_ctx *ctx, int32_t cap, float *keys, float *keys_un, float *keys_normal, int32_t *index_in_last,
                       uint8_t *live, int32_t *state, int32_t *info)
{
    SeqState *q = seq_of(ctx, "pagk_sequence_read");
    if (!q || !q->started || !keys_un || cap < 1 || cap > q->p.cap) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const SeqState::KeySet &s = q->set[(q->frames - 1) & 1];
    const size_t n = (size_t)cap;
    const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (then plain copies: the arrays are the caller's, pinned or not)
    if (keys) HIPCHK(ctx, hipMemcpy(keys, s.keys, n * 8, d2h));
    HIPCHK(ctx, hipMemcpy(keys_un, s.keys_un, n * 8, d2h));
    if (keys_normal) HIPCHK(ctx, hipMemcpy(keys_normal, s.keys_normal, n * 8, d2h));
    if (index_in_last) HIPCHK(ctx, hipMemcpy(index_in_last, s.index_in_last, n * 4, d2h));
    if (live) HIPCHK(ctx, hipMemcpy(live, s.live, n, d2h));
    if (state) HIPCHK(ctx, hipMemcpy(state, q->state, PAGK_HANDOVER_STATE_WORDS * 4, d2h));
    if (info) HIPCHK(ctx, hipMemcpy(info, q->info, PAGK_DETECT_INFO_WORDS * 4, d2h));
    return lv_check(ctx);
}

int pagk_sequence_read_pair(pagk_ctx *ctx, int32_t cap, uint8_t *status, float *pt_predict, float *pt_predict_un, float *err)
{
    SeqState *q = seq_of(ctx, "pagk_sequence_read_pair");
    if (!q || !q->started || !q->stepped || cap < 1 || cap > q->p.cap) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)cap;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (status) HIPCHK(ctx, hipMemcpy(status, q->st, n, hipMemcpyDeviceToHost));
    if (pt_predict) HIPCHK(ctx, hipMemcpy(pt_predict, q->pp, n * 8, hipMemcpyDeviceToHost));
    if (pt_predict_un) HIPCHK(ctx, hipMemcpy(pt_predict_un, q->ppu, n * 8, hipMemcpyDeviceToHost));
    if (err) HIPCHK(ctx, hipMemcpy(err, q->lk_err, n * 4, hipMemcpyDeviceToHost));
    return lv_check(ctx);
}

int pagk_sequence_status(pagk_ctx *ctx, int32_t *words)
{
    SeqState *sq = seq_of(ctx, "pagk_sequence_status");
    if (!sq || !words) return PAGK_E_ARG;
    const SeqState &q = *sq;
    words[0] = q.started ? q.frames : 0;
    words[1] = q.last_graph ? 1 : 0;
    words[2] = (q.graph[0] >= 0) + (q.graph[1] >= 0);
    words[3] = q.res.depth;
    return PAGK_OK;
}

// ---- the result ring of a sequence (no counterpart in the reference, which hands over mvPtIndexInLastFrame: src/frame.cpp:135,192) ----
int pagk_sequence_results_layout(int32_t cap, int32_t sensor, pagk_results_layout *layout)
{
    if (!layout || cap < 1 || cap > kLkMaxRows || (sensor & ~1)) return PAGK_E_ARG;
    int64_t off[kResultsParts + 1];
    results_layout(cap, off);
    memset(layout, 0, sizeof *layout);
    layout->header = off[RES_HEADER], layout->state = off[RES_STATE], layout->info = off[RES_INFO], layout->keys = off[RES_KEYS];
    layout->keys_un = off[RES_KEYS_UN], layout->keys_normal = off[RES_KEYS_NORMAL], layout->index_in_last = off[RES_INDEX];
    layout->live = off[RES_LIVE], layout->track_id = off[RES_TRACK_ID], layout->age = off[RES_AGE];
    layout->velocity = off[RES_VELOCITY], layout->status = off[RES_STATUS], layout->pt_predict = off[RES_PT_PREDICT];
    layout->pt_predict_un = off[RES_PT_PREDICT_UN], layout->err = off[RES_ERR], layout->bytes = off[kResultsParts];
    layout->cap = cap, layout->sensor = sensor;
    return PAGK_OK;
}

int pagk_sequence_results_create(pagk_ctx *ctx, int32_t depth)
{
    SeqState *q = seq_of(ctx, "pagk_sequence_results_create");
    if (!q || seq_grouped(ctx, "pagk_sequence_results_create")) return PAGK_E_ARG;
    const char *why = nullptr;
    if (q->res.depth) why = "the sequence has a result ring already";
    else if (q->ever_started) why = "after pagk_sequence_start: the ring is made in front of the first frame";
    else if (in_capture(ctx)) why = "inside a graph capture";
    else if (depth < 2 || depth > SeqState::Results::kMaxDepth) why = "depth is outside 2 .. 8";
    if (why) {
        snprintf(ctx->err, sizeof(ctx->err), "pagk_sequence_results_create: %s", why);
        return PAGK_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)q->p.cap;
    int64_t off[kResultsParts + 1];
    results_layout(q->p.cap, off);
    // the record | track_id[2][cap] | age[2][cap] | next_id[2]
    const size_t sizes[6] = {(size_t)off[kResultsParts], n * 8, n * 8, n * 4, n * 4, 256};
    const Layout<6> lay(sizes);
    DevBuf &b = ctx->buf[pagk_ctx::RESULTS];
    int rc = reserve(ctx, b, lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, "the result ring's block", "destroy the graphs first");
    if (rc) return rc;
    SeqState::Results &r = q->res;
    r.bytes = sizes[0];
    r.rec = lay.at<uint8_t>(b.ptr, 0);
    r.id[0] = lay.at<int64_t>(b.ptr, 1), r.id[1] = lay.at<int64_t>(b.ptr, 2);
    r.age[0] = lay.at<int32_t>(b.ptr, 3), r.age[1] = lay.at<int32_t>(b.ptr, 4);
    r.next[0] = lay.at<int64_t>(b.ptr, 5), r.next[1] = r.next[0] + 16;   // (each parity's word in a 128-byte half of its own)
    for (int k = 0; k < depth; k++) {
        if (hipHostMalloc(&r.pinned[k], r.bytes, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&r.copied[k], hipEventDisableTiming) != hipSuccess) {
            snprintf(ctx->err, sizeof(ctx->err), "pagk_sequence_results_create: no pinned result block of %zu bytes", r.bytes);
            seq_results_free(*q);
            return PAGK_E_NOMEM;
        }
        memset(r.pinned[k], 0, r.bytes);
        r.frame_of[k] = -1;
    }
    // (state of its own, which pagk_selftest_fill_workspaces leaves alone: the padding of the record stays zero)
    if (hipMemsetAsync(b.ptr, 0, lay.total, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        seq_results_free(*q);
        snprintf(ctx->err, sizeof(ctx->err), "pagk_sequence_results_create: the block could not be cleared");
        return PAGK_E_HIP;
    }
    r.depth = depth;
    return PAGK_OK;
}

// the block of `frame`, or -1 with the reason in ctx->err
static int results_block(pagk_ctx *ctx, SeqState *q, const char *what, int32_t frame)
{
    const SeqState::Results &r = q->res;
    if (!r.depth) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: the sequence has no result ring (pagk_sequence_results_create)", what);
        return -1;
    }
    const int submitted = q->started ? q->frames : 0;
    if (frame < 0 || frame >= submitted || frame < submitted - r.depth || r.frame_of[frame % r.depth] != frame) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: frame %d is outside the ring (%d frames handed in, depth %d)", what, frame, submitted,
                 r.depth);
        return -1;
    }
    return frame % r.depth;
}

int pagk_sequence_fetch(pagk_ctx *ctx, int32_t frame, pagk_sequence_result *result)
{
    SeqState *q = seq_of(ctx, "pagk_sequence_fetch");
    if (!q || !result) return PAGK_E_ARG;
    const int b = results_block(ctx, q, "pagk_sequence_fetch", frame);
    if (b < 0) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(q->res.copied[b]));   // this frame's copy only, never the stream
    const uint8_t *base = static_cast<const uint8_t *>(q->res.pinned[b]);
    int64_t off[kResultsParts + 1];
    results_layout(q->p.cap, off);
    ResultsHeader h;
    memcpy(&h, base + off[RES_HEADER], sizeof h);
    memset(result, 0, sizeof *result);
    result->frame = h.frame, result->cap = h.cap, result->n_live = h.n_live, result->n_new = h.n_new;
    result->next_id = h.next_id, result->t = h.t;
    result->state = reinterpret_cast<const int32_t *>(base + off[RES_STATE]);
    result->info = reinterpret_cast<const int32_t *>(base + off[RES_INFO]);
    result->keys = reinterpret_cast<const float *>(base + off[RES_KEYS]);
    result->keys_un = reinterpret_cast<const float *>(base + off[RES_KEYS_UN]);
    result->keys_normal = reinterpret_cast<const float *>(base + off[RES_KEYS_NORMAL]);
    result->index_in_last = reinterpret_cast<const int32_t *>(base + off[RES_INDEX]);
    result->live = base + off[RES_LIVE];
    result->track_id = reinterpret_cast<const int64_t *>(base + off[RES_TRACK_ID]);
    result->age = reinterpret_cast<const int32_t *>(base + off[RES_AGE]);
    result->velocity = reinterpret_cast<const float *>(base + off[RES_VELOCITY]);
    result->status = base + off[RES_STATUS];
    result->pt_predict = reinterpret_cast<const float *>(base + off[RES_PT_PREDICT]);
    result->pt_predict_un = reinterpret_cast<const float *>(base + off[RES_PT_PREDICT_UN]);
    result->err = reinterpret_cast<const float *>(base + off[RES_ERR]);
    return lv_check(ctx);
}

int pagk_sequence_poll(pagk_ctx *ctx, int32_t frame)
{
    SeqState *q = seq_of(ctx, "pagk_sequence_poll");
    if (!q) return PAGK_E_ARG;
    const int b = results_block(ctx, q, "pagk_sequence_poll", frame);
    if (b < 0) return PAGK_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const hipError_t e = hipEventQuery(q->res.copied[b]);
    if (e == hipErrorNotReady) return 0;
    HIPCHK(ctx, e);
    return 1;
}

// ---- the sequence group: k cameras stepped together (Examples/Demo/RealSenseD435i.cpp:199-321, one loop per camera) -----------
namespace {

// the group `lead` leads, or nullptr with the reason in lead->err
GroupState *group_of(pagk_ctx *lead, const char *what)
{
    if (!lead) return nullptr;
    if (lead->capturing) {
        snprintf(lead->err, sizeof(lead->err), "%s between pagk_graph_begin and pagk_graph_end: the group captures its own graphs", what);
        return nullptr;
    }
    if (!lead->group || lead->group->members[0] != lead) {
        snprintf(lead->err, sizeof(lead->err), "%s: the context leads no sequence group (pagk_sequence_group_create)", what);
        return nullptr;
    }
    return lead->group;
}

// the group of a call of the plain (`sensor` false) or the sensor form; the other kind is refused with a text
GroupState *group_of_kind(pagk_ctx *lead, const char *what, bool sensor)
{
    GroupState *g = group_of(lead, what);
    if (g && g->sensor != sensor) {
        snprintf(lead->err, sizeof(lead->err), "%s: the group is %s", what,
                 g->sensor ? "one of sensor sequences (pagk_sequence_group_start_sensor, pagk_sequence_group_step_sensor)"
                           : "one of plain sequences (pagk_sequence_group_start, pagk_sequence_group_step)");
        return nullptr;
    }
    return g;
}

// While a group step is issued every member works on the lead's stream: the batched calls then have nothing to order
// between streams (no event crosses into a capture), and what falls back to k launches lands in the same chain.
struct GroupStreams {
    explicit GroupStreams(GroupState &g) : g_(g)
    {
        for (pagk_ctx *c : g.members) saved_.push_back(c->stream), c->stream = g.members[0]->stream;
    }
    ~GroupStreams()
    {
        for (size_t j = 0; j < g_.members.size(); j++) g_.members[j]->stream = saved_[j];
    }
    GroupStreams(const GroupStreams &) = delete;
    GroupStreams &operator=(const GroupStreams &) = delete;
    GroupState &g_;
    std::vector<hipStream_t> saved_;
};

GroupState::Held group_held(pagk_ctx *c)
{
    const DevBuf &hint = c->buf[pagk_ctx::PRIO_HINT];
    return {c->buf[pagk_ctx::FIT].ptr, c->buf[pagk_ctx::HAND].ptr, hint.ptr, hint.bytes, c->buf[pagk_ctx::FAST].ptr,
            c->buf[pagk_ctx::RECT_ENTRIES].ptr, {c->slots[0].u8[0], c->slots[1].u8[0]}, c->buf[pagk_ctx::SEQ].ptr,
            c->rect_w, c->rect_h, c->rect_wp, c->buf[pagk_ctx::RESULTS].ptr, c->buf[pagk_ctx::SEQ].ptr,
            {c->buf[pagk_ctx::LK_PYR].ptr, c->buf[pagk_ctx::LK_PYR + 1].ptr},
            {c->buf[pagk_ctx::LK_PYR].bytes, c->buf[pagk_ctx::LK_PYR + 1].bytes}};
}

bool group_held_equal(const GroupState::Held &a, const GroupState::Held &b, bool sensor, bool rings, bool lk)
{
    if (a.fit != b.fit || a.hand != b.hand || a.hint != b.hint || a.hint_bytes != b.hint_bytes) return false;
    if (lk && (a.lk_pyr[0] != b.lk_pyr[0] || a.lk_pyr[1] != b.lk_pyr[1] || a.lk_pyr_bytes[0] != b.lk_pyr_bytes[0] ||
               a.lk_pyr_bytes[1] != b.lk_pyr_bytes[1] || a.level0[0] != b.level0[0] || a.level0[1] != b.level0[1] ||
               a.seq != b.seq))
        return false;
    if (rings && (a.results != b.results || a.results_seq != b.results_seq)) return false;
    return !sensor || (a.fast == b.fast && a.entries == b.entries && a.level0[0] == b.level0[0] && a.level0[1] == b.level0[1] &&
                       a.seq == b.seq && a.rect_w == b.rect_w && a.rect_h == b.rect_h && a.rect_wp == b.rect_wp);
}

// the FAST grid and workspace of a detecting member, as handover_launch takes them (reserved by the member's own first step)
int group_fast(pagk_ctx *ctx, const pagk_sequence_params &p, FastGrid *g, FastWs *fws, int32_t *n_features)
{
    if (!fast_grid(p.width, p.height, g)) return PAGK_E_ARG;
    *n_features = p.fast.n_features ? p.fast.n_features : p.target_n;
    return *n_features < 1 ? PAGK_E_ARG : fast_workspace(ctx, *g, *n_features, fws);
}

// Camera j's record of parity c: the arguments its own launches of seq_issue would carry.
int group_record(pagk_ctx *ctx, int c, GroupRec *out)
{
    SeqState &q = *ctx->seq;
    const pagk_sequence_params &p = q.p;
    const SeqState::KeySet &ref = q.set[1 - c], &dst = q.set[c];
    GroupRec r;
    memset(&r, 0, sizeof r);
    r.predict = gyro_predict_args(&p.track, p.width, p.height, nullptr, nullptr, q.rot, p.cap, ref.keys_un, q.pu, q.pd, q.st_in, q.aff,
                                  ref.live);
    r.n = p.cap, r.half_patch = p.track.half_patch;
    r.pf_status_pm = q.status, r.pf_pix_err = q.pix_err, r.pf_dist_pred = q.dist_pred, r.pf_pt_pm = q.pt_dist, r.pf_pt_pm_un = q.pt_un;
    r.pf_status_out = q.st, r.pf_pt_predict = q.pp, r.pf_pt_predict_un = q.ppu, r.pf_kept = q.kept, r.pf_thresholds = q.th;
    if (p.validate) {   // pagk_geometry_validation_device(ref.keys_un, q.ppu, q.st, sigma, q.cnt, q.score)
        FitWs w;
        int rc = fit_workspace(ctx, p.cap, p.fit.iters_H + p.fit.iters_F, &w);
        if (rc) return rc;
        r.fit_pts1 = ref.keys_un, r.fit_pts2 = q.ppu, r.fit_status = q.st;
        r.fit_p1 = w.p1, r.fit_p2 = w.p2, r.fit_idx = w.idx;
        r.fit = fit_args(&p.fit, w, w.models, w.info, nullptr, nullptr, nullptr);
        r.sigma = p.sigma, r.inl_H = w.inl_H, r.inl_F = w.inl_F, r.scores = w.scores;
        r.val_cnt = q.cnt, r.val_score = q.score;
    }
    // pagk_frame_handover_device(q.st, q.pp, q.ppu, the list in the input block, key set c, the context's own mask, q.state)
    const DevBuf &hand = ctx->buf[pagk_ctx::HAND];
    r.mask_bytes = (int64_t)p.width * p.height;
    if (!hand.ptr || hand.bytes < (size_t)r.mask_bytes) {
        snprintf(ctx->err, sizeof(ctx->err), "the hand-over's mask has not been reserved");
        return PAGK_E_ARG;
    }
    handover_fill_args(&r.hand, &p.track, p.width, p.height, p.cap, p.target_n, p.new_point_threshold);
    if (p.detector == 2) {   // (a sensor group's) the detector's list, as handover_launch fills it for one camera
        FastGrid g;
        FastWs fws;
        int32_t n_features;
        int rc = group_fast(ctx, p, &g, &fws, &n_features);
        if (rc) return rc;
        r.hand.cand_cap = fws.out_bound, r.hand.n_cand = q.info, r.hand.cand_un = fws.cand;
    } else {
        r.hand.cand_cap = p.cand_cap;
        r.hand.n_cand = reinterpret_cast<const int32_t *>(q.in + q.off_ncand);
        r.hand.cand_un = reinterpret_cast<const float *>(q.in + q.off_cand);
    }
    r.hand.status = q.st, r.hand.pt_predict = q.pp, r.hand.pt_predict_un = q.ppu;
    r.hand.keys = dst.keys, r.hand.keys_un = dst.keys_un, r.hand.keys_normal = dst.keys_normal;
    r.hand.index_in_last = dst.index_in_last, r.hand.live = dst.live, r.hand.mask = static_cast<uint8_t *>(hand.ptr);
    r.hand.state = q.state;
    handover_hint_args(ctx, &r.hand);
    *out = r;
    return PAGK_OK;
}

// Camera j's record of parity c of the stages a sensor step adds: the arguments its own launches of seq_issue would carry
// (rect_into_slot, k_gyro_integrate, handover_launch's plan and detector, k_flow_velocity).
int rig_record(pagk_ctx *ctx, int c, RigRec *out)
{
    SeqState &q = *ctx->seq;
    const pagk_sequence_params &p = q.p;
    RigRec r;
    memset(&r, 0, sizeof r);
    const FrameSlot &s = ctx->slots[c];
    if (q.s.raw) {
        if (!ctx->buf[pagk_ctx::RECT_ENTRIES].ptr || ctx->rect_w != p.width || ctx->rect_h != p.height || !s.u8[0] || s.w != p.width ||
            s.h != p.height) {
            snprintf(ctx->err, sizeof(ctx->err), "the sequence is %d x %d, the maps are now %d x %d (pagk_rectify_set_maps)", p.width,
                     p.height, ctx->rect_w, ctx->rect_h);
            return PAGK_E_ARG;
        }
        r.rect = rect_args(ctx, &q.s.rectify, q.in, q.s.src_width, q.s.src_height, (int64_t)q.row_bytes, s.u8[0]);
    }
    r.gyro = seq_gyro_args(q);
    if (p.detector == 2) {
        FastGrid g;
        FastWs fws;
        int32_t n_features;
        int rc = group_fast(ctx, p, &g, &fws, &n_features);
        if (rc) return rc;
        r.cap = p.cap, r.target_n = p.target_n, r.new_point_threshold = p.new_point_threshold;
        r.plan_status = q.st, r.plan_state = q.state, r.plan_ctl = fws.ctl;
        // level 0 as the pyramid of this parity reads it: the rectified slot, or the gray frame in the input block
        const uint8_t *img0 = q.s.raw ? s.u8[0] : q.in;
        r.cells = fast_cell_args(&p.fast, img0, p.width, g, fws, fws.ctl + kFastCtlSkip);
        r.n_cells = fws.n_cells, r.cell_off = fws.cell_off, r.ctl = fws.ctl, r.kxy = fws.kxy, r.kscore = fws.kscore;
        r.tree = fast_tree_args(n_features, g, nullptr, fws.out_bound, fws.cand, nullptr, q.info, fws.ctl + kFastCtlSkip, fws);
    }
    r.flow = seq_flow_args(q, c);
    *out = r;
    return PAGK_OK;
}

// Camera j's record of parity c of the Lucas-Kanade stages: the arguments its own launches of seq_frame and lk_flow_slots
// would carry (the copy of level 0, lk_pyramid_slot's pyrDown launches of slot c, k_lk_flow of slots 1 - c and c).
int lk_record(pagk_ctx *ctx, int c, LkGroupRec *out)
{
    SeqState &q = *ctx->seq;
    const pagk_sequence_params &p = q.p;
    const SeqState::KeySet &ref = q.set[1 - c];
    LkGroupRec r;
    memset(&r, 0, sizeof r);
    const bool raw = q.sensor && q.s.raw;
    const FrameSlot &s = ctx->slots[c];
    // level 0 of slot c as seq_frame leaves it: the rectified slot, or the parity's copy of the frame
    if (!lk_slot_ok(s) || s.w != p.width || s.h != p.height || s.pitch0 != p.width || s.img0 != (raw ? s.u8[0] : q.img[c])) {
        snprintf(ctx->err, sizeof(ctx->err), "frame slot %d no longer holds the sequence's frame", c);
        return PAGK_E_ARG;
    }
    const bool init = p.lk_initial_flow != 0;   // (as seq_issue hands them to lk_flow_slots)
    int rc = lk_flow_args(ctx, &p.lk, &p.track, 1 - c, c, p.cap, ref.keys_un, init ? q.pu : nullptr, init ? q.st_in : ref.live, q.state,
                          q.ppu, q.pp, q.st, nullptr, q.lk_err, nullptr, q.lk_info, &r.flow);
    if (rc) return rc;
    int lw[kLkMaxLevels], lh[kLkMaxLevels];
    const int top = lk_levels(s.w, s.h, &p.lk, lw, lh);
    const Layout<kLkMaxLevels> lay = lk_layout(lw, lh, top);
    const DevBuf &pyr = ctx->buf[pagk_ctx::LK_PYR + c];
    if (top < 0 || top != r.flow.t.top || (top > 0 && (!pyr.ptr || pyr.bytes < lay.total))) return PAGK_E_ARG;
    for (int l = 1; l <= top; l++) r.pyr[l - 1] = lk_pyr_args(s, lay, pyr.ptr, lw, lh, l);
    if (!raw) r.copy_src = q.in, r.copy_dst = q.img[c], r.copy_bytes = (long long)p.width * p.height;
    *out = r;
    return PAGK_OK;
}

// The tables, once per group: after the member-by-member step every buffer a record points into has its final size.
int group_table(pagk_ctx *lead, GroupState &g)
{
    const int k = (int)g.members.size();
    if (g.table_built) {
        for (int j = 0; j < k; j++) {
            if (!group_held_equal(group_held(g.members[j]), g.held[j], g.sensor, g.rings, g.lk)) {
                snprintf(lead->err, sizeof(lead->err), "a workspace of member %d moved under the group's table (a call outside the group made it "
                         "grow): destroy the group (pagk_sequence_group_destroy)", j);
                return PAGK_E_ARG;
            }
        }
        return PAGK_OK;
    }
    try {
        std::vector<GroupRec> host((size_t)2 * k);
        std::vector<RigRec> rig(g.sensor ? (size_t)2 * k : 0);
        std::vector<ResultsArgs> packs(g.rings ? (size_t)2 * k : 0);
        std::vector<LkGroupRec> lks(g.lk ? (size_t)2 * k : 0);
        for (int c = 0; c < 2; c++)
            for (int j = 0; j < k; j++) {
                pagk_ctx *m = g.members[j];
                int rc = group_record(m, c, &host[(size_t)c * k + j]);
                if (!rc && g.sensor) rc = rig_record(m, c, &rig[(size_t)c * k + j]);
                if (!rc && g.rings) packs[(size_t)c * k + j] = seq_results_args(*m->seq, c);
                if (!rc && g.lk) rc = lk_record(m, c, &lks[(size_t)c * k + j]);
                if (rc) {
                    if (m != lead) snprintf(lead->err, sizeof(lead->err), "camera %d: %s", j, m->err);
                    return rc;
                }
            }
        g.held.clear();
        for (int j = 0; j < k; j++) g.held.push_back(group_held(g.members[j]));
        if (g.sensor) {
            for (int j = 1; j < k; j++)   // (one launch of the rectification: one grid, one row pitch of the entries)
                if (g.held[j].rect_wp != g.held[0].rect_wp) {
                    snprintf(lead->err, sizeof(lead->err), "camera %d's map entries are laid out differently from the lead's", j);
                    return PAGK_E_ARG;
                }
            g.n_cells = rig[0].n_cells;   // (the detector's grid is the size's: one for the group)
            HIPCHK(lead, hipMemcpyAsync(lead->buf[pagk_ctx::GROUP_SENSOR].ptr, rig.data(), rig.size() * sizeof(RigRec),
                                        hipMemcpyHostToDevice, lead->stream));
        }
        if (g.lk)
            HIPCHK(lead, hipMemcpyAsync(lead->buf[pagk_ctx::GROUP_LK].ptr, lks.data(), lks.size() * sizeof(LkGroupRec),
                                        hipMemcpyHostToDevice, lead->stream));
        if (g.rings)
            HIPCHK(lead, hipMemcpyAsync(lead->buf[pagk_ctx::GROUP_RESULTS].ptr, packs.data(), packs.size() * sizeof(ResultsArgs),
                                        hipMemcpyHostToDevice, lead->stream));
        HIPCHK(lead, hipMemcpyAsync(lead->buf[pagk_ctx::GROUP].ptr, host.data(), host.size() * sizeof(GroupRec), hipMemcpyHostToDevice,
                                    lead->stream));
        HIPCHK(lead, hipStreamSynchronize(lead->stream));   // (host, rig, packs and lks are locals)
    } catch (const std::bad_alloc &) {
        return PAGK_E_NOMEM;
    }
    g.table_built = true;
    return PAGK_OK;
}

// The stage launches of a frame of parity c for all cameras, on the lead's stream (which every member works on: GroupStreams).
int group_issue(pagk_ctx *lead, GroupState &g, int c)
{
    const int k = (int)g.members.size();
    const pagk_sequence_params &p = lead->seq->p;
    pagk_ctx *const *ctxs = g.members.data();
    constexpr int K = pagk_ctx::kBatchMaxStreams;
    int32_t slot_cur[K], slot_ref[K], width[K], height[K], n[K];
    int64_t step[K];
    const void *data[K];
    const float *pt_ref[K], *pt_init[K], *affine[K];
    const uint8_t *status_in[K];
    pagk_outputs out[K];
    // (Lucas-Kanade starts from the prediction when lk_initial_flow says so, as seq_issue decides)
    const bool predicts = g.lk ? p.lk_initial_flow != 0 : p.track.has_gyro_predict_initial != 0;
    const pagk_sequence_sensor &sn = lead->seq->s;
    const bool raw = g.sensor && sn.raw;
    for (int j = 0; j < k; j++) {
        const SeqState &q = *ctxs[j]->seq;
        const SeqState::KeySet &ref = q.set[1 - c];
        slot_cur[j] = c, slot_ref[j] = 1 - c, width[j] = p.width, height[j] = p.height, step[j] = p.width, n[j] = p.cap;
        // raw frames: the slot's own level 0, in place, as rect_into_slot builds one camera's pyramid
        // (Lucas-Kanade reads level 0 in place for a whole pair: the parity's own copy of the frame, as seq_frame makes it)
        data[j] = raw ? ctxs[j]->slots[c].u8[0] : g.lk ? q.img[c] : q.in;
        pt_ref[j] = ref.keys_un, affine[j] = q.aff;
        pt_init[j] = predicts ? q.pu : ref.keys_un;              // (as seq_issue hands them to pagk_track_device)
        status_in[j] = predicts ? q.st_in : ref.live;
        out[j] = pagk_outputs{q.pt_un, q.pt_dist, q.status, q.pix_err, q.dist_pred, nullptr, nullptr};
    }
    const GroupRec *table = static_cast<const GroupRec *>(lead->buf[pagk_ctx::GROUP].ptr) + (size_t)c * k;
    const unsigned kk = (unsigned)k;
    hipStream_t s = lead->stream;
    const RigRec *rig = g.sensor ? static_cast<const RigRec *>(lead->buf[pagk_ctx::GROUP_SENSOR].ptr) + (size_t)c * k : nullptr;
    if (raw) {   // every camera's raw frame through its own maps into its own slot (rect_launch's grid and instantiation)
        const long long threads = (long long)(lead->rect_wp >> 2) * lead->rect_h;
        const dim3 grd((unsigned)((threads + 255) / 256), kk), blk(256);
        const bool pair = sn.src_width >= 2;
        if (sn.rectify.channels == 1) {
            if (pair) hipLaunchKernelGGL((k_rig_rectify<1, true>), grd, blk, 0, s, rig);
            else hipLaunchKernelGGL((k_rig_rectify<1, false>), grd, blk, 0, s, rig);
        } else if (sn.rectify.channels == 3) {
            if (pair) hipLaunchKernelGGL((k_rig_rectify<3, true>), grd, blk, 0, s, rig);
            else hipLaunchKernelGGL((k_rig_rectify<3, false>), grd, blk, 0, s, rig);
        } else {
            if (pair) hipLaunchKernelGGL((k_rig_rectify<4, true>), grd, blk, 0, s, rig);
            else hipLaunchKernelGGL((k_rig_rectify<4, false>), grd, blk, 0, s, rig);
        }
        HIPCHK(lead, hipGetLastError());
    }
    const LkGroupRec *lks = g.lk ? static_cast<const LkGroupRec *>(lead->buf[pagk_ctx::GROUP_LK].ptr) + (size_t)c * k : nullptr;
    if (g.lk && !raw) {   // every camera's frame into its parity copy of level 0 (seq_frame's copy)
        const int64_t px = (int64_t)p.width * p.height;
        hipLaunchKernelGGL(k_group_lk_copy, dim3((unsigned)((px + 4095) / 4096), kk), dim3(256), 0, s, lks);
        HIPCHK(lead, hipGetLastError());
    }
    int rc = pagk_frame_set_device_batch(ctxs, k, slot_cur, data, width, height, step, p.track.pyramids);
    if (rc) return rc;
    if (g.lk) {   // lk_pyramid_slot's launches, one per level for the rig: the level sizes are the group's
        int lw[kLkMaxLevels], lh[kLkMaxLevels];
        const int top = lk_levels(p.width, p.height, &p.lk, lw, lh);
        for (int l = 1; l <= top; l++)
            hipLaunchKernelGGL(k_group_lk_pyrdown, dim3((unsigned)((lw[l] + 63) / 64), (unsigned)((lh[l] + 3) / 4), kk), dim3(256), 0, s,
                               lks, l);
        HIPCHK(lead, hipGetLastError());
    }
    if (g.sensor) hipLaunchKernelGGL(k_rig_gyro_integrate, dim3(1, kk), dim3(64), 0, s, rig);   // (always, as seq_issue does)
    if (predicts) hipLaunchKernelGGL(k_group_gyro_predict, dim3((unsigned)((p.cap + 255) / 256), kk), dim3(256), 0, s, table);
    HIPCHK(lead, hipGetLastError());
    if (g.lk) {   // lk_flow_slots' clear of the info words and its launch; type 0 never enters Step 3
        hipLaunchKernelGGL(k_group_lk_clear, dim3(1, kk), dim3(64), 0, s, lks);
        hipLaunchKernelGGL(lk_group_flow_kernel(2 * p.lk.half_patch + 1), dim3((unsigned)((p.cap + 3) / 4), kk), dim3(256), 0, s, lks);
    } else {
        if ((rc = pagk_track_device_batch(ctxs, k, &p.track, slot_ref, slot_cur, n, pt_ref, pt_init, affine, status_in, out))) return rc;
        hipLaunchKernelGGL(k_group_post_filter, dim3(1, kk), dim3(1024), 0, s, table);
    }
    HIPCHK(lead, hipGetLastError());
    if (p.validate) {
        hipLaunchKernelGGL(k_group_fit_compact, dim3(1, kk), dim3(1024), 0, s, table);
        hipLaunchKernelGGL(k_group_fit_hyp, dim3((unsigned)fit_hyp_blocks(&p.fit), kk), dim3(256), 0, s, table);
        hipLaunchKernelGGL(k_group_fit_refit, dim3(2, kk), dim3(256), 0, s, table);
        hipLaunchKernelGGL(k_group_scores_fit, dim3(2, kk), dim3(256), 0, s, table);
        hipLaunchKernelGGL(k_group_fit_select, dim3(1, kk), dim3(1024), 0, s, table);
        HIPCHK(lead, hipGetLastError());
    }
    const int64_t bytes = (int64_t)p.width * p.height;
    hipLaunchKernelGGL(k_group_handover_fill, dim3((unsigned)((bytes + 4095) / 4096), kk), dim3(256), 0, s, table);
    hipLaunchKernelGGL(k_group_handover_holes, dim3((unsigned)(((int64_t)p.cap * 14 + 255) / 256), kk), dim3(256), 0, s, table);
    if (p.detector == 2) {   // the plan and the detector in front of the keys, every camera under its own skip word
        const unsigned n_cells = (unsigned)g.n_cells;
        hipLaunchKernelGGL(k_rig_handover_plan, dim3(1, kk), dim3(1024), 0, s, rig);
        hipLaunchKernelGGL(k_rig_fast_cells, dim3(n_cells, kk), dim3(256), 0, s, rig);
        hipLaunchKernelGGL(k_rig_fast_offsets, dim3(1, kk), dim3(1024), 0, s, rig);
        hipLaunchKernelGGL(k_rig_fast_gather, dim3(n_cells, kk), dim3(256), 0, s, rig);
        hipLaunchKernelGGL(k_rig_fast_tree, dim3(1, kk), dim3(1024), 0, s, rig);
        HIPCHK(lead, hipGetLastError());
    }
    hipLaunchKernelGGL(k_group_handover_keys, dim3(1, kk), dim3(1024), 0, s, table);
    if (g.sensor && sn.flow_velocity)
        hipLaunchKernelGGL(k_rig_flow_velocity, dim3((unsigned)((p.cap + 255) / 256), kk), dim3(256), 0, s, rig);
    if (g.rings) {   // the last launch, as in seq_issue: every camera's record
        const ResultsArgs *packs = static_cast<const ResultsArgs *>(lead->buf[pagk_ctx::GROUP_RESULTS].ptr) + (size_t)c * k;
        hipLaunchKernelGGL(k_group_results_pack, dim3(results_blocks(p.cap), kk), dim3(1024), 0, s, packs);
    }
    HIPCHK(lead, hipGetLastError());
    return PAGK_OK;
}

// every camera's frame and list as pagk_sequence_start / pagk_sequence_step would check them
int group_inputs_check(pagk_ctx *lead, const GroupState &g, const char *what, const pagk_image *frames, const float *const *cand,
                       const int32_t *n_cand)
{
    const bool lists = g.members[0]->seq->p.detector == 0;   // (a detecting group takes no lists, as a detecting sequence)
    if (!frames || (lists ? !cand || !n_cand : cand || n_cand)) return PAGK_E_ARG;
    for (size_t j = 0; j < g.members.size(); j++)
        if (seq_inputs_check(*g.members[j]->seq, &frames[j], lists ? cand[j] : nullptr, lists ? n_cand[j] : 0)) {
            snprintf(lead->err, sizeof(lead->err), "%s: camera %zu's frame or candidate list is refused", what, j);
            return PAGK_E_ARG;
        }
    return PAGK_OK;
}

void group_drop(GroupState *g)
{
    pagk_ctx *lead = g->members[0];
    (void)hipSetDevice(lead->device);
    for (pagk_ctx *m : g->members) (void)hipStreamSynchronize(m->stream);
    for (int &id : g->graph) {
        if (id >= 0) (void)pagk_graph_destroy(lead, id);
        id = -1;
    }
    (void)release(lead, lead->buf[pagk_ctx::GROUP]);
    if (g->rings) (void)release(lead, lead->buf[pagk_ctx::GROUP_RESULTS]);
    if (g->sensor) (void)release(lead, lead->buf[pagk_ctx::GROUP_SENSOR]);
    if (g->lk) (void)release(lead, lead->buf[pagk_ctx::GROUP_LK]);
    for (pagk_ctx *m : g->members) m->group = nullptr;
    delete g;
}

}  // namespace

int pagk_sequence_group_check(const pagk_sequence_params *p)
{
    int rc = pagk_sequence_params_check(p);
    if (rc) return rc;
    return p->tracker == PAGK_SEQ_PATCHMATCH && p->detector == 0 ? PAGK_OK : PAGK_E_ARG;
}

// pagk_sequence_group_create (`sensor` false), pagk_sequence_group_create_sensor and pagk_sequence_group_create_lk (`lk`: the
// kind, plain or sensor, is the lead's, and every member's): one list of refusals, one GroupState
static int group_create(pagk_ctx *const *ctxs, int32_t k, bool sensor, const char *what, bool lk = false)
{
    if (!ctxs || !ctxs[0]) return PAGK_E_ARG;
    pagk_ctx *lead = ctxs[0];
    auto refuse = [&](const char *why, int j) {
        snprintf(lead->err, sizeof(lead->err), "%s: context %d %s", what, j, why);
        return PAGK_E_ARG;
    };
    if (k < 1 || k > pagk_ctx::kBatchMaxStreams) {
        snprintf(lead->err, sizeof(lead->err), "%s: k = %d is outside 1 .. %d", what, k, pagk_ctx::kBatchMaxStreams);
        return PAGK_E_ARG;
    }
    for (int j = 0; j < k; j++) {
        pagk_ctx *c = ctxs[j];
        if (!c) return refuse("is NULL", j);
        if (c->device != lead->device) return refuse("lives on another device than the lead", j);
        for (int i = 0; i < j; i++)
            if (ctxs[i] == c) return refuse("is listed twice", j);
        if (!c->seq) return refuse("has no sequence (pagk_sequence_create)", j);
        if (lk && j == 0) sensor = c->seq->sensor;
        if (lk && c->seq->sensor != sensor)
            return refuse("mixes plain and sensor sequences: the members of a Lucas-Kanade group are all of the lead's kind", j);
        if (!sensor && c->seq->sensor)
            return refuse("holds a sensor sequence: out of scope of the group (pagk_sequence_group_create_sensor)", j);
        if (sensor && !c->seq->sensor) return refuse("holds a plain sequence (pagk_sequence_group_create)", j);
        if (c->group) return refuse("is a member of a group already", j);
        if (in_capture(c)) return refuse("is inside a graph capture", j);
        if (memcmp(&c->seq->p, &lead->seq->p, sizeof(pagk_sequence_params)) != 0)
            return refuse("is configured differently from the lead: the parameters of a group are byte-equal", j);
        if (c->seq->res.depth != lead->seq->res.depth)
            return refuse("differs from the lead in its result ring: all members have one of the same depth, or none has", j);
        if (sensor) {   // everything of the sensor block but Rbc: every camera has its own extrinsic rotation
            pagk_sequence_sensor a = c->seq->s;
            memcpy(a.Rbc, lead->seq->s.Rbc, sizeof a.Rbc);
            if (memcmp(&a, &lead->seq->s, sizeof a) != 0)
                return refuse("is configured differently from the lead: the sensor blocks of a group differ in Rbc only", j);
        }
    }
    if (lk) {
        if (pagk_sequence_group_lk_check(&lead->seq->p, sensor ? &lead->seq->s : nullptr)) {
            snprintf(lead->err, sizeof(lead->err), "%s: the group serves Lucas-Kanade (tracker type 0) with %s", what,
                     sensor ? "the caller's candidate lists or the FAST detector (pagk_sequence_group_lk_check)"
                            : "the caller's candidate lists (pagk_sequence_group_lk_check)");
            return PAGK_E_ARG;
        }
    } else if (sensor ? pagk_sequence_group_sensor_check(&lead->seq->p, &lead->seq->s) : pagk_sequence_group_check(&lead->seq->p)) {
        snprintf(lead->err, sizeof(lead->err), "%s: the group serves PatchMatch with %s", what,
                 sensor ? "the caller's candidate lists or the FAST detector (pagk_sequence_group_sensor_check)"
                        : "the caller's candidate lists (pagk_sequence_group_check)");
        return PAGK_E_ARG;
    }
    HIPCHK(lead, hipSetDevice(lead->device));
    // (no graph of the group exists yet: whatever graphs the lead holds do not point into the table)
    int rc = reserve(lead, lead->buf[pagk_ctx::GROUP], align_up((size_t)2 * k * sizeof(GroupRec), kPartAlign), NOT_IN_CAPTURE,
                     "the sequence group's table");
    if (rc) return rc;
    if (sensor && (rc = reserve(lead, lead->buf[pagk_ctx::GROUP_SENSOR], align_up((size_t)2 * k * sizeof(RigRec), kPartAlign),
                                NOT_IN_CAPTURE, "the sensor group's table")))
        return rc;
    if (lk && (rc = reserve(lead, lead->buf[pagk_ctx::GROUP_LK], align_up((size_t)2 * k * sizeof(LkGroupRec), kPartAlign),
                            NOT_IN_CAPTURE, "the Lucas-Kanade group's table")))
        return rc;
    const bool rings = lead->seq->res.depth != 0;
    if (rings && (rc = reserve(lead, lead->buf[pagk_ctx::GROUP_RESULTS], align_up((size_t)2 * k * sizeof(ResultsArgs), kPartAlign),
                               NOT_IN_CAPTURE, "the group's table of result records")))
        return rc;
    GroupState *g = new (std::nothrow) GroupState();
    if (!g) return PAGK_E_NOMEM;
    g->sensor = sensor, g->rings = rings, g->lk = lk;
    try {
        g->members.assign(ctxs, ctxs + k);
    } catch (const std::bad_alloc &) {
        delete g;
        return PAGK_E_NOMEM;
    }
    for (int j = 0; j < k; j++) ctxs[j]->group = g;
    return PAGK_OK;
}

int pagk_sequence_group_create(pagk_ctx *const *ctxs, int32_t k) { return group_create(ctxs, k, false, "pagk_sequence_group_create"); }

int pagk_sequence_group_sensor_check(const pagk_sequence_params *p, const pagk_sequence_sensor *s)
{
    int rc = pagk_sequence_params_check(p);
    if (rc || (rc = pagk_sequence_sensor_check(s))) return rc;
    return p->tracker == PAGK_SEQ_PATCHMATCH && (p->detector == 0 || p->detector == 2) ? PAGK_OK : PAGK_E_ARG;
}

int pagk_sequence_group_create_sensor(pagk_ctx *const *ctxs, int32_t k)
{
    return group_create(ctxs, k, true, "pagk_sequence_group_create_sensor");
}

int pagk_sequence_group_lk_check(const pagk_sequence_params *p, const pagk_sequence_sensor *s)
{
    int rc = pagk_sequence_params_check(p);
    if (rc || (s && (rc = pagk_sequence_sensor_check(s)))) return rc;
    // the detectors whose batched kernels exist for the kind of group: the caller's lists, and FAST for sensor members
    return p->tracker == PAGK_SEQ_LK && (p->detector == 0 || (s && p->detector == 2)) ? PAGK_OK : PAGK_E_ARG;
}

int pagk_sequence_group_create_lk(pagk_ctx *const *ctxs, int32_t k)
{
    return group_create(ctxs, k, false, "pagk_sequence_group_create_lk", true);
}

int pagk_sequence_group_destroy(pagk_ctx *lead)
{
    GroupState *g = group_of(lead, "pagk_sequence_group_destroy");
    if (!g) return PAGK_E_ARG;
    group_drop(g);
    return PAGK_OK;
}

// pagk_sequence_group_start (t NULL) and pagk_sequence_group_start_sensor: k times the member's own start
static int group_start(pagk_ctx *lead, const char *what, bool sensor, const pagk_image *frames, const double *t,
                       const float *const *cand, const int32_t *n_cand)
{
    GroupState *g = group_of_kind(lead, what, sensor);
    if (!g || (sensor && !t) || group_inputs_check(lead, *g, what, frames, cand, n_cand)) return PAGK_E_ARG;
    const size_t k = g->members.size();
    for (size_t j = 0; sensor && j < k; j++)
        if (!std::isfinite(t[j])) {
            snprintf(lead->err, sizeof(lead->err), "%s: camera %zu's time stamp is not finite", what, j);
            return PAGK_E_ARG;
        }
    for (size_t j = 0; j < k; j++) {
        pagk_ctx *m = g->members[j];
        int rc = seq_start(m, m->seq, &frames[j], cand ? cand[j] : nullptr, n_cand ? n_cand[j] : 0, sensor ? t[j] : 0.0);
        if (rc) {
            if (m != lead) snprintf(lead->err, sizeof(lead->err), "camera %zu: %s", j, m->err);
            return rc;
        }
    }
    g->last_graph = false;
    return PAGK_OK;
}

int pagk_sequence_group_start(pagk_ctx *lead, const pagk_image *frames, const float *const *cand, const int32_t *n_cand)
{
    return group_start(lead, "pagk_sequence_group_start", false, frames, nullptr, cand, n_cand);
}

int pagk_sequence_group_start_sensor(pagk_ctx *lead, const pagk_image *raws, const double *t, const float *const *cand,
                                     const int32_t *n_cand)
{
    return group_start(lead, "pagk_sequence_group_start_sensor", true, raws, t, cand, n_cand);
}

// pagk_sequence_group_step (rot9, no windows) and pagk_sequence_group_step_sensor (windows, no rot9): one issue order
static int group_step(pagk_ctx *lead, const char *what, bool sensor, const pagk_image *frames, const float *rot9,
                      const pagk_imu_window *windows, const float *const *cand, const int32_t *n_cand, int32_t mode)
{
    GroupState *gp = group_of_kind(lead, what, sensor);
    if (!gp || (sensor && !windows) || group_inputs_check(lead, *gp, what, frames, cand, n_cand) ||
        (mode != PAGK_SEQ_GRAPH && mode != PAGK_SEQ_DIRECT))
        return PAGK_E_ARG;
    GroupState &g = *gp;
    const int k = (int)g.members.size();
    const pagk_sequence_params &p = lead->seq->p;
    for (int j = 0; j < k; j++) {
        const SeqState &q = *g.members[j]->seq;
        if (!q.started || q.frames != lead->seq->frames) {
            snprintf(lead->err, sizeof(lead->err), "%s: %s (pagk_sequence_group_start)", what,
                     q.started ? "the members do not stand at the same frame" : "a member has not been started");
            return PAGK_E_ARG;
        }
    }
    if (!sensor && (g.lk ? p.lk_initial_flow : p.track.has_gyro_predict_initial) && !rot9) {
        snprintf(lead->err, sizeof(lead->err), "%s: this tracker predicts: rot9 is required", what);
        return PAGK_E_ARG;
    }
    for (int j = 0; sensor && j < k; j++)   // every camera's window, on the host, before anything is enqueued
        if (seq_window_check(lead, *g.members[j]->seq, what, &windows[j])) {
            char text[sizeof lead->err];
            memcpy(text, lead->err, sizeof text);
            snprintf(lead->err, sizeof(lead->err), "camera %d: %.*s", j, (int)sizeof(text) - 16, text);
            return PAGK_E_ARG;
        }
    HIPCHK(lead, hipSetDevice(lead->device));
    const int c = lead->seq->frames & 1;
    int rc = PAGK_OK;
    if (g.members_done && (rc = group_table(lead, g))) return rc;   // (in front of everything that enqueues)
    // 1. what the members' streams have enqueued (reads, a step alone before the group was made) comes first
    for (int j = 1; j < k; j++)
        if (g.members[j]->stream != lead->stream) {
            HIPCHK(lead, hipEventRecord(g.members[j]->ev_batch, g.members[j]->stream));
            HIPCHK(lead, hipStreamWaitEvent(lead->stream, g.members[j]->ev_batch, 0));
        }
    {
        GroupStreams on_lead(g);
        // 2. the inputs: each member's ring, each member's fixed block
        for (int j = 0; j < k && !rc; j++) {
            pagk_ctx *m = g.members[j];
            rc = seq_feed(m, *m->seq, &frames[j], rot9 ? rot9 + 9 * j : nullptr, cand ? cand[j] : nullptr, n_cand ? n_cand[j] : 0,
                          sensor ? &windows[j] : nullptr);
            if (!rc && sensor) m->seq->t_last = windows[j].t_cur;
            if (rc && m != lead) snprintf(lead->err, sizeof(lead->err), "camera %d: %s", j, m->err);
        }
        if (rc) return rc;
        // 3. the stages
        bool replay = false;
        if (!g.members_done) {   // every member's own launches: its fit workspace, its mask, its hints get their size
            for (int j = 0; j < k; j++) {
                pagk_ctx *m = g.members[j];
                if ((rc = seq_issue(m, *m->seq, c))) {
                    if (m != lead) snprintf(lead->err, sizeof(lead->err), "camera %d: %s", j, m->err);
                    return rc;
                }
                m->seq->direct_done[c] = true;
            }
            g.members_done = true;
            g.direct_done[c] = true;
        } else if (mode == PAGK_SEQ_GRAPH && g.direct_done[c] && g.batched_done) {
            if (g.graph[c] < 0) {
                if ((rc = pagk_graph_begin(lead))) return rc;
                rc = group_issue(lead, g, c);
                int32_t id = -1;
                const int rc_end = pagk_graph_end(lead, &id);
                if (rc || rc_end) {
                    if (!rc_end && id >= 0) (void)pagk_graph_destroy(lead, id);
                    return rc ? rc : rc_end;
                }
                g.graph[c] = id;
            }
            if ((rc = pagk_graph_launch(lead, g.graph[c]))) return rc;
            replay = true;
        } else {   // also the first batched step, and the first step of each parity, in graph mode: allocations happen outside a capture
            if ((rc = group_issue(lead, g, c))) return rc;
            g.batched_done = true;
            g.direct_done[c] = true;
        }
        g.last_graph = replay;
        // behind the graph, in front of the event every member's stream waits for: every member's record into its own ring
        for (int j = 0; j < k; j++) {
            pagk_ctx *m = g.members[j];
            if ((rc = seq_results_post(m, *m->seq, m->seq->frames))) {
                if (m != lead) snprintf(lead->err, sizeof(lead->err), "camera %d: %s", j, m->err);
                return rc;
            }
        }
        for (pagk_ctx *m : g.members) {
            m->seq->frames++;
            m->seq->stepped = true;
            m->seq->last_graph = replay;
        }
    }
    // 4. a member's synchronous reads wait for its own stream: that stream sees the step
    bool others = false;
    for (int j = 1; j < k; j++) others = others || g.members[j]->stream != lead->stream;
    if (others) {
        HIPCHK(lead, hipEventRecord(lead->ev_batch, lead->stream));
        for (int j = 1; j < k; j++)
            if (g.members[j]->stream != lead->stream) HIPCHK(lead, hipStreamWaitEvent(g.members[j]->stream, lead->ev_batch, 0));
    }
    return PAGK_OK;
}

int pagk_sequence_group_step(pagk_ctx *lead, const pagk_image *frames, const float *rot9, const float *const *cand,
                             const int32_t *n_cand, int32_t mode)
{
    return group_step(lead, "pagk_sequence_group_step", false, frames, rot9, nullptr, cand, n_cand, mode);
}

int pagk_sequence_group_step_sensor(pagk_ctx *lead, const pagk_image *raws, const pagk_imu_window *windows, const float *const *cand,
                                    const int32_t *n_cand, int32_t mode)
{
    return group_step(lead, "pagk_sequence_group_step_sensor", true, raws, nullptr, windows, cand, n_cand, mode);
}

int pagk_sequence_group_status(pagk_ctx *lead, int32_t *words)
{
    GroupState *g = group_of(lead, "pagk_sequence_group_status");
    if (!g || !words) return PAGK_E_ARG;
    const SeqState &q = *lead->seq;
    words[0] = q.started ? q.frames : 0;
    words[1] = g->last_graph ? 1 : 0;
    words[2] = (g->graph[0] >= 0) + (g->graph[1] >= 0);
    words[3] = (int32_t)g->members.size();
    return PAGK_OK;
}

}  // extern "C"

#include "pagk_multi.h"
