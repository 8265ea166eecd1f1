// stream_graph_loop.cpp -- the loop of examples/stream_resident.cpp with nothing left on the host between two frame
// pairs: Step 3 (pagk_post_filter_device) and the hand-over of the survivors to the next pair
// (pagk_frame_handover_device) run on the device, every launch is sized by the fixed capacity, and a frame is ONE
// pagk_graph_launch.  Per new frame the host copies the image and nine rotation floats into fixed device buffers and
// replays  [pyramid -> pagk_gyro_predict_device_live -> pagk_track_device -> pagk_post_filter_device ->
// pagk_frame_handover_device];  the even and the odd frame (they differ in their frame slots and key-array sets) are
// two graphs, each captured after one direct run.
// The file's keypoints are the candidate list of the first-frame hand-over (target_n = their number; the mask is all
// ones, so all are taken in order); every later frame gets an empty candidate list and there is no geometry validation,
// so the program prints the lines of stream_resident: dead slots and the stable compaction leave every live feature and
// the ordered Step-3 sum as they are there.  Counts and points are read back only to print them.
//
// --detect closes the loop: the hand-over is pagk_frame_handover_detect_device, so the keypoints of the first frame and
// every later top-up are the reference's goodFeaturesToTrack corners (src/frame.cpp:181-184), detected on the device on
// the current frame under the mask the hand-over has just built.  The file's keypoints then only give the count
// (target_n); no candidate list goes to the device at all, and each line also tells how many corners were added.
//
// --detect-fast closes the loop the same way with the detector the reference's front-ends construct (ORBextractor with
// one level, src/ORBextractor.cc:1148-1205: FAST in cells of about 30 pixels, then the quadtree down to target_n nodes):
// the hand-over is pagk_frame_handover_fast_device.  The lines are those of --detect.
//
// --rectify puts the camera's lens in front of the loop (reference Examples/Demo/RealSenseD435i.cpp:202: cv::remap on every
// frame): the file's images are taken for the ideal view, the program synthesises the DISTORTED frames a real lens would
// deliver (the inverse of the file's Brown-Conrady model, by fixed-point iteration, applied with pagk_rectify), and the
// loop then feeds those raw frames: pagk_frame_rectify_device (maps from pagk_undistort_maps, set once) replaces
// pagk_frame_set_device inside each graph.  The same lines are printed.  --detect / --detect-fast and --rectify combine.
//
// --inverse tracks in the template-Jacobian mode (pagk_params::inverse = PAGK_INVERSE_TEMPLATE, include/pagk.h): the same loop
// and the same lines, with that mode's results.  Combines with every other flag.
//
// Input: the file of stream_resident.cpp.
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I /opt/rocm/include -I include examples/stream_graph_loop.cpp
//        -L <pkg> -l:libpagk_hip.so -L /opt/rocm/lib -lamdhip64 -Wl,-rpath,<pkg> -Wl,-rpath,/opt/rocm/lib
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pagk.h"

#define CHECK_HIP(x)                                                                  \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            std::fprintf(stderr, "%s -> %s\n", #x, hipGetErrorString(e_));            \
            return 10;                                                                \
        }                                                                             \
    } while (0)
#define CHECK_PAGK(x)                                                                 \
    do {                                                                              \
        int rc_ = (x);                                                                \
        if (rc_ != PAGK_OK) {                                                         \
            std::fprintf(stderr, "%s -> %s (%s)\n", #x, pagk_strerror(rc_), pagk_last_error(ctx)); \
            return 11;                                                                \
        }                                                                             \
    } while (0)

struct KeySet {
    float *keys, *keys_un, *keys_normal;
    int32_t *index_in_last;
    uint8_t *live;
};

int main(int argc, char **argv)
{
    bool detect = false, rectify = false, fast = false, inverse = false;   // fast: the detector of --detect is the FAST one
    for (int k = 1; k < argc; k++)
        if (!std::strcmp(argv[k], "--detect") || !std::strcmp(argv[k], "--rectify") || !std::strcmp(argv[k], "--detect-fast") ||
            !std::strcmp(argv[k], "--inverse")) {
            (argv[k][2] == 'd' ? detect : (argv[k][2] == 'i' ? inverse : rectify)) = true;
            if (!std::strcmp(argv[k], "--detect-fast")) fast = true;
            for (int j = k; j + 1 < argc; j++) argv[j] = argv[j + 1];
            argc--, k--;
        }
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s [--detect | --detect-fast] [--rectify] [--inverse] sequence.bin [half_patch iterations pyramids]\n", argv[0]);
        return 2;
    }
    const int half = argc > 2 ? std::atoi(argv[2]) : 5, iters = argc > 3 ? std::atoi(argv[3]) : 10,
              pyr = argc > 4 ? std::atoi(argv[4]) : 3;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[4];
    float K[9], dist[4];
    if (std::fread(hdr, 4, 4, f) != 4 || std::fread(K, 4, 9, f) != 9 || std::fread(dist, 4, 4, f) != 4) return 4;
    const int nf = hdr[0], w = hdr[1], h = hdr[2], nk = hdr[3];
    std::vector<std::vector<unsigned char>> img(nf, std::vector<unsigned char>((size_t)w * h));
    for (auto &im : img)
        if (std::fread(im.data(), 1, im.size(), f) != im.size()) return 5;
    std::vector<float> kp((size_t)nk * 2), Rs((size_t)(nf - 1) * 9), KRK((size_t)(nf - 1) * 9);
    if (std::fread(kp.data(), 4, kp.size(), f) != kp.size() || std::fread(Rs.data(), 4, Rs.size(), f) != Rs.size() ||
        std::fread(KRK.data(), 4, KRK.size(), f) != KRK.size())
        return 6;
    std::fclose(f);
    if (nk < 1) {
        std::printf("survivors 0 checksum %.6f\n", 0.0);
        return 0;
    }

    pagk_ctx *ctx = nullptr;
    if (pagk_create(&ctx, 0) != PAGK_OK) {
        std::fprintf(stderr, "no HIP device\n");
        return 7;
    }
    // src/gyro_aided_tracker.cpp:276-282 + eType 4 (:402-408)
    pagk_params p;
    pagk_params_default(&p);
    p.half_patch = half, p.iterations = iters, p.pyramids = pyr;
    p.has_gyro_predict_initial = 1, p.consider_illumination = 1, p.consider_affine = 1, p.regularization_penalty = 0;
    if (inverse) p.inverse = PAGK_INVERSE_TEMPLATE;
    p.fx = K[0], p.fy = K[4], p.cx = K[2], p.cy = K[5];
    p.n_dist_coef = 4;
    for (int k = 0; k < 4; k++) p.dist_coef[k] = dist[k];

    pagk_rectify_params rp;
    pagk_rectify_params_default(&rp);   // one channel
    if (rectify) {
        // the distorted frames: raw(u, v) = ideal(K x), x the undistorted normalised point of (u, v) -- five rounds of
        // x <- (x_d - tangential(x)) / radial(x), cv::undistortPoints' iteration -- sampled with the library's own remap
        const size_t px = (size_t)w * h;
        std::vector<float> mx(px), my(px);
        const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3];
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++) {
                const double xd = (u - K[2]) / K[0], yd = (v - K[5]) / K[4];
                double x = xd, y = yd;
                for (int it = 0; it < 5; it++) {
                    const double r2 = x * x + y * y, kr = 1.0 + (k2 * r2 + k1) * r2;
                    x = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / kr;
                    y = (yd - (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) / kr;
                }
                mx[(size_t)v * w + u] = (float)(K[0] * x + K[2]);
                my[(size_t)v * w + u] = (float)(K[4] * y + K[5]);
            }
        CHECK_PAGK(pagk_rectify_set_maps(ctx, mx.data(), my.data(), w, h, (int64_t)w * 4));
        std::vector<unsigned char> raw(px);
        for (auto &im : img) {
            CHECK_PAGK(pagk_rectify(ctx, &rp, im.data(), w, h, w, raw.data(), w));
            im = raw;
        }
        // ... and the maps the loop rectifies them with: initUndistortRectifyMap of the same camera (include/imu_types.h:60-65)
        const double d4[4] = {k1, k2, p1, p2};
        CHECK_PAGK(pagk_undistort_maps(K[0], K[4], K[2], K[5], d4, 4, K[0], K[4], K[2], K[5], w, h, mx.data(), my.data()));
        CHECK_PAGK(pagk_rectify_set_maps(ctx, mx.data(), my.data(), w, h, (int64_t)w * 4));
    }
    // a frame into a slot: the image as it is, or the raw frame through the maps
    auto frame_into = [&](int slot, const unsigned char *d_img) -> int {
        return rectify ? pagk_frame_rectify_device(ctx, slot, &rp, d_img, w, h, w, pyr) : pagk_frame_set_device(ctx, slot, d_img, w, h, w, pyr);
    };

    // everything a frame touches lives at a fixed device address; the capacity is the initial keypoint count
    const int32_t cap = nk;
    const size_t n8 = (size_t)cap * 8;
    hipStream_t stream;
    CHECK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));  // (a capture needs a stream of its own)
    CHECK_PAGK(pagk_set_stream(ctx, stream));
    KeySet ks[2];
    for (auto &s : ks) {
        CHECK_HIP(hipMalloc((void **)&s.keys, n8));
        CHECK_HIP(hipMalloc((void **)&s.keys_un, n8));
        CHECK_HIP(hipMalloc((void **)&s.keys_normal, n8));
        CHECK_HIP(hipMalloc((void **)&s.index_in_last, (size_t)cap * 4));
        CHECK_HIP(hipMalloc((void **)&s.live, (size_t)cap));
    }
    unsigned char *d_frame;
    float *d_rot, *d_cand, *d_pu, *d_pd, *d_aff, *d_ptun, *d_ptdist, *d_pp, *d_ppu;
    uint8_t *d_st_in, *d_st_pm, *d_st;
    double *d_err, *d_dist;
    int32_t *d_ncand, *d_kept, *d_state, *d_info;
    CHECK_HIP(hipMalloc((void **)&d_frame, (size_t)w * h));
    CHECK_HIP(hipMalloc((void **)&d_rot, 9 * 4));
    CHECK_HIP(hipMalloc((void **)&d_cand, n8));
    CHECK_HIP(hipMalloc((void **)&d_pu, n8));
    CHECK_HIP(hipMalloc((void **)&d_pd, n8));
    CHECK_HIP(hipMalloc((void **)&d_aff, (size_t)cap * 16));
    CHECK_HIP(hipMalloc((void **)&d_ptun, n8));
    CHECK_HIP(hipMalloc((void **)&d_ptdist, n8));
    CHECK_HIP(hipMalloc((void **)&d_pp, n8));
    CHECK_HIP(hipMalloc((void **)&d_ppu, n8));
    CHECK_HIP(hipMalloc((void **)&d_st_in, (size_t)cap));
    CHECK_HIP(hipMalloc((void **)&d_st_pm, (size_t)cap));
    CHECK_HIP(hipMalloc((void **)&d_st, (size_t)cap));
    CHECK_HIP(hipMalloc((void **)&d_err, n8));
    CHECK_HIP(hipMalloc((void **)&d_dist, n8));
    CHECK_HIP(hipMalloc((void **)&d_ncand, 4));
    CHECK_HIP(hipMalloc((void **)&d_kept, 4));
    CHECK_HIP(hipMalloc((void **)&d_state, PAGK_HANDOVER_STATE_WORDS * 4));
    CHECK_HIP(hipMalloc((void **)&d_info, PAGK_DETECT_INFO_WORDS * 4));
    CHECK_HIP(hipMemset(d_st, 0, (size_t)cap));
    CHECK_HIP(hipMemset(d_pp, 0, n8));
    CHECK_HIP(hipMemset(d_ppu, 0, n8));
    CHECK_HIP(hipMemset(d_state, 0, PAGK_HANDOVER_STATE_WORDS * 4));  // reach_flag starts down
    pagk_outputs d_out{d_ptun, d_ptdist, d_st_pm, d_err, d_dist, nullptr, nullptr};
    // --detect: Frame::DetectKeyPoints' arguments (src/frame.cpp:181-184) and mThresholdOfPredictNewKeyPoint = 0.8 mN
    pagk_detect_params det;
    pagk_detect_params_default(&det);
    const double new_point_threshold = detect ? 0.8 * nk : 0.0;
    // --detect-fast: the ORBextractor both front-ends construct (20, 7, one level); nfeatures = target_n
    pagk_fast_params fp;
    pagk_fast_params_default(&fp);

    // first frame (Examples/Demo/RealSenseD435i.cpp:221-235): its pyramid, and the hand-over with an all-zero status
    // takes the file's keypoints, in order, into key set 0
    int32_t n_cand = nk;
    CHECK_HIP(hipMemcpy(d_cand, kp.data(), n8, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_ncand, &n_cand, 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_frame, img[0].data(), (size_t)w * h, hipMemcpyHostToDevice));
    CHECK_PAGK(frame_into(0, d_frame));
    if (fast)
        CHECK_PAGK(pagk_frame_handover_fast_device(ctx, &p, w, h, cap, nk, new_point_threshold, d_st, d_pp, d_ppu, &fp, 0,
                                                   ks[0].keys, ks[0].keys_un, ks[0].keys_normal, ks[0].index_in_last,
                                                   ks[0].live, nullptr, d_state, d_info));
    else if (detect)
        CHECK_PAGK(pagk_frame_handover_detect_device(ctx, &p, w, h, cap, nk, new_point_threshold, d_st, d_pp, d_ppu, &det, 0,
                                                     ks[0].keys, ks[0].keys_un, ks[0].keys_normal, ks[0].index_in_last,
                                                     ks[0].live, nullptr, d_state, d_info));
    else
        CHECK_PAGK(pagk_frame_handover_device(ctx, &p, w, h, cap, nk, 0.0, d_st, d_pp, d_ppu, cap, d_ncand, d_cand, ks[0].keys,
                                              ks[0].keys_un, ks[0].keys_normal, ks[0].index_in_last, ks[0].live, nullptr,
                                              d_state));
    CHECK_PAGK(pagk_sync(ctx));
    n_cand = 0;  // no detector from here on: the list only shrinks, as in stream_resident
    CHECK_HIP(hipMemcpy(d_ncand, &n_cand, 4, hipMemcpyHostToDevice));

    auto frame_work = [&](int par) -> int {  // frame slot `par` = current, key set 1 - par = reference keypoints
        const KeySet &ref = ks[1 - par], &dst = ks[par];
        CHECK_PAGK(frame_into(par, d_frame));
        CHECK_PAGK(pagk_gyro_predict_device_live(ctx, &p, w, h, d_rot, cap, ref.keys_un, ref.live, d_pu, d_pd, d_st_in,
                                                 d_aff));
        CHECK_PAGK(pagk_track_device(ctx, &p, 1 - par, par, cap, ref.keys_un, d_pu, d_aff, d_st_in, &d_out));
        // Step 3 (src/gyro_aided_tracker.cpp:289-341), then Examples/Demo/RealSenseD435i.cpp:254-258 on the device
        CHECK_PAGK(pagk_post_filter_device(ctx, cap, half, d_st_pm, d_err, d_dist, d_ptdist, d_ptun, d_st, d_pp, d_ppu,
                                           d_kept, nullptr));
        if (fast)
            CHECK_PAGK(pagk_frame_handover_fast_device(ctx, &p, w, h, cap, nk, new_point_threshold, d_st, d_pp, d_ppu, &fp, par,
                                                       dst.keys, dst.keys_un, dst.keys_normal, dst.index_in_last, dst.live,
                                                       nullptr, d_state, d_info));
        else if (detect)   // the top-up comes from the frame just tracked into, under this call's mask
            CHECK_PAGK(pagk_frame_handover_detect_device(ctx, &p, w, h, cap, nk, new_point_threshold, d_st, d_pp, d_ppu, &det,
                                                         par, dst.keys, dst.keys_un, dst.keys_normal, dst.index_in_last,
                                                         dst.live, nullptr, d_state, d_info));
        else
            CHECK_PAGK(pagk_frame_handover_device(ctx, &p, w, h, cap, nk, 0.0, d_st, d_pp, d_ppu, cap, d_ncand, d_cand, dst.keys,
                                                  dst.keys_un, dst.keys_normal, dst.index_in_last, dst.live, nullptr, d_state));
        return 0;
    };

    int32_t graph[2] = {-1, -1};
    bool ran_directly[2] = {false, false};
    int n = nk;
    if (detect) {
        int32_t state[PAGK_HANDOVER_STATE_WORDS];
        CHECK_HIP(hipMemcpy(state, d_state, sizeof state, hipMemcpyDeviceToHost));
        n = state[0];
        std::printf("first frame detected %d of %d\n", n, nk);
    }
    double checksum = 0;
    std::vector<float> keys_un((size_t)cap * 2);
    for (int k = 1; k < nf && n > 0; k++) {
        const int par = k & 1;
        float rot[9];
        for (int j = 0; j < 6; j++) rot[j] = KRK[(size_t)(k - 1) * 9 + j];
        for (int j = 0; j < 3; j++) rot[6 + j] = Rs[(size_t)(k - 1) * 9 + 6 + j];
        CHECK_HIP(hipMemcpyAsync(d_frame, img[k].data(), (size_t)w * h, hipMemcpyHostToDevice, stream));
        CHECK_HIP(hipMemcpyAsync(d_rot, rot, sizeof rot, hipMemcpyHostToDevice, stream));
        if (!ran_directly[par]) {  // allocations happen outside a capture
            if (int rc = frame_work(par)) return rc;
            ran_directly[par] = true;
        } else {
            if (graph[par] < 0) {
                CHECK_PAGK(pagk_graph_begin(ctx));
                const int rc = frame_work(par);
                const int rc2 = pagk_graph_end(ctx, &graph[par]);
                if (rc) return rc;
                CHECK_PAGK(rc2);
            }
            CHECK_PAGK(pagk_graph_launch(ctx, graph[par]));
        }
        // only to print: the counts, and the survivors' points for the checksum
        int32_t kept = 0, state[PAGK_HANDOVER_STATE_WORDS];
        CHECK_PAGK(pagk_sync(ctx));
        CHECK_HIP(hipMemcpy(&kept, d_kept, 4, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(state, d_state, sizeof state, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(keys_un.data(), ks[par].keys_un, n8, hipMemcpyDeviceToHost));
        if (detect)
            std::printf("pair %d tracked %d of %d, added %d\n", k, kept, n, state[3]);
        else
            std::printf("pair %d tracked %d of %d\n", k, kept, n);
        for (int i = 0; i < state[2]; i++) checksum += keys_un[2 * i] + 2.0 * keys_un[2 * i + 1];
        n = state[0];
    }
    std::printf("survivors %d checksum %.6f\n", n, checksum);
    for (int g : graph)
        if (g >= 0) CHECK_PAGK(pagk_graph_destroy(ctx, g));
    pagk_destroy(ctx);
    (void)hipStreamDestroy(stream);
    return 0;
}
