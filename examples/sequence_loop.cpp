// sequence_loop.cpp -- the reference's main loop (Examples/Demo/RealSenseD435i.cpp:199-321) on the sequence the context
// owns: grab a frame and the gyro rotation, hand them in, read the state words.  Plain C ABI: no HIP header, no device
// array of the caller's, no bookkeeping between frames (examples/stream_graph_loop.cpp is the same loop built by hand
// from the device entry points).
//
//   sequence_loop <seq.bin> <target_n> <cap> [--lk | --lk-gyro] [--detect | --detect-fast] [--direct]
//
// seq.bin: int32 n_frames, width, height, n_cand | float K[9] | float dist[4] | n_frames images | n_frames candidate lists
// (n_cand x 2 floats) | n_frames - 1 rotations (9 floats: rows 0 and 1 of K R K^-1, the third row of R).
// Prints one line per frame: the hand-over's state words [total reach_flag survivors added rejected].
// Build: g++ -std=c++17 -I include examples/sequence_loop.cpp -L <pkg> -l:libpagk_hip.so -Wl,-rpath,<pkg>
//
//   sequence_loop <seq.bin> <target_n> <cap> --cameras K [--lk | --lk-gyro] [--direct]
//
// A rig: K copies of the loop stepped together through a sequence group (pagk_sequence_group_*), every stage of a frame one
// launch for all cameras.  Camera j sees the file's frames and rotations and, so that the cameras differ, the candidate
// list of frame (k + j) mod n_frames.  Prints "camera j frame k: ..." with the same state words, camera by camera per frame.
// With --lk or --lk-gyro the rig tracks with Lucas-Kanade (pagk_sequence_group_create_lk): the baseline arm of the
// comparison (src/gyro_aided_tracker.cpp:353-380) through the same calls.
//
//   sequence_loop <dir> <target_n> <cap> --sensor [--lk | --lk-gyro] [--detect | --detect-fast] [--direct]
//
// The sensor form: what the demo reads from disk (Examples/Demo/RealSenseD435i.cpp:74-141) goes into the sequence as it is,
// with no arithmetic in this file.  <dir>/image_file_list.txt and <dir>/imu.txt are read through csrc/host/sequence_io.h
// (LoadImageList, LoadImu, ImuWindow); image decoding is the application's, so each listed name "<stamp_ns>.png" stands for
// the headerless raw frame <dir>/<stamp_ns>.raw (src_height rows of src_width x channels bytes).  <dir>/sensor.bin: int32
// width, height, src_width, src_height, channels, n_cand | float K[9] | dist[4] | Rbc[9] | bias[3] | map_x, map_y (height x
// width floats each) | one candidate list (n_cand x 2 floats) per frame.  Prints the same state words.
// Build: add -DPAGK_EXAMPLE_SENSOR -I <pkg>/csrc/host -l:libpagk_tracker.so
//
//   sequence_loop <dir> <target_n> <cap> --sensor --cameras K [--lk | --lk-gyro] [--detect-fast] [--direct]
//
// A rig of sensor sequences (pagk_sequence_group_*_sensor; with --lk or --lk-gyro pagk_sequence_group_create_lk): K contexts, each with the file's maps and Rbc, stepped together
// with the raw frames and the IMU window as they come from disk.  So that the cameras differ, camera j sees the raw frame
// (k + j) mod n_frames and (without --detect-fast) the candidate list of that frame.  Prints "camera j frame k: ...".
//
//   ... --pipeline DEPTH  (every form above; DEPTH 2 .. 8)
//
// The pipelined loop: the sequence gets a result ring of DEPTH pinned blocks (pagk_sequence_results_create), frames are handed
// in without waiting, and the record of frame k is fetched (pagk_sequence_fetch: it waits for that frame's copy only) after
// frame k + DEPTH - 1 was handed in.  Prints the same lines as the lock-step loop, from the records: a diff of the two outputs
// is empty.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pagk.h"
#ifdef PAGK_EXAMPLE_SENSOR
#include "sequence_io.h"
#endif

#define CHECK(call)                                                                                        \
    do {                                                                                                   \
        int rc_ = (call);                                                                                  \
        if (rc_ != PAGK_OK) {                                                                              \
            fprintf(stderr, "%s -> %s (%s)\n", #call, pagk_strerror(rc_), ctx ? pagk_last_error(ctx) : ""); \
            return 2;                                                                                      \
        }                                                                                                  \
    } while (0)

// --pipeline: the line of frame k of a camera (-1: the only one), from its record in the ring
static int print_fetched(pagk_ctx *c, int k, int camera)
{
    pagk_sequence_result r;
    const int rc = pagk_sequence_fetch(c, k, &r);
    if (rc != PAGK_OK) return fprintf(stderr, "pagk_sequence_fetch -> %s (%s)\n", pagk_strerror(rc), pagk_last_error(c)), rc;
    if (camera >= 0) printf("camera %d ", camera);
    printf("frame %d: %d %d %d %d %d\n", r.frame, r.state[0], r.state[1], r.state[2], r.state[3], r.state[4]);
    return PAGK_OK;
}

// the frames whose records are due once frame k has been handed in: k - depth + 1, and behind the last frame the rest
static int fetch_due(pagk_ctx *const *ctxs, int K, bool rig, int k, int nf, int depth)
{
    const int first = k - depth + 1 < 0 ? 0 : k - depth + 1, last = k == nf - 1 ? k : k - depth + 1;
    for (int f = first; f <= last; f++)
        for (int j = 0; j < K; j++)
            if (print_fetched(ctxs[j], f, rig ? j : -1) != PAGK_OK) return 2;
    return 0;
}

template <class T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return fread(v.data(), sizeof(T), n, f) == n;
}

// :199-321 for K cameras at once: K contexts with one sequence each, grouped; the lead's calls step them all
static int rig_loop(const pagk_sequence_params &sp, int K, int mode, int depth, int nf, int w, int h, int nc,
                    const std::vector<std::vector<uint8_t>> &img, const std::vector<std::vector<float>> &cand,
                    const std::vector<std::vector<float>> &rot)
{
    pagk_ctx *ctx = nullptr;   // (the lead: CHECK reports its text)
    std::vector<pagk_ctx *> ctxs(K, nullptr);
    for (int j = 0; j < K; j++) {
        int rc = pagk_create(&ctxs[j], 0);
        if (rc != PAGK_OK) return fprintf(stderr, "pagk_create: %s, no fallback\n", pagk_strerror(rc)), 3;
        if (j == 0) ctx = ctxs[0];
        rc = pagk_sequence_create(ctxs[j], &sp);
        if (rc == PAGK_OK && depth) rc = pagk_sequence_results_create(ctxs[j], depth);
        if (rc != PAGK_OK) return fprintf(stderr, "pagk_sequence_create -> %s (%s)\n", pagk_strerror(rc), pagk_last_error(ctxs[j])), 2;
    }
    // (the Lucas-Kanade group is made by its own call and driven by the same ones)
    CHECK(sp.tracker == PAGK_SEQ_LK ? pagk_sequence_group_create_lk(ctxs.data(), K) : pagk_sequence_group_create(ctxs.data(), K));
    std::vector<pagk_image> frames(K);
    std::vector<const float *> lists(K);
    std::vector<int32_t> counts(K, nc);
    std::vector<float> rot9((size_t)K * 9), keys_un((size_t)sp.cap * 2);
    int32_t state[PAGK_HANDOVER_STATE_WORDS];
    for (int k = 0; k < nf; k++) {
        for (int j = 0; j < K; j++) {
            frames[j] = pagk_image{img[k].data(), w, h, w};
            lists[j] = cand[(k + j) % nf].data();
            if (k) memcpy(&rot9[(size_t)j * 9], rot[k - 1].data(), 9 * sizeof(float));
        }
        if (k == 0)
            CHECK(pagk_sequence_group_start(ctx, frames.data(), lists.data(), counts.data()));
        else
            CHECK(pagk_sequence_group_step(ctx, frames.data(), rot9.data(), lists.data(), counts.data(), mode));
        if (depth) {   // a member's fetches keep working while it is grouped
            if (fetch_due(ctxs.data(), K, true, k, nf, depth)) return 2;
            continue;
        }
        for (int j = 0; j < K; j++) {   // a member's reads keep working while it is grouped
            int rc = pagk_sequence_read(ctxs[j], sp.cap, nullptr, keys_un.data(), nullptr, nullptr, nullptr, state, nullptr);
            if (rc != PAGK_OK) return fprintf(stderr, "pagk_sequence_read -> %s (%s)\n", pagk_strerror(rc), pagk_last_error(ctxs[j])), 2;
            printf("camera %d frame %d: %d %d %d %d %d\n", j, k, state[0], state[1], state[2], state[3], state[4]);
        }
    }
    int32_t words[PAGK_SEQ_STATUS_WORDS];
    CHECK(pagk_sequence_group_status(ctx, words));
    fprintf(stderr, "%d cameras, %d frames, %d graphs\n", words[3], words[0], words[2]);
    CHECK(pagk_sequence_group_destroy(ctx));
    for (int j = K - 1; j >= 0; j--) pagk_destroy(ctxs[j]);   // (each with its sequence)
    return 0;
}

#ifdef PAGK_EXAMPLE_SENSOR
// what the sensor forms read from <dir>: the two lists through csrc/host/sequence_io.h, sensor.bin, the raw frames
struct SensorFiles {
    std::string dir;
    std::vector<std::pair<double, std::string>> frames;
    std::vector<IMU::Point> imu;
    std::vector<float> K, dist, Rbc, bias, map_x, map_y;
    std::vector<std::vector<float>> cand;
    int w = 0, h = 0, ws = 0, hs = 0, cn = 0, nc = 0, nf = 0;

    int load(const std::string &d)
    {
        dir = d;
        if (!pagk_seq::LoadImageList(dir + "/image_file_list.txt", frames) || !pagk_seq::LoadImu(dir + "/imu.txt", imu) || frames.empty())
            return fprintf(stderr, "cannot read image_file_list.txt / imu.txt in %s\n", dir.c_str()), 1;
        FILE *f = fopen((dir + "/sensor.bin").c_str(), "rb");
        int32_t hdr[6];
        if (!f || fread(hdr, 4, 6, f) != 6 || !read_n(f, K, 9) || !read_n(f, dist, 4) || !read_n(f, Rbc, 9) || !read_n(f, bias, 3))
            return fprintf(stderr, "cannot read sensor.bin\n"), 1;
        w = hdr[0], h = hdr[1], ws = hdr[2], hs = hdr[3], cn = hdr[4], nc = hdr[5], nf = (int)frames.size();
        cand.resize(nf);
        bool ok = read_n(f, map_x, (size_t)w * h) && read_n(f, map_y, (size_t)w * h);
        for (int k = 0; ok && k < nf; k++) ok = read_n(f, cand[k], (size_t)nc * 2);
        fclose(f);
        return ok ? 0 : (fprintf(stderr, "sensor.bin is short\n"), 1);
    }
    // the demo's configuration with the file's camera; the sensor block of the file's frames
    bool configure(pagk_sequence_params &sp, pagk_sequence_sensor &ss) const
    {
        sp.track.half_patch = 5, sp.track.iterations = 10, sp.track.pyramids = 3, sp.track.has_gyro_predict_initial = 1;
        sp.track.fx = K[0], sp.track.fy = K[4], sp.track.cx = K[2], sp.track.cy = K[5];
        for (int i = 0; i < 4; i++) sp.track.dist_coef[i] = dist[i];
        sp.track.n_dist_coef = 4;
        sp.lk.half_patch = 5;
        sp.width = w, sp.height = h, sp.new_point_threshold = 0.8 * sp.target_n;
        sp.cand_cap = nc > 0 ? nc : 1;
        pagk_sequence_sensor_default(&ss);
        ss.rectify.channels = cn, ss.raw = 1, ss.src_width = ws, ss.src_height = hs;
        memcpy(ss.Rbc, Rbc.data(), sizeof ss.Rbc);
        return pagk_sequence_params_check(&sp) == PAGK_OK && pagk_sequence_sensor_check(&ss) == PAGK_OK;
    }
    // "<stamp_ns>.png" of the list stands for the headerless raw frame <dir>/<stamp_ns>.raw
    bool raw(int k, std::vector<uint8_t> &buf) const
    {
        std::string name = frames[k].second;
        const size_t slash = name.rfind('/'), dot = name.rfind(".png");
        name = dir + "/" + name.substr(slash == std::string::npos ? 0 : slash + 1, dot - (slash == std::string::npos ? 0 : slash + 1)) + ".raw";
        buf.resize((size_t)ws * hs * cn);
        FILE *fi = fopen(name.c_str(), "rb");
        const bool ok = fi && fread(buf.data(), 1, buf.size(), fi) == buf.size();
        if (fi) fclose(fi);
        if (!ok) fprintf(stderr, "cannot read %s\n", name.c_str());
        return ok;
    }
};

// :199-321 on a sensor sequence: a raw frame and the IMU samples since the last frame in, the next pair's keypoints out
static int sensor_loop(const std::string &dir, pagk_sequence_params sp, int mode, int depth)
{
    pagk_ctx *ctx = nullptr;
    SensorFiles in;
    if (in.load(dir)) return 1;
    const int ws = in.ws, hs = in.hs, cn = in.cn, nc = in.nc, nf = in.nf;
    pagk_sequence_sensor ss;
    if (!in.configure(sp, ss)) return fprintf(stderr, "the parameters are refused\n"), 1;
    int rc = pagk_create(&ctx, 0);
    if (rc != PAGK_OK) return fprintf(stderr, "pagk_create: %s, no fallback\n", pagk_strerror(rc)), 3;
    CHECK(pagk_rectify_set_maps(ctx, in.map_x.data(), in.map_y.data(), in.w, in.h, (int64_t)in.w * 4));
    CHECK(pagk_sequence_create_sensor(ctx, &sp, &ss));
    if (depth) CHECK(pagk_sequence_results_create(ctx, depth));
    const bool list = sp.detector == 0;
    pagk_seq::ImuWindow windows(in.imu);
    std::vector<uint8_t> raw;
    std::vector<float> keys_un((size_t)sp.cap * 2);
    std::vector<double> t;
    std::vector<float> rates;
    int32_t state[PAGK_HANDOVER_STATE_WORDS];
    double t_prev = 0;
    for (int k = 0; k < nf; k++) {
        if (!in.raw(k, raw)) return 1;
        const pagk_image frame = {raw.data(), ws, hs, (int64_t)ws * cn};
        const float *c = list ? in.cand[k].data() : nullptr;
        const std::vector<IMU::Point> samples = windows.Next(t_prev, in.frames[k].first);   // :207-218
        if (k == 0) {
            CHECK(pagk_sequence_start_sensor(ctx, &frame, in.frames[k].first, c, list ? nc : 0));
        } else {
            t.clear(), rates.clear();
            for (const IMU::Point &s : samples) {
                t.push_back(s.t);
                rates.push_back(s.w.x), rates.push_back(s.w.y), rates.push_back(s.w.z);
            }
            const pagk_imu_window win = {t_prev, in.frames[k].first, (int32_t)samples.size(), t.data(), rates.data(),
                                         {in.bias[0], in.bias[1], in.bias[2]}};
            CHECK(pagk_sequence_step_sensor(ctx, &frame, &win, c, list ? nc : 0, mode));
        }
        t_prev = in.frames[k].first;
        if (depth) {
            if (fetch_due(&ctx, 1, false, k, nf, depth)) return 2;
            continue;
        }
        CHECK(pagk_sequence_read(ctx, sp.cap, nullptr, keys_un.data(), nullptr, nullptr, nullptr, state, nullptr));
        printf("frame %d: %d %d %d %d %d\n", k, state[0], state[1], state[2], state[3], state[4]);
    }
    int32_t words[PAGK_SEQ_STATUS_WORDS];
    CHECK(pagk_sequence_status(ctx, words));
    fprintf(stderr, "%d frames, %d graphs\n", words[0], words[2]);
    CHECK(pagk_sequence_destroy(ctx));
    pagk_destroy(ctx);
    return 0;
}

// ... and for K cameras at once: K sensor sequences, grouped; the lead's calls step them all, nothing is computed outside
static int sensor_rig_loop(const std::string &dir, pagk_sequence_params sp, int K, int mode, int depth)
{
    pagk_ctx *ctx = nullptr;   // (the lead: CHECK reports its text)
    SensorFiles in;
    if (in.load(dir)) return 1;
    const int ws = in.ws, hs = in.hs, cn = in.cn, nc = in.nc, nf = in.nf;
    pagk_sequence_sensor ss;
    const bool lk = sp.tracker == PAGK_SEQ_LK;
    if (!in.configure(sp, ss) || (lk ? pagk_sequence_group_lk_check(&sp, &ss) : pagk_sequence_group_sensor_check(&sp, &ss)) != PAGK_OK)
        return fprintf(stderr, "--sensor --cameras: PatchMatch or Lucas-Kanade with the file's candidate lists or --detect-fast\n"), 1;
    std::vector<pagk_ctx *> ctxs(K, nullptr);
    for (int j = 0; j < K; j++) {
        int rc = pagk_create(&ctxs[j], 0);
        if (rc != PAGK_OK) return fprintf(stderr, "pagk_create: %s, no fallback\n", pagk_strerror(rc)), 3;
        if (j == 0) ctx = ctxs[0];
        if ((rc = pagk_rectify_set_maps(ctxs[j], in.map_x.data(), in.map_y.data(), in.w, in.h, (int64_t)in.w * 4)) != PAGK_OK ||
            (rc = pagk_sequence_create_sensor(ctxs[j], &sp, &ss)) != PAGK_OK ||
            (depth && (rc = pagk_sequence_results_create(ctxs[j], depth)) != PAGK_OK))
            return fprintf(stderr, "camera %d -> %s (%s)\n", j, pagk_strerror(rc), pagk_last_error(ctxs[j])), 2;
    }
    CHECK(lk ? pagk_sequence_group_create_lk(ctxs.data(), K) : pagk_sequence_group_create_sensor(ctxs.data(), K));
    const bool list = sp.detector == 0;
    pagk_seq::ImuWindow windows(in.imu);
    std::vector<std::vector<uint8_t>> raw(K);
    std::vector<pagk_image> frames(K);
    std::vector<pagk_imu_window> wins(K);
    std::vector<const float *> lists(K);
    std::vector<int32_t> counts(K, nc);
    std::vector<double> stamps(K), t;
    std::vector<float> rates, keys_un((size_t)sp.cap * 2);
    int32_t state[PAGK_HANDOVER_STATE_WORDS];
    double t_prev = 0;
    for (int k = 0; k < nf; k++) {
        for (int j = 0; j < K; j++) {
            if (!in.raw((k + j) % nf, raw[j])) return 1;
            frames[j] = pagk_image{raw[j].data(), ws, hs, (int64_t)ws * cn};
            lists[j] = in.cand[(k + j) % nf].data();
            stamps[j] = in.frames[k].first;
        }
        const std::vector<IMU::Point> samples = windows.Next(t_prev, in.frames[k].first);   // :207-218, one IMU for the rig
        if (k == 0) {
            CHECK(pagk_sequence_group_start_sensor(ctx, frames.data(), stamps.data(), list ? lists.data() : nullptr,
                                                   list ? counts.data() : nullptr));
        } else {
            t.clear(), rates.clear();
            for (const IMU::Point &s : samples) {
                t.push_back(s.t);
                rates.push_back(s.w.x), rates.push_back(s.w.y), rates.push_back(s.w.z);
            }
            for (int j = 0; j < K; j++)
                wins[j] = pagk_imu_window{t_prev, in.frames[k].first, (int32_t)samples.size(), t.data(), rates.data(),
                                          {in.bias[0], in.bias[1], in.bias[2]}};
            CHECK(pagk_sequence_group_step_sensor(ctx, frames.data(), wins.data(), list ? lists.data() : nullptr,
                                                  list ? counts.data() : nullptr, mode));
        }
        t_prev = in.frames[k].first;
        if (depth) {   // a member's fetches keep working while it is grouped
            if (fetch_due(ctxs.data(), K, true, k, nf, depth)) return 2;
            continue;
        }
        for (int j = 0; j < K; j++) {   // a member's reads keep working while it is grouped
            int rc = pagk_sequence_read(ctxs[j], sp.cap, nullptr, keys_un.data(), nullptr, nullptr, nullptr, state, nullptr);
            if (rc != PAGK_OK) return fprintf(stderr, "pagk_sequence_read -> %s (%s)\n", pagk_strerror(rc), pagk_last_error(ctxs[j])), 2;
            printf("camera %d frame %d: %d %d %d %d %d\n", j, k, state[0], state[1], state[2], state[3], state[4]);
        }
    }
    int32_t words[PAGK_SEQ_STATUS_WORDS];
    CHECK(pagk_sequence_group_status(ctx, words));
    fprintf(stderr, "%d cameras, %d frames, %d graphs\n", words[3], words[0], words[2]);
    CHECK(pagk_sequence_group_destroy(ctx));
    for (int j = K - 1; j >= 0; j--) pagk_destroy(ctxs[j]);   // (each with its sequence)
    return 0;
}
#endif

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s seq.bin|dir target_n cap [--sensor] [--cameras K] [--lk | --lk-gyro] [--detect | --detect-fast] [--direct] [--pipeline DEPTH]\n", argv[0]);
        return 1;
    }
    pagk_ctx *ctx = nullptr;
    pagk_sequence_params sp;
    pagk_sequence_params_default(&sp);
    sp.target_n = atoi(argv[2]), sp.cap = atoi(argv[3]);
    int mode = PAGK_SEQ_GRAPH;
    bool sensor = false;
    int cameras = 0, depth = 0;
    for (int i = 4; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--lk") sp.tracker = PAGK_SEQ_LK, sp.lk_initial_flow = 0;
        else if (a == "--lk-gyro") sp.tracker = PAGK_SEQ_LK, sp.lk_initial_flow = 1;
        else if (a == "--detect") sp.detector = 1;
        else if (a == "--detect-fast") sp.detector = 2;
        else if (a == "--direct") mode = PAGK_SEQ_DIRECT;
        else if (a == "--sensor") sensor = true;
        else if (a == "--cameras" && i + 1 < argc) cameras = atoi(argv[++i]);
        else if (a == "--pipeline" && i + 1 < argc) depth = atoi(argv[++i]);
        else return fprintf(stderr, "unknown flag %s\n", argv[i]), 1;
    }
    if (depth && (depth < 2 || depth > 8)) return fprintf(stderr, "--pipeline: a ring of 2 .. 8 blocks\n"), 1;
    if (sensor) {
#ifdef PAGK_EXAMPLE_SENSOR
        if (cameras < 0 || cameras > 64) return fprintf(stderr, "--cameras: 1 .. 64 cameras\n"), 1;
        return cameras ? sensor_rig_loop(argv[1], sp, cameras, mode, depth) : sensor_loop(argv[1], sp, mode, depth);
#else
        return fprintf(stderr, "--sensor: build with -DPAGK_EXAMPLE_SENSOR against csrc/host/sequence_io.h and libpagk_tracker.so\n"), 1;
#endif
    }
    FILE *f = fopen(argv[1], "rb");
    int32_t hdr[4];
    std::vector<float> K, dist;
    if (!f || fread(hdr, 4, 4, f) != 4 || !read_n(f, K, 9) || !read_n(f, dist, 4)) return fprintf(stderr, "cannot read %s\n", argv[1]), 1;
    const int nf = hdr[0], w = hdr[1], h = hdr[2], nc = hdr[3];
    std::vector<std::vector<uint8_t>> img(nf);
    std::vector<std::vector<float>> cand(nf), rot(nf > 0 ? nf - 1 : 0);
    bool ok = nf >= 1;
    for (int k = 0; ok && k < nf; k++) ok = read_n(f, img[k], (size_t)w * h);
    for (int k = 0; ok && k < nf; k++) ok = read_n(f, cand[k], (size_t)nc * 2);
    for (int k = 0; ok && k + 1 < nf; k++) ok = read_n(f, rot[k], 9);
    fclose(f);
    if (!ok) return fprintf(stderr, "%s is short\n", argv[1]), 1;

    // the configuration of the reference's demo: half patch 5, 10 iterations, 3 levels, the camera of the file
    sp.track.half_patch = 5, sp.track.iterations = 10, sp.track.pyramids = 3, sp.track.has_gyro_predict_initial = 1;
    sp.track.fx = K[0], sp.track.fy = K[4], sp.track.cx = K[2], sp.track.cy = K[5];
    for (int i = 0; i < 4; i++) sp.track.dist_coef[i] = dist[i];
    sp.track.n_dist_coef = 4;
    sp.lk.half_patch = 5;
    sp.width = w, sp.height = h, sp.new_point_threshold = 0.8 * sp.target_n;
    sp.cand_cap = nc > 0 ? nc : 1;
    if (pagk_sequence_params_check(&sp) != PAGK_OK) return fprintf(stderr, "the parameters are refused\n"), 1;
    if (cameras) {
        const int ok_rig = sp.tracker == PAGK_SEQ_LK ? pagk_sequence_group_lk_check(&sp, nullptr) : pagk_sequence_group_check(&sp);
        if (cameras < 1 || cameras > 64 || ok_rig != PAGK_OK)
            return fprintf(stderr, "--cameras: 1 .. 64 cameras, PatchMatch or Lucas-Kanade with the file's candidate lists\n"), 1;
        return rig_loop(sp, cameras, mode, depth, nf, w, h, nc, img, cand, rot);
    }

    int rc = pagk_create(&ctx, 0);
    if (rc != PAGK_OK) return fprintf(stderr, "pagk_create: %s, no fallback\n", pagk_strerror(rc)), 3;
    CHECK(pagk_sequence_create(ctx, &sp));
    if (depth) CHECK(pagk_sequence_results_create(ctx, depth));
    const bool list = sp.detector == 0;
    std::vector<float> keys_un((size_t)sp.cap * 2);
    int32_t state[PAGK_HANDOVER_STATE_WORDS];
    for (int k = 0; k < nf; k++) {   // :199-321: one frame and one rotation in, the next pair's keypoints out
        const pagk_image frame = {img[k].data(), w, h, w};
        const float *c = list ? cand[k].data() : nullptr;
        if (k == 0)
            CHECK(pagk_sequence_start(ctx, &frame, c, list ? nc : 0));
        else
            CHECK(pagk_sequence_step(ctx, &frame, rot[k - 1].data(), c, list ? nc : 0, mode));
        if (depth) {   // no waiting here: the record of frame k - depth + 1 is due, later frames are in flight
            if (fetch_due(&ctx, 1, false, k, nf, depth)) return 2;
            continue;
        }
        CHECK(pagk_sequence_read(ctx, sp.cap, nullptr, keys_un.data(), nullptr, nullptr, nullptr, state, nullptr));
        printf("frame %d: %d %d %d %d %d\n", k, state[0], state[1], state[2], state[3], state[4]);
    }
    int32_t words[PAGK_SEQ_STATUS_WORDS];
    CHECK(pagk_sequence_status(ctx, words));
    fprintf(stderr, "%d frames, %d graphs\n", words[0], words[2]);
    CHECK(pagk_sequence_destroy(ctx));
    pagk_destroy(ctx);
    return 0;
}
