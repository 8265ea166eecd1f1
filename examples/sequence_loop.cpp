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
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pagk.h"

#define CHECK(call)                                                                                        \
    do {                                                                                                   \
        int rc_ = (call);                                                                                  \
        if (rc_ != PAGK_OK) {                                                                              \
            fprintf(stderr, "%s -> %s (%s)\n", #call, pagk_strerror(rc_), ctx ? pagk_last_error(ctx) : ""); \
            return 2;                                                                                      \
        }                                                                                                  \
    } while (0)

template <class T>
static bool read_n(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s seq.bin target_n cap [--lk | --lk-gyro] [--detect | --detect-fast] [--direct]\n", argv[0]);
        return 1;
    }
    pagk_ctx *ctx = nullptr;
    pagk_sequence_params sp;
    pagk_sequence_params_default(&sp);
    sp.target_n = atoi(argv[2]), sp.cap = atoi(argv[3]);
    int mode = PAGK_SEQ_GRAPH;
    for (int i = 4; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--lk") sp.tracker = PAGK_SEQ_LK, sp.lk_initial_flow = 0;
        else if (a == "--lk-gyro") sp.tracker = PAGK_SEQ_LK, sp.lk_initial_flow = 1;
        else if (a == "--detect") sp.detector = 1;
        else if (a == "--detect-fast") sp.detector = 2;
        else if (a == "--direct") mode = PAGK_SEQ_DIRECT;
        else return fprintf(stderr, "unknown flag %s\n", argv[i]), 1;
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

    int rc = pagk_create(&ctx, 0);
    if (rc != PAGK_OK) return fprintf(stderr, "pagk_create: %s, no fallback\n", pagk_strerror(rc)), 3;
    CHECK(pagk_sequence_create(ctx, &sp));
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
