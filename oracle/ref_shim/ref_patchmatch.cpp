// ref_patchmatch.cpp -- runs the reference's OWN src/patch_match.cpp and src/utils.cpp, compiled unchanged against the
// stand-ins of this directory, over a case file.  TEST INFRASTRUCTURE; built into oracle/_ref/ (never committed) by
// `make -C oracle ref` when the reference's sources are at $(REFERENCE).  Grown from tools/ref_dump/dump_patchmatch.cpp --
// the kit for a REAL OpenCV + Eigen build -- and reads and writes that file's formats, so tools/ref_dump/export_cases.py and
// import_ref.py serve both.
//
//   ref_patchmatch <case.in> <case.ref>          PatchMatch::OpticalFlowMultiLevel()   (src/patch_match.cpp:79-142)
//   ref_patchmatch --ncc <case.ncc> <case.out>   the two free NCC overloads            (src/utils.cpp:110-148, :166-202)
//
// What is the reference's and what is not: every statement of OpticalFlowMultiLevel, ..._onePixel, the member GetPixelValue,
// DistortPoints / DistortVecPoints, PatchMatch::NCC, the free NCC and the free GetPixelValue is the reference's text, compiled
// with its own flags (-O3, no -march).  Third-party arithmetic is the oracle's definition: cv::resize is
// pagk_oracle_pyr_down, H.llt().solve(b) is pagk_oracle_llt_solve4, update.norm() has the documented mask-0 shape, and
// log(double) below is pagk_oracle_log (libm's is not bit-reproducible across hosts, oracle/README.md).
//
// Case file, version 1 (tools/ref_dump/dump_patchmatch.cpp) or version 2, little endian:
//   char magic[8] = "PAGKIN1\0" | "PAGKIN2\0"; int32 W, H, N, half_patch, iterations, pyramids;
//   int32 has_gyro, illumination, affine, penalty, ncc;
//   version 2 only: int32 n_dist_coef (4 or 5), step (bytes per image row, >= W; the padding is zero);
//   float cam[8] = fx fy cx cy k1 k2 p1 p2;  version 2: float cam[9], k3 last;
//   uint8 ref[H*W]; uint8 cur[H*W]  (rows packed, whatever the step);
//   float pt_ref[N*2]; float pt_init[N*2]; float affine[N*4]; uint8 status_in[N];
// Result file: "PAGKREF1", as dump_patchmatch.cpp writes it; the text tail says what this binary was built from.
// NCC file: char magic[8] = "PAGKNC1\0"; int32 W, H, N, half_patch, step, use_affine; uint8 ref[H*W]; uint8 cur[H*W];
//   float pt_ref[N*2]; float pt_cur[N*2]; float affine[N*4];
// NCC result: char magic[8] = "PAGKNCR1"; int32 N; float ncc_images[N] (two-image overload); float ncc_values[N] (the
//   overload that takes the reference patch's values and mean, here sampled with the free GetPixelValue in NCC's own order).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gyro_aided_tracker.h"   // the stand-in of this directory
#include "patch_match.h"          // the reference's include/
#include "utils.h"

// log(double) of the penalty term (src/patch_match.cpp:305): the project's definition, on both sides (-fno-builtin-log keeps
// the compiler from folding or replacing the call)
extern "C" double log(double x) noexcept { return pagk_oracle_log(x); }

static const char BUILT_WITH[] =
    "\nreference src/patch_match.cpp:33-469 and src/utils.cpp:25-202 with include/patch_match.h and include/utils.h:32-46, "
    "compiled unchanged (g++ -O3 -std=c++14 -ffp-contract=off, no -march); project stand-ins for OpenCV and Eigen "
    "(oracle/ref_shim); the oracle's llt (pagk_oracle_llt_solve4, norm in the mask-0 shape), resize (pagk_oracle_pyr_down) "
    "and log (pagk_oracle_log)\n";

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE *f, const T *p, size_t n) { fwrite(p, sizeof(T), n, f); }

static bool read_image(FILE *f, cv::Mat &m)
{
    for (int r = 0; r < m.rows; r++)
        if (!rd(f, m.ptr<uint8_t>(r), (size_t)m.cols)) return false;
    return true;
}

static cv::Mat affine_mat(const float *a)
{
    cv::Mat A(2, 2, CV_32F);
    A.at<float>(0, 0) = a[0], A.at<float>(0, 1) = a[1], A.at<float>(1, 0) = a[2], A.at<float>(1, 1) = a[3];
    return A;
}

static int run_patchmatch(const char *in_path, const char *out_path)
{
    FILE *fi = fopen(in_path, "rb");
    char magic[8];
    int32_t hd[13] = {0};
    float cam[9] = {0};
    if (!fi || !rd(fi, magic, 8)) return 3;
    const int version = memcmp(magic, "PAGKIN1", 8) == 0 ? 1 : memcmp(magic, "PAGKIN2", 8) == 0 ? 2 : 0;
    if (!version || !rd(fi, hd, version == 1 ? 11 : 13) || !rd(fi, cam, version == 1 ? 8 : 9)) return 3;
    const int W = hd[0], H = hd[1], N = hd[2], half = hd[3], iters = hd[4], L = hd[5];
    const bool has_gyro = hd[6], illum = hd[7], affine_on = hd[8], penalty = hd[9], ncc_on = hd[10];
    const int n_dist = version == 1 ? 4 : hd[11], step = version == 1 ? W : hd[12];
    if (W < 1 || H < 1 || N < 0 || step < W || (n_dist != 4 && n_dist != 5)) return 3;
    cv::Mat ref = cv::Mat::with_step(H, W, CV_8UC1, (size_t)step), cur = cv::Mat::with_step(H, W, CV_8UC1, (size_t)step);
    std::vector<float> pt_ref((size_t)N * 2), pt_init((size_t)N * 2), aff((size_t)N * 4);
    std::vector<uint8_t> status_in((size_t)N);
    if (!read_image(fi, ref) || !read_image(fi, cur) || !rd(fi, pt_ref.data(), pt_ref.size()) ||
        !rd(fi, pt_init.data(), pt_init.size()) || !rd(fi, aff.data(), aff.size()) || !rd(fi, status_in.data(), status_in.size()))
        return 4;
    fclose(fi);

    // the state GyroPredictFeatures() leaves on the tracker before PatchMatch is constructed
    GyroAidedTracker tracker;
    tracker.mImgGrayRef = ref, tracker.mImgGrayCur = cur;
    tracker.mK = cv::Mat(3, 3, CV_32F);
    tracker.mK.at<float>(0, 0) = cam[0], tracker.mK.at<float>(1, 1) = cam[1], tracker.mK.at<float>(0, 2) = cam[2],
    tracker.mK.at<float>(1, 2) = cam[3], tracker.mK.at<float>(2, 2) = 1.f;
    tracker.mDistCoef = cv::Mat(n_dist, 1, CV_32F);
    for (int k = 0; k < n_dist; k++) tracker.mDistCoef.at<float>(k) = cam[4 + k];
    for (int i = 0; i < N; i++) {
        tracker.mvKeysRef.push_back(cv::KeyPoint(pt_ref[2 * i], pt_ref[2 * i + 1], 1.f));
        tracker.mvKeysRefUn.push_back(tracker.mvKeysRef.back());
        tracker.mvPtPredictUn.push_back(cv::Point2f(pt_init[2 * i], pt_init[2 * i + 1]));
        tracker.mvPtPredict.push_back(tracker.mvPtPredictUn.back());
        tracker.mvStatus.push_back(status_in[i]);
        tracker.mvAffineDeformationMatrix.push_back(affine_mat(&aff[4 * (size_t)i]));
    }

    PatchMatch pm(&tracker, half, iters, L, has_gyro, /*bInverse_=*/false, illum, affine_on, penalty, ncc_on);
    pm.OpticalFlowMultiLevel();

    FILE *fo = fopen(out_path, "wb");
    if (!fo) return 5;
    const int32_t out_hd[2] = {N, L};
    wr(fo, "PAGKREF1", 8);
    wr(fo, out_hd, 2);
    for (int i = 0; i < N; i++) wr(fo, &tracker.mvPtPredictAfterPatchMatchedUn[i].x, 1), wr(fo, &tracker.mvPtPredictAfterPatchMatchedUn[i].y, 1);
    for (int i = 0; i < N; i++) wr(fo, &tracker.mvPtPredictAfterPatchMatched[i].x, 1), wr(fo, &tracker.mvPtPredictAfterPatchMatched[i].y, 1);
    wr(fo, tracker.mvStatusAfterPatchMatched.data(), (size_t)N);
    wr(fo, tracker.mvPixelErrorsOfPatchMatched.data(), (size_t)N);
    wr(fo, tracker.mvDistanceBetweenPredictedAndPatchMatched.data(), (size_t)N);
    wr(fo, tracker.mvNccAfterPatchMatched.data(), (size_t)N);
    // the resize chain of CreatePyramids, replayed (here the oracle's definition; with a real OpenCV it pins cv::resize)
    cv::Mat p1 = ref, p2 = cur;
    for (int l = 1; l < L; l++) {
        cv::Mat q1, q2;
        cv::resize(p1, q1, cv::Size(p1.cols * 0.5, p1.rows * 0.5));
        cv::resize(p2, q2, cv::Size(p2.cols * 0.5, p2.rows * 0.5));
        const int32_t wh[2] = {q1.cols, q1.rows};
        wr(fo, wh, 2);
        for (int r = 0; r < q1.rows; r++) wr(fo, q1.ptr<uint8_t>(r), (size_t)q1.cols);
        for (int r = 0; r < q2.rows; r++) wr(fo, q2.ptr<uint8_t>(r), (size_t)q2.cols);
        p1 = q1, p2 = q2;
    }
    fputs(BUILT_WITH, fo);
    return fclose(fo) == 0 ? 0 : 5;
}

static int run_ncc(const char *in_path, const char *out_path)
{
    FILE *fi = fopen(in_path, "rb");
    char magic[8];
    int32_t hd[6];
    if (!fi || !rd(fi, magic, 8) || memcmp(magic, "PAGKNC1", 8) != 0 || !rd(fi, hd, 6)) return 3;
    const int W = hd[0], H = hd[1], N = hd[2], half = hd[3], step = hd[4];
    const bool use_affine = hd[5];
    if (W < 1 || H < 1 || N < 0 || half < 1 || step < W) return 3;
    cv::Mat ref = cv::Mat::with_step(H, W, CV_8UC1, (size_t)step), cur = cv::Mat::with_step(H, W, CV_8UC1, (size_t)step);
    std::vector<float> pt_ref((size_t)N * 2), pt_cur((size_t)N * 2), aff((size_t)N * 4);
    if (!read_image(fi, ref) || !read_image(fi, cur) || !rd(fi, pt_ref.data(), pt_ref.size()) ||
        !rd(fi, pt_cur.data(), pt_cur.size()) || !rd(fi, aff.data(), aff.size()))
        return 4;
    fclose(fi);
    std::vector<float> by_images((size_t)N), by_values((size_t)N);
    for (int i = 0; i < N; i++) {
        const cv::Point2f pr(pt_ref[2 * i], pt_ref[2 * i + 1]), pc(pt_cur[2 * i], pt_cur[2 * i + 1]);
        const cv::Mat A = use_affine ? affine_mat(&aff[4 * (size_t)i]) : cv::Mat();
        by_images[i] = NCC(half, ref, cur, pr, pc, A);
        // the reference patch as a caller of the other overload prepares it: the free sampler, x outer and y inner
        std::vector<float> values;
        float mean = 0.0f;
        for (int x = -half; x <= half; x++)
            for (int y = -half; y <= half; y++) {
                values.push_back(GetPixelValue(ref, pr.x + x, pr.y + y));
                mean += values.back();
            }
        mean /= values.size();
        by_values[i] = NCC(half, values, mean, cur, pc, A);
    }
    FILE *fo = fopen(out_path, "wb");
    if (!fo) return 5;
    const int32_t n32 = N;
    wr(fo, "PAGKNCR1", 8);
    wr(fo, &n32, 1);
    wr(fo, by_images.data(), by_images.size());
    wr(fo, by_values.data(), by_values.size());
    return fclose(fo) == 0 ? 0 : 5;
}

int main(int argc, char **argv)
{
    if (argc == 3) return run_patchmatch(argv[1], argv[2]);
    if (argc == 4 && strcmp(argv[1], "--ncc") == 0) return run_ncc(argv[2], argv[3]);
    fprintf(stderr, "usage: %s <case.in> <case.ref>\n       %s --ncc <case.ncc> <case.out>\n", argv[0], argv[0]);
    return 2;
}
