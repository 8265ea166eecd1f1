// ref_orb.cpp -- runs the reference's OWN src/ORBextractor.cc, compiled unchanged under its own include/ORBextractor.h against
// the stand-in OpenCV of ref_shim/orb, over a case file.  TEST INFRASTRUCTURE; built into oracle/_ref/ (never committed) by
// `make -C oracle ref` when the reference's sources are at $(REFERENCE).  The sibling of ref_patchmatch.cpp and ref_tracker.cpp.
//
//   ref_orb <case.in> <case.out>     one case: DetectFeatures() or operator()
//   ref_orb --table                  the sampling table the reference's constructor copies, 1024 integers as text on stdout
//                                    (tests/test_reference_orb_cpu.py reads it from the pipe; it is never written to a file)
//
// What is the reference's and what is not: every statement of src/ORBextractor.cc is the reference's text, compiled with its own
// flags (-O3, no -march).  Third-party arithmetic is the project's definition (oracle/README.md): cv::FAST, resize,
// copyMakeBorder, GaussianBlur and fastAtan2 are pagk_oracle_fast9 / _resize_linear / _border_reflect101 / _blur7 /
// _fast_atan2, cvRound rounds ties to even, std::cos(float) and std::sin(float) are pagk_oracle_sin_cos narrowed to float (sinf,
// cosf and sincosf are defined below and take precedence over libm's), and pow is pagk_oracle_pow_int (it aborts on an exponent
// that is no integer).
//
// The one step of the reference that depends on nothing in its input is sort() over pair<int, ExtractorNode *> (:708): nodes of
// equal size are ordered by their ADDRESSES.  Global operator new here is a monotone bump allocator, so the address order is the
// creation order: ascending by default -- the "creation number" rule of include/pagk.h -- and descending on a switch -- that
// rule reversed.  Built with -DREF_ORB_DEFAULT_ALLOC (ref_orb_san) the program keeps the default allocator, so that the
// sanitizer sees the heap; its results are then comparable only where no two sorted nodes have equal sizes.
//
// Case file (ref_arrays.h): img uint8 [H, W]; cfg int32 [8] = n_features, n_levels, ini_threshold, min_threshold,
//   mode (0 DetectFeatures, 1 operator()), descending allocator, border filled with 0xA5, own table (leave `pattern` as the
//   constructor made it); scale float32 [1]; mask uint8 [H, W] (optional: all ones, the reference dereferences an empty one);
//   pattern int32 [1024] (mode 1 without own table).
// Result file: scale, inv_scale float32 [L]; quota int32 [L]; umax int32 [16]; level_<l> uint8 [h_l, w_l] (the view, not the
//   border); kp float32 [n, 2]; size, response, angle float32 [n]; octave int32 [n]; desc uint8 [n, 32] (mode 1);
//   fast_log int32 [calls, 7] = level, x0, y0 (the sub-image's origin in the level image, from its data pointer), width, height,
//   threshold, keypoints returned; fast_keys float32 [total, 4] = call, x, y, response of every keypoint cv::FAST returned.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <sys/mman.h>

#include <ORBextractor.h>

#include "ref_arrays.h"

// ---- the definitions that stand for libm ---------------------------------------------------------------------------------------
extern "C" float sinf(float x) noexcept
{
    double sn, cs;
    pagk_oracle_sin_cos((double)x, &sn, &cs);
    return (float)sn;
}
extern "C" float cosf(float x) noexcept
{
    double sn, cs;
    pagk_oracle_sin_cos((double)x, &sn, &cs);
    return (float)cs;
}
// the compiler joins the cosine and the sine of :137 into one sincosf call
extern "C" void sincosf(float x, float *s, float *c) noexcept
{
    double sn, cs;
    pagk_oracle_sin_cos((double)x, &sn, &cs);
    *s = (float)sn, *c = (float)cs;
}
// pow((double)factor, (double)nlevels) of :461
extern "C" double pow(double base, double exponent) noexcept
{
    int32_t ok = 0;
    const double p = pagk_oracle_pow_int(base, exponent, &ok);
    if (!ok) cv::shim_unreachable("pow with an exponent that is no integer in [0, 64]");
    return p;
}

// ---- the allocator -------------------------------------------------------------------------------------------------------------
#ifndef REF_ORB_DEFAULT_ALLOC
namespace {
const size_t ARENA_BYTES = (size_t)1 << 32;   // address space only: pages are touched as they are used
unsigned char *g_arena = nullptr, *g_low = nullptr, *g_high = nullptr;
bool g_descending = false;

void *bump(size_t n)
{
    if (!g_arena) {
        void *p = mmap(nullptr, ARENA_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) abort();
        g_arena = g_low = (unsigned char *)p, g_high = g_arena + ARENA_BYTES;
    }
    n = (n + 15) & ~(size_t)15;
    if (n == 0) n = 16;
    if ((size_t)(g_high - g_low) < n) {
        fprintf(stderr, "ref_orb: the allocator's arena is used up\n");
        abort();
    }
    if (g_descending) return g_high -= n;
    void *p = g_low;
    g_low += n;
    return p;
}
}   // namespace
void *operator new(size_t n) { return bump(n); }
void *operator new[](size_t n) { return bump(n); }
void *operator new(size_t n, const std::nothrow_t &) noexcept { return bump(n); }
void *operator new[](size_t n, const std::nothrow_t &) noexcept { return bump(n); }
void operator delete(void *) noexcept {}
void operator delete[](void *) noexcept {}
void operator delete(void *, size_t) noexcept {}
void operator delete[](void *, size_t) noexcept {}
static void set_descending(bool on) { g_descending = on; }
#else
static void set_descending(bool) {}
#endif

// ---- the extractor with its protected members in reach -------------------------------------------------------------------------
namespace {
struct Extractor : ORB_SLAM2::ORBextractor {
    using ORB_SLAM2::ORBextractor::ORBextractor;
    using ORB_SLAM2::ORBextractor::mnFeaturesPerLevel;
    using ORB_SLAM2::ORBextractor::mvInvScaleFactor;
    using ORB_SLAM2::ORBextractor::mvScaleFactor;
    using ORB_SLAM2::ORBextractor::pattern;
    using ORB_SLAM2::ORBextractor::umax;
};

Extractor *g_ex = nullptr;
bool g_border_a5 = false;
std::vector<int32_t> g_fast_log;
std::vector<float> g_fast_keys;
}   // namespace

// ---- the stand-in's functions: each the oracle's definition ----------------------------------------------------------------------
namespace cv {

void FAST(InputArray image, std::vector<KeyPoint> &keypoints, int threshold, bool nms)
{
    const Mat sub = image.getMat();
    if (!nms) shim_unreachable("FAST without non-maximum suppression");
    // which level, and where in it: from the data pointer alone
    int level = -1, x0 = 0, y0 = 0;
    for (size_t l = 0; g_ex && l < g_ex->mvImagePyramid.size(); l++) {
        const Mat &lv = g_ex->mvImagePyramid[l];
        if (lv.empty() || lv.step != sub.step || sub.data < lv.data || sub.data >= lv.data + (size_t)lv.rows * lv.step) continue;
        const size_t off = (size_t)(sub.data - lv.data);
        level = (int)l, y0 = (int)(off / lv.step), x0 = (int)(off % lv.step);
    }
    const int cap = ((sub.cols + 1) / 2) * ((sub.rows + 1) / 2) + 1;   // at most one pixel of any 2 x 2 block survives
    std::vector<int32_t> xys((size_t)cap * 3);
    const int n = sub.empty() ? 0 : pagk_oracle_fast9(sub.data, (int64_t)sub.step, sub.cols, sub.rows, threshold, cap, xys.data());
    if (n < 0) shim_unreachable("a FAST result beyond its bound");
    keypoints.clear();
    const int32_t call = (int32_t)(g_fast_log.size() / 7);
    for (int k = 0; k < n; k++) {
        keypoints.push_back(KeyPoint((float)xys[3 * k], (float)xys[3 * k + 1], 7.f, -1.f, (float)xys[3 * k + 2]));
        for (float v : {(float)call, (float)xys[3 * k], (float)xys[3 * k + 1], (float)xys[3 * k + 2]}) g_fast_keys.push_back(v);
    }
    for (int32_t v : {level, x0, y0, sub.cols, sub.rows, threshold, n}) g_fast_log.push_back(v);
}

void resize(InputArray src_, OutputArray dst_, Size dsize, double fx, double fy, int interpolation)
{
    const Mat src = src_.getMat();
    if (fx != 0 || fy != 0 || interpolation != INTER_LINEAR) shim_unreachable("resize by factors or with another interpolation");
    dst_.create(dsize, src.type());   // the destination of :1220 has that size: its memory, a view into temp, stays
    Mat &dst = dst_.getMatRef();
    if (pagk_oracle_resize_linear(src.data, src.cols, src.rows, (int64_t)src.step, dst.data, dst.cols, dst.rows, (int64_t)dst.step))
        shim_unreachable("this resize");
}

void copyMakeBorder(InputArray src_, OutputArray dst_, int top, int bottom, int left, int right, int type)
{
    const Mat src = src_.getMat();
    if (top != bottom || top != left || top != right || (type != BORDER_REFLECT_101 && type != BORDER_REFLECT_101 + BORDER_ISOLATED))
        shim_unreachable("copyMakeBorder with unequal borders or another border type");
    dst_.create(src.rows + 2 * top, src.cols + 2 * top, src.type());   // temp of :1214 has that size: no reallocation
    Mat &dst = dst_.getMatRef();
    uchar *inner = dst.data + (size_t)top * dst.step + (size_t)top;
    if (src.data != inner)   // level 0 copies the image in; above, the source IS the interior of temp
        for (int r = 0; r < src.rows; r++) std::memmove(inner + (size_t)r * dst.step, src.ptr(r), (size_t)src.cols);
    if (pagk_oracle_border_reflect101(dst.data, (int64_t)dst.step, src.cols, src.rows, top, g_border_a5 ? 0xA5 : -1))
        shim_unreachable("this border");
}

void GaussianBlur(InputArray src_, OutputArray dst_, Size ksize, double sigma_x, double sigma_y, int type)
{
    const Mat src = src_.getMat().clone();   // the reference blurs in place
    if (ksize.width != 7 || ksize.height != 7 || sigma_x != 2 || sigma_y != 2 || type != BORDER_REFLECT_101)
        shim_unreachable("a Gaussian blur other than 7 x 7, sigma 2, BORDER_REFLECT_101");
    static const int32_t taps[4] = {54, 49, 34, 18};
    dst_.create(src.rows, src.cols, src.type());
    Mat &dst = dst_.getMatRef();
    if (pagk_oracle_blur7(src.data, src.cols, src.rows, (int64_t)src.step, taps, dst.data, (int64_t)dst.step)) shim_unreachable("this blur");
}

}   // namespace cv

int main(int argc, char **argv)
{
    using namespace ref_arrays;
    if (argc == 2 && std::string(argv[1]) == "--table") {
        Extractor ex(1, 1.2f, 1, 20, 7);
        for (const cv::Point &p : ex.pattern) printf("%d %d\n", p.x, p.y);
        return ex.pattern.size() == 512 ? 0 : 6;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: %s <case.in> <case.out> | --table\n", argv[0]);
        return 2;
    }
    Arrays in;
    if (!read_arrays(argv[1], in)) return 3;
    for (const char *need : {"img", "cfg", "scale"})
        if (!in.count(need)) return 3;
    const Array &im = in["img"];
    const int H = im.dims[0], W = im.dims[1];
    if (im.dtype != 0 || H < 1 || W < 1 || in["cfg"].count() != 8 || in["scale"].count() != 1) return 3;
    const int32_t *cfg = in["cfg"].as<int32_t>();
    const int n_features = cfg[0], n_levels = cfg[1], mode = cfg[4];
    const bool own_table = cfg[7] != 0;
    if (n_levels < 1 || n_levels > 8 || (mode != 0 && mode != 1)) return 3;
    if (mode == 1 && !own_table && (!in.count("pattern") || in["pattern"].count() != 1024)) return 3;
    if (in.count("mask") && (in["mask"].dims[0] != H || in["mask"].dims[1] != W)) return 3;

    cv::Mat image(H, W, CV_8UC1), mask(H, W, CV_8UC1);
    for (int r = 0; r < H; r++) {
        memcpy(image.ptr(r), im.as<uint8_t>() + (size_t)r * W, (size_t)W);
        if (in.count("mask")) memcpy(mask.ptr(r), in["mask"].as<uint8_t>() + (size_t)r * W, (size_t)W);
        else memset(mask.ptr(r), 1, (size_t)W);
    }
    g_border_a5 = cfg[6] != 0;
    set_descending(cfg[5] != 0);

    Extractor ex(n_features, in["scale"].as<float>()[0], n_levels, cfg[2], cfg[3]);
    g_ex = &ex;
    if (!own_table && in.count("pattern"))   // the sampling pattern is a case input
        for (int k = 0; k < 512; k++) ex.pattern[k] = cv::Point(in["pattern"].as<int32_t>()[2 * k], in["pattern"].as<int32_t>()[2 * k + 1]);

    std::vector<cv::KeyPoint> keys;
    cv::Mat desc;
    if (mode == 1) ex(image, mask, keys, desc);
    else ex.DetectFeatures(image, mask, keys);
    set_descending(false);

    Writer w(argv[2]);
    if (!w.f) return 5;
    w.f32("scale", ex.mvScaleFactor), w.f32("inv_scale", ex.mvInvScaleFactor);
    w.i32("quota", std::vector<int32_t>(ex.mnFeaturesPerLevel.begin(), ex.mnFeaturesPerLevel.end()));
    w.i32("umax", std::vector<int32_t>(ex.umax.begin(), ex.umax.end()));
    for (int l = 0; l < n_levels; l++) {
        const cv::Mat &lv = ex.mvImagePyramid[l];
        std::vector<uint8_t> px((size_t)lv.rows * lv.cols);
        for (int r = 0; r < lv.rows; r++) memcpy(px.data() + (size_t)r * lv.cols, lv.ptr(r), (size_t)lv.cols);
        w.put(("level_" + std::to_string(l)).c_str(), 0, 2, lv.rows, lv.cols, 1, px.data());
    }
    std::vector<float> kp, size, resp, angle;
    std::vector<int32_t> octave;
    for (const cv::KeyPoint &k : keys)
        kp.push_back(k.pt.x), kp.push_back(k.pt.y), size.push_back(k.size), resp.push_back(k.response), angle.push_back(k.angle), octave.push_back(k.octave);
    const int32_t n = (int32_t)keys.size();
    w.put("kp", 2, 2, n, 2, 1, kp.data());
    w.f32("size", size), w.f32("response", resp), w.f32("angle", angle), w.i32("octave", octave);
    if (mode == 1) {
        if (desc.rows != n || (n && desc.cols != 32)) return 6;
        std::vector<uint8_t> d((size_t)n * 32);
        for (int r = 0; r < n; r++) memcpy(d.data() + (size_t)r * 32, desc.ptr(r), 32);
        w.put("desc", 0, 2, n, 32, 1, d.data());
    }
    w.put("fast_log", 1, 2, (int32_t)(g_fast_log.size() / 7), 7, 1, g_fast_log.data());
    w.put("fast_keys", 2, 2, (int32_t)(g_fast_keys.size() / 4), 4, 1, g_fast_keys.data());
    return w.close();
}
