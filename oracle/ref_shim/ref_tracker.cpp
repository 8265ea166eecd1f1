// ref_tracker.cpp -- runs the reference's OWN src/gyro_aided_tracker.cpp (with src/patch_match.cpp and src/utils.cpp), compiled
// unchanged against the stand-ins of this directory and the reference's own include/gyro_aided_tracker.h, over a case file.
// TEST INFRASTRUCTURE; built into oracle/_ref/ (never committed) by `make -C oracle ref` when the reference's sources are at
// $(REFERENCE).  The sibling of ref_patchmatch.cpp.
//
//   ref_tracker --track    <case.in> <case.out> <scratch dir>   TrackFeatures(), eType 1-6
//   ref_tracker --validate <case.in> <case.out> <scratch dir>   GeometryValidation()
//   ref_tracker --search   <case.in> <case.out> <scratch dir>   SearchByGyroPredict()
//   ref_tracker --klt      <case.in> <case.out> <scratch dir>   TrackFeatures() eType 0, then SearchByOpencvKLT()
//
// The private functions are reached only through these public ones.  What is the reference's and what is not: every statement
// of src/gyro_aided_tracker.cpp is the reference's text, compiled with its own flags (-O3, no -march).  Third-party arithmetic
// is the project's definition (oracle/README.md): the cv::Mat products / transposes / inverses are pagk_oracle_mat_*, std::sin
// and std::cos of a float are pagk_oracle_sin_cos narrowed to float (sinf, cosf and sincosf are defined below and take
// precedence over libm's), radiusMatch is the stand-in's definition.  Whole third-party algorithms are INPUTS: findHomography and
// findFundamentalMat return the case's H21 and F21, calcOpticalFlowPyrLK returns the case's points, status and error.
//
// Case and result files: little endian, char magic[8] = "PAGKARR1"; int32 count; then count arrays, each
//   char name[24] (zero padded); int32 dtype (0 uint8, 1 int32, 2 float32, 3 float64); int32 ndim (<= 3); int32 dims[3];
//   the elements, row-major.
// Inputs (all modes): img_ref, img_cur uint8 [H, W]; cam float32 [9] = fx fy cx cy k1 k2 p1 p2 k3; cfg int32 [5] = n_dist_coef,
//   half_patch, eType, ePredictMethod, mbNCC; times float64 [2] = t_ref, t_cur; imu_t float64 [n]; imu_w float32 [n, 3];
//   bias float32 [3]; rbc float32 [9]; keys_ref, keys_ref_un float32 [N, 2]; keys_cur, keys_cur_un float32 [M, 2].
//   --validate adds status uint8 [N], pt_predict_un float32 [N, 2], H21, F21 float64 [9].
//   --klt adds lk_pt float32 [N, 2], lk_status uint8 [N], lk_err float32 [N] for each of the two LK calls (lk_*, lk2_*).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// angle brackets: the include path alone decides, and on it the reference's own include/gyro_aided_tracker.h comes before the
// stand-in of that name that lies next to this file
#include <gyro_aided_tracker.h>

extern "C" double log(double x) noexcept { return pagk_oracle_log(x); }
// std::sin(float) / std::cos(float) (src/gyro_aided_tracker.cpp:583): the project's definition, narrowed to float
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
// <cmath>'s std::sin(float) is __builtin_sinf, which no -fno-builtin flag reaches: the compiler joins the sine and the cosine of
// :583 into one sincosf call.  Defined here as well, so that no member of the family resolves to libm
// (tests/test_reference_tracker_cpu.py looks at the program's undefined symbols).
extern "C" void sincosf(float x, float *s, float *c) noexcept
{
    double sn, cs;
    pagk_oracle_sin_cos((double)x, &sn, &cs);
    *s = (float)sn, *c = (float)cs;
}

namespace {

struct Array {
    int32_t dtype = 0, ndim = 0, dims[3] = {1, 1, 1};
    std::vector<uint8_t> bytes;
    size_t count() const { return (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2]; }
    template <typename T> const T *as() const { return reinterpret_cast<const T *>(bytes.data()); }
};
const size_t ELEM[4] = {1, 4, 4, 8};
typedef std::map<std::string, Array> Arrays;

bool read_arrays(const char *path, Arrays &out)
{
    FILE *f = fopen(path, "rb");
    char magic[8];
    int32_t count = 0;
    if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "PAGKARR1", 8) != 0 || fread(&count, 4, 1, f) != 1) return false;
    for (int32_t k = 0; k < count; k++) {
        char name[25] = {0};
        Array a;
        if (fread(name, 1, 24, f) != 24 || fread(&a.dtype, 4, 1, f) != 1 || fread(&a.ndim, 4, 1, f) != 1 || fread(a.dims, 4, 3, f) != 3) return false;
        if (a.dtype < 0 || a.dtype > 3 || a.ndim < 0 || a.ndim > 3 || a.dims[0] < 0 || a.dims[1] < 0 || a.dims[2] < 0) return false;
        a.bytes.resize(a.count() * ELEM[a.dtype]);
        if (!a.bytes.empty() && fread(a.bytes.data(), 1, a.bytes.size(), f) != a.bytes.size()) return false;
        out[name] = a;
    }
    fclose(f);
    return true;
}

struct Writer {
    FILE *f;
    int32_t count = 0;
    explicit Writer(const char *path) : f(fopen(path, "wb"))
    {
        if (f) fwrite("PAGKARR1", 1, 8, f), fwrite(&count, 4, 1, f);
    }
    void put(const char *name, int32_t dtype, int32_t ndim, int32_t d0, int32_t d1, int32_t d2, const void *data)
    {
        char nm[24] = {0};
        strncpy(nm, name, 23);
        const int32_t dims[3] = {d0, d1, d2};
        fwrite(nm, 1, 24, f), fwrite(&dtype, 4, 1, f), fwrite(&ndim, 4, 1, f), fwrite(dims, 4, 3, f);
        const size_t n = (size_t)d0 * (size_t)d1 * (size_t)d2 * ELEM[dtype];
        if (n) fwrite(data, 1, n, f);
        count++;
    }
    void i32(const char *name, int32_t v) { put(name, 1, 1, 1, 1, 1, &v); }
    void points(const char *name, const std::vector<cv::Point2f> &v)
    {
        std::vector<float> xy;
        for (const cv::Point2f &p : v) xy.push_back(p.x), xy.push_back(p.y);
        put(name, 2, 2, (int32_t)v.size(), 2, 1, xy.data());
    }
    void mat(const char *name, const cv::Mat &m)
    {
        std::vector<float> v;
        for (int r = 0; r < m.rows; r++)
            for (int c = 0; c < m.cols; c++) v.push_back(m.at<float>(r, c));
        put(name, 2, 2, m.rows, m.cols, 1, v.data());
    }
    int close()
    {
        if (fseek(f, 8, SEEK_SET) != 0 || fwrite(&count, 4, 1, f) != 1) return 5;
        return fclose(f) == 0 ? 0 : 5;
    }
};

// the inputs that stand for third-party algorithms
const Arrays *g_case = nullptr;
int g_lk_calls = 0;

std::vector<cv::KeyPoint> keypoints(const Arrays &in, const char *name)
{
    std::vector<cv::KeyPoint> v;
    const Arrays::const_iterator it = in.find(name);
    if (it == in.end()) return v;
    const float *p = it->second.as<float>();
    for (int32_t i = 0; i < it->second.dims[0]; i++) v.push_back(cv::KeyPoint(p[2 * i], p[2 * i + 1], 1.f));
    return v;
}

cv::Mat mat_f64_3x3(const Array &a)
{
    cv::Mat m(3, 3, CV_64F);
    for (int k = 0; k < 9; k++) m.at<double>(k / 3, k % 3) = a.as<double>()[k];
    return m;
}

}   // namespace

namespace cv {
Mat findHomography(const std::vector<Point2f> &, const std::vector<Point2f> &, int, double, Mat &) { return mat_f64_3x3(g_case->at("H21")); }
Mat findFundamentalMat(const std::vector<Point2f> &, const std::vector<Point2f> &, int, double, double, Mat &) { return mat_f64_3x3(g_case->at("F21")); }
void calcOpticalFlowPyrLK(const Mat &, const Mat &, const std::vector<Point2f> &prev_pts, std::vector<Point2f> &next_pts,
                          std::vector<uchar> &status, std::vector<float> &err, Size, int, TermCriteria, int, double)
{
    const bool second = g_lk_calls++ > 0 && g_case->count("lk2_pt");
    const Array &pt = g_case->at(second ? "lk2_pt" : "lk_pt"), &st = g_case->at(second ? "lk2_status" : "lk_status"),
                &er = g_case->at(second ? "lk2_err" : "lk_err");
    const size_t n = prev_pts.size();
    if ((size_t)pt.dims[0] != n || st.count() != n || er.count() != n) shim_unreachable("an LK result of another size than the points");
    next_pts.resize(n), status.resize(n), err.resize(n);
    for (size_t i = 0; i < n; i++) next_pts[i] = Point2f(pt.as<float>()[2 * i], pt.as<float>()[2 * i + 1]), status[i] = st.as<uint8_t>()[i], err[i] = er.as<float>()[i];
}
}   // namespace cv

static void write_track_state(Writer &w, GyroAidedTracker &t)
{
    const int32_t N = t.mN;
    w.mat("Rcl", t.mRcl), w.mat("KRKinv", t.mKRKinv);
    w.points("pt_predict", t.mvPtPredict), w.points("pt_predict_un", t.mvPtPredictUn);
    w.points("pt_gyro_predict", t.mvPtGyroPredict), w.points("pt_gyro_predict_un", t.mvPtGyroPredictUn);
    w.put("status", 0, 1, (int32_t)t.mvStatus.size(), 1, 1, t.mvStatus.data());
    w.points("flows_predict_un", t.mvFlowsPredictUn);
    // the affine matrices and the corner flows: zeros where the reference left the entry empty, affine_set says which
    std::vector<float> aff((size_t)N * 4, 0.f), corners((size_t)N * 8, 0.f);
    std::vector<uint8_t> aff_set((size_t)N, 0);
    for (int32_t i = 0; i < N; i++) {
        const cv::Mat &A = t.mvAffineDeformationMatrix[i];
        if (!A.empty()) {
            aff_set[i] = 1;
            for (int k = 0; k < 4; k++) aff[4 * (size_t)i + k] = A.at<float>(k / 2, k % 2);
        }
        const std::vector<cv::Point2f> &c = t.mvvFlowsPredictCorners[i];
        for (size_t j = 0; j < c.size() && j < 4; j++) corners[8 * (size_t)i + 2 * j] = c[j].x, corners[8 * (size_t)i + 2 * j + 1] = c[j].y;
    }
    w.put("affine", 2, 2, N, 4, 1, aff.data()), w.put("affine_set", 0, 1, N, 1, 1, aff_set.data());
    w.put("corner_flows", 2, 3, N, 4, 2, corners.data());
    if ((int32_t)t.mvStatusAfterPatchMatched.size() == N && t.mType != GyroAidedTracker::GYRO_PREDICT && t.mType != GyroAidedTracker::OPENCV_OPTICAL_FLOW_PYR_LK) {
        w.points("pm_pt", t.mvPtPredictAfterPatchMatched), w.points("pm_pt_un", t.mvPtPredictAfterPatchMatchedUn);
        w.put("pm_status", 0, 1, N, 1, 1, t.mvStatusAfterPatchMatched.data());
        w.put("pm_pix_err", 3, 1, N, 1, 1, t.mvPixelErrorsOfPatchMatched.data());
        w.put("pm_dist_pred", 3, 1, N, 1, 1, t.mvDistanceBetweenPredictedAndPatchMatched.data());
        w.put("pm_ncc", 2, 1, N, 1, 1, t.mvNccAfterPatchMatched.data());
    }
}

static void write_matches(Writer &w, const std::vector<GyroAidedTracker::sMatch> &m)
{
    std::vector<int32_t> q, tr, lv;
    std::vector<float> d, c;
    for (const GyroAidedTracker::sMatch &x : m) q.push_back(x.queryIdx), tr.push_back(x.trainIdx), lv.push_back(x.level), d.push_back(x.distance), c.push_back(x.ncc);
    const int32_t k = (int32_t)m.size();
    w.put("match_query", 1, 1, k, 1, 1, q.data()), w.put("match_train", 1, 1, k, 1, 1, tr.data()), w.put("match_level", 1, 1, k, 1, 1, lv.data());
    w.put("match_dist", 2, 1, k, 1, 1, d.data()), w.put("match_ncc", 2, 1, k, 1, 1, c.data());
}

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s --track|--validate|--search|--klt <case.in> <case.out> <scratch dir>\n", argv[0]);
        return 2;
    }
    const std::string mode = argv[1];
    Arrays in;
    if (!read_arrays(argv[2], in)) return 3;
    g_case = &in;
    for (const char *need : {"img_ref", "img_cur", "cam", "cfg", "times", "imu_t", "imu_w", "bias", "rbc", "keys_ref", "keys_ref_un"})
        if (!in.count(need)) return 3;
    const Array &ir = in["img_ref"], &ic = in["img_cur"];
    const int H = ir.dims[0], W = ir.dims[1];
    const int32_t *cfg = in["cfg"].as<int32_t>();
    const float *cam = in["cam"].as<float>();
    if (H < 1 || W < 1 || ic.dims[0] != H || ic.dims[1] != W || in["cfg"].count() != 5 || in["cam"].count() != 9 || (cfg[0] != 4 && cfg[0] != 5)) return 3;
    cv::Mat ref(H, W, CV_8UC1), cur(H, W, CV_8UC1);
    for (int r = 0; r < H; r++) memcpy(ref.ptr<uint8_t>(r), ir.as<uint8_t>() + (size_t)r * W, (size_t)W), memcpy(cur.ptr<uint8_t>(r), ic.as<uint8_t>() + (size_t)r * W, (size_t)W);
    cv::Mat K = cv::Mat::eye(3, 3, CV_32F), dist(cfg[0], 1, CV_32F), rbc(3, 3, CV_32F), no_table;
    K.at<float>(0, 0) = cam[0], K.at<float>(1, 1) = cam[1], K.at<float>(0, 2) = cam[2], K.at<float>(1, 2) = cam[3];
    for (int k = 0; k < cfg[0]; k++) dist.at<float>(k) = cam[4 + k];
    for (int k = 0; k < 9; k++) rbc.at<float>(k / 3, k % 3) = in["rbc"].as<float>()[k];
    const std::vector<cv::KeyPoint> keys_ref = keypoints(in, "keys_ref"), keys_ref_un = keypoints(in, "keys_ref_un"),
                                    keys_cur = keypoints(in, "keys_cur"), keys_cur_un = keypoints(in, "keys_cur_un");
    if (keys_ref.size() != keys_ref_un.size() || keys_cur.size() != keys_cur_un.size()) return 3;
    std::vector<IMU::Point> imu;
    const Array &it = in["imu_t"], &iw = in["imu_w"];
    if (iw.count() != 3 * it.count()) return 3;
    for (size_t i = 0; i < it.count(); i++) imu.push_back(IMU::Point(0.f, 0.f, 0.f, iw.as<float>()[3 * i], iw.as<float>()[3 * i + 1], iw.as<float>()[3 * i + 2], it.as<double>()[i]));
    const cv::Point3f bias(in["bias"].as<float>()[0], in["bias"].as<float>()[1], in["bias"].as<float>()[2]);
    std::string scratch = argv[4];
    if (scratch.empty() || scratch.back() != '/') scratch += '/';

    GyroAidedTracker tracker(in["times"].as<double>()[1], in["times"].as<double>()[0], ref, cur, keys_ref, keys_cur, keys_ref_un, keys_cur_un, imu,
                             bias, K, dist, no_table, (GyroAidedTracker::eType)cfg[2], (GyroAidedTracker::ePredictMethod)cfg[3], scratch, cfg[1]);
    tracker.mRbc = rbc;   // the raw-arguments constructor leaves it empty
    tracker.mbNCC = cfg[4] != 0;
    const int32_t N = tracker.mN;

    Writer w(argv[3]);
    if (!w.f) return 5;
    if (mode == "--track") {
        if (cfg[2] < 1 || cfg[2] > 6) return 3;
        w.i32("ret", tracker.TrackFeatures());
        write_track_state(w, tracker);
    } else if (mode == "--validate") {
        if (!in.count("status") || !in.count("pt_predict_un") || !in.count("H21") || !in.count("F21") || (int32_t)in["status"].count() != N ||
            in["pt_predict_un"].dims[0] != N)
            return 3;
        for (int32_t i = 0; i < N; i++) {
            tracker.mvStatus[i] = in["status"].as<uint8_t>()[i];
            tracker.mvPtPredictUn[i] = cv::Point2f(in["pt_predict_un"].as<float>()[2 * i], in["pt_predict_un"].as<float>()[2 * i + 1]);
        }
        w.i32("ret", tracker.GeometryValidation());
        w.put("status", 0, 1, N, 1, 1, tracker.mvStatus.data());
        // H12 as CheckHomography computes it (:598), for the callers that take it as an argument
        const cv::Mat H12 = mat_f64_3x3(in["H21"]).inv();
        double h12[9];
        for (int k = 0; k < 9; k++) h12[k] = H12.at<double>(k / 3, k % 3);
        w.put("H12", 3, 1, 9, 1, 1, h12);
    } else if (mode == "--search") {
        if (cfg[2] < 1 || cfg[2] > 6) return 3;
        w.i32("ret", tracker.SearchByGyroPredict());
        write_track_state(w, tracker);
        int32_t cap = 1;
        for (int32_t i = 0; i < N; i++) cap = std::max(cap, (int32_t)tracker.mvvNearNeighbors[i].size());
        std::vector<int32_t> count((size_t)N), idx((size_t)N * cap, -1), level((size_t)N * cap, 0);
        std::vector<float> d((size_t)N * cap, 0.f), c((size_t)N * cap, 0.f);
        for (int32_t i = 0; i < N; i++) {
            const std::vector<GyroAidedTracker::sMatch> &l = tracker.mvvNearNeighbors[i];
            count[i] = (int32_t)l.size();
            for (size_t j = 0; j < l.size(); j++) {
                if (l[j].queryIdx != i) return 6;
                idx[(size_t)i * cap + j] = l[j].trainIdx, level[(size_t)i * cap + j] = l[j].level, d[(size_t)i * cap + j] = l[j].distance, c[(size_t)i * cap + j] = l[j].ncc;
            }
        }
        w.put("nbr_count", 1, 1, N, 1, 1, count.data()), w.put("nbr_idx", 1, 2, N, cap, 1, idx.data()), w.put("nbr_level", 1, 2, N, cap, 1, level.data());
        w.put("nbr_dist", 2, 2, N, cap, 1, d.data()), w.put("nbr_ncc", 2, 2, N, cap, 1, c.data());
        write_matches(w, tracker.mvMatches);
        w.points("flows_error_un", tracker.mvFlowsErrorUn);
    } else if (mode == "--klt") {
        if (cfg[2] != 0 || !in.count("lk_pt") || !in.count("lk_status") || !in.count("lk_err")) return 3;
        tracker.TrackFeatures();   // type 0 returns an indeterminate count (n_predict is never assigned, :350-380): not written
        w.mat("Rcl", tracker.mRcl), w.mat("KRKinv", tracker.mKRKinv);
        w.points("track_pt_predict", tracker.mvPtPredict), w.points("track_pt_predict_un", tracker.mvPtPredictUn);
        w.put("track_status", 0, 1, (int32_t)tracker.mvStatus.size(), 1, 1, tracker.mvStatus.data());
        w.points("flows_predict_un", tracker.mvFlowsPredictUn);
        w.i32("ret", tracker.SearchByOpencvKLT());
        w.points("pt_predict", tracker.mvPtPredict);
        w.put("status", 0, 1, (int32_t)tracker.mvStatus.size(), 1, 1, tracker.mvStatus.data());
        write_matches(w, tracker.mvMatches);
        w.put("disparities", 3, 1, (int32_t)tracker.mvDisparities.size(), 1, 1, tracker.mvDisparities.data());
    } else
        return 2;
    return w.close();
}
