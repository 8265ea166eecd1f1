// Stand-in for the slice of OpenCV that the reference's src/patch_match.cpp, src/utils.cpp and src/gyro_aided_tracker.cpp
// (with the headers that file pulls in: gyro_aided_tracker.h, imu_types.h, frame.h, ORBextractor.h) touch.
//
// TEST INFRASTRUCTURE (oracle/README.md, "The reference's own text, compiled").  Project text, written from OpenCV's
// documented interfaces: it exists so that the two reference sources compile UNCHANGED and their own statements -- the
// promotions, the loop order, the clamps, the branches -- can be run against the oracle.  It is not OpenCV: only the members
// those files use exist, and the arithmetic OpenCV itself would contribute (cv::resize, the cv::Mat products, transposes
// and inverses) is the oracle's definition (pagk_oracle_pyr_down, pagk_oracle_mat_*).  Whole third-party algorithms -- the
// RANSAC fits, calcOpticalFlowPyrLK -- are only declared here: a program that reaches them defines them and returns the
// matrices and points its case supplies (ref_tracker.cpp).
//
// cv::Mat here owns zero-initialised memory with two extra rows and 16 bytes of slack behind the image, and may carry a row
// step larger than cols whose padding bytes are zero: the samplers of the reference read past the image at its right and
// bottom edge -- the member GetPixelValue up to one row and one byte, the free one of include/utils.h (whose `>` clamp lets
// y == rows through) up to two rows and one byte -- and those taps then land on the values oracle and product define (0).
#ifndef PAGK_REF_SHIM_OPENCV_HPP
#define PAGK_REF_SHIM_OPENCV_HPP

#include <algorithm>
#include <cassert>   // (OpenCV's core headers bring assert() with them; the reference relies on it)
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../../pagk_oracle.h"

typedef unsigned char uchar;

#define CV_8U 0
#define CV_32F 5
#define CV_64F 6
#define CV_MAKETYPE(depth, cn) ((depth) + (((cn) - 1) << 3))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_32FC2 CV_MAKETYPE(CV_32F, 2)

namespace cv {

[[noreturn]] inline void shim_unreachable(const char *what)
{
    std::fprintf(stderr, "ref_shim: %s is not part of the stand-in (never reached on the PatchMatch path)\n", what);
    std::abort();
}

// OpenCV's Point_<T>: scaling by an int / float / double multiplies in the wider of the two types and narrows to T
// (saturate_cast<float> of a double is a plain conversion); division exists as operator/=(Point_&, double) etc.
template <typename T>
struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<float> Point2f;
typedef Point_<int> Point2i;
typedef Point2i Point;

// Point3_<T>: the same promotion rules
template <typename T>
struct Point3_ {
    T x, y, z;
    Point3_() : x(0), y(0), z(0) {}
    Point3_(T x_, T y_, T z_) : x(x_), y(y_), z(z_) {}
};
typedef Point3_<float> Point3f;
template <typename T> inline Point3_<T> operator+(const Point3_<T> &a, const Point3_<T> &b) { return Point3_<T>(T(a.x + b.x), T(a.y + b.y), T(a.z + b.z)); }
template <typename T> inline Point3_<T> operator-(const Point3_<T> &a, const Point3_<T> &b) { return Point3_<T>(T(a.x - b.x), T(a.y - b.y), T(a.z - b.z)); }
template <typename T> inline Point3_<T> operator*(const Point3_<T> &a, float b) { return Point3_<T>(T(a.x * b), T(a.y * b), T(a.z * b)); }
template <typename T> inline Point3_<T> operator*(const Point3_<T> &a, double b) { return Point3_<T>(T(a.x * b), T(a.y * b), T(a.z * b)); }

template <typename T> inline Point_<T> operator+(const Point_<T> &a, const Point_<T> &b) { return Point_<T>(T(a.x + b.x), T(a.y + b.y)); }
template <typename T> inline Point_<T> operator-(const Point_<T> &a, const Point_<T> &b) { return Point_<T>(T(a.x - b.x), T(a.y - b.y)); }
template <typename T> inline Point_<T> operator*(const Point_<T> &a, int b) { return Point_<T>(T(a.x * b), T(a.y * b)); }
template <typename T> inline Point_<T> operator*(const Point_<T> &a, float b) { return Point_<T>(T(a.x * b), T(a.y * b)); }
template <typename T> inline Point_<T> operator*(const Point_<T> &a, double b) { return Point_<T>(T(a.x * b), T(a.y * b)); }
template <typename T> inline Point_<T> operator*(int a, const Point_<T> &b) { return Point_<T>(T(b.x * a), T(b.y * a)); }
template <typename T> inline Point_<T> operator*(float a, const Point_<T> &b) { return Point_<T>(T(b.x * a), T(b.y * a)); }
template <typename T> inline Point_<T> operator*(double a, const Point_<T> &b) { return Point_<T>(T(b.x * a), T(b.y * a)); }
template <typename T> inline Point_<T> operator/(const Point_<T> &a, int b) { return Point_<T>(T(a.x / b), T(a.y / b)); }
template <typename T> inline Point_<T> operator/(const Point_<T> &a, float b) { return Point_<T>(T(a.x / b), T(a.y / b)); }
template <typename T> inline Point_<T> operator/(const Point_<T> &a, double b) { return Point_<T>(T(a.x / b), T(a.y / b)); }

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct Range {
    int start, end;
    Range() : start(0), end(0) {}
    Range(int s, int e) : start(s), end(e) {}
};

template <typename T, int N>
struct Vec {
    T val[N];
    T &operator[](int i) { return val[i]; }
    const T &operator[](int i) const { return val[i]; }
};
typedef Vec<float, 2> Vec2f;

struct KeyPoint {
    Point2f pt;
    float size;
    KeyPoint() : size(0) {}
    KeyPoint(float x, float y, float size_) : pt(x, y), size(size_) {}
};

struct MatExpr;

class Mat {
public:
    int rows, cols;
    uchar *data;
    size_t step;   // bytes per row

    Mat() : rows(0), cols(0), data(nullptr), step(0), elem_(0) {}
    Mat(int rows_, int cols_, int type) { create(rows_, cols_, type, 0); }
    Mat(Size size, int type) { create(size.height, size.width, type, 0); }
    // not in OpenCV's interface: a Mat with a chosen row step (a non-continuous image; the padding bytes stay 0)
    static Mat with_step(int rows_, int cols_, int type, size_t step_bytes)
    {
        Mat m;
        m.create(rows_, cols_, type, step_bytes);
        return m;
    }

    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    size_t total() const { return (size_t)rows * (size_t)cols; }
    size_t elemSize() const { return elem_; }

    template <typename T> T &at(int r, int c) { return *reinterpret_cast<T *>(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    template <typename T> const T &at(int r, int c) const { return *reinterpret_cast<const T *>(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    // single index: element i of a vector stored as one row or as one column
    template <typename T> T &at(int i) { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
    template <typename T> const T &at(int i) const { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
    template <typename T> T *ptr(int r) { return reinterpret_cast<T *>(data + (size_t)r * step); }
    template <typename T> const T *ptr(int r) const { return reinterpret_cast<const T *>(data + (size_t)r * step); }

    // ---- what src/gyro_aided_tracker.cpp adds: small float / double matrices.  A copy shares the buffer, as in OpenCV. ----
    int type() const { return type_; }
    static Mat zeros(int rows_, int cols_, int type) { return Mat(rows_, cols_, type); }
    static Mat eye(int rows_, int cols_, int type)
    {
        Mat m(rows_, cols_, type);
        for (int i = 0; i < std::min(rows_, cols_); i++) {
            if (type == CV_32F) m.at<float>(i, i) = 1.0f;
            else if (type == CV_64F) m.at<double>(i, i) = 1.0;
            else shim_unreachable("cv::Mat::eye of this type");
        }
        return m;
    }
    // Mat(vector<Point2f>): N x 1, two channels (the data is copied here; nothing on the path writes through it)
    explicit Mat(const std::vector<Point2f> &v)
    {
        create((int)v.size(), 1, CV_32FC2, 0);
        for (size_t i = 0; i < v.size(); i++) at<Vec2f>((int)i, 0)[0] = v[i].x, at<Vec2f>((int)i, 0)[1] = v[i].y;
    }
    // reshape(1) / reshape(1, rows) of a continuous two-channel column: the same floats as rows x 2, one channel
    Mat reshape(int cn, int new_rows = 0) const
    {
        if (cn != 1 || type_ != CV_32FC2 || cols != 1 || (new_rows != 0 && new_rows != rows)) shim_unreachable("cv::Mat::reshape of this shape");
        Mat m(rows, 2, CV_32F);
        if (rows > 0) std::memcpy(m.data, data, (size_t)rows * 2 * sizeof(float));
        return m;
    }
    Mat clone() const
    {
        Mat m = with_step(rows, cols, type_, step);
        if (data) std::memcpy(m.data, data, (size_t)rows * step);
        return m;
    }
    void copyTo(Mat &dst) const { dst = clone(); }
    Mat colRange(int c0, int c1) const { return block(0, rows, c0, c1); }
    Mat rowRange(int r0, int r1) const { return block(r0, r1, 0, cols); }
    Mat t() const
    {
        Mat m(cols, rows, type_);
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) {
                if (type_ == CV_32F) m.at<float>(c, r) = at<float>(r, c);
                else if (type_ == CV_64F) m.at<double>(c, r) = at<double>(r, c);
                else shim_unreachable("cv::Mat::t of this type");
            }
        return m;
    }
    // inv(): third-party arithmetic, the oracle's definitions (oracle/README.md)
    Mat inv() const
    {
        Mat m(rows, cols, type_);
        float a[9], o[9];
        if (type_ == CV_32F && rows == cols && (rows == 2 || rows == 3)) {
            for (int r = 0; r < rows; r++)
                for (int c = 0; c < cols; c++) a[r * cols + c] = at<float>(r, c);
            if (rows == 2) pagk_oracle_mat_inv2(a, o);
            else pagk_oracle_mat_inv3(a, o);
            for (int r = 0; r < rows; r++)
                for (int c = 0; c < cols; c++) m.at<float>(r, c) = o[r * cols + c];
        } else if (type_ == CV_64F && rows == 3 && cols == 3) {
            double ad[9], od[9];
            for (int k = 0; k < 9; k++) ad[k] = at<double>(k / 3, k % 3);
            pagk_oracle_mat_inv3d(ad, od);
            for (int k = 0; k < 9; k++) m.at<double>(k / 3, k % 3) = od[k];
        } else
            shim_unreachable("cv::Mat::inv of this shape");
        return m;
    }
    Mat &operator*=(const Mat &b);
    Mat(const MatExpr &e);
    Mat &operator=(const MatExpr &e);

private:
    Mat block(int r0, int r1, int c0, int c1) const
    {
        Mat m(r1 - r0, c1 - c0, type_);
        for (int r = r0; r < r1; r++) std::memcpy(m.data + (size_t)(r - r0) * m.step, data + (size_t)r * step + (size_t)c0 * elem_, (size_t)(c1 - c0) * elem_);
        return m;
    }
    void create(int rows_, int cols_, int type, size_t step_bytes)
    {
        const int depth = type & 7, cn = (type >> 3) + 1;
        elem_ = (size_t)(depth == CV_64F ? 8 : depth == CV_32F ? 4 : 1) * (size_t)cn;
        type_ = type;
        rows = rows_, cols = cols_;
        step = step_bytes ? step_bytes : (size_t)cols_ * elem_;
        if (step < (size_t)cols_ * elem_) shim_unreachable("a row step below the row length");
        const size_t bytes = ((size_t)rows_ + 2) * step + 16;   // two zero rows and 16 zero bytes behind the image
        buf_ = std::shared_ptr<uchar>(static_cast<uchar *>(std::calloc(bytes, 1)), std::free);
        data = buf_.get();
    }
    std::shared_ptr<uchar> buf_;
    size_t elem_;
    int type_ = 0;
};

// ---- cv::Mat algebra of src/gyro_aided_tracker.cpp (CV_32F, one channel) ------------------------------------------------
// Third-party arithmetic, defined by the project (oracle/README.md): a product of two matrices is pagk_oracle_mat_mul (f32
// factors, an f64 accumulator, one rounding per element, narrowed per product); a sum of two matrices is an f32 sum; a matrix
// scaled or divided by a scalar becomes an expression whose elements stay f64 -- scaled, divided and added in the order the
// source writes them -- and are rounded to f32 once, where the expression is stored into a Mat.
struct MatExpr {
    int rows, cols;
    std::vector<double> v;
};
inline std::vector<float> shim_floats(const Mat &a)
{
    if (a.type() != CV_32F) shim_unreachable("cv::Mat algebra on another type than CV_32F");
    std::vector<float> v((size_t)a.rows * (size_t)a.cols);
    for (int r = 0; r < a.rows; r++)
        for (int c = 0; c < a.cols; c++) v[(size_t)r * a.cols + c] = a.at<float>(r, c);
    return v;
}
inline Mat shim_mat(int rows, int cols, const float *v)
{
    Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) m.at<float>(r, c) = v[(size_t)r * cols + c];
    return m;
}
inline Mat operator*(const Mat &a, const Mat &b)
{
    if (a.cols != b.rows) shim_unreachable("cv::Mat product of these shapes");
    const std::vector<float> fa = shim_floats(a), fb = shim_floats(b);
    std::vector<float> o((size_t)a.rows * (size_t)b.cols);
    if (pagk_oracle_mat_mul(a.rows, a.cols, b.cols, fa.data(), fb.data(), o.data()) != 0) shim_unreachable("cv::Mat product of an empty matrix");
    return shim_mat(a.rows, b.cols, o.data());
}
inline Mat &Mat::operator*=(const Mat &b) { return *this = *this * b; }
inline Mat operator+(const Mat &a, const Mat &b)
{
    if (a.rows != b.rows || a.cols != b.cols) shim_unreachable("cv::Mat sum of these shapes");
    const std::vector<float> fa = shim_floats(a), fb = shim_floats(b);
    std::vector<float> o(fa.size());
    for (size_t k = 0; k < o.size(); k++) o[k] = fa[k] + fb[k];
    return shim_mat(a.rows, a.cols, o.data());
}
inline MatExpr shim_expr(const Mat &a)
{
    const std::vector<float> fa = shim_floats(a);
    MatExpr e{a.rows, a.cols, std::vector<double>(fa.begin(), fa.end())};
    return e;
}
inline MatExpr operator*(const Mat &a, double s)
{
    MatExpr e = shim_expr(a);
    for (double &x : e.v) x = x * s;
    return e;
}
inline MatExpr operator*(MatExpr e, double s)
{
    for (double &x : e.v) x = x * s;
    return e;
}
inline MatExpr operator/(MatExpr e, double s)
{
    for (double &x : e.v) x = x / s;
    return e;
}
inline MatExpr operator/(const Mat &a, double s) { return shim_expr(a) / s; }
inline MatExpr operator+(MatExpr a, const MatExpr &b)
{
    if (a.rows != b.rows || a.cols != b.cols) shim_unreachable("cv::MatExpr sum of these shapes");
    for (size_t k = 0; k < a.v.size(); k++) a.v[k] = a.v[k] + b.v[k];
    return a;
}
inline MatExpr operator+(const Mat &a, const MatExpr &b) { return shim_expr(a) + b; }
inline MatExpr operator+(const MatExpr &a, const Mat &b) { return a + shim_expr(b); }
inline Mat::Mat(const MatExpr &e)
{
    create(e.rows, e.cols, CV_32F, 0);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) at<float>(r, c) = (float)e.v[(size_t)r * cols + c];
}
inline Mat &Mat::operator=(const MatExpr &e) { return *this = Mat(e); }

// (cv::Mat_<float>(3,3) << a, b, ...): each value converted to T, row by row
template <typename T>
struct MatCommaInitializer_ {
    Mat m;
    int k;
    template <typename V> MatCommaInitializer_ &operator,(V v)
    {
        m.at<T>(k / m.cols, k % m.cols) = T(v);
        k++;
        return *this;
    }
    operator Mat() const { return m; }
};
template <typename T>
struct Mat_ : Mat {
    Mat_(int rows_, int cols_) : Mat(rows_, cols_, sizeof(T) == 8 ? CV_64F : CV_32F) {}
};
template <typename T, typename V> inline MatCommaInitializer_<T> operator<<(const Mat_<T> &m, V v)
{
    MatCommaInitializer_<T> ci{m, 0};
    return (ci, v);
}

// ---- names that only have to parse, and third-party algorithms that a case supplies ---------------------------------------
typedef const Mat &InputArray;
typedef Mat &OutputArray;
struct TermCriteria {
    enum { COUNT = 1, MAX_ITER = COUNT, EPS = 2 };
    int type, maxCount;
    double epsilon;
    TermCriteria(int type_, int maxCount_, double epsilon_) : type(type_), maxCount(maxCount_), epsilon(epsilon_) {}
};
enum { RANSAC = 8, FM_RANSAC = 8, NORM_L2 = 4 };
#define CV_FM_RANSAC cv::FM_RANSAC
inline Mat getOptimalNewCameraMatrix(const Mat &, const Mat &, Size, double, Size, int) { shim_unreachable("cv::getOptimalNewCameraMatrix"); }
inline void initUndistortRectifyMap(const Mat &, const Mat &, const Mat &, const Mat &, Size, int, Mat &, Mat &) { shim_unreachable("cv::initUndistortRectifyMap"); }
// inputs of a case, defined by the program that links the tracker (oracle/ref_shim/ref_tracker.cpp)
Mat findHomography(const std::vector<Point2f> &pts1, const std::vector<Point2f> &pts2, int method, double threshold, Mat &mask);
Mat findFundamentalMat(const std::vector<Point2f> &pts1, const std::vector<Point2f> &pts2, int method, double threshold, double confidence, Mat &mask);
void calcOpticalFlowPyrLK(const Mat &prev, const Mat &next, const std::vector<Point2f> &prev_pts, std::vector<Point2f> &next_pts,
                          std::vector<uchar> &status, std::vector<float> &err, Size win, int max_level, TermCriteria criteria, int flags,
                          double min_eig_threshold);

struct DMatch {
    int queryIdx, trainIdx, imgIdx;
    float distance;
    DMatch() : queryIdx(-1), trainIdx(-1), imgIdx(-1), distance(3.402823466e+38f) {}
    DMatch(int q, int t, float d) : queryIdx(q), trainIdx(t), imgIdx(-1), distance(d) {}
};
// BFMatcher(NORM_L2).radiusMatch on rows of two floats: every train row within maxDistance (<=) of a query row, nearest first,
// equal distances in index order; the distance is the f32 square root of the f32 sum of squares -- the definition the KLT
// search of tests/associate_ref.c uses (third-party arithmetic: a definition, not OpenCV's batch-distance kernel).
struct BFMatcher {
    explicit BFMatcher(int norm) { if (norm != NORM_L2) shim_unreachable("cv::BFMatcher of another norm"); }
    void radiusMatch(const Mat &query, const Mat &train, std::vector<std::vector<DMatch>> &matches, float maxDistance) const
    {
        matches.assign((size_t)query.rows, std::vector<DMatch>());
        for (int i = 0; i < query.rows; i++)
            for (int j = 0; j < train.rows; j++) {
                const float dx = query.at<float>(i, 0) - train.at<float>(j, 0), dy = query.at<float>(i, 1) - train.at<float>(j, 1);
                const float d = std::sqrt(dx * dx + dy * dy);
                if (!(d <= maxDistance)) continue;
                std::vector<DMatch> &nn = matches[(size_t)i];
                size_t p = nn.size();
                nn.push_back(DMatch());
                while (p > 0 && d < nn[p - 1].distance) nn[p] = nn[p - 1], p--;
                nn[p] = DMatch(i, j, d);
            }
    }
};

// cv::resize as the reference calls it (8UC1, default interpolation, dsize = half the parent): third-party arithmetic,
// supplied by the oracle's definition on both sides of the comparison.
inline void resize(const Mat &src, Mat &dst, Size dsize)
{
    if (dsize.width != (int)(src.cols * 0.5) || dsize.height != (int)(src.rows * 0.5)) shim_unreachable("cv::resize to another size than half");
    dst = Mat(dsize.height, dsize.width, CV_8UC1);
    if (dsize.width < 1 || dsize.height < 1) shim_unreachable("cv::resize to an empty image");
    if (pagk_oracle_pyr_down(src.data, src.cols, src.rows, (int64_t)src.step, dst.data) != 0) shim_unreachable("cv::resize of this shape");
}

// Features are independent of each other: the body runs once over the whole range.
inline void parallel_for_(const Range &range, std::function<void(const Range &)> body, double = -1.) { body(range); }

inline void undistortPoints(const Mat &, Mat &, const Mat &, const Mat &, const Mat &, const Mat &) { shim_unreachable("cv::undistortPoints"); }

}   // namespace cv

#endif
