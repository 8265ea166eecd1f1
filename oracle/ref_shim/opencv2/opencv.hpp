// Stand-in for the slice of OpenCV that the reference's src/patch_match.cpp and src/utils.cpp touch.
//
// TEST INFRASTRUCTURE (oracle/README.md, "The reference's own text, compiled").  Project text, written from OpenCV's
// documented interfaces: it exists so that the two reference sources compile UNCHANGED and their own statements -- the
// promotions, the loop order, the clamps, the branches -- can be run against the oracle.  It is not OpenCV: only the members
// those two files use exist, and the arithmetic OpenCV itself would contribute (cv::resize) is the oracle's definition.
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
#include <functional>
#include <memory>
#include <vector>

#include "../../pagk_oracle.h"

typedef unsigned char uchar;

#define CV_8U 0
#define CV_32F 5
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

    Mat reshape(int, int = 0) const { shim_unreachable("cv::Mat::reshape"); }

private:
    void create(int rows_, int cols_, int type, size_t step_bytes)
    {
        const int depth = type & 7, cn = (type >> 3) + 1;
        elem_ = (size_t)(depth == CV_32F ? 4 : 1) * (size_t)cn;
        rows = rows_, cols = cols_;
        step = step_bytes ? step_bytes : (size_t)cols_ * elem_;
        if (step < (size_t)cols_ * elem_) shim_unreachable("a row step below the row length");
        const size_t bytes = ((size_t)rows_ + 2) * step + 16;   // two zero rows and 16 zero bytes behind the image
        buf_ = std::shared_ptr<uchar>(static_cast<uchar *>(std::calloc(bytes, 1)), std::free);
        data = buf_.get();
    }
    std::shared_ptr<uchar> buf_;
    size_t elem_;
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
