// Stand-in for the slice of OpenCV that the reference's src/ORBextractor.cc touches under its own include/ORBextractor.h.
//
// TEST INFRASTRUCTURE (oracle/README.md, "The reference's own text, compiled").  Project text, written from OpenCV's documented
// interfaces, for the program oracle/_ref/ref_orb alone: it comes first on that target's include path, so the stand-in of
// ref_shim/opencv2 (whose cv::Mat copies on rowRange / colRange) is never seen there.  It is not OpenCV: only the members that
// file uses exist, and the arithmetic OpenCV itself would contribute -- FAST, resize, copyMakeBorder, GaussianBlur, fastAtan2,
// cvRound -- is the project's definition (pagk_oracle_fast9 and its neighbours, oracle/pagk_oracle_cv.h).
//
// cv::Mat here is a VIEW: rowRange, colRange and operator()(Rect) share the parent's memory, create() keeps the memory when size
// and type already match, and assigning Mat::zeros(...) to a Mat of that size fills it in place -- ComputePyramid resizes into a
// view of `temp`, copyMakeBorder fills `temp` around it, and computeDescriptors zeroes and fills a rowRange of the output.  A
// buffer is zero-initialised and keeps two zero rows and 16 zero bytes of slack behind it, as the other stand-in's does.
#ifndef PAGK_REF_SHIM_ORB_CORE_HPP
#define PAGK_REF_SHIM_ORB_CORE_HPP

#include <algorithm>
#include <cassert>   // (OpenCV's core headers bring assert() with them; the reference relies on it)
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../../../pagk_oracle_cv.h"

typedef unsigned char uchar;

#define CV_8U 0
#define CV_8UC1 0
#define CV_PI 3.1415926535897932384626433832795

namespace cv {

[[noreturn]] inline void shim_unreachable(const char *what)
{
    std::fprintf(stderr, "ref_shim/orb: %s is not part of the stand-in\n", what);
    std::abort();
}

// cvRound: ties to even (the SSE conversion of OpenCV's x86-64 build); cvFloor and cvCeil alongside it
inline int cvRound(float v) { return (int)std::lrintf(v); }
inline int cvRound(double v) { return (int)std::lrint(v); }
inline int cvRound(int v) { return v; }
inline int cvFloor(float v) { return (int)std::floor(v); }
inline int cvFloor(double v) { return (int)std::floor(v); }
inline int cvCeil(float v) { return (int)std::ceil(v); }
inline int cvCeil(double v) { return (int)std::ceil(v); }

inline float fastAtan2(float y, float x) { return pagk_oracle_fast_atan2(y, x); }

// OpenCV's Point_<T>: a pair of T and nothing else ((const Point *)bit_pattern_31_ walks an int array), converted element by
// element; pt *= float multiplies in float (saturate_cast<float> of a float is the value)
template <typename T>
struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<float> Point2f;
typedef Point_<int> Point2i;
typedef Point2i Point;
template <typename T> inline Point_<T> &operator*=(Point_<T> &a, float b)
{
    a.x = T(a.x * b), a.y = T(a.y * b);
    return a;
}

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct Rect {
    int x, y, width, height;
    Rect() : x(0), y(0), width(0), height(0) {}
    Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

struct KeyPoint {
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
    KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
    KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0, int class_id_ = -1)
        : pt(x, y), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
};

struct MatZeros {   // what Mat::zeros returns: a recipe, applied in place by Mat::operator=
    int rows, cols, type;
};

class Mat {
public:
    int rows, cols;
    uchar *data;
    size_t step;   // bytes per row of the buffer this views

    Mat() : rows(0), cols(0), data(nullptr), step(0) {}
    Mat(int r, int c, int type) : Mat() { create(r, c, type); }
    Mat(Size s, int type) : Mat() { create(s.height, s.width, type); }

    void create(int r, int c, int type)
    {
        if (type != CV_8UC1) shim_unreachable("a matrix of another type than 8UC1");
        if (r < 0 || c < 0) shim_unreachable("a negative size");
        if (data && r == rows && c == cols) return;   // OpenCV keeps the memory (and the view) when size and type match
        rows = r, cols = c, step = (size_t)c;
        const size_t bytes = (size_t)(r + 2) * step + 16;   // zeroed, with two rows and 16 bytes of slack
        buf_.reset((uchar *)std::calloc(bytes, 1), std::free);
        if (!buf_) shim_unreachable("memory");
        data = buf_.get();
    }
    void create(Size s, int type) { create(s.height, s.width, type); }
    void release()
    {
        buf_.reset();
        rows = cols = 0, data = nullptr, step = 0;
    }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    int type() const { return CV_8UC1; }
    size_t step1() const { return step; }

    Mat rowRange(int a, int b) const { return view(0, a, cols, b - a); }
    Mat colRange(int a, int b) const { return view(a, 0, b - a, rows); }
    Mat operator()(const Rect &r) const { return view(r.x, r.y, r.width, r.height); }
    Mat clone() const
    {
        Mat m(rows, cols, CV_8UC1);
        for (int r = 0; r < rows; r++) std::memcpy(m.ptr(r), ptr(r), (size_t)cols);
        return m;
    }
    static MatZeros zeros(int r, int c, int type) { return MatZeros{r, c, type}; }
    Mat &operator=(const MatZeros &z)
    {
        create(z.rows, z.cols, z.type);
        for (int r = 0; r < rows; r++) std::memset(ptr(r), 0, (size_t)cols);
        return *this;
    }

    // at<>() and ptr() check nothing, as OpenCV's release build: a centre pointer plus offsets is how the reference reads
    template <typename T> T &at(int r, int c) { return *(T *)(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    template <typename T> const T &at(int r, int c) const { return *(const T *)(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    uchar *ptr(int r = 0) { return data + (size_t)r * step; }
    const uchar *ptr(int r = 0) const { return data + (size_t)r * step; }
    template <typename T> T *ptr(int r = 0) { return (T *)(data + (size_t)r * step); }
    template <typename T> const T *ptr(int r = 0) const { return (const T *)(data + (size_t)r * step); }

private:
    Mat view(int x, int y, int w, int h) const
    {
        if (x < 0 || y < 0 || w < 0 || h < 0 || x + w > cols || y + h > rows) shim_unreachable("a view outside its matrix");
        Mat m;
        m.buf_ = buf_, m.rows = h, m.cols = w, m.step = step, m.data = data + (size_t)y * step + (size_t)x;
        return m;
    }
    std::shared_ptr<uchar> buf_;
};

// InputArray / OutputArray: a pointer to the caller's Mat; getMat() is a header that shares its memory
class _InputArray {
public:
    _InputArray(const Mat &m) : m_(&m) {}
    bool empty() const { return m_->empty(); }
    Mat getMat() const { return *m_; }

protected:
    const Mat *m_;
};
class _OutputArray : public _InputArray {
public:
    _OutputArray(Mat &m) : _InputArray(m), out_(&m) {}
    void release() const { out_->release(); }
    void create(int rows, int cols, int type) const { out_->create(rows, cols, type); }
    void create(Size s, int type) const { out_->create(s, type); }
    Mat &getMatRef() const { return *out_; }

private:
    Mat *out_;
};
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;

enum { INTER_LINEAR = 1 };
enum { BORDER_REFLECT_101 = 4, BORDER_ISOLATED = 16 };

// Defined by the program (ref_orb.cpp): each logs or switches something a test looks at, and calls the oracle's definition.
void FAST(InputArray image, std::vector<KeyPoint> &keypoints, int threshold, bool nonmaxSuppression = true);
void resize(InputArray src, OutputArray dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR);
void copyMakeBorder(InputArray src, OutputArray dst, int top, int bottom, int left, int right, int borderType);
void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY = 0, int borderType = BORDER_REFLECT_101);

struct KeyPointsFilter {   // only ComputeKeyPointsOld reaches it, and nothing calls that
    static void retainBest(std::vector<KeyPoint> &, int) { shim_unreachable("KeyPointsFilter::retainBest"); }
};

}   // namespace cv

#endif
