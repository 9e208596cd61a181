// NOT OpenCV: a stand-in for exactly the cv names the reference's include/lkpyramid.h and src/lkpyramid.cpp use, so that
// tests/flow_reader.py can compile that file where it lies and drive its own LKOpticalFlowKernel::trackImage.  The LK arithmetic and the
// Scharr derivative are then the reference's own compiled statements; what this file RESTATES, from OpenCV's documentation, is library
// behaviour: cv::Mat with ROI, cv::pyrDown for 8-bit single channel (separable [1 4 6 4 1], integer sums, (s + 128) >> 8,
// BORDER_REFLECT_101, size ((w + 1) / 2, (h + 1) / 2)), cv::copyMakeBorder for REFLECT_101 and CONSTANT (always as with BORDER_ISOLATED:
// every call of the file either passes it or has a source that is no sub-matrix), cvRound (cvtss2si: to nearest, ties to even), cvFloor,
// and the handful of v_int16x8 operations as scalar loops on int16 (the values never leave int16, so wrapping and saturating products
// agree).  tests/flow_checker.py restates the same behaviour a second time, independently; no OpenCV exists on the machines of this
// project to confirm either, the two must agree bytewise.  parallel_for_ runs serially.  The SSE intrinsics of the file come from the
// host compiler's <emmintrin.h>.  Test infrastructure.
#pragma once
#include <emmintrin.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

typedef unsigned char uchar;
typedef unsigned short ushort;

#define CV_MAJOR_VERSION 4
#define CV_8U 0
#define CV_8S 1
#define CV_16U 2
#define CV_16S 3
#define CV_32S 4
#define CV_32F 5
#define CV_64F 6
#define CV_MAKETYPE(depth, cn) (((depth) & 7) + (((cn) - 1) << 3))
#define CV_SSE2 1
#define CV_CPU_SSE2 2
#define CV_CPU_NEON 100
#define CV_DECL_ALIGNED(x) __attribute__((aligned(x)))
#define CV_Assert(expr) do { if (!(expr)) { std::fprintf(stderr, "CV_Assert failed: %s (%s:%d)\n", #expr, __FILE__, __LINE__); std::abort(); } } while (0)

inline int cvRound(float v) { return _mm_cvtss_si32(_mm_set_ss(v)); }
inline int cvRound(double v) { return _mm_cvtsd_si32(_mm_set_sd(v)); }
inline int cvRound(int v) { return v; }
inline int cvFloor(float v) { const __m128 t = _mm_set_ss(v); const int i = _mm_cvtss_si32(t); return i - _mm_movemask_ps(_mm_cmplt_ss(t, _mm_cvtsi32_ss(t, i))); }
inline int cvFloor(double v) { const __m128d t = _mm_set_sd(v); const int i = _mm_cvtsd_si32(t); return i - _mm_movemask_pd(_mm_cmplt_sd(t, _mm_cvtsi32_sd(t, i))); }

namespace cv {

enum { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT_101 = 4, BORDER_TRANSPARENT = 5,
       BORDER_REFLECT101 = BORDER_REFLECT_101, BORDER_DEFAULT = BORDER_REFLECT_101, BORDER_ISOLATED = 16 };
enum { OPTFLOW_USE_INITIAL_FLOW = 4, OPTFLOW_LK_GET_MIN_EIGENVALS = 8 };

template <class T> struct DataType;
template <> struct DataType<uchar> { enum { depth = CV_8U }; };
template <> struct DataType<short> { enum { depth = CV_16S }; };
template <> struct DataType<float> { enum { depth = CV_32F }; };

inline bool checkHardwareSupport(int) { return true; }
inline size_t alignSize(size_t sz, int n) { return (sz + n - 1) & -(size_t)n; }
template <class T> inline T *alignPtr(T *p, int n = (int)sizeof(T)) { return (T *)(((size_t)p + n - 1) & -(size_t)n); }

template <class T> struct Size_ {
    T width, height;
    Size_() : width(0), height(0) {}
    Size_(T w, T h) : width(w), height(h) {}
    T area() const { return width * height; }
    bool operator==(const Size_ &o) const { return width == o.width && height == o.height; }
    bool operator!=(const Size_ &o) const { return !(*this == o); }
};
typedef Size_<int> Size;

template <class T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
    Point_ &operator+=(const Point_ &o) { x = (T)(x + o.x); y = (T)(y + o.y); return *this; }
    Point_ &operator-=(const Point_ &o) { x = (T)(x - o.x); y = (T)(y - o.y); return *this; }
    double ddot(const Point_ &o) const { return (double)x * o.x + (double)y * o.y; }
};
template <class T> inline Point_<T> operator+(const Point_<T> &a, const Point_<T> &b) { return Point_<T>((T)(a.x + b.x), (T)(a.y + b.y)); }
template <class T> inline Point_<T> operator-(const Point_<T> &a, const Point_<T> &b) { return Point_<T>((T)(a.x - b.x), (T)(a.y - b.y)); }
template <class T> inline Point_<T> operator*(const Point_<T> &a, int b) { return Point_<T>((T)(a.x * b), (T)(a.y * b)); }
template <class T> inline Point_<T> operator*(const Point_<T> &a, float b) { return Point_<T>((T)(a.x * b), (T)(a.y * b)); }
template <class T> inline Point_<T> operator*(const Point_<T> &a, double b) { return Point_<T>((T)(a.x * b), (T)(a.y * b)); }
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;

struct Rect { int x, y, width, height; Rect() : x(0), y(0), width(0), height(0) {} Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {} };
struct Range { int start, end; Range() : start(0), end(0) {} Range(int s, int e) : start(s), end(e) {} };

struct TermCriteria {
    enum { COUNT = 1, MAX_ITER = COUNT, EPS = 2 };
    int type, maxCount;
    double epsilon;
    TermCriteria() : type(0), maxCount(0), epsilon(0) {}
    TermCriteria(int t, int c, double e) : type(t), maxCount(c), epsilon(e) {}
};

template <class T> class AutoBuffer {
public:
    explicit AutoBuffer(size_t n) : v(n + 16) {}
    operator T *() { return v.data(); }
    operator const T *() const { return v.data(); }
private:
    std::vector<T> v;
};

template <class T> using Ptr = std::shared_ptr<T>;
template <class T, class... A> inline Ptr<T> makePtr(A &&...a) { return std::make_shared<T>(std::forward<A>(a)...); }

// a matrix header over a shared or a caller's buffer; a sub-matrix knows the buffer it was cut from (locateROI, adjustROI)
class Mat {
public:
    int rows = 0, cols = 0;
    size_t step = 0;
    uchar *data = nullptr;

    Mat() {}
    Mat(int r, int c, int t) { create(r, c, t); }
    Mat(int r, int c, int t, void *p) { init(r, c, t, (uchar *)p); }
    Mat(Size s, int t, void *p) { init(s.height, s.width, t, (uchar *)p); }

    void create(int r, int c, int t) {
        if (data && r == rows && c == cols && t == type_) return;
        const size_t es = esz(t);
        buf = std::make_shared<std::vector<uchar>>((size_t)r * c * es + 64, (uchar)0);
        init(r, c, t, buf->data());
    }
    void create(Size s, int t) { create(s.height, s.width, t); }
    void release() { *this = Mat(); }
    int type() const { return type_; }
    int depth() const { return type_ & 7; }
    int channels() const { return (type_ >> 3) + 1; }
    size_t elemSize1() const { static const size_t s[8] = {1, 1, 2, 2, 4, 4, 8, 2}; return s[type_ & 7]; }
    size_t elemSize() const { return esz(type_); }
    Size size() const { return Size(cols, rows); }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    bool isContinuous() const { return step == (size_t)cols * elemSize(); }
    bool isSubmatrix() const { return rows != wrows || cols != wcols; }
    uchar *ptr(int y = 0) { return data + (size_t)y * step; }
    const uchar *ptr(int y = 0) const { return data + (size_t)y * step; }
    template <class T> T *ptr(int y = 0) { return (T *)(data + (ptrdiff_t)y * (ptrdiff_t)step); }
    template <class T> const T *ptr(int y = 0) const { return (const T *)(data + (ptrdiff_t)y * (ptrdiff_t)step); }
    void locateROI(Size &whole, Point &ofs) const {
        const size_t d = (size_t)(data - start);
        ofs.y = step ? (int)(d / step) : 0;
        ofs.x = step ? (int)((d - (size_t)ofs.y * step) / elemSize()) : 0;
        whole = Size(wcols, wrows);
    }
    Mat &adjustROI(int dtop, int dbottom, int dleft, int dright) {
        Size whole; Point ofs;
        locateROI(whole, ofs);
        const int r1 = std::max(ofs.y - dtop, 0), r2 = std::min(ofs.y + rows + dbottom, whole.height);
        const int c1 = std::max(ofs.x - dleft, 0), c2 = std::min(ofs.x + cols + dright, whole.width);
        data = start + (size_t)r1 * step + (size_t)c1 * elemSize();
        rows = r2 - r1; cols = c2 - c1;
        return *this;
    }
    Mat operator()(const Rect &r) const {
        CV_Assert(r.x >= 0 && r.y >= 0 && r.x + r.width <= cols && r.y + r.height <= rows);
        Mat m(*this);
        m.data = data + (size_t)r.y * step + (size_t)r.x * elemSize();
        m.rows = r.height; m.cols = r.width;
        return m;
    }
    void copyTo(Mat dst) const {
        CV_Assert(dst.rows == rows && dst.cols == cols && dst.type_ == type_);
        for (int y = 0; y < rows; y++) std::memmove(dst.ptr(y), ptr(y), (size_t)cols * elemSize());
    }
    int checkVector(int elemChannels, int depth_ = -1, bool = true) const {
        if (depth_ >= 0 && depth() != depth_) return -1;
        if (channels() == elemChannels && (rows == 1 || cols == 1)) return rows * cols;
        if (channels() == 1 && cols == elemChannels) return rows;
        return -1;
    }

private:
    static size_t esz(int t) { static const size_t s[8] = {1, 1, 2, 2, 4, 4, 8, 2}; return s[t & 7] * (size_t)((t >> 3) + 1); }
    void init(int r, int c, int t, uchar *p) { rows = wrows = r; cols = wcols = c; type_ = t; step = (size_t)c * esz(t); data = start = p; }
    int type_ = 0, wrows = 0, wcols = 0;
    uchar *start = nullptr;
    std::shared_ptr<std::vector<uchar>> buf;
};

// InputArray and its relatives: one proxy over a Mat or a vector of Mats
class _Array {
public:
    _Array() {}
    _Array(const Mat &m) : mat(const_cast<Mat *>(&m)) {}
    _Array(const std::vector<Mat> &v) : vec(const_cast<std::vector<Mat> *>(&v)) {}
    Mat getMat(int i = -1) const { return vec ? (*vec)[i < 0 ? 0 : i] : (mat ? *mat : Mat()); }
    Mat &getMatRef(int i = -1) const { return vec ? (*vec)[i < 0 ? 0 : i] : *mat; }
    bool needed() const { return mat != nullptr || vec != nullptr; }
    void release() const { if (mat) mat->release(); if (vec) vec->clear(); }
    void create(int r, int c, int t, int = -1, bool = false, int = 0) const { if (vec) vec->resize((size_t)r * c); else if (mat) mat->create(r, c, t); }
    void create(Size s, int t, int = -1, bool = false, int = 0) const { create(s.height, s.width, t); }
private:
    Mat *mat = nullptr;
    std::vector<Mat> *vec = nullptr;
};
typedef const _Array &InputArray;
typedef const _Array &OutputArray;
typedef const _Array &InputOutputArray;
typedef const _Array &OutputArrayOfArrays;
inline const _Array &noArray() { static const _Array none; return none; }

class ParallelLoopBody {
public:
    virtual ~ParallelLoopBody() {}
    virtual void operator()(const Range &range) const = 0;
};
inline void parallel_for_(const Range &range, const ParallelLoopBody &body, double = -1.) { body(range); }
inline void parallel_for_(const Range &range, std::function<void(const Range &)> fn, double = -1.) { fn(range); }

// cv::borderInterpolate for BORDER_REFLECT_101
inline int borderInterpolate(int p, int len, int) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do { if (p < 0) p = -p; else p = len - 1 - (p - len) - 1; } while ((unsigned)p >= (unsigned)len);
    return p;
}

// REFLECT_101 or CONSTANT (zeros), as with BORDER_ISOLATED; src may be the interior of dst
inline void copyMakeBorder(const Mat &src, Mat &dst, int top, int bottom, int left, int right, int borderType) {
    const int kind = borderType & ~BORDER_ISOLATED;
    CV_Assert(kind == BORDER_REFLECT_101 || kind == BORDER_CONSTANT);
    if (dst.rows != src.rows + top + bottom || dst.cols != src.cols + left + right || dst.type() != src.type()) dst.create(src.rows + top + bottom, src.cols + left + right, src.type());
    const size_t es = src.elemSize();
    for (int y = 0; y < dst.rows; y++)
        for (int x = 0; x < dst.cols; x++) {
            uchar *d = dst.ptr(y) + (size_t)x * es;
            const int sy = y - top, sx = x - left;
            const bool inside = sy >= 0 && sy < src.rows && sx >= 0 && sx < src.cols;
            if (!inside && kind == BORDER_CONSTANT) { std::memset(d, 0, es); continue; }
            const uchar *s = src.ptr(borderInterpolate(sy, src.rows, kind)) + (size_t)borderInterpolate(sx, src.cols, kind) * es;
            if (s != d) std::memmove(d, s, es);
        }
}

// 8-bit single channel: a horizontal pass into rows of int, then the vertical one
inline void pyrDown(const Mat &src, Mat &dst, const Size &dsize = Size(), int borderType = BORDER_DEFAULT) {
    CV_Assert(src.type() == CV_8U && borderType == BORDER_REFLECT_101);
    const Size ds = dsize.width > 0 ? dsize : Size((src.cols + 1) / 2, (src.rows + 1) / 2);
    if (dst.rows != ds.height || dst.cols != ds.width || dst.type() != src.type()) dst.create(ds.height, ds.width, src.type());
    std::vector<int> hor((size_t)src.rows * ds.width);
    for (int y = 0; y < src.rows; y++) {
        const uchar *s = src.ptr(y);
        for (int x = 0; x < ds.width; x++) {
            const int m2 = borderInterpolate(2 * x - 2, src.cols, borderType), m1 = borderInterpolate(2 * x - 1, src.cols, borderType);
            const int p1 = borderInterpolate(2 * x + 1, src.cols, borderType), p2 = borderInterpolate(2 * x + 2, src.cols, borderType);
            hor[(size_t)y * ds.width + x] = s[borderInterpolate(2 * x, src.cols, borderType)] * 6 + (s[m1] + s[p1]) * 4 + s[m2] + s[p2];
        }
    }
    for (int y = 0; y < ds.height; y++) {
        const int *r[5];
        for (int k = 0; k < 5; k++) r[k] = &hor[(size_t)borderInterpolate(2 * y + k - 2, src.rows, borderType) * ds.width];
        uchar *d = dst.ptr(y);
        for (int x = 0; x < ds.width; x++) d[x] = (uchar)((r[2][x] * 6 + (r[1][x] + r[3][x]) * 4 + r[0][x] + r[4][x] + 128) >> 8);
    }
}

// universal intrinsics: eight int16 lanes as scalar loops
struct v_uint16x8 { ushort v[8]; };
struct v_int16x8 { short v[8]; };
inline v_int16x8 v_setall_s16(short a) { v_int16x8 r; for (int i = 0; i < 8; i++) r.v[i] = a; return r; }
inline v_uint16x8 v_load_expand(const uchar *p) { v_uint16x8 r; for (int i = 0; i < 8; i++) r.v[i] = p[i]; return r; }
inline v_int16x8 v_reinterpret_as_s16(const v_uint16x8 &a) { v_int16x8 r; for (int i = 0; i < 8; i++) r.v[i] = (short)a.v[i]; return r; }
inline v_int16x8 v_load(const short *p) { v_int16x8 r; std::memcpy(r.v, p, sizeof r.v); return r; }
inline void v_store(short *p, const v_int16x8 &a) { std::memcpy(p, a.v, sizeof a.v); }
inline void v_store_interleave(short *p, const v_int16x8 &a, const v_int16x8 &b) { for (int i = 0; i < 8; i++) { p[2 * i] = a.v[i]; p[2 * i + 1] = b.v[i]; } }
inline v_int16x8 operator+(const v_int16x8 &a, const v_int16x8 &b) { v_int16x8 r; for (int i = 0; i < 8; i++) r.v[i] = (short)(a.v[i] + b.v[i]); return r; }
inline v_int16x8 operator-(const v_int16x8 &a, const v_int16x8 &b) { v_int16x8 r; for (int i = 0; i < 8; i++) r.v[i] = (short)(a.v[i] - b.v[i]); return r; }
inline v_int16x8 operator*(const v_int16x8 &a, const v_int16x8 &b) { v_int16x8 r; for (int i = 0; i < 8; i++) r.v[i] = (short)(a.v[i] * b.v[i]); return r; }

}  // namespace cv
