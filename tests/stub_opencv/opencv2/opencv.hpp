// NOT OpenCV: a stand-in for the cv names the reference's node file uses, like oracle/ref_shim/opencv2/opencv.hpp, but with PIXELS and
// with OpenCV's 8-bit arithmetic, for tests/vio_ref_reader.cpp alone: cv::Mat is a view of a caller's packed 3-channel byte image,
// `double * Vec3b` is saturate_cast<uchar> of every channel (cvRound = lrint: to nearest, ties to even, clamped to 0 ... 255),
// `Vec3b + Vec3b` saturates, `Vec3f += Vec3b` and `Vec3f - Vec3f` are float operations.  Put in front of oracle/ref_shim
// on the include path, it lets cloudFrame::getRgb (src/lioOptimization.cpp:99-140) run on an image.  Test infrastructure.
#pragma once
#include <cmath>
#include <cstdlib>
namespace cv {
template <class T> inline T saturate_cast(double x) { return static_cast<T>(x); }
template <> inline unsigned char saturate_cast<unsigned char>(double x) { const long r = std::lrint(x); return (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r)); }
template <class T> inline T saturate_sum(int x) { return static_cast<T>(x); }
template <> inline unsigned char saturate_sum<unsigned char>(int x) { return (unsigned char)(x < 0 ? 0 : (x > 255 ? 255 : x)); }
template <class T, int N> struct Vec {
    T v[N];
    Vec() { for (int i = 0; i < N; ++i) v[i] = T(0); }
    Vec(T a, T b, T c) { static_assert(N == 3, "3-channel"); v[0] = a; v[1] = b; v[2] = c; }
    template <class U> Vec(const Vec<U, N> &o) { for (int i = 0; i < N; ++i) v[i] = static_cast<T>(o.v[i]); }
    T &operator[](int i) { return v[i]; }
    const T &operator[](int i) const { return v[i]; }
    T &operator()(int i) { return v[i]; }
    const T &operator()(int i) const { return v[i]; }
    template <class U> Vec &operator+=(const Vec<U, N> &o) { for (int i = 0; i < N; ++i) v[i] = static_cast<T>(v[i] + o.v[i]); return *this; }
};
typedef Vec<unsigned char, 3> Vec3b;
typedef Vec<float, 3> Vec3f;
inline Vec3b operator+(const Vec3b &a, const Vec3b &b) { Vec3b r; for (int i = 0; i < 3; ++i) r.v[i] = saturate_sum<unsigned char>((int)a.v[i] + (int)b.v[i]); return r; }
inline Vec3f operator+(const Vec3f &a, const Vec3f &b) { Vec3f r; for (int i = 0; i < 3; ++i) r.v[i] = a.v[i] + b.v[i]; return r; }
template <class T, int N> Vec<T, N> operator-(const Vec<T, N> &a, const Vec<T, N> &b) { Vec<T, N> r; for (int i = 0; i < N; ++i) r.v[i] = static_cast<T>(a.v[i] - b.v[i]); return r; }
template <class T, int N> Vec<T, N> operator*(double s, const Vec<T, N> &a) { Vec<T, N> r; for (int i = 0; i < N; ++i) r.v[i] = saturate_cast<T>(s * a.v[i]); return r; }
class Mat {
public:
    int rows = 0, cols = 0;
    unsigned char *data = nullptr;       // rows x cols x 3 bytes, rows packed; the caller's
    bool empty() const { return data == nullptr; }
    void release() { data = nullptr; rows = cols = 0; }
    Mat clone() const { return *this; }
    template <class T> T &at(int r, int c) { return reinterpret_cast<T *>(data + (size_t)r * cols * 3)[c]; }
    template <class T> T *ptr(int r) { return reinterpret_cast<T *>(data + (size_t)r * cols * 3); }
};
class RNG { public: RNG() {} explicit RNG(unsigned long long) {} };
struct Scalar { double v[4]; };
}  // namespace cv
