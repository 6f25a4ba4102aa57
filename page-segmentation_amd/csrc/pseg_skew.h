// pseg_skew.h -- the integer contract of the skew estimate and of the rotation (include/pseg.h), once: the device
// kernels, the host twins (pseg_skew.hip) and the sanitizer check program (tools/skew_check.cpp) all walk these functions.
// Every division is a floor division and every shift an arithmetic one; nothing here is floating point except sk_cs, which only
// the host calls.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace pseg {

constexpr int SK_STRIP = 32;                          // columns of a strip
constexpr int SK_MAX_STEPS = 128;                     // candidates are -steps .. steps
constexpr int SK_MAX_SIDE = 16384;                    // rows / columns of a map
constexpr int SK_DENOM_MIN = 64, SK_DENOM_MAX = 4096;
constexpr int SK_MAX_STRIPS = SK_MAX_SIDE / SK_STRIP; // 512
constexpr int SK_ONE = 16384;                         // the scale of (C, S); source coordinates are in 1 / (2 SK_ONE) pixel

// floor(a / b) for b > 0
__host__ __device__ inline int sk_floordiv(int a, int b) {
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ inline int sk_strips(int W) { return (W + SK_STRIP - 1) / SK_STRIP; }
// the doubled nominal centre of strip k relative to the map's centre: |cx2| <= W + 32
__host__ __device__ inline int sk_cx2(int k, int W) { return 2 * SK_STRIP * k + SK_STRIP - W; }
// rows that candidate a moves strip k by: |a cx2 + D| <= 128 * 16416 + 4096 < 2^22
__host__ __device__ inline int sk_off(int a, int k, int W, int D) { return sk_floordiv(a * sk_cx2(k, W) + D, 2 * D); }
__host__ __device__ inline int sk_abs(int v) { return v < 0 ? -v : v; }
// the apron: off is monotone in a * cx2, so its extremes lie at a = +-A and the first or the last strip
__host__ __device__ inline int sk_apron(int A, int W, int D) {
    const int K = sk_strips(W);
    int m = sk_abs(sk_off(A, 0, W, D));
    const int c[3] = {sk_abs(sk_off(-A, 0, W, D)), sk_abs(sk_off(A, K - 1, W, D)), sk_abs(sk_off(-A, K - 1, W, D))};
    for (int i = 0; i < 3; ++i) m = c[i] > m ? c[i] : m;
    return m;
}
// the winner's order: the larger score; then the smaller |a|; then a > 0
__host__ __device__ inline bool sk_better(unsigned long long s, int a, unsigned long long bs, int ba) {
    if (s != bs) return s > bs;
    if (sk_abs(a) != sk_abs(ba)) return sk_abs(a) < sk_abs(ba);
    return a > ba;
}
__host__ __device__ inline bool sk_is_ink(unsigned b, bool from_gray) { return from_gray ? b <= 127u : b != 0u; }

// (C, S) of the rotation by index a over D, in units of 1 / SK_ONE: host only (the device reads a table)
inline void sk_cs(int a, int D, int* C, int* S) {
    const double r = std::sqrt((double)(D * D + a * a));
    *C = (int)std::floor(16384.0 * D / r + 0.5);
    const int s = (int)std::floor(16384.0 * (a < 0 ? -a : a) / r + 0.5);
    *S = a < 0 ? -s : s;
}
// source coordinates of output pixel (y, x) in 1 / 32768 pixel: |X|, |Y| < 2^30
__host__ __device__ inline void sk_src_xy(int y, int x, int H, int W, int C, int S, int* X, int* Y) {
    const int u = 2 * x - (W - 1), v = 2 * y - (H - 1);
    *X = C * u - S * v + (W - 1) * SK_ONE;
    *Y = S * u + C * v + (H - 1) * SK_ONE;
}
__host__ __device__ inline unsigned sk_tap(const uint8_t* src, int H, int W, int ys, int xs, unsigned fill) {
    return ((unsigned)ys < (unsigned)H && (unsigned)xs < (unsigned)W) ? src[(size_t)ys * W + xs] : fill;
}
template <int ORDER>
__host__ __device__ inline unsigned sk_sample(const uint8_t* src, int H, int W, int C, int S, unsigned fill, int y, int x) {
    int X, Y;
    sk_src_xy(y, x, H, W, C, S, &X, &Y);
    if (ORDER == 0) return sk_tap(src, H, W, (Y + SK_ONE) >> 15, (X + SK_ONE) >> 15, fill);
    const int x0 = X >> 15, y0 = Y >> 15;
    const long long fx = X & 32767, fy = Y & 32767, w = 32768;
    const long long p00 = sk_tap(src, H, W, y0, x0, fill), p01 = sk_tap(src, H, W, y0, x0 + 1, fill);
    const long long p10 = sk_tap(src, H, W, y0 + 1, x0, fill), p11 = sk_tap(src, H, W, y0 + 1, x0 + 1, fill);
    return (unsigned)(((w - fx) * (w - fy) * p00 + fx * (w - fy) * p01 + (w - fx) * fy * p10 + fx * fy * p11 + (1ll << 29)) >> 30);
}

}  // namespace pseg
