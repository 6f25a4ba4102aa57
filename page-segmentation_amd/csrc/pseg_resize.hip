// pseg_resize.hip -- line-height normalisation on the GPU: the pixel work of
// lib/dataset.py:114-150 (scale_binary, scale_image, prepare_images) and lib/util.py:21-29
// (preserving_resize).  The reference delegates to scikit-image 0.17.2 (resize / rescale ->
// scipy.ndimage.gaussian_filter -> warp); the kernels below restate that arithmetic in float64
// with the same operation order (no FMA contraction: -ffp-contract=off), so results equal
// oracle/resize.py bit for bit:
//   * anti-aliasing: separable Gaussian, 'mirror' boundary, scipy's symmetric accumulation order
//     (centre tap, then tap pairs from the outermost inwards); a uint8 image stays uint8 between
//     the passes (truncating cast), as scipy keeps the input dtype;
//   * warp: input coordinate = f*o + (f/2 - 0.5), f = in/out; order 0 rounds half away from zero,
//     order 3 is a 4x4 Catmull-Rom around floor(coord) (columns first, then rows), 'reflect'
//     index mapping, result clipped to the [min, max] of the (filtered) input.
// All kernels are HBM-bound streaming / gather kernels: one thread per output pixel, consecutive
// threads on consecutive x (coalesced rows); algorithmic bytes per pixel are in DESIGN.md.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pseg_list.h"

namespace pseg {

// periodic 'mirror' / skimage 'reflect' extension (no edge repeat): d c b | a b c d | c b a
__device__ __forceinline__ int mirror_idx(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

template <typename T>
__device__ __forceinline__ double ld(const T* p, size_t i) { return (double)p[i]; }

// one pass of scipy.ndimage.correlate1d with a symmetric kernel, mode 'mirror'
template <typename T, int AXIS>
__global__ __launch_bounds__(256) void gauss_pass_kernel(const T* src, int H, int W, const double* w, int radius, T* dst) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int i = AXIS == 0 ? y : x, n = AXIS == 0 ? H : W;
    const size_t row = (size_t)y * W;
    double acc = ld(src, row + x) * w[radius];
    for (int j = radius; j >= 1; --j) {
        const int lo = mirror_idx(i - j, n), hi = mirror_idx(i + j, n);
        const double a = AXIS == 0 ? ld(src, (size_t)lo * W + x) : ld(src, row + lo);
        const double b = AXIS == 0 ? ld(src, (size_t)hi * W + x) : ld(src, row + hi);
        acc = acc + (a + b) * w[radius - j];
    }
    dst[row + x] = (T)acc;   // uint8: C truncation, as scipy's line buffer copy
}

// order-preserving map double -> uint64 (for atomic min / max)
__device__ __forceinline__ unsigned long long ord_enc(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
static inline double ord_dec(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// 16-byte vector loads for the two streaming reductions below: VEC elements per thread and trip
template <typename T> struct Vec16;
template <> struct Vec16<uint8_t> { static constexpr int N = 16; };
template <> struct Vec16<double> { static constexpr int N = 2; };

// calls f(value as double) for every element of src[0..n): 16-byte loads over the aligned body, scalar tail
template <typename T, typename F>
__device__ __forceinline__ void for_each_vec(const T* src, size_t n, F f) {
    constexpr int N = Vec16<T>::N;
    const size_t nv = n / N;
    const uint4* sv = (const uint4*)src;     // hipMalloc'ed planes: 256-byte aligned
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const uint4 v = sv[i];
        T e[N];
        memcpy(e, &v, 16);
#pragma unroll
        for (int k = 0; k < N; ++k) f((double)e[k]);
    }
    if (blockIdx.x == 0 && threadIdx.x < n - nv * N) f((double)src[nv * N + threadIdx.x]);
}

// stats[0] = min (encoded), stats[1] = max (encoded); one atomic pair per workgroup
template <typename T>
__global__ __launch_bounds__(256) void minmax_kernel(const T* src, size_t n, unsigned long long* stats) {
    __shared__ unsigned long long smn[4], smx[4];
    double lo = 1.0e308, hi = -1.0e308;
    for_each_vec<T>(src, n, [&](double v) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; });
    unsigned long long mn = ord_enc(lo), mx = ord_enc(hi);
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const unsigned long long a = __shfl_xor(mn, sh), b = __shfl_xor(mx, sh);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { mn = smn[w] < mn ? smn[w] : mn; mx = smx[w] > mx ? smx[w] : mx; }
        atomicMin(&stats[0], mn);
        atomicMax(&stats[1], mx);
    }
}

// stats[2] != 0  <=>  some value differs from both min and max  <=>  len(np.unique(img)) > 2
template <typename T>
__global__ __launch_bounds__(256) void third_value_kernel(const T* src, size_t n, unsigned long long* stats) {
    const unsigned long long emn = stats[0], emx = stats[1];
    const unsigned long long umn = (emn >> 63) ? (emn & 0x7fffffffffffffffull) : ~emn;
    const unsigned long long umx = (emx >> 63) ? (emx & 0x7fffffffffffffffull) : ~emx;
    const double lo = __longlong_as_double((long long)umn), hi = __longlong_as_double((long long)umx);
    bool any = false;
    for_each_vec<T>(src, n, [&](double v) { any |= (v != lo) & (v != hi); });
    if (__any(any) && (threadIdx.x & 63) == 0) atomicOr(&stats[2], 1ull);
}

__device__ __forceinline__ double cubic(double x, double f0, double f1, double f2, double f3) {
    return f1 + 0.5 * x * (f2 - f0 + x * (2.0 * f0 - 5.0 * f1 + 4.0 * f2 - f3 + x * (3.0 * (f1 - f2) + f3 - f0)));
}

// order-3 warp, output float64 clipped to [lo, hi] (encoded in stats[0..1])
template <typename T>
__global__ __launch_bounds__(256) void bicubic_kernel(const T* src, int H, int W, double* dst, int Ho, int Wo,
                                                      double fy, double ty, double fx, double tx,
                                                      const unsigned long long* stats) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= Wo) return;
    const double yr = fy * (double)oy + ty, xc = fx * (double)ox + tx;
    const double r0f = floor(yr), c0f = floor(xc);
    const double tr = yr - r0f, tc = xc - c0f;
    const int r0 = (int)r0f - 1, c0 = (int)c0f - 1;
    int cols[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cols[k] = mirror_idx(c0 + k, W);
    double fr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t row = (size_t)mirror_idx(r0 + k, H) * W;
        fr[k] = cubic(tc, ld(src, row + cols[0]), ld(src, row + cols[1]), ld(src, row + cols[2]), ld(src, row + cols[3]));
    }
    double v = cubic(tr, fr[0], fr[1], fr[2], fr[3]);
    unsigned long long u0 = stats[0], u1 = stats[1];
    u0 = (u0 >> 63) ? (u0 & 0x7fffffffffffffffull) : ~u0;
    u1 = (u1 >> 63) ? (u1 & 0x7fffffffffffffffull) : ~u1;
    const double lo = __longlong_as_double((long long)u0), hi = __longlong_as_double((long long)u1);
    v = v < lo ? lo : (v > hi ? hi : v);     // np.clip
    dst[(size_t)oy * Wo + ox] = v;
}

// order-0 warp = gather of whole pixels (EB bytes each)
template <int EB>
__global__ __launch_bounds__(256) void nearest_kernel(const uint8_t* src, int H, int W, uint8_t* dst, int Ho, int Wo,
                                                      double fy, double ty, double fx, double tx) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= Wo) return;
    const double yr = fy * (double)oy + ty, xc = fx * (double)ox + tx;
    const int r = mirror_idx((int)(yr > 0.0 ? yr + 0.5 : yr - 0.5), H);
    const int c = mirror_idx((int)(xc > 0.0 ? xc + 0.5 : xc - 0.5), W);
    const uint8_t* s = src + ((size_t)r * W + c) * EB;
    uint8_t* d = dst + ((size_t)oy * Wo + ox) * EB;
    if (EB == 1) *d = *s;
    else if (EB == 2) *(uint16_t*)d = *(const uint16_t*)s;
    else if (EB == 4) *(uint32_t*)d = *(const uint32_t*)s;
    else if (EB == 8) *(uint64_t*)d = *(const uint64_t*)s;
    else
        for (int b = 0; b < EB; ++b) d[b] = s[b];
}

// elementwise steps of prepare_images (lib/dataset.py:135-146)
//   MODE 0: uint8 binary -> ink map:  out = uint8(1.0 - (gt1 ? b / 255 : b))
//   MODE 1: float64 v    -> float64:  out = 1.0 - v / 255
//   MODE 2: float64 v    -> uint8:    out = uint8((1.0 - v / 255) * 255)
//   MODE 3: float64 v    -> uint8:    out = uint8(v * 255)
template <int MODE>
__global__ __launch_bounds__(256) void prep_map_kernel(const void* src, void* dst, size_t n, const unsigned long long* stats) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (MODE == 0) {
        unsigned long long u1 = stats[1];
        u1 = (u1 >> 63) ? (u1 & 0x7fffffffffffffffull) : ~u1;
        const bool gt1 = __longlong_as_double((long long)u1) > 1.0;
        const double b = (double)((const uint8_t*)src)[i];
        ((uint8_t*)dst)[i] = (uint8_t)(1.0 - (gt1 ? b / 255.0 : b));
    } else if (MODE == 1) {
        ((double*)dst)[i] = 1.0 - ((const double*)src)[i] / 255.0;
    } else if (MODE == 2) {
        ((uint8_t*)dst)[i] = (uint8_t)((1.0 - ((const double*)src)[i] / 255.0) * 255.0);
    } else {
        ((uint8_t*)dst)[i] = (uint8_t)(((const double*)src)[i] * 255.0);
    }
}

// ---- affine warp of the augmentation pipeline (lib/data_generator.py -> keras-preprocessing
// apply_affine_transform -> scipy.ndimage.affine_transform, mode 'nearest') -------------------------------
// order 3: scipy edge-pads the plane by 12 pixels, runs the cubic B-spline prefilter (pole sqrt(3) - 2, gain 6,
// mirror initialisation) along both axes in float64 and evaluates the four-tap B-spline at
// M (r, c) + offset with coordinates clamped to the padded plane; order 0: floor(coord + 0.5), clamped.
constexpr int WARP_PAD = 12;

__global__ __launch_bounds__(256) void warp_pad_kernel(const float* src, int H, int W, double* dst, int pad) {
    const int Wp = W + 2 * pad, Hp = H + 2 * pad;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= Wp || y >= Hp) return;
    const int sy = min(max(y - pad, 0), H - 1), sx = min(max(x - pad, 0), W - 1);
    dst[(size_t)y * Wp + x] = (double)src[(size_t)sy * W + sx];
}

// ---- the line recurrence of the cubic prefilter, shared by the thread-per-line kernel below and the tiled kernel of the device
// sample builder (spline3_prefilter_tile_kernel).  A line is reached through an accessor `a(i)` (sample i of the line: strided
// global memory there, an LDS tile here); every function keeps one sequence of float64 operations, so both users give the same bits.
// reflect = 0: mirror boundary (whole-sample symmetric: scipy's 'mirror', and what it uses for 'constant' and 'wrap');
// reflect = 1: half-sample symmetric ('reflect': c[-1 - i] = c[i]) -- scipy >= 1.6 ni_splines.c _init_causal_reflect / _anticausal_reflect
constexpr double SPLINE3_Z = -0.2679491924311227;          // sqrt(3) - 2
constexpr int SPLINE3_HORIZON = 28;                        // |z|^k < 1e-15 after 27 terms

struct LineGlobal {
    double* p;
    size_t st;
    __device__ __forceinline__ double& operator()(int i) const { return p[i * st]; }
};

template <class A>
__device__ __forceinline__ void spline3_gain(const A& a, int i0, int i1) {
    for (int i = i0; i < i1; ++i) a(i) *= 6.0;      // gain (1 - z)(1 - 1/z)
}

// c+[0] of a line of n > 1 gained samples: reads a(0 .. 27) of a long line, the whole line (closed form) when n <= 28
template <class A>
__device__ __forceinline__ double spline3_causal_init(const A& a, int n, int reflect) {
    const double z = SPLINE3_Z;
    const int hor = min(n, SPLINE3_HORIZON);
    if (reflect) {
        // c+[0] = c[0] + z sum_{i >= 0} z^i c[i] over the half-sample-symmetric extension; exact closed form for short lines
        const double c0 = a(0);
        double sum;
        if (hor < n) {
            double zi = 1.0;
            sum = 0.0;
            for (int i = 0; i < hor; ++i) { sum += zi * a(i); zi *= z; }
            sum *= z;
        } else {
            double zn = 1.0;
            for (int i = 0; i < n; ++i) zn *= z;              // z^n
            double zi = z;
            sum = a(0) + zn * a(n - 1);
            for (int i = 1; i < n; ++i) { sum += zi * (a(i) + zn * a(n - 1 - i)); zi *= z; }
            sum *= z / (1.0 - zn * zn);
        }
        return sum + c0;
    }
    // mirror boundary: c+[0] = sum_k z^k c[k]
    double zi = z, sum = a(0);
    if (hor < n) {
        for (int i = 1; i < hor; ++i) { sum += zi * a(i); zi *= z; }
    } else {
        const double iz = 1.0 / z;
        double z2 = 1.0;
        for (int i = 0; i < n - 1; ++i) z2 *= z;          // z^(n-1)
        double z2n = z2;
        sum = a(0) + z2 * a(n - 1);
        z2 = z2 * z2 * iz;
        zi = z;
        for (int i = 1; i < n - 1; ++i) { sum += (zi + z2) * a(i); zi *= z; z2 *= iz; }
        sum /= (1.0 - z2n * z2n);
    }
    return sum;
}

// a(i) += z a(i - 1) for i in [i0, i1); prev = a(i0 - 1); returns a(i1 - 1)
template <class A>
__device__ __forceinline__ double spline3_causal_sweep(const A& a, int i0, int i1, double prev) {
    const double z = SPLINE3_Z;
    for (int i = i0; i < i1; ++i) { prev = a(i) + z * prev; a(i) = prev; }
    return prev;
}

// c-[n - 1] from the causal results c+[n - 2], c+[n - 1]
__device__ __forceinline__ double spline3_anticausal_init(double before_last, double last, int reflect) {
    const double z = SPLINE3_Z;
    return reflect ? last * (z / (z - 1.0)) : (z / (z * z - 1.0)) * (z * before_last + last);
}

// a(i) = z (a(i + 1) - a(i)) for i = i1 down to i0; next = a(i1 + 1); returns a(i0)
template <class A>
__device__ __forceinline__ double spline3_anticausal_sweep(const A& a, int i1, int i0, double next) {
    const double z = SPLINE3_Z;
    for (int i = i1; i >= i0; --i) { next = z * (next - a(i)); a(i) = next; }
    return next;
}

// one thread = one line (row: AXIS 1, column: AXIS 0) of the padded plane, in place
template <int AXIS>
__global__ __launch_bounds__(64) void spline3_prefilter_kernel(double* c, int Hp, int Wp, int reflect = 0) {
    const int line = blockIdx.x * 64 + threadIdx.x;
    const int nlines = AXIS == 1 ? Hp : Wp, n = AXIS == 1 ? Wp : Hp;
    if (line >= nlines) return;
    const LineGlobal a{AXIS == 1 ? c + (size_t)line * Wp : c + line, AXIS == 1 ? (size_t)1 : (size_t)Wp};
    if (n == 1) return;                             // (scipy leaves a line of one sample as it is)
    spline3_gain(a, 0, n);
    a(0) = spline3_causal_init(a, n, reflect);
    spline3_causal_sweep(a, 1, n, a(0));
    a(n - 1) = spline3_anticausal_init(a(n - 2), a(n - 1), reflect);
    spline3_anticausal_sweep(a, n - 2, 0, a(n - 1));
}

// fill_mode 'constant' / 'reflect' / 'wrap' (scipy.ndimage >= 1.6 geometric transforms, ni_interpolation.c map_coordinate): the plane
// is NOT padded; the prefilter runs on it with the boundary of the mode ('reflect': half-sample symmetric; 'constant' and 'wrap':
// mirror -- scipy has no exact spline boundary for those two); the coordinate is mapped by the mode ('constant': outside [0, n - 1]
// on either axis gives `cval`; 'reflect': d c b a | a b c d | d c b a; 'wrap': period n - 1, scipy's legacy 'wrap'), may stay a
// fraction outside the plane, and the tap INDICES are mapped by the prefilter's boundary.
__device__ __forceinline__ int warp_mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i = (i < 0 ? -i : i) % p;
    return i < n ? i : p - i;
}
__device__ __forceinline__ int warp_reflect_idx(int i, int n) {       // ... -2 -> 1, -1 -> 0, n -> n - 1, n + 1 -> n - 2 ...
    if (n == 1) return 0;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}
enum { WARP_CONST = 1, WARP_REFLECT = 2, WARP_WRAP = 3 };
template <int MODE>
__device__ __forceinline__ double warp_map_coord(double x, int n) {   // scipy map_coordinate, same operations in the same order
    if (MODE == WARP_REFLECT) {
        if (x < 0.0) {
            if (n <= 1) return 0.0;
            const double sz2 = 2.0 * n;
            if (x < -sz2) x = sz2 * (double)(long long)(-x / sz2) + x;
            x = x < -(double)n ? x + sz2 : -x - 1.0;
        } else if (x > (double)(n - 1)) {
            if (n <= 1) return 0.0;
            const double sz2 = 2.0 * n;
            x -= sz2 * (double)(long long)(x / sz2);
            if (x >= (double)n) x = sz2 - x - 1.0;
        }
    } else if (MODE == WARP_WRAP) {
        if (x < 0.0) {
            if (n <= 1) return 0.0;
            const double sz = n - 1;
            x += sz * ((double)(long long)(-x / sz) + 1.0);
        } else if (x > (double)(n - 1)) {
            if (n <= 1) return 0.0;
            const double sz = n - 1;
            x -= sz * (double)(long long)(x / sz);
        }
    }
    return x;
}
// ---- the sampling arithmetic of the warp, shared by the one-plane kernels below and the fused kernel of the device sample
// builder (aug_warp_kernel): coordinate mapping, tap index mapping, the B-spline weights and their row-then-column accumulation.
// MODE 0 is 'nearest' (scipy's mode of keras-preprocessing's default): cubic taps on the plane edge-padded by WARP_PAD.
__device__ __forceinline__ void warp_src_coord(double m00, double m01, double m10, double m11, double o0, double o1, int r, int c,
                                               double* y, double* x) {
    *y = m00 * (double)r + m01 * (double)c + o0;
    *x = m10 * (double)r + m11 * (double)c + o1;
}
// maps (y, x) by the mode; false: the pixel takes `cval` ('constant', source coordinate outside the plane)
template <int MODE>
__device__ __forceinline__ bool warp_map_point(double* y, double* x, int H, int W) {
    if (MODE == WARP_CONST) {
        if (*y < 0.0 || *y > (double)(H - 1) || *x < 0.0 || *x > (double)(W - 1)) return false;
    } else if (MODE != 0) {
        *y = warp_map_coord<MODE>(*y, H);
        *x = warp_map_coord<MODE>(*x, W);
    }
    return true;
}
template <int MODE>
__device__ __forceinline__ int warp_tap(int i, int n) {
    if (MODE == 0) return min(max(i, 0), n - 1);
    return MODE == WARP_REFLECT ? warp_reflect_idx(i, n) : warp_mirror(i, n);
}
// order 0: index of the source pixel of the mapped point
template <int MODE>
__device__ __forceinline__ size_t warp_nearest_index(double y, double x, int H, int W) {
    return (size_t)warp_tap<MODE>((int)floor(y + 0.5), H) * W + warp_tap<MODE>((int)floor(x + 0.5), W);
}
__device__ __forceinline__ void bspline3_weights(double t, double* w) {
    const double u = 1.0 - t;
    w[0] = u * u * u / 6.0;
    w[1] = (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0;
    w[2] = (4.0 - 6.0 * u * u + 3.0 * u * u * u) / 6.0;
    w[3] = t * t * t / 6.0;
}
// order 3: the four-by-four B-spline sum around the mapped point on the (Hc, Wc) coefficient plane (MODE 0: the padded plane,
// the point moved by the pad and clamped to it)
template <int MODE>
__device__ __forceinline__ double warp_cubic_sample(const double* coef, int Hc, int Wc, double y, double x) {
    if (MODE == 0) {
        y = fmin(fmax(y + WARP_PAD, 0.0), (double)(Hc - 1));
        x = fmin(fmax(x + WARP_PAD, 0.0), (double)(Wc - 1));
    }
    const int y0 = (int)floor(y), x0 = (int)floor(x);
    const double ty = y - y0, tx = x - x0;
    double wy[4], wx[4];
    bspline3_weights(ty, wy);
    bspline3_weights(tx, wx);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = warp_tap<MODE>(y0 - 1 + i, Hc);
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) row += wx[j] * coef[(size_t)yy * Wc + warp_tap<MODE>(x0 - 1 + j, Wc)];
        acc += wy[i] * row;
    }
    return acc;
}

template <int ORDER, int MODE>
__global__ __launch_bounds__(256) void affine_warp_mode_kernel(const double* coef, const float* src, int H, int W, float* dst,
                                                               double m00, double m01, double m10, double m11, double o0, double o1, float cval) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c >= W) return;
    double y, x;
    warp_src_coord(m00, m01, m10, m11, o0, o1, r, c, &y, &x);
    if (!warp_map_point<MODE>(&y, &x, H, W)) { dst[(size_t)r * W + c] = cval; return; }
    if (ORDER == 0) {
        dst[(size_t)r * W + c] = src[warp_nearest_index<MODE>(y, x, H, W)];
        return;
    }
    dst[(size_t)r * W + c] = (float)warp_cubic_sample<MODE>(coef, H, W, y, x);
}

template <int ORDER>
__global__ __launch_bounds__(256) void affine_warp_kernel(const double* coef, const float* src, int H, int W, float* dst,
                                                          double m00, double m01, double m10, double m11, double o0, double o1) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c >= W) return;
    double y, x;
    warp_src_coord(m00, m01, m10, m11, o0, o1, r, c, &y, &x);
    if (ORDER == 0) {
        dst[(size_t)r * W + c] = src[warp_nearest_index<0>(y, x, H, W)];
        return;
    }
    dst[(size_t)r * W + c] = (float)warp_cubic_sample<0>(coef, H + 2 * WARP_PAD, W + 2 * WARP_PAD, y, x);
}

static void warp_coeffs(int n_in, int n_out, double* f, double* t) {
    *f = (double)n_in / (double)n_out;
    *t = *f * 0.5 - 0.5;
}

static std::vector<double> host_gauss(double sigma, int* radius) {
    const int r = (int)(4.0 * sigma + 0.5);
    std::vector<double> w(2 * r + 1);
    double s = 0.0;
    for (int i = -r; i <= r; ++i) s += (w[i + r] = std::exp(-0.5 / (sigma * sigma) * (double)(i * i)));
    for (auto& v : w) v /= s;
    *radius = r;
    return w;   // symmetric: the [::-1] of scipy is the identity
}

struct DevMem {
    std::vector<void*> ptrs;
    ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T>
    int alloc(T** p, size_t count) {
        *p = nullptr;
        PSEG_HIP(hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)));
        ptrs.push_back(*p);
        return PSEG_OK;
    }
};

static int stats_reset(unsigned long long* d_stats, hipStream_t st) {
    const unsigned long long init[3] = {~0ull, 0ull, 0ull};
    PSEG_HIP(hipMemcpyAsync(d_stats, init, sizeof(init), hipMemcpyHostToDevice, st));
    return PSEG_OK;
}

template <typename T>
static int compute_stats(const T* d, size_t n, unsigned long long* d_stats, bool third, hipStream_t st) {
    PSEG_TRY(stats_reset(d_stats, st));
    const int grid = (int)std::min<size_t>((n / Vec16<T>::N + 255) / 256 + 1, 1024);
    minmax_kernel<T><<<grid, 256, 0, st>>>(d, n, d_stats);
    if (third) third_value_kernel<T><<<grid, 256, 0, st>>>(d, n, d_stats);
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

// scale_image on device planes.  d_src: T plane (H, W); d_out: float64 (Ho, Wo).  wy / wx: host
// kernels (NULL: built here with libm exp); scratch planes are allocated from `mem`.
template <typename T>
static int scale_image_dev(DevMem& mem, const T* d_src, int H, int W, double* d_out, int Ho, int Wo,
                           const double* wy, int ry, const double* wx, int rx, unsigned long long* d_stats,
                           hipStream_t st) {
    const size_t n = (size_t)H * W;
    PSEG_TRY(compute_stats<T>(d_src, n, d_stats, true, st));
    unsigned long long hs[3];
    PSEG_HIP(hipMemcpyAsync(hs, d_stats, sizeof(hs), hipMemcpyDeviceToHost, st));
    PSEG_HIP(hipStreamSynchronize(st));
    const bool aa = hs[2] != 0;
    const T* cur = d_src;
    if (aa) {
        const double sig[2] = {std::max(0.0, ((double)H / (double)Ho - 1.0) / 2.0),
                               std::max(0.0, ((double)W / (double)Wo - 1.0) / 2.0)};
        const double* hw[2] = {wy, wx};
        int hr[2] = {ry, rx};
        for (int axis = 0; axis < 2; ++axis) {
            if (sig[axis] <= 1e-15) continue;
            std::vector<double> own;
            if (!hw[axis]) { own = host_gauss(sig[axis], &hr[axis]); hw[axis] = own.data(); }
            if (hr[axis] != (int)(4.0 * sig[axis] + 0.5))
                return fail(PSEG_EINVAL, "anti-aliasing kernel radius %d does not match sigma %.17g", hr[axis], sig[axis]);
            double* d_w = nullptr;
            T* d_tmp = nullptr;
            PSEG_TRY(mem.alloc(&d_w, (size_t)2 * hr[axis] + 1));
            PSEG_TRY(mem.alloc(&d_tmp, n));
            PSEG_HIP(hipMemcpyAsync(d_w, hw[axis], ((size_t)2 * hr[axis] + 1) * 8, hipMemcpyHostToDevice, st));
            PSEG_HIP(hipStreamSynchronize(st));   // `own` may go out of scope
            const dim3 grid(cdiv(W, 256), H);
            if (axis == 0) gauss_pass_kernel<T, 0><<<grid, 256, 0, st>>>(cur, H, W, d_w, hr[axis], d_tmp);
            else gauss_pass_kernel<T, 1><<<grid, 256, 0, st>>>(cur, H, W, d_w, hr[axis], d_tmp);
            PSEG_HIP(hipGetLastError());
            cur = d_tmp;
        }
        if (cur != d_src) PSEG_TRY(compute_stats<T>(cur, n, d_stats, false, st));   // clip range of the filtered image
    }
    double fy, ty, fx, tx;
    warp_coeffs(H, Ho, &fy, &ty);
    warp_coeffs(W, Wo, &fx, &tx);
    bicubic_kernel<T><<<dim3(cdiv(Wo, 256), Ho), 256, 0, st>>>(cur, H, W, d_out, Ho, Wo, fy, ty, fx, tx, d_stats);
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

static int nearest_dev(const void* d_src, int H, int W, int eb, void* d_dst, int Ho, int Wo, hipStream_t st) {
    double fy, ty, fx, tx;
    warp_coeffs(H, Ho, &fy, &ty);
    warp_coeffs(W, Wo, &fx, &tx);
    const dim3 grid(cdiv(Wo, 256), Ho);
    const uint8_t* s = (const uint8_t*)d_src;
    uint8_t* d = (uint8_t*)d_dst;
    switch (eb) {
        case 1: nearest_kernel<1><<<grid, 256, 0, st>>>(s, H, W, d, Ho, Wo, fy, ty, fx, tx); break;
        case 2: nearest_kernel<2><<<grid, 256, 0, st>>>(s, H, W, d, Ho, Wo, fy, ty, fx, tx); break;
        case 4: nearest_kernel<4><<<grid, 256, 0, st>>>(s, H, W, d, Ho, Wo, fy, ty, fx, tx); break;
        case 8: nearest_kernel<8><<<grid, 256, 0, st>>>(s, H, W, d, Ho, Wo, fy, ty, fx, tx); break;
        case 3: nearest_kernel<3><<<grid, 256, 0, st>>>(s, H, W, d, Ho, Wo, fy, ty, fx, tx); break;
        default: return fail(PSEG_EUNSUPPORTED, "element size %d (supported: 1, 2, 3, 4, 8 bytes)", eb);
    }
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

static int check_shape(int H, int W, int Ho, int Wo) {
    if (H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return fail(PSEG_EINVAL, "empty image or target shape (%d,%d)->(%d,%d)", H, W, Ho, Wo);
    if ((int64_t)H * W > 0x7fffffffLL || (int64_t)Ho * Wo > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "image too large");
    return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_rescale_shape(int H, int W, double scale, int* Ho, int* Wo) {
    if (!Ho || !Wo) return fail(PSEG_EINVAL, "NULL argument");
    // np.round: half to even (nearbyint in the default rounding mode)
    *Ho = (int)std::nearbyint(scale * (double)H);
    *Wo = (int)std::nearbyint(scale * (double)W);
    return PSEG_OK;
}

int pseg_gaussian_kernel(double sigma, double* w, int cap, int* radius) {
    if (!radius || !(sigma > 0.0)) return fail(PSEG_EINVAL, "bad argument");
    int r = 0;
    const std::vector<double> k = host_gauss(sigma, &r);
    *radius = r;
    if (w) {
        if (cap < 2 * r + 1) return fail(PSEG_EINVAL, "kernel needs %d entries, capacity %d", 2 * r + 1, cap);
        memcpy(w, k.data(), k.size() * 8);
    }
    return PSEG_OK;
}

int pseg_resize_nearest(int device, const void* src, int H, int W, int elem_bytes, void* dst, int Ho, int Wo) {
    if (!src || !dst) return fail(PSEG_EINVAL, "NULL argument");
    PSEG_TRY(check_shape(H, W, Ho, Wo));
    PSEG_TRY(open_device(device));
    DevMem mem;
    uint8_t *d_s = nullptr, *d_d = nullptr;
    const size_t ns = (size_t)H * W * elem_bytes, nd = (size_t)Ho * Wo * elem_bytes;
    PSEG_TRY(mem.alloc(&d_s, ns));
    PSEG_TRY(mem.alloc(&d_d, nd));
    PSEG_HIP(hipMemcpy(d_s, src, ns, hipMemcpyHostToDevice));
    PSEG_TRY(nearest_dev(d_s, H, W, elem_bytes, d_d, Ho, Wo, nullptr));
    PSEG_HIP(hipMemcpy(dst, d_d, nd, hipMemcpyDeviceToHost));
    return PSEG_OK;
}

int pseg_resize_nearest_device(int device, const void* d_src, int H, int W, int elem_bytes, void* d_dst, int Ho, int Wo, void* stream) {
    if (!d_src || !d_dst) return fail(PSEG_EINVAL, "NULL argument");
    PSEG_TRY(check_shape(H, W, Ho, Wo));
    PSEG_TRY(open_device(device));
    return nearest_dev(d_src, H, W, elem_bytes, d_dst, Ho, Wo, (hipStream_t)stream);
}

int pseg_scale_image(int device, const void* src, int src_is_f64, int H, int W, double* dst, int Ho, int Wo,
                     const double* wy, int ry, const double* wx, int rx) {
    if (!src || !dst) return fail(PSEG_EINVAL, "NULL argument");
    PSEG_TRY(check_shape(H, W, Ho, Wo));
    PSEG_TRY(open_device(device));
    DevMem mem;
    const size_t n = (size_t)H * W, no = (size_t)Ho * Wo;
    unsigned long long* d_stats = nullptr;
    double* d_out = nullptr;
    PSEG_TRY(mem.alloc(&d_stats, 4));
    PSEG_TRY(mem.alloc(&d_out, no));
    if (src_is_f64) {
        double* d_s = nullptr;
        PSEG_TRY(mem.alloc(&d_s, n));
        PSEG_HIP(hipMemcpy(d_s, src, n * 8, hipMemcpyHostToDevice));
        PSEG_TRY(scale_image_dev<double>(mem, d_s, H, W, d_out, Ho, Wo, wy, ry, wx, rx, d_stats, nullptr));
    } else {
        uint8_t* d_s = nullptr;
        PSEG_TRY(mem.alloc(&d_s, n));
        PSEG_HIP(hipMemcpy(d_s, src, n, hipMemcpyHostToDevice));
        PSEG_TRY(scale_image_dev<uint8_t>(mem, d_s, H, W, d_out, Ho, Wo, wy, ry, wx, rx, d_stats, nullptr));
    }
    PSEG_HIP(hipMemcpy(dst, d_out, no * 8, hipMemcpyDeviceToHost));
    return PSEG_OK;
}

int pseg_affine_warp(int device, const float* src, int H, int W, const double m[4], const double off[2], int order,
                     float* dst) {
    return pseg_affine_warp_fill(device, src, H, W, m, off, order, 0, 0.0f, dst);
}

int pseg_affine_warp_fill(int device, const float* src, int H, int W, const double m[4], const double off[2], int order,
                          int fill_mode, float cval, float* dst) {
    if (!src || !dst || !m || !off) return fail(PSEG_EINVAL, "NULL argument");
    if (order != 0 && order != 3) return fail(PSEG_EUNSUPPORTED, "interpolation order %d (0 and 3 are built)", order);
    if (fill_mode < 0 || fill_mode > 3) return fail(PSEG_EUNSUPPORTED, "fill mode %d (0 'nearest', 1 'constant', 2 'reflect', 3 'wrap')", fill_mode);
    PSEG_TRY(check_shape(H, W, H, W));
    PSEG_TRY(open_device(device));
    DevMem mem;
    const size_t n = (size_t)H * W;
    float *d_s = nullptr, *d_d = nullptr;
    PSEG_TRY(mem.alloc(&d_s, n));
    PSEG_TRY(mem.alloc(&d_d, n));
    PSEG_HIP(hipMemcpy(d_s, src, n * 4, hipMemcpyHostToDevice));
    const dim3 grid(cdiv(W, 256), H);
    double* d_c = nullptr;
    if (order == 3) {
        const int pad = fill_mode == 0 ? WARP_PAD : 0;       // (every mode but 'nearest': scipy filters the plane itself)
        const int Hp = H + 2 * pad, Wp = W + 2 * pad;
        PSEG_TRY(mem.alloc(&d_c, (size_t)Hp * Wp));
        warp_pad_kernel<<<dim3(cdiv(Wp, 256), Hp), 256>>>(d_s, H, W, d_c, pad);
        spline3_prefilter_kernel<0><<<cdiv(Wp, 64), 64>>>(d_c, Hp, Wp, fill_mode == 2);     // axis 0 first, as scipy's spline_filter
        spline3_prefilter_kernel<1><<<cdiv(Hp, 64), 64>>>(d_c, Hp, Wp, fill_mode == 2);
    }
#define PSEG_WARP(ORD_)                                                                                                                  \
    switch (fill_mode) {                                                                                                                 \
        case 0: affine_warp_kernel<ORD_><<<grid, 256>>>(d_c, d_s, H, W, d_d, m[0], m[1], m[2], m[3], off[0], off[1]); break;             \
        case 1: affine_warp_mode_kernel<ORD_, WARP_CONST><<<grid, 256>>>(d_c, d_s, H, W, d_d, m[0], m[1], m[2], m[3], off[0], off[1], cval); break;   \
        case 2: affine_warp_mode_kernel<ORD_, WARP_REFLECT><<<grid, 256>>>(d_c, d_s, H, W, d_d, m[0], m[1], m[2], m[3], off[0], off[1], cval); break; \
        default: affine_warp_mode_kernel<ORD_, WARP_WRAP><<<grid, 256>>>(d_c, d_s, H, W, d_d, m[0], m[1], m[2], m[3], off[0], off[1], cval); break;   \
    }
    if (order == 0) { PSEG_WARP(0) } else { PSEG_WARP(3) }
#undef PSEG_WARP
    PSEG_HIP(hipGetLastError());
    PSEG_HIP(hipMemcpy(dst, d_d, n * 4, hipMemcpyDeviceToHost));
    return PSEG_OK;
}

// keras-preprocessing 1.1.2 apply_brightness_shift(x, brightness, scale=False) on one image plane (lib/trainer.py:21,33: the
// brightness_range of AugmentationSettings reaches the IMAGE generator only):
//   lo, hi = min(x), max(x); local = lo < 0 or hi > 255
//   u = uint8(local ? (x - lo) / (hi - lo) * 255 : x)                     array_to_img (float32 arithmetic, C cast = truncation)
//   v = PIL ImageEnhance.Brightness: blend(black, u, b) = b in [0, 1] ? uint8(b * u) : clip(b * u, 0, 255) truncated   (float32)
//   y = local ? v / 255 * (hi - lo) + lo : v                               img_to_array, float32
__global__ __launch_bounds__(256) void brightness_minmax_kernel(const float* x, size_t n, unsigned* mm) {
    float lo = INFINITY, hi = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const float v = x[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0) {
        // order-preserving map float -> unsigned so that atomicMin / atomicMax work on the bits
        auto key = [](float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
        atomicMin(&mm[0], key(lo));
        atomicMax(&mm[1], key(hi));
    }
}
__global__ __launch_bounds__(256) void brightness_apply_kernel(const float* x, float* y, size_t n, const unsigned* mm, float b) {
    auto unkey = [](unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); };
    const float lo = unkey(mm[0]), hi = unkey(mm[1]);
    const bool local = lo < 0.0f || hi > 255.0f;
    const float span = hi - lo;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v = x[i];
        if (local) { v = v - lo; if (span != 0.0f) v = v / span; v = v * 255.0f; }
        const float u = (float)(unsigned char)(int)v;          // astype('uint8'): truncation (values are in range here)
        const float t = b * u;
        float w;
        if (b >= 0.0f && b <= 1.0f) w = (float)(unsigned char)(int)t;
        else w = t <= 0.0f ? 0.0f : (t >= 255.0f ? 255.0f : (float)(unsigned char)(int)t);
        y[i] = local ? w / 255.0f * span + lo : w;
    }
}

int pseg_brightness_shift(int device, const float* src, int64_t n, float brightness, float* dst) {
    if (!src || !dst || n < 1) return fail(PSEG_EINVAL, "NULL argument / empty plane");
    PSEG_TRY(open_device(device));
    DevMem mem;
    float *d_s = nullptr, *d_d = nullptr;
    unsigned* d_mm = nullptr;
    PSEG_TRY(mem.alloc(&d_s, (size_t)n));
    PSEG_TRY(mem.alloc(&d_d, (size_t)n));
    PSEG_TRY(mem.alloc(&d_mm, 2));
    const unsigned init[2] = {0xffffffffu, 0u};
    PSEG_HIP(hipMemcpy(d_mm, init, 8, hipMemcpyHostToDevice));
    PSEG_HIP(hipMemcpy(d_s, src, (size_t)n * 4, hipMemcpyHostToDevice));
    const int grid = (int)std::min<size_t>(((size_t)n + 255) / 256, 2048);
    brightness_minmax_kernel<<<grid, 256>>>(d_s, (size_t)n, d_mm);
    brightness_apply_kernel<<<grid, 256>>>(d_s, d_d, (size_t)n, d_mm, brightness);
    PSEG_HIP(hipGetLastError());
    PSEG_HIP(hipMemcpy(dst, d_d, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PSEG_OK;
}

int pseg_prepare_images(int device, const uint8_t* image, const uint8_t* binary, int H0, int W0, int H1, int W1,
                        const double* wy1, int ry1, const double* wx1, int rx1, int H2, int W2,
                        const double* wy2, int ry2, const double* wx2, int rx2, uint8_t* out_img,
                        uint8_t* out_bin, uint8_t* out_orig_bin, double* out_stage1) {
    if (!image || !binary || !out_img || !out_bin) return fail(PSEG_EINVAL, "NULL argument");
    PSEG_TRY(check_shape(H0, W0, H1, W1));
    const bool two = H2 > 0 && W2 > 0;
    if (two) PSEG_TRY(check_shape(H1, W1, H2, W2));
    PSEG_TRY(open_device(device));
    DevMem mem;
    hipStream_t st = nullptr;
    const size_t n0 = (size_t)H0 * W0, n1 = (size_t)H1 * W1, n2 = two ? (size_t)H2 * W2 : 0;
    uint8_t *d_img = nullptr, *d_bin = nullptr, *d_ink0 = nullptr, *d_ink1 = nullptr, *d_o8 = nullptr;
    double* d_s1 = nullptr;
    unsigned long long* d_stats = nullptr;
    PSEG_TRY(mem.alloc(&d_img, n0));
    PSEG_TRY(mem.alloc(&d_bin, n0));
    PSEG_TRY(mem.alloc(&d_ink0, n0));
    PSEG_TRY(mem.alloc(&d_ink1, n1));
    PSEG_TRY(mem.alloc(&d_s1, n1));
    PSEG_TRY(mem.alloc(&d_o8, two ? n2 : n1));
    PSEG_TRY(mem.alloc(&d_stats, 4));
    PSEG_HIP(hipMemcpyAsync(d_img, image, n0, hipMemcpyHostToDevice, st));
    PSEG_HIP(hipMemcpyAsync(d_bin, binary, n0, hipMemcpyHostToDevice, st));
    // binary: orig_bin = b/255 if max > 1 else b; ink = uint8(1 - orig_bin); bin = 1 - nearest(orig_bin)
    // (the gather commutes with the per-pixel map, so the ink map is gathered)
    PSEG_TRY(compute_stats<uint8_t>(d_bin, n0, d_stats, false, st));
    prep_map_kernel<0><<<(unsigned)((n0 + 255) / 256), 256, 0, st>>>(d_bin, d_ink0, n0, d_stats);
    PSEG_HIP(hipGetLastError());
    PSEG_TRY(nearest_dev(d_ink0, H0, W0, 1, d_ink1, H1, W1, st));
    // image: stage 1 on the uint8 scan
    PSEG_TRY(scale_image_dev<uint8_t>(mem, d_img, H0, W0, d_s1, H1, W1, wy1, ry1, wx1, rx1, d_stats, st));
    if (out_stage1) PSEG_HIP(hipMemcpyAsync(out_stage1, d_s1, n1 * 8, hipMemcpyDeviceToHost, st));
    if (!two) {
        prep_map_kernel<2><<<(unsigned)((n1 + 255) / 256), 256, 0, st>>>(d_s1, d_o8, n1, d_stats);
        PSEG_HIP(hipGetLastError());
        PSEG_HIP(hipMemcpyAsync(out_img, d_o8, n1, hipMemcpyDeviceToHost, st));
        PSEG_HIP(hipMemcpyAsync(out_bin, d_ink1, n1, hipMemcpyDeviceToHost, st));
    } else {
        double *d_f1 = nullptr, *d_s2 = nullptr;
        uint8_t* d_ink2 = nullptr;
        PSEG_TRY(mem.alloc(&d_f1, n1));
        PSEG_TRY(mem.alloc(&d_s2, n2));
        PSEG_TRY(mem.alloc(&d_ink2, n2));
        prep_map_kernel<1><<<(unsigned)((n1 + 255) / 256), 256, 0, st>>>(d_s1, d_f1, n1, d_stats);
        PSEG_HIP(hipGetLastError());
        PSEG_TRY(scale_image_dev<double>(mem, d_f1, H1, W1, d_s2, H2, W2, wy2, ry2, wx2, rx2, d_stats, st));
        prep_map_kernel<3><<<(unsigned)((n2 + 255) / 256), 256, 0, st>>>(d_s2, d_o8, n2, d_stats);
        PSEG_HIP(hipGetLastError());
        PSEG_TRY(nearest_dev(d_ink1, H1, W1, 1, d_ink2, H2, W2, st));
        PSEG_HIP(hipMemcpyAsync(out_img, d_o8, n2, hipMemcpyDeviceToHost, st));
        PSEG_HIP(hipMemcpyAsync(out_bin, d_ink2, n2, hipMemcpyDeviceToHost, st));
    }
    if (out_orig_bin) PSEG_HIP(hipMemcpyAsync(out_orig_bin, d_ink0, n0, hipMemcpyDeviceToHost, st));
    PSEG_HIP(hipStreamSynchronize(st));
    return PSEG_OK;
}

}  // extern "C"

// ---- device-resident augmented training sample (pseg_train_forward_backward_aug / pseg_train_augment_sample) ------------------
// lib/network.py:149-161 for one sample without a trip through host arrays: uint8 page -> float64 coefficient plane -> tiled
// prefilter -> ONE fused warp launch per channel that also warps the mask (order 0) and writes both at their flipped
// positions -> brightness in place.  The float64 arithmetic is that of the one-plane entries above (the shared inline functions),
// so the sample has their bits; what differs is staging (uint8 in, no host planes), fusion and how the prefilter is spread.
namespace pseg {

// uint8 (H,W,C) channel ch -> float64 (H + 2 pad, W + 2 pad), edge-padded (uint8 -> float32 -> float64 is exact, so is this)
__global__ __launch_bounds__(256) void aug_pad_u8_kernel(const uint8_t* src, int H, int W, int C, int ch, double* dst, int pad) {
    const int Wp = W + 2 * pad, Hp = H + 2 * pad;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= Wp || y >= Hp) return;
    const int sy = min(max(y - pad, 0), H - 1), sx = min(max(x - pad, 0), W - 1);
    dst[(size_t)y * Wp + x] = (double)src[((size_t)sy * W + sx) * C + ch];
}

// The prefilter of one axis, 64 lines per workgroup.  The thread-per-line kernel walks global memory sample by sample: a
// dependent load and store per step, and along rows (AXIS 1) adjacent lanes Wp * 8 bytes apart.  Here the workgroup moves
// 64 x 64 sample tiles between the plane and LDS with 512-byte row segments (all 256 threads, the next tile's loads in flight
// while the current one is filtered), and lane l of wave 0 advances line l through the tile: forward over the chunks (gain,
// causal initialisation from the first chunk, causal sweep, anticausal initialisation at the line's end), then backward.
// Tile pitch 65 doubles: a row pass reads tile[l][i] -- lane stride 130 dwords = 2 mod 64, a ds_read_b64 half-wave covers the 64
// banks once; a column pass reads tile[i][l], consecutive.
constexpr int PF_TILE = 64, PF_PITCH = 65;

struct LineTile {
    double* t;      // sample i0 of the lane's line
    int st, i0;
    __device__ __forceinline__ double& operator()(int i) const { return t[(i - i0) * st]; }
};

template <int AXIS>
__global__ __launch_bounds__(256) void spline3_prefilter_tile_kernel(double* c, int Hp, int Wp, int reflect) {
    __shared__ double tile[PF_TILE * PF_PITCH];
    const int nlines = AXIS == 1 ? Hp : Wp, n = AXIS == 1 ? Wp : Hp;
    if (n == 1) return;                             // (scipy leaves a line of one sample as it is)
    const int line0 = blockIdx.x * PF_TILE;
    const int tid = threadIdx.x, tc = tid & 63, tr0 = tid >> 6;
    const int nchunks = (n + PF_TILE - 1) / PF_TILE;
    double reg[16];
    // tile (r, tc) <-> plane (R0 + r, C0 + tc); a thread always moves the same 16 elements of a tile
    auto load = [&](int k) {
        const int R0 = AXIS == 1 ? line0 : k * PF_TILE, C0 = AXIS == 1 ? k * PF_TILE : line0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int r = R0 + tr0 + 4 * j;
            reg[j] = (r < Hp && C0 + tc < Wp) ? c[(size_t)r * Wp + C0 + tc] : 0.0;
        }
    };
    auto store = [&](int k) {
        const int R0 = AXIS == 1 ? line0 : k * PF_TILE, C0 = AXIS == 1 ? k * PF_TILE : line0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int r = R0 + tr0 + 4 * j;
            if (r < Hp && C0 + tc < Wp) c[(size_t)r * Wp + C0 + tc] = tile[(tr0 + 4 * j) * PF_PITCH + tc];
        }
    };
    const bool active = tid < PF_TILE && line0 + tid < nlines;
    double* const lane = tile + (AXIS == 1 ? tid * PF_PITCH : tid);   // (only dereferenced by active lanes: tid < 64)
    const int lst = AXIS == 1 ? 1 : PF_PITCH;
    double carry = 0.0;
    load(0);
    for (int k = 0; k < nchunks; ++k) {
#pragma unroll
        for (int j = 0; j < 16; ++j) tile[(tr0 + 4 * j) * PF_PITCH + tc] = reg[j] * 6.0;     // spline3_gain on the way in
        __syncthreads();
        if (k + 1 < nchunks) load(k + 1);
        if (active) {
            const int i0 = k * PF_TILE, i1 = min(n, i0 + PF_TILE);
            const LineTile a{lane, lst, i0};
            double before = carry;                  // c+[i0 - 1]
            if (k == 0) {
                carry = spline3_causal_init(a, n, reflect);
                a(0) = carry;
                carry = spline3_causal_sweep(a, 1, i1, carry);
            } else {
                carry = spline3_causal_sweep(a, i0, i1, carry);
            }
            if (k == nchunks - 1) {
                if (n - 2 >= i0) before = a(n - 2);
                carry = spline3_anticausal_init(before, carry, reflect);
                a(n - 1) = carry;
            }
        }
        __syncthreads();
        store(k);
        __syncthreads();
    }
    // backward: the last chunk is still in the tile; a thread reloads only what it stored itself
    if (nchunks > 1) load(nchunks - 2);
    for (int k = nchunks - 1; k >= 0; --k) {
        if (k < nchunks - 1) {
#pragma unroll
            for (int j = 0; j < 16; ++j) tile[(tr0 + 4 * j) * PF_PITCH + tc] = reg[j];
            __syncthreads();
            if (k > 0) load(k - 1);
        }
        if (active) {
            const int i0 = k * PF_TILE;
            const LineTile a{lane, lst, i0};
            const int i1 = k == nchunks - 1 ? n - 2 : i0 + PF_TILE - 1;     // carry = c-[i1 + 1]
            carry = spline3_anticausal_sweep(a, i1, i0, carry);
        }
        __syncthreads();
        store(k);
        __syncthreads();
    }
}

__device__ __forceinline__ unsigned brightness_key(float f) {     // the keys of brightness_minmax_kernel
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// every lane of the wave calls this (lanes without a pixel pass +inf / -inf)
__device__ __forceinline__ void aug_minmax(float lo, float hi, unsigned* mm) {
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[0], brightness_key(lo));
        atomicMax(&mm[1], brightness_key(hi));
    }
}

template <int MODE>
__device__ __forceinline__ uint8_t aug_mask_sample(const uint8_t* mask, int H, int W, double y, double x, uint8_t fill) {
    if (!warp_map_point<MODE>(&y, &x, H, W)) return fill;
    return mask[warp_nearest_index<MODE>(y, x, H, W)];
}

// One thread per output pixel of channel ch: cubic sample of the channel's coefficient plane, order-0 sample of the mask
// (with channel 0), both written at the flipped position; min / max of the float sample for the brightness stretch (mm != NULL).
template <int IMODE>
__global__ __launch_bounds__(256) void aug_warp_kernel(const double* coef, const uint8_t* mask, int H, int W, int C, int ch,
                                                       float* out_img, uint8_t* out_mask, double m00, double m01, double m10, double m11,
                                                       double o0, double o1, unsigned flips, float image_cval, int mask_mode,
                                                       uint8_t mask_fill, unsigned* mm) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    if (c < W) {
        double y, x;
        warp_src_coord(m00, m01, m10, m11, o0, o1, r, c, &y, &x);
        const size_t o = (size_t)((flips & 2u) ? H - 1 - r : r) * W + ((flips & 1u) ? W - 1 - c : c);
        if (ch == 0) {
            uint8_t mv;
            switch (mask_mode) {
                case 0: mv = aug_mask_sample<0>(mask, H, W, y, x, mask_fill); break;
                case WARP_CONST: mv = aug_mask_sample<WARP_CONST>(mask, H, W, y, x, mask_fill); break;
                case WARP_REFLECT: mv = aug_mask_sample<WARP_REFLECT>(mask, H, W, y, x, mask_fill); break;
                default: mv = aug_mask_sample<WARP_WRAP>(mask, H, W, y, x, mask_fill); break;
            }
            out_mask[o] = mv;
        }
        float v = image_cval;
        if (warp_map_point<IMODE>(&y, &x, H, W))
            v = (float)warp_cubic_sample<IMODE>(coef, IMODE == 0 ? H + 2 * WARP_PAD : H, IMODE == 0 ? W + 2 * WARP_PAD : W, y, x);
        out_img[o * C + ch] = v;
        lo = hi = v;
    }
    if (mm) aug_minmax(lo, hi, mm);
}

// no warp (the generator skips it for the identity): the exact uint8 values, flipped
__global__ __launch_bounds__(256) void aug_flip_kernel(const uint8_t* img, const uint8_t* mask, int H, int W, int C, float* out_img,
                                                       uint8_t* out_mask, unsigned flips, unsigned* mm) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    if (c < W) {
        const size_t i = (size_t)r * W + c;
        const size_t o = (size_t)((flips & 2u) ? H - 1 - r : r) * W + ((flips & 1u) ? W - 1 - c : c);
        out_mask[o] = mask[i];
        for (int ch = 0; ch < C; ++ch) {
            const float v = (float)img[i * C + ch];
            out_img[o * C + ch] = v;
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    if (mm) aug_minmax(lo, hi, mm);
}

size_t augment_coef_count(int H, int W, int image_fill) {
    const int pad = image_fill == 0 ? WARP_PAD : 0;
    return (size_t)(H + 2 * pad) * (W + 2 * pad);
}

int augment_sample_device(const AugSample& a, hipStream_t st) {
    const int H = a.H, W = a.W, C = a.C;
    const dim3 grid(cdiv(W, 256), H);
    unsigned* mm = a.use_brightness ? a.d_mm : nullptr;
    if (mm) {
        static const unsigned init[2] = {0xffffffffu, 0u};
        PSEG_HIP(hipMemcpyAsync(mm, init, 8, hipMemcpyHostToDevice, st));
    }
    if (!a.m) {
        aug_flip_kernel<<<grid, 256, 0, st>>>(a.d_src_img, a.d_src_mask, H, W, C, a.d_img, a.d_mask, a.flips, mm);
    } else {
        const int pad = a.image_fill == 0 ? WARP_PAD : 0;       // (every mode but 'nearest': scipy filters the plane itself)
        const int Hp = H + 2 * pad, Wp = W + 2 * pad;
        const uint8_t mfill = (uint8_t)(int)a.mask_cval;
        const double* m = a.m;
        const double* off = a.off;
        for (int ch = 0; ch < C; ++ch) {
            aug_pad_u8_kernel<<<dim3(cdiv(Wp, 256), Hp), 256, 0, st>>>(a.d_src_img, H, W, C, ch, a.d_coef, pad);
            spline3_prefilter_tile_kernel<0><<<cdiv(Wp, PF_TILE), 256, 0, st>>>(a.d_coef, Hp, Wp, a.image_fill == 2);   // axis 0 first, as scipy's spline_filter
            spline3_prefilter_tile_kernel<1><<<cdiv(Hp, PF_TILE), 256, 0, st>>>(a.d_coef, Hp, Wp, a.image_fill == 2);
#define PSEG_AUG_WARP(MODE_)                                                                                                              \
    aug_warp_kernel<MODE_><<<grid, 256, 0, st>>>(a.d_coef, a.d_src_mask, H, W, C, ch, a.d_img, a.d_mask, m[0], m[1], m[2], m[3], off[0], \
                                                 off[1], a.flips, a.image_cval, a.mask_fill, mfill, mm)
            switch (a.image_fill) {
                case 0: PSEG_AUG_WARP(0); break;
                case 1: PSEG_AUG_WARP(WARP_CONST); break;
                case 2: PSEG_AUG_WARP(WARP_REFLECT); break;
                default: PSEG_AUG_WARP(WARP_WRAP); break;
            }
#undef PSEG_AUG_WARP
        }
    }
    if (a.use_brightness) {
        const size_t n = (size_t)H * W * C;
        const int bgrid = (int)std::min<size_t>((n + 255) / 256, 2048);
        brightness_apply_kernel<<<bgrid, 256, 0, st>>>(a.d_img, a.d_img, n, a.d_mm, a.brightness);
    }
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

int augment_check(int H, int W, const double* m, const double* off, unsigned flips, int image_fill, int mask_fill, float mask_cval) {
    PSEG_TRY(check_shape(H, W, H, W));
    if ((m == nullptr) != (off == nullptr)) return fail(PSEG_EINVAL, "matrix and offset come together (both NULL: no warp)");
    if (flips & ~3u) return fail(PSEG_EINVAL, "flips 0x%x (bit 0 horizontal, bit 1 vertical)", flips);
    if (image_fill < 0 || image_fill > 3 || mask_fill < 0 || mask_fill > 3)
        return fail(PSEG_EUNSUPPORTED, "fill modes %d / %d (0 'nearest', 1 'constant', 2 'reflect', 3 'wrap')", image_fill, mask_fill);
    if (!(mask_cval >= 0.0f && mask_cval <= 255.0f) || mask_cval != (float)(int)mask_cval)
        return fail(PSEG_EINVAL, "mask_cval %g is not an integer in 0..255 (the mask is built as uint8)", (double)mask_cval);
    return PSEG_OK;
}

}  // namespace pseg

// ---- device-resident front end of the scan chain (pseg_predict_chain_scans_png / pseg_prepare_scans) ---------------------------
// pseg_prepare_images(scan, where(scan > 127, 255, 0)) without the max_width stage, for the case it is called for: a uint8 scan whose
// binarisation is a function of the scan (ink = scan <= 127, also where no pixel is above 127: the 0 / 255 map has max 0 there, is not
// divided, and 1 - 0 is ink everywhere).  The float64 operations per pixel are those of gauss_pass_kernel, bicubic_kernel and
// prep_map_kernel<2> in their order (the shared inline functions, -ffp-contract=off), so the bytes are theirs.  What differs: min, max
// and "more than two distinct values" of a uint8 plane are read off a 256-bit presence bitmap that the kernels OR into the scan's
// record (no ordered-double atomics, no read on the host: the anti-aliasing decision stays on the device); both Gaussian passes run
// through LDS in one launch; clip, inversion, conversion and the ink map's gather ride in the sampler.  At most three launches a scan.
namespace pseg {

constexpr int SF_TH = 32, SF_TW = 64, SF_RMAX = 8;            // output tile of the fused Gaussian and its radius cap
constexpr int SF_PITCH = SF_TW + 2 * SF_RMAX;                 // bytes per LDS tile row

// ORs value v into the workgroup's LDS bitmap; `prev` (the last value this thread has set) skips the runs of a page
__device__ __forceinline__ void bm_or(unsigned* s_bm, unsigned v, unsigned& prev) {
    if (v == prev) return;
    prev = v;
    const unsigned bit = 1u << (v & 31);
    if (!(s_bm[v >> 5] & bit)) atomicOr(&s_bm[v >> 5], bit);
}
__device__ __forceinline__ void bm_or_word(unsigned* s_bm, unsigned word, unsigned& prev) {
#pragma unroll
    for (int k = 0; k < 4; ++k) bm_or(s_bm, (word >> (8 * k)) & 255u, prev);
}
// the workgroup's bitmap into the record: eight 32-bit atomics (every thread calls this)
__device__ __forceinline__ void bm_flush(const unsigned* s_bm, unsigned* rec) {
    __syncthreads();
    if (threadIdx.x < 8 && s_bm[threadIdx.x]) atomicOr(&rec[threadIdx.x], s_bm[threadIdx.x]);
}
__device__ __forceinline__ int bm_count(const unsigned* rec) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) n += __popc(rec[k]);
    return n;
}
__device__ __forceinline__ void bm_range(const unsigned* rec, double* lo, double* hi) {
    int mn = 0, mx = 0;
    for (int k = 7; k >= 0; --k)
        if (rec[k]) mn = 32 * k + __ffs(rec[k]) - 1;
    for (int k = 0; k < 8; ++k)
        if (rec[k]) mx = 32 * k + 31 - __clz(rec[k]);
    *lo = (double)mn;
    *hi = (double)mx;
}

// One pass over the scan, 16-byte loads: the presence bitmap -> rec[0..8), and (orig != NULL) the scan-sized ink map scan <= 127
__global__ __launch_bounds__(256) void scan_stats_kernel(const uint8_t* scan, size_t n, unsigned* rec, uint8_t* orig) {
    __shared__ unsigned s_bm[8];
    if (threadIdx.x < 8) s_bm[threadIdx.x] = 0;
    __syncthreads();
    unsigned prev = 256;
    const size_t nv = n / 16;
    const uint4* sv = (const uint4*)scan;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const uint4 v = sv[i];
        bm_or_word(s_bm, v.x, prev);
        bm_or_word(s_bm, v.y, prev);
        bm_or_word(s_bm, v.z, prev);
        bm_or_word(s_bm, v.w, prev);
        // a byte is <= 127 where its top bit is clear
        if (orig) ((uint4*)orig)[i] = make_uint4((~v.x >> 7) & 0x01010101u, (~v.y >> 7) & 0x01010101u, (~v.z >> 7) & 0x01010101u, (~v.w >> 7) & 0x01010101u);
    }
    if (blockIdx.x == 0 && threadIdx.x < n - nv * 16) {
        const unsigned v = scan[nv * 16 + threadIdx.x];
        bm_or(s_bm, v, prev);
        if (orig) orig[nv * 16 + threadIdx.x] = v <= 127u;
    }
    bm_flush(s_bm, rec);
}

// Both anti-aliasing passes of one SF_TH x SF_TW tile through LDS: the tile with its halo as bytes (mirror indexing, as the passes
// index the plane), axis 0 into a second tile truncated to uint8, axis 1 from that tile, the result to `dst` and its bitmap to
// rec[8..16).  ry / rx = 0: no pass on that axis.  w: the scan's weights, axis 0 then axis 1.  Where the scan's bitmap rec[0..8) holds
// two values or fewer the scan's bytes are stored instead (scale_image filters only images of more than two distinct values).
__global__ __launch_bounds__(256) void scan_gauss_tile_kernel(const uint8_t* scan, int H, int W, const double* w, int ry, int rx,
                                                              uint8_t* dst, unsigned* rec) {
    __shared__ uint8_t s_in[(SF_TH + 2 * SF_RMAX) * SF_PITCH];
    __shared__ uint8_t s_mid[SF_TH * SF_PITCH];
    __shared__ double s_w[2][2 * SF_RMAX + 1];
    __shared__ unsigned s_bm[8];
    const int tid = threadIdx.x, x0 = blockIdx.x * SF_TW, y0 = blockIdx.y * SF_TH;
    const int cw = SF_TW + 2 * rx, ch = SF_TH + 2 * ry;
    if (tid < 8) s_bm[tid] = 0;
    if (ry > 0 && tid < 2 * ry + 1) s_w[0][tid] = w[tid];
    if (rx > 0 && tid < 2 * rx + 1) s_w[1][tid] = w[(ry > 0 ? 2 * ry + 1 : 0) + tid];
    for (int i = tid; i < ch * cw; i += 256) {
        const int r = i / cw, c = i - r * cw;
        int gy = y0 - ry + r, gx = x0 - rx + c;
        if ((unsigned)gy >= (unsigned)H) gy = mirror_idx(gy, H);
        if ((unsigned)gx >= (unsigned)W) gx = mirror_idx(gx, W);
        s_in[r * SF_PITCH + c] = scan[(size_t)gy * W + gx];
    }
    __syncthreads();
    const bool aa = bm_count(rec) > 2;
    unsigned prev = 256;
    if (aa) {
        // axis 0: every column of the tile with its halo, the SF_TH rows of the output
        for (int i = tid; i < SF_TH * cw; i += 256) {
            const int r = i / cw, c = i - r * cw;
            const uint8_t* p = s_in + (r + ry) * SF_PITCH + c;
            uint8_t v = *p;
            if (ry > 0) {
                double acc = ld(p, 0) * s_w[0][ry];
                for (int j = ry; j >= 1; --j) acc = acc + (ld(p - j * SF_PITCH, 0) + ld(p + j * SF_PITCH, 0)) * s_w[0][ry - j];
                v = (uint8_t)acc;   // C truncation between the passes, as gauss_pass_kernel<uint8_t, 0> stores it
            }
            s_mid[r * SF_PITCH + c] = v;
        }
        __syncthreads();
    }
    const uint8_t* s_src = aa ? s_mid : s_in + ry * SF_PITCH;
    for (int i = tid; i < SF_TH * SF_TW; i += 256) {
        const int r = i / SF_TW, c = i - r * SF_TW;
        const uint8_t* p = s_src + r * SF_PITCH + c + rx;
        uint8_t v = *p;
        if (aa && rx > 0) {
            double acc = ld(p, 0) * s_w[1][rx];
            for (int j = rx; j >= 1; --j) acc = acc + (ld(p - j, 0) + ld(p + j, 0)) * s_w[1][rx - j];
            v = (uint8_t)acc;
        }
        if (y0 + r < H && x0 + c < W) {
            dst[(size_t)(y0 + r) * W + x0 + c] = v;
            bm_or(s_bm, v, prev);
        }
    }
    bm_flush(s_bm, rec + 8);
}

// Behind the one-pass-per-launch kernels (a radius above SF_RMAX): the bitmap of the filtered plane -> rec[8..16); where the scan's
// own bitmap holds two values or fewer, the scan's bytes replace the plane first.  Both planes are 16-byte aligned.
__global__ __launch_bounds__(256) void scan_select_kernel(const uint8_t* scan, uint8_t* filt, size_t n, unsigned* rec) {
    __shared__ unsigned s_bm[8];
    if (threadIdx.x < 8) s_bm[threadIdx.x] = 0;
    __syncthreads();
    const bool aa = bm_count(rec) > 2;
    unsigned prev = 256;
    const size_t nv = n / 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const uint4 v = aa ? ((const uint4*)filt)[i] : ((const uint4*)scan)[i];
        if (!aa) ((uint4*)filt)[i] = v;
        bm_or_word(s_bm, v.x, prev);
        bm_or_word(s_bm, v.y, prev);
        bm_or_word(s_bm, v.z, prev);
        bm_or_word(s_bm, v.w, prev);
    }
    if (blockIdx.x == 0 && threadIdx.x < n - nv * 16) {
        const size_t i = nv * 16 + threadIdx.x;
        const uint8_t v = aa ? filt[i] : scan[i];
        if (!aa) filt[i] = v;
        bm_or(s_bm, v, prev);
    }
    bm_flush(s_bm, rec + 8);
}

// One thread per page pixel: bicubic_kernel's taps from the (filtered) uint8 plane, the clip to the plane's range (bm: its bitmap),
// prep_map_kernel<2>'s inversion and conversion; and for the same pixel nearest_kernel's coordinate into the scan, ink = scan <= 127
// (the gather commutes with the per-pixel map).  bin may be NULL.  INK: `scan` is the scan-sized ink map (an adaptive binarisation
// has written it), gathered as it is.
template <bool INK>
__global__ __launch_bounds__(256) void scan_sample_kernel(const uint8_t* plane, const uint8_t* scan, int H, int W, uint8_t* img, uint8_t* bin,
                                                          int Ho, int Wo, double fy, double ty, double fx, double tx, const unsigned* bm) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= Wo) return;
    const double yr = fy * (double)oy + ty, xc = fx * (double)ox + tx;
    const double r0f = floor(yr), c0f = floor(xc);
    const double tr = yr - r0f, tc = xc - c0f;
    const int r0 = (int)r0f - 1, c0 = (int)c0f - 1;
    int cols[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cols[k] = mirror_idx(c0 + k, W);
    double fr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t row = (size_t)mirror_idx(r0 + k, H) * W;
        fr[k] = cubic(tc, ld(plane, row + cols[0]), ld(plane, row + cols[1]), ld(plane, row + cols[2]), ld(plane, row + cols[3]));
    }
    double v = cubic(tr, fr[0], fr[1], fr[2], fr[3]);
    double lo, hi;
    bm_range(bm, &lo, &hi);
    v = v < lo ? lo : (v > hi ? hi : v);     // np.clip
    const size_t o = (size_t)oy * Wo + ox;
    img[o] = (uint8_t)((1.0 - v / 255.0) * 255.0);
    if (bin) {
        const int r = mirror_idx((int)(yr > 0.0 ? yr + 0.5 : yr - 0.5), H);
        const int c = mirror_idx((int)(xc > 0.0 ? xc + 0.5 : xc - 0.5), W);
        bin[o] = INK ? scan[(size_t)r * W + c] : (uint8_t)(scan[(size_t)r * W + c] <= 127);
    }
}

// the passes of a scan: radius per axis, 0 where scale_image_dev runs none (sigma <= 1e-15) or the pass is the identity (radius 0:
// its one weight is 1.0)
static void scan_radii(const pseg_scan& s, double sig[2], int rad[2]) {
    sig[0] = std::max(0.0, ((double)s.H0 / (double)s.H - 1.0) / 2.0);
    sig[1] = std::max(0.0, ((double)s.W0 / (double)s.W - 1.0) / 2.0);
    for (int a = 0; a < 2; ++a) rad[a] = sig[a] <= 1e-15 ? 0 : (int)(4.0 * sig[a] + 0.5);
}

int scan_front_check(const pseg_scan& s, int index) {
    if (!s.gray) return fail(PSEG_EINVAL, "scan %d: NULL argument", index);
    if (s.H0 <= 0 || s.W0 <= 0 || s.H <= 0 || s.W <= 0) return fail(PSEG_EINVAL, "scan %d: empty scan or page shape (%d,%d)->(%d,%d)", index, s.H0, s.W0, s.H, s.W);
    if ((int64_t)s.H0 * s.W0 > 0x7fffffffLL || (int64_t)s.H * s.W > 0x7fffffffLL || s.H0 > 65535 || s.H > 65535)
        return fail(PSEG_EUNSUPPORTED, "scan %d: image too large", index);
    double sig[2];
    int rad[2];
    scan_radii(s, sig, rad);
    const double* w[2] = {s.wy, s.wx};
    const int given[2] = {s.ry, s.rx};
    for (int a = 0; a < 2; ++a)
        if (sig[a] > 1e-15 && w[a] && given[a] != rad[a])
            return fail(PSEG_EINVAL, "scan %d: anti-aliasing kernel radius %d does not match sigma %.17g", index, given[a], sig[a]);
    return PSEG_OK;
}

size_t scan_front_weights(const pseg_scan& s, double* dst) {
    double sig[2];
    int rad[2];
    scan_radii(s, sig, rad);
    const double* w[2] = {s.wy, s.wx};
    size_t n = 0;
    for (int a = 0; a < 2; ++a) {
        if (rad[a] == 0) continue;
        const size_t k = (size_t)2 * rad[a] + 1;
        if (dst) {
            if (w[a]) memcpy(dst + n, w[a], k * 8);
            else {
                int r = 0;
                const std::vector<double> own = host_gauss(sig[a], &r);
                memcpy(dst + n, own.data(), k * 8);
            }
        }
        n += k;
    }
    return n;
}

// the filtered planes of a scan
static size_t scan_filt_work(const pseg_scan& s) {
    double sig[2];
    int rad[2];
    scan_radii(s, sig, rad);
    if (rad[0] == 0 && rad[1] == 0) return 0;
    const bool fused = rad[0] <= SF_RMAX && rad[1] <= SF_RMAX;
    return up256((size_t)s.H0 * s.W0) * (!fused && rad[0] > 0 && rad[1] > 0 ? 2 : 1);
}

// behind them, for an adaptive binarisation: the row-sum plane; for that or a despeckling: the scan-sized ink plane unless d_orig takes
// it; for a despeckling: its per-tile workspace
size_t scan_front_work(const pseg_scan& s, const pseg_binarize* how, const pseg_despeckle* dsp) {
    const bool adaptive = how && how->window != 0, clean = dsp && dsp->max_area != 0;
    size_t b = scan_filt_work(s);
    if (adaptive) b += binarize_rows_bytes(s.H0, s.W0);
    if ((adaptive || clean) && !s.final_is_scan) b += up256((size_t)s.H0 * s.W0);
    if (clean) b += despeckle_work_bytes(s.H0, s.W0);
    return b;
}

int scan_front_enqueue(const pseg_scan& s, const uint8_t* d_scan, const double* d_w, uint8_t* d_work, unsigned* d_rec, uint8_t* d_img,
                       uint8_t* d_bin, uint8_t* d_orig, hipStream_t st, const pseg_binarize* how, const pseg_despeckle* dsp) {
    const int H0 = s.H0, W0 = s.W0;
    const size_t n0 = (size_t)H0 * W0;
    double sig[2];
    int rad[2];
    scan_radii(s, sig, rad);
    const int sgrid = (int)std::min<size_t>((n0 / 16 + 255) / 256 + 1, 1024);
    // an adaptive ink map: into d_orig where that is asked for, else (for the sampler's gather alone) into the workspace
    // a despeckling: the ink plane is materialised whatever the threshold (a fixed one's by the statistics pass) and cleaned in place
    uint8_t* d_ink = nullptr;
    const bool adaptive = how && how->window != 0, clean = dsp && dsp->max_area != 0;
    uint8_t* stats_orig = d_orig;
    if ((adaptive || clean) && (d_bin || d_orig)) {
        if (!d_work) return fail(PSEG_EINVAL, "scan front end: no workspace for the binarisation");
        uint8_t* const rows = d_work + scan_filt_work(s);
        uint8_t* const plane = rows + (adaptive ? binarize_rows_bytes(H0, W0) : 0);
        uint8_t* const ink = d_orig ? d_orig : plane;
        if (!d_orig && s.final_is_scan) return fail(PSEG_EINVAL, "scan front end: no ink plane in the workspace of a final_is_scan scan");
        if (adaptive) PSEG_TRY(binarize_enqueue(d_scan, H0, W0, *how, rows, ink, nullptr, st));
        stats_orig = adaptive ? nullptr : ink;
        d_ink = ink;
    }
    scan_stats_kernel<<<sgrid, 256, 0, st>>>(d_scan, n0, d_rec, stats_orig);
    if (clean && d_ink) {
        uint8_t* const dwork = d_work + scan_filt_work(s) + (adaptive ? binarize_rows_bytes(H0, W0) : 0) + (s.final_is_scan ? 0 : up256(n0));
        PSEG_TRY(despeckle_enqueue(d_ink, H0, W0, *dsp, dwork, st));
    }
    const uint8_t* plane = d_scan;
    const unsigned* bm = d_rec;
    if (rad[0] > 0 || rad[1] > 0) {
        if (!d_work || !d_w) return fail(PSEG_EINVAL, "scan front end: no workspace for the filtered plane");
        if (rad[0] <= SF_RMAX && rad[1] <= SF_RMAX) {
            scan_gauss_tile_kernel<<<dim3(cdiv(W0, SF_TW), cdiv(H0, SF_TH)), 256, 0, st>>>(d_scan, H0, W0, d_w, rad[0], rad[1], d_work, d_rec);
        } else {
            // one pass per launch, the last one into the first plane of the workspace
            const dim3 grid(cdiv(W0, 256), H0);
            uint8_t* const second = d_work + up256(n0);
            const uint8_t* cur = d_scan;
            if (rad[0] > 0) {
                uint8_t* const out = rad[1] > 0 ? second : d_work;
                gauss_pass_kernel<uint8_t, 0><<<grid, 256, 0, st>>>(cur, H0, W0, d_w, rad[0], out);
                cur = out;
            }
            if (rad[1] > 0) gauss_pass_kernel<uint8_t, 1><<<grid, 256, 0, st>>>(cur, H0, W0, d_w + (rad[0] > 0 ? 2 * rad[0] + 1 : 0), rad[1], d_work);
            scan_select_kernel<<<sgrid, 256, 0, st>>>(d_scan, d_work, n0, d_rec);
        }
        plane = d_work;
        bm = d_rec + 8;
    }
    double fy, ty, fx, tx;
    warp_coeffs(H0, s.H, &fy, &ty);
    warp_coeffs(W0, s.W, &fx, &tx);
    if (d_ink) scan_sample_kernel<true><<<dim3(cdiv(s.W, 256), s.H), 256, 0, st>>>(plane, d_ink, H0, W0, d_img, d_bin, s.H, s.W, fy, ty, fx, tx, bm);
    else scan_sample_kernel<false><<<dim3(cdiv(s.W, 256), s.H), 256, 0, st>>>(plane, d_scan, H0, W0, d_img, d_bin, s.H, s.W, fy, ty, fx, tx, bm);
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

}  // namespace pseg

extern "C" int pseg_prepare_scans(int device, int n, const pseg_scan* scans, uint8_t* const* out_img, uint8_t* const* out_bin,
                                  uint8_t* const* out_orig) {
    return pseg_prepare_scans_bin(device, n, scans, nullptr, out_img, out_bin, out_orig);
}

extern "C" int pseg_prepare_scans_bin(int device, int n, const pseg_scan* scans, const pseg_binarize* how, uint8_t* const* out_img,
                                      uint8_t* const* out_bin, uint8_t* const* out_orig) {
    return pseg_prepare_scans_clean(device, n, scans, how, nullptr, out_img, out_bin, out_orig);
}

extern "C" int pseg_prepare_scans_clean(int device, int n, const pseg_scan* scans, const pseg_binarize* how, const pseg_despeckle* dsp,
                                        uint8_t* const* out_img, uint8_t* const* out_bin, uint8_t* const* out_orig) {
    if (n < 0 || (n > 0 && (!scans || !out_img || !out_bin))) return fail(PSEG_EINVAL, "bad argument");
    // every scan is checked, and the staging laid out, before any device work starts
    struct At { size_t scan, work, w, img; };
    std::vector<At> at(n);
    size_t b_scan = 0, b_work = 0, n_w = 0, b_img = 0;
    for (int i = 0; i < n; ++i) {
        PSEG_TRY(scan_front_check(scans[i], i));
        if (how) PSEG_TRY(binarize_check(how[i], i));
        if (dsp) PSEG_TRY(despeckle_check(dsp[i], i, "scan"));
        if (!out_img[i] || !out_bin[i]) return fail(PSEG_EINVAL, "scan %d: NULL argument", i);
        at[i] = At{b_scan, b_work, n_w, b_img};
        b_scan += up256((size_t)scans[i].H0 * scans[i].W0);
        pseg_scan alone = scans[i];                             // (final_is_scan is the chain's: here the ink plane may have no other home)
        alone.final_is_scan = 0;
        b_work += scan_front_work(alone, binarize_of(how, i), despeckle_of(dsp, i));
        n_w += scan_front_weights(scans[i], nullptr);
        b_img += up256((size_t)scans[i].H * scans[i].W);
    }
    if (n == 0) return PSEG_OK;
    PSEG_TRY(open_device(device));
    DevMem mem;
    hipStream_t st = nullptr;
    uint8_t *d_scan = nullptr, *d_work = nullptr, *d_img = nullptr, *d_bin = nullptr, *d_orig = nullptr;
    double* d_w = nullptr;
    unsigned* d_rec = nullptr;
    PSEG_TRY(mem.alloc(&d_scan, b_scan));
    PSEG_TRY(mem.alloc(&d_work, b_work));
    PSEG_TRY(mem.alloc(&d_w, n_w));
    PSEG_TRY(mem.alloc(&d_rec, (size_t)n * SCAN_REC_WORDS));
    PSEG_TRY(mem.alloc(&d_img, b_img));
    PSEG_TRY(mem.alloc(&d_bin, b_img));
    PSEG_TRY(mem.alloc(&d_orig, b_scan));
    std::vector<double> h_w(std::max<size_t>(n_w, 1));
    for (int i = 0; i < n; ++i) scan_front_weights(scans[i], h_w.data() + at[i].w);
    GroupDrain drain{st};                                       // never disarmed: h_w and the caller's arrays outlive the copies
    if (n_w) PSEG_HIP(hipMemcpyAsync(d_w, h_w.data(), n_w * 8, hipMemcpyHostToDevice, st));
    PSEG_HIP(hipMemsetAsync(d_rec, 0, (size_t)n * SCAN_REC_WORDS * sizeof(unsigned), st));
    for (int i = 0; i < n; ++i) {
        pseg_scan s = scans[i];
        s.final_is_scan = 0;
        const size_t n0 = (size_t)s.H0 * s.W0, n1 = (size_t)s.H * s.W;
        uint8_t* const orig = out_orig && out_orig[i] ? d_orig + at[i].scan : nullptr;
        PSEG_HIP(hipMemcpyAsync(d_scan + at[i].scan, s.gray, n0, hipMemcpyHostToDevice, st));
        PSEG_TRY(scan_front_enqueue(s, d_scan + at[i].scan, d_w + at[i].w, d_work + at[i].work, d_rec + (size_t)i * SCAN_REC_WORDS,
                                    d_img + at[i].img, d_bin + at[i].img, orig, st, binarize_of(how, i), despeckle_of(dsp, i)));
        PSEG_HIP(hipMemcpyAsync(out_img[i], d_img + at[i].img, n1, hipMemcpyDeviceToHost, st));
        PSEG_HIP(hipMemcpyAsync(out_bin[i], d_bin + at[i].img, n1, hipMemcpyDeviceToHost, st));
        if (orig) PSEG_HIP(hipMemcpyAsync(out_orig[i], orig, n0, hipMemcpyDeviceToHost, st));
    }
    PSEG_HIP(hipStreamSynchronize(st));
    return PSEG_OK;
}
