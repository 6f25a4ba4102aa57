// pseg_binarize.h -- what the device kernels and the host entry of the adaptive binarisation share (pseg_binarize.hip):
// the index rule, the packed moments and the decision.  One body each for the host and the device; every source is built with
// -ffp-contract=off, so both give the same bits.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace pseg {

constexpr int BZ_WINDOW_MIN = 3, BZ_WINDOW_MAX = 255;

// periodic 'mirror' extension without an edge repeat (NumPy's mode='reflect', mirror_idx of pseg_resize.hip): d c b | a b c d | c b a
__host__ __device__ inline int bz_mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// Both moments of a pixel in one 64-bit word: the sum of squares in the low BZ_SQ_BITS bits, the sum above them.  A sum over at most
// BZ_PACK_MAX pixels keeps both fields inside their widths (255^2 * 2^24 < 2^40, 255 * 2^24 < 2^32 > the 24 bits left: the sum's
// bound is what limits the count), so one 64-bit add or subtract moves both and a difference of two prefix words is the pair of
// differences.  The window sums need 255 * 255^2 < 2^24 and 255^2 * 255^2 < 2^32.
constexpr int BZ_SQ_BITS = 40;
constexpr unsigned long long BZ_SQ_MASK = (1ull << BZ_SQ_BITS) - 1ull;
constexpr long long BZ_PACK_MAX = ((1ll << (64 - BZ_SQ_BITS)) - 1) / 255;          // 65793 pixels
static_assert(255ll * 255 * BZ_PACK_MAX <= (long long)BZ_SQ_MASK, "the squares of that many pixels fit their field");
static_assert((long long)BZ_WINDOW_MAX * BZ_WINDOW_MAX <= BZ_PACK_MAX, "a window's moments fit the packed word");
__host__ __device__ inline unsigned long long bz_pack(unsigned v) { return ((unsigned long long)v << BZ_SQ_BITS) | (unsigned long long)(v * v); }

// Sauvola's decision for a pixel of value v from the integer moments of its n window samples: *T is the float64 threshold, the return
// value ink = v <= T.  Float64 throughout, in this operation order.
__host__ __device__ inline bool bz_decide(unsigned long long packed, unsigned v, double n, double k, double R, double* T) {
    const double S1 = (double)(packed >> BZ_SQ_BITS), S2 = (double)(packed & BZ_SQ_MASK);
    const double m = S1 / n;
    const double var = S2 / n - m * m;
    const double s = sqrt(var > 0.0 ? var : 0.0);
    const double t = m * (1.0 + k * (s / R - 1.0));
    *T = t;
    return (double)v <= t;
}

}  // namespace pseg
