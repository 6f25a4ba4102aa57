// pseg_despeckle.h -- what the device kernels and the host entry of the despeckling share (pseg_despeckle.hip): the
// range of max_area, the decision and the size arithmetic.  One body each for the host and the device.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace pseg {

constexpr int DS_AREA_MAX = 1 << 24;               // 16 777 216

// a component of `size` pixels is a speck, and is erased, when it has at most max_area pixels
__host__ __device__ inline bool ds_speck(unsigned size, int max_area) { return size <= (unsigned)max_area; }

// size counters are 32-bit and saturate.  A map has fewer than 2^31 pixels (the entries refuse a larger one), so no component's sum
// ever reaches the bound: the saturation only keeps a broken table from wrapping a huge size into a small one.
__host__ __device__ inline unsigned ds_add_sat(unsigned a, unsigned b) { const unsigned s = a + b; return s < a ? 0xffffffffu : s; }

}  // namespace pseg
