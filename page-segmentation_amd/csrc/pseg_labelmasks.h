// pseg_labelmasks.h -- what the device kernel and the host entry of the label-map loader share (pseg_labelmasks.hip):
// the source coordinate of an output pixel, the packed colour table and the label of a pixel.  One body each for the host and the
// device; every source is built with -ffp-contract=off, so both give the same bits.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace pseg {

constexpr int LM_COLORS_MAX = 256;     // entries of the colour table
constexpr int LM_BINS = 257;           // counters per mask: one per id, and [256] for the pixels of unknown colour

// periodic 'mirror' extension without an edge repeat (mirror_idx of pseg_resize.hip): d c b | a b c d | c b a
__host__ __device__ inline int lm_mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// the order-0 warp of pseg_resize.hip per axis (warp_coeffs): output index o reads source coordinate f * o + t
__host__ __device__ inline void lm_coeffs(int n_in, int n_out, double* f, double* t) {
    *f = (double)n_in / (double)n_out;
    *t = *f * 0.5 - 0.5;
}

// nearest_kernel's source index of output index o: f * o + t, rounded half away from zero, mirrored into [0, n_in)
__host__ __device__ inline int lm_src_index(int o, double f, double t, int n_in) {
    const double v = f * (double)o + t;
    return lm_mirror((int)(v > 0.0 ? v + 0.5 : v - 0.5), n_in);
}

// one table entry: the colour in the high 24 bits, the id in the low 8
__host__ __device__ inline uint32_t lm_pack(unsigned r, unsigned g, unsigned b, unsigned id) { return (r << 24) | (g << 16) | (b << 8) | id; }

// What a thread remembers between neighbouring pixels: the last colour looked up and what it gave.  Region masks are flat, so
// most pixels end here without a search.
struct LmLast {
    uint32_t key = 0xffffffffu;        // no 24-bit colour
    uint32_t id = 0;
    bool unknown = false;
};

// The label of source pixel `col` of a row: for a 3-channel row the id of the table entry of its colour, 0 and *unknown where
// there is none (linear search, the first n entries of tab); for a 1-channel row the byte itself.
__host__ __device__ inline uint32_t lm_label(const uint8_t* __restrict__ row, int col, int channels, const uint32_t* tab, int n, LmLast& last,
                                             bool* unknown) {
    if (channels == 1) {
        *unknown = false;
        return row[col];
    }
    const uint8_t* const p = row + (size_t)col * 3;
    const uint32_t key = ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | (uint32_t)p[2];
    if (key != last.key) {
        last.key = key;
        last.id = 0;
        last.unknown = true;
        for (int k = 0; k < n; ++k) {
            const uint32_t w = tab[k];
            if ((w >> 8) == key) {
                last.id = w & 255u;
                last.unknown = false;
                break;
            }
        }
    }
    *unknown = last.unknown;
    return last.id;
}

}  // namespace pseg
