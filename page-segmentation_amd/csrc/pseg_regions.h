// pseg_regions.h -- what the device kernels and the host entry of the text regions share (pseg_regions.hip): the bit
// planes' word, border and offset arithmetic.  One body each for the host and the device.
//
// A plane holds 64 pixels to a 64-bit word: bit b of word j of a row is pixel 64 j + b.  A plane at rest is CANONICAL: the bits of a
// row's last word beyond W are 0.  dil(m, k)[x] = OR of m[x + d - k/2], d in 0..k-1, m = 0 outside the map; ero is the same
// expression with AND and m = 1 outside, i.e. the complement of the dilation of the complement WITH THE SAME OFFSETS (OpenCV's
// rule: anchor k/2, the element is not reflected).  So one loader serves both: it hands out the word (dilation) or its complement
// (erosion) with everything outside the map -- words beyond the row, rows beyond the map, the tail bits of the last word -- as 0, the
// passes only ever OR, and the store complements an erosion's result and clears the tail again.
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/pseg.h"

namespace pseg {

constexpr int RG_SIDE_MAX = 255;                   // a side of a rectangle: 1..255
constexpr int RG_TH = 32, RG_TW = 64;              // a component tile: 32 rows of one word
constexpr int RG_SLOTS = 2 * (RG_TH + RG_TW);      // root slots of a tile: an open component owns a pixel of the rim (188 pixels)
constexpr int RG_RIM = 2 * (RG_TH + RG_TW);        // rim table: [0,64) top row, [64,128) bottom row, [128,160) left column, [160,192) right column
constexpr int RG_BAND = 128;                       // output rows of a morphology workgroup
constexpr int RG_WC = 4;                           // word columns of a morphology workgroup
constexpr int RG_ROWS_MAX = RG_BAND + RG_SIDE_MAX - 1;   // rows of a band with its halo of k - 1
constexpr int RG_ROW_INTS = 8;                     // a table row: x0, y0, x1, y1 (exclusive), area, seed_y, seed_x, 0
static_assert(RG_SLOTS <= 255, "a slot is a byte; 255 says none");

typedef unsigned long long rg_word;

__host__ __device__ inline int rg_words(int W) { return (W + 63) >> 6; }
// the pixels of word j that lie inside a row of W pixels
__host__ __device__ inline rg_word rg_tail_mask(int W, int j) {
    const int left = W - (j << 6);
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : ((1ull << left) - 1ull);
}
// word j of a row as the passes see it: the plane's word, or its complement for an erosion; 0 wherever the map is not
__host__ __device__ inline rg_word rg_load(const rg_word* row, int wpr, int W, int j, bool ero) {
    if (j < 0 || j >= wpr) return 0ull;
    const rg_word w = row[j];
    return (ero ? ~w : w) & rg_tail_mask(W, j);
}
// what a pass's OR becomes in the plane: complemented back for an erosion, canonical again
__host__ __device__ inline rg_word rg_store(rg_word v, int W, int j, bool ero) { return (ero ? ~v : v) & rg_tail_mask(W, j); }

// element i of a five-word window, i in 0..5 (5: beyond it, 0), without indexing by a variable
__host__ __device__ inline rg_word rg_pick(rg_word v0, rg_word v1, rg_word v2, rg_word v3, rg_word v4, int i) {
    return i == 0 ? v0 : i == 1 ? v1 : i == 2 ? v2 : i == 3 ? v3 : i == 4 ? v4 : 0ull;
}

// The x pass of word j: out[x] = OR of in[x + d - k/2], d in 0..k-1.  The words j-2 .. j+2 are one 320-bit string (pixel 64 j + b at
// position 128 + b); F[p] = OR of the k positions from p on, by shift-and-OR doubling across the words (1, 2, 4, ... while twice the
// width still fits k, then one more shift by k - width); the answer is the 64 positions from 128 - k/2.  k/2 <= 127 and
// k - 1 - k/2 <= 127, so nothing beyond the five words is ever asked for.
__host__ __device__ inline rg_word rg_xpass(const rg_word* row, int wpr, int W, int j, int k, bool ero) {
    rg_word v0 = rg_load(row, wpr, W, j - 2, ero), v1 = rg_load(row, wpr, W, j - 1, ero), v2 = rg_load(row, wpr, W, j, ero),
            v3 = rg_load(row, wpr, W, j + 1, ero), v4 = rg_load(row, wpr, W, j + 2, ero);
    if (k <= 1) return v2;
    int p = 1;
    for (int it = 0; it < 8 && 2 * p <= k; ++it) {
        if (p < 64) {
            const int up = 64 - p;
            v0 |= (v0 >> p) | (v1 << up);
            v1 |= (v1 >> p) | (v2 << up);
            v2 |= (v2 >> p) | (v3 << up);
            v3 |= (v3 >> p) | (v4 << up);
            v4 |= (v4 >> p);
        } else {                                   // p == 64: a whole word
            v0 |= v1; v1 |= v2; v2 |= v3; v3 |= v4;
        }
        p <<= 1;
    }
    const int s = k - p;                           // 0 <= s < p <= 128
    if (s > 0) {
        const int q = s >> 6, b = s & 63;
        // the string shifted down by q words (q is 0 or 1), then by b bits
        const rg_word a0 = q ? v1 : v0, a1 = q ? v2 : v1, a2 = q ? v3 : v2, a3 = q ? v4 : v3, a4 = q ? 0ull : v4;
        if (b) {
            const int up = 64 - b;
            v0 |= (a0 >> b) | (a1 << up);
            v1 |= (a1 >> b) | (a2 << up);
            v2 |= (a2 >> b) | (a3 << up);
            v3 |= (a3 >> b) | (a4 << up);
            v4 |= (a4 >> b);
        } else {
            v0 |= a0; v1 |= a1; v2 |= a2; v3 |= a3; v4 |= a4;
        }
    }
    const int e = 128 - (k >> 1);                  // 1 <= e <= 128
    const int q = e >> 6, b = e & 63;
    const rg_word lo = rg_pick(v0, v1, v2, v3, v4, q), hi = rg_pick(v0, v1, v2, v3, v4, q + 1);
    return b ? (lo >> b) | (hi << (64 - b)) : lo;
}

// the first row a band's window reads for output row y0: row r of the band's rows is map row y0 - k/2 + r, and output row y0 + o is
// the OR of rows o .. o + k - 1
__host__ __device__ inline int rg_band_first(int y0, int k) { return y0 - (k >> 1); }

__host__ __device__ inline bool rg_side_ok(int k) { return k >= 1 && k <= RG_SIDE_MAX; }

// ---- the crack polygon of a region on a canonical bit plane (the word-run walk of the device tracer and of its host twin) -------------
// Directions: 0 east, 1 south, 2 west, 3 north (y grows downwards).  At a corner, heading d, `right` is the pixel ahead on the
// region's side and `left` the one ahead on the other side.
__host__ __device__ inline int rg_turn(int d, bool right, bool left) { return !right ? ((d + 1) & 3) : left ? ((d + 3) & 3) : d; }

__host__ __device__ inline bool rg_bit(const rg_word* T, int H, int W, int wpr, int x, int y) {
    return x >= 0 && x < W && y >= 0 && y < H && ((T[(size_t)y * wpr + (x >> 6)] >> (x & 63)) & 1ull) != 0;
}
__host__ __device__ inline int rg_ctz(rg_word v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (int)__ffsll((long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}
__host__ __device__ inline int rg_clz(rg_word v) {
#ifdef __HIP_DEVICE_COMPILE__
    return (int)__clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}

// How many corners in a row, from corner x on, go straight on a horizontal heading: R is the row of the `right` pixels, L the row of
// the `left` ones (either may be NULL: a row outside the map).  East: the pixels x, x + 1, ... with R set and L unset, a word at a
// time by ctz; west: the pixels x - 1, x - 2, ... by clz.  The planes are canonical, so a run ends at the map's last column by itself.
__host__ __device__ inline int rg_hrun(const rg_word* R, const rg_word* L, int wpr, int x, bool east) {
    if (!R) return 0;
    int n = 0;
    if (east) {
        int j = x >> 6, b = x & 63;
        for (int it = 0; it < wpr && j < wpr; ++it, ++j, b = 0) {
            const rg_word bad = ~((R[j] & ~(L ? L[j] : 0ull)) >> b);   // the shift brings in zeros: c <= 64 - b
            const int c = bad ? rg_ctz(bad) : 64;
            n += c;
            if (c < 64 - b) break;
        }
    } else {
        if (x <= 0) return 0;
        int j = (x - 1) >> 6, b = (x - 1) & 63;
        for (int it = 0; it < wpr && j >= 0; ++it, --j, b = 63) {
            const rg_word g = (R[j] & ~(L ? L[j] : 0ull)) << (63 - b);
            const int c = ~g ? rg_clz(~g) : 64;
            n += c < b + 1 ? c : b + 1;
            if (c < b + 1) break;
        }
    }
    return n;
}

// The walk from the seed (sx, sy) of a region of plane T: clockwise from the seed's top-left corner, arriving there heading north;
// a vertex wherever the direction changes.  Horizontal stretches are taken a run at a time (rg_hrun), vertical ones row by row.
// Returns the number of vertices, or -1 when the walk does not close within 4 (H + 1) (W + 1) + 4 steps.  xy may be NULL (count
// only); never more than `limit` vertices are written.
__host__ __device__ inline long long rg_trace_words(const rg_word* T, int H, int W, int wpr, int sx, int sy, int32_t* xy, long long limit) {
    int vx = sx, vy = sy, d = 3;
    long long nv = 0, steps = 0;
    const long long bound = 4ll * ((long long)H + 1) * ((long long)W + 1) + 4;
    for (long long it = 0; it < bound && steps < bound; ++it) {
        if (d == 0 || d == 2) {
            // east: right (x, vy), left (x, vy - 1); west: right (x - 1, vy - 1), left (x - 1, vy)
            const int ry = d == 0 ? vy : vy - 1, ly = d == 0 ? vy - 1 : vy;
            const int n = rg_hrun(ry >= 0 && ry < H ? T + (size_t)ry * wpr : nullptr, ly >= 0 && ly < H ? T + (size_t)ly * wpr : nullptr, wpr, vx, d == 0);
            if (n > 0) {
                vx += d == 0 ? n : -n;
                steps += n;
                if (vx == sx && vy == sy) return nv;
            }
        }
        int rx, ry, lx, ly;
        switch (d) {
            case 0: rx = vx; ry = vy; lx = vx; ly = vy - 1; break;
            case 1: rx = vx - 1; ry = vy; lx = vx; ly = vy; break;
            case 2: rx = vx - 1; ry = vy - 1; lx = vx - 1; ly = vy; break;
            default: rx = vx; ry = vy - 1; lx = vx - 1; ly = vy - 1; break;
        }
        const int nd = rg_turn(d, rg_bit(T, H, W, wpr, rx, ry), rg_bit(T, H, W, wpr, lx, ly));
        if (nd != d) {
            if (xy && nv < limit) { xy[2 * nv] = vx; xy[2 * nv + 1] = vy; }
            ++nv;
        }
        d = nd;
        vx += d == 0 ? 1 : d == 2 ? -1 : 0;
        vy += d == 1 ? 1 : d == 3 ? -1 : 0;
        ++steps;
        if (vx == sx && vy == sy) return nv;
    }
    return -1;
}

// ---- the stream-ordered stage for the page chain (pseg_regions.hip; host) --------------------------------------------------------------
// Label maps already on the device in; plane 2, the unsorted rows, the counts, the vertex counts, their offsets, the maps' records
// (total, first vertex, status, fits) and the vertices (max_vertices per map, map k at k * max_vertices) on the device out, at these
// byte offsets of a workspace of `bytes` bytes.  rg_stage_plan sizes it up front (host arithmetic); rg_stage_enqueue fills the
// page-locked table (tab_bytes) and launches on the caller's stream: no host wait, no allocation.  d_cap and h_cap are what the caller
// really holds at d and h_tab: a layout that outgrows either is refused before anything is launched.
struct RgStageLay { size_t cnt, rows, nv, voff, mapv, xy, bytes, tab_bytes; };
constexpr int RG_MAPV = 4;                         // long long per map: the vertex total, its first vertex in the group's array, the status, fits
int rg_stage_check(const pseg_regions& how, const char* what, int i);
int rg_stage_plan(int n, const int* H, const int* W, int max_regions, long long max_vertices, RgStageLay* out);
int rg_stage_enqueue(hipStream_t st, uint8_t* d, void* h_tab, int n, const uint8_t* const* d_labels, const int* H, const int* W,
                     const pseg_regions* how, int max_regions, long long max_vertices, size_t d_cap, size_t h_cap, RgStageLay* out);
void rg_stage_blob(int count, int max_regions, long long max_vertices, const long long* mapv, int32_t* rows, const long long* nv,
                   const long long* voff, const int32_t* xy, std::vector<int32_t>& blob);

}  // namespace pseg
