// pseg_lineheight.hip -- compute_char_height (lib/image_ops.py:58-82) for a LIST of scans, device-resident: pseg_char_heights.
//
// Three ragged launches per group of scans, one read-back:
//   ch_hist_kernel    histogram of every scan into the scan's record (16-byte loads, LDS histograms, <= 256 atomics per workgroup)
//   ch_otsu_kernel    one thread per scan: otsu_from_hist (pseg_common.h, the host entry's own loop) -> the record's threshold
//   ch_window_kernel  one workgroup per (scan, owned tile): thresholds a window around the tile into bit rows in LDS, labels its runs
//                     there (union-find over run indices), and adds the height of every glyph-shaped component whose first pixel
//                     lies in the owned tile to the height bins of the scan's record.
// No label image, no component list, nothing that grows with the component count.  Why the window decides exactly: the glyph
// filter (glyph_shaped) admits only bounding boxes below GLYPH_H_HI rows and GLYPH_W_HI columns.  A fragment of the window whose
// first pixel (top-most row, left-most in it) lies in the owned tile and which reaches the window's left, right or bottom side spans
// more than CH_LEFT, CH_RIGHT columns or CH_BELOW rows, so neither it nor the component it is part of passes the filter; a fragment
// that reaches the top side has its first pixel above the owned tile; every other fragment is a whole component of the scan, and its
// first pixel lies in exactly one owned tile.  So the filter on the fragment's box IS the test, and no side has to be looked at.
#include "pseg_list.h"

#include <algorithm>

namespace pseg {

constexpr int CH_TH = 32, CH_TW = 64;                                  // the owned tile
constexpr int CH_ABOVE = 1, CH_BELOW = GLYPH_H_HI - 1, CH_LEFT = 64, CH_RIGHT = 64;   // the window's aprons
static_assert(CH_BELOW >= GLYPH_H_HI - 1 && CH_LEFT >= GLYPH_W_HI - 1 && CH_RIGHT >= GLYPH_W_HI - 1 && CH_ABOVE >= 1,
              "a fragment that reaches a window side from the owned tile must fail the glyph filter by its box alone");
static_assert(CH_TW == 64 && CH_LEFT == 64 && CH_RIGHT == 64, "a window row is three 64-bit words, the owned tile the middle one");
constexpr int CH_ROWS = CH_ABOVE + CH_TH + CH_BELOW;                   // 92
constexpr int CH_WORDS = 3, CH_COLS = 64 * CH_WORDS;
constexpr int CH_ITEMS = CH_ROWS * CH_WORDS;                           // (row, word) pairs: 276
constexpr int CH_MAXRUNS = CH_ROWS * (CH_COLS / 2);                    // every other pixel starts a run: 8832
constexpr int CH_SLOTS = CH_TH * (CH_TW / 2);                          // runs that start in the owned tile: 1024
constexpr int CH_NTH = 320;                                            // five waves: one (row, word) pair per thread
static_assert(CH_ITEMS <= CH_NTH && CH_ITEMS + 1 <= 64 * 5 && CH_NTH % 64 == 0, "one pass over the pairs; wave 0 scans them five per lane");
constexpr int CH_BIN0 = GLYPH_H_LO + 1, CH_NBINS = GLYPH_H_HI - GLYPH_H_LO - 1;   // heights 11 .. 59: 49 bins
// a scan's record, 32-bit words: the histogram, the threshold, the height bins
constexpr int CH_REC_HIST = 0, CH_REC_THR = 256, CH_REC_BINS = 260, CH_REC_WORDS = 320;
static_assert(CH_REC_BINS + CH_NBINS <= CH_REC_WORDS, "record layout");
constexpr int CH_HIST_BLOCKS = 256;                                    // histogram workgroups of one scan, at most

// one scan of a group: the prefix tables of the ragged launches (tile0: window workgroups, blk0: histogram workgroups in front of it)
struct ChScan {
    int H, W, tiles_x, tile0, blk0, nblk;
    unsigned long long off;                                            // the scan's bytes in the group's buffer, 16-byte aligned
};

template <int ChScan::*FIRST>
__device__ __forceinline__ int ch_scan_of(const ChScan* __restrict__ tab, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                                  // largest i with tab[i].*FIRST <= b
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].*FIRST <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void ch_hist_kernel(const uint8_t* __restrict__ scans, const ChScan* __restrict__ tab, int n,
                                                       unsigned* __restrict__ rec) {
    __shared__ unsigned h[4][256];                                     // one histogram per wave
    const int i = ch_scan_of<&ChScan::blk0>(tab, n, (int)blockIdx.x);
    const ChScan s = tab[i];
    const int b = (int)blockIdx.x - s.blk0;
    for (int k = 0; k < 4; ++k) h[k][threadIdx.x] = 0;
    __syncthreads();
    unsigned* const hw = h[threadIdx.x >> 6];
    const uint8_t* const p = scans + s.off;
    const size_t nbytes = (size_t)s.H * s.W, n16 = nbytes >> 4;
    for (size_t q = (size_t)b * 256 + threadIdx.x; q < n16; q += (size_t)s.nblk * 256) {
        const uint4 v = ((const uint4*)p)[q];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        unsigned prev = w[0] & 255u, cnt = 0;                          // equal neighbours share one LDS add (flat margins)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned c = (w[k >> 2] >> ((k & 3) * 8)) & 255u;
            if (c == prev) ++cnt;
            else { atomicAdd(&hw[prev], cnt); prev = c; cnt = 1; }
        }
        atomicAdd(&hw[prev], cnt);
    }
    if (b == 0)
        for (size_t q = (n16 << 4) + threadIdx.x; q < nbytes; q += 256) atomicAdd(&hw[p[q]], 1u);
    __syncthreads();
    const unsigned sum = h[0][threadIdx.x] + h[1][threadIdx.x] + h[2][threadIdx.x] + h[3][threadIdx.x];
    if (sum) atomicAdd(&rec[(size_t)i * CH_REC_WORDS + CH_REC_HIST + threadIdx.x], sum);
}

__global__ void ch_otsu_kernel(const ChScan* __restrict__ tab, int n, unsigned* rec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned* const r = rec + (size_t)i * CH_REC_WORDS;
    r[CH_REC_THR] = (unsigned)otsu_from_hist(r + CH_REC_HIST, (int64_t)tab[i].H * tab[i].W);
}

__device__ __forceinline__ unsigned long long ch_le(int b) { return b >= 63 ? ~0ull : ((2ull << b) - 1ull); }   // bits 0 .. b
// first pixels of the runs of (row, word)
__device__ __forceinline__ unsigned long long ch_starts(const unsigned long long* bits, int it) {
    const unsigned long long m = bits[it];
    const unsigned long long carry = (it % CH_WORDS) ? bits[it - 1] >> 63 : 0ull;
    return m & ~((m << 1) | carry);
}
// last column of the run of `row` that holds column c
__device__ __forceinline__ int ch_run_end(const unsigned long long* bits, int row, int c) {
    unsigned long long gap = ~bits[row * CH_WORDS + (c >> 6)] & (~0ull << (c & 63));
    for (int w = c >> 6; w < CH_WORDS; ++w) {
        if (gap) return w * 64 + __builtin_ctzll(gap) - 1;
        if (w + 1 < CH_WORDS) gap = ~bits[row * CH_WORDS + w + 1];
    }
    return CH_COLS - 1;
}
__device__ __forceinline__ int ch_find(const int* P, int x) {
    const volatile int* V = P;
    for (int it = 0; it < CH_MAXRUNS; ++it) {                          // (a chain is shorter than the run list)
        const int p = V[x];
        if (p == x) break;
        x = p;
    }
    return x;
}
// the smaller root becomes the root: a fragment's root is its first run, top-most row, left-most in it
__device__ __forceinline__ void ch_unite(int* P, int a, int b) {
    for (int it = 0; it < CH_MAXRUNS; ++it) {
        a = ch_find(P, a);
        b = ch_find(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&P[a], b);
        if (old == a) return;
        a = old;                                                       // another thread linked a first: join what it linked to
    }
}

__global__ __launch_bounds__(CH_NTH) void ch_window_kernel(const uint8_t* __restrict__ scans, const ChScan* __restrict__ tab, int n, int inverse,
                                                           unsigned* __restrict__ rec) {
    __shared__ unsigned long long bits[CH_ITEMS];                      // ink of the window, [row][word]
    __shared__ int runbase[CH_ITEMS + 1];                              // runs in front of (row, word), in row-major order
    __shared__ int parent[CH_MAXRUNS];                                 // union-find over run indices
    __shared__ unsigned ymax[CH_SLOTS], xmax[CH_SLOTS], xmin[CH_SLOTS];   // the box of the fragment rooted at the k-th run of an owned row
    __shared__ unsigned bins[CH_NBINS];
    const int tid = threadIdx.x;
    const int i = ch_scan_of<&ChScan::tile0>(tab, n, (int)blockIdx.x);
    const ChScan s = tab[i];
    const int tile = (int)blockIdx.x - s.tile0;
    const int ty = tile / s.tiles_x, tx = tile - ty * s.tiles_x;
    const int y0 = ty * CH_TH - CH_ABOVE, x0 = tx * CH_TW - CH_LEFT;   // the window's first row and column
    const int t = (int)rec[(size_t)i * CH_REC_WORDS + CH_REC_THR];
    const bool inv = inverse != 0;
    const uint8_t* const p = scans + s.off;
    // ---- the window as bit rows: ink = (pixel > t) == inverse (binarize_kernel), paper outside the scan.  A thread takes four
    // pixels (one dword where rows are dword-aligned), eight threads make a 32-bit word.
    {
        unsigned* const bits32 = (unsigned*)bits;
        constexpr int NDW = CH_ROWS * (CH_COLS / 4);
        static_assert(NDW % 8 == 0 && (CH_COLS / 4) % 8 == 0, "eight neighbouring lanes fill one word");
        const bool w4 = (s.W & 3) == 0;
        for (int g0 = 0; g0 < NDW; g0 += CH_NTH) {
            const int g = g0 + tid;
            unsigned nib = 0;
            if (g < NDW) {
                const int row = g / (CH_COLS / 4), c4 = g - row * (CH_COLS / 4);
                const int y = y0 + row, x = x0 + 4 * c4;              // x is a multiple of four
                if (y >= 0 && y < s.H && x >= 0 && x < s.W) {
                    const uint8_t* const q = p + (size_t)y * s.W + x;
                    if (w4 || x + 3 < s.W) {
                        unsigned v;
                        if (w4) v = *(const unsigned*)q;
                        else v = q[0] | (q[1] << 8) | (q[2] << 16) | ((unsigned)q[3] << 24);
#pragma unroll
                        for (int k = 0; k < 4; ++k) nib |= (unsigned)(((int)((v >> (8 * k)) & 255u) > t) == inv) << k;
                    } else {
                        for (int k = 0; k < 4; ++k)
                            if (x + k < s.W) nib |= (unsigned)(((int)q[k] > t) == inv) << k;
                    }
                }
            }
            unsigned v = nib << (4 * (g & 7));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            v |= __shfl_xor(v, 4);
            if (g < NDW && (g & 7) == 0) bits32[g >> 3] = v;
        }
    }
    for (int k = tid; k < CH_SLOTS; k += CH_NTH) { ymax[k] = 0; xmax[k] = 0; xmin[k] = CH_COLS; }
    if (tid < CH_NBINS) bins[tid] = 0;
    __syncthreads();
    if (!__syncthreads_or(tid < CH_TH && bits[(CH_ABOVE + tid) * CH_WORDS + 1] != 0)) return;   // no first pixel here
    // ---- the run list: runs are numbered by row, then column
    unsigned long long st0 = 0;
    if (tid < CH_ITEMS) { st0 = ch_starts(bits, tid); runbase[tid] = __popcll(st0); }
    __syncthreads();
    if (tid < 64) {
        int v[5], sum = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) { const int j = tid * 5 + k; v[k] = j < CH_ITEMS ? runbase[j] : 0; sum += v[k]; }
        int inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (tid >= o) inc += u; }
        int run = inc - sum;
#pragma unroll
        for (int k = 0; k < 5; ++k) { const int j = tid * 5 + k; if (j <= CH_ITEMS) runbase[j] = run; run += v[k]; }
    }
    __syncthreads();
    const int total = runbase[CH_ITEMS];                               // <= CH_MAXRUNS: a row of CH_COLS pixels has at most CH_COLS / 2 runs
    for (int k = tid; k < total; k += CH_NTH) parent[k] = k;
    __syncthreads();
    // ---- unions with the overlapping runs of the row above (4-connectivity)
    const int row = tid / CH_WORDS, word = tid - row * CH_WORDS;
    if (tid < CH_ITEMS && row > 0) {
        unsigned long long st = st0;
        const int base = runbase[tid];
        for (int k = 0; k < 32 && st; ++k) {                           // a word starts at most 32 runs
            const int cs = word * 64 + __builtin_ctzll(st);
            st &= st - 1;
            const int ce = ch_run_end(bits, row, cs);
            for (int w = cs >> 6; w <= (ce >> 6); ++w) {
                const int lo = w == (cs >> 6) ? (cs & 63) : 0, hi = w == (ce >> 6) ? (ce & 63) : 63;
                const int up_it = (row - 1) * CH_WORDS + w;
                const unsigned long long ov = bits[up_it] & ch_le(hi) & (~0ull << lo);
                unsigned long long gs = ov & ~(ov << 1);               // one bit per run of the row above under this span
                if (!gs) continue;
                const unsigned long long ust = ch_starts(bits, up_it);
                const int ubase = runbase[up_it];
                for (int j = 0; j < 32 && gs; ++j) {
                    const int b = __builtin_ctzll(gs);
                    gs &= gs - 1;
                    ch_unite(parent, base + k, ubase + __popcll(ust & ch_le(b)) - 1);   // (no start up to b in this word: the run that comes in from the left)
                }
            }
        }
    }
    __syncthreads();
    // ---- every run adds its extent to the box of its root, where that root starts in the owned tile
    if (tid < CH_ITEMS && row > 0) {
        unsigned long long st = st0;
        const int base = runbase[tid];
        const int own0 = runbase[CH_ABOVE * CH_WORDS], own1 = runbase[(CH_ABOVE + CH_TH) * CH_WORDS];
        for (int k = 0; k < 32 && st; ++k) {
            const int cs = word * 64 + __builtin_ctzll(st);
            st &= st - 1;
            const int root = ch_find(parent, base + k);
            if (root < own0 || root >= own1) continue;
            int lo = CH_ABOVE * CH_WORDS, hi = (CH_ABOVE + CH_TH) * CH_WORDS - 1;
            while (lo < hi) {                                          // the (row, word) pair whose runs hold `root`
                const int mid = (lo + hi + 1) >> 1;
                if (runbase[mid] <= root) lo = mid; else hi = mid - 1;
            }
            if (lo % CH_WORDS != 1) continue;
            const int slot = (lo / CH_WORDS - CH_ABOVE) * (CH_TW / 2) + (root - runbase[lo]);
            atomicMax(&ymax[slot], (unsigned)row);
            atomicMax(&xmax[slot], (unsigned)ch_run_end(bits, row, cs));
            atomicMin(&xmin[slot], (unsigned)cs);
        }
    }
    __syncthreads();
    for (int k = tid; k < CH_SLOTS; k += CH_NTH) {
        const int ym = (int)ymax[k];
        if (!ym) continue;                                             // (a root's own row is >= CH_ABOVE >= 1)
        const int h = ym - (k / (CH_TW / 2) + CH_ABOVE) + 1, w = (int)xmax[k] - (int)xmin[k] + 1;
        if (glyph_shaped(h, w)) atomicAdd(&bins[h - CH_BIN0], 1u);
    }
    __syncthreads();
    if (tid < CH_NBINS && bins[tid]) atomicAdd(&rec[(size_t)i * CH_REC_WORDS + CH_REC_BINS + tid], bins[tid]);
}

// ---- workspace: grow-only, one per device (the group's table, records and scan bytes; a page-locked copy of table and records);
// a call holds the device's lock to its end and ends synchronised.  pseg_release_workspace frees it.
struct ChWs {
    GrowDev dev; GrowPin pin;
    void release() { dev.release(); pin.release(); }
};
static PerDevice<ChWs> g_ch;

// upper median of the heights a record's bins hold: the smallest h whose cumulative count exceeds n / 2 -- hs[hs.size() / 2] of the sorted list
static int median_from_bins(const unsigned* bins, int n_bins, int first) {
    unsigned long long n = 0, cum = 0;
    for (int k = 0; k < n_bins; ++k) n += bins[k];
    if (n == 0) return -1;
    for (int k = 0; k < n_bins; ++k) {
        cum += bins[k];
        if (cum > n / 2) return first + k;
    }
    return -1;
}

static int ch_group(ChWs& ws, int g0, int g1, const uint8_t* const* gray, const int* H, const int* W, int inverse, int* heights, int* otsu) {
    const int n = g1 - g0;
    constexpr size_t tab_b = (size_t)LIST_GROUP_ITEMS * sizeof(ChScan), rec_b = (size_t)LIST_GROUP_ITEMS * CH_REC_WORDS * 4;
    static_assert(tab_b % 16 == 0 && rec_b % 16 == 0, "the scans start 16-byte aligned");
    PSEG_TRY(ws.pin.ensure(tab_b + rec_b, "line-height records"));
    ChScan* const h_tab = ws.pin.as<ChScan>();
    Bump at{tab_b + rec_b};
    long long tiles = 0, blks = 0;
    for (int k = 0; k < n; ++k) {
        ChScan& s = h_tab[k];
        s.H = H[g0 + k]; s.W = W[g0 + k];
        const size_t bytes = (size_t)s.H * s.W;
        s.tiles_x = cdiv(s.W, CH_TW);
        s.tile0 = (int)tiles;
        s.blk0 = (int)blks;
        s.nblk = (int)std::max<size_t>(1, std::min<size_t>(CH_HIST_BLOCKS, ((bytes >> 4) + 1023) / 1024));
        s.off = at.take(bytes, 16);
        tiles += (long long)s.tiles_x * cdiv(s.H, CH_TH);
        blks += s.nblk;
    }
    if (tiles > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "scans %d..%d: too many tiles for one launch", g0, g1 - 1);
    PSEG_TRY(ws.dev.ensure(at.off, "line-height workspace"));
    uint8_t* const d = ws.dev.p;
    ChScan* const d_tab = (ChScan*)d;
    unsigned* const d_rec = (unsigned*)(d + tab_b);
    hipStream_t st = nullptr;
    GroupDrain drain{st};
    PSEG_HIP(hipMemcpyAsync(d_tab, h_tab, (size_t)n * sizeof(ChScan), hipMemcpyHostToDevice, st));
    PSEG_HIP(hipMemsetAsync(d_rec, 0, (size_t)n * CH_REC_WORDS * 4, st));
    for (int k = 0; k < n; ++k)
        PSEG_HIP(hipMemcpyAsync(d + h_tab[k].off, gray[g0 + k], (size_t)h_tab[k].H * h_tab[k].W, hipMemcpyHostToDevice, st));
    ch_hist_kernel<<<(unsigned)blks, 256, 0, st>>>(d, d_tab, n, d_rec);
    ch_otsu_kernel<<<cdiv(n, 64), 64, 0, st>>>(d_tab, n, d_rec);
    ch_window_kernel<<<(unsigned)tiles, CH_NTH, 0, st>>>(d, d_tab, n, inverse, d_rec);
    PSEG_HIP(hipGetLastError());
    unsigned* const h_rec = (unsigned*)(ws.pin.p + tab_b);
    PSEG_HIP(hipMemcpyAsync(h_rec, d_rec, (size_t)n * CH_REC_WORDS * 4, hipMemcpyDeviceToHost, st));
    PSEG_HIP(hipStreamSynchronize(st));                                // the group's one wait
    drain.armed = false;
    for (int k = 0; k < n; ++k) {
        const unsigned* r = h_rec + (size_t)k * CH_REC_WORDS;
        heights[g0 + k] = median_from_bins(r + CH_REC_BINS, CH_NBINS, CH_BIN0);
        otsu[g0 + k] = (int)r[CH_REC_THR];
    }
    return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_char_heights(int device, int n, const uint8_t* const* gray, const int* H, const int* W, int inverse, int* heights, int* otsu) {
    if (n == 0) return PSEG_OK;
    if (n < 0 || !gray || !H || !W || !heights) return fail(PSEG_EINVAL, n < 0 ? "negative scan count" : "NULL argument");
    for (int i = 0; i < n; ++i) {
        if (!gray[i]) return fail(PSEG_EINVAL, "scan %d: NULL argument", i);
        if (H[i] <= 0 || W[i] <= 0) return fail(PSEG_EINVAL, "scan %d: empty image", i);
        if ((int64_t)H[i] * W[i] > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "scan %d: image too large", i);
    }
    std::vector<int> hs((size_t)n), ts((size_t)n);                     // the caller's arrays are written once every group has run
    PSEG_TRY(run_list(g_ch, device, n, [&](int i) { return (size_t)H[i] * W[i]; },
                      [&](ChWs& ws, int g0, int g1) { return ch_group(ws, g0, g1, gray, H, W, inverse, hs.data(), ts.data()); }));
    std::copy(hs.begin(), hs.end(), heights);
    if (otsu) std::copy(ts.begin(), ts.end(), otsu);
    return PSEG_OK;
}

int pseg_char_height_window(int* tile_h, int* tile_w, int* above, int* below, int* left, int* right) {
    if (tile_h) *tile_h = CH_TH;
    if (tile_w) *tile_w = CH_TW;
    if (above) *above = CH_ABOVE;
    if (below) *below = CH_BELOW;
    if (left) *left = CH_LEFT;
    if (right) *right = CH_RIGHT;
    return PSEG_OK;
}

int pseg_char_height_median(const uint32_t* bins, int n_bins, int first, int* height) {
    if (!bins || !height || n_bins < 0) return fail(PSEG_EINVAL, "bad argument");
    *height = median_from_bins(bins, n_bins, first);
    return PSEG_OK;
}

}  // extern "C"
