// pseg_binarize.hip -- Sauvola's adaptive threshold over a square window for a LIST of gray scans, device-resident
// (pseg_binarize_scans), for one scan inside the scan chain's front end (binarize_enqueue), and on the host (pseg_binarize_scans_host).
//
// The cost per pixel does not depend on the window.  Two launches, integer sums only:
//   bz_rows_*   one workgroup per (row, segment of BZ_CAP - 2 r columns): the segment with its mirrored halo goes through LDS, every
//               thread sums BZ_EPT neighbouring pixels, a wave-level scan and one LDS pass make the prefix P of the packed moments
//               (pseg_binarize.h), and P[x + r + 1] - P[x - r] is written as one 64-bit word per pixel, 16 bytes per store
//   bz_cols_*   one thread per column of a band of BZ_BAND rows: the first window from 2 r + 1 words, then one add and one subtract
//               per row, bz_decide on the pair of sums, the ink byte and (where asked for) the float64 threshold
// _list: ragged over a group's scans through a table (as ch_hist_kernel, pseg_lineheight.hip); _one: one scan, the record by value.
#include "pseg_list.h"
#include "pseg_binarize.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pseg {

constexpr int BZ_NTH = 256, BZ_EPT = 8, BZ_CAP = BZ_NTH * BZ_EPT;      // row kernel: threads, pixels per thread, padded pixels per segment
constexpr int BZ_BAND = 64, BZ_CT = 64;                                // column kernel: rows per band, columns per workgroup (one wave)
static_assert(BZ_CAP <= BZ_PACK_MAX, "a segment's prefix fits the packed word");
static_assert(BZ_CAP - (BZ_WINDOW_MAX - 1) > 0 && (BZ_CAP % 2) == 0, "a segment owns an even, positive number of columns at every window");

// one scan: geometry, parameters, planes (device pointers) and the prefix tables of the ragged launches
struct BzScan {
    const uint8_t* scan;                // H x W, dense; 16-byte aligned, readable up to the next multiple of 16 bytes behind its end
    unsigned long long* rows;           // H x pitch row sums, 16-byte aligned (untouched for a fixed entry)
    uint8_t* ink;                       // H x W
    double* thr;                        // H x W or NULL
    double k, R, n;                     // n = window * window
    int H, W, r, fixed;                 // fixed: ink = scan <= 127, no window
    int pitch, seg, segs, tiles_x;      // words per row of `rows`; columns a row workgroup owns, such workgroups per row; column tiles
    int row0, col0;                     // workgroups of the group's scans in front of this one (row / column launch)
};

static inline int bz_pitch(int W) { return (W + 1) & ~1; }

template <int BzScan::*FIRST>
__device__ __forceinline__ int bz_scan_of(const BzScan* __restrict__ tab, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                                  // largest i with tab[i].*FIRST <= b
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].*FIRST <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void bz_rows_body(const BzScan& s, int blk) {
    __shared__ uint4 s_raw[(BZ_CAP + 32) / 16];                        // the row's bytes from the 16-byte boundary in front of the segment's first
    __shared__ unsigned long long s_P[BZ_CAP + 1];                     // P[p]: packed moments of the padded pixels in front of p
    __shared__ unsigned long long s_wave[BZ_NTH / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int y = blk / s.segs, sg = blk - y * s.segs;
    const int x0 = sg * s.seg, xe = min(s.W, x0 + s.seg);             // the columns owned: [x0, xe)
    const int N = xe - x0 + 2 * s.r;                                   // padded pixel p is column x0 - r + p: N <= BZ_CAP
    const int a = max(0, x0 - s.r), b = min(s.W, xe + s.r);            // the columns read; every mirrored index of the halo lies in [a, b)
    const uint8_t* const row = s.scan + (size_t)y * s.W + a;
    const unsigned mis = (unsigned)((uintptr_t)row & 15);
    const uint4* const src = (const uint4*)(row - mis);
    const int nv = (int)(mis + (unsigned)(b - a) + 15u) >> 4;         // <= (15 + BZ_CAP + 15) / 16
    for (int i = tid; i < nv; i += BZ_NTH) s_raw[i] = src[i];
    __syncthreads();
    const uint8_t* const raw = (const uint8_t*)s_raw + mis;            // raw[x - a]
    unsigned long long loc[BZ_EPT], tot = 0;
    const int p0 = tid * BZ_EPT;
#pragma unroll
    for (int j = 0; j < BZ_EPT; ++j) {
        const int p = p0 + j;
        unsigned v = 0;
        if (p < N) {
            int x = x0 - s.r + p;
            if ((unsigned)x >= (unsigned)s.W) x = bz_mirror(x, s.W);
            v = raw[x - a];
        }
        tot += bz_pack(v);
        loc[j] = tot;
    }
    unsigned long long inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) s_wave[tid >> 6] = inc;
    __syncthreads();
    unsigned long long base = inc - tot;
    for (int w = 0; w < (tid >> 6); ++w) base += s_wave[w];
    if (tid == 0) s_P[0] = 0;
#pragma unroll
    for (int j = 0; j < BZ_EPT; ++j) s_P[p0 + j + 1] = base + loc[j];
    __syncthreads();
    unsigned long long* const out = s.rows + (size_t)y * s.pitch + x0; // 16-byte aligned: pitch and x0 are even
    const int no = xe - x0, w = 2 * s.r + 1;
    for (int q = 2 * tid; q < no; q += 2 * BZ_NTH) {
        const unsigned long long r0 = s_P[q + w] - s_P[q];
        if (q + 1 < no) *(ulonglong2*)(out + q) = make_ulonglong2(r0, s_P[q + 1 + w] - s_P[q + 1]);
        else out[q] = r0;
    }
}

__device__ __forceinline__ void bz_cols_body(const BzScan& s, int blk) {
    const int by = blk / s.tiles_x, tx = blk - by * s.tiles_x;
    const int x = tx * BZ_CT + (int)threadIdx.x;
    if (x >= s.W) return;
    const int y0 = by * BZ_BAND, y1 = min(s.H, y0 + BZ_BAND);
    if (s.fixed) {
        for (int y = y0; y < y1; ++y) {
            const size_t o = (size_t)y * s.W + x;
            s.ink[o] = s.scan[o] <= 127;
            if (s.thr) s.thr[o] = 127.0;
        }
        return;
    }
    const unsigned long long* const rows = s.rows + x;
    unsigned long long S = 0;
    for (int dy = -s.r; dy <= s.r; ++dy) {
        int yy = y0 + dy;
        if ((unsigned)yy >= (unsigned)s.H) yy = bz_mirror(yy, s.H);
        S += rows[(size_t)yy * s.pitch];
    }
    for (int y = y0;;) {
        const size_t o = (size_t)y * s.W + x;
        double T;
        s.ink[o] = bz_decide(S, s.scan[o], s.n, s.k, s.R, &T);
        if (s.thr) s.thr[o] = T;
        if (++y >= y1) break;
        int ya = y + s.r, ys = y - s.r - 1;                            // the row that enters and the row that leaves
        if (ya >= s.H) ya = bz_mirror(ya, s.H);
        if (ys < 0) ys = bz_mirror(ys, s.H);
        S += rows[(size_t)ya * s.pitch] - rows[(size_t)ys * s.pitch];
    }
}

__global__ __launch_bounds__(BZ_NTH) void bz_rows_list_kernel(const BzScan* __restrict__ tab, int n) {
    const int i = bz_scan_of<&BzScan::row0>(tab, n, (int)blockIdx.x);
    const BzScan s = tab[i];
    bz_rows_body(s, (int)blockIdx.x - s.row0);
}
__global__ __launch_bounds__(BZ_CT) void bz_cols_list_kernel(const BzScan* __restrict__ tab, int n) {
    const int i = bz_scan_of<&BzScan::col0>(tab, n, (int)blockIdx.x);
    const BzScan s = tab[i];
    bz_cols_body(s, (int)blockIdx.x - s.col0);
}
__global__ __launch_bounds__(BZ_NTH) void bz_rows_one_kernel(const BzScan s) { bz_rows_body(s, (int)blockIdx.x); }
__global__ __launch_bounds__(BZ_CT) void bz_cols_one_kernel(const BzScan s) { bz_cols_body(s, (int)blockIdx.x); }

// geometry and parameters of one scan; *row_blocks / *col_blocks: the workgroups of its two launches (no row launch for a fixed entry)
static void bz_fill(BzScan& s, int H, int W, const pseg_binarize& how, long long* row_blocks, long long* col_blocks) {
    s.H = H; s.W = W;
    s.fixed = how.window == 0;
    s.r = how.window / 2;
    s.k = how.k; s.R = how.R;
    s.n = (double)how.window * (double)how.window;
    s.pitch = bz_pitch(W);
    s.seg = BZ_CAP - 2 * s.r;
    s.segs = cdiv(W, s.seg);
    s.tiles_x = cdiv(W, BZ_CT);
    *row_blocks = s.fixed ? 0 : (long long)H * s.segs;
    *col_blocks = (long long)s.tiles_x * cdiv(H, BZ_BAND);
}

int binarize_check(const pseg_binarize& b, int index) {
    if (b.window == 0) return PSEG_OK;
    if (b.window < BZ_WINDOW_MIN || b.window > BZ_WINDOW_MAX)
        return fail(PSEG_EINVAL, "scan %d: window %d outside %d..%d (0: the fixed threshold)", index, b.window, BZ_WINDOW_MIN, BZ_WINDOW_MAX);
    if ((b.window & 1) == 0) return fail(PSEG_EINVAL, "scan %d: even window %d", index, b.window);
    if (!(b.k >= 0.0 && b.k <= 1.0)) return fail(PSEG_EINVAL, "scan %d: k %g outside [0, 1]", index, b.k);
    if (!(b.R > 0.0) || !std::isfinite(b.R)) return fail(PSEG_EINVAL, "scan %d: R %g is not a positive number", index, b.R);
    return PSEG_OK;
}

size_t binarize_rows_bytes(int H, int W) { return up256((size_t)H * bz_pitch(W) * sizeof(unsigned long long)); }

int binarize_enqueue(const uint8_t* d_scan, int H, int W, const pseg_binarize& how, uint8_t* d_rows, uint8_t* d_ink, double* d_thr, hipStream_t st) {
    BzScan s;
    memset(&s, 0, sizeof s);
    long long rb = 0, cb = 0;
    bz_fill(s, H, W, how, &rb, &cb);
    if (rb > 0x7fffffffLL || cb > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "binarisation: a %d x %d scan is too large for one launch", H, W);
    s.scan = d_scan; s.rows = (unsigned long long*)d_rows; s.ink = d_ink; s.thr = d_thr;
    if (rb) bz_rows_one_kernel<<<(unsigned)rb, BZ_NTH, 0, st>>>(s);
    bz_cols_one_kernel<<<(unsigned)cb, BZ_CT, 0, st>>>(s);
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

// ---- workspace of the list entry: grow-only, one per device (the group's table, scans and planes; a page-locked copy of the table);
// a call holds the device's lock to its end and ends synchronised.  pseg_release_workspace frees it.
struct BzWs {
    GrowDev dev; GrowPin pin;
    void release() { dev.release(); pin.release(); }
};
static PerDevice<BzWs> g_bz;

static int bz_group(BzWs& ws, int g0, int g1, const uint8_t* const* gray, const int* H, const int* W, const pseg_binarize* how,
                    uint8_t* const* out_ink, double* const* out_thr) {
    const int n = g1 - g0;
    constexpr size_t tab_b = up256((size_t)LIST_GROUP_ITEMS * sizeof(BzScan));
    PSEG_TRY(ws.pin.ensure(tab_b, "binarisation table"));
    BzScan* const h_tab = ws.pin.as<BzScan>();
    memset(h_tab, 0, tab_b);
    std::vector<size_t> o_scan(n), o_rows(n), o_ink(n), o_thr(n);
    Bump at{tab_b};
    long long rows_total = 0, cols_total = 0;
    for (int k = 0; k < n; ++k) {
        const int i = g0 + k;
        BzScan& s = h_tab[k];
        long long rb = 0, cb = 0;
        bz_fill(s, H[i], W[i], how[i], &rb, &cb);
        s.row0 = (int)rows_total;
        s.col0 = (int)cols_total;
        rows_total += rb;
        cols_total += cb;
        if (rows_total > 0x7fffffffLL || cols_total > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "scans %d..%d: too many tiles for one launch", g0, g1 - 1);
        const size_t px = (size_t)s.H * s.W;
        o_scan[k] = at.take(px);
        o_ink[k] = at.take(px);
        o_rows[k] = at.take(s.fixed ? 0 : binarize_rows_bytes(s.H, s.W));
        o_thr[k] = at.take(out_thr && out_thr[i] ? px * sizeof(double) : 0);
    }
    PSEG_TRY(ws.dev.ensure(at.off, "binarisation workspace"));
    uint8_t* const d = ws.dev.p;
    for (int k = 0; k < n; ++k) {
        BzScan& s = h_tab[k];
        s.scan = d + o_scan[k];
        s.ink = d + o_ink[k];
        s.rows = (unsigned long long*)(d + o_rows[k]);
        s.thr = out_thr && out_thr[g0 + k] ? (double*)(d + o_thr[k]) : nullptr;
    }
    hipStream_t st = nullptr;
    GroupDrain drain{st};
    PSEG_HIP(hipMemcpyAsync(d, h_tab, (size_t)n * sizeof(BzScan), hipMemcpyHostToDevice, st));
    for (int k = 0; k < n; ++k)
        PSEG_HIP(hipMemcpyAsync(d + o_scan[k], gray[g0 + k], (size_t)h_tab[k].H * h_tab[k].W, hipMemcpyHostToDevice, st));
    if (rows_total) bz_rows_list_kernel<<<(unsigned)rows_total, BZ_NTH, 0, st>>>((const BzScan*)d, n);
    bz_cols_list_kernel<<<(unsigned)cols_total, BZ_CT, 0, st>>>((const BzScan*)d, n);
    PSEG_HIP(hipGetLastError());
    for (int k = 0; k < n; ++k) {
        const size_t px = (size_t)h_tab[k].H * h_tab[k].W;
        PSEG_HIP(hipMemcpyAsync(out_ink[g0 + k], d + o_ink[k], px, hipMemcpyDeviceToHost, st));
        if (h_tab[k].thr) PSEG_HIP(hipMemcpyAsync(out_thr[g0 + k], d + o_thr[k], px * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    PSEG_HIP(hipStreamSynchronize(st));                                // the group's one wait
    drain.armed = false;
    return PSEG_OK;
}

// what both list entries refuse, before any work
static int bz_check_list(int n, const uint8_t* const* gray, const int* H, const int* W, const pseg_binarize* how, uint8_t* const* out_ink) {
    if (n < 0 || !gray || !H || !W || !how || !out_ink) return fail(PSEG_EINVAL, n < 0 ? "negative scan count" : "NULL argument");
    for (int i = 0; i < n; ++i) {
        if (!gray[i] || !out_ink[i]) return fail(PSEG_EINVAL, "scan %d: NULL argument", i);
        if (H[i] <= 0 || W[i] <= 0) return fail(PSEG_EINVAL, "scan %d: empty image", i);
        if ((int64_t)H[i] * W[i] > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "scan %d: image too large", i);
        PSEG_TRY(binarize_check(how[i], i));
    }
    return PSEG_OK;
}

// one scan on the host: the row sums of every row by a prefix, then the window sums of all columns slid down row by row
static void bz_host_one(const uint8_t* g, int H, int W, const pseg_binarize& how, uint8_t* ink, double* thr) {
    const size_t px = (size_t)H * W;
    if (how.window == 0) {
        for (size_t o = 0; o < px; ++o) {
            ink[o] = g[o] <= 127;
            if (thr) thr[o] = 127.0;
        }
        return;
    }
    const int r = how.window / 2;
    const double n = (double)how.window * (double)how.window;
    std::vector<unsigned long long> rows(px), P((size_t)W + 2 * r + 1), S((size_t)W, 0);
    for (int y = 0; y < H; ++y) {
        const uint8_t* const row = g + (size_t)y * W;
        P[0] = 0;
        for (int p = 0; p < W + 2 * r; ++p) {                          // (a row's prefix may pass the packed fields' widths: the differences are
            const int x = p - r;                                       //  taken modulo 2^64 and each lies inside them)
            P[(size_t)p + 1] = P[p] + bz_pack(row[(unsigned)x < (unsigned)W ? x : bz_mirror(x, W)]);
        }
        for (int x = 0; x < W; ++x) rows[(size_t)y * W + x] = P[(size_t)x + 2 * r + 1] - P[x];
    }
    for (int dy = -r; dy <= r; ++dy) {
        const unsigned long long* const a = rows.data() + (size_t)bz_mirror(dy, H) * W;
        for (int x = 0; x < W; ++x) S[x] += a[x];
    }
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            const size_t o = (size_t)y * W + x;
            double T;
            ink[o] = bz_decide(S[x], g[o], n, how.k, how.R, &T);
            if (thr) thr[o] = T;
        }
        if (y + 1 == H) break;
        const unsigned long long* const a = rows.data() + (size_t)bz_mirror(y + 1 + r, H) * W;
        const unsigned long long* const b = rows.data() + (size_t)bz_mirror(y - r, H) * W;
        for (int x = 0; x < W; ++x) S[x] += a[x] - b[x];
    }
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_binarize_scans(int device, int n, const uint8_t* const* gray, const int* H, const int* W, const pseg_binarize* how,
                        uint8_t* const* out_ink, double* const* out_threshold) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(bz_check_list(n, gray, H, W, how, out_ink));
    return run_list(g_bz, device, n, [&](int i) { return (size_t)H[i] * W[i]; },
                    [&](BzWs& ws, int g0, int g1) { return bz_group(ws, g0, g1, gray, H, W, how, out_ink, out_threshold); });
}

int pseg_binarize_scans_host(int n, const uint8_t* const* gray, const int* H, const int* W, const pseg_binarize* how,
                             uint8_t* const* out_ink, double* const* out_threshold) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(bz_check_list(n, gray, H, W, how, out_ink));
    for (int i = 0; i < n; ++i) bz_host_one(gray[i], H[i], W[i], how[i], out_ink[i], out_threshold ? out_threshold[i] : nullptr);
    return PSEG_OK;
}

int pseg_binarize_geometry(int* segment, int* band, int* tile, int* vector) {
    if (segment) *segment = BZ_CAP;
    if (band) *band = BZ_BAND;
    if (tile) *tile = BZ_CT;
    if (vector) *vector = 16;
    return PSEG_OK;
}

}  // extern "C"
