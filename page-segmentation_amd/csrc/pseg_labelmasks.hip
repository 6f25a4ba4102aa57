// pseg_labelmasks.hip -- the label maps of a LIST of training masks, device-resident (pseg_label_masks) and on the host
// (pseg_label_masks_host): colour -> id through a table and the order-0 resize to the page's shape in one pass, with the number of
// pixels per id and of unknown colour.  Lookup and gather commute: only the sampled source pixels are read.
//
// One ragged launch per group over a table (as bz_cols_list_kernel, pseg_binarize.hip).  A workgroup owns LM_TH rows of LM_RUNS
// runs; a thread owns one run of a row.  Run 0 of a row is the 0..7 pixels in front of the first 8-byte boundary of the dense label
// map, run j >= 1 the LM_RUN pixels behind boundary j - 1: every full run is one 8-byte store, whatever W is, and the head and the
// row's tail go byte by byte.  The colour table sits in LDS, one word per entry, and is searched linearly; the counts go into 257
// LDS counters per workgroup, a thread adding once per stretch of equal ids, and the non-zero ones into the mask's row of 64-bit
// counters with one vector atomic each.
#include "pseg_list.h"
#include "pseg_labelmasks.h"

#include <cstring>

namespace pseg {

constexpr int LM_NTH = 256, LM_RUN = 8, LM_RUNS = 32, LM_TH = LM_NTH / LM_RUNS;    // threads, pixels per run, runs and rows per workgroup
static_assert(LM_RUN == 8, "a full run is one uint2 store");
static_assert((long long)LM_NTH * LM_RUN < (1ll << 32), "a workgroup's pixels fit a 32-bit counter");

// one mask: geometry, warp coefficients, planes (device pointers) and the prefix of the ragged launch
struct LmMask {
    const uint8_t* src;                 // H0 x W0 x channels, dense
    uint8_t* out;                       // H x W, dense, 8-byte aligned
    double fy, ty, fx, tx;
    int H0, W0, channels, H, W;
    int tiles_x, blk0;                  // workgroups per band of LM_TH rows; workgroups of the group's masks in front of this one
};

static inline size_t lm_src_bytes(const pseg_mask_src& m) { return (size_t)m.H0 * m.W0 * m.channels; }
// runs of a row: the head and the 8-byte words the row touches behind it
static inline int lm_tiles_x(int W) { return cdiv(cdiv(W, LM_RUN) + 1, LM_RUNS); }

__device__ __forceinline__ int lm_mask_of(const LmMask* __restrict__ tab, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                                  // largest i with tab[i].blk0 <= b
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// a thread's counting: one LDS add per stretch of equal ids
struct LmTally {
    uint32_t id = 0, n = 0, unknown = 0;
    __device__ __forceinline__ void add(unsigned* s_cnt, uint32_t v, bool unk) {
        if (v != id && n) { atomicAdd(&s_cnt[id], n); n = 0; }
        id = v;
        ++n;
        unknown += unk;
    }
    __device__ __forceinline__ void flush(unsigned* s_cnt) {
        if (n) atomicAdd(&s_cnt[id], n);
        if (unknown) atomicAdd(&s_cnt[LM_COLORS_MAX], unknown);
    }
};

template <bool COUNTS>
__global__ __launch_bounds__(LM_NTH) void lm_list_kernel(const LmMask* __restrict__ tab, int n, const uint32_t* __restrict__ colors, int n_colors,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ uint32_t s_tab[LM_COLORS_MAX];
    __shared__ unsigned s_cnt[COUNTS ? LM_BINS : 1];
    const int tid = threadIdx.x;
    const int i = lm_mask_of(tab, n, (int)blockIdx.x);
    const LmMask s = tab[i];
    for (int k = tid; k < n_colors; k += LM_NTH) s_tab[k] = colors[k];
    if (COUNTS)
        for (int k = tid; k < LM_BINS; k += LM_NTH) s_cnt[k] = 0;
    __syncthreads();
    const int blk = (int)blockIdx.x - s.blk0;
    const int by = blk / s.tiles_x, bx = blk - by * s.tiles_x;
    const int r = by * LM_TH + tid / LM_RUNS, j = bx * LM_RUNS + (tid & (LM_RUNS - 1));
    if (r < s.H) {
        const size_t row0 = (size_t)r * s.W;
        const int head = min(s.W, (int)((8u - (unsigned)(row0 & 7)) & 7u));          // pixels in front of the row's first 8-byte boundary
        // run j >= 1 starts at head + 8 (j - 1) <= W + 8 LM_RUNS: no overflow for any W of an image that passed the checks
        const int c0 = j == 0 ? 0 : head + (j - 1) * LM_RUN;
        const int c1 = j == 0 ? head : min(s.W, c0 + LM_RUN);
        if (c0 < c1) {
            const uint8_t* const srow = s.src + (size_t)lm_src_index(r, s.fy, s.ty, s.H0) * s.W0 * s.channels;
            uint8_t* const orow = s.out + row0;
            LmLast last;
            LmTally tally;
            if (c1 - c0 == LM_RUN && j > 0) {                                          // orow + c0 is 8-byte aligned
                uint32_t w[2] = {0, 0};
#pragma unroll
                for (int q = 0; q < LM_RUN; ++q) {
                    bool unk;
                    const uint32_t v = lm_label(srow, lm_src_index(c0 + q, s.fx, s.tx, s.W0), s.channels, s_tab, n_colors, last, &unk);
                    w[q >> 2] |= v << (8 * (q & 3));
                    if (COUNTS) tally.add(s_cnt, v, unk);
                }
                *(uint2*)(orow + c0) = make_uint2(w[0], w[1]);
            } else {
                for (int c = c0; c < c1; ++c) {                                        // the head and the ragged tail: at most 7 pixels
                    bool unk;
                    const uint32_t v = lm_label(srow, lm_src_index(c, s.fx, s.tx, s.W0), s.channels, s_tab, n_colors, last, &unk);
                    orow[c] = (uint8_t)v;
                    if (COUNTS) tally.add(s_cnt, v, unk);
                }
            }
            if (COUNTS) tally.flush(s_cnt);
        }
    }
    if (COUNTS) {
        __syncthreads();
        unsigned long long* const mine = counts + (size_t)i * LM_BINS;
        for (int k = tid; k < LM_BINS; k += LM_NTH)
            if (s_cnt[k]) atomicAdd(&mine[k], (unsigned long long)s_cnt[k]);
    }
}

// ---- workspace: grow-only, one per device (the group's table, colour table, counters, sources and label maps; a page-locked copy of
// the tables and the counters' read-back slot); a call holds the device's lock to its end and ends synchronised.
struct LmWs {
    GrowDev dev; GrowPin pin;
    void release() { dev.release(); pin.release(); }
};
static PerDevice<LmWs> g_lm;

// the packed table of a checked colour list
static void lm_table(const uint8_t* colors, const uint8_t* ids, int n_colors, uint32_t* tab) {
    for (int k = 0; k < n_colors; ++k) tab[k] = lm_pack(colors[3 * k], colors[3 * k + 1], colors[3 * k + 2], ids[k]);
}

static int lm_group(LmWs& ws, int g0, int g1, const pseg_mask_src* masks, const int* H, const int* W, const uint32_t* table, int n_colors,
                    uint8_t* const* out_labels, int64_t* out_counts) {
    const int n = g1 - g0;
    constexpr size_t tab_b = up256((size_t)LIST_GROUP_ITEMS * sizeof(LmMask));
    constexpr size_t col_b = up256((size_t)LM_COLORS_MAX * sizeof(uint32_t));
    constexpr size_t cnt_b = up256((size_t)LIST_GROUP_ITEMS * LM_BINS * sizeof(unsigned long long));
    PSEG_TRY(ws.pin.ensure(tab_b + col_b + cnt_b, "label-map tables"));
    LmMask* const h_tab = ws.pin.as<LmMask>();
    uint32_t* const h_col = (uint32_t*)(ws.pin.p + tab_b);
    const unsigned long long* const h_cnt = (const unsigned long long*)(ws.pin.p + tab_b + col_b);
    memset(h_tab, 0, tab_b);
    memset(h_col, 0, col_b);
    memcpy(h_col, table, (size_t)n_colors * sizeof(uint32_t));
    std::vector<size_t> o_src(n), o_out(n);
    Bump at{tab_b + col_b + cnt_b};
    long long blocks = 0;
    for (int k = 0; k < n; ++k) {
        const int i = g0 + k;
        LmMask& s = h_tab[k];
        s.H0 = masks[i].H0; s.W0 = masks[i].W0; s.channels = masks[i].channels; s.H = H[i]; s.W = W[i];
        lm_coeffs(s.H0, s.H, &s.fy, &s.ty);
        lm_coeffs(s.W0, s.W, &s.fx, &s.tx);
        s.tiles_x = lm_tiles_x(s.W);
        s.blk0 = (int)blocks;
        blocks += (long long)s.tiles_x * cdiv(s.H, LM_TH);
        if (blocks > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "masks %d..%d: too many tiles for one launch", g0, g1 - 1);
        o_src[k] = at.take(lm_src_bytes(masks[i]));
        o_out[k] = at.take((size_t)s.H * s.W);
    }
    PSEG_TRY(ws.dev.ensure(at.off, "label-map workspace"));
    uint8_t* const d = ws.dev.p;
    for (int k = 0; k < n; ++k) {
        h_tab[k].src = d + o_src[k];
        h_tab[k].out = d + o_out[k];
    }
    const uint32_t* const d_col = (const uint32_t*)(d + tab_b);
    unsigned long long* const d_cnt = (unsigned long long*)(d + tab_b + col_b);
    hipStream_t st = nullptr;
    GroupDrain drain{st};
    PSEG_HIP(hipMemcpyAsync(d, h_tab, tab_b + col_b, hipMemcpyHostToDevice, st));
    for (int k = 0; k < n; ++k) PSEG_HIP(hipMemcpyAsync(d + o_src[k], masks[g0 + k].px, lm_src_bytes(masks[g0 + k]), hipMemcpyHostToDevice, st));
    if (out_counts) {
        PSEG_HIP(hipMemsetAsync(d_cnt, 0, (size_t)n * LM_BINS * sizeof(unsigned long long), st));
        lm_list_kernel<true><<<(unsigned)blocks, LM_NTH, 0, st>>>((const LmMask*)d, n, d_col, n_colors, d_cnt);
    } else {
        lm_list_kernel<false><<<(unsigned)blocks, LM_NTH, 0, st>>>((const LmMask*)d, n, d_col, n_colors, nullptr);
    }
    PSEG_HIP(hipGetLastError());
    for (int k = 0; k < n; ++k)
        PSEG_HIP(hipMemcpyAsync(out_labels[g0 + k], d + o_out[k], (size_t)h_tab[k].H * h_tab[k].W, hipMemcpyDeviceToHost, st));
    if (out_counts) PSEG_HIP(hipMemcpyAsync((void*)h_cnt, d_cnt, (size_t)n * LM_BINS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PSEG_HIP(hipStreamSynchronize(st));                                // the group's one wait
    drain.armed = false;
    if (out_counts)
        for (size_t k = 0; k < (size_t)n * LM_BINS; ++k) out_counts[(size_t)g0 * LM_BINS + k] = (int64_t)h_cnt[k];
    return PSEG_OK;
}

// what both entries refuse, before any work; *table (LM_COLORS_MAX words) receives the packed colours
static int lm_check_list(int n, const pseg_mask_src* masks, const int* H, const int* W, const uint8_t* colors, const uint8_t* ids, int n_colors,
                         uint8_t* const* out_labels, uint32_t* table) {
    if (n < 0 || !masks || !H || !W || !out_labels) return fail(PSEG_EINVAL, n < 0 ? "negative mask count" : "NULL argument");
    if (n_colors < 0 || n_colors > LM_COLORS_MAX) return fail(PSEG_EINVAL, "%d colours (0..%d)", n_colors, LM_COLORS_MAX);
    for (int i = 0; i < n; ++i) {
        const pseg_mask_src& m = masks[i];
        if (!m.px || !out_labels[i]) return fail(PSEG_EINVAL, "mask %d: NULL argument", i);
        if (m.H0 <= 0 || m.W0 <= 0 || H[i] <= 0 || W[i] <= 0) return fail(PSEG_EINVAL, "mask %d: empty source or output shape (%d,%d)->(%d,%d)", i, m.H0, m.W0, H[i], W[i]);
        if (m.channels != 1 && m.channels != 3) return fail(PSEG_EINVAL, "mask %d: %d channels (3: RGB, 1: ids)", i, m.channels);
        if (m.channels == 3 && n_colors > 0 && (!colors || !ids)) return fail(PSEG_EINVAL, "mask %d: an RGB mask and %d colours, but a NULL table", i, n_colors);
        if ((int64_t)m.H0 * m.W0 > 0x7fffffffLL / 4 || (int64_t)H[i] * W[i] > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "mask %d: image too large", i);
    }
    if (colors && ids) {
        lm_table(colors, ids, n_colors, table);
        for (int a = 1; a < n_colors; ++a)
            for (int b = 0; b < a; ++b)
                if ((table[a] >> 8) == (table[b] >> 8))
                    return fail(PSEG_EINVAL, "colour %d repeats colour %d (%u,%u,%u)", a, b, colors[3 * a], colors[3 * a + 1], colors[3 * a + 2]);
    }
    return PSEG_OK;
}

static void lm_host_one(const pseg_mask_src& m, int H, int W, const uint32_t* table, int n_colors, uint8_t* out, int64_t* counts) {
    double fy, ty, fx, tx;
    lm_coeffs(m.H0, H, &fy, &ty);
    lm_coeffs(m.W0, W, &fx, &tx);
    if (counts) memset(counts, 0, LM_BINS * sizeof(int64_t));
    std::vector<int> cols(W);
    for (int c = 0; c < W; ++c) cols[c] = lm_src_index(c, fx, tx, m.W0);
    for (int r = 0; r < H; ++r) {
        const uint8_t* const srow = m.px + (size_t)lm_src_index(r, fy, ty, m.H0) * m.W0 * m.channels;
        LmLast last;
        for (int c = 0; c < W; ++c) {
            bool unk;
            const uint32_t v = lm_label(srow, cols[c], m.channels, table, n_colors, last, &unk);
            out[(size_t)r * W + c] = (uint8_t)v;
            if (counts) { ++counts[v]; counts[LM_COLORS_MAX] += unk; }
        }
    }
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_label_masks(int device, int n, const pseg_mask_src* masks, const int* H, const int* W, const uint8_t* colors, const uint8_t* ids,
                     int n_colors, uint8_t* const* out_labels, int64_t* out_counts) {
    if (n == 0) return PSEG_OK;
    uint32_t table[LM_COLORS_MAX] = {0};
    PSEG_TRY(lm_check_list(n, masks, H, W, colors, ids, n_colors, out_labels, table));
    if (!colors || !ids) n_colors = 0;                                 // (only 1-channel masks, or no colours at all)
    return run_list(g_lm, device, n, [&](int i) { return lm_src_bytes(masks[i]); },
                    [&](LmWs& ws, int g0, int g1) { return lm_group(ws, g0, g1, masks, H, W, table, n_colors, out_labels, out_counts); });
}

int pseg_label_masks_host(int n, const pseg_mask_src* masks, const int* H, const int* W, const uint8_t* colors, const uint8_t* ids, int n_colors,
                          uint8_t* const* out_labels, int64_t* out_counts) {
    if (n == 0) return PSEG_OK;
    uint32_t table[LM_COLORS_MAX] = {0};
    PSEG_TRY(lm_check_list(n, masks, H, W, colors, ids, n_colors, out_labels, table));
    if (!colors || !ids) n_colors = 0;
    for (int i = 0; i < n; ++i) lm_host_one(masks[i], H[i], W[i], table, n_colors, out_labels[i], out_counts ? out_counts + (size_t)i * LM_BINS : nullptr);
    return PSEG_OK;
}

int pseg_label_masks_geometry(int* run, int* runs, int* rows, int* group_masks, int64_t* group_bytes) {
    if (run) *run = LM_RUN;
    if (runs) *runs = LM_RUNS;
    if (rows) *rows = LM_TH;
    if (group_masks) *group_masks = LIST_GROUP_ITEMS;
    if (group_bytes) *group_bytes = (int64_t)LIST_GROUP_BYTES;
    return PSEG_OK;
}

int pseg_label_masks_groups(int n, const pseg_mask_src* masks, int* group_of) {
    if (n < 0 || (n > 0 && (!masks || !group_of))) return fail(PSEG_EINVAL, n < 0 ? "negative mask count" : "NULL argument");
    for (int i = 0; i < n; ++i)
        if (masks[i].H0 <= 0 || masks[i].W0 <= 0 || (masks[i].channels != 1 && masks[i].channels != 3) || (int64_t)masks[i].H0 * masks[i].W0 > 0x7fffffffLL / 4)
            return fail(PSEG_EINVAL, "mask %d: empty shape, or channels other than 1 or 3", i);
    int g = 0;
    for (int g0 = 0; g0 < n; ++g) {
        const int g1 = list_group_end(n, g0, [&](int i) { return lm_src_bytes(masks[i]); });
        for (int i = g0; i < g1; ++i) group_of[i] = g;
        g0 = g1;
    }
    return PSEG_OK;
}

}  // extern "C"
