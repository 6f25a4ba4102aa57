// pseg_skew.hip -- the skew of a LIST of ink maps from strip profiles, and their exact rotation, device-resident and on the host
// (DESIGN.md 5n).  The contract is integer arithmetic and lives in pseg_skew.h; this file has the kernels, the group function of the
// three list entries (estimate, rotate, both) and the host twins, which walk the same functions in plain loops.
//
// A group costs up to four ragged launches over a table and ONE host wait:
//   sk_strips_kernel   a thread per (row, strip): the map's ink bytes of 32 columns counted into one byte of R (16-byte loads
//                      between the 16-byte boundaries of the dense map, bytes in front of and behind them);
//   sk_score_kernel    a workgroup per (candidate, map): the candidate's strip offsets in LDS, lanes stride over the profile rows
//                      -M .. H-1+M, a 64-bit sum of squares per lane, a wave and a workgroup reduction, ONE plain store;
//   sk_pick_kernel     a wave per map: the winner under the tie rule, one int;
//   sk_rotate_kernel   a thread per run of 8 output pixels between the 8-byte boundaries of the dense output (as lm_list_kernel),
//                      (C, S) from the table at the index given or at the winner read from device memory.
// No atomics: the scores are deterministic.  Every index below is bounded by an argument check or a table entry the host built.
#include <cstring>

#include "pseg_list.h"
#include "pseg_skew.h"

namespace pseg {

constexpr int SK_NTH = 256;                                            // threads of the strip, score and rotate workgroups
constexpr int SK_RUN = 8, SK_RUNS = 32, SK_TH = SK_NTH / SK_RUNS;      // rotation: pixels per run, runs and rows per workgroup
static_assert(SK_RUN == 8, "a full run is one uint2 store");
static_assert(SK_STRIP == 32, "a strip's count fits a byte and two 16-byte loads cover it");

// one map of a group; every pointer is a device pointer
struct SkMap {
    const uint8_t* ink;                 // what the strips count: an ink map (non-zero = ink) or a gray scan (from_gray)
    const uint8_t* src;                 // what the rotation reads
    uint8_t* out;                       // the rotated map, 8-byte aligned
    uint8_t* R;                         // H x K strip counts
    unsigned long long* scores;         // 2 A + 1
    const int* cs;                      // the (C, S) pair of index 0; the pairs of -A .. A lie around it
    int* winner;                        // the estimate's index
    int H, W, K, A, D, M;
    int from_gray, order, fill, use_winner;
    int sblk0, rblk0, tiles_x, pad;     // workgroups of the group's maps in front of this one: strips, rotation; rotation workgroups per band
};

template <bool ROT>
__device__ __forceinline__ int sk_map_of(const SkMap* __restrict__ tab, int n, int b) {
    int lo = 0, hi = n - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {                       // largest i whose prefix is <= b
        const int mid = (lo + hi + 1) >> 1;
        if ((ROT ? tab[mid].rblk0 : tab[mid].sblk0) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ink bytes of a word: non-zero bytes, or bytes <= 127 (high bit clear)
__device__ __forceinline__ int sk_count4(uint32_t w, bool from_gray) {
    const uint32_t hi = 0x80808080u;
    return __popc(from_gray ? (~w & hi) : ((((w & ~hi) + ~hi) | w) & hi));
}

__global__ __launch_bounds__(SK_NTH) void sk_strips_kernel(const SkMap* __restrict__ tab, int n) {
    const int i = sk_map_of<false>(tab, n, (int)blockIdx.x);
    const SkMap& m = tab[i];
    const int H = m.H, W = m.W, K = m.K;
    const long long item = (long long)((int)blockIdx.x - m.sblk0) * SK_NTH + threadIdx.x;
    if (item >= (long long)H * K) return;
    const int y = (int)(item / K), k = (int)(item - (long long)y * K);
    const bool fg = m.from_gray != 0;
    const size_t o = (size_t)y * W + (size_t)k * SK_STRIP;             // the map starts at a multiple of 256 bytes
    const int cnt = min(SK_STRIP, W - k * SK_STRIP);
    const uint8_t* const p = m.ink + o;
    const int head = min(cnt, (int)((16u - (unsigned)(o & 15)) & 15u));
    int c = 0, s = 0;
    for (; c < head; ++c) s += sk_is_ink(p[c], fg);
    for (; c + 16 <= cnt; c += 16) {
        const uint4 v = *(const uint4*)(p + c);
        s += sk_count4(v.x, fg) + sk_count4(v.y, fg) + sk_count4(v.z, fg) + sk_count4(v.w, fg);
    }
    for (; c < cnt; ++c) s += sk_is_ink(p[c], fg);
    m.R[item] = (uint8_t)s;
}

__device__ __forceinline__ unsigned long long sk_shfl_xor64(unsigned long long v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return (unsigned long long)hi << 32 | lo;
}

// grid (candidates of the group's widest map, maps)
__global__ __launch_bounds__(SK_NTH) void sk_score_kernel(const SkMap* __restrict__ tab) {
    __shared__ int s_off[SK_MAX_STRIPS];
    __shared__ unsigned long long s_part[SK_NTH / 64];
    const SkMap& m = tab[blockIdx.y];
    const int A = m.A;
    if ((int)blockIdx.x > 2 * A) return;
    const int a = (int)blockIdx.x - A, H = m.H, K = m.K, M = m.M;
    for (int k = threadIdx.x; k < K; k += SK_NTH) s_off[k] = sk_off(a, k, m.W, m.D);
    __syncthreads();
    const uint8_t* __restrict__ const R = m.R;
    unsigned long long acc = 0;
    for (int j = -M + (int)threadIdx.x; j <= H - 1 + M; j += SK_NTH) {
        unsigned p = 0;
        for (int k = 0; k < K; ++k) {
            const int y = j + s_off[k];
            if ((unsigned)y < (unsigned)H) p += R[(size_t)y * K + k];
        }
        acc += (unsigned long long)p * p;                              // p <= W <= 2^14
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += sk_shfl_xor64(acc, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < SK_NTH / 64; ++w) t += s_part[w];
        m.scores[blockIdx.x] = t;
    }
}

// one wave per map
__global__ __launch_bounds__(64) void sk_pick_kernel(const SkMap* __restrict__ tab) {
    const SkMap& m = tab[blockIdx.x];
    const int A = m.A;
    unsigned long long bs = 0;
    int ba = 0;                                                        // (score 0 at index 0 loses to nothing it should win against)
    bool have = false;
    for (int c = threadIdx.x; c <= 2 * A; c += 64) {
        const unsigned long long s = m.scores[c];
        if (!have || sk_better(s, c - A, bs, ba)) { bs = s; ba = c - A; have = true; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long os = sk_shfl_xor64(bs, o);
        const int oa = __shfl_xor(ba, o), oh = __shfl_xor((int)have, o);
        if (oh && (!have || sk_better(os, oa, bs, ba))) { bs = os; ba = oa; have = true; }
    }
    if (threadIdx.x == 0) *m.winner = ba;
}

template <int ORDER>
__device__ __forceinline__ void sk_rotate_run(const SkMap& m, int C, int S, int r, int c0, int c1, bool whole) {
    uint8_t* const orow = m.out + (size_t)r * m.W;
    const unsigned fill = (unsigned)m.fill;
    if (whole) {                                                       // orow + c0 is 8-byte aligned
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int q = 0; q < SK_RUN; ++q) w[q >> 2] |= sk_sample<ORDER>(m.src, m.H, m.W, C, S, fill, r, c0 + q) << (8 * (q & 3));
        *(uint2*)(orow + c0) = make_uint2(w[0], w[1]);
    } else {
        for (int c = c0; c < c1; ++c) orow[c] = (uint8_t)sk_sample<ORDER>(m.src, m.H, m.W, C, S, fill, r, c);
    }
}

__global__ __launch_bounds__(SK_NTH) void sk_rotate_kernel(const SkMap* __restrict__ tab, int n) {
    const int i = sk_map_of<true>(tab, n, (int)blockIdx.x);
    const SkMap& m = tab[i];
    const int blk = (int)blockIdx.x - m.rblk0;
    const int by = blk / m.tiles_x, bx = blk - by * m.tiles_x;
    const int r = by * SK_TH + (int)threadIdx.x / SK_RUNS, j = bx * SK_RUNS + ((int)threadIdx.x & (SK_RUNS - 1));
    if (r >= m.H) return;
    int idx = 0;
    if (m.use_winner) idx = max(-m.A, min(m.A, *m.winner));            // (the pick kernel wrote it within -A .. A)
    const int C = m.cs[2 * idx], S = m.cs[2 * idx + 1];
    const size_t row0 = (size_t)r * m.W;
    const int head = min(m.W, (int)((8u - (unsigned)(row0 & 7)) & 7u));  // pixels in front of the row's first 8-byte boundary
    const int c0 = j == 0 ? 0 : head + (j - 1) * SK_RUN;
    const int c1 = j == 0 ? head : min(m.W, c0 + SK_RUN);
    if (c0 >= c1) return;
    const bool whole = j > 0 && c1 - c0 == SK_RUN;
    if (m.order == 0) sk_rotate_run<0>(m, C, S, r, c0, c1, whole);
    else sk_rotate_run<1>(m, C, S, r, c0, c1, whole);
}

// ---- workspace: grow-only, one per device (tables, scores, winners, the group's maps, strip counts and outputs; a page-locked copy
// of the tables and the read-back slots), under its own lock and on its own stream.  pseg_release_workspace frees it.
struct SkWs {
    GrowDev dev; GrowPin pin; hipStream_t st = nullptr;
    void release() {
        dev.release();
        pin.release();
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
};
static PerDevice<SkWs> g_sk;


// what a list call does: the estimate (ink, how), the rotation (src, rot), or both with the rotation at the winner (order 1, fill 255)
struct SkCall {
    bool estimate, rotate;
    const uint8_t* const* src;          // what is rotated (and, for both, counted as src <= 127 where ink[i] is NULL)
    const uint8_t* const* ink;          // what is counted; for both: NULL, or NULL entries
    const int* H; const int* W;
    const pseg_skew* how;
    const pseg_rotate* rot;
    uint8_t* const* out;
    int32_t* out_index;
    uint64_t* const* out_scores;
};
static inline const uint8_t* sk_ink_of(const SkCall& c, int i) { return c.ink ? c.ink[i] : nullptr; }
static inline int sk_rot_tiles_x(int W) { return cdiv(cdiv(W, SK_RUN) + 1, SK_RUNS); }

static int sk_group(SkWs& ws, int g0, int g1, const SkCall& c) {
    const int n = g1 - g0;
    constexpr int NC = 2 * SK_MAX_STEPS + 1;
    constexpr size_t tab_b = up256((size_t)LIST_GROUP_ITEMS * sizeof(SkMap));
    constexpr size_t cs_b = up256((size_t)LIST_GROUP_ITEMS * NC * 2 * sizeof(int));
    constexpr size_t win_b = up256((size_t)LIST_GROUP_ITEMS * sizeof(int));
    constexpr size_t sc_b = up256((size_t)LIST_GROUP_ITEMS * NC * sizeof(unsigned long long));
    constexpr size_t head_b = tab_b + cs_b + win_b + sc_b;
    PSEG_TRY(ws.pin.ensure(head_b, "skew tables"));
    SkMap* const h_tab = ws.pin.as<SkMap>();
    int* const h_cs = (int*)(ws.pin.p + tab_b);
    const int* const h_win = (const int*)(ws.pin.p + tab_b + cs_b);
    const unsigned long long* const h_sc = (const unsigned long long*)(ws.pin.p + tab_b + cs_b + win_b);
    std::memset(h_tab, 0, tab_b);
    std::vector<size_t> o_ink(n, 0), o_src(n, 0), o_out(n, 0), o_R(n, 0);
    Bump at{head_b};
    long long sblocks = 0, rblocks = 0;
    int cand_max = 0;
    for (int k = 0; k < n; ++k) {
        const int i = g0 + k;
        SkMap& m = h_tab[k];
        const size_t px = (size_t)c.H[i] * c.W[i];
        m.H = c.H[i]; m.W = c.W[i]; m.K = sk_strips(m.W);
        int* const cs = h_cs + (size_t)k * NC * 2;
        if (c.rotate) {
            m.rblk0 = (int)rblocks;
            m.tiles_x = sk_rot_tiles_x(m.W);
            rblocks += (long long)m.tiles_x * cdiv(m.H, SK_TH);
            o_src[k] = at.take(px);
            o_out[k] = at.take(px);
            if (!c.estimate) {
                m.order = c.rot[i].order; m.fill = c.rot[i].fill;
                sk_cs(c.rot[i].index, c.rot[i].denom, &cs[0], &cs[1]);
            }
        }
        if (c.estimate) {
            m.A = c.how[i].steps; m.D = c.how[i].denom; m.M = sk_apron(m.A, m.W, m.D);
            m.from_gray = c.rotate && !sk_ink_of(c, i);
            m.sblk0 = (int)sblocks;
            sblocks += cdiv(m.H * m.K, SK_NTH);                        // H K <= 16384 * 512
            cand_max = std::max(cand_max, 2 * m.A + 1);
            o_ink[k] = m.from_gray ? o_src[k] : at.take(px);           // a scan that is counted as it is lies once
            o_R[k] = at.take((size_t)m.H * m.K);
            if (c.rotate) {                                            // the winner's pair, whichever it will be
                m.use_winner = 1; m.order = 1; m.fill = 255;
                for (int a = -m.A; a <= m.A; ++a) sk_cs(a, m.D, &cs[2 * (a + m.A)], &cs[2 * (a + m.A) + 1]);
            }
        }
    }
    if (sblocks > 0x7fffffffLL || rblocks > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "maps %d..%d: too many workgroups for one launch", g0, g1 - 1);
    PSEG_TRY(ws.dev.ensure(at.off, "skew workspace"));
    if (!ws.st) PSEG_HIP(hipStreamCreateWithFlags(&ws.st, hipStreamNonBlocking));
    hipStream_t st = ws.st;
    uint8_t* const d = ws.dev.p;
    const SkMap* const d_tab = (const SkMap*)d;
    int* const d_cs = (int*)(d + tab_b);
    int* const d_win = (int*)(d + tab_b + cs_b);
    unsigned long long* const d_sc = (unsigned long long*)(d + tab_b + cs_b + win_b);
    for (int k = 0; k < n; ++k) {
        SkMap& m = h_tab[k];
        m.scores = d_sc + (size_t)k * NC;
        m.winner = d_win + k;
        m.cs = d_cs + (size_t)k * NC * 2 + (m.use_winner ? 2 * m.A : 0);
        if (c.estimate) { m.ink = d + o_ink[k]; m.R = d + o_R[k]; }
        if (c.rotate) { m.src = d + o_src[k]; m.out = d + o_out[k]; }
    }
    GroupDrain drain{st};
    PSEG_HIP(hipMemcpyAsync(d, h_tab, tab_b + (c.rotate ? cs_b : 0), hipMemcpyHostToDevice, st));
    for (int k = 0; k < n; ++k) {
        const int i = g0 + k;
        const size_t px = (size_t)h_tab[k].H * h_tab[k].W;
        if (c.rotate) PSEG_HIP(hipMemcpyAsync(d + o_src[k], c.src[i], px, hipMemcpyHostToDevice, st));
        if (c.estimate && !h_tab[k].from_gray) PSEG_HIP(hipMemcpyAsync(d + o_ink[k], c.ink[i], px, hipMemcpyHostToDevice, st));
    }
    if (c.estimate) {
        sk_strips_kernel<<<(unsigned)sblocks, SK_NTH, 0, st>>>(d_tab, n);
        sk_score_kernel<<<dim3((unsigned)cand_max, (unsigned)n), SK_NTH, 0, st>>>(d_tab);
        sk_pick_kernel<<<(unsigned)n, 64, 0, st>>>(d_tab);
    }
    if (c.rotate) sk_rotate_kernel<<<(unsigned)rblocks, SK_NTH, 0, st>>>(d_tab, n);
    PSEG_HIP(hipGetLastError());
    if (c.rotate)
        for (int k = 0; k < n; ++k)
            PSEG_HIP(hipMemcpyAsync(c.out[g0 + k], d + o_out[k], (size_t)h_tab[k].H * h_tab[k].W, hipMemcpyDeviceToHost, st));
    bool want_scores = false;
    for (int k = 0; k < n && c.out_scores; ++k) want_scores |= c.out_scores[g0 + k] != nullptr;
    if (c.estimate) {
        PSEG_HIP(hipMemcpyAsync((void*)h_win, d_win, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
        if (want_scores) PSEG_HIP(hipMemcpyAsync((void*)h_sc, d_sc, (size_t)n * NC * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    PSEG_HIP(hipStreamSynchronize(st));                                // the group's one wait
    drain.armed = false;
    for (int k = 0; k < n && c.estimate; ++k) {
        if (c.out_index) c.out_index[g0 + k] = h_win[k];
        if (c.out_scores && c.out_scores[g0 + k])
            for (int a = 0; a <= 2 * h_tab[k].A; ++a) c.out_scores[g0 + k][a] = (uint64_t)h_sc[(size_t)k * NC + a];
    }
    return PSEG_OK;
}

// ---- what the entries refuse, before any work ----
static int sk_check_shape(int i, int H, int W) {
    if (H < 1 || W < 1 || H > SK_MAX_SIDE || W > SK_MAX_SIDE) return fail(PSEG_EINVAL, "map %d: shape (%d,%d) outside 1..%d", i, H, W, SK_MAX_SIDE);
    return PSEG_OK;
}
static int sk_check_how(int i, const pseg_skew& s) {
    if (s.denom < SK_DENOM_MIN || s.denom > SK_DENOM_MAX) return fail(PSEG_EINVAL, "map %d: denom %d outside %d..%d", i, s.denom, SK_DENOM_MIN, SK_DENOM_MAX);
    if (s.steps < 1 || s.steps > SK_MAX_STEPS || 4 * s.steps > s.denom)
        return fail(PSEG_EINVAL, "map %d: steps %d outside 1..%d, or above denom / 4 (denom %d)", i, s.steps, SK_MAX_STEPS, s.denom);
    return PSEG_OK;
}
static int sk_check_skew(int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_skew* how, int32_t* out_index) {
    if (n < 0 || !ink || !H || !W || !how || !out_index) return fail(PSEG_EINVAL, n < 0 ? "negative map count" : "NULL argument");
    for (int i = 0; i < n; ++i) {
        if (!ink[i]) return fail(PSEG_EINVAL, "map %d: NULL argument", i);
        PSEG_TRY(sk_check_shape(i, H[i], W[i]));
        PSEG_TRY(sk_check_how(i, how[i]));
    }
    return PSEG_OK;
}
static int sk_check_rotate(int n, const uint8_t* const* src, const int* H, const int* W, const pseg_rotate* rot, uint8_t* const* out) {
    if (n < 0 || !src || !H || !W || !rot || !out) return fail(PSEG_EINVAL, n < 0 ? "negative map count" : "NULL argument");
    for (int i = 0; i < n; ++i) {
        if (!src[i] || !out[i]) return fail(PSEG_EINVAL, "map %d: NULL argument", i);
        if (src[i] == out[i]) return fail(PSEG_EINVAL, "map %d: a rotation cannot work in place", i);
        PSEG_TRY(sk_check_shape(i, H[i], W[i]));
        const pseg_rotate& r = rot[i];
        if (r.denom < SK_DENOM_MIN || r.denom > SK_DENOM_MAX) return fail(PSEG_EINVAL, "map %d: denom %d outside %d..%d", i, r.denom, SK_DENOM_MIN, SK_DENOM_MAX);
        if (r.index < -SK_DENOM_MAX || r.index > SK_DENOM_MAX || 4 * sk_abs(r.index) > r.denom)
            return fail(PSEG_EINVAL, "map %d: index %d above denom / 4 (denom %d)", i, r.index, r.denom);
        if (r.order != 0 && r.order != 1) return fail(PSEG_EINVAL, "map %d: order %d (0 or 1)", i, r.order);
        if (r.fill < 0 || r.fill > 255) return fail(PSEG_EINVAL, "map %d: fill %d outside 0..255", i, r.fill);
    }
    return PSEG_OK;
}
static int sk_check_deskew(int n, const uint8_t* const* gray, const int* H, const int* W, const pseg_skew* how, uint8_t* const* out_gray,
                           int32_t* out_index) {
    if (n < 0 || !gray || !H || !W || !how || !out_gray || !out_index) return fail(PSEG_EINVAL, n < 0 ? "negative map count" : "NULL argument");
    for (int i = 0; i < n; ++i) {
        if (!gray[i] || !out_gray[i]) return fail(PSEG_EINVAL, "map %d: NULL argument", i);
        if (gray[i] == out_gray[i]) return fail(PSEG_EINVAL, "map %d: a rotation cannot work in place", i);
        PSEG_TRY(sk_check_shape(i, H[i], W[i]));
        PSEG_TRY(sk_check_how(i, how[i]));
    }
    return PSEG_OK;
}

// ---- the host twins: the same functions in plain loops ----
static int sk_host_skew(const uint8_t* ink, bool from_gray, int H, int W, const pseg_skew& how, uint64_t* scores) {
    const int K = sk_strips(W), A = how.steps, D = how.denom, M = sk_apron(A, W, D);
    std::vector<uint8_t> R((size_t)H * K);
    for (int y = 0; y < H; ++y)
        for (int k = 0; k < K; ++k) {
            int s = 0;
            for (int x = k * SK_STRIP; x < std::min(W, (k + 1) * SK_STRIP); ++x) s += sk_is_ink(ink[(size_t)y * W + x], from_gray);
            R[(size_t)y * K + k] = (uint8_t)s;
        }
    std::vector<unsigned> P((size_t)H + 2 * M);
    unsigned long long bs = 0;
    int ba = 0;
    for (int a = -A; a <= A; ++a) {
        std::fill(P.begin(), P.end(), 0u);
        for (int k = 0; k < K; ++k) {
            const int off = sk_off(a, k, W, D);                        // R[y][k] lands in P[y - off], |off| <= M
            for (int y = 0; y < H; ++y) P[(size_t)(y - off + M)] += R[(size_t)y * K + k];
        }
        unsigned long long s = 0;
        for (unsigned p : P) s += (unsigned long long)p * p;
        if (scores) scores[a + A] = s;
        if (a == -A || sk_better(s, a, bs, ba)) { bs = s; ba = a; }
    }
    return ba;
}
static void sk_host_rotate(const uint8_t* src, int H, int W, int index, int denom, int order, int fill, uint8_t* out) {
    int C, S;
    sk_cs(index, denom, &C, &S);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            out[(size_t)y * W + x] = (uint8_t)(order == 0 ? sk_sample<0>(src, H, W, C, S, (unsigned)fill, y, x)
                                                          : sk_sample<1>(src, H, W, C, S, (unsigned)fill, y, x));
}

static size_t sk_bytes(const int* H, const int* W, int i) { return (size_t)H[i] * W[i]; }

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_skew_maps(int device, int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_skew* how, int32_t* out_index,
                   uint64_t* const* out_scores) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(sk_check_skew(n, ink, H, W, how, out_index));
    const SkCall c{true, false, nullptr, ink, H, W, how, nullptr, nullptr, out_index, out_scores};
    return run_list(g_sk, device, n, [&](int i) { return sk_bytes(H, W, i); }, [&](SkWs& ws, int g0, int g1) { return sk_group(ws, g0, g1, c); });
}

int pseg_skew_maps_host(int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_skew* how, int32_t* out_index,
                        uint64_t* const* out_scores) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(sk_check_skew(n, ink, H, W, how, out_index));
    for (int i = 0; i < n; ++i) out_index[i] = sk_host_skew(ink[i], false, H[i], W[i], how[i], out_scores ? out_scores[i] : nullptr);
    return PSEG_OK;
}

int pseg_rotate_maps(int device, int n, const uint8_t* const* src, const int* H, const int* W, const pseg_rotate* rot, uint8_t* const* out) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(sk_check_rotate(n, src, H, W, rot, out));
    const SkCall c{false, true, src, nullptr, H, W, nullptr, rot, out, nullptr, nullptr};
    return run_list(g_sk, device, n, [&](int i) { return sk_bytes(H, W, i); }, [&](SkWs& ws, int g0, int g1) { return sk_group(ws, g0, g1, c); });
}

int pseg_rotate_maps_host(int n, const uint8_t* const* src, const int* H, const int* W, const pseg_rotate* rot, uint8_t* const* out) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(sk_check_rotate(n, src, H, W, rot, out));
    for (int i = 0; i < n; ++i) sk_host_rotate(src[i], H[i], W[i], rot[i].index, rot[i].denom, rot[i].order, rot[i].fill, out[i]);
    return PSEG_OK;
}

int pseg_deskew_scans(int device, int n, const uint8_t* const* gray, const uint8_t* const* ink, const int* H, const int* W, const pseg_skew* how,
                      uint8_t* const* out_gray, int32_t* out_index) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(sk_check_deskew(n, gray, H, W, how, out_gray, out_index));
    const SkCall c{true, true, gray, ink, H, W, how, nullptr, out_gray, out_index, nullptr};
    return run_list(g_sk, device, n, [&](int i) { return sk_bytes(H, W, i); }, [&](SkWs& ws, int g0, int g1) { return sk_group(ws, g0, g1, c); });
}

int pseg_deskew_scans_host(int n, const uint8_t* const* gray, const uint8_t* const* ink, const int* H, const int* W, const pseg_skew* how,
                           uint8_t* const* out_gray, int32_t* out_index) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(sk_check_deskew(n, gray, H, W, how, out_gray, out_index));
    for (int i = 0; i < n; ++i) {
        const uint8_t* const m = ink ? ink[i] : nullptr;
        out_index[i] = sk_host_skew(m ? m : gray[i], !m, H[i], W[i], how[i], nullptr);
        sk_host_rotate(gray[i], H[i], W[i], out_index[i], how[i].denom, 1, 255, out_gray[i]);
    }
    return PSEG_OK;
}

int pseg_skew_geometry(int* strip, int* max_steps, int* max_side) {
    if (strip) *strip = SK_STRIP;
    if (max_steps) *max_steps = SK_MAX_STEPS;
    if (max_side) *max_side = SK_MAX_SIDE;
    return PSEG_OK;
}

}  // extern "C"
