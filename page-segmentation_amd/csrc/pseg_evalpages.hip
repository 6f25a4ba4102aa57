// pseg_evalpages.hip -- a list of pages scored against ground truth in one device-resident call: per page the joint
// (ink, mask class, predicted class) histogram of pseg_eval_confusion, the number of ink components, and per rule the summed verdicts
// of ConnectedComponentEval.run_per_component(cc_matching(...) / cc_equal(...)) with or without only_label (lib/evaluation.py:52-117).
//
// The component part is the vote's tile path (pseg_post.hip) with judged components in place of applied winners: a
// workgroup labels the runs of a 32 x 64 tile in LDS; a component with no ink neighbour across the tile's edge is CLOSED and is judged
// against every rule on the spot; an OPEN one takes one of the tile's 192 root slots (parent + a row of counters), and three small
// launches join the slots across tile edges, add the counters of redirected slots to their final root, and judge the final roots.
// The sums are order-free, so no component numbering, no label image, no sort and no component list exist: beyond the three maps the
// workspace is a fixed number of bytes per tile.  The rules name at most 16 distinct WATCHED labels; a component carries its size, its
// pixels with pred == mask, and per watched label its pixels of that label in pred and in mask -- not a class histogram.
//
// Every loop bound below is an argument, a constant or a table entry the host built; every find / unite loop is bounded (parents only
// ever decrease, so a chain is shorter than the index space, and the larger root of a union strictly decreases from try to try).
#include <algorithm>
#include <cstring>
#include <vector>

#include "pseg_list.h"

namespace pseg {

constexpr int EP_TH = 32, EP_TW = 64;
constexpr int EP_OPEN_MAX = 2 * (EP_TH + EP_TW);   // an open root owns at least one pixel of the tile's rim (188 pixels)
constexpr int EP_RUN_MAX = EP_TH * EP_TW / 2;      // runs of a tile: at most every other pixel starts one
constexpr int EP_HALF = EP_RUN_MAX / 2;            // 16-bit counters, two runs to a word (a tile has 2 048 pixels: no carry crosses)
// rim table of a tile: slot of the root of the pixel at [0, 64) top row, [64, 128) bottom row, [128, 160) left column, [160, 192) right column
constexpr int EP_RIM = 2 * (EP_TH + EP_TW);
// border unions a tile lists: <= 64 starts of ink above the (widened) spans of its top row, <= 96 pixel pairs across its left edge, 2 corners
constexpr int EP_TASK_MAX = 192;
constexpr int EP_RULES = 8, EP_WATCH = 2 * EP_RULES;
constexpr int EP_VER = EP_RULES * 4 + 1;           // a page's verdict counters, then its component count
constexpr int EP_HIST_BLOCKS = 256;                // histogram workgroups of one page, at most

// li / fi: place of the rule's label / filter label among the watched labels, -1: none (cc_equal has no label; filter label 0 is no filter)
struct EpRule { int kind, li, fi, pad; double t_tp, t_fp, t_mask, t_filter; };
struct EpRules { int n_rules, n_watch; int watch[EP_WATCH]; EpRule r[EP_RULES]; };
// one page of a group: the prefix tables of the ragged launches (tile0: tile workgroups, blk0: histogram workgroups in front of it)
struct EpPage {
    int H, W, tiles_x, tile0, blk0, nblk, has_bin, pad;
    unsigned long long pred, mask, bin;            // the maps' bytes in the group's buffer, 256-byte aligned
};

template <int EpPage::*FIRST>
__device__ __forceinline__ int ep_page_of(const EpPage* __restrict__ tab, int n, int b) {
    int lo = 0, hi = n - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {   // largest i with tab[i].*FIRST <= b (pages without workgroups share their successor's entry)
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].*FIRST <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- joint histogram: counts[b][m][p] of pseg_eval_confusion, into the page's record -------------------------------------------
__device__ __forceinline__ void ep_bump(unsigned* h, unsigned long long* out, int use_lds, int key, unsigned c) {
    if (use_lds) atomicAdd(&h[key], c);
    else atomicAdd(&out[key], (unsigned long long)c);
}
__global__ __launch_bounds__(256) void ep_hist_kernel(const uint8_t* __restrict__ buf, const EpPage* __restrict__ tab, int n, int ncls,
                                                      int use_lds, unsigned long long* __restrict__ rec, int rec_words) {
    extern __shared__ unsigned eph[];
    const int K = ncls + 1, slots = 2 * K * K;
    const int i = ep_page_of<&EpPage::blk0>(tab, n, (int)blockIdx.x);
    const EpPage pg = tab[i];
    const int b = (int)blockIdx.x - pg.blk0;
    if (use_lds) {
        for (int k = threadIdx.x; k < slots; k += 256) eph[k] = 0;
        __syncthreads();
    }
    unsigned long long* const out = rec + (size_t)i * rec_words;
    const uint8_t* const P = buf + pg.pred;
    const uint8_t* const M = buf + pg.mask;
    const uint8_t* const B = pg.has_bin ? buf + pg.bin : nullptr;
    const size_t nbytes = (size_t)pg.H * pg.W, n16 = nbytes >> 4;
    for (size_t q = (size_t)b * 256 + threadIdx.x; q < n16; q += (size_t)pg.nblk * 256) {
        const uint4 vp = ((const uint4*)P)[q], vm = ((const uint4*)M)[q];
        const uint4 vb = B ? ((const uint4*)B)[q] : make_uint4(~0u, ~0u, ~0u, ~0u);
        const unsigned wp[4] = {vp.x, vp.y, vp.z, vp.w}, wm[4] = {vm.x, vm.y, vm.z, vm.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
        int prev = 0;
        unsigned cnt = 0;                                              // equal neighbours share one add (paper, text blocks)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int sh = (k & 3) * 8;
            const int p = min((int)((wp[k >> 2] >> sh) & 255u), ncls), m = min((int)((wm[k >> 2] >> sh) & 255u), ncls);
            const int key = ((((wb[k >> 2] >> sh) & 255u) ? K : 0) + m) * K + p;
            if (cnt && key == prev) ++cnt;
            else { if (cnt) ep_bump(eph, out, use_lds, prev, cnt); prev = key; cnt = 1; }
        }
        ep_bump(eph, out, use_lds, prev, cnt);
    }
    if (b == 0)
        for (size_t q = (n16 << 4) + threadIdx.x; q < nbytes; q += 256) {
            const int p = min((int)P[q], ncls), m = min((int)M[q], ncls);
            ep_bump(eph, out, use_lds, (((B ? B[q] != 0 : true) ? K : 0) + m) * K + p, 1u);
        }
    if (use_lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < slots; k += 256)
            if (eph[k]) atomicAdd(&out[k], (unsigned long long)eph[k]);
    }
}

// ---- the verdict of one component ------------------------------------------------------------------------------------------------
// s pixels, e of them with pred == mask, pl / ml with pred / mask == the rule's label, pf / mf with pred / mask == its filter label.
// The quotients are IEEE double divisions of two integers below 2^31 and the comparisons double comparisons (-ffp-contract=off):
// the bits Python's int / int >= float has.  false: the rule's only_label filter drops the component.
__device__ __forceinline__ bool ep_judge(const EpRule& R, unsigned s, unsigned e, unsigned pl, unsigned ml, unsigned pf, unsigned mf, unsigned v[3]) {
    const double ds = (double)s;
    if (R.fi >= 0 && !((double)mf / ds >= R.t_filter || pf > 0)) return false;
    if (R.kind == 0) {
        const double qp = (double)pl / ds, qm = (double)ml / ds;
        const bool ptp = qp >= R.t_tp, pfp = qp >= R.t_fp, mm = qm >= R.t_mask;
        v[0] = ptp && mm; v[1] = pfp && !mm; v[2] = mm && !ptp;
    } else {
        const bool ok = (double)e / ds >= R.t_tp;
        v[0] = ok; v[1] = !ok; v[2] = 0;
    }
    return true;
}

// ---- union-find: LDS (run indices of a tile) and global (root slot ids of a group) -----------------------------------------------
// Links only ever point at a smaller index of the same component, so a chain has fewer hops than the index space: `cap`.
__device__ __forceinline__ int ep_lds_find(const int* lab, int x) {
    for (int it = 0; it < EP_RUN_MAX; ++it) {
        const int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) break;
        x = p;
    }
    return x;
}
// a lost atomicMin hands back a link below the larger root: max(a, b) strictly decreases, EP_RUN_MAX tries at the very most
__device__ __forceinline__ void ep_lds_union(int* lab, int a, int b) {
    for (int it = 0; it < EP_RUN_MAX; ++it) {
        a = ep_lds_find(lab, a);
        b = ep_lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}
// path halving as uf_find_halve (pseg_post.hip): a halving store replaces a non-root's link by one further up its own chain
__device__ __forceinline__ int ep_find(int* L, int x, int cap) {
    for (int it = 0; it < cap; ++it) {
        const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        const int g = __hip_atomic_load(&L[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g == p) return p;
        __hip_atomic_store(&L[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
    return x;
}
__device__ __forceinline__ void ep_union(int* L, int a, int b, int cap) {
    for (int it = 0; it < cap; ++it) {
        a = ep_find(L, a, cap);
        b = ep_find(L, b, cap);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ unsigned long long ep_le(int b) { return b >= 63 ? ~0ull : ((2ull << b) - 1ull); }   // bits 0 .. b
// the columns a run [s0, e] touches in the row above / below: itself, for connectivity 8 one more to either side
template <bool C8>
__device__ __forceinline__ unsigned long long ep_reach(unsigned long long S) { return C8 ? (S | (S << 1) | (S >> 1)) : S; }
// the rows of the column beside the tile that pixel (r, edge column) touches
template <bool C8>
__device__ __forceinline__ unsigned ep_reach_rows(int r) { const unsigned b = 1u << r; return C8 ? (b | (b << 1) | (b >> 1)) : b; }

// One workgroup per (page, 32 x 64 tile).  The three maps are read once and become bit rows: ink, pred == mask, and per watched label
// pred == label and mask == label (all under ink).  A tile is then its run list (vote_tile_kernel's: row | first lane << 5 | last
// lane << 11, ordered by row and column); runs are joined with the runs of the row above that they touch, every counter of a
// component is a sum over its runs of popcount(bit row & run span).  The label counters are taken rule by rule (four 2 KiB rows of
// 16-bit counters, not 2 + 2 * 16 of them): a closed root is judged in that pass, an open root stores its row entries (plain stores).
template <bool C8>
__global__ __launch_bounds__(256) void ep_tile_kernel(const uint8_t* __restrict__ buf, const EpRules* __restrict__ rules, const EpPage* __restrict__ tab,
                                                      int n_pages, int* __restrict__ P, unsigned* __restrict__ cnt_g, int cw,
                                                      uint8_t* __restrict__ rimtab, unsigned* __restrict__ tasks, int* __restrict__ rootn,
                                                      int* __restrict__ taskn, unsigned long long* __restrict__ rec, int rec_words, int ver0) {
    constexpr int NTH = 256, RPW = EP_TH / 4;
    __shared__ unsigned long long ink[EP_TH + 2];                      // ink of tile rows -1 .. EP_TH
    __shared__ unsigned long long eqm[EP_TH];                          // pred == mask
    __shared__ unsigned long long pm[EP_WATCH][EP_TH], mm[EP_WATCH][EP_TH];
    __shared__ unsigned lr[2], cor[2];                                 // ink left / right of the tile (bit = row); beside the row above / below: bit 0 left, 1 right
    __shared__ int rowcnt[EP_TH], rowbase[EP_TH + 1];
    __shared__ unsigned rl[EP_RUN_MAX];                                // the runs (| an open root's slot << 17)
    __shared__ int parent[EP_RUN_MAX];
    __shared__ unsigned cse[2 * EP_HALF];                              // size, pred == mask
    __shared__ unsigned cl[4 * EP_HALF];                               // of the rule at hand: pred / mask == label, pred / mask == filter label
    __shared__ unsigned openbits[EP_RUN_MAX / 32];
    __shared__ unsigned ver[EP_VER];
    __shared__ int nopen, ntask;
    const int tile = blockIdx.x;
    const int pi = ep_page_of<&EpPage::tile0>(tab, n_pages, tile);
    const EpPage pg = tab[pi];
    const int H = pg.H, W = pg.W;
    const int lt = tile - pg.tile0, ty = lt / pg.tiles_x, tx = lt - ty * pg.tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y0 = ty * EP_TH, x0 = tx * EP_TW, x = x0 + lane;
    const int rw0 = wave * RPW;
    const uint8_t* const bin = buf + pg.bin;
    const uint8_t* const pred = buf + pg.pred;
    const uint8_t* const mask = buf + pg.mask;
    const int nw = min(rules->n_watch, EP_WATCH), nr = min(rules->n_rules, EP_RULES);
    for (int i = threadIdx.x; i < 2 * EP_HALF; i += NTH) cse[i] = 0;
    if (threadIdx.x < EP_RUN_MAX / 32) openbits[threadIdx.x] = 0;
    if (threadIdx.x < EP_VER) ver[threadIdx.x] = 0;
    if (threadIdx.x == 0) { nopen = 0; ntask = 0; }
    // ---- the maps -> bit rows; waves 0, 1 also fetch the row above / below the tile (and the two pixels beside it), waves 2, 3 the columns beside it
    unsigned long long mr[RPW];
    int nruns_w = 0;
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int r = rw0 + j, y = y0 + r;
        const bool in = y < H && x < W;
        const size_t o = (size_t)y * W + x;
        const unsigned b = in ? bin[o] : 0u, p = in ? pred[o] : 0u, m = in ? mask[o] : 0u;
        const bool fg = b != 0;
        const unsigned long long mi = __ballot(fg);
        const unsigned long long me = __ballot(fg && p == m);
        mr[j] = mi;
        const int n = __popcll(mi & ~(mi << 1));
        nruns_w += n;
        if (lane == 0) { ink[r + 1] = mi; rowcnt[r] = n; eqm[r] = me; }
        if (mi) {                                                      // (uniform)
            for (int w = 0; w < nw; ++w) {
                const unsigned lab = (unsigned)rules->watch[w];
                const unsigned long long a = __ballot(fg && p == lab), c = __ballot(fg && m == lab);
                if (lane == 0) { pm[w][r] = a; mm[w][r] = c; }
            }
        }
    }
    {
        bool hv = false, hc = false;
        if (wave < 2) {
            const int y = wave == 0 ? y0 - 1 : y0 + EP_TH;
            const bool row_ok = y >= 0 && y < H;
            hv = row_ok && x < W && bin[(size_t)y * W + x] != 0;
            if (C8 && lane < 2) {
                const int xx = lane == 0 ? x0 - 1 : x0 + EP_TW;
                hc = row_ok && xx >= 0 && xx < W && bin[(size_t)y * W + xx] != 0;
            }
        } else {
            const int y = y0 + (lane & 31), xx = wave == 2 ? x0 - 1 : x0 + EP_TW;
            hv = lane < 32 && y < H && xx >= 0 && xx < W && bin[(size_t)y * W + xx] != 0;
        }
        const unsigned long long bv = __ballot(hv), bc = __ballot(hc);
        if (lane == 0) {
            if (wave == 0) { ink[0] = bv; cor[0] = (unsigned)bc & 3u; }
            else if (wave == 1) { ink[EP_TH + 1] = bv; cor[1] = (unsigned)bc & 3u; }
            else lr[wave - 2] = (unsigned)bv;
        }
    }
    if (!__syncthreads_or(nruns_w)) {                                  // a tile of paper
        if (threadIdx.x == 0) { rootn[tile] = 0; taskn[tile] = 0; }
        return;
    }
    // ---- the run list, every run its own parent ----
    int excl, n_all;
    {
        const int v = lane < EP_TH ? rowcnt[lane] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < EP_TH; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        excl = inc - v;
        n_all = min(__shfl(inc, EP_TH - 1), EP_RUN_MAX);
        if (wave == 0 && lane <= EP_TH) rowbase[lane] = lane < EP_TH ? excl : n_all;
    }
    const unsigned long long le = ep_le(lane);
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int r = rw0 + j;
        const unsigned long long m = mr[j];
        const int base = __shfl(excl, r);
        if (m == 0) continue;
        const unsigned long long fm = m & ~(m << 1);
        if ((fm >> lane) & 1) {
            const unsigned long long brk = ~(m & (m << 1));            // lanes that do not continue the lane to their left
            const unsigned long long above = brk & ~le;
            const int e = above ? __builtin_ctzll(above) - 1 : 63;
            const int idx = base + __popcll(fm & (le >> 1));
            rl[idx] = (unsigned)(r | lane << 5 | e << 11);
            parent[idx] = idx;
        }
    }
    __syncthreads();
    // ---- unions with the runs of the row above that this run touches (at most 33 of them) ----
    for (int t = threadIdx.x; t < n_all; t += NTH) {
        const unsigned rc = rl[t];
        const int r = rc & 31, s0 = (rc >> 5) & 63, e = (rc >> 11) & 63;
        if (r == 0) continue;
        const unsigned long long mp = ink[r];                          // (row r - 1)
        unsigned long long ov = ep_reach<C8>(ep_le(e) & ~(ep_le(s0) >> 1)) & mp;
        const unsigned long long fmp = mp & ~(mp << 1);
        const int base = rowbase[r - 1];
        for (int it = 0; it < EP_TW / 2 + 1 && ov; ++it) {
            const int b = __builtin_ctzll(ov);
            const int u = base + __popcll(fmp & ep_le(b)) - 1;
            ep_lds_union(parent, t, u);
            ov &= ~ep_le((rl[u] >> 11) & 63);
        }
    }
    __syncthreads();
    // ---- roots, size and pred == mask, open components ----
    const unsigned long long m_up = ink[0], m_dn = ink[EP_TH + 1];
    const unsigned lr0 = lr[0], lr1 = lr[1], cup = cor[0], cdn = cor[1];
    for (int t = threadIdx.x; t < n_all; t += NTH) {
        const unsigned rc = rl[t];
        const int r = rc & 31, s0 = (rc >> 5) & 63, e = (rc >> 11) & 63;
        const unsigned long long S = ep_le(e) & ~(ep_le(s0) >> 1), Sx = ep_reach<C8>(S);
        const int rt = ep_lds_find(parent, t);
        if (rt != t) __hip_atomic_store(&parent[t], rt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (the unions are over: later phases read the root here)
        const int sh = (rt & 1) * 16;
        __hip_atomic_fetch_add(&cse[rt >> 1], (unsigned)(e - s0 + 1) << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const unsigned ne = (unsigned)__popcll(eqm[r] & S);
        if (ne) __hip_atomic_fetch_add(&cse[EP_HALF + (rt >> 1)], ne << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        bool rim = false;
        if (r == 0) rim |= (Sx & m_up) != 0 || (C8 && ((s0 == 0 && (cup & 1u)) || (e == EP_TW - 1 && (cup & 2u))));
        if (r == EP_TH - 1) rim |= (Sx & m_dn) != 0 || (C8 && ((s0 == 0 && (cdn & 1u)) || (e == EP_TW - 1 && (cdn & 2u))));
        if (s0 == 0) rim |= (lr0 & ep_reach_rows<C8>(r)) != 0;
        if (e == EP_TW - 1) rim |= (lr1 & ep_reach_rows<C8>(r)) != 0;
        if (rim) atomicOr(&openbits[rt >> 5], 1u << (rt & 31));
    }
    __syncthreads();
    // ---- closed roots: counted; open roots: a slot, its parent, size and pred == mask ----
    for (int t0 = 0; t0 < n_all; t0 += NTH) {
        const int t = t0 + threadIdx.x;
        bool open_root = false, closed_root = false;
        if (t < n_all && parent[t] == t) {
            open_root = (openbits[t >> 5] >> (t & 31)) & 1;
            closed_root = !open_root;
        }
        const unsigned long long orm = __ballot(open_root), crm = __ballot(closed_root);
        if (crm && lane == 0) atomicAdd(&ver[EP_VER - 1], (unsigned)__popcll(crm));
        if (orm) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&nopen, __popcll(orm));
            base = __shfl(base, 0);
            if (open_root) {
                const int k = min(base + __popcll(orm & (le >> 1)), EP_OPEN_MAX - 1);   // (the slot bound holds: DESIGN.md 5h)
                const int id = tile * EP_OPEN_MAX + k, sh = (t & 1) * 16;
                rl[t] |= (unsigned)k << 17;
                P[id] = id;
                cnt_g[(size_t)id * cw] = (cse[t >> 1] >> sh) & 0xffffu;
                cnt_g[(size_t)id * cw + 1] = (cse[EP_HALF + (t >> 1)] >> sh) & 0xffffu;
            }
        }
    }
    // ---- rule by rule: the label counters of every root; closed roots judged, open roots' row entries stored ----
    for (int ri = 0; ri < nr; ++ri) {
        const EpRule R = rules->r[ri];
        __syncthreads();
        for (int i = threadIdx.x; i < 4 * EP_HALF; i += NTH) cl[i] = 0;
        __syncthreads();
        for (int t = threadIdx.x; t < n_all; t += NTH) {
            const unsigned rc = rl[t];
            const int r = rc & 31, s0 = (rc >> 5) & 63, e = (rc >> 11) & 63;
            const unsigned long long S = ep_le(e) & ~(ep_le(s0) >> 1);
            const int rt = parent[t], sh = (rt & 1) * 16;
            if (R.li >= 0) {
                const unsigned a = (unsigned)__popcll(pm[R.li][r] & S), c = (unsigned)__popcll(mm[R.li][r] & S);
                if (a) __hip_atomic_fetch_add(&cl[rt >> 1], a << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (c) __hip_atomic_fetch_add(&cl[EP_HALF + (rt >> 1)], c << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (R.fi >= 0) {
                const unsigned a = (unsigned)__popcll(pm[R.fi][r] & S), c = (unsigned)__popcll(mm[R.fi][r] & S);
                if (a) __hip_atomic_fetch_add(&cl[2 * EP_HALF + (rt >> 1)], a << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (c) __hip_atomic_fetch_add(&cl[3 * EP_HALF + (rt >> 1)], c << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < n_all; t += NTH) {
            if (parent[t] != t) continue;
            const int sh = (t & 1) * 16, h = t >> 1;
            const unsigned s = (cse[h] >> sh) & 0xffffu, e = (cse[EP_HALF + h] >> sh) & 0xffffu;
            const unsigned pl = (cl[h] >> sh) & 0xffffu, ml = (cl[EP_HALF + h] >> sh) & 0xffffu;
            const unsigned pf = (cl[2 * EP_HALF + h] >> sh) & 0xffffu, mf = (cl[3 * EP_HALF + h] >> sh) & 0xffffu;
            if ((openbits[t >> 5] >> (t & 31)) & 1) {
                unsigned* const row = cnt_g + (size_t)(tile * EP_OPEN_MAX + (int)(rl[t] >> 17)) * cw;
                if (R.li >= 0) { row[2 + 2 * R.li] = pl; row[3 + 2 * R.li] = ml; }
                if (R.fi >= 0) { row[2 + 2 * R.fi] = pf; row[3 + 2 * R.fi] = mf; }
            } else {
                unsigned v[3];
                if (ep_judge(R, s, e, pl, ml, pf, mf, v)) {
                    atomicAdd(&ver[ri * 4 + 3], 1u);
                    for (int k = 0; k < 3; ++k) if (v[k]) atomicAdd(&ver[ri * 4 + k], 1u);
                }
            }
        }
    }
    __syncthreads();
    // ---- open runs: the root's slot at their rim pixels, the unions across this tile's top and left edge ----
    // (the tiles below / right list theirs.)  slot | place in the neighbour's rim table << 8 | neighbour << 16: 0 above, 1 left,
    // 2 above left, 3 above right.  Ink that is adjacent in the neighbour's rim is one component there: one task per start of such a stretch.
    uint8_t* const rim = rimtab + (size_t)tile * EP_RIM;
    unsigned* const tk = tasks + (size_t)tile * EP_TASK_MAX;
    for (int t = threadIdx.x; t < n_all; t += NTH) {
        const int rt = parent[t];
        if (!((openbits[rt >> 5] >> (rt & 31)) & 1)) continue;
        const unsigned rc = rl[t];
        const unsigned k = rl[rt] >> 17;
        const int r = rc & 31, s0 = (rc >> 5) & 63, e = (rc >> 11) & 63;
        const unsigned long long S = ep_le(e) & ~(ep_le(s0) >> 1), Sx = ep_reach<C8>(S);
        if (r == 0) for (int b = s0; b <= e; ++b) rim[b] = (uint8_t)k;
        if (r == EP_TH - 1) for (int b = s0; b <= e; ++b) rim[EP_TW + b] = (uint8_t)k;
        if (s0 == 0) rim[2 * EP_TW + r] = (uint8_t)k;
        if (e == EP_TW - 1) rim[2 * EP_TW + EP_TH + r] = (uint8_t)k;
        if (r == 0) {
            const unsigned long long w = Sx & m_up;
            unsigned long long st = w & ~(w << 1);
            for (int it = 0; it < EP_TW / 2 + 1 && st; ++it) {
                const int i = atomicAdd(&ntask, 1);
                if (i < EP_TASK_MAX) tk[i] = k | (unsigned)(EP_TW + __builtin_ctzll(st)) << 8;
                st &= st - 1;
            }
            if (C8 && s0 == 0 && (cup & 1u)) {
                const int i = atomicAdd(&ntask, 1);
                if (i < EP_TASK_MAX) tk[i] = k | (unsigned)(EP_TW + EP_TW - 1) << 8 | 2u << 16;
            }
            if (C8 && e == EP_TW - 1 && (cup & 2u)) {
                const int i = atomicAdd(&ntask, 1);
                if (i < EP_TASK_MAX) tk[i] = k | (unsigned)EP_TW << 8 | 3u << 16;
            }
        }
        if (s0 == 0) {
            unsigned nb = lr0 & ep_reach_rows<C8>(r);
            for (int it = 0; it < 3 && nb; ++it) {
                const int i = atomicAdd(&ntask, 1);
                if (i < EP_TASK_MAX) tk[i] = k | (unsigned)(2 * EP_TW + EP_TH + __builtin_ctz(nb)) << 8 | 1u << 16;
                nb &= nb - 1;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) { rootn[tile] = min(nopen, EP_OPEN_MAX); taskn[tile] = min(ntask, EP_TASK_MAX); }
    if (threadIdx.x < EP_VER && ver[threadIdx.x])
        atomicAdd(&rec[(size_t)pi * rec_words + ver0 + threadIdx.x], (unsigned long long)ver[threadIdx.x]);
}

// unions of the open components across tile edges, on the root slot ids: a wave per tile takes the tile's task list and looks the
// neighbour's slot up in ITS rim table.  A slot the neighbour never handed out is skipped (cannot happen: the pixel looked up has an
// ink neighbour across its tile's edge, so its component is open there).
__global__ __launch_bounds__(256) void ep_border_kernel(const EpPage* __restrict__ tab, int n_pages, const uint8_t* __restrict__ rimtab,
                                                        const unsigned* __restrict__ tasks, const int* __restrict__ taskn,
                                                        const int* __restrict__ rootn, int* P, int tiles, int cap) {
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tiles) return;
    const int n = min(taskn[tile], EP_TASK_MAX);
    if (n == 0) return;
    const int tiles_x = tab[ep_page_of<&EpPage::tile0>(tab, n_pages, tile)].tiles_x;
    for (int i = lane; i < n; i += 64) {
        const unsigned t = tasks[(size_t)tile * EP_TASK_MAX + i];
        const int k = (int)(t & 255u), place = (int)((t >> 8) & 255u), dir = (int)(t >> 16);
        const int nb = tile - (dir == 1 ? 1 : dir == 0 ? tiles_x : dir == 2 ? tiles_x + 1 : tiles_x - 1);
        if (nb < 0 || nb >= tiles || place >= EP_RIM) continue;
        const int ks = rimtab[(size_t)nb * EP_RIM + place];
        if (k >= rootn[tile] || ks >= rootn[nb]) continue;
        ep_union(P, tile * EP_OPEN_MAX + k, nb * EP_OPEN_MAX + ks, cap);
    }
}

// counters of the root slots that a border union redirected: added to the final root's row, and the slot pointed straight at it.
// One wave per tile; the lanes that share their final root are summed first, one lane adds (vote_merge_kernel's scheme).
__global__ __launch_bounds__(256) void ep_merge_kernel(int* P, unsigned* cnt_g, int cw, const int* __restrict__ rootn, int tiles, int cap) {
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tiles) return;
    const int n = min(rootn[tile], EP_OPEN_MAX);
    for (int base = 0; base < n; base += 64) {
        int id = 0, r = -1;
        if (base + lane < n) {
            id = tile * EP_OPEN_MAX + base + lane;
            r = ep_find(P, id, cap);
            if (r == id) r = -1;
            else __hip_atomic_store(&P[id], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (int g = 0; g < 64; ++g) {                                 // group after group of the distinct roots among the lanes
            const unsigned long long act = __ballot(r >= 0);
            if (act == 0) break;
            const int r0 = __builtin_amdgcn_readlane(r, __builtin_ctzll(act));
            const bool mine = r == r0;
            for (int c = 0; c < cw; ++c) {
                unsigned sum = mine ? cnt_g[(size_t)id * cw + c] : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
                if (lane == 0 && sum) atomicAdd(&cnt_g[(size_t)r0 * cw + c], sum);
            }
            if (mine) r = -1;
        }
    }
}

// every slot that is still a root is one component: judged like a closed one, counted.  One wave per tile, sums in LDS first.
__global__ __launch_bounds__(256) void ep_judge_kernel(const EpRules* __restrict__ rules, const EpPage* __restrict__ tab, int n_pages,
                                                       const int* __restrict__ P, const unsigned* __restrict__ cnt_g, int cw,
                                                       const int* __restrict__ rootn, int tiles, unsigned long long* __restrict__ rec,
                                                       int rec_words, int ver0) {
    __shared__ unsigned ver[4][EP_VER];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + wave;
    for (int i = threadIdx.x; i < 4 * EP_VER; i += 256) (&ver[0][0])[i] = 0;
    __syncthreads();
    const int n = tile < tiles ? min(rootn[tile], EP_OPEN_MAX) : 0;
    const int nr = min(rules->n_rules, EP_RULES);
    for (int k = lane; k < n; k += 64) {
        const int id = tile * EP_OPEN_MAX + k;
        if (P[id] != id) continue;
        const unsigned* const row = cnt_g + (size_t)id * cw;
        const unsigned s = row[0], e = row[1];
        atomicAdd(&ver[wave][EP_VER - 1], 1u);
        for (int ri = 0; ri < nr; ++ri) {
            const EpRule R = rules->r[ri];
            const unsigned pl = R.li >= 0 ? row[2 + 2 * R.li] : 0u, ml = R.li >= 0 ? row[3 + 2 * R.li] : 0u;
            const unsigned pf = R.fi >= 0 ? row[2 + 2 * R.fi] : 0u, mf = R.fi >= 0 ? row[3 + 2 * R.fi] : 0u;
            unsigned v[3];
            if (ep_judge(R, s, e, pl, ml, pf, mf, v)) {
                atomicAdd(&ver[wave][ri * 4 + 3], 1u);
                for (int j = 0; j < 3; ++j) if (v[j]) atomicAdd(&ver[wave][ri * 4 + j], 1u);
            }
        }
    }
    __syncthreads();
    if (n > 0 && lane < EP_VER && ver[wave][lane]) {
        const int pi = ep_page_of<&EpPage::tile0>(tab, n_pages, tile);
        atomicAdd(&rec[(size_t)pi * rec_words + ver0 + lane], (unsigned long long)ver[wave][lane]);
    }
}

// ---- workspace: grow-only, one per device (table, records, the group's maps, the per-tile arrays; a page-locked copy of table and
// records), under its own lock and on its own stream; a call holds the lock to its end and every group ends synchronised.
// pseg_release_workspace frees it.
struct EpWs {
    GrowDev dev; GrowPin pin; hipStream_t st = nullptr;
    void release() {
        dev.release();
        pin.release();
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
};
static PerDevice<EpWs> g_ep;

struct EpOut { std::vector<int64_t> counts, comps, verdicts; };

static int ep_group(EpWs& ws, int g0, int g1, const pseg_eval_page* pages, int ncls, int conn, const EpRules& rules, EpOut& out) {
    const int n = g1 - g0, K = ncls + 1;
    const size_t slots = (size_t)2 * K * K;
    const int ver0 = (int)slots, rec_words = (int)slots + EP_VER, cw = 2 + 2 * rules.n_watch;
    const size_t tab_b = up256(sizeof(EpRules) + (size_t)LIST_GROUP_ITEMS * sizeof(EpPage)), rec_b = up256((size_t)n * rec_words * 8);
    PSEG_TRY(ws.pin.ensure(tab_b + rec_b, "page-score records"));
    std::memcpy(ws.pin.p, &rules, sizeof(EpRules));
    EpPage* const h_tab = (EpPage*)(ws.pin.p + sizeof(EpRules));
    Bump at{tab_b + rec_b};
    long long tiles = 0, blks = 0;
    for (int k = 0; k < n; ++k) {
        const pseg_eval_page& s = pages[g0 + k];
        EpPage& t = h_tab[k];
        const size_t bytes = (size_t)s.H * s.W;
        t.H = s.H; t.W = s.W; t.pad = 0;
        t.has_bin = s.binary != nullptr;
        t.tiles_x = std::max(1, cdiv(s.W, EP_TW));
        t.tile0 = (int)tiles;
        t.blk0 = (int)blks;
        t.nblk = bytes ? (int)std::max<size_t>(1, std::min<size_t>(EP_HIST_BLOCKS, ((bytes >> 4) + 1023) / 1024)) : 0;
        t.pred = at.take(bytes);
        t.mask = at.take(bytes);
        t.bin = at.take(t.has_bin ? bytes : 0);
        if (t.has_bin && bytes) tiles += (long long)t.tiles_x * cdiv(s.H, EP_TH);
        blks += t.nblk;
    }
    if (tiles * EP_OPEN_MAX > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "pages %d..%d: too many tiles for 32-bit slot ids", g0, g1 - 1);
    // per tile: 192 root slots (parent + cw counters each), the rim table, the task list, two list lengths
    const size_t nslots = (size_t)tiles * EP_OPEN_MAX;
    const size_t o_par = at.take(nslots * 4), o_cnt = at.take(nslots * cw * 4), o_rim = at.take((size_t)tiles * EP_RIM);
    const size_t o_task = at.take((size_t)tiles * EP_TASK_MAX * 4), o_rootn = at.take((size_t)tiles * 4), o_taskn = at.take((size_t)tiles * 4);
    PSEG_TRY(ws.dev.ensure(at.off, "page-score workspace"));
    if (!ws.st) PSEG_HIP(hipStreamCreateWithFlags(&ws.st, hipStreamNonBlocking));
    hipStream_t st = ws.st;
    uint8_t* const d = ws.dev.p;
    const EpRules* const d_rules = (const EpRules*)d;
    const EpPage* const d_tab = (const EpPage*)(d + sizeof(EpRules));
    unsigned long long* const d_rec = (unsigned long long*)(d + tab_b);
    GroupDrain drain{st};
    PSEG_HIP(hipMemcpyAsync(d, ws.pin.p, sizeof(EpRules) + (size_t)n * sizeof(EpPage), hipMemcpyHostToDevice, st));
    PSEG_HIP(hipMemsetAsync(d_rec, 0, (size_t)n * rec_words * 8, st));
    for (int k = 0; k < n; ++k) {
        const pseg_eval_page& s = pages[g0 + k];
        const size_t bytes = (size_t)s.H * s.W;
        if (!bytes) continue;
        PSEG_HIP(hipMemcpyAsync(d + h_tab[k].pred, s.pred, bytes, hipMemcpyHostToDevice, st));
        PSEG_HIP(hipMemcpyAsync(d + h_tab[k].mask, s.mask, bytes, hipMemcpyHostToDevice, st));
        if (s.binary) PSEG_HIP(hipMemcpyAsync(d + h_tab[k].bin, s.binary, bytes, hipMemcpyHostToDevice, st));
    }
    if (blks > 0) {
        const int use_lds = slots * 4 <= 48 * 1024;
        ep_hist_kernel<<<(unsigned)blks, 256, use_lds ? slots * 4 : 0, st>>>(d, d_tab, n, ncls, use_lds, d_rec, rec_words);
    }
    if (tiles > 0) {
        int* const d_par = (int*)(d + o_par);
        unsigned* const d_cnt = (unsigned*)(d + o_cnt);
        uint8_t* const d_rim = d + o_rim;
        unsigned* const d_task = (unsigned*)(d + o_task);
        int* const d_rootn = (int*)(d + o_rootn);
        int* const d_taskn = (int*)(d + o_taskn);
        const int nt = (int)tiles, cap = (int)nslots;
        if (conn == 8)
            ep_tile_kernel<true><<<nt, 256, 0, st>>>(d, d_rules, d_tab, n, d_par, d_cnt, cw, d_rim, d_task, d_rootn, d_taskn, d_rec, rec_words, ver0);
        else
            ep_tile_kernel<false><<<nt, 256, 0, st>>>(d, d_rules, d_tab, n, d_par, d_cnt, cw, d_rim, d_task, d_rootn, d_taskn, d_rec, rec_words, ver0);
        ep_border_kernel<<<cdiv(nt, 4), 256, 0, st>>>(d_tab, n, d_rim, d_task, d_taskn, d_rootn, d_par, nt, cap);
        ep_merge_kernel<<<cdiv(nt, 4), 256, 0, st>>>(d_par, d_cnt, cw, d_rootn, nt, cap);
        ep_judge_kernel<<<cdiv(nt, 4), 256, 0, st>>>(d_rules, d_tab, n, d_par, d_cnt, cw, d_rootn, nt, d_rec, rec_words, ver0);
    }
    PSEG_HIP(hipGetLastError());
    const unsigned long long* const h_rec = (const unsigned long long*)(ws.pin.p + tab_b);
    PSEG_HIP(hipMemcpyAsync(ws.pin.p + tab_b, d_rec, (size_t)n * rec_words * 8, hipMemcpyDeviceToHost, st));
    PSEG_HIP(hipStreamSynchronize(st));                                // the group's one wait
    drain.armed = false;
    for (int k = 0; k < n; ++k) {
        const unsigned long long* r = h_rec + (size_t)k * rec_words;
        if (!out.counts.empty()) std::copy(r, r + slots, out.counts.begin() + (size_t)(g0 + k) * slots);
        if (!out.comps.empty()) out.comps[g0 + k] = (int64_t)r[ver0 + EP_VER - 1];
        for (size_t j = 0; !out.verdicts.empty() && j < (size_t)rules.n_rules * 4; ++j)
            out.verdicts[(size_t)(g0 + k) * rules.n_rules * 4 + j] = (int64_t)r[ver0 + j];
    }
    return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_eval_page_groups(int n_pages, const int* H, const int* W, int* first, int* count, int max_groups) {
    if (n_pages < 0 || (n_pages > 0 && (!H || !W))) return fail(PSEG_EINVAL, n_pages < 0 ? "negative page count" : "NULL argument");
    for (int i = 0; i < n_pages; ++i)
        if (H[i] < 0 || W[i] < 0) return fail(PSEG_EINVAL, "page %d: negative size", i);
    int ng = 0;
    for (int g0 = 0; g0 < n_pages; ++ng) {
        const int g1 = list_group_end(n_pages, g0, [&](int i) { return (size_t)H[i] * W[i]; });
        if (ng < max_groups) {
            if (first) first[ng] = g0;
            if (count) count[ng] = g1 - g0;
        }
        g0 = g1;
    }
    return ng;
}

int pseg_eval_pages(int device, int n_pages, const pseg_eval_page* pages, int n_classes, int connectivity, int n_rules,
                    const pseg_eval_rule* rules, int64_t* counts, int64_t* components, int64_t* verdicts) {
    if (n_pages < 0) return fail(PSEG_EINVAL, "negative page count");
    if (n_classes < 1 || n_classes > 255) return fail(PSEG_EINVAL, "n_classes %d outside 1..255", n_classes);
    if (connectivity != 4 && connectivity != 8) return fail(PSEG_EINVAL, "connectivity %d (4 or 8)", connectivity);
    if (n_rules < 0 || n_rules > EP_RULES) return fail(PSEG_EINVAL, "%d rules (0..%d)", n_rules, EP_RULES);
    if ((n_rules > 0 && !rules) || (n_pages > 0 && !pages)) return fail(PSEG_EINVAL, "NULL argument");
    EpRules R;
    std::memset(&R, 0, sizeof(R));
    R.n_rules = n_rules;
    auto watch = [&](int label) {
        for (int w = 0; w < R.n_watch; ++w) if (R.watch[w] == label) return w;
        R.watch[R.n_watch] = label;
        return R.n_watch++;
    };
    for (int i = 0; i < n_rules; ++i) {
        const pseg_eval_rule& s = rules[i];
        if (s.kind != 0 && s.kind != 1) return fail(PSEG_EINVAL, "rule %d: kind %d (0: cc_matching, 1: cc_equal)", i, s.kind);
        if (s.label < 0 || s.label >= n_classes) return fail(PSEG_EINVAL, "rule %d: label %d outside [0, %d)", i, s.label, n_classes);
        if (s.filter_label < 0 || s.filter_label >= n_classes)
            return fail(PSEG_EINVAL, "rule %d: filter label %d outside [0, %d)", i, s.filter_label, n_classes);
        EpRule& r = R.r[i];
        r.kind = s.kind;
        r.li = s.kind == 0 ? watch(s.label) : -1;
        r.fi = s.filter_label ? watch(s.filter_label) : -1;
        r.t_tp = s.threshold_tp; r.t_fp = s.threshold_fp; r.t_mask = s.threshold_mask; r.t_filter = s.filter_threshold;
    }
    for (int i = 0; i < n_pages; ++i) {
        const pseg_eval_page& p = pages[i];
        if (p.H < 0 || p.W < 0) return fail(PSEG_EINVAL, "page %d: negative size", i);
        if ((int64_t)p.H * p.W > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "page %d: too large for 32-bit counters", i);
        if ((int64_t)p.H * p.W > 0 && (!p.pred || !p.mask)) return fail(PSEG_EINVAL, "page %d: NULL map", i);
    }
    if (n_pages == 0) return PSEG_OK;
    const size_t slots = (size_t)2 * (n_classes + 1) * (n_classes + 1);
    EpOut out;                                                         // the caller's arrays are written once every group has run
    if (counts) out.counts.assign((size_t)n_pages * slots, 0);
    if (components) out.comps.assign((size_t)n_pages, 0);
    if (verdicts && n_rules) out.verdicts.assign((size_t)n_pages * n_rules * 4, 0);
    PSEG_TRY(run_list(g_ep, device, n_pages, [&](int i) { return (size_t)pages[i].H * pages[i].W; },
                      [&](EpWs& ws, int g0, int g1) { return ep_group(ws, g0, g1, pages, n_classes, connectivity, R, out); }));
    if (counts) std::copy(out.counts.begin(), out.counts.end(), counts);
    if (components) std::copy(out.comps.begin(), out.comps.end(), components);
    if (verdicts && n_rules) std::copy(out.verdicts.begin(), out.verdicts.end(), verdicts);
    return PSEG_OK;
}

}  // extern "C"
