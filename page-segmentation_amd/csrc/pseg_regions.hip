// pseg_regions.hip -- the text regions of a list of label maps in one device-resident call: lab == t, a close, an
// open, a double dilation and an erosion with rectangles, the holes of the result filled, and the 4-connected components of that as
// a table of boxes, areas and seeds.  The host entry and the crack-polygon tracer live here too.
//
// Everything runs on bit planes (pseg_regions.h).  A morphology launch does one operation for every map of the group: a workgroup
// takes RG_BAND output rows of RG_WC word columns, runs the x pass (rg_xpass, shared with the host) for the band's rows and its halo
// of k - 1 rows into LDS, and ORs k rows together there by doubling.  The component machine is the page scorer's and the
// despeckling's closed / open tile scheme cut down to bit tiles: a workgroup labels the pixels of a 32 x 64 tile in LDS (a pixel
// starts at its run's first pixel, runs are joined with the run above at the start of every stretch they share); a component with no
// set neighbour across the tile's edge is CLOSED and is finished on the spot; an OPEN one takes one of the tile's 192 root slots, and
// three small launches join the slots across the tile edges (rg_border_kernel, from the tiles' rim tables), fold the redirected slots'
// records into their final root (rg_merge_kernel) and act on the final roots (rg_apply_kernel / rg_emit_kernel).  It runs twice:
// MODE 0 on the complement of the joined plane with a "touches the map's edge" flag -- a component without it is a hole and is set
// in T; MODE 1 on T with box, area and seed -- a final root appends its row to the map's table through an atomic counter.
//
// Every loop bound below is an argument, a constant or a table entry the host built; every find / unite loop is bounded (links only
// ever point at a smaller index of the same component).  After the border launch the links are at rest, and every later walk follows
// them to the root without a store: a link is never taken for a root.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pseg_list.h"
#include "pseg_regions.h"

namespace pseg {

constexpr int RG_NPX = RG_TH * RG_TW;
constexpr int RG_STAT = 5;                         // MODE 1 record of a slot: area, min x, max x, max y, seed (y * W + x; min y is the seed's row)
constexpr int RG_OPS = 7;

// one map of a group: tile0 and mb0 are the prefix tables of the ragged launches (component tiles / morphology workgroups before it)
struct RgMap {
    int H, W, wpr, label;
    int k[3];
    int tile0, tiles_x, mb0, mbx, want_mask;
    unsigned long long lab;                        // the label map's bytes on the device (an address; the mask's bytes on the way back)
    unsigned long long plane_off;                  // three planes of H * wpr words, in the group's workspace
    unsigned long long row_off;                    // the map's first row in the group's table
};

__device__ __forceinline__ int rg_map_of_tile(const RgMap* __restrict__ tab, int n, int b) {
    int lo = 0, hi = n - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {   // largest i with tab[i].tile0 <= b
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].tile0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ int rg_map_of_mb(const RgMap* __restrict__ tab, int n, int b) {
    int lo = 0, hi = n - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].mb0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ rg_word* rg_plane(uint8_t* buf, const RgMap& pg, int which) {
    return (rg_word*)(buf + pg.plane_off) + (size_t)which * pg.H * pg.wpr;
}
__device__ __forceinline__ rg_word rg_below(int b) { return b <= 0 ? 0ull : b >= 64 ? ~0ull : ((1ull << b) - 1ull); }   // bits 0 .. b-1

// ---- lab == t -> plane 0; plane 2 -> bytes.  One workgroup per 32 x 64 tile, a wave per 8 rows, a lane per column ------------------
__global__ __launch_bounds__(256) void rg_pack_kernel(uint8_t* buf, const RgMap* __restrict__ tab, int n) {
    const int tile = blockIdx.x, pi = rg_map_of_tile(tab, n, tile);
    const RgMap pg = tab[pi];
    const int lt = tile - pg.tile0, ty = lt / pg.tiles_x, tx = lt - ty * pg.tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t* const lab = (const uint8_t*)pg.lab;
    rg_word* const A = rg_plane(buf, pg, 0);
    const int x = tx * RG_TW + lane;
#pragma unroll
    for (int j = 0; j < RG_TH / 4; ++j) {
        const int y = ty * RG_TH + wave * (RG_TH / 4) + j;
        const bool in = y < pg.H && x < pg.W;
        const bool v = in && (int)lab[(size_t)y * pg.W + x] == pg.label;
        const rg_word w = __ballot(v);
        if (lane == 0 && y < pg.H) A[(size_t)y * pg.wpr + tx] = w;
    }
}
__global__ __launch_bounds__(256) void rg_unpack_kernel(uint8_t* buf, const RgMap* __restrict__ tab, int n) {
    const int tile = blockIdx.x, pi = rg_map_of_tile(tab, n, tile);
    const RgMap pg = tab[pi];
    if (!pg.want_mask) return;
    const int lt = tile - pg.tile0, ty = lt / pg.tiles_x, tx = lt - ty * pg.tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* const out = (uint8_t*)pg.lab;
    const rg_word* const T = rg_plane(buf, pg, 2);
    const int x = tx * RG_TW + lane;
#pragma unroll
    for (int j = 0; j < RG_TH / 4; ++j) {
        const int y = ty * RG_TH + wave * (RG_TH / 4) + j;
        if (y < pg.H && x < pg.W) out[(size_t)y * pg.W + x] = (uint8_t)((T[(size_t)y * pg.wpr + tx] >> lane) & 1ull);
    }
}

// ---- one rectangle operation of every map: x pass into LDS, y pass by doubling there -----------------------------------------------
// op: 0 dil k1 (0 -> 1), 1 ero k1 (1 -> 0), 2 ero k2 (0 -> 1), 3 dil k2 (1 -> 0), 4 dil k3 (0 -> 1), 5 dil k3 (1 -> 2), 6 ero k3 (2 -> 1)
__host__ __device__ inline int rg_op_src(int op) { return op == 6 ? 2 : (op & 1); }
__host__ __device__ inline int rg_op_dst(int op) { return op == 5 ? 2 : op == 6 ? 1 : ((op & 1) ^ 1); }
__host__ __device__ inline bool rg_op_ero(int op) { return op == 1 || op == 2 || op == 6; }
__host__ __device__ inline int rg_op_side(int op) { return op < 2 ? 0 : op < 4 ? 1 : 2; }

__global__ __launch_bounds__(256) void rg_morph_kernel(uint8_t* buf, const RgMap* __restrict__ tab, int n, int op) {
    __shared__ rg_word ls[2][RG_ROWS_MAX * RG_WC];
    const int blk = blockIdx.x, pi = rg_map_of_mb(tab, n, blk);
    const RgMap pg = tab[pi];
    const int lb = blk - pg.mb0, by = lb / pg.mbx, bx = lb - by * pg.mbx;
    const int H = pg.H, W = pg.W, wpr = pg.wpr;
    const int side = rg_op_side(op);
    const int k = min(max(side == 0 ? pg.k[0] : side == 1 ? pg.k[1] : pg.k[2], 1), RG_SIDE_MAX);   // (no indexing of the copy by a variable)
    const bool ero = rg_op_ero(op);
    const rg_word* const src = rg_plane(buf, pg, rg_op_src(op));
    rg_word* const dst = rg_plane(buf, pg, rg_op_dst(op));
    const int y0 = by * RG_BAND, j0 = bx * RG_WC;
    const int nout = min(RG_BAND, H - y0);
    if (nout <= 0) return;
    const int R = nout + k - 1, yf = rg_band_first(y0, k);             // R <= RG_ROWS_MAX
    for (int i = threadIdx.x; i < R * RG_WC; i += 256) {
        const int r = i / RG_WC, c = i - r * RG_WC, y = yf + r, j = j0 + c;
        ls[0][i] = (y >= 0 && y < H && j < wpr) ? rg_xpass(src + (size_t)y * wpr, wpr, W, j, k, ero) : 0ull;
    }
    __syncthreads();
    int cur = 0, p = 1;
    for (int it = 0; it < 8 && 2 * p <= k; ++it) {                     // ls[cur][r]: the OR of rows r .. r + p - 1
        for (int i = threadIdx.x; i < R * RG_WC; i += 256) {
            const int r = i / RG_WC;
            rg_word v = ls[cur][i];
            if (r + p < R) v |= ls[cur][i + p * RG_WC];
            ls[cur ^ 1][i] = v;
        }
        __syncthreads();
        cur ^= 1;
        p <<= 1;
    }
    const int s = k - p;                                               // rows o .. o + p - 1 and o + s .. o + k - 1; o + s + (row stride) stays below R
    for (int i = threadIdx.x; i < nout * RG_WC; i += 256) {
        const int o = i / RG_WC, c = i - o * RG_WC, j = j0 + c;
        if (j >= wpr) continue;
        const rg_word v = ls[cur][i] | ls[cur][i + s * RG_WC];
        dst[(size_t)(y0 + o) * wpr + j] = rg_store(v, W, j, ero);
    }
}

// ---- union-find: LDS (pixels of a tile) and global (root slot ids of a group) ------------------------------------------------------
__device__ __forceinline__ int rg_lds_find(const int* lab, int x) {
    for (int it = 0; it < RG_NPX; ++it) {
        const int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) break;
        x = p;
    }
    return x;
}
// a lost atomicMin hands back a link below the larger root: max(a, b) strictly decreases
__device__ __forceinline__ void rg_lds_union(int* lab, int a, int b) {
    for (int it = 0; it < RG_NPX; ++it) {
        a = rg_lds_find(lab, a);
        b = rg_lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}
// the border launch's find: no store at all, so no link ever moves except by a union's atomicMin at a root
__device__ __forceinline__ int rg_find(const int* L, int x, int cap) {
    for (int it = 0; it < cap; ++it) {
        const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x || p < 0 || p >= cap) break;
        x = p;
    }
    return x;
}
__device__ __forceinline__ void rg_union(int* L, int a, int b, int cap) {
    for (int it = 0; it < cap; ++it) {
        a = rg_find(L, a, cap);
        b = rg_find(L, b, cap);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}
// the root of x once every union is over (a launch later): the links are followed to the end
__device__ __forceinline__ int rg_root(const int* __restrict__ L, int x, int cap) {
    for (int it = 0; it < cap; ++it) {
        const int p = L[x];
        if (p == x || p < 0 || p >= cap) break;
        x = p;
    }
    return x;
}

__device__ __forceinline__ void rg_put_row(int* __restrict__ rows, int* __restrict__ counts, const RgMap& pg, int pi, int max_regions,
                                           int area, int minx, int maxx, int maxy, int seed) {
    const int idx = atomicAdd(&counts[pi], 1);
    if (idx >= max_regions) return;
    int* const r = rows + ((size_t)pg.row_off + idx) * RG_ROW_INTS;
    const int sy = seed / pg.W, sx = seed - sy * pg.W;
    r[0] = minx; r[1] = sy; r[2] = maxx + 1; r[3] = maxy + 1; r[4] = area; r[5] = sy; r[6] = sx; r[7] = 0;
}

// One workgroup per (map, 32 x 64 tile).  MODE 0: the pixels are the complement of plane 1 inside the map, a component's record is
// "touches the map's edge", plane 2 becomes plane 0 | plane 1 | the tile's closed holes.  MODE 1: the pixels are plane 2, the record is
// area, box and seed, a closed component's row goes to the table.
template <int MODE>
__global__ __launch_bounds__(256) void rg_tile_kernel(uint8_t* buf, const RgMap* __restrict__ tab, int n, int* P, int* __restrict__ stat,
                                                      uint8_t* __restrict__ slotpl, uint8_t* __restrict__ rimtab, int* __restrict__ rootn,
                                                      int* __restrict__ rows, int* __restrict__ counts, int max_regions) {
    constexpr int RPW = RG_TH / 4, NS = MODE ? RG_NPX : 1;
    __shared__ rg_word ink[RG_TH + 2];                                 // tile rows -1 .. RG_TH
    __shared__ unsigned lrm[2];                                        // set pixels left / right of the tile (bit = row)
    __shared__ int parent[RG_NPX];
    __shared__ int st_area[NS], st_minx[NS], st_maxx[NS], st_maxy[NS];
    __shared__ uint8_t slotk[RG_NPX];
    __shared__ unsigned openb[RG_NPX / 32], flagb[RG_NPX / 32];
    __shared__ int nopen;
    const int tile = blockIdx.x, pi = rg_map_of_tile(tab, n, tile);
    const RgMap pg = tab[pi];
    const int H = pg.H, W = pg.W, wpr = pg.wpr;
    const int lt = tile - pg.tile0, ty = lt / pg.tiles_x, tx = lt - ty * pg.tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y0 = ty * RG_TH, x0 = tx * RG_TW;
    const rg_word* const S = rg_plane(buf, pg, MODE == 0 ? 1 : 2);
    rg_word* const T = rg_plane(buf, pg, 2);
    if (threadIdx.x < RG_TH + 2) {
        const int y = y0 + (int)threadIdx.x - 1;
        ink[threadIdx.x] = (y >= 0 && y < H) ? rg_load(S + (size_t)y * wpr, wpr, W, tx, MODE == 0) : 0ull;
        if (MODE == 0 && threadIdx.x >= 1 && threadIdx.x <= RG_TH && y < H)
            T[(size_t)y * wpr + tx] = rg_plane(buf, pg, 0)[(size_t)y * wpr + tx] | S[(size_t)y * wpr + tx];
    }
    if (wave == 1) {
        const int y = y0 + lane;
        const bool ok = lane < RG_TH && y < H;
        const bool lb = ok && (rg_load(S + (size_t)(ok ? y : 0) * wpr, wpr, W, tx - 1, MODE == 0) >> 63) != 0;
        const bool rb = ok && (rg_load(S + (size_t)(ok ? y : 0) * wpr, wpr, W, tx + 1, MODE == 0) & 1ull) != 0;
        const rg_word bl = __ballot(lb), br = __ballot(rb);
        if (lane == 0) { lrm[0] = (unsigned)bl; lrm[1] = (unsigned)br; }
    }
    if (threadIdx.x < RG_NPX / 32) { openb[threadIdx.x] = 0; flagb[threadIdx.x] = 0; }
    if (threadIdx.x == 0) nopen = 0;
    __syncthreads();
    if (!__syncthreads_or(threadIdx.x < RG_TH && ink[threadIdx.x + 1] != 0ull)) {   // nothing set in this tile
        if (threadIdx.x == 0) rootn[tile] = 0;
        return;
    }
    // ---- every pixel starts at the first pixel of its run ----
    const int rw0 = wave * RPW;
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int r = rw0 + j, p = r * RG_TW + lane;
        const rg_word m = ink[r + 1];
        int start = lane;
        if ((m >> lane) & 1ull) {
            const rg_word z = ~m & rg_below(lane);
            start = z ? 64 - __builtin_clzll(z) : 0;
        }
        parent[p] = r * RG_TW + start;
        if constexpr (MODE != 0) { st_area[p] = 0; st_minx[p] = RG_TW; st_maxx[p] = -1; st_maxy[p] = -1; }
    }
    __syncthreads();
    // ---- a run and the run above it are joined once per stretch of columns they share ----
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int r = rw0 + j, p = r * RG_TW + lane;
        if (r == 0) continue;
        const rg_word ov = ink[r + 1] & ink[r];
        const rg_word stt = ov & ~(ov << 1);
        if ((stt >> lane) & 1ull) rg_lds_union(parent, p, p - RG_TW);
    }
    __syncthreads();
    // ---- roots; per run: the record, open (a set neighbour across the tile's edge), the flag ----
    const rg_word m_up = ink[0], m_dn = ink[RG_TH + 1];
    const unsigned lr0 = lrm[0], lr1 = lrm[1];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int r = rw0 + j, p = r * RG_TW + lane;
        const rg_word m = ink[r + 1];
        if (!((m >> lane) & 1ull)) continue;
        const int rt = rg_lds_find(parent, p);
        if (rt != p) __hip_atomic_store(&parent[p], rt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // the unions are over
        if (lane > 0 && ((m >> (lane - 1)) & 1ull)) continue;          // the run's first pixel speaks for the run
        const rg_word above = ~m & ~rg_below(lane + 1);
        const int e = above ? __builtin_ctzll(above) - 1 : 63;
        const rg_word run = rg_below(e + 1) & ~rg_below(lane);
        if constexpr (MODE != 0) {
            atomicAdd(&st_area[rt], e - lane + 1);
            atomicMin(&st_minx[rt], lane);
            atomicMax(&st_maxx[rt], e);
            atomicMax(&st_maxy[rt], r);
        }
        bool open = false;
        if (r == 0) open |= (run & m_up) != 0ull;
        if (r == RG_TH - 1) open |= (run & m_dn) != 0ull;
        if (lane == 0) open |= ((lr0 >> r) & 1u) != 0u;
        if (e == RG_TW - 1) open |= ((lr1 >> r) & 1u) != 0u;
        if (open) atomicOr(&openb[rt >> 5], 1u << (rt & 31));
        if (MODE == 0) {
            const int y = y0 + r;
            if (y == 0 || y == H - 1 || x0 + lane == 0 || x0 + e == W - 1) atomicOr(&flagb[rt >> 5], 1u << (rt & 31));
        }
    }
    __syncthreads();
    // ---- closed roots are finished here; open roots take a slot ----
    for (int t0 = 0; t0 < RG_NPX; t0 += 256) {
        const int t = t0 + (int)threadIdx.x, r = t >> 6, c = t & 63;
        const bool set = (ink[r + 1] >> c) & 1ull;
        const bool is_root = set && parent[t] == t;
        const bool is_open = is_root && ((openb[t >> 5] >> (t & 31)) & 1u);
        const int seed = (y0 + r) * W + x0 + c;                        // the root is the component's first pixel of the tile in raster order
        if constexpr (MODE != 0)
            if (is_root && !is_open) rg_put_row(rows, counts, pg, pi, max_regions, st_area[t], x0 + st_minx[t], x0 + st_maxx[t], y0 + st_maxy[t], seed);
        const rg_word orm = __ballot(is_open);
        if (orm) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&nopen, __popcll(orm));
            base = __shfl(base, 0);
            if (is_open) {
                const int k = min(base + __popcll(orm & rg_below(lane)), RG_SLOTS - 1);   // (188 rim pixels: the bound holds)
                const int id = tile * RG_SLOTS + k;
                slotk[t] = (uint8_t)k;
                P[id] = id;
                if constexpr (MODE != 0) {
                    int* const s = stat + (size_t)id * RG_STAT;
                    s[0] = st_area[t]; s[1] = x0 + st_minx[t]; s[2] = x0 + st_maxx[t]; s[3] = y0 + st_maxy[t]; s[4] = seed;
                } else {
                    stat[id] = (int)((flagb[t >> 5] >> (t & 31)) & 1u);
                }
            }
        }
    }
    __syncthreads();
    // ---- MODE 0: the closed holes into plane 2, every pixel's slot into the slot plane; both: the rim table ----
    const int n_open = nopen;
    if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const int r = rw0 + j, p = r * RG_TW + lane, y = y0 + r;
            const bool set = (ink[r + 1] >> lane) & 1ull;
            const int rt = set ? parent[p] : 0;
            const bool op = set && ((openb[rt >> 5] >> (rt & 31)) & 1u);
            const bool hole = set && !op && !((flagb[rt >> 5] >> (rt & 31)) & 1u);
            const rg_word hw = __ballot(hole);
            if (lane == 0 && hw && y < H) T[(size_t)y * wpr + tx] |= hw;
            if (n_open > 0) slotpl[(size_t)tile * RG_NPX + p] = op ? slotk[rt] : (uint8_t)255;
        }
    }
    if (threadIdx.x < RG_RIM) {
        const int q = threadIdx.x;
        const int r = q < RG_TW ? 0 : q < 2 * RG_TW ? RG_TH - 1 : q < 2 * RG_TW + RG_TH ? q - 2 * RG_TW : q - 2 * RG_TW - RG_TH;
        const int c = q < RG_TW ? q : q < 2 * RG_TW ? q - RG_TW : q < 2 * RG_TW + RG_TH ? 0 : RG_TW - 1;
        const bool set = (ink[r + 1] >> c) & 1ull;
        const int rt = set ? parent[r * RG_TW + c] : 0;
        const bool op = set && ((openb[rt >> 5] >> (rt & 31)) & 1u);
        rimtab[(size_t)tile * RG_RIM + q] = op ? slotk[rt] : (uint8_t)255;
    }
    if (threadIdx.x == 0) rootn[tile] = min(n_open, RG_SLOTS);
}

// unions of the open components across tile edges, on the root slot ids: a wave per tile joins the pixels of its top row with the
// bottom row of the tile above and those of its left column with the right column of the tile to the left, from the two rim tables.
// A pair whose neighbours in the rim are the same two slots is skipped.  A tile without an open root never wrote its rim table: it is
// not read.
__global__ __launch_bounds__(256) void rg_border_kernel(const RgMap* __restrict__ tab, int n, const uint8_t* __restrict__ rimtab,
                                                        const int* __restrict__ rootn, int* P, int tiles, int cap) {
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tiles) return;
    const int nr = rootn[tile];
    if (nr <= 0) return;
    const RgMap pg = tab[rg_map_of_tile(tab, n, tile)];
    const int lt = tile - pg.tile0, ty = lt / pg.tiles_x, tx = lt - ty * pg.tiles_x;
    const uint8_t* const mine = rimtab + (size_t)tile * RG_RIM;
    if (ty > 0) {
        const int nb = tile - pg.tiles_x, nn = rootn[nb];
        if (nn > 0) {
            const uint8_t* const theirs = rimtab + (size_t)nb * RG_RIM + RG_TW;
            const int k = mine[lane], ks = theirs[lane];
            const bool same = lane > 0 && mine[lane - 1] == k && theirs[lane - 1] == ks;
            if (k < nr && ks < nn && !same) rg_union(P, tile * RG_SLOTS + k, nb * RG_SLOTS + ks, cap);
        }
    }
    if (tx > 0 && lane < RG_TH) {
        const int nb = tile - 1, nn = rootn[nb];
        if (nn > 0) {
            const uint8_t* const me = mine + 2 * RG_TW;
            const uint8_t* const theirs = rimtab + (size_t)nb * RG_RIM + 2 * RG_TW + RG_TH;
            const int k = me[lane], ks = theirs[lane];
            const bool same = lane > 0 && me[lane - 1] == k && theirs[lane - 1] == ks;
            if (k < nr && ks < nn && !same) rg_union(P, tile * RG_SLOTS + k, nb * RG_SLOTS + ks, cap);
        }
    }
}

// the record of every slot that a border union redirected, folded into its final root's.  Only final roots are written, only
// redirected slots are read: nothing that is read here changes here.  One wave per tile.
template <int MODE>
__global__ __launch_bounds__(256) void rg_merge_kernel(const int* __restrict__ P, int* stat, const int* __restrict__ rootn, int tiles, int cap) {
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tiles) return;
    const int nr = min(rootn[tile], RG_SLOTS);
    for (int k = lane; k < nr; k += 64) {
        const int id = tile * RG_SLOTS + k, r = rg_root(P, id, cap);
        if (r == id) continue;
        if (MODE) {
            const int* const s = stat + (size_t)id * RG_STAT;
            int* const d = stat + (size_t)r * RG_STAT;
            atomicAdd(&d[0], s[0]);
            atomicMin(&d[1], s[1]);
            atomicMax(&d[2], s[2]);
            atomicMax(&d[3], s[3]);
            atomicMin(&d[4], s[4]);
        } else if (stat[id]) {
            atomicOr(&stat[r], 1);
        }
    }
}

// MODE 0's end: the pixels of every open component whose final root never touched the map's edge are holes: set in plane 2.  One
// workgroup per tile; the tile's words are this workgroup's alone.
__global__ __launch_bounds__(256) void rg_apply_kernel(uint8_t* buf, const RgMap* __restrict__ tab, int n, const int* __restrict__ P,
                                                       const int* __restrict__ stat, const uint8_t* __restrict__ slotpl,
                                                       const int* __restrict__ rootn, int cap) {
    __shared__ uint8_t hole[RG_SLOTS];
    const int tile = blockIdx.x;
    const int nr = min(rootn[tile], RG_SLOTS);
    if (nr <= 0) return;
    const RgMap pg = tab[rg_map_of_tile(tab, n, tile)];
    const int lt = tile - pg.tile0, ty = lt / pg.tiles_x, tx = lt - ty * pg.tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)threadIdx.x < nr) hole[threadIdx.x] = stat[rg_root(P, tile * RG_SLOTS + (int)threadIdx.x, cap)] ? 0 : 1;
    __syncthreads();
    rg_word* const T = rg_plane(buf, pg, 2);
#pragma unroll
    for (int j = 0; j < RG_TH / 4; ++j) {
        const int r = wave * (RG_TH / 4) + j, y = ty * RG_TH + r;
        const int k = slotpl[(size_t)tile * RG_NPX + r * RG_TW + lane];
        const rg_word hw = __ballot(k < nr && hole[k]);
        if (lane == 0 && hw && y < pg.H) T[(size_t)y * pg.wpr + tx] |= hw & rg_tail_mask(pg.W, tx);
    }
}

// MODE 1's end: every slot that is still a root is one region: its row.  One wave per tile.
__global__ __launch_bounds__(256) void rg_emit_kernel(const RgMap* __restrict__ tab, int n, const int* __restrict__ P, const int* __restrict__ stat,
                                                      const int* __restrict__ rootn, int tiles, int* __restrict__ rows,
                                                      int* __restrict__ counts, int max_regions) {
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tiles) return;
    const int nr = min(rootn[tile], RG_SLOTS);
    if (nr <= 0) return;
    const int pi = rg_map_of_tile(tab, n, tile);
    const RgMap pg = tab[pi];
    for (int k = lane; k < nr; k += 64) {
        const int id = tile * RG_SLOTS + k;
        if (P[id] != id) continue;
        const int* const s = stat + (size_t)id * RG_STAT;
        rg_put_row(rows, counts, pg, pi, max_regions, s[0], s[1], s[2], s[3], s[4]);
    }
}

// ---- the crack polygons of the emitted rows, from plane 2: a count pass, a scan, a write pass --------------------------
// One lane per emitted row (map k, row r in the order the rows were appended): the walk of pseg_regions.h from the row's seed.  A walk
// is a chain of dependent loads, so a lane per region keeps 64 of them in flight per wave; the word scans need no helper lanes.
// WRITE 0: nv[k * max_regions + r] = the vertex count, -1 for a walk that gave up.  WRITE 1: the vertices at voff[...], only for a
// map that the scan let through (mapv[4 k + 3]), and never more of them than the count pass counted.
template <int WRITE>
__global__ __launch_bounds__(64) void rg_trace_kernel(const uint8_t* buf, const RgMap* __restrict__ tab, int n, const int* __restrict__ rows,
                                                      const int* __restrict__ counts, int max_regions, long long* nv,
                                                      const long long* __restrict__ voff, const long long* __restrict__ mapv, int* xy) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    const int k = (int)(t / max_regions), r = (int)(t - (long long)k * max_regions);
    if (k >= n) return;
    const int c = counts[k];
    if (c > max_regions || r >= c) return;
    if (WRITE && !mapv[(size_t)k * RG_MAPV + 3]) return;
    const RgMap pg = tab[k];
    const rg_word* const T = (const rg_word*)(buf + pg.plane_off) + (size_t)2 * pg.H * pg.wpr;
    const int* const row = rows + ((size_t)pg.row_off + r) * RG_ROW_INTS;
    const int sy = row[5], sx = row[6];
    const bool seed_ok = sy >= 0 && sy < pg.H && sx >= 0 && sx < pg.W;
    if (WRITE) {
        const long long cnt = nv[t];
        if (seed_ok && cnt > 0) (void)rg_trace_words(T, pg.H, pg.W, pg.wpr, sx, sy, xy + 2 * voff[t], cnt);
    } else {
        nv[t] = seed_ok ? rg_trace_words(T, pg.H, pg.W, pg.wpr, sx, sy, nullptr, 0) : -1;
    }
}

// The exclusive scan of the counts over the rows of the group, one workgroup: voff[k * max_regions + r] = where row r of map k
// starts in the group's vertex array, mapv[4 k ..] = the map's total, its first vertex, its status and whether the write pass runs.
// per_map: every map owns vcap vertices at k * vcap; else the maps lie one behind the other in vcap vertices for the group, and a
// map that does not fit still moves the offsets on (the totals are always delivered).  A map with a walk that gave up, or with more
// rows than max_regions, has no vertices.
__global__ __launch_bounds__(256) void rg_scan_kernel(const int* __restrict__ counts, int n, int max_regions, const long long* __restrict__ nv,
                                                      long long* __restrict__ voff, long long* __restrict__ mapv, long long vcap, int per_map) {
    __shared__ long long part[256];
    __shared__ int bad;
    const int tid = threadIdx.x;
    long long run = 0;                                                 // uniform: the vertices of the maps before k
    for (int k = 0; k < n; ++k) {
        const int c = counts[k], m = (c > max_regions || c < 0) ? 0 : c;
        const long long* const v = nv + (size_t)k * max_regions;
        if (tid == 0) bad = 0;
        __syncthreads();
        long long sum = 0;
        bool neg = false;
        for (int r = tid; r < m; r += 256) {
            const long long x = v[r];
            neg |= x < 0;
            sum += x < 0 ? 0 : x;
        }
        if (neg) atomicOr(&bad, 1);
        part[tid] = sum;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) part[tid] += part[tid + s];
            __syncthreads();
        }
        const bool gave_up = bad != 0;
        const long long tot = gave_up ? 0 : part[0];
        const long long base = per_map ? (long long)k * vcap : run;
        const bool fits = !gave_up && c <= max_regions && (per_map ? tot <= vcap : base + tot <= vcap);
        __syncthreads();
        long long carry = base;
        for (int r0 = 0; r0 < m; r0 += 256) {                          // inclusive scan of a chunk of 256 by doubling
            const int r = r0 + tid;
            const long long x = (r < m && !gave_up) ? v[r] : 0;
            part[tid] = x;
            __syncthreads();
            for (int s = 1; s < 256; s <<= 1) {
                const long long add = tid >= s ? part[tid - s] : 0;
                __syncthreads();
                part[tid] += add;
                __syncthreads();
            }
            if (r < m) voff[(size_t)k * max_regions + r] = carry + part[tid] - x;
            carry += part[255];
            __syncthreads();
        }
        if (tid == 0) {
            long long* const o = mapv + (size_t)k * RG_MAPV;
            o[0] = tot; o[1] = base; o[2] = gave_up ? (long long)PSEG_EHIP : (c > max_regions ? (long long)PSEG_EUNSUPPORTED : (long long)PSEG_OK); o[3] = fits ? 1 : 0;
        }
        run += tot;
    }
}

// ---- workspace: grow-only, one per device, under its own lock and on its own stream; a call holds the lock to its end and every
// group ends synchronised.  pseg_release_workspace frees it.
struct RgWs {
    GrowDev dev; GrowPin pin, pinv; hipStream_t st = nullptr;   // pinv: the vertices of a polygon call's group
    void release() {
        dev.release();
        pin.release();
        pinv.release();
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
};
static PerDevice<RgWs> g_rg;

static bool rg_row_less(const int* a, const int* b) { return a[5] != b[5] ? a[5] < b[5] : a[6] < b[6]; }
// a map's rows by seed (the device appends them in no order)
static void rg_sort_rows(int* rows, int count) {
    struct Row { int v[RG_ROW_INTS]; };
    Row* const r = (Row*)rows;
    std::sort(r, r + count, [](const Row& a, const Row& b) { return rg_row_less(a.v, b.v); });
}

// ---- the stream-ordered stage: label maps on the device in, plane 2, the unsorted rows and the counts on the device out -------------
// rg_plan lays a group out in a workspace of lay.bytes bytes (host arithmetic; the caller sizes its buffer with it up front) and fills
// the maps' table except the label addresses; rg_enqueue launches the group on the caller's stream: no host wait, no allocation.
struct RgLay {
    size_t cnt, rows, par, stat, slot, rim, rootn, nv, voff, mapv, xy, bytes;   // byte offsets in the workspace; the table is at 0
    int tiles, mbs, poly, per_map;
    long long vcap;                                // vertices: of every map (per_map) or of the group
};

static int rg_plan(int n, const int* H, const int* W, const pseg_regions* how, int max_regions, int poly, long long vcap, int per_map,
                   RgMap* h_tab, RgLay& lay) {
    const size_t tab_b = up256((size_t)n * sizeof(RgMap));
    std::memset(h_tab, 0, tab_b);
    Bump at{tab_b};
    lay.cnt = at.take((size_t)n * 4);
    lay.rows = at.take((size_t)n * max_regions * RG_ROW_INTS * 4);
    long long tiles = 0, mbs = 0;
    for (int k = 0; k < n; ++k) {
        RgMap& t = h_tab[k];
        t.H = H[k]; t.W = W[k]; t.wpr = rg_words(W[k]);
        if (how) { t.label = how[k].label; t.k[0] = how[k].k_close; t.k[1] = how[k].k_open; t.k[2] = how[k].k_join; }
        t.tiles_x = t.wpr; t.tile0 = (int)tiles;
        t.mbx = cdiv(t.wpr, RG_WC); t.mb0 = (int)mbs;
        t.plane_off = at.take((size_t)3 * H[k] * t.wpr * 8);
        t.row_off = (unsigned long long)k * max_regions;
        tiles += (long long)t.tiles_x * cdiv(H[k], RG_TH);
        mbs += (long long)t.mbx * cdiv(H[k], RG_BAND);
    }
    if (tiles * RG_SLOTS > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "%d maps: too many tiles for 32-bit slot ids", n);
    const size_t nslots = (size_t)tiles * RG_SLOTS;
    lay.par = at.take(nslots * 4);
    lay.stat = at.take(nslots * RG_STAT * 4);
    lay.slot = at.take((size_t)tiles * RG_NPX);
    lay.rim = at.take((size_t)tiles * RG_RIM);
    lay.rootn = at.take((size_t)tiles * 4);
    lay.nv = lay.voff = lay.mapv = lay.xy = at.off;
    if (poly) {
        lay.nv = at.take((size_t)n * max_regions * 8);
        lay.voff = at.take((size_t)n * max_regions * 8);
        lay.mapv = at.take((size_t)n * RG_MAPV * 8);
        lay.xy = at.take((size_t)(per_map ? vcap * n : vcap) * 8);
    }
    lay.bytes = at.off;
    lay.tiles = (int)tiles; lay.mbs = (int)mbs; lay.poly = poly; lay.per_map = per_map; lay.vcap = vcap;
    return PSEG_OK;
}

static int rg_enqueue(hipStream_t st, uint8_t* d, const RgMap* h_tab, const RgLay& lay, int n, int max_regions) {
    const RgMap* const d_tab = (const RgMap*)d;
    int* const d_cnt = (int*)(d + lay.cnt);
    int* const d_rows = (int*)(d + lay.rows);
    int* const d_par = (int*)(d + lay.par);
    int* const d_stat = (int*)(d + lay.stat);
    uint8_t* const d_slot = d + lay.slot;
    uint8_t* const d_rim = d + lay.rim;
    int* const d_rootn = (int*)(d + lay.rootn);
    PSEG_HIP(hipMemcpyAsync(d, h_tab, (size_t)n * sizeof(RgMap), hipMemcpyHostToDevice, st));
    PSEG_HIP(hipMemsetAsync(d_cnt, 0, (size_t)n * 4, st));
    const int nt = lay.tiles, nm = lay.mbs, cap = nt * RG_SLOTS;
    rg_pack_kernel<<<nt, 256, 0, st>>>(d, d_tab, n);
    for (int op = 0; op < RG_OPS; ++op) rg_morph_kernel<<<nm, 256, 0, st>>>(d, d_tab, n, op);
    rg_tile_kernel<0><<<nt, 256, 0, st>>>(d, d_tab, n, d_par, d_stat, d_slot, d_rim, d_rootn, d_rows, d_cnt, max_regions);
    rg_border_kernel<<<cdiv(nt, 4), 256, 0, st>>>(d_tab, n, d_rim, d_rootn, d_par, nt, cap);
    rg_merge_kernel<0><<<cdiv(nt, 4), 256, 0, st>>>(d_par, d_stat, d_rootn, nt, cap);
    rg_apply_kernel<<<nt, 256, 0, st>>>(d, d_tab, n, d_par, d_stat, d_slot, d_rootn, cap);
    rg_tile_kernel<1><<<nt, 256, 0, st>>>(d, d_tab, n, d_par, d_stat, d_slot, d_rim, d_rootn, d_rows, d_cnt, max_regions);
    rg_border_kernel<<<cdiv(nt, 4), 256, 0, st>>>(d_tab, n, d_rim, d_rootn, d_par, nt, cap);
    rg_merge_kernel<1><<<cdiv(nt, 4), 256, 0, st>>>(d_par, d_stat, d_rootn, nt, cap);
    rg_emit_kernel<<<cdiv(nt, 4), 256, 0, st>>>(d_tab, n, d_par, d_stat, d_rootn, nt, d_rows, d_cnt, max_regions);
    bool any_mask = false;
    for (int k = 0; k < n; ++k) any_mask |= h_tab[k].want_mask != 0;
    if (any_mask) rg_unpack_kernel<<<nt, 256, 0, st>>>(d, d_tab, n);
    if (lay.poly && max_regions > 0) {
        long long* const d_nv = (long long*)(d + lay.nv);
        long long* const d_voff = (long long*)(d + lay.voff);
        long long* const d_mapv = (long long*)(d + lay.mapv);
        const int nb = cdiv(n * max_regions, 64);                       // (rg_check_list: the table's ints fit 31 bits)
        rg_trace_kernel<0><<<nb, 64, 0, st>>>(d, d_tab, n, d_rows, d_cnt, max_regions, d_nv, d_voff, d_mapv, nullptr);
        rg_scan_kernel<<<1, 256, 0, st>>>(d_cnt, n, max_regions, d_nv, d_voff, d_mapv, lay.vcap, lay.per_map);
        rg_trace_kernel<1><<<nb, 64, 0, st>>>(d, d_tab, n, d_rows, d_cnt, max_regions, d_nv, d_voff, d_mapv, (int*)(d + lay.xy));
    }
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

// what a polygon call gathers over its groups before anything reaches the caller's arrays
struct RgPolyOut {
    int64_t cap;
    std::vector<int32_t> xy;                       // the vertices so far, in the order of the sorted rows
    std::vector<int64_t> first;                    // n x (max_regions + 1)
    std::vector<int> status;
    int64_t need = 0;                              // the vertices of the list so far
};

// a map's sorted rows, its polygons behind the list's, its row of offsets: seg(j) hands out the vertices of the row that was at j
// before the sort and their number
template <class Seg>
static void rg_poly_map(RgPolyOut& po, int i, int max_regions, int32_t* rows, int c, int st, long long tot, Seg seg) {
    int64_t* const f = po.first.data() + (size_t)i * (max_regions + 1);
    po.status[i] = st;
    const bool over = po.need + tot > po.cap || po.need > po.cap;
    po.need += tot;
    if (st != PSEG_OK || over) {
        for (int j = 0; j <= max_regions; ++j) f[j] = (int64_t)(po.xy.size() / 2);
        return;
    }
    for (int j = 0; j < c; ++j) {
        long long nv = 0;
        const int32_t* const src = seg(rows[(size_t)j * RG_ROW_INTS + 7], &nv);
        rows[(size_t)j * RG_ROW_INTS + 7] = 0;
        f[j] = (int64_t)(po.xy.size() / 2);
        po.xy.insert(po.xy.end(), src, src + 2 * nv);
    }
    for (int j = c; j <= max_regions; ++j) f[j] = (int64_t)(po.xy.size() / 2);
}

static int rg_group(RgWs& ws, int g0, int g1, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                    uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count, RgPolyOut* po) {
    const int n = g1 - g0;
    const size_t tab_b = up256((size_t)n * sizeof(RgMap));
    long long vcap = 0;
    if (po && max_regions > 0) {                                       // no polygon has more vertices than twice the map's corners
        for (int k = 0; k < n; ++k) vcap += 2ll * (H[g0 + k] + 1) * (W[g0 + k] + 1);
        vcap = std::min<long long>(vcap, std::max<int64_t>(po->cap - po->need, 0));
    }
    const size_t rows_n = (size_t)n * max_regions;
    Bump hp{tab_b};                                                    // the page-locked records: table, counts, rows, vertex counts, offsets, map records
    const size_t p_cnt = hp.take((size_t)n * 4), p_rows = hp.take(rows_n * RG_ROW_INTS * 4), p_nv = hp.take(po ? rows_n * 8 : 0),
                 p_voff = hp.take(po ? rows_n * 8 : 0), p_mapv = hp.take(po ? (size_t)n * RG_MAPV * 8 : 0);
    PSEG_TRY(ws.pin.ensure(hp.off, "text regions records"));
    RgMap* const h_tab = ws.pin.as<RgMap>();
    RgLay lay;
    PSEG_TRY(rg_plan(n, H + g0, W + g0, how + g0, max_regions, po != nullptr, vcap, 0, h_tab, lay));
    Bump at{lay.bytes};                                                // the label maps' bytes behind the stage's workspace
    std::vector<size_t> lab_off(n);
    for (int k = 0; k < n; ++k) lab_off[k] = at.take((size_t)H[g0 + k] * W[g0 + k]);
    PSEG_TRY(ws.dev.ensure(at.off, "text regions workspace"));
    if (!ws.st) PSEG_HIP(hipStreamCreateWithFlags(&ws.st, hipStreamNonBlocking));
    hipStream_t st = ws.st;
    uint8_t* const d = ws.dev.p;
    for (int k = 0; k < n; ++k) {
        h_tab[k].lab = (unsigned long long)(uintptr_t)(d + lab_off[k]);
        h_tab[k].want_mask = out_mask && out_mask[g0 + k];
    }
    GroupDrain drain{st};
    for (int k = 0; k < n; ++k)
        PSEG_HIP(hipMemcpyAsync(d + lab_off[k], labels[g0 + k], (size_t)h_tab[k].H * h_tab[k].W, hipMemcpyHostToDevice, st));
    PSEG_TRY(rg_enqueue(st, d, h_tab, lay, n, max_regions));
    for (int k = 0; k < n; ++k)
        if (h_tab[k].want_mask)
            PSEG_HIP(hipMemcpyAsync(out_mask[g0 + k], d + lab_off[k], (size_t)h_tab[k].H * h_tab[k].W, hipMemcpyDeviceToHost, st));
    int* const h_cnt = (int*)(ws.pin.p + p_cnt);
    int* const h_rows = (int*)(ws.pin.p + p_rows);
    const long long* const h_nv = (const long long*)(ws.pin.p + p_nv);
    const long long* const h_voff = (const long long*)(ws.pin.p + p_voff);
    const long long* const h_mapv = (const long long*)(ws.pin.p + p_mapv);
    PSEG_HIP(hipMemcpyAsync(h_cnt, d + lay.cnt, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (max_regions > 0 && out_table)
        PSEG_HIP(hipMemcpyAsync(h_rows, d + lay.rows, rows_n * RG_ROW_INTS * 4, hipMemcpyDeviceToHost, st));
    if (po && max_regions > 0) PSEG_HIP(hipMemcpyAsync((void*)h_mapv, d + lay.mapv, (size_t)n * RG_MAPV * 8, hipMemcpyDeviceToHost, st));
    PSEG_HIP(hipStreamSynchronize(st));                                // the group's one wait (a polygon call: one more for the vertices)
    const int32_t* h_xy = nullptr;
    if (po && max_regions > 0) {
        long long gtot = 0;
        for (int k = 0; k < n; ++k) gtot += h_mapv[(size_t)k * RG_MAPV];
        if (gtot > 0 && gtot <= vcap) {                                // exactly what the group holds: per map its rows' counts and offsets, then the vertices
            PSEG_TRY(ws.pinv.ensure((size_t)gtot * 8, "text regions vertices"));
            for (int k = 0; k < n; ++k) {
                const int c = h_cnt[k];
                if (c <= 0 || c > max_regions) continue;
                const size_t o = (size_t)k * max_regions * 8;
                PSEG_HIP(hipMemcpyAsync((uint8_t*)h_nv + o, d + lay.nv + o, (size_t)c * 8, hipMemcpyDeviceToHost, st));
                PSEG_HIP(hipMemcpyAsync((uint8_t*)h_voff + o, d + lay.voff + o, (size_t)c * 8, hipMemcpyDeviceToHost, st));
            }
            PSEG_HIP(hipMemcpyAsync(ws.pinv.p, d + lay.xy, (size_t)gtot * 8, hipMemcpyDeviceToHost, st));
            PSEG_HIP(hipStreamSynchronize(st));
            h_xy = (const int32_t*)ws.pinv.p;
        }
    }
    drain.armed = false;
    for (int k = 0; k < n; ++k) {
        const int c = h_cnt[k];
        out_count[g0 + k] = c;
        const bool rows_ok = out_table && c <= max_regions && c > 0;
        int* const src = h_rows + (size_t)k * max_regions * RG_ROW_INTS;
        if (rows_ok) {
            if (po) for (int j = 0; j < c; ++j) src[(size_t)j * RG_ROW_INTS + 7] = j;   // the sort carries a row's place along
            rg_sort_rows(src, c);
        }
        if (po) {
            const long long* const mv = h_mapv + (size_t)k * RG_MAPV;
            const int stt = c > max_regions ? (int)PSEG_EUNSUPPORTED : max_regions > 0 ? (int)mv[2] : (int)PSEG_OK;
            rg_poly_map(*po, g0 + k, max_regions, src, rows_ok ? c : 0, stt, (max_regions > 0 && stt == PSEG_OK) ? mv[0] : 0, [&](int j, long long* nv) {
                const size_t t = (size_t)k * max_regions + j;
                *nv = h_xy ? h_nv[t] : 0;
                return h_xy ? h_xy + 2 * h_voff[t] : nullptr;
            });
        }
        if (rows_ok) std::memcpy(out_table + (size_t)(g0 + k) * max_regions * RG_ROW_INTS, src, (size_t)c * RG_ROW_INTS * 4);
    }
    return PSEG_OK;
}

// ---- the stage as the page chain sees it (pseg_regions.h) ---------------------------------------------------------------------------
int rg_stage_check(const pseg_regions& how, const char* what, int i) {
    if (how.label < 0 || how.label > 255) return fail(PSEG_EINVAL, "%s %d: label %d outside 0..255", what, i, how.label);
    const int k[3] = {how.k_close, how.k_open, how.k_join};
    for (int j = 0; j < 3; ++j)
        if (!rg_side_ok(k[j])) return fail(PSEG_EINVAL, "%s %d: side %d outside 1..%d", what, i, k[j], RG_SIDE_MAX);
    return PSEG_OK;
}
static void rg_stage_lay(const RgLay& lay, int n, RgStageLay* out) {
    out->cnt = lay.cnt; out->rows = lay.rows; out->nv = lay.nv; out->voff = lay.voff; out->mapv = lay.mapv; out->xy = lay.xy;
    out->bytes = lay.bytes; out->tab_bytes = up256((size_t)n * sizeof(RgMap));
}
int rg_stage_plan(int n, const int* H, const int* W, int max_regions, long long max_vertices, RgStageLay* out) {
    std::vector<RgMap> tab(up256((size_t)n * sizeof(RgMap)) / sizeof(RgMap) + 1);
    RgLay lay;
    PSEG_TRY(rg_plan(n, H, W, nullptr, max_regions, 1, max_vertices, 1, tab.data(), lay));
    rg_stage_lay(lay, n, out);
    return PSEG_OK;
}
int rg_stage_enqueue(hipStream_t st, uint8_t* d, void* h_tab, int n, const uint8_t* const* d_labels, const int* H, const int* W,
                     const pseg_regions* how, int max_regions, long long max_vertices, size_t d_cap, size_t h_cap, RgStageLay* out) {
    RgLay lay;
    RgMap* const tab = (RgMap*)h_tab;
    if (up256((size_t)n * sizeof(RgMap)) > h_cap) return fail(PSEG_EHIP, "regions stage: a table of %d maps does not fit %zu page-locked bytes", n, h_cap);
    PSEG_TRY(rg_plan(n, H, W, how, max_regions, 1, max_vertices, 1, tab, lay));
    if (lay.bytes > d_cap) return fail(PSEG_EHIP, "regions stage: %zu bytes of workspace, %zu reserved", lay.bytes, d_cap);   // before anything is launched
    for (int k = 0; k < n; ++k) tab[k].lab = (unsigned long long)(uintptr_t)d_labels[k];
    rg_stage_lay(lay, n, out);
    return rg_enqueue(st, d, tab, lay, n, max_regions);
}
// One page's blob from what the stage left (pseg.h, pseg_predict_chain_pages_regions_png): rows, nv and voff are the page's first
// min(count, max_regions) entries in the order the device appended them (rows is sorted here), xy the page's vertices, base its first
// vertex in the group's array.
void rg_stage_blob(int count, int max_regions, long long max_vertices, const long long* mapv, int32_t* rows, const long long* nv,
                   const long long* voff, const int32_t* xy, std::vector<int32_t>& blob) {
    const long long tot = mapv[0], base = mapv[1];
    const int st = count > max_regions ? (int)PSEG_EUNSUPPORTED : mapv[2] != PSEG_OK ? (int)mapv[2] : tot > max_vertices ? (int)PSEG_ENOMEM : (int)PSEG_OK;
    blob.assign(4, 0);
    blob[0] = count; blob[1] = (int32_t)tot; blob[2] = st;
    if (count > max_regions || count <= 0) return;
    for (int j = 0; j < count; ++j) rows[(size_t)j * RG_ROW_INTS + 7] = j;
    rg_sort_rows(rows, count);
    std::vector<int> perm(count);
    for (int j = 0; j < count; ++j) { perm[j] = rows[(size_t)j * RG_ROW_INTS + 7]; rows[(size_t)j * RG_ROW_INTS + 7] = 0; }
    blob.insert(blob.end(), rows, rows + (size_t)count * RG_ROW_INTS);
    if (st != PSEG_OK) return;
    const size_t o_first = blob.size();
    blob.resize(o_first + count + 1 + 2 * (size_t)tot);
    int32_t* const first = blob.data() + o_first;
    int32_t* const out = first + count + 1;
    long long run = 0;
    for (int j = 0; j < count; ++j) {
        const int s = perm[j];
        first[j] = (int32_t)run;
        std::memcpy(out + 2 * run, xy + 2 * (voff[s] - base), (size_t)nv[s] * 8);
        run += nv[s];
    }
    first[count] = (int32_t)run;
}

// what both list entries refuse, before any work
static int rg_check_list(int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how, int max_regions,
                         const int32_t* out_table, const int* out_count) {
    if (n < 0 || !labels || !H || !W || !how || !out_count) return fail(PSEG_EINVAL, n < 0 ? "negative map count" : "NULL argument");
    if (max_regions < 0 || (max_regions > 0 && !out_table)) return fail(PSEG_EINVAL, "max_regions %d with %s table", max_regions, out_table ? "a" : "no");
    if ((int64_t)max_regions * n * RG_ROW_INTS > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "a table of %d rows for each of %d maps is too large", max_regions, n);
    for (int i = 0; i < n; ++i) {
        if (!labels[i]) return fail(PSEG_EINVAL, "map %d: NULL argument", i);
        if (H[i] <= 0 || W[i] <= 0) return fail(PSEG_EINVAL, "map %d: empty image (%d,%d)", i, H[i], W[i]);
        if ((int64_t)H[i] * W[i] > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "map %d: image too large", i);
        PSEG_TRY(rg_stage_check(how[i], "map", i));
    }
    return PSEG_OK;
}

// ---- the host entry: the same planes and the same x pass, a plain y pass, a two-pass union-find over the whole page ------------------
static void rg_host_op(const std::vector<rg_word>& src, std::vector<rg_word>& dst, int H, int W, int k, bool ero) {
    const int wpr = rg_words(W);
    std::vector<rg_word> mid((size_t)H * wpr);
    for (int y = 0; y < H; ++y)
        for (int j = 0; j < wpr; ++j) mid[(size_t)y * wpr + j] = rg_xpass(src.data() + (size_t)y * wpr, wpr, W, j, k, ero);
    dst.assign((size_t)H * wpr, 0ull);
    for (int y = 0; y < H; ++y) {
        const int yf = rg_band_first(y, k);
        for (int j = 0; j < wpr; ++j) {
            rg_word v = 0ull;
            for (int d = 0; d < k; ++d) {
                const int yy = yf + d;
                if (yy >= 0 && yy < H) v |= mid[(size_t)yy * wpr + j];
            }
            dst[(size_t)y * wpr + j] = rg_store(v, W, j, ero);
        }
    }
}
static int rg_host_find(std::vector<int>& p, int x) {
    int r = x;
    while (p[r] != r) r = p[r];
    while (p[x] != r) { const int nx = p[x]; p[x] = r; x = nx; }
    return r;
}
// 4-connected components of the non-zero bytes: lab (class root per pixel, -1 elsewhere) and the parent array
static void rg_host_label(const std::vector<uint8_t>& px, int H, int W, std::vector<int>& lab, std::vector<int>& par) {
    lab.assign(px.size(), -1);
    par.clear();
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t o = (size_t)y * W + x;
            if (!px[o]) continue;
            int l = -1;
            if (x > 0 && lab[o - 1] >= 0) l = rg_host_find(par, lab[o - 1]);
            if (y > 0 && lab[o - W] >= 0) {
                const int r = rg_host_find(par, lab[o - W]);
                if (l < 0) l = r;
                else if (r != l) { const int a = std::min(l, r), b = std::max(l, r); par[b] = a; l = a; }
            }
            if (l < 0) { l = (int)par.size(); par.push_back(l); }
            lab[o] = l;
        }
    for (size_t o = 0; o < px.size(); ++o)
        if (lab[o] >= 0) lab[o] = rg_host_find(par, lab[o]);
}
static void rg_host_one(const uint8_t* labels, int H, int W, const pseg_regions& how, uint8_t* out_mask, int max_regions, int32_t* table, int* count,
                        std::vector<rg_word>* plane_T = nullptr) {
    const int wpr = rg_words(W);
    const size_t px = (size_t)H * W;
    std::vector<rg_word> A((size_t)H * wpr, 0ull), B, C;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if ((int)labels[(size_t)y * W + x] == how.label) A[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
    const int k[3] = {how.k_close, how.k_open, how.k_join};
    rg_host_op(A, B, H, W, k[0], false);
    rg_host_op(B, A, H, W, k[0], true);
    rg_host_op(A, B, H, W, k[1], true);
    rg_host_op(B, A, H, W, k[1], false);                               // A: m3
    rg_host_op(A, B, H, W, k[2], false);
    rg_host_op(B, C, H, W, k[2], false);
    rg_host_op(C, B, H, W, k[2], true);                                // B: the joined plane
    std::vector<uint8_t> bg(px), T(px);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t w = (size_t)y * wpr + (x >> 6);
            bg[(size_t)y * W + x] = !((B[w] >> (x & 63)) & 1ull);
            T[(size_t)y * W + x] = (uint8_t)(((A[w] | B[w]) >> (x & 63)) & 1ull);
        }
    std::vector<int> lab, par;
    rg_host_label(bg, H, W, lab, par);
    std::vector<uint8_t> edge(par.size(), 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t o = (size_t)y * W + x;
            if (lab[o] >= 0 && (y == 0 || y == H - 1 || x == 0 || x == W - 1)) edge[lab[o]] = 1;
        }
    for (size_t o = 0; o < px; ++o)
        if (lab[o] >= 0 && !edge[lab[o]]) T[o] = 1;
    rg_host_label(T, H, W, lab, par);
    // the classes in raster order of their first pixel: the rows come out sorted by seed
    std::vector<int> row_of(par.size(), -1);
    std::vector<int32_t> rows;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int l = lab[(size_t)y * W + x];
            if (l < 0) continue;
            if (row_of[l] < 0) {
                row_of[l] = (int)(rows.size() / RG_ROW_INTS);
                const int32_t r[RG_ROW_INTS] = {x, y, x + 1, y + 1, 0, y, x, 0};
                rows.insert(rows.end(), r, r + RG_ROW_INTS);
            }
            int32_t* const r = rows.data() + (size_t)row_of[l] * RG_ROW_INTS;
            r[0] = std::min(r[0], x); r[2] = std::max(r[2], x + 1); r[3] = std::max(r[3], y + 1); ++r[4];
        }
    const int c = (int)(rows.size() / RG_ROW_INTS);
    *count = c;
    if (table && c <= max_regions && c > 0) std::memcpy(table, rows.data(), rows.size() * 4);
    if (out_mask) std::memcpy(out_mask, T.data(), px);
    if (plane_T) {                                                     // T as the device leaves it: a canonical bit plane
        plane_T->assign((size_t)H * wpr, 0ull);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (T[(size_t)y * W + x]) (*plane_T)[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
    }
}

// ---- the crack polygon of a region: its outer boundary along pixel edges, clockwise from the seed's top-left corner -----------------
// At a corner, heading d, `right` is the pixel ahead on the region's side and `left` the one ahead on the other side: right unset ->
// turn right (also when left is set: pixels that meet only diagonally stay apart); both set -> turn left; else straight on.
// Returns the number of vertices (direction changes), or -1 when the walk does not close within its bound; xy may be NULL (count only).
static long long rg_trace_one(const uint8_t* mask, int H, int W, int sx, int sy, int32_t* xy) {
    static const int DX[4] = {1, 0, -1, 0}, DY[4] = {0, 1, 0, -1};     // east, south, west, north (y grows downwards)
    auto at = [&](int x, int y) { return x >= 0 && x < W && y >= 0 && y < H && mask[(size_t)y * W + x] != 0; };
    int vx = sx, vy = sy, d = 3;                                       // arriving at the start corner heading north
    long long nv = 0;
    const long long bound = 4ll * ((long long)H + 1) * ((long long)W + 1) + 4;
    for (long long it = 0; it < bound; ++it) {
        int rx, ry, lx, ly;
        switch (d) {
            case 0: rx = vx; ry = vy; lx = vx; ly = vy - 1; break;
            case 1: rx = vx - 1; ry = vy; lx = vx; ly = vy; break;
            case 2: rx = vx - 1; ry = vy - 1; lx = vx - 1; ly = vy; break;
            default: rx = vx; ry = vy - 1; lx = vx - 1; ly = vy - 1; break;
        }
        const int nd = !at(rx, ry) ? ((d + 1) & 3) : at(lx, ly) ? ((d + 3) & 3) : d;
        if (nd != d) {
            if (xy) { xy[2 * nv] = vx; xy[2 * nv + 1] = vy; }
            ++nv;
        }
        d = nd;
        vx += DX[d]; vy += DY[d];
        if (vx == sx && vy == sy) return nv;
    }
    return -1;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_text_regions(int device, int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                      uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(rg_check_list(n, labels, H, W, how, max_regions, out_table, out_count));
    return run_list(g_rg, device, n, [&](int i) { return (size_t)H[i] * W[i]; }, [&](RgWs& ws, int g0, int g1) {
        return rg_group(ws, g0, g1, labels, H, W, how, out_mask, max_regions, out_table, out_count, nullptr);
    });
}

int pseg_text_regions_host(int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                           uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(rg_check_list(n, labels, H, W, how, max_regions, out_table, out_count));
    for (int i = 0; i < n; ++i)
        rg_host_one(labels[i], H[i], W[i], how[i], out_mask ? out_mask[i] : nullptr, max_regions,
                    out_table ? out_table + (size_t)i * max_regions * RG_ROW_INTS : nullptr, &out_count[i]);
    return PSEG_OK;
}

}  // extern "C"

namespace pseg {

static int rg_check_poly(int n, const int32_t* xy, int64_t cap, const int64_t* first, const int* status) {
    if (n > 0 && (!first || !status)) return fail(PSEG_EINVAL, "NULL argument");
    if (cap < 0 || (cap > 0 && !xy)) return fail(PSEG_EINVAL, "a vertex capacity of %lld with %s array", (long long)cap, xy ? "an" : "no");
    return PSEG_OK;
}
static void rg_poly_begin(RgPolyOut& po, int n, int max_regions, int64_t cap) {
    po.cap = cap;
    po.first.assign((size_t)n * (max_regions + 1), 0);
    po.status.assign(n, PSEG_OK);
}
// the capacity protocol: too small -> the needed total in the last offset, no vertex and no other offset
static void rg_poly_deliver(const RgPolyOut& po, int n, int max_regions, int32_t* xy, int64_t* first, int* status) {
    std::memcpy(status, po.status.data(), (size_t)n * sizeof(int));
    if (po.need > po.cap) {
        first[(size_t)n * (max_regions + 1) - 1] = po.need;
        return;
    }
    if (!po.xy.empty()) std::memcpy(xy, po.xy.data(), po.xy.size() * 4);
    std::memcpy(first, po.first.data(), po.first.size() * 8);
}

}  // namespace pseg

extern "C" {

int pseg_text_regions_poly(int device, int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                           uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count,
                           int32_t* xy, int64_t cap, int64_t* first, int* status) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(rg_check_list(n, labels, H, W, how, max_regions, out_table, out_count));
    PSEG_TRY(rg_check_poly(n, xy, cap, first, status));
    RgPolyOut po;
    rg_poly_begin(po, n, max_regions, cap);
    PSEG_TRY(run_list(g_rg, device, n, [&](int i) { return (size_t)H[i] * W[i]; }, [&](RgWs& ws, int g0, int g1) {
        return rg_group(ws, g0, g1, labels, H, W, how, out_mask, max_regions, out_table, out_count, &po);
    }));
    rg_poly_deliver(po, n, max_regions, xy, first, status);
    return PSEG_OK;
}

int pseg_text_regions_poly_host(int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                                uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count,
                                int32_t* xy, int64_t cap, int64_t* first, int* status) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(rg_check_list(n, labels, H, W, how, max_regions, out_table, out_count));
    PSEG_TRY(rg_check_poly(n, xy, cap, first, status));
    RgPolyOut po;
    rg_poly_begin(po, n, max_regions, cap);
    std::vector<rg_word> T;
    std::vector<int32_t> rows, seg;
    std::vector<long long> nv, off;
    for (int i = 0; i < n; ++i) {
        int32_t* const tb = out_table ? out_table + (size_t)i * max_regions * RG_ROW_INTS : nullptr;
        rg_host_one(labels[i], H[i], W[i], how[i], out_mask ? out_mask[i] : nullptr, max_regions, tb, &out_count[i], &T);
        const int c = out_count[i], wpr = rg_words(W[i]);
        const bool rows_ok = tb && c <= max_regions && c > 0;
        int st = c > max_regions ? PSEG_EUNSUPPORTED : PSEG_OK;
        rows.assign(tb, tb + (rows_ok ? (size_t)c * RG_ROW_INTS : 0));
        nv.assign(rows_ok ? c : 0, 0);
        off.assign(rows_ok ? c + 1 : 1, 0);
        for (int j = 0; rows_ok && j < c; ++j) {
            nv[j] = rg_trace_words(T.data(), H[i], W[i], wpr, rows[(size_t)j * RG_ROW_INTS + 6], rows[(size_t)j * RG_ROW_INTS + 5], nullptr, 0);
            if (nv[j] < 0) st = PSEG_EHIP;
            off[j + 1] = off[j] + (nv[j] < 0 ? 0 : nv[j]);
            rows[(size_t)j * RG_ROW_INTS + 7] = j;
        }
        const long long tot = st == PSEG_OK ? off.back() : 0;
        const bool fits = st == PSEG_OK && po.need + tot <= po.cap;
        seg.assign(fits ? (size_t)tot * 2 : 0, 0);                     // exactly the map's vertices
        for (int j = 0; fits && j < c; ++j)
            (void)rg_trace_words(T.data(), H[i], W[i], wpr, rows[(size_t)j * RG_ROW_INTS + 6], rows[(size_t)j * RG_ROW_INTS + 5], seg.data() + 2 * off[j], nv[j]);
        rg_poly_map(po, i, max_regions, rows.data(), rows_ok ? c : 0, st, tot, [&](int j, long long* cnt) {
            *cnt = fits ? nv[j] : 0;
            return fits ? seg.data() + 2 * off[j] : (const int32_t*)nullptr;
        });
    }
    rg_poly_deliver(po, n, max_regions, xy, first, status);
    return PSEG_OK;
}

int pseg_regions_geometry(int* word, int* band, int* band_words, int* tile_h, int* tile_w, int* slots) {
    if (word) *word = 64;
    if (band) *band = RG_BAND;
    if (band_words) *band_words = RG_WC;
    if (tile_h) *tile_h = RG_TH;
    if (tile_w) *tile_w = RG_TW;
    if (slots) *slots = RG_SLOTS;
    return PSEG_OK;
}

int pseg_trace_regions_host(const uint8_t* mask, int H, int W, int n_regions, const int32_t* table, int32_t* xy, int64_t cap, int64_t* first) {
    if (!mask || !first || n_regions < 0 || (n_regions > 0 && !table) || cap < 0 || (cap > 0 && !xy)) return fail(PSEG_EINVAL, "NULL or negative argument");
    if (H <= 0 || W <= 0) return fail(PSEG_EINVAL, "empty image (%d,%d)", H, W);
    if ((int64_t)H * W > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "image too large");
    std::vector<int64_t> off((size_t)n_regions + 1, 0);
    for (int i = 0; i < n_regions; ++i) {
        const int sy = table[(size_t)i * RG_ROW_INTS + 5], sx = table[(size_t)i * RG_ROW_INTS + 6];
        if (sy < 0 || sy >= H || sx < 0 || sx >= W || !mask[(size_t)sy * W + sx] || (sx > 0 && mask[(size_t)sy * W + sx - 1]) ||
            (sy > 0 && mask[(size_t)(sy - 1) * W + sx]))
            return fail(PSEG_EINVAL, "region %d: (%d,%d) is not the seed of a region of this mask", i, sy, sx);
        const long long nv = rg_trace_one(mask, H, W, sx, sy, nullptr);
        if (nv < 0) return fail(PSEG_EINVAL, "region %d: the boundary does not close", i);
        off[i + 1] = off[i] + nv;
    }
    if (off[n_regions] > cap) {                                        // too small: the needed size, no vertex
        first[n_regions] = off[n_regions];
        return PSEG_OK;
    }
    for (int i = 0; i < n_regions; ++i)
        (void)rg_trace_one(mask, H, W, table[(size_t)i * RG_ROW_INTS + 6], table[(size_t)i * RG_ROW_INTS + 5], xy + 2 * off[i]);
    for (int i = 0; i <= n_regions; ++i) first[i] = off[i];
    return PSEG_OK;
}

}  // extern "C"
