// pseg_despeckle.hip -- small ink components erased from a list of ink maps in one device-resident call: every
// component (connectivity 4 or 8) of at most max_area pixels becomes paper, every other ink pixel becomes 1.
//
// The scheme is the page scorer's (pseg_evalpages.hip) with one counter per component and an ink map written back: a
// workgroup labels the runs of a 32 x 64 tile in LDS; a component with no ink neighbour across the tile's edge is CLOSED, is decided
// on the spot and, where it is a speck, cleared in the workgroup's own tile; an OPEN one takes one of the tile's 192 root slots
// (parent + a 32-bit size), its runs go to the tile's run list, and three small launches join the slots across tile edges, add the
// sizes of redirected slots to their final root, and clear the listed runs whose final root is a speck.  The map is worked on in
// place: a tile only ever writes bytes of its own 32 x 64 pixels, byte by byte, and a ring pixel that a neighbour may already have
// cleared never decides anything (DESIGN.md 5k has the argument).
//
// Every loop bound below is an argument, a constant or a table entry the host built; every find / unite loop is bounded (parents only
// ever decrease, so a chain is shorter than the index space, and the larger root of a union strictly decreases from try to try).
#include <algorithm>
#include <cstring>
#include <vector>

#include "pseg_list.h"
#include "pseg_despeckle.h"

namespace pseg {

constexpr int DS_TH = 32, DS_TW = 64;
constexpr int DS_OPEN_MAX = 2 * (DS_TH + DS_TW);   // an open root owns at least one pixel of the tile's rim (188 pixels)
constexpr int DS_RUN_MAX = DS_TH * DS_TW / 2;      // runs of a tile: at most every other pixel starts one
constexpr int DS_HALF = DS_RUN_MAX / 2;            // 16-bit sizes, two runs to a word (a tile has 2 048 pixels: no carry crosses)
// rim table of a tile: slot of the root of the pixel at [0, 64) top row, [64, 128) bottom row, [128, 160) left column, [160, 192) right column
constexpr int DS_RIM = 2 * (DS_TH + DS_TW);
// border unions a tile lists: <= 64 starts of ink above the (widened) spans of its top row, <= 96 pixel pairs across its left edge, 2 corners
constexpr int DS_TASK_MAX = 192;
static_assert(DS_OPEN_MAX <= 256, "a slot is a byte of the rim table and eight bits of a run word");

// one despeckled map of a group: tile0 is the prefix table of the ragged launches (the tile workgroups in front of it)
struct DsMap {
    int H, W, tiles_x, tile0, max_area, pad[3];
    unsigned long long off;                        // the map's bytes in the group's buffer, 256-byte aligned
};

__device__ __forceinline__ int ds_map_of(const DsMap* __restrict__ tab, int n, int b) {
    int lo = 0, hi = n - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {   // largest i with tab[i].tile0 <= b
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].tile0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- union-find: LDS (run indices of a tile) and global (root slot ids of a group) -----------------------------------------------
// Links only ever point at a smaller index of the same component, so a chain has fewer hops than the index space: `cap`.
__device__ __forceinline__ int ds_lds_find(const int* lab, int x) {
    for (int it = 0; it < DS_RUN_MAX; ++it) {
        const int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) break;
        x = p;
    }
    return x;
}
// a lost atomicMin hands back a link below the larger root: max(a, b) strictly decreases, DS_RUN_MAX tries at the very most
__device__ __forceinline__ void ds_lds_union(int* lab, int a, int b) {
    for (int it = 0; it < DS_RUN_MAX; ++it) {
        a = ds_lds_find(lab, a);
        b = ds_lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}
// path halving: a halving store replaces a non-root's link by one further up its own chain
__device__ __forceinline__ int ds_find(int* L, int x, int cap) {
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
// the root of x once every union is over, without a store.  The merge launch points a redirected slot straight at its final root, but
// a halving store of another wave's find may land after that store and leave a link further down the chain: a link is followed, never
// taken for the root.
__device__ __forceinline__ int ds_root(const int* __restrict__ L, int x, int cap) {
    for (int it = 0; it < cap; ++it) {
        const int p = L[x];
        if (p == x || p < 0 || p >= cap) break;
        x = p;
    }
    return x;
}
__device__ __forceinline__ void ds_union(int* L, int a, int b, int cap) {
    for (int it = 0; it < cap; ++it) {
        a = ds_find(L, a, cap);
        b = ds_find(L, b, cap);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ unsigned long long ds_le(int b) { return b >= 63 ? ~0ull : ((2ull << b) - 1ull); }   // bits 0 .. b
// the columns a run [s0, e] touches in the row above / below: itself, for connectivity 8 one more to either side
template <bool C8>
__device__ __forceinline__ unsigned long long ds_reach(unsigned long long S) { return C8 ? (S | (S << 1) | (S >> 1)) : S; }
// the rows of the column beside the tile that pixel (r, edge column) touches
template <bool C8>
__device__ __forceinline__ unsigned ds_reach_rows(int r) { const unsigned b = 1u << r; return C8 ? (b | (b << 1) | (b >> 1)) : b; }

// One workgroup per (map, 32 x 64 tile); `tile_base` is the first tile of this launch (the maps of either connectivity are
// consecutive in the table).  n_maps == 0: the one map `one` of the scan chain's front end, which has no table on the device.  The map is read once and becomes bit rows; a tile is then its run list (row | first lane << 5 | last
// lane << 11, ordered by row and column); runs are joined with the runs of the row above that they touch; a component's size is the
// sum of its runs' lengths.  Closed specks are cleared here, every other ink byte of the tile that is not 1 becomes 1; an open root
// takes a slot, and its runs (| slot << 17) go to the tile's run list.  rec: per map the erased components, the erased pixels, the
// kept components.
template <bool C8>
__global__ __launch_bounds__(256) void ds_tile_kernel(uint8_t* buf, const DsMap* __restrict__ tab, int n_maps, DsMap one, int tile_base,
                                                      int* __restrict__ P, unsigned* __restrict__ size_g, uint8_t* __restrict__ rimtab,
                                                      unsigned* __restrict__ tasks, unsigned* __restrict__ runs, int* __restrict__ rootn,
                                                      int* __restrict__ taskn, int* __restrict__ runn, unsigned long long* __restrict__ rec) {
    constexpr int NTH = 256, RPW = DS_TH / 4;
    __shared__ unsigned long long ink[DS_TH + 2];                      // ink of tile rows -1 .. DS_TH
    __shared__ unsigned long long clr[DS_TH];                          // the pixels of closed specks
    __shared__ unsigned lr[2], cor[2];                                 // ink left / right of the tile (bit = row); beside the row above / below: bit 0 left, 1 right
    __shared__ int rowcnt[DS_TH], rowbase[DS_TH + 1];
    __shared__ unsigned rl[DS_RUN_MAX];                                // the runs (| an open root's slot << 17)
    __shared__ int parent[DS_RUN_MAX];
    __shared__ unsigned csz[DS_HALF];                                  // sizes
    __shared__ unsigned openbits[DS_RUN_MAX / 32], specbits[DS_RUN_MAX / 32];
    __shared__ unsigned cnt[3];
    __shared__ int nopen, ntask, nrun;
    const int tile = tile_base + (int)blockIdx.x;
    const int pi = n_maps > 0 ? ds_map_of(tab, n_maps, tile) : 0;
    const DsMap pg = n_maps > 0 ? tab[pi] : one;
    const int H = pg.H, W = pg.W;
    const int lt = tile - pg.tile0, ty = lt / pg.tiles_x, tx = lt - ty * pg.tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y0 = ty * DS_TH, x0 = tx * DS_TW, x = x0 + lane;
    const int rw0 = wave * RPW;
    uint8_t* const img = buf + pg.off;
    for (int i = threadIdx.x; i < DS_HALF; i += NTH) csz[i] = 0;
    if (threadIdx.x < DS_RUN_MAX / 32) { openbits[threadIdx.x] = 0; specbits[threadIdx.x] = 0; }
    if (threadIdx.x < DS_TH) clr[threadIdx.x] = 0;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) { nopen = 0; ntask = 0; nrun = 0; }
    // ---- the map -> bit rows; waves 0, 1 also fetch the row above / below the tile (and the two pixels beside it), waves 2, 3 the columns beside it
    unsigned long long mr[RPW], m1[RPW];                               // ink; ink whose byte is not 1
    int nruns_w = 0;
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int r = rw0 + j, y = y0 + r;
        const bool in = y < H && x < W;
        const unsigned b = in ? img[(size_t)y * W + x] : 0u;
        const unsigned long long mi = __ballot(b != 0);
        mr[j] = mi;
        m1[j] = __ballot(b > 1u);
        const int n = __popcll(mi & ~(mi << 1));
        nruns_w += n;
        if (lane == 0) { ink[r + 1] = mi; rowcnt[r] = n; }
    }
    {
        bool hv = false, hc = false;
        if (wave < 2) {
            const int y = wave == 0 ? y0 - 1 : y0 + DS_TH;
            const bool row_ok = y >= 0 && y < H;
            hv = row_ok && x < W && img[(size_t)y * W + x] != 0;
            if (C8 && lane < 2) {
                const int xx = lane == 0 ? x0 - 1 : x0 + DS_TW;
                hc = row_ok && xx >= 0 && xx < W && img[(size_t)y * W + xx] != 0;
            }
        } else {
            const int y = y0 + (lane & 31), xx = wave == 2 ? x0 - 1 : x0 + DS_TW;
            hv = lane < 32 && y < H && xx >= 0 && xx < W && img[(size_t)y * W + xx] != 0;
        }
        const unsigned long long bv = __ballot(hv), bc = __ballot(hc);
        if (lane == 0) {
            if (wave == 0) { ink[0] = bv; cor[0] = (unsigned)bc & 3u; }
            else if (wave == 1) { ink[DS_TH + 1] = bv; cor[1] = (unsigned)bc & 3u; }
            else lr[wave - 2] = (unsigned)bv;
        }
    }
    if (!__syncthreads_or(nruns_w)) {                                  // a tile of paper
        if (threadIdx.x == 0) { rootn[tile] = 0; taskn[tile] = 0; runn[tile] = 0; }
        return;
    }
    // ---- the run list, every run its own parent ----
    int excl, n_all;
    {
        const int v = lane < DS_TH ? rowcnt[lane] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < DS_TH; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        excl = inc - v;
        n_all = min(__shfl(inc, DS_TH - 1), DS_RUN_MAX);
        if (wave == 0 && lane <= DS_TH) rowbase[lane] = lane < DS_TH ? excl : n_all;
    }
    const unsigned long long le = ds_le(lane);
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
        unsigned long long ov = ds_reach<C8>(ds_le(e) & ~(ds_le(s0) >> 1)) & mp;
        const unsigned long long fmp = mp & ~(mp << 1);
        const int base = rowbase[r - 1];
        for (int it = 0; it < DS_TW / 2 + 1 && ov; ++it) {
            const int b = __builtin_ctzll(ov);
            const int u = base + __popcll(fmp & ds_le(b)) - 1;
            ds_lds_union(parent, t, u);
            ov &= ~ds_le((rl[u] >> 11) & 63);
        }
    }
    __syncthreads();
    // ---- roots, sizes, open components ----
    const unsigned long long m_up = ink[0], m_dn = ink[DS_TH + 1];
    const unsigned lr0 = lr[0], lr1 = lr[1], cup = cor[0], cdn = cor[1];
    for (int t = threadIdx.x; t < n_all; t += NTH) {
        const unsigned rc = rl[t];
        const int r = rc & 31, s0 = (rc >> 5) & 63, e = (rc >> 11) & 63;
        const unsigned long long S = ds_le(e) & ~(ds_le(s0) >> 1), Sx = ds_reach<C8>(S);
        const int rt = ds_lds_find(parent, t);
        if (rt != t) __hip_atomic_store(&parent[t], rt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (the unions are over: later phases read the root here)
        __hip_atomic_fetch_add(&csz[rt >> 1], (unsigned)(e - s0 + 1) << ((rt & 1) * 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        bool rim = false;
        if (r == 0) rim |= (Sx & m_up) != 0 || (C8 && ((s0 == 0 && (cup & 1u)) || (e == DS_TW - 1 && (cup & 2u))));
        if (r == DS_TH - 1) rim |= (Sx & m_dn) != 0 || (C8 && ((s0 == 0 && (cdn & 1u)) || (e == DS_TW - 1 && (cdn & 2u))));
        if (s0 == 0) rim |= (lr0 & ds_reach_rows<C8>(r)) != 0;
        if (e == DS_TW - 1) rim |= (lr1 & ds_reach_rows<C8>(r)) != 0;
        if (rim) atomicOr(&openbits[rt >> 5], 1u << (rt & 31));
    }
    __syncthreads();
    // ---- closed roots: decided and counted; open roots: a slot, its parent and size ----
    for (int t0 = 0; t0 < n_all; t0 += NTH) {
        const int t = t0 + threadIdx.x;
        bool open_root = false, closed_root = false;
        if (t < n_all && parent[t] == t) {
            open_root = (openbits[t >> 5] >> (t & 31)) & 1;
            closed_root = !open_root;
        }
        const unsigned sz = t < n_all ? (csz[t >> 1] >> ((t & 1) * 16)) & 0xffffu : 0u;
        const bool speck = closed_root && ds_speck(sz, pg.max_area);
        if (speck) atomicOr(&specbits[t >> 5], 1u << (t & 31));
        const unsigned long long orm = __ballot(open_root), crm = __ballot(closed_root), spm = __ballot(speck);
        if (spm) {
            unsigned px = speck ? sz : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) px += __shfl_xor(px, o);  // (at most 2 048 in all)
            if (lane == 0) { atomicAdd(&cnt[0], (unsigned)__popcll(spm)); atomicAdd(&cnt[1], px); }
        }
        if ((crm & ~spm) && lane == 0) atomicAdd(&cnt[2], (unsigned)__popcll(crm & ~spm));
        if (orm) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&nopen, __popcll(orm));
            base = __shfl(base, 0);
            if (open_root) {
                const int k = min(base + __popcll(orm & (le >> 1)), DS_OPEN_MAX - 1);   // (the slot bound holds: DESIGN.md 5k)
                const int id = tile * DS_OPEN_MAX + k;
                rl[t] |= (unsigned)k << 17;
                P[id] = id;
                size_g[id] = sz;
            }
        }
    }
    __syncthreads();
    // ---- the pixels of closed specks, row by row ----
    for (int t = threadIdx.x; t < n_all; t += NTH) {
        const int rt = parent[t];
        if (!((specbits[rt >> 5] >> (rt & 31)) & 1)) continue;
        const unsigned rc = rl[t];
        const int r = rc & 31, s0 = (rc >> 5) & 63, e = (rc >> 11) & 63;
        atomicOr(&clr[r], ds_le(e) & ~(ds_le(s0) >> 1));
    }
    __syncthreads();
    // ---- this tile's bytes: a closed speck becomes paper, any other ink 1.  Byte stores to the tile's own pixels only. ----
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int r = rw0 + j, y = y0 + r;
        if (!(y < H && x < W)) continue;
        const unsigned long long c = clr[r];
        if ((c >> lane) & 1) img[(size_t)y * W + x] = 0;
        else if ((m1[j] >> lane) & 1) img[(size_t)y * W + x] = 1;
    }
    // ---- open runs: the run list, the root's slot at their rim pixels, the unions across this tile's top and left edge ----
    // (the tiles below / right list theirs.)  slot | place in the neighbour's rim table << 8 | neighbour << 16: 0 above, 1 left,
    // 2 above left, 3 above right.  Ink that is adjacent in the neighbour's rim is one component there: one task per start of such a stretch.
    uint8_t* const rim = rimtab + (size_t)tile * DS_RIM;
    unsigned* const tk = tasks + (size_t)tile * DS_TASK_MAX;
    unsigned* const rn = runs + (size_t)tile * DS_RUN_MAX;
    for (int t = threadIdx.x; t < n_all; t += NTH) {
        const int rt = parent[t];
        if (!((openbits[rt >> 5] >> (rt & 31)) & 1)) continue;
        const unsigned rc = rl[t];
        const unsigned k = rl[rt] >> 17;
        const int r = rc & 31, s0 = (rc >> 5) & 63, e = (rc >> 11) & 63;
        const unsigned long long S = ds_le(e) & ~(ds_le(s0) >> 1), Sx = ds_reach<C8>(S);
        {
            const int i = atomicAdd(&nrun, 1);
            if (i < DS_RUN_MAX) rn[i] = (rc & 0x1ffffu) | k << 17;
        }
        if (r == 0) for (int b = s0; b <= e; ++b) rim[b] = (uint8_t)k;
        if (r == DS_TH - 1) for (int b = s0; b <= e; ++b) rim[DS_TW + b] = (uint8_t)k;
        if (s0 == 0) rim[2 * DS_TW + r] = (uint8_t)k;
        if (e == DS_TW - 1) rim[2 * DS_TW + DS_TH + r] = (uint8_t)k;
        if (r == 0) {
            const unsigned long long w = Sx & m_up;
            unsigned long long st = w & ~(w << 1);
            for (int it = 0; it < DS_TW / 2 + 1 && st; ++it) {
                const int i = atomicAdd(&ntask, 1);
                if (i < DS_TASK_MAX) tk[i] = k | (unsigned)(DS_TW + __builtin_ctzll(st)) << 8;
                st &= st - 1;
            }
            if (C8 && s0 == 0 && (cup & 1u)) {
                const int i = atomicAdd(&ntask, 1);
                if (i < DS_TASK_MAX) tk[i] = k | (unsigned)(DS_TW + DS_TW - 1) << 8 | 2u << 16;
            }
            if (C8 && e == DS_TW - 1 && (cup & 2u)) {
                const int i = atomicAdd(&ntask, 1);
                if (i < DS_TASK_MAX) tk[i] = k | (unsigned)DS_TW << 8 | 3u << 16;
            }
        }
        if (s0 == 0) {
            unsigned nb = lr0 & ds_reach_rows<C8>(r);
            for (int it = 0; it < 3 && nb; ++it) {
                const int i = atomicAdd(&ntask, 1);
                if (i < DS_TASK_MAX) tk[i] = k | (unsigned)(2 * DS_TW + DS_TH + __builtin_ctz(nb)) << 8 | 1u << 16;
                nb &= nb - 1;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) { rootn[tile] = min(nopen, DS_OPEN_MAX); taskn[tile] = min(ntask, DS_TASK_MAX); runn[tile] = min(nrun, DS_RUN_MAX); }
    if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&rec[(size_t)pi * 3 + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// unions of the open components across tile edges, on the root slot ids: a wave per tile takes the tile's task list and looks the
// neighbour's slot up in ITS rim table.  A slot the neighbour never handed out is skipped (cannot happen: the pixel looked up has an
// ink neighbour across its tile's edge, so its component is open there).  A neighbour is a tile of the same map: the tasks name
// pixels inside the map, and a map's tiles are consecutive.
__global__ __launch_bounds__(256) void ds_border_kernel(const DsMap* __restrict__ tab, int n_maps, int one_tiles_x, const uint8_t* __restrict__ rimtab,
                                                        const unsigned* __restrict__ tasks, const int* __restrict__ taskn,
                                                        const int* __restrict__ rootn, int* P, int tiles, int cap) {
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tiles) return;
    const int n = min(taskn[tile], DS_TASK_MAX);
    if (n == 0) return;
    const int tiles_x = n_maps > 0 ? tab[ds_map_of(tab, n_maps, tile)].tiles_x : one_tiles_x;
    for (int i = lane; i < n; i += 64) {
        const unsigned t = tasks[(size_t)tile * DS_TASK_MAX + i];
        const int k = (int)(t & 255u), place = (int)((t >> 8) & 255u), dir = (int)(t >> 16);
        const int nb = tile - (dir == 1 ? 1 : dir == 0 ? tiles_x : dir == 2 ? tiles_x + 1 : tiles_x - 1);
        if (nb < 0 || nb >= tiles || place >= DS_RIM) continue;
        const int ks = rimtab[(size_t)nb * DS_RIM + place];
        if (k >= rootn[tile] || ks >= rootn[nb]) continue;
        ds_union(P, tile * DS_OPEN_MAX + k, nb * DS_OPEN_MAX + ks, cap);
    }
}

// sizes of the root slots that a border union redirected: added to the final root's, and the slot pointed straight at it.  One wave
// per tile; the lanes that share their final root are summed first, one lane adds.  A final root's size is the pixel count of one
// component of one map, below 2^31: the 32-bit atomic add does not wrap (the lanes' sum saturates all the same).
__global__ __launch_bounds__(256) void ds_merge_kernel(int* P, unsigned* size_g, const int* __restrict__ rootn, int tiles, int cap) {
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tiles) return;
    const int n = min(rootn[tile], DS_OPEN_MAX);
    for (int base = 0; base < n; base += 64) {
        int id = 0, r = -1;
        if (base + lane < n) {
            id = tile * DS_OPEN_MAX + base + lane;
            r = ds_find(P, id, cap);
            if (r == id) r = -1;
            else __hip_atomic_store(&P[id], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (int g = 0; g < 64; ++g) {                                 // group after group of the distinct roots among the lanes
            const unsigned long long act = __ballot(r >= 0);
            if (act == 0) break;
            const int r0 = __builtin_amdgcn_readlane(r, __builtin_ctzll(act));
            const bool mine = r == r0;
            unsigned sum = mine ? size_g[id] : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum = ds_add_sat(sum, __shfl_xor(sum, o));
            if (lane == 0 && sum) atomicAdd(&size_g[r0], sum);
            if (mine) r = -1;
        }
    }
}

// every slot that is still a root is one component: counted as erased or kept; every listed run whose final root (ds_root: the links
// are at rest by now) is a speck becomes paper (byte stores to the run's own pixels, inside its tile).  One wave per tile.
__global__ __launch_bounds__(256) void ds_apply_kernel(uint8_t* buf, const DsMap* __restrict__ tab, int n_maps, DsMap one, const int* __restrict__ P,
                                                       const unsigned* __restrict__ size_g, const unsigned* __restrict__ runs,
                                                       const int* __restrict__ rootn, const int* __restrict__ runn, int tiles, int cap,
                                                       unsigned long long* __restrict__ rec) {
    const int tile = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tiles) return;
    const int n = min(rootn[tile], DS_OPEN_MAX);
    if (n == 0) return;                                                // no open root, no listed run
    const int pi = n_maps > 0 ? ds_map_of(tab, n_maps, tile) : 0;
    const DsMap pg = n_maps > 0 ? tab[pi] : one;
    unsigned ce = 0, ck = 0;
    unsigned long long pe = 0;
    for (int k = lane; k < n; k += 64) {
        const int id = tile * DS_OPEN_MAX + k;
        if (P[id] != id) continue;
        const unsigned sz = size_g[id];
        if (ds_speck(sz, pg.max_area)) { ++ce; pe += sz; } else ++ck;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ce += __shfl_xor(ce, o); ck += __shfl_xor(ck, o); pe += __shfl_xor(pe, o); }
    if (lane == 0) {
        if (ce) atomicAdd(&rec[(size_t)pi * 3], (unsigned long long)ce);
        if (pe) atomicAdd(&rec[(size_t)pi * 3 + 1], pe);
        if (ck) atomicAdd(&rec[(size_t)pi * 3 + 2], (unsigned long long)ck);
    }
    const int nr = min(runn[tile], DS_RUN_MAX);
    const int lt = tile - pg.tile0, ty = lt / pg.tiles_x, tx = lt - ty * pg.tiles_x;
    uint8_t* const img = buf + pg.off;
    for (int i = lane; i < nr; i += 64) {
        const unsigned rc = runs[(size_t)tile * DS_RUN_MAX + i];
        const int k = (int)(rc >> 17);
        if (k >= n) continue;
        const int root = ds_root(P, tile * DS_OPEN_MAX + k, cap);
        if (!ds_speck(size_g[root], pg.max_area)) continue;
        const int y = ty * DS_TH + (int)(rc & 31u), s0 = (int)((rc >> 5) & 63u), e = (int)((rc >> 11) & 63u);
        if (y >= pg.H) continue;
        for (int b = s0; b <= e; ++b) {
            const int x = tx * DS_TW + b;
            if (x < pg.W) img[(size_t)y * pg.W + x] = 0;
        }
    }
}

// ---- workspace: grow-only, one per device (table, records, the group's maps, the per-tile arrays; a page-locked copy of table and
// records), under its own lock and on its own stream; a call holds the lock to its end and every group ends synchronised.
// pseg_release_workspace frees it.
struct DsWs {
    GrowDev dev; GrowPin pin; hipStream_t st = nullptr;
    void release() {
        dev.release();
        pin.release();
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
};
static PerDevice<DsWs> g_ds;

// per tile: 192 root slots (parent + size), the rim table, the task list, the run list, three list lengths
size_t despeckle_tile_bytes() { return (size_t)DS_OPEN_MAX * 8 + DS_RIM + (size_t)DS_TASK_MAX * 4 + (size_t)DS_RUN_MAX * 4 + 12; }

// where the per-tile arrays of `tiles` tiles lie behind `base` bytes (every array starts at a multiple of 256)
struct DsLayout { size_t par, size, rim, task, run, rootn, taskn, runn, total; };
static DsLayout ds_layout(size_t base, size_t tiles) {
    DsLayout L;
    const size_t nslots = tiles * DS_OPEN_MAX;
    Bump at{base};
    L.par = at.take(nslots * 4);
    L.size = at.take(nslots * 4);
    L.rim = at.take(tiles * DS_RIM);
    L.task = at.take(tiles * DS_TASK_MAX * 4);
    L.run = at.take(tiles * DS_RUN_MAX * 4);
    L.rootn = at.take(tiles * 4);
    L.taskn = at.take(tiles * 4);
    L.runn = at.take(tiles * 4);
    L.total = at.off;
    return L;
}

// the launches over `nt` tiles, the first nt8 of them of connectivity 8: four, or five where both connectivities occur
static void ds_launch(uint8_t* d, const DsLayout& L, uint8_t* buf, const DsMap* d_tab, int n, const DsMap& one, int nt, int nt8,
                      unsigned long long* d_rec, hipStream_t st) {
    int* const d_par = (int*)(d + L.par);
    unsigned* const d_size = (unsigned*)(d + L.size);
    uint8_t* const d_rim = d + L.rim;
    unsigned* const d_task = (unsigned*)(d + L.task);
    unsigned* const d_run = (unsigned*)(d + L.run);
    int* const d_rootn = (int*)(d + L.rootn);
    int* const d_taskn = (int*)(d + L.taskn);
    int* const d_runn = (int*)(d + L.runn);
    const int cap = nt * DS_OPEN_MAX;
    if (nt8 > 0)
        ds_tile_kernel<true><<<nt8, 256, 0, st>>>(buf, d_tab, n, one, 0, d_par, d_size, d_rim, d_task, d_run, d_rootn, d_taskn, d_runn, d_rec);
    if (nt > nt8)
        ds_tile_kernel<false><<<nt - nt8, 256, 0, st>>>(buf, d_tab, n, one, nt8, d_par, d_size, d_rim, d_task, d_run, d_rootn, d_taskn, d_runn, d_rec);
    ds_border_kernel<<<cdiv(nt, 4), 256, 0, st>>>(d_tab, n, one.tiles_x, d_rim, d_task, d_taskn, d_rootn, d_par, nt, cap);
    ds_merge_kernel<<<cdiv(nt, 4), 256, 0, st>>>(d_par, d_size, d_rootn, nt, cap);
    ds_apply_kernel<<<cdiv(nt, 4), 256, 0, st>>>(buf, d_tab, n, one, d_par, d_size, d_run, d_rootn, d_runn, nt, cap, d_rec);
}

// One map on the device for the scan chain's front end: enqueued on `st` without a wait, a table or an allocation.  d_work:
// despeckle_work_bytes(H, W) bytes, 256-byte aligned (the counters, which nobody reads back, then the per-tile arrays).
static long long ds_tiles(int H, int W) { return (long long)cdiv(W, DS_TW) * cdiv(H, DS_TH); }
size_t despeckle_work_bytes(int H, int W) { return ds_layout(256, (size_t)ds_tiles(H, W)).total; }
int despeckle_enqueue(uint8_t* d_ink, int H, int W, const pseg_despeckle& how, uint8_t* d_work, hipStream_t st) {
    if (how.max_area == 0) return PSEG_OK;
    if (!d_ink || !d_work) return fail(PSEG_EINVAL, "despeckle: no ink plane or no workspace");
    const long long tiles = ds_tiles(H, W);
    if (tiles * DS_OPEN_MAX > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "despeckle: a %d x %d map has too many tiles for 32-bit slot ids", H, W);
    DsMap one;
    std::memset(&one, 0, sizeof one);
    one.H = H; one.W = W; one.max_area = how.max_area;
    one.tiles_x = cdiv(W, DS_TW);
    const int nt = (int)tiles;
    ds_launch(d_work, ds_layout(256, (size_t)tiles), d_ink, nullptr, 0, one, nt, how.connectivity == 8 ? nt : 0, (unsigned long long*)d_work, st);
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

static int ds_group(DsWs& ws, int g0, int g1, const uint8_t* const* ink, const int* H, const int* W, const pseg_despeckle* how,
                    uint8_t* const* out, int64_t* out_counts) {
    constexpr int GROUP_MAX = LIST_GROUP_ITEMS;
    constexpr size_t tab_b = up256((size_t)GROUP_MAX * sizeof(DsMap)), rec_b = up256((size_t)GROUP_MAX * 3 * 8);
    // the table: the maps of connectivity 8, then those of connectivity 4; a map that is not despeckled has no entry
    int idx[GROUP_MAX], n = 0, n8 = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = g0; i < g1 && n < GROUP_MAX; ++i)
            if (how[i].max_area != 0 && (how[i].connectivity == 8) == (pass == 0)) { idx[n++] = i; n8 += pass == 0; }
    if (n > 0) {
        PSEG_TRY(ws.pin.ensure(tab_b + rec_b, "despeckle records"));
        DsMap* const h_tab = ws.pin.as<DsMap>();
        std::memset(h_tab, 0, tab_b);
        Bump at{tab_b + rec_b};
        long long tiles = 0, tiles8 = 0;
        for (int k = 0; k < n; ++k) {
            const int i = idx[k];
            DsMap& t = h_tab[k];
            t.H = H[i]; t.W = W[i]; t.max_area = how[i].max_area;
            t.tiles_x = cdiv(W[i], DS_TW);
            t.tile0 = (int)tiles;
            t.off = at.take((size_t)H[i] * W[i]);
            tiles += (long long)t.tiles_x * cdiv(H[i], DS_TH);
            if (k < n8) tiles8 = tiles;
        }
        if (tiles * DS_OPEN_MAX > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "maps %d..%d: too many tiles for 32-bit slot ids", g0, g1 - 1);
        const DsLayout L = ds_layout(at.off, (size_t)tiles);
        PSEG_TRY(ws.dev.ensure(L.total, "despeckle workspace"));
        if (!ws.st) PSEG_HIP(hipStreamCreateWithFlags(&ws.st, hipStreamNonBlocking));
        hipStream_t st = ws.st;
        uint8_t* const d = ws.dev.p;
        const DsMap* const d_tab = (const DsMap*)d;
        unsigned long long* const d_rec = (unsigned long long*)(d + tab_b);
        GroupDrain drain{st};
        PSEG_HIP(hipMemcpyAsync(d, h_tab, (size_t)n * sizeof(DsMap), hipMemcpyHostToDevice, st));
        PSEG_HIP(hipMemsetAsync(d_rec, 0, (size_t)n * 3 * 8, st));
        for (int k = 0; k < n; ++k)
            PSEG_HIP(hipMemcpyAsync(d + h_tab[k].off, ink[idx[k]], (size_t)h_tab[k].H * h_tab[k].W, hipMemcpyHostToDevice, st));
        ds_launch(d, L, d, d_tab, n, h_tab[0], (int)tiles, (int)tiles8, d_rec, st);
        PSEG_HIP(hipGetLastError());
        for (int k = 0; k < n; ++k)
            PSEG_HIP(hipMemcpyAsync(out[idx[k]], d + h_tab[k].off, (size_t)h_tab[k].H * h_tab[k].W, hipMemcpyDeviceToHost, st));
        PSEG_HIP(hipMemcpyAsync(ws.pin.p + tab_b, d_rec, (size_t)n * 3 * 8, hipMemcpyDeviceToHost, st));
        PSEG_HIP(hipStreamSynchronize(st));                            // the group's one wait
        drain.armed = false;
        const unsigned long long* const h_rec = (const unsigned long long*)(ws.pin.p + tab_b);
        for (int k = 0; k < n && out_counts; ++k)
            for (int j = 0; j < 3; ++j) out_counts[(size_t)idx[k] * 3 + j] = (int64_t)h_rec[(size_t)k * 3 + j];
    }
    for (int i = g0; i < g1; ++i) {                                    // the maps that are not despeckled: their bytes
        if (how[i].max_area != 0) continue;
        if (out[i] != ink[i]) std::memmove(out[i], ink[i], (size_t)H[i] * W[i]);
        for (int j = 0; j < 3 && out_counts; ++j) out_counts[(size_t)i * 3 + j] = 0;
    }
    return PSEG_OK;
}

// what both list entries refuse, before any work
static int ds_check_list(int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_despeckle* how, uint8_t* const* out) {
    if (n < 0 || !ink || !H || !W || !how || !out) return fail(PSEG_EINVAL, n < 0 ? "negative map count" : "NULL argument");
    for (int i = 0; i < n; ++i) {
        if (!ink[i] || !out[i]) return fail(PSEG_EINVAL, "map %d: NULL argument", i);
        if (H[i] <= 0 || W[i] <= 0) return fail(PSEG_EINVAL, "map %d: empty image (%d,%d)", i, H[i], W[i]);
        if ((int64_t)H[i] * W[i] > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "map %d: image too large", i);
        PSEG_TRY(despeckle_check(how[i], i));
    }
    return PSEG_OK;
}

int despeckle_check(const pseg_despeckle& d, int index, const char* what) {
    if (d.max_area < 0 || d.max_area > DS_AREA_MAX) return fail(PSEG_EINVAL, "%s %d: max_area %d outside 0..%d", what, index, d.max_area, DS_AREA_MAX);
    if (d.max_area != 0 && d.connectivity != 4 && d.connectivity != 8) return fail(PSEG_EINVAL, "%s %d: connectivity %d (4 or 8)", what, index, d.connectivity);
    return PSEG_OK;
}

// one map on the host: a two-pass union-find over the page.  Pass 1 gives every ink pixel the label of a neighbour that came before
// it (left, and above: one pixel for connectivity 4, three for 8) and unites the labels that meet; pass 2 sizes the classes and writes.
static int ds_host_find(std::vector<int>& p, int x) {
    int r = x;
    while (p[r] != r) r = p[r];
    while (p[x] != r) { const int nx = p[x]; p[x] = r; x = nx; }
    return r;
}
static void ds_host_one(const uint8_t* ink, int H, int W, const pseg_despeckle& how, uint8_t* out, int64_t* counts) {
    const size_t px = (size_t)H * W;
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    if (how.max_area == 0) {
        if (out != ink) std::memmove(out, ink, px);
        return;
    }
    const bool c8 = how.connectivity == 8;
    std::vector<int> lab(px, -1), par;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t o = (size_t)y * W + x;
            if (!ink[o]) continue;
            int l = -1;
            auto meet = [&](size_t q) {
                if (lab[q] < 0) return;
                const int r = ds_host_find(par, lab[q]);
                if (l < 0) l = r;
                else if (r != l) { const int a = std::min(l, r), b = std::max(l, r); par[b] = a; l = a; }
            };
            if (x > 0) meet(o - 1);
            if (y > 0) {
                meet(o - W);
                if (c8 && x > 0) meet(o - W - 1);
                if (c8 && x + 1 < W) meet(o - W + 1);
            }
            if (l < 0) { l = (int)par.size(); par.push_back(l); }
            lab[o] = l;
        }
    std::vector<unsigned> size(par.size(), 0u);
    for (size_t o = 0; o < px; ++o)
        if (lab[o] >= 0) { lab[o] = ds_host_find(par, lab[o]); size[lab[o]] = ds_add_sat(size[lab[o]], 1u); }
    for (size_t l = 0; l < par.size() && counts; ++l) {
        if (par[l] != (int)l) continue;
        if (ds_speck(size[l], how.max_area)) { ++counts[0]; counts[1] += size[l]; } else ++counts[2];
    }
    for (size_t o = 0; o < px; ++o) out[o] = lab[o] >= 0 && !ds_speck(size[lab[o]], how.max_area);
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_despeckle_maps(int device, int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_despeckle* how,
                        uint8_t* const* out, int64_t* out_counts) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(ds_check_list(n, ink, H, W, how, out));
    return run_list(g_ds, device, n, [&](int i) { return (size_t)H[i] * W[i]; },
                    [&](DsWs& ws, int g0, int g1) { return ds_group(ws, g0, g1, ink, H, W, how, out, out_counts); });
}

int pseg_despeckle_maps_host(int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_despeckle* how,
                             uint8_t* const* out, int64_t* out_counts) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(ds_check_list(n, ink, H, W, how, out));
    for (int i = 0; i < n; ++i) ds_host_one(ink[i], H[i], W[i], how[i], out[i], out_counts ? out_counts + (size_t)i * 3 : nullptr);
    return PSEG_OK;
}

int pseg_despeckle_geometry(int* tile_h, int* tile_w, int* slots, int* run_cap) {
    if (tile_h) *tile_h = DS_TH;
    if (tile_w) *tile_w = DS_TW;
    if (slots) *slots = DS_OPEN_MAX;
    if (run_cap) *run_cap = DS_RUN_MAX;
    return PSEG_OK;
}

}  // extern "C"
