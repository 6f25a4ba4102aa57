// pseg_tiles.hip -- tiled prediction: the label map of a page of any size from same-shape tiles.
//
// Network.predict_single_data (lib/network.py:248-260) pads the page to a multiple of 32 (lib/model.py:10-42), runs the graph and
// takes the argmax.  A logit depends on the input within the graph's receptive field only, and the graph's arithmetic at a pixel
// does not depend on where the 32-pixel grid's origin lies as long as it lies on the page's own grid: a tile cut on that grid with
// `halo` pixels of context on every side that is not the canvas edge has, away from those sides, the page's logits bit for bit.
// The tiles run through the page-slot path (predict_device_pages) and a kernel writes every tile's owned rectangle into the page's map.
#include <algorithm>

#include "pseg_common.h"

namespace pseg {

constexpr int TILE_DEFAULT = 2048;   // tile edge of tile = 0, every graph
constexpr int TILE_UNIT = 16;        // tiles per page-slot unit at most (pseg_predict_pages_device's count)

struct TileRec { int y, x, oy0, oy1, ox0, ox1; };           // origin on the canvas; owned rectangle [oy0, oy1) x [ox0, ox1), canvas coordinates
struct TilePlan { int th = 0, tw = 0, Hp = 0, Wp = 0; std::vector<TileRec> t; };
struct TileTab { TileRec t[TILE_UNIT]; };                   // a unit's records, a kernel argument (owned rectangles clipped to the page)

// One axis of the plan: tile extent t = min(T, Np), stride t - 2 halo, origins min(k stride, Np - t) up to the first that reaches
// Np - t; tile k owns from the end of tile k - 1's range to y_k + t - halo, the last one to Np.
static void tile_axis(int Np, int T, int halo, int* t_out, std::vector<int>& org, std::vector<int>& lo, std::vector<int>& hi) {
    const int t = std::min(T, Np), s = t - 2 * halo;
    *t_out = t;
    int prev = 0;
    for (long long k = 0;; ++k) {
        const int y = (int)std::min<long long>(k * s, Np - t);
        const bool last = y == Np - t;
        org.push_back(y);
        lo.push_back(prev);
        hi.push_back(last ? Np : y + t - halo);
        prev = hi.back();
        if (last) break;
    }
}
// The pass that ends the plan (as chain_plan_check): per axis the ranges tile [0, Np) in order -- with tiles that are products of a
// row and a column range, every canvas pixel then has exactly one owner --, an owned pixel lies at least `halo` from every tile edge
// that is not the canvas edge, origins are multiples of 32 and tiles lie inside the canvas.  O(tiles per axis).
static int tile_axis_check(int Np, int t, int halo, const std::vector<int>& org, const std::vector<int>& lo, const std::vector<int>& hi) {
    int next = 0;
    for (size_t k = 0; k < org.size(); ++k) {
        const int y = org[k];
        bool ok = y >= 0 && y % 32 == 0 && y <= Np - t && lo[k] == next && hi[k] > lo[k];
        ok = ok && (y == 0 ? lo[k] == 0 : lo[k] - y >= halo) && (y + t == Np ? hi[k] == Np : y + t - hi[k] >= halo);
        if (!ok) return fail(PSEG_EHIP, "tile plan: tile %zu of an axis of %d (tile %d, halo %d) breaks an invariant", k, Np, t, halo);
        next = hi[k];
    }
    if (next != Np) return fail(PSEG_EHIP, "tile plan: the owned ranges end at %d of %d", next, Np);
    return PSEG_OK;
}

// No HIP call.  tile = 0: TILE_DEFAULT.
static int tile_plan(int arch, int H, int W, int tile, TilePlan* out) {
    if (arch < PSEG_ARCH_FCN_SKIP || arch > PSEG_ARCH_RES_UNET) return fail(PSEG_EINVAL, "tile plan: unknown architecture %d", arch);
    if (H <= 0 || W <= 0 || H > 0x7FFFFFE0 || W > 0x7FFFFFE0) return fail(PSEG_EINVAL, "tile plan: bad shape %d x %d", H, W);
    const int halo = halo_of(arch);
    if (tile == 0) tile = TILE_DEFAULT;
    if (tile < 2 * halo + 32 || tile % 32 != 0)
        return fail(PSEG_EINVAL, "tile plan: tile %d (a multiple of 32, at least 2 x the halo of %d + 32 = %d; 0 = the default of %d)", tile, halo, 2 * halo + 32,
                    TILE_DEFAULT);
    TilePlan& p = *out;
    p.Hp = round_up(H, 32);
    p.Wp = round_up(W, 32);
    std::vector<int> oy, ly, hy, ox, lx, hx;
    tile_axis(p.Hp, tile, halo, &p.th, oy, ly, hy);
    tile_axis(p.Wp, tile, halo, &p.tw, ox, lx, hx);
    PSEG_TRY(tile_axis_check(p.Hp, p.th, halo, oy, ly, hy));
    PSEG_TRY(tile_axis_check(p.Wp, p.tw, halo, ox, lx, hx));
    if ((unsigned long long)oy.size() * ox.size() > 0x7FFFFFFFull) return fail(PSEG_EINVAL, "tile plan: %zu x %zu tiles", oy.size(), ox.size());
    p.t.clear();
    p.t.reserve(oy.size() * ox.size());
    for (size_t i = 0; i < oy.size(); ++i)
        for (size_t j = 0; j < ox.size(); ++j) p.t.push_back(TileRec{oy[i], ox[j], ly[i], hy[i], lx[j], hx[j]});
    return PSEG_OK;
}

// Tile blockIdx.y of the unit out of the resident H x W x C page: the page's bytes in [y, y + th) x [x, x + tw), zeros outside the page.
// A tile row is tw * C bytes, a multiple of 32: sixteen bytes per thread and store, and a store never crosses a row.  The page's rows
// have any length, so its bytes are read one by one unless the run of sixteen happens to start on a word.
__global__ __launch_bounds__(256) void tiles_cut_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ tiles, const TileTab tab, int H, int W, int C,
                                                        int th, int tw) {
    const TileRec m = tab.t[blockIdx.y];
    const size_t rowb = (size_t)tw * C, n16 = (size_t)th * rowb / 16, wb = (size_t)W * C;
    uint4* dst = (uint4*)(tiles + (size_t)blockIdx.y * th * rowb);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i * 16, r = b / rowb, c = b - r * rowb;
        const size_t gy = (size_t)m.y + r, gc = (size_t)m.x * C + c;          // the page's row, byte of that row
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (gy < (size_t)H && gc < wb) {
            const uint8_t* src = img + gy * wb + gc;
            if (gc + 16 <= wb && (((size_t)src) & 3) == 0) {
                const uint32_t* s4 = (const uint32_t*)src;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = s4[j];
            } else {
                const int nb = (int)(wb - gc < 16 ? wb - gc : 16);
                for (int j = 0; j < nb; ++j) v[j >> 2] |= (uint32_t)src[j] << (8 * (j & 3));
            }
        }
        dst[i] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// Tile blockIdx.y's owned rectangle (the table's is clipped to the page) out of the tile's th x tw label map into the page's dense
// H x W map(s); rectangles of different tiles are disjoint.
__global__ __launch_bounds__(256) void tiles_stitch_kernel(const uint8_t* __restrict__ tlab, uint8_t* __restrict__ out_u8, int64_t* __restrict__ out_i64,
                                                           const TileTab tab, int W, int th, int tw) {
    const TileRec m = tab.t[blockIdx.y];
    if (m.oy1 <= m.oy0 || m.ox1 <= m.ox0) return;
    const size_t rw = (size_t)(m.ox1 - m.ox0), n = (size_t)(m.oy1 - m.oy0) * rw;
    const uint8_t* src = tlab + (size_t)blockIdx.y * th * tw + (size_t)(m.oy0 - m.y) * tw + (size_t)(m.ox0 - m.x);
    const size_t o0 = (size_t)m.oy0 * W + m.ox0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / rw, c = i - r * rw;
        const uint8_t v = src[r * tw + c];
        if (out_u8) out_u8[o0 + r * W + c] = v;
        if (out_i64) out_i64[o0 + r * W + c] = v;
    }
}

int predict_tiled_device(Engine& e, const uint8_t* d_img, int H, int W, int tile, int64_t* d_labels, uint8_t* d_labels_u8, hipStream_t st) {
    if (!d_img || (!d_labels && !d_labels_u8)) return fail(PSEG_EINVAL, "NULL argument / no label map requested");
    if (e.n_classes > 256) return fail(PSEG_EUNSUPPORTED, "tiled prediction keeps uint8 tile label maps (<= 256 classes)");
    TilePlan p;
    PSEG_TRY(tile_plan(e.arch, H, W, tile, &p));
    PSEG_HIP(hipSetDevice(e.device));
    for (auto& q : e.params)
        if (!q.set) return fail(PSEG_EINVAL, "weight '%s' was never set", q.name.c_str());
    if (e.weights_dirty) PSEG_TRY(upload_weights(e));      // (before pages_capable is asked: the plans exist after the first upload, see batch_unit_cap)
    const int n = (int)p.t.size();
    if (n == 1) return predict_device(e, d_img, H, W, nullptr, nullptr, d_labels, d_labels_u8, st, nullptr);
    // units of tiles through the page slots; an engine without page units (float32, PSEG_NO_PAGE_BATCH) takes the tiles one by one
    int cap = fit_unit_slots(e, p.th, p.tw, std::min(TILE_UNIT, n));
    const size_t tpx = (size_t)p.th * p.tw, img_b = (size_t)cap * tpx * e.in_ch, lab_b = (size_t)cap * tpx;
    if (e.tile_img.cap < img_b || e.tile_lab.cap < lab_b || !e.tile_img.p || !e.tile_lab.p) {
        PSEG_HIP(hipStreamSynchronize(st));                // a reallocation must not race with an earlier call's work on the staging
        PSEG_TRY(e.tile_img.ensure(img_b, "tiles"));
        PSEG_TRY(e.tile_lab.ensure(lab_b, "tile label maps"));
    }
    for (int i = 0; i < n;) {
        const int g = std::min(cap, n - i);
        TileTab tab{};
        for (int k = 0; k < g; ++k) {
            TileRec r = p.t[i + k];
            // what the kernels index with: re-checked here against the buffers they write (the plan's pass has checked the geometry)
            if (r.y < 0 || r.x < 0 || r.y + p.th > p.Hp || r.x + p.tw > p.Wp || r.oy0 < r.y || r.oy1 > r.y + p.th || r.ox0 < r.x || r.ox1 > r.x + p.tw)
                return fail(PSEG_EHIP, "tile plan: tile %d leaves its canvas", i + k);
            r.oy1 = std::min(r.oy1, H);
            r.ox1 = std::min(r.ox1, W);
            tab.t[k] = r;
        }
        const unsigned bx_cut = (unsigned)std::min<size_t>((tpx * e.in_ch / 16 + 255) / 256, 1024);
        tiles_cut_kernel<<<dim3(bx_cut, g), 256, 0, st>>>(d_img, e.tile_img.p, tab, H, W, e.in_ch, p.th, p.tw);
        PSEG_HIP(hipGetLastError());
        const int rc = g > 1 ? predict_device_pages(e, e.tile_img.p, g, p.th, p.tw, nullptr, e.tile_lab.p, st)
                             : predict_device(e, e.tile_img.p, p.th, p.tw, nullptr, nullptr, nullptr, e.tile_lab.p, st, nullptr);
        if (rc == PSEG_ENOMEM && cap > 1) { cap = (cap + 1) / 2; continue; }     // (set_canvas left the engine without a canvas: half the slots)
        PSEG_TRY(rc);
        tiles_stitch_kernel<<<dim3((unsigned)std::min<size_t>((tpx + 255) / 256, 1024), g), 256, 0, st>>>(e.tile_lab.p, d_labels_u8, d_labels, tab, W, p.th, p.tw);
        PSEG_HIP(hipGetLastError());
        i += g;
    }
    return PSEG_OK;
}

// AUTO: the pages the whole-page path cannot take -- the bf16 guard refuses the canvas, or one slot of it does not fit the device's
// free memory (a canvas the engine holds already fits).  Which route a page took does not show in its map.
static bool tiling_applies(Engine& e, int H, int W) {
    if (e.tiling_mode == PSEG_TILING_OFF || H <= 0 || W <= 0 || e.n_classes > 256) return false;
    if (e.tiling_mode == PSEG_TILING_ALWAYS) return true;
    const int Hp = round_up(H, 32), Wp = round_up(W, 32);
    if (canvas_refused(e, Hp, Wp)) return true;
    if (Hp == e.Hp && Wp == e.Wp) return false;
    return !page_slot_fits(e, H, W);
}

int predict_labels_routed(Engine& e, const uint8_t* d_img, int H, int W, int64_t* d_labels, uint8_t* d_labels_u8, hipStream_t st) {
    if (e.tiling_mode != PSEG_TILING_OFF && (d_labels || d_labels_u8)) {
        PSEG_HIP(hipSetDevice(e.device));
        if (tiling_applies(e, H, W)) return predict_tiled_device(e, d_img, H, W, e.tiling_tile, d_labels, d_labels_u8, st);
    }
    return predict_device(e, d_img, H, W, nullptr, nullptr, d_labels, d_labels_u8, st, nullptr);
}

}  // namespace pseg

using namespace pseg;

extern "C" int pseg_tile_plan(int arch, int H, int W, int tile, int* tile_h, int* tile_w, int* origin_y, int* origin_x, int* owned, int max_tiles) {
    TilePlan p;
    PSEG_TRY(tile_plan(arch, H, W, tile, &p));
    if (tile_h) *tile_h = p.th;
    if (tile_w) *tile_w = p.tw;
    const int n = (int)p.t.size();
    if (n > max_tiles && (origin_y || origin_x || owned)) return fail(PSEG_EINVAL, "%d tiles, room for %d", n, max_tiles);
    for (int k = 0; k < n; ++k) {
        const TileRec& r = p.t[k];
        if (origin_y) origin_y[k] = r.y;
        if (origin_x) origin_x[k] = r.x;
        if (owned) { owned[4 * k] = r.oy0; owned[4 * k + 1] = r.oy1; owned[4 * k + 2] = r.ox0; owned[4 * k + 3] = r.ox1; }
    }
    return n;
}

extern "C" int pseg_predict_tiled_device(pseg_engine* h, const uint8_t* d_img, int H, int W, int tile, int64_t* d_labels, uint8_t* d_labels_u8,
                                         void* stream) {
    if (!h) return fail(PSEG_EINVAL, "NULL engine");
    KnobScope knob_scope(h->e);
    return predict_tiled_device(h->e, d_img, H, W, tile, d_labels, d_labels_u8, stream ? (hipStream_t)stream : h->e.stream);
}

extern "C" int pseg_predict_tiled(pseg_engine* h, const uint8_t* img, int H, int W, int tile, int64_t* labels, uint8_t* labels_u8) {
    if (!h || !img || (!labels && !labels_u8)) return fail(PSEG_EINVAL, "NULL argument / no label map requested");
    KnobScope knob_scope(h->e);
    if (H <= 0 || W <= 0) return fail(PSEG_EINVAL, "empty page %dx%d", H, W);
    Engine& e = h->e;
    PSEG_HIP(hipSetDevice(e.device));
    const size_t npx = (size_t)H * W, o8 = labels ? npx * 8 : 0;
    PSEG_TRY(e.img_stage.ensure(npx * e.in_ch, "page"));
    PSEG_TRY(e.lab_stage.ensure(o8 + (labels_u8 ? npx : 0), "labels"));
    PSEG_HIP(hipMemcpyAsync(e.img_stage.p, img, npx * e.in_ch, hipMemcpyHostToDevice, e.stream));
    PSEG_TRY(predict_tiled_device(e, e.img_stage.p, H, W, tile, labels ? e.lab_stage.as<int64_t>() : nullptr, labels_u8 ? e.lab_stage.p + o8 : nullptr, e.stream));
    if (labels) PSEG_HIP(hipMemcpyAsync(labels, e.lab_stage.p, npx * 8, hipMemcpyDeviceToHost, e.stream));
    if (labels_u8) PSEG_HIP(hipMemcpyAsync(labels_u8, e.lab_stage.p + o8, npx, hipMemcpyDeviceToHost, e.stream));
    return engine_status(e, e.stream);
}

extern "C" int pseg_engine_set_tiling(pseg_engine* h, int mode, int tile) {
    if (!h) return fail(PSEG_EINVAL, "NULL engine");
    if (mode != PSEG_TILING_OFF && mode != PSEG_TILING_AUTO && mode != PSEG_TILING_ALWAYS) return fail(PSEG_EINVAL, "tiling mode %d", mode);
    TilePlan p;
    PSEG_TRY(tile_plan(h->e.arch, 32, 32, tile, &p));     // (the tile edge's own checks)
    h->e.tiling_mode = mode;
    h->e.tiling_tile = tile;
    return PSEG_OK;
}

extern "C" int pseg_engine_page_fits(pseg_engine* h, int H, int W) {
    if (!h) return fail(PSEG_EINVAL, "NULL engine");
    if (H <= 0 || W <= 0) return fail(PSEG_EINVAL, "empty page %dx%d", H, W);
    Engine& e = h->e;
    const int Hp = round_up(H, 32), Wp = round_up(W, 32);
    if (canvas_refused(e, Hp, Wp)) return 0;
    if (Hp == e.Hp && Wp == e.Wp) return 1;
    PSEG_HIP(hipSetDevice(e.device));
    return page_slot_fits(e, H, W) ? 1 : 0;
}
