// pseg_chain.hip -- the Predictor's chain as one device-resident call (lib/predictor.py:32-54):
//   Network.predict_single_data (argmax labels)  ->  [scale_to_original_shape: nearest resize of the label map,
//   lib/output.py:63-79]  ->  the post-processors in PredictSettings.post_process order (lib/postprocess.py:9-42)  ->
//   [generate_output_masks, lib/output.py:44-60].
// The reference hands a NumPy int64 map from stage to stage; here the uint8 label map stays in HBM between the stages
// (rounds 1-2 sent it down and up again around every stage: 25 MB each way per stage at 2048x1536), the page and the
// binarisation go up once, and only what the caller asked for comes down -- by DMA straight into the caller's arrays when
// those are page-locked (pseg_host_alloc / the Python shim's pooled pinned arrays).
#include <algorithm>
#include <cstring>

#include "pseg_list.h"
#include "pseg_regions.h"

namespace pseg {

// One of the two staging sets of the page chain (pseg_predict_chain_pages_png): everything a unit of pages touches.
struct PagesSet {
    enum { IMG = 0, LAB = 1, LAB2 = 2, BIN = 3, PNG = 4, PAD = 5, CLAB = 6, SCAN = 7, FILT = 8, REC = 9, RGN = 10, NDEV = 11 };
    // pages / network labels / resize + bbox ping-pong / binarisations / encoder workspace / mixed units: the pages padded to canvas-sized
    // page slots / the slots' canvas-sized label maps / scan chain: the unit's scans / their filtered planes / their records / the regions
    // stage's workspace (pseg_regions.h, RgStageLay)
    GrowDev d[NDEV];
    GrowPin h_in;                        // pages and binarisations of callers with pageable arrays
    GrowPin h_out;                       // the unit's encoded streams (+ label maps), grown to the bytes units really have
    GrowPin h_tot;                       // [pages][4] stream sizes (unsigned long long)
    GrowPin h_rg;                        // the regions stage: its table of maps, then the unit's counts and map records as they come back
};
struct ChainPagesState {
    PagesSet set[2];
    PipeSet ev[2];                      // uploads landed / compute + sizes landed / downloads landed
    GrowDev d_lut;
    GrowDev d_tab;                       // the page table of a mixed call (one MixedPage per page of the list, in the planner's order) ...
    GrowPin h_tab;                       // ... and its page-locked source
    GrowDev d_wt;                        // the anti-aliasing weights of a scan call (every scan's doubles, in the planner's order) ...
    GrowPin h_wt;                        // ... and their page-locked source
};

struct ChainState {
    hipStream_t s_aux = nullptr;        // uploads of the binarisation / colour table beside the network's kernels
    hipEvent_t ev_aux = nullptr;
    GrowDev buf[7];
    ChainPagesState* pages = nullptr;
};
enum { CB_IMG = 0, CB_LAB = 1, CB_LAB2 = 2, CB_BIN = 3, CB_MASKS = 4, CB_LUT = 5, CB_I64 = 6 };

// the staging sets' memory (device and page-locked); the events and the colour table stay.  The caller has waited for the device.
static void pages_release(ChainPagesState& p) {
    for (GrowDev* b : {&p.d_tab, &p.d_wt}) b->release();
    for (GrowPin* b : {&p.h_tab, &p.h_wt}) b->release();
    for (PagesSet& s : p.set) {
        for (GrowDev& b : s.d) b.release();
        for (GrowPin* b : {&s.h_in, &s.h_out, &s.h_tot, &s.h_rg}) b->release();
    }
}

void chain_trim(Engine& e) {
    auto* c = (ChainState*)e.chain;
    if (c && c->pages) pages_release(*c->pages);
}

void chain_free(Engine& e) {
    auto* c = (ChainState*)e.chain;
    if (!c) return;
    if (c->pages) {
        pages_release(*c->pages);
        for (PipeSet& s : c->pages->ev) s.destroy();
        c->pages->d_lut.release();
        delete c->pages;
    }
    for (GrowDev& b : c->buf) b.release();
    if (c->ev_aux) (void)hipEventDestroy(c->ev_aux);
    if (c->s_aux) (void)hipStreamDestroy(c->s_aux);
    delete c;
    e.chain = nullptr;
}

// the engine's chain state with its stream and event, made on the first chain call
static int chain_state(Engine& e) {
    if (e.chain) return PSEG_OK;
    auto* nc = new ChainState();
    e.chain = nc;
    PSEG_HIP(hipStreamCreateWithFlags(&nc->s_aux, hipStreamNonBlocking));
    PSEG_HIP(hipEventCreateWithFlags(&nc->ev_aux, hipEventDisableTiming));
    return PSEG_OK;
}

__global__ void chain_widen_kernel(const uint8_t* in, int64_t* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = in[i];
}

// Mixed units: every page of the unit (blockIdx.y) from its dense H x W x C bytes into its canvas-sized slot, zeros outside the page.
// Four bytes per thread: a slot's rows are multiples of 32 bytes, so a word never crosses a row.
__global__ __launch_bounds__(256) void pages_pad_kernel(const uint8_t* img, uint8_t* padded, const MixedPage* tab, int Hp, int Wp, int C) {
    const MixedPage& m = tab[blockIdx.y];
    const size_t rowb = (size_t)Wp * C, n4 = (size_t)Hp * rowb / 4, wb = (size_t)m.W * C;
    const uint8_t* src = img + m.img_off;
    uint32_t* dst = (uint32_t*)(padded + (size_t)blockIdx.y * Hp * rowb);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i * 4, r = b / rowb, c = b - r * rowb;
        uint32_t v = 0;
        if (r < (size_t)m.H)
            for (int j = 0; j < 4; ++j)
                if (c + j < wb) v |= (uint32_t)src[r * wb + c + j] << (8 * j);
        dst[i] = v;
    }
}
// ... and back: the top-left H x W of every slot's canvas-sized label map, densely, where resize, vote and encoder expect the page's map
__global__ __launch_bounds__(256) void pages_crop_kernel(const uint8_t* clab, uint8_t* lab, const MixedPage* tab, int Hp, int Wp) {
    const MixedPage& m = tab[blockIdx.y];
    const uint8_t* src = clab + (size_t)blockIdx.y * Hp * Wp;
    uint8_t* dst = lab + m.lab_off;
    const size_t n = (size_t)m.H * m.W, w = (size_t)m.W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / w;
        dst[i] = src[r * Wp + (i - r * w)];
    }
}
}  // namespace pseg

using namespace pseg;

// the masks of a chain call as PNG streams (pseg_predict_chain_png) instead of raw arrays
struct ChainPng { uint8_t* const* out; const size_t* cap; size_t* n_bytes; int level; };

// The argument checks of a chain call, shared by the single-page entries (page < 0) and the page list (the message names the page).
struct ChainReq { bool resize, want_masks, need_bin; int Hl, Wl; };
static int chain_check(const Engine& e, int page, const uint8_t* img, int H, int W, int Ho, int Wo, const uint8_t* binary, const int* post_ops,
                       int n_post, unsigned flags, bool want_masks, bool want_png, const uint8_t* lut, int n_lut, int level, ChainReq* r) {
    char at[32] = "";
    if (page >= 0) snprintf(at, sizeof at, "page %d: ", page);
    if (!img) return fail(PSEG_EINVAL, "%sNULL argument", at);
    if (H <= 0 || W <= 0 || n_post < 0 || (n_post > 0 && !post_ops)) return fail(PSEG_EINVAL, "%sbad argument", at);
    if (e.n_classes > 256) return fail(PSEG_EUNSUPPORTED, "the chain keeps a uint8 label map (<= 256 classes)");
    if (flags & ~(unsigned)PSEG_CHAIN_EXACT_LABELS) return fail(PSEG_EINVAL, "unknown flag bits 0x%x", flags);
    r->resize = Ho > 0 && Wo > 0 && (Ho != H || Wo != W);
    r->Hl = r->resize ? Ho : H;
    r->Wl = r->resize ? Wo : W;
    r->want_masks = want_masks;
    r->need_bin = want_masks;
    for (int i = 0; i < n_post; ++i) {
        if (post_ops[i] != PSEG_POST_CC_VOTE && post_ops[i] != PSEG_POST_BBOX) return fail(PSEG_EINVAL, "unknown post-processor id %d", post_ops[i]);
        r->need_bin |= post_ops[i] == PSEG_POST_CC_VOTE;
    }
    if (r->need_bin && !binary) return fail(PSEG_EINVAL, "%sthe vote / the masks need the binarisation", at);
    if (want_masks && (!lut || n_lut < 1)) return fail(PSEG_EINVAL, "the masks need the colour table");
    if (want_png) {
        if (n_lut > 256) return fail(PSEG_EINVAL, "n_lut %d out of range (1..256)", n_lut);
        if (level != 0 && level != 1) return fail(PSEG_EINVAL, "png: level %d (0 = fixed Huffman codes, 1 = dynamic codes per band)", level);
    }
    return PSEG_OK;
}
// Where chain_post_enqueue's walk ends: 0 = the network's map, 1 = bufA, 2 = bufB.  The page list's plan places the final maps with
// this before anything runs, so it stands beside the walk: the two change together.
static int chain_final_slot(bool resize, const int* post_ops, int n_post) {
    int where = resize ? 1 : 0;
    for (int i = 0; i < n_post; ++i)
        if (post_ops[i] == PSEG_POST_BBOX) where = where == 1 ? 2 : 1;
    return where;
}
// scale_to_original_shape (an order-0 gather of the label map, preserving_resize(pred, original_shape)), then the post-processors in
// order: the vote works in place, the boxes ping-pong between bufA and bufB.  bin_ready (may be NULL): the binarisation's upload, waited
// for behind the resize.  *final (may be NULL): the map the walk ended in.
static int chain_post_enqueue(Engine& e, uint8_t* lab, uint8_t* bufA, uint8_t* bufB, const uint8_t* bin, int H, int W, int Hl, int Wl, bool resize,
                              const int* post_ops, int n_post, hipStream_t st, uint8_t** final, hipEvent_t bin_ready = nullptr) {
    uint8_t* cur = lab;
    if (resize) {
        PSEG_TRY(pseg_resize_nearest_device(e.device, cur, H, W, 1, bufA, Hl, Wl, st));
        cur = bufA;
    }
    if (bin_ready) PSEG_HIP(hipStreamWaitEvent(st, bin_ready, 0));
    for (int i = 0; i < n_post; ++i) {
        if (post_ops[i] == PSEG_POST_CC_VOTE) {
            PSEG_TRY(pseg_cc_vote_device_u8(e.device, cur, bin, Hl, Wl, e.n_classes, st));
        } else {
            uint8_t* const dst = cur == bufA ? bufB : bufA;
            PSEG_TRY(pseg_bbox_fill_device_u8(e.device, cur, dst, Hl, Wl, e.n_classes, st));
            cur = dst;
        }
    }
    if (final) *final = cur;
    return PSEG_OK;
}

static int chain_run(pseg_engine* h, const uint8_t* img, int H, int W, int Ho, int Wo, const uint8_t* binary,
                     const int* post_ops, int n_post, unsigned flags, int64_t* labels, uint8_t* labels_u8,
                     const uint8_t* lut, int n_lut, uint8_t* color, uint8_t* overlay, uint8_t* inverted,
                     uint8_t* fg_color, const ChainPng* png) {
    if (!h || !img) return fail(PSEG_EINVAL, "NULL argument");
    KnobScope knob_scope(h->e);
    Engine& e = h->e;
    const bool want_png = png && (png->out[0] || png->out[1] || png->out[2] || png->out[3]);
    const bool want_masks = color || overlay || inverted || fg_color || want_png;
    ChainReq req;
    PSEG_TRY(chain_check(e, -1, img, H, W, Ho, Wo, binary, post_ops, n_post, flags, want_masks, want_png, lut, n_lut, png ? png->level : 0, &req));
    const bool need_bin = req.need_bin;
    const int Hl = req.Hl, Wl = req.Wl;
    if (want_png) {
        const size_t bound = pseg_png_bound_lv(Hl, Wl, 3, 0, png->level);
        for (int k = 0; k < 4; ++k)
            if (png->out[k] && png->cap[k] < bound) return fail(PSEG_EINVAL, "png: output buffer %d of %zu bytes, pseg_png_bound is %zu", k, png->cap[k], bound);
    }
    PSEG_HIP(hipSetDevice(e.device));
    PSEG_TRY(chain_state(e));
    ChainState& c = *(ChainState*)e.chain;
    hipStream_t st = e.stream;
    const size_t npx = (size_t)H * W, nl = (size_t)Hl * Wl;
    const size_t nla = (nl + 255) & ~(size_t)255;          // buffer stride: the mask / vote kernels want 4-byte aligned maps
    // a reallocation must not race with the previous call's work: every call ends synchronised, so the buffers are idle here
    PSEG_TRY(c.buf[CB_IMG].ensure(npx * e.in_ch, "chain page"));
    PSEG_TRY(c.buf[CB_LAB].ensure(npx, "chain labels"));
    PSEG_TRY(c.buf[CB_LAB2].ensure(2 * nla, "chain resize + box maps"));          // resize target + bounding-box ping-pong
    if (need_bin) PSEG_TRY(c.buf[CB_BIN].ensure(nl, "chain binarisation"));
    if (want_masks && !want_png) PSEG_TRY(c.buf[CB_MASKS].ensure(4 * nla * 3, "chain masks"));
    if (want_masks) PSEG_TRY(c.buf[CB_LUT].ensure((size_t)n_lut * 3, "chain colour table"));
    if (labels) PSEG_TRY(c.buf[CB_I64].ensure(nl * 8, "chain int64 labels"));
    uint8_t* const d_img = c.buf[CB_IMG].p, * const d_bin = c.buf[CB_BIN].p, * const d_lut = c.buf[CB_LUT].p;
    StreamDrain drain{{st, c.s_aux, nullptr}};
    // uploads: the page on the engine's stream (the network waits for it anyway), binarisation and colour table beside it
    PSEG_HIP(hipMemcpyAsync(d_img, img, npx * e.in_ch, hipMemcpyHostToDevice, st));
    if (need_bin) PSEG_HIP(hipMemcpyAsync(d_bin, binary, nl, hipMemcpyHostToDevice, c.s_aux));
    if (want_masks) PSEG_HIP(hipMemcpyAsync(d_lut, lut, (size_t)n_lut * 3, hipMemcpyHostToDevice, c.s_aux));
    if (need_bin) PSEG_HIP(hipEventRecord(c.ev_aux, c.s_aux));
    // 1. the network: uint8 argmax labels (float32 engine: bit-exact; bf16 engine: throughput labels, or the label-exact mode)
    if ((flags & PSEG_CHAIN_EXACT_LABELS) && e.mode == PSEG_MODE_BF16)
        PSEG_TRY(pseg_predict_exact_labels_device(h, d_img, H, W, c.buf[CB_LAB].p, nullptr, nullptr, st));
    else
        PSEG_TRY(predict_labels_routed(e, d_img, H, W, nullptr, c.buf[CB_LAB].p, st));      // (in tiles where the engine's tiling mode says so: the same map)
    // 2. / 3. resize and post-processors
    uint8_t* cur = nullptr;
    PSEG_TRY(chain_post_enqueue(e, c.buf[CB_LAB].p, c.buf[CB_LAB2].p, c.buf[CB_LAB2].p + nla, d_bin, H, W, Hl, Wl, req.resize, post_ops, n_post, st, &cur,
                                need_bin ? c.ev_aux : nullptr));
    // 4. outputs
    if (labels_u8) PSEG_HIP(hipMemcpyAsync(labels_u8, cur, nl, hipMemcpyDeviceToHost, st));
    if (labels) {
        chain_widen_kernel<<<(int)std::min<size_t>((nl + 255) / 256, 8192), 256, 0, st>>>(cur, (int64_t*)c.buf[CB_I64].p, nl);
        PSEG_HIP(hipMemcpyAsync(labels, c.buf[CB_I64].p, nl * 8, hipMemcpyDeviceToHost, st));
    }
    if (want_png) {
        // the band kernel selects the masks' pixels itself: the RGB masks are never written; synchronises `st`
        PSEG_TRY(pseg_masks_png_device_u8_lv(e.device, cur, d_bin, d_lut, n_lut, Hl, Wl, 0, png->level, png->out, png->cap, png->n_bytes, st));
    } else if (want_masks) {
        uint8_t* m = c.buf[CB_MASKS].p;
        uint8_t* dm[4] = {color ? m : nullptr, overlay ? m + nla * 3 : nullptr, inverted ? m + 2 * nla * 3 : nullptr, fg_color ? m + 3 * nla * 3 : nullptr};
        PSEG_TRY(pseg_masks_device_u8(e.device, cur, d_bin, d_lut, n_lut, Hl, Wl, dm[0], dm[1], dm[2], dm[3], st));
        uint8_t* hm[4] = {color, overlay, inverted, fg_color};
        for (int k = 0; k < 4; ++k)
            if (hm[k]) PSEG_HIP(hipMemcpyAsync(hm[k], dm[k], nl * 3, hipMemcpyDeviceToHost, st));
    }
    PSEG_HIP(hipStreamSynchronize(c.s_aux));
    return engine_status(e, st);
}

extern "C" int pseg_predict_chain(pseg_engine* h, const uint8_t* img, int H, int W, int Ho, int Wo, const uint8_t* binary,
                                  const int* post_ops, int n_post, unsigned flags, int64_t* labels, uint8_t* labels_u8,
                                  const uint8_t* lut, int n_lut, uint8_t* color, uint8_t* overlay, uint8_t* inverted,
                                  uint8_t* fg_color) {
    return chain_run(h, img, H, W, Ho, Wo, binary, post_ops, n_post, flags, labels, labels_u8, lut, n_lut, color, overlay, inverted, fg_color, nullptr);
}

extern "C" int pseg_predict_chain_png_lv(pseg_engine* h, const uint8_t* img, int H, int W, int Ho, int Wo, const uint8_t* binary,
                                         const int* post_ops, int n_post, unsigned flags, int64_t* labels, uint8_t* labels_u8,
                                         const uint8_t* lut, int n_lut, int level, uint8_t* const png[4], const size_t cap[4], size_t n_bytes[4]) {
    if (!png || !cap || !n_bytes) return fail(PSEG_EINVAL, "NULL argument");
    for (int k = 0; k < 4; ++k) n_bytes[k] = 0;
    const ChainPng req{png, cap, n_bytes, level};
    return chain_run(h, img, H, W, Ho, Wo, binary, post_ops, n_post, flags, labels, labels_u8, lut, n_lut, nullptr, nullptr, nullptr, nullptr, &req);
}

extern "C" int pseg_predict_chain_png(pseg_engine* h, const uint8_t* img, int H, int W, int Ho, int Wo, const uint8_t* binary,
                                      const int* post_ops, int n_post, unsigned flags, int64_t* labels, uint8_t* labels_u8,
                                      const uint8_t* lut, int n_lut, uint8_t* const png[4], const size_t cap[4], size_t n_bytes[4]) {
    return pseg_predict_chain_png_lv(h, img, H, W, Ho, Wo, binary, post_ops, n_post, flags, labels, labels_u8, lut, n_lut, 0, png, cap, n_bytes);
}
// ---- a page list through the chain to PNG streams (lib/predictor.py:27-30 x :49-54) ------------------------------------------

// The mixed planner: pages by canvas (stable: canvases by first appearance, list order within one), then plan_units over the canvases
static void plan_units_mixed(int n, const int* H, const int* W, int cap, std::vector<int>& order, std::vector<int>& ub, std::vector<int>& ug) {
    std::vector<int> Hc(n), Wc(n), first(n);
    std::vector<std::pair<int, int>> seen;
    for (int i = 0; i < n; ++i) {
        const std::pair<int, int> cv(round_up(H[i], 32), round_up(W[i], 32));
        size_t k = 0;
        while (k < seen.size() && seen[k] != cv) ++k;
        if (k == seen.size()) seen.push_back(cv);
        first[i] = (int)k;
    }
    order.resize(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
    for (int i = 0; i < n; ++i) { Hc[i] = seen[first[order[i]]].first; Wc[i] = seen[first[order[i]]].second; }
    plan_units(n, Hc.data(), Wc.data(), nullptr, nullptr, cap, ub, ug);
}

extern "C" int pseg_chain_units_mixed(int n_pages, const int* H, const int* W, int cap, int* order, int* unit_first, int* unit_count, int max_units) {
    if (n_pages < 0 || (n_pages > 0 && (!H || !W)) || cap < 1) return fail(PSEG_EINVAL, "bad argument");
    for (int i = 0; i < n_pages; ++i)
        if (H[i] <= 0 || W[i] <= 0 || H[i] > 0x7FFFFFE0 || W[i] > 0x7FFFFFE0) return fail(PSEG_EINVAL, "page %d: bad shape %d x %d", i, H[i], W[i]);
    std::vector<int> ord, ub, ug;
    plan_units_mixed(n_pages, H, W, cap, ord, ub, ug);
    if ((int)ub.size() > max_units && (unit_first || unit_count)) return fail(PSEG_EINVAL, "%zu units, room for %d", ub.size(), max_units);
    for (int i = 0; i < n_pages && order; ++i) order[i] = ord[i];
    for (size_t u = 0; u < ub.size(); ++u) {
        if (unit_first) unit_first[u] = ub[u];
        if (unit_count) unit_count[u] = ug[u];
    }
    return (int)ub.size();
}

extern "C" int pseg_chain_units(int n_pages, const int* H, const int* W, const int* Ho, const int* Wo, int cap, int* unit_first, int* unit_count,
                                int max_units) {
    if (n_pages < 0 || (n_pages > 0 && (!H || !W)) || cap < 1) return fail(PSEG_EINVAL, "bad argument");
    std::vector<int> ub, ug;
    plan_units(n_pages, H, W, Ho, Wo, cap, ub, ug);
    if ((int)ub.size() > max_units && (unit_first || unit_count)) return fail(PSEG_EINVAL, "%zu units, room for %d", ub.size(), max_units);
    for (size_t u = 0; u < ub.size(); ++u) {
        if (unit_first) unit_first[u] = ub[u];
        if (unit_count) unit_count[u] = ug[u];
    }
    return (int)ub.size();
}
// ---- the page-list entries: check -> plan -> reserve -> run ---------------------------------------------------------------
// The plan of a call, host arithmetic alone.  Positions are those of the planner's order: ord maps one to the caller's page (the
// identity unless mixed); unit u holds positions ub[u] .. ub[u] + ug[u].  tab says per position where the page, its maps and its
// binarisation lie in the unit's staging set (a mixed call's kernels read it on the device); mx* are the blocks' largest extents.
struct ChainUnit { bool slots; PngPages L; PngPagesMixed M; };      // page slots through the network; the encoder's layout (same-shape / mixed)
struct ChainPlan {
    bool mixed = false, two_maps = false, any_bin = false;
    int n = 0, in_ch = 1;
    std::vector<int> ord, ub, ug;
    std::vector<ChainUnit> un;
    std::vector<MixedPage> tab;
    std::vector<size_t> lab2_off, scan_off, filt_off, wt_off;       // LAB2; a scan call: the scan in SCAN, its filtered plane (and an adaptive binarisation's planes) in FILT, its weights in the call's table
    size_t n_wt = 0, mx[PagesSet::NDEV] = {}, mx_in = 0, mx_tot = 0, mx_rg_pin = 0;
    const pseg_regions* rg = nullptr;                               // the regions stage: per page of the caller's list, or none
    int rg_R = 0; long long rg_V = 0;                               // its max_regions and max_vertices
};

// what the regions stage of a unit needs: its workspace and its page-locked records (the table, the counts, the map records)
static int chain_rg_sizes(const ChainPlan& p, int i0, int g, size_t* dev, size_t* pin) {
    std::vector<int> Hl(g), Wl(g);
    for (int k = 0; k < g; ++k) { Hl[k] = p.tab[i0 + k].Hl; Wl[k] = p.tab[i0 + k].Wl; }
    RgStageLay lay;
    PSEG_TRY(rg_stage_plan(g, Hl.data(), Wl.data(), p.rg_R, p.rg_V, &lay));
    *dev = lay.bytes;
    *pin = lay.tab_bytes + up256((size_t)g * 4) + up256((size_t)g * RG_MAPV * 8);
    return PSEG_OK;
}

// The pass that ends the plan: every block of every page lies inside its mx[], the offsets that kernels and DMA rely on are aligned
// (or dense: same-shape pages go up in one DMA, same-shape page slots write their maps one behind the other), the units tile the list
// and the final maps are where chain_post_enqueue's walk will leave them.  O(n); a violation is a bug of the planner.
static int chain_plan_check(const ChainPlan& p, const std::vector<ChainReq>& req, const pseg_scan* scans, const pseg_binarize* how, const pseg_despeckle* dsp,
                            const int* post_ops, int n_post) {
    typedef PagesSet B;
    std::vector<char> seen(p.n, 0);
    int next = 0;
    for (size_t u = 0; u < p.ub.size(); ++u) {
        const int i0 = p.ub[u], g = p.ug[u];
        const ChainUnit& q = p.un[u];
        if (i0 != next || g < 1 || g > p.n - i0) return fail(PSEG_EHIP, "page chain plan: unit %zu does not continue the list at position %d", u, next);
        next = i0 + g;
        const size_t cpx = (size_t)round_up(p.tab[i0].H, 32) * round_up(p.tab[i0].W, 32);
        bool unit_ok = (p.mixed ? q.M.bytes : q.L.bytes) <= p.mx[B::PNG] && (size_t)g * 4 * sizeof(unsigned long long) <= p.mx_tot &&
                       (!scans || (size_t)g * SCAN_REC_WORDS * sizeof(unsigned) <= p.mx[B::REC]) &&
                       (!(p.mixed && q.slots) || ((size_t)g * cpx * p.in_ch <= p.mx[B::PAD] && (size_t)g * cpx <= p.mx[B::CLAB]));
        size_t in_b = 0, dense_img = 0, dense_lab = 0;
        for (int i = i0; i < next; ++i) {
            const int pi = p.ord[i];
            if (pi < 0 || pi >= p.n || seen[pi]) return fail(PSEG_EHIP, "page chain plan: position %d names page %d twice or none", i, pi);
            seen[pi] = 1;
            const MixedPage& m = p.tab[i];
            const size_t npx = (size_t)m.H * m.W, nl = (size_t)m.Hl * m.Wl, nla = up256(nl);
            bool ok = m.img_off + npx * p.in_ch <= p.mx[B::IMG] && m.lab_off + npx <= p.mx[B::LAB];
            ok = ok && (p.mixed ? m.img_off % 256 == 0 : m.img_off == dense_img) && (!p.mixed && q.slots ? m.lab_off == dense_lab : m.lab_off % 256 == 0);
            if (p.two_maps) ok = ok && p.lab2_off[i] % 256 == 0 && p.lab2_off[i] + 2 * nla <= p.mx[B::LAB2];
            if (req[pi].need_bin) ok = ok && m.bin_off % 256 == 0 && m.bin_off + nl <= p.mx[B::BIN];
            const int where = chain_final_slot(req[pi].resize, post_ops, n_post);
            ok = ok && (where == 0 || p.two_maps) && m.pred_sel == (where ? 1 : 0) &&
                 m.pred_off == (where == 0 ? m.lab_off : p.lab2_off[i] + (where == 2 ? nla : 0));
            if (scans) {
                const size_t sb = (size_t)scans[pi].H0 * scans[pi].W0;
                ok = ok && p.scan_off[i] % 256 == 0 && p.scan_off[i] + sb <= p.mx[B::SCAN] && p.filt_off[i] % 16 == 0 &&
                     p.filt_off[i] + scan_front_work(scans[pi], binarize_of(how, pi), despeckle_of(dsp, pi)) <= p.mx[B::FILT] && p.wt_off[i] + scan_front_weights(scans[pi], nullptr) <= p.n_wt;
                in_b += sb;
            } else in_b += npx * p.in_ch + (req[pi].need_bin ? nl : 0);
            if (!ok) return fail(PSEG_EHIP, "page chain plan: page %d does not lie inside its staging blocks", pi);
            dense_img += npx * p.in_ch;
            dense_lab += npx;
        }
        if (p.rg) {
            size_t dev = 0, pin = 0;
            PSEG_TRY(chain_rg_sizes(p, i0, g, &dev, &pin));
            unit_ok = unit_ok && dev <= p.mx[B::RGN] && pin <= p.mx_rg_pin;
        }
        if (!unit_ok || in_b > p.mx_in) return fail(PSEG_EHIP, "page chain plan: unit %zu (page %d ...) outgrows its staging", u, p.ord[i0]);
    }
    if (next != p.n) return fail(PSEG_EHIP, "page chain plan: the units end at position %d of %d", next, p.n);
    return PSEG_OK;
}

// No HIP call.  mixed = false: units are runs of same-shape pages in list order (pseg_chain_units); mixed = true: pages of one canvas
// (pseg_chain_units_mixed).  scans != NULL: a scan call (mixed), whose pages and ink maps the front end writes on the device.
static int chain_pages_plan(int n, const int* H, const int* W, const int* Ho, const int* Wo, const std::vector<ChainReq>& req, const pseg_scan* scans,
                            const pseg_binarize* how, const pseg_despeckle* dsp, const int* post_ops, int n_post, int in_ch, int cap, bool page_slots, bool mixed,
                            int level, int nout, const pseg_regions* rg, int max_regions, int max_vertices, ChainPlan* out) {
    typedef PagesSet B;
    ChainPlan& p = *out;
    p.rg = rg; p.rg_R = max_regions; p.rg_V = max_vertices;
    p.mixed = mixed;
    p.n = n;
    p.in_ch = in_ch;
    for (int i = 0; i < n; ++i) { p.any_bin |= req[i].need_bin; p.two_maps |= req[i].resize; }
    for (int i = 0; i < n_post; ++i) p.two_maps |= post_ops[i] == PSEG_POST_BBOX;
    if (mixed) plan_units_mixed(n, H, W, cap, p.ord, p.ub, p.ug);
    else {
        p.ord.resize(n);
        for (int i = 0; i < n; ++i) p.ord[i] = i;
        plan_units(n, H, W, Ho, Wo, cap, p.ub, p.ug);
    }
    p.un.resize(p.ub.size());
    p.tab.resize(n);
    p.lab2_off.assign(n, 0);
    for (auto* v : {&p.scan_off, &p.filt_off, &p.wt_off}) v->assign(scans ? n : 0, 0);
    for (size_t u = 0; u < p.ub.size(); ++u) {
        const int i0 = p.ub[u], g = p.ug[u], p0 = p.ord[i0];
        ChainUnit& q = p.un[u];
        // (same-shape page slots write the unit's maps one behind the other; mixed slots are canvases, cropped to aligned maps)
        q.slots = page_slots && g > 1 && (mixed || ((size_t)H[p0] * W[p0]) % 4 == 0);
        q.L = PngPages{0, 0, 0, 0, 0, 0, 0, 0};
        q.M = PngPagesMixed{0, 0, 0};
        size_t o_img = 0, o_lab = 0, o_bin = 0, o_lab2 = 0, lab_b = 0, in_b = 0, o_scan = 0, o_filt = 0;
        for (int i = i0; i < i0 + g; ++i) {
            const int pi = p.ord[i];
            MixedPage& m = p.tab[i];
            memset(&m, 0, sizeof m);
            const size_t npx = (size_t)H[pi] * W[pi], nl = (size_t)req[pi].Hl * req[pi].Wl, nla = up256(nl);   // (the vote kernels want 4-byte aligned maps)
            m.H = H[pi]; m.W = W[pi]; m.Hl = req[pi].Hl; m.Wl = req[pi].Wl;
            m.img_off = o_img; m.lab_off = o_lab; m.bin_off = o_bin;
            p.lab2_off[i] = o_lab2;
            o_img += mixed ? up256(npx * in_ch) : npx * in_ch;
            o_lab += !mixed && q.slots ? npx : up256(npx);
            lab_b += up256(npx);
            o_bin += nla;
            o_lab2 += 2 * nla;
            in_b += scans ? (size_t)scans[pi].H0 * scans[pi].W0 : npx * in_ch + (req[pi].need_bin ? nl : 0);
            if (scans) {
                p.scan_off[i] = o_scan;
                p.filt_off[i] = o_filt;
                p.wt_off[i] = p.n_wt;
                o_scan += up256((size_t)scans[pi].H0 * scans[pi].W0);
                o_filt += scan_front_work(scans[pi], binarize_of(how, pi), despeckle_of(dsp, pi));
                p.n_wt += scan_front_weights(scans[pi], nullptr);
            }
            const int where = chain_final_slot(req[pi].resize, post_ops, n_post);      // the page's final map, ahead of time
            m.pred_sel = where ? 1 : 0;
            m.pred_off = where == 0 ? m.lab_off : p.lab2_off[i] + (where == 2 ? nla : 0);
        }
        if (nout > 0) {
            if (mixed) PSEG_TRY(png_pages_layout_mixed(level, nout, g, &p.tab[i0], &q.M));
            else PSEG_TRY(png_pages_layout(req[p0].Hl, req[p0].Wl, level, nout, g, &q.L));
        }
        const size_t cpx = mixed && q.slots ? (size_t)round_up(H[p0], 32) * round_up(W[p0], 32) : 0;
        size_t rg_dev = 0, rg_pin = 0;
        if (p.rg) PSEG_TRY(chain_rg_sizes(p, i0, g, &rg_dev, &rg_pin));
        p.mx_rg_pin = std::max(p.mx_rg_pin, rg_pin);
        const size_t ext[B::NDEV] = {o_img, lab_b, p.two_maps ? o_lab2 : 0, p.any_bin ? o_bin : 0, mixed ? q.M.bytes : q.L.bytes, (size_t)g * cpx * in_ch,
                                     (size_t)g * cpx, o_scan, o_filt, scans ? (size_t)g * SCAN_REC_WORDS * sizeof(unsigned) : 0, rg_dev};
        for (int k = 0; k < B::NDEV; ++k) p.mx[k] = std::max(p.mx[k], ext[k]);
        p.mx_in = std::max(p.mx_in, in_b);
        p.mx_tot = std::max(p.mx_tot, (size_t)g * 4 * sizeof(unsigned long long));
    }
    return chain_plan_check(p, req, scans, how, dsp, post_ops, n_post);
}

// Both sets sized for the largest unit while they are idle (a call ends drained; the page-locked stream staging alone grows while the call runs,
// see download), then the call-wide tables -- colour table, page table, weights: one upload each on the copy stream in front of every unit's up event.
static int pages_reserve(ChainPagesState& ps, const ChainPlan& p, bool any_pageable, const uint8_t* lut, int n_lut, const pseg_scan* scans, hipStream_t s_in) {
    for (PagesSet& s : ps.set) {
        for (int k = 0; k < PagesSet::NDEV; ++k)
            if (p.mx[k]) PSEG_TRY(s.d[k].ensure(p.mx[k], "page chain staging"));
        if (any_pageable) PSEG_TRY(s.h_in.ensure(p.mx_in, "page chain staging"));
        PSEG_TRY(s.h_tot.ensure(std::max<size_t>(p.mx_tot, 64), "page chain staging"));
        if (p.mx_rg_pin) PSEG_TRY(s.h_rg.ensure(p.mx_rg_pin, "page chain staging"));
    }
    if (lut) {
        PSEG_TRY(ps.d_lut.ensure(768, "page chain colour table"));
        PSEG_HIP(hipMemcpyAsync(ps.d_lut.p, lut, (size_t)n_lut * 3, hipMemcpyHostToDevice, s_in));
    }
    if (p.mixed) {
        const size_t nb = (size_t)p.n * sizeof(MixedPage);
        PSEG_TRY(ps.d_tab.ensure(nb, "page chain page table"));
        PSEG_TRY(ps.h_tab.ensure(nb, "page chain page table"));
        memcpy(ps.h_tab.p, p.tab.data(), nb);
        PSEG_HIP(hipMemcpyAsync(ps.d_tab.p, ps.h_tab.p, nb, hipMemcpyHostToDevice, s_in));
    }
    if (scans && p.n_wt) {
        PSEG_TRY(ps.d_wt.ensure(p.n_wt * 8, "scan chain weights"));
        PSEG_TRY(ps.h_wt.ensure(p.n_wt * 8, "scan chain weights"));
        for (int i = 0; i < p.n; ++i) scan_front_weights(scans[p.ord[i]], (double*)ps.h_wt.p + p.wt_off[i]);
        PSEG_HIP(hipMemcpyAsync(ps.d_wt.p, ps.h_wt.p, p.n_wt * 8, hipMemcpyHostToDevice, s_in));
    }
    return PSEG_OK;
}

// The page chain's stages of run_pipeline: unit u in set u % 2.  imgs[i] is page i -- a scan call: scan i's gray plane, and binaries
// stands for the ink map that the front end makes on the device.
struct PagesRun {
    typedef PagesSet B;
    pseg_engine* h;
    const ChainPlan& p;
    ChainPagesState& ps;
    const std::vector<ChainReq>& req;
    const uint8_t* const* imgs; const uint8_t* const* binaries; const pseg_scan* scans; const pseg_binarize* how; const pseg_despeckle* dsp;
    const int* post_ops; int n_post; bool exact;
    const uint8_t* lut; int n_lut, level, nout; const int* mask_id; bool want_lab;      // lut NULL: no masks
    pseg_chain_sink sink; void* user;
    hipStream_t s_in, st, s_out;
    // where a unit's outputs lie in its page-locked slot: per page the requested streams (8-byte aligned), then the label map (and the
    // sizes, copied out of the set's page-locked words: those are written again by the unit after next while this one is delivered)
    std::vector<size_t> offs[2], tot[2];
    // the regions stage (p.rg): the layout of the unit's workspace; per page where its rows, vertex counts, offsets and vertices lie in the
    // page-locked slot; the counts and map records, copied out of the set's page-locked words for the same reason; the blob under way
    RgStageLay rg_lay[2];
    std::vector<size_t> rg_of[2];
    std::vector<int> rg_cnt[2];
    std::vector<long long> rg_mapv[2];
    std::vector<int32_t> rg_blob;

    static uint8_t* final_map(const PagesSet& s, const MixedPage& m) { return s.d[m.pred_sel ? B::LAB2 : B::LAB].p + m.pred_off; }
    bool pinned(int pi) const { return host_is_pinned(imgs[pi]) && (scans || !req[pi].need_bin || host_is_pinned(binaries[pi])); }
    bool unit_pinned(int u) const { bool all = true; for (int k = 0; k < p.ug[u]; ++k) all = all && pinned(p.ord[p.ub[u] + k]); return all; }
    int reserve() {
        bool any_pageable = false;
        for (int i = 0; i < p.n && !any_pageable; ++i) any_pageable = !pinned(i);
        return pages_reserve(ps, p, any_pageable, lut, n_lut, scans, s_in);
    }
    int upload_scans(int u, const PipeSet& ev) {      // a scan call's upload(u): the unit's scans into the set's SCAN block
        PagesSet& s = ps.set[u & 1];
        const int i0 = p.ub[u], g = p.ug[u];
        const bool direct = unit_pinned(u);
        if (!direct) PSEG_HIP(hipEventSynchronize(ev.up));     // the page-locked slot: last read by the uploads of unit u - 2
        size_t hp = 0;
        for (int i = i0; i < i0 + g; ++i) {
            const pseg_scan& sc = scans[p.ord[i]];
            const size_t nb = (size_t)sc.H0 * sc.W0;
            const uint8_t* src = sc.gray;
            if (!direct) { memcpy(s.h_in.p + hp, sc.gray, nb); src = s.h_in.p + hp; hp += nb; }
            PSEG_HIP(hipMemcpyAsync(s.d[B::SCAN].p + p.scan_off[i], src, nb, hipMemcpyHostToDevice, s_in));
        }
        return PSEG_OK;
    }
    int upload(int u, const PipeSet& ev) {
        if (scans) return upload_scans(u, ev);
        PagesSet& s = ps.set[u & 1];
        const int i0 = p.ub[u], i1 = i0 + p.ug[u];
        const bool bin = req[p.ord[i0]].need_bin;               // (the same for every page of a call)
        if (unit_pinned(u)) {
            for (int i = i0; i < i1; ++i) {
                const MixedPage& m = p.tab[i];
                PSEG_HIP(hipMemcpyAsync(s.d[B::IMG].p + m.img_off, imgs[p.ord[i]], (size_t)m.H * m.W * p.in_ch, hipMemcpyHostToDevice, s_in));
                if (bin) PSEG_HIP(hipMemcpyAsync(s.d[B::BIN].p + m.bin_off, binaries[p.ord[i]], (size_t)m.Hl * m.Wl, hipMemcpyHostToDevice, s_in));
            }
            return PSEG_OK;
        }
        PSEG_HIP(hipEventSynchronize(ev.up));                  // through the page-locked slot: last read by the uploads of unit u - 2
        size_t hp = 0;                                         // the pages densely, the binarisations densely behind them
        for (int pass = 0; pass < (bin ? 2 : 1); ++pass)
            for (int i = i0; i < i1; ++i) {
                const size_t nb = pass ? (size_t)p.tab[i].Hl * p.tab[i].Wl : (size_t)p.tab[i].H * p.tab[i].W * p.in_ch;
                memcpy(s.h_in.p + hp, pass ? binaries[p.ord[i]] : imgs[p.ord[i]], nb);
                hp += nb;
            }
        hp = 0;                                                // same-shape pages lie densely in IMG too: one DMA; a mixed unit's start at aligned offsets
        for (int pass = 0; pass < (bin ? 2 : 1); ++pass)
            for (int i = i0; i < i1; ++i) {
                const MixedPage& m = p.tab[i];
                const size_t nb = pass ? (size_t)m.Hl * m.Wl : (size_t)m.H * m.W * p.in_ch;
                if (pass) PSEG_HIP(hipMemcpyAsync(s.d[B::BIN].p + m.bin_off, s.h_in.p + hp, nb, hipMemcpyHostToDevice, s_in));
                else if (p.mixed) PSEG_HIP(hipMemcpyAsync(s.d[B::IMG].p + m.img_off, s.h_in.p + hp, nb, hipMemcpyHostToDevice, s_in));
                else if (i + 1 == i1) PSEG_HIP(hipMemcpyAsync(s.d[B::IMG].p, s.h_in.p, hp + nb, hipMemcpyHostToDevice, s_in));
                hp += nb;
            }
        return PSEG_OK;
    }
    int before_compute(int u) {
        // a canvas change re-allocates / clears the activation tensors: the previous unit must have left them
        const Engine& e = h->e;
        const MixedPage& m = p.tab[p.ub[u]];
        if (round_up(m.H, 32) != e.Hp || round_up(m.W, 32) != e.Wp || (p.un[u].slots && p.ug[u] > e.pages)) PSEG_HIP(hipStreamSynchronize(st));
        return PSEG_OK;
    }
    // 0. a scan call: the front end per scan writes the page and the ink map of the final shape
    int front_end(int u, PagesSet& s) {
        const int i0 = p.ub[u], g = p.ug[u];
        PSEG_HIP(hipMemsetAsync(s.d[B::REC].p, 0, (size_t)g * SCAN_REC_WORDS * sizeof(unsigned), st));
        for (int i = i0; i < i0 + g; ++i) {
            const int pi = p.ord[i];
            const MixedPage& m = p.tab[i];
            uint8_t* const ink = req[pi].need_bin ? s.d[B::BIN].p + m.bin_off : nullptr;
            const bool hi = scans[pi].final_is_scan != 0;
            PSEG_TRY(scan_front_enqueue(scans[pi], s.d[B::SCAN].p + p.scan_off[i], ps.d_wt.p ? (double*)ps.d_wt.p + p.wt_off[i] : nullptr,
                                        s.d[B::FILT].p ? s.d[B::FILT].p + p.filt_off[i] : nullptr, (unsigned*)s.d[B::REC].p + (size_t)(i - i0) * SCAN_REC_WORDS,
                                        s.d[B::IMG].p + m.img_off, hi ? nullptr : ink, hi ? ink : nullptr, st, binarize_of(how, pi), despeckle_of(dsp, pi)));
        }
        return PSEG_OK;
    }
    // 1. the network, in one of three forms
    int network(int u, PagesSet& s) {
        Engine& e = h->e;
        const int i0 = p.ub[u], g = p.ug[u];
        const MixedPage* d_tab = (const MixedPage*)ps.d_tab.p + i0;
        if (p.un[u].slots && p.mixed) {
            // pad every page into its canvas-sized slot, run the slots, crop every label map back to its page: three steps whatever g
            const int Hc = round_up(p.tab[i0].H, 32), Wc = round_up(p.tab[i0].W, 32);
            const size_t cpx = (size_t)Hc * Wc;
            const unsigned bx = (unsigned)std::min<size_t>((cpx * e.in_ch / 4 + 255) / 256, 1024);
            pages_pad_kernel<<<dim3(bx, g), 256, 0, st>>>(s.d[B::IMG].p, s.d[B::PAD].p, d_tab, Hc, Wc, e.in_ch);
            PSEG_HIP(hipGetLastError());
            PSEG_TRY(predict_device_pages(e, s.d[B::PAD].p, g, Hc, Wc, nullptr, s.d[B::CLAB].p, st));
            pages_crop_kernel<<<dim3((unsigned)std::min<size_t>((cpx + 255) / 256, 1024), g), 256, 0, st>>>(s.d[B::CLAB].p, s.d[B::LAB].p, d_tab, Hc, Wc);
            PSEG_HIP(hipGetLastError());
        } else if (p.un[u].slots) PSEG_TRY(predict_device_pages(e, s.d[B::IMG].p, g, p.tab[i0].H, p.tab[i0].W, nullptr, s.d[B::LAB].p, st));
        else
            for (int i = i0; i < i0 + g; ++i) {                // (a mixed unit's pages share the canvas: no change between them)
                const MixedPage& m = p.tab[i];
                const uint8_t* im = s.d[B::IMG].p + m.img_off;
                uint8_t* lab = s.d[B::LAB].p + m.lab_off;
                if (exact) PSEG_TRY(pseg_predict_exact_labels_device(h, im, m.H, m.W, lab, nullptr, nullptr, st));
                else PSEG_TRY(predict_device(e, im, m.H, m.W, nullptr, nullptr, nullptr, lab, st, nullptr));
            }
        return PSEG_OK;
    }
    // 2./3. per page, in chain_run's order: resize, then the post-processors (the vote's workspace is one per device)
    int post(int u, PagesSet& s) {
        for (int i = p.ub[u]; i < p.ub[u] + p.ug[u]; ++i) {
            const MixedPage& m = p.tab[i];
            uint8_t* const bufA = p.two_maps ? s.d[B::LAB2].p + p.lab2_off[i] : nullptr;
            uint8_t* const bufB = p.two_maps ? bufA + up256((size_t)m.Hl * m.Wl) : nullptr;
            PSEG_TRY(chain_post_enqueue(h->e, s.d[B::LAB].p + m.lab_off, bufA, bufB, s.d[B::BIN].p + m.bin_off, m.H, m.W, m.Hl, m.Wl, req[p.ord[i]].resize,
                                        post_ops, n_post, st, nullptr));
        }
        return PSEG_OK;
    }
    // 4. the masks of all pages as PNG streams: one set of launches; the sizes go to page-locked memory
    int encode(int u, PagesSet& s) {
        const int i0 = p.ub[u], g = p.ug[u];
        const MixedPage* t = &p.tab[i0];
        if (p.mixed)
            PSEG_TRY(png_pages_enqueue_mixed(p.un[u].M, t, (const MixedPage*)ps.d_tab.p + i0, g, s.d[B::PNG].p, s.d[B::PNG].cap, s.d[B::LAB].p, s.d[B::LAB2].p,
                                             s.d[B::BIN].p, ps.d_lut.p, n_lut, level, nout, mask_id, st));
        else
            PSEG_TRY(png_pages_enqueue(p.un[u].L, s.d[B::PNG].p, final_map(s, t[0]), g > 1 ? (size_t)(t[1].pred_off - t[0].pred_off) : 0, s.d[B::BIN].p,
                                       up256((size_t)t[0].Hl * t[0].Wl), ps.d_lut.p, n_lut, t[0].Hl, t[0].Wl, level, nout, mask_id, g, st));
        PSEG_HIP(hipMemcpyAsync(s.h_tot.p, s.d[B::PNG].p, (size_t)g * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        return PSEG_OK;
    }
    // 5. the text regions of the unit's final maps, where they lie: the stage of pseg_regions.hip and its tracer; the counts and the map
    // records go to page-locked memory, as the streams' sizes do
    int regions(int u, PagesSet& s) {
        const int i0 = p.ub[u], g = p.ug[u];
        std::vector<const uint8_t*> lab(g);
        std::vector<int> Hl(g), Wl(g);
        std::vector<pseg_regions> hw(g);
        for (int k = 0; k < g; ++k) {
            const MixedPage& m = p.tab[i0 + k];
            lab[k] = final_map(s, m); Hl[k] = m.Hl; Wl[k] = m.Wl; hw[k] = p.rg[p.ord[i0 + k]];
        }
        RgStageLay& L = rg_lay[u & 1];
        uint8_t* const d = s.d[B::RGN].p;
        // the buffers' real capacities go along: the stage refuses a layout that outgrows them, whatever the plan said
        const size_t rec_b = up256((size_t)g * 4) + up256((size_t)g * RG_MAPV * 8);
        if (s.h_rg.cap < rec_b) return fail(PSEG_EHIP, "page chain: the regions records of unit %d outgrow their staging", u);
        PSEG_TRY(rg_stage_enqueue(st, d, s.h_rg.p, g, lab.data(), Hl.data(), Wl.data(), hw.data(), p.rg_R, p.rg_V, s.d[B::RGN].cap, s.h_rg.cap - rec_b, &L));
        PSEG_HIP(hipMemcpyAsync(s.h_rg.p + L.tab_bytes, d + L.cnt, (size_t)g * 4, hipMemcpyDeviceToHost, st));
        PSEG_HIP(hipMemcpyAsync(s.h_rg.p + L.tab_bytes + up256((size_t)g * 4), d + L.mapv, (size_t)g * RG_MAPV * 8, hipMemcpyDeviceToHost, st));
        return PSEG_OK;
    }
    int compute(int u, const PipeSet&) {
        PagesSet& s = ps.set[u & 1];
        if (scans) PSEG_TRY(front_end(u, s));
        PSEG_TRY(network(u, s));
        PSEG_TRY(post(u, s));
        if (nout > 0) PSEG_TRY(encode(u, s));
        return p.rg ? regions(u, s) : PSEG_OK;
    }
    int download(int u, const PipeSet& ev) {
        PagesSet& s = ps.set[u & 1];
        const int i0 = p.ub[u], g = p.ug[u];
        const PngPages& L = p.un[u].L;
        PSEG_HIP(hipEventSynchronize(ev.done));                // the sizes are here
        const unsigned long long* h_tot = (const unsigned long long*)s.h_tot.p;
        std::vector<size_t>& of = offs[u & 1];
        of.assign((size_t)g * 5 + 1, 0);
        std::vector<size_t>& tt = tot[u & 1];
        tt.assign((size_t)g * 4, 0);
        size_t pos = 0;
        for (int k = 0; k < g; ++k) {
            const size_t bound = p.mixed ? (size_t)p.tab[i0 + k].bound : L.bound;
            for (int j = 0; j < 4; ++j) {
                of[(size_t)k * 5 + j] = pos;
                if (j >= nout) continue;
                const unsigned long long t = h_tot[(size_t)k * 4 + j];
                if (t < 80 || t > bound) return fail(PSEG_EHIP, "png: encoded size %llu outside (0, bound %zu] (page %d)", t, bound, p.ord[i0 + k]);
                tt[(size_t)k * 4 + j] = (size_t)t;
                pos += ((size_t)t + 7) & ~(size_t)7;
            }
            of[(size_t)k * 5 + 4] = pos;
            if (want_lab) pos += ((size_t)p.tab[i0 + k].Hl * p.tab[i0 + k].Wl + 7) & ~(size_t)7;
        }
        of[(size_t)g * 5] = pos;
        const RgStageLay& RL = rg_lay[u & 1];
        if (p.rg) {                                            // per page exactly what it holds: rows, vertex counts, offsets, vertices
            const int* h_cnt = (const int*)(s.h_rg.p + RL.tab_bytes);
            const long long* h_mapv = (const long long*)(s.h_rg.p + RL.tab_bytes + up256((size_t)g * 4));
            rg_cnt[u & 1].assign(h_cnt, h_cnt + g);
            rg_mapv[u & 1].assign(h_mapv, h_mapv + (size_t)g * RG_MAPV);
            std::vector<size_t>& ro = rg_of[u & 1];
            ro.assign((size_t)g * 4, 0);
            for (int k = 0; k < g; ++k) {
                const int c = h_cnt[k];
                const size_t cc = c < 0 || c > p.rg_R ? 0 : (size_t)c;
                const long long tv = h_mapv[(size_t)k * RG_MAPV];
                if (tv < 0 || (h_mapv[(size_t)k * RG_MAPV + 3] && tv > p.rg_V)) return fail(PSEG_EHIP, "regions: page %d reports %lld vertices", p.ord[i0 + k], tv);
                ro[(size_t)k * 4] = pos; pos += cc * RG_ROW_INTS * 4;
                ro[(size_t)k * 4 + 1] = pos; pos += cc * 8;
                ro[(size_t)k * 4 + 2] = pos; pos += cc * 8;
                ro[(size_t)k * 4 + 3] = pos; pos += h_mapv[(size_t)k * RG_MAPV + 3] ? (size_t)tv * 8 : 0;
            }
        }
        // the slot was handed to the sink by finish(u - 2): idle.  It grows to what units really hold, with a quarter of headroom.
        if (s.h_out.cap < pos) PSEG_TRY(s.h_out.ensure(pos + pos / 4 + 4096, "page chain streams"));
        for (int k = 0; k < g; ++k) {
            const MixedPage& m = p.tab[i0 + k];
            for (int j = 0; j < nout; ++j) {
                const uint8_t* src = p.mixed ? s.d[B::PNG].p + m.ws_off + (size_t)j * m.per + m.slots_b + m.meta_b + m.offs_b
                                             : s.d[B::PNG].p + L.head + (size_t)(g > 1 ? k : 0) * L.page + (size_t)j * L.per + L.slots_b + L.meta_b + L.offs_b;
                PSEG_HIP(hipMemcpyAsync(s.h_out.p + of[(size_t)k * 5 + j], src, tt[(size_t)k * 4 + j], hipMemcpyDeviceToHost, s_out));
            }
            if (want_lab) PSEG_HIP(hipMemcpyAsync(s.h_out.p + of[(size_t)k * 5 + 4], final_map(s, m), (size_t)m.Hl * m.Wl, hipMemcpyDeviceToHost, s_out));
            if (p.rg) {
                const std::vector<size_t>& ro = rg_of[u & 1];
                const uint8_t* const d = s.d[B::RGN].p;
                const size_t r0 = (size_t)k * p.rg_R, cc = (ro[(size_t)k * 4 + 2] - ro[(size_t)k * 4 + 1]) / 8;
                const size_t nvb = rg_mapv[u & 1][(size_t)k * RG_MAPV + 3] ? (size_t)rg_mapv[u & 1][(size_t)k * RG_MAPV] * 8 : 0;
                if (cc) {
                    PSEG_HIP(hipMemcpyAsync(s.h_out.p + ro[(size_t)k * 4], d + RL.rows + r0 * RG_ROW_INTS * 4, cc * RG_ROW_INTS * 4, hipMemcpyDeviceToHost, s_out));
                    PSEG_HIP(hipMemcpyAsync(s.h_out.p + ro[(size_t)k * 4 + 1], d + RL.nv + r0 * 8, cc * 8, hipMemcpyDeviceToHost, s_out));
                    PSEG_HIP(hipMemcpyAsync(s.h_out.p + ro[(size_t)k * 4 + 2], d + RL.voff + r0 * 8, cc * 8, hipMemcpyDeviceToHost, s_out));
                }
                if (nvb) PSEG_HIP(hipMemcpyAsync(s.h_out.p + ro[(size_t)k * 4 + 3], d + RL.xy + (size_t)k * p.rg_V * 8, nvb, hipMemcpyDeviceToHost, s_out));
            }
        }
        return PSEG_OK;
    }
    bool has_finish(int) const { return true; }
    int finish(int u) {                        // chunk CRCs, then the sink: the planner's order, `which` ascending; on the calling thread
        const PagesSet& s = ps.set[u & 1];
        const std::vector<size_t>& of = offs[u & 1];
        for (int k = 0; k < p.ug[u]; ++k) {
            const int pi = p.ord[p.ub[u] + k];
            const MixedPage& m = p.tab[p.ub[u] + k];
            for (int j = 0; j < nout; ++j) {
                uint8_t* out = s.h_out.p + of[(size_t)k * 5 + j];
                const size_t t = tot[u & 1][(size_t)k * 4 + j];
                PSEG_TRY(png_finish_host(out, t));
                if (sink(user, pi, mask_id[j], out, t) != 0) return fail(PSEG_ECALLBACK, "the sink stopped the call at page %d, output %d", pi, mask_id[j]);
            }
            if (want_lab && sink(user, pi, 4, s.h_out.p + of[(size_t)k * 5 + 4], (size_t)m.Hl * m.Wl) != 0)
                return fail(PSEG_ECALLBACK, "the sink stopped the call at page %d, output 4", pi);
            if (p.rg) {
                const std::vector<size_t>& ro = rg_of[u & 1];
                rg_stage_blob(rg_cnt[u & 1][k], p.rg_R, p.rg_V, &rg_mapv[u & 1][(size_t)k * RG_MAPV], (int32_t*)(s.h_out.p + ro[(size_t)k * 4]),
                              (const long long*)(s.h_out.p + ro[(size_t)k * 4 + 1]), (const long long*)(s.h_out.p + ro[(size_t)k * 4 + 2]),
                              (const int32_t*)(s.h_out.p + ro[(size_t)k * 4 + 3]), rg_blob);
                if (sink(user, pi, 5, (const uint8_t*)rg_blob.data(), rg_blob.size() * 4) != 0)
                    return fail(PSEG_ECALLBACK, "the sink stopped the call at page %d, output 5", pi);
            }
        }
        return PSEG_OK;
    }
};

// The body of the page-list entries (pages, mixed pages; scans != NULL: pseg_predict_chain_scans_png, where H, W, Ho, Wo are the
// pages' shapes as for the page entries).
static int chain_pages_run(pseg_engine* h, int n, const uint8_t* const* imgs, const int* H, const int* W, const int* Ho, const int* Wo,
                           const uint8_t* const* binaries, const int* post_ops, int n_post, unsigned flags, const uint8_t* lut, int n_lut, int level,
                           unsigned want, int unit_cap, pseg_chain_sink sink, void* user, const bool mixed, const pseg_scan* scans = nullptr,
                           const pseg_binarize* how = nullptr, const pseg_despeckle* dsp = nullptr, const pseg_regions* rg = nullptr, int max_regions = 0,
                           int max_vertices = 0) {
    if (!h) return fail(PSEG_EINVAL, "NULL engine");
    KnobScope knob_scope(h->e);
    Engine& e = h->e;
    if (n < 0 || (n > 0 && (!imgs || !H || !W))) return fail(PSEG_EINVAL, "bad argument");
    if (scans && (e.in_ch != 1 || !mixed)) return fail(PSEG_EUNSUPPORTED, "the scan chain takes an engine with one input channel (this one has %d)", e.in_ch);
    if (!sink) return fail(PSEG_EINVAL, "NULL sink");
    if (want == 0 || (want & ~(rg ? 63u : 31u)))
        return fail(PSEG_EINVAL, "want 0x%x: bits 0..3 select the masks, bit 4 the label map%s, at least one", want, rg ? ", bit 5 the text regions" : "");
    if (!(want & 32u)) rg = nullptr;                           // the stage runs only where it is asked for
    if (rg && (max_regions < 1 || max_vertices < 0 || (int64_t)max_regions * 64 * RG_ROW_INTS > 0x7fffffffLL))
        return fail(PSEG_EINVAL, "regions: max_regions %d, max_vertices %d", max_regions, max_vertices);
    if (unit_cap < 0 || unit_cap > 64) return fail(PSEG_EINVAL, "unit_cap %d (0 = default, at most 64)", unit_cap);
    int mask_id[4] = {0, 0, 0, 0}, nout = 0;
    for (int k = 0; k < 4; ++k)
        if (want & (1u << k)) mask_id[nout++] = k;
    const bool want_png = nout > 0;
    // every page is checked before any device work starts
    std::vector<ChainReq> req(n);
    for (int i = 0; i < n; ++i) {
        PSEG_TRY(chain_check(e, i, imgs[i], H[i], W[i], Ho ? Ho[i] : 0, Wo ? Wo[i] : 0, binaries ? binaries[i] : nullptr, post_ops, n_post, flags,
                             want_png, want_png, lut, n_lut, level, &req[i]));
        if (want_png && pseg_png_bound_lv(req[i].Hl, req[i].Wl, 3, 0, level) == 0) return fail(PSEG_EINVAL, "page %d: png: a row of %d pixels is too long", i, req[i].Wl);
        if (mixed && (H[i] > 0x7FFFFFE0 || W[i] > 0x7FFFFFE0)) return fail(PSEG_EINVAL, "page %d: bad shape %d x %d", i, H[i], W[i]);
        if (rg) {
            PSEG_TRY(rg_stage_check(rg[i], "page", i));
            if ((int64_t)req[i].Hl * req[i].Wl > 0x7fffffffLL) return fail(PSEG_EUNSUPPORTED, "page %d: map too large for the regions", i);
        }
    }
    if (n == 0) return PSEG_OK;
    PSEG_HIP(hipSetDevice(e.device));
    PSEG_TRY(chain_state(e));
    ChainState& c = *(ChainState*)e.chain;
    if (!c.pages) c.pages = new ChainPagesState();
    for (PipeSet& s : c.pages->ev) PSEG_TRY(s.create());
    hipStream_t s_in = nullptr, s_out = nullptr;
    PSEG_TRY(batch_copy_streams(e, &s_in, &s_out));
    // units: pseg_predict_batch's rule over (H, W, final H, final W), or over the canvas.  A bf16 engine's unit goes through the network
    // as page slots (run_bf16_pages) unless the label-exact mode is asked for; any unit's masks are encoded in one set of launches.
    const bool exact = (flags & PSEG_CHAIN_EXACT_LABELS) && e.mode == PSEG_MODE_BF16;
    int cap = batch_unit_cap(e, n, H, W);     // (uploads the weights: the plans decide whether pages travel as page slots)
    if (cap < 0) return cap;
    const bool page_slots = !exact && pages_capable(e);
    if (unit_cap > 0) {
        cap = unit_cap;
        if (page_slots) {
            int hm = 0, wm = 0;
            for (int i = 0; i < n; ++i)
                if ((size_t)H[i] * W[i] > (size_t)hm * wm) { hm = H[i]; wm = W[i]; }
            cap = fit_unit_slots(e, hm, wm, cap);
        }
    } else if (!page_slots) cap = std::min(8, std::max(1, n / 4));       // (the encoder's launches still take a unit's pages together)
    ChainPlan plan;
    PSEG_TRY(chain_pages_plan(n, H, W, Ho, Wo, req, scans, how, dsp, post_ops, n_post, e.in_ch, cap, page_slots, mixed, level, nout, rg, max_regions, max_vertices, &plan));
    PagesRun run{h, plan, *c.pages, req, imgs, binaries, scans, how, dsp, post_ops, n_post, exact, want_png ? lut : nullptr, n_lut, level, nout, mask_id,
                 (want & 16u) != 0, sink, user, s_in, e.stream, s_out, {}, {}};
    PSEG_TRY(run_pipeline(run, (int)plan.ub.size(), c.pages->ev, s_in, e.stream, s_out));
    return engine_status(e, e.stream);
}

extern "C" int pseg_predict_chain_pages_png(pseg_engine* h, int n, const uint8_t* const* imgs, const int* H, const int* W, const int* Ho,
                                            const int* Wo, const uint8_t* const* binaries, const int* post_ops, int n_post, unsigned flags,
                                            const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap, pseg_chain_sink sink,
                                            void* user) {
    return pseg_predict_chain_pages_regions_png(h, n, imgs, H, W, Ho, Wo, binaries, post_ops, n_post, flags, lut, n_lut, level, want, unit_cap, 0, nullptr, 0, 0,
                                                sink, user);
}

extern "C" int pseg_predict_chain_pages_mixed_png(pseg_engine* h, int n, const uint8_t* const* imgs, const int* H, const int* W, const int* Ho,
                                                  const int* Wo, const uint8_t* const* binaries, const int* post_ops, int n_post, unsigned flags,
                                                  const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap, pseg_chain_sink sink,
                                                  void* user) {
    return pseg_predict_chain_pages_regions_png(h, n, imgs, H, W, Ho, Wo, binaries, post_ops, n_post, flags, lut, n_lut, level, want, unit_cap, 1, nullptr, 0, 0,
                                                sink, user);
}

extern "C" int pseg_predict_chain_pages_regions_png(pseg_engine* h, int n, const uint8_t* const* imgs, const int* H, const int* W, const int* Ho,
                                                    const int* Wo, const uint8_t* const* binaries, const int* post_ops, int n_post, unsigned flags,
                                                    const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap, int mixed,
                                                    const pseg_regions* how, int max_regions, int max_vertices, pseg_chain_sink sink, void* user) {
    return chain_pages_run(h, n, imgs, H, W, Ho, Wo, binaries, post_ops, n_post, flags, lut, n_lut, level, want, unit_cap, sink, user, mixed != 0, nullptr,
                           nullptr, nullptr, how, max_regions, max_vertices);
}

extern "C" int pseg_predict_chain_scans_png(pseg_engine* h, int n, const pseg_scan* scans, const int* post_ops, int n_post, unsigned flags,
                                            const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap, pseg_chain_sink sink, void* user) {
    return pseg_predict_chain_scans_bin_png(h, n, scans, nullptr, post_ops, n_post, flags, lut, n_lut, level, want, unit_cap, sink, user);
}

extern "C" int pseg_predict_chain_scans_bin_png(pseg_engine* h, int n, const pseg_scan* scans, const pseg_binarize* how, const int* post_ops, int n_post,
                                                unsigned flags, const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap,
                                                pseg_chain_sink sink, void* user) {
    return pseg_predict_chain_scans_clean_png(h, n, scans, how, nullptr, post_ops, n_post, flags, lut, n_lut, level, want, unit_cap, sink, user);
}

extern "C" int pseg_predict_chain_scans_clean_png(pseg_engine* h, int n, const pseg_scan* scans, const pseg_binarize* how, const pseg_despeckle* dsp,
                                                  const int* post_ops, int n_post, unsigned flags, const uint8_t* lut, int n_lut, int level, unsigned want,
                                                  int unit_cap, pseg_chain_sink sink, void* user) {
    return pseg_predict_chain_scans_regions_png(h, n, scans, how, dsp, post_ops, n_post, flags, lut, n_lut, level, want, unit_cap, nullptr, 0, 0, sink, user);
}

extern "C" int pseg_predict_chain_scans_regions_png(pseg_engine* h, int n, const pseg_scan* scans, const pseg_binarize* how, const pseg_despeckle* dsp,
                                                    const int* post_ops, int n_post, unsigned flags, const uint8_t* lut, int n_lut, int level, unsigned want,
                                                    int unit_cap, const pseg_regions* rg, int max_regions, int max_vertices, pseg_chain_sink sink,
                                                    void* user) {
    if (n < 0 || (n > 0 && !scans)) return fail(PSEG_EINVAL, "bad argument");
    if (!sink) return fail(PSEG_EINVAL, "NULL sink");
    // every scan is checked before any device work starts; the pages' shapes then go through the page entries' checks
    std::vector<const uint8_t*> gray(n);
    std::vector<int> H(n), W(n), Ho(n), Wo(n);
    for (int i = 0; i < n; ++i) {
        PSEG_TRY(scan_front_check(scans[i], i));
        if (how) PSEG_TRY(binarize_check(how[i], i));
        if (dsp) PSEG_TRY(despeckle_check(dsp[i], i, "scan"));
        gray[i] = scans[i].gray;
        H[i] = scans[i].H;
        W[i] = scans[i].W;
        Ho[i] = scans[i].final_is_scan ? scans[i].H0 : 0;
        Wo[i] = scans[i].final_is_scan ? scans[i].W0 : 0;
    }
    return chain_pages_run(h, n, gray.data(), H.data(), W.data(), Ho.data(), Wo.data(), gray.data(), post_ops, n_post, flags, lut, n_lut, level, want,
                           unit_cap, sink, user, true, scans, how, dsp, rg, max_regions, max_vertices);
}
