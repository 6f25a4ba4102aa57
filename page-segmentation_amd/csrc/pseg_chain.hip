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

#include "pseg_common.h"

namespace pseg {

// One of the two staging sets of the page chain (pseg_predict_chain_pages_png): everything a unit of pages touches.
struct PagesSet {
    enum { IMG = 0, LAB = 1, LAB2 = 2, BIN = 3, PNG = 4, PAD = 5, CLAB = 6, SCAN = 7, FILT = 8, REC = 9, NDEV = 10 };
    // pages / network labels / resize + bbox ping-pong / binarisations / encoder workspace / mixed units: the pages padded to canvas-sized
    // page slots / the slots' canvas-sized label maps / scan chain: the unit's scans / their filtered planes / their records
    uint8_t* d[NDEV] = {};
    size_t d_bytes[NDEV] = {};
    uint8_t* h_in = nullptr;            // page-locked: pages and binarisations of callers with pageable arrays
    uint8_t* h_out = nullptr;           // page-locked: the unit's encoded streams (+ label maps), grown to the bytes units really have
    unsigned long long* h_tot = nullptr;   // page-locked: [pages][4] stream sizes
    size_t h_in_bytes = 0, h_out_bytes = 0, h_tot_bytes = 0;
    hipEvent_t up = nullptr, done = nullptr, down = nullptr;   // uploads landed / compute + sizes landed / downloads landed
};
struct ChainPagesState {
    PagesSet set[2];
    uint8_t* d_lut = nullptr;
    MixedPage* d_tab = nullptr;         // the page table of a mixed call (one entry per page of the list, in the planner's order) ...
    MixedPage* h_tab = nullptr;         // ... and its page-locked source
    size_t tab_entries = 0;
    double* d_wt = nullptr;             // the anti-aliasing weights of a scan call (every scan's, in the planner's order) ...
    double* h_wt = nullptr;             // ... and their page-locked source
    size_t wt_entries = 0;
};

struct ChainState {
    hipStream_t s_aux = nullptr;        // uploads of the binarisation / colour table beside the network's kernels
    hipEvent_t ev_aux = nullptr;
    uint8_t* d_buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ChainPagesState* pages = nullptr;
};
enum { CB_IMG = 0, CB_LAB = 1, CB_LAB2 = 2, CB_BIN = 3, CB_MASKS = 4, CB_LUT = 5, CB_I64 = 6 };

static int censure(ChainState& c, int slot, size_t bytes) {
    if (c.cap[slot] >= bytes && c.d_buf[slot]) return PSEG_OK;
    if (c.d_buf[slot]) (void)hipFree(c.d_buf[slot]);
    c.d_buf[slot] = nullptr;
    c.cap[slot] = 0;
    PSEG_HIP(hipMalloc((void**)&c.d_buf[slot], bytes));
    c.cap[slot] = bytes;
    return PSEG_OK;
}

// the staging sets' memory (device and page-locked); the events stay.  The caller has waited for the device.
static void pages_release(ChainPagesState& p) {
    if (p.d_tab) (void)hipFree(p.d_tab);
    if (p.h_tab) (void)hipHostFree(p.h_tab);
    p.d_tab = p.h_tab = nullptr;
    p.tab_entries = 0;
    if (p.d_wt) (void)hipFree(p.d_wt);
    if (p.h_wt) (void)hipHostFree(p.h_wt);
    p.d_wt = p.h_wt = nullptr;
    p.wt_entries = 0;
    for (PagesSet& s : p.set) {
        for (int i = 0; i < PagesSet::NDEV; ++i) { if (s.d[i]) (void)hipFree(s.d[i]); s.d[i] = nullptr; s.d_bytes[i] = 0; }
        if (s.h_in) (void)hipHostFree(s.h_in);
        if (s.h_out) (void)hipHostFree(s.h_out);
        if (s.h_tot) (void)hipHostFree(s.h_tot);
        s.h_in = s.h_out = nullptr;
        s.h_tot = nullptr;
        s.h_in_bytes = s.h_out_bytes = s.h_tot_bytes = 0;
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
        for (PagesSet& s : c->pages->set) {
            if (s.up) (void)hipEventDestroy(s.up);
            if (s.done) (void)hipEventDestroy(s.done);
            if (s.down) (void)hipEventDestroy(s.down);
        }
        if (c->pages->d_lut) (void)hipFree(c->pages->d_lut);
        delete c->pages;
    }
    for (int i = 0; i < 8; ++i) if (c->d_buf[i]) (void)hipFree(c->d_buf[i]);
    if (c->ev_aux) (void)hipEventDestroy(c->ev_aux);
    if (c->s_aux) (void)hipStreamDestroy(c->s_aux);
    delete c;
    e.chain = nullptr;
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
    const bool resize = req.resize, need_bin = req.need_bin;
    const int Hl = req.Hl, Wl = req.Wl;
    if (want_png) {
        const size_t bound = pseg_png_bound_lv(Hl, Wl, 3, 0, png->level);
        for (int k = 0; k < 4; ++k)
            if (png->out[k] && png->cap[k] < bound) return fail(PSEG_EINVAL, "png: output buffer %d of %zu bytes, pseg_png_bound is %zu", k, png->cap[k], bound);
    }
    PSEG_HIP(hipSetDevice(e.device));
    if (!e.chain) {
        auto* nc = new ChainState();
        e.chain = nc;
        PSEG_HIP(hipStreamCreateWithFlags(&nc->s_aux, hipStreamNonBlocking));
        PSEG_HIP(hipEventCreateWithFlags(&nc->ev_aux, hipEventDisableTiming));
    }
    ChainState& c = *(ChainState*)e.chain;
    hipStream_t st = e.stream;
    const size_t npx = (size_t)H * W, nl = (size_t)Hl * Wl;
    const size_t nla = (nl + 255) & ~(size_t)255;          // buffer stride: the mask / vote kernels want 4-byte aligned maps
    // a reallocation must not race with the previous call's work: every call ends synchronised, so the buffers are idle here
    PSEG_TRY(censure(c, CB_IMG, npx * e.in_ch));
    PSEG_TRY(censure(c, CB_LAB, npx));
    PSEG_TRY(censure(c, CB_LAB2, 2 * nla));          // resize target + bounding-box ping-pong
    if (need_bin) PSEG_TRY(censure(c, CB_BIN, nl));
    if (want_masks) { if (!want_png) PSEG_TRY(censure(c, CB_MASKS, 4 * nla * 3)); PSEG_TRY(censure(c, CB_LUT, (size_t)n_lut * 3)); }
    if (labels) PSEG_TRY(censure(c, CB_I64, nl * 8));
    // every way out -- also an error return in the middle -- ends with both streams drained: copies from / to the caller's host
    // arrays must not be in flight when the caller gets its buffers back
    struct Drain { hipStream_t a, b; ~Drain() { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); } } drain{st, c.s_aux};
    // uploads: the page on the engine's stream (the network waits for it anyway), binarisation and colour table beside it
    PSEG_HIP(hipMemcpyAsync(c.d_buf[CB_IMG], img, npx * e.in_ch, hipMemcpyHostToDevice, st));
    if (need_bin) PSEG_HIP(hipMemcpyAsync(c.d_buf[CB_BIN], binary, nl, hipMemcpyHostToDevice, c.s_aux));
    if (want_masks) PSEG_HIP(hipMemcpyAsync(c.d_buf[CB_LUT], lut, (size_t)n_lut * 3, hipMemcpyHostToDevice, c.s_aux));
    if (need_bin) PSEG_HIP(hipEventRecord(c.ev_aux, c.s_aux));
    // 1. the network: uint8 argmax labels (float32 engine: bit-exact; bf16 engine: throughput labels, or the label-exact mode)
    if ((flags & PSEG_CHAIN_EXACT_LABELS) && e.mode == PSEG_MODE_BF16)
        PSEG_TRY(pseg_predict_exact_labels_device(h, c.d_buf[CB_IMG], H, W, c.d_buf[CB_LAB], nullptr, nullptr, st));
    else
        PSEG_TRY(predict_device(e, c.d_buf[CB_IMG], H, W, nullptr, nullptr, nullptr, c.d_buf[CB_LAB], st, nullptr));
    uint8_t* cur = c.d_buf[CB_LAB];
    uint8_t* const bufA = c.d_buf[CB_LAB2];
    uint8_t* const bufB = c.d_buf[CB_LAB2] + nla;
    // 2. scale_to_original_shape: order-0 gather of the label map (preserving_resize(pred, original_shape))
    if (resize) {
        PSEG_TRY(pseg_resize_nearest_device(e.device, cur, H, W, 1, bufA, Hl, Wl, st));
        cur = bufA;
    }
    // 3. post-processors, in order
    if (need_bin) PSEG_HIP(hipStreamWaitEvent(st, c.ev_aux, 0));
    for (int i = 0; i < n_post; ++i) {
        if (post_ops[i] == PSEG_POST_CC_VOTE) {
            PSEG_TRY(pseg_cc_vote_device_u8(e.device, cur, c.d_buf[CB_BIN], Hl, Wl, e.n_classes, st));
        } else {
            uint8_t* const dst = cur == bufA ? bufB : bufA;
            PSEG_TRY(pseg_bbox_fill_device_u8(e.device, cur, dst, Hl, Wl, e.n_classes, st));
            cur = dst;
        }
    }
    // 4. outputs
    if (labels_u8) PSEG_HIP(hipMemcpyAsync(labels_u8, cur, nl, hipMemcpyDeviceToHost, st));
    if (labels) {
        chain_widen_kernel<<<(int)std::min<size_t>((nl + 255) / 256, 8192), 256, 0, st>>>(cur, (int64_t*)c.d_buf[CB_I64], nl);
        PSEG_HIP(hipMemcpyAsync(labels, c.d_buf[CB_I64], nl * 8, hipMemcpyDeviceToHost, st));
    }
    if (want_png) {
        // the band kernel selects the masks' pixels itself: the RGB masks are never written; synchronises `st`
        PSEG_TRY(pseg_masks_png_device_u8_lv(e.device, cur, c.d_buf[CB_BIN], c.d_buf[CB_LUT], n_lut, Hl, Wl, 0, png->level, png->out, png->cap, png->n_bytes, st));
    } else if (want_masks) {
        uint8_t* m = c.d_buf[CB_MASKS];
        uint8_t* dm[4] = {color ? m : nullptr, overlay ? m + nla * 3 : nullptr, inverted ? m + 2 * nla * 3 : nullptr, fg_color ? m + 3 * nla * 3 : nullptr};
        PSEG_TRY(pseg_masks_device_u8(e.device, cur, c.d_buf[CB_BIN], c.d_buf[CB_LUT], n_lut, Hl, Wl, dm[0], dm[1], dm[2], dm[3], st));
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
static int pages_ensure_dev(PagesSet& s, int slot, size_t bytes) {
    if (s.d_bytes[slot] >= bytes && s.d[slot]) return PSEG_OK;
    if (s.d[slot]) (void)hipFree(s.d[slot]);
    s.d[slot] = nullptr;
    s.d_bytes[slot] = 0;
    if (hipMalloc((void**)&s.d[slot], bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PSEG_ENOMEM, "hipMalloc(page chain staging, %zu bytes) failed", bytes);
    }
    s.d_bytes[slot] = bytes;
    return PSEG_OK;
}
template <class T>
static int pages_ensure_host(T** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes && *p) return PSEG_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipHostMalloc((void**)p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PSEG_ENOMEM, "hipHostMalloc(page chain staging, %zu bytes) failed", bytes);
    }
    *cap = bytes;
    return PSEG_OK;
}
static bool pages_is_pinned(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

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

// The body of the page-list entries.  mixed = false: units are runs of same-shape pages in list order (pseg_chain_units).  mixed = true:
// units are pages of one canvas (pseg_chain_units_mixed); `ord` maps a position of the planner's order to the caller's page.
// scans != NULL (pseg_predict_chain_scans_png; mixed): imgs[i] is scan i's gray plane and binaries[i] stands for the ink map that the
// front end makes on the device -- upload() brings the unit's scans, compute() starts with the front end (scan_front_enqueue), which
// writes the pages and ink maps where upload() puts them otherwise; H, W, Ho, Wo are the pages' shapes as for the page entries.
static int chain_pages_run(pseg_engine* h, int n, const uint8_t* const* imgs, const int* H, const int* W, const int* Ho, const int* Wo,
                           const uint8_t* const* binaries, const int* post_ops, int n_post, unsigned flags, const uint8_t* lut, int n_lut, int level,
                           unsigned want, int unit_cap, pseg_chain_sink sink, void* user, const bool mixed, const pseg_scan* scans = nullptr) {
    if (!h) return fail(PSEG_EINVAL, "NULL engine");
    KnobScope knob_scope(h->e);
    Engine& e = h->e;
    if (n < 0 || (n > 0 && (!imgs || !H || !W))) return fail(PSEG_EINVAL, "bad argument");
    if (scans && (e.in_ch != 1 || !mixed)) return fail(PSEG_EUNSUPPORTED, "the scan chain takes an engine with one input channel (this one has %d)", e.in_ch);
    if (!sink) return fail(PSEG_EINVAL, "NULL sink");
    if (want == 0 || (want & ~31u)) return fail(PSEG_EINVAL, "want 0x%x: bits 0..3 select the masks, bit 4 the label map, at least one", want);
    if (unit_cap < 0 || unit_cap > 64) return fail(PSEG_EINVAL, "unit_cap %d (0 = default, at most 64)", unit_cap);
    int mask_id[4] = {0, 0, 0, 0}, nout = 0;
    for (int k = 0; k < 4; ++k)
        if (want & (1u << k)) mask_id[nout++] = k;
    const bool want_lab = (want & 16u) != 0, want_png = nout > 0;
    // every page is checked before any device work starts
    std::vector<ChainReq> req(n);
    bool any_bin = false, two_maps = false;
    for (int i = 0; i < n; ++i) {
        PSEG_TRY(chain_check(e, i, imgs[i], H[i], W[i], Ho ? Ho[i] : 0, Wo ? Wo[i] : 0, binaries ? binaries[i] : nullptr, post_ops, n_post, flags,
                             want_png, want_png, lut, n_lut, level, &req[i]));
        if (want_png && pseg_png_bound_lv(req[i].Hl, req[i].Wl, 3, 0, level) == 0) return fail(PSEG_EINVAL, "page %d: png: a row of %d pixels is too long", i, req[i].Wl);
        if (mixed && (H[i] > 0x7FFFFFE0 || W[i] > 0x7FFFFFE0)) return fail(PSEG_EINVAL, "page %d: bad shape %d x %d", i, H[i], W[i]);
        any_bin |= req[i].need_bin;
        two_maps |= req[i].resize;
    }
    if (n == 0) return PSEG_OK;
    for (int i = 0; i < n_post; ++i) two_maps |= post_ops[i] == PSEG_POST_BBOX;
    PSEG_HIP(hipSetDevice(e.device));
    if (!e.chain) {
        auto* nc = new ChainState();
        e.chain = nc;
        PSEG_HIP(hipStreamCreateWithFlags(&nc->s_aux, hipStreamNonBlocking));
        PSEG_HIP(hipEventCreateWithFlags(&nc->ev_aux, hipEventDisableTiming));
    }
    ChainState& c = *(ChainState*)e.chain;
    if (!c.pages) c.pages = new ChainPagesState();
    ChainPagesState& ps = *c.pages;
    for (PagesSet& s : ps.set) {
        if (!s.up) PSEG_HIP(hipEventCreateWithFlags(&s.up, hipEventDisableTiming));
        if (!s.done) PSEG_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        if (!s.down) PSEG_HIP(hipEventCreateWithFlags(&s.down, hipEventDisableTiming));
    }
    hipStream_t s_in = nullptr, s_out = nullptr, st = e.stream;
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
    std::vector<int> ord, ub, ug;
    if (mixed) plan_units_mixed(n, H, W, cap, ord, ub, ug);
    else {
        ord.resize(n);
        for (int i = 0; i < n; ++i) ord[i] = i;
        plan_units(n, H, W, Ho, Wo, cap, ub, ug);
    }
    const int nu = (int)ub.size();
    // per position of the planner's order: where the page, its maps and its binarisation lie in the unit's staging set (tab; a mixed
    // call's kernels read it on the device); per unit: the encoder's layout
    struct Unit { bool slots; PngPages L; PngPagesMixed M; };
    std::vector<Unit> un(nu);
    std::vector<MixedPage> tab(n);
    std::vector<size_t> lab2_off(n, 0);
    // a scan call, per position: where the scan and its filtered plane lie in the set's SCAN / FILT blocks, its weights in the call's table
    std::vector<size_t> scan_off(scans ? n : 0, 0), filt_off(scans ? n : 0, 0), wt_off(scans ? n : 0, 0);
    size_t n_wt = 0;
    size_t mx[PagesSet::NDEV] = {}, mx_in = 0, mx_tot = 0;
    for (int u = 0; u < nu; ++u) {
        const int i0 = ub[u], g = ug[u], p0 = ord[i0];
        Unit& q = un[u];
        // (same-shape page slots write the unit's maps one behind the other; mixed slots are canvases, cropped to aligned maps)
        q.slots = page_slots && g > 1 && (mixed || ((size_t)H[p0] * W[p0]) % 4 == 0);
        q.L = PngPages{0, 0, 0, 0, 0, 0, 0, 0};
        q.M = PngPagesMixed{0, 0, 0};
        size_t o_img = 0, o_lab = 0, o_bin = 0, o_lab2 = 0, lab_b = 0, in_b = 0, o_scan = 0, o_filt = 0;
        for (int k = 0; k < g; ++k) {
            const int pi = ord[i0 + k];
            MixedPage& m = tab[i0 + k];
            memset(&m, 0, sizeof m);
            const size_t npx = (size_t)H[pi] * W[pi], nl = (size_t)req[pi].Hl * req[pi].Wl, nla = up256(nl);   // (the vote kernels want 4-byte aligned maps)
            m.H = H[pi]; m.W = W[pi]; m.Hl = req[pi].Hl; m.Wl = req[pi].Wl;
            m.img_off = o_img; m.lab_off = o_lab; m.bin_off = o_bin;
            lab2_off[i0 + k] = o_lab2;
            o_img += mixed ? up256(npx * e.in_ch) : npx * e.in_ch;
            o_lab += !mixed && q.slots ? npx : up256(npx);
            lab_b += up256(npx);
            o_bin += nla;
            o_lab2 += 2 * nla;
            in_b += scans ? (size_t)scans[pi].H0 * scans[pi].W0 : npx * e.in_ch + (req[pi].need_bin ? nl : 0);
            if (scans) {
                scan_off[i0 + k] = o_scan;
                filt_off[i0 + k] = o_filt;
                wt_off[i0 + k] = n_wt;
                o_scan += up256((size_t)scans[pi].H0 * scans[pi].W0);
                o_filt += scan_front_work(scans[pi]);
                n_wt += scan_front_weights(scans[pi], nullptr);
            }
            // where the page's final map will lie: compute()'s walk through resize and post-processors, ahead of time
            int where = req[pi].resize ? 1 : 0;                        // 0: LAB, 1: bufA, 2: bufB
            for (int i = 0; i < n_post; ++i)
                if (post_ops[i] == PSEG_POST_BBOX) where = where == 1 ? 2 : 1;
            m.pred_sel = where ? 1 : 0;
            m.pred_off = where == 0 ? m.lab_off : lab2_off[i0 + k] + (where == 2 ? nla : 0);
        }
        if (want_png) {
            if (mixed) PSEG_TRY(png_pages_layout_mixed(level, nout, g, &tab[i0], &q.M));
            else PSEG_TRY(png_pages_layout(req[p0].Hl, req[p0].Wl, level, nout, g, &q.L));
        }
        mx[PagesSet::IMG] = std::max(mx[PagesSet::IMG], o_img);
        mx[PagesSet::LAB] = std::max(mx[PagesSet::LAB], lab_b);
        if (two_maps) mx[PagesSet::LAB2] = std::max(mx[PagesSet::LAB2], o_lab2);
        if (any_bin) mx[PagesSet::BIN] = std::max(mx[PagesSet::BIN], o_bin);
        mx[PagesSet::PNG] = std::max(mx[PagesSet::PNG], mixed ? q.M.bytes : q.L.bytes);
        if (scans) {
            mx[PagesSet::SCAN] = std::max(mx[PagesSet::SCAN], o_scan);
            mx[PagesSet::FILT] = std::max(mx[PagesSet::FILT], o_filt);
            mx[PagesSet::REC] = std::max(mx[PagesSet::REC], (size_t)g * SCAN_REC_WORDS * sizeof(unsigned));
        }
        if (mixed && q.slots) {
            const size_t cpx = (size_t)round_up(H[p0], 32) * round_up(W[p0], 32);
            mx[PagesSet::PAD] = std::max(mx[PagesSet::PAD], (size_t)g * cpx * e.in_ch);
            mx[PagesSet::CLAB] = std::max(mx[PagesSet::CLAB], (size_t)g * cpx);
        }
        mx_in = std::max(mx_in, in_b);
        mx_tot = std::max(mx_tot, (size_t)g * 4 * sizeof(unsigned long long));
    }
    // every way out -- also an error return in the middle and a sink that says stop -- ends with the three streams drained
    struct Drain { hipStream_t a, b, c; ~Drain() { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); (void)hipStreamSynchronize(c); } } drain{s_in, st, s_out};
    // a reallocation must not race with work that uses the block: every call ends drained, so the sets are idle here, and they are
    // sized for the largest unit up front.  The page-locked stream staging alone grows while the call runs (see download).
    bool any_pageable = false;
    for (int i = 0; i < n && !any_pageable; ++i)
        any_pageable = !pages_is_pinned(imgs[i]) || (!scans && req[i].need_bin && !pages_is_pinned(binaries[i]));
    for (PagesSet& s : ps.set) {
        for (int k = 0; k < PagesSet::NDEV; ++k)
            if (mx[k]) PSEG_TRY(pages_ensure_dev(s, k, mx[k]));
        if (any_pageable) PSEG_TRY(pages_ensure_host(&s.h_in, &s.h_in_bytes, mx_in));
        PSEG_TRY(pages_ensure_host(&s.h_tot, &s.h_tot_bytes, std::max<size_t>(mx_tot, 64)));
    }
    if (want_png) {
        if (!ps.d_lut) PSEG_HIP(hipMalloc((void**)&ps.d_lut, 768));
        PSEG_HIP(hipMemcpyAsync(ps.d_lut, lut, (size_t)n_lut * 3, hipMemcpyHostToDevice, s_in));      // (ordered in front of every unit's up event)
    }
    if (mixed) {
        // the whole call's page table goes up once, on the copy stream, in front of every unit's up event: no unit waits for it
        if (ps.tab_entries < (size_t)n) {
            if (ps.d_tab) (void)hipFree(ps.d_tab);
            if (ps.h_tab) (void)hipHostFree(ps.h_tab);
            ps.d_tab = ps.h_tab = nullptr;
            ps.tab_entries = 0;
            if (hipMalloc((void**)&ps.d_tab, (size_t)n * sizeof(MixedPage)) != hipSuccess || hipHostMalloc((void**)&ps.h_tab, (size_t)n * sizeof(MixedPage), hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return fail(PSEG_ENOMEM, "page chain: no memory for the table of %d pages", n);
            }
            ps.tab_entries = (size_t)n;
        }
        memcpy(ps.h_tab, tab.data(), (size_t)n * sizeof(MixedPage));
        PSEG_HIP(hipMemcpyAsync(ps.d_tab, ps.h_tab, (size_t)n * sizeof(MixedPage), hipMemcpyHostToDevice, s_in));
    }
    if (scans && n_wt) {
        // the weights of the whole call, in the planner's order: one page-locked table, one upload in front of every unit's up event
        if (ps.wt_entries < n_wt) {
            if (ps.d_wt) (void)hipFree(ps.d_wt);
            if (ps.h_wt) (void)hipHostFree(ps.h_wt);
            ps.d_wt = ps.h_wt = nullptr;
            ps.wt_entries = 0;
            if (hipMalloc((void**)&ps.d_wt, n_wt * 8) != hipSuccess || hipHostMalloc((void**)&ps.h_wt, n_wt * 8, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return fail(PSEG_ENOMEM, "scan chain: no memory for the table of %zu weights", n_wt);
            }
            ps.wt_entries = n_wt;
        }
        for (int i = 0; i < n; ++i) scan_front_weights(scans[ord[i]], ps.h_wt + wt_off[i]);
        PSEG_HIP(hipMemcpyAsync(ps.d_wt, ps.h_wt, n_wt * 8, hipMemcpyHostToDevice, s_in));
    }
    auto upload_scans = [&](int u) -> int {    // a scan call's upload(u): the unit's scans into the set's SCAN block
        PagesSet& s = ps.set[u & 1];
        const int i0 = ub[u], g = ug[u];
        PSEG_HIP(hipStreamWaitEvent(s_in, s.done, 0));         // the set's scans have been read (unit u - 2)
        bool pinned = true;
        for (int k = 0; k < g; ++k) pinned = pinned && pages_is_pinned(imgs[ord[i0 + k]]);
        if (!pinned) PSEG_HIP(hipEventSynchronize(s.up));      // the page-locked slot: last read by the uploads of unit u - 2
        size_t hp = 0;
        for (int k = 0; k < g; ++k) {
            const pseg_scan& sc = scans[ord[i0 + k]];
            const size_t nb = (size_t)sc.H0 * sc.W0;
            const uint8_t* src = sc.gray;
            if (!pinned) { memcpy(s.h_in + hp, sc.gray, nb); src = s.h_in + hp; hp += nb; }
            PSEG_HIP(hipMemcpyAsync(s.d[PagesSet::SCAN] + scan_off[i0 + k], src, nb, hipMemcpyHostToDevice, s_in));
        }
        PSEG_HIP(hipEventRecord(s.up, s_in));
        return PSEG_OK;
    };
    auto upload = [&](int u) -> int {          // unit u -> set u % 2
        if (scans) return upload_scans(u);
        PagesSet& s = ps.set[u & 1];
        const int i0 = ub[u], g = ug[u];
        const bool bin = req[ord[i0]].need_bin;                 // (the same for every page of a call)
        PSEG_HIP(hipStreamWaitEvent(s_in, s.done, 0));         // the set's pages and binarisations have been read (unit u - 2)
        bool pinned = true;
        for (int k = 0; k < g; ++k) pinned = pinned && pages_is_pinned(imgs[ord[i0 + k]]) && (!bin || pages_is_pinned(binaries[ord[i0 + k]]));
        if (pinned) {
            for (int k = 0; k < g; ++k) {
                const MixedPage& m = tab[i0 + k];
                const int pi = ord[i0 + k];
                PSEG_HIP(hipMemcpyAsync(s.d[PagesSet::IMG] + m.img_off, imgs[pi], (size_t)m.H * m.W * e.in_ch, hipMemcpyHostToDevice, s_in));
                if (bin) PSEG_HIP(hipMemcpyAsync(s.d[PagesSet::BIN] + m.bin_off, binaries[pi], (size_t)m.Hl * m.Wl, hipMemcpyHostToDevice, s_in));
            }
        } else {                               // through the page-locked slot: last read by the uploads of unit u - 2
            PSEG_HIP(hipEventSynchronize(s.up));
            size_t hp = 0;                     // the pages densely, the binarisations densely behind them
            for (int k = 0; k < g; ++k) {
                const size_t pb = (size_t)tab[i0 + k].H * tab[i0 + k].W * e.in_ch;
                memcpy(s.h_in + hp, imgs[ord[i0 + k]], pb);
                hp += pb;
            }
            const size_t all_pages = hp;
            for (int k = 0; k < g && bin; ++k) {
                const size_t nl = (size_t)tab[i0 + k].Hl * tab[i0 + k].Wl;
                memcpy(s.h_in + hp, binaries[ord[i0 + k]], nl);
                hp += nl;
            }
            if (!mixed) PSEG_HIP(hipMemcpyAsync(s.d[PagesSet::IMG], s.h_in, all_pages, hipMemcpyHostToDevice, s_in));
            hp = 0;
            for (int k = 0; k < g && mixed; ++k) {             // (a mixed unit's pages start at aligned offsets)
                const size_t pb = (size_t)tab[i0 + k].H * tab[i0 + k].W * e.in_ch;
                PSEG_HIP(hipMemcpyAsync(s.d[PagesSet::IMG] + tab[i0 + k].img_off, s.h_in + hp, pb, hipMemcpyHostToDevice, s_in));
                hp += pb;
            }
            hp = all_pages;
            for (int k = 0; k < g && bin; ++k) {
                const size_t nl = (size_t)tab[i0 + k].Hl * tab[i0 + k].Wl;
                PSEG_HIP(hipMemcpyAsync(s.d[PagesSet::BIN] + tab[i0 + k].bin_off, s.h_in + hp, nl, hipMemcpyHostToDevice, s_in));
                hp += nl;
            }
        }
        PSEG_HIP(hipEventRecord(s.up, s_in));
        return PSEG_OK;
    };
    std::vector<uint8_t*> fin(n, nullptr);     // per position: the page's final label map
    auto compute = [&](int u) -> int {
        PagesSet& s = ps.set[u & 1];
        const Unit& q = un[u];
        const int i0 = ub[u], g = ug[u], Hc = round_up(H[ord[i0]], 32), Wc = round_up(W[ord[i0]], 32);
        // a canvas change re-allocates / clears the activation tensors: the previous unit must have left them
        if (Hc != e.Hp || Wc != e.Wp || (q.slots && g > e.pages)) PSEG_HIP(hipStreamSynchronize(st));
        PSEG_HIP(hipStreamWaitEvent(st, s.up, 0));
        PSEG_HIP(hipStreamWaitEvent(st, s.down, 0));           // the streams and maps of unit u - 2 have left the set
        // 0. a scan call: the front end per scan writes the page and the ink map of the final shape
        if (scans) {
            PSEG_HIP(hipMemsetAsync(s.d[PagesSet::REC], 0, (size_t)g * SCAN_REC_WORDS * sizeof(unsigned), st));
            for (int k = 0; k < g; ++k) {
                const int pi = ord[i0 + k];
                const MixedPage& m = tab[i0 + k];
                uint8_t* const ink = req[pi].need_bin ? s.d[PagesSet::BIN] + m.bin_off : nullptr;
                const bool hi = scans[pi].final_is_scan != 0;
                PSEG_TRY(scan_front_enqueue(scans[pi], s.d[PagesSet::SCAN] + scan_off[i0 + k], ps.d_wt ? ps.d_wt + wt_off[i0 + k] : nullptr,
                                            s.d[PagesSet::FILT] ? s.d[PagesSet::FILT] + filt_off[i0 + k] : nullptr,
                                            (unsigned*)s.d[PagesSet::REC] + (size_t)k * SCAN_REC_WORDS, s.d[PagesSet::IMG] + m.img_off,
                                            hi ? nullptr : ink, hi ? ink : nullptr, st));
            }
        }
        // 1. the network
        if (q.slots && mixed) {
            // pad every page into its canvas-sized slot, run the slots, crop every label map back to its page: three steps whatever g
            const size_t cpx = (size_t)Hc * Wc;
            if ((size_t)g * cpx * e.in_ch > s.d_bytes[PagesSet::PAD] || (size_t)g * cpx > s.d_bytes[PagesSet::CLAB])
                return fail(PSEG_EHIP, "page chain: the padded slots of unit %d outgrow their staging", u);
            const unsigned bx = (unsigned)std::min<size_t>((cpx * e.in_ch / 4 + 255) / 256, 1024);
            pages_pad_kernel<<<dim3(bx, g), 256, 0, st>>>(s.d[PagesSet::IMG], s.d[PagesSet::PAD], ps.d_tab + i0, Hc, Wc, e.in_ch);
            PSEG_HIP(hipGetLastError());
            PSEG_TRY(predict_device_pages(e, s.d[PagesSet::PAD], g, Hc, Wc, nullptr, s.d[PagesSet::CLAB], st));
            pages_crop_kernel<<<dim3((unsigned)std::min<size_t>((cpx + 255) / 256, 1024), g), 256, 0, st>>>(s.d[PagesSet::CLAB], s.d[PagesSet::LAB], ps.d_tab + i0, Hc, Wc);
            PSEG_HIP(hipGetLastError());
        } else if (q.slots) PSEG_TRY(predict_device_pages(e, s.d[PagesSet::IMG], g, H[ord[i0]], W[ord[i0]], nullptr, s.d[PagesSet::LAB], st));
        else
            for (int k = 0; k < g; ++k) {                      // (a mixed unit's pages share the canvas: no change between them)
                const MixedPage& m = tab[i0 + k];
                const uint8_t* im = s.d[PagesSet::IMG] + m.img_off;
                uint8_t* lab = s.d[PagesSet::LAB] + m.lab_off;
                if (exact) PSEG_TRY(pseg_predict_exact_labels_device(h, im, m.H, m.W, lab, nullptr, nullptr, st));
                else PSEG_TRY(predict_device(e, im, m.H, m.W, nullptr, nullptr, nullptr, lab, st, nullptr));
            }
        // 2./3. per page, in chain_run's order: resize, then the post-processors (the vote's workspace is one per device)
        for (int k = 0; k < g; ++k) {
            const MixedPage& m = tab[i0 + k];
            const size_t nla = up256((size_t)m.Hl * m.Wl);
            uint8_t* cur = s.d[PagesSet::LAB] + m.lab_off;
            uint8_t* const bufA = two_maps ? s.d[PagesSet::LAB2] + lab2_off[i0 + k] : nullptr;
            uint8_t* const bufB = two_maps ? bufA + nla : nullptr;
            if (req[ord[i0 + k]].resize) {
                PSEG_TRY(pseg_resize_nearest_device(e.device, cur, m.H, m.W, 1, bufA, m.Hl, m.Wl, st));
                cur = bufA;
            }
            for (int i = 0; i < n_post; ++i) {
                if (post_ops[i] == PSEG_POST_CC_VOTE) {
                    PSEG_TRY(pseg_cc_vote_device_u8(e.device, cur, s.d[PagesSet::BIN] + m.bin_off, m.Hl, m.Wl, e.n_classes, st));
                } else {
                    uint8_t* const dst = cur == bufA ? bufB : bufA;
                    PSEG_TRY(pseg_bbox_fill_device_u8(e.device, cur, dst, m.Hl, m.Wl, e.n_classes, st));
                    cur = dst;
                }
            }
            if (cur != s.d[m.pred_sel ? PagesSet::LAB2 : PagesSet::LAB] + m.pred_off) return fail(PSEG_EHIP, "page chain: the final map of page %d is not where the table says", ord[i0 + k]);
            fin[i0 + k] = cur;
        }
        // 4. the masks of all pages as PNG streams: one set of launches; the sizes go to page-locked memory
        if (want_png) {
            if (mixed)
                PSEG_TRY(png_pages_enqueue_mixed(q.M, &tab[i0], ps.d_tab + i0, g, s.d[PagesSet::PNG], s.d_bytes[PagesSet::PNG], s.d[PagesSet::LAB],
                                                 s.d[PagesSet::LAB2], s.d[PagesSet::BIN], ps.d_lut, n_lut, level, nout, mask_id, st));
            else
                PSEG_TRY(png_pages_enqueue(q.L, s.d[PagesSet::PNG], fin[i0], g > 1 ? (size_t)(tab[i0 + 1].pred_off - tab[i0].pred_off) : 0, s.d[PagesSet::BIN],
                                           up256((size_t)tab[i0].Hl * tab[i0].Wl), ps.d_lut, n_lut, tab[i0].Hl, tab[i0].Wl, level, nout, mask_id, g, st));
            PSEG_HIP(hipMemcpyAsync(s.h_tot, s.d[PagesSet::PNG], (size_t)g * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        }
        PSEG_HIP(hipEventRecord(s.done, st));
        return PSEG_OK;
    };
    // where a unit's outputs lie in its page-locked slot: per page the requested streams (8-byte aligned), then the label map
    // (and the sizes, copied out of the set's page-locked words: those are written again by the unit after next while this one is
    // still being delivered)
    std::vector<std::vector<size_t>> offs(2), tot(2);
    auto download = [&](int u) -> int {
        PagesSet& s = ps.set[u & 1];
        const Unit& q = un[u];
        const int i0 = ub[u], g = ug[u];
        PSEG_HIP(hipEventSynchronize(s.done));                 // the sizes are here
        std::vector<size_t>& of = offs[u & 1];
        of.assign((size_t)g * 5 + 1, 0);
        std::vector<size_t>& tt = tot[u & 1];
        tt.assign((size_t)g * 4, 0);
        size_t pos = 0;
        for (int k = 0; k < g; ++k) {
            const size_t bound = mixed ? (size_t)tab[i0 + k].bound : q.L.bound;
            for (int j = 0; j < 4; ++j) {
                of[(size_t)k * 5 + j] = pos;
                if (j >= nout) continue;
                const unsigned long long t = s.h_tot[(size_t)k * 4 + j];
                if (t < 80 || t > bound) return fail(PSEG_EHIP, "png: encoded size %llu outside (0, bound %zu] (page %d)", t, bound, ord[i0 + k]);
                tt[(size_t)k * 4 + j] = (size_t)t;
                pos += ((size_t)t + 7) & ~(size_t)7;
            }
            of[(size_t)k * 5 + 4] = pos;
            if (want_lab) pos += ((size_t)tab[i0 + k].Hl * tab[i0 + k].Wl + 7) & ~(size_t)7;
        }
        of[(size_t)g * 5] = pos;
        // the slot was handed to the sink by deliver(u - 2): idle.  It grows to what units really hold, with a quarter of headroom.
        if (s.h_out_bytes < pos) PSEG_TRY(pages_ensure_host(&s.h_out, &s.h_out_bytes, pos + pos / 4 + 4096));
        for (int k = 0; k < g; ++k) {
            const MixedPage& m = tab[i0 + k];
            for (int j = 0; j < nout; ++j) {
                const uint8_t* src = mixed ? s.d[PagesSet::PNG] + m.ws_off + (size_t)j * m.per + m.slots_b + m.meta_b + m.offs_b
                                           : s.d[PagesSet::PNG] + q.L.head + (size_t)(g > 1 ? k : 0) * q.L.page + (size_t)j * q.L.per + q.L.slots_b + q.L.meta_b + q.L.offs_b;
                PSEG_HIP(hipMemcpyAsync(s.h_out + of[(size_t)k * 5 + j], src, tt[(size_t)k * 4 + j], hipMemcpyDeviceToHost, s_out));
            }
            if (want_lab) PSEG_HIP(hipMemcpyAsync(s.h_out + of[(size_t)k * 5 + 4], fin[i0 + k], (size_t)m.Hl * m.Wl, hipMemcpyDeviceToHost, s_out));
        }
        PSEG_HIP(hipEventRecord(s.down, s_out));
        return PSEG_OK;
    };
    auto deliver = [&](int u) -> int {         // chunk CRCs, then the sink: the planner's order, `which` ascending; on the calling thread
        PagesSet& s = ps.set[u & 1];
        const std::vector<size_t>& of = offs[u & 1];
        PSEG_HIP(hipEventSynchronize(s.down));
        for (int k = 0; k < ug[u]; ++k) {
            const int pi = ord[ub[u] + k];
            for (int j = 0; j < nout; ++j) {
                uint8_t* p = s.h_out + of[(size_t)k * 5 + j];
                const size_t t = tot[u & 1][(size_t)k * 4 + j];
                PSEG_TRY(png_finish_host(p, t));
                if (sink(user, pi, mask_id[j], p, t) != 0) return fail(PSEG_ECALLBACK, "the sink stopped the call at page %d, output %d", pi, mask_id[j]);
            }
            if (want_lab && sink(user, pi, 4, s.h_out + of[(size_t)k * 5 + 4], (size_t)tab[ub[u] + k].Hl * tab[ub[u] + k].Wl) != 0)
                return fail(PSEG_ECALLBACK, "the sink stopped the call at page %d, output 4", pi);
        }
        return PSEG_OK;
    };
    // the host enqueues unit u + 1 before it waits for unit u's sizes; while the device works it finishes unit u - 1
    PSEG_TRY(upload(0));
    PSEG_TRY(compute(0));
    for (int u = 0; u < nu; ++u) {
        if (u + 1 < nu) { PSEG_TRY(upload(u + 1)); PSEG_TRY(compute(u + 1)); }
        PSEG_TRY(download(u));
        if (u > 0) PSEG_TRY(deliver(u - 1));
    }
    PSEG_TRY(deliver(nu - 1));
    PSEG_HIP(hipStreamSynchronize(s_out));
    return engine_status(e, st);
}

extern "C" int pseg_predict_chain_pages_png(pseg_engine* h, int n, const uint8_t* const* imgs, const int* H, const int* W, const int* Ho,
                                            const int* Wo, const uint8_t* const* binaries, const int* post_ops, int n_post, unsigned flags,
                                            const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap, pseg_chain_sink sink,
                                            void* user) {
    return chain_pages_run(h, n, imgs, H, W, Ho, Wo, binaries, post_ops, n_post, flags, lut, n_lut, level, want, unit_cap, sink, user, false);
}

extern "C" int pseg_predict_chain_pages_mixed_png(pseg_engine* h, int n, const uint8_t* const* imgs, const int* H, const int* W, const int* Ho,
                                                  const int* Wo, const uint8_t* const* binaries, const int* post_ops, int n_post, unsigned flags,
                                                  const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap, pseg_chain_sink sink,
                                                  void* user) {
    return chain_pages_run(h, n, imgs, H, W, Ho, Wo, binaries, post_ops, n_post, flags, lut, n_lut, level, want, unit_cap, sink, user, true);
}

extern "C" int pseg_predict_chain_scans_png(pseg_engine* h, int n, const pseg_scan* scans, const int* post_ops, int n_post, unsigned flags,
                                            const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap, pseg_chain_sink sink, void* user) {
    if (n < 0 || (n > 0 && !scans)) return fail(PSEG_EINVAL, "bad argument");
    if (!sink) return fail(PSEG_EINVAL, "NULL sink");
    // every scan is checked before any device work starts; the pages' shapes then go through the page entries' checks
    std::vector<const uint8_t*> gray(n);
    std::vector<int> H(n), W(n), Ho(n), Wo(n);
    for (int i = 0; i < n; ++i) {
        PSEG_TRY(scan_front_check(scans[i], i));
        gray[i] = scans[i].gray;
        H[i] = scans[i].H;
        W[i] = scans[i].W;
        Ho[i] = scans[i].final_is_scan ? scans[i].H0 : 0;
        Wo[i] = scans[i].final_is_scan ? scans[i].W0 : 0;
    }
    return chain_pages_run(h, n, gray.data(), H.data(), W.data(), Ho.data(), Wo.data(), gray.data(), post_ops, n_post, flags, lut, n_lut, level, want,
                           unit_cap, sink, user, true, scans);
}
