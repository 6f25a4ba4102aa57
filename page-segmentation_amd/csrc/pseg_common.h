// pseg_common.h -- shared declarations of the libpseg.so sources (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pseg.h"

struct pseg_engine;
namespace pseg {

// ---- error plumbing (thread-local message, int status: SURVEY.md 8b "Errors") -------------
std::string& last_error();
int fail(int code, const char* fmt, ...);

#define PSEG_HIP(expr)                                                                         \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return ::pseg::fail(PSEG_EHIP, "%s failed: %s (%s:%d)", #expr,                     \
                                hipGetErrorString(_e), __FILE__, __LINE__);                    \
    } while (0)

#define PSEG_TRY(expr)                                                                         \
    do {                                                                                       \
        int _rc = (expr);                                                                      \
        if (_rc != PSEG_OK) return _rc;                                                        \
    } while (0)

// ---- host-side plumbing shared by pseg_predict_batch and the page chain ---------------------
// A grow-only buffer of device (HOST = false) or page-locked host memory.  ensure() keeps a block that is large enough, else frees it and
// allocates `bytes` (the caller knows that nothing on the device still uses it); a failure is PSEG_ENOMEM with the buffer's name and size.
template <bool HOST>
struct GrowBuf {
    uint8_t* p = nullptr;
    size_t cap = 0;
    template <class T> T* as() const { return (T*)p; }
    int ensure(size_t bytes, const char* what) {
        if (cap >= bytes && p) return PSEG_OK;
        release();
        if ((HOST ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes)) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return fail(PSEG_ENOMEM, "%s(%s, %zu bytes) failed", HOST ? "hipHostMalloc" : "hipMalloc", what, bytes);
        }
        cap = bytes;
        return PSEG_OK;
    }
    void release() { if (p) (void)(HOST ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
};
typedef GrowBuf<false> GrowDev;
typedef GrowBuf<true> GrowPin;
// true when `p` is page-locked host memory the runtime knows (hipHostMalloc / hipHostRegister): DMA goes straight to it
inline bool host_is_pinned(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}
// Every way out of a call -- also an error return in the middle -- ends with its streams drained: copies from / to the caller's
// host arrays and the page-locked slots must not be in flight when the caller gets its buffers back.
struct StreamDrain {
    hipStream_t s[3];
    ~StreamDrain() { for (hipStream_t x : s) if (x) (void)hipStreamSynchronize(x); }
};

// The two-set pipeline of pseg_predict_batch and the page chain.  Unit u works in set u % 2; the set's events say when its buffers
// are free again:  up = the unit's uploads landed (s_in),  done = its compute landed (st),  down = its downloads landed (s_out).
struct PipeSet {
    hipEvent_t up = nullptr, done = nullptr, down = nullptr;
    int create() {
        for (hipEvent_t* ev : {&up, &done, &down})
            if (!*ev) PSEG_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
        return PSEG_OK;
    }
    void destroy() { for (hipEvent_t* ev : {&up, &done, &down}) { if (*ev) (void)hipEventDestroy(*ev); *ev = nullptr; } }
};
// upload(u) and compute(u) of one unit.  The uploads wait until unit u - 2's compute has read the set's inputs; the compute waits for them
// and until unit u - 2's downloads have left the set's outputs.  before_compute: the stage's host-side hook (the wait in front of a canvas change).
template <class Stage>
int pipe_enqueue(Stage& g, int u, const PipeSet& s, hipStream_t s_in, hipStream_t st) {
    PSEG_HIP(hipStreamWaitEvent(s_in, s.done, 0));          // (a no-op before the first record)
    PSEG_TRY(g.upload(u, s));
    PSEG_HIP(hipEventRecord(s.up, s_in));
    PSEG_TRY(g.before_compute(u));
    PSEG_HIP(hipStreamWaitEvent(st, s.up, 0));
    PSEG_HIP(hipStreamWaitEvent(st, s.down, 0));
    PSEG_TRY(g.compute(u, s));
    PSEG_HIP(hipEventRecord(s.done, st));
    return PSEG_OK;
}
// `nu` units of `g` over set[0..1]: g.reserve() sizes every buffer for the largest unit while the sets are idle (a call ends drained), then
// the host enqueues unit u + 1 before it downloads unit u, and finishes unit u - 1 while the device works.  download(u) keeps its own wait for
// `done` (on the host where it needs the unit's sizes, else on s_out); finish(u), for the units that have one, runs on the calling thread.
template <class Stage>
int run_pipeline(Stage& g, int nu, const PipeSet* set, hipStream_t s_in, hipStream_t st, hipStream_t s_out) {
    StreamDrain drain{{s_in, st, s_out}};
    PSEG_TRY(g.reserve());
    if (nu > 0) PSEG_TRY(pipe_enqueue(g, 0, set[0], s_in, st));
    for (int u = 0; u <= nu; ++u) {
        if (u + 1 < nu) PSEG_TRY(pipe_enqueue(g, u + 1, set[(u + 1) & 1], s_in, st));
        if (u < nu) {
            PSEG_TRY(g.download(u, set[u & 1]));
            PSEG_HIP(hipEventRecord(set[u & 1].down, s_out));
        }
        if (u > 0 && g.has_finish(u - 1)) {
            PSEG_HIP(hipEventSynchronize(set[(u - 1) & 1].down));
            PSEG_TRY(g.finish(u - 1));
        }
    }
    PSEG_HIP(hipStreamSynchronize(s_out));
    return PSEG_OK;
}

// Knobs.  Two kinds, one lookup (PSEG_KNOB):
//   * ENVIRONMENT knobs -- the PSEG_ENV_KNOBS list below, thirteen names, documented in README.md: operational choices a deployment
//     may make (page-unit size, the persistent kernel families off, checks, logging).  Nothing else in the process environment
//     reaches the release library.
//   * PLAN SWITCHES -- alternative kernel / fusion choices that must not change results beyond the documented bars; every one is
//     exercised by a bit-identity or tolerance test.  They exist for those tests and for A/B measurements and enter ONLY through
//     pseg_create_plan's `switches` string ("PSEG_NO_DQ=1;PSEG_NO_PAIRC2=1"); the Python test harness builds that string from
//     os.environ when pseg_amd.engine.PLAN_FROM_ENV is set (tests/conftest.py, tools/), a product caller never does.
// pseg_create* takes ONE snapshot (the listed environment knobs + the plan switches) for the new engine; the engine keeps it for
// its whole life (std::shared_ptr) and every entry point that takes an engine answers queries from the engine's OWN snapshot
// (KnobScope, thread-local) -- plan-time and launch-time reads of one engine always agree, and neither a later change of the
// environment nor the creation of another engine (the float32 companion of the label-exact mode inherits its parent's snapshot)
// can alter a running engine.  Engine-less entries (post-process, resize) read the newest environment snapshot.  Each call site
// caches its answer per snapshot id.  The bf16 conv path relies on that agreement: the switches that select a kernel are read when a
// layer is packed (mfma_pack_op keeps the answers in the plan's flags) and no launch reads them again.  The diagnostic build reads
// the live environment instead; changing a switch between weight upload and launch was never supported there.
// Knobs that produce WRONG results (timing ablations: PSEG_DBG, PSEG_XM_DBG, PSEG_SP_DBG, PSEG_PP_NODMA, PSEG_PP_NOEPI, the
// in-kernel trace stamps) exist only in the diagnostic build (libpseg_diag.so, -DPSEG_DIAG=1, which reads everything from the
// environment): PSEG_DIAG_KNOB is a constant nullptr in the release library (tests/test_abi.py checks that the release .so does
// not even hold the names).
#define PSEG_ENV_KNOBS                                                                                                          \
    "PSEG_BATCH_PAGES", "PSEG_NO_PAGE_BATCH", "PSEG_GENERIC", "PSEG_NO_SP", "PSEG_NO_PP", "PSEG_NO_WS", "PSEG_SP_CHECK",        \
    "PSEG_EXACT_TAU", "PSEG_EXACT_FULL", "PSEG_TRAIN_ONE_STREAM", "PSEG_LOG_GENERIC", "PSEG_LOG_SP", "PSEG_CCL_GLOBAL"
#ifndef PSEG_DIAG
#define PSEG_DIAG 0
#endif
struct KnobSnap;                                  // id + the PSEG_* variables at the time of the snapshot
std::shared_ptr<const KnobSnap> knobs_snapshot(const char* plan = nullptr); // the listed environment knobs now (+ plan switches "A=1;B=2"); without a plan it also becomes the "newest" one
unsigned knob_generation();                       // id of the snapshot in scope (the engine's, else the newest), >= 1
const char* knob_lookup(const char* name);        // value in that snapshot, or nullptr
struct Engine;
struct KnobScope {                                // RAII: knob queries on this thread read `e`'s snapshot
    explicit KnobScope(const Engine& e);
    ~KnobScope();
    const KnobSnap* prev;
};
#if PSEG_DIAG
#define PSEG_KNOB(name) getenv(name)
#define PSEG_DIAG_KNOB(name) getenv(name)
#else
#define PSEG_KNOB(name)                                                                                   \
    ([]() -> const char* {                                                                                \
        static thread_local unsigned gen_ = 0;       /* per thread: no torn (id, value) pairs */         \
        static thread_local const char* v_ = nullptr;                                                     \
        const unsigned g_ = ::pseg::knob_generation();                                                    \
        if (gen_ != g_) {                                                                                 \
            v_ = ::pseg::knob_lookup(name);                                                               \
            gen_ = g_;                                                                                    \
        }                                                                                                 \
        return v_;                                                                                        \
    }())
#define PSEG_DIAG_KNOB(name) ((const char*)nullptr)
#endif

constexpr int PSEG_CHAIN_BLOCK = 16;   // float32 mode: input channels per pass of the accumulation chain (oracle/pseg_oracle.c ORC_CHAIN_BLOCK)
constexpr int PSEG_MAXC = 64;   // classes the train-step metric slots and the wide bf16 logits kernel are sized for
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return cdiv(a, b) * b; }
// TF SAME padding in front of one axis: pad_total = max((out - 1) * stride + k - in, 0), before = total / 2; a stride-1 Conv2DTranspose runs
// as a convolution with the flipped kernel, where "before" and "after" swap (odd k: equal)
static inline int same_pad(int out, int in, int k, int stride, bool transposed) {
    const int total = std::max((out - 1) * stride + k - in, 0);
    return transposed ? total - total / 2 : total / 2;
}
// What a launcher that may decline a layer answers: PSEG_OK (launched), ROUTE_NO (not a layer for this route: ask the next), or an
// error (< 0).  The bf16 routes of mfma_launch_conv and the float32 routes of launch_conv_exact / forward_deconv2 share it.
constexpr int ROUTE_NO = 1;
// Every kernel with dynamic LDS is launched here: the CU's whole 160 KB allowed once per device and kernel instance, the launch, its
// error.  dev < 0: the current device is looked up.  `more`: the kernel's arguments behind its record.
template <auto KERNEL, typename Arg, typename... More>
int launch_lds(const Arg& a, dim3 grid, unsigned threads, size_t lds, int dev, hipStream_t st, More... more) {
    static bool attr_set[64] = {false};
    if (dev < 0) PSEG_HIP(hipGetDevice(&dev));
    if (!attr_set[dev & 63]) {
        PSEG_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set[dev & 63] = true;
    }
    KERNEL<<<grid, threads, lds, st>>>(a, more...);
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}
// crop / tile halo: >= the receptive-field radius of the graph (fcn / fcn_skip: 75 pixels counting the one-sided growth of the
// 2x2 pools; unet ~122, res_unet ~124), a multiple of 32.  Shared by the label-exact mode's crops and the tile plan.
static inline int halo_of(int arch) { return (arch == PSEG_ARCH_FCN_SKIP || arch == PSEG_ARCH_FCN) ? 96 : 160; }

// ---- graph description ---------------------------------------------------------------------
enum OpType { OP_CONV = 0, OP_DECONV2 = 1, OP_POOL = 2, OP_LOGITS = 3, OP_BN = 4 };

struct Tensor {
    std::string name;   // producing Keras layer name ("input", "conv2d", "max_pooling2d", ...)
    int s = 0;          // log2 down-scale relative to the padded canvas
    int C = 0;          // true channel count
    int Cs = 0;         // storage channels: C (f32 mode) or round_up(C, 8) (bf16 mode)
    void* d = nullptr;  // device buffer, NHWC, (Hp>>s) x (Wp>>s) x Cs -- of the page slot in use (Engine::pages slots; slot 0 = base)
    void* base = nullptr;       // slot 0 in the address map in use (install_map): `pages` slots of page_bytes each (bf16 page batches), d == base
                                // outside a per-page run.  Full map: == own; compact map: inside Engine::arena, or its start for a tensor no launch touches
    size_t page_bytes = 0;      // bytes of one page slot at the current canvas
    void* own = nullptr;        // full map: this tensor's own allocation
    size_t bytes = 0;           // ... and its size
    bool fused = false; // bf16 mode: never written to HBM (lives only inside a fused kernel)
    bool relu_stored = false;   // bf16 mode: stored after the pre-activation ReLU of its readers (mfma_plan_graph)
};

struct Param {
    std::string name;   // "conv2d/kernel", ...
    int64_t shape[4] = {0, 0, 0, 0};
    int ndim = 0;
    std::vector<float> host;  // Keras layout
    bool set = false;
};

struct Op {
    int type = OP_CONV;
    std::string layer;   // Keras layer name
    int k = 1, stride = 1;
    bool transposed = false;  // Conv2DTranspose stride 1: flip + swap channels at upload
    int src0 = -1, src1 = -1; // concat [src0, src1]
    int up0 = 0, up1 = 0;     // nearest x2 upsample folded into the gather
    int in_relu = 0, relu = 0;
    int add = -1;             // residual addend tensor (Add()), applied after bias
    int dst = -1;
    int pool_dst = -1;        // bf16 mode: fused 2x2 max-pool output
    int relu_dst = -1;        // bf16 mode: second output tensor holding max(x, 0) for the pre-activation readers (mfma_plan_graph)
    int kparam = -1, bparam = -1;   // OP_BN: gamma / beta of the BatchNormalization layer
    int mmparam = -1, mvparam = -1; // OP_BN: moving_mean / moving_variance
    int bn_c0 = 0;                  // OP_BN: first channel of this op's slice of the layer's vectors (a BN over a
                                    // Concatenate runs as one op per source tensor)
    int Cin = 0, Cout = 0;
    // device weights
    float* d_w = nullptr;     // f32 correlation form [KH][KW][Cin][Cout] (+slack) / [2][2][Cin][Cout]; OP_BN: [gamma|beta|mean|var][C]
    float* d_b = nullptr;     // f32 bias; OP_BN: [batch mean | 1/sqrt(var+eps)][C] of the last training forward, then 4*C doubles of reduction scratch
    float* d_wrem = nullptr;  // f32 mode: the left-over output channels' kernel as shifted copies (conv_xb_kernel REM), owned by the op,
    size_t wrem_bytes = 0;    //   sized at upload_weights, rebuilt by the launcher whenever wrem_valid is false (weights changed)
    bool wrem_valid = false;
    void* plan = nullptr;     // bf16 mode: MfmaPlan (pseg_mfma.hip), owned by the op
    bool fused_away = false;  // bf16 mode: op folded into a neighbour (pool -> conv epilogue, logits -> deconv tail)
    int fuse1 = -1;           // bf16 mode: OP_CONV that recomputes this first-layer op on its halo tile
    int tail_logits = -1;     // bf16 mode: OP_DECONV2 that also runs this OP_LOGITS (fused tail)
    int dq_fuse = -1;         // bf16 mode: OP_CONV (k5, 80 couts) whose epilogue also runs this later OP_DECONV2 (k2 s2) on its accumulators; the deconv is fused_away
    int into_tail = -1;       // bf16 mode: OP_DECONV2 (ReLU) computed inside the composed-tail kernel of this later OP_DECONV2 (fused_away)
    bool pool_only = false;   // bf16 mode: the full-resolution output is read by nothing but the fused pool: it is not stored
    int skiplog = -1;         // bf16 mode: conv whose output only feeds (a fused pool and) this OP_LOGITS as the skip: it stores
                              // its logits contribution (f32, padded classes) instead of the full-resolution tensor
    int nw_hint = 4;          // bf16 mode: waves per workgroup the plan should be packed for (4 or 8)
    float dropout = 0.0f;     // Dropout(rate) on this op's output: identity at inference, applied by the train step
    double flops_per_canvas_px = 0;  // algorithmic, true channels
    int timing_slot = -1;
};

// ---- bf16 MFMA path (pseg_mfma.hip) ----------------------------------------------------------
struct Engine;
// host-side packing + upload; w = correlation-form f32 weights as uploaded for the exact path
int mfma_pack_op(Engine& e, Op& op, const std::vector<float>& w, const std::vector<float>& bias);
void mfma_free_op(Op& op);
int mfma_plan_graph(Engine& e);                              // pool fusion etc., once per engine
int mfma_launch_conv(Engine& e, Op& op, hipStream_t st);     // OP_CONV
int mfma_launch_deconv2(Engine& e, Op& op, hipStream_t st);  // OP_DECONV2
int mfma_launch_pool(Engine& e, Op& op, hipStream_t st);     // OP_POOL (unfused fallback)
int mfma_launch_logits(Engine& e, Op& op, float* d_logits, float* d_probs, int64_t* d_labels,
                       uint8_t* d_labels_u8, hipStream_t st);
int mfma_preprocess(Engine& e, const uint8_t* d_img, hipStream_t st);
bool mfma_input_is_staged(const Engine& e);                 // false: every reader of the input takes the uint8 page itself, the input tensor is never written

struct TimingSlot {
    std::string name;
    double flops = 0;   // algorithmic flops of one launch at the current canvas
    double total_ms = 0;
    int64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// ---- the two address maps of a bf16 engine -------------------------------------------------------------------------
// FULL: one allocation per tensor (Tensor::own) and one for the skip-logits plane -- what pseg_get_activation reads; the only map of a
// float32 engine.  COMPACT: one arena; a tensor's bytes are reused by tensors that are produced after its last reader (plan_arena).
// One row of the compact plan: a tensor some launch writes or reads (tensor = index, -1: the skip-logits plane).
struct ArenaRow {
    std::string name;
    int tensor = -1;
    size_t bytes = 0, offset = 0;        // inside one page slot of the arena
    int producer = 0, last_reader = 0;   // indices into ArenaPlan::launches: the live range, both ends included
    bool shared = false;                 // false: private, once-zeroed bytes behind the shared part (its producer leaves stored bytes unwritten)
};
struct ArenaPlan {
    std::vector<std::string> launches;   // the kernels of one page in launch order ("preprocess" first where the input tensor is staged)
    std::vector<ArenaRow> rows;          // in the order they were placed (producer launch, larger first)
    size_t shared_bytes = 0;             // [0, shared_bytes): the part tensors share (what PSEG_COMPACT_POISON fills)
    size_t total_bytes = 0;              // one slot of the arena
    size_t full_bytes = 0;               // one slot of the full map (every tensor + the skip-logits plane)
    size_t untouched_max = 0;            // the largest tensor no launch touches (it is handed the arena's start)
};
struct Engine;
// Host arithmetic over the graph as mfma_plan_graph left it (no HIP call): pseg_graph.cpp.  bf16 engines only.
int plan_arena(const Engine& e, int Hp, int Wp, ArenaPlan& out);
bool mfma_reads_page(const Engine& e, const Op& op);   // a first layer that takes the uint8 page itself (pseg_mfma.hip: is_conv1_special)
enum { MAP_FULL = 0, MAP_COMPACT = 1 };
struct CanvasMap { int Hp = 0, Wp = 0, pages = 0; };   // the canvas and page slots a map's buffers are laid out for (Hp = 0: none)

struct Engine {
    std::shared_ptr<const KnobSnap> knobs;   // the PSEG_* snapshot this engine was created under (see PSEG_KNOB)
    int arch = 0, n_classes = 0, in_ch = 1, device = 0, mode = 0;
    unsigned flags = 0;            // PSEG_FLAG_* of pseg_create_ex
    bool bn_training = false;      // float32 engine, while a TRAINING forward runs: BatchNormalization layers use batch statistics and update their moving ones
    hipStream_t stream = nullptr;
    std::vector<Tensor> tensors;
    std::vector<Param> params;
    std::vector<Op> ops;
    int input_tensor = 0;
    // canvas
    int H = 0, W = 0, Hp = 0, Wp = 0;
    int pages = 1;                 // page slots every activation tensor has room for (bf16 page batches: pseg_predict_batch)
    // Hp, Wp, pages and every Tensor::base / page_bytes describe the map in use; set_canvas lays a map out and installs it
    CanvasMap maps[2];             // MAP_FULL, MAP_COMPACT
    int map_in_use = MAP_FULL;
    bool host_parity = false;      // while pseg_predict runs: the full map, whatever is asked for (pseg_get_activation is documented against it)
    int act_H = 0, act_W = 0;      // the page of the last run on the full map (0: none so far) -- what pseg_get_activation answers from
    void* arena = nullptr;         // compact map: `pages` slots of arena_plan.total_bytes, slot p at arena + p * total_bytes, a tensor at ArenaRow::offset inside its slot
    size_t arena_bytes = 0;        // bytes allocated
    ArenaPlan arena_plan;          // ... laid out by this plan (maps[MAP_COMPACT]'s canvas)
    void* skip_own = nullptr;      // full map: the skip-logits plane's own allocation (fcn_skip: conv2's logits contribution, f32 [canvas pixel][4 or 8])
    size_t skip_own_bytes = 0;
    void* skip_base = nullptr;     // the plane in the map in use: slot 0, skip_bytes long (0: the graph has none), the next slot's skip_stride further
    size_t skip_bytes = 0, skip_stride = 0;
    int page = 0;                  // page slot the per-page launches of a batch run are working on
    int batch_pages = 0;           // > 1 while a launch covers that many page slots at once (a tile index carries the page)
    bool weights_dirty = true;
    bool exact_dirty = true;       // label-exact mode: the float32 companion's weights / the calibrated threshold are stale
    float* d_lut = nullptr;        // 256-entry u/255 table (f32)
    const uint8_t* cur_img = nullptr;  // bf16 mode: the uint8 page of the running predict call
    float* cur_logits = nullptr;       // bf16 mode: output pointers of the running predict call
    float* cur_probs = nullptr;
    int64_t* cur_labels = nullptr;
    uint8_t* cur_labels_u8 = nullptr;
    float* cur_margin = nullptr;       // bf16 mode: top-1 minus top-2 logit map requested by the running call (label-exact mode)
    bool margin_done = false;          // ... and whether the tail kernel of the graph wrote it (else it is derived from the logits)
    GrowDev logits_tmp;            // H*W*C f32 when the caller does not want logits
    GrowDev img_stage, lab_stage, prob_stage, logit_stage;   // pseg_predict's device copies of the caller's arrays
    int tiling_mode = 0, tiling_tile = 0;   // pseg_engine_set_tiling: PSEG_TILING_*, the tile edge (0: the default)
    GrowDev tile_img, tile_lab;    // tiled prediction (pseg_tiles.hip): the tiles of a unit one behind the other, their uint8 label maps
    void* train = nullptr;   // TrainState (pseg_train.hip), f32 mode only
    void* exact = nullptr;   // ExactState (pseg_exactlabels.hip): float32 companion engine, margin / flag buffers of the label-exact mode
    // BatchState owns the two copy streams (s_in, s_out), its event triples and staging slots; the page chain borrows the streams
    // (batch_copy_streams) and owns everything else it uses: ChainState has the aux stream and event of the single-page chain, its
    // buffers, and the page list's two staging sets with their own event triples.  Compute of both runs on Engine::stream.
    void* batch = nullptr;   // BatchState (pseg_engine.hip), freed by pseg_destroy
    void* chain = nullptr;   // ChainState (pseg_chain.hip), freed by chain_free; chain_trim frees the page list's staging memory
    void* dist = nullptr;    // DistState (pseg_allreduce_init): RCCL communicator of the data-parallel train step
    uint32_t drop_key = 0;   // != 0 while a TRAINING forward runs: Dropout layers are live (key = seed / step mix)
    const float* cur_img_f32 = nullptr;   // float32 exact mode: float page (0..255 scale) instead of the uint8 one (augmented training samples)
    int* d_sp_err = nullptr;   // bf16 mode: the give-up record of conv_sp_kernel's bounded counter waits (8 ints: code, wave, need, have,
    int* h_sp_err = nullptr;   //   need2, have2, workgroup, op index), zero while all is well; h_: its pinned read-back slot (engine_status)
    // timing
    bool timing = false;
    std::vector<TimingSlot> slots;
    std::vector<hipEvent_t> event_pool;

    int tH(const Tensor& t) const { return Hp >> t.s; }
    int tW(const Tensor& t) const { return Wp >> t.s; }
};

// f32-exact conv launcher shared with the training path (pseg_train.hip)
struct ConvArgs {
    const float* src0;
    const float* src1;
    int C0, C1;
    int up0, up1;
    int Hin, Win;  // logical input dims (after the folded upsample)
    const float* w;
    const float* bias;
    const float* add;
    float* dst;
    int KH, KW, stride, pt, pl, Hout, Wout, Cout, in_relu, relu;
    const float* mask;   // training dgrad: input value counts only where mask (same layout as src0) > 0
    int dst_pitch;       // pixels per output row (0: Wout) -- crop / canvas-pitched outputs
    int out_sy, out_sx, out_oy, out_ox;   // MFMA kernel only: output pixel (y*sy + oy, x*sx + ox); 0 strides = 1
    int deconv4;         // MFMA kernel only: Conv2DTranspose k2 s2 as one GEMM, n = ab*Cout + co -> (2y + a, 2x + b)
    int dbg;             // MFMA kernel only: timing experiments (PSEG_XM_DBG: 1 no staging loads, 2 no stores, 4 no k-loop) -- wrong results
    void* unused_[2];    // read by nothing: holds the place of two retired fields, so that every compiled kernel keeps its argument layout
    const float* wrem = nullptr;   // blocked MFMA kernel, set by its launcher: the left-over output channels' kernel, shifted copies [KH][KW + DX - 1][Cin][16] (conv_xb_kernel REM)
    float* wrem_buf = nullptr;     // caller-owned buffer for that kernel (wrem_bytes_for() bytes; null or too small: padded cout tiles instead)
    size_t wrem_cap = 0;
    bool* wrem_valid = nullptr;    // null: rebuild on every launch (scratch weights); else rebuilt when *wrem_valid is false, then set
};
// bytes of ConvArgs.wrem_buf a KH x KW, Cin -> Cout stride-1 layer needs for its left-over channel tile, 0 when it has none
size_t wrem_bytes_for(int KH, int KW, int Cin, int Cout);
// Asks its routes in order -- first-layer vector ALU, matrix core, 1x1, scalar -- and always launches: PSEG_OK or an error.
int launch_conv_exact(const ConvArgs& a, hipStream_t st);
// HBM-bound float32 layers on the vector ALU (pseg_exact_valu.hip): first layer; Conv2DTranspose k2 s2, optionally with the
// logits layer + argmax behind it.  PSEG_OK / ROUTE_NO / error.
struct TailArgs {
    const float* src0; const float* src1; int C0, C1, Hin, Win;
    const float* w; const float* bias; int Cout, relu;
    float* dst;
    const float* skip; int Cs;
    const float* wl; const float* bl; int ncls;
    int H, W;
    float* logits; int64_t* labels; uint8_t* labels_u8;
};
int launch_conv_first_valu(const ConvArgs& a, hipStream_t st);
int launch_deconv2_valu(const TailArgs& a, bool tail, hipStream_t st);
int launch_conv_exact_mfma(const ConvArgs& a, hipStream_t st);   // matrix cores (pseg_exact_mfma.hip): PSEG_OK / ROUTE_NO / error
// split form of UpSampling2D(2) -> Conv2D(k2) (pseg_upsplit.hip)
struct UpSplit;
int upsplit_create(UpSplit** out, const std::vector<float>& w, const std::vector<float>& bias, int Cin, int Cs0, int Cout, int CoS);
void upsplit_free(UpSplit* u);
int upsplit_launch(UpSplit* u, const uint16_t* src, int Hs, int Ws, uint16_t* dst, int relu, hipStream_t st);
// BatchNormalization (pseg_bn.hip), NHWC float32 tensors of npx pixels x C channels; `par` = [gamma|beta|moving_mean|moving_var][C]
constexpr float PSEG_BN_EPS = 1e-3f;        // tf.keras.layers.BatchNormalization defaults (lib/model.py:268,315 pass none)
constexpr float PSEG_BN_MOMENTUM = 0.99f;
int bn_infer(const float* x, float* y, size_t npx, int C, const float* par, float* saved, int relu, hipStream_t st);
int bn_train_forward(const float* x, float* y, size_t npx, int C, float* par, float* saved, int relu, int up, hipStream_t st);
int bn_backward(const float* x, const float* y_mask, const float* dy, float* dx_accum, size_t npx, int C, const float* par,
                float* saved, float* dgamma, float* dbeta, hipStream_t st);
int bn_infer_bf16(const uint16_t* x, uint16_t* y, size_t npx, int Cs, const float* scale_shift, int relu, hipStream_t st);
size_t bn_saved_bytes(int C);
// Dropout mask of element i under `key`: keep iff hash(i, key) >= rate (inverted dropout, kept values * 1/(1-rate))
void launch_dropout(float* x, size_t n, uint32_t key, float rate, hipStream_t st);
int ccl_roots(const uint8_t* d_bin, int* d_L, int H, int W, int connectivity, hipStream_t st);   // pseg_post.hip
// cv2 getThreshVal_Otsu_8u restated (OpenCV 4.5.5 modules/imgproc/src/thresh.cpp, published algorithm): first maximum of
// q1*q2*(mu1-mu2)^2, double precision.  One body for the host (pseg_otsu_char_height) and the device (otsu_kernel of
// pseg_lineheight.hip): every source is built with -ffp-contract=off, so both give the same bits.
__host__ __device__ inline int otsu_from_hist(const unsigned* h, int64_t n) {
    const double scale = 1.0 / (double)n;
    double mu = 0;
    for (int i = 0; i < 256; ++i) mu += i * (double)h[i];
    mu *= scale;
    double mu1 = 0, q1 = 0, max_sigma = 0;
    int max_val = 0;
    const double eps = 1.1920928955078125e-07;  // FLT_EPSILON
    for (int i = 0; i < 256; ++i) {
        const double p_i = h[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1.0 - q1;
        const double lo = q2 < q1 ? q2 : q1, hi = q1 < q2 ? q2 : q1;   // std::min / std::max
        if (lo < eps || hi > 1.0 - eps) continue;
        mu1 = (mu1 + i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
    }
    return max_val;
}
// The glyph filter of compute_char_height (lib/image_ops.py:70-76), the one place its six constants live: a component counts when
// GLYPH_H_LO < h < GLYPH_H_HI, GLYPH_W_LO < w < GLYPH_W_HI and GLYPH_AR_LO < w / h < GLYPH_AR_HI (h, w: extents of its bounding box).
constexpr int GLYPH_H_LO = 10, GLYPH_H_HI = 60, GLYPH_W_LO = 5, GLYPH_W_HI = 50;
constexpr double GLYPH_AR_LO = 0.5, GLYPH_AR_HI = 2;
__host__ __device__ inline bool glyph_shaped(int h, int w) {
    if (!(GLYPH_H_LO < h && h < GLYPH_H_HI && GLYPH_W_LO < w && w < GLYPH_W_HI)) return false;
    const double ar = (double)w / (double)h;
    return GLYPH_AR_LO < ar && ar < GLYPH_AR_HI;
}
// pseg_png.hip, for the page chain: the masks of `pages` label maps of one shape as PNG streams in one set of launches, enqueued on
// `st` without a wait; the workspace (PngPages::bytes, from png_pages_layout) is the caller's.  Page p's sizes: ((u64*)d_ws)[4 p + k];
// its stream k (k-th requested mask): d_ws + head + p * page + k * per + slots_b + meta_b + offs_b, chunk CRCs left to
// png_finish_host on the downloaded bytes.
struct PngPages { size_t bytes, head, page, per, slots_b, meta_b, offs_b, bound; };
int png_pages_layout(int H, int W, int level, int nout, int pages, PngPages* L);
int png_pages_enqueue(const PngPages& L, uint8_t* d_ws, const uint8_t* d_pred, size_t page_pred, const uint8_t* d_bin, size_t page_bin,
                      const uint8_t* d_lut, int n_lut, int H, int W, int level, int nout, const int mask_id[4], int pages, hipStream_t st);
int png_finish_host(uint8_t* png, size_t total);
// One page of a mixed unit (pseg_predict_chain_pages_mixed_png): pages of one canvas, each with its own shape.  The chain fills the
// first block, png_pages_layout_mixed the encoder's.  All offsets are bytes from the start of the staging block they name.
struct MixedPage {
    int H, W;                                 // the network's page; dense in IMG at img_off, its dense H x W label map in LAB at lab_off
    int Hl, Wl;                               // the final label map: in LAB (pred_sel 0) or LAB2 (pred_sel 1) at pred_off, binarisation at bin_off
    int pred_sel, L, R, nb;                   // encoder: filtered bytes per row, rows per band, bands
    int band0, pad;                           // bands of the unit's pages in front of this one (the prefix table of the ragged launches)
    unsigned long long img_off, lab_off, pred_off, bin_off;
    unsigned long long slot, ws_off, per, slots_b, meta_b, offs_b, bound;   // the page's part of the encoder workspace (as PngPages, per page)
};
constexpr int PNG_MIXED_MAX = 64;             // pages of one ragged launch
// The masks of `pages` label maps of DIFFERENT shapes as PNG streams in one set of launches over the flattened (page, band) pairs.
// png_pages_layout_mixed reads Hl, Wl of tab[0..pages) and fills the encoder's fields; png_pages_enqueue_mixed validates the table
// (h_tab, the host's copy of d_tab) against the workspace and launches.  Page p's sizes: ((u64*)d_ws)[4 p + k]; its stream k:
// d_ws + ws_off + k * per + slots_b + meta_b + offs_b.  A page's stream is the single-image encoder's, byte for byte.
struct PngPagesMixed { size_t bytes, head; int bands; };
int png_pages_layout_mixed(int level, int nout, int pages, MixedPage* tab, PngPagesMixed* L);
int png_pages_enqueue_mixed(const PngPagesMixed& L, const MixedPage* h_tab, const MixedPage* d_tab, int pages, uint8_t* d_ws, size_t ws_bytes,
                            const uint8_t* d_pred0, const uint8_t* d_pred1, const uint8_t* d_bin, const uint8_t* d_lut, int n_lut, int level,
                            int nout, const int mask_id[4], hipStream_t st);
// pseg_resize.hip, for the scan chain (pseg_predict_chain_scans_png): the device-resident front end of one scan.
// scan_front_check validates shapes and radii; scan_front_weights writes the scan's weights (axis 0, then axis 1; 2 r + 1 doubles
// each, none for an axis without a pass) to `dst` (NULL: count only) and returns their number; scan_front_work is the bytes of
// filtered-plane workspace the scan needs (0: no pass on either axis).  scan_front_enqueue launches on `st` without a wait: d_rec
// (SCAN_REC_WORDS zeroed words) is the scan's record, d_w its weights on the device, d_img / d_bin the (H,W) outputs, d_orig the
// scan-sized ink map; d_bin and d_orig may be NULL.  d_scan, d_work and d_orig are 16-byte aligned.
constexpr int SCAN_REC_WORDS = 16;
// how: the scan's binarisation (NULL or window 0: ink = scan <= 127).  With an adaptive one the workspace grows by the row-sum plane
// and -- unless final_is_scan, where d_orig is the destination -- the scan-sized ink plane, both behind the filtered planes; the
// binarisation kernels write the ink map and the sampler gathers from it.  d_scan is readable up to the next multiple of 16 bytes.
// dsp: the scan's despeckling (NULL or max_area 0: none).  With one the scan-sized ink plane is always materialised (a fixed
// threshold's by the statistics pass), the workspace grows by that plane (unless final_is_scan) and, behind it, by
// despeckle_work_bytes(H0, W0); the despeckle launches run on the plane in front of the sampler, which gathers from it.
int scan_front_check(const pseg_scan& s, int index);
size_t scan_front_weights(const pseg_scan& s, double* dst);
size_t scan_front_work(const pseg_scan& s, const pseg_binarize* how = nullptr, const pseg_despeckle* dsp = nullptr);
int scan_front_enqueue(const pseg_scan& s, const uint8_t* d_scan, const double* d_w, uint8_t* d_work, unsigned* d_rec, uint8_t* d_img,
                       uint8_t* d_bin, uint8_t* d_orig, hipStream_t st, const pseg_binarize* how = nullptr, const pseg_despeckle* dsp = nullptr);
// pseg_binarize.hip: binarize_check refuses a bad pseg_binarize ("scan <index>: ..."); binarize_rows_bytes is the row-sum plane of an
// H x W scan (a multiple of 256); binarize_enqueue launches the two kernels of one scan on `st` without a wait: d_scan 16-byte
// aligned and readable up to the next multiple of 16 bytes, d_rows 16-byte aligned, d_ink H x W, d_thr float64 H x W or NULL.
int binarize_check(const pseg_binarize& b, int index);
size_t binarize_rows_bytes(int H, int W);
int binarize_enqueue(const uint8_t* d_scan, int H, int W, const pseg_binarize& how, uint8_t* d_rows, uint8_t* d_ink, double* d_thr, hipStream_t st);
// pseg_despeckle.hip: despeckle_check refuses a bad pseg_despeckle ("map <index>: ..."); despeckle_tile_bytes is the workspace of one
// 32 x 64 tile (root slots, rim table, task list, run list, list lengths).  For the scan chain's front end:
// despeckle_work_bytes is the workspace of one H x W map (a multiple of 256: 256 bytes, then the per-tile arrays); despeckle_enqueue
// launches the four kernels of one map on `st` without a wait, in place on d_ink (H x W, non-zero = ink; kept ink becomes 1); d_work
// is 256-byte aligned.  max_area == 0: no launch.
int despeckle_check(const pseg_despeckle& d, int index, const char* what = "map");
size_t despeckle_tile_bytes();
size_t despeckle_work_bytes(int H, int W);
int despeckle_enqueue(uint8_t* d_ink, int H, int W, const pseg_despeckle& how, uint8_t* d_work, hipStream_t st);
// the entry of a list that asks for a despeckling, or NULL
inline const pseg_despeckle* despeckle_of(const pseg_despeckle* how, int i) { return how && how[i].max_area != 0 ? &how[i] : nullptr; }
// the entry of a list that asks for an adaptive binarisation, or NULL
inline const pseg_binarize* binarize_of(const pseg_binarize* how, int i) { return how && how[i].window != 0 ? &how[i] : nullptr; }
// pseg_engine.hip, shared by pseg_predict_batch and the page chain
void plan_units(int n, const int* H, const int* W, const int* Ho, const int* Wo, int cap, std::vector<int>& ub, std::vector<int>& ug);
int fit_unit_slots(Engine& e, int H, int W, int want);              // page slots a unit of `want` pages of this shape gets (1: no page units)
int batch_copy_streams(Engine& e, hipStream_t* s_in, hipStream_t* s_out);   // pseg_predict_batch's upload / download streams
void chain_trim(Engine& e);                                          // pseg_chain.hip: frees the page chain's staging sets (pseg_engine_trim)
int batch_unit_cap(Engine& e, int n, const int* H, const int* W);   // pseg_predict_batch's pages per unit for this list (uploads the weights)
int predict_device_pages(Engine& e, const uint8_t* d_imgs, int n, int H, int W, int64_t* d_labels, uint8_t* d_labels_u8, hipStream_t st);
bool pages_capable(Engine& e);
int upload_weights(Engine& e);
// one page through the engine's graph, device buffers, asynchronous on `st` (every output optional)
int predict_device(Engine& e, const uint8_t* d_img, int H, int W, float* d_logits, float* d_probs, int64_t* d_labels,
                   uint8_t* d_labels_u8, hipStream_t st, float* d_margin);
void launch_margin_from_logits(const float* d_logits, size_t n, int C, float* d_margin, hipStream_t st);
bool mfma_tail_emits_margin(const Engine& e);   // the bf16 graph's tail kernel writes the margin map itself
int create_engine(int arch, int n_classes, int in_channels, int device, int mode, unsigned flags,
                  std::shared_ptr<const KnobSnap> inherit, struct ::pseg_engine** out, const char* plan = nullptr);   // pseg_create_ex; `inherit` = a parent engine's knob snapshot
void exact_free(Engine& e);
void chain_free(Engine& e);
void dist_free(Engine& e);                      // RCCL communicator (pseg_dist.hip)                     // Predictor chain buffers (pseg_chain.hip)                     // label-exact mode state (pseg_exactlabels.hip)
int set_canvas(Engine& e, int H, int W, hipStream_t st, int pages = 1, bool labels_only = false);   // labels_only: the call returns label maps (and margins) alone -- the compact map, unless PSEG_NO_COMPACT or pseg_predict
// What set_canvas refuses and what a page slot costs, host arithmetic over the graph's tensors (shared with fit_page_slots and the
// AUTO tiling mode).  canvas_refused: a bf16 engine whose largest tensor at this canvas would reach 4 GiB; canvas_slot_bytes: the
// activation tensors of one page slot; page_slot_fits: one whole-page slot leaves a fifth of the device's free memory untouched
// (what the engine already holds counts as free).
bool canvas_refused(const Engine& e, int Hp, int Wp);
size_t canvas_slot_bytes(const Engine& e, int Hp, int Wp);
size_t skip_plane_bytes(const Engine& e, int Hp, int Wp);          // one slot of the skip-logits plane, 0 where the graph has none
bool compact_wanted(const Engine& e);                               // a bf16 engine without PSEG_NO_COMPACT
bool page_slot_fits(Engine& e, int H, int W);
// pseg_tiles.hip: one page's label map(s) from same-shape tiles through the page-slot path, asynchronous on `st`; and the network
// stage of the label-only entries: tiled where the engine's tiling mode asks for it, else predict_device
int predict_tiled_device(Engine& e, const uint8_t* d_img, int H, int W, int tile, int64_t* d_labels, uint8_t* d_labels_u8, hipStream_t st);
int predict_labels_routed(Engine& e, const uint8_t* d_img, int H, int W, int64_t* d_labels, uint8_t* d_labels_u8, hipStream_t st);
// Waits for `st`, then reports -- and clears -- the engine's device-side error record: PSEG_EHIP when a counter wait of
// conv_sp_kernel gave up since the last report (the label maps produced since then are not to be trusted).  Called by every
// entry that synchronises with the host anyway and by pseg_engine_status (for the callers of the asynchronous _device entries).
int engine_status(Engine& e, hipStream_t st);
bool mfma_op_batchable(const Engine& e, const Op& op);      // the op's kernel takes several page slots in one launch
int run_exact(Engine& e, const uint8_t* d_img, float* d_logits, float* d_probs, int64_t* d_labels,
              uint8_t* d_labels_u8, hipStream_t st);
// training state (pseg_train.hip)
int train_sync_weights_to_host(Engine& e);
void train_free(Engine& e);
// one augmented training sample built on the device (pseg_resize.hip; arguments as pseg_train_forward_backward_aug).  d_src_*: the
// uploaded uint8 page (H,W,C) and mask; d_coef: augment_coef_count() doubles (unused when m == NULL); d_mm: 2 unsigned;
// d_img: float32 (H,W,C) out, d_mask: uint8 (H,W) out.  All work is enqueued on the stream; nothing is allocated.
struct AugSample {
    const uint8_t* d_src_img;
    const uint8_t* d_src_mask;
    int H, W, C;
    const double* m;        // host, 4 doubles; NULL: no warp
    const double* off;      // host, 2 doubles
    unsigned flips;
    int image_fill, mask_fill;
    float image_cval, mask_cval;
    int use_brightness;
    float brightness;
    double* d_coef;
    unsigned* d_mm;
    float* d_img;
    uint8_t* d_mask;
};
int augment_check(int H, int W, const double* m, const double* off, unsigned flips, int image_fill, int mask_fill, float mask_cval);
size_t augment_coef_count(int H, int W, int image_fill);
int augment_sample_device(const AugSample& a, hipStream_t st);

int time_begin(Engine& e, Op& op, hipStream_t st, hipEvent_t* ev0);
int time_end(Engine& e, Op& op, hipStream_t st, hipEvent_t ev0);

}  // namespace pseg

// the opaque handle of include/pseg.h
struct pseg_engine {
    pseg::Engine e;
};
