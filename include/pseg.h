/*
 * pseg.h -- C ABI of libpseg.so, the MI355X (gfx950) engine for the per-pixel
 * page-segmentation hot path of ocr4all_pixel_classifier.
 *
 * The reference (pure Python over TensorFlow/OpenCV) has no FFI layer; the boundary this
 * library sits behind is the Python API of ocr4all_pixel_classifier.lib.
 * Each entry point names the reference interface it replaces.  Signatures carry plain
 * pointers and sizes only -- no torch / numpy types.  Every function returns 0 on success
 * and a negative PSEG_E* code on failure; pseg_last_error() returns a thread-local message
 * (the Python shim raises it as Exception, the reference's error style).
 *
 * Ownership: the library never retains a caller pointer past the call.  Device buffers are
 * owned by the opaque pseg_engine.  "_device" variants take pointers that are already
 * resident in HBM on the engine's device and enqueue on the given hipStream_t (passed as
 * void*; NULL = the engine's own stream) without synchronising.
 */
#ifndef PSEG_H
#define PSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSEG_ABI_VERSION 1

/* lib/architecture.py:6-11 -- the in-scope Architecture members. */
enum { PSEG_ARCH_FCN_SKIP = 0, PSEG_ARCH_FCN = 1, PSEG_ARCH_UNET = 2, PSEG_ARCH_RES_UNET = 3 };

/* Arithmetic mode.  F32_EXACT: float32 tensors, one sequential fmaf chain per output -- slabs of 16 input
 * channels, (ky,kx,ci) inside a slab -- bit-identical to oracle/pseg_oracle.c.  BF16: bf16 activations + bf16 kernels,
 * float32 MFMA accumulation (throughput mode, BASELINE.json configs[1]). */
enum { PSEG_MODE_F32_EXACT = 0, PSEG_MODE_BF16 = 1 };

enum {
    PSEG_OK = 0,
    PSEG_EINVAL = -1,   /* bad argument / shape */
    PSEG_ENOTFOUND = -2, /* unknown weight name */
    PSEG_EHIP = -3,     /* HIP runtime error (message has the hipError string) */
    PSEG_ENOMEM = -4,
    PSEG_EUNSUPPORTED = -5,
    PSEG_ECALLBACK = -6 /* a caller's callback asked to stop (pseg_predict_chain_pages_png's sink) */
};

typedef struct pseg_engine pseg_engine;

int pseg_abi_version(void);
const char* pseg_last_error(void);

/* Number of visible HIP devices (0 when none; never fails). */
int pseg_device_count(void);

/* ---- Network: lib/network.py:18-107 (graph construction + weight loading) ------------- */

/* Replaces model_constructor.model()([input, binary], n_classes) (lib/network.py:89) for
 * lib/model.py:45 (fcn_skip), :206 (fcn), :151 (unet), :237 (res_unet). */
int pseg_create(int arch, int n_classes, int in_channels, int device, int mode,
                pseg_engine** out);
/* ... with graph options.  PSEG_FLAG_BATCHNORM: tf.keras.layers.BatchNormalization (defaults: epsilon 1e-3, momentum
 * 0.99) at the sites the reference's constructors provide for it -- res_unet's bn_act (lib/model.py:265-271: in front
 * of every pre-activation ReLU and behind every shortcut convolution; the reference hard-wires its switch to False)
 * -- the same placement as conv_block_simple's Conv2D -> BatchNormalization -> ReLU (lib/model.py:310-317) behind the
 * shortcut convolutions.  Adds "batch_normalization[_N]/gamma|beta|moving_mean|moving_variance" to the weight table
 * (Keras order).  Prediction and pseg_eval_step use the moving statistics; pseg_train_forward_backward normalises with
 * the page's batch statistics, updates the moving ones and back-propagates through the layer.  Only
 * PSEG_ARCH_RES_UNET has such sites (PSEG_EUNSUPPORTED otherwise).  flags = 0 is pseg_create. */
enum { PSEG_FLAG_BATCHNORM = 1 };
int pseg_create_ex(int arch, int n_classes, int in_channels, int device, int mode, unsigned flags,
                   pseg_engine** out);
/* ... with PLAN SWITCHES: alternative kernel / fusion choices of the bf16 and float32 engines ("PSEG_NO_DQ=1;PSEG_NO_PAIRC2=1";
 * NULL or "" = pseg_create_ex).  Test and measurement entry: every switch leaves the results within the documented bars (most
 * are bit-identical) and is pinned by a test; the process environment cannot set them -- the release library reads only the
 * names pseg_env_knobs() lists from the environment (README.md documents them), once per engine at creation. */
int pseg_create_plan(int arch, int n_classes, int in_channels, int device, int mode, unsigned flags, const char* switches,
                     pseg_engine** out);
/* the environment variables the release library reads, one per line (static storage) */
const char* pseg_env_knobs(void);
int pseg_destroy(pseg_engine* e);

/* Weight table in Keras creation order; names are Keras' default layer names plus
 * "/kernel" or "/bias" ("conv2d/kernel", "conv2d_transpose_1/bias", "logits/kernel", ...).
 * Layouts are Keras': Conv2D (kh,kw,Cin,Cout), Conv2DTranspose (kh,kw,Cout,Cin), bias (Cout). */
int pseg_num_weights(const pseg_engine* e);
int pseg_weight_info(const pseg_engine* e, int index, char* name, size_t name_cap,
                     int64_t shape[4], int* ndim);
/* Replaces model.load_weights (lib/network.py:106-107) / model.set_weights. */
int pseg_set_weights(pseg_engine* e, const char* name, const float* data, const int64_t* shape,
                     int ndim);
int pseg_get_weights(const pseg_engine* e, const char* name, float* out, int64_t count);

/* ---- Predict: lib/network.py:248-260 (Network.predict_single_data) -------------------- */

/* img: uint8 (H,W) network input (inverted, line-height normalised page).  Computes
 * x/255 -> pad to 32 -> FCN -> crop -> logits -> softmax / argmax.  Any of logits (H,W,C f32),
 * probs (H,W,C f32), labels (H,W int64) may be NULL.  Host pointers; synchronous. */
int pseg_predict(pseg_engine* e, const uint8_t* img, int H, int W, float* logits, float* probs,
                 int64_t* labels);

/* Same with device-resident buffers; asynchronous on `stream`.  labels_u8 is an optional
 * compact label map (n_classes <= 256). */
int pseg_predict_device(pseg_engine* e, const uint8_t* d_img, int H, int W, float* d_logits,
                        float* d_probs, int64_t* d_labels, uint8_t* d_labels_u8, void* stream);

/* Predictor.predict's page loop (lib/predictor.py:27-30) for n_pages pages of ONE shape that are resident on the device:
 * d_imgs = the pages one behind the other (n_pages * H * W * in_channels bytes), d_labels / d_labels_u8 = the label maps
 * one behind the other (either may be NULL).  bf16 engines keep a page slot per page in every activation tensor and give
 * the low-resolution layers (from 1/4 resolution down: fcn / fcn_skip's conv5 ... deconv3, the plain convolutions of unet /
 * res_unet) all slots in one launch (a page alone leaves them a partly filled chip); float32 engines run the pages one after
 * the other.  Each map equals pseg_predict_device's for that page.  Asynchronous
 * on `stream`.  The slots per unit (16, PSEG_BATCH_PAGES) are cut to what the device's free memory holds, and halved
 * again when an allocation fails all the same (PSEG_ENOMEM only when a single slot does not fit). */
int pseg_predict_pages_device(pseg_engine* e, const uint8_t* d_imgs, int n_pages, int H, int W, int64_t* d_labels,
                              uint8_t* d_labels_u8, void* stream);

/* ---- Tiled prediction: the label map of a page of any size ------------------------------------------------------- */

/* The reference pads a page to a multiple of 32, runs the graph on the whole of it and crops (lib/model.py:10-42); it has no tiles.
 * A bf16 engine refuses a page once a tensor of its graph would reach 4 GiB (fcn_skip: a canvas of 8192 x 8192, unet: about
 * 5790 x 5790), and any engine fails with PSEG_ENOMEM where one page's activation tensors do not fit the device.  These entries cut
 * such a page into same-shape tiles whose stitched label map EQUALS the whole page's wherever the whole page can run -- no
 * tolerance: a tile carries `halo` pixels of context (96 for fcn / fcn_skip, 160 for unet / res_unet: at least the receptive-field
 * radius) on every side that is not the canvas edge, starts on the page's 32-pixel grid and never extends past the page's own
 * canvas (a page zero-extended past its canvas is another page to lib/model.py:20-26's padding).
 *
 * pseg_tile_plan -- host arithmetic, no device.  Per axis, with Np = the extent rounded up to 32 and T = `tile` (a multiple of 32,
 * at least 2 halo + 32; 0: the default, 2048): tile extent t = min(T, Np); stride s = t - 2 halo; origins y_k = min(k s, Np - t)
 * for k = 0, 1, ... up to the first y_k == Np - t; tile k owns [end of tile k - 1's range, y_k + t - halo), the first range starts
 * at 0, the last ends at Np.  A tile is a row range x a column range (row-major: column index fastest); all tiles of a page have
 * the shape (*tile_h, *tile_w); tile content = the page's pixels in [y, y + tile_h) x [x, x + tile_w), zeros outside the H x W page.
 * Returns the number of tiles (>= 1) and fills origin_y / origin_x [n] and owned [n][4] = {y0, y1, x0, x1} (canvas coordinates,
 * half-open; every output may be NULL; PSEG_EINVAL when there are more than max_tiles tiles and an array to fill), or a negative
 * PSEG_E* (PSEG_EINVAL: bad arch / shape / tile).  Checked before it returns: every canvas pixel has exactly one owner, an owned
 * pixel lies at least halo from every tile edge that is not a canvas edge, origins are multiples of 32, tiles lie inside the canvas. */
int pseg_tile_plan(int arch, int H, int W, int tile, int* tile_h, int* tile_w, int* origin_y, int* origin_x, int* owned, int max_tiles);

/* Network.predict_single_data's `pred` (lib/network.py:259) of a device-resident page through that plan: one launch cuts up to 16
 * tiles out of the page, they run as one unit of page slots (pseg_predict_pages_device's path; the count is cut to what the
 * device's free memory holds; float32 engines and PSEG_NO_PAGE_BATCH run tile by tile), one launch writes every tile's owned
 * rectangle into d_labels (int64) and / or d_labels_u8 (dense H x W; either may be NULL, not both).  A page of one tile runs as
 * pseg_predict_device.  Asynchronous on `stream`; the tile staging (two grow-only buffers of the engine, freed by pseg_engine_trim)
 * is grown behind a wait for `stream`.  <= 256 classes.  pseg_predict_tiled: the host-array form, synchronous. */
int pseg_predict_tiled_device(pseg_engine* e, const uint8_t* d_img, int H, int W, int tile, int64_t* d_labels, uint8_t* d_labels_u8,
                              void* stream);
int pseg_predict_tiled(pseg_engine* e, const uint8_t* img, int H, int W, int tile, int64_t* labels, uint8_t* labels_u8);

/* Where tiles are used without the caller asking.  The mode is read by the network stage of pseg_predict, pseg_predict_device and
 * pseg_predict_chain[_png[_lv]] when label maps alone are requested (logits and probs NULL) and PSEG_CHAIN_EXACT_LABELS is not set;
 * every other request keeps the whole-page path and its refusals, as do the page-list entries (_batch, _chain_pages*, _chain_scans*).
 *   PSEG_TILING_OFF     the default: the whole page, always.
 *   PSEG_TILING_AUTO    tiles for the pages the whole-page path cannot take: the bf16 4 GiB guard refuses the canvas, or one
 *                       page slot of it does not fit the device's free memory (pseg_engine_page_fits says which pages those are).
 *   PSEG_TILING_ALWAYS  tiles for every page.
 * The maps are identical, so the route a page took does not show in the output.  `tile`: pseg_tile_plan's. */
enum { PSEG_TILING_OFF = 0, PSEG_TILING_AUTO = 1, PSEG_TILING_ALWAYS = 2 };
int pseg_engine_set_tiling(pseg_engine* e, int mode, int tile);
/* 1: the whole-page path takes an H x W page on this engine now; 0: it would refuse it (4 GiB guard) or its slot does not fit the
 * free device memory -- the pages PSEG_TILING_AUTO tiles; negative: PSEG_E*. */
int pseg_engine_page_fits(pseg_engine* e, int H, int W);

/* Device-side error record of the engine -- the asynchronous `_device` entries cannot report what a kernel finds while it
 * runs.  Waits for `stream` (NULL: the engine's own), then reports AND clears: PSEG_OK, or PSEG_EHIP when one of the bounded
 * counter waits of the streamed-weights kernel (conv_sp_kernel: the 1/8-resolution layers of every page) gave up since the last
 * report -- the label maps produced since then are not valid (lib/network.py:256-259 has no such state: predict_on_batch either
 * returns the map or raises).  Every host-synchronous entry (pseg_predict, _batch, _chain, _exact_labels) runs the same check
 * before it returns; callers of pseg_predict_device / pseg_predict_pages_device call this where they synchronise. */
int pseg_engine_status(pseg_engine* e, void* stream);

/* Frees the activation memory (both address maps, all page slots) and the tile staging of the engine; the next predict call allocates what
 * its page needs.  An engine grows to the largest canvas x page-slot count it has seen and keeps that; this is the way back
 * (tf.keras.backend.clear_session in lib/trainer.py:112 is the reference's).  Waits for the device.
 *
 * A bf16 engine has two address maps.  The entries that return label maps alone (with or without the margin map: pseg_predict_device
 * without logits and probs, _pages_device, _batch, the chain, tiled and label-exact entries) run on the COMPACT map: one arena per page
 * slot in which a tensor takes the bytes of tensors whose last reader has run (pseg_plan_arena; fcn_skip at 2048x1536: 0.21 GB per slot,
 * 16 slots 3.4 GB).  pseg_predict, and any call that asks for logits or probabilities, runs on the FULL map: one buffer per tensor
 * (0.9 GB per slot), which is what pseg_get_activation reads.  The label maps are the same bits on either.  Plan switch
 * PSEG_NO_COMPACT=1: the full map for everything. */
int pseg_engine_trim(pseg_engine* e);

/* The compact map's plan for an H x W page of a bf16 engine created with these plan `switches` (NULL: none) -- host arithmetic over
 * the graph, no device.  One row per tensor that some kernel launch of a page writes or reads (a layer fused into a neighbour counts
 * in the launch that runs it; "skip_logits" is fcn_skip's plane of conv2's logits contribution); tensors no launch touches have no row
 * and no bytes.  A tensor's live range is [producer, last_reader], indices into the page's launch order (the names say which kernels);
 * two rows whose live ranges intersect never overlap in bytes, and a tensor never takes bytes that a launch reads in the same launch
 * that writes it.  Offsets are multiples of 256 inside one page slot; page slot p of a unit starts p * *arena_bytes further.
 * shared = 0: the tensor's producer leaves stored bytes unwritten (the pad channels behind a stand-alone Conv2DTranspose k2 s2), so it
 * keeps private bytes, zeroed when the canvas is laid out.  *full_bytes: one slot of the full map.  Returns the number of rows and
 * fills rows[0 .. n) (NULL: count only; PSEG_EINVAL when max_rows is too small), or a negative PSEG_E*. */
typedef struct pseg_arena_row {
    char name[48], producer_name[32], last_reader_name[32];
    int64_t bytes, offset;
    int producer, last_reader, shared, reserved;
} pseg_arena_row;
int pseg_plan_arena(int arch, int n_classes, int in_channels, const char* switches, int H, int W, pseg_arena_row* rows, int max_rows,
                    int64_t* arena_bytes, int64_t* full_bytes);

/* Predictor.predict (lib/predictor.py:27-30): label maps of a list of pages of individual sizes.
 * The upload of page i+1 and the download of page i-1 overlap the compute of page i (two staging
 * slots, separate copy streams); runs of consecutive pages of one shape travel and compute as a unit (up to 8 pages,
 * pseg_predict_pages_device).  labels[i] (int64, H[i]*W[i]) and/or labels_u8[i]; either array may
 * be NULL, not both.  Host pointers; returns when every page is back. */
int pseg_predict_batch(pseg_engine* e, int n_pages, const uint8_t* const* imgs, const int* H,
                       const int* W, int64_t* const* labels, uint8_t* const* labels_u8);
/* How pseg_predict_batch cuts a page list into units (host logic, no device needed): runs of consecutive same-shape pages, at
 * most `cap` per unit, unit sizes 1, 2, 4 ... at the head of the list and ... 4, 2, 1 at its tail (the first upload and the last
 * download have no compute beside them).  Returns the number of units (>= 0) and fills unit_first / unit_count (each may be NULL),
 * or a negative PSEG_E*.  lib/predictor.py:27-30 has no such notion: the reference loops page by page. */
int pseg_batch_units(int n_pages, const int* H, const int* W, int cap, int* unit_first, int* unit_count, int max_units);

/* ---- Predictor chain: lib/predictor.py:32-54 ---------------------------------------------------------------- */

/* Predictor.predict_single / predict_masks as ONE device-resident call: Network.predict_single_data's argmax labels ->
 * [scale_to_original_shape (lib/output.py:63-79): order-0 resize of the label map to (Ho, Wo); Ho = 0: none] -> the
 * post-processors of PredictSettings.post_process in order (PSEG_POST_CC_VOTE = vote_connected_component_class,
 * PSEG_POST_BBOX = add_bounding_boxes; lib/postprocess.py:9-42) -> [generate_output_masks (lib/output.py:44-60)].
 * The uint8 label map stays in HBM between the stages; page and binarisation go up once, only the requested outputs
 * come down (DMA straight into page-locked caller memory).  img: uint8 (H,W[,in_channels]); binary: the ink map the vote
 * and the masks read, shape = the label map's final shape ((Ho,Wo) if resized, else (H,W)), may be NULL when neither is
 * asked for; flags: PSEG_CHAIN_EXACT_LABELS runs a bf16 engine's network stage in the label-exact mode.  Outputs (host,
 * each optional): labels int64 / labels_u8 (final shape), color / overlay / inverted / fg_color (final shape x 3).
 * Synchronous; <= 256 classes. */
enum { PSEG_POST_CC_VOTE = 1, PSEG_POST_BBOX = 2 };
enum { PSEG_CHAIN_EXACT_LABELS = 1 };
int pseg_predict_chain(pseg_engine* e, const uint8_t* img, int H, int W, int Ho, int Wo, const uint8_t* binary,
                       const int* post_ops, int n_post, unsigned flags, int64_t* labels, uint8_t* labels_u8,
                       const uint8_t* lut, int n_lut, uint8_t* color, uint8_t* overlay, uint8_t* inverted,
                       uint8_t* fg_color);

/* Label-exact throughput mode (lib/network.py:259: argmax of the float32 logits).  A bf16 engine's label map differs
 * from the float32 engine's only at near-ties of the two largest logits.  pseg_predict_margin_device runs the graph
 * and also writes the margin map (float32 (H,W): top-1 minus top-2 logit; labels_u8 optional).
 * pseg_predict_exact_labels_device aims at the float32 engine's label map at a fraction of its cost: bf16 pass +
 * margin, then the 32x32 blocks that hold a pixel with margin < tau are grouped into rectangles by a cost model and
 * re-evaluated, with their receptive-field halo, by a float32 companion engine (the bit-exact referee, same weights);
 * when the crops would cost more than one float32 pass over the page, the page goes through the float32 engine whole.
 * CALIBRATED, NOT PROVEN: tau starts at 4 x the bf16 path's measured logit error on three calibration crops and is
 * kept >= 2 x the largest change of a margin seen on ANY refereed pixel since the last weight change (every crop is
 * also a measurement; sentinel blocks are refereed on every page; an unflagged pixel that flips doubles tau) -- an
 * unflagged pixel outside every refereed rectangle is trusted on that evidence.  PSEG_MODE_F32_EXACT is the only mode
 * that is bit-exact by construction.  Synchronises `stream` internally (the flag map is read by the host).
 * d_labels (int64) and d_margin are optional outputs.  pseg_label_exact_stats: {tau, calibration logit error,
 * flagged pixel fraction, refereed block fraction, refereed area (with halos) / page area, tau escalations,
 * whole-page fallback (0/1), labels changed by the referee} of the last call; pseg_label_exact_stats_ex appends
 * {running margin error, rectangles refereed, cost-model price of the crops / price of the whole page, block edge,
 * 1 when the page went to the float32 engine directly -- after three whole-page referees in a row the next eight pages
 * skip the bf16 pass --} (`cap` doubles are written). */
int pseg_predict_margin_device(pseg_engine* e, const uint8_t* d_img, int H, int W, uint8_t* d_labels_u8,
                               float* d_margin, void* stream);
int pseg_predict_exact_labels_device(pseg_engine* e, const uint8_t* d_img, int H, int W, uint8_t* d_labels_u8,
                                     int64_t* d_labels, float* d_margin, void* stream);
/* Host-buffer form (Network.predict_single_data's `pred`, lib/network.py:259): either output may be NULL, not both. */
int pseg_predict_exact_labels(pseg_engine* e, const uint8_t* img, int H, int W, int64_t* labels, uint8_t* labels_u8);
int pseg_label_exact_stats(const pseg_engine* e, double out[8]);
int pseg_label_exact_stats_ex(const pseg_engine* e, double* out, int cap);

/* Page-locked host memory for the host-buffer entries ("uint8 page in pinned host memory -> label
 * map in host memory").  Pages and label maps that live in buffers from pseg_host_alloc, or in caller memory
 * registered with pseg_host_register, move by DMA straight between the caller's buffer and HBM, overlapped with
 * compute; any other (pageable) buffer is staged through the engine's two-slot pinned ring by the calling thread.
 * The reference keeps pages in NumPy arrays (lib/dataset.py:18-29); the Python shim offers pinned_empty(). */
int pseg_host_alloc(void** p, size_t bytes);
int pseg_host_free(void* p);
int pseg_host_register(void* p, size_t bytes);
int pseg_host_unregister(void* p);

/* Copy an intermediate activation to the host as float32 NHWC (true channel count) --
 * layer-by-layer parity tests.  `layer` is the Keras layer name.  dims[3] = {H,W,C} of the
 * padded canvas at that layer.  Answers from the last run on the full address map (pseg_engine_trim's note): the last pseg_predict,
 * or the last call that asked for logits or probabilities.  PSEG_EINVAL while there has been none -- the labels-only entries do
 * not materialise activations, whatever ran through them leaves this call's answer as it was.  PSEG_EUNSUPPORTED for a tensor the bf16 plan
 * never writes as such: one that lives inside a fused kernel, one stored after its readers' ReLU, and
 * "input" where the first layer reads the uint8 page itself (one-channel fcn graphs). */
int pseg_get_activation(pseg_engine* e, const char* layer, float* out, int64_t cap, int dims[3]);

/* The engine's own hipStream_t (what NULL stream arguments mean; the train step always runs on it): lets a caller
 * order its own work -- e.g. the data-parallel gradient all-reduce -- against the engine's kernels without
 * synchronising the device. */
void* pseg_engine_stream(pseg_engine* e);

/* Algorithmic forward FLOPs per canvas pixel (2 per MAC, true channel counts): the figure
 * SURVEY.md 8(d) quotes (113 700 for fcn_skip C=3). */
double pseg_flops_per_pixel(const pseg_engine* e);

/* Average duration in ms of the `slot`-th kernel class over the launches since the last
 * reset, measured with HIP events on the launch stream (bench.py roofline).  Timing is off
 * unless enabled; enabling inserts events around every launch. */
int pseg_timing_enable(pseg_engine* e, int on);
int pseg_timing_reset(pseg_engine* e);
int pseg_timing_num_slots(const pseg_engine* e);
int pseg_timing_get(pseg_engine* e, int slot, char* name, size_t name_cap, double* total_ms,
                    int64_t* launches, double* flops);

/* ---- Train: lib/network.py:90-104,167-246 (compile + fit), lib/metrics.py:8-17,60-85 ------- */

/* Training state of a PSEG_MODE_F32_EXACT engine (all four graphs, up to 64 classes): Keras-formulation Adam
 * (lib/architecture.py:83; beta1 .9, beta2 .999, eps 1e-7 are Keras' defaults) with per-tensor
 * clip-by-norm (`clipnorm`, lib/network.py:97; <= 0 disables) and optional clip-by-value. */
int pseg_train_init(pseg_engine* e, float beta1, float beta2, float eps, float clipnorm,
                    float clipvalue);

/* Optimizers (lib/architecture.py:71-90), each with Keras' TF 2.5 default hyper-parameters -- the
 * reference passes only lr / clipnorm / clipvalue (lib/network.py:92-102).  Default after
 * pseg_train_init: Adam.  Switching resets the optimizer state and the step count. */
enum { PSEG_OPT_ADAM = 0, PSEG_OPT_ADAMAX = 1, PSEG_OPT_ADADELTA = 2, PSEG_OPT_ADAGRAD = 3,
       PSEG_OPT_RMSPROP = 4, PSEG_OPT_SGD = 5, PSEG_OPT_NADAM = 6 };
int pseg_train_set_optimizer(pseg_engine* e, int optimizer);

/* Dropout (unet: lib/model.py:167,172, rate 0.5) is live in pseg_train_forward_backward* and the identity in
 * pseg_eval_step / pseg_predict*.  The mask of training forward number n (counted from this call) is a counter-based
 * function of (seed, n, layer, element): reproducible, different every step.  Default seed 0x1234. */
int pseg_train_set_dropout_seed(pseg_engine* e, uint32_t seed);

/* Loss functions (lib/metrics.py:8-9,72-133; `Loss` enum).  metrics[0] of the step calls is the selected
 * loss; the three other metrics stay accuracy / jacard_coef / dice_coef.  Default: cross-entropy. */
enum { PSEG_LOSS_CE = 0, PSEG_LOSS_JACCARD = 1, PSEG_LOSS_DICE = 2, PSEG_LOSS_HINGE = 3, PSEG_LOSS_FOCAL = 4,
       PSEG_LOSS_DICE_CE = 5 };
int pseg_train_set_loss(pseg_engine* e, int loss);

/* One sample (batch of one page, as the reference: lib/network.py:151-153): forward, mean sparse
 * softmax cross-entropy + metrics, backward.  img uint8 (H,W), mask uint8 class ids (H,W), host
 * pointers.  metrics = {loss, accuracy, jacard_coef, dice_coef} of this sample.  Gradients stay
 * in the engine's flat gradient buffer until pseg_train_apply. */
int pseg_train_forward_backward(pseg_engine* e, const uint8_t* img, const uint8_t* mask, int H,
                                int W, float metrics[4]);

/* Same with a float32 page on the 0..255 scale (an augmented sample, lib/network.py:149-161: the cubic warp
 * leaves non-integer values); the network input is img / 255.0f. */
int pseg_train_forward_backward_f32(pseg_engine* e, const float* img, const uint8_t* mask, int H, int W,
                                    float metrics[4]);

/* lib/network.py:149-161 as ONE device-resident call: image (uint8 (H,W[,in_channels])) -> float32 ->
 * per channel cubic warp (order 3, image fill mode / cval) -> flips -> brightness; mask (uint8 (H,W)) ->
 * order-0 warp (mask fill mode / cval) -> flips -> uint8; then the step of pseg_train_forward_backward_f32.
 * m (4 doubles) / off (2): output pixel (r,c) samples the input at m (r,c) + off; m == NULL: no warp (the
 * generator skips it for the identity).  flips: bit 0 horizontal, bit 1 vertical.  fill modes 0..3 as
 * pseg_affine_warp_fill.  mask_cval must be an integer in 0..255 (else PSEG_EINVAL).  use_brightness != 0:
 * pseg_brightness_shift(brightness) over all channels of the warped, flipped sample.
 * Both uint8 arrays are uploaded once on the engine's stream and the sample is built in buffers of the train state
 * (grown on the first page of a size -- PSEG_ENOMEM when that fails --, none allocated in steady state); all work runs
 * on the engine's stream and the only host wait is the metrics read.  The sample has the bits of the host-array path
 * (pseg_affine_warp_fill per channel, NumPy flips, pseg_brightness_shift): the float64 operation sequences are shared. */
int pseg_train_forward_backward_aug(pseg_engine* e, const uint8_t* img, const uint8_t* mask, int H, int W,
                                    const double* m, const double* off, unsigned flips,
                                    int image_fill_mode, float image_cval, int mask_fill_mode, float mask_cval,
                                    int use_brightness, float brightness, float metrics[4]);
/* The sample that call trains on, copied to the host (tests, create-your-own-loop users): out_img float32
 * (H,W[,in_channels]) on the 0..255 scale, out_mask uint8 (H,W).  Needs pseg_train_init, no canvas.  Host-synchronous:
 * waits for the engine's stream before it returns (both outputs are then complete). */
int pseg_train_augment_sample(pseg_engine* e, const uint8_t* img, const uint8_t* mask, int H, int W,
                              const double* m, const double* off, unsigned flips,
                              int image_fill_mode, float image_cval, int mask_fill_mode, float mask_cval,
                              int use_brightness, float brightness, float* out_img, uint8_t* out_mask);

/* The flat device gradient buffer (all parameters in weight-table order, then the metric
 * accumulators): data-parallel training all-reduces exactly this buffer (one RCCL call), then
 * applies with grad_scale = 1/world. */
int pseg_train_grad_buffer(pseg_engine* e, float** d_grad, int64_t* count);
int pseg_train_metrics(pseg_engine* e, float metrics[4]);

/* Data-parallel training (the build's only collective; the reference trains in one process,
 * lib/network.py:235-241): one process per GPU, every rank runs pseg_train_forward_backward on its own page, then ONE
 * all-reduce(sum) of the flat gradient buffer over RCCL / xGMI, then pseg_train_apply(lr, 1/world) on every rank (clip
 * after averaging, identical updates).  RCCL is bound at run time (dlopen): libpseg.so does not link it.
 *   pseg_allreduce_unique_id: rank 0 creates the 128-byte communicator id; the caller hands it to the other ranks.
 *   pseg_allreduce_init:      ncclCommInitRank on the engine's device (collective: every rank calls it).
 *   pseg_train_allreduce:     the all-reduce, in place, enqueued on the engine's stream (no synchronisation).
 *   pseg_allreduce_destroy:   releases the communicator (pseg_destroy does it too). */
int pseg_allreduce_unique_id(uint8_t id[128]);
int pseg_allreduce_init(pseg_engine* e, int rank, int world, const uint8_t id[128]);
int pseg_train_allreduce(pseg_engine* e);
int pseg_allreduce_destroy(pseg_engine* e);
/* 1 when the build pinned the dlopen'ed RCCL entry points (ncclUniqueId size, ncclFloat32 / ncclSum values, the five prototypes)
 * against <rccl/rccl.h> with static_asserts, 0 when that header was absent at build time. */
int pseg_rccl_abi_pinned(void);

/* Clip + Adam update of every parameter with the (scaled) gradients; t += 1. */
int pseg_train_apply(pseg_engine* e, float lr, float grad_scale);

/* Gradient of one parameter in Keras layout (tests). */
int pseg_train_get_gradient(pseg_engine* e, const char* name, float* out, int64_t count);

/* ONE layer's weight (+ bias) gradient on the caller's device tensors (tests): the launch the train step makes for such a
 * layer -- same argument helpers, same kernel choice, same ordered reductions -- on the engine's stream, under its plan
 * switches, with the train state's partial-sum scratch.  Needs pseg_train_init; host-synchronous.  NHWC float32 tensors.
 *   mode 0: conv / logits.  dW[ky][kx][ci0 + ci][co] = sum over (y, x) of Xz[y*stride + ky - pt][x*stride + kx - pl][ci] * dY'[y][x][co],
 *           Xz zero outside the Hx x Wx map, read through a nearest x2 upsample when `xup` (X then holds (Hx/2) x (Wx/2)
 *           pixels), rectified when `in_relu`; dY' = dY where maskY > 0 (maskY NULL: dY); pt / pl: TF SAME for (Hy, Wy).
 *           Hy = ceil(Hx / stride), Wy likewise; stride 1 or 2.  `logits`: KW = 1, no padding, the Hy x Wy page in the
 *           top-left corner of an Hx x Wx canvas (Hy <= Hx, Wy <= Wx), no mask.
 *   mode 1: Conv2DTranspose k2 s2.  dW[a][b][ci][co] = sum over (i, j) of X[i][j][ci] * dY'[2i + a][2j + b][co]; Hy = 2 Hx, Wy = 2 Wx.
 *   dB[co] = sum of dY' (NULL: none; a transposed conv takes one only where a two-source instance runs).
 * X holds XC0 channels per pixel, rows `xpitch` pixels apart; X1 (NULL: none) XC1 channels of the same extent: the second
 * concat source, taken in the same launch (logits and transposed convs that have a two-source instance, ci0 = 0,
 * Cin = XC0 + XC1).  Other layers run one source per call: channels ci0 .. ci0 + XC0 of a dW with Cin input channels.
 * dY / maskY rows are Wy pixels of Cout channels.  slots > 0 replaces "compute units x workgroups per unit" in the strip
 * planners of the flattened-row, channel-block and two-source kernels (0: ask the device); strip_rows > 0 replaces the train
 * step's rows-per-strip proposal for the kernels that take it from the caller (0: the train step's formula).
 * ran (may be NULL) reports the launch. */
enum { PSEG_WGRAD_PAIR = 0, PSEG_WGRAD_FLAT = 1, PSEG_WGRAD_BLK = 2, PSEG_WGRAD_C1 = 3, PSEG_WGRAD_KX5 = 4, PSEG_WGRAD_TAP = 5,
       PSEG_WGRAD_WIDE = 6 };
typedef struct pseg_wgrad_layer {
    const float* X;
    const float* X1;
    const float* dY;
    const float* maskY;
    float* dW;
    float* dB;
    int32_t mode, KW, stride, xup, in_relu, logits;
    int32_t XC0, XC1, ci0, Cin, Cout;
    int32_t Hx, Wx, xpitch, Hy, Wy;
    int32_t slots, strip_rows;
} pseg_wgrad_layer;
typedef struct pseg_wgrad_plan {
    int32_t variant;         /* PSEG_WGRAD_* */
    int32_t instance;        /* PAIR / FLAT / BLK: row of the kernel's instance table; else -1 */
    int32_t ti, tj;          /* C1 / KX5 / TAP / WIDE: the template instance (tiles of 16 rows x 16 columns); else 0 */
    int32_t lds_staged;      /* KX5: 1 = the LDS-staged form, 0 = the direct one */
    int32_t strip_rows;      /* rows of the walk per strip */
    int32_t cgroups;         /* column groups a row strip is cut into (1 where the kernel has none) */
    int32_t nstrips;         /* workgroup strips = rows of the partial-sum scratch */
    int32_t piece_width;     /* PAIR / FLAT / BLK: pixels per column piece; else 0 */
    int32_t deterministic;   /* 1 = partial sums + ordered reduction, 0 = float atomics into dW / dB (which the caller zeroed) */
} pseg_wgrad_plan;
int pseg_train_wgrad_layer(pseg_engine* e, const pseg_wgrad_layer* layer, pseg_wgrad_plan* ran);

/* model.evaluate step (lib/network.py:244-246): forward + loss/metrics only. */
int pseg_eval_step(pseg_engine* e, const uint8_t* img, const uint8_t* mask, int H, int W,
                   float metrics[4]);

/* ---- Post-process: lib/postprocess.py, lib/output.py ---------------------------------- */

/* vote_connected_component_class (lib/postprocess.py:9-26): 4-connected components of
 * `binary` (non-zero = ink); each takes its most frequent class in pred (ties -> lowest).
 * pred int64 (H,W) is updated in place, as the reference does. Host pointers. */
int pseg_cc_vote(int device, int64_t* pred, const uint8_t* binary, int H, int W, int n_classes);
/* Device variant: asynchronous on `stream`.  The label / histogram workspace is cached per device; calls from
 * different streams or threads are ordered against each other by an event (pseg_release_workspace frees it). */
int pseg_cc_vote_device(int device, int64_t* d_pred, const uint8_t* d_binary, int H, int W,
                        int n_classes, void* stream);

/* The same vote on the compact uint8 label map pseg_predict_device emits (n_classes <= 256): 4 instead of 25
 * algorithmic bytes per pixel; widen to int64 only at the host boundary. */
int pseg_cc_vote_device_u8(int device, uint8_t* d_pred, const uint8_t* d_binary, int H, int W,
                           int n_classes, void* stream);
/* Frees every workspace the library caches for this device: the vote's (after waiting for its last user), the PNG encoder's, the
 * bounding-box scratch of pseg_bbox_fill_device_u8 and those of the list entries below, with their streams and events. */
int pseg_release_workspace(int device);

/* add_bounding_boxes (lib/postprocess.py:29-42): every 4-connected component of each class
 * paints its bounding box; higher classes overwrite lower. out may alias nothing. */
int pseg_bbox_fill(int device, const int64_t* pred, int64_t* out, int H, int W, int n_classes);

/* add_bounding_boxes on the compact uint8 label map, device buffers (d_out must not alias d_pred); synchronises `stream`. */
int pseg_bbox_fill_device_u8(int device, const uint8_t* d_pred, uint8_t* d_out, int H, int W, int n_classes, void* stream);

/* generate_output_masks (lib/output.py:44-60).  lut: n_lut x 3 uint8 label->RGB
 * (ColorMap.to_rgb_array).  Outputs (H,W,3) uint8; any may be NULL. */
int pseg_masks(int device, const int64_t* pred, const uint8_t* binary, const uint8_t* lut,
               int n_lut, int H, int W, uint8_t* color, uint8_t* overlay, uint8_t* inverted,
               uint8_t* fg_color);
int pseg_masks_device(int device, const int64_t* d_pred, const uint8_t* d_binary,
                      const uint8_t* d_lut, int n_lut, int H, int W, uint8_t* d_color,
                      uint8_t* d_overlay, uint8_t* d_inverted, uint8_t* d_fg_color, void* stream);

/* generate_output_masks on the compact uint8 label map (14 instead of 21 algorithmic bytes per pixel); d_pred and
 * d_binary must be 4-byte aligned. */
int pseg_masks_device_u8(int device, const uint8_t* d_pred, const uint8_t* d_binary,
                         const uint8_t* d_lut, int n_lut, int H, int W, uint8_t* d_color,
                         uint8_t* d_overlay, uint8_t* d_inverted, uint8_t* d_fg_color, void* stream);

/* ---- PNG output: lib/output.py:20-41 (Image.fromarray(mask).save(...)) --------------------------------------------- */

/* PNG encoder whose pixels are in device memory.  The stream is signature | IHDR | IDAT(zlib header) | one IDAT per band of
 * `band_rows` rows | IDAT(final empty stored block, Adler-32) | IEND; 8-bit truecolour (channels = 3) or 8-bit gray (1),
 * non-interlaced, every scanline filtered with Up.  A band is one fixed-Huffman deflate block closed by an empty stored block
 * (zlib's sync flush), encoded by one workgroup independently of all others; matches are runs against the pixel to the left.
 * band_rows = 0: the default, max(1, 16384 / (channels * W + 1)) rows; any value is cut to H and to 2^30 filtered bytes per band.
 *
 * pseg_png_bound: upper bound of the encoded size, pure arithmetic (no device).  With L = channels * W + 1 bytes per filtered
 * scanline and bands of n = rows * L bytes each,
 *     bound = 80 + sum over the bands of (12 + n + n / 8 + 8)
 * (80 = signature 8 + IHDR 25 + first IDAT 14 + last IDAT 21 + IEND 12; 12 = chunk framing; a band costs at most 3 + 9 n + 7 + 3
 * bits -- block header, 9 bits per byte, end of block, stored-block header -- padded to a byte, plus 4).  0 for a bad shape. */
size_t pseg_png_bound(int H, int W, int channels, int band_rows);
/* d_src: (H,W[,3]) uint8 in device memory; out: host memory (page-locked for best speed) of cap >= pseg_png_bound(...) bytes
 * (else PSEG_EINVAL); *n_bytes = the stream's size.  Runs on `stream` and waits for it (synchronous); never writes past cap. */
int pseg_png_encode_device(int device, const uint8_t* d_src, int H, int W, int channels, int band_rows, uint8_t* out, size_t cap,
                           size_t* n_bytes, void* stream);
/* generate_output_masks (lib/output.py:44-60) + PNG in one pass: the band kernel computes the masks' pixels from the uint8 label
 * map, the binarisation and the colour table (pseg_masks_device_u8's selection), the RGB masks never exist in memory.
 * Order: color / overlay / inverted / fg_color; out[k] == NULL: mask k is not wanted (n_bytes[k] = 0). */
int pseg_masks_png_device_u8(int device, const uint8_t* d_pred, const uint8_t* d_binary, const uint8_t* d_lut, int n_lut, int H, int W,
                             int band_rows, uint8_t* const out[4], const size_t cap[4], size_t n_bytes[4], void* stream);
/* Host-array counterparts: upload, encode, download (pseg_masks' pattern).  pseg_masks_png takes the reference's int64 label map;
 * labels outside the colour table are black, as in pseg_masks (PSEG_EINVAL if the table has all 256 entries and such a label occurs). */
int pseg_png_encode(int device, const uint8_t* src, int H, int W, int channels, int band_rows, uint8_t* out, size_t cap, size_t* n_bytes);
int pseg_masks_png(int device, const int64_t* pred, const uint8_t* binary, const uint8_t* lut, int n_lut, int H, int W, int band_rows,
                   uint8_t* const out[4], const size_t cap[4], size_t n_bytes[4]);
/* pseg_predict_chain with the masks as PNG streams: same stages, same label outputs; png[k] (host, cap[k] >= pseg_png_bound(Hl, Wl,
 * 3, 0) bytes, NULL: not wanted) in the order color / overlay / inverted / fg_color, n_bytes[k] their sizes. */
int pseg_predict_chain_png(pseg_engine* e, const uint8_t* img, int H, int W, int Ho, int Wo, const uint8_t* binary,
                           const int* post_ops, int n_post, unsigned flags, int64_t* labels, uint8_t* labels_u8,
                           const uint8_t* lut, int n_lut, uint8_t* const png[4], const size_t cap[4], size_t n_bytes[4]);

/* The same entries with a compression `level`; the entries above are level 0.  Any other level than 0 or 1: PSEG_EINVAL (the
 * bound: 0).
 *   0  one fixed-Huffman block per band, as described above.
 *   1  a band's workgroup walks its tokens twice: it counts the literal/length symbols, builds a Huffman code of at most 15
 *      bits for them (two one-bit distance codes beside it: every match of a band has the same distance), prices the band as a
 *      dynamic block -- header included -- and as a fixed one, and writes the smaller (a tie: fixed, the band is then level 0's
 *      band of the same rows bit for bit).  The tokens are level 0's.  No band grows, so the bound's formula holds; only the
 *      default band differs: band_rows = 0 is max(1, 65536 / (channels * W + 1)) rows, over which the header amortises. */
size_t pseg_png_bound_lv(int H, int W, int channels, int band_rows, int level);
int pseg_png_encode_device_lv(int device, const uint8_t* d_src, int H, int W, int channels, int band_rows, int level, uint8_t* out,
                              size_t cap, size_t* n_bytes, void* stream);
int pseg_masks_png_device_u8_lv(int device, const uint8_t* d_pred, const uint8_t* d_binary, const uint8_t* d_lut, int n_lut, int H, int W,
                                int band_rows, int level, uint8_t* const out[4], const size_t cap[4], size_t n_bytes[4], void* stream);
int pseg_png_encode_lv(int device, const uint8_t* src, int H, int W, int channels, int band_rows, int level, uint8_t* out, size_t cap,
                       size_t* n_bytes);
int pseg_masks_png_lv(int device, const int64_t* pred, const uint8_t* binary, const uint8_t* lut, int n_lut, int H, int W, int band_rows,
                      int level, uint8_t* const out[4], const size_t cap[4], size_t n_bytes[4]);
int pseg_predict_chain_png_lv(pseg_engine* e, const uint8_t* img, int H, int W, int Ho, int Wo, const uint8_t* binary,
                              const int* post_ops, int n_post, unsigned flags, int64_t* labels, uint8_t* labels_u8,
                              const uint8_t* lut, int n_lut, int level, uint8_t* const png[4], const size_t cap[4], size_t n_bytes[4]);
/* Predictor.predict's page loop (lib/predictor.py:27-30) over the whole chain, to PNG: a list of pages in, their mask PNG streams
 * (and, with bit 4 of `want`, the final uint8 label maps) out through `sink`.  Stages, post-processors, `flags`, `lut` and `level`
 * are pseg_predict_chain_png_lv's, and every stream and label map has that call's bytes for the page alone.  Ho / Wo: NULL, or per page
 * the final shape (0: no rescale); binaries[i]: the page's ink map in its final shape (the array, or an entry, may be NULL where
 * neither the vote nor a mask needs it).  All pages are checked before any device work starts (PSEG_EINVAL names the page).
 *
 * The list is cut into units by pseg_chain_units (at most `unit_cap` pages; 0: pseg_predict_batch's choice for the list).  A unit's
 * pages go up together; a bf16 engine without PSEG_CHAIN_EXACT_LABELS runs their network stage over page slots
 * (pseg_predict_pages_device's path), any other engine page after page; resize, vote and boxes follow per page on the engine's
 * stream; then ONE set of encoder launches writes all requested masks of all pages of the unit.  Two staging sets and
 * pseg_predict_batch's two copy streams: unit u + 1 is enqueued before the host waits for unit u's sizes, the downloads carry
 * exactly the encoded bytes, and the host fills the chunk CRCs of unit u - 1 and hands it to `sink` while the device works.
 *
 * sink(user, page, which, data, n_bytes): called on the calling thread only (no thread is created), in page order and `which`
 * ascending (0 color, 1 overlay, 2 inverted, 3 fg_color: PNG streams; 4: the uint8 label map); `data` is valid during the call
 * only.  A non-zero return stops the call: PSEG_ECALLBACK.  Every return -- also an error in the middle -- leaves the streams
 * drained and the engine usable.  The call ends with pseg_engine_status's check: on PSEG_EHIP the pages delivered by it are not to
 * be trusted.  n_pages == 0: PSEG_OK, no sink call.
 *
 * The staging sets (device: pages, label maps, binarisations, the encoder's workspace for a unit; page-locked host: uploads of
 * pageable arrays and the encoded streams, grown to the largest unit's actual bytes, not to pseg_png_bound x pages) belong to the
 * engine.  pseg_engine_trim frees their memory (device and page-locked); their events, the colour table and pseg_predict_chain's
 * own single-page buffers stay until pseg_destroy. */
typedef int (*pseg_chain_sink)(void* user, int page, int which, const uint8_t* data, size_t n_bytes);
int pseg_predict_chain_pages_png(pseg_engine* e, int n_pages, const uint8_t* const* imgs, const int* H, const int* W,
                                 const int* Ho, const int* Wo, const uint8_t* const* binaries,
                                 const int* post_ops, int n_post, unsigned flags,
                                 const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap,
                                 pseg_chain_sink sink, void* user);
/* How that call cuts its list (host logic only): pseg_batch_units' rule with (H, W, Ho, Wo) as a page's shape; Ho / Wo NULL: exactly
 * pseg_batch_units. */
int pseg_chain_units(int n_pages, const int* H, const int* W, const int* Ho, const int* Wo, int cap,
                     int* unit_first, int* unit_count, int max_units);
/* pseg_predict_chain_pages_png for lists whose pages differ in shape (every scan scaled by its own line height): same arguments,
 * same bytes per (page, output), other units.  A page's label map equals the top-left H x W of the label map of the page
 * zero-padded to its canvas (H, W rounded up to multiples of 32), so the list is cut by CANVAS: pseg_chain_units_mixed brings the
 * pages of one canvas together and cuts them with pseg_chain_units' rule; the final shapes play no part.  A unit's pages go up
 * densely.  A bf16 engine without PSEG_CHAIN_EXACT_LABELS pads the pages of a unit of two or more into canvas-sized page slots
 * (one launch), runs the network stage over the slots and crops every label map back to its page (one launch); any other engine
 * runs the unit's pages one after the other at their own shapes, on the one canvas.  Resize, vote and boxes follow per page, and
 * ONE set of encoder launches over the flattened (page, band) pairs writes the masks of all pages of the unit, whatever their final
 * shapes.  The device changes canvas once per distinct canvas of the list, not once per page.
 * The sink is called unit by unit in the planner's order, the pages of a unit in the permuted order, `which` ascending; `page` is
 * the page's index in the caller's list, and every (page, output) arrives exactly once.  Everything else -- checks, staging sets,
 * the drained return, PSEG_ECALLBACK, the final status check -- is pseg_predict_chain_pages_png's. */
int pseg_predict_chain_pages_mixed_png(pseg_engine* e, int n_pages, const uint8_t* const* imgs, const int* H, const int* W,
                                       const int* Ho, const int* Wo, const uint8_t* const* binaries,
                                       const int* post_ops, int n_post, unsigned flags,
                                       const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap,
                                       pseg_chain_sink sink, void* user);
/* How that call cuts its list (host logic only).  order[n_pages] (may be NULL): a permutation of the pages -- stable, canvases by
 * first appearance, list order within a canvas.  The units are pseg_chain_units' cut of the permuted list with the canvas as the
 * page's shape; unit_first indexes permuted positions.  Returns the number of units; errors as pseg_chain_units. */
int pseg_chain_units_mixed(int n_pages, const int* H, const int* W, int cap, int* order,
                           int* unit_first, int* unit_count, int max_units);

/* The code lengths level 1 uses, on the host (pure arithmetic, no device; the device runs the same function): counts[n] ->
 * lengths[n], 0 exactly for a count of 0, none above `limit`, a complete prefix code when two or more symbols occur (one symbol:
 * length 1), the Huffman code's lengths whenever those fit the limit.  n in 1..286, limit in 1..15, at most 2^limit symbols in
 * use, the counts' sum below 2^32; else PSEG_EINVAL. */
int pseg_png_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lengths);

/* compute_char_height (lib/image_ops.py:58-82) minus the file read: Otsu threshold, invert
 * unless `inverse`, 4-connected components, keep glyph-shaped ones, upper median of heights.
 * *height = -1 when no component qualifies (the reference returns None). *otsu gets the
 * threshold (may be NULL). */
int pseg_otsu_char_height(int device, const uint8_t* gray, int H, int W, int inverse,
                          int* height, int* otsu);

/* compute_char_height (lib/image_ops.py:58-82) for a list of scans in one device-resident call: heights[i] and otsu[i] (may be
 * NULL) are what pseg_otsu_char_height returns for gray[i] (H[i] x W[i], dense), for every input; a height of -1 means that no
 * component qualifies.  Host pointers, synchronous.  No label image and no component list: per scan a histogram launch, the Otsu
 * loop on the device, and a launch that labels a window around every 32 x 64 tile in LDS and bins the heights of the glyph-shaped
 * components (lib/image_ops.py:70-76) whose first pixel the tile owns; the upper median (lib/image_ops.py:77-82) is taken from 49
 * bins on the host.  The list is cut into GROUPS in list order: a group ends after 64 scans, or before the scan that would bring
 * its bytes above 64 MiB (a larger scan is a group of its own).  A group costs three launches and ONE host wait, for its records;
 * nothing is allocated per scan.  The workspace -- the group's scan bytes, 1280 bytes of record and 32 bytes of table per scan -- is
 * grow-only, cached per device and freed by pseg_release_workspace.
 * n == 0 returns PSEG_OK before a device is touched.  Every scan is checked before any device work and the message names it
 * ("scan 3: ..."): a NULL pointer or an empty shape is PSEG_EINVAL, H * W > 0x7fffffff PSEG_EUNSUPPORTED; nothing is written to
 * heights / otsu then, nor on any other error. */
int pseg_char_heights(int device, int n, const uint8_t* const* gray, const int* H, const int* W, int inverse,
                      int* heights, int* otsu);
/* The geometry that call's window kernel was compiled with (host arithmetic, no device; every pointer may be NULL): the owned
 * tile and the rows / columns of the scan a workgroup labels around it.  The glyph filter of lib/image_ops.py:72-76 admits boxes
 * of at most 59 rows and 49 columns, so with below >= 59, left >= 49, right >= 49 and above >= 1 a window decides exactly which
 * components with their first pixel in its tile qualify. */
int pseg_char_height_window(int* tile_h, int* tile_w, int* above, int* below, int* left, int* right);
/* The upper median of lib/image_ops.py:77-82 from height bins, as pseg_char_heights takes it (host arithmetic): bins[k] components
 * of height first + k; *height = the smallest height whose cumulative count exceeds n / 2 (integer division; sorted(hs)[len(hs) / 2]),
 * -1 when all bins are empty. */
int pseg_char_height_median(const uint32_t* bins, int n_bins, int first, int* height);

/* ---- PNG scans decoded on the device ---------------------------------------- */

/* The container of a PNG file held in memory (host arithmetic, no device): signature, IHDR first with length 13, the CRC of every
 * critical chunk, consecutive IDAT chunks (any of them may be empty), IEND.  Ancillary chunks are skipped unread, except tRNS.
 * *H, *W, *channels (each may be NULL) are set whenever IHDR could be read, else 0.  Returns PSEG_OK for what the decoder takes: bit
 * depth 8, colour type 0 (gray) or 2 (RGB), no interlace, no tRNS, H * (1 + W * channels) <= 0x7fffffff; PSEG_EUNSUPPORTED for every
 * other sound PNG (1/2/4/16 bit, palette, alpha, Adam7, tRNS, a critical chunk it does not know); PSEG_EINVAL for a broken
 * container.  No message is set: the value is a classification, not a failure of the call. */
int pseg_png_probe(const uint8_t* file, size_t n_bytes, int* H, int* W, int* channels);
/* n PNG files held in memory -> their gray scans, PIL's Image.open(f).convert("L") (RGB: (R*19595 + G*38470 + B*7471 + 0x8000) >> 16),
 * inflated and unfiltered on the device.  out[i]: H * W bytes of host memory for file i (shape from pseg_png_probe).  status[i] is
 * pseg_png_probe's value, or PSEG_EINVAL where the container is sound but the zlib stream is not (bad header, code set, symbol or
 * distance, wrong length, wrong Adler-32) or a row's filter byte is above 4.  out[i] of a file whose status is not PSEG_OK is left
 * untouched, and the other files are unaffected.  The call itself fails only on bad arguments (nothing is written then, status
 * included) or HIP errors.  n == 0 returns PSEG_OK before a device is touched; so does a list without a single sound file.
 * The sound files are cut into groups in list order: 64 files, or 64 MiB of inflated bytes.  A group is one upload of its IDAT
 * payloads (copied by the host into page-locked staging), two launches with one workgroup per file, one read-back and ONE host
 * wait.  The workspace (staging, IDAT and inflated bytes, gray scans, one record per file) is grow-only, cached per device, guarded
 * by its own lock and used on its own stream: the call may run on one thread while another thread runs an engine entry.
 * pseg_release_workspace frees it. */
int pseg_png_decode_gray(int device, int n, const uint8_t* const* files, const size_t* n_bytes, uint8_t* const* out, int* status);
/* The same with d_out[i] in device memory.  stream: the caller's stream whose enqueued work still uses the outputs (NULL: none); the
 * decoder's own stream waits for it.  The call returns after its last group's wait: the outputs are complete then. */
int pseg_png_decode_gray_device(int device, int n, const uint8_t* const* files, const size_t* n_bytes, uint8_t* const* d_out, int* status,
                                void* stream);
/* The same decoder run serially on the host, no device: the code the kernels are compiled from (csrc/pseg_pngdec.h). */
int pseg_png_decode_gray_host(int n, const uint8_t* const* files, const size_t* n_bytes, uint8_t* const* out, int* status);

/* ---- Line-height normalisation: lib/dataset.py:114-150, lib/util.py:21-29 ------------------ */

/* Output shape of skimage.transform.rescale as scale_binary calls it (lib/dataset.py:115):
 * np.round(scale * shape), half to even.  Host arithmetic only. */
int pseg_rescale_shape(int H, int W, double scale, int* Ho, int* Wo);

/* The anti-aliasing kernel scipy.ndimage.gaussian_filter builds for one axis: radius =
 * int(4 sigma + 0.5), w[i] = exp(-i^2 / 2 sigma^2) / sum, 2*radius+1 entries.  Uses libm's exp; a
 * caller that needs bit parity with a NumPy-based reference passes NumPy's kernel instead (the
 * two exp implementations can differ in the last bit).  w may be NULL to query the radius. */
int pseg_gaussian_kernel(double sigma, double* w, int cap, int* radius);

/* preserving_resize (lib/util.py:21-29) / scale_binary's gather (lib/dataset.py:114-119): order-0
 * warp of an (H,W) image of elem_bytes-sized pixels (1, 2, 3, 4 or 8) to (Ho,Wo).  Host pointers. */
int pseg_resize_nearest(int device, const void* src, int H, int W, int elem_bytes, void* dst,
                        int Ho, int Wo);

/* The same gather on device buffers, asynchronous on `stream` (scale_to_original_shape inside the Predictor chain). */
int pseg_resize_nearest_device(int device, const void* d_src, int H, int W, int elem_bytes, void* d_dst, int Ho, int Wo,
                               void* stream);

/* scale_image (lib/dataset.py:122-128): bicubic resize of a uint8 or float64 (H,W) plane to a
 * float64 (Ho,Wo) plane, clipped to the input range; Gaussian anti-aliasing (sigma = max(0,
 * (in/out - 1)/2) per axis) iff the image has more than two distinct values.  wy / wx: the
 * per-axis kernels with radii ry / rx (NULL: built with pseg_gaussian_kernel). */
int pseg_scale_image(int device, const void* src, int src_is_f64, int H, int W, double* dst,
                     int Ho, int Wo, const double* wy, int ry, const double* wx, int rx);

/* Augmentation warp (lib/data_generator.py / lib/network.py:149-161: keras-preprocessing's
 * apply_affine_transform -> scipy.ndimage.affine_transform(x, m, off, order, mode='nearest')): output pixel
 * (r, c) samples the input at m (r, c) + off; order 3 = cubic B-spline with prefilter (image), order 0 =
 * nearest (binary, mask).  float32 (H,W) planes, host pointers. */
int pseg_affine_warp(int device, const float* src, int H, int W, const double m[4], const double off[2],
                     int order, float* dst);
/* ... with the other fill mode the reference's AugmentationSettings name (lib/trainer.py:23-28 image_fill_mode / binary_fill_mode /
 * mask_fill_mode and *_cval -> keras-preprocessing apply_affine_transform(fill_mode, cval)): fill_mode 0 'nearest', 1 'constant'
 * (scipy mode='constant': cval where the source coordinate leaves [0, n - 1]; the spline prefilter runs on the unpadded plane),
 * 2 'reflect' (d c b a | a b c d | d c b a; half-sample-symmetric prefilter), 3 'wrap' (scipy's legacy 'wrap': period n - 1,
 * mirror prefilter) -- the four values keras-preprocessing accepts; semantics of scipy >= 1.6's map_coordinate. */
int pseg_affine_warp_fill(int device, const float* src, int H, int W, const double m[4], const double off[2],
                          int order, int fill_mode, float cval, float* dst);
/* AugmentationSettings.brightness_range (lib/trainer.py:21,33; removed from the binary / mask generators at :45,50): the image
 * generator draws one factor per sample and keras-preprocessing 1.1.2 applies apply_brightness_shift(x, factor, scale=False) --
 * through an 8-bit PIL image: planes outside [0, 255] are stretched to it first and mapped back afterwards, the gain is
 * PIL's ImageEnhance.Brightness (truncating blend with black, clipped).  src / dst: float32 planes of n values (all channels of
 * the sample: min / max are taken over the whole array), host pointers; dst may equal src. */
int pseg_brightness_shift(int device, const float* src, int64_t n, float brightness, float* dst);

/* ---- evaluation reductions ------------------------------------------------------------ */

/* Joint histogram behind fgpa / fgoverlap_per_class (lib/image_ops.py:8-55) and count_matches /
 * total_accuracy (lib/evaluation.py:8-32): counts[b][m][p] = pixels with (binary != 0) == b, mask label m,
 * predicted label p; (n_classes + 1) slots per axis, the last one collects labels outside [0, n_classes).
 * pred / mask: n labels of pred_bytes / mask_bytes (1, 4 or 8; signed for 4 and 8) each; binary may be NULL
 * (every pixel counts as ink).  counts: 2 * (n_classes+1)^2 int64.  Host pointers. */
int pseg_eval_confusion(int device, const void* pred, int pred_bytes, const void* mask, int mask_bytes,
                        const uint8_t* binary, int64_t n, int n_classes, int64_t* counts);

/* cv2.connectedComponentsWithStats(binary, connectivity)'s label image (lib/evaluation.py:84-85): 0 = paper,
 * components numbered 1.. in the order OpenCV's scan meets them (connectivity 4: raster order of the first
 * pixel; 8: raster order of the first 2x2 block).  labels: int32 (H,W); *num_labels counts the background. */
int pseg_cc_label(int device, const uint8_t* binary, int H, int W, int connectivity, int32_t* labels,
                  int32_t* num_labels);

/* Per-component tables for ConnectedComponentEval (lib/evaluation.py:73-117); every output may be NULL.
 * stats: int32 [num_labels][5] = cv2's LEFT, TOP, WIDTH, HEIGHT, AREA; centroids: double [num_labels][2]
 * (x, y); eq[l] = pixels of l with pred == mask; hist_pred / hist_mask: [num_labels][n_classes+1] class
 * counts (last slot: out of range); order: the H*W pixel indices sorted by (label, raster position), so
 * that `bbox(image)[component]` (lib/evaluation.py:104-106) is image.ravel()[order[o:o+area]]. */
int pseg_cc_tables(int device, const int32_t* labels, int H, int W, int num_labels, const void* pred,
                   int pred_bytes, const void* mask, int mask_bytes, int n_classes, int32_t* stats,
                   double* centroids, int64_t* eq, int64_t* hist_pred, int64_t* hist_mask, int32_t* order);

/* ---- a list of pages scored in one device-resident call ----------------------------- */

/* One page of pseg_eval_pages: pred and mask are uint8 (H,W) label maps; binary is uint8 (H,W) with ink != 0, or NULL. */
typedef struct pseg_eval_page {
    const uint8_t* pred;
    const uint8_t* mask;
    const uint8_t* binary;
    int H, W;
} pseg_eval_page;

/* One component matcher of lib/evaluation.py with its only_label filter (lib/evaluation.py:52-70, 87-101). */
typedef struct pseg_eval_rule {
    int kind;                    /* 0: cc_matching, 1: cc_equal (its threshold in threshold_tp) */
    int label;
    double threshold_tp, threshold_fp, threshold_mask;
    int filter_label;            /* only_label(); 0: no filter */
    double filter_threshold;
} pseg_eval_rule;

/* count_matches / total_accuracy / fgpa / fgoverlap_per_class (lib/evaluation.py:8-32, lib/image_ops.py:8-55) and the summed
 * verdicts of ConnectedComponentEval.run_per_component(cc_matching(...) / cc_equal(...)) (lib/evaluation.py:73-117) for a list of
 * pages.  All arrays are host pointers; any of the three outputs may be NULL.
 *   counts[page]     = what pseg_eval_confusion(pred, 1, mask, 1, binary, H*W, n_classes, ...) returns for the page (binary == NULL:
 *                      every pixel counts as ink).
 *   components[page] = the `connectivity`-connected components of binary != 0 (0 for binary == NULL: such a page has no components,
 *                      and its verdicts are zero).
 *   verdicts[page][r] for rule r, over the components the rule KEEPS: with s the component's pixel count, e its pixels with
 *                      pred == mask (raw bytes), P[L] / M[L] its pixels with pred == L / mask == L, a component is kept when
 *                      filter_label == 0, or M[fl] / s >= filter_threshold, or P[fl] > 0 (ConnectedComponentEval._filter: a falsy
 *                      label is no filter).  kind 0 adds (ptp && mm, pfp && !mm, mm && !ptp) to slots 0..2, with ptp = P[l] / s >=
 *                      threshold_tp, pfp = P[l] / s >= threshold_fp, mm = M[l] / s >= threshold_mask; kind 1 adds 1 to slot 0 when
 *                      e / s >= threshold_tp, else to slot 1.  Slot 3 counts the kept components.  The quotients are IEEE double
 *                      divisions of the two integers, the comparisons double comparisons: a decision has Python's bits.
 * These are the sums of what run_per_component yields; they are order-free, and no component numbering is produced.
 * n_classes in 1..255, connectivity 4 or 8, n_rules in 0..8, every rule label and filter label in [0, n_classes), H, W >= 0 (a page
 * without pixels gives zeros).  Every page and rule is checked before the first device call and PSEG_EINVAL names it ("page 3: ...",
 * "rule 1: ..."); the caller's arrays are written only after the last group has run, and not at all on an error.  n_pages == 0
 * returns PSEG_OK with no device work.
 * The list is cut into GROUPS in list order (pseg_eval_page_groups): a group ends after 64 pages, or before the page that would
 * bring its pixels above 64 Mi (a larger page is a group of its own).  A group is one table upload, one memset of its records, its
 * maps copied to 256-byte-aligned offsets, five launches ragged over the group (histogram; 32 x 64 tiles: closed components judged
 * in LDS, open ones to root slots; unions across tile edges; counters to final roots; final roots judged), the records into
 * page-locked memory and ONE host wait.  No label image, sort or component list: beyond the maps the workspace is 192 root slots
 * (4 + 4 * (2 + 2 * watched labels) bytes each), 192 bytes of rim table, 768 bytes of union tasks and 8 bytes of list lengths per
 * tile.  It is grow-only, cached per device, guarded by its own lock and used on its own stream; pseg_release_workspace frees it. */
int pseg_eval_pages(int device, int n_pages, const pseg_eval_page* pages, int n_classes, int connectivity,
                    int n_rules, const pseg_eval_rule* rules,
                    int64_t* counts,      /* [n_pages][2][K][K], K = n_classes + 1: pseg_eval_confusion's layout per page */
                    int64_t* components,  /* [n_pages]: ink components of the page */
                    int64_t* verdicts);   /* [n_pages][n_rules][4] */
/* How pseg_eval_pages cuts a page list into groups (host logic, no device needed).  Returns the number of groups (>= 0) and fills
 * first / count (each may be NULL) for the first max_groups of them, or a negative PSEG_E*. */
int pseg_eval_page_groups(int n_pages, const int* H, const int* W, int* first, int* count, int max_groups); /* host only */

/* prepare_images (lib/dataset.py:131-150), all pixel work on the device in one call.
 * image, binary: uint8 (H0,W0) scan and binarisation (paper = 1 or 255).  (H1,W1) =
 * pseg_rescale_shape(H0, W0, target_line_height / line_height_px); (H2,W2) = the max_width stage
 * (pseg_rescale_shape(H1, W1, max_width / W1) when that factor is < 1), or 0,0 for none.
 * Outputs: out_img uint8 network input (ink bright), out_bin uint8 ink = 1, both of the final
 * shape; out_orig_bin (H0,W0) ink map (may be NULL); out_stage1 float64 (H1,W1) bicubic result
 * before inversion (may be NULL; tests). */
int pseg_prepare_images(int device, const uint8_t* image, const uint8_t* binary, int H0, int W0,
                        int H1, int W1, const double* wy1, int ry1, const double* wx1, int rx1,
                        int H2, int W2, const double* wy2, int ry2, const double* wx2, int rx2,
                        uint8_t* out_img, uint8_t* out_bin, uint8_t* out_orig_bin,
                        double* out_stage1);

/* ---- Scans straight into the page chain: binarisation and line-height normalisation on the device ------------------------ */

/* One gray scan and the page it becomes.  gray: uint8 (H0,W0), ink dark.  (H,W) = pseg_rescale_shape(H0, W0, target_line_height /
 * line_height_px).  wy / wx: the anti-aliasing weights of axis 0 / axis 1 (2 r + 1 doubles; NULL: built with
 * pseg_gaussian_kernel); ry / rx must equal int(4 sigma + 0.5) with sigma = max(0, (in / out - 1) / 2) of the axis, and are not
 * read where sigma <= 1e-15 (no pass on that axis).  final_is_scan (pseg_predict_chain_scans_png only): the label map is rescaled
 * to (H0,W0) and voted / masked against the scan-sized ink map (PredictSettings.high_res_output). */
typedef struct pseg_scan {
    const uint8_t* gray;
    int H0, W0;
    int H, W;
    const double* wy;
    int ry;
    const double* wx;
    int rx;
    int final_is_scan;
} pseg_scan;

/* pseg_prepare_images(scan, where(scan > 127, 255, 0)) without a max_width stage for n scans, bit for bit, by the device-resident
 * front end of pseg_predict_chain_scans_png: the binarisation is never an input (ink is scan <= 127), and per scan at most three
 * launches run -- a pass that ORs the scan's 256-bit value bitmap into its record (min, max and "more than two distinct values"
 * are read from it on the device) and writes the scan-sized ink map where asked for; a tiled Gaussian that runs both
 * anti-aliasing passes through LDS (radii up to 8; larger ones take the one-pass-per-launch kernels) and stores the scan
 * unfiltered where the record says two values or fewer; a sampler that does the bicubic taps, the clip, the inversion and the
 * nearest gather of the ink map per output pixel.  No allocation, device-to-host read or wait happens between the launches.
 * Host pointers: out_img[i], out_bin[i]: uint8 (H,W); out_orig[i]: uint8 (H0,W0), the array or an entry may be NULL.  Every scan is
 * checked before any device work starts (PSEG_EINVAL names the scan). */
int pseg_prepare_scans(int device, int n, const pseg_scan* scans, uint8_t* const* out_img, uint8_t* const* out_bin,
                       uint8_t* const* out_orig);

/* pseg_predict_chain_pages_mixed_png with scans in place of pages and binarisations: a unit's scans go up into a staging slot of
 * the set, the front end above writes every page and its ink map (final_is_scan: the scan-sized one) where the unit's network
 * stage and post-processors read them, and everything behind that is the mixed page chain -- same units (by the canvas of
 * (H,W)), same bytes per (scan, output) as that call fed with pseg_prepare_images' outputs, same sink contract, same drained
 * return.  The filtered planes, the per-scan records and the call's weights table (page-locked, uploaded once) are staging of the
 * engine, sized up front for the largest unit; pseg_engine_trim frees them.  Only an engine with one input channel takes this
 * entry (PSEG_EUNSUPPORTED otherwise).  Every scan is checked before any device work starts. */
int pseg_predict_chain_scans_png(pseg_engine* e, int n_scans, const pseg_scan* scans,
                                 const int* post_ops, int n_post, unsigned flags,
                                 const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap,
                                 pseg_chain_sink sink, void* user);

/* ---- Adaptive binarisation of scans on the device ------------------------------------------------------- */

/* How a scan becomes its ink map.  window == 0: the fixed threshold, ink = scan <= 127 (k and R are not read).  Otherwise Sauvola's
 * threshold over a square window of odd side `window`, 3 .. 255, radius r = window / 2, indices outside the scan mirrored without an
 * edge repeat (NumPy's mode='reflect'), so that every pixel has n = window * window samples:
 *   S1 = sum of the window's values, S2 = sum of their squares (integers);  m = S1 / n;  var = S2 / n - m * m;
 *   s = sqrt(max(var, 0));  T = m * (1 + k * (s / R - 1));  ink = value <= T
 * in float64, in this operation order.  0 <= k <= 1, R > 0; the usual choice is k = 0.2, R = 128. */
typedef struct pseg_binarize {
    int window;
    double k, R;
} pseg_binarize;

/* The ink maps of n gray scans (gray[i]: uint8 H[i] x W[i], dense) in one device-resident call: out_ink[i] uint8 H x W, ink = 1;
 * out_threshold (the array or any entry may be NULL): float64 H x W, the threshold T of every pixel (127 for a fixed entry).  how has
 * one entry per scan.  Host pointers, synchronous.  The cost per pixel does not depend on the window: a launch writes the packed
 * row sums (one 64-bit word per pixel), a second one slides the window sums down every column and decides; integer sums only.  The
 * list is cut into groups as pseg_char_heights cuts it (64 scans, or 64 MiB of scan bytes); a group costs two ragged launches and
 * ONE host wait, nothing is allocated per scan.  The workspace (per pixel: the scan, the ink map, 8 bytes of row sums and 8 bytes
 * of threshold where asked for) is grow-only, cached per device and freed by pseg_release_workspace.
 * n == 0 returns PSEG_OK before a device is touched.  Every scan is checked before any device work and the message names it
 * ("scan 3: ..."): an even window, a window outside 3 .. 255 other than 0, k outside [0, 1], R <= 0, a NULL pointer or an empty
 * shape is PSEG_EINVAL; nothing is written to the outputs then. */
int pseg_binarize_scans(int device, int n, const uint8_t* const* gray, const int* H, const int* W, const pseg_binarize* how,
                        uint8_t* const* out_ink, double* const* out_threshold);
/* The same on the host, without a device: the same decision function over the same integer sums, the same bits. */
int pseg_binarize_scans_host(int n, const uint8_t* const* gray, const int* H, const int* W, const pseg_binarize* how,
                             uint8_t* const* out_ink, double* const* out_threshold);

/* The geometry the device kernels were compiled with (host arithmetic, no device; every pointer may be NULL): a row workgroup takes
 * *segment padded pixels, i.e. owns segment - (window - 1) columns of a row; a column workgroup slides *tile columns down *band
 * rows; rows go through LDS in *vector-byte loads from an aligned address. */
int pseg_binarize_geometry(int* segment, int* band, int* tile, int* vector);

/* pseg_prepare_scans with the binarisation of scan i given by how[i]: equals pseg_prepare_images(scan, where(ink, 0, 255)) with ink
 * from pseg_binarize_scans, bit for bit.  how == NULL, or window == 0, is pseg_prepare_scans' own path.  With an adaptive entry the
 * scan-sized ink map is written by the binarisation kernels (into out_orig's staging where asked for, else into workspace), the
 * statistics pass writes none and the sampler gathers from it; no allocation, read-back or wait enters the front end.  how is
 * checked for every scan before any device work, as above. */
int pseg_prepare_scans_bin(int device, int n, const pseg_scan* scans, const pseg_binarize* how, uint8_t* const* out_img,
                           uint8_t* const* out_bin, uint8_t* const* out_orig);
/* pseg_predict_chain_scans_png with the binarisation of scan i given by how[i] (NULL, or window == 0: that call's own path): the
 * ink map that the vote, the masks and the final_is_scan route work on is the adaptive one.  The ink plane (where the scan-sized
 * map is not the unit's binarisation itself) and the row sums are part of the filtered-plane staging, sized up front. */
int pseg_predict_chain_scans_bin_png(pseg_engine* e, int n_scans, const pseg_scan* scans, const pseg_binarize* how,
                                     const int* post_ops, int n_post, unsigned flags,
                                     const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap,
                                     pseg_chain_sink sink, void* user);

/* ---- Training masks as label maps on the device ---------------------------------------------------------- */

/* One ground-truth mask as it was decoded: px is H0 x W0 x channels bytes, dense.  channels == 3: RGB, a colour table turns a pixel
 * into its label id; channels == 1: the bytes are label ids already. */
typedef struct pseg_mask_src {
    const uint8_t* px;
    int H0, W0, channels;
} pseg_mask_src;

/* The label maps of n masks at the shapes of their pages, in one device-resident call: out_labels[i] is uint8 H[i] x W[i], dense.
 * Output pixel (r, c) reads source pixel (sr, sc), the coordinate of pseg_resize_nearest: per axis f = n_in / n_out,
 * v = f * o + (f * 0.5 - 0.5) in float64, rounded half away from zero, mirrored without an edge repeat.  Its label is, for an RGB
 * source, the id of the table entry whose colour equals the pixel's three bytes, and 0 where none does (an unknown colour); for a
 * 1-channel source the byte itself.  The table: n_colors entries, 0 .. 256, colors n_colors x 3 bytes and ids n_colors bytes; a
 * colour mapped to id 0 is a known colour; n_colors == 0 is legal (every RGB pixel is unknown; colors and ids may be NULL then, and
 * for a list of 1-channel masks).  This is the label map of "colours to ids on the whole mask, then pseg_resize_nearest", byte for
 * byte: the lookup is pointwise and the gather moves whole pixels, so the two commute and only the sampled pixels are looked up.
 * out_counts (may be NULL): n x 257 int64; [i][k], k < 256: the output pixels of mask i that received id k; [i][256]: its output
 * pixels of unknown colour (they are counted under id 0 as well).
 * Host pointers, synchronous.  The list is cut into groups as pseg_char_heights and pseg_binarize_scans cut theirs (64 masks, or 64
 * MiB of source bytes; a single larger mask is a group of its own); a group costs ONE ragged launch and ONE host wait, nothing is
 * allocated per mask.  The workspace (per source pixel its 3 or 1 bytes, per output pixel 1 byte, the tables and 257 64-bit
 * counters per mask of a group) is grow-only, cached per device and freed by pseg_release_workspace.
 * n == 0 returns PSEG_OK before a device is touched.  Every mask is checked before any device work and the message names it
 * ("mask 3: ..."): a NULL pointer, an empty source or output shape, channels other than 1 or 3, n_colors outside 0 .. 256, a
 * duplicate colour, or an RGB mask with n_colors > 0 and a NULL table is PSEG_EINVAL; nothing is written to any output then. */
int pseg_label_masks(int device, int n, const pseg_mask_src* masks, const int* H, const int* W,
                     const uint8_t* colors, const uint8_t* ids, int n_colors, uint8_t* const* out_labels, int64_t* out_counts);
/* The same on the host, without a device: the same coordinate and lookup functions, the same bytes and counts. */
int pseg_label_masks_host(int n, const pseg_mask_src* masks, const int* H, const int* W,
                          const uint8_t* colors, const uint8_t* ids, int n_colors, uint8_t* const* out_labels, int64_t* out_counts);

/* The geometry the device kernel was compiled with and the group cut (host arithmetic, no device; every pointer may be NULL): a
 * thread owns *run consecutive output pixels of a row, written with one *run-byte store where the run is whole; a workgroup owns
 * *runs runs of each of *rows rows; a group ends after *group_masks masks or before *group_bytes source bytes are passed. */
int pseg_label_masks_geometry(int* run, int* runs, int* rows, int* group_masks, int64_t* group_bytes);
/* group_of[i]: the group pseg_label_masks puts mask i into (only H0, W0 and channels are read; host arithmetic, no device). */
int pseg_label_masks_groups(int n, const pseg_mask_src* masks, int* group_of);

/* ---- Despeckling of ink maps on the device ---------------------------------------------------------------- */

/* How an ink map is despeckled: every ink component (connectivity 4 or 8) of at most max_area pixels becomes paper.
 * 1 <= max_area <= 16 777 216.  max_area == 0: the map is not despeckled (connectivity is not read). */
typedef struct pseg_despeckle {
    int max_area;
    int connectivity;
} pseg_despeckle;

/* n ink maps (ink[i]: uint8 H[i] x W[i], dense, non-zero = ink) without their specks, in one device-resident call.  For a map with
 * max_area >= 1, integer-exact:
 *   lab, k = scipy.ndimage.label(ink != 0, structure)          (the cross for connectivity 4, 3 x 3 ones for 8)
 *   size   = bincount(lab);   out = (lab > 0) & (size[lab] > max_area)          as uint8: kept ink is 1, everything else 0
 * so the operation is idempotent.  A map with max_area == 0 is copied to out[i] byte for byte and causes no device work.
 * out[i] may be ink[i].  out_counts (may be NULL): n x 3 int64: the components erased, the pixels erased, the components kept
 * (zeros for a map that is not despeckled).
 * Host pointers, synchronous.  The list is cut into groups as pseg_binarize_scans cuts it (64 maps, or 64 MiB of map bytes); a group
 * costs four ragged launches (five where both connectivities occur in it) and ONE host wait, nothing is allocated per map.  The
 * workspace (per pixel the map's byte; per 32 x 64 tile the bytes pseg_despeckle_geometry's constants imply: root slots with parent
 * and size, rim table, task list, run list) is grow-only, cached per device with its own stream and freed by pseg_release_workspace.
 * n == 0 returns PSEG_OK before a device is touched.  Every map is checked before any device work and the message names it
 * ("map 3: ..."): max_area outside 0 .. 16 777 216, a connectivity other than 4 or 8, a NULL pointer or an empty shape is
 * PSEG_EINVAL, a map of 2^31 pixels or more PSEG_EUNSUPPORTED; nothing is written to the outputs then.  An output is written only
 * by a group that ran. */
int pseg_despeckle_maps(int device, int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_despeckle* how,
                        uint8_t* const* out, int64_t* out_counts);
/* The same on the host, without a device: a two-pass union-find over the whole page (not the tile scheme), the same bytes and counts. */
int pseg_despeckle_maps_host(int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_despeckle* how,
                             uint8_t* const* out, int64_t* out_counts);
/* pseg_prepare_scans_bin with the despeckling of scan i given by dsp[i]: equals pseg_prepare_images(scan, where(clean, 0, 255)) with
 * clean = pseg_despeckle_maps of the scan's ink map (pseg_binarize_scans' for an adaptive entry, scan <= 127 else), bit for bit.
 * dsp == NULL, or max_area == 0, is pseg_prepare_scans_bin's own path and bytes.  With a despeckle entry the scan-sized ink plane is
 * always materialised (for a fixed threshold the statistics pass writes it), the despeckle launches run on it in front of the
 * sampler, which gathers from it; the plane and the per-tile workspace are part of the staging, sized up front: no allocation,
 * read-back or wait enters the front end.  how and dsp are checked for every scan before any device work ("scan 3: ..."). */
int pseg_prepare_scans_clean(int device, int n, const pseg_scan* scans, const pseg_binarize* how, const pseg_despeckle* dsp,
                             uint8_t* const* out_img, uint8_t* const* out_bin, uint8_t* const* out_orig);
/* pseg_predict_chain_scans_bin_png with the despeckling of scan i given by dsp[i] (NULL, or max_area == 0: that call's own path): the
 * ink map that the vote, the masks and the final_is_scan route work on is the despeckled one (on that route the plane is the unit's
 * binarisation block itself).  A call that needs no ink map -- neither masks nor a vote -- launches nothing for it. */
int pseg_predict_chain_scans_clean_png(pseg_engine* e, int n_scans, const pseg_scan* scans, const pseg_binarize* how,
                                       const pseg_despeckle* dsp, const int* post_ops, int n_post, unsigned flags,
                                       const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap,
                                       pseg_chain_sink sink, void* user);
/* The geometry the device kernels were compiled with (host arithmetic, no device; every pointer may be NULL): a workgroup labels a
 * *tile_h x *tile_w tile; a tile has *slots root slots for the components that reach across its edge and lists at most *run_cap runs. */
int pseg_despeckle_geometry(int* tile_h, int* tile_w, int* slots, int* run_cap);

/* ---- Text regions from label maps on the device: rectangle morphology, hole filling, a region table ---------- */

/* How a label map becomes text regions: the label id (0..255) and the sides of the three rectangles (each 1..255; a side of 1 is the
 * identity): k_close closes, k_open opens, k_join joins (two dilations, one erosion). */
typedef struct pseg_regions {
    int label;
    int k_close;
    int k_open;
    int k_join;
} pseg_regions;

/* The text regions of n label maps (labels[i]: uint8 H[i] x W[i], dense) in one device-resident call.  Integer-exact, for map i with
 * t = how[i].label and the sides k1, k2, k3:
 *   dil(m, k)[y, x] = OR  over dy, dx in 0..k-1 of m[y + dy - k/2, x + dx - k/2],  m = 0 outside the map
 *   ero(m, k)[y, x] = AND over the SAME offsets,                                    m = 1 outside the map
 *   m0 = (lab == t);  m1 = ero(dil(m0, k1), k1);  m3 = dil(ero(m1, k2), k2);  rt = ero(dil(dil(m3, k3), k3), k3)
 *   T  = m3 | fill(rt)        fill: rt plus every 4-connected component of ~rt that touches no edge of the map
 *                             (scipy.ndimage.binary_fill_holes with its default structure)
 * Both operations use the same offsets (anchor k/2, the element is not reflected): with an even k a close is a close shifted by one
 * pixel, neither extensive nor idempotent, and the contract keeps that.  This restates OpenCV's documented rules for cv2.dilate /
 * cv2.erode with a rectangle and what the reference's get_text_contours does with them; parity with cv2 itself is UNPINNED (OpenCV
 * is not part of the build or test environment).  Not reproduced on purpose: cv2's reversed contour order, the white islands inside
 * a region that RETR_CCOMP would also list, and cv2's vertex sets.
 * The regions are the 4-connected components of T.  out_mask (may be NULL, and so may single entries): out_mask[i] is uint8
 * H[i] x W[i], 1 = T.  out_table (may be NULL with max_regions == 0): n x max_regions x 8 int32, one row per region: x0, y0, x1, y1
 * (exclusive), area, seed_y, seed_x, 0; the seed is the region's first pixel in raster order and the rows are sorted by it.
 * out_count[i] is always the true number of regions of map i; its rows are valid only when out_count[i] <= max_regions and are left
 * untouched otherwise.
 * Host pointers, synchronous.  The list is cut into groups as pseg_despeckle_maps cuts it (64 maps, or 64 MiB of map bytes); a group
 * costs a fixed number of ragged launches (pack, seven rectangle operations, four per component pass, unpack) and ONE host wait,
 * nothing is allocated per map.  The workspace (per pixel the map's byte and three bit planes; per 32 x 64 tile the bytes
 * pseg_regions_geometry's constants imply; the tables) is grow-only, cached per device with its own stream and freed by
 * pseg_release_workspace.  n == 0 returns PSEG_OK before a device is touched.  Every map is checked before any device work and the
 * message names it ("map 3: ..."): a side outside 1..255, a label outside 0..255, a NULL pointer or an empty shape is PSEG_EINVAL, a
 * map of 2^31 pixels or more PSEG_EUNSUPPORTED; nothing is written to the outputs then. */
int pseg_text_regions(int device, int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                      uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count);
/* The same bytes on the host, without a device: the same word arithmetic for the x pass, a plain y pass, and a two-pass union-find
 * over the whole page (not the tile scheme). */
int pseg_text_regions_host(int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                           uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count);
/* The constants the kernels were compiled with (host arithmetic, no device; every pointer may be NULL): a plane word holds *word
 * pixels; a morphology workgroup owns *band rows of *band_words words; a component workgroup labels a *tile_h x *tile_w tile, which
 * has *slots root slots for the components that reach across its edge. */
int pseg_regions_geometry(int* word, int* band, int* band_words, int* tile_h, int* tile_w, int* slots);
/* The crack polygons of the regions of a mask (uint8 H x W, non-zero = T; table: n_regions rows as above, only the seeds are read), on
 * the host: the outer boundary of a region along pixel edges, clockwise, from the seed's top-left corner; vertices are pixel corners
 * (x in 0..W, y in 0..H) and only direction changes are kept; where two pixels meet only diagonally the walk turns so that they stay
 * apart.  xy: cap int32 (x, y) pairs; first: n_regions + 1 offsets in vertices (region i owns [first[i], first[i + 1])).  When cap is
 * too small, the needed size is returned in first[n_regions], no vertex and no other offset is written, and the call is PSEG_OK.  A
 * row whose seed is not the first pixel of a region of the mask is PSEG_EINVAL. */
int pseg_trace_regions_host(const uint8_t* mask, int H, int W, int n_regions, const int32_t* table, int32_t* xy, int64_t cap, int64_t* first);
/* pseg_text_regions with the crack polygons traced on the device, from the bit plane of T (64 pixels to a word; horizontal stretches
 * are taken a word at a time): a count pass, a scan of the counts over the group's rows and a write pass, one lane per region, no host
 * wait between them.  Table, counts and masks are exactly pseg_text_regions'; the polygons are exactly pseg_trace_regions_host's for
 * the same rows.  xy: cap int32 (x, y) pairs for the whole list; first: n x (max_regions + 1) offsets in vertices: region r of map i
 * owns [first[i][r], first[i][r + 1]), the offsets run across the list (first[i][0] is the end of map i - 1) and those behind a map's
 * last region repeat its end.  status[i]: PSEG_OK; PSEG_EUNSUPPORTED when out_count[i] > max_regions (no polygons, its row of offsets
 * is the running offset); PSEG_EHIP when a walk did not close within its bound of 4 (H + 1) (W + 1) + 4 steps (likewise).  When the
 * list's vertex total exceeds cap, first[n - 1][max_regions] holds the needed total, no vertex and no other offset is written, tables,
 * counts, masks and status are valid, and the call is PSEG_OK.  Refused as pseg_text_regions refuses, and PSEG_EINVAL for a NULL first
 * or status, a negative cap, or a cap without xy; nothing is written then.  A group costs pseg_text_regions' launches, three more, and
 * a second host wait for exactly the rows' vertex counts, offsets and vertices it holds. */
int pseg_text_regions_poly(int device, int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                           uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count,
                           int32_t* xy, int64_t cap, int64_t* first /* n x (max_regions + 1) */, int* status /* n */);
/* The same bytes on the host, without a device: pseg_text_regions_host, then the same word-run walk over host bit planes. */
int pseg_text_regions_poly_host(int n, const uint8_t* const* labels, const int* H, const int* W, const pseg_regions* how,
                                uint8_t* const* out_mask, int max_regions, int32_t* out_table, int* out_count,
                                int32_t* xy, int64_t cap, int64_t* first, int* status);
/* The page chain with the text regions as a stage: pseg_predict_chain_pages_png (mixed == 0) or pseg_predict_chain_pages_mixed_png
 * (mixed != 0) with bit 5 of `want`: after a unit's post-processors its final label maps go, where they lie on the device, through
 * pseg_text_regions' launches and the tracer of pseg_text_regions_poly on the engine's stream; the maps never visit the host for it.
 * how: one pseg_regions per page of the list (checked before any device work: "page 3: ..."); how == NULL is the plain entry (bit 5
 * is refused then), and without bit 5 nothing of the stage runs.  want == 32 alone is a valid request.  max_regions >= 1 and
 * max_vertices >= 0 are every page's capacities.  The stage's workspace and records belong to the staging sets: sized by the plan,
 * freed by pseg_engine_trim; after a unit's done event exactly the rows and vertices its pages hold are downloaded.
 * sink(user, page, 5, blob, n_bytes) comes after the page's label map.  The blob is int32: n_regions, n_vertices, status, 0; then
 * n_regions rows of 8 (pseg_text_regions' table, sorted by seed); then n_regions + 1 offsets in vertices; then n_vertices (x, y)
 * pairs.  n_regions > max_regions: the header alone, status PSEG_EUNSUPPORTED.  n_vertices > max_vertices: the header and the rows,
 * status PSEG_ENOMEM (n_vertices is what the page needs).  A walk that gave up: the header and the rows, status PSEG_EHIP. */
int pseg_predict_chain_pages_regions_png(pseg_engine* e, int n_pages, const uint8_t* const* imgs, const int* H, const int* W,
                                         const int* Ho, const int* Wo, const uint8_t* const* binaries, const int* post_ops, int n_post,
                                         unsigned flags, const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap, int mixed,
                                         const pseg_regions* how, int max_regions, int max_vertices, pseg_chain_sink sink, void* user);
/* pseg_predict_chain_scans_clean_png with the same stage (rg: one pseg_regions per scan, or NULL). */
int pseg_predict_chain_scans_regions_png(pseg_engine* e, int n_scans, const pseg_scan* scans, const pseg_binarize* how,
                                         const pseg_despeckle* dsp, const int* post_ops, int n_post, unsigned flags,
                                         const uint8_t* lut, int n_lut, int level, unsigned want, int unit_cap,
                                         const pseg_regions* rg, int max_regions, int max_vertices, pseg_chain_sink sink, void* user);

/* ---- Deskewing on the device: the skew of an ink map from strip profiles, an exact rotation --------------------- */

/* Integer arithmetic only: every division below is a floor division, every >> an arithmetic shift, for negative values too.
 * Limits: 1 <= H, W <= 16384; a denominator 64 <= D <= 4096; steps 1 <= A <= 128 with 4 A <= D (a slope is at most 1/4); for a
 * rotation |index| * 4 <= D, order 0 or 1, fill 0..255.  Anything else is PSEG_EINVAL, the message names the map ("map 3: ...") and
 * nothing is written.  n == 0 returns PSEG_OK before a device is touched.
 *
 * THE SKEW of an ink map (uint8, dense, non-zero = ink):
 *   strips      a strip is 32 columns wide, K = ceil(W / 32); R[y][k] = ink pixels of row y in columns 32 k .. min(32 k + 31, W - 1)
 *   candidates  a = -A .. A, the slope of candidate a is a / D
 *   centre      cx2(k) = 64 k + 32 - W: the doubled nominal centre of strip k relative to the map's centre (also for a ragged last strip)
 *   offset      off(a, k) = floor((a * cx2(k) + D) / (2 D))
 *   apron       M = max |off(a, k)| over candidates and strips (reached at a = +-A, k = 0 or K - 1)
 *   profile     P_a[j] = sum over k of R[j + off(a, k)][k]  for j = -M .. H - 1 + M; rows outside 0 .. H - 1 count 0.  The apron
 *               drops nothing: the sum of P_a is the same for every a
 *   score       score(a) = sum over j of P_a[j]^2, uint64 (at most 2^28 * 2^15)
 *   winner      the largest score; ties go to the smallest |a|, then to a > 0.  A map without ink has index 0
 * Text lines that run along y = y0 + (a / D) (x - cx) make candidate a the sharpest.
 *
 * THE ROTATION by index a over D: the output has the input's shape and is turned about the map's centre.
 *   r = sqrt((double)(D D + a a));  C = floor(16384.0 * D / r + 0.5);  S = sign(a) * floor(16384.0 * |a| / r + 0.5)   (on the host)
 *   for output pixel (y, x):  u = 2 x - (W - 1),  v = 2 y - (H - 1)
 *     X = C u - S v + (W - 1) * 16384,   Y = S u + C v + (H - 1) * 16384      source coordinates in 1 / 32768 pixel, |X|, |Y| < 2^30
 *   order 0:  xs = (X + 16384) >> 15, ys likewise;  out = src[ys][xs], or fill outside the map
 *   order 1:  x0 = X >> 15, fx = X & 32767, y0, fy likewise, w = 32768;
 *             out = ((w-fx)(w-fy) p00 + fx (w-fy) p01 + (w-fx) fy p10 + fx fy p11 + 2^29) >> 30   in 64 bits; a tap outside takes fill
 * Index 0 is the identity, byte for byte.  Rotating by the estimated index makes the text lines horizontal; an output cannot be
 * its own source. */
typedef struct pseg_skew   { int steps, denom; } pseg_skew;
typedef struct pseg_rotate { int index, denom, order, fill; } pseg_rotate;

/* The skew indices of n ink maps.  out_scores: NULL, or n pointers each NULL or to 2 * steps + 1 scores (candidate a at a + steps).
 * Host pointers, synchronous.  The list is cut into groups as pseg_despeckle_maps cuts it (64 maps, or 64 MiB of map bytes); a group
 * costs three ragged launches (strip counts, a workgroup per candidate and map with one plain store -- no atomics, so the scores are
 * deterministic --, the pick) and ONE host wait, nothing is allocated per map.  The workspace is grow-only, cached per device with
 * its own stream and freed by pseg_release_workspace.  Every map is checked before any device work. */
int pseg_skew_maps(int device, int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_skew* how,
                   int32_t* out_index, uint64_t* const* out_scores);
/* The same on the host, without a device: the same functions (csrc/pseg_skew.h) in plain loops. */
int pseg_skew_maps_host(int n, const uint8_t* const* ink, const int* H, const int* W, const pseg_skew* how,
                        int32_t* out_index, uint64_t* const* out_scores);
/* n maps rotated, one launch and one wait per group. */
int pseg_rotate_maps(int device, int n, const uint8_t* const* src, const int* H, const int* W, const pseg_rotate* rot,
                     uint8_t* const* out);
int pseg_rotate_maps_host(int n, const uint8_t* const* src, const int* H, const int* W, const pseg_rotate* rot,
                          uint8_t* const* out);
/* Estimate and correct in one device-resident call.  ink[i] NULL (or ink NULL): ink = gray <= 127, decided on the device.
 * out_gray[i] = gray[i] rotated by the winner, order 1, fill 255; out_index[i] the winner.  Four launches and one wait per group:
 * no host wait lies between the estimate and the rotation, which reads the winner from device memory. */
int pseg_deskew_scans(int device, int n, const uint8_t* const* gray, const uint8_t* const* ink, const int* H, const int* W,
                      const pseg_skew* how, uint8_t* const* out_gray, int32_t* out_index);
int pseg_deskew_scans_host(int n, const uint8_t* const* gray, const uint8_t* const* ink, const int* H, const int* W,
                           const pseg_skew* how, uint8_t* const* out_gray, int32_t* out_index);
/* The constants of the contract (host arithmetic, no device; every pointer may be NULL). */
int pseg_skew_geometry(int* strip, int* max_steps, int* max_side);

#ifdef __cplusplus
}
#endif
#endif /* PSEG_H */
