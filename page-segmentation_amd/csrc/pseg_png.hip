// pseg_png.hip -- PNG encoder whose pixels are in device memory (lib/output.py:20-41 writes the three masks with
// PIL.Image.save; the reference has no device-side counterpart).  The output is a complete PNG byte stream:
//
//   signature | IHDR | IDAT(78 01) | IDAT(band 0) | IDAT(band 1) | ... | IDAT(01 00 00 FF FF, Adler-32) | IEND
//
// The image is cut into bands of R rows; one workgroup deflates one band, independently of every other, into its own slot
// of the workspace.  A band is ONE fixed-Huffman block (BFINAL = 0) followed by an empty stored block (the zlib "sync
// flush": 00 00 FF FF after the three header bits and the padding), so it ends on a byte and the bands concatenate into one
// valid deflate stream; the last IDAT holds the final empty stored block and the Adler-32.  Three launches, ordered by the
// stream -- no workgroup waits for another:
//   1. png_band_kernel   bands -> slots, per band {bytes, Adler partial (sum, weighted sum)}
//   2. png_frame_kernel  scan of the band sizes -> final offsets, the combined Adler-32, signature / IHDR / first and last
//                        IDAT / IEND, the total size
//   3. png_gather_kernel bands -> their final offsets with the chunk framing
// The chunk CRCs run over the COMPRESSED bytes; the host fills them in on the downloaded stream (table-driven, slicing by 8).
//
// Inside a band: every scanline is filtered with Up (filter byte 2; the row above comes from the SOURCE, also for a band's
// first row; the image's first row sees zeros).  The band's filtered bytes are walked in segments of 4096 bytes: 256 threads
// x 16 bytes.  Matches are runs against the byte `channels` back (the pixel to the left; zeros of the Up filter match at any
// distance), never reaching in front of the band's first byte; a run is cut at a segment start and into tokens of 258
// with a remainder of >= 3 as a shorter match and 1 or 2 as literals.  Token bit lengths are prefix-summed over the workgroup,
// the bits are ORed into an LDS bit buffer (deflate packs LSB first, Huffman codes go in bit-reversed) and whole 32-bit words
// are streamed to the slot; the partial last word is carried into the next segment.  No match has a distance other than
// `channels` (1 or 3), so deflate's 32 768-byte window is never a concern.
//
// Level 1 (png_band_kernel<SRC, 1>): the same tokens, but the band's workgroup first counts them (pass A), builds a Huffman code
// of at most 15 bits for the literal/length symbols it saw (png_code_lengths; two one-bit distance codes beside it), prices the
// band as a dynamic and as a fixed block and packs the cheaper one (pass B; the dynamic header goes into the bit buffer in front
// of segment 0).  A band that stays fixed is level 0's band bit for bit, so no band outgrows png_band_bound.
#include <algorithm>

#include "pseg_list.h"

namespace pseg {

constexpr int PNG_T = 256;                    // threads of a band workgroup
constexpr int PNG_BPT = 16;                   // filtered bytes per thread and segment
constexpr int PNG_SEG = PNG_T * PNG_BPT;      // 4096
constexpr int PNG_BITW = PNG_SEG * 9 / 32 + 8;   // words of the bit buffer: 31 carried bits + 9 bits per byte + 49 bits of band end
constexpr int PNG_NSYM = 286;                 // literal/length alphabet; the histogram holds two more counters: matches, extra bits
constexpr int PNG_CLWS = 1024;                // words of png_code_lengths' work space (n <= 286)
constexpr int PNG_HDRW = 136;                 // words kept for a dynamic block header: 17 + 19 * 3 + 289 code-length tokens of <= 14 bits
constexpr int PNG_BITW1 = PNG_SEG * 15 / 32 + PNG_HDRW + 8;   // level 1: 15 bits per byte + header or carry + band end
constexpr unsigned ADLER_M = 65521u;
constexpr size_t PNG_MAX_ROW = (size_t)1 << 30;  // filtered bytes of a row / of a band: in-band indices are ints
constexpr size_t PNG_FIXED = 8 + 25 + 14 + 21 + 12;   // signature, IHDR, IDAT(78 01), IDAT(final block + Adler), IEND
constexpr size_t PNG_HEAD = 8 + 25 + 14;

struct PngBandMeta { unsigned bytes, a, b, pad; };    // compressed bytes; Adler partial: sum of bytes, sum of byte * (n - i), both mod 65521

struct PngJob {
    int H, W, C, R, nb, L;                    // L = C * W + 1 filtered bytes per row, nb = ceil(H / R) bands
    size_t slot;                              // bytes between two bands' slots
    uint8_t* slots[4];
    PngBandMeta* meta[4];
    unsigned long long* offs[4];              // final offset of every band's chunk
    uint8_t* out[4];                          // the assembled stream
    unsigned long long* total;                // [pages][4] its size
    int mask_id[4];
    size_t page;                              // bytes between two pages' slots, band tables, offsets and streams (blockIdx.z / blockIdx.y
                                              // selects the page); 0 with one page
    // ragged launches over pages of different shapes (png_pages_enqueue_mixed) alone: H .. slot, the per-output pointers and `page`
    // above are unused, slots[0] is the workspace and a page's geometry and offsets come from its table entry
    const MixedPage* tab;                     // [npages], band0 ascending from 0
    int npages;
    const uint8_t* pred_alt;                  // the label maps of pages with pred_sel = 1
};

// the page of workgroup `b` of a ragged launch: the last entry whose first band is not behind b (uniform: scalar loads)
__device__ __forceinline__ const MixedPage* png_mixed_page(const PngJob& J, int b) {
    int p = 0;
    for (int k = 1; k < J.npages; ++k)
        if (J.tab[k].band0 <= b) p = k;
    return J.tab + p;
}


// ---- host arithmetic ------------------------------------------------------------------------------------------------
static inline size_t png_band_bound(size_t n) { return n + n / 8 + 8; }   // header 3 + 9 n + end-of-block 7 + stored header 3 bits, padded, + 4
static int png_rows(int H, int W, int C, int band_rows, int level) {
    const size_t L = (size_t)W * C + 1;
    size_t r = band_rows > 0 ? (size_t)band_rows : std::max<size_t>(1, (level ? 65536 : 16384) / L);   // level 1: the header amortises
    r = std::min(r, (size_t)H);
    r = std::min(r, std::max<size_t>(1, PNG_MAX_ROW / L));
    return (int)r;
}
static bool png_shape_ok(int H, int W, int C) { return H >= 1 && W >= 1 && (C == 1 || C == 3) && (size_t)W * C + 1 <= PNG_MAX_ROW; }
static size_t png_bound(int H, int W, int C, int band_rows, int level) {
    if (!png_shape_ok(H, W, C) || band_rows < 0 || (level != 0 && level != 1)) return 0;
    const size_t L = (size_t)W * C + 1, R = png_rows(H, W, C, band_rows, level);
    const size_t nfull = (size_t)H / R, rem = (size_t)H % R;
    size_t t = PNG_FIXED + nfull * (12 + png_band_bound(R * L));
    if (rem) t += 12 + png_band_bound(rem * L);
    return t;
}

// ---- fixed Huffman codes (RFC 1951 3.2.6), already bit-reversed for LSB-first packing -----------------------------------
__host__ __device__ __forceinline__ int png_fixed_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
__device__ __forceinline__ void png_fixed(int sym, unsigned& code, int& cb) {
    if (sym < 144) { cb = 8; code = __brev(0x30u + (unsigned)sym) >> 24; }
    else if (sym < 256) { cb = 9; code = __brev(0x190u + (unsigned)(sym - 144)) >> 23; }
    else if (sym < 280) { cb = 7; code = __brev((unsigned)(sym - 256)) >> 25; }
    else { cb = 8; code = __brev(0xC0u + (unsigned)(sym - 280)) >> 24; }
}
// match of `len` (3..258): its length symbol and extra bits (RFC 1951 3.2.5); the distance code follows it
__device__ __forceinline__ void png_match(int len, int& sym, unsigned& extra, int& eb) {
    eb = 0;
    extra = 0;
    if (len == 258) sym = 285;
    else {
        const int l = len - 3;
        if (l < 8) sym = 257 + l;
        else {
            const int n = 31 - __clz(l);
            eb = n - 2;
            sym = 261 + 4 * eb + ((l - (1 << n)) >> eb);
            extra = (unsigned)(l - (1 << n)) & ((1u << eb) - 1);
        }
    }
}
// a token's bits: the symbol's code (bit-reversed, `cb` bits), the extra bits, for a match the band's distance code
__device__ __forceinline__ void png_bits(unsigned c, int cb, unsigned extra, int eb, bool dist, unsigned dcode, int dbits, unsigned& code, int& nb) {
    code = c | (extra << cb);
    nb = cb + eb;
    if (dist) { code |= dcode << nb; nb += dbits; }
}

// ---- code lengths of a length-limited prefix code (level 1; both the literal/length and the code-length alphabet) ----------
// counts[n] -> lengths[n]: 0 for a symbol that does not occur, 1 for a single used symbol, otherwise a complete prefix code
// with no length above `limit` (n <= 286, used symbols <= 2^limit, sum of the counts < 2^32).  Where the Huffman tree fits
// the limit its lengths are returned (an optimal code); where it does not, leaves below the limit are raised to it and the
// Kraft sum is brought back to 1 by moving codes one level down, then the lengths go to the symbols by descending count.
// Two steps so that a workgroup can share the first: png_cl_rank sorts (every symbol counts the symbols in front of it;
// symbols first, first + stride, ...), png_cl_build is serial.  ws: PNG_CLWS words.
__host__ __device__ inline void png_cl_rank(const uint32_t* counts, int n, uint8_t* lengths, uint32_t* ws, int first, int stride) {
    uint16_t* ord = (uint16_t*)(ws + 857);
    for (int s = first; s < n; s += stride) {
        lengths[s] = 0;
        const uint32_t c = counts[s];
        if (!c) continue;
        int r = 0;
        for (int q = 0; q < n; ++q) {
            const uint32_t d = counts[q];
            r += (d != 0 && (d < c || (d == c && q < s))) ? 1 : 0;
        }
        ord[r] = (uint16_t)s;                 // ascending by (count, symbol)
    }
}
__host__ __device__ inline void png_cl_build(const uint32_t* counts, int n, int limit, uint8_t* lengths, uint32_t* ws) {
    uint32_t* wt = ws;                        // [2k-1] node weights, then node depths: leaves in sorted order, then the inner nodes
    uint16_t* par = (uint16_t*)(ws + 571);    // [2k-1] parent of a node
    const uint16_t* ord = (const uint16_t*)(ws + 857);
    uint32_t* num = ws + 1000;                // [limit+1] codes per length
    int k = 0;
    for (int s = 0; s < n; ++s) k += counts[s] != 0 ? 1 : 0;
    if (k == 0) return;
    if (k == 1) { lengths[ord[0]] = 1; return; }
    for (int i = 0; i < k; ++i) wt[i] = counts[ord[i]];
    int i = 0, j = k, next = k;               // two queues: sorted leaves, inner nodes in creation order (ascending too)
    while (next < 2 * k - 1) {
        uint32_t w = 0;
        for (int two = 0; two < 2; ++two) {
            const int pick = (i < k && (j >= next || wt[i] <= wt[j])) ? i++ : j++;
            w += wt[pick];
            par[pick] = (uint16_t)next;
        }
        wt[next++] = w;
    }
    wt[2 * k - 2] = 0;
    for (int v = 2 * k - 3; v >= 0; --v) wt[v] = wt[par[v]] + 1;      // a parent is created behind its children
    for (int l = 0; l <= limit; ++l) num[l] = 0;
    for (int v = 0; v < k; ++v) ++num[wt[v] < (uint32_t)limit ? wt[v] : (uint32_t)limit];
    uint32_t total = 0;                       // Kraft sum in units of 2^-limit: above 2^limit only where leaves were raised
    for (int l = 1; l <= limit; ++l) total += num[l] << (limit - l);
    while (total > (1u << limit)) {
        --num[limit];
        for (int l = limit - 1; l > 0; --l)
            if (num[l]) { --num[l]; num[l + 1] += 2; break; }
        --total;
    }
    int p = 0;
    for (int l = limit; l >= 1; --l)
        for (uint32_t c = 0; c < num[l]; ++c) lengths[ord[p++]] = (uint8_t)l;
}
__host__ __device__ inline void png_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lengths, uint32_t* ws) {
    png_cl_rank(counts, n, lengths, ws, 0, 1);
    png_cl_build(counts, n, limit, lengths, ws);
}

// ---- workgroup scans over one int per thread (four waves of 64) -------------------------------------------------------------
__device__ __forceinline__ int png_scan_max_before(int v, int* sh) {      // max over the threads in front, -1 if none
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(x, d, 64); if (lane >= d) x = max(x, o); }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int ex = __shfl_up(x, 1, 64);
    if (lane == 0) ex = -1;
    for (int k = 0; k < w; ++k) ex = max(ex, sh[k]);
    __syncthreads();
    return ex;
}
__device__ __forceinline__ int png_scan_min_after(int v, int none, int* sh) {   // min over the threads behind, `none` if none
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_down(x, d, 64); if (lane + d < 64) x = min(x, o); }
    if (lane == 0) sh[w] = x;
    __syncthreads();
    int ex = __shfl_down(x, 1, 64);
    if (lane == 63) ex = none;
    for (int k = w + 1; k < PNG_T / 64; ++k) ex = min(ex, sh[k]);
    __syncthreads();
    return ex;
}
__device__ __forceinline__ int png_scan_sum_before(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(x, d, 64); if (lane >= d) x += o; }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int ex = x - v;
    total = 0;
    for (int k = 0; k < PNG_T / 64; ++k) { if (k < w) ex += sh[k]; total += sh[k]; }
    __syncthreads();
    return ex;
}

// ---- pixel sources: one pixel as 0x00BBGGRR (gray: the low byte) ------------------------------------------------------------
struct PngSrcPlain {                          // interleaved 8-bit buffer, 1 or 3 channels
    static constexpr bool LUT = false;
    const uint8_t* p;
    int W, C;
    size_t page = 0;                          // bytes between two pages' images
    __device__ __forceinline__ PngSrcPlain at(unsigned pg) const { PngSrcPlain s = *this; s.p += pg * page; return s; }
    __device__ __forceinline__ uint32_t px(int row, int x, int, const uint32_t*) const {
        const uint8_t* q = p + ((size_t)row * W + x) * C;
        return C == 1 ? (uint32_t)q[0] : ((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16));
    }
};
struct PngSrcMasks {                          // generate_output_masks (lib/output.py:44-60) on the fly: masks_kernel's selection
    static constexpr bool LUT = true;
    const uint8_t* pred;
    const uint8_t* bin;
    const uint8_t* lut;
    int n_lut, W;
    size_t page_pred = 0, page_bin = 0;       // bytes between two pages' label maps / binarisations
    __device__ __forceinline__ PngSrcMasks at(unsigned pg) const { PngSrcMasks s = *this; s.pred += pg * page_pred; s.bin += pg * page_bin; return s; }
    __device__ __forceinline__ PngSrcMasks mixed(const MixedPage& m, const uint8_t* pred_alt) const {
        PngSrcMasks s = *this;
        s.pred = (m.pred_sel ? pred_alt : pred) + m.pred_off;
        s.bin = bin + m.bin_off;
        s.W = m.Wl;
        return s;
    }
    __device__ __forceinline__ uint32_t px(int row, int x, int mask, const uint32_t* slut) const {
        const size_t p = (size_t)row * W + x;
        const uint32_t rgb = slut[pred[p]];
        const unsigned b = bin[p];
        switch (mask) {
            case 0: return rgb;
            case 1: return b == 1 ? 0u : rgb;
            case 2: return b == 0 ? 0u : rgb;
            default: return b != 1 ? 0u : rgb;
        }
    }
};

// The tokens of one thread's 16 bytes: emit(symbol 0..285, extra bits, their count, has a distance) in stream order; the code
// comes from a lookup afterwards.  eqm: bit j set = byte j continues a run; pl: last run break in front of the chunk (segment
// position, -1: none); nf: first break behind it (slen: none).
template <class F>
__device__ __forceinline__ void png_walk(const uint32_t (&w4)[4], int cnt, unsigned eqm, int p0, int pl, int nf, F emit) {
    const unsigned brk = ~eqm & ((1u << cnt) - 1u);
    int last_break = pl;
    for (int j = 0; j < cnt; ++j) {
        const unsigned v = (w4[j >> 2] >> (8 * (j & 3))) & 255u;
        const int p = p0 + j;
        if (!((eqm >> j) & 1u)) {
            last_break = p;
            emit((int)v, 0u, 0, false);
            continue;
        }
        const unsigned behind = j + 1 < 32 ? brk >> (j + 1) : 0u;
        const int e = behind ? p + 1 + (__ffs(behind) - 1) : nf;
        const int s = last_break + 1;
        const int k = p - s, q = k - k % 258;
        const int c = min(258, (e - s) - q);
        if (c < 3) emit((int)v, 0u, 0, false);
        else if (k == q) {
            int sym, eb;
            unsigned extra;
            png_match(c, sym, extra, eb);
            emit(sym, extra, eb, true);
        }
    }
}

// One segment of a band: the filtered bytes of this thread's chunk (w4, also to s_in), their Adler sums, the run flags and the
// two scans over the run breaks.  Ends behind a workgroup barrier; what the caller wrote to LDS in front of it is visible.
template <class SRC>
__device__ __forceinline__ void png_segment(const SRC& src, int mask, int row0, int L, int D, int base, int slen, const uint32_t* s_lut,
                                            uint8_t* s_in, int* s_w, uint32_t (&w4)[4], int& cnt, unsigned& eqm, int& pl, int& nf,
                                            unsigned& a_sum, unsigned& b_sum) {
    const int t = threadIdx.x, p0 = t * PNG_BPT;
    cnt = min(PNG_BPT, max(0, slen - p0));
    w4[0] = w4[1] = w4[2] = w4[3] = 0u;
    a_sum = 0;
    b_sum = 0;
    if (cnt > 0) {
        const int i0 = base + p0;
        int r = i0 / L, c = i0 - r * L;
        int grow = row0 + r, x = 0, ch = 0;
        if (c > 0) { x = (c - 1) / D; ch = (c - 1) - x * D; }
        bool need = true;
        uint32_t cur = 0, up = 0;
        for (int j = 0; j < cnt; ++j) {
            uint32_t v;
            if (c == 0) { v = 2u; x = 0; ch = 0; need = true; }          // filter type: Up
            else {
                if (need) {
                    cur = src.px(grow, x, mask, s_lut);
                    up = grow > 0 ? src.px(grow - 1, x, mask, s_lut) : 0u;
                    need = false;
                }
                v = ((cur >> (8 * ch)) - (up >> (8 * ch))) & 255u;
                if (++ch == D) { ch = 0; ++x; need = true; }
            }
            w4[j >> 2] |= v << (8 * (j & 3));
            a_sum += v;
            b_sum += v * (unsigned)(cnt - j);
            if (++c == L) { c = 0; ++grow; }
        }
    }
    *(uint4*)(s_in + 16 + p0) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    __syncthreads();
    // run flags: byte == the byte D in front of it (none in front of the band or the segment)
    eqm = 0;
    for (int j = 0; j < cnt; ++j) {
        const int p = p0 + j;
        if (base + p >= D && s_in[16 + p] == s_in[16 + p - D]) eqm |= 1u << j;
    }
    const unsigned brk = ~eqm & ((1u << cnt) - 1u);
    const int lb = brk ? p0 + (31 - __clz(brk)) : -1;
    const int fb = brk ? p0 + (__ffs(brk) - 1) : slen;
    pl = png_scan_max_before(lb, s_w);
    nf = png_scan_min_after(fb, slen, s_w);
}

// The dynamic block header of a band (RFC 1951 3.2.7) from the literal/length code lengths: thread 0.  The code-length sequence
// (HLIT literal/length lengths, then the two distance codes) is run-length coded with 17 / 18 for runs of zeros, no 16; its 19
// symbols get a code of at most 7 bits from the same png_code_lengths.  With `bits` the header is also written to the (zeroed)
// bit buffer.  -> its size in bits.  hw: 256 words of LDS behind png_code_lengths' work space.
__device__ inline int png_dyn_header(const uint8_t* s_len, int D, uint32_t* ws, uint32_t* bits) {
    uint32_t* hw = ws + PNG_CLWS;
    uint16_t* tok = (uint16_t*)hw;            // [<= 289] symbol | extra << 5
    uint32_t* cl_cnt = hw + 152;              // [19]
    uint8_t* cl_len = (uint8_t*)(hw + 172);   // [19]
    uint16_t* cl_code = (uint16_t*)(hw + 180);   // [19] bit-reversed
    int hlit = 257;
    for (int s = PNG_NSYM - 1; s >= 257; --s)
        if (s_len[s]) { hlit = s + 1; break; }
    const int hdist = D == 1 ? 2 : 3;         // two distance codes of one bit: 0 and 1, or 0 and 2 (the band's only distance is D)
    const int nseq = hlit + hdist;
    auto seq = [&](int i) -> int { return i < hlit ? (int)s_len[i] : (D == 3 && i - hlit == 1) ? 0 : 1; };
    for (int k = 0; k < 19; ++k) cl_cnt[k] = 0;
    int ntok = 0;
    for (int i = 0; i < nseq;) {
        const int v = seq(i);
        int r = 1;
        if (v == 0) while (r < 138 && i + r < nseq && seq(i + r) == 0) ++r;
        int sym = v, extra = 0;
        if (r >= 11) { sym = 18; extra = r - 11; }
        else if (r >= 3) { sym = 17; extra = r - 3; }
        else r = 1;
        tok[ntok++] = (uint16_t)(sym | (extra << 5));
        ++cl_cnt[sym];
        i += r;
    }
    png_code_lengths(cl_cnt, 19, 7, cl_len, ws);
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 4;
    for (int k = 18; k >= 4; --k)
        if (cl_len[order[k]]) { hclen = k + 1; break; }
    int size = 3 + 5 + 5 + 4 + 3 * hclen;
    for (int k = 0; k < 19; ++k) size += (int)cl_cnt[k] * ((int)cl_len[k] + (k == 17 ? 3 : k == 18 ? 7 : 0));
    if (!bits) return size;
    unsigned code = 0;                        // canonical codes (RFC 1951 3.2.2), shortest first, symbols ascending
    for (int l = 1; l <= 7; ++l) {
        for (int k = 0; k < 19; ++k)
            if (cl_len[k] == l) cl_code[k] = (uint16_t)(__brev(code++) >> (32 - l));
        code <<= 1;
    }
    int pos = 0;
    auto put = [&](unsigned v, int nb) {
        const unsigned long long x = (unsigned long long)v << (pos & 31);
        bits[pos >> 5] |= (uint32_t)x;
        if (x >> 32) bits[(pos >> 5) + 1] |= (uint32_t)(x >> 32);
        pos += nb;
    };
    put(4u, 3);                               // BFINAL = 0, BTYPE = 10 (dynamic Huffman), LSB first
    put((unsigned)(hlit - 257), 5);
    put((unsigned)(hdist - 1), 5);
    put((unsigned)(hclen - 4), 4);
    for (int k = 0; k < hclen; ++k) put(cl_len[order[k]], 3);
    for (int k = 0; k < ntok; ++k) {
        const int sym = tok[k] & 31, extra = tok[k] >> 5;
        put(cl_code[sym], cl_len[sym]);
        if (sym == 17) put((unsigned)extra, 3);
        else if (sym == 18) put((unsigned)extra, 7);
    }
    return pos;
}

// LV 0: one fixed-Huffman block per band.  LV 1: two passes over the band's tokens -- A counts the symbols, the workgroup builds
// a code for them and prices the band both ways, B packs with the cheaper of the two (a tie goes to the fixed code: the band is
// then LV 0's band bit for bit).
// PAGES 1: blockIdx.z selects one of several images of one shape (J.page, the source's page strides); PAGES 0: the kernel is the
// single-image kernel, instruction for instruction.  PAGES 2: blockIdx.x runs over the flattened (page, band) pairs of images of
// different shapes; the workgroup finds its page in J.tab and takes every bound and offset from that entry.
template <class SRC, int PAGES>
__device__ __forceinline__ SRC png_src_of(const SRC& s, const PngJob& J, const MixedPage* mp) {
    if constexpr (PAGES == 2) return s.mixed(*mp, J.pred_alt);
    else if constexpr (PAGES == 1) return s.at(blockIdx.z);
    else return s;
}
template <class SRC, int LV, int PAGES = 0>
__global__ __launch_bounds__(PNG_T) void png_band_kernel(SRC src0, PngJob J) {
    const MixedPage* const mp = PAGES == 2 ? png_mixed_page(J, (int)blockIdx.x) : nullptr;
    const SRC src = png_src_of<SRC, PAGES>(src0, J, mp);
    const size_t pg = PAGES == 1 ? (size_t)blockIdx.z * J.page : 0;
    __shared__ __attribute__((aligned(16))) uint8_t s_in[16 + PNG_SEG];   // [13..15]: the three bytes in front of the segment
    __shared__ uint32_t s_bits[LV ? PNG_BITW1 : PNG_BITW];
    __shared__ int s_w[4];
    __shared__ unsigned s_ad[2];
    __shared__ uint32_t s_lut[256];
    __shared__ uint32_t s_hist[LV ? PNG_NSYM + 2 : 1];        // [286]: matches, [287]: extra bits
    __shared__ uint32_t s_code[LV ? PNG_NSYM : 1];            // code (bit-reversed) | length << 16
    __shared__ uint8_t s_len[LV ? PNG_NSYM + 2 : 1];
    __shared__ uint32_t s_ws[LV ? PNG_CLWS + 256 : 1];
    __shared__ unsigned long long s_cost[2];                  // literal/length bits of the band: dynamic, fixed
    __shared__ int s_hdr[18];                                 // [0]: the dynamic header's bits; [1..15]: first code of a length; [17]: the written header's bits
    const int t = threadIdx.x, band = PAGES == 2 ? (int)blockIdx.x - mp->band0 : (int)blockIdx.x, o = blockIdx.y, mask = J.mask_id[o];
    const int jR = PAGES == 2 ? mp->R : J.R, jH = PAGES == 2 ? mp->Hl : J.H;
    if constexpr (SRC::LUT) {
        s_lut[t] = t < src.n_lut ? (uint32_t)src.lut[t * 3] | ((uint32_t)src.lut[t * 3 + 1] << 8) | ((uint32_t)src.lut[t * 3 + 2] << 16) : 0u;
    }
    if constexpr (LV != 0) {
        for (int k = t; k < PNG_NSYM + 2; k += PNG_T) s_hist[k] = 0u;
        if (t < 2) s_cost[t] = 0ull;
    }
    __syncthreads();
    const int row0 = band * jR, rows = min(jR, jH - row0);
    const int L = PAGES == 2 ? mp->L : J.L, D = J.C;
    const int n = rows * L;                                   // <= 2^30 (png_rows)
    uint32_t* const out = PAGES == 2 ? (uint32_t*)(J.slots[0] + mp->ws_off + (size_t)o * mp->per + (size_t)band * mp->slot)
                                     : (uint32_t*)(J.slots[o] + pg + (size_t)band * J.slot);
    unsigned out_w = 0;                                       // words of the slot written so far
    uint32_t carry_word = 2u;                                 // block header: BFINAL = 0, BTYPE = 01 (fixed Huffman), LSB first
    int carry_bits = 3;                                       // LV 1, first segment: the header's whole words and its partial word
    unsigned dcode = D == 1 ? 0u : 8u;                        // fixed: distance code 0 (00000) / 2 (00010 -> reversed 01000)
    int dbits = 5;
    unsigned adA = 0, adB = 0;
    const int nseg = (n + PNG_SEG - 1) / PNG_SEG;
    uint32_t w4[4];
    int cnt, pl, nf;
    unsigned eqm, a_sum, b_sum;
    const int p0 = t * PNG_BPT;
    if constexpr (LV != 0) {
        // pass A: the band's histogram
        unsigned n_match = 0, n_extra = 0;
        for (int sg = 0; sg < nseg; ++sg) {
            const int base = sg * PNG_SEG, slen = min(PNG_SEG, n - base);
            png_segment(src, mask, row0, L, D, base, slen, s_lut, s_in, s_w, w4, cnt, eqm, pl, nf, a_sum, b_sum);
            int hs = 0;
            unsigned hc = 0;                                  // equal symbols in a row go to the histogram as one add
            png_walk(w4, cnt, eqm, p0, pl, nf, [&](int sym, unsigned, int eb, bool dist) {
                if (sym != hs && hc) { atomicAdd(&s_hist[hs], hc); hc = 0; }
                hs = sym;
                ++hc;
                n_extra += (unsigned)eb;
                n_match += dist ? 1u : 0u;
            });
            if (hc) atomicAdd(&s_hist[hs], hc);
            if (sg + 1 < nseg && t < 3) {
                const uint8_t v = s_in[16 + PNG_SEG - 3 + t];
                s_in[13 + t] = v;
            }
            __syncthreads();
        }
        if (n_match) atomicAdd(&s_hist[PNG_NSYM], n_match);
        if (n_extra) atomicAdd(&s_hist[PNG_NSYM + 1], n_extra);
        if (t == 0) atomicAdd(&s_hist[256], 1u);              // end of block
        for (int k = t; k < PNG_BITW1; k += PNG_T) s_bits[k] = 0u;
        __syncthreads();
        // the literal/length code, the header's size, the band's size both ways
        png_cl_rank(s_hist, PNG_NSYM, s_len, s_ws, t, PNG_T);
        __syncthreads();
        if (t == 0) {
            png_cl_build(s_hist, PNG_NSYM, 15, s_len, s_ws);
            unsigned code = 0;                                // first canonical code of every length (RFC 1951 3.2.2)
            for (int l = 1; l <= 15; ++l) {
                s_hdr[l] = (int)code;
                unsigned c = 0;
                for (int s = 0; s < PNG_NSYM; ++s) c += s_len[s] == l ? 1u : 0u;
                code = (code + c) << 1;
            }
            s_hdr[0] = png_dyn_header(s_len, D, s_ws, nullptr);
        }
        __syncthreads();
        {
            unsigned long long dyn = 0, fix = 0;
            for (int s = t; s < PNG_NSYM; s += PNG_T) {
                const unsigned long long h = s_hist[s];
                dyn += h * s_len[s];
                fix += h * (unsigned)png_fixed_len(s);
            }
            if (dyn) atomicAdd(&s_cost[0], dyn);
            if (fix) atomicAdd(&s_cost[1], fix);
        }
        __syncthreads();
        const unsigned long long matches = s_hist[PNG_NSYM];  // (the extra bits cost the same both ways)
        const bool dynamic = (unsigned long long)s_hdr[0] + s_cost[0] + matches < 3ull + s_cost[1] + 5ull * matches;
        for (int s = t; s < PNG_NSYM; s += PNG_T) {
            unsigned code = 0;
            int cb = 0;
            if (dynamic) {
                cb = s_len[s];
                if (cb) {
                    unsigned r = 0;                           // symbols of this length in front of s
                    for (int q = 0; q < s; ++q) r += s_len[q] == cb ? 1u : 0u;
                    code = __brev((unsigned)s_hdr[cb] + r) >> (32 - cb);
                }
            } else png_fixed(s, code, cb);
            s_code[s] = code | ((unsigned)cb << 16);
        }
        if (dynamic) {
            dcode = D == 1 ? 0u : 1u;                         // distance code 0 is "0"; D = 3: code 2 is "1"
            dbits = 1;
            if (t == 0) s_hdr[17] = png_dyn_header(s_len, D, s_ws, s_bits);
            __syncthreads();
            carry_bits = s_hdr[17];
        } else {
            if (t == 0) s_bits[0] = carry_word;
            __syncthreads();
        }
    }
    // LV 0: the only pass; LV 1: pass B
    for (int sg = 0; sg < nseg; ++sg) {
        const int base = sg * PNG_SEG, slen = min(PNG_SEG, n - base);
        const bool last = sg == nseg - 1;
        // 1. the filtered bytes of this thread's chunk; the bit buffer starts as the carried partial word
        if (LV == 0 || sg > 0)
            for (int k = t; k < (LV ? PNG_BITW1 : PNG_BITW); k += PNG_T) s_bits[k] = k == 0 ? carry_word : 0u;
        if (t == 0) { s_ad[0] = 0; s_ad[1] = 0; }
        png_segment(src, mask, row0, L, D, base, slen, s_lut, s_in, s_w, w4, cnt, eqm, pl, nf, a_sum, b_sum);
        // 2. Adler partial of the segment
        if (cnt > 0) {
            const unsigned after = (unsigned)(slen - (p0 + cnt));
            atomicAdd(&s_ad[0], a_sum);
            atomicAdd(&s_ad[1], (b_sum + a_sum * after) % ADLER_M);
        }
        auto lookup = [&](int sym, unsigned extra, int eb, bool dist, unsigned& code, int& nb) {
            unsigned c;
            int cb;
            if constexpr (LV == 0) png_fixed(sym, c, cb);
            else { const uint32_t e = s_code[sym]; c = e & 0xFFFFu; cb = (int)(e >> 16); }
            png_bits(c, cb, extra, eb, dist, dcode, dbits, code, nb);
        };
        // 3. bit lengths -> bit offsets
        int bits = 0;
        png_walk(w4, cnt, eqm, p0, pl, nf, [&](int sym, unsigned extra, int eb, bool dist) {
            unsigned code;
            int nb;
            lookup(sym, extra, eb, dist, code, nb);
            bits += nb;
        });
        int seg_bits = 0;
        int off = carry_bits + png_scan_sum_before(bits, s_w, seg_bits);
        // 4. pack
        png_walk(w4, cnt, eqm, p0, pl, nf, [&](int sym, unsigned extra, int eb, bool dist) {
            unsigned code;
            int nb;
            lookup(sym, extra, eb, dist, code, nb);
            const unsigned long long v = (unsigned long long)code << (off & 31);
            atomicOr(&s_bits[off >> 5], (uint32_t)v);
            if (v >> 32) atomicOr(&s_bits[(off >> 5) + 1], (uint32_t)(v >> 32));
            off += nb;
        });
        int T = carry_bits + seg_bits;
        if (last) {
            if constexpr (LV == 0) T += 7;    // end-of-block (0000000)
            else {
                const uint32_t e = s_code[256];
                if (t == 0) {
                    const unsigned long long v = (unsigned long long)(e & 0xFFFFu) << (T & 31);
                    atomicOr(&s_bits[T >> 5], (uint32_t)v);
                    if (v >> 32) atomicOr(&s_bits[(T >> 5) + 1], (uint32_t)(v >> 32));
                }
                T += (int)(e >> 16);
            }
            T += 3;                           // ... then an empty stored block: BFINAL = 0, BTYPE = 00
            T = (T + 7) & ~7;                 // ... padded to a byte, LEN = 0000, NLEN = FFFF
            if (t == 0) {
                const int f = T + 16;
                const unsigned long long v = 0xFFFFull << (f & 31);
                atomicOr(&s_bits[f >> 5], (uint32_t)v);
                if (v >> 32) atomicOr(&s_bits[(f >> 5) + 1], (uint32_t)(v >> 32));
            }
            T += 32;
        }
        __syncthreads();
        // 5. whole words to the slot; the partial word and the Adler sums are carried
        const int nW = last ? (T + 31) >> 5 : T >> 5;
        for (int k = t; k < nW; k += PNG_T) out[out_w + k] = s_bits[k];
        carry_word = s_bits[T >> 5];
        carry_bits = T & 31;
        {
            const unsigned A2 = s_ad[0] % ADLER_M, B2 = s_ad[1] % ADLER_M;
            adB = (adB + (unsigned)slen * adA + B2) % ADLER_M;      // 4096 * 65520 + 2 * 65520 < 2^32
            adA = (adA + A2) % ADLER_M;
        }
        if (last) {
            if (t == 0) {
                PngBandMeta m;
                m.bytes = out_w * 4u + (unsigned)(T >> 3);
                m.a = adA; m.b = adB; m.pad = 0;
                if constexpr (PAGES == 2) ((PngBandMeta*)(J.slots[0] + mp->ws_off + (size_t)o * mp->per + mp->slots_b))[band] = m;
                else ((PngBandMeta*)((uint8_t*)J.meta[o] + pg))[band] = m;
            }
        } else {
            out_w += (unsigned)nW;
            if (t < 3) {
                const uint8_t v = s_in[16 + PNG_SEG - 3 + t];
                s_in[13 + t] = v;
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void png_be32(uint8_t* p, uint32_t v) { p[0] = v >> 24; p[1] = v >> 16; p[2] = v >> 8; p[3] = v; }

// One workgroup per output: band sizes -> final offsets; Adler-32 of the whole filtered image; everything but the IDAT bands.
// (the geometry and the output's band table, offsets, stream and size word are arguments: the same body frames a page of a ragged launch)
struct PngFrameGeo { int H, W, C, R, L, nb; };
__device__ __forceinline__ void png_frame_body(const PngFrameGeo J, const PngBandMeta* meta, unsigned long long* const offs, uint8_t* const stream,
                                               unsigned long long* const total) {
    __shared__ unsigned long long s_tot[PNG_T];
    __shared__ unsigned long long s_a, s_b;
    const int t = threadIdx.x;
    const int per = (J.nb + PNG_T - 1) / PNG_T;
    const int b0 = min(J.nb, t * per), b1 = min(J.nb, b0 + per);
    if (t == 0) { s_a = 0; s_b = 0; }
    unsigned long long sum = 0;
    for (int b = b0; b < b1; ++b) sum += (unsigned long long)meta[b].bytes + 12u;
    s_tot[t] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long run = PNG_HEAD;
        for (int k = 0; k < PNG_T; ++k) { const unsigned long long v = s_tot[k]; s_tot[k] = run; run += v; }
    }
    __syncthreads();
    const unsigned long long ntotal = (unsigned long long)J.H * (unsigned long long)J.L;
    unsigned long long off = s_tot[t], a = 0, bsum = 0;
    for (int b = b0; b < b1; ++b) {
        offs[b] = off;
        off += (unsigned long long)meta[b].bytes + 12u;
        const unsigned long long end = (unsigned long long)min((long long)(b + 1) * J.R, (long long)J.H) * (unsigned long long)J.L;
        const unsigned long long after = (ntotal - end) % ADLER_M;           // the "length mod 65521" of the combine
        a += meta[b].a;
        bsum += ((unsigned long long)meta[b].b + (unsigned long long)meta[b].a * after) % ADLER_M;
    }
    atomicAdd(&s_a, a);
    atomicAdd(&s_b, bsum);
    __syncthreads();
    if (t == PNG_T - 1) {
        const unsigned long long end = off;                   // behind the last band's chunk (the threads behind the last band hold it too)
        const uint32_t s1 = (uint32_t)((1u + s_a % ADLER_M) % ADLER_M);
        const uint32_t s2 = (uint32_t)((ntotal % ADLER_M + s_b % ADLER_M) % ADLER_M);
        uint8_t* p = stream;
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
        for (int k = 0; k < 8; ++k) p[k] = sig[k];
        png_be32(p + 8, 13);
        p[12] = 'I'; p[13] = 'H'; p[14] = 'D'; p[15] = 'R';
        png_be32(p + 16, (uint32_t)J.W);
        png_be32(p + 20, (uint32_t)J.H);
        p[24] = 8; p[25] = J.C == 3 ? 2 : 0; p[26] = 0; p[27] = 0; p[28] = 0;
        png_be32(p + 29, 0);                                  // CRCs: the host fills them in
        png_be32(p + 33, 2);
        p[37] = 'I'; p[38] = 'D'; p[39] = 'A'; p[40] = 'T';
        p[41] = 0x78; p[42] = 0x01;                           // zlib header: deflate, 32 KiB window, fastest
        png_be32(p + 43, 0);
        uint8_t* q = p + end;
        png_be32(q, 9);
        q[4] = 'I'; q[5] = 'D'; q[6] = 'A'; q[7] = 'T';
        q[8] = 0x01; q[9] = 0; q[10] = 0; q[11] = 0xFF; q[12] = 0xFF;     // final empty stored block
        png_be32(q + 13, (s2 << 16) | s1);
        png_be32(q + 17, 0);
        png_be32(q + 21, 0);
        q[25] = 'I'; q[26] = 'E'; q[27] = 'N'; q[28] = 'D';
        png_be32(q + 29, 0);
        *total = end + 21 + 12;
    }
}
__global__ __launch_bounds__(PNG_T) void png_frame_kernel(PngJob J) {
    const int o = blockIdx.x;
    const size_t pg = (size_t)blockIdx.y * J.page;
    png_frame_body(PngFrameGeo{J.H, J.W, J.C, J.R, J.L, J.nb}, (const PngBandMeta*)((const uint8_t*)J.meta[o] + pg),
                   (unsigned long long*)((uint8_t*)J.offs[o] + pg), J.out[o] + pg, J.total + (size_t)blockIdx.y * 4 + o);
}
// ragged: blockIdx.y is the page of the unit, its geometry and workspace from the table
__global__ __launch_bounds__(PNG_T) void png_frame_mixed_kernel(PngJob J) {
    const int o = blockIdx.x;
    const MixedPage& m = J.tab[blockIdx.y];
    uint8_t* const q = J.slots[0] + m.ws_off + (size_t)o * m.per;
    png_frame_body(PngFrameGeo{m.Hl, m.Wl, J.C, m.R, m.L, m.nb}, (const PngBandMeta*)(q + m.slots_b), (unsigned long long*)(q + m.slots_b + m.meta_b),
                   q + m.slots_b + m.meta_b + m.offs_b, J.total + (size_t)blockIdx.y * 4 + o);
}

__device__ __forceinline__ void png_gather_body(const PngBandMeta* meta, const uint8_t* slots, size_t slot, const unsigned long long* offs,
                                                uint8_t* stream, int band) {
    const int t = threadIdx.x;
    const unsigned sz = meta[band].bytes;
    const uint8_t* src = slots + (size_t)band * slot;
    uint8_t* dst = stream + offs[band];
    if (t == 0) { png_be32(dst, sz); dst[4] = 'I'; dst[5] = 'D'; dst[6] = 'A'; dst[7] = 'T'; png_be32(dst + 8 + sz, 0); }
    for (unsigned k = t; k < sz; k += PNG_T) dst[8 + k] = src[k];
}
__global__ __launch_bounds__(PNG_T) void png_gather_kernel(PngJob J) {
    const int o = blockIdx.y;
    const size_t pg = (size_t)blockIdx.z * J.page;
    png_gather_body((const PngBandMeta*)((const uint8_t*)J.meta[o] + pg), J.slots[o] + pg, J.slot,
                    (const unsigned long long*)((const uint8_t*)J.offs[o] + pg), J.out[o] + pg, (int)blockIdx.x);
}
__global__ __launch_bounds__(PNG_T) void png_gather_mixed_kernel(PngJob J) {
    const int o = blockIdx.y;
    const MixedPage* const mp = png_mixed_page(J, (int)blockIdx.x);
    uint8_t* const q = J.slots[0] + mp->ws_off + (size_t)o * mp->per;
    png_gather_body((const PngBandMeta*)(q + mp->slots_b), q, mp->slot, (const unsigned long long*)(q + mp->slots_b + mp->meta_b),
                    q + mp->slots_b + mp->meta_b + mp->offs_b, (int)blockIdx.x - mp->band0);
}

// ---- CRC-32 (host, over the downloaded stream) ------------------------------------------------------------------------------
static uint32_t g_crc_tab[8][256];
static std::once_flag g_crc_once;
static void crc_init() {
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        g_crc_tab[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
        for (int s = 1; s < 8; ++s) g_crc_tab[s][i] = (g_crc_tab[s - 1][i] >> 8) ^ g_crc_tab[0][g_crc_tab[s - 1][i] & 255];
}
static uint32_t crc32_of(const uint8_t* p, size_t n) {
    std::call_once(g_crc_once, crc_init);
    uint32_t c = 0xFFFFFFFFu;
    while (n >= 8) {
        const uint32_t lo = ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)) ^ c;
        c = g_crc_tab[7][lo & 255] ^ g_crc_tab[6][(lo >> 8) & 255] ^ g_crc_tab[5][(lo >> 16) & 255] ^ g_crc_tab[4][lo >> 24] ^
            g_crc_tab[3][p[4]] ^ g_crc_tab[2][p[5]] ^ g_crc_tab[1][p[6]] ^ g_crc_tab[0][p[7]];
        p += 8;
        n -= 8;
    }
    while (n--) c = g_crc_tab[0][(c ^ *p++) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
static int png_fill_crcs(uint8_t* png, size_t total) {
    size_t pos = 8;
    while (pos < total) {
        if (pos + 12 > total) return fail(PSEG_EHIP, "png: chunk framing runs past the stream");
        const size_t len = ((size_t)png[pos] << 24) | ((size_t)png[pos + 1] << 16) | ((size_t)png[pos + 2] << 8) | png[pos + 3];
        if (pos + 12 + len > total) return fail(PSEG_EHIP, "png: chunk framing runs past the stream");
        const uint32_t c = crc32_of(png + pos + 4, 4 + len);
        uint8_t* q = png + pos + 8 + len;
        q[0] = c >> 24; q[1] = c >> 16; q[2] = c >> 8; q[3] = c;
        pos += 12 + len;
    }
    return PSEG_OK;
}

// ---- workspace: grow-only, one per device (band slots, band tables, the assembled streams); a call holds the device's lock to
// its end and ends synchronised, so one call at a time uses it.  pseg_release_workspace frees it. -------------------------------
struct PngWs {
    GrowDev dev;
    void release() { dev.release(); }
};
static PerDevice<PngWs> g_png;

// Encodes `nout` images of one shape from `src` (output k = mask mask_id[k]) into host[k]; synchronises `st`.
template <class SRC>
static int png_run(int device, const SRC& src, int H, int W, int C, int band_rows, int level, int nout, uint8_t* const host[4],
                   size_t* const nbytes[4], const int mask_id[4], hipStream_t st) {
    const size_t bound = png_bound(H, W, C, band_rows, level);
    PngJob J;
    J.H = H; J.W = W; J.C = C; J.R = png_rows(H, W, C, band_rows, level);
    J.nb = (int)(((size_t)H + J.R - 1) / J.R);
    J.L = W * C + 1;
    J.slot = (png_band_bound((size_t)J.R * J.L) + 3) & ~(size_t)3;
    J.page = 0;
    J.tab = nullptr; J.npages = 0; J.pred_alt = nullptr;
    Bump blk;                                                          // one output's block: band slots, band table, offsets, stream
    const size_t o_slots = blk.take((size_t)J.nb * J.slot), o_meta = blk.take((size_t)J.nb * sizeof(PngBandMeta)),
                 o_offs = blk.take((size_t)J.nb * 8), o_out = blk.take(bound + 32);
    const size_t per = blk.off, need = 256 + (size_t)nout * per;
    std::lock_guard<std::mutex> lk(g_png.mu[device]);
    GrowDev& w = g_png.ws[device].dev;
    PSEG_TRY(w.ensure(need, "png workspace"));
    uint8_t* base = w.p;
    J.total = (unsigned long long*)base;
    for (int k = 0; k < 4; ++k) {
        uint8_t* q = base + 256 + (size_t)std::min(k, nout - 1) * per;
        J.slots[k] = q + o_slots;
        J.meta[k] = (PngBandMeta*)(q + o_meta);
        J.offs[k] = (unsigned long long*)(q + o_offs);
        J.out[k] = q + o_out;
        J.mask_id[k] = mask_id[std::min(k, nout - 1)];
    }
    if (level == 0) png_band_kernel<SRC, 0><<<dim3(J.nb, nout), PNG_T, 0, st>>>(src, J);
    else png_band_kernel<SRC, 1><<<dim3(J.nb, nout), PNG_T, 0, st>>>(src, J);
    png_frame_kernel<<<nout, PNG_T, 0, st>>>(J);
    png_gather_kernel<<<dim3(J.nb, nout), PNG_T, 0, st>>>(J);
    PSEG_HIP(hipGetLastError());
    unsigned long long total[4] = {0, 0, 0, 0};
    PSEG_HIP(hipMemcpyAsync(total, J.total, sizeof(total), hipMemcpyDeviceToHost, st));
    PSEG_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < nout; ++k)
        if (total[k] < PNG_FIXED || total[k] > bound) return fail(PSEG_EHIP, "png: encoded size %llu outside (0, bound %zu]", total[k], bound);
    for (int k = 0; k < nout; ++k) PSEG_HIP(hipMemcpyAsync(host[k], J.out[k], (size_t)total[k], hipMemcpyDeviceToHost, st));
    PSEG_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < nout; ++k) {
        PSEG_TRY(png_fill_crcs(host[k], (size_t)total[k]));
        *nbytes[k] = (size_t)total[k];
    }
    return PSEG_OK;
}

// ---- many images of one shape in one set of launches, asynchronously (the page chain, pseg_chain.hip) ------------------------------
// The workspace is the caller's: [pages][4] sizes, then per page `nout` blocks of {band slots, band table, offsets, stream}.  Nothing
// here waits, locks or allocates.
int png_pages_layout(int H, int W, int level, int nout, int pages, PngPages* L) {
    if (!png_shape_ok(H, W, 3) || (level != 0 && level != 1) || nout < 1 || nout > 4 || pages < 1 || pages > 65535)
        return fail(PSEG_EINVAL, "png: %d pages of %d x %d pixels, %d outputs, level %d", pages, H, W, nout, level);
    const int R = png_rows(H, W, 3, 0, level), nb = (int)(((size_t)H + R - 1) / R);
    const size_t Lb = (size_t)W * 3 + 1, slot = (png_band_bound((size_t)R * Lb) + 3) & ~(size_t)3;
    L->bound = png_bound(H, W, 3, 0, level);
    L->slots_b = up256((size_t)nb * slot);
    L->meta_b = up256((size_t)nb * sizeof(PngBandMeta));
    L->offs_b = up256((size_t)nb * 8);
    L->per = L->slots_b + L->meta_b + L->offs_b + up256(L->bound + 32);
    L->page = (size_t)nout * L->per;
    L->head = up256((size_t)pages * 4 * sizeof(unsigned long long));
    L->bytes = L->head + (size_t)pages * L->page;
    return PSEG_OK;
}

int png_pages_enqueue(const PngPages& L, uint8_t* d_ws, const uint8_t* d_pred, size_t page_pred, const uint8_t* d_bin, size_t page_bin,
                      const uint8_t* d_lut, int n_lut, int H, int W, int level, int nout, const int mask_id[4], int pages, hipStream_t st) {
    PngJob J;
    J.H = H; J.W = W; J.C = 3; J.R = png_rows(H, W, 3, 0, level);
    J.nb = (int)(((size_t)H + J.R - 1) / J.R);
    J.L = W * 3 + 1;
    J.slot = (png_band_bound((size_t)J.R * J.L) + 3) & ~(size_t)3;
    J.page = pages > 1 ? L.page : 0;
    J.tab = nullptr; J.npages = 0; J.pred_alt = nullptr;
    J.total = (unsigned long long*)d_ws;
    for (int k = 0; k < 4; ++k) {
        uint8_t* q = d_ws + L.head + (size_t)std::min(k, nout - 1) * L.per;
        J.slots[k] = q;
        J.meta[k] = (PngBandMeta*)(q + L.slots_b);
        J.offs[k] = (unsigned long long*)(q + L.slots_b + L.meta_b);
        J.out[k] = q + L.slots_b + L.meta_b + L.offs_b;
        J.mask_id[k] = mask_id[std::min(k, nout - 1)];
    }
    PngSrcMasks src{d_pred, d_bin, d_lut, n_lut, W, pages > 1 ? page_pred : 0, pages > 1 ? page_bin : 0};
    if (pages == 1) {
        if (level == 0) png_band_kernel<PngSrcMasks, 0><<<dim3(J.nb, nout), PNG_T, 0, st>>>(src, J);
        else png_band_kernel<PngSrcMasks, 1><<<dim3(J.nb, nout), PNG_T, 0, st>>>(src, J);
    } else {
        if (level == 0) png_band_kernel<PngSrcMasks, 0, 1><<<dim3(J.nb, nout, pages), PNG_T, 0, st>>>(src, J);
        else png_band_kernel<PngSrcMasks, 1, 1><<<dim3(J.nb, nout, pages), PNG_T, 0, st>>>(src, J);
    }
    png_frame_kernel<<<dim3(nout, pages), PNG_T, 0, st>>>(J);
    png_gather_kernel<<<dim3(J.nb, nout, pages), PNG_T, 0, st>>>(J);
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

// ---- many images of different shapes in one set of launches (the page chain's mixed units) ----------------------------------------
int png_pages_layout_mixed(int level, int nout, int pages, MixedPage* tab, PngPagesMixed* L) {
    if (!tab || !L || (level != 0 && level != 1) || nout < 1 || nout > 4 || pages < 1 || pages > PNG_MIXED_MAX)
        return fail(PSEG_EINVAL, "png: a ragged launch of %d pages (1..%d), %d outputs, level %d", pages, PNG_MIXED_MAX, nout, level);
    L->head = up256((size_t)pages * 4 * sizeof(unsigned long long));
    size_t pos = L->head;
    long long bands = 0;
    for (int p = 0; p < pages; ++p) {
        MixedPage& m = tab[p];
        if (!png_shape_ok(m.Hl, m.Wl, 3)) return fail(PSEG_EINVAL, "png: page %d of the unit: %d x %d pixels", p, m.Hl, m.Wl);
        m.R = png_rows(m.Hl, m.Wl, 3, 0, level);
        m.nb = (int)(((size_t)m.Hl + m.R - 1) / m.R);
        m.L = m.Wl * 3 + 1;
        m.slot = (png_band_bound((size_t)m.R * m.L) + 3) & ~(size_t)3;
        m.bound = png_bound(m.Hl, m.Wl, 3, 0, level);
        m.slots_b = up256((size_t)m.nb * m.slot);
        m.meta_b = up256((size_t)m.nb * sizeof(PngBandMeta));
        m.offs_b = up256((size_t)m.nb * 8);
        m.per = m.slots_b + m.meta_b + m.offs_b + up256(m.bound + 32);
        m.ws_off = pos;
        m.band0 = (int)bands;
        m.pad = 0;
        pos += (size_t)nout * m.per;
        bands += m.nb;
        if (bands > 0x7FFFFFFF) return fail(PSEG_EINVAL, "png: more than 2^31 bands in one ragged launch");
    }
    L->bytes = pos;
    L->bands = (int)bands;
    return PSEG_OK;
}

int png_pages_enqueue_mixed(const PngPagesMixed& L, const MixedPage* h_tab, const MixedPage* d_tab, int pages, uint8_t* d_ws, size_t ws_bytes,
                            const uint8_t* d_pred0, const uint8_t* d_pred1, const uint8_t* d_bin, const uint8_t* d_lut, int n_lut, int level,
                            int nout, const int mask_id[4], hipStream_t st) {
    // the kernels take every loop bound and every offset from the table: it is checked against the workspace before anything runs
    if (!h_tab || !d_tab || !d_ws || pages < 1 || pages > PNG_MIXED_MAX || nout < 1 || nout > 4 || (level != 0 && level != 1) || L.bytes > ws_bytes)
        return fail(PSEG_EINVAL, "png: bad ragged launch (%d pages, %d outputs, workspace %zu of %zu bytes)", pages, nout, ws_bytes, L.bytes);
    long long bands = 0;
    size_t pos = L.head;
    for (int p = 0; p < pages; ++p) {
        const MixedPage& m = h_tab[p];
        bool ok = png_shape_ok(m.Hl, m.Wl, 3) && m.R == png_rows(m.Hl, m.Wl, 3, 0, level) && m.R >= 1 && m.L == m.Wl * 3 + 1 &&
                  m.nb == (int)(((size_t)m.Hl + m.R - 1) / m.R) && m.band0 == bands && m.ws_off == pos && m.ws_off % 256 == 0 &&
                  m.slot >= png_band_bound((size_t)m.R * m.L) && m.slot % 4 == 0 && m.slots_b >= (size_t)m.nb * m.slot && m.slots_b % 256 == 0 &&
                  m.meta_b >= (size_t)m.nb * sizeof(PngBandMeta) && m.meta_b % 256 == 0 && m.offs_b >= (size_t)m.nb * 8 && m.offs_b % 256 == 0 &&
                  m.bound == png_bound(m.Hl, m.Wl, 3, 0, level) && m.per >= m.slots_b + m.meta_b + m.offs_b + m.bound + 32 &&
                  (m.pred_sel == 0 || (m.pred_sel == 1 && d_pred1));
        if (!ok) return fail(PSEG_EINVAL, "png: ragged launch: the table entry of page %d does not fit its shape %d x %d", p, m.Hl, m.Wl);
        pos += (size_t)nout * m.per;
        bands += m.nb;
    }
    if (pos != L.bytes || bands != L.bands || bands < 1) return fail(PSEG_EINVAL, "png: ragged launch: the table does not fit the layout");
    PngJob J;
    J.H = J.W = J.R = J.nb = J.L = 0;
    J.C = 3;
    J.slot = 0;
    J.page = 0;
    J.total = (unsigned long long*)d_ws;
    for (int k = 0; k < 4; ++k) {
        J.slots[k] = d_ws;
        J.meta[k] = nullptr; J.offs[k] = nullptr; J.out[k] = nullptr;
        J.mask_id[k] = mask_id[std::min(k, nout - 1)];
    }
    J.tab = d_tab;
    J.npages = pages;
    J.pred_alt = d_pred1;
    PngSrcMasks src{d_pred0, d_bin, d_lut, n_lut, 0, 0, 0};
    if (level == 0) png_band_kernel<PngSrcMasks, 0, 2><<<dim3(L.bands, nout), PNG_T, 0, st>>>(src, J);
    else png_band_kernel<PngSrcMasks, 1, 2><<<dim3(L.bands, nout), PNG_T, 0, st>>>(src, J);
    png_frame_mixed_kernel<<<dim3(nout, pages), PNG_T, 0, st>>>(J);
    png_gather_mixed_kernel<<<dim3(L.bands, nout), PNG_T, 0, st>>>(J);
    PSEG_HIP(hipGetLastError());
    return PSEG_OK;
}

int png_finish_host(uint8_t* png, size_t total) { return png_fill_crcs(png, total); }

static int png_check(int H, int W, int channels, int band_rows, int level) {
    if (level != 0 && level != 1) return fail(PSEG_EINVAL, "png: level %d (0 = fixed Huffman codes, 1 = dynamic codes per band)", level);
    if (H < 1 || W < 1) return fail(PSEG_EINVAL, "png: image of %d x %d pixels", H, W);
    if (channels != 1 && channels != 3) return fail(PSEG_EINVAL, "png: %d channels (1 = gray or 3 = RGB)", channels);
    if (band_rows < 0) return fail(PSEG_EINVAL, "png: band_rows %d (0 = default)", band_rows);
    if (!png_shape_ok(H, W, channels)) return fail(PSEG_EINVAL, "png: a row of %d pixels is too long", W);
    return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

size_t pseg_png_bound_lv(int H, int W, int channels, int band_rows, int level) { return png_bound(H, W, channels, band_rows, level); }
size_t pseg_png_bound(int H, int W, int channels, int band_rows) { return pseg_png_bound_lv(H, W, channels, band_rows, 0); }

int pseg_png_code_lengths(const uint32_t* counts, int n, int limit, uint8_t* lengths) {
    if (!counts || !lengths) return fail(PSEG_EINVAL, "NULL argument");
    if (n < 1 || n > PNG_NSYM || limit < 1 || limit > 15) return fail(PSEG_EINVAL, "png_code_lengths: %d symbols (1..286), limit %d (1..15)", n, limit);
    unsigned long long sum = 0;
    int used = 0;
    for (int s = 0; s < n; ++s) { sum += counts[s]; used += counts[s] != 0; }
    if (sum >> 32) return fail(PSEG_EINVAL, "png_code_lengths: the counts sum to 2^32 or more");
    if (used > (1 << limit)) return fail(PSEG_EINVAL, "png_code_lengths: %d used symbols have no code of at most %d bits", used, limit);
    uint32_t ws[PNG_CLWS];
    png_code_lengths(counts, n, limit, lengths, ws);
    return PSEG_OK;
}

int pseg_png_encode_device_lv(int device, const uint8_t* d_src, int H, int W, int channels, int band_rows, int level, uint8_t* out, size_t cap,
                              size_t* n_bytes, void* stream) {
    if (!d_src || !out || !n_bytes) return fail(PSEG_EINVAL, "NULL argument");
    PSEG_TRY(png_check(H, W, channels, band_rows, level));
    if (cap < png_bound(H, W, channels, band_rows, level))
        return fail(PSEG_EINVAL, "png: output buffer of %zu bytes, pseg_png_bound is %zu", cap, png_bound(H, W, channels, band_rows, level));
    PSEG_TRY(open_device(device));
    PngSrcPlain src{d_src, W, channels};
    uint8_t* const host[4] = {out, nullptr, nullptr, nullptr};
    size_t* const nb[4] = {n_bytes, nullptr, nullptr, nullptr};
    const int ids[4] = {0, 0, 0, 0};
    return png_run(device, src, H, W, channels, band_rows, level, 1, host, nb, ids, (hipStream_t)stream);
}
int pseg_png_encode_device(int device, const uint8_t* d_src, int H, int W, int channels, int band_rows, uint8_t* out, size_t cap,
                           size_t* n_bytes, void* stream) {
    return pseg_png_encode_device_lv(device, d_src, H, W, channels, band_rows, 0, out, cap, n_bytes, stream);
}

int pseg_masks_png_device_u8_lv(int device, const uint8_t* d_pred, const uint8_t* d_binary, const uint8_t* d_lut, int n_lut, int H, int W,
                                int band_rows, int level, uint8_t* const out[4], const size_t cap[4], size_t n_bytes[4], void* stream) {
    if (!d_pred || !d_binary || !d_lut || !out || !cap || !n_bytes) return fail(PSEG_EINVAL, "NULL argument");
    if (n_lut < 1 || n_lut > 256) return fail(PSEG_EINVAL, "n_lut %d out of range (1..256)", n_lut);
    PSEG_TRY(png_check(H, W, 3, band_rows, level));
    const size_t bound = png_bound(H, W, 3, band_rows, level);
    uint8_t* host[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t* nb[4] = {nullptr, nullptr, nullptr, nullptr};
    int ids[4] = {0, 0, 0, 0}, nout = 0;
    for (int k = 0; k < 4; ++k) {
        n_bytes[k] = 0;
        if (!out[k]) continue;
        if (cap[k] < bound) return fail(PSEG_EINVAL, "png: output buffer %d of %zu bytes, pseg_png_bound is %zu", k, cap[k], bound);
        host[nout] = out[k]; nb[nout] = &n_bytes[k]; ids[nout] = k;
        ++nout;
    }
    if (nout == 0) return PSEG_OK;
    PSEG_TRY(open_device(device));
    PngSrcMasks src{d_pred, d_binary, d_lut, n_lut, W};
    return png_run(device, src, H, W, 3, band_rows, level, nout, host, nb, ids, (hipStream_t)stream);
}
int pseg_masks_png_device_u8(int device, const uint8_t* d_pred, const uint8_t* d_binary, const uint8_t* d_lut, int n_lut, int H, int W,
                             int band_rows, uint8_t* const out[4], const size_t cap[4], size_t n_bytes[4], void* stream) {
    return pseg_masks_png_device_u8_lv(device, d_pred, d_binary, d_lut, n_lut, H, W, band_rows, 0, out, cap, n_bytes, stream);
}

int pseg_png_encode_lv(int device, const uint8_t* src, int H, int W, int channels, int band_rows, int level, uint8_t* out, size_t cap,
                       size_t* n_bytes) {
    if (!src || !out || !n_bytes) return fail(PSEG_EINVAL, "NULL argument");
    PSEG_TRY(png_check(H, W, channels, band_rows, level));
    if (cap < png_bound(H, W, channels, band_rows, level))
        return fail(PSEG_EINVAL, "png: output buffer of %zu bytes, pseg_png_bound is %zu", cap, png_bound(H, W, channels, band_rows, level));
    PSEG_TRY(open_device(device));
    const size_t n = (size_t)H * W * channels;
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, n) != hipSuccess) { (void)hipGetLastError(); return fail(PSEG_ENOMEM, "hipMalloc failed in png_encode"); }
    int rc = PSEG_OK;
    if (hipMemcpy(d, src, n, hipMemcpyHostToDevice) != hipSuccess) rc = fail(PSEG_EHIP, "H2D copy failed");
    if (rc == PSEG_OK) rc = pseg_png_encode_device_lv(device, d, H, W, channels, band_rows, level, out, cap, n_bytes, nullptr);
    (void)hipFree(d);
    return rc;
}
int pseg_png_encode(int device, const uint8_t* src, int H, int W, int channels, int band_rows, uint8_t* out, size_t cap, size_t* n_bytes) {
    return pseg_png_encode_lv(device, src, H, W, channels, band_rows, 0, out, cap, n_bytes);
}

int pseg_masks_png_lv(int device, const int64_t* pred, const uint8_t* binary, const uint8_t* lut, int n_lut, int H, int W, int band_rows,
                      int level, uint8_t* const out[4], const size_t cap[4], size_t n_bytes[4]) {
    if (!pred || !binary || !lut || !out || !cap || !n_bytes) return fail(PSEG_EINVAL, "NULL argument");
    if (n_lut < 1 || n_lut > 256) return fail(PSEG_EINVAL, "n_lut %d out of range (1..256)", n_lut);
    PSEG_TRY(png_check(H, W, 3, band_rows, level));
    PSEG_TRY(open_device(device));
    const size_t n = (size_t)H * W;
    // labels outside the colour table are black (masks_kernel): on the uint8 map they become 255, which is black while the table
    // has fewer than 256 entries
    std::vector<uint8_t> lab(n);
    bool outside = false;
    for (size_t i = 0; i < n; ++i) {
        const int64_t l = pred[i];
        if (l >= 0 && l < n_lut) lab[i] = (uint8_t)l;
        else { lab[i] = 255; outside = true; }
    }
    if (outside && n_lut == 256) return fail(PSEG_EINVAL, "png: labels outside a 256-entry colour table");
    uint8_t* d = nullptr;
    const size_t off_bin = (n + 255) & ~(size_t)255, off_lut = off_bin + ((n + 255) & ~(size_t)255);
    if (hipMalloc((void**)&d, off_lut + 768) != hipSuccess) { (void)hipGetLastError(); return fail(PSEG_ENOMEM, "hipMalloc failed in masks_png"); }
    int rc = PSEG_OK;
    if (hipMemcpy(d, lab.data(), n, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + off_bin, binary, n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + off_lut, lut, (size_t)n_lut * 3, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(PSEG_EHIP, "H2D copy failed");
    if (rc == PSEG_OK) rc = pseg_masks_png_device_u8_lv(device, d, d + off_bin, d + off_lut, n_lut, H, W, band_rows, level, out, cap, n_bytes, nullptr);
    (void)hipFree(d);
    return rc;
}
int pseg_masks_png(int device, const int64_t* pred, const uint8_t* binary, const uint8_t* lut, int n_lut, int H, int W, int band_rows,
                   uint8_t* const out[4], const size_t cap[4], size_t n_bytes[4]) {
    return pseg_masks_png_lv(device, pred, binary, lut, n_lut, H, W, band_rows, 0, out, cap, n_bytes);
}

}  // extern "C"
