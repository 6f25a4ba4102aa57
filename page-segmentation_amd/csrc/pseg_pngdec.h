// pseg_pngdec.h -- the PNG reader's core, one body for the host and the device: zlib header, bit reader, the three
// deflate block types with every validity check of zlib's inflate, the five PNG filters, the gray conversion.  The code is written
// against an IO policy (lane, lanes, sync, in_u32, put, copy, stored, finish): the host's (HostIO, below) is one lane over plain arrays, the device's (pseg_pngdec.hip) one wave whose lanes
// run the symbol walk in step and share table fills, match copies and flushes.  Whatever the policy:
//   * every read of the stream is bounded by its byte count (BitReader::refill, the stored-block check),
//   * every write is bounded by the expected inflated size (checked before put / copy / stored),
//   * every loop consumes input bits or produces output bytes, or has a constant trip count,
// so a malformed stream ends in an error code.  No recursion, no allocation, no arrays indexed at run time outside the tables the
// caller hands in (on the device: LDS; no scratch).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSEG_HD __host__ __device__
#else
#define PSEG_HD
#endif

namespace pseg {
namespace pngdec {

constexpr int OK = 0, BAD = -1;
constexpr int LIT_FAST = 10, DIST_FAST = 8, CL_FAST = 7;   // bits of the one-lookup tables; longer codes take the canonical walk
constexpr unsigned ADLER_MOD = 65521u;

// A canonical Huffman code: count[l] codes of length l, the symbols sorted by (length, value), and a table over the next FAST
// stream bits: (symbol << 4) | length, 0 where the code is longer than FAST bits or the bits are no code at all.
template <int NSYM, int FAST>
struct Huff {
    static constexpr int nsym = NSYM, fast_bits = FAST;
    uint16_t count[16], offs[16], first[16];
    uint16_t symbol[NSYM];
    uint16_t fast[1 << FAST];
};
struct Tables {
    Huff<288, LIT_FAST> lit;
    Huff<32, DIST_FAST> dist;
    Huff<19, CL_FAST> cl;
    uint8_t lens[288 + 32];
};

enum HuffKind { KIND_CODES = 0, KIND_LENS = 1, KIND_DISTS = 2 };

// lens[0..n) -> h.  BAD for an over-subscribed set, and for an incomplete one unless it is empty or -- not for the code-length
// code -- a single code of one bit (zlib's inflate_table).  The leader counts and sorts; every lane fills its share of the table.
template <class IO, class H>
PSEG_HD inline int huff_build(IO& io, H& h, const uint8_t* lens, int n, int kind) {
    io.sync();                                                         // lens are written, the last block's reads of h are done
    if (io.lane() == 0) {
        for (int l = 0; l < 16; ++l) h.count[l] = 0;
        for (int i = 0; i < n; ++i) h.count[lens[i]]++;
        unsigned off = 0, code = 0;
        h.offs[0] = 0;
        for (int l = 1; l < 16; ++l) {
            h.offs[l] = (uint16_t)off;
            h.first[l] = (uint16_t)off;                                // for now: the next free slot of the length
            off += h.count[l];
        }
        for (int i = 0; i < n; ++i)
            if (lens[i]) h.symbol[h.first[lens[i]]++] = (uint16_t)i;
        h.first[0] = 0;
        for (int l = 1; l < 16; ++l) {                                 // the first code of every length
            h.first[l] = (uint16_t)code;
            code = (code + h.count[l]) << 1;
        }
    }
    for (int k = io.lane(); k < (1 << H::fast_bits); k += io.lanes()) h.fast[k] = 0;
    io.sync();
    int left = 1, max = 0, total = 0;
    for (int l = 1; l < 16; ++l) {
        const int c = (int)h.count[l];
        left = (left << 1) - c;
        if (left < 0) return BAD;                                      // over-subscribed
        if (c) max = l;
        total += c;
    }
    if (left > 0 && max != 0 && (kind == KIND_CODES || max != 1)) return BAD;   // incomplete
    for (int idx = io.lane(); idx < total; idx += io.lanes()) {
        const unsigned sym = h.symbol[idx], l = lens[sym];
        if (l > (unsigned)H::fast_bits) continue;
        const unsigned code = h.first[l] + ((unsigned)idx - h.offs[l]);
        unsigned rev = 0;
        for (unsigned b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
        for (unsigned k = rev; k < (1u << H::fast_bits); k += 1u << l) h.fast[k] = (uint16_t)((sym << 4) | l);
    }
    io.sync();
    return OK;
}

// The symbol the low bits of `buf` start with, its length in *len; BAD where they are no code of h.
template <class H>
PSEG_HD inline int huff_decode(const H& h, uint64_t buf, int* len) {
    const unsigned e = h.fast[(unsigned)buf & ((1u << H::fast_bits) - 1u)];
    if (e & 15u) { *len = (int)(e & 15u); return (int)(e >> 4); }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {                                     // the canonical walk, one bit per length
        code |= (int)((buf >> (l - 1)) & 1u);
        const int count = (int)h.count[l];
        if (code - count < first) { *len = l; return h.symbol[index + (code - first)]; }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return BAD;
}

// The stream's bits, least significant first.  refill never reads at or past n_in; take() is only called with n <= cnt.
struct BitReader {
    uint64_t buf = 0;
    int cnt = 0;
    size_t pos = 0;
    template <class IO>
    PSEG_HD inline void refill(IO& io, size_t n_in) {
        while (cnt <= 32 && pos < n_in) {
            const unsigned sh = (unsigned)(pos & 3);
            size_t nb = 4 - sh;
            if (nb > n_in - pos) nb = n_in - pos;
            uint32_t w = io.in_u32(pos - sh, n_in) >> (8 * sh);
            if (nb < 4) w &= (1u << (8 * nb)) - 1u;
            buf |= (uint64_t)w << cnt;
            cnt += 8 * (int)nb;
            pos += nb;
        }
    }
    PSEG_HD inline unsigned take(int n) {
        const unsigned v = (unsigned)(buf & ((1ull << n) - 1ull));
        buf >>= n;
        cnt -= n;
        return v;
    }
};

// RFC 1950 + 1951.  n_in bytes of zlib stream through io -> exactly `expect` bytes, Adler-32 checked.  OK or BAD.
template <class IO>
PSEG_HD inline int inflate_zlib(IO& io, Tables& t, size_t n_in, size_t expect) {
    static constexpr uint16_t LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static constexpr uint8_t LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static constexpr uint16_t DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static constexpr uint8_t DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static constexpr uint8_t CLORD[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    BitReader br;
    br.refill(io, n_in);
    if (br.cnt < 16) return BAD;
    const unsigned cmf = br.take(8), flg = br.take(8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return BAD;
    size_t out = 0;
    for (unsigned last = 0; !last;) {
        br.refill(io, n_in);
        if (br.cnt < 3) return BAD;
        last = br.take(1);
        const unsigned type = br.take(2);
        if (type == 0) {                                               // ---- stored
            br.take(br.cnt & 7);
            br.refill(io, n_in);
            if (br.cnt < 32) return BAD;
            const unsigned len = br.take(16), nlen = br.take(16);
            if ((len ^ 0xffffu) != nlen) return BAD;
            br.pos -= (size_t)(br.cnt >> 3);                           // whole bytes back to the stream
            br.cnt = 0;
            br.buf = 0;
            if (len > n_in - br.pos || len > expect - out) return BAD;
            io.stored(out, br.pos, len);
            out += len;
            br.pos += len;
            continue;
        }
        if (type == 3) return BAD;
        if (type == 1) {                                               // ---- fixed codes (32 distance codes of 5 bits: 30 and 31 are refused below)
            io.sync();
            for (int i = io.lane(); i < 288 + 32; i += io.lanes()) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
            if (huff_build(io, t.lit, t.lens, 288, KIND_LENS) != OK) return BAD;
            if (huff_build(io, t.dist, t.lens + 288, 32, KIND_DISTS) != OK) return BAD;
        } else {                                                       // ---- dynamic codes
            if (br.cnt < 14) return BAD;
            const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
            if (nlen > 286 || ndist > 30) return BAD;
            io.sync();
            if (io.lane() == 0)
                for (int i = 0; i < 19; ++i) t.lens[i] = 0;
            for (int i = 0; i < ncode; ++i) {
                br.refill(io, n_in);
                if (br.cnt < 3) return BAD;
                const unsigned v = br.take(3);
                if (io.lane() == 0) t.lens[CLORD[i]] = (uint8_t)v;
            }
            if (huff_build(io, t.cl, t.lens, 19, KIND_CODES) != OK) return BAD;
            int prev = 0;
            for (int i = 0; i < nlen + ndist;) {
                br.refill(io, n_in);
                int l = 0;
                const int sym = huff_decode(t.cl, br.buf, &l);
                if (sym < 0 || l > br.cnt) return BAD;
                br.take(l);
                if (sym < 16) {
                    if (io.lane() == 0) t.lens[i] = (uint8_t)sym;
                    prev = sym;
                    ++i;
                    continue;
                }
                int rep, val = 0;
                if (sym == 16) {
                    if (i == 0 || br.cnt < 2) return BAD;              // nothing to repeat
                    val = prev;
                    rep = 3 + (int)br.take(2);
                } else if (sym == 17) {
                    if (br.cnt < 3) return BAD;
                    rep = 3 + (int)br.take(3);
                } else {
                    if (br.cnt < 7) return BAD;
                    rep = 11 + (int)br.take(7);
                }
                if (i + rep > nlen + ndist) return BAD;                // a repeat past HLIT + HDIST
                if (io.lane() == 0)
                    for (int k = 0; k < rep; ++k) t.lens[i + k] = (uint8_t)val;
                i += rep;
                prev = val;
            }
            io.sync();
            if (t.lens[256] == 0) return BAD;                          // no end-of-block code
            // the distance lengths move behind slot 288 so that both sets start where the fixed block's do
            io.sync();
            if (io.lane() == 0)
                for (int k = ndist - 1; k >= 0; --k) t.lens[288 + k] = t.lens[nlen + k];
            if (huff_build(io, t.lit, t.lens, nlen, KIND_LENS) != OK) return BAD;
            if (huff_build(io, t.dist, t.lens + 288, ndist, KIND_DISTS) != OK) return BAD;
        }
        for (;;) {                                                     // ---- the symbol walk: every turn takes at least one bit
            br.refill(io, n_in);
            int l = 0;
            int sym = huff_decode(t.lit, br.buf, &l);
            if (sym < 0 || l > br.cnt) return BAD;
            br.take(l);
            if (sym < 256) {
                if (out >= expect) return BAD;
                io.put(out, (uint8_t)sym);
                ++out;
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) return BAD;                                 // 286, 287
            if ((int)LEXT[sym] > br.cnt) return BAD;
            const unsigned len = LBASE[sym] + br.take(LEXT[sym]);
            br.refill(io, n_in);
            const int ds = huff_decode(t.dist, br.buf, &l);
            if (ds < 0 || l > br.cnt) return BAD;
            br.take(l);
            if (ds >= 30) return BAD;                                  // 30, 31
            if ((int)DEXT[ds] > br.cnt) return BAD;
            const unsigned dist = DBASE[ds] + br.take(DEXT[ds]);
            if (dist > out) return BAD;                                // before the start of the output
            if (len > expect - out) return BAD;
            io.copy(out, dist, len);
            out += len;
        }
    }
    br.take(br.cnt & 7);
    br.refill(io, n_in);
    if (br.cnt < 32) return BAD;
    unsigned want = 0;
    for (int k = 0; k < 4; ++k) want = (want << 8) | br.take(8);
    if (out != expect) return BAD;
    return io.finish(out) == want ? OK : BAD;
}

// ---- the host's policy: one lane, plain arrays ----------------------------------------------------------------------------------
struct HostIO {
    const uint8_t* in;
    uint8_t* outp;
    PSEG_HD inline int lane() const { return 0; }
    PSEG_HD inline int lanes() const { return 1; }
    PSEG_HD inline void sync() const {}
    PSEG_HD inline uint32_t in_u32(size_t p, size_t n_in) const {
        uint32_t w = 0;
        for (int k = 0; k < 4; ++k)
            if (p + k < n_in) w |= (uint32_t)in[p + k] << (8 * k);
        return w;
    }
    PSEG_HD inline void put(size_t pos, uint8_t v) { outp[pos] = v; }
    PSEG_HD inline void copy(size_t pos, unsigned dist, unsigned len) {
        for (unsigned i = 0; i < len; ++i) outp[pos + i] = outp[pos + i - dist];
    }
    PSEG_HD inline void stored(size_t pos, size_t ipos, unsigned len) {
        for (unsigned i = 0; i < len; ++i) outp[pos + i] = in[ipos + i];
    }
    PSEG_HD inline uint32_t finish(size_t n) const {
        uint32_t a = 1, b = 0;
        for (size_t i = 0; i < n;) {
            size_t e = i + 5552 < n ? i + 5552 : n;                    // 5552 bytes keep b below 2^32
            for (; i < e; ++i) { a += outp[i]; b += a; }
            a %= ADLER_MOD;
            b %= ADLER_MOD;
        }
        return (b << 16) | a;
    }
};

// ---- PNG filters (RFC 2083 6): x the filtered byte, a left, b up, c upper left (0 outside the image) ----------------------------
PSEG_HD inline unsigned unfilter_byte(unsigned ft, unsigned x, unsigned a, unsigned b, unsigned c) {
    unsigned p = 0;
    if (ft == 1) p = a;
    else if (ft == 2) p = b;
    else if (ft == 3) p = (a + b) >> 1;
    else if (ft == 4) {
        const int pa0 = (int)b - (int)c, pb0 = (int)a - (int)c, pc0 = pa0 + pb0;
        const int pa = pa0 < 0 ? -pa0 : pa0, pb = pb0 < 0 ? -pb0 : pb0, pc = pc0 < 0 ? -pc0 : pc0;
        p = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x + p) & 255u;
}
// PIL's convert("L") of an RGB pixel (ITU-R 601-2 luma, 16-bit fixed point, rounded)
PSEG_HD inline unsigned gray_of_rgb(unsigned r, unsigned g, unsigned b) { return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16; }

// The host's unfilter: raw = H rows of (filter byte, W * bpp bytes), every filter byte <= 4 (the caller checked), reconstructed in
// place; gray = H * W bytes.
inline void unfilter_host(uint8_t* raw, int H, int W, int bpp, uint8_t* gray) {
    const size_t L = (size_t)W * bpp;
    for (int y = 0; y < H; ++y) {
        uint8_t* const row = raw + (size_t)y * (L + 1) + 1;
        const uint8_t* const up = y ? row - (L + 1) : nullptr;
        const unsigned ft = row[-1];
        for (size_t j = 0; j < L; ++j) {
            const unsigned a = j >= (size_t)bpp ? row[j - bpp] : 0u, b = up ? up[j] : 0u, c = (up && j >= (size_t)bpp) ? up[j - bpp] : 0u;
            row[j] = (uint8_t)unfilter_byte(ft, row[j], a, b, c);
        }
        uint8_t* const g = gray + (size_t)y * W;
        if (bpp == 1) for (int x = 0; x < W; ++x) g[x] = row[x];
        else for (int x = 0; x < W; ++x) g[x] = (uint8_t)gray_of_rgb(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
    }
}


// ---- the container (host only) --------------------------------------------------------------------------------------------------
constexpr int ST_OK = 0, ST_EINVAL = -1, ST_EUNSUPPORTED = -5;         // PSEG_OK, PSEG_EINVAL, PSEG_EUNSUPPORTED of include/pseg.h

inline uint32_t crc32_of(const uint8_t* p, size_t n) {                 // table-driven, slicing by 8
    struct Tab {
        uint32_t t[8][256];
        Tab() {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
                t[0][i] = c;
            }
            for (uint32_t i = 0; i < 256; ++i)
                for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 255u];
        }
    };
    static const Tab T;
    uint32_t c = 0xffffffffu;
    while (n >= 8) {
        const uint32_t lo = c ^ ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
        c = T.t[7][lo & 255u] ^ T.t[6][(lo >> 8) & 255u] ^ T.t[5][(lo >> 16) & 255u] ^ T.t[4][lo >> 24] ^
            T.t[3][p[4]] ^ T.t[2][p[5]] ^ T.t[1][p[6]] ^ T.t[0][p[7]];
        p += 8;
        n -= 8;
    }
    while (n--) c = T.t[0][(c ^ *p++) & 255u] ^ (c >> 8);
    return c ^ 0xffffffffu;
}
inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

struct Span { size_t off, len; };
struct Probe {
    int status = ST_EINVAL;
    int H = 0, W = 0, channels = 0;                                    // set whenever the IHDR chunk could be read
    size_t n_idat = 0;                                                 // payload bytes of all IDAT chunks
};
// The file's container: signature, IHDR first with length 13, the CRC of every critical chunk, consecutive IDAT chunks (any of them
// may be empty), IEND.  Ancillary chunks are skipped unread, but tRNS is noted.  A broken container is ST_EINVAL; a sound one that
// is not 8-bit gray or RGB without interlace and tRNS, holds a critical chunk this reader does not know, or inflates to more than
// 0x7fffffff bytes is ST_EUNSUPPORTED.  `on_idat(off, len)` sees every IDAT payload in order (also of files that end up refused).
template <class F>
inline Probe probe(const uint8_t* f, size_t n, F on_idat) {
    static const uint8_t SIG[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
    Probe r;
    if (!f || n < 8) return r;
    for (int k = 0; k < 8; ++k)
        if (f[k] != SIG[k]) return r;
    size_t pos = 8;
    bool first = true, seen_idat = false, idat_closed = false, seen_end = false, trns = false, unknown = false, plte = false;
    unsigned depth = 0, ctype = 0, interlace = 0;
    while (!seen_end) {
        if (n - pos < 12) return r;                                    // no room for a chunk: no IEND
        const uint32_t len = be32(f + pos);
        if (len > 0x7fffffffu || (size_t)len > n - pos - 12) return r;
        const uint8_t* const type = f + pos + 4;
        const uint8_t* const data = type + 4;
        for (int k = 0; k < 4; ++k)
            if (!((type[k] >= 'A' && type[k] <= 'Z') || (type[k] >= 'a' && type[k] <= 'z'))) return r;
        const bool critical = !(type[0] & 32u);
        const uint32_t tag = be32(type);
        if (first != (tag == 0x49484452u)) return r;                   // IHDR first, and only there
        if (critical && crc32_of(type, 4 + (size_t)len) != be32(data + len)) return r;
        if (tag == 0x49484452u) {
            if (len != 13) return r;
            const uint32_t w = be32(data), h = be32(data + 4);
            depth = data[8]; ctype = data[9]; interlace = data[12];
            if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu || data[10] != 0 || data[11] != 0 || interlace > 1) return r;
            const bool d_ok = ctype == 0 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                            : ctype == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                            : (ctype == 2 || ctype == 4 || ctype == 6) ? (depth == 8 || depth == 16) : false;
            if (!d_ok) return r;
            r.W = (int)w; r.H = (int)h;
            r.channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : 4;
        } else if (tag == 0x49444154u) {                               // IDAT
            if (idat_closed) return r;
            seen_idat = true;
            r.n_idat += len;
            on_idat((size_t)(data - f), (size_t)len);
        } else {
            if (seen_idat) idat_closed = true;
            if (tag == 0x49454e44u) seen_end = true;                   // IEND
            else if (tag == 0x504c5445u) plte = true;                  // PLTE
            else if (tag == 0x74524e53u) trns = true;                  // tRNS
            else if (critical) unknown = true;
        }
        first = false;
        pos += 12 + (size_t)len;
    }
    if (!seen_idat) return r;
    if (ctype == 3 && !plte) return r;
    const unsigned long long inflated = (unsigned long long)r.H * (1ull + (unsigned long long)r.W * r.channels);
    const bool ours = depth == 8 && (ctype == 0 || ctype == 2) && interlace == 0 && !trns && !unknown && inflated <= 0x7fffffffull && r.n_idat <= 0x7fffffffull;
    r.status = ours ? ST_OK : ST_EUNSUPPORTED;
    return r;
}

// One file through the shared core on the host: status as probe's, ST_EINVAL also for a bad stream or filter byte.  `out` (H * W
// bytes) is written only when the file is sound.  work: the caller's scratch, reused from file to file.
struct HostWork { uint8_t* idat = nullptr; size_t idat_cap = 0; uint8_t* raw = nullptr; size_t raw_cap = 0; Tables t; };
}  // namespace pngdec
}  // namespace pseg
#include <cstdlib>
#include <cstring>
namespace pseg {
namespace pngdec {
inline void host_work_free(HostWork& w) { free(w.idat); free(w.raw); w.idat = w.raw = nullptr; w.idat_cap = w.raw_cap = 0; }
inline bool host_work_fit(uint8_t*& p, size_t& cap, size_t need) {
    if (cap >= need && p) return true;
    free(p);
    p = (uint8_t*)malloc(need ? need : 1);
    cap = p ? need : 0;
    return p != nullptr;
}
// < 0: out of memory (the caller's error); else the file's status
inline int decode_gray_host_one(const uint8_t* f, size_t n, uint8_t* out, HostWork& w, int* status) {
    Probe pr = probe(f, n, [](size_t, size_t) {});
    *status = pr.status;
    if (pr.status != ST_OK) return 0;
    const size_t L = (size_t)pr.W * pr.channels, expect = (size_t)pr.H * (L + 1);
    if (!host_work_fit(w.idat, w.idat_cap, pr.n_idat) || !host_work_fit(w.raw, w.raw_cap, expect)) return -1;
    size_t at = 0;
    uint8_t* const idat = w.idat;
    probe(f, n, [&](size_t off, size_t len) { memcpy(idat + at, f + off, len); at += len; });
    HostIO io{idat, w.raw};
    if (inflate_zlib(io, w.t, pr.n_idat, expect) != OK) { *status = ST_EINVAL; return 0; }
    for (int y = 0; y < pr.H; ++y)
        if (w.raw[(size_t)y * (L + 1)] > 4) { *status = ST_EINVAL; return 0; }
    unfilter_host(w.raw, pr.H, pr.W, pr.channels, out);
    return 0;
}

}  // namespace pngdec
}  // namespace pseg
