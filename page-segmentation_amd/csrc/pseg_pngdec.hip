// pseg_pngdec.hip -- PNG scans decoded on the device: pseg_png_probe, pseg_png_decode_gray[_device|_host].
//
// The host reads the container (pseg_pngdec.h: probe) and copies the IDAT payloads of a group of files into page-locked staging;
// two launches per group, one workgroup of one wave per file, the parallelism is across files:
//   pngdec_inflate_kernel   the shared core's inflate_zlib under DevIO: the lanes run the symbol walk in step (every branch is
//                           uniform, the state lives in registers), lane 0 writes literals, the lanes share table fills, match
//                           copies, stored blocks and flushes.  Input comes through an 8 KiB window in LDS, output goes into a
//                           64 KiB ring in LDS -- every back-reference (<= 32768) reads the ring -- and leaves it in 16-byte units,
//                           Adler-32 summed on the way out.
//   pngdec_unfilter_kernel  64 rows per pass, lane k on row r0 + k one byte behind lane k - 1: "up" is the neighbour lane's last
//                           result, "left" and "upper left" a per-lane history of bpp bytes; writes the gray scan.
// The file's record carries its status; a file that fails anywhere writes no output byte.
#include "pseg_list.h"
#include "pseg_pngdec.h"

#include <algorithm>
#include <cstring>

namespace pseg {

constexpr int PD_NTH = 64;                                             // one wave
constexpr unsigned PD_RING = 65536, PD_MASK = PD_RING - 1;             // output ring: a power of two >= 32768 + PD_FLUSH + 16 + 258
constexpr unsigned PD_WIN = 8192;                                      // input window
constexpr unsigned PD_FLUSH = 16384;                                   // the ring is flushed once this much is waiting
constexpr unsigned PD_PIECE = 8192;                                    // stored blocks enter the ring in pieces of this size
static_assert(PD_RING >= 32768 + PD_FLUSH + 16 + 258 && PD_RING >= 32768 + PD_FLUSH + 16 + PD_PIECE, "a write never lands on a byte that waits for its flush or that a match may still read");

struct PdRec {
    unsigned long long in_off, inf_off;                                // the file's IDAT bytes and inflated bytes in the workspace, 16-byte aligned
    uint8_t* out;                                                      // H * W gray bytes
    unsigned in_len, expect;
    int H, W, ch, status;
};
static_assert(sizeof(PdRec) % 16 == 0, "records in front of 16-byte aligned data");

struct DevIO {
    const uint8_t* in;                                                 // 16-byte aligned, readable up to in_len rounded up to 16
    uint8_t* outg;
    uint8_t* ring;
    uint8_t* win;
    size_t in_len16;
    size_t win_base = ~(size_t)0;
    size_t flushed = 0;
    unsigned a = 1, b = 0;
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int lanes() const { return PD_NTH; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t in_u32(size_t p, size_t) {
        if (p < win_base || p >= win_base + PD_WIN) {
            __syncthreads();
            win_base = p & ~(size_t)15;
            for (unsigned k = threadIdx.x * 16u; k < PD_WIN; k += PD_NTH * 16u)
                if (win_base + k < in_len16) *(uint4*)(win + k) = *(const uint4*)(in + win_base + k);
            __syncthreads();
        }
        return *(const uint32_t*)(win + (p - win_base));
    }
    // [flushed, e) leaves the ring; e is a multiple of 16 unless `final`
    __device__ __forceinline__ void flush(size_t e, bool final) {
        __syncthreads();
        const size_t n = e - flushed;
        unsigned long long s1 = 0, s2 = 0;
        for (size_t u = flushed + (size_t)threadIdx.x * 16; u + 16 <= e; u += (size_t)PD_NTH * 16) {
            const uint4 v = *(const uint4*)(ring + ((unsigned)u & PD_MASK));
            *(uint4*)(outg + u) = v;
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
            unsigned long long sum = 0, wsum = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const unsigned d = (w[k >> 2] >> ((k & 3) * 8)) & 255u;
                sum += d;
                wsum += (unsigned)k * d;
            }
            s1 += sum;
            s2 += (unsigned long long)(n - (u - flushed)) * sum - wsum;
        }
        if (final) {
            const size_t u = (e & ~(size_t)15) + threadIdx.x;
            if (threadIdx.x < 16 && u < e) {
                const unsigned d = ring[(unsigned)u & PD_MASK];
                outg[u] = (uint8_t)d;
                s1 += d;
                s2 += (unsigned long long)(n - (u - flushed)) * d;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
        b = (unsigned)((b + (unsigned long long)(n % pngdec::ADLER_MOD) * a + s2 % pngdec::ADLER_MOD) % pngdec::ADLER_MOD);
        a = (unsigned)((a + s1) % pngdec::ADLER_MOD);
        flushed = e;
        __syncthreads();
    }
    __device__ __forceinline__ void room(size_t pos) {
        if (pos - flushed >= PD_FLUSH) flush(pos & ~(size_t)15, false);
    }
    __device__ __forceinline__ void put(size_t pos, uint8_t v) {
        room(pos);
        if (threadIdx.x == 0) ring[(unsigned)pos & PD_MASK] = v;
    }
    // zlib's byte-by-byte copy: byte i is byte i % dist of the dist bytes in front of pos, all of them written before this call
    __device__ __forceinline__ void copy(size_t pos, unsigned dist, unsigned len) {
        room(pos);
        __syncthreads();
        for (unsigned i = threadIdx.x; i < len; i += PD_NTH) {
            const unsigned k = dist >= len ? i : (dist == 1 ? 0u : i % dist);
            ring[(unsigned)(pos + i) & PD_MASK] = ring[(unsigned)(pos - dist + k) & PD_MASK];
        }
        __syncthreads();
    }
    __device__ __forceinline__ void stored(size_t pos, size_t ipos, unsigned len) {
        for (unsigned done = 0; done < len;) {
            const unsigned m = min(len - done, PD_PIECE);
            room(pos + done);
            __syncthreads();
            for (unsigned i = threadIdx.x; i < m; i += PD_NTH) ring[(unsigned)(pos + done + i) & PD_MASK] = in[ipos + done + i];
            __syncthreads();
            done += m;
        }
    }
    __device__ __forceinline__ uint32_t finish(size_t n) {
        flush(n, true);
        return (b << 16) | a;
    }
};

__global__ __launch_bounds__(PD_NTH) void pngdec_inflate_kernel(uint8_t* __restrict__ ws, PdRec* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[PD_RING];
    __shared__ __attribute__((aligned(16))) uint8_t win[PD_WIN];
    __shared__ pngdec::Tables t;
    const PdRec r = rec[blockIdx.x];
    DevIO io;
    io.in = ws + r.in_off;
    io.outg = ws + r.inf_off;
    io.ring = ring;
    io.win = win;
    io.in_len16 = ((size_t)r.in_len + 15) & ~(size_t)15;
    const int st = pngdec::inflate_zlib(io, t, (size_t)r.in_len, (size_t)r.expect);
    if (st != pngdec::OK && threadIdx.x == 0) rec[blockIdx.x].status = PSEG_EINVAL;
}

__global__ __launch_bounds__(PD_NTH) void pngdec_unfilter_kernel(uint8_t* ws, PdRec* rec) {
    const PdRec r = rec[blockIdx.x];
    if (r.status != PSEG_OK) return;
    const int lane = (int)threadIdx.x, bpp = r.ch;
    const int L = r.W * bpp;
    const size_t stride = (size_t)L + 1;
    uint8_t* const raw = ws + r.inf_off;
    int bad = 0;
    for (int y = lane; y < r.H; y += PD_NTH) bad |= raw[(size_t)y * stride] > 4;
    if (__syncthreads_or(bad)) {                                       // before the first output byte
        if (lane == 0) rec[blockIdx.x].status = PSEG_EINVAL;
        return;
    }
    for (int r0 = 0; r0 < r.H; r0 += PD_NTH) {
        const int row = r0 + lane;
        const bool valid = row < r.H;
        uint8_t* const p = raw + (size_t)(valid ? row : r.H - 1) * stride + 1;
        const uint8_t* const up_row = r0 ? raw + (size_t)(r0 - 1) * stride + 1 : nullptr;   // lane 0's "up": the last row of the pass before
        uint8_t* const g = r.out + (size_t)(valid ? row : r.H - 1) * r.W;
        const unsigned ft = p[-1];
        unsigned a0 = 0, a1 = 0, a2 = 0, c0 = 0, c1 = 0, c2 = 0, mine = 0;
        int px = 0, sub = 0;                                           // the pixel and the byte in it (bpp 3)
        for (int t = 0; t < L + PD_NTH - 1; ++t) {
            const int j = t - lane;                                    // lane k - 1 finished column j one step ago
            const unsigned from_up = __shfl_up(mine, 1);
            const bool active = valid && j >= 0 && j < L;
            const int jc = min(max(j, 0), L - 1);
            const unsigned x = p[jc];
            const unsigned b = lane ? from_up : (up_row ? (unsigned)up_row[jc] : 0u);
            const unsigned v = pngdec::unfilter_byte(ft, x, bpp == 1 ? a0 : a2, b, bpp == 1 ? c0 : c2);
            if (active) {
                if (lane == PD_NTH - 1) p[jc] = (uint8_t)v;            // the next pass reads this row as its "up"
                if (bpp == 1) g[jc] = (uint8_t)v;
                else {
                    if (sub == 2) { g[px] = (uint8_t)pngdec::gray_of_rgb(a1, a0, v); ++px; sub = 0; }
                    else ++sub;
                }
                a2 = a1; a1 = a0; a0 = v;
                c2 = c1; c1 = c0; c0 = b;
                mine = v;
            }
        }
        __syncthreads();                                               // lane 63's row is in memory before lane 0 reads it
    }
}

// ---- workspace: grow-only, one per device, guarded by its own lock; its own stream.  pseg_release_workspace frees it.
struct PdWs {
    GrowDev dev; GrowPin pin, pin_out; hipStream_t st = nullptr; hipEvent_t ev = nullptr;
    void release() {
        dev.release();
        pin.release();
        pin_out.release();
        if (st) (void)hipStreamDestroy(st);
        if (ev) (void)hipEventDestroy(ev);
        st = nullptr;
        ev = nullptr;
    }
};
static PerDevice<PdWs> g_pd;

struct PdFile { pngdec::Probe pr; std::vector<pngdec::Span> idat; };
static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// files[idx[0..n)], all sound containers: one upload, two launches, one read-back, one wait.  to_host: gray bytes come back through
// page-locked staging and reach outs[i] only for the files that decoded; else outs[i] is device memory the unfilter kernel writes.
static int pd_group(PdWs& ws, const int* idx, int n, const uint8_t* const* files, const std::vector<PdFile>& pf, uint8_t* const* outs,
                    bool to_host, int* status) {
    constexpr size_t rec_b = (size_t)LIST_GROUP_ITEMS * sizeof(PdRec);
    size_t idat_b = 0, inf_b = 0, gray_b = 0;
    for (int k = 0; k < n; ++k) {
        const pngdec::Probe& pr = pf[idx[k]].pr;
        idat_b += up16(pr.n_idat);
        inf_b += up16((size_t)pr.H * ((size_t)pr.W * pr.channels + 1));
        gray_b += up16((size_t)pr.H * pr.W);
    }
    if (!to_host) gray_b = 0;
    PSEG_TRY(ws.pin.ensure(rec_b + idat_b, "PNG decoder staging"));
    PSEG_TRY(ws.dev.ensure(rec_b + idat_b + inf_b + gray_b, "PNG decoder workspace"));
    if (to_host) PSEG_TRY(ws.pin_out.ensure(rec_b + gray_b, "PNG decoder read-back"));
    uint8_t* const d = ws.dev.p;
    PdRec* const h_rec = ws.pin.as<PdRec>();
    Bump in{rec_b}, inf{rec_b + idat_b}, gray{rec_b + idat_b + inf_b};
    for (int k = 0; k < n; ++k) {
        const PdFile& f = pf[idx[k]];
        PdRec& r = h_rec[k];
        r.in_len = (unsigned)f.pr.n_idat;
        r.expect = (unsigned)((size_t)f.pr.H * ((size_t)f.pr.W * f.pr.channels + 1));
        r.in_off = in.take(f.pr.n_idat, 16); r.inf_off = inf.take(r.expect, 16);
        r.H = f.pr.H; r.W = f.pr.W; r.ch = f.pr.channels; r.status = PSEG_OK;
        r.out = to_host ? d + gray.take((size_t)r.H * r.W, 16) : outs[idx[k]];
        uint8_t* dst = ws.pin.p + r.in_off;
        for (const pngdec::Span& s : f.idat) { memcpy(dst, files[idx[k]] + s.off, s.len); dst += s.len; }
        memset(dst, 0, up16(f.pr.n_idat) - f.pr.n_idat);
    }
    hipStream_t st = ws.st;
    GroupDrain drain{st};
    PSEG_HIP(hipMemcpyAsync(d, ws.pin.p, rec_b + idat_b, hipMemcpyHostToDevice, st));
    pngdec_inflate_kernel<<<(unsigned)n, PD_NTH, 0, st>>>(d, (PdRec*)d);
    pngdec_unfilter_kernel<<<(unsigned)n, PD_NTH, 0, st>>>(d, (PdRec*)d);
    PSEG_HIP(hipGetLastError());
    const PdRec* back = nullptr;
    if (to_host) {
        PSEG_HIP(hipMemcpyAsync(ws.pin_out.p, d, rec_b, hipMemcpyDeviceToHost, st));
        if (gray_b) PSEG_HIP(hipMemcpyAsync(ws.pin_out.p + rec_b, d + rec_b + idat_b + inf_b, gray_b, hipMemcpyDeviceToHost, st));
        back = ws.pin_out.as<PdRec>();
    } else {
        PSEG_HIP(hipMemcpyAsync(ws.pin.p, d, rec_b, hipMemcpyDeviceToHost, st));
        back = ws.pin.as<PdRec>();
    }
    PSEG_HIP(hipStreamSynchronize(st));                                // the group's one wait
    drain.armed = false;
    size_t g_off = rec_b;
    for (int k = 0; k < n; ++k) {
        const PdRec& r = back[k];
        status[idx[k]] = r.status == PSEG_OK ? PSEG_OK : PSEG_EINVAL;
        if (to_host) {
            if (r.status == PSEG_OK) memcpy(outs[idx[k]], ws.pin_out.p + g_off, (size_t)r.H * r.W);
            g_off += up16((size_t)r.H * r.W);
        }
    }
    return PSEG_OK;
}

static int pd_check_args(int n, const uint8_t* const* files, const size_t* n_bytes, uint8_t* const* out, int* status) {
    if (n < 0 || !files || !n_bytes || !out || !status) return fail(PSEG_EINVAL, n < 0 ? "negative file count" : "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!files[i] || !out[i]) return fail(PSEG_EINVAL, "file %d: NULL argument", i);
    return PSEG_OK;
}

static int pd_decode(int device, int n, const uint8_t* const* files, const size_t* n_bytes, uint8_t* const* outs, int* status, bool to_host,
                     hipStream_t after) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(pd_check_args(n, files, n_bytes, outs, status));
    std::vector<PdFile> pf((size_t)n);
    std::vector<int> st((size_t)n), ok;
    for (int i = 0; i < n; ++i) {
        std::vector<pngdec::Span>& v = pf[i].idat;
        pf[i].pr = pngdec::probe(files[i], n_bytes[i], [&v](size_t off, size_t len) { if (len) v.push_back({off, len}); });
        st[i] = pf[i].pr.status;
        if (st[i] == PSEG_OK) ok.push_back(i);
    }
    if (!ok.empty()) {
        auto inflated = [&](int k) {
            const pngdec::Probe& pr = pf[ok[k]].pr;
            return (size_t)pr.H * ((size_t)pr.W * pr.channels + 1);
        };
        auto first = [&](PdWs& ws) {
            if (!ws.st) PSEG_HIP(hipStreamCreateWithFlags(&ws.st, hipStreamNonBlocking));
            if (after) {                                               // what the caller's stream still does with the outputs comes first
                if (!ws.ev) PSEG_HIP(hipEventCreateWithFlags(&ws.ev, hipEventDisableTiming));
                PSEG_HIP(hipEventRecord(ws.ev, after));
                PSEG_HIP(hipStreamWaitEvent(ws.st, ws.ev, 0));
            }
            return (int)PSEG_OK;
        };
        PSEG_TRY(run_list(g_pd, device, (int)ok.size(), inflated, first, [&](PdWs& ws, int g0, int g1) {
            return pd_group(ws, ok.data() + g0, g1 - g0, files, pf, outs, to_host, st.data());
        }));
    }
    std::copy(st.begin(), st.end(), status);
    return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_png_probe(const uint8_t* file, size_t n_bytes, int* H, int* W, int* channels) {
    const pngdec::Probe pr = pngdec::probe(file, n_bytes, [](size_t, size_t) {});
    if (H) *H = pr.H;
    if (W) *W = pr.W;
    if (channels) *channels = pr.channels;
    return pr.status;
}

int pseg_png_decode_gray(int device, int n, const uint8_t* const* files, const size_t* n_bytes, uint8_t* const* out, int* status) {
    return pd_decode(device, n, files, n_bytes, out, status, true, nullptr);
}

int pseg_png_decode_gray_device(int device, int n, const uint8_t* const* files, const size_t* n_bytes, uint8_t* const* d_out, int* status,
                                void* stream) {
    return pd_decode(device, n, files, n_bytes, d_out, status, false, (hipStream_t)stream);
}

int pseg_png_decode_gray_host(int n, const uint8_t* const* files, const size_t* n_bytes, uint8_t* const* out, int* status) {
    if (n == 0) return PSEG_OK;
    PSEG_TRY(pd_check_args(n, files, n_bytes, out, status));
    pngdec::HostWork* w = new pngdec::HostWork();
    int rc = PSEG_OK;
    for (int i = 0; i < n && rc == PSEG_OK; ++i)
        if (pngdec::decode_gray_host_one(files[i], n_bytes[i], out[i], *w, &status[i]) < 0) rc = fail(PSEG_ENOMEM, "file %d: out of host memory", i);
    pngdec::host_work_free(*w);
    delete w;
    return rc;
}

}  // extern "C"
