// pseg_exact_mfma.hip -- float32-exact convolution on the matrix cores.
//
// v_mfma_f32_16x16x4_f32 accumulates its four k-values as the sequential chain
// acc = fmaf(a[k], b[k], acc), k = 0..3, and continues the chain across instructions (checked on
// MI355X by tools/microtests/mfma_f32_chain.hip: 256/256 outputs bitwise equal at K = 100).  With
// k ordered as the oracle's loop nest -- (block of 16 input channels, ky, kx, ci inside the block), oracle/pseg_oracle.c
// -- the kernels below therefore produce the SAME bits as the scalar chain, at MFMA rate (157 TFLOP/s f32 peak):
//   * out-of-image taps and the channel padding of a block to a multiple of four feed x = 0 (and w = 0):
//     fmaf(0, w, acc) == acc exactly (acc is never -0: it starts at +0);
//   * then acc + bias (+ residual), ReLU -- the same operation sequence as the scalar kernel.
// Round 3: the chain is BLOCKED over the input channels (rounds 1-2 ran it over all channels inside each tap, which
// forced all-channel LDS tiles: 140 KB for fcn_skip's 120-channel layer, no LDS form at all for unet's 1024).  A
// workgroup now stages a 16-channel slab of its halo tile (31 KB for a k5 layer: four to five workgroups per CU, so one
// workgroup's staging hides under the others' MFMAs), runs every tap over it, and moves to the next slab with the
// accumulators in registers; any channel count fits, predict and train share one order and one kernel.
//
// Layout: D[cout][pixel] per 16x16 tile; lane l = (p16 = l & 15, g = l >> 4).
//   A (weights):  lane holds w[k = 4s + g][cout = 16t + p16]   (global load, L1/L2 resident)
//   B (pixels):   lane holds x[pixel p16][channel 4s + g]        (ds_read_b32 from the LDS tile)
//   D:            lane holds couts 16t + 4g .. +3 of pixel p16  (16-byte store)
// LDS pixel stride 18 floats (2 mod 4): 16 pixels x 2 lane groups hit 32 distinct banks (conflict-free ds_read_b32).
// out_sy/out_sx/out_oy/out_ox scatter the output pixel grid (Conv2DTranspose k2 s2 = four 1x1
// convolutions, one per sub-pixel, written to (2y + a, 2x + b)).
#include <algorithm>
#include <type_traits>

#include "pseg_common.h"

namespace pseg {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int XTW = 32;   // output tile width (two 16-pixel MFMA column tiles)

// MT = pixel tiles per wave (4: two rows x two column tiles, 2: one row), NT = cout tiles per workgroup.
// FLAT = false: k-steps are (tap, four channels), channels zero-padded to a multiple of four per tap
//               (all lanes of a k-step share the tap: scalar tap loop, no per-lane bookkeeping);
// FLAT = true : K flattened across taps, k = (ky*KW + kx)*Cin + ci (first layers: Cin = 1 packs four
//               taps into one MFMA instead of wasting three quarters of it).
// Both orders are the oracle's chain order; the padded / trailing k feed w = 0 against a finite x.
template <int MT, int NT, bool FLAT>
__global__ __launch_bounds__(256) void conv_exact_mfma_kernel(ConvArgs a, int Cp, int THH, int TWH, int CB) {
    extern __shared__ __attribute__((aligned(16))) float xt[];   // [THH][TWH][Cp]
    constexpr int RW = MT / 2;            // output rows per wave
    constexpr int TH = 4 * RW;            // output rows per workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p16 = lane & 15, g = lane >> 4;
    const int tiles_x = (a.Wout + XTW - 1) / XTW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int oy0 = ty * TH, ox0 = tx * XTW;
    const int iy0 = oy0 * a.stride - a.pt, ix0 = ox0 * a.stride - a.pl;
    const int Cin = a.C0 + a.C1;
    const int co_base = blockIdx.y * (NT * 16);
    const int Ntot = a.deconv4 ? 4 * a.Cout : a.Cout;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Channel blocks: every launch passes CB == Cin (one block: the first layers' flattened chain); with a smaller CB the chain
    // would run (block, ky, kx, ci) over tiles of CB channels.
    for (int cb = 0; cb < Cin; cb += CB) {
    const int cn = min(CB, Cin - cb);
    if (cb) __syncthreads();                         // every wave is done reading the previous block's tile
    // ---- stage the halo tile: the block's input channels, zeros outside the image and in the channel pad
    const int npx = THH * TWH;
    // One item = (pixel, 64-channel slice): lanes over channels.  Eight items are fetched before the first one is used: a
    // value looked at right behind its load (ReLU, mask, the store itself) costs a full memory latency per item, and a
    // wave has ~110 of them per tile -- that chain, not the MFMAs, was most of this kernel's time on the thin layers.
    constexpr int FJ = 16;                               // 64-float pieces of a tile row in flight per wave
    if (a.dbg & 1) {
        for (int i = tid; i < npx * Cp; i += 256) xt[i] = 0.0f;
    } else if (!a.up0 && !a.up1 && cn == Cin && a.C0 < 64 && a.C1 < 64) {
        // Thin layers (every source under 64 channels: all of fcn / fcn_skip and their data gradients): a tile row is ONE
        // contiguous run of TWH * C floats per source tensor -- lanes over that run (all 64 busy instead of C of them),
        // sixteen pieces requested before the first is used; a Concatenate is two such runs side by side in the LDS pixel.
        // (The lanes-over-channels path below spent 0.85 of deconv5's 1.19 ms on its two-source tile: 0.26 TB/s.)
        for (int srcsel = 0; srcsel < (a.src1 ? 2 : 1); ++srcsel) {
        const int C = srcsel ? a.C1 : a.C0, cbase = srcsel ? a.C0 : 0;
        const float* const sbase = srcsel ? a.src1 : a.src0;
        const float* const mbase = srcsel ? nullptr : a.mask;
        const int rowf = TWH * C, nj = (rowf + 63) >> 6;
        const unsigned invc = (1u << 20) / (unsigned)C + 1u;     // e < 67 * 64: e * invc < 2^32
        int dj0[FJ];                                     // the first sixteen pieces' (pixel, LDS offset), the same for every row
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
            const int e = j * 64 + lane;
            const int px = (int)(((unsigned)e * invc) >> 20), c = e - px * C;
            dj0[j] = e < rowf ? (px << 16 | (px * Cp + cbase + c)) : -1;
        }
        for (int r = wave; r < THH; r += 4) {
            const int iy = iy0 + r;
            const bool rowok = iy >= 0 && iy < a.Hin;
            const size_t ro = ((size_t)(rowok ? iy : 0) * a.Win) * C;
            const float* srow = sbase + ro + (ptrdiff_t)ix0 * C;           // (lanes left of the image are masked below)
            const float* mrow = mbase ? mbase + ro + (ptrdiff_t)ix0 * C : nullptr;
            float* drow = xt + (size_t)r * TWH * Cp;
            for (int j0 = 0; j0 < nj; j0 += FJ) {
                float v[FJ], mv[FJ];
                int dj[FJ];                              // LDS offset of the piece's float inside the tile row, or -1
#pragma unroll
                for (int j = 0; j < FJ; ++j) {
                    const int e = (j0 + j) * 64 + lane;
                    int pk = dj0[j];
                    if (j0) {
                        const int px_ = (int)(((unsigned)e * invc) >> 20), c = e - px_ * C;
                        pk = e < rowf ? (px_ << 16 | (px_ * Cp + cbase + c)) : -1;
                    }
                    const int px = pk >> 16;
                    dj[j] = pk < 0 ? -1 : (pk & 0xFFFF);
                    v[j] = 0.0f;
                    mv[j] = 1.0f;
                    if (pk >= 0 && rowok && (unsigned)(ix0 + px) < (unsigned)a.Win) {
                        v[j] = srow[e];
                        if (mrow) mv[j] = mrow[e];
                    }
                }
#pragma unroll
                for (int j = 0; j < FJ; ++j) {
                    float x = v[j];
                    if (a.in_relu) x = x > 0.0f ? x : 0.0f;
                    x = mv[j] > 0.0f ? x : 0.0f;
                    if (dj[j] >= 0) drow[dj[j]] = x;
                }
            }
        }
        }
        // the channel pad of every pixel (k-steps run over 4 * ceil(Cin / 4) channels)
        for (int i = tid; i < npx * (Cp - Cin); i += 256) {
            const int p = i / (Cp - Cin), c = Cin + i - p * (Cp - Cin);
            xt[p * Cp + c] = 0.0f;
        }
    } else {
        constexpr int SU = 8;
        const int nch = (Cp + 63) >> 6;                  // slices per pixel
        const int nit = ((npx - wave + 3) >> 2) * nch;   // items of this wave
        for (int it0 = 0; it0 < nit; it0 += SU) {
            float v[SU], mv[SU];
            int dsto[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int it = it0 + u;
                const int pq = it / nch, sl = it - pq * nch;
                const int p = wave + 4 * pq, cl = sl * 64 + lane;
                const int r = p / TWH, c = p - r * TWH;
                const int iy = iy0 + r, ix = ix0 + c;
                const bool in = it < nit && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
                const int ch = cb + cl;
                v[u] = 0.0f;
                mv[u] = 1.0f;
                dsto[u] = (it < nit && cl < Cp) ? p * Cp + cl : -1;
                if (in && cl < cn) {
                    if (ch < a.C0) {
                        const size_t o = ((size_t)(iy >> a.up0) * (a.Win >> a.up0) + (ix >> a.up0)) * a.C0 + ch;
                        v[u] = a.src0[o];
                        if (a.mask) mv[u] = a.mask[o];
                    } else {
                        v[u] = a.src1[((size_t)(iy >> a.up1) * (a.Win >> a.up1) + (ix >> a.up1)) * a.C1 + (ch - a.C0)];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                float x = v[u];
                if (a.in_relu) x = x > 0.0f ? x : 0.0f;
                x = mv[u] > 0.0f ? x : 0.0f;
                if (dsto[u] >= 0) xt[dsto[u]] = x;
            }
        }
    }
    __syncthreads();

    int pixoff[MT];   // float offset of this lane's pixel at tap (0,0), channel 0
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int row = wave * RW + (m >> 1), col = (m & 1) * 16 + p16;
        pixoff[m] = (row * a.stride * TWH + col * a.stride) * Cp;
    }
    // this lane's weight column per cout tile: w[k*Cout + wcol] (transposed conv k2 s2 as one GEMM over
    // n = ab*Cout + co: the sub-pixel's kernel starts ab*Cin*Cout further on), or -1 past the layer
    int wcol[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = co_base + t * 16 + p16;
        const int ab = a.deconv4 ? n / a.Cout : 0;
        wcol[t] = n < Ntot ? ab * Cin * a.Cout + (n - ab * a.Cout) : -1;
    }
    // Lanes without a weight to load (channel / cout padding, k past the layer) read the first float of the zero slack
    // every weight buffer carries behind its last element: the load is unconditional and its result needs no select, so
    // the loads of k-step s + 1 stay in flight under the MFMAs of k-step s (as a conditional load they compiled to
    // branches with a full memory wait right behind them).
    const int zoff = (a.deconv4 ? 4 : a.KH * a.KW) * Cin * a.Cout;
    float xa[MT], wa[NT], xb[MT], wb[NT];
#define PSEG_XMMA(XF, WF)                                                                        \
    _Pragma("unroll") for (int t = 0; t < NT; ++t)                                               \
        _Pragma("unroll") for (int m = 0; m < MT; ++m)                                           \
            acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(WF[t], XF[m], acc[m][t], 0, 0, 0);
    if (a.dbg & 4) {
    } else if constexpr (!FLAT) {
        const int nks = (cn + 3) >> 2;         // k-steps per tap
        for (int ky = 0; ky < a.KH; ++ky)
            for (int kx = 0; kx < a.KW; ++kx) {
                const int wbase = ((ky * a.KW + kx) * Cin + cb) * a.Cout;
                const float* wt = a.w + wbase;
                const int toff = (ky * TWH + kx) * Cp + g;
                auto load = [&](float* xf, float* wf, int s) {
                    const int ci = 4 * s + g;
#pragma unroll
                    for (int m = 0; m < MT; ++m) xf[m] = xt[pixoff[m] + toff + 4 * s];
                    const bool okc = ci < cn;
#pragma unroll
                    for (int t = 0; t < NT; ++t) wf[t] = wt[(okc && wcol[t] >= 0) ? ci * a.Cout + wcol[t] : zoff - wbase];
                };
                load(xa, wa, 0);
                int s = 0;
                for (; s + 2 <= nks; s += 2) {
                    load(xb, wb, s + 1);
                    PSEG_XMMA(xa, wa)
                    if (s + 2 < nks) load(xa, wa, s + 2);
                    PSEG_XMMA(xb, wb)
                }
                if (s < nks) { PSEG_XMMA(xa, wa) }
            }
    } else {
        const int Ktot = a.KH * a.KW * Cin;
        const int nks = (Ktot + 3) >> 2;
        const int wraps = Cin >= 4 ? 1 : 4;          // tap boundaries one step of four can cross
        int k_l = g, ci_l = g, kx_l = 0, toff_l = 0;  // this lane's k, channel, kernel column, tap offset
        auto wrap = [&]() {
            for (int w = 0; w < wraps; ++w) {
                const bool wr = ci_l >= Cin;
                ci_l -= wr ? Cin : 0;
                kx_l += wr ? 1 : 0;
                toff_l += wr ? Cp : 0;
                const bool rw = kx_l == a.KW;
                kx_l = rw ? 0 : kx_l;
                toff_l += rw ? (TWH - a.KW) * Cp : 0;
            }
        };
        wrap();
        auto load = [&](float* xf, float* wf) {
            const bool okk = k_l < Ktot;
            const int xo = okk ? toff_l + ci_l : 0;
#pragma unroll
            for (int m = 0; m < MT; ++m) xf[m] = xt[pixoff[m] + xo];
#pragma unroll
            for (int t = 0; t < NT; ++t) wf[t] = a.w[(okk && wcol[t] >= 0) ? k_l * a.Cout + wcol[t] : zoff];
            k_l += 4;
            ci_l += 4;
            wrap();
        };
        load(xa, wa);
        int s = 0;
        for (; s + 2 <= nks; s += 2) {
            load(xb, wb);
            PSEG_XMMA(xa, wa)
            load(xa, wa);
            PSEG_XMMA(xb, wb)
        }
        if (s < nks) { PSEG_XMMA(xa, wa) }
    }
    }   // channel blocks
#undef PSEG_XMMA

    // ---- epilogue: acc + bias (+ add), ReLU; lane owns n = 4g..4g+3 of pixel p16 in every tile.  The lane's four values are
    // consecutive output channels of one pixel (of one sub-pixel, for the transposed GEMM: Cout % 4 == 0 keeps a quad inside
    // its sub-pixel): one 16-byte (or two 8-byte, Cout even) store instead of four 4-byte ones -- Conv2DTranspose k2 s2 at full
    // resolution (deconv5: 252 MB of output) spent 1.28 ms in scalar scatter stores.
    const int osy = a.out_sy ? a.out_sy : 1, osx = a.out_sx ? a.out_sx : 1;
    const int pitch = a.dst_pitch ? a.dst_pitch : a.Wout;
    const int vecw = (a.Cout & 3) == 0 ? 4 : ((a.Cout & 1) == 0 ? 2 : 1);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int y = oy0 + wave * RW + (m >> 1), x = ox0 + (m & 1) * 16 + p16;
        if (y >= a.Hout || x >= a.Wout || ((a.dbg & 2) && acc[m][0][0] != 123.456f)) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n0 = co_base + t * 16 + 4 * g;
            if (n0 >= Ntot) continue;
            float v[4];
            size_t off[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + r;
                const int nn = n < Ntot ? n : n0;                 // (values past the layer are never stored)
                const int ab = a.deconv4 ? nn / a.Cout : 0;
                const int co = nn - ab * a.Cout;
                const size_t opix = a.deconv4 ? (size_t)(2 * y + (ab >> 1)) * pitch + (size_t)(2 * x + (ab & 1))
                                              : (size_t)(y * osy + a.out_oy) * pitch + (size_t)(x * osx + a.out_ox);
                off[r] = opix * a.Cout + co;
                v[r] = a.bias ? acc[m][t][r] + a.bias[co] : acc[m][t][r];
            }
            if (a.add) {
                if (vecw == 4 && n0 + 3 < Ntot) {
                    const float4 ad = *(const float4*)(a.add + off[0]);
                    v[0] = v[0] + ad.x; v[1] = v[1] + ad.y; v[2] = v[2] + ad.z; v[3] = v[3] + ad.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n0 + r < Ntot) v[r] = v[r] + a.add[off[r]];
                }
            }
            if (a.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.0f ? v[r] : 0.0f;
            }
            if (vecw == 4 && n0 + 3 < Ntot) {
                *(float4*)(a.dst + off[0]) = make_float4(v[0], v[1], v[2], v[3]);
            } else if (vecw >= 2) {
                if (n0 + 1 < Ntot) *(float2*)(a.dst + off[0]) = make_float2(v[0], v[1]);
                else a.dst[off[0]] = v[0];
                if (n0 + 3 < Ntot) *(float2*)(a.dst + off[2]) = make_float2(v[2], v[3]);
                else if (n0 + 2 < Ntot) a.dst[off[2]] = v[2];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < Ntot) a.dst[off[r]] = v[r];
            }
        }
    }
}

// ---- blocked-chain kernel (every layer with Cin >= 8) -----------------------------------------------------------------
constexpr int XCB = PSEG_CHAIN_BLOCK;   // input channels per pass of the chain (oracle/pseg_oracle.c: ORC_CHAIN_BLOCK)
constexpr int XCP = XCB + 2;     // LDS pixel pitch in floats

// MT = pixel tiles per wave (4: two rows x two column tiles, 2: one row), NT = cout tiles per workgroup (<= 4: 64 accumulator
// registers, four waves per SIMD).  One (tap, four channels) k-step = MT ds_read_b32 + NT global loads for MT x NT MFMAs of
// 32 cycles each; the k-steps of a slab form ONE software-pipelined stream across taps (the fragments of step q + 1 are
// requested before the MFMAs of step q; a per-tap pipeline would expose a load latency every four k-steps).
// REM (0, 4 or 8): output channels left over behind the NT full tiles.  A 16-row tile for 4 or 8 channels multiplies
// padding (Cout = 40 on three tiles: 17 %, Cout = 20 on two: 37 %).  The left-over rows are instead filled with the same
// channels of DX = 16 / REM horizontally neighbouring pixels: row (dx, j) of the tile is channel 16 NT + j of pixel
// DX * p + dx, its columns are pixel groups p, and its kernel is the layer's kernel shifted by dx along kx (zero outside:
// KW + DX - 1 taps per kernel row; a.wrem, built by wrem_kernel).  Each output still sees its own taps in (slab, ky, kx, ci)
// order with exact-zero products in between -- the same bits -- and the tile covers DX times the pixels: 6/5 x 1/2 (REM 8)
// or 8/5 x 1/4 (REM 4) of a padded tile's MFMAs.
template <int MT, int NT, int TAILK, int REM = 0>
__global__ __launch_bounds__(256) void conv_xb_kernel(ConvArgs a, int THH, int TWH, unsigned inv_twh) {
    extern __shared__ __attribute__((aligned(16))) float xt[];   // [THH][TWH][XCP]
    constexpr int RW = MT / 2;            // output rows per wave
    constexpr int TH = 4 * RW;            // output rows per workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p16 = lane & 15, g = lane >> 4;
    const int tiles_x = (a.Wout + XTW - 1) / XTW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int oy0 = ty * TH, ox0 = tx * XTW;
    const int iy0 = oy0 * a.stride - a.pt, ix0 = ox0 * a.stride - a.pl;
    const int Cin = a.C0 + a.C1;
    const int co_base = blockIdx.y * (NT * 16);
    const int Ntot = a.deconv4 ? 4 * a.Cout : a.Cout;
    const int npx = THH * TWH;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    int xbase[MT];   // float offset of this lane's fragment element at tap (0,0), k-step 0 of a slab: its pixel, channel g
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int row = wave * RW + (m >> 1), col = (m & 1) * 16 + p16;
        xbase[m] = (row * a.stride * TWH + col * a.stride) * XCP + g;
    }
    // this lane's weight byte offset per cout tile: w[(k = g)*Cout + column] (transposed conv k2 s2 as one GEMM over
    // n = ab*Cout + co: the sub-pixel's kernel starts ab*Cin*Cout further on); out of range past the layer (reads 0)
    const unsigned wbytes = (unsigned)((size_t)(a.deconv4 ? 4 : a.KH * a.KW) * Cin * a.Cout * 4);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, wbytes, 0x00020000);
    unsigned voff[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = co_base + t * 16 + p16;
        const int ab = a.deconv4 ? n / a.Cout : 0;
        voff[t] = n < Ntot ? (unsigned)(ab * Cin * a.Cout + (n - ab * a.Cout) + g * a.Cout) * 4u : 0x7ffffff0u;
    }
    const bool pairs = ((a.C0 | a.C1) & 1) == 0;     // even channel counts: a lane stages two channels with 8-byte accesses
    // left-over channels (REM): RT tiles per wave over its RW rows -- pixel pairs of one row each (REM 8) or pixel quads of
    // both rows (REM 4: columns 0-7 the upper row's quads, 8-15 the lower row's)
    constexpr int DX = REM ? 16 / REM : 1;
    constexpr int RT = REM == 8 ? RW : (REM == 4 ? RW / 2 : 0);
    static_assert(REM == 0 || (MT == 4 && (REM == 4 || REM == 8)), "left-over channel tiles: 8-row workgroup tiles only");
    f32x4 accr[RT ? RT : 1];
    int xrbase[RT ? RT : 1];
#pragma unroll
    for (int rt = 0; rt < (RT ? RT : 1); ++rt) {
        accr[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int row = REM == 8 ? wave * RW + rt : wave * RW + rt * 2 + (p16 >> 3);
        const int col = REM == 8 ? 2 * p16 : 4 * (p16 & 7);
        xrbase[rt] = (row * TWH + col) * XCP + g;
    }
    const int KWR = a.KW + DX - 1;
    const __amdgpu_buffer_rsrc_t wrrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(REM ? a.wrem : a.w), 0, REM ? (unsigned)((size_t)a.KH * KWR * Cin * 16 * 4) : 0u, 0x00020000);
    const unsigned voffr = (unsigned)(g * 16 + p16) * 4u;

    // One slab = stage 16 channels of the halo tile, run every tap over them.  `nks_tag` carries the k-steps per tap as a
    // compile-time constant.  The full slabs run in the loop below (four k-steps per tap); a shorter last slab (TAILK, picked
    // by the host from the channel count) follows the loop as straight-line code -- with both forms inside one loop the
    // accumulators were allocated more than twice over (80 AGPRs for 32 accumulator registers at NT = 2, 156 for 64 at
    // NT = 4: two waves per SIMD instead of three or four).
    auto process_slab = [&](const int cb, auto nks_tag) {
        const int cn = min(XCB, Cin - cb);
        if (cb) __syncthreads();                     // every wave is done reading the previous slab
        // ---- stage the slab: channels cb .. cb+15 of the halo tile (zeros outside the image and past the layer's channels).
        // An item = (pixel, channel pair): eight pixels per wave trip, their 16 channels 64 contiguous bytes each; SU trips are
        // requested before the first value is touched (a value looked at right behind its load costs a full memory latency).
        constexpr int SU = 8;
        if (PSEG_DIAG && (a.dbg & 1)) {                 // timing ablation (diagnostic build): no staging loads
            for (int i = tid; i < npx * XCP; i += 256) xt[i] = 0.0f;
        } else if (pairs && !a.mask) {
            // the common form (forward layers, data gradients without a ReLU mask): no mask values to keep in flight
            const int sp = lane >> 3, c2 = (lane & 7) * 2;
            const int ch = cb + c2;
            const bool chok = ch < Cin;
            const bool second = ch >= a.C0;
            const float* const sb = second ? a.src1 : a.src0;
            const int C = second ? a.C1 : a.C0, chl = second ? ch - a.C0 : ch, up = second ? a.up1 : a.up0;
            const int Ws = a.Win >> up;
            const int ngrp = (npx + 7) >> 3;
            for (int g0 = wave; g0 < ngrp; g0 += 4 * SU) {
                float2 v[SU];
                int dsto[SU];
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    const int grp = g0 + 4 * u, p = grp * 8 + sp;
                    const bool valid = grp < ngrp && p < npx;
                    const int r = (int)(((unsigned)p * inv_twh) >> 20), c = p - r * TWH;
                    const int iy = iy0 + r, ix = ix0 + c;
                    dsto[u] = valid ? p * XCP + c2 : -1;
                    v[u] = make_float2(0.0f, 0.0f);
                    if (valid && chok && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win)
                        v[u] = *(const float2*)(sb + ((size_t)(iy >> up) * Ws + (ix >> up)) * C + chl);
                }
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    float2 x = v[u];
                    if (a.in_relu) { x.x = x.x > 0.0f ? x.x : 0.0f; x.y = x.y > 0.0f ? x.y : 0.0f; }
                    if (dsto[u] >= 0) *(float2*)(xt + dsto[u]) = x;
                }
            }
        } else if (pairs) {
            const int sp = lane >> 3, c2 = (lane & 7) * 2;
            const int ch = cb + c2;
            const bool chok = ch < Cin;
            const bool second = ch >= a.C0;
            const float* const sb = second ? a.src1 : a.src0;
            const int C = second ? a.C1 : a.C0, chl = second ? ch - a.C0 : ch, up = second ? a.up1 : a.up0;
            const int Ws = a.Win >> up;
            const float* const mb = second ? nullptr : a.mask;
            const int ngrp = (npx + 7) >> 3;
            constexpr int SM = 4;
            for (int g0 = wave; g0 < ngrp; g0 += 4 * SM) {
                float2 v[SM], mv[SM];
                int dsto[SM];
#pragma unroll
                for (int u = 0; u < SM; ++u) {
                    const int grp = g0 + 4 * u, p = grp * 8 + sp;
                    const bool valid = grp < ngrp && p < npx;
                    const int r = (int)(((unsigned)p * inv_twh) >> 20), c = p - r * TWH;
                    const int iy = iy0 + r, ix = ix0 + c;
                    dsto[u] = valid ? p * XCP + c2 : -1;
                    v[u] = make_float2(0.0f, 0.0f);
                    mv[u] = make_float2(1.0f, 1.0f);
                    if (valid && chok && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) {
                        const size_t o = ((size_t)(iy >> up) * Ws + (ix >> up)) * C + chl;
                        v[u] = *(const float2*)(sb + o);
                        if (mb) mv[u] = *(const float2*)(mb + o);
                    }
                }
#pragma unroll
                for (int u = 0; u < SM; ++u) {
                    float2 x = v[u];
                    if (a.in_relu) { x.x = x.x > 0.0f ? x.x : 0.0f; x.y = x.y > 0.0f ? x.y : 0.0f; }
                    x.x = mv[u].x > 0.0f ? x.x : 0.0f;
                    x.y = mv[u].y > 0.0f ? x.y : 0.0f;
                    if (dsto[u] >= 0) *(float2*)(xt + dsto[u]) = x;
                }
            }
        } else {
            const int sp = lane >> 4, c1 = lane & 15;
            const int ch = cb + c1;
            const bool chok = ch < Cin;
            const bool second = ch >= a.C0;
            const float* const sb = second ? a.src1 : a.src0;
            const int C = second ? a.C1 : a.C0, chl = second ? ch - a.C0 : ch, up = second ? a.up1 : a.up0;
            const int Ws = a.Win >> up;
            const float* const mb = second ? nullptr : a.mask;
            const int ngrp = (npx + 3) >> 2;
            for (int g0 = wave; g0 < ngrp; g0 += 4 * SU) {
                float v[SU], mv[SU];
                int dsto[SU];
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    const int grp = g0 + 4 * u, p = grp * 4 + sp;
                    const bool valid = grp < ngrp && p < npx;
                    const int r = (int)(((unsigned)p * inv_twh) >> 20), c = p - r * TWH;
                    const int iy = iy0 + r, ix = ix0 + c;
                    dsto[u] = valid ? p * XCP + c1 : -1;
                    v[u] = 0.0f;
                    mv[u] = 1.0f;
                    if (valid && chok && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) {
                        const size_t o = ((size_t)(iy >> up) * Ws + (ix >> up)) * C + chl;
                        v[u] = sb[o];
                        if (mb) mv[u] = mb[o];
                    }
                }
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    float x = v[u];
                    if (a.in_relu) x = x > 0.0f ? x : 0.0f;
                    x = mv[u] > 0.0f ? x : 0.0f;
                    if (dsto[u] >= 0) xt[dsto[u]] = x;
                }
            }
        }
        __syncthreads();

        // ---- the slab's k-steps: (ky, kx, four channels).  The pipeline unit is a TAP: the (up to) four k-steps of a tap are
        // requested while the MFMAs of the tap before it run (two register sets).  No vector ALU instruction per fragment:
        //   * pixel fragments: ds_read_b32 with the k-step's channel offset as the instruction's immediate; the per-lane
        //     base address moves once per tap (MT adds per 4 x MT x NT MFMAs);
        //   * weight fragments: buffer loads -- per-lane byte offset fixed for the whole kernel (voff), the (tap, slab,
        //     k-step) part in the scalar offset; lanes without a weight (cout padding) carry an out-of-range offset, for
        //     which the hardware returns 0, and the channel padding of the last slab needs no select at all: its x is
        //     the slab's zero fill, and 0 * (a finite neighbouring weight, or the 0 behind the buffer's end) adds nothing.
        // (The first version computed a 64-bit address and an exec-masked select per weight load and a shift-add per LDS
        // read: ~22 vector ALU instructions per 8 MFMAs.  Vector ALU and matrix instructions share a SIMD's issue port:
        // with the fragment loads switched off that build ran 1131 instead of 1430 us on conv2 -- tools/ab_f32.sh.)
        (void)cn;
        const int KHW = a.deconv4 ? 1 : a.KH * a.KW;
        const int KWe = a.deconv4 ? 1 : a.KW;
        int kx_ = 0, toff = 0;                                 // wave-uniform walk state: LDS float offset of the tap ...
        unsigned wso = (unsigned)(cb * a.Cout) * 4u;            // ... and byte offset of (tap, slab) in the weight buffer
        const unsigned wstep = (unsigned)(Cin * a.Cout) * 4u, kstep = (unsigned)(4 * a.Cout) * 4u;
        float xf[4][MT], wf[4][NT];                             // fragments of the tap's (up to) four k-steps
        const int ntap = (PSEG_DIAG && (a.dbg & 4)) ? 0 : KHW;  // dbg & 4: no k-loop
        // NKS = k-steps per tap, a compile-time constant inside the loop (straight-line tap bodies: with a run-time count
        // the per-k-step branches cut the body into basic blocks and the compiler issued each tap's loads right in front
        // of its own MFMAs).  ONE register set, one tap of lead: k-step s of tap T + 1 is requested into the registers of
        // k-step s of tap T as soon as that step's MFMAs have been issued.
        auto run_ksteps = [&](auto nks_c) {
            constexpr int NKS = decltype(nks_c)::value;
            const float* xp[MT];
            auto point = [&]() {                                // fragment pointers / weight offset of the tap the walk is at
#pragma unroll
                for (int m = 0; m < MT; ++m) xp[m] = xt + xbase[m] + toff;
            };
            auto advance = [&]() {
                toff += XCP;
                wso += wstep;
                if (++kx_ == KWe) { kx_ = 0; toff += (TWH - KWe) * XCP; }
            };
            auto request = [&](int s4, unsigned wo) {           // k-step s4 of the tap `xp` / `wo` point at
                if (PSEG_DIAG && (a.dbg & 8)) {                 // timing ablation: no weight loads
#pragma unroll
                    for (int t = 0; t < NT; ++t) wf[s4][t] = (float)(wo + t);
                } else {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        wf[s4][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrsrc, voff[t], wo + (unsigned)s4 * kstep, 0));
                }
                if (PSEG_DIAG && (a.dbg & 16)) {                // timing ablation: no LDS fragment reads
#pragma unroll
                    for (int m = 0; m < MT; ++m) xf[s4][m] = (float)(wo + m);
                } else {
#pragma unroll
                    for (int m = 0; m < MT; ++m) xf[s4][m] = xp[m][4 * s4];
                }
            };
            auto mma = [&](int s4) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s4][t], xf[s4][m], acc[m][t], 0, 0, 0);
            };
            if (ntap <= 0) return;
            point();
#pragma unroll
            for (int s4 = 0; s4 < NKS; ++s4) request(s4, wso);
            for (int tap = 0; tap + 1 < ntap; ++tap) {
                advance();
                point();                                         // the NEXT tap
#pragma unroll
                for (int s4 = 0; s4 < NKS; ++s4) {
                    mma(s4);
                    request(s4, wso);
                }
            }
#pragma unroll
            for (int s4 = 0; s4 < NKS; ++s4) mma(s4);
        };
        run_ksteps(nks_tag);

        // ---- the left-over channels' tile(s): the same walk over KH x (KW + DX - 1) taps of the shifted kernel
        if constexpr (REM != 0) {
            constexpr int NKS = decltype(nks_tag)::value;
            int kxr = 0, toffr = 0;
            unsigned wsr = (unsigned)(cb * 16) * 4u;
            const unsigned wstepr = (unsigned)(Cin * 16) * 4u, kstepr = 4u * 16u * 4u;
            const int ntapr = (PSEG_DIAG && (a.dbg & 4)) ? 0 : a.KH * KWR;
            float xq[4][RT], wq[4];
            const float* xpr[RT];
            auto pointr = [&]() {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) xpr[rt] = xt + xrbase[rt] + toffr;
            };
            auto advancer = [&]() {
                toffr += XCP;
                wsr += wstepr;
                if (++kxr == KWR) { kxr = 0; toffr += (TWH - KWR) * XCP; }
            };
            auto requestr = [&](int s4, unsigned wo) {
                wq[s4] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrrsrc, voffr, wo + (unsigned)s4 * kstepr, 0));
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) xq[s4][rt] = xpr[rt][4 * s4];
            };
            auto mmar = [&](int s4) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) accr[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[s4], xq[s4][rt], accr[rt], 0, 0, 0);
            };
            if (ntapr > 0) {
                pointr();
#pragma unroll
                for (int s4 = 0; s4 < NKS; ++s4) requestr(s4, wsr);
                for (int tap = 0; tap + 1 < ntapr; ++tap) {
                    advancer();
                    pointr();
#pragma unroll
                    for (int s4 = 0; s4 < NKS; ++s4) {
                        mmar(s4);
                        requestr(s4, wsr);
                    }
                }
#pragma unroll
                for (int s4 = 0; s4 < NKS; ++s4) mmar(s4);
            }
        }
    };
    const int nfull = (TAILK == 0) ? (Cin + XCB - 1) / XCB : Cin / XCB;     // (TAILK == 0: a last slab of 13..15 channels also takes four k-steps)
    for (int sb = 0; sb < nfull; ++sb) process_slab(sb * XCB, std::integral_constant<int, 4>{});
    if constexpr (TAILK != 0) process_slab(nfull * XCB, std::integral_constant<int, TAILK>{});

    // ---- epilogue: acc + bias (+ add), ReLU; lane owns n = 4g..4g+3 of pixel p16 in every tile.  The lane's four values are
    // consecutive output channels of one pixel (of one sub-pixel, for the transposed GEMM: Cout % 4 == 0 keeps a quad inside
    // its sub-pixel): one 16-byte (or two 8-byte, Cout even) store instead of four 4-byte ones.
    const int osy = a.out_sy ? a.out_sy : 1, osx = a.out_sx ? a.out_sx : 1;
    const int pitch = a.dst_pitch ? a.dst_pitch : a.Wout;
    const int vecw = (a.Cout & 3) == 0 ? 4 : ((a.Cout & 1) == 0 ? 2 : 1);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int y = oy0 + wave * RW + (m >> 1), x = ox0 + (m & 1) * 16 + p16;
        if (y >= a.Hout || x >= a.Wout || (PSEG_DIAG && (a.dbg & 2) && acc[m][0][0] != 123.456f)) continue;   // dbg & 2: no stores
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n0 = co_base + t * 16 + 4 * g;
            if (n0 >= Ntot) continue;
            float v[4];
            size_t off[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + r;
                const int nn = n < Ntot ? n : n0;                 // (values past the layer are never stored)
                const int ab = a.deconv4 ? nn / a.Cout : 0;
                const int co = nn - ab * a.Cout;
                const size_t opix = a.deconv4 ? (size_t)(2 * y + (ab >> 1)) * pitch + (size_t)(2 * x + (ab & 1))
                                              : (size_t)(y * osy + a.out_oy) * pitch + (size_t)(x * osx + a.out_ox);
                off[r] = opix * a.Cout + co;
                v[r] = a.bias ? acc[m][t][r] + a.bias[co] : acc[m][t][r];
            }
            if (a.add) {
                if (vecw == 4 && n0 + 3 < Ntot) {
                    const float4 ad = *(const float4*)(a.add + off[0]);
                    v[0] = v[0] + ad.x; v[1] = v[1] + ad.y; v[2] = v[2] + ad.z; v[3] = v[3] + ad.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n0 + r < Ntot) v[r] = v[r] + a.add[off[r]];
                }
            }
            if (a.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.0f ? v[r] : 0.0f;
            }
            if (vecw == 4 && n0 + 3 < Ntot) {
                *(float4*)(a.dst + off[0]) = make_float4(v[0], v[1], v[2], v[3]);
            } else if (vecw >= 2) {
                if (n0 + 1 < Ntot) *(float2*)(a.dst + off[0]) = make_float2(v[0], v[1]);
                else a.dst[off[0]] = v[0];
                if (n0 + 3 < Ntot) *(float2*)(a.dst + off[2]) = make_float2(v[2], v[3]);
                else if (n0 + 2 < Ntot) a.dst[off[2]] = v[2];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < Ntot) a.dst[off[r]] = v[r];
            }
        }
    }
    if constexpr (REM != 0) {
        // left-over channels: lane (p16, g) holds rows 4g .. 4g+3 = channels 16 NT + j0 .. + 3 of pixel DX * column + dx
        const int dx = (4 * g) / REM, j0 = (4 * g) % REM;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int y = REM == 8 ? oy0 + wave * RW + rt : oy0 + wave * RW + rt * 2 + (p16 >> 3);
            const int x = REM == 8 ? ox0 + 2 * p16 + dx : ox0 + 4 * (p16 & 7) + dx;
            if (y >= a.Hout || x >= a.Wout || (PSEG_DIAG && (a.dbg & 2) && accr[rt][0] != 123.456f)) continue;
            const int n0 = NT * 16 + j0;
            const size_t off0 = ((size_t)y * pitch + (size_t)x) * a.Cout + n0;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = a.bias ? accr[rt][r] + a.bias[n0 + r] : accr[rt][r];
            if (a.add) {
                const float4 ad = *(const float4*)(a.add + off0);
                v[0] = v[0] + ad.x; v[1] = v[1] + ad.y; v[2] = v[2] + ad.z; v[3] = v[3] + ad.w;
            }
            if (a.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.0f ? v[r] : 0.0f;
            }
            *(float4*)(a.dst + off0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// wr[ky][kxp][ci][dx * rem + j] = w[ky][kxp - dx][ci][cmain + j] (0 when kxp - dx is not a tap): the left-over channels'
// kernel as DX shifted copies, one per pixel of the group a tile column stands for (see conv_xb_kernel, REM)
__global__ void wrem_kernel(const float* w, int KH, int KW, int Cin, int Cout, int cmain, int rem, float* wr) {
    const int dxn = 16 / rem, KWR = KW + dxn - 1;
    const int n = KH * KWR * Cin * 16;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int row = i & 15, ci = (i >> 4) % Cin, t = (i >> 4) / Cin;
        const int kxp = t % KWR, ky = t / KWR;
        const int dx = row / rem, j = row - dx * rem, kx = kxp - dx;
        wr[i] = (kx >= 0 && kx < KW) ? w[((size_t)(ky * KW + kx) * Cin + ci) * Cout + cmain + j] : 0.0f;
    }
}

size_t wrem_bytes_for(int KH, int KW, int Cin, int Cout) {
    const int rem = Cout % 16, ntm = Cout / 16;
    if (!((rem == 4 || rem == 8) && (ntm == 1 || ntm == 2))) return 0;
    return (size_t)KH * (KW + 16 / rem - 1) * Cin * 16 * 4;
}

// ---- launch: choose, prepare, launch -----------------------------------------------------------------------------------------
// What the matrix-core route does with one layer: a function of the ConvArgs (and the PSEG_EXACT_* plan switches) alone.
enum XFamily { XF_NONE, XF_FLAT, XF_BLOCKED, XF_BLOCKED_REM };   // not a layer for these kernels / conv_exact_mfma_kernel / conv_xb_kernel / ... with REM
struct XChoice {
    XFamily family = XF_NONE;
    int MT = 0, NT = 0, nblk = 0;   // pixel tiles per wave, cout tiles per workgroup, cout blocks (grid.y)
    int tailk = 0;                  // k-steps of the last channel slab when it has at most 12 channels, else 0 (a full slab's loop)
    int rem = 0, ntm = 0;           // XF_BLOCKED_REM: the left-over output channels (4 or 8) and the full cout tiles in front of them
    int THH = 0, TWH = 0, Cp = 0;   // halo tile rows, columns; XF_FLAT: its channel pitch
    size_t lds = 0;
    dim3 grid;
};

// first layers (fewer than 8 input channels): K flattened across taps (one slab: the oracle's order), all-channel tile
static XChoice choose_flat(const ConvArgs& a, int Cin, int ntall) {
    XChoice c;
    if (a.deconv4) return c;
    c.Cp = std::max(Cin, 2);
    while (c.Cp % 4 != 2) ++c.Cp;
    c.MT = 4;
    c.THH = (8 - 1) * a.stride + a.KH;
    c.TWH = (XTW - 1) * a.stride + a.KW;
    c.lds = (size_t)c.THH * c.TWH * c.Cp * 4;
    if (c.lds > 150 * 1024) return c;
    c.NT = ntall <= 4 ? ntall : (ntall == 5 ? 5 : 4);
    c.nblk = cdiv(ntall, c.NT);
    c.grid = dim3(cdiv(a.Wout, XTW) * cdiv(a.Hout, 8), c.nblk);
    c.family = XF_FLAT;
    return c;
}

// Cout tiles per workgroup and cout blocks of the blocked chain.  At most four tiles (64 accumulator registers), split evenly over
// the cout blocks; small layers (1/8-resolution: 192 tiles for 256 CUs) split further until the chip is full -- restaging a 31 KB
// slab per cout block costs little next to 25 taps of float32 MFMAs.
static void choose_cout_split(int ntall, int tiles, int* NT_out, int* nblk_out) {
    int nblk = cdiv(ntall, 4), NT = cdiv(ntall, nblk);
    while (NT > 1 && tiles * nblk < 1024) { --NT; nblk = cdiv(ntall, NT); }
    NT = cdiv(ntall, nblk);                    // even split: 4 tiles over 2 blocks are 2 + 2, not 3 + 1 (idle MFMAs on the empty tiles)
    // quarter-resolution layers of a 2048x1536 page (768 tiles): the chip holds 768 three- or four-tile workgroups at once (three
    // waves per SIMD), so one cout block beats two -- 3 tiles cannot split evenly (2 + 1 with a dead tile: deconv3 612 -> 461 us),
    // 4 tiles as 2 + 2 stage every slab twice (conv5 / conv6 226 -> 218, 326 -> 308 us).
    if ((ntall == 3 || ntall == 4) && nblk == 2 && tiles >= 512) { NT = ntall; nblk = 1; }
    *NT_out = NT;
    *nblk_out = nblk;
}

// left-over output channels (Cout = 16 k + 4 or + 8) as shifted-pixel tiles instead of a padded cout tile: 8-row tiles of a plain
// stride-1 layer with at least 512 tiles (PSEG_EXACT_REM_ANY: any size; PSEG_EXACT_NO_REM: never) whose caller lent a buffer for
// the shifted kernel copies
static bool rem_form_pays(const ConvArgs& a, int Cin, int MT, int tiles) {
    const int rem = a.Cout % 16, ntm = a.Cout / 16;
    return (rem == 4 || rem == 8) && (ntm == 1 || ntm == 2) && MT == 4 && !a.deconv4 && a.stride == 1 && !a.out_sy && !a.out_sx &&
           (tiles >= 512 || PSEG_KNOB("PSEG_EXACT_REM_ANY")) && !PSEG_KNOB("PSEG_EXACT_NO_REM") && a.wrem_buf &&
           a.wrem_cap >= wrem_bytes_for(a.KH, a.KW, Cin, a.Cout);
}

// blocked chain: 8-row tiles unless the 16-channel slab of a strided layer's halo tile would leave fewer than three workgroups per
// CU (then 4-row tiles)
static XChoice choose_blocked(const ConvArgs& a, int Cin, int ntall) {
    XChoice c;
    c.TWH = (XTW - 1) * a.stride + a.KW;
    auto lds_of = [&](int mt) { return (size_t)((4 * (mt / 2) - 1) * a.stride + a.KH) * c.TWH * XCP * 4; };
    c.MT = (lds_of(4) <= 52 * 1024) ? 4 : 2;
    c.lds = lds_of(c.MT);
    if (c.lds > 150 * 1024) return c;
    const int TH = 4 * (c.MT / 2);
    c.THH = (TH - 1) * a.stride + a.KH;
    const int tiles = cdiv(a.Wout, XTW) * cdiv(a.Hout, TH);
    const int tail_ch = Cin % XCB;                              // channels of the last slab (0: a full one)
    c.tailk = (tail_ch == 0 || tail_ch > 12) ? 0 : (tail_ch + 3) / 4;
    if (rem_form_pays(a, Cin, c.MT, tiles)) {
        c.family = XF_BLOCKED_REM;
        c.rem = a.Cout % 16;
        c.ntm = c.NT = a.Cout / 16;
        c.nblk = 1;
    } else {
        c.family = XF_BLOCKED;
        choose_cout_split(ntall, tiles, &c.NT, &c.nblk);
    }
    c.grid = dim3(tiles, c.nblk);
    return c;
}

static XChoice choose_exact_mfma(const ConvArgs& a) {
    const int Cin = a.C0 + a.C1;
    if (Cin < 1 || a.Cout < 1 || a.KH != a.KW) return XChoice();
    const int Ntot = a.deconv4 ? 4 * a.Cout : a.Cout;
    if (Ntot < 8) return XChoice();            // a handful of couts (logits): the 1x1 / scalar kernels waste less
    return Cin < 8 ? choose_flat(a, Cin, cdiv(Ntot, 16)) : choose_blocked(a, Cin, cdiv(Ntot, 16));
}

// The shifted copies of the left-over channels' kernel live in a buffer of the caller's (the op's, beside its kernel; the train
// step's scratch for the flipped kernels of the data gradients) and are rebuilt only when the weights behind them changed -- no
// allocation, no pool, nothing but kernels on `st`.  No validity flag: rebuilt on every launch.
static void prepare_wrem(const ConvArgs& a, const XChoice& c, hipStream_t st) {
    if (a.wrem_valid && *a.wrem_valid) return;
    const size_t wbytes = wrem_bytes_for(a.KH, a.KW, a.C0 + a.C1, a.Cout);
    wrem_kernel<<<(int)std::min<size_t>((wbytes / 4 + 255) / 256, 1024), 256, 0, st>>>(a.w, a.KH, a.KW, a.C0 + a.C1, a.Cout, c.ntm * 16, c.rem, a.wrem_buf);
    if (a.wrem_valid) *a.wrem_valid = true;
}

// the instance tables
static int launch_flat(const ConvArgs& a, const XChoice& c, hipStream_t st) {
    const int Cin = a.C0 + a.C1;
    switch (c.NT) {
        case 1: return launch_lds<conv_exact_mfma_kernel<4, 1, true>>(a, c.grid, 256, c.lds, -1, st, c.Cp, c.THH, c.TWH, Cin);
        case 2: return launch_lds<conv_exact_mfma_kernel<4, 2, true>>(a, c.grid, 256, c.lds, -1, st, c.Cp, c.THH, c.TWH, Cin);
        case 3: return launch_lds<conv_exact_mfma_kernel<4, 3, true>>(a, c.grid, 256, c.lds, -1, st, c.Cp, c.THH, c.TWH, Cin);
        case 4: return launch_lds<conv_exact_mfma_kernel<4, 4, true>>(a, c.grid, 256, c.lds, -1, st, c.Cp, c.THH, c.TWH, Cin);
        default: return launch_lds<conv_exact_mfma_kernel<4, 5, true>>(a, c.grid, 256, c.lds, -1, st, c.Cp, c.THH, c.TWH, Cin);
    }
}
template <int MT, int NT, int REM = 0>
static int launch_xb(const ConvArgs& a, const XChoice& c, hipStream_t st) {
    const unsigned inv_twh = (1u << 20) / (unsigned)c.TWH + 1u;
    switch (c.tailk) {
        case 0: return launch_lds<conv_xb_kernel<MT, NT, 0, REM>>(a, c.grid, 256, c.lds, -1, st, c.THH, c.TWH, inv_twh);
        case 1: return launch_lds<conv_xb_kernel<MT, NT, 1, REM>>(a, c.grid, 256, c.lds, -1, st, c.THH, c.TWH, inv_twh);
        case 2: return launch_lds<conv_xb_kernel<MT, NT, 2, REM>>(a, c.grid, 256, c.lds, -1, st, c.THH, c.TWH, inv_twh);
        default: return launch_lds<conv_xb_kernel<MT, NT, 3, REM>>(a, c.grid, 256, c.lds, -1, st, c.THH, c.TWH, inv_twh);
    }
}
static int launch_blocked(const ConvArgs& a, const XChoice& c, hipStream_t st) {
    if (c.family == XF_BLOCKED_REM) {
        if (c.ntm == 1) return c.rem == 4 ? launch_xb<4, 1, 4>(a, c, st) : launch_xb<4, 1, 8>(a, c, st);
        return c.rem == 4 ? launch_xb<4, 2, 4>(a, c, st) : launch_xb<4, 2, 8>(a, c, st);
    }
    switch (c.MT * 10 + c.NT) {
        case 41: return launch_xb<4, 1>(a, c, st);
        case 42: return launch_xb<4, 2>(a, c, st);
        case 43: return launch_xb<4, 3>(a, c, st);
        case 44: return launch_xb<4, 4>(a, c, st);
        case 21: return launch_xb<2, 1>(a, c, st);
        case 22: return launch_xb<2, 2>(a, c, st);
        case 23: return launch_xb<2, 3>(a, c, st);
        case 24: return launch_xb<2, 4>(a, c, st);
    }
    return ROUTE_NO;
}

// PSEG_OK when the layer was launched on a matrix-core kernel, ROUTE_NO when it is not one for them (the caller falls back to the
// 1x1 / scalar kernels: a handful of output channels), an error otherwise.
int launch_conv_exact_mfma(const ConvArgs& a_in, hipStream_t st) {
    const XChoice c = choose_exact_mfma(a_in);
    if (c.family == XF_NONE) return ROUTE_NO;
    if (c.family == XF_BLOCKED_REM) prepare_wrem(a_in, c, st);
    ConvArgs a = a_in;                         // the kernel's copy: what the choice says, nothing else, differs from the caller's
    if (const char* dv = PSEG_DIAG_KNOB("PSEG_XM_DBG")) a.dbg = atoi(dv);   // wrong-result timing switches: diagnostic build only
    if (c.family == XF_BLOCKED_REM) a.wrem = a.wrem_buf;
    return c.family == XF_FLAT ? launch_flat(a, c, st) : launch_blocked(a, c, st);
}

}  // namespace pseg
