// The embedding CNN on the device: the reference's ESPNetv2 segmentation net EESPNet_Seg(classes = C, s = 1) in eval mode: the
// kernels, the weight arena, the workspace and the launch sequence, shared by the two sources that hold the entry points:
// espnet.hip (tmpnn_espnet_arena_floats, tmpnn_espnet_ws_bytes, tmpnn_espnet_fwd, and for single pixels
// tmpnn_espnet_centres_ws_bytes, tmpnn_espnet_trunk, tmpnn_espnet_centres) and espnet_train.hip (the training forward, which is
// this forward with the pre-activations of the trained layers kept).  include/tmpnn.h; host definition:
// trackmpnn_amd.espnet.espnet_host.  float32 NCHW throughout; every BatchNorm arrives folded into a per-channel scale and
// shift, every PReLU as per-channel slopes (a layer without an activation carries slopes of 1, without a norm scale 1 shift 0).
//
// k_esp_pool      3x3 stride-2 pad-1 average that counts the padding (every window / 9): the image pyramid, the PSP chain, and
//                 (ACT) the pooled half of a DownSampler, which adds what the reinforcement kernel left in the output and
//                 applies the block's PReLU in place.
// k_esp_level1    3x3 stride-2 conv 3 -> 32 + scale/shift + PReLU: a thread per output pixel keeps the 27 inputs and walks
//                 the 32 channels; the weights are wave-uniform reads.
// k_esp_reinf     input reinforcement of a DownSampler on the pyramid image of its level: 3x3 conv 3 -> 3 + norm + PReLU in
//                 registers, then the 1x1 conv 3 -> nout + norm written into all nout channels of the DownSampler's output
//                 (32 channels a thread; grid y walks the channel tiles and every tile recomputes the three values).
// k_esp_pw        grouped or dense pointwise conv: lanes along the pixels of a plane (coalesced NCHW rows), CO_T output
//                 channels of one group in registers (32 or 8: pw_wide), the input channels of the group walked in order; the weights are
//                 stored [k][cout], so a channel tile's weights for one k are CO_T contiguous floats at a wave-uniform
//                 address (scalar loads feeding the FMAs; no LDS staging is needed for them).  Two sources: channels
//                 [0, ca) from a, [ca, cin) from b -- both halves of a torch.cat read in place.  Epilogue: scale/shift,
//                 optional residual, PReLU.
// k_esp_dw        the EESP transform: a workgroup stages a tile of ONE reduced channel plus a halo of 4 (the largest dilation)
//                 in LDS, computes the four dilated depthwise 3x3 convs of stride S, adds them in the reference's order
//                 (out_k = conv_k + out_{k-1}), applies the norm and PReLU after the concat and writes channels
//                 c, n + c, 2n + c, 3n + c.
// k_esp_bilinear  align_corners=True resize; VEC = 4 writes 16 bytes a lane (the x2 steps, the final one a pure streaming
//                 write of T C H W floats); a thread keeps its columns' indices and weights, and the blended source rows, for
//                 4 output rows, and reads the four source columns its 4 outputs touch once per source row.  Source coordinates are exact: o (in - 1) / (out - 1) by integer division, the
//                 weight is remainder / (out - 1) rounded once; an axis of one input or output pixel reads index 0.
// k_esp_psp_up    one PSP stage behind its pooled map: depthwise 3x3 (no norm) evaluated at the four bilinear corners and
//                 blended into the stage's slot of the 5 x 128 channel buffer the PSP projection reads.
// k_esp_centres   the decoder tail behind the 1/8-size map at single pixels, a workgroup per pixel (described at the kernel).
//
// No atomics: every output element has one owner thread and every sum a fixed order that depends on the shapes alone, never
// on T (an image is grid z), so results are bitwise reproducible and image i of a batch equals the same image alone.
//
// Bounds.  Every kernel guards its pixel index against the plane; tap reads test the coordinate against the map; channel
// tiles of k_esp_pw clamp the weight column to the group's last channel and guard the store.  Plane and per-image sizes are
// held below 2^31 by the host check (C H W < 2^31); batch offsets are size_t.
#pragma once
#include "common.h"

#include <algorithm>
#include <utility>

using namespace tmpnn;

namespace {

constexpr int ESP_THREADS = 256;
constexpr int ESP_HALO = 4;                  // largest dilation of an EESP branch
constexpr int ESP_TH = 8, ESP_TW = 64;       // output tile of k_esp_dw
constexpr int ESP_PSP = 128;                 // channels of the level-3 merge and of every PSP stage
constexpr int ESP_REINF_CO = 32;             // output channels a thread of k_esp_reinf writes (grid y walks the rest)
constexpr int ESP_UP_ROWS = 4;               // output rows a thread of k_esp_bilinear writes

__device__ __forceinline__ float prelu(float v, float a) { return v > 0.0f ? v : a * v; }

// The forms of the decoder tail's arithmetic, written out so that the dense kernels and k_esp_centres round alike (this file is
// compiled with contraction on, and which product of (1 - l) p + l q the compiler fuses is its choice per site).
// esp_norm      the epilogue of a pointwise conv: one fused multiply-add.
// esp_lerp_fma  fma(1 - l, p, l q): the vertical blend of an x2 resize, and its row blend in columns 0 .. 2 of every four.
// esp_lerp_sep  (1 - l) p + l q with both products rounded: the row blend in column 3 of every four.  That split is what the
//               library has computed since the resize kernel took four columns a thread; the maps keep those bits.
__device__ __forceinline__ float esp_norm(float acc, float scale, float shift) { return fmaf(acc, scale, shift); }
__device__ __forceinline__ float esp_lerp_fma(float l, float p, float q) { return fmaf(1.0f - l, p, l * q); }
__device__ __forceinline__ float esp_lerp_sep(float l, float p, float q) {
#pragma clang fp contract(off)
    const float a = (1.0f - l) * p, b = l * q;
    return a + b;
}
// the row blend of output column x of an x2 resize (k_esp_bilinear<4>: a thread's columns are x0 .. x0 + 3, x0 a multiple of 4)
__device__ __forceinline__ float esp_lerp_col(int x, float l, float p, float q) {
    return (x & 3) == 3 ? esp_lerp_sep(l, p, q) : esp_lerp_fma(l, p, q);
}

template <bool ACT>
__global__ __launch_bounds__(ESP_THREADS) void k_esp_pool(const float* __restrict__ in, size_t in_bs, int h, int w, float* out,
                                                          size_t out_bs, int ho, int wo, const float* __restrict__ slope) {
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx >= ho * wo) return;
    const int c = blockIdx.y, y = idx / wo, x = idx - y * wo;
    const float* p = in + (size_t)blockIdx.z * in_bs + (size_t)c * h * w;
    float s = 0.0f;
#pragma unroll
    for (int a = -1; a <= 1; ++a) {
        const int iy = 2 * y + a;
#pragma unroll
        for (int b = -1; b <= 1; ++b) {
            const int ix = 2 * x + b;
            if (iy >= 0 && iy < h && ix >= 0 && ix < w) s += p[iy * w + ix];
        }
    }
    float v = s / 9.0f;
    float* o = out + (size_t)blockIdx.z * out_bs + (size_t)c * ho * wo + idx;
    if (ACT) v = prelu(v + *o, slope[c]);
    *o = v;
}

// wgt: [32][3][3][3] | scale [32] | shift [32] | slope [32]
__global__ __launch_bounds__(ESP_THREADS) void k_esp_level1(const float* __restrict__ img, int h, int w, const float* __restrict__ wgt,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ slope, float* __restrict__ out, int ho, int wo) {
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx >= ho * wo) return;
    const int y = idx / wo, x = idx - y * wo;
    const float* p = img + (size_t)blockIdx.z * 3 * h * w;
    float v[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int iy = 2 * y - 1 + a, ix = 2 * x - 1 + b;
                v[(c * 3 + a) * 3 + b] = (iy >= 0 && iy < h && ix >= 0 && ix < w) ? p[((size_t)c * h + iy) * w + ix] : 0.0f;
            }
    float* o = out + (size_t)blockIdx.z * 32 * ho * wo + idx;
    for (int co = 0; co < 32; ++co) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 27; ++k) s = fmaf(v[k], wgt[co * 27 + k], s);
        o[(size_t)co * ho * wo] = prelu(s * scale[co] + shift[co], slope[co]);
    }
}

// w3: [3][3][3][3]; s3, t3, a3: [3]; w1t: [3][nout]; scale, shift: [nout].  img: the pyramid image of this level [T][3][h][w].
__global__ __launch_bounds__(ESP_THREADS) void k_esp_reinf(const float* __restrict__ img, int h, int w, const float* __restrict__ w3,
                                                           const float* __restrict__ s3, const float* __restrict__ t3,
                                                           const float* __restrict__ a3, const float* __restrict__ w1t,
                                                           const float* __restrict__ scale, const float* __restrict__ shift, int nout,
                                                           float* __restrict__ out) {
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    const int P = h * w;
    if (idx >= P) return;
    const int y = idx / w, x = idx - y * w;
    const float* p = img + (size_t)blockIdx.z * 3 * P;
    float v[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int iy = y - 1 + a, ix = x - 1 + b;
                v[(c * 3 + a) * 3 + b] = (iy >= 0 && iy < h && ix >= 0 && ix < w) ? p[((size_t)c * h + iy) * w + ix] : 0.0f;
            }
    float m[3];
#pragma unroll
    for (int co = 0; co < 3; ++co) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 27; ++k) s = fmaf(v[k], w3[co * 27 + k], s);
        m[co] = prelu(s * s3[co] + t3[co], a3[co]);
    }
    float* o = out + (size_t)blockIdx.z * nout * P + idx;
    const int c0 = blockIdx.y * ESP_REINF_CO, c1 = min(nout, c0 + ESP_REINF_CO);
    for (int co = c0; co < c1; ++co) {
        float s = m[0] * w1t[co];
        s = fmaf(m[1], w1t[nout + co], s);
        s = fmaf(m[2], w1t[2 * nout + co], s);
        o[(size_t)co * P] = s * scale[co] + shift[co];
    }
}

// out[t][co][pix] = prelu((sum_k x[t][g kg + k][pix] wt[k][co]) scale[co] + shift[co] (+ res[t][co][pix]), slope[co]); res may be
// `out` itself (each element is read and then written by its one owner), so neither carries __restrict__.
// SAVE (the training forward): the value in front of the PReLU goes to pre[t][co][pix] (batch stride pre_bs) as well.
template <int CO_T, int UNROLL, bool SAVE = false>
__global__ __launch_bounds__(ESP_THREADS) void k_esp_pw(const float* __restrict__ a, size_t a_bs, int ca, const float* __restrict__ b,
                                                        size_t b_bs, int cin, int cout, int groups, int P,
                                                        const float* __restrict__ wt, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ slope,
                                                        const float* res, size_t res_bs, float* out, size_t out_bs,
                                                        float* __restrict__ pre = nullptr, size_t pre_bs = 0) {
    const int pix = blockIdx.x * ESP_THREADS + threadIdx.x;
    const int kg = cin / groups, cpg = cout / groups;
    const int tiles = (cpg + CO_T - 1) / CO_T;
    const int g = blockIdx.y / tiles, tl = blockIdx.y - g * tiles;
    const int co0 = g * cpg + tl * CO_T;
    const int nco = min(CO_T, cpg - tl * CO_T);
    const size_t t = blockIdx.z;
    const bool live = pix < P;
    const int px = live ? pix : 0;               // an idle lane reads pixel 0 and stores nothing
    float acc[CO_T];
#pragma unroll
    for (int j = 0; j < CO_T; ++j) acc[j] = 0.0f;
    const float* w0 = wt + co0;
    if (nco == CO_T) {
#pragma unroll UNROLL
        for (int k = 0; k < kg; ++k) {
            const int ci = g * kg + k;
            const float* src = ci < ca ? a + t * a_bs + (size_t)ci * P : b + t * b_bs + (size_t)(ci - ca) * P;
            const float x = src[px];
            const float* wr = w0 + (size_t)k * cout;
#pragma unroll
            for (int j = 0; j < CO_T; ++j) acc[j] = fmaf(x, wr[j], acc[j]);
        }
    } else {
        for (int k = 0; k < kg; ++k) {
            const int ci = g * kg + k;
            const float* src = ci < ca ? a + t * a_bs + (size_t)ci * P : b + t * b_bs + (size_t)(ci - ca) * P;
            const float x = src[px];
            const float* wr = w0 + (size_t)k * cout;
#pragma unroll
            for (int j = 0; j < CO_T; ++j) acc[j] = fmaf(x, wr[min(j, nco - 1)], acc[j]);
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < CO_T; ++j) {
        if (j < nco) {
            const int co = co0 + j;
            float v = esp_norm(acc[j], scale[co], shift[co]);
            if (res) v += res[t * res_bs + (size_t)co * P + pix];
            if constexpr (SAVE) pre[t * pre_bs + (size_t)co * P + pix] = v;
            out[t * out_bs + (size_t)co * P + pix] = prelu(v, slope[co]);
        }
    }
}

// in [T][n][h][w] (one reduced channel per blockIdx.y); wdw [4][n][9]; scale, shift, slope [4n]; out [T][4n][ho][wo].
template <int S>
__global__ __launch_bounds__(ESP_THREADS) void k_esp_dw(const float* __restrict__ in, size_t in_bs, int n, int h, int w,
                                                        const float* __restrict__ wdw, int d0, int d1, int d2, int d3,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        const float* __restrict__ slope, float* __restrict__ out, size_t out_bs, int ho,
                                                        int wo, int tiles_x) {
    constexpr int IH = (ESP_TH - 1) * S + 1 + 2 * ESP_HALO, IW = (ESP_TW - 1) * S + 1 + 2 * ESP_HALO;
    __shared__ float tile[IH][IW + 1];
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int c = blockIdx.y;
    const int oy0 = ty * ESP_TH, ox0 = tx * ESP_TW;
    const int iy0 = oy0 * S - ESP_HALO, ix0 = ox0 * S - ESP_HALO;
    const float* p = in + (size_t)blockIdx.z * in_bs + (size_t)c * h * w;
    for (int i = threadIdx.x; i < IH * IW; i += ESP_THREADS) {
        const int r = i / IW, q = i - r * IW;
        const int gy = iy0 + r, gx = ix0 + q;
        tile[r][q] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? p[gy * w + gx] : 0.0f;
    }
    __syncthreads();
    const int dil[4] = {d0, d1, d2, d3};
    const int lx = threadIdx.x & (ESP_TW - 1), ly = threadIdx.x / ESP_TW;
    const int ox = ox0 + lx;
    float* o = out + (size_t)blockIdx.z * out_bs;
    for (int rr = ly; rr < ESP_TH; rr += ESP_THREADS / ESP_TW) {
        const int oy = oy0 + rr;
        if (oy >= ho || ox >= wo) continue;
        const int cy = rr * S + ESP_HALO, cx = lx * S + ESP_HALO;
        float run = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = dil[k];                                    // 1 .. ESP_HALO: the taps stay inside the staged tile
            const float* wk = wdw + ((size_t)k * n + c) * 9;
            float s = 0.0f;
#pragma unroll
            for (int u = -1; u <= 1; ++u)
#pragma unroll
                for (int v = -1; v <= 1; ++v) s = fmaf(wk[(u + 1) * 3 + (v + 1)], tile[cy + u * d][cx + v * d], s);
            run = k == 0 ? s : s + run;                              // out_k = conv_k + out_{k-1}
            const int co = k * n + c;
            o[((size_t)co * ho + oy) * wo + ox] = prelu(run * scale[co] + shift[co], slope[co]);
        }
    }
}

// source index and weight of output coordinate o on an axis resized n_in -> n_out with align_corners=True
__device__ __forceinline__ void esp_axis(int o, int n_in, int n_out, int& i0, int& i1, float& lam) {
    if (n_out <= 1 || n_in <= 1) {
        i0 = i1 = 0;
        lam = 0.0f;
        return;
    }
    const int num = o * (n_in - 1), den = n_out - 1;
    i0 = num / den;
    lam = (float)(num - i0 * den) / (float)den;
    i1 = min(i0 + 1, n_in - 1);
}

__device__ __forceinline__ float esp_sel4(const float (&p)[4], int i) { return i == 0 ? p[0] : i == 1 ? p[1] : i == 2 ? p[2] : p[3]; }

// one source row blended along x for the VEC output columns of a thread.  VEC = 4 (an exact x2 step): the eight taps lie in the
// four columns from xa[0] on -- a step is below 1/2, so xa[3] <= xa[0] + 2 -- which are read once and selected from.
template <int VEC>
__device__ __forceinline__ void esp_blend_row(const float* __restrict__ row, int wi, const int (&xa)[VEC], const int (&xb)[VEC],
                                              const float (&lx)[VEC], float (&h)[VEC]) {
    if constexpr (VEC == 4) {
        float p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = row[min(xa[0] + i, wi - 1)];
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = esp_lerp_col(j, lx[j], esp_sel4(p, xa[j] - xa[0]), esp_sel4(p, xb[j] - xa[0]));
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) h[j] = (1.0f - lx[j]) * row[xa[j]] + lx[j] * row[xb[j]];
    }
}

// A thread writes VEC columns of ESP_UP_ROWS consecutive output rows: the columns' indices and weights are formed once, and a
// blended source row is kept while the next output row still reads it (consecutive output rows share one of their two).
template <int VEC>
__global__ __launch_bounds__(ESP_THREADS) void k_esp_bilinear(const float* __restrict__ in, size_t in_bs, int hi, int wi,
                                                              float* __restrict__ out, size_t out_bs, int ho, int wo) {
    const int wv = wo / VEC;                                         // (the host launches VEC = 4 only for wo = 2 wi, wi even)
    const int hg = (ho + ESP_UP_ROWS - 1) / ESP_UP_ROWS;
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx >= hg * wv) return;
    const int yg = idx / wv, x0 = (idx - yg * wv) * VEC;
    const int c = blockIdx.y;
    const float* p = in + (size_t)blockIdx.z * in_bs + (size_t)c * hi * wi;
    int xa[VEC], xb[VEC];
    float lx[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) esp_axis(x0 + j, wi, wo, xa[j], xb[j], lx[j]);
    int ra = -1, rb = -1;                                            // the source rows whose blends ha, hb hold
    float ha[VEC], hb[VEC];
    for (int y = yg * ESP_UP_ROWS; y < min(ho, (yg + 1) * ESP_UP_ROWS); ++y) {
        int y0, y1;
        float ly;
        esp_axis(y, hi, ho, y0, y1, ly);
        if (y0 != ra) {
            if (y0 == rb) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) ha[j] = hb[j];
            } else {
                esp_blend_row<VEC>(p + (size_t)y0 * wi, wi, xa, xb, lx, ha);
            }
            ra = y0;
        }
        if (y1 != ra && y1 != rb) {
            esp_blend_row<VEC>(p + (size_t)y1 * wi, wi, xa, xb, lx, hb);
            rb = y1;
        }
        float v[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float lo = y1 == ra ? ha[j] : hb[j];
            if constexpr (VEC == 4)
                v[j] = esp_lerp_fma(ly, ha[j], lo);
            else
                v[j] = (1.0f - ly) * ha[j] + ly * lo;
        }
        float* o = out + (size_t)blockIdx.z * out_bs + ((size_t)c * ho + y) * wo + x0;
        if constexpr (VEC == 4)
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int j = 0; j < VEC; ++j) o[j] = v[j];
    }
}

__device__ __forceinline__ float esp_dw3(const float* __restrict__ p, int h, int w, int y, int x, const float* __restrict__ w9) {
    float s = 0.0f;
#pragma unroll
    for (int u = -1; u <= 1; ++u)
#pragma unroll
        for (int v = -1; v <= 1; ++v) {
            const int iy = y + u, ix = x + v;
            if (iy >= 0 && iy < h && ix >= 0 && ix < w) s = fmaf(w9[(u + 1) * 3 + (v + 1)], p[iy * w + ix], s);
        }
    return s;
}

// pooled [T][128][hp][wp]; w [128][9]; out: the stage's slot [T][..][128][h][w] of the PSP buffer
__global__ __launch_bounds__(ESP_THREADS) void k_esp_psp_up(const float* __restrict__ pooled, size_t in_bs, int hp, int wp,
                                                            const float* __restrict__ wgt, float* __restrict__ out, size_t out_bs, int h,
                                                            int w) {
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx >= h * w) return;
    const int y = idx / w, x = idx - y * w, c = blockIdx.y;
    const float* p = pooled + (size_t)blockIdx.z * in_bs + (size_t)c * hp * wp;
    const float* w9 = wgt + (size_t)c * 9;
    int y0, y1, xa, xb;
    float ly, lx;
    esp_axis(y, hp, h, y0, y1, ly);
    esp_axis(x, wp, w, xa, xb, lx);
    const float top = (1.0f - lx) * esp_dw3(p, hp, wp, y0, xa, w9) + lx * esp_dw3(p, hp, wp, y0, xb, w9);
    const float bot = (1.0f - lx) * esp_dw3(p, hp, wp, y1, xa, w9) + lx * esp_dw3(p, hp, wp, y1, xb, w9);
    out[(size_t)blockIdx.z * out_bs + (size_t)c * h * w + idx] = (1.0f - ly) * top + ly * bot;
}

// ---- the decoder tail at single pixels (tmpnn_espnet_centres) ---------------------------------------------------------------
// Everything behind m3 is pointwise convs and x2 resizes, so output pixel (y, x) needs m1 at <= 2 x 2 pixels, m2 at <= 3 x 3 and
// m3 at the taps of those.  One workgroup per requested pixel:
//   1  xs [64 + C][12]  cat[out_l2, up(m3)] at the 3 x 3 pixels of level 2 from (by, bx) on (9 of a row of 12 floats: a lane reads
//                       its k's nine values as three 16-byte words), the upper half blended from m3
//   2  ms [9][C]        project_l2 at those pixels
//   3  xs [32 + C][4]   cat[out_l1, up(m2)] at the 2 x 2 pixels of level 1, the upper half blended from ms
//   4  m1s [4][C]       project_l1 at those pixels
//   5  logits[d][c]     the final blend
// Every sum is the chain of k_esp_pw (acc = 0, fmaf over k ascending, source a then b) and every epilogue and blend the helper
// the dense kernels use, with the column of the dense resize that would have written the pixel, so the values equal the dense
// map's bit for bit.  A conv gives lane c output channel c and all staged pixels: the pixels are independent accumulators, the
// weight row wt[k][.] one coalesced load, and the loop holds no branch, so eight weight loads are in flight.
// LDS: 320 x 12 + 9 x 256 floats = 24 576 bytes for every C (stages 3 and 4 reuse the first array).
constexpr int ESPC_MAX_C = 256;              // channels a workgroup of ESP_THREADS lanes serves
constexpr int ESPC_N2 = 9, ESPC_S2 = 12;     // pixels staged at level 2 and the floats of their row in xs
constexpr int ESPC_N1 = 4;                   // pixels staged at level 1
constexpr int ESPC_XS = (64 + ESPC_MAX_C) * ESPC_S2;
constexpr int ESPC_M1 = (32 + ESPC_MAX_C) * ESPC_N1;          // m1s starts here, behind the staged input of stage 4
static_assert(ESPC_M1 + ESPC_N1 * ESPC_MAX_C <= ESPC_XS && ESPC_MAX_C <= ESP_THREADS, "stage 4 fits the first array; a lane a channel");

struct EspTail {
    const float *l1, *l2, *m3;                                 // [T][32][h2][w2], [T][64][h4][w4], [T][C][h8][w8]
    const float *w2, *scale2, *shift2, *slope2;                // project_l2: wt [64 + C][C]
    const float *w1, *scale1, *shift1, *slope1;                // project_l1: wt [32 + C][C]
};

// out[p][c] = prelu(norm(sum_k xs[k][p] wt[k][c])) for the NP pixels staged in xs ([cin][NS]); out is [NP][C]; lane c < C
template <int NP, int NS>
__device__ __forceinline__ void espc_conv(const float* xs, int cin, int C, int c, const float* __restrict__ wt,
                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                          const float* __restrict__ slope, float* out) {
    float acc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[j] = 0.0f;
#pragma unroll 8
    for (int k = 0; k < cin; ++k) {
        const float w = wt[(size_t)k * C + c];
#pragma unroll
        for (int j = 0; j < NP; ++j) acc[j] = fmaf(xs[k * NS + j], w, acc[j]);
    }
    const float sc = scale[c], sh = shift[c], sl = slope[c];
#pragma unroll
    for (int j = 0; j < NP; ++j) out[j * C + c] = prelu(esp_norm(acc[j], sc, sh), sl);
}

// the value of an x2 resize (hi x wi -> 2 hi x 2 wi) at output (y, x), as k_esp_bilinear<4> forms it; src(yy, xx) reads the source
template <class Src>
__device__ __forceinline__ float espc_up(int y, int x, int hi, int wi, Src src) {
    int y0, y1, x0, x1;
    float ly, lx;
    esp_axis(y, hi, 2 * hi, y0, y1, ly);
    esp_axis(x, wi, 2 * wi, x0, x1, lx);
    const float top = esp_lerp_col(x, lx, src(y0, x0), src(y0, x1));
    const float bot = esp_lerp_col(x, lx, src(y1, x0), src(y1, x1));
    return esp_lerp_fma(ly, top, bot);
}

__global__ __launch_bounds__(ESP_THREADS) void k_esp_centres(EspTail a, int C, int T, int H, int W, const int32_t* __restrict__ pix,
                                                             float* __restrict__ logits, int32_t* __restrict__ flags) {
    __shared__ __align__(16) float xs[ESPC_XS];
    __shared__ __align__(16) float ms[ESPC_N2 * ESPC_MAX_C];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8;
    const int plane = H * W;                                                // (T H W < 2^31: the host check)
    int px = pix[d];
    const bool bad = px < 0 || px >= T * plane;
    px = px < 0 ? 0 : (px >= T * plane ? T * plane - 1 : px);
    if (tid == 0) flags[d] = bad ? 1 : 0;
    const int t = px / plane, rem = px - t * plane, y = rem / W, x = rem - y * W;
    // level 1: the 2 x 2 pixels (ya0 | ya1, xa0 | xa1) of m1 under (y, x); level 2: the 3 x 3 pixels of m2 from (by, bx) on under those
    int ya0, ya1, xa0, xa1, by, bx, unused;
    float lya, lxa, lam;
    esp_axis(y, h2, H, ya0, ya1, lya);
    esp_axis(x, w2, W, xa0, xa1, lxa);
    esp_axis(ya0, h4, h2, by, unused, lam);
    esp_axis(xa0, w4, w2, bx, unused, lam);

    // 1: cat[out_l2, up(m3)] at level-2 pixel (min(by + r, h4 - 1), min(bx + q, w4 - 1)), p = 3 r + q
    {
        const float* l2 = a.l2 + (size_t)t * 64 * h4 * w4;
        const float* m3 = a.m3 + (size_t)t * C * h8 * w8;
#pragma unroll 3
        for (int i = tid; i < 64 * ESPC_N2; i += ESP_THREADS) {
            const int k = i / ESPC_N2, p = i - k * ESPC_N2, r = p / 3, q = p - 3 * r;
            xs[k * ESPC_S2 + p] = l2[((size_t)k * h4 + min(by + r, h4 - 1)) * w4 + min(bx + q, w4 - 1)];
        }
#pragma unroll 2
        for (int i = tid; i < C * ESPC_N2; i += ESP_THREADS) {
            const int c = i / ESPC_N2, p = i - c * ESPC_N2, r = p / 3, q = p - 3 * r;
            const float* src = m3 + (size_t)c * h8 * w8;
            xs[(64 + c) * ESPC_S2 + p] =
                espc_up(min(by + r, h4 - 1), min(bx + q, w4 - 1), h8, w8, [&](int yy, int xx) { return src[yy * w8 + xx]; });
        }
    }
    __syncthreads();
    // 2: project_l2
    if (tid < C) espc_conv<ESPC_N2, ESPC_S2>(xs, 64 + C, C, tid, a.w2, a.scale2, a.shift2, a.slope2, ms);
    __syncthreads();
    // 3: cat[out_l1, up(m2)] at level-1 pixel (ya0 or ya1, xa0 or xa1), p = 2 r + q; the taps of m2 lie in the staged 3 x 3
    {
        const float* l1 = a.l1 + (size_t)t * 32 * h2 * w2;
        for (int i = tid; i < 32 * ESPC_N1; i += ESP_THREADS) {
            const int k = i / ESPC_N1, p = i - k * ESPC_N1;
            xs[i] = l1[((size_t)k * h2 + ((p >> 1) ? ya1 : ya0)) * w2 + ((p & 1) ? xa1 : xa0)];
        }
        for (int i = tid; i < C * ESPC_N1; i += ESP_THREADS) {
            const int c = i / ESPC_N1, p = i - c * ESPC_N1;
            const float* src = ms + c;
            xs[32 * ESPC_N1 + i] = espc_up((p >> 1) ? ya1 : ya0, (p & 1) ? xa1 : xa0, h4, w4, [&](int yy, int xx) {
                const int ry = min(max(yy - by, 0), 2), rx = min(max(xx - bx, 0), 2);      // (0 .. 2 by construction; never outside ms)
                return src[(ry * 3 + rx) * C];
            });
        }
    }
    __syncthreads();
    // 4: project_l1 (no norm, no activation: scale 1, shift 0, slopes 1 in the arena, applied as the dense kernel applies them)
    float* m1s = xs + ESPC_M1;
    if (tid < C) espc_conv<ESPC_N1, ESPC_N1>(xs, 32 + C, C, tid, a.w1, a.scale1, a.shift1, a.slope1, m1s);
    __syncthreads();
    // 5: the final x2 resize at (y, x)
    if (tid < C) {
        const float top = esp_lerp_col(x, lxa, m1s[tid], m1s[C + tid]);
        const float bot = esp_lerp_col(x, lxa, m1s[2 * C + tid], m1s[3 * C + tid]);
        logits[(size_t)d * C + tid] = esp_lerp_fma(lya, top, bot);
    }
}

// ---- the weight arena (include/tmpnn.h documents the order; trackmpnn_amd/espnet.py packs it) -------------------------------
struct Arena {
    const float* p;
    size_t at;
    const float* take(size_t n) {
        const float* r = p ? p + at : nullptr;
        at += (n + 3) & ~(size_t)3;
        return r;
    }
};
struct Pw { const float *wt, *scale, *shift, *slope; int cin, cout, groups; };
struct Dw { const float *w, *scale, *shift, *slope; int n; };
struct Eesp { Pw proj; Dw dw; Pw exp; };
struct Down { const float *w3, *s3, *t3, *a3, *w1t, *scale, *shift, *pool_slope; int nin, nout; Eesp e; };
struct Net {
    const float *l1_w, *l1_scale, *l1_shift, *l1_slope;
    Down d2, d3, d4;
    Eesp l3[3], l4[7], psp_e;
    Pw proj4, psp_proj, proj3, proj2, proj1;
    const float* psp_w[4];
};

Pw take_pw(Arena& a, int cin, int cout, int groups) {
    Pw p;
    p.cin = cin, p.cout = cout, p.groups = groups;
    p.wt = a.take((size_t)(cin / groups) * cout);
    p.scale = a.take(cout), p.shift = a.take(cout), p.slope = a.take(cout);
    return p;
}
Eesp take_eesp(Arena& a, int nin, int nout) {
    Eesp e;
    const int n = nout / 4;
    e.proj = take_pw(a, nin, n, 4);
    e.dw.n = n;
    e.dw.w = a.take((size_t)4 * n * 9);
    e.dw.scale = a.take(nout), e.dw.shift = a.take(nout), e.dw.slope = a.take(nout);
    e.exp = take_pw(a, nout, nout, 4);
    return e;
}
Down take_down(Arena& a, int nin, int nout) {
    Down d;
    d.nin = nin, d.nout = nout;
    d.w3 = a.take(81), d.s3 = a.take(3), d.t3 = a.take(3), d.a3 = a.take(3);
    d.w1t = a.take((size_t)3 * nout), d.scale = a.take(nout), d.shift = a.take(nout);
    d.pool_slope = a.take(nin);
    d.e = take_eesp(a, nin, nout - nin);
    return d;
}
size_t walk_arena(const float* base, int C, Net& n) {
    Arena a{base, 0};
    n.l1_w = a.take(32 * 27), n.l1_scale = a.take(32), n.l1_shift = a.take(32), n.l1_slope = a.take(32);
    n.d2 = take_down(a, 32, 64);
    n.d3 = take_down(a, 64, 128);
    for (auto& e : n.l3) e = take_eesp(a, 128, 128);
    n.d4 = take_down(a, 128, 256);
    for (auto& e : n.l4) e = take_eesp(a, 256, 256);
    n.proj4 = take_pw(a, 256, ESP_PSP, 1);
    n.psp_e = take_eesp(a, 2 * ESP_PSP, ESP_PSP);
    for (auto& w : n.psp_w) w = a.take(ESP_PSP * 9);
    n.psp_proj = take_pw(a, 5 * ESP_PSP, ESP_PSP, 1);
    n.proj3 = take_pw(a, ESP_PSP, C, 1);
    n.proj2 = take_pw(a, 64 + C, C, 1);
    n.proj1 = take_pw(a, 32 + C, C, 1);
    return a.at;
}

// ---- the workspace: every intermediate map of one call, per image (x T) --------------------------------------------------
struct Ws {
    float *img2, *img4, *img8, *img16, *l1, *l2, *l3a, *l3b, *l4a, *l4b, *red, *cat, *p4, *up4, *psp, *pool_a, *pool_b, *pspo, *m3,
        *up3, *m2, *up2, *m1;
};
// tail = false: without the four maps of the dense decoder tail (up3, m2, up2, m1), which are carved last, so the trunk's arrays lie
// at the same offsets in both layouts
size_t walk_ws(void* base, int T, int H, int W, int C, Ws& s, bool tail = true) {
    WsCarver cv{reinterpret_cast<char*>(base)};
    const size_t t = (size_t)T, P2 = (size_t)(H / 2) * (W / 2), P4 = P2 / 4, P8 = P4 / 4, P16 = P8 / 4;
    const size_t Pp = (size_t)((H / 8 + 1) / 2) * ((W / 8 + 1) / 2);
    s.img2 = cv.take<float>(t * 3 * P2), s.img4 = cv.take<float>(t * 3 * P4), s.img8 = cv.take<float>(t * 3 * P8);
    s.img16 = cv.take<float>(t * 3 * P16);
    s.l1 = cv.take<float>(t * 32 * P2), s.l2 = cv.take<float>(t * 64 * P4);
    s.l3a = cv.take<float>(t * 128 * P8), s.l3b = cv.take<float>(t * 128 * P8);
    s.l4a = cv.take<float>(t * 256 * P16), s.l4b = cv.take<float>(t * 256 * P16);
    s.red = cv.take<float>(t * 8 * P2);          // the reduced map of an EESP: at most 8 x P2 = 16 x P4 = 32 x P8 = 64 x P16
    s.cat = cv.take<float>(t * 32 * P4);         // its four fused branches: at most 32 x P4 (64 x P8, 128 x P8, 256 x P16)
    s.p4 = cv.take<float>(t * ESP_PSP * P16), s.up4 = cv.take<float>(t * ESP_PSP * P8);
    s.psp = cv.take<float>(t * 5 * ESP_PSP * P8);
    s.pool_a = cv.take<float>(t * ESP_PSP * Pp), s.pool_b = cv.take<float>(t * ESP_PSP * Pp);
    s.pspo = cv.take<float>(t * ESP_PSP * P8);
    s.m3 = cv.take<float>(t * C * P8);
    s.up3 = s.m2 = s.up2 = s.m1 = nullptr;
    if (tail) {
        s.up3 = cv.take<float>(t * C * P4), s.m2 = cv.take<float>(t * C * P4);
        s.up2 = cv.take<float>(t * C * P2), s.m1 = cv.take<float>(t * C * P2);
    }
    return (size_t)(cv.p - reinterpret_cast<char*>(base));
}

struct Run {
    hipStream_t st;
    int T;
    int rc;
};
#define ESP_CHECK(r, what)                                       \
    do {                                                         \
        if (int rc_ = check_launch("espnet_fwd (" what ")")) {   \
            (r).rc = rc_;                                        \
            return;                                              \
        }                                                        \
    } while (0)

inline dim3 grid_px(size_t px, int y, int T) { return dim3((unsigned)((px + ESP_THREADS - 1) / ESP_THREADS), (unsigned)y, (unsigned)T); }

void run_pool(Run& r, const float* in, size_t in_bs, int C, int h, int w, float* out, size_t out_bs, const float* slope) {
    if (r.rc) return;
    const int ho = (h + 1) / 2, wo = (w + 1) / 2;
    if (slope)
        k_esp_pool<true><<<grid_px((size_t)ho * wo, C, r.T), ESP_THREADS, 0, r.st>>>(in, in_bs, h, w, out, out_bs, ho, wo, slope);
    else
        k_esp_pool<false><<<grid_px((size_t)ho * wo, C, r.T), ESP_THREADS, 0, r.st>>>(in, in_bs, h, w, out, out_bs, ho, wo, slope);
    ESP_CHECK(r, "average pool");
}

// The channel tile of a pointwise conv.  32 channels a lane read every input value once per 32 outputs: the form of the layers that
// carry the FLOPs (project_l1, project_l2 at full size), whose weights leave room for two k in flight.  A layer whose 32-channel tiles
// would not give every CU a workgroup is bound by the latency of its chain over k instead: 8 channels a lane give four times the
// workgroups and eight k in flight.  The choice depends on the layer and the plane, never on T, and every output is the same
// ascending chain of fmaf over k in both, so it changes no bit.
constexpr int ESP_CUS = 256;
bool pw_wide(const Pw& p, int P) {
    const int cpg = p.cout / p.groups;
    return cpg % 32 == 0 && (long)((P + ESP_THREADS - 1) / ESP_THREADS) * p.groups * (cpg / 32) >= ESP_CUS;
}

void run_pw(Run& r, const Pw& p, const float* a, size_t a_bs, int ca, const float* b, size_t b_bs, int P, const float* res, size_t res_bs,
            float* out, size_t out_bs, float* pre = nullptr) {
    if (r.rc) return;
    const int cpg = p.cout / p.groups;
    if (pre) {                                   // the training forward of a trained layer: the same tile, the same chain over k
        const size_t pre_bs = (size_t)p.cout * P;
        if (pw_wide(p, P)) {
            k_esp_pw<32, 2, true><<<grid_px(P, p.groups * (cpg / 32), r.T), ESP_THREADS, 0, r.st>>>(
                a, a_bs, ca, b, b_bs, p.cin, p.cout, p.groups, P, p.wt, p.scale, p.shift, p.slope, res, res_bs, out, out_bs, pre, pre_bs);
        } else {
            const int tiles = (cpg + 7) / 8;
            k_esp_pw<8, 8, true><<<grid_px(P, p.groups * tiles, r.T), ESP_THREADS, 0, r.st>>>(
                a, a_bs, ca, b, b_bs, p.cin, p.cout, p.groups, P, p.wt, p.scale, p.shift, p.slope, res, res_bs, out, out_bs, pre, pre_bs);
        }
        ESP_CHECK(r, "pointwise conv");
        return;
    }
    if (pw_wide(p, P)) {
        k_esp_pw<32, 2><<<grid_px(P, p.groups * (cpg / 32), r.T), ESP_THREADS, 0, r.st>>>(a, a_bs, ca, b, b_bs, p.cin, p.cout, p.groups, P, p.wt,
                                                                                         p.scale, p.shift, p.slope, res, res_bs, out, out_bs);
    } else {
        const int tiles = (cpg + 7) / 8;
        k_esp_pw<8, 8><<<grid_px(P, p.groups * tiles, r.T), ESP_THREADS, 0, r.st>>>(a, a_bs, ca, b, b_bs, p.cin, p.cout, p.groups, P, p.wt,
                                                                                   p.scale, p.shift, p.slope, res, res_bs, out, out_bs);
    }
    ESP_CHECK(r, "pointwise conv");
}

void run_dw(Run& r, const Dw& d, const int* dil, int stride, const float* in, int h, int w, float* out) {
    if (r.rc) return;
    const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
    const int tx = (wo + ESP_TW - 1) / ESP_TW, ty = (ho + ESP_TH - 1) / ESP_TH;
    const dim3 grid((unsigned)(tx * ty), (unsigned)d.n, (unsigned)r.T);
    const size_t in_bs = (size_t)d.n * h * w, out_bs = (size_t)4 * d.n * ho * wo;
    if (stride == 2)
        k_esp_dw<2><<<grid, ESP_THREADS, 0, r.st>>>(in, in_bs, d.n, h, w, d.w, dil[0], dil[1], dil[2], dil[3], d.scale, d.shift, d.slope, out,
                                                    out_bs, ho, wo, tx);
    else
        k_esp_dw<1><<<grid, ESP_THREADS, 0, r.st>>>(in, in_bs, d.n, h, w, d.w, dil[0], dil[1], dil[2], dil[3], d.scale, d.shift, d.slope, out,
                                                    out_bs, ho, wo, tx);
    ESP_CHECK(r, "EESP transform");
}

void run_bilinear(Run& r, const float* in, size_t in_bs, int C, int hi, int wi, float* out, size_t out_bs, int ho, int wo) {
    if (r.rc) return;
    const int hg = (ho + ESP_UP_ROWS - 1) / ESP_UP_ROWS;
    if (wo == 2 * wi && wo % 4 == 0 && aligned16(out) && out_bs % 4 == 0)
        k_esp_bilinear<4><<<grid_px((size_t)hg * (wo / 4), C, r.T), ESP_THREADS, 0, r.st>>>(in, in_bs, hi, wi, out, out_bs, ho, wo);
    else
        k_esp_bilinear<1><<<grid_px((size_t)hg * wo, C, r.T), ESP_THREADS, 0, r.st>>>(in, in_bs, hi, wi, out, out_bs, ho, wo);
    ESP_CHECK(r, "bilinear resize");
}

constexpr int DIL_1234[4] = {1, 2, 3, 4};      // r_lim >= 9: kernel sizes 3 5 7 9
constexpr int DIL_1123[4] = {1, 1, 2, 3};      // r_lim = 7: 3 5 7 3, sorted 3 3 5 7

// EESP of stride 1: in [T][nin][h][w] (second source b for the channels from ca on) -> out [T][..][nout][h][w] (batch stride out_bs)
// pre_red, pre_exp (the training forward): where the two pointwise convs leave the values in front of their PReLUs, dense [T][c][h w]
void run_eesp(Run& r, const Eesp& e, const int* dil, const float* a, size_t a_bs, int ca, const float* b, size_t b_bs, int h, int w,
              bool residual, float* out, size_t out_bs, const Ws& s, float* pre_red = nullptr, float* pre_exp = nullptr) {
    const int P = h * w, n = e.dw.n;
    run_pw(r, e.proj, a, a_bs, ca, b, b_bs, P, nullptr, 0, s.red, (size_t)n * P, pre_red);
    run_dw(r, e.dw, dil, 1, s.red, h, w, s.cat);
    run_pw(r, e.exp, s.cat, (size_t)4 * n * P, 4 * n, nullptr, 0, P, residual ? a : nullptr, a_bs, out, out_bs, pre_exp);
}

// DownSampler: in [T][nin][h][w], img: the pyramid image at (h / 2, w / 2) -> out [T][nout][h / 2][w / 2]
void run_down(Run& r, const Down& d, const int* dil, const float* in, int h, int w, const float* img, float* out, const Ws& s) {
    if (r.rc) return;
    const int ho = h / 2, wo = w / 2, Po = ho * wo, n = d.e.dw.n;
    k_esp_reinf<<<grid_px(Po, (d.nout + ESP_REINF_CO - 1) / ESP_REINF_CO, r.T), ESP_THREADS, 0, r.st>>>(img, ho, wo, d.w3, d.s3, d.t3, d.a3, d.w1t, d.scale, d.shift, d.nout, out);
    ESP_CHECK(r, "input reinforcement");
    const size_t out_bs = (size_t)d.nout * Po;
    run_pool(r, in, (size_t)d.nin * h * w, d.nin, h, w, out, out_bs, d.pool_slope);
    run_pw(r, d.e.proj, in, (size_t)d.nin * h * w, d.nin, nullptr, 0, h * w, nullptr, 0, s.red, (size_t)n * h * w);
    run_dw(r, d.e.dw, dil, 2, s.red, h, w, s.cat);
    float* hi = out + (size_t)d.nin * Po;        // the EESP half of the cat: + the reinforcement already there, then the block's PReLU
    run_pw(r, d.e.exp, s.cat, (size_t)4 * n * Po, 4 * n, nullptr, 0, Po, hi, out_bs, hi, out_bs);
}

constexpr int ESP_MAX_T = 65535, ESP_MAX_C = 1024;

bool shape_ok(int T, int H, int W, int C) {
    return T >= 1 && T <= ESP_MAX_T && C >= 1 && C <= ESP_MAX_C && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0 &&
           (int64_t)std::max(C, 160) * H * W < ((int64_t)1 << 31);
}

// the host checks every entry point shares; `who` names the caller in the message
int check_call(const char* who, const void* arena, const void* images, const void* ws, const void* out, int T, int H, int W, int C) {
    TM_REQUIRE(arena != nullptr && images != nullptr && ws != nullptr && out != nullptr, "%s: null pointer (arena, images, ws, out)", who);
    TM_REQUIRE(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "%s: H=%d W=%d (positive multiples of 16)", who, H, W);
    TM_REQUIRE(shape_ok(T, H, W, C), "%s: T=%d C=%d H=%d W=%d (1 <= T <= %d, 1 <= C <= %d, max(C, 160) H W < 2^31)", who, T, C, H, W,
               ESP_MAX_T, ESP_MAX_C);
    TM_REQUIRE(aligned16(arena) && aligned16(images) && aligned16(ws) && aligned16(out), "%s: pointers must be 16-byte aligned", who);
    return TMPNN_OK;
}

// What a training forward keeps for its backward, each dense [T][c][pixels]; a null pointer keeps nothing there.
//   pre3      project_l3 / act_l3 in front of the PReLU [T][C][P8]
//   pre4, pre_red, pre_exp, pre_psp   the same of proj_L4_C [128][P16], pspMod.0.proj_1x1 [32][P8], pspMod.0.conv_1x1_exp / module_act
//             [128][P8] and pspMod.1.project [128][P8]
//   pooled    the four pooled maps of the PSP chain, which the plain forward ping-pongs through pool_a / pool_b (all four or none)
struct TrainKeep {
    float *pre3 = nullptr, *pre4 = nullptr, *pre_red = nullptr, *pre_exp = nullptr, *pre_psp = nullptr;
    float* pooled[4] = {nullptr, nullptr, nullptr, nullptr};
};

// The trunk: every launch of the forward up to and including m3 (65), shared by tmpnn_espnet_fwd and tmpnn_espnet_trunk.
int run_trunk(const Net& n, const Ws& s, const float* images, int T, int H, int W, int C, hipStream_t st, const TrainKeep& keep = TrainKeep()) {
    Run r{st, T, 0};
    const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8, h16 = H / 16, w16 = W / 16;
    const size_t P2 = (size_t)h2 * w2, P4 = (size_t)h4 * w4, P8 = (size_t)h8 * w8, P16 = (size_t)h16 * w16;
    // the image pyramid every DownSampler's reinforcement reads (the reference pools the full image again in each of them)
    run_pool(r, images, (size_t)3 * H * W, 3, H, W, s.img2, 3 * P2, nullptr);
    run_pool(r, s.img2, 3 * P2, 3, h2, w2, s.img4, 3 * P4, nullptr);
    run_pool(r, s.img4, 3 * P4, 3, h4, w4, s.img8, 3 * P8, nullptr);
    run_pool(r, s.img8, 3 * P8, 3, h8, w8, s.img16, 3 * P16, nullptr);
    if (r.rc) return r.rc;
    k_esp_level1<<<grid_px(P2, 1, T), ESP_THREADS, 0, r.st>>>(images, H, W, n.l1_w, n.l1_scale, n.l1_shift, n.l1_slope, s.l1, h2, w2);
    if (int rc = check_launch("espnet_fwd (level1)")) return rc;
    // encoder
    run_down(r, n.d2, DIL_1234, s.l1, h2, w2, s.img4, s.l2, s);
    run_down(r, n.d3, DIL_1234, s.l2, h4, w4, s.img8, s.l3a, s);
    float *cur = s.l3a, *nxt = s.l3b;
    for (const Eesp& e : n.l3) {
        run_eesp(r, e, DIL_1234, cur, 128 * P8, 128, nullptr, 0, h8, w8, true, nxt, 128 * P8, s);
        std::swap(cur, nxt);
    }
    const float* out_l3 = cur;
    run_down(r, n.d4, DIL_1234, out_l3, h8, w8, s.img16, s.l4a, s);
    cur = s.l4a, nxt = s.l4b;
    for (const Eesp& e : n.l4) {
        run_eesp(r, e, DIL_1123, cur, 256 * P16, 256, nullptr, 0, h16, w16, true, nxt, 256 * P16, s);
        std::swap(cur, nxt);
    }
    const float* out_l4 = cur;
    // decoder
    run_pw(r, n.proj4, out_l4, 256 * P16, 256, nullptr, 0, (int)P16, nullptr, 0, s.p4, ESP_PSP * P16, keep.pre4);
    run_bilinear(r, s.p4, ESP_PSP * P16, ESP_PSP, h16, w16, s.up4, ESP_PSP * P8, h8, w8);
    const size_t psp_bs = 5 * ESP_PSP * P8;
    run_eesp(r, n.psp_e, DIL_1123, out_l3, 128 * P8, 128, s.up4, ESP_PSP * P8, h8, w8, false, s.psp, psp_bs, s, keep.pre_red, keep.pre_exp);
    {
        const float* prev = s.psp;
        size_t prev_bs = psp_bs;
        int ph = h8, pw = w8;
        float *pa = s.pool_a, *pb = s.pool_b;
        for (int k = 0; k < 4; ++k) {
            const int qh = (ph + 1) / 2, qw = (pw + 1) / 2;
            const size_t q_bs = (size_t)ESP_PSP * qh * qw;
            if (keep.pooled[k]) pa = keep.pooled[k];
            run_pool(r, prev, prev_bs, ESP_PSP, ph, pw, pa, q_bs, nullptr);
            if (r.rc) return r.rc;
            k_esp_psp_up<<<grid_px(P8, ESP_PSP, T), ESP_THREADS, 0, r.st>>>(pa, q_bs, qh, qw, n.psp_w[k], s.psp + (size_t)(k + 1) * ESP_PSP * P8,
                                                                         psp_bs, h8, w8);
            if (int rc = check_launch("espnet_fwd (PSP stage)")) return rc;
            prev = pa, prev_bs = q_bs, ph = qh, pw = qw;
            std::swap(pa, pb);
        }
    }
    run_pw(r, n.psp_proj, s.psp, psp_bs, 5 * ESP_PSP, nullptr, 0, (int)P8, nullptr, 0, s.pspo, ESP_PSP * P8, keep.pre_psp);
    run_pw(r, n.proj3, s.pspo, ESP_PSP * P8, ESP_PSP, nullptr, 0, (int)P8, nullptr, 0, s.m3, C * P8, keep.pre3);
    return r.rc;
}

// The dense decoder tail behind m3 (5 launches).  pre2 (the training forward): project_l2's pre-activation, [T][C][P4].
int run_tail(const Net& n, const Ws& s, int T, int H, int W, int C, float* out, hipStream_t st, float* pre2 = nullptr) {
    Run r{st, T, 0};
    const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8;
    const size_t P2 = (size_t)h2 * w2, P4 = (size_t)h4 * w4, P8 = (size_t)h8 * w8;
    run_bilinear(r, s.m3, C * P8, C, h8, w8, s.up3, C * P4, h4, w4);
    run_pw(r, n.proj2, s.l2, 64 * P4, 64, s.up3, C * P4, (int)P4, nullptr, 0, s.m2, C * P4, pre2);
    run_bilinear(r, s.m2, C * P4, C, h4, w4, s.up2, C * P2, h2, w2);
    run_pw(r, n.proj1, s.l1, 32 * P2, 32, s.up2, C * P2, (int)P2, nullptr, 0, s.m1, C * P2);
    run_bilinear(r, s.m1, C * P2, C, h2, w2, out, (size_t)C * H * W, H, W);
    return r.rc;
}

}  // namespace
