// Training the embedding CNN's decoder on the device, encoder frozen (tmpnn_espnet_train_param_floats, tmpnn_espnet_train_table,
// tmpnn_espnet_train_ws_bytes, tmpnn_espnet_train_bwd_ws_bytes, tmpnn_espnet_refold, tmpnn_espnet_train_fwd,
// tmpnn_espnet_train_bwd; include/tmpnn.h; host definition: trackmpnn_amd.espnet.espnet_decoder_grads_host).
//
// The function differentiated is the eval forward of espnet_net.h: running statistics, Dropout2d the identity.  This file trains
// the decoder BEHIND merge_l3: project_l3 / act_l3, project_l2 and project_l1 (9 tensors); pspMod and proj_L4_C are frozen with the
// encoder, and the gradients handed back are those at the encoder taps out_l1 and out_l2.
//
// Forward: the launches of tmpnn_espnet_fwd, the two trained layers that end in a PReLU instantiated with SAVE, which also
// stores the value in front of the PReLU (its backward needs the sign, and no output tells it once a slope is zero or negative).
//
// Backward, for each of the three levels from the output down:
//   k_espt_up2_adj  adjoint of the x2 align_corners resize in gather form: a thread owns a source pixel, walks the 4 x 4 output
//                   pixels that can read it, forms their coordinates with the forward's esp_axis and adds weight x gradient in a
//                   fixed order.
//   k_espt_act      dz = dy PReLU'(pre) in place, with the per-channel sums (sum dz, sum over pre <= 0 of dy pre) of one plane
//                   chunk over all images in float64, reduced in a fixed tree: partials [C][chunks][2].
//   k_espt_wsum     G[co][ci] = sum over images and pixels of dz[co] x[ci], x the two halves of the forward's cat read in place: a
//                   workgroup owns a 64 x 64 tile of G and one chunk of the plane, stages 32 pixels of both operands in LDS, a
//                   thread keeps 4 x 4 sums in float32 over the 32 staged pixels and adds them into float64 after every such
//                   step; the cross-workgroup partials [chunks][cout][cin] are float64.
//   k_espt_fin      one workgroup per output channel: sums the partials in order, and with y = s (W x) + t, s = w / sqrt(v + eps):
//                   d conv.weight = s G, d bn.weight = (sum_ci W G - m sum dz) / sqrt(v + eps), d bn.bias = sum dz, d slope;
//                   all ADDED into the flat gradient buffer (every element has one owner).
//   k_espt_dx       d cat = (s W)^T dz: a thread per pixel, 8 input channels in registers, the output channels walked in order;
//                   the weights are read from the parameters as they lie ([cout][cin]); the cat splits by pointer: channels below
//                   ca are the tap gradient (skipped when nobody asked), the rest goes on to the next adjoint resize.
// k_espt_refold rewrites the trained layers' arena segments from the parameters in float64, rounded once: the bits of pack_arena.
//
// No atomics; every sum has a fixed order that depends on the shapes alone; 13 launches whatever T is.
#include "espnet_net.h"

namespace {

constexpr double ESPT_EPS = 1e-5;                // BatchNorm's eps (trackmpnn_amd.espnet.BN_EPS)
constexpr int ESPT_NT = 9;                       // trained tensors
constexpr int ESPT_TILE = 64, ESPT_PK = 32;      // k_espt_wsum: the tile of G and the pixels staged per step
constexpr int ESPT_CHUNK = 2048;                 // pixels of a plane chunk (one workgroup's share of a plane, over all images)
constexpr int ESPT_MAX_CHUNKS = 256;
constexpr int ESPT_CI_T = 8;                     // input channels a thread of k_espt_dx keeps

// ---- the parameter table ---------------------------------------------------------------------------------------------------
struct TrainLayer {                              // one pointwise layer: offsets in floats into the parameter / stats buffers, -1: none
    long w, bnw, bnb, slope, mean, var;
    int cin, cout;
};
struct TrainTable {
    TrainLayer l3, l2, l1;
    size_t floats;
};
TrainTable train_table(int C) {
    TrainTable t;
    long o = 0;
    auto take = [&](long n) { const long at = o; o += n; return at; };
    t.l3.cin = ESP_PSP, t.l3.cout = C;
    t.l3.w = take((long)C * ESP_PSP), t.l3.bnw = take(C), t.l3.bnb = take(C), t.l3.slope = take(C);
    t.l3.mean = 0, t.l3.var = C;
    t.l2.cin = 64 + C, t.l2.cout = C;
    t.l2.w = take((long)C * (64 + C)), t.l2.bnw = take(C), t.l2.bnb = take(C), t.l2.slope = take(C);
    t.l2.mean = 2 * (long)C, t.l2.var = 3 * (long)C;
    t.l1.cin = 32 + C, t.l1.cout = C;
    t.l1.w = take((long)C * (32 + C)), t.l1.bnw = t.l1.bnb = t.l1.slope = t.l1.mean = t.l1.var = -1;
    t.floats = (size_t)o;
    return t;
}

// ---- refold ----------------------------------------------------------------------------------------------------------------
struct RefoldLayer {
    const float *w, *bnw, *bnb, *slope, *mean, *var;     // parameters and frozen statistics (bnw null: weights only)
    float *wt, *scale, *shift, *slope_out;               // the layer's arena segments
    int cin, cout;
};
struct RefoldArgs { RefoldLayer l[3]; };

__device__ __forceinline__ void espt_fold(double w, double b, double m, double v, float& scale, float& shift) {
#pragma clang fp contract(off)
    const double s = w / sqrt(v + ESPT_EPS);
    const double ms = m * s;                     // (fold_bn rounds the product, then the difference: no fma)
    scale = (float)s;
    shift = (float)(b - ms);
}

__global__ __launch_bounds__(ESP_THREADS) void k_espt_refold(RefoldArgs a) {
    const RefoldLayer& L = a.l[blockIdx.y];
    const int nw = L.cin * L.cout;
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx < nw) {
        const int k = idx / L.cout, co = idx - k * L.cout;
        L.wt[idx] = L.w[(size_t)co * L.cin + k];
    } else if (idx < nw + L.cout && L.bnw != nullptr) {
        const int c = idx - nw;
        float sc, sh;
        espt_fold((double)L.bnw[c], (double)L.bnb[c], (double)L.mean[c], (double)L.var[c], sc, sh);
        L.scale[c] = sc, L.shift[c] = sh, L.slope_out[c] = L.slope[c];
    }
}

// ---- adjoint of the x2 resize ----------------------------------------------------------------------------------------------
// weight of source index s in output coordinate o of an axis n_in -> n_out (0 where o does not read s)
__device__ __forceinline__ float espt_axis_w(int o, int s, int n_in, int n_out) {
    if (o < 0 || o >= n_out) return 0.0f;
    int i0, i1;
    float lam;
    esp_axis(o, n_in, n_out, i0, i1, lam);
    float w = 0.0f;
    if (i0 == s) w += 1.0f - lam;
    if (i1 == s) w += lam;
    return w;
}

// dy [T][C][2 hi][2 wi] -> dx [T][C][hi][wi].  Output o reads the sources floor(c) and floor(c) + 1 of c = o (n - 1) / (2 n - 1), which
// lies in [o / 2 - 1 / 2, o / 2]: source s is read by o in 2 s - 1 .. 2 s + 2 at most.
__global__ __launch_bounds__(ESP_THREADS) void k_espt_up2_adj(const float* __restrict__ dy, int hi, int wi, float* __restrict__ dx) {
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx >= hi * wi) return;
    const int sy = idx / wi, sx = idx - sy * wi, c = blockIdx.y, C = gridDim.y;
    const int ho = 2 * hi, wo = 2 * wi;
    const float* p = dy + ((size_t)blockIdx.z * C + c) * ho * wo;
    float wx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wx[j] = espt_axis_w(2 * sx - 1 + j, sx, wi, wo);
    float g = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int oy = 2 * sy - 1 + i;
        const float wy = espt_axis_w(oy, sy, hi, ho);
        if (wy == 0.0f) continue;                // (also every row outside the map)
        float r = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = 2 * sx - 1 + j;
            if (wx[j] != 0.0f) r = fmaf(wx[j], p[(size_t)oy * wo + ox], r);
        }
        g = fmaf(wy, r, g);
    }
    dx[((size_t)blockIdx.z * C + c) * hi * wi + idx] = g;
}

// ---- PReLU backward with the per-channel sums ------------------------------------------------------------------------------
__device__ __forceinline__ double espt_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = ESP_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// d [T][C][P] (dy in, dz out), pre [T][C][P]; part [C][chunks][2]; grid (chunks, C)
__global__ __launch_bounds__(ESP_THREADS) void k_espt_act(float* d, const float* __restrict__ pre, const float* __restrict__ slope, int T,
                                                          int P, int chunk, double* __restrict__ part) {
    __shared__ double red[ESP_THREADS];
    const int c = blockIdx.y, C = gridDim.y;
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    const float a = slope[c];
    double sz = 0.0, sa = 0.0;
    for (int t = 0; t < T; ++t) {
        const size_t base = ((size_t)t * C + c) * P;
        for (int p = p0 + threadIdx.x; p < p1; p += ESP_THREADS) {
            const float g = d[base + p], x = pre[base + p];
            const float dz = x > 0.0f ? g : a * g;
            d[base + p] = dz;
            sz += (double)dz;
            if (!(x > 0.0f)) sa += (double)g * (double)x;
        }
    }
    sz = espt_block_sum(sz, red);
    sa = espt_block_sum(sa, red);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)c * gridDim.x + blockIdx.x) * 2;
        o[0] = sz, o[1] = sa;
    }
}

// ---- the weight-side reduction ---------------------------------------------------------------------------------------------
// dz [T][cout][P]; x: channels [0, ca) from a [T][ca][P], [ca, cin) from b [T][cin - ca][P]; part [chunks][cout][cin] float64.
// grid (chunks, tiles_co * tiles_ci)
__global__ __launch_bounds__(ESP_THREADS) void k_espt_wsum(const float* __restrict__ dz, const float* __restrict__ a, int ca,
                                                           const float* __restrict__ b, int cin, int cout, int T, int P, int chunk,
                                                           double* __restrict__ part) {
    __shared__ float sd[ESPT_PK][ESPT_TILE + 1];
    __shared__ float sx[ESPT_PK][ESPT_TILE + 1];
    const int tiles_ci = (cin + ESPT_TILE - 1) / ESPT_TILE;
    const int tco = blockIdx.y / tiles_ci, tci = blockIdx.y - tco * tiles_ci;
    const int co0 = tco * ESPT_TILE, ci0 = tci * ESPT_TILE;
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int t = 0; t < T; ++t) {
        for (int q = p0; q < p1; q += ESPT_PK) {
            float f[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) f[i][j] = 0.0f;
#pragma unroll
            for (int r = 0; r < ESPT_TILE * ESPT_PK / ESP_THREADS; ++r) {
                const int i = threadIdx.x + r * ESP_THREADS;
                const int ch = i / ESPT_PK, px = i - ch * ESPT_PK, gp = q + px;
                const int co = co0 + ch, ci = ci0 + ch;
                float vd = 0.0f, vx = 0.0f;
                if (gp < p1) {
                    if (co < cout) vd = dz[((size_t)t * cout + co) * P + gp];
                    if (ci < cin) vx = ci < ca ? a[((size_t)t * ca + ci) * P + gp] : b[((size_t)t * (cin - ca) + (ci - ca)) * P + gp];
                }
                sd[px][ch] = vd, sx[px][ch] = vx;
            }
            __syncthreads();
#pragma unroll 8
            for (int k = 0; k < ESPT_PK; ++k) {
                float u[4], v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) u[i] = sd[k][ty * 4 + i], v[i] = sx[k][tx * 4 + i];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) f[i][j] = fmaf(u[i], v[j], f[i][j]);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += (double)f[i][j];
        }
    }
    double* o = part + (size_t)blockIdx.x * cout * cin;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + ty * 4 + i, ci = ci0 + tx * 4 + j;
            if (co < cout && ci < cin) o[(size_t)co * cin + ci] = acc[i][j];
        }
}

// One workgroup per output channel.  w [cout][cin] the layer's conv weight; bnw null: no norm and no activation (project_l1).
// part_w [chunks_w][cout][cin], part_a [cout][chunks_a][2].  Gradients are added into g_*.
__global__ __launch_bounds__(ESP_THREADS) void k_espt_fin(const double* __restrict__ part_w, int chunks_w, const double* __restrict__ part_a,
                                                          int chunks_a, const float* __restrict__ w, const float* __restrict__ bnw,
                                                          const float* __restrict__ mean, const float* __restrict__ var, int cin, int cout,
                                                          float* g_w, float* g_bnw, float* g_bnb, float* g_slope) {
    __shared__ double red[ESP_THREADS];
    const int co = blockIdx.x;
    double s = 1.0, inv = 1.0;
    if (bnw != nullptr) {
        inv = 1.0 / sqrt((double)var[co] + ESPT_EPS);
        s = (double)bnw[co] * inv;
    }
    double wg = 0.0;
    for (int ci = threadIdx.x; ci < cin; ci += ESP_THREADS) {
        double G = 0.0;
        for (int k = 0; k < chunks_w; ++k) G += part_w[((size_t)k * cout + co) * cin + ci];
        const size_t at = (size_t)co * cin + ci;
        g_w[at] += (float)(s * G);
        wg += (double)w[at] * G;
    }
    if (bnw == nullptr) return;
    wg = espt_block_sum(wg, red);
    if (threadIdx.x == 0) {
        double sz = 0.0, sa = 0.0;
        for (int k = 0; k < chunks_a; ++k) {
            sz += part_a[((size_t)co * chunks_a + k) * 2];
            sa += part_a[((size_t)co * chunks_a + k) * 2 + 1];
        }
        g_bnb[co] += (float)sz;
        g_bnw[co] += (float)((wg - (double)mean[co] * sz) * inv);
        g_slope[co] += (float)sa;
    }
}

// ---- the data side of a pointwise conv -------------------------------------------------------------------------------------
// d cat[ci] = sum_co (scale[co] dz[co]) w[co][ci] for ci in [c_lo, cin): channels below ca to tap [T][ca][P], the others to
// up [T][cin - ca][P].  grid (pixels, tiles of ESPT_CI_T over [c_lo, cin), T); c_lo is 0 or ca.
__global__ __launch_bounds__(ESP_THREADS) void k_espt_dx(const float* __restrict__ dz, const float* __restrict__ w,
                                                         const float* __restrict__ scale, int cin, int cout, int ca, int c_lo, int P,
                                                         float* __restrict__ tap, float* __restrict__ up) {
    const int pix = blockIdx.x * ESP_THREADS + threadIdx.x;
    const int ci0 = c_lo + blockIdx.y * ESPT_CI_T;
    const int nci = min(ESPT_CI_T, cin - ci0);
    const size_t t = blockIdx.z;
    const bool live = pix < P;
    const int px = live ? pix : 0;
    float acc[ESPT_CI_T];
#pragma unroll
    for (int j = 0; j < ESPT_CI_T; ++j) acc[j] = 0.0f;
    const float* src = dz + t * cout * P + px;
#pragma unroll 4
    for (int co = 0; co < cout; ++co) {
        const float v = src[(size_t)co * P] * scale[co];
        const float* wr = w + (size_t)co * cin + ci0;
#pragma unroll
        for (int j = 0; j < ESPT_CI_T; ++j) acc[j] = fmaf(v, wr[min(j, nci - 1)], acc[j]);
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < ESPT_CI_T; ++j) {
        if (j < nci) {
            const int ci = ci0 + j;
            if (ci < ca)
                tap[(t * ca + ci) * P + pix] = acc[j];
            else
                up[(t * (cin - ca) + (ci - ca)) * P + pix] = acc[j];
        }
    }
}

// ---- workspaces ------------------------------------------------------------------------------------------------------------
struct TrainWs {
    Ws s;
    float *pre3, *pre2;
};
size_t walk_train_ws(void* base, int T, int H, int W, int C, TrainWs& w) {
    const size_t fwd = walk_ws(base, T, H, W, C, w.s);
    WsCarver cv{reinterpret_cast<char*>(base) + align16(fwd)};
    const size_t t = (size_t)T, P4 = (size_t)(H / 4) * (W / 4), P8 = P4 / 4;
    w.pre3 = cv.take<float>(t * C * P8), w.pre2 = cv.take<float>(t * C * P4);
    return (size_t)(cv.p - reinterpret_cast<char*>(base));
}

inline int chunks_of(size_t P) { return (int)std::min<size_t>((P + ESPT_CHUNK - 1) / ESPT_CHUNK, ESPT_MAX_CHUNKS); }
// the pixels of one chunk: a multiple of ESPT_PK, so that every staged step but a plane's last is full
inline int chunk_px(size_t P) {
    const size_t n = chunks_of(P), c = (P + n - 1) / n;
    return (int)((c + ESPT_PK - 1) / ESPT_PK * ESPT_PK);
}

struct BwdWs {
    float *d_m1, *d_up2, *d_m2, *d_up3, *d_m3;
    double *part_w, *part_a;
};
size_t walk_bwd_ws(void* base, int T, int H, int W, int C, BwdWs& b) {
    WsCarver cv{reinterpret_cast<char*>(base)};
    const size_t t = (size_t)T, P2 = (size_t)(H / 2) * (W / 2), P4 = P2 / 4, P8 = P4 / 4;
    b.d_m1 = cv.take<float>(t * C * P2), b.d_up2 = cv.take<float>(t * C * P2);
    b.d_m2 = cv.take<float>(t * C * P4), b.d_up3 = cv.take<float>(t * C * P4);
    b.d_m3 = cv.take<float>(t * C * P8);
    const size_t c = (size_t)C;
    const size_t pw = std::max({(size_t)chunks_of(P2) * c * (32 + c), (size_t)chunks_of(P4) * c * (64 + c), (size_t)chunks_of(P8) * c * ESP_PSP});
    b.part_w = cv.take<double>(pw);
    b.part_a = cv.take<double>(c * ESPT_MAX_CHUNKS * 2);
    return (size_t)(cv.p - reinterpret_cast<char*>(base));
}

#define ESPT_CHECK(what)                                                  \
    do {                                                                  \
        if (int rc_ = check_launch("espnet_train_bwd (" what ")")) return rc_; \
    } while (0)

// one level of the backward: d (the gradient at the layer's output, [T][C][P]) -> the layer's parameter gradients, and the
// gradient of its cat input (tap: channels below ca, may be null; up: the others, null when nothing lies behind)
int bwd_layer(const TrainLayer& L, const Pw& pw, const float* params, const float* stats, float* grads, float* d, const float* pre,
              const float* xa, int ca, const float* xb, int T, int P, const BwdWs& b, float* tap, float* up, hipStream_t st) {
    const int nch = chunks_of(P), chunk = chunk_px(P);
    const bool act = L.bnw >= 0;
    if (act) {
        k_espt_act<<<dim3(nch, L.cout), ESP_THREADS, 0, st>>>(d, pre, params + L.slope, T, P, chunk, b.part_a);
        ESPT_CHECK("PReLU backward");
    }
    const int tiles = ((L.cout + ESPT_TILE - 1) / ESPT_TILE) * ((L.cin + ESPT_TILE - 1) / ESPT_TILE);
    k_espt_wsum<<<dim3(nch, tiles), ESP_THREADS, 0, st>>>(d, xa, ca, xb, L.cin, L.cout, T, P, chunk, b.part_w);
    ESPT_CHECK("weight-side reduction");
    k_espt_fin<<<dim3(L.cout), ESP_THREADS, 0, st>>>(b.part_w, nch, b.part_a, nch, params + L.w, act ? params + L.bnw : nullptr,
                                                     act ? stats + L.mean : nullptr, act ? stats + L.var : nullptr, L.cin, L.cout,
                                                     grads + L.w, act ? grads + L.bnw : nullptr, act ? grads + L.bnb : nullptr,
                                                     act ? grads + L.slope : nullptr);
    ESPT_CHECK("parameter gradients");
    if (up != nullptr || tap != nullptr) {
        const int c_lo = tap != nullptr ? 0 : ca, c_hi = up != nullptr ? L.cin : ca;
        // (a tap without what lies behind it is never asked for: up is null only at the cut, where tap is null too)
        k_espt_dx<<<grid_px(P, (c_hi - c_lo + ESPT_CI_T - 1) / ESPT_CI_T, T), ESP_THREADS, 0, st>>>(d, params + L.w, pw.scale, L.cin, L.cout, ca,
                                                                                                 c_lo, P, tap, up);
        ESPT_CHECK("data-side conv");
    }
    return TMPNN_OK;
}

}  // namespace

extern "C" size_t tmpnn_espnet_train_param_floats(int C) {
    if (C < 1 || C > ESP_MAX_C) return 0;
    return train_table(C).floats;
}

extern "C" int tmpnn_espnet_train_table(int C, int64_t* rows, int cap) {
    TM_REQUIRE(C >= 1 && C <= ESP_MAX_C, "espnet_train_table: C=%d (1 .. %d)", C, ESP_MAX_C);
    TM_REQUIRE(cap == 0 || rows != nullptr, "espnet_train_table: null rows");
    const TrainTable t = train_table(C);
    Net n;
    // (walk_arena leaves null pointers on a null base: the segments' offsets are read off a base that is never dereferenced)
    const float* const base = reinterpret_cast<const float*>(uintptr_t(16));
    walk_arena(base, C, n);
    auto off = [&](const float* p) { return (int64_t)(p - base); };
    const int64_t tab[ESPT_NT][3] = {
        {t.l3.w, (int64_t)C * ESP_PSP, off(n.proj3.wt)}, {t.l3.bnw, C, off(n.proj3.scale)}, {t.l3.bnb, C, off(n.proj3.shift)},
        {t.l3.slope, C, off(n.proj3.slope)},
        {t.l2.w, (int64_t)C * (64 + C), off(n.proj2.wt)}, {t.l2.bnw, C, off(n.proj2.scale)}, {t.l2.bnb, C, off(n.proj2.shift)},
        {t.l2.slope, C, off(n.proj2.slope)},
        {t.l1.w, (int64_t)C * (32 + C), off(n.proj1.wt)}};
    for (int i = 0; i < ESPT_NT && i < cap; ++i)
        for (int j = 0; j < 3; ++j) rows[i * 3 + j] = tab[i][j];
    return ESPT_NT;
}

extern "C" size_t tmpnn_espnet_train_ws_bytes(int T, int H, int W, int C) {
    if (!shape_ok(T, H, W, C)) return 0;
    TrainWs w;
    return walk_train_ws(nullptr, T, H, W, C, w);
}

extern "C" size_t tmpnn_espnet_train_bwd_ws_bytes(int T, int H, int W, int C) {
    if (!shape_ok(T, H, W, C)) return 0;
    BwdWs b;
    return walk_bwd_ws(nullptr, T, H, W, C, b);
}

extern "C" int tmpnn_espnet_refold(float* arena, int C, const float* params, const float* stats, tmpnn_stream stream) {
    TM_REQUIRE(C >= 1 && C <= ESP_MAX_C, "espnet_refold: C=%d (1 .. %d)", C, ESP_MAX_C);
    TM_REQUIRE(arena != nullptr && params != nullptr && stats != nullptr, "espnet_refold: null pointer (arena, params, stats)");
    const TrainTable t = train_table(C);
    Net n;
    walk_arena(arena, C, n);
    RefoldArgs a;
    const TrainLayer* ls[3] = {&t.l3, &t.l2, &t.l1};
    const Pw* ps[3] = {&n.proj3, &n.proj2, &n.proj1};
    int most = 0;
    for (int i = 0; i < 3; ++i) {
        const TrainLayer& L = *ls[i];
        RefoldLayer& r = a.l[i];
        const bool act = L.bnw >= 0;
        r.w = params + L.w;
        r.bnw = act ? params + L.bnw : nullptr, r.bnb = act ? params + L.bnb : nullptr, r.slope = act ? params + L.slope : nullptr;
        r.mean = act ? stats + L.mean : nullptr, r.var = act ? stats + L.var : nullptr;
        r.wt = const_cast<float*>(ps[i]->wt), r.scale = const_cast<float*>(ps[i]->scale), r.shift = const_cast<float*>(ps[i]->shift);
        r.slope_out = const_cast<float*>(ps[i]->slope);
        r.cin = L.cin, r.cout = L.cout;
        most = std::max(most, L.cin * L.cout + L.cout);
    }
    k_espt_refold<<<dim3((most + ESP_THREADS - 1) / ESP_THREADS, 3), ESP_THREADS, 0, as_stream(stream)>>>(a);
    return check_launch("espnet_refold");
}

extern "C" int tmpnn_espnet_train_fwd(const float* arena, int C, const float* images, int T, int H, int W, void* ws, size_t ws_bytes,
                                      float* out, tmpnn_stream stream) {
    if (int rc = check_call("espnet_train_fwd", arena, images, ws, out, T, H, W, C)) return rc;
    Net n;
    walk_arena(arena, C, n);
    TrainWs w;
    const size_t need = walk_train_ws(ws, T, H, W, C, w);
    if (ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "espnet_train_fwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if (int rc = run_trunk(n, w.s, images, T, H, W, C, as_stream(stream), w.pre3)) return rc;
    return run_tail(n, w.s, T, H, W, C, out, as_stream(stream), w.pre2);
}

extern "C" int tmpnn_espnet_train_bwd(const float* arena, int C, const float* params, const float* stats, int T, int H, int W, const void* ws,
                                      size_t ws_bytes, const float* d_out, void* bws, size_t bws_bytes, float* grads, float* d_l1,
                                      float* d_l2, tmpnn_stream stream) {
    if (int rc = check_call("espnet_train_bwd", arena, d_out, ws, bws, T, H, W, C)) return rc;
    TM_REQUIRE(params != nullptr && stats != nullptr && grads != nullptr, "espnet_train_bwd: null pointer (params, stats, grads)");
    TM_REQUIRE((d_l1 == nullptr) == (d_l2 == nullptr), "espnet_train_bwd: d_l1 and d_l2 are given together or not at all");
    Net n;
    walk_arena(arena, C, n);
    TrainWs w;
    const size_t need = walk_train_ws(const_cast<void*>(ws), T, H, W, C, w);
    if (ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "espnet_train_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    BwdWs b;
    const size_t bneed = walk_bwd_ws(bws, T, H, W, C, b);
    if (bws_bytes < bneed) return set_error(TMPNN_EWORKSPACE, "espnet_train_bwd: backward workspace of %zu bytes, %zu needed", bws_bytes, bneed);
    const TrainTable t = train_table(C);
    hipStream_t st = as_stream(stream);
    const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8;
    const int P2 = h2 * w2, P4 = h4 * w4, P8 = h8 * w8;
    k_espt_up2_adj<<<grid_px(P2, C, T), ESP_THREADS, 0, st>>>(d_out, h2, w2, b.d_m1);
    ESPT_CHECK("resize adjoint");
    if (int rc = bwd_layer(t.l1, n.proj1, params, stats, grads, b.d_m1, nullptr, w.s.l1, 32, w.s.up2, T, P2, b, d_l1, b.d_up2, st)) return rc;
    k_espt_up2_adj<<<grid_px(P4, C, T), ESP_THREADS, 0, st>>>(b.d_up2, h4, w4, b.d_m2);
    ESPT_CHECK("resize adjoint");
    if (int rc = bwd_layer(t.l2, n.proj2, params, stats, grads, b.d_m2, w.pre2, w.s.l2, 64, w.s.up3, T, P4, b, d_l2, b.d_up3, st)) return rc;
    k_espt_up2_adj<<<grid_px(P8, C, T), ESP_THREADS, 0, st>>>(b.d_up3, h8, w8, b.d_m3);
    ESPT_CHECK("resize adjoint");
    // the cut: merge_l3 and everything in front of it is frozen, so nothing is carried past project_l3
    return bwd_layer(t.l3, n.proj3, params, stats, grads, b.d_m3, w.pre3, w.s.pspo, ESP_PSP, nullptr, T, P8, b, nullptr, nullptr, st);
}
