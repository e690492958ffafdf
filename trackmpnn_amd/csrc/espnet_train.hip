// Training the embedding CNN's decoder on the device, encoder frozen (tmpnn_espnet_train_param_floats, tmpnn_espnet_train_table,
// tmpnn_espnet_train_ws_bytes, tmpnn_espnet_train_bwd_ws_bytes, tmpnn_espnet_refold, tmpnn_espnet_train_fwd,
// tmpnn_espnet_train_bwd, and the tmpnn_espnet_dec_* siblings of the seven; include/tmpnn.h; host definition:
// trackmpnn_amd.espnet.espnet_decoder_grads_host).
//
// The function differentiated is the eval forward of espnet_net.h: running statistics, Dropout2d the identity.  The first part of
// this file trains the decoder BEHIND merge_l3: project_l3 / act_l3, project_l2 and project_l1 (9 tensors); pspMod and proj_L4_C
// are frozen with the encoder, and the gradients handed back are those at the encoder taps out_l1 and out_l2.  The second part
// (from "The whole decoder" on) trains all 36 tensors with the same kernels for the tail, in the same order, and carries on.
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
    int groups = 1;                              // the conv weight is [cout][cin / groups]
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
// dz [T][cout][P]; x: channels [0, ca) from a [T][ca][P], [ca, cin) from b [T][cin - ca][P]; part [chunks][cout][kg] float64, kg = cin /
// groups the input channels of a group (output channel co of group g pairs with the inputs g kg .. g kg + kg - 1 only).
// grid (chunks, tiles_co * tiles_ci of one group, groups)
__global__ __launch_bounds__(ESP_THREADS) void k_espt_wsum(const float* __restrict__ dz, const float* __restrict__ a, int ca,
                                                           const float* __restrict__ b, int cin, int cout, int T, int P, int chunk,
                                                           double* __restrict__ part) {
    __shared__ float sd[ESPT_PK][ESPT_TILE + 1];
    __shared__ float sx[ESPT_PK][ESPT_TILE + 1];
    const int groups = gridDim.z, g = blockIdx.z, kg = cin / groups, cpg = cout / groups;
    const int tiles_ci = (kg + ESPT_TILE - 1) / ESPT_TILE;
    const int tco = blockIdx.y / tiles_ci, tci = blockIdx.y - tco * tiles_ci;
    const int co0 = tco * ESPT_TILE, ci0 = tci * ESPT_TILE;       // within the group
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
                const int co = g * cpg + co0 + ch, ci = g * kg + ci0 + ch;
                float vd = 0.0f, vx = 0.0f;
                if (gp < p1) {
                    if (co0 + ch < cpg) vd = dz[((size_t)t * cout + co) * P + gp];
                    if (ci0 + ch < kg) vx = ci < ca ? a[((size_t)t * ca + ci) * P + gp] : b[((size_t)t * (cin - ca) + (ci - ca)) * P + gp];
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
    double* o = part + (size_t)blockIdx.x * cout * kg;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + ty * 4 + i, ci = ci0 + tx * 4 + j;
            if (co < cpg && ci < kg) o[(size_t)(g * cpg + co) * kg + ci] = acc[i][j];
        }
}

// One workgroup per output channel.  w [cout][cin] the layer's conv weight (cin: the input channels of one group); bnw null: no norm
// and no activation (project_l1).  part_w [chunks_w][cout][cin], part_a [cout][chunks_a][2].  Gradients are added into g_*.
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
// up [T][cin - ca][P].  grid (pixels, tiles of ESPT_CI_T over [c_lo, cin), T); c_lo is 0 or ca.  A grouped conv (w [cout][cin /
// groups]) sums over the output channels of the tile's group only; a tile never straddles two groups (the host checks that
// ESPT_CI_T divides cin / groups and c_lo).
__global__ __launch_bounds__(ESP_THREADS) void k_espt_dx(const float* __restrict__ dz, const float* __restrict__ w,
                                                         const float* __restrict__ scale, int cin, int cout, int groups, int ca, int c_lo,
                                                         int P, float* __restrict__ tap, float* __restrict__ up) {
    const int pix = blockIdx.x * ESP_THREADS + threadIdx.x;
    const int ci0 = c_lo + blockIdx.y * ESPT_CI_T;
    const int nci = min(ESPT_CI_T, cin - ci0);
    const int kg = cin / groups, cpg = cout / groups, g = ci0 / kg;
    const int cb = g * cpg, k0 = ci0 - g * kg;   // the group's first output channel; the tile's first column of w
    const size_t t = blockIdx.z;
    const bool live = pix < P;
    const int px = live ? pix : 0;
    float acc[ESPT_CI_T];
#pragma unroll
    for (int j = 0; j < ESPT_CI_T; ++j) acc[j] = 0.0f;
    const float* src = dz + t * cout * P + px;
#pragma unroll 4
    for (int co = cb; co < cb + cpg; ++co) {
        const float v = src[(size_t)co * P] * scale[co];
        const float* wr = w + (size_t)co * kg + k0;
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
    const int kg = L.cin / L.groups, cpg = L.cout / L.groups;
    const int tiles = ((cpg + ESPT_TILE - 1) / ESPT_TILE) * ((kg + ESPT_TILE - 1) / ESPT_TILE);
    k_espt_wsum<<<dim3(nch, tiles, L.groups), ESP_THREADS, 0, st>>>(d, xa, ca, xb, L.cin, L.cout, T, P, chunk, b.part_w);
    ESPT_CHECK("weight-side reduction");
    k_espt_fin<<<dim3(L.cout), ESP_THREADS, 0, st>>>(b.part_w, nch, b.part_a, nch, params + L.w, act ? params + L.bnw : nullptr,
                                                     act ? stats + L.mean : nullptr, act ? stats + L.var : nullptr, kg, L.cout,
                                                     grads + L.w, act ? grads + L.bnw : nullptr, act ? grads + L.bnb : nullptr,
                                                     act ? grads + L.slope : nullptr);
    ESPT_CHECK("parameter gradients");
    if (up != nullptr || tap != nullptr) {
        const int c_lo = tap != nullptr ? 0 : ca, c_hi = up != nullptr ? L.cin : ca;
        // (a tap without what lies behind it is never asked for: up is null only at the cut, where tap is null too)
        k_espt_dx<<<grid_px(P, (c_hi - c_lo + ESPT_CI_T - 1) / ESPT_CI_T, T), ESP_THREADS, 0, st>>>(d, params + L.w, pw.scale, L.cin, L.cout, L.groups,
                                                                                                 ca, c_lo, P, tap, up);
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
    TrainKeep keep;
    keep.pre3 = w.pre3;
    if (int rc = run_trunk(n, w.s, images, T, H, W, C, as_stream(stream), keep)) return rc;
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

// ======================================================================================================================================
// The whole decoder (tmpnn_espnet_dec_param_floats, tmpnn_espnet_dec_table, tmpnn_espnet_dec_ws_bytes, tmpnn_espnet_dec_bwd_ws_bytes,
// tmpnn_espnet_dec_refold, tmpnn_espnet_dec_fwd, tmpnn_espnet_dec_bwd): all 36 tensors of the decoder trained, the encoder frozen, the
// gradients handed back those at the four encoder taps.  The tail behind merge_l3 is the code above, launch for launch; this part
// carries the gradient on from act_l3's pre-activation:
//   k_espt_dx           project_l3's data side gives d merge_l3
//   pspMod.1.project    k_espt_act / k_espt_wsum / k_espt_fin / k_espt_dx over the five-slot PSP buffer
//   the PSP stages, k = 3 .. 0
//     k_espd_resize_adj adjoint of the general align_corners resize (hp, wp) -> (h8, w8) in gather form: a thread owns a pooled
//                       pixel and walks the outputs that read it, their weights formed by the forward's esp_axis
//     k_espd_dw_wsum    the weight side of a depthwise 3x3: a workgroup per channel, nine float64 sums over images and pixels
//     k_espd_dw_adj     the data side (the taps mirrored) plus the adjoint of the 3x3 / stride 2 average pool of the next stage's
//                       pooled map: d pooled_k = dw^T(up^T(d slot_{k+1})) + pool^T(d pooled_{k+1}); with no depthwise part and
//                       d slot_0 added it gives d feats
//   pspMod.0 (EESP)     conv_1x1_exp / module_act by the pointwise kernels with groups; k_espd_cat_bwd recomputes the four fused
//                       branches from the reduced map in k_esp_dw's order, takes br_after_cat's PReLU and norm (float64 partials
//                       per plane chunk, finished by k_espd_cat_fin) and leaves d conv_k, the suffix sums of d out_j, in place;
//                       k_espd_dw_wsum / k_espd_dw_adj with the dilations 1 1 2 3 give the depthwise gradients and d red;
//                       proj_1x1 by the pointwise kernels with groups: the cat splits by pointer into the tap out_l3 and the
//                       gradient of the upsampled proj_L4_C map
//   k_espt_up2_adj, then proj_L4_C by the pointwise kernels: its data side is the tap out_l4
// 48 launches whatever T is (47 without the taps); no atomics; every tensor is finished by one owner that adds into the flat gradient.
namespace {

constexpr int ESPD_NT = 36;                      // trained tensors
constexpr int ESPD_N = ESP_PSP / 4;              // reduced channels of pspMod.0

struct DecTable {
    TrainLayer p4, red, exp, psp, l3, l2, l1;    // proj_L4_C, pspMod.0.proj_1x1, pspMod.0.conv_1x1_exp (slope: module_act), pspMod.1.project
    long dw;                                     // pspMod.0.spp_dw.0 .. 3 [4][32][9]
    long cat_bnw, cat_bnb, cat_slope, cat_mean, cat_var;              // pspMod.0.br_after_cat
    long stage[4];                               // pspMod.1.stages.k [128][9]
    size_t floats;
};
DecTable dec_table(int C) {
    DecTable t;
    long o = 0, so = 0;
    auto take = [&](long n) { const long at = o; o += n; return at; };
    auto stat = [&](long n) { const long at = so; so += n; return at; };
    auto layer = [&](TrainLayer& L, int cin, int cout, int groups, bool norm) {
        L.cin = cin, L.cout = cout, L.groups = groups;
        L.w = take((long)cout * (cin / groups));
        L.bnw = L.bnb = L.slope = L.mean = L.var = -1;
        if (norm) L.bnw = take(cout), L.bnb = take(cout), L.mean = stat(cout), L.var = stat(cout);
    };
    layer(t.p4, 256, ESP_PSP, 1, true), t.p4.slope = take(ESP_PSP);
    layer(t.red, 2 * ESP_PSP, ESPD_N, 4, true), t.red.slope = take(ESPD_N);
    t.dw = take(4 * ESPD_N * 9);
    layer(t.exp, ESP_PSP, ESP_PSP, 4, true);
    t.cat_bnw = take(ESP_PSP), t.cat_bnb = take(ESP_PSP), t.cat_mean = stat(ESP_PSP), t.cat_var = stat(ESP_PSP);
    t.cat_slope = take(ESP_PSP);
    t.exp.slope = take(ESP_PSP);
    for (long& s : t.stage) s = take(ESP_PSP * 9);
    layer(t.psp, 5 * ESP_PSP, ESP_PSP, 1, true), t.psp.slope = take(ESP_PSP);
    layer(t.l3, ESP_PSP, C, 1, true), t.l3.slope = take(C);
    layer(t.l2, 64 + C, C, 1, true), t.l2.slope = take(C);
    layer(t.l1, 32 + C, C, 1, false);
    t.floats = (size_t)o;
    return t;
}

// ---- refold ----------------------------------------------------------------------------------------------------------------
enum { ESPD_TRANSPOSE = 0, ESPD_COPY = 1, ESPD_FOLD = 2 };
struct DecRefoldOp {                             // TRANSPOSE: dst [n / cout][cout] = src [cout][n / cout]; COPY: dst [n] = src [n];
    const float *src, *b, *mean, *var;           // FOLD: (dst, dst2) [n] = the folded scale and shift of (src, b, mean, var)
    float *dst, *dst2;
    int kind, n, cout;
};
constexpr int ESPD_OPS = 26;
struct DecRefoldArgs { DecRefoldOp op[ESPD_OPS]; };

__global__ __launch_bounds__(ESP_THREADS) void k_espd_refold(DecRefoldArgs a) {
    const DecRefoldOp& o = a.op[blockIdx.y];
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx >= o.n) return;
    if (o.kind == ESPD_TRANSPOSE) {
        const int k = idx / o.cout, co = idx - k * o.cout;
        o.dst[idx] = o.src[(size_t)co * (o.n / o.cout) + k];
    } else if (o.kind == ESPD_COPY) {
        o.dst[idx] = o.src[idx];
    } else {
        float sc, sh;
        espt_fold((double)o.src[idx], (double)o.b[idx], (double)o.mean[idx], (double)o.var[idx], sc, sh);
        o.dst[idx] = sc, o.dst2[idx] = sh;
    }
}

// ---- adjoint of the general resize -------------------------------------------------------------------------------------------
// the outputs lo .. hi of an axis n_in -> n_out that can read source s: floor(o (n_in - 1) / (n_out - 1)) is s - 1 or s
__device__ __forceinline__ void espd_readers(int s, int n_in, int n_out, int& lo, int& hi) {
    if (n_in <= 1 || n_out <= 1) {               // esp_axis: every output reads index 0
        lo = 0, hi = n_out - 1;
        return;
    }
    const int m = n_in - 1, den = n_out - 1;
    lo = s == 0 ? 0 : ((s - 1) * den + m - 1) / m;
    hi = min(n_out - 1, ((s + 1) * den + m - 1) / m - 1);
}

// dy [T][..][C][ho][wo] (batch stride dy_bs) -> dx [T][C][hi][wi]; grid (pixels of the source, C, T)
__global__ __launch_bounds__(ESP_THREADS) void k_espd_resize_adj(const float* __restrict__ dy, size_t dy_bs, int ho, int wo, int hi, int wi,
                                                                 float* __restrict__ dx) {
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx >= hi * wi) return;
    const int sy = idx / wi, sx = idx - sy * wi, c = blockIdx.y, C = gridDim.y;
    const float* p = dy + (size_t)blockIdx.z * dy_bs + (size_t)c * ho * wo;
    int ylo, yhi, xlo, xhi;
    espd_readers(sy, hi, ho, ylo, yhi);
    espd_readers(sx, wi, wo, xlo, xhi);
    float g = 0.0f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = espt_axis_w(oy, sy, hi, ho);
        if (wy == 0.0f) continue;
        float r = 0.0f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const float wx = espt_axis_w(ox, sx, wi, wo);
            if (wx != 0.0f) r = fmaf(wx, p[(size_t)oy * wo + ox], r);
        }
        g = fmaf(wy, r, g);
    }
    dx[((size_t)blockIdx.z * C + c) * hi * wi + idx] = g;
}

// ---- depthwise 3x3: data side (+ the pool's adjoint) and weight side -----------------------------------------------------------
// out[t][c][p] = add[t][c][p] + sum_{k < K} sum_uv w[k n + c][u][v] dD[t][k n + c][p - dil_k (u, v)] + (sum over the pooled pixels
// q whose 3x3 / stride 2 / pad 1 window holds p of dq[t][c][q]) / 9; n = gridDim.y; add (batch stride add_bs) and dq [T][n][hq][wq]
// may be null, K may be 0.  out [T][n][h][w]; grid (pixels, n, T)
__global__ __launch_bounds__(ESP_THREADS) void k_espd_dw_adj(const float* __restrict__ add, size_t add_bs, const float* __restrict__ dD, int K,
                                                             int h, int w, const float* __restrict__ wgt, int d0, int d1, int d2, int d3,
                                                             const float* __restrict__ dq, int hq, int wq, float* __restrict__ out) {
    const int idx = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (idx >= h * w) return;
    const int y = idx / w, x = idx - y * w, c = blockIdx.y, n = gridDim.y;
    const size_t t = blockIdx.z, P = (size_t)h * w;
    const int dil[4] = {d0, d1, d2, d3};
    float g = add ? add[t * add_bs + (size_t)c * P + idx] : 0.0f;
    for (int k = 0; k < K; ++k) {
        const float* p = dD + (t * K * n + (size_t)k * n + c) * P;
        const float* w9 = wgt + ((size_t)k * n + c) * 9;
        const int d = dil[k];
        float s = 0.0f;
#pragma unroll
        for (int u = -1; u <= 1; ++u)
#pragma unroll
            for (int v = -1; v <= 1; ++v) {
                const int iy = y - u * d, ix = x - v * d;
                if (iy >= 0 && iy < h && ix >= 0 && ix < w) s = fmaf(w9[(u + 1) * 3 + (v + 1)], p[iy * w + ix], s);
            }
        g += s;
    }
    if (dq) {
        const float* q = dq + (t * n + c) * (size_t)hq * wq;
        float s = 0.0f;
#pragma unroll
        for (int a = -1; a <= 1; ++a) {
            const int ny = y - a;                // 2 qy + a = y
#pragma unroll
            for (int b = -1; b <= 1; ++b) {
                const int nx = x - b;
                if (ny >= 0 && nx >= 0 && !(ny & 1) && !(nx & 1) && ny / 2 < hq && nx / 2 < wq) s += q[(ny / 2) * wq + nx / 2];
            }
        }
        g += s / 9.0f;
    }
    out[(t * n + c) * P + idx] = g;
}

// g_w[cc][u][v] += sum over images and pixels of dD[t][cc][p] src[t][cc % n][p + dil_{cc / n} (u, v)]; dD [T][CC][h][w], src
// [T][n][h][w]; one workgroup per cc of CC = gridDim.x; float64 throughout, a thread's pixels in order, then the fixed tree
__global__ __launch_bounds__(ESP_THREADS) void k_espd_dw_wsum(const float* __restrict__ dD, const float* __restrict__ src, int n, int h, int w,
                                                              int d0, int d1, int d2, int d3, int T, float* g_w) {
    __shared__ double red[ESP_THREADS];
    const int cc = blockIdx.x, CC = gridDim.x, k = cc / n, c = cc - k * n, P = h * w;
    const int d = k == 0 ? d0 : k == 1 ? d1 : k == 2 ? d2 : d3;
    double acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = 0.0;
    for (int t = 0; t < T; ++t) {
        const float* pd = dD + ((size_t)t * CC + cc) * P;
        const float* ps = src + ((size_t)t * n + c) * P;
        for (int p = threadIdx.x; p < P; p += ESP_THREADS) {
            const double g = (double)pd[p];
            const int y = p / w, x = p - y * w;
#pragma unroll
            for (int u = -1; u <= 1; ++u)
#pragma unroll
                for (int v = -1; v <= 1; ++v) {
                    const int iy = y + u * d, ix = x + v * d;
                    if (iy >= 0 && iy < h && ix >= 0 && ix < w) acc[(u + 1) * 3 + (v + 1)] += g * (double)ps[iy * w + ix];
                }
        }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const double r = espt_block_sum(acc[j], red);
        if (threadIdx.x == 0) g_w[(size_t)cc * 9 + j] += (float)r;
    }
}

// ---- br_after_cat of the EESP ------------------------------------------------------------------------------------------------
// d [T][4 n][P]: d cat in, d conv_k out (conv_k the k-th dilated depthwise conv: out_k = conv_k + out_{k-1}, so d conv_k is the sum
// of d out_j over j >= k).  red [T][n][P] the reduced map; the branches are recomputed as k_esp_dw forms them.  part [4 n][chunks][3]:
// (sum dz, sum over pre <= 0 of dy pre, sum dz out_k), dz the gradient in front of the PReLU.  grid (chunks, n)
__global__ __launch_bounds__(ESP_THREADS) void k_espd_cat_bwd(float* d, const float* __restrict__ rmap, int n, int h, int w,
                                                              const float* __restrict__ wdw, int d0, int d1, int d2, int d3,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              const float* __restrict__ slope, int T, int chunk, double* __restrict__ part) {
    __shared__ double red[ESP_THREADS];
    const int c = blockIdx.y, P = h * w;
    const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
    const int dil[4] = {d0, d1, d2, d3};
    double acc[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
    for (int t = 0; t < T; ++t) {
        const float* r = rmap + ((size_t)t * n + c) * P;
        float* dt = d + (size_t)t * 4 * n * P;
        for (int p = p0 + threadIdx.x; p < p1; p += ESP_THREADS) {
            const int y = p / w, x = p - y * w;
            float run = 0.0f, dr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int dd = dil[k], co = k * n + c;
                const float* wk = wdw + (size_t)co * 9;
                float s = 0.0f;
#pragma unroll
                for (int u = -1; u <= 1; ++u)
#pragma unroll
                    for (int v = -1; v <= 1; ++v) {
                        const int iy = y + u * dd, ix = x + v * dd;
                        const float val = (iy >= 0 && iy < h && ix >= 0 && ix < w) ? r[iy * w + ix] : 0.0f;
                        s = fmaf(wk[(u + 1) * 3 + (v + 1)], val, s);
                    }
                run = k == 0 ? s : s + run;
                const float pre = run * scale[co] + shift[co];
                const float g = dt[(size_t)co * P + p];
                const float dz = pre > 0.0f ? g : slope[co] * g;
                acc[k][0] += (double)dz;
                if (!(pre > 0.0f)) acc[k][1] += (double)g * (double)pre;
                acc[k][2] += (double)dz * (double)run;
                dr[k] = dz * scale[co];
            }
            float suf = dr[3];
            dt[((size_t)3 * n + c) * P + p] = suf;
#pragma unroll
            for (int k = 2; k >= 0; --k) {
                suf = dr[k] + suf;
                dt[((size_t)k * n + c) * P + p] = suf;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double v = espt_block_sum(acc[k][j], red);
            if (threadIdx.x == 0) part[((size_t)(k * n + c) * gridDim.x + blockIdx.x) * 3 + j] = v;
        }
}

// a thread per channel: pre = out_k s + (b - m s), s = w / sqrt(v + eps): d bn.weight = (sum dz out_k - m sum dz) / sqrt(v + eps)
__global__ __launch_bounds__(ESP_THREADS) void k_espd_cat_fin(const double* __restrict__ part, int chunks, int c4, const float* __restrict__ mean,
                                                              const float* __restrict__ var, float* g_bnw, float* g_bnb, float* g_slope) {
    const int co = blockIdx.x * ESP_THREADS + threadIdx.x;
    if (co >= c4) return;
    double sz = 0.0, sa = 0.0, sr = 0.0;
    for (int k = 0; k < chunks; ++k) {
        const double* q = part + ((size_t)co * chunks + k) * 3;
        sz += q[0], sa += q[1], sr += q[2];
    }
    const double inv = 1.0 / sqrt((double)var[co] + ESPT_EPS);
    g_bnb[co] += (float)sz;
    g_bnw[co] += (float)((sr - (double)mean[co] * sz) * inv);
    g_slope[co] += (float)sa;
}

// ---- workspaces ------------------------------------------------------------------------------------------------------------
struct PspDims { int h[4], w[4]; size_t px; };   // the pooled maps of the PSP chain and their pixels in all
PspDims psp_dims(int H, int W) {
    PspDims d;
    int h = H / 8, w = W / 8;
    d.px = 0;
    for (int k = 0; k < 4; ++k) {
        h = (h + 1) / 2, w = (w + 1) / 2;
        d.h[k] = h, d.w[k] = w, d.px += (size_t)h * w;
    }
    return d;
}

struct DecWs {
    TrainWs t;
    TrainKeep keep;
};
size_t walk_dec_ws(void* base, int T, int H, int W, int C, DecWs& w) {
    const size_t tail = walk_train_ws(base, T, H, W, C, w.t);
    WsCarver cv{reinterpret_cast<char*>(base) + align16(tail)};
    const size_t t = (size_t)T, P8 = (size_t)(H / 8) * (W / 8), P16 = P8 / 4;
    const PspDims pd = psp_dims(H, W);
    w.keep.pre3 = w.t.pre3;
    w.keep.pre4 = cv.take<float>(t * ESP_PSP * P16), w.keep.pre_red = cv.take<float>(t * ESPD_N * P8);
    w.keep.pre_exp = cv.take<float>(t * ESP_PSP * P8), w.keep.pre_psp = cv.take<float>(t * ESP_PSP * P8);
    for (int k = 0; k < 4; ++k) w.keep.pooled[k] = cv.take<float>(t * ESP_PSP * pd.h[k] * pd.w[k]);
    return (size_t)(cv.p - reinterpret_cast<char*>(base));
}

struct DecBwdWs {
    BwdWs t;                                     // the tail's maps, and the partial sums sized for every layer of the decoder
    float *d_pspo, *d_psp, *d_u, *dq_a, *dq_b, *d_feats, *d_cat, *d_red, *d_up4, *d_p4;
    double* part_c;
};
size_t walk_dec_bwd_ws(void* base, int T, int H, int W, int C, DecBwdWs& b) {
    WsCarver cv{reinterpret_cast<char*>(base)};
    const size_t t = (size_t)T, P2 = (size_t)(H / 2) * (W / 2), P4 = P2 / 4, P8 = P4 / 4, P16 = P8 / 4;
    const PspDims pd = psp_dims(H, W);
    const size_t Pp = (size_t)pd.h[0] * pd.w[0];
    b.t.d_m1 = cv.take<float>(t * C * P2), b.t.d_up2 = cv.take<float>(t * C * P2);
    b.t.d_m2 = cv.take<float>(t * C * P4), b.t.d_up3 = cv.take<float>(t * C * P4);
    b.t.d_m3 = cv.take<float>(t * C * P8);
    const size_t c = (size_t)C, psp = ESP_PSP;
    const size_t pw = std::max({(size_t)chunks_of(P2) * c * (32 + c), (size_t)chunks_of(P4) * c * (64 + c), (size_t)chunks_of(P8) * c * psp,
                                (size_t)chunks_of(P8) * psp * 5 * psp, (size_t)chunks_of(P16) * psp * 256});
    b.t.part_w = cv.take<double>(pw);
    b.t.part_a = cv.take<double>(std::max(c, psp) * ESPT_MAX_CHUNKS * 2);
    b.d_pspo = cv.take<float>(t * psp * P8), b.d_psp = cv.take<float>(t * 5 * psp * P8);
    b.d_u = cv.take<float>(t * psp * Pp), b.dq_a = cv.take<float>(t * psp * Pp), b.dq_b = cv.take<float>(t * psp * Pp);
    b.d_feats = cv.take<float>(t * psp * P8), b.d_cat = cv.take<float>(t * psp * P8), b.d_red = cv.take<float>(t * ESPD_N * P8);
    b.d_up4 = cv.take<float>(t * psp * P8), b.d_p4 = cv.take<float>(t * psp * P16);
    b.part_c = cv.take<double>(psp * ESPT_MAX_CHUNKS * 3);
    return (size_t)(cv.p - reinterpret_cast<char*>(base));
}

#undef ESPT_CHECK
#define ESPT_CHECK(what)                                                \
    do {                                                                \
        if (int rc_ = check_launch("espnet_dec_bwd (" what ")")) return rc_; \
    } while (0)

// the encoder outputs the decoder reads: run_trunk swaps its two buffers once per EESP of the level
const float* enc_l3(const Net& n, const Ws& s) { return (sizeof(n.l3) / sizeof(n.l3[0])) % 2 ? s.l3b : s.l3a; }
const float* enc_l4(const Net& n, const Ws& s) { return (sizeof(n.l4) / sizeof(n.l4[0])) % 2 ? s.l4b : s.l4a; }

}  // namespace

extern "C" size_t tmpnn_espnet_dec_param_floats(int C) {
    if (C < 1 || C > ESP_MAX_C) return 0;
    return dec_table(C).floats;
}

extern "C" int tmpnn_espnet_dec_table(int C, int64_t* rows, int cap) {
    TM_REQUIRE(C >= 1 && C <= ESP_MAX_C, "espnet_dec_table: C=%d (1 .. %d)", C, ESP_MAX_C);
    TM_REQUIRE(cap == 0 || rows != nullptr, "espnet_dec_table: null rows");
    const DecTable t = dec_table(C);
    Net n;
    const float* const base = reinterpret_cast<const float*>(uintptr_t(16));      // (never dereferenced: tmpnn_espnet_train_table)
    walk_arena(base, C, n);
    auto off = [&](const float* p) { return (int64_t)(p - base); };
    int i = 0;
    auto row = [&](long at, int64_t cnt, const float* seg) {
        if (i < cap) rows[i * 3] = at, rows[i * 3 + 1] = cnt, rows[i * 3 + 2] = off(seg);
        ++i;
    };
    auto layer = [&](const TrainLayer& L, const Pw& p, bool slope) {
        row(L.w, (int64_t)L.cout * (L.cin / L.groups), p.wt);
        if (L.bnw >= 0) row(L.bnw, L.cout, p.scale), row(L.bnb, L.cout, p.shift);
        if (slope) row(L.slope, L.cout, p.slope);
    };
    layer(t.p4, n.proj4, true);
    layer(t.red, n.psp_e.proj, true);
    for (int k = 0; k < 4; ++k) row(t.dw + (long)k * ESPD_N * 9, ESPD_N * 9, n.psp_e.dw.w + (size_t)k * ESPD_N * 9);
    layer(t.exp, n.psp_e.exp, false);
    row(t.cat_bnw, ESP_PSP, n.psp_e.dw.scale), row(t.cat_bnb, ESP_PSP, n.psp_e.dw.shift), row(t.cat_slope, ESP_PSP, n.psp_e.dw.slope);
    row(t.exp.slope, ESP_PSP, n.psp_e.exp.slope);
    for (int k = 0; k < 4; ++k) row(t.stage[k], ESP_PSP * 9, n.psp_w[k]);
    layer(t.psp, n.psp_proj, true);
    layer(t.l3, n.proj3, true);
    layer(t.l2, n.proj2, true);
    layer(t.l1, n.proj1, false);
    return i;                                    // ESPD_NT
}

extern "C" size_t tmpnn_espnet_dec_ws_bytes(int T, int H, int W, int C) {
    if (!shape_ok(T, H, W, C)) return 0;
    DecWs w;
    return walk_dec_ws(nullptr, T, H, W, C, w);
}

extern "C" size_t tmpnn_espnet_dec_bwd_ws_bytes(int T, int H, int W, int C) {
    if (!shape_ok(T, H, W, C)) return 0;
    DecBwdWs b;
    return walk_dec_bwd_ws(nullptr, T, H, W, C, b);
}

extern "C" int tmpnn_espnet_dec_refold(float* arena, int C, const float* params, const float* stats, tmpnn_stream stream) {
    TM_REQUIRE(C >= 1 && C <= ESP_MAX_C, "espnet_dec_refold: C=%d (1 .. %d)", C, ESP_MAX_C);
    TM_REQUIRE(arena != nullptr && params != nullptr && stats != nullptr, "espnet_dec_refold: null pointer (arena, params, stats)");
    const DecTable t = dec_table(C);
    Net n;
    walk_arena(arena, C, n);
    DecRefoldArgs a;
    int i = 0, most = 0;
    auto put = [&](int kind, const float* src, const float* b, const float* mean, const float* var, const float* dst, const float* dst2, int cnt,
                   int cout) {
        a.op[i++] = DecRefoldOp{src, b, mean, var, const_cast<float*>(dst), const_cast<float*>(dst2), kind, cnt, cout};
        most = std::max(most, cnt);
    };
    auto copy = [&](long at, const float* dst, int cnt) { put(ESPD_COPY, params + at, nullptr, nullptr, nullptr, dst, nullptr, cnt, 1); };
    auto fold = [&](long bnw, long bnb, long mean, long var, const float* scale, const float* shift, int cnt) {
        put(ESPD_FOLD, params + bnw, params + bnb, stats + mean, stats + var, scale, shift, cnt, 1);
    };
    auto layer = [&](const TrainLayer& L, const Pw& p) {
        put(ESPD_TRANSPOSE, params + L.w, nullptr, nullptr, nullptr, p.wt, nullptr, L.cout * (L.cin / L.groups), L.cout);
        if (L.bnw >= 0) fold(L.bnw, L.bnb, L.mean, L.var, p.scale, p.shift, L.cout);
        if (L.slope >= 0) copy(L.slope, p.slope, L.cout);
    };
    layer(t.p4, n.proj4), layer(t.red, n.psp_e.proj), layer(t.exp, n.psp_e.exp), layer(t.psp, n.psp_proj);
    layer(t.l3, n.proj3), layer(t.l2, n.proj2), layer(t.l1, n.proj1);
    copy(t.dw, n.psp_e.dw.w, 4 * ESPD_N * 9);
    fold(t.cat_bnw, t.cat_bnb, t.cat_mean, t.cat_var, n.psp_e.dw.scale, n.psp_e.dw.shift, ESP_PSP);
    copy(t.cat_slope, n.psp_e.dw.slope, ESP_PSP);
    for (int k = 0; k < 4; ++k) copy(t.stage[k], n.psp_w[k], ESP_PSP * 9);
    if (i != ESPD_OPS) return set_error(TMPNN_EINVAL, "espnet_dec_refold: %d segments listed, %d expected", i, ESPD_OPS);
    k_espd_refold<<<dim3((most + ESP_THREADS - 1) / ESP_THREADS, ESPD_OPS), ESP_THREADS, 0, as_stream(stream)>>>(a);
    return check_launch("espnet_dec_refold");
}

extern "C" int tmpnn_espnet_dec_fwd(const float* arena, int C, const float* images, int T, int H, int W, void* ws, size_t ws_bytes,
                                    float* out, tmpnn_stream stream) {
    if (int rc = check_call("espnet_dec_fwd", arena, images, ws, out, T, H, W, C)) return rc;
    Net n;
    walk_arena(arena, C, n);
    DecWs w;
    const size_t need = walk_dec_ws(ws, T, H, W, C, w);
    if (ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "espnet_dec_fwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if (int rc = run_trunk(n, w.t.s, images, T, H, W, C, as_stream(stream), w.keep)) return rc;
    return run_tail(n, w.t.s, T, H, W, C, out, as_stream(stream), w.t.pre2);
}

extern "C" int tmpnn_espnet_dec_bwd(const float* arena, int C, const float* params, const float* stats, int T, int H, int W, const void* ws,
                                    size_t ws_bytes, const float* d_out, void* bws, size_t bws_bytes, float* grads, float* d_l1, float* d_l2,
                                    float* d_l3, float* d_l4, tmpnn_stream stream) {
    if (int rc = check_call("espnet_dec_bwd", arena, d_out, ws, bws, T, H, W, C)) return rc;
    TM_REQUIRE(params != nullptr && stats != nullptr && grads != nullptr, "espnet_dec_bwd: null pointer (params, stats, grads)");
    TM_REQUIRE((d_l1 == nullptr) == (d_l2 == nullptr) && (d_l1 == nullptr) == (d_l3 == nullptr) && (d_l1 == nullptr) == (d_l4 == nullptr),
               "espnet_dec_bwd: d_l1, d_l2, d_l3 and d_l4 are given together or not at all");
    static_assert(ESPD_N % ESPT_CI_T == 0 && (2 * ESP_PSP / 4) % ESPT_CI_T == 0, "a tile of k_espt_dx lies in one group");
    Net n;
    walk_arena(arena, C, n);
    DecWs w;
    const size_t need = walk_dec_ws(const_cast<void*>(ws), T, H, W, C, w);
    if (ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "espnet_dec_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    DecBwdWs b;
    const size_t bneed = walk_dec_bwd_ws(bws, T, H, W, C, b);
    if (bws_bytes < bneed) return set_error(TMPNN_EWORKSPACE, "espnet_dec_bwd: backward workspace of %zu bytes, %zu needed", bws_bytes, bneed);
    const DecTable t = dec_table(C);
    const Ws& s = w.t.s;
    const TrainKeep& kp = w.keep;
    hipStream_t st = as_stream(stream);
    const int h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8, h16 = H / 16, w16 = W / 16;
    const int P2 = h2 * w2, P4 = h4 * w4, P8 = h8 * w8, P16 = h16 * w16;
    // the tail: the launches of tmpnn_espnet_train_bwd, project_l3's data side added
    k_espt_up2_adj<<<grid_px(P2, C, T), ESP_THREADS, 0, st>>>(d_out, h2, w2, b.t.d_m1);
    ESPT_CHECK("resize adjoint");
    if (int rc = bwd_layer(t.l1, n.proj1, params, stats, grads, b.t.d_m1, nullptr, s.l1, 32, s.up2, T, P2, b.t, d_l1, b.t.d_up2, st)) return rc;
    k_espt_up2_adj<<<grid_px(P4, C, T), ESP_THREADS, 0, st>>>(b.t.d_up2, h4, w4, b.t.d_m2);
    ESPT_CHECK("resize adjoint");
    if (int rc = bwd_layer(t.l2, n.proj2, params, stats, grads, b.t.d_m2, w.t.pre2, s.l2, 64, s.up3, T, P4, b.t, d_l2, b.t.d_up3, st)) return rc;
    k_espt_up2_adj<<<grid_px(P8, C, T), ESP_THREADS, 0, st>>>(b.t.d_up3, h8, w8, b.t.d_m3);
    ESPT_CHECK("resize adjoint");
    if (int rc = bwd_layer(t.l3, n.proj3, params, stats, grads, b.t.d_m3, kp.pre3, s.pspo, ESP_PSP, nullptr, T, P8, b.t, b.d_pspo, nullptr, st))
        return rc;
    // pspMod.1.project over the five slots
    const size_t psp_bs = (size_t)5 * ESP_PSP * P8;
    if (int rc = bwd_layer(t.psp, n.psp_proj, params, stats, grads, b.d_pspo, kp.pre_psp, s.psp, 5 * ESP_PSP, nullptr, T, P8, b.t, b.d_psp, nullptr,
                           st))
        return rc;
    // the PSP stages from the smallest map up: d pooled_k = dw^T(up^T(d slot_{k+1})) + pool^T(d pooled_{k+1})
    const PspDims pd = psp_dims(H, W);
    const float* dq = nullptr;
    for (int k = 3; k >= 0; --k) {
        const int hp = pd.h[k], wp = pd.w[k];
        k_espd_resize_adj<<<grid_px((size_t)hp * wp, ESP_PSP, T), ESP_THREADS, 0, st>>>(b.d_psp + (size_t)(k + 1) * ESP_PSP * P8, psp_bs, h8, w8, hp, wp,
                                                                                     b.d_u);
        ESPT_CHECK("PSP resize adjoint");
        k_espd_dw_wsum<<<dim3(ESP_PSP), ESP_THREADS, 0, st>>>(b.d_u, kp.pooled[k], ESP_PSP, hp, wp, 1, 1, 1, 1, T, grads + t.stage[k]);
        ESPT_CHECK("PSP stage weights");
        float* dp = (k & 1) ? b.dq_a : b.dq_b;
        k_espd_dw_adj<<<grid_px((size_t)hp * wp, ESP_PSP, T), ESP_THREADS, 0, st>>>(nullptr, 0, b.d_u, 1, hp, wp, params + t.stage[k], 1, 1, 1, 1, dq,
                                                                                 k < 3 ? pd.h[k + 1] : 0, k < 3 ? pd.w[k + 1] : 0, dp);
        ESPT_CHECK("PSP stage data side");
        dq = dp;
    }
    k_espd_dw_adj<<<grid_px(P8, ESP_PSP, T), ESP_THREADS, 0, st>>>(b.d_psp, psp_bs, nullptr, 0, h8, w8, nullptr, 1, 1, 1, 1, dq, pd.h[0], pd.w[0],
                                                                b.d_feats);
    ESPT_CHECK("PSP pool adjoint");
    // pspMod.0: module_act and conv_1x1_exp, br_after_cat and the fused branches, the depthwise convs, proj_1x1
    if (int rc = bwd_layer(t.exp, n.psp_e.exp, params, stats, grads, b.d_feats, kp.pre_exp, s.cat, ESP_PSP, nullptr, T, P8, b.t, b.d_cat, nullptr, st))
        return rc;
    const int nch = chunks_of(P8), chunk = chunk_px(P8);
    const int* dl = DIL_1123;
    k_espd_cat_bwd<<<dim3(nch, ESPD_N), ESP_THREADS, 0, st>>>(b.d_cat, s.red, ESPD_N, h8, w8, params + t.dw, dl[0], dl[1], dl[2], dl[3],
                                                            n.psp_e.dw.scale, n.psp_e.dw.shift, params + t.cat_slope, T, chunk, b.part_c);
    ESPT_CHECK("br_after_cat");
    k_espd_cat_fin<<<dim3((ESP_PSP + ESP_THREADS - 1) / ESP_THREADS), ESP_THREADS, 0, st>>>(b.part_c, nch, ESP_PSP, stats + t.cat_mean, stats + t.cat_var,
                                                                                         grads + t.cat_bnw, grads + t.cat_bnb, grads + t.cat_slope);
    ESPT_CHECK("br_after_cat gradients");
    k_espd_dw_wsum<<<dim3(ESP_PSP), ESP_THREADS, 0, st>>>(b.d_cat, s.red, ESPD_N, h8, w8, dl[0], dl[1], dl[2], dl[3], T, grads + t.dw);
    ESPT_CHECK("EESP depthwise weights");
    k_espd_dw_adj<<<grid_px(P8, ESPD_N, T), ESP_THREADS, 0, st>>>(nullptr, 0, b.d_cat, 4, h8, w8, params + t.dw, dl[0], dl[1], dl[2], dl[3], nullptr, 0, 0,
                                                               b.d_red);
    ESPT_CHECK("EESP depthwise data side");
    if (int rc = bwd_layer(t.red, n.psp_e.proj, params, stats, grads, b.d_red, kp.pre_red, enc_l3(n, s), ESP_PSP, s.up4, T, P8, b.t, d_l3, b.d_up4, st))
        return rc;
    // the cat split by pointer: channels 128 .. 255 go back through the x2 resize to proj_L4_C, whose data side is the tap out_l4
    k_espt_up2_adj<<<grid_px(P16, ESP_PSP, T), ESP_THREADS, 0, st>>>(b.d_up4, h16, w16, b.d_p4);
    ESPT_CHECK("resize adjoint");
    return bwd_layer(t.p4, n.proj4, params, stats, grads, b.d_p4, kp.pre4, enc_l4(n, s), 256, nullptr, T, P16, b.t, d_l4, nullptr, st);
}
