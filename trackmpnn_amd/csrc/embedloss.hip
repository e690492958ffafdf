// The embedding loss on the device (tmpnn_embed_loss_ws, tmpnn_embed_loss_fwd, tmpnn_embed_loss_bwd; include/tmpnn.h; host
// definition: trackmpnn_amd.embedloss.embedding_loss_host).  The reference's discriminative pull-push loss (models/loss.py:118-159)
// walks the clusters of one chunk in a Python loop, the cluster pairs in a C * C loop, and asks the host for np.unique.  Here a
// cluster is the labelled rows of a chunk that share a track id, found without a sort the way k_vis_bwd finds the sharers of a
// pixel: a wave per row scans its chunk's ids 64 at a time with one ballot.  The scan is n / 64 steps a row for a chunk of n rows,
// whatever the chunk holds, so there is no limit on rows or clusters per chunk; the one limit is EL_MAX_D rows per call.
//
// k_el_chunk       one thread per row: the row's chunk = the first b whose (clamped) bounds hold it, -1: in none.  With valid
//                  offsets the chunks are disjoint; with bad ones this still makes the chunks a partition of the rows.
// k_el_leader      one wave per labelled row: the lowest row of its chunk with its id is the cluster's leader.  A wave scans the
//                  rows below its own and leaves at the first equal id; a leader scans from its row on and adds its cluster's
//                  rows in ascending order (lane l owns channels l, l + 64, ...), counts them, and stores the mean at its row.
// k_el_dist        one wave per labelled row: d_i = |x_i - mu| by an xor butterfly (every lane ends with the same bits) and the
//                  row's share relu(d_i - delta_var)^2 / n_c of the variance term.  A leader then walks the chunk's other leaders
//                  in ascending order: m = |mu_c - mu_c'|, its sum of relu(delta_dist - m)^2, the number of leaders C, and
//                  v_c = -(4 / (C (C - 1))) sum relu(delta_dist - m) (mu_c - mu_c') / m for the backward.
// k_el_reduce      one wave per chunk, as k_vis_reduce: lanes walk the chunk's rows in strides of 64 and a butterfly adds the 64
//                  partial sums, so the order depends on the chunk's bounds alone.  loss[b], the two terms, the counts.
// k_el_bwd_leader  one wave per leader: t_c = (v_c - sum_i u_i) / n_c over its rows in ascending order.
// k_el_bwd_rows    one wave per row: d_features = g[b] (u_k + t_c); unlabelled rows and rows in no chunk get zeros.
//
// No atomics anywhere: every sum has one owner and a fixed order, so the results are bitwise reproducible from run to run.
//
// Contraction is OFF for this file, so each product and each sum below is one rounded float32 operation, in the order the host
// definition states.  The results are still not the host's bit for bit in float32: the host adds the W channels of a norm and
// the rows of a chunk left to right where the device uses butterflies.  The tests compare against the host in float64 within
// a bound derived from the lengths of these sums.
//
// The rows are read with one coalesced 4-byte load per lane and 64 channels (256 contiguous bytes a wave): W and the row
// stride are run-time values without an alignment rule, and at W = 128 a 16-byte load would leave half the wave idle.
//
// Every index is bounded before use: chunk boundaries are clamped to [0, D] (and counted), a row's chunk lies in [-1, B), and a
// leader is a row of the same chunk.  Everything else the kernels index is workspace they wrote themselves.
#pragma clang fp contract(off)
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int EL_THREADS = 256;              // four waves: four rows (or chunks) per workgroup
constexpr int EL_WAVES = EL_THREADS / 64;
constexpr int EL_MAX_W = 1024;
constexpr int64_t EL_MAX_D = 1 << 17;         // rows per call (as VH_MAX_D: the scans are pairwise within a chunk)

struct ElWs {
    float *mu, *v, *t;                        // [D][W]: at a leader's row its cluster's mean, v_c, t_c
    float *dist, *hq, *pair;                  // [D]: d_i; relu(d_i - delta_var)^2 / n_c; a leader's sum over the other leaders
    int32_t *chunk_of, *leader, *ncl;         // [D]: the row's chunk or -1; its leader or -1; at a leader's row n_c
};

__device__ __forceinline__ float el_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int el_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the clamped bounds of chunk b (b in [0, B)); true when they had to be clamped
__device__ __forceinline__ bool el_bounds(const tmpnn_embed_loss& a, int b, int64_t& lo, int64_t& hi) {
    lo = 0;
    hi = a.D;
    if (a.offsets == nullptr) return false;
    lo = a.offsets[b];
    hi = a.offsets[b + 1];
    if (lo < 0 || hi < lo || hi > a.D) {
        lo = lo < 0 ? 0 : (lo > a.D ? a.D : lo);
        hi = hi < lo ? lo : (hi > a.D ? a.D : hi);
        return true;
    }
    return false;
}

__global__ __launch_bounds__(EL_THREADS) void k_el_chunk(tmpnn_embed_loss a, ElWs w) {
    const int64_t i = (int64_t)blockIdx.x * EL_THREADS + threadIdx.x;
    if (i >= a.D) return;
    int mine = -1;
    for (int b = 0; b < a.B; ++b) {
        int64_t lo, hi;
        el_bounds(a, b, lo, hi);
        if (i >= lo && i < hi) { mine = b; break; }
    }
    w.chunk_of[i] = mine;
}

template <int NK>
__global__ __launch_bounds__(EL_THREADS) void k_el_leader(tmpnn_embed_loss a, ElWs w) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * EL_WAVES + (threadIdx.x >> 6);     // (wave-uniform)
    if (i >= a.D) return;
    const int b = w.chunk_of[i];
    const int id = a.track[i];
    int64_t lead = -1;
    if (b >= 0 && b < a.B && id >= 0) {                                         // (wave-uniform)
        int64_t lo, hi;
        el_bounds(a, b, lo, hi);
        lead = i;
        for (int64_t j0 = lo; j0 < i; j0 += 64) {                               // a lower row with this id leads the cluster
            const int64_t j = j0 + lane;
            const unsigned long long hits = __ballot(j < i && w.chunk_of[j] == b && a.track[j] == id);
            if (hits) { lead = j0 + (__ffsll((long long)hits) - 1); break; }
        }
        if (lead == i) {
            float acc[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) acc[k] = 0.0f;
            int n = 0;
            for (int64_t j0 = i; j0 < hi; j0 += 64) {
                const int64_t j = j0 + lane;
                unsigned long long hits = __ballot(j < hi && w.chunk_of[j] == b && a.track[j] == id);
                n += __popcll(hits);
                while (hits) {                                                  // ascending rows
                    const int64_t r = j0 + (__ffsll((long long)hits) - 1);
                    hits &= hits - 1;
                    const float* x = a.features + r * (int64_t)a.ld;
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        const int c = lane + 64 * k;
                        if (c < a.W) acc[k] += x[c];
                    }
                }
            }
            float* mu = w.mu + i * (int64_t)a.W;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int c = lane + 64 * k;
                if (c < a.W) mu[c] = acc[k] / (float)n;
            }
            if (lane == 0) w.ncl[i] = n;
        }
    }
    if (lane == 0) w.leader[i] = (int32_t)lead;
}

template <int NK>
__global__ __launch_bounds__(EL_THREADS) void k_el_dist(tmpnn_embed_loss a, ElWs w) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * EL_WAVES + (threadIdx.x >> 6);     // (wave-uniform)
    if (i >= a.D) return;
    const int64_t lead = w.leader[i];
    const int b = w.chunk_of[i];
    if (lead < 0 || lead >= a.D || b < 0 || b >= a.B) {
        if (lane == 0) { w.dist[i] = 0.0f; w.hq[i] = 0.0f; w.pair[i] = 0.0f; }
        return;
    }
    const float* x = a.features + i * (int64_t)a.ld;
    const float* mu = w.mu + lead * (int64_t)a.W;
    float m_own[NK];
    float ss = 0.0f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        m_own[k] = c < a.W ? mu[c] : 0.0f;
        const float df = c < a.W ? x[c] - m_own[k] : 0.0f;
        ss += df * df;
    }
    const float d = sqrtf(el_wave_sum(ss));
    const float h = fmaxf(d - a.delta_var, 0.0f);
    const int n = w.ncl[lead];
    float pair = 0.0f;
    if (lead == i) {                                                            // (wave-uniform) the chunk's other leaders
        int64_t lo, hi;
        el_bounds(a, b, lo, hi);
        float vacc[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) vacc[k] = 0.0f;
        int C = 0;
        for (int64_t j0 = lo; j0 < hi; j0 += 64) {
            const int64_t j = j0 + lane;
            unsigned long long hits = __ballot(j < hi && w.chunk_of[j] == b && (int64_t)w.leader[j] == j);
            C += __popcll(hits);
            while (hits) {                                                      // ascending leaders
                const int64_t r = j0 + (__ffsll((long long)hits) - 1);
                hits &= hits - 1;
                if (r == i) continue;
                const float* mo = w.mu + r * (int64_t)a.W;
                float df[NK];
                float s2 = 0.0f;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int c = lane + 64 * k;
                    df[k] = c < a.W ? m_own[k] - mo[c] : 0.0f;
                    s2 += df[k] * df[k];
                }
                const float m = sqrtf(el_wave_sum(s2));
                const float hd = fmaxf(a.delta_dist - m, 0.0f);
                pair += hd * hd;
                if (m > 0.0f && hd > 0.0f) {                                    // (at m == 0 the direction term is 0)
#pragma unroll
                    for (int k = 0; k < NK; ++k) vacc[k] += (hd * df[k]) / m;
                }
            }
        }
        const float scale = C > 1 ? -4.0f / ((float)C * (float)(C - 1)) : 0.0f;
        float* v = w.v + i * (int64_t)a.W;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = lane + 64 * k;
            if (c < a.W) v[c] = scale * vacc[k];
        }
    }
    if (lane == 0) {
        w.dist[i] = d;
        w.hq[i] = n > 0 ? (h * h) / (float)n : 0.0f;
        w.pair[i] = pair;
    }
}

__global__ __launch_bounds__(EL_THREADS) void k_el_reduce(tmpnn_embed_loss a, ElWs w) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * EL_WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;
    int64_t lo, hi;
    const int bad = el_bounds(a, b, lo, hi) ? 1 : 0;
    float accv = 0.0f, accd = 0.0f;
    int n_lab = 0, C = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) {
        if (w.chunk_of[i] != b) continue;
        const int64_t lead = w.leader[i];
        if (lead < 0) continue;
        ++n_lab;
        accv += w.hq[i];
        if (lead == i) { ++C; accd += w.pair[i]; }
    }
    accv = el_wave_sum(accv);
    accd = el_wave_sum(accd);
    n_lab = el_wave_sum(n_lab);
    C = el_wave_sum(C);
    if (lane == 0) {
        const float var = C > 0 ? accv / (float)C : 0.0f;
        const float dst = C > 1 ? accd / ((float)C * (float)(C - 1)) : 0.0f;
        a.loss[b] = var + dst;
        a.terms[2 * b] = var;
        a.terms[2 * b + 1] = dst;
        a.count[4 * b] = n_lab;
        a.count[4 * b + 1] = C;
        a.count[4 * b + 2] = bad;
        a.count[4 * b + 3] = (int32_t)(hi - lo);
    }
}

// u's scalar factor of a row at distance d in a cluster of n rows among C clusters: 2 relu(d - delta_var) / (d C n); 0 at d == 0
__device__ __forceinline__ float el_ucoef(float d, float delta_var, int C, int n) {
    const float h = fmaxf(d - delta_var, 0.0f);
    return (h > 0.0f && d > 0.0f) ? (2.0f * h) / (d * ((float)C * (float)n)) : 0.0f;
}

template <int NK>
__global__ __launch_bounds__(EL_THREADS) void k_el_bwd_leader(tmpnn_embed_loss a, ElWs w) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * EL_WAVES + (threadIdx.x >> 6);     // (wave-uniform)
    if (i >= a.D) return;
    const int b = w.chunk_of[i];
    if ((int64_t)w.leader[i] != i || b < 0 || b >= a.B) return;
    int64_t lo, hi;
    el_bounds(a, b, lo, hi);
    const int C = a.count[4 * b + 1], n = w.ncl[i];
    if (C <= 0 || n <= 0) return;
    const float* mu = w.mu + i * (int64_t)a.W;
    float m_own[NK], su[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        m_own[k] = c < a.W ? mu[c] : 0.0f;
        su[k] = 0.0f;
    }
    for (int64_t j0 = i; j0 < hi; j0 += 64) {
        const int64_t j = j0 + lane;
        unsigned long long hits = __ballot(j < hi && w.chunk_of[j] == b && (int64_t)w.leader[j] == i);
        while (hits) {                                                          // ascending rows
            const int64_t r = j0 + (__ffsll((long long)hits) - 1);
            hits &= hits - 1;
            const float uc = el_ucoef(w.dist[r], a.delta_var, C, n);
            if (uc == 0.0f) continue;
            const float* x = a.features + r * (int64_t)a.ld;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int c = lane + 64 * k;
                if (c < a.W) su[k] += uc * (x[c] - m_own[k]);
            }
        }
    }
    const float* v = w.v + i * (int64_t)a.W;
    float* t = w.t + i * (int64_t)a.W;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        if (c < a.W) t[c] = (v[c] - su[k]) / (float)n;
    }
}

template <int NK>
__global__ __launch_bounds__(EL_THREADS) void k_el_bwd_rows(tmpnn_embed_loss a, ElWs w, const float* __restrict__ g,
                                                            float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * EL_WAVES + (threadIdx.x >> 6);     // (wave-uniform)
    if (i >= a.D) return;
    float* out = dx + i * (int64_t)a.ld;
    const int64_t lead = w.leader[i];
    const int b = w.chunk_of[i];
    const int C = (lead >= 0 && lead < a.D && b >= 0 && b < a.B) ? a.count[4 * b + 1] : 0;
    if (C <= 0) {                                                               // no label, or in no chunk
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = lane + 64 * k;
            if (c < a.W) out[c] = 0.0f;
        }
        return;
    }
    const float gb = g[b];
    const float uc = el_ucoef(w.dist[i], a.delta_var, C, w.ncl[lead]);
    const float* x = a.features + i * (int64_t)a.ld;
    const float* mu = w.mu + lead * (int64_t)a.W;
    const float* t = w.t + lead * (int64_t)a.W;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        if (c < a.W) out[c] = gb * (uc * (x[c] - mu[c]) + t[c]);
    }
}

size_t ws_bytes(int64_t D, int W) {
    const size_t d = (size_t)D;
    return 3 * align16(d * (size_t)W * sizeof(float)) + 3 * align16(d * sizeof(float)) + 3 * align16(d * sizeof(int32_t));
}

ElWs carve(const tmpnn_embed_loss* a) {
    WsCarver c{static_cast<char*>(a->ws)};
    const size_t d = (size_t)a->D, dw = d * (size_t)a->W;
    ElWs w;
    w.mu = c.take<float>(dw);
    w.v = c.take<float>(dw);
    w.t = c.take<float>(dw);
    w.dist = c.take<float>(d);
    w.hq = c.take<float>(d);
    w.pair = c.take<float>(d);
    w.chunk_of = c.take<int32_t>(d);
    w.leader = c.take<int32_t>(d);
    w.ncl = c.take<int32_t>(d);
    return w;
}

int check_args(const tmpnn_embed_loss* a, const char* who) {
    TM_REQUIRE(a != nullptr, "%s: the call struct is null", who);
    TM_REQUIRE(a->B >= 1 && a->D >= 0 && a->D <= EL_MAX_D, "%s: B=%d D=%lld (B >= 1, 0 <= D <= %lld)", who, a->B, (long long)a->D,
               (long long)EL_MAX_D);
    TM_REQUIRE(a->W >= 1 && a->W <= EL_MAX_W && a->ld >= a->W, "%s: W=%d ld=%d (1 <= W <= %d, ld >= W)", who, a->W, a->ld, EL_MAX_W);
    TM_REQUIRE(a->delta_var >= 0.0f && a->delta_var <= 3.0e38f && a->delta_dist >= 0.0f && a->delta_dist <= 3.0e38f,
               "%s: delta_var, delta_dist must be finite and not negative", who);
    TM_REQUIRE(a->loss && a->terms && a->count, "%s: null loss, terms or count", who);
    TM_REQUIRE(a->offsets != nullptr || a->B == 1, "%s: offsets is null with B=%d", who, a->B);
    TM_REQUIRE(a->D == 0 || (a->features && a->track), "%s: null features or track", who);
    TM_REQUIRE(a->D == 0 || (a->ws != nullptr && aligned16(a->ws) && a->ws_bytes >= ws_bytes(a->D, a->W)),
               "%s: workspace of %zu bytes, 16-byte aligned, expected (tmpnn_embed_loss_ws)", who, ws_bytes(a->D, a->W));
    return TMPNN_OK;
}

// one wave per row, the kernel instantiated for the lane's channel count: W <= 128, <= 256, <= 1024
#define EL_LAUNCH_ROWS(kernel, a, st, ...)                                                                              \
    do {                                                                                                                \
        const dim3 grid_((unsigned)ceil_div((a)->D, EL_WAVES)), block_(EL_THREADS);                                     \
        if ((a)->W <= 128) hipLaunchKernelGGL(kernel<2>, grid_, block_, 0, st, __VA_ARGS__);                            \
        else if ((a)->W <= 256) hipLaunchKernelGGL(kernel<4>, grid_, block_, 0, st, __VA_ARGS__);                       \
        else hipLaunchKernelGGL(kernel<16>, grid_, block_, 0, st, __VA_ARGS__);                                         \
    } while (0)

}  // namespace

extern "C" size_t tmpnn_embed_loss_ws(int64_t D, int W) {
    if (D <= 0 || D > EL_MAX_D || W < 1 || W > EL_MAX_W) return 0;
    return ws_bytes(D, W);
}

extern "C" int tmpnn_embed_loss_fwd(const tmpnn_embed_loss* a, tmpnn_stream stream) {
    if (int rc = check_args(a, "embed_loss_fwd")) return rc;
    hipStream_t st = as_stream(stream);
    ElWs w{};
    if (a->D > 0) {
        w = carve(a);
        hipLaunchKernelGGL(k_el_chunk, dim3((unsigned)ceil_div(a->D, EL_THREADS)), dim3(EL_THREADS), 0, st, *a, w);
        if (int rc = check_launch("embed_loss_fwd (chunks of the rows)")) return rc;
        EL_LAUNCH_ROWS(k_el_leader, a, st, *a, w);
        if (int rc = check_launch("embed_loss_fwd (leaders, means)")) return rc;
        EL_LAUNCH_ROWS(k_el_dist, a, st, *a, w);
        if (int rc = check_launch("embed_loss_fwd (distances, leader pairs)")) return rc;
    }
    hipLaunchKernelGGL(k_el_reduce, dim3((unsigned)ceil_div(a->B, EL_WAVES)), dim3(EL_THREADS), 0, st, *a, w);
    return check_launch("embed_loss_fwd (chunks)");
}

extern "C" int tmpnn_embed_loss_bwd(const tmpnn_embed_loss* a, const float* g, float* d_features, tmpnn_stream stream) {
    if (int rc = check_args(a, "embed_loss_bwd")) return rc;
    TM_REQUIRE(g != nullptr && (a->D == 0 || d_features != nullptr), "embed_loss_bwd: g or d_features is null");
    if (a->D == 0) return TMPNN_OK;
    hipStream_t st = as_stream(stream);
    const ElWs w = carve(a);
    EL_LAUNCH_ROWS(k_el_bwd_leader, a, st, *a, w);
    if (int rc = check_launch("embed_loss_bwd (leaders)")) return rc;
    EL_LAUNCH_ROWS(k_el_bwd_rows, a, st, *a, w, g, d_features);
    return check_launch("embed_loss_bwd (rows)");
}
