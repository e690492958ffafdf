// The visual head on the device (tmpnn_vis_head_fwd, tmpnn_vis_head_bwd, tmpnn_vis_head_pixels, tmpnn_vis_head_rows_from_logits;
// include/tmpnn.h; host definition:
// trackmpnn_amd.vishead.vis_head_host).  The reference reads the embedding CNN's map at every box centre in a Python loop with one
// indexing kernel per detection (dataset/kitti_mot.py:391-412), then torch.cat, F.softmax and the standardisation (:558-566), and
// for training a np.vectorize label map and nn.CrossEntropyLoss (models/loss.py:162-181).
//
// k_vis_fwd     one wave per detection, lane l owns channels l and l + 64.  The centre pixel in float32 (below), the two gathered
//               logits, the wave's maximum and sum of exponentials by xor butterflies (every lane ends with the same bits), the
//               standardised softmax row into the caller's rows at its own stride and column, the contiguous logits, and per row
//               the (maximum, sum) pair, the negative log-likelihood of its label, the pixel and the flags.
// k_vis_pixels, k_vis_rows_logits   the same head behind a CNN that answers per pixel (tmpnn_espnet_centres): the pixels and flags
//               alone, a thread per row; then, over logits the caller gathered at them, the rows by k_vis_fwd's own code (vh_row)
//               and, in one more workgroup, the one chunk's counts by k_vis_reduce's (vh_chunk).  They live here because this file
//               is built with contraction off: the centre rule and the softmax stay the arithmetic of k_vis_fwd.
// k_vis_reduce  one wave per chunk: lanes walk the chunk's rows in strides of 64 and a butterfly adds the 64 partial sums, so the
//               order of the additions depends on the chunk's bounds alone.  loss[b], the counts, and per row its chunk and its
//               scatter key (the pixel of a labelled row, -1 otherwise).
// k_vis_bwd     one wave per detection.  Rows with equal keys share a pixel of dmaps; the lowest of them owns it.  A wave scans
//               the keys below its row (64 a step, one ballot) and leaves at the first equal one; an owner scans the keys from
//               its row on, and for every sharer, in ascending row order, recomputes the sharer's softmax from its saved logits
//               and (maximum, sum) exactly as the forward did and adds coef * (softmax - onehot); one store per channel.  The
//               memset before it zeroes every other pixel.  No atomics: the result is bitwise reproducible.  The scan is
//               D / 64 steps a row whatever the frames hold, so there is no per-frame limit; it grows with D * D, so a call takes
//               at most VH_MAX_D = 131 072 detections (a batch of 64 KITTI chunks holds about 5 000).
//
// The centre is the reference's float32 arithmetic: ((a + b) / 2) * input / im / down_ratio, truncated toward zero.  Contraction is
// OFF for this file (the sum, the product and the quotients must stay separate operations) and each quotient is formed in float64
// and rounded to float32, which for float32 operands is the correctly rounded float32 quotient (53 >= 2 * 24 + 2); no reciprocal.
//
// Every index is bounded before use: the centre is clamped to the map (and flagged), a map_of outside [0, T) reads map 0 (and is
// flagged), chunk boundaries are clamped to [0, D] (and counted), and the backward checks every saved pixel and chunk again.
#pragma clang fp contract(off)
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int VH_C = 128;                    // channels of the map = columns of a row
constexpr int VH_THREADS = 256;              // four waves: four detections (or chunks) per workgroup
constexpr int VH_WAVES = VH_THREADS / 64;
constexpr int VH_CLAMPED = 1, VH_BADMAP = 2;
constexpr int64_t VH_MAX_D = 1 << 17;         // detections per call: the backward's scan is D / 64 steps a row, D * D / 64 key loads in all

__device__ __forceinline__ float vh_div(float a, float b) { return (float)((double)a / (double)b); }

// the map index under the centre of [lo, hi] along an axis of n pixels; `clamped` is set when it lay outside (or was NaN)
__device__ __forceinline__ int vh_centre(float lo, float hi, float input, float im, float down, int n, bool& clamped) {
    const float c = vh_div(vh_div(((lo + hi) / 2.0f) * input, im), down);
    const float t = truncf(c);
    if (!(t >= 0.0f)) { clamped = true; return 0; }
    if ((double)t > (double)(n - 1)) { clamped = true; return n - 1; }
    return (int)t;
}

__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the pixel row d reads: the centre rule, the clamps and the flags (k_vis_fwd and k_vis_pixels)
__device__ __forceinline__ int32_t vh_pixel(const tmpnn_vis_head& a, int64_t d, int& m, int64_t& inmap, int& fl) {
    const float x1 = a.box[4 * d], y1 = a.box[4 * d + 1], x2 = a.box[4 * d + 2], y2 = a.box[4 * d + 3];
    const float im_h = a.im_hw ? a.im_hw[2 * d] : a.im_h, im_w = a.im_hw ? a.im_hw[2 * d + 1] : a.im_w;
    bool clamped = false;
    const int cx = vh_centre(x1, x2, a.input_w, im_w, a.down_ratio, a.Wm, clamped);
    const int cy = vh_centre(y1, y2, a.input_h, im_h, a.down_ratio, a.Hm, clamped);
    m = a.map_of[d];
    fl = clamped ? VH_CLAMPED : 0;
    if (m < 0 || m >= a.T) { m = 0; fl |= VH_BADMAP; }
    inmap = (int64_t)cy * a.Wm + cx;                                            // < plane
    return (int32_t)((int64_t)m * a.Hm * a.Wm + inmap);
}

// a wave's row from its two logits a lane (k_vis_fwd and k_vis_rows_logits): maximum, exponentials, sum, the standardised
// softmax into the caller's rows, the (maximum, sum) pair and the row's negative log-likelihood
__device__ __forceinline__ void vh_row(const tmpnn_vis_head& a, int64_t d, int lane, float v0, float v1) {
    const float mx = wave_max(fmaxf(v0, v1));
    const float e0 = expf(v0 - mx), e1 = expf(v1 - mx);
    const float s = wave_sum(e0 + e1);
    float* row = a.rows + d * (int64_t)a.ld_rows + a.col;
    row[lane] = (e0 / s - a.mean[lane]) / a.std[lane];
    row[lane + 64] = (e1 / s - a.mean[lane + 64]) / a.std[lane + 64];
    const int tr = a.track ? a.track[d] : -1;
    float nll = 0.0f;
    if (tr >= 0) {                                                              // (wave-uniform)
        const int c = tr & (VH_C - 1);                                          // track % 128
        const float t0 = __shfl(v0, c & 63), t1 = __shfl(v1, c & 63);
        nll = (mx + logf(s)) - (c < 64 ? t0 : t1);
    }
    if (lane == 0) {
        a.stat[2 * d] = mx;
        a.stat[2 * d + 1] = s;
        a.nll[d] = nll;
    }
}

__global__ __launch_bounds__(VH_THREADS) void k_vis_fwd(tmpnn_vis_head a) {
    const int lane = threadIdx.x & 63;
    const int64_t d = (int64_t)blockIdx.x * VH_WAVES + (threadIdx.x >> 6);     // (wave-uniform)
    if (d >= a.D) return;
    int m, fl;
    int64_t inmap;
    const int32_t px = vh_pixel(a, d, m, inmap, fl);
    const int64_t plane = (int64_t)a.Hm * a.Wm;
    const float* src = a.maps + (int64_t)m * VH_C * plane + inmap;
    const float v0 = src[(int64_t)lane * plane], v1 = src[(int64_t)(lane + 64) * plane];
    vh_row(a, d, lane, v0, v1);
    a.logits[d * VH_C + lane] = v0;
    a.logits[d * VH_C + lane + 64] = v1;
    if (lane == 0) {
        a.pix[d] = px;
        a.flag[d] = fl;
        a.chunk_of[d] = -1;
        a.key[d] = -1;
    }
}

// the pixel and the flags of every row alone, a thread per row (tmpnn_vis_head_pixels): what a per-centre CNN is asked for
__global__ __launch_bounds__(VH_THREADS) void k_vis_pixels(tmpnn_vis_head a) {
    const int64_t d = (int64_t)blockIdx.x * VH_THREADS + threadIdx.x;
    if (d >= a.D) return;
    int m, fl;
    int64_t inmap;
    a.pix[d] = vh_pixel(a, d, m, inmap, fl);
    a.flag[d] = fl;
}

__device__ __forceinline__ void vh_chunk(const tmpnn_vis_head& a, int b, int lane) {
    int64_t lo = 0, hi = a.D;
    int bad = 0;
    if (a.offsets) {
        lo = a.offsets[b];
        hi = a.offsets[b + 1];
        if (lo < 0 || hi < lo || hi > a.D) {
            bad = 1;
            lo = lo < 0 ? 0 : (lo > a.D ? a.D : lo);
            hi = hi < lo ? lo : (hi > a.D ? a.D : hi);
        }
    }
    float acc = 0.0f;
    int n = 0, n_clamped = 0, n_bad = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) {
        const int fl = a.flag[i];
        const bool lab = a.track != nullptr && a.track[i] >= 0;
        if (lab) { acc += a.nll[i]; ++n; }
        n_clamped += fl & VH_CLAMPED;
        n_bad += (fl & VH_BADMAP) ? 1 : 0;
        a.chunk_of[i] = b;
        a.key[i] = lab ? a.pix[i] : -1;
    }
    acc = wave_sum(acc);
    n = wave_sum(n);
    n_clamped = wave_sum(n_clamped);
    n_bad = wave_sum(n_bad);
    if (lane == 0) {
        a.loss[b] = n > 0 ? acc / (float)n : 0.0f;
        a.count[4 * b] = n;
        a.count[4 * b + 1] = n_clamped;
        a.count[4 * b + 2] = n_bad + bad;
        a.count[4 * b + 3] = (int32_t)(hi - lo);
    }
}

__global__ __launch_bounds__(VH_THREADS) void k_vis_reduce(tmpnn_vis_head a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * VH_WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;
    vh_chunk(a, b, lane);
}

// Rows from logits that are already gathered (tmpnn_vis_head_rows_from_logits; inference: no track, one chunk): a wave per row
// runs vh_row over a.logits; the first wave of one more workgroup is the chunk's k_vis_reduce -- it reads the flags of the
// launch before (k_vis_pixels) and no nll, and writes chunk_of and key, which the row waves leave alone.
__global__ __launch_bounds__(VH_THREADS) void k_vis_rows_logits(tmpnn_vis_head a) {
    const int lane = threadIdx.x & 63;
    const int64_t row_blocks = (a.D + VH_WAVES - 1) / VH_WAVES;
    if ((int64_t)blockIdx.x >= row_blocks) {
        if ((threadIdx.x >> 6) == 0) vh_chunk(a, 0, lane);
        return;
    }
    const int64_t d = (int64_t)blockIdx.x * VH_WAVES + (threadIdx.x >> 6);     // (wave-uniform)
    if (d >= a.D) return;
    vh_row(a, d, lane, a.logits[d * VH_C + lane], a.logits[d * VH_C + lane + 64]);
}

__global__ __launch_bounds__(VH_THREADS) void k_vis_bwd(tmpnn_vis_head a, const float* __restrict__ g, float* __restrict__ dmaps) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * VH_WAVES + (threadIdx.x >> 6);     // (wave-uniform)
    if (i >= a.D) return;
    const int my = a.key[i];
    const int64_t plane = (int64_t)a.Hm * a.Wm;
    if (my < 0 || (int64_t)my >= (int64_t)a.T * plane) return;                  // no label, or in no chunk: nothing to add
    for (int64_t j0 = 0; j0 < i; j0 += 64) {                                    // a lower row on this pixel owns it
        const int64_t j = j0 + lane;
        if (__ballot(j < i && a.key[j] == my)) return;
    }
    float acc0 = 0.0f, acc1 = 0.0f;
    for (int64_t j0 = i & ~(int64_t)63; j0 < a.D; j0 += 64) {
        const int64_t j = j0 + lane;
        unsigned long long hits = __ballot(j >= i && j < a.D && a.key[j] == my);
        while (hits) {                                                          // ascending rows
            const int64_t r = j0 + (__ffsll((long long)hits) - 1);
            hits &= hits - 1;
            const int br = a.chunk_of[r];
            if (br < 0 || br >= a.B) continue;
            const int n = a.count[4 * br];
            if (n <= 0) continue;
            const float coef = g[br] / (float)n;
            const float mx = a.stat[2 * r], s = a.stat[2 * r + 1];
            const int c = a.track[r] & (VH_C - 1);
            const float p0 = expf(a.logits[r * VH_C + lane] - mx) / s, p1 = expf(a.logits[r * VH_C + lane + 64] - mx) / s;
            acc0 += coef * (p0 - (lane == c ? 1.0f : 0.0f));
            acc1 += coef * (p1 - (lane + 64 == c ? 1.0f : 0.0f));
        }
    }
    const int64_t m = my / plane, inmap = my % plane;
    float* dst = dmaps + m * VH_C * plane + inmap;
    dst[(int64_t)lane * plane] = acc0;
    dst[(int64_t)(lane + 64) * plane] = acc1;
}

// the ownership scan of k_vis_bwd for a gradient that is handed in: the owner of a pixel adds d_logits of its sharers in ascending
// row order and stores once (tmpnn_vis_head_scatter)
__global__ __launch_bounds__(VH_THREADS) void k_vis_scatter(tmpnn_vis_head a, const float* __restrict__ dl, float* __restrict__ dmaps) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * VH_WAVES + (threadIdx.x >> 6);     // (wave-uniform)
    if (i >= a.D) return;
    const int my = a.key[i];
    const int64_t plane = (int64_t)a.Hm * a.Wm;
    if (my < 0 || (int64_t)my >= (int64_t)a.T * plane) return;                  // no label, or in no chunk: nothing to add
    for (int64_t j0 = 0; j0 < i; j0 += 64) {                                    // a lower row on this pixel owns it
        const int64_t j = j0 + lane;
        if (__ballot(j < i && a.key[j] == my)) return;
    }
    float acc0 = 0.0f, acc1 = 0.0f;
    for (int64_t j0 = i & ~(int64_t)63; j0 < a.D; j0 += 64) {
        const int64_t j = j0 + lane;
        unsigned long long hits = __ballot(j >= i && j < a.D && a.key[j] == my);
        while (hits) {                                                          // ascending rows
            const int64_t r = j0 + (__ffsll((long long)hits) - 1);
            hits &= hits - 1;
            acc0 += dl[r * VH_C + lane];
            acc1 += dl[r * VH_C + lane + 64];
        }
    }
    const int64_t m = my / plane, inmap = my % plane;
    float* dst = dmaps + m * VH_C * plane + inmap;
    dst[(int64_t)lane * plane] = acc0;
    dst[(int64_t)(lane + 64) * plane] = acc1;
}

int check_args(const tmpnn_vis_head* a, const char* who, bool need_maps = true) {
    TM_REQUIRE(a != nullptr, "%s: the call struct is null", who);
    TM_REQUIRE(a->T >= 1 && a->Hm >= 1 && a->Wm >= 1 && (int64_t)a->T * a->Hm * a->Wm < 0x7fffffffLL, "%s: maps of %d x %d x %d pixels "
               "(T * Hm * Wm must fit in int32)", who, a->T, a->Hm, a->Wm);
    TM_REQUIRE(a->B >= 1 && a->D >= 0 && a->D <= VH_MAX_D, "%s: B=%d D=%lld (B >= 1, 0 <= D <= %lld)", who, a->B, (long long)a->D,
               (long long)VH_MAX_D);
    const float geo[3] = {a->input_h, a->input_w, a->down_ratio};
    for (float v : geo) TM_REQUIRE(v > 0.0f && v <= 3.0e38f, "%s: input_h, input_w, down_ratio must be finite and positive", who);
    TM_REQUIRE(a->im_hw != nullptr || (a->im_h > 0.0f && a->im_h <= 3.0e38f && a->im_w > 0.0f && a->im_w <= 3.0e38f),
               "%s: im_hw is null and im_h, im_w are not finite and positive", who);
    TM_REQUIRE(a->col >= 0 && a->ld_rows >= VH_C && a->col <= a->ld_rows - VH_C, "%s: col=%d ld_rows=%d", who, a->col, a->ld_rows);
    TM_REQUIRE((a->maps || !need_maps) && a->mean && a->std && a->loss && a->count, "%s: null maps, mean, std, loss or count", who);
    TM_REQUIRE(a->offsets != nullptr || a->B == 1, "%s: offsets is null with B=%d", who, a->B);
    TM_REQUIRE(a->D == 0 || (a->box && a->map_of && a->rows && a->logits && a->stat && a->nll && a->pix && a->flag && a->chunk_of && a->key),
               "%s: null per-detection arrays", who);
    return TMPNN_OK;
}

}  // namespace

extern "C" int tmpnn_vis_head_fwd(const tmpnn_vis_head* a, tmpnn_stream stream) {
    if (int rc = check_args(a, "vis_head_fwd")) return rc;
    if (a->D > 0) {
        hipLaunchKernelGGL(k_vis_fwd, dim3((unsigned)ceil_div(a->D, VH_WAVES)), dim3(VH_THREADS), 0, as_stream(stream), *a);
        if (int rc = check_launch("vis_head_fwd (rows)")) return rc;
    }
    hipLaunchKernelGGL(k_vis_reduce, dim3((unsigned)ceil_div(a->B, VH_WAVES)), dim3(VH_THREADS), 0, as_stream(stream), *a);
    return check_launch("vis_head_fwd (chunks)");
}

extern "C" int tmpnn_vis_head_bwd(const tmpnn_vis_head* a, const float* g, float* dmaps, tmpnn_stream stream) {
    if (int rc = check_args(a, "vis_head_bwd")) return rc;
    TM_REQUIRE(g != nullptr && dmaps != nullptr, "vis_head_bwd: g or dmaps is null");
    const size_t bytes = sizeof(float) * (size_t)a->T * VH_C * (size_t)a->Hm * (size_t)a->Wm;
    hipError_t e = hipMemsetAsync(dmaps, 0, bytes, as_stream(stream));
    if (e != hipSuccess) return set_error(TMPNN_ELAUNCH, "vis_head_bwd (memset): %s", hipGetErrorString(e));
    if (a->D > 0 && a->track != nullptr) {
        hipLaunchKernelGGL(k_vis_bwd, dim3((unsigned)ceil_div(a->D, VH_WAVES)), dim3(VH_THREADS), 0, as_stream(stream), *a, g, dmaps);
        if (int rc = check_launch("vis_head_bwd (scatter)")) return rc;
    }
    return TMPNN_OK;
}

extern "C" int tmpnn_vis_head_scatter(const tmpnn_vis_head* a, const float* d_logits, float* dmaps, tmpnn_stream stream) {
    if (int rc = check_args(a, "vis_head_scatter")) return rc;
    TM_REQUIRE(dmaps != nullptr && (a->D == 0 || d_logits != nullptr), "vis_head_scatter: d_logits or dmaps is null");
    const size_t bytes = sizeof(float) * (size_t)a->T * VH_C * (size_t)a->Hm * (size_t)a->Wm;
    hipError_t e = hipMemsetAsync(dmaps, 0, bytes, as_stream(stream));
    if (e != hipSuccess) return set_error(TMPNN_ELAUNCH, "vis_head_scatter (memset): %s", hipGetErrorString(e));
    if (a->D > 0 && a->track != nullptr) {
        hipLaunchKernelGGL(k_vis_scatter, dim3((unsigned)ceil_div(a->D, VH_WAVES)), dim3(VH_THREADS), 0, as_stream(stream), *a, d_logits,
                           dmaps);
        if (int rc = check_launch("vis_head_scatter")) return rc;
    }
    return TMPNN_OK;
}

extern "C" int tmpnn_vis_head_pixels(const tmpnn_vis_head* a, tmpnn_stream stream) {
    if (int rc = check_args(a, "vis_head_pixels", false)) return rc;
    if (a->D == 0) return TMPNN_OK;
    hipLaunchKernelGGL(k_vis_pixels, dim3((unsigned)ceil_div(a->D, VH_THREADS)), dim3(VH_THREADS), 0, as_stream(stream), *a);
    return check_launch("vis_head_pixels");
}

extern "C" int tmpnn_vis_head_rows_from_logits(const tmpnn_vis_head* a, tmpnn_stream stream) {
    if (int rc = check_args(a, "vis_head_rows_from_logits", false)) return rc;
    TM_REQUIRE(a->track == nullptr && a->offsets == nullptr && a->B == 1, "vis_head_rows_from_logits: inference only (track and offsets "
               "NULL, B = 1); a loss takes tmpnn_vis_head_fwd over the dense maps");
    hipLaunchKernelGGL(k_vis_rows_logits, dim3((unsigned)ceil_div(a->D, VH_WAVES) + 1), dim3(VH_THREADS), 0, as_stream(stream), *a);
    return check_launch("vis_head_rows_from_logits");
}
