// The optimizer step on the device: torch.optim.Adam (reference train.py:329, stepped at train.py:135) over the flat gradient
// bucket in ONE launch, and the per-parameter gradient statistics of --plot-gradients (utils/gradients.py:23) in one launch.
//
// A parameter keeps its own storage: segment s of the table is (its device pointer, its start in the flat buffers, its element
// count), and gradient / exp_avg / exp_avg_sq are three flat fp32 buffers laid out like the bucket.  The work list cuts every
// segment into chunks of OPT_CHUNK elements, (segment, offset in the segment) per chunk, built once on the host; a workgroup
// takes chunks blockIdx.x, blockIdx.x + gridDim.x, ...  A chunk whose flat offset and parameter address are both 16-byte
// aligned moves float4s (its last 1..3 elements one by one); any other chunk (a segment behind a bias of 1 element) moves
// single floats, still coalesced.
//
// lr and the step count live in device memory (struct tmpnn_adam_state), so a captured launch replays with the current values.
// Every workgroup reads the step count BEFORE it adds to the ticket, and the workgroup whose add finds gridDim.x - 1 earlier
// ones advances the count and clears the ticket: when it does, every other workgroup has read.  One integer atomic per
// workgroup; no atomics on floats, every element is written by one thread: two runs give the same bits.
#include "common.h"

namespace tmpnn {

static constexpr int OPT_THREADS = 256;
static constexpr int OPT_CHUNK = 4 * OPT_THREADS;       // elements of a work item: one float4 per thread
static constexpr int OPT_MAX_GRID = 2048;
static constexpr int GF_THREADS = 1024;
static constexpr int GF_UNROLL = 4;

struct AdamConsts {
    float beta2, omb1, omb2, eps, wd, gscale;
    float step_size, bc2_sqrt;                           // lr / (1 - beta1^t);  sqrt(1 - beta2^t)
};

// one element; the order of operations is torch's (_single_tensor_adam): lerp for exp_avg, sqrt(v) / sqrt(bc2) + eps
__device__ inline void adam1(float& g, float& p, float& m, float& v, const AdamConsts& c) {
    // the product is rounded BEFORE the decay term is added, so that grad_scale equals flat.mul_(scale) and a plain step.
    // __fmul_rn is a plain multiply to this compiler, which then contracts it into fma(g, gscale, wd * p): the empty asm makes
    // the rounded product a value of its own.
    float gs = g * c.gscale;
    asm volatile("" : "+v"(gs));
    const float gd = gs + c.wd * p;
    m = m + c.omb1 * (gd - m);
    v = c.beta2 * v + (c.omb2 * gd) * gd;
    const float den = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p - c.step_size * (m / den);
}

__global__ __launch_bounds__(OPT_THREADS) void k_adam_step(const tmpnn_optim_seg* __restrict__ segs, int P,
                                                           const int32_t* __restrict__ work, int nwork, float* grad,
                                                           float* exp_avg, float* exp_avg_sq, long n_flat,
                                                           tmpnn_adam_state* st, float beta2, float omb1, float omb2,
                                                           double beta1d, double beta2d, float eps, float wd, float gscale,
                                                           int zero_grads) {
    __shared__ float s_c[2];
    const int tid = threadIdx.x;
    float t_new = 0.f;
    if (tid == 0) {
        // (agent-scope loads: the values another launch, or torch, wrote; never this launch -- see the ticket below)
        const double lr = __hip_atomic_load(&st->lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float t0 = __hip_atomic_load(&st->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t_new = t0 + 1.0f;
        const double bc1 = 1.0 - pow(beta1d, (double)t_new);
        const double bc2 = 1.0 - pow(beta2d, (double)t_new);
        s_c[0] = (float)(lr / bc1);
        s_c[1] = (float)sqrt(bc2);
    }
    __syncthreads();
    AdamConsts c;
    c.beta2 = beta2, c.omb1 = omb1, c.omb2 = omb2, c.eps = eps, c.wd = wd, c.gscale = gscale;
    c.step_size = s_c[0], c.bc2_sqrt = s_c[1];

    for (int w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int s = work[2 * w], off = work[2 * w + 1];
        if (s < 0 || s >= P) continue;                                          // (a table that does not fit moves nothing)
        const tmpnn_optim_seg sg = segs[s];
        if (sg.p == nullptr || sg.start < 0 || sg.count <= 0 || sg.start + sg.count > n_flat || off < 0 || off >= sg.count)
            continue;
        const long rest = sg.count - off;
        const int cnt = rest < OPT_CHUNK ? (int)rest : OPT_CHUNK;
        float* pp = sg.p + off;
        const long f0 = sg.start + off;
        float *pg = grad + f0, *pm = exp_avg + f0, *pv = exp_avg_sq + f0;
        const bool al = ((f0 & 3) == 0) && ((reinterpret_cast<uintptr_t>(pp) & 15u) == 0);   // (uniform over the workgroup)
        const int e0 = 4 * tid;
        if (al && e0 + 4 <= cnt) {
            float4 g4 = *reinterpret_cast<const float4*>(pg + e0);
            float4 p4 = *reinterpret_cast<const float4*>(pp + e0);
            float4 m4 = *reinterpret_cast<const float4*>(pm + e0);
            float4 v4 = *reinterpret_cast<const float4*>(pv + e0);
            adam1(g4.x, p4.x, m4.x, v4.x, c);
            adam1(g4.y, p4.y, m4.y, v4.y, c);
            adam1(g4.z, p4.z, m4.z, v4.z, c);
            adam1(g4.w, p4.w, m4.w, v4.w, c);
            *reinterpret_cast<float4*>(pp + e0) = p4;
            *reinterpret_cast<float4*>(pm + e0) = m4;
            *reinterpret_cast<float4*>(pv + e0) = v4;
            if (zero_grads) *reinterpret_cast<float4*>(pg + e0) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (al) {
            for (int e = e0; e < cnt; ++e) {                                    // the chunk's last 1..3 elements (one thread)
                float g = pg[e], p = pp[e], m = pm[e], v = pv[e];
                adam1(g, p, m, v, c);
                pp[e] = p, pm[e] = m, pv[e] = v;
                if (zero_grads) pg[e] = 0.f;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {                                       // unaligned chunk: lane-contiguous single floats
                const int e = tid + k * OPT_THREADS;
                if (e < cnt) {
                    float g = pg[e], p = pp[e], m = pm[e], v = pv[e];
                    adam1(g, p, m, v, c);
                    pp[e] = p, pm[e] = m, pv[e] = v;
                    if (zero_grads) pg[e] = 0.f;
                }
            }
        }
    }
    if (tid == 0) {
        // this workgroup read lr / step above (their values are in registers): take a ticket; the last one moves the count
        const int old = __hip_atomic_fetch_add(&st->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == (int)gridDim.x - 1) {
            __hip_atomic_store(&st->step, t_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&st->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// One workgroup per segment: sum |g| in fp64 (each thread its strided elements in sequence, then a fixed tree), max |g| with
// torch's NaN rule (a NaN wins), the count of non-finite elements.  stats [P][3] fp64 = mean |g|, max |g|, non-finite count.
__global__ __launch_bounds__(GF_THREADS) void k_grad_flow(const tmpnn_optim_seg* __restrict__ segs, const float* __restrict__ grad,
                                                          long n_flat, double* __restrict__ stats) {
    __shared__ double s_sum[GF_THREADS];
    __shared__ float s_max[GF_THREADS];
    __shared__ long long s_bad[GF_THREADS];
    const int tid = threadIdx.x;
    const tmpnn_optim_seg sg = segs[blockIdx.x];
    double* out = stats + 3 * (size_t)blockIdx.x;
    if (sg.start < 0 || sg.count <= 0 || sg.start + sg.count > n_flat) {        // (uniform) nothing to read: NaN, NaN, 0
        if (tid == 0) out[0] = out[1] = __builtin_nan(""), out[2] = 0.0;
        return;
    }
    const float* g = grad + sg.start;
    const long n = sg.count;
    double sum = 0.0;
    float mx = 0.f;
    bool nan = false;
    long long bad = 0;
    for (long i0 = tid; i0 < n; i0 += (long)GF_THREADS * GF_UNROLL) {
        float a[GF_UNROLL];
#pragma unroll
        for (int u = 0; u < GF_UNROLL; ++u) {
            const long i = i0 + (long)u * GF_THREADS;
            a[u] = fabsf(g[i < n ? i : n - 1]);                                 // (clamped: the loads go out back to back)
        }
#pragma unroll
        for (int u = 0; u < GF_UNROLL; ++u) {
            if (i0 + (long)u * GF_THREADS >= n) continue;
            sum += (double)a[u];
            nan |= a[u] != a[u];
            mx = fmaxf(mx, a[u]);                                               // (fmaxf drops a NaN: carried in `nan`)
            bad += !(a[u] <= 3.402823466e38f);
        }
    }
    s_sum[tid] = sum, s_max[tid] = nan ? __builtin_nanf("") : mx, s_bad[tid] = bad;
    __syncthreads();
    for (int half = GF_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) {
            s_sum[tid] += s_sum[tid + half];
            const float x = s_max[tid], y = s_max[tid + half];
            s_max[tid] = (x != x || y != y) ? __builtin_nanf("") : fmaxf(x, y);
            s_bad[tid] += s_bad[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = s_sum[0] / (double)n;
        out[1] = (double)s_max[0];
        out[2] = (double)s_bad[0];
    }
}

}  // namespace tmpnn

using namespace tmpnn;

extern "C" {

int tmpnn_optim_chunk(void) { return OPT_CHUNK; }

int tmpnn_adam_step(const tmpnn_optim_seg* segs, int P, const int32_t* work, int nwork, float* grad, float* exp_avg,
                    float* exp_avg_sq, int64_t n_flat, tmpnn_adam_state* state, double beta1, double beta2, double eps,
                    double weight_decay, float grad_scale, int zero_grads, tmpnn_stream stream) {
    TM_REQUIRE(segs != nullptr && work != nullptr, "adam_step: segment table / work list is null");
    TM_REQUIRE(P > 0 && nwork > 0, "adam_step: empty table (P=%d, nwork=%d)", P, nwork);
    TM_REQUIRE(n_flat > 0, "adam_step: n_flat=%lld", (long long)n_flat);
    TM_REQUIRE(grad && exp_avg && exp_avg_sq, "adam_step: grad / exp_avg / exp_avg_sq is null");
    TM_REQUIRE(state != nullptr, "adam_step: state is null");
    TM_REQUIRE(aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(state),
               "adam_step: the flat buffers and the state must be 16-byte aligned");
    TM_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_step: betas (%g, %g) outside [0, 1)", beta1, beta2);
    TM_REQUIRE(eps >= 0.0 && weight_decay >= 0.0, "adam_step: eps=%g weight_decay=%g", eps, weight_decay);
    TM_REQUIRE(grad_scale == grad_scale, "adam_step: grad_scale is NaN");
    const int grid = nwork < OPT_MAX_GRID ? nwork : OPT_MAX_GRID;
    hipLaunchKernelGGL(k_adam_step, dim3(grid), dim3(OPT_THREADS), 0, as_stream(stream), segs, P, work, nwork, grad, exp_avg,
                       exp_avg_sq, (long)n_flat, state, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), beta1, beta2,
                       (float)eps, (float)weight_decay, grad_scale, zero_grads ? 1 : 0);
    return check_launch("adam_step");
}

int tmpnn_grad_flow(const tmpnn_optim_seg* segs, int P, const float* grad, int64_t n_flat, double* stats, tmpnn_stream stream) {
    TM_REQUIRE(segs != nullptr, "grad_flow: segment table is null");
    TM_REQUIRE(P > 0, "grad_flow: empty table (P=%d)", P);
    TM_REQUIRE(n_flat > 0, "grad_flow: n_flat=%lld", (long long)n_flat);
    TM_REQUIRE(grad != nullptr && stats != nullptr, "grad_flow: grad / stats is null");
    hipLaunchKernelGGL(k_grad_flow, dim3(P), dim3(GF_THREADS), 0, as_stream(stream), segs, grad, (long)n_flat, stats);
    return check_launch("grad_flow");
}

}  // extern "C"
