// GRU cells of the factor-graph update, BACKWARD: data and weight gradients as stand-alone kernels (generic,
// LDS-resident f32, bf16x6) and in ONE pass (k_gru_bwd_two), the slab reductions, and their entry points.  Shared helpers:
// gru_common.h; the forward: gru_fwd.hip.
#include "gru_common.h"

namespace tmpnn {

// ------------------------------------------------------------------------------------------
// backward, data path
// ------------------------------------------------------------------------------------------


// grid: (ceil(R/128), (IN+H)/(32*NT)); a block's NT*32 output columns lie entirely in d_msg
// (virtual column < IN) or in d_h.
template <int NT>
__global__ __launch_bounds__(256) void k_gru_bwd_data(GruBwdDataArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, half = lane >> 5;
    const int r0 = (blockIdx.x * 4 + wave) * 32;
    if (r0 >= a.R) return;
    const int H = a.H;
    const int vcol0 = blockIdx.y * (32 * NT);
    const bool is_dx = vcol0 < a.IN;
    const int n0 = is_dx ? vcol0 : vcol0 - a.IN;
    const float* __restrict__ W = is_dx ? a.w_ih : a.w_hh;
    const int ldw = is_dx ? a.IN : H;
    const int li = min(r0 + c, a.R - 1);
    const int row = a.rows[li];
    const size_t gp = a.gate_plane;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    for (int fb = 0; fb < H / 32; ++fb) {
        const int f0 = fb * 32 + half * 16;
        float dh[16], r[16], z[16], n[16], hn[16], hp[16];
        dh_load16(a.up, row, f0, dh);
        const float* g0 = a.gates + (size_t)row * H + f0;
        load16(g0, r);
        load16(g0 + gp, z);
        load16(g0 + 2 * gp, n);
        load16(g0 + 3 * gp, hn);
        load16(a.h + (size_t)row * a.ld_h + f0, hp);
        float ar[16], az[16], an[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float dn = dh[i] * (1.0f - z[i]) * (1.0f - n[i] * n[i]);
            ar[i] = dn * hn[i] * r[i] * (1.0f - r[i]);
            az[i] = dh[i] * (hp[i] - n[i]) * z[i] * (1.0f - z[i]);
            an[i] = is_dx ? dn : dn * r[i];
        }
        const float* __restrict__ wr = W + (size_t)f0 * ldw + n0 + c;
        const float* __restrict__ wz = W + (size_t)(H + f0) * ldw + n0 + c;
        const float* __restrict__ wn = W + (size_t)(2 * H + f0) * ldw + n0 + c;
        // (weights of four k-steps requested together, as in k_gru_fwd)
#pragma unroll
        for (int s0 = 0; s0 < 16; s0 += 4) {
            float bw[4][3 * NT];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    bw[u][3 * t] = wr[(size_t)(s0 + u) * ldw + t * 32];
                    bw[u][3 * t + 1] = wz[(size_t)(s0 + u) * ldw + t * 32];
                    bw[u][3 * t + 2] = wn[(size_t)(s0 + u) * ldw + t * 32];
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    acc[t] = mfma32(ar[s0 + u], bw[u][3 * t], acc[t]);
                    acc[t] = mfma32(az[s0 + u], bw[u][3 * t + 1], acc[t]);
                    acc[t] = mfma32(an[s0 + u], bw[u][3 * t + 2], acc[t]);
                }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + t * 32 + c;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int lpos = r0 + acc_row(reg, half);
            if (lpos < a.R) {
                const int orow = a.rows[lpos];
                if (is_dx) {
                    a.d_msg[(size_t)orow * a.ld_dmsg + col] = acc[t][reg];
                } else {
                    const float zz = a.gates[gp + (size_t)orow * H + col];
                    float v = acc[t][reg] + dh_at(a.up, orow, col) * zz;
                    if (a.add_msg)
                        v += a.add_msg[(size_t)a.add_src[lpos] * a.ld_add + col] -
                             a.add_msg[(size_t)a.add_dst[lpos] * a.ld_add + col];
                    a.d_h[(size_t)orow * a.ld_dh + col] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// backward, weight path:  dW_ih = d_gi^T x,  dW_hh = d_gh^T h,  db = column sums
// One WAVE = one worker (row slab rs, 32 gate features q, up to 4 x 32 columns of [x | h]).
// Partial products go to slabs, reduced afterwards in a fixed order (no float atomics).
// ------------------------------------------------------------------------------------------




template <int XMODE>
__global__ __launch_bounds__(256) void k_gru_bwd_weights(GruBwdWArgs a) {
    const int lane = threadIdx.x & 63;
    const int c = lane & 31, half = lane >> 5;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long nworkers = (long)a.n_rs * a.NQ * a.NCH;
    if (w >= nworkers) return;
    const int q = (int)(w % a.NQ);
    const int ch = (int)((w / a.NQ) % a.NCH);
    const int rs = (int)(w / ((long)a.NQ * a.NCH));
    const int H = a.H, XH = a.IN + a.H;
    const int ntw = min(4, XH / 32 - ch * 4);
    const int g = (q * 32) / H;               // gate of this worker's 32 features
    const int f = (q * 32) % H + c;           // hidden feature of this lane
    const size_t gp = a.gate_plane;
    const int lo = rs * a.RS, hi = min(a.R, lo + a.RS);

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    float sum_i = 0.f, sum_h = 0.f;

    for (int p = lo; p < hi; p += 2) {
        const int lpos_raw = p + half;
        const bool valid = lpos_raw < hi;
        const int lpos = valid ? lpos_raw : hi - 1;
        const int orow = a.rows[lpos];
        const float dh = dh_at(a.up, orow, f);
        const float* gq = a.gates + (size_t)orow * H + f;
        const float r = gq[0], z = gq[gp], n = gq[2 * gp], hn = gq[3 * gp];
        const float hp = a.h[(size_t)orow * a.ld_h + f];
        const float dn = dh * (1.0f - z) * (1.0f - n * n);
        float ai, ah;
        if (g == 0) { ai = dn * hn * r * (1.0f - r); ah = ai; }
        else if (g == 1) { ai = dh * (hp - n) * z * (1.0f - z); ah = ai; }
        else { ai = dn; ah = dn * r; }
        if (!valid) { ai = 0.f; ah = 0.f; }
        sum_i += ai;
        sum_h += ah;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < ntw) {
                const int vcol = ch * 128 + t * 32 + c;
                if (ch * 128 + t * 32 < a.IN) {
                    acc[t] = mfma32(ai, load_x1<XMODE>(a, lpos, orow, vcol), acc[t]);
                } else {
                    acc[t] = mfma32(ah, a.h[(size_t)orow * a.ld_h + vcol - a.IN], acc[t]);
                }
            }
        }
    }
    float* sw = a.slab_w + (size_t)rs * (3 * H) * XH;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t < ntw) {
            const int vcol = ch * 128 + t * 32 + c;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int j = q * 32 + acc_row(reg, half);
                sw[(size_t)j * XH + vcol] = acc[t][reg];
            }
        }
    }
    if (ch == 0) {
        sum_i += __shfl_xor(sum_i, 32);
        sum_h += __shfl_xor(sum_h, 32);
        if (half == 0) {
            float* sb = a.slab_b + (size_t)rs * 2 * (3 * H);
            sb[q * 32 + c] = sum_i;
            sb[3 * H + q * 32 + c] = sum_h;
        }
    }
}


struct GRaw { float dh[16], r[16], z[16], n[16], hn[16], hp[16]; };

template <int UP>
__device__ __forceinline__ void g_issue(const GruBwdDataArgs& a, int H, int fb, int row, int half, GRaw& g) {
    const int f0 = fb * 32 + half * 16;
    const size_t gp = a.gate_plane;
    dh_load16_t<UP>(a.up, row, f0, g.dh);
    const float* g0 = a.gates + (size_t)row * H + f0;
    load16(g0, g.r);
    load16(g0 + gp, g.z);
    load16(g0 + 2 * gp, g.n);
    load16(g0 + 3 * gp, g.hn);
    load16(a.h + (size_t)row * a.ld_h + f0, g.hp);
}

// d_msg = d_gi @ W_ih and d_h = d_hout*z + d_gh @ W_hh in ONE pass over the gates
template <int H, int IN, int UP, bool FUSE>
__global__ __launch_bounds__(512) void k_gru_bwd_data_lds(GruBwdDataArgs a, int ntiles) {
    extern __shared__ float lds[];
    constexpr int NTX = IN / 32, NTH = H / 32, NF = H / 32;
    float* sWih = lds;                 // [3H][IN]
    float* sWhh = lds + 3 * H * IN;    // [3H][H]
    for (int i = threadIdx.x * 4; i < 3 * H * IN; i += 512 * 4)
        *reinterpret_cast<float4*>(sWih + i) = *reinterpret_cast<const float4*>(a.w_ih + i);
    for (int i = threadIdx.x * 4; i < 3 * H * H; i += 512 * 4)
        *reinterpret_cast<float4*>(sWhh + i) = *reinterpret_cast<const float4*>(a.w_hh + i);
    // 32-row tiles are pulled from an LDS counter; the two waves of a SIMD (w, w+4) get different static
    // priorities so they do not run their MFMA and their store phases in lockstep (see k_gru_fwd_lds)
    int* next_item = reinterpret_cast<int*>(lds + 3 * H * (IN + H));
    if (threadIdx.x == 0) *next_item = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, half = lane >> 5;
    const size_t gp = a.gate_plane;
    if ((__builtin_amdgcn_readfirstlane(wave) >> 2) == 0) __builtin_amdgcn_s_setprio(2);
    const int items_total = ntiles * 8;
    const int per_block = (items_total + gridDim.x - 1) / gridDim.x;
    const int item_lo = blockIdx.x * per_block;
    const int item_hi = min(items_total, item_lo + per_block);

    for (;;) {
        int item = 0;
        if (lane == 0) item = atomicAdd(next_item, 1);
        item = __builtin_amdgcn_readfirstlane(item) + item_lo;
        if (item >= item_hi) break;
        const int r0 = item * 32;
        if (r0 >= a.R) continue;
        const int li = min(r0 + c, a.R - 1);
        const int row = a.rows[li];
        f32x16 accx[NTX], acch[NTH];
#pragma unroll
        for (int t = 0; t < NTX; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) accx[t][i] = 0.f;
#pragma unroll
        for (int t = 0; t < NTH; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acch[t][i] = 0.f;
        GRaw cur, nxt;
        g_issue<UP>(a, H, 0, row, half, cur);
#pragma unroll
        for (int fb = 0; fb < NF; ++fb) {
            const int f0 = fb * 32 + half * 16;
            float ar[16], az[16], an[16], anr[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float dn = cur.dh[i] * (1.0f - cur.z[i]) * (1.0f - cur.n[i] * cur.n[i]);
                ar[i] = dn * cur.hn[i] * cur.r[i] * (1.0f - cur.r[i]);
                az[i] = cur.dh[i] * (cur.hp[i] - cur.n[i]) * cur.z[i] * (1.0f - cur.z[i]);
                an[i] = dn;
                anr[i] = dn * cur.r[i];
            }
            // the next feature block's rows are requested half way through this block's MFMAs: early
            // enough to hide their latency, late enough that half of this block's operands are dead
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                if (s == 8) {
                    if (fb + 1 < NF) g_issue<UP>(a, H, fb + 1, row, half, nxt);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const float* wx = sWih + (f0 + s) * IN + c;
                const float* wh = sWhh + (f0 + s) * H + c;
#pragma unroll
                for (int t = 0; t < NTX; ++t) {       // weights first: transposed accumulator (lane = row)
                    accx[t] = mfma32(wx[t * 32], ar[s], accx[t]);
                    accx[t] = mfma32(wx[H * IN + t * 32], az[s], accx[t]);
                    accx[t] = mfma32(wx[2 * H * IN + t * 32], an[s], accx[t]);
                }
#pragma unroll
                for (int t = 0; t < NTH; ++t) {
                    acch[t] = mfma32(wh[t * 32], ar[s], acch[t]);
                    acch[t] = mfma32(wh[H * H + t * 32], az[s], acch[t]);
                    acch[t] = mfma32(wh[2 * H * H + t * 32], anr[s], acch[t]);
                }
            }
            cur = nxt;
        }
        // epilogue: lane = its own row; register 4q+i <-> column 8q + 4*half + i of the tile
        const bool live = r0 + c < a.R;
        if (live) {
#pragma unroll
            for (int t = 0; t < NTX; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(a.d_msg + (size_t)row * a.ld_dmsg + t * 32 + 8 * q + 4 * half) =
                        make_float4(accx[t][4 * q], accx[t][4 * q + 1], accx[t][4 * q + 2], accx[t][4 * q + 3]);
        }
        int srow = 0, drow = 0;
        if (FUSE) { srow = a.add_src[li]; drow = a.add_dst[li]; }
        const float dyr = (UP & 2) ? a.up.dy[row] : 0.f;
#pragma unroll
        for (int t = 0; t < NTH; ++t) {
            float4 ex[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = t * 32 + 8 * q + 4 * half;
                const float4 zz = *reinterpret_cast<const float4*>(a.gates + gp + (size_t)row * H + col);
                float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
                if (UP & 1) d = *reinterpret_cast<const float4*>(a.up.d_hout + (size_t)row * a.up.ld_dhout + col);
                if (UP & 2) {
                    const float4 w = *reinterpret_cast<const float4*>(a.up.w_head + col);
                    d.x += dyr * w.x; d.y += dyr * w.y; d.z += dyr * w.z; d.w += dyr * w.w;
                }
                ex[q] = make_float4(d.x * zz.x, d.y * zz.y, d.z * zz.z, d.w * zz.w);
                if (FUSE) {
                    const float4 u = *reinterpret_cast<const float4*>(a.add_msg + (size_t)srow * a.ld_add + col);
                    const float4 v = *reinterpret_cast<const float4*>(a.add_msg + (size_t)drow * a.ld_add + col);
                    ex[q].x += u.x - v.x; ex[q].y += u.y - v.y; ex[q].z += u.z - v.z; ex[q].w += u.w - v.w;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (live) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(a.d_h + (size_t)row * a.ld_dh + t * 32 + 8 * q + 4 * half) =
                        make_float4(acch[t][4 * q] + ex[q].x, acch[t][4 * q + 1] + ex[q].y, acch[t][4 * q + 2] + ex[q].z,
                                    acch[t][4 * q + 3] + ex[q].w);
            }
        }
    }
}

// The same pass on the bf16 pipe (bf16x6, see mfma_x6), IN == H.  Both transposed weight matrices sit in LDS as
// three bf16 pieces [piece][column of x|h][3H + 8] (k = gate feature j contiguous; 150 KiB at H = 64), a lane's
// operand is 8 consecutive hidden features of its row per k block: k = g*H + 16*fblk + 8*(lane>>5) + j, so
// the two lane halves read adjacent 32-byte runs of the same 128-byte line of every gate plane.
struct GRaw8 { float4 dh[2], r[2], z[2], n[2], hn[2], hp[2]; };

template <int UP>
__device__ __forceinline__ void g_issue8(const GruBwdDataArgs& a, int H, int f0, int row, GRaw8& g) {
    const size_t gp = a.gate_plane;
    if (UP & 1) {
        const float4* p = reinterpret_cast<const float4*>(a.up.d_hout + (size_t)row * a.up.ld_dhout + f0);
        g.dh[0] = p[0]; g.dh[1] = p[1];
    } else {
        g.dh[0] = make_float4(0.f, 0.f, 0.f, 0.f); g.dh[1] = g.dh[0];
    }
    const float4* g0 = reinterpret_cast<const float4*>(a.gates + (size_t)row * H + f0);
    g.r[0] = g0[0]; g.r[1] = g0[1];
    const float4* g1 = reinterpret_cast<const float4*>(a.gates + gp + (size_t)row * H + f0);
    g.z[0] = g1[0]; g.z[1] = g1[1];
    const float4* g2 = reinterpret_cast<const float4*>(a.gates + 2 * gp + (size_t)row * H + f0);
    g.n[0] = g2[0]; g.n[1] = g2[1];
    const float4* g3 = reinterpret_cast<const float4*>(a.gates + 3 * gp + (size_t)row * H + f0);
    g.hn[0] = g3[0]; g.hn[1] = g3[1];
    const float4* hp = reinterpret_cast<const float4*>(a.h + (size_t)row * a.ld_h + f0);
    g.hp[0] = hp[0]; g.hp[1] = hp[1];
}

__device__ __forceinline__ void f4_to_arr(const float4& u, const float4& v, float* o) {
    o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w; o[4] = v.x; o[5] = v.y; o[6] = v.z; o[7] = v.w;
}
__device__ __forceinline__ Split8 split8_arr(const float* x) {
    return split8(make_float4(x[0], x[1], x[2], x[3]), make_float4(x[4], x[5], x[6], x[7]));
}

template <int H, int UP, bool FUSE>
__global__ __launch_bounds__(512) void k_gru_bwd_data_split(GruBwdDataArgs a, int ntiles) {
    extern __shared__ float lds[];
    constexpr int IN = H, XH = IN + H, J = 3 * H, JP = J + 8, NT = H / 32, NFB = H / 16;
    uint16_t* sWT = reinterpret_cast<uint16_t*>(lds);         // [3][XH][JP]
    for (int i = threadIdx.x; i < J * IN / 4; i += 512) {
        const int j = i / (IN / 4), c0 = (i % (IN / 4)) * 4;
        const float4 wi = *reinterpret_cast<const float4*>(a.w_ih + (size_t)j * IN + c0);
        const float4 wh = *reinterpret_cast<const float4*>(a.w_hh + (size_t)j * H + c0);
        const float wiv[4] = {wi.x, wi.y, wi.z, wi.w}, whv[4] = {wh.x, wh.y, wh.z, wh.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            uint16_t q1, q2, q3;
            split1(wiv[e], q1, q2, q3);
            sWT[(0 * XH + c0 + e) * JP + j] = q1; sWT[(1 * XH + c0 + e) * JP + j] = q2; sWT[(2 * XH + c0 + e) * JP + j] = q3;
            split1(whv[e], q1, q2, q3);
            sWT[(0 * XH + IN + c0 + e) * JP + j] = q1; sWT[(1 * XH + IN + c0 + e) * JP + j] = q2; sWT[(2 * XH + IN + c0 + e) * JP + j] = q3;
        }
    }
    int* next_item = reinterpret_cast<int*>(sWT + 3 * XH * JP);
    float* sHead = reinterpret_cast<float*>(next_item + 4);          // output head slice (UP & 2), read with ds_read_b128
    if ((UP & 2) && threadIdx.x < H) sHead[threadIdx.x] = a.up.w_head[threadIdx.x];
    if (threadIdx.x == 0) *next_item = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, half = lane >> 5;
    const size_t gp = a.gate_plane;
    if ((__builtin_amdgcn_readfirstlane(wave) >> 2) == 0) __builtin_amdgcn_s_setprio(2);
    const int items_total = ntiles * 8;
    const int per_block = (items_total + gridDim.x - 1) / gridDim.x;
    const int item_lo = blockIdx.x * per_block;
    const int item_hi = min(items_total, item_lo + per_block);

    for (;;) {
        int item = 0;
        if (lane == 0) item = atomicAdd(next_item, 1);
        item = __builtin_amdgcn_readfirstlane(item) + item_lo;
        if (item >= item_hi) break;
        const int r0 = item * 32;
        if (r0 >= a.R) continue;
        const int li = min(r0 + c, a.R - 1);
        const int row = a.rows[li];
        const float dyr = (UP & 2) ? a.up.dy[row] : 0.f;
        f32x16 accx[NT], acch[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) { accx[t][i] = 0.f; acch[t][i] = 0.f; }
        GRaw8 cur, nxt;
        g_issue8<UP>(a, H, 8 * half, row, cur);
#pragma unroll
        for (int fb = 0; fb < NFB; ++fb) {
            const int f0 = 16 * fb + 8 * half;
            float dh[8], r[8], z[8], n[8], hn[8], hp[8];
            f4_to_arr(cur.dh[0], cur.dh[1], dh); f4_to_arr(cur.r[0], cur.r[1], r); f4_to_arr(cur.z[0], cur.z[1], z);
            f4_to_arr(cur.n[0], cur.n[1], n); f4_to_arr(cur.hn[0], cur.hn[1], hn); f4_to_arr(cur.hp[0], cur.hp[1], hp);
            if (UP & 2) {
                const float4 w0 = *reinterpret_cast<const float4*>(sHead + f0);
                const float4 w1 = *reinterpret_cast<const float4*>(sHead + f0 + 4);
                dh[0] += dyr * w0.x; dh[1] += dyr * w0.y; dh[2] += dyr * w0.z; dh[3] += dyr * w0.w;
                dh[4] += dyr * w1.x; dh[5] += dyr * w1.y; dh[6] += dyr * w1.z; dh[7] += dyr * w1.w;
            }
            float ar[8], az[8], an[8], anr[8], ex[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float dn = dh[i] * (1.0f - z[i]) * (1.0f - n[i] * n[i]);
                ar[i] = dn * hn[i] * r[i] * (1.0f - r[i]);
                az[i] = dh[i] * (hp[i] - n[i]) * z[i] * (1.0f - z[i]);
                an[i] = dn;
                anr[i] = dn * r[i];
                ex[i] = dh[i] * z[i];
            }
            const Split8 sr = split8_arr(ar), sz = split8_arr(az), sn = split8_arr(an), snr = split8_arr(anr);
            // the pass-through term d_h += dh (.) z rides the matrix pipe as well: the three pieces of dh*z times an
            // identity fragment built in registers land in the accumulator layout exactly (1.0 is a bf16), so the
            // epilogue does not have to read z and dh a second time
            {
                const Split8 se = split8_arr(ex);
                const int te = (16 * fb) / 32;                           // the h tile that holds this block's 16 columns
                const int d = c - (16 * fb - 32 * te + 8 * half);         // this lane's output column relative to its k run
                const bool in = d >= 0 && d < 8;
                const uint32_t one = (d & 1) ? 0x3F800000u : 0x00003F80u;
                uint4 idf;
                idf.x = (in && (d >> 1) == 0) ? one : 0u;
                idf.y = (in && (d >> 1) == 1) ? one : 0u;
                idf.z = (in && (d >> 1) == 2) ? one : 0u;
                idf.w = (in && (d >> 1) == 3) ? one : 0u;
                acch[te] = mfma_bf16(idf, se.p3, acch[te]);
                acch[te] = mfma_bf16(idf, se.p2, acch[te]);
                acch[te] = mfma_bf16(idf, se.p1, acch[te]);
            }
            if (fb + 1 < NFB) g_issue8<UP>(a, H, 16 * (fb + 1) + 8 * half, row, nxt);
            __builtin_amdgcn_sched_barrier(0);
            const uint16_t* wp0 = sWT + c * JP + f0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const uint16_t* wx = wp0 + (t * 32) * JP + g * H;
                    const uint4 x1 = *reinterpret_cast<const uint4*>(wx);
                    const uint4 x2 = *reinterpret_cast<const uint4*>(wx + XH * JP);
                    const uint4 x3 = *reinterpret_cast<const uint4*>(wx + 2 * XH * JP);
                    accx[t] = mfma_x6(x1, x2, x3, g == 0 ? sr : (g == 1 ? sz : sn), accx[t]);
                    const uint16_t* wh = wp0 + (IN + t * 32) * JP + g * H;
                    const uint4 h1 = *reinterpret_cast<const uint4*>(wh);
                    const uint4 h2 = *reinterpret_cast<const uint4*>(wh + XH * JP);
                    const uint4 h3 = *reinterpret_cast<const uint4*>(wh + 2 * XH * JP);
                    acch[t] = mfma_x6(h1, h2, h3, g == 0 ? sr : (g == 1 ? sz : snr), acch[t]);
                }
            }
            cur = nxt;
        }
        // epilogue: lane = its own row; register 4q+i <-> column 8q + 4*half + i of the tile
        const bool live = r0 + c < a.R;
        if (live) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(a.d_msg + (size_t)row * a.ld_dmsg + t * 32 + 8 * q + 4 * half) =
                        make_float4(accx[t][4 * q], accx[t][4 * q + 1], accx[t][4 * q + 2], accx[t][4 * q + 3]);
        }
        int srow = 0, drow = 0;
        if (FUSE) { srow = a.add_src[li]; drow = a.add_dst[li]; }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float4 ex4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ex4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (FUSE) {
                    const int col = t * 32 + 8 * q + 4 * half;
                    const float4 u = *reinterpret_cast<const float4*>(a.add_msg + (size_t)srow * a.ld_add + col);
                    const float4 v = *reinterpret_cast<const float4*>(a.add_msg + (size_t)drow * a.ld_add + col);
                    ex4[q] = make_float4(u.x - v.x, u.y - v.y, u.z - v.z, u.w - v.w);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (live) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(a.d_h + (size_t)row * a.ld_dh + t * 32 + 8 * q + 4 * half) =
                        make_float4(acch[t][4 * q] + ex4[q].x, acch[t][4 * q + 1] + ex4[q].y, acch[t][4 * q + 2] + ex4[q].z,
                                    acch[t][4 * q + 3] + ex4[q].w);
            }
        }
    }
}

// Weight gradient, block-staged (IN == H): 32-row tiles of d_g = [dr|dz|dn|dn*r] and [x|h] are formed
// once in LDS and consumed by all four waves as MFMA operands (A = d_g^T, B = [x|h]); each wave owns
// 3 x (H/32) output tiles of dW_ih (waves 0,1) or dW_hh (waves 2,3).  Persistent blocks keep their
// partial dW in registers over all their tiles and write ONE slab each.
template <int H, int XMODE, int UP>
__global__ __launch_bounds__(256, 2) void k_gru_bwd_weights_lds(GruBwdWArgs a, int ntiles) {
    constexpr int NC = H / 32;           // column tiles per matrix
    constexpr int DG = 4 * H;            // dr | dz | dn | dnr
    constexpr int XHW = 2 * H;           // x | h
    constexpr int F8 = H / 8;            // threads per row in the staging phase
    constexpr int RT = 256 / F8;         // rows per tile (32 at H = 64)
    static_assert(RT == 32, "staging layout assumes 32-row tiles");
    __shared__ float s_dg[RT * DG];
    __shared__ float s_xh[RT * XHW];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, half = lane >> 5;
    const int which = wave >> 1;                 // 0: dW_ih (x columns), 1: dW_hh (h columns)
    const int jt0 = (wave & 1) * 3 * (H / 64) ;  // first of this wave's j tiles (3H/32 tiles split in two)
    constexpr int NJ = 3 * H / 64;               // j tiles per wave
    const size_t gp = a.gate_plane;
    const int srow = tid / F8, f8 = (tid % F8) * 8;

    f32x16 acc[NJ][NC];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < NC; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][t][i] = 0.f;
    float csum = 0.f;                            // column sum of d_g column `tid` (bias gradients)

    // LDS column of A for (j tile, lane): the n gate of dW_hh reads the dn*r block
    int colA[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int jj = (jt0 + j) * 32 + c;
        colA[j] = (which == 1 && jj >= 2 * H) ? jj + H : jj;
    }
    const int colB0 = which * H + c;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // ---- stage: 8 features of one row per thread
        const int lpos_raw = tile * RT + srow;
        const bool valid = lpos_raw < a.R;
        const int lpos = valid ? lpos_raw : a.R - 1;
        const int orow = a.rows[lpos];
        float dh[8], r[8], z[8], n[8], hn[8], hp[8], x[8];
        {
            const float4* p;
            float4 u, v;
            if (UP & 1) {
                p = reinterpret_cast<const float4*>(a.up.d_hout + (size_t)orow * a.up.ld_dhout + f8);
                u = p[0]; v = p[1];
            } else {
                u = make_float4(0.f, 0.f, 0.f, 0.f); v = u;
            }
            if (UP & 2) {
                const float d = a.up.dy[orow];
                const float4* q = reinterpret_cast<const float4*>(a.up.w_head + f8);
                const float4 w0 = q[0], w1 = q[1];
                u.x += d * w0.x; u.y += d * w0.y; u.z += d * w0.z; u.w += d * w0.w;
                v.x += d * w1.x; v.y += d * w1.y; v.z += d * w1.z; v.w += d * w1.w;
            }
            dh[0] = u.x; dh[1] = u.y; dh[2] = u.z; dh[3] = u.w; dh[4] = v.x; dh[5] = v.y; dh[6] = v.z; dh[7] = v.w;
            p = reinterpret_cast<const float4*>(a.gates + (size_t)orow * H + f8);
            u = p[0]; v = p[1];
            r[0] = u.x; r[1] = u.y; r[2] = u.z; r[3] = u.w; r[4] = v.x; r[5] = v.y; r[6] = v.z; r[7] = v.w;
            p = reinterpret_cast<const float4*>(a.gates + gp + (size_t)orow * H + f8);
            u = p[0]; v = p[1];
            z[0] = u.x; z[1] = u.y; z[2] = u.z; z[3] = u.w; z[4] = v.x; z[5] = v.y; z[6] = v.z; z[7] = v.w;
            p = reinterpret_cast<const float4*>(a.gates + 2 * gp + (size_t)orow * H + f8);
            u = p[0]; v = p[1];
            n[0] = u.x; n[1] = u.y; n[2] = u.z; n[3] = u.w; n[4] = v.x; n[5] = v.y; n[6] = v.z; n[7] = v.w;
            p = reinterpret_cast<const float4*>(a.gates + 3 * gp + (size_t)orow * H + f8);
            u = p[0]; v = p[1];
            hn[0] = u.x; hn[1] = u.y; hn[2] = u.z; hn[3] = u.w; hn[4] = v.x; hn[5] = v.y; hn[6] = v.z; hn[7] = v.w;
            p = reinterpret_cast<const float4*>(a.h + (size_t)orow * a.ld_h + f8);
            u = p[0]; v = p[1];
            hp[0] = u.x; hp[1] = u.y; hp[2] = u.z; hp[3] = u.w; hp[4] = v.x; hp[5] = v.y; hp[6] = v.z; hp[7] = v.w;
            if (XMODE == 0) {
                p = reinterpret_cast<const float4*>(a.msg + (size_t)(a.msg_compact ? lpos : orow) * a.ld_msg + f8);
                u = p[0]; v = p[1];
                x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = v.x; x[5] = v.y; x[6] = v.z; x[7] = v.w;
            } else {
                p = reinterpret_cast<const float4*>(a.h + (size_t)a.src[lpos] * a.ld_h + f8);
                u = p[0]; v = p[1];
                const float4* q = reinterpret_cast<const float4*>(a.h + (size_t)a.dst[lpos] * a.ld_h + f8);
                const float4 u2 = q[0], v2 = q[1];
                x[0] = u.x - u2.x; x[1] = u.y - u2.y; x[2] = u.z - u2.z; x[3] = u.w - u2.w;
                x[4] = v.x - v2.x; x[5] = v.y - v2.y; x[6] = v.z - v2.z; x[7] = v.w - v2.w;
            }
        }
        float dr[8], dz[8], dn[8], dnr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float d0 = valid ? dh[i] : 0.f;
            const float t = d0 * (1.0f - z[i]) * (1.0f - n[i] * n[i]);
            dn[i] = t;
            dnr[i] = t * r[i];
            dr[i] = t * hn[i] * r[i] * (1.0f - r[i]);
            dz[i] = d0 * (hp[i] - n[i]) * z[i] * (1.0f - z[i]);
        }
        __syncthreads();                         // the previous tile's MFMA phase has drained the LDS
        {
            float* d = s_dg + srow * DG + f8;
            *reinterpret_cast<float4*>(d) = make_float4(dr[0], dr[1], dr[2], dr[3]);
            *reinterpret_cast<float4*>(d + 4) = make_float4(dr[4], dr[5], dr[6], dr[7]);
            *reinterpret_cast<float4*>(d + H) = make_float4(dz[0], dz[1], dz[2], dz[3]);
            *reinterpret_cast<float4*>(d + H + 4) = make_float4(dz[4], dz[5], dz[6], dz[7]);
            *reinterpret_cast<float4*>(d + 2 * H) = make_float4(dn[0], dn[1], dn[2], dn[3]);
            *reinterpret_cast<float4*>(d + 2 * H + 4) = make_float4(dn[4], dn[5], dn[6], dn[7]);
            *reinterpret_cast<float4*>(d + 3 * H) = make_float4(dnr[0], dnr[1], dnr[2], dnr[3]);
            *reinterpret_cast<float4*>(d + 3 * H + 4) = make_float4(dnr[4], dnr[5], dnr[6], dnr[7]);
            float* e = s_xh + srow * XHW + f8;
            *reinterpret_cast<float4*>(e) = make_float4(x[0], x[1], x[2], x[3]);
            *reinterpret_cast<float4*>(e + 4) = make_float4(x[4], x[5], x[6], x[7]);
            *reinterpret_cast<float4*>(e + H) = make_float4(hp[0], hp[1], hp[2], hp[3]);
            *reinterpret_cast<float4*>(e + H + 4) = make_float4(hp[4], hp[5], hp[6], hp[7]);
        }
        __syncthreads();
        if (tid < DG) {
#pragma unroll 8
            for (int rr = 0; rr < RT; ++rr) csum += s_dg[rr * DG + tid];
        }
        // ---- MFMA: one step eats two rows (lane half picks the row)
#pragma unroll 4
        for (int s = 0; s < RT / 2; ++s) {
            const float* ar = s_dg + (2 * s + half) * DG;
            const float* br = s_xh + (2 * s + half) * XHW + colB0;
            float av[NJ], bv[NC];
#pragma unroll
            for (int j = 0; j < NJ; ++j) av[j] = ar[colA[j]];
#pragma unroll
            for (int t = 0; t < NC; ++t) bv[t] = br[t * 32];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int t = 0; t < NC; ++t) acc[j][t] = mfma32(av[j], bv[t], acc[j][t]);
        }
    }
    // ---- one slab per block: [3H][IN+H] weights, then [2][3H] biases
    float* sw = a.slab_w + (size_t)blockIdx.x * (3 * H) * XHW;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < NC; ++t)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int jj = (jt0 + j) * 32 + acc_row(reg, half);
                sw[(size_t)jj * XHW + which * H + t * 32 + c] = acc[j][t][reg];
            }
    if (tid < DG) {
        const float sum = csum;
        float* sb = a.slab_b + (size_t)blockIdx.x * 6 * H;
        const int g = tid / H, f = tid % H;
        if (g < 3) sb[g * H + f] = sum;                   // d_gi sums: dr | dz | dn
        if (g < 2) sb[3 * H + g * H + f] = sum;           // d_gh sums: dr | dz | dn*r
        if (g == 3) sb[3 * H + 2 * H + f] = sum;
    }
}


// ------------------------------------------------------------------------------------------
// Weight gradient on the bf16 pipe (bf16x6), H = IN = 64.  dW = d_g^T [x|h] contracts over ROWS, so both MFMA
// operands need 8 consecutive rows of one column per lane -- the transpose of how the data lies in HBM.
// Staging is the same as in k_gru_bwd_weights_lds (a thread owns 8 features of one row, 16-byte coalesced
// loads), but the 32-row tiles of d_g = [dr|dz|dn|dn*r] and [x|h] are written ROW-major as three bf16 pieces
// and the operands are fetched with the transposing LDS read ds_read_b64_tr_b16 (a 16-lane group reads
// 4 rows x 16 columns and receives them column-major): two reads give a lane its 8 rows.
// The 64-byte chunks of a row are XOR-swizzled with (row & 3), so the four rows of one transposing read fall
// into different bank windows without padding: 72 KiB per block, two 4-wave blocks per CU as before.
// ------------------------------------------------------------------------------------------
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 lds_read_tr(const uint16_t* p) {
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(p));
    return __builtin_bit_cast(uint2, v);
}
// element offset of (row, col) in a swizzled row-major bf16 image with `cols` columns (cols*2 bytes a multiple of 256)
template <int COLS>
__device__ __forceinline__ int swz_off(int row, int col) {
    return row * COLS + ((((col >> 5) ^ (row & 3)) << 5) | (col & 31));
}

struct WRaw { float4 dh[2], r[2], z[2], n[2], hn[2], hp[2], x[2], x2[2]; bool valid; };
// row ids of one staged row: fetched one tile AHEAD of the rows themselves, so the row loads of a tile do not
// start with a dependent index round trip (the kernel has no room to prefetch the rows; see the register note)
struct WIds { int lpos, orow, s, d; bool valid; };

template <int XMODE>
__device__ __forceinline__ WIds w_ids(const GruBwdWArgs& a, int tile, int srow) {
    WIds w;
    const int lpos_raw = tile * 32 + srow;
    w.valid = lpos_raw < a.R;
    w.lpos = w.valid ? lpos_raw : a.R - 1;
    w.orow = a.rows[w.lpos];
    w.s = XMODE != 0 ? a.src[w.lpos] : 0;
    w.d = XMODE != 0 ? a.dst[w.lpos] : 0;
    return w;
}

template <int XMODE, int UP>
__device__ __forceinline__ void w_issue(const GruBwdWArgs& a, const WIds& w, int f8, const float* s_head, WRaw& q) {
    constexpr int H = 64;
    q.valid = w.valid;
    const int lpos = w.lpos;
    const int orow = w.orow;
    const size_t gp = a.gate_plane;
    const float4* p;
    if (UP & 1) {
        p = reinterpret_cast<const float4*>(a.up.d_hout + (size_t)orow * a.up.ld_dhout + f8);
        q.dh[0] = p[0]; q.dh[1] = p[1];
    } else {
        q.dh[0] = make_float4(0.f, 0.f, 0.f, 0.f); q.dh[1] = q.dh[0];
    }
    if (UP & 2) {
        const float d = a.up.dy[orow];
        const float4* wh = reinterpret_cast<const float4*>(s_head + f8);       // head slice, staged in LDS once per block
        const float4 w0 = wh[0], w1 = wh[1];
        q.dh[0].x += d * w0.x; q.dh[0].y += d * w0.y; q.dh[0].z += d * w0.z; q.dh[0].w += d * w0.w;
        q.dh[1].x += d * w1.x; q.dh[1].y += d * w1.y; q.dh[1].z += d * w1.z; q.dh[1].w += d * w1.w;
    }
    p = reinterpret_cast<const float4*>(a.gates + (size_t)orow * H + f8);
    q.r[0] = p[0]; q.r[1] = p[1];
    p = reinterpret_cast<const float4*>(a.gates + gp + (size_t)orow * H + f8);
    q.z[0] = p[0]; q.z[1] = p[1];
    p = reinterpret_cast<const float4*>(a.gates + 2 * gp + (size_t)orow * H + f8);
    q.n[0] = p[0]; q.n[1] = p[1];
    p = reinterpret_cast<const float4*>(a.gates + 3 * gp + (size_t)orow * H + f8);
    q.hn[0] = p[0]; q.hn[1] = p[1];
    p = reinterpret_cast<const float4*>(a.h + (size_t)orow * a.ld_h + f8);
    q.hp[0] = p[0]; q.hp[1] = p[1];
    if (XMODE == 0) {
        p = reinterpret_cast<const float4*>(a.msg + (size_t)(a.msg_compact ? lpos : orow) * a.ld_msg + f8);
        q.x[0] = p[0]; q.x[1] = p[1];
    } else {
        p = reinterpret_cast<const float4*>(a.h + (size_t)w.s * a.ld_h + f8);
        q.x[0] = p[0]; q.x[1] = p[1];
        p = reinterpret_cast<const float4*>(a.h + (size_t)w.d * a.ld_h + f8);
        q.x2[0] = p[0]; q.x2[1] = p[1];
    }
}

template <int XMODE, int UP>
__global__ __launch_bounds__(256, 2) void k_gru_bwd_weights_split(GruBwdWArgs a, int ntiles) {
    constexpr int H = 64, DG = 4 * H, XHW = 2 * H, RT = 32, NJ = 3, NC = 2;
    extern __shared__ float lds[];
    uint16_t* sA = reinterpret_cast<uint16_t*>(lds);           // [3][RT][DG]   swizzled
    uint16_t* sB = sA + 3 * RT * DG;                           // [3][RT][XHW]  swizzled
    float* s_head = reinterpret_cast<float*>(sB + 3 * RT * XHW);   // [H] output head slice (UP & 2)
    if ((UP & 2) && threadIdx.x < H) s_head[threadIdx.x] = a.up.w_head[threadIdx.x];
    if (UP & 2) __syncthreads();
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, half = lane >> 5;
    const int which = wave >> 1;                 // 0: dW_ih (x columns), 1: dW_hh (h columns)
    const int jt0 = (wave & 1) * NJ;
    const int srow = tid >> 3, f8 = (tid & 7) * 8;
    // transposing-read coordinates of this lane: row q (+ 8*half, + 4 for the second read), columns 16*(g&1) + 4p
    const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3, tg = (lane >> 4) & 1;

    f32x16 acc[NJ][NC];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < NC; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][t][i] = 0.f;
    float cs[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) cs[k][i] = 0.f;

    int colA0[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int jj0 = (jt0 + j) * 32;
        colA0[j] = (which == 1 && jj0 >= 2 * H) ? jj0 + H : jj0;
    }

    WIds ids = w_ids<XMODE>(a, min((int)blockIdx.x, ntiles - 1), srow);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // (no cross-tile prefetch of the rows: the six accumulator tiles leave no room for it; the CU's second block
        //  covers that latency.  The row IDS of the next tile are fetched during this tile.)
        WRaw raw;
        w_issue<XMODE, UP>(a, ids, f8, s_head, raw);
        ids = w_ids<XMODE>(a, min(tile + (int)gridDim.x, ntiles - 1), srow);
        float dh[8], r[8], z[8], n[8], hn[8], hp[8], x[8];
        f4_to_arr(raw.dh[0], raw.dh[1], dh); f4_to_arr(raw.r[0], raw.r[1], r); f4_to_arr(raw.z[0], raw.z[1], z);
        f4_to_arr(raw.n[0], raw.n[1], n); f4_to_arr(raw.hn[0], raw.hn[1], hn); f4_to_arr(raw.hp[0], raw.hp[1], hp);
        f4_to_arr(raw.x[0], raw.x[1], x);
        if (XMODE != 0) {
            float x2[8];
            f4_to_arr(raw.x2[0], raw.x2[1], x2);
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] -= x2[i];
        }
        float dr[8], dz[8], dn[8], dnr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float d0 = raw.valid ? dh[i] : 0.f;
            const float t = d0 * (1.0f - z[i]) * (1.0f - n[i] * n[i]);
            dn[i] = t;
            dnr[i] = t * r[i];
            dr[i] = t * hn[i] * r[i] * (1.0f - r[i]);
            dz[i] = d0 * (hp[i] - n[i]) * z[i] * (1.0f - z[i]);
            cs[0][i] += dr[i]; cs[1][i] += dz[i]; cs[2][i] += dn[i]; cs[3][i] += dnr[i];
        }
        __syncthreads();                         // the previous tile's matrix phase has drained the LDS
        {
            // split each array right before its store (one array's pieces live at a time: the kernel sits at the
            // 256-register limit of two blocks per CU)
            constexpr int PA = RT * DG, PB = RT * XHW;
#define W_PUT(img, off, plane, arr)                                                                         \
    do {                                                                                                     \
        const Split8 sp_ = split8_arr(arr);                                                                  \
        uint16_t* d_ = (img) + (off);                                                                        \
        *reinterpret_cast<uint4*>(d_) = sp_.p1;                                                              \
        *reinterpret_cast<uint4*>(d_ + (plane)) = sp_.p2;                                                    \
        *reinterpret_cast<uint4*>(d_ + 2 * (plane)) = sp_.p3;                                                \
    } while (0)
            W_PUT(sA, swz_off<DG>(srow, f8), PA, dr);
            W_PUT(sA, swz_off<DG>(srow, H + f8), PA, dz);
            W_PUT(sA, swz_off<DG>(srow, 2 * H + f8), PA, dn);
            W_PUT(sA, swz_off<DG>(srow, 3 * H + f8), PA, dnr);
            W_PUT(sB, swz_off<XHW>(srow, f8), PB, x);
            W_PUT(sB, swz_off<XHW>(srow, H + f8), PB, hp);
#undef W_PUT
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < RT / 16; ++kb) {
            const int row0 = kb * 16 + 8 * half + tq;          // first read; the second is 4 rows further ((row & 3) == tq for both)
            Split8 b[NC];
#pragma unroll
            for (int t = 0; t < NC; ++t) {
                const int col = which * H + t * 32 + 16 * tg + 4 * tp;
                const uint16_t* p0 = sB + swz_off<XHW>(row0, col);
                const uint16_t* p1 = sB + swz_off<XHW>(row0 + 4, col);
                constexpr int PB = RT * XHW;
                const uint2 u0 = lds_read_tr(p0), u1 = lds_read_tr(p1);
                const uint2 v0 = lds_read_tr(p0 + PB), v1 = lds_read_tr(p1 + PB);
                const uint2 w0 = lds_read_tr(p0 + 2 * PB), w1 = lds_read_tr(p1 + 2 * PB);
                b[t].p1 = make_uint4(u0.x, u0.y, u1.x, u1.y);
                b[t].p2 = make_uint4(v0.x, v0.y, v1.x, v1.y);
                b[t].p3 = make_uint4(w0.x, w0.y, w1.x, w1.y);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = colA0[j] + 16 * tg + 4 * tp;
                const uint16_t* p0 = sA + swz_off<DG>(row0, col);
                const uint16_t* p1 = sA + swz_off<DG>(row0 + 4, col);
                constexpr int PA = RT * DG;
                const uint2 u0 = lds_read_tr(p0), u1 = lds_read_tr(p1);
                const uint2 v0 = lds_read_tr(p0 + PA), v1 = lds_read_tr(p1 + PA);
                const uint2 w0 = lds_read_tr(p0 + 2 * PA), w1 = lds_read_tr(p1 + 2 * PA);
                const uint4 a1 = make_uint4(u0.x, u0.y, u1.x, u1.y);
                const uint4 a2 = make_uint4(v0.x, v0.y, v1.x, v1.y);
                const uint4 a3 = make_uint4(w0.x, w0.y, w1.x, w1.y);
#pragma unroll
                for (int t = 0; t < NC; ++t) acc[j][t] = mfma_x6(a1, a2, a3, b[t], acc[j][t]);
            }
        }
    }
    // ---- one slab per block: [3H][IN+H] weights, then [2][3H] biases
    float* sw = a.slab_w + (size_t)blockIdx.x * (3 * H) * XHW;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < NC; ++t)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int jj = (jt0 + j) * 32 + acc_row(reg, half);
                sw[(size_t)jj * XHW + which * H + t * 32 + c] = acc[j][t][reg];
            }
    // bias gradients: column sums of d_g; 32 threads (one per tile row) hold partial sums of the same 8 features
    __syncthreads();
    float* red = lds;                                          // [32 rows][256] floats = 32 KiB (the images are dead)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) red[srow * DG + k * H + f8 + i] = cs[k][i];
    __syncthreads();
    {
        float sum = 0.f;
#pragma unroll 8
        for (int rr = 0; rr < RT; ++rr) sum += red[rr * DG + tid];
        float* sb = a.slab_b + (size_t)blockIdx.x * 6 * H;
        const int g = tid / H, ff = tid % H;
        if (g < 3) sb[g * H + ff] = sum;                   // d_gi sums: dr | dz | dn
        if (g < 2) sb[3 * H + g * H + ff] = sum;           // d_gh sums: dr | dz | dn*r
        if (g == 3) sb[3 * H + 2 * H + ff] = sum;
    }
}

// Weight gradient for the wide cells (H or IN a multiple of 64 beyond the 64/64 case): the same block-staged
// scheme, tiled over the OUTPUT.  blockIdx.y = (fc, cc) picks 64 hidden features (-> 192 rows of dW: the
// r, z and n gate of those features) and 128 columns of [x | h]; blockIdx.x is the row slab.  Per 32-row
// tile the block forms d_g = [dr|dz|dn|dn*r] for its 64 features and the 128-column operand slice in LDS
// (48 KiB, two blocks per CU) and each wave accumulates 3 x 2 output tiles, as above.  A 64-column half of
// a chunk never straddles the x / h boundary (IN, H multiples of 64), so a wave is wholly dW_ih or dW_hh.
template <int XMODE, int UP>
__global__ __launch_bounds__(256, 2) void k_gru_bwd_weights_chunk(GruBwdWArgs a, int ntiles, int n_cc) {
    constexpr int FC = 64, CC = 128, DG = 4 * FC, RT = 32;
    __shared__ float s_dg[RT * DG];
    __shared__ float s_xh[RT * CC];
    const int H = a.H, IN = a.IN, XH = IN + H;
    const int fc = blockIdx.y / n_cc, cc = blockIdx.y % n_cc;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, half = lane >> 5;
    const int col0 = cc * CC + (wave >> 1) * 64;     // first [x|h] column of this wave's two column tiles
    const bool col_live = col0 < XH;
    const bool is_h = col0 >= IN;
    const int jt0 = (wave & 1) * 3;                  // chunk-local j tiles: gate = jt >> 1, 32-half = jt & 1
    const size_t gp = a.gate_plane;
    const int srow = tid >> 3, q8 = tid & 7;
    const int f8 = fc * FC + q8 * 8;                 // this thread's 8 hidden features
    const int vc0 = cc * CC + q8 * 16;               // ... and its 16 operand columns

    f32x16 acc[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][t][i] = 0.f;
    float csum = 0.f;
    int colA[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int jj = (jt0 + j) * 32 + c;
        colA[j] = (is_h && jj >= 2 * FC) ? jj + FC : jj;
    }
    const int colB0 = (wave >> 1) * 64 + c;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int lpos_raw = tile * RT + srow;
        const bool valid = lpos_raw < a.R;
        const int lpos = valid ? lpos_raw : a.R - 1;
        const int orow = a.rows[lpos];
        float4 xv[4];
        if (vc0 >= XH) {
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (vc0 >= IN) {
            const float4* p = reinterpret_cast<const float4*>(a.h + (size_t)orow * a.ld_h + (vc0 - IN));
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = p[i];
        } else if (XMODE == 0) {
            const float4* p = reinterpret_cast<const float4*>(a.msg + (size_t)(a.msg_compact ? lpos : orow) * a.ld_msg + vc0);
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = p[i];
        } else if (XMODE == 1) {
            const float4* p = reinterpret_cast<const float4*>(a.h + (size_t)a.src[lpos] * a.ld_h + vc0);
            const float4* q = reinterpret_cast<const float4*>(a.h + (size_t)a.dst[lpos] * a.ld_h + vc0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 u = p[i], v = q[i];
                xv[i] = make_float4(u.x - v.x, u.y - v.y, u.z - v.z, u.w - v.w);
            }
        } else {
            const float4* p = vc0 < H ? reinterpret_cast<const float4*>(a.h + (size_t)a.src[lpos] * a.ld_h + vc0)
                                      : reinterpret_cast<const float4*>(a.h + (size_t)a.dst[lpos] * a.ld_h + (vc0 - H));
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = p[i];
        }
        float dh[8], r[8], z[8], n[8], hn[8], hp[8];
        {
            const float4* p;
            float4 u, v;
            if (UP & 1) {
                p = reinterpret_cast<const float4*>(a.up.d_hout + (size_t)orow * a.up.ld_dhout + f8);
                u = p[0]; v = p[1];
            } else {
                u = make_float4(0.f, 0.f, 0.f, 0.f); v = u;
            }
            if (UP & 2) {
                const float d = a.up.dy[orow];
                const float4* q = reinterpret_cast<const float4*>(a.up.w_head + f8);
                const float4 w0 = q[0], w1 = q[1];
                u.x += d * w0.x; u.y += d * w0.y; u.z += d * w0.z; u.w += d * w0.w;
                v.x += d * w1.x; v.y += d * w1.y; v.z += d * w1.z; v.w += d * w1.w;
            }
            dh[0] = u.x; dh[1] = u.y; dh[2] = u.z; dh[3] = u.w; dh[4] = v.x; dh[5] = v.y; dh[6] = v.z; dh[7] = v.w;
            p = reinterpret_cast<const float4*>(a.gates + (size_t)orow * H + f8);
            u = p[0]; v = p[1];
            r[0] = u.x; r[1] = u.y; r[2] = u.z; r[3] = u.w; r[4] = v.x; r[5] = v.y; r[6] = v.z; r[7] = v.w;
            p = reinterpret_cast<const float4*>(a.gates + gp + (size_t)orow * H + f8);
            u = p[0]; v = p[1];
            z[0] = u.x; z[1] = u.y; z[2] = u.z; z[3] = u.w; z[4] = v.x; z[5] = v.y; z[6] = v.z; z[7] = v.w;
            p = reinterpret_cast<const float4*>(a.gates + 2 * gp + (size_t)orow * H + f8);
            u = p[0]; v = p[1];
            n[0] = u.x; n[1] = u.y; n[2] = u.z; n[3] = u.w; n[4] = v.x; n[5] = v.y; n[6] = v.z; n[7] = v.w;
            p = reinterpret_cast<const float4*>(a.gates + 3 * gp + (size_t)orow * H + f8);
            u = p[0]; v = p[1];
            hn[0] = u.x; hn[1] = u.y; hn[2] = u.z; hn[3] = u.w; hn[4] = v.x; hn[5] = v.y; hn[6] = v.z; hn[7] = v.w;
            p = reinterpret_cast<const float4*>(a.h + (size_t)orow * a.ld_h + f8);
            u = p[0]; v = p[1];
            hp[0] = u.x; hp[1] = u.y; hp[2] = u.z; hp[3] = u.w; hp[4] = v.x; hp[5] = v.y; hp[6] = v.z; hp[7] = v.w;
        }
        float dr[8], dz[8], dn[8], dnr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float d0 = valid ? dh[i] : 0.f;
            const float t = d0 * (1.0f - z[i]) * (1.0f - n[i] * n[i]);
            dn[i] = t;
            dnr[i] = t * r[i];
            dr[i] = t * hn[i] * r[i] * (1.0f - r[i]);
            dz[i] = d0 * (hp[i] - n[i]) * z[i] * (1.0f - z[i]);
        }
        __syncthreads();                         // the previous tile's MFMA phase has drained the LDS
        {
            float* d = s_dg + srow * DG + q8 * 8;
            *reinterpret_cast<float4*>(d) = make_float4(dr[0], dr[1], dr[2], dr[3]);
            *reinterpret_cast<float4*>(d + 4) = make_float4(dr[4], dr[5], dr[6], dr[7]);
            *reinterpret_cast<float4*>(d + FC) = make_float4(dz[0], dz[1], dz[2], dz[3]);
            *reinterpret_cast<float4*>(d + FC + 4) = make_float4(dz[4], dz[5], dz[6], dz[7]);
            *reinterpret_cast<float4*>(d + 2 * FC) = make_float4(dn[0], dn[1], dn[2], dn[3]);
            *reinterpret_cast<float4*>(d + 2 * FC + 4) = make_float4(dn[4], dn[5], dn[6], dn[7]);
            *reinterpret_cast<float4*>(d + 3 * FC) = make_float4(dnr[0], dnr[1], dnr[2], dnr[3]);
            *reinterpret_cast<float4*>(d + 3 * FC + 4) = make_float4(dnr[4], dnr[5], dnr[6], dnr[7]);
            float* e = s_xh + srow * CC + q8 * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(e + 4 * i) = xv[i];
        }
        __syncthreads();
        if (cc == 0) {
#pragma unroll 8
            for (int rr = 0; rr < RT; ++rr) csum += s_dg[rr * DG + tid];
        }
        if (col_live) {
#pragma unroll 4
            for (int s = 0; s < RT / 2; ++s) {
                const float* ar = s_dg + (2 * s + half) * DG;
                const float* br = s_xh + (2 * s + half) * CC + colB0;
                float av[3], bv[2];
#pragma unroll
                for (int j = 0; j < 3; ++j) av[j] = ar[colA[j]];
#pragma unroll
                for (int t = 0; t < 2; ++t) bv[t] = br[t * 32];
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[j][t] = mfma32(av[j], bv[t], acc[j][t]);
            }
        }
    }
    if (col_live) {
        float* sw = a.slab_w + (size_t)blockIdx.x * (3 * H) * XH;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int jt = jt0 + j;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int jj = (jt >> 1) * H + fc * FC + (jt & 1) * 32 + acc_row(reg, half);
                    sw[(size_t)jj * XH + col0 + t * 32 + c] = acc[j][t][reg];
                }
        }
    }
    if (cc == 0) {
        float* sb = a.slab_b + (size_t)blockIdx.x * 6 * H;
        const int g = tid / FC, f = fc * FC + tid % FC;
        if (g < 3) sb[g * H + f] = csum;                  // d_gi sums: dr | dz | dn
        if (g < 2) sb[3 * H + g * H + f] = csum;          // d_gh sums: dr | dz | dn*r
        if (g == 3) sb[3 * H + 2 * H + f] = csum;
    }
}


// ==========================================================================================
// One-pass backward of one cell (H = 64, IN = H, bf16x6 products): data gradient AND weight gradient from ONE
// read of dh, the four gate planes and h.  The two stand-alone kernels stream those six planes twice (56H bytes per
// row together); this one moves 32H.  What kept the two apart was LDS: 150 KiB of transposed weight pieces (data)
// and 72 KiB of operand images (weights) do not fit together.  Here the WEIGHTS LIVE IN REGISTERS: a block is four
// waves, one per SIMD, each with the full 512-register budget; wave w owns one 32-column tile of the 128 output
// columns [d_msg | d_h] and keeps its 32 x 192 slice of W_ih / W_hh as MFMA A operands (three bf16 pieces, 144
// registers) for the whole kernel.  Per 32-row tile
//   * every thread forms 8 columns of one row of d_g = [dr|dz|dn|dn*r], [x|h] and dh*z (+ the fused row-F adjoint),
//     splits them into bf16 pieces and stores them row-major into ONE set of LDS images (80 KiB, double buffered)
//     that serves both products: `ds_read_b128` with lane = row gives the B operand of the data product,
//     `ds_read_b64_tr_b16` gives d_g^T and [x|h] as the operands of dW (image (b) of the guide's dual-use layout:
//     16-byte chunk ch of row r sits at ch ^ (((r&3)<<2) | ((r>>2)&3)), conflict-free for both kinds of read);
//   * wave w runs its 72 data MFMAs (transposed accumulator, lane = row) and its 72 weight-gradient MFMAs (six
//     accumulator tiles kept over all tiles of the persistent block, one slab per block at the end);
//   * the rows of tile i+2 are requested as soon as tile i+1's registers have been consumed, so every load has a
//     whole tile time to land; one barrier per tile.
// ==========================================================================================
struct GruBwdFusedArgs {
    const int32_t* rows; int R; const int32_t* src; const int32_t* dst;
    const float* msg; int ld_msg; int msg_compact;
    const float* h; int ld_h;
    const float* w_ih; const float* w_hh;
    const float* gates; size_t gate_plane;
    DhSrc up;
    float* d_msg; int ld_dmsg; float* d_h; int ld_dh;
    const int32_t* add_src; const int32_t* add_dst; const float* add_msg; int ld_add;
    float* slab_w; float* slab_b;
    int ld_wih;            // row stride of w_ih (= IN; the concat message's two halves are passed as column slices of [3H][2H])
};

__device__ __forceinline__ int dui_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
// element index of (row, col) in a [32][128] bf16 dual-use image
__device__ __forceinline__ int dui_off(int row, int col) {
    return row * 128 + ((((col >> 3) ^ dui_swz(row)) << 3) | (col & 7));
}

// One thread stages 4 columns of one row in each HALF of a tile (rows 0..15 = stream A, 16..31 = stream B); the two
// streams are requested, consumed and re-requested half a tile apart, so that only one half's arrays are alive at a time.
struct HalfIds { int orow, s, d, mrow; bool valid; };
struct HalfRaw { float4 dh, r, z, n, hn, hp, xa, xb, ea, eb; float dy; };
struct HalfVals { float dr[4], dz[4], dn[4], dnr[4], x[4], hp[4], ex[4]; };

template <int XMODE, bool FUSE>
__device__ __forceinline__ HalfIds half_ids(const GruBwdFusedArgs& a, int tile, bool tv, int row) {
    HalfIds w;
    const int lr = tile * 32 + row;
    w.valid = tv && lr < a.R;
    const int lpos = w.valid ? lr : a.R - 1;
    w.orow = a.rows[lpos];
    // with XMODE != 0 the fused adjoint gathers through the cell's own src / dst (checked on the host)
    w.s = XMODE != 0 ? a.src[lpos] : (FUSE ? a.add_src[lpos] : 0);
    w.d = XMODE != 0 ? a.dst[lpos] : (FUSE ? a.add_dst[lpos] : 0);
    w.mrow = XMODE == 0 ? (a.msg_compact ? lpos : w.orow) : 0;
    return w;
}

// the row's own planes ...
template <int UP>
__device__ __forceinline__ void half_issue_main(const GruBwdFusedArgs& a, const HalfIds& w, int f4, HalfRaw& q) {
    constexpr int H = 64;
    const size_t gp = a.gate_plane;
    if (UP & 1) q.dh = *reinterpret_cast<const float4*>(a.up.d_hout + (size_t)w.orow * a.up.ld_dhout + f4);
    if (UP & 2) q.dy = a.up.dy[w.orow];
    const float* g0 = a.gates + (size_t)w.orow * H + f4;
    q.r = *reinterpret_cast<const float4*>(g0);
    q.z = *reinterpret_cast<const float4*>(g0 + gp);
    q.n = *reinterpret_cast<const float4*>(g0 + 2 * gp);
    q.hn = *reinterpret_cast<const float4*>(g0 + 3 * gp);
    q.hp = *reinterpret_cast<const float4*>(a.h + (size_t)w.orow * a.ld_h + f4);
}
// ... and what it gathers from its endpoints (det rows, mostly L2 hits: requested later, consumed last)
template <int XMODE, bool FUSE>
__device__ __forceinline__ void half_issue_gather(const GruBwdFusedArgs& a, const HalfIds& w, int f4, HalfRaw& q) {
    if (XMODE == 0) {
        q.xa = *reinterpret_cast<const float4*>(a.msg + (size_t)w.mrow * a.ld_msg + f4);
    } else {
        q.xa = *reinterpret_cast<const float4*>(a.h + (size_t)w.s * a.ld_h + f4);
        q.xb = *reinterpret_cast<const float4*>(a.h + (size_t)w.d * a.ld_h + f4);
    }
    if (FUSE) {                                   // the fused row-F adjoint gathers through the cell's own src / dst
        q.ea = *reinterpret_cast<const float4*>(a.add_msg + (size_t)w.s * a.ld_add + f4);
        q.eb = *reinterpret_cast<const float4*>(a.add_msg + (size_t)w.d * a.ld_add + f4);
    }
}
template <int XMODE, int UP, bool FUSE>
__device__ __forceinline__ void half_issue(const GruBwdFusedArgs& a, const HalfIds& w, int f4, HalfRaw& q) {
    half_issue_main<UP>(a, w, f4, q);
    half_issue_gather<XMODE, FUSE>(a, w, f4, q);
}

template <int XMODE, int UP, bool FUSE>
__device__ __forceinline__ void half_vals(const HalfRaw& q, bool valid, const float* head4, HalfVals& v) {
    const float dh[4] = {q.dh.x, q.dh.y, q.dh.z, q.dh.w}, r[4] = {q.r.x, q.r.y, q.r.z, q.r.w};
    const float z[4] = {q.z.x, q.z.y, q.z.z, q.z.w}, n[4] = {q.n.x, q.n.y, q.n.z, q.n.w};
    const float hn[4] = {q.hn.x, q.hn.y, q.hn.z, q.hn.w}, hp[4] = {q.hp.x, q.hp.y, q.hp.z, q.hp.w};
    const float xa[4] = {q.xa.x, q.xa.y, q.xa.z, q.xa.w}, xb[4] = {q.xb.x, q.xb.y, q.xb.z, q.xb.w};
    const float ea[4] = {q.ea.x, q.ea.y, q.ea.z, q.ea.w}, eb[4] = {q.eb.x, q.eb.y, q.eb.z, q.eb.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float d0 = (UP & 1) ? dh[i] : 0.f;
        if (UP & 2) d0 += q.dy * head4[i];
        d0 = valid ? d0 : 0.f;
        const float t = d0 * (1.0f - z[i]) * (1.0f - n[i] * n[i]);
        v.dn[i] = t;
        v.dnr[i] = t * r[i];
        v.dr[i] = t * hn[i] * r[i] * (1.0f - r[i]);
        v.dz[i] = d0 * (hp[i] - n[i]) * z[i] * (1.0f - z[i]);
        v.ex[i] = d0 * z[i];
        if (FUSE) v.ex[i] += ea[i] - eb[i];
        v.hp[i] = hp[i];
        v.x[i] = XMODE != 0 ? xa[i] - xb[i] : xa[i];
    }
}

// four consecutive columns of one row -> three bf16 pieces, 8 bytes each
__device__ __forceinline__ void half_put(uint16_t* img, int off, int pstride, const float* arr) {
    uint2 p1, p2, p3;
    split_pair(arr[0], arr[1], p1.x, p2.x, p3.x);
    split_pair(arr[2], arr[3], p1.y, p2.y, p3.y);
    *reinterpret_cast<uint2*>(img + off) = p1;
    *reinterpret_cast<uint2*>(img + off + pstride) = p2;
    *reinterpret_cast<uint2*>(img + off + 2 * pstride) = p3;
}

#define ONE_PIN4(q) asm volatile("" : "+v"((q).x), "+v"((q).y), "+v"((q).z), "+v"((q).w))
// One sixth of a stream's staging, computed from the landed rows right where it is stored (the empty asm pins the work
// to its half-group: left alone the compiler forms and splits all arrays up front and carries ~60 registers of pieces
// through the matrix phase).  d0 = upstream gradient, t = d0 (1-z)(1-n^2) are carried from slice 0 to the later ones.
template <int XMODE, int UP, bool FUSE>
__device__ __forceinline__ void half_slice(int SL, HalfRaw& q, bool valid, const float* head4, float (&d0)[4], float (&t)[4],
                                           uint16_t* img, int s0, int s1, int se, int SUB, int PA, int PB, int OFF_B,
                                           int OFF_E) {
    float o[4];
    if (SL == 0) {
        if (UP & 1) ONE_PIN4(q.dh);
        ONE_PIN4(q.z); ONE_PIN4(q.n); ONE_PIN4(q.hn); ONE_PIN4(q.r);
        const float dh[4] = {q.dh.x, q.dh.y, q.dh.z, q.dh.w}, r[4] = {q.r.x, q.r.y, q.r.z, q.r.w};
        const float z[4] = {q.z.x, q.z.y, q.z.z, q.z.w}, n[4] = {q.n.x, q.n.y, q.n.z, q.n.w};
        const float hn[4] = {q.hn.x, q.hn.y, q.hn.z, q.hn.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float d = (UP & 1) ? dh[i] : 0.f;
            if (UP & 2) d += q.dy * head4[i];
            d0[i] = valid ? d : 0.f;
            t[i] = d0[i] * (1.0f - z[i]) * (1.0f - n[i] * n[i]);
            o[i] = t[i] * hn[i] * r[i] * (1.0f - r[i]);
        }
        half_put(img, s0, PA, o);
    } else if (SL == 1) {
        ONE_PIN4(q.hp);
        const float z[4] = {q.z.x, q.z.y, q.z.z, q.z.w}, n[4] = {q.n.x, q.n.y, q.n.z, q.n.w};
        const float hp[4] = {q.hp.x, q.hp.y, q.hp.z, q.hp.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = d0[i] * (hp[i] - n[i]) * z[i] * (1.0f - z[i]);
        half_put(img, s1, PA, o);
    } else if (SL == 2) {
        asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
        half_put(img, SUB + s0, PA, t);
    } else if (SL == 3) {
        asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
        const float r[4] = {q.r.x, q.r.y, q.r.z, q.r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = t[i] * r[i];
        half_put(img, SUB + s1, PA, o);
    } else if (SL == 4) {
        ONE_PIN4(q.xa);
        const float xa[4] = {q.xa.x, q.xa.y, q.xa.z, q.xa.w}, xb[4] = {q.xb.x, q.xb.y, q.xb.z, q.xb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = XMODE != 0 ? xa[i] - xb[i] : xa[i];
        half_put(img + OFF_B, s0, PB, o);
    } else {
        ONE_PIN4(q.hp);
        const float hp[4] = {q.hp.x, q.hp.y, q.hp.z, q.hp.w}, z[4] = {q.z.x, q.z.y, q.z.z, q.z.w};
        half_put(img + OFF_B, s1, PB, hp);
        const float ea[4] = {q.ea.x, q.ea.y, q.ea.z, q.ea.w}, eb[4] = {q.eb.x, q.eb.y, q.eb.z, q.eb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[i] = d0[i] * z[i];
            if (FUSE) o[i] += ea[i] - eb[i];
        }
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(img + OFF_E) + se) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

__device__ __forceinline__ float dot2_ones(uint32_t two_bf16, float acc) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, two_bf16), __builtin_bit_cast(bf16x2, 0x3F803F80u), acc, false);
}

// product `c` of the six that make one fp32 product (smallest terms first; see mfma_x6)
template <int C>
__device__ __forceinline__ f32x16 mfma_c(const uint4 (&a)[3], const Split8& b, f32x16 acc) {
    if (C == 0) return mfma_bf16(a[2], b.p1, acc);
    if (C == 1) return mfma_bf16(a[0], b.p3, acc);
    if (C == 2) return mfma_bf16(a[1], b.p2, acc);
    if (C == 3) return mfma_bf16(a[1], b.p1, acc);
    if (C == 4) return mfma_bf16(a[0], b.p2, acc);
    return mfma_bf16(a[0], b.p1, acc);
}

#ifdef TMPNN_KEEP_VARIANTS      // the round-2 four-wave form of the one-pass backward: comparison builds only
template <int XMODE, int UP, bool FUSE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_gru_bwd_one(GruBwdFusedArgs a, int ntiles) {
    constexpr int H = 64;
    constexpr int SUB = 32 * 128;                  // elements of one [32][128] image
    constexpr int PA = 2 * SUB, PB = SUB;          // piece strides of the d_g (two images) and [x|h] (one) sets
    constexpr int OFF_B = 3 * PA, OFF_E = OFF_B + 3 * PB;          // in uint16 elements
    constexpr int BUF = OFF_E + 32 * 64 * 2;       // 40960 elements = 80 KiB per buffer
    extern __shared__ float lds[];
    uint16_t* const lds16 = reinterpret_cast<uint16_t*>(lds);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int c = lane & 31, half = lane >> 5;
    const int hr = tid >> 4, f4 = (tid & 15) * 4;  // staging: row hr (stream A) / 16 + hr (stream B), columns f4..f4+3
    // ---- roles
    const bool is_dx = wave < 2;                   // data product: waves 0,1 -> d_msg columns, 2,3 -> d_h columns
    const int n0 = (wave & 1) * 32;
    const int which = wave >> 1;                   // weight gradient: waves 0,1 -> dW_ih, 2,3 -> dW_hh
    const int jt0 = (wave & 1) * 3;
    // ---- this wave's slice of W^T as A operands: lane (c, half), k-step ks: W[16 ks + 8 half + i][n0 + c]
    uint4 wq[12][3];
    {
        const float* W = is_dx ? a.w_ih : a.w_hh;
#pragma unroll
        for (int ks = 0; ks < 12; ++ks) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = W[(size_t)(16 * ks + 8 * half + i) * H + n0 + c];
            const Split8 s = split8_arr(v);
            wq[ks][0] = s.p1; wq[ks][1] = s.p2; wq[ks][2] = s.p3;
        }
    }
    float head4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) head4[i] = (UP & 2) ? a.up.w_head[f4 + i] : 0.f;
    // ---- staging offsets: rows hr and 16 + hr have the same chunk permutation up to the (row >> 2) & 3 bits
    const int stA0 = dui_off(hr, f4), stA1 = dui_off(hr, 64 + f4);
    const int seA = hr * 64 + (((f4 >> 2) ^ (hr & 15)) << 2);
    constexpr int stB = 16 * 128, seB = 16 * 64;   // row 16 + hr has row hr's chunk permutation: a constant offset
    // ---- data product reads: lane = row c
    const int swzc = dui_swz(c), rowc = c * 128;
    const int hix = is_dx ? 0 : 64;                // d_h takes dn*r (image columns 192..255) for the n gate
    // ---- transposed reads (weight gradient): rows 8 half + tq (+4) of a 16-row block, columns 16 tg + 4 tp
    const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3, tg = (lane >> 4) & 1;
    const int trow = (8 * half + tq) * 128, tsw0 = (tq << 2) | (2 * half), tsw1 = tsw0 | 1;
    int offA[3][2], offB[2][2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int jj0 = (jt0 + j) * 32;
        const int col = (which == 1 && jj0 >= 2 * H) ? jj0 + H : jj0;        // image column of the tile's first d_g column
        const int ch = ((col & 127) >> 3) + 2 * tg + (tp >> 1);
        offA[j][0] = (col >> 7) * SUB + trow + ((ch ^ tsw0) << 3) + 4 * (tp & 1);
        offA[j][1] = (col >> 7) * SUB + trow + 4 * 128 + ((ch ^ tsw1) << 3) + 4 * (tp & 1);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ch = ((which * H + t * 32) >> 3) + 2 * tg + (tp >> 1);
        offB[t][0] = OFF_B + trow + ((ch ^ tsw0) << 3) + 4 * (tp & 1);
        offB[t][1] = OFF_B + trow + 4 * 128 + ((ch ^ tsw1) << 3) + 4 * (tp & 1);
    }
    const int eoff = c * 64;                       // dh*z image: float index of row c

    f32x16 acc[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][t][i] = 0.f;
    // bias gradients = column sums of d_g: taken from the A operands of the weight gradient (a lane holds 8 rows of
    // one column as bf16 pieces; v_dot2c_f32_bf16 against (1, 1) adds two of them per instruction)
    float bsum[3] = {0.f, 0.f, 0.f};

    const int G = gridDim.x;
    const int nmine = (ntiles - (int)blockIdx.x + G - 1) / G;      // >= 1: the grid never exceeds ntiles
    HalfRaw rawA, rawB;
    HalfVals v;
#define ONE_STAGE(img, s0, s1, se)                                                                           \
    do {                                                                                                     \
        half_put((img), (s0), PA, v.dr); half_put((img), (s1), PA, v.dz);                                    \
        half_put((img), SUB + (s0), PA, v.dn); half_put((img), SUB + (s1), PA, v.dnr);                       \
        half_put((img) + OFF_B, (s0), PB, v.x); half_put((img) + OFF_B, (s1), PB, v.hp);                     \
        *reinterpret_cast<float4*>(reinterpret_cast<float*>((img) + OFF_E) + (se)) =                         \
            make_float4(v.ex[0], v.ex[1], v.ex[2], v.ex[3]);                                                 \
    } while (0)
    // ---- prologue: tile 0 staged into buffer 0, tile 1 requested, ids of tile 2 fetched
    bool validA, validB;
    HalfIds idA, idB;
    {
        const HalfIds a0 = half_ids<XMODE, FUSE>(a, blockIdx.x, true, hr), b0 = half_ids<XMODE, FUSE>(a, blockIdx.x, true, 16 + hr);
        half_issue<XMODE, UP, FUSE>(a, a0, f4, rawA);
        half_issue<XMODE, UP, FUSE>(a, b0, f4, rawB);
        const HalfIds a1 = half_ids<XMODE, FUSE>(a, blockIdx.x + G, 1 < nmine, hr);
        const HalfIds b1 = half_ids<XMODE, FUSE>(a, blockIdx.x + G, 1 < nmine, 16 + hr);
        half_vals<XMODE, UP, FUSE>(rawA, a0.valid, head4, v);
        ONE_STAGE(lds16, stA0, stA1, seA);
        half_issue<XMODE, UP, FUSE>(a, a1, f4, rawA);
        half_vals<XMODE, UP, FUSE>(rawB, b0.valid, head4, v);
        ONE_STAGE(lds16, stA0 + stB, stA1 + stB, seA + seB);
        half_issue<XMODE, UP, FUSE>(a, b1, f4, rawB);
        validA = a1.valid; validB = b1.valid;
        idA = half_ids<XMODE, FUSE>(a, blockIdx.x + 2 * G, 2 < nmine, hr);
        idB = b1;                                  // stream B's gathers of tile 1 are requested (again) at hs 5 of tile 0
    }
    // epilogue row of tile 0 (lane = row c)
    int erow = a.rows[min((int)blockIdx.x * 32 + c, a.R - 1)];
    bool elive = (int)blockIdx.x * 32 + c < a.R;
    __syncthreads();

    for (int it = 0; it < nmine; ++it) {
        const int tile = blockIdx.x + it * G;
        uint16_t* const cur = lds16 + (it & 1) * BUF;
        uint16_t* const nxt = lds16 + ((it & 1) ^ 1) * BUF;
        // operand reads of the matrix phase
        Split8 bD[2], bt[2];
        uint4 aW[1][3];
#define ONE_LD_D(ks)                                                                                         \
    do {                                                                                                     \
        int inrow_ = ((2 * ((ks) & 7) + half) ^ swzc) << 3;                                                  \
        if ((ks) >= 8) inrow_ ^= hix;                                                                        \
        const uint16_t* p_ = cur + ((ks) >> 3) * SUB + rowc + inrow_;                                        \
        bD[(ks) & 1].p1 = *reinterpret_cast<const uint4*>(p_);                                               \
        bD[(ks) & 1].p2 = *reinterpret_cast<const uint4*>(p_ + PA);                                          \
        bD[(ks) & 1].p3 = *reinterpret_cast<const uint4*>(p_ + 2 * PA);                                      \
    } while (0)
#define ONE_LD_TR(base0, base1, pstride, q1, q2, q3)                                                         \
    do {                                                                                                     \
        const uint16_t* p0_ = (base0);                                                                       \
        const uint16_t* p1_ = (base1);                                                                       \
        const uint2 u0_ = lds_read_tr(p0_), u1_ = lds_read_tr(p1_);                                          \
        const uint2 v0_ = lds_read_tr(p0_ + (pstride)), v1_ = lds_read_tr(p1_ + (pstride));                 \
        const uint2 w0_ = lds_read_tr(p0_ + 2 * (pstride)), w1_ = lds_read_tr(p1_ + 2 * (pstride));         \
        (q1) = make_uint4(u0_.x, u0_.y, u1_.x, u1_.y);                                                       \
        (q2) = make_uint4(v0_.x, v0_.y, v1_.x, v1_.y);                                                       \
        (q3) = make_uint4(w0_.x, w0_.y, w1_.x, w1_.y);                                                       \
    } while (0)
#define ONE_LD_BT(kb)                                                                                        \
    do {                                                                                                     \
        ONE_LD_TR(cur + (kb) * 2048 + offB[0][0], cur + (kb) * 2048 + offB[0][1], PB, bt[0].p1, bt[0].p2, bt[0].p3); \
        ONE_LD_TR(cur + (kb) * 2048 + offB[1][0], cur + (kb) * 2048 + offB[1][1], PB, bt[1].p1, bt[1].p2, bt[1].p3); \
    } while (0)
#define ONE_LD_A(g)                                                                                          \
    ONE_LD_TR(cur + ((g) / 3) * 2048 + offA[(g) % 3][0], cur + ((g) / 3) * 2048 + offA[(g) % 3][1], PA,      \
              aW[0][0], aW[0][1], aW[0][2])
        ONE_LD_D(0);
        ONE_LD_BT(0);
        ONE_LD_A(0);
        const int erow_n = a.rows[min((tile + G) * 32 + c, a.R - 1)];
        const bool elive_n = (it + 1 < nmine) && ((tile + G) * 32 + c < a.R);

        f32x16 accd;
#pragma unroll
        for (int i = 0; i < 16; ++i) accd[i] = 0.f;
        float d0[4], tt[4];
        // 12 half-groups: k-step hs of the data product (6 MFMAs, one chain) interleaved with half of weight-gradient
        // group hs/2 (6 MFMAs on two chains); the staging of one array of the next tile rides along with each
#pragma unroll
        for (int hs = 0; hs < 12; ++hs) {
            const int g = hs >> 1, kk = hs & 1, j = g % 3;
            if (hs + 1 < 12) ONE_LD_D(hs + 1);
            if (kk == 0) {
                acc[j][0] = mfma_c<0>(aW[0], bt[0], acc[j][0]);  accd = mfma_c<0>(wq[hs], bD[hs & 1], accd);
                acc[j][1] = mfma_c<0>(aW[0], bt[1], acc[j][1]);  accd = mfma_c<1>(wq[hs], bD[hs & 1], accd);
                acc[j][0] = mfma_c<1>(aW[0], bt[0], acc[j][0]);  accd = mfma_c<2>(wq[hs], bD[hs & 1], accd);
                acc[j][1] = mfma_c<1>(aW[0], bt[1], acc[j][1]);  accd = mfma_c<3>(wq[hs], bD[hs & 1], accd);
                acc[j][0] = mfma_c<2>(aW[0], bt[0], acc[j][0]);  accd = mfma_c<4>(wq[hs], bD[hs & 1], accd);
                acc[j][1] = mfma_c<2>(aW[0], bt[1], acc[j][1]);  accd = mfma_c<5>(wq[hs], bD[hs & 1], accd);
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) {
                    const uint4 q = aW[0][pc];
                    bsum[j] = dot2_ones(q.x, bsum[j]); bsum[j] = dot2_ones(q.y, bsum[j]);
                    bsum[j] = dot2_ones(q.z, bsum[j]); bsum[j] = dot2_ones(q.w, bsum[j]);
                }
            } else {
                accd = mfma_c<0>(wq[hs], bD[hs & 1], accd);  acc[j][0] = mfma_c<3>(aW[0], bt[0], acc[j][0]);
                accd = mfma_c<1>(wq[hs], bD[hs & 1], accd);  acc[j][1] = mfma_c<3>(aW[0], bt[1], acc[j][1]);
                accd = mfma_c<2>(wq[hs], bD[hs & 1], accd);  acc[j][0] = mfma_c<4>(aW[0], bt[0], acc[j][0]);
                accd = mfma_c<3>(wq[hs], bD[hs & 1], accd);  acc[j][1] = mfma_c<4>(aW[0], bt[1], acc[j][1]);
                accd = mfma_c<4>(wq[hs], bD[hs & 1], accd);  acc[j][0] = mfma_c<5>(aW[0], bt[0], acc[j][0]);
                accd = mfma_c<5>(wq[hs], bD[hs & 1], accd);  acc[j][1] = mfma_c<5>(aW[0], bt[1], acc[j][1]);
            }
            if (kk == 1 && g + 1 < 6) ONE_LD_A(g + 1);
            if (hs == 5) ONE_LD_BT(1);
            // staging of the next tile: stream A (rows 0..15) in half-groups 0..5, stream B (rows 16..31) in 6..11; a
            // stream's rows are requested again as soon as its last slice has consumed them (half a tile ahead of use)
            if (hs < 6)
                half_slice<XMODE, UP, FUSE>(hs % 6, rawA, validA, head4, d0, tt, nxt, stA0, stA1, seA, SUB, PA, PB, OFF_B, OFF_E);
            else
                half_slice<XMODE, UP, FUSE>(hs % 6, rawB, validB, head4, d0, tt, nxt, stA0 + stB, stA1 + stB, seA + seB, SUB,
                                                    PA, PB, OFF_B, OFF_E);
            __builtin_amdgcn_sched_barrier(0);
            // stream A: own planes re-requested after its last slice (hs 5), its gathers half a tile later (hs 11);
            // stream B: own planes at hs 11, gathers at hs 5 of the next tile -- only one stream's gather registers
            // are alive at a time
            if (hs == 5) {
                half_issue_main<UP>(a, idA, f4, rawA);
                half_issue_gather<XMODE, FUSE>(a, idB, f4, rawB);
                __builtin_amdgcn_sched_barrier(0);
                validB = idB.valid;
                idB = half_ids<XMODE, FUSE>(a, tile + 2 * G, it + 2 < nmine, 16 + hr);
            }
            if (hs == 11) {
                half_issue_main<UP>(a, idB, f4, rawB);
                half_issue_gather<XMODE, FUSE>(a, idA, f4, rawA);
                __builtin_amdgcn_sched_barrier(0);
                validA = idA.valid;
                idA = half_ids<XMODE, FUSE>(a, tile + 3 * G, it + 3 < nmine, hr);
            }
        }
#undef ONE_LD_A
#undef ONE_LD_BT
#undef ONE_LD_TR
#undef ONE_LD_D
        // epilogue: lane = row c; register 4q+i <-> column 8q + 4 half + i of the wave's 32-column tile
        if (is_dx) {
            if (elive) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(a.d_msg + (size_t)erow * a.ld_dmsg + n0 + 8 * q + 4 * half) =
                        make_float4(accd[4 * q], accd[4 * q + 1], accd[4 * q + 2], accd[4 * q + 3]);
            }
        } else {
            const float* e = reinterpret_cast<const float*>(cur + OFF_E) + eoff;
            float4 ex4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) ex4[q] = *reinterpret_cast<const float4*>(e + ((((n0 + 8 * q + 4 * half) >> 2) ^ (c & 15)) << 2));
            if (elive) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(a.d_h + (size_t)erow * a.ld_dh + n0 + 8 * q + 4 * half) =
                        make_float4(accd[4 * q] + ex4[q].x, accd[4 * q + 1] + ex4[q].y, accd[4 * q + 2] + ex4[q].z,
                                    accd[4 * q + 3] + ex4[q].w);
            }
        }
        erow = erow_n; elive = elive_n;
        __syncthreads();
    }
#undef ONE_STAGE
    // ---- one slab per block: [3H][IN+H] weights, then [2][3H] biases
    float* sw = a.slab_w + (size_t)blockIdx.x * (3 * H) * (2 * H);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int jj = (jt0 + j) * 32 + acc_row(reg, half);
                sw[(size_t)jj * (2 * H) + which * H + t * 32 + c] = acc[j][t][reg];
            }
    // bias slabs: column m = lane & 31 of A tile jt0 + j; the two lane halves hold rows 8 half .. 8 half + 7 of every block
    float* sb = a.slab_b + (size_t)blockIdx.x * 6 * H;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float tot = bsum[j] + __shfl_xor(bsum[j], 32);
        const int col = (jt0 + j) * 32 + c;                 // 0..191 in the wave's own gate order
        if (half == 0) {
            if (which == 0) {                               // d_gi = dr | dz | dn ; dr and dz are also the first two of d_gh
                sb[col] = tot;
                if (col < 2 * H) sb[3 * H + col] = tot;
            } else if (col >= 2 * H) {                      // d_gh's n gate: dn * r
                sb[3 * H + col] = tot;
            }
        }
    }
}
#endif  // TMPNN_KEEP_VARIANTS

// ==========================================================================================
// The one-pass backward at TWO waves per SIMD (k_gru_bwd_two): the same LDS images, the same products and slabs as
// k_gru_bwd_one, but a block is eight 256-register waves, so that on every SIMD one wave's LDS reads, staging arithmetic
// and waits run under the other's MFMAs (k_gru_bwd_one, one 512-register wave per SIMD, issues everything itself and its
// parts add up).  What makes 256 registers enough:
//   * waves 0-3 take the W_ih side (d_msg, dW_ih), waves 4-7 the W_hh side (d_h, dW_hh); wave q of a side owns 16 output
//     columns of the data product on v_mfma_f32_16x16x32_bf16 (its W^T slice: 16 x 192 x three pieces = 72 registers,
//     half of the 32-column slice) and three of the side's twelve 32 x 32 tiles of dW (48 registers);
//   * a thread stages ONE row (32 rows x 16 threads), slice by slice between the MFMA groups; every plane is requested
//     again right after the slice that consumed it last, so each load has 2/3 of a tile period or more to land and no
//     second register set holds rows in flight;
//   * operand fragments are read one MFMA group ahead at most.
// The data product's row read of a [32][128] image takes the four 16-byte chunks {4 kq + s} (not {4 s + kq}) for k-step s,
// lane group kq: all lanes of a ds_read_b128 service group then XOR the same chunk bits into the row swizzle and the read
// is conflict-free (the plain assignment is 2-way on this layout); W's k order is permuted to match.
// ==========================================================================================
__device__ __forceinline__ f32x4 mfma16_bf16(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <int C>
__device__ __forceinline__ f32x4 mfma16_c(const uint4 (&a)[3], const uint4 (&b)[3], f32x4 acc) {
    if (C == 0) return mfma16_bf16(a[2], b[0], acc);
    if (C == 1) return mfma16_bf16(a[0], b[2], acc);
    if (C == 2) return mfma16_bf16(a[1], b[1], acc);
    if (C == 3) return mfma16_bf16(a[1], b[0], acc);
    if (C == 4) return mfma16_bf16(a[0], b[1], acc);
    return mfma16_bf16(a[0], b[0], acc);
}
template <int C>
__device__ __forceinline__ f32x16 mfma32_c(const uint4 (&a)[3], const uint4 (&b)[3], f32x16 acc) {
    if (C == 0) return mfma_bf16(a[2], b[0], acc);
    if (C == 1) return mfma_bf16(a[0], b[2], acc);
    if (C == 2) return mfma_bf16(a[1], b[1], acc);
    if (C == 3) return mfma_bf16(a[1], b[0], acc);
    if (C == 4) return mfma_bf16(a[0], b[1], acc);
    return mfma_bf16(a[0], b[0], acc);
}

#define TWO_MARK(i) do { } while (0)
struct TwoRaw { float4 dh, r, z, n, hn, hp, xa, xb, ea, eb; float dy; };
// (the gate planes are read exactly once; requesting them nontemporal was measured to change nothing: 3.87-3.88 vs 3.87-3.90 ms
//  per 6.03 M rows, the L1's pending-request queue is full either way -- switch removed in round 4)
#define TWO_LD4(p) (*reinterpret_cast<const float4*>(p))

#ifndef TWO_SCHED
#define TWO_SCHED 1     // 1: a group's staging slice sits between its operand reads and its MFMAs with no scheduling fence (the
                        // compiler spreads it under the MFMAs: 2.10 -> 2.00 ms per 3 M rows); 0: fenced, slice after the MFMAs
#endif
#ifndef TWO_EXP
#define TWO_EXP 0          // build-time elimination experiments (1: no global requests, 2: no staging, 4: no MFMAs, 16: no epilogue stores)
#endif
// XMODE 2 (round 4, the concat message [h[src] | h[dst]], IN = 2H): the cell's backward as TWO launches over column halves of
// W_ih -- x = h[src[r]] alone, w_ih / d_msg / dW_ih pointing at the half -- the second with HHS = false: nothing of the W_hh
// side leaves the kernel (no d_h, no dW_hh, no bias sums: the first launch has them).  Its W_hh-side waves still run their
// products: skipping them on a wave-uniform branch cost 28-72 bytes of scratch inside the loop and made the launch SLOWER
// than a full one (485 vs 383 us per 0.8 M rows) -- a scratch reload drains every row request in flight.
template <int XMODE, int UP, bool FUSE, bool HHS = true>
__global__ __launch_bounds__(512) void k_gru_bwd_two(GruBwdFusedArgs a, int ntiles) {
    constexpr int exp_ = TWO_EXP;
    constexpr int H = 64;
    constexpr int SUB = 32 * 128;
    constexpr int PA = 2 * SUB, PB = SUB;
    constexpr int OFF_B = 3 * PA, OFF_E = OFF_B + 3 * PB;
    constexpr int BUF = OFF_E + 32 * 64 * 2;       // 80 KiB per buffer (uint16 elements)
    extern __shared__ float lds[];
    uint16_t* const lds16 = reinterpret_cast<uint16_t*>(lds);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int role = wave >> 2, q = wave & 3;                 // role 0: W_ih side, 1: W_hh side
    const int lrole = role;
    // ---- data product (16x16x32): lane (j = tile row within a 16-row half, kq = k group)
    const int j16 = lane & 15, kq = lane >> 4;
    // staging: thread tid takes row tid >> 4, columns 4 (tid & 15) .. + 3 -- written through (wave, kq, j16), which the
    // matrix phase keeps alive anyway (a separate copy of the thread id ends up in scratch, and a scratch reload waits for
    // EVERY request in flight)
    const int srow = 4 * wave + kq, f4 = 4 * j16;
    const int n0 = 16 * q;
    uint4 wq[6][3];
    {
        const float* W = role == 0 ? a.w_ih : a.w_hh;
        const int ldw = role == 0 ? a.ld_wih : H;
#pragma unroll
        for (int s6 = 0; s6 < 6; ++s6) {
            const int ch = s6 < 4 ? 4 * kq + s6 : 16 + 4 * (s6 - 4) + kq;      // 8-column chunk of the 192 gate columns
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = W[(size_t)(8 * ch + i) * ldw + n0 + j16];
            const Split8 sp = split8_arr(v);
            wq[s6][0] = sp.p1; wq[s6][1] = sp.p2; wq[s6][2] = sp.p3;
        }
    }
    const float headl = (UP & 2) ? a.up.w_head[lane] : 0.f;   // w_head[lane]; a thread's four come by ds_bpermute in slice 0
    const int st0 = dui_off(srow, f4);                         // columns 64 + f4: st0 ^ 64
    const int se0 = srow * 64 + (((f4 >> 2) ^ (srow & 15)) << 2);
    // row reads of the data product: rows j16 and 16 + j16 share the swizzle
    const int swzj = dui_swz(j16), rowj = j16 * 128;
    const int hix = lrole == 0 ? 0 : 64;                       // d_h takes dn*r (image columns 192..255) for the n gate
    // ---- weight gradient (32x32x16, transposed reads): A tiles jt0 + {0,1,2} of the side's six, operand tile t
    const int half = lane >> 5, c32 = lane & 31;
    const int jt0 = (q >> 1) * 3, tt = q & 1;
    const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3, tg = (lane >> 4) & 1;
    const int trow = (8 * half + tq) * 128, tsw0 = (tq << 2) | (2 * half);
    int offA[3], offB;                                         // second read of a pair: (off ^ 8) + 4 * 128
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int jj0 = (jt0 + j) * 32;
        const int col = (lrole == 1 && jj0 >= 2 * H) ? jj0 + H : jj0;
        const int ch = ((col & 127) >> 3) + 2 * tg + (tp >> 1);
        offA[j] = (col >> 7) * SUB + trow + ((ch ^ tsw0) << 3) + 4 * (tp & 1);
    }
    {
        const int ch = ((lrole * H + tt * 32) >> 3) + 2 * tg + (tp >> 1);
        offB = OFF_B + trow + ((ch ^ tsw0) << 3) + 4 * (tp & 1);
    }
    f32x16 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    float bsum[3] = {0.f, 0.f, 0.f};

    const int G = gridDim.x;
    const int nmine = (ntiles - (int)blockIdx.x + G - 1) / G;       // >= 1
    TwoRaw raw;
    float d0[4], tv[4];
    // ids: a tile's row id is needed for its own planes (requested one tile ahead of its staging), its endpoints for the
    // gathers (requested half a tile ahead)
    auto row_of = [&](int tile, bool tvld, bool& vld) -> int {
        const int lr = tile * 32 + srow;
        vld = tvld && lr < a.R;
        return vld ? lr : a.R - 1;
    };
    // ---- the six staging slices of one row; what a slice consumes last is requested again right behind it
#define TWO_SLICE(SL, img, vld)                                                                              \
    do {                                                                                                     \
        float o_[4];                                                                                         \
        if ((SL) == 0) {                                                                                     \
            const float dh_[4] = {raw.dh.x, raw.dh.y, raw.dh.z, raw.dh.w}, r_[4] = {raw.r.x, raw.r.y, raw.r.z, raw.r.w}; \
            const float z_[4] = {raw.z.x, raw.z.y, raw.z.z, raw.z.w}, n_[4] = {raw.n.x, raw.n.y, raw.n.z, raw.n.w}; \
            const float hn_[4] = {raw.hn.x, raw.hn.y, raw.hn.z, raw.hn.w};                                   \
            float q_[4];                                                                                     \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                  \
                float d_ = (UP & 1) ? dh_[i] : 0.f;                                                          \
                if (UP & 2) d_ += raw.dy * __shfl(headl, f4 + i);                                                        \
                d0[i] = (vld) ? d_ : 0.f;                                                                    \
                tv[i] = d0[i] * (1.0f - z_[i]) * (1.0f - n_[i] * n_[i]);                                     \
                q_[i] = tv[i] * r_[i];                                                                       \
                o_[i] = q_[i] * hn_[i] * (1.0f - r_[i]);                                                     \
            }                                                                                                \
            half_put((img), st0, PA, o_);                                                                    \
            half_put((img), SUB + (st0 ^ 64), PA, q_);                                                       \
        } else if ((SL) == 1) {                                                                              \
            const float z_[4] = {raw.z.x, raw.z.y, raw.z.z, raw.z.w}, n_[4] = {raw.n.x, raw.n.y, raw.n.z, raw.n.w}; \
            const float hp_[4] = {raw.hp.x, raw.hp.y, raw.hp.z, raw.hp.w};                                   \
            float e_[4];                                                                                     \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                  \
                o_[i] = d0[i] * (hp_[i] - n_[i]) * z_[i] * (1.0f - z_[i]);                                   \
                e_[i] = d0[i] * z_[i];                                                                       \
            }                                                                                                \
            half_put((img), st0 ^ 64, PA, o_);                                                               \
            *reinterpret_cast<float4*>(reinterpret_cast<float*>((img) + OFF_E) + se0) = make_float4(e_[0], e_[1], e_[2], e_[3]); \
        } else if ((SL) == 2) {                                                                              \
            const float hp_[4] = {raw.hp.x, raw.hp.y, raw.hp.z, raw.hp.w};                                   \
            half_put((img) + OFF_B, st0 ^ 64, PB, hp_);                                                      \
        } else if ((SL) == 3) {                                                                              \
            half_put((img), SUB + st0, PA, tv);                                                              \
        } else if ((SL) == 5) {                                                                              \
            const float xa_[4] = {raw.xa.x, raw.xa.y, raw.xa.z, raw.xa.w}, xb_[4] = {raw.xb.x, raw.xb.y, raw.xb.z, raw.xb.w}; \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) o_[i] = XMODE == 1 ? xa_[i] - xb_[i] : xa_[i];     \
            half_put((img) + OFF_B, st0, PB, o_);                                                            \
            if (FUSE) {                                                                                      \
                float4* ep_ = reinterpret_cast<float4*>(reinterpret_cast<float*>((img) + OFF_E) + se0);      \
                float4 e4_ = *ep_;                                                                           \
                e4_.x += raw.ea.x - raw.eb.x; e4_.y += raw.ea.y - raw.eb.y;                                  \
                e4_.z += raw.ea.z - raw.eb.z; e4_.w += raw.ea.w - raw.eb.w;                                  \
                *ep_ = e4_;                                                                                  \
            }                                                                                                \
        }                                                                                                    \
    } while (0)
    // the planes slice SL consumed last, requested for row position lp (orow = a.rows[lp])
#define TWO_ISSUE_MAIN(SL, orow_)                                                                            \
    do {                                                                                                     \
        const size_t gp_ = a.gate_plane;                                                                     \
        const float* g0_ = a.gates + (size_t)(orow_) * H + f4;                                               \
        if ((SL) == 0) {                                                                                     \
            if (UP & 1) raw.dh = *reinterpret_cast<const float4*>(a.up.d_hout + (size_t)(orow_) * a.up.ld_dhout + f4); \
            if (UP & 2) raw.dy = a.up.dy[(orow_)];                                                           \
            raw.hn = TWO_LD4(g0_ + 3 * gp_);                                                                 \
            raw.r = TWO_LD4(g0_);                                                                            \
        } else if ((SL) == 1) {                                                                              \
            raw.n = TWO_LD4(g0_ + 2 * gp_);                                                                  \
            raw.z = TWO_LD4(g0_ + gp_);                                                                      \
        } else if ((SL) == 2) {                                                                              \
            raw.hp = *reinterpret_cast<const float4*>(a.h + (size_t)(orow_) * a.ld_h + f4);                  \
        }                                                                                                    \
    } while (0)
    // a row's gathers (its endpoints' rows / its message row), requested half a tile ahead of slice 5; the ids themselves
    // (gs_, gd_) were fetched a tile earlier: a load chain inside the phase would drain every request in flight
#define TWO_ISSUE_GATHER(gs_, gd_)                                                                           \
    do {                                                                                                     \
        if (XMODE == 0) raw.xa = *reinterpret_cast<const float4*>(a.msg + (size_t)(gs_) * a.ld_msg + f4);    \
        if (XMODE != 0) {                                                                                    \
            raw.xa = *reinterpret_cast<const float4*>(a.h + (size_t)(gs_) * a.ld_h + f4);                    \
            if (XMODE == 1) raw.xb = *reinterpret_cast<const float4*>(a.h + (size_t)(gd_) * a.ld_h + f4);    \
            if (FUSE) {                                                                                      \
                raw.ea = *reinterpret_cast<const float4*>(a.add_msg + (size_t)(gs_) * a.ld_add + f4);        \
                raw.eb = *reinterpret_cast<const float4*>(a.add_msg + (size_t)(gd_) * a.ld_add + f4);        \
            }                                                                                                \
        }                                                                                                    \
    } while (0)
    // XMODE 0: gs = the message row (FUSE with XMODE 0 is not offered: the node cell has no fused adjoint)
#define TWO_GATHER_IDS(lp_, gs_, gd_)                                                                        \
    do {                                                                                                     \
        if (XMODE == 0) { (gs_) = a.msg_compact ? (lp_) : a.rows[(lp_)]; (gd_) = 0; }                        \
        else { (gs_) = a.src[(lp_)]; (gd_) = a.dst[(lp_)]; }                                                 \
    } while (0)

    // ---- prologue: tile 0 staged into buffer 0, tile 1's planes requested
    bool valid_cur, valid_n;
    int gs_cur, gd_cur;                           // endpoints (message row) of the tile being staged, for its gathers
    int orow_n;                                   // row id of the tile after that (for its planes)
    {
        bool v0, v1;
        const int lp0 = row_of(blockIdx.x, true, v0);
        const int o0 = a.rows[lp0];
        TWO_GATHER_IDS(lp0, gs_cur, gd_cur);
        TWO_ISSUE_MAIN(0, o0); TWO_ISSUE_MAIN(1, o0); TWO_ISSUE_MAIN(2, o0); TWO_ISSUE_GATHER(gs_cur, gd_cur);
        const int lp1 = row_of(blockIdx.x + G, 1 < nmine, v1);
        const int o1 = a.rows[lp1];
        TWO_SLICE(0, lds16, v0); TWO_ISSUE_MAIN(0, o1);
        TWO_SLICE(1, lds16, v0); TWO_ISSUE_MAIN(1, o1);
        TWO_SLICE(2, lds16, v0); TWO_ISSUE_MAIN(2, o1);
        TWO_SLICE(3, lds16, v0);
        TWO_SLICE(5, lds16, v0);
        valid_cur = v1;
        TWO_GATHER_IDS(lp1, gs_cur, gd_cur);
        const int lp2 = row_of(blockIdx.x + 2 * G, 2 < nmine, valid_n);
        orow_n = a.rows[lp2];
    }
    __syncthreads();

    // one group's share of the staging: slice s6 of the next tile, then the requests for what it freed.  (Staggering the
    // SIMD partners -- the W_hh side staging before its MFMA group, or waves 4-7 / odd waves started a few hundred cycles
    // late every tile -- was measured and changed nothing)
#define TWO_STAGE(ROLE_)                                                                                     \
    do {                                                                                                     \
        if (!(exp_ & 2)) TWO_SLICE(s6, nxt, valid_cur);                                                      \
        if (!(exp_ & 1)) {                                                                                   \
            TWO_ISSUE_MAIN(s6, orow_n);                                                                      \
            /* the gathers two groups ahead of slice 5 (det rows: mostly L2 hits); held over the whole phase they */ \
            /* push a dozen registers into scratch, and a scratch reload waits for every request in flight        */ \
            if (s6 == 3) TWO_ISSUE_GATHER(gs_cur, gd_cur);                                                   \
        }                                                                                                    \
        if (TWO_SCHED == 0) __builtin_amdgcn_sched_barrier(0);                                               \
    } while (0)
    for (int it = 0; it < nmine; ++it) {
        const int tile = blockIdx.x + it * G;
        uint16_t* const cur = lds16 + (it & 1) * BUF;
        uint16_t* const nxt = lds16 + ((it & 1) ^ 1) * BUF;
        // epilogue rows of this tile (lane -> rows j16 and 16 + j16), requested FIRST in the phase: at the epilogue the wait
        // then leaves every later request of the phase (the next tiles' planes) in flight
        const int er0 = a.rows[min(tile * 32 + j16, a.R - 1)], er1 = a.rows[min(tile * 32 + 16 + j16, a.R - 1)];
        const bool el0 = tile * 32 + j16 < a.R, el1 = tile * 32 + 16 + j16 < a.R;
        f32x4 accd[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) { accd[0][i] = 0.f; accd[1][i] = 0.f; }
#pragma unroll
        for (int s6 = 0; s6 < 6; ++s6) {
            const int kb = s6 / 3, j = s6 % 3;
            uint4 bd[3], aw[3], bt[3];
            const uint16_t* pd;
            {
                const int chunk = s6 < 4 ? 4 * kq + s6 : 4 * (s6 - 4) + kq;
                int inrow = (chunk ^ swzj) << 3;
                if (s6 >= 4) inrow ^= hix;
                pd = cur + (s6 >= 4 ? SUB : 0) + rowj + inrow;
            }
            // the dW group first: its operands are dead once its six MFMAs have issued, and the row operand of the data
            // product arrives under them (one operand set alive at a time)
            {
                const uint16_t* p0 = cur + kb * 2048 + offB;
                const uint16_t* p1 = cur + kb * 2048 + (offB ^ 8) + 4 * 128;
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) {
                    const uint2 u0 = lds_read_tr(p0 + pc * PB), u1 = lds_read_tr(p1 + pc * PB);
                    bt[pc] = make_uint4(u0.x, u0.y, u1.x, u1.y);
                }
            }
            {
                const uint16_t* p0 = cur + kb * 2048 + offA[j];
                const uint16_t* p1 = cur + kb * 2048 + (offA[j] ^ 8) + 4 * 128;
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) {
                    const uint2 u0 = lds_read_tr(p0 + pc * PA), u1 = lds_read_tr(p1 + pc * PA);
                    aw[pc] = make_uint4(u0.x, u0.y, u1.x, u1.y);
                }
            }
            TWO_MARK(0);                                        // dW operand reads (transposing LDS reads) issued and back
            if (TWO_SCHED >= 1) TWO_STAGE(0);
            TWO_MARK(1);                                        // staging slice of the next tile (waits for its rows) + re-requests
            if (!(exp_ & 4)) {
            acc[j] = mfma32_c<0>(aw, bt, acc[j]); acc[j] = mfma32_c<1>(aw, bt, acc[j]);
            acc[j] = mfma32_c<2>(aw, bt, acc[j]); acc[j] = mfma32_c<3>(aw, bt, acc[j]);
            acc[j] = mfma32_c<4>(aw, bt, acc[j]); acc[j] = mfma32_c<5>(aw, bt, acc[j]);
            } else { acc[j][0] += __uint_as_float(aw[0].x ^ bt[0].x ^ aw[1].y ^ bt[1].y ^ aw[2].z ^ bt[2].z); }
            if (HHS && kb == tt && !(exp_ & 8)) {               // bias gradient: column sums from the A operands (the two waves
                                                                // that read the same A tiles take one 16-row block each)
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) {
                    const uint4 v = aw[pc];
                    bsum[j] = dot2_ones(v.x, bsum[j]); bsum[j] = dot2_ones(v.y, bsum[j]);
                    bsum[j] = dot2_ones(v.z, bsum[j]); bsum[j] = dot2_ones(v.w, bsum[j]);
                }
            }
            if (TWO_SCHED == 0) __builtin_amdgcn_sched_barrier(0);
            TWO_MARK(2);                                        // six 32 x 32 x 16 MFMAs of dW + the bias dot products
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) bd[pc] = *reinterpret_cast<const uint4*>(pd + pc * PA);
            if (!(exp_ & 4)) {
            accd[0] = mfma16_c<0>(wq[s6], bd, accd[0]); accd[0] = mfma16_c<1>(wq[s6], bd, accd[0]);
            accd[0] = mfma16_c<2>(wq[s6], bd, accd[0]); accd[0] = mfma16_c<3>(wq[s6], bd, accd[0]);
            accd[0] = mfma16_c<4>(wq[s6], bd, accd[0]); accd[0] = mfma16_c<5>(wq[s6], bd, accd[0]);
            } else { accd[0][0] += __uint_as_float(bd[0].x ^ bd[1].y ^ bd[2].z); }
            if (TWO_SCHED == 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) bd[pc] = *reinterpret_cast<const uint4*>(pd + pc * PA + 16 * 128);
            if (!(exp_ & 4)) {
            accd[1] = mfma16_c<0>(wq[s6], bd, accd[1]); accd[1] = mfma16_c<1>(wq[s6], bd, accd[1]);
            accd[1] = mfma16_c<2>(wq[s6], bd, accd[1]); accd[1] = mfma16_c<3>(wq[s6], bd, accd[1]);
            accd[1] = mfma16_c<4>(wq[s6], bd, accd[1]); accd[1] = mfma16_c<5>(wq[s6], bd, accd[1]);
            } else { accd[1][0] += __uint_as_float(bd[0].x ^ bd[1].y ^ bd[2].z); }
            if (TWO_SCHED == 0) __builtin_amdgcn_sched_barrier(0);
            // ---- staging slice s6 of the next tile; what it freed is requested for the tile after that
            if (TWO_SCHED == 0) TWO_STAGE(0);
            __builtin_amdgcn_sched_barrier(0);
            TWO_MARK(3);                                        // row operand reads + twelve 16 x 16 x 32 MFMAs of the data product
        }
        // the staged tile's successor becomes the tile being staged; its successor's row id is fetched
        {
            bool vnn;
            const int lp2 = row_of(tile + 2 * G, it + 2 < nmine, vnn);
            TWO_GATHER_IDS(lp2, gs_cur, gd_cur);
            valid_cur = valid_n;
            const int lp3 = row_of(tile + 3 * G, it + 3 < nmine, valid_n);
            orow_n = a.rows[lp3];
            (void)vnn;
        }
        // ---- epilogue: lane (j16, kq) holds columns n0 + 4 kq .. + 3 of rows j16 and 16 + j16
        int cofs = n0 + 4 * kq;
        asm volatile("" : "+v"(cofs));             // (kept as ONE register: hoisted, the two 64-bit column bases are spilled)
        if (exp_ & 16) {                           // (timing experiment: no epilogue stores)
            if (accd[0][0] + accd[1][1] + (float)er0 + (float)er1 == 123.456f) a.d_msg[cofs] = 1.f;
        } else if (role == 0) {
            if (el0) *reinterpret_cast<float4*>(a.d_msg + ((size_t)er0 * a.ld_dmsg + cofs)) =
                         make_float4(accd[0][0], accd[0][1], accd[0][2], accd[0][3]);
            if (el1) *reinterpret_cast<float4*>(a.d_msg + ((size_t)er1 * a.ld_dmsg + cofs)) =
                         make_float4(accd[1][0], accd[1][1], accd[1][2], accd[1][3]);
        } else if (HHS) {
            const float* e = reinterpret_cast<const float*>(cur + OFF_E);
            const int cq = cofs >> 2;
            const float4 x0 = *reinterpret_cast<const float4*>(e + j16 * 64 + ((cq ^ j16) << 2));
            const float4 x1 = *reinterpret_cast<const float4*>(e + (16 + j16) * 64 + ((cq ^ j16) << 2));
            if (el0) *reinterpret_cast<float4*>(a.d_h + ((size_t)er0 * a.ld_dh + cofs)) =
                         make_float4(accd[0][0] + x0.x, accd[0][1] + x0.y, accd[0][2] + x0.z, accd[0][3] + x0.w);
            if (el1) *reinterpret_cast<float4*>(a.d_h + ((size_t)er1 * a.ld_dh + cofs)) =
                         make_float4(accd[1][0] + x1.x, accd[1][1] + x1.y, accd[1][2] + x1.z, accd[1][3] + x1.w);
        }
        TWO_MARK(4);                                            // next ids + epilogue (row ids wait, stores)
        __syncthreads();
        TWO_MARK(5);                                            // barrier
    }
#undef TWO_STAGE
#undef TWO_GATHER_IDS
#undef TWO_ISSUE_GATHER
#undef TWO_ISSUE_MAIN
#undef TWO_SLICE
    // ---- one slab per block: [3H][IN+H] weights, then [2][3H] biases
    float* sw = a.slab_w + (size_t)blockIdx.x * (3 * H) * (2 * H);
    if (HHS || role == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int jj = (jt0 + j) * 32 + acc_row(reg, half);
                sw[(size_t)jj * (2 * H) + role * H + tt * 32 + c32] = acc[j][reg];
            }
    }
    // bias slabs: wave (tt = 0) + wave (tt = 1) of the same A tiles, in that order, through the now idle LDS
    {
        float* red = lds;                                      // [8 waves][96]
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float tot = bsum[j] + __shfl_xor(bsum[j], 32);
            if (half == 0) red[wave * 96 + j * 32 + c32] = tot;
        }
        __syncthreads();
        if (HHS && tt == 0 && half == 0) {
            float* sb = a.slab_b + (size_t)blockIdx.x * 6 * H;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                sb[role * 3 * H + (jt0 + j) * 32 + c32] = red[wave * 96 + j * 32 + c32] + red[(wave + 1) * 96 + j * 32 + c32];
        }
    }
}

// ==========================================================================================
// The one-pass backward of rows whose incoming state is ZERO (k_gru_bwd_zs: H = IN = 64, diff message): a forward call's new
// edge rows (functional.py mp_forward zero-fills them).  With h_prev = 0: dW_hh gets nothing, ghn = b_hn exactly (the fourth
// gate plane is not read), dz = -d0 n z (1-z), and d_h is not formed -- the rows' d_h lies at or behind the call's first new
// row, which no one reads (d_h_in is d_hcat[:N_old]; the row-F adjoint lands in d_h too and is dropped with it).  What is left
// is the W_ih side of k_gru_bwd_two, spread over all eight waves of the block:
//   * wave (role, q): data product d_msg = d_gi W_ih for the 16 columns 16 q .. of the tile's rows 16 role .. + 15 (the same
//     W^T slice in registers as k_gru_bwd_two), and dW_ih tiles jt0 + {0,1,2} / tt for the K-step (row half) `role` only; the
//     role-1 partials go to the slab's (unused) W_hh columns and the reduction adds the two halves (k_gru_reduce_w_zs);
//   * the bias gradients are f32 column sums taken in the staging: a thread keeps the four sums of its row position and
//     columns (dr, dz, dn, dn r; db_ih = [dr|dz|dn], db_hh = [dr|dz|dn r]) and the block folds its 32 row positions in order
//     at the end;
//   * LDS: the images of k_gru_bwd_two at the same offsets without the E image (72 KiB per buffer; the dn r and h halves
//     stay unwritten).
// Every wave runs the same straight-line code: role only moves addresses (no role branch, no scratch in the loop).
// ==========================================================================================
//
// RC (gate_plane == 0, struct tmpnn_zs_gate_src): the forward saved no gate planes for these rows and the staging forms r, z, n
// itself from the projected det rows P the forward read -- six 16-byte gathers per row and thread (L2 hits: a 32-row tile touches
// about 11 det rows) instead of three streamed plane loads, and the forward's own expressions, so the planes it would have
// stored are reproduced bit for bit (zs_gate / zs_gate_n below mirror k_gru_fwd_split_tiled<., ., true>'s epilogue; the sums
// b_ir + b_hr, b_iz + b_hz and b_in sit in 768 B of LDS behind the two image sets, formed as the forward's sBias).  The kernel
// is at its register limit (256), so the requests are staggered over the six groups of an iteration and never hold more
// registers than the plane loads did: per iteration  0: slices 0 + 1, request dh | 1: slice 3, request x | 2: request the P_r
// pair | 3: slice 5, request the P_z pair | 4: request the P_n pair, r <- P_r pair | 5: z <- P_z pair, n <- P_n pair and r  (the
// gate arithmetic sits in the groups without dW products).  The det positions ride with orow_n, two tiles ahead.
// The compiler's report: 256 registers for every UP, no scratch access inside the tile loop for UP = 1, 3; UP = 2 reloads one spilled
// register (srow) per tile in the index block at the end of the iteration, where only the dh request is outstanding.
// The gate source rides in fields of GruBwdFusedArgs this kernel does not otherwise read (ZsGateSrc names them): msg / ld_msg
// = P and its row stride (as in the forward's arguments), add_src / add_dst = the det positions, add_msg = b_ih; b_hh = b_hn - 2H
// (a kernel parameter of its own would change the signature of the plane-reading instantiation too, which keeps its ISA).
struct ZsGateSrc { const float* proj; int ld_proj; const int32_t* src_pos; const int32_t* dst_pos; const float* b_ih; const float* b_hh; };

// a zero-state row's r or z from its two projected rows: the accumulator of the forward is +0 there and is added first
__device__ __forceinline__ float zs_gate(float ps, float pd, float bsum) { return sigmoidf_((0.0f + (ps - pd)) + bsum); }
__device__ __forceinline__ float zs_gate_n(float ps, float pd, float b_in, float r, float b_hn) {
    return tanhf_(gru_n_preact((ps - pd) + b_in, r, 0.0f + b_hn));
}

template <int UP, bool RC = false>
__global__ __launch_bounds__(512) void k_gru_bwd_zs(GruBwdFusedArgs a, const float* __restrict__ b_hn, int ntiles) {
    constexpr int H = 64;
    constexpr int SUB = 32 * 128;
    constexpr int PA = 2 * SUB, PB = SUB;
    constexpr int OFF_B = 3 * PA;
    constexpr int BUF = OFF_B + 3 * PB;            // 72 KiB per buffer (uint16 elements)
    extern __shared__ float lds[];
    uint16_t* const lds16 = reinterpret_cast<uint16_t*>(lds);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int role = wave >> 2, q = wave & 3;                 // role: row half of the data product, K-step of dW
    const int j16 = lane & 15, kq = lane >> 4;
    const int srow = 4 * wave + kq, f4 = 4 * j16;
    const int n0 = 16 * q;
    uint4 wq[6][3];
#pragma unroll
    for (int s6 = 0; s6 < 6; ++s6) {
        const int ch = s6 < 4 ? 4 * kq + s6 : 16 + 4 * (s6 - 4) + kq;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = a.w_ih[(size_t)(8 * ch + i) * a.ld_wih + n0 + j16];
        const Split8 sp = split8_arr(v);
        wq[s6][0] = sp.p1; wq[s6][1] = sp.p2; wq[s6][2] = sp.p3;
    }
    const float headl = (UP & 2) ? a.up.w_head[lane] : 0.f;
    const float4 bhn = *reinterpret_cast<const float4*>(b_hn + f4);
    const int st0 = dui_off(srow, f4);
    const int swzj = dui_swz(j16), rowj = (16 * role + j16) * 128;
    const int half = lane >> 5, c32 = lane & 31;
    const int jt0 = (q >> 1) * 3, tt = q & 1;
    const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3, tg = (lane >> 4) & 1;
    const int trow = (8 * half + tq) * 128, tsw0 = (tq << 2) | (2 * half);
    const int kofs = role * 2048;                              // K-step `role`: rows 16 role .. + 15
    int offA[3], offB;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int col = (jt0 + j) * 32;
        const int ch = ((col & 127) >> 3) + 2 * tg + (tp >> 1);
        offA[j] = kofs + (col >> 7) * SUB + trow + ((ch ^ tsw0) << 3) + 4 * (tp & 1);
    }
    {
        const int ch = ((tt * 32) >> 3) + 2 * tg + (tp >> 1);
        offB = kofs + OFF_B + trow + ((ch ^ tsw0) << 3) + 4 * (tp & 1);
    }
    f32x16 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    float bs_r[4] = {0.f, 0.f, 0.f, 0.f}, bs_z[4] = {0.f, 0.f, 0.f, 0.f};
    float bs_n[4] = {0.f, 0.f, 0.f, 0.f}, bs_nr[4] = {0.f, 0.f, 0.f, 0.f};

    const int G = gridDim.x;
    const int nmine = (ntiles - (int)blockIdx.x + G - 1) / G;       // >= 1
    struct { float4 dh, r, z, n, xa, xb; float dy; } raw;
    float d0[4], tv[4];
    // RC: r, z, n of raw are computed from the pairs of projected-row quarters in rp; the bias sums [b_ir + b_hr | b_iz + b_hz | b_in]
    // lie behind the two image sets (BUF floats)
    struct { float4 pa, pb, qa, qb, na, nb; } rp;
    const ZsGateSrc gsrc{a.msg, a.ld_msg, a.add_src, a.add_dst, a.add_msg, b_hn - 2 * H};
    float* const sgb = lds + BUF;
    if constexpr (RC) {
        if (tid < 3 * H) sgb[tid] = tid < 2 * H ? gsrc.b_ih[tid] + gsrc.b_hh[tid] : gsrc.b_ih[tid];
        __syncthreads();
    }
    auto row_of = [&](int tile, bool tvld, bool& vld) -> int {
        const int lr = tile * 32 + srow;
        vld = tvld && lr < a.R;
        return vld ? lr : a.R - 1;
    };
    // staging of one row: slice 0 dr (+ the r, n, n r sums), 1 dz, 3 dn, 5 x; rows past R stage zeros (d0 = 0)
#define ZS_SLICE(SL, img, vld)                                                                               \
    do {                                                                                                     \
        float o_[4];                                                                                         \
        if ((SL) == 0) {                                                                                     \
            const float dh_[4] = {raw.dh.x, raw.dh.y, raw.dh.z, raw.dh.w}, r_[4] = {raw.r.x, raw.r.y, raw.r.z, raw.r.w}; \
            const float z_[4] = {raw.z.x, raw.z.y, raw.z.z, raw.z.w}, n_[4] = {raw.n.x, raw.n.y, raw.n.z, raw.n.w}; \
            const float hn_[4] = {bhn.x, bhn.y, bhn.z, bhn.w};                                               \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                  \
                float d_ = (UP & 1) ? dh_[i] : 0.f;                                                          \
                if (UP & 2) d_ += raw.dy * __shfl(headl, f4 + i);                                            \
                d0[i] = (vld) ? d_ : 0.f;                                                                    \
                tv[i] = d0[i] * (1.0f - z_[i]) * (1.0f - n_[i] * n_[i]);                                     \
                const float q_ = tv[i] * r_[i];                                                              \
                o_[i] = q_ * hn_[i] * (1.0f - r_[i]);                                                        \
                bs_r[i] += o_[i]; bs_n[i] += tv[i]; bs_nr[i] += q_;                                          \
            }                                                                                                \
            half_put((img), st0, PA, o_);                                                                    \
        } else if ((SL) == 1) {                                                                              \
            const float z_[4] = {raw.z.x, raw.z.y, raw.z.z, raw.z.w}, n_[4] = {raw.n.x, raw.n.y, raw.n.z, raw.n.w}; \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                  \
                o_[i] = d0[i] * (0.0f - n_[i]) * z_[i] * (1.0f - z_[i]);                                     \
                bs_z[i] += o_[i];                                                                            \
            }                                                                                                \
            half_put((img), st0 ^ 64, PA, o_);                                                               \
        } else if ((SL) == 3) {                                                                              \
            half_put((img), SUB + st0, PA, tv);                                                              \
        } else if ((SL) == 5) {                                                                              \
            const float xa_[4] = {raw.xa.x, raw.xa.y, raw.xa.z, raw.xa.w}, xb_[4] = {raw.xb.x, raw.xb.y, raw.xb.z, raw.xb.w}; \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) o_[i] = xa_[i] - xb_[i];                           \
            half_put((img) + OFF_B, st0, PB, o_);                                                            \
        }                                                                                                    \
    } while (0)
#define ZS_ISSUE_MAIN(SL, orow_)                                                                             \
    do {                                                                                                     \
        const size_t gp_ = a.gate_plane;                                                                     \
        const float* g0_ = a.gates + (size_t)(orow_) * H + f4;                                               \
        if ((SL) == 0) {                                                                                     \
            if (UP & 1) raw.dh = *reinterpret_cast<const float4*>(a.up.d_hout + (size_t)(orow_) * a.up.ld_dhout + f4); \
            if (UP & 2) raw.dy = a.up.dy[(orow_)];                                                           \
            raw.r = TWO_LD4(g0_);                                                                            \
        } else if ((SL) == 1) {                                                                              \
            raw.n = TWO_LD4(g0_ + 2 * gp_);                                                                  \
            raw.z = TWO_LD4(g0_ + gp_);                                                                      \
        }                                                                                                    \
    } while (0)
#define ZS_ISSUE_GATHER(gs_, gd_)                                                                            \
    do {                                                                                                     \
        raw.xa = *reinterpret_cast<const float4*>(a.h + (size_t)(gs_) * a.ld_h + f4);                        \
        raw.xb = *reinterpret_cast<const float4*>(a.h + (size_t)(gd_) * a.ld_h + f4);                        \
    } while (0)

    // RC: the three pairs of projected-row quarters of one row (det positions sp_, dp_) and the gates formed from them
#define ZS_ISSUE_P(G3, A_, B_, sp_, dp_)                                                                     \
    do {                                                                                                     \
        rp.A_ = *reinterpret_cast<const float4*>(gsrc.proj + (size_t)(sp_) * gsrc.ld_proj + (G3) * H + f4); \
        rp.B_ = *reinterpret_cast<const float4*>(gsrc.proj + (size_t)(dp_) * gsrc.ld_proj + (G3) * H + f4); \
    } while (0)
#define ZS_GATE(G3, A_, B_, OUT_)                                                                            \
    do {                                                                                                     \
        const float4 b_ = *reinterpret_cast<const float4*>(sgb + (G3) * H + f4);                             \
        raw.OUT_ = make_float4(zs_gate(rp.A_.x, rp.B_.x, b_.x), zs_gate(rp.A_.y, rp.B_.y, b_.y),             \
                               zs_gate(rp.A_.z, rp.B_.z, b_.z), zs_gate(rp.A_.w, rp.B_.w, b_.w));            \
    } while (0)
#define ZS_GATE_N()                                                                                          \
    do {                                                                                                     \
        const float4 b_ = *reinterpret_cast<const float4*>(sgb + 2 * H + f4);                                \
        raw.n = make_float4(zs_gate_n(rp.na.x, rp.nb.x, b_.x, raw.r.x, bhn.x),                               \
                            zs_gate_n(rp.na.y, rp.nb.y, b_.y, raw.r.y, bhn.y),                               \
                            zs_gate_n(rp.na.z, rp.nb.z, b_.z, raw.r.z, bhn.z),                               \
                            zs_gate_n(rp.na.w, rp.nb.w, b_.w, raw.r.w, bhn.w));                              \
    } while (0)
#define ZS_ISSUE_DH(orow_)                                                                                   \
    do {                                                                                                     \
        if (UP & 1) raw.dh = *reinterpret_cast<const float4*>(a.up.d_hout + (size_t)(orow_) * a.up.ld_dhout + f4); \
        if (UP & 2) raw.dy = a.up.dy[(orow_)];                                                               \
    } while (0)

    // ---- prologue: tile 0 staged into buffer 0, tile 1's planes requested (as k_gru_bwd_two)
    bool valid_cur, valid_n;
    int gs_cur, gd_cur;
    int orow_n;
    int sp_n = 0, dp_n = 0;                                     // RC: det positions of the rows of orow_n's tile
    if constexpr (RC) {
        bool v0, v1;
        const int lp0 = row_of(blockIdx.x, true, v0);
        const int o0 = a.rows[lp0];
        gs_cur = a.src[lp0]; gd_cur = a.dst[lp0];
        const int sp0 = gsrc.src_pos[lp0], dp0 = gsrc.dst_pos[lp0];
        ZS_ISSUE_DH(o0); ZS_ISSUE_GATHER(gs_cur, gd_cur);
        ZS_ISSUE_P(0, pa, pb, sp0, dp0); ZS_ISSUE_P(1, qa, qb, sp0, dp0); ZS_ISSUE_P(2, na, nb, sp0, dp0);
        const int lp1 = row_of(blockIdx.x + G, 1 < nmine, v1);
        const int o1 = a.rows[lp1];
        const int sp1 = gsrc.src_pos[lp1], dp1 = gsrc.dst_pos[lp1];
        ZS_GATE(0, pa, pb, r); ZS_GATE(1, qa, qb, z); ZS_GATE_N();
        ZS_SLICE(0, lds16, v0); ZS_SLICE(1, lds16, v0); ZS_SLICE(3, lds16, v0); ZS_SLICE(5, lds16, v0);
        ZS_ISSUE_DH(o1);
        ZS_ISSUE_P(0, pa, pb, sp1, dp1); ZS_GATE(0, pa, pb, r);
        ZS_ISSUE_P(1, qa, qb, sp1, dp1); ZS_GATE(1, qa, qb, z);
        ZS_ISSUE_P(2, na, nb, sp1, dp1); ZS_GATE_N();
        valid_cur = v1;
        gs_cur = a.src[lp1]; gd_cur = a.dst[lp1];
        const int lp2 = row_of(blockIdx.x + 2 * G, 2 < nmine, valid_n);
        orow_n = a.rows[lp2];
        sp_n = gsrc.src_pos[lp2]; dp_n = gsrc.dst_pos[lp2];
    } else {
        bool v0, v1;
        const int lp0 = row_of(blockIdx.x, true, v0);
        const int o0 = a.rows[lp0];
        gs_cur = a.src[lp0]; gd_cur = a.dst[lp0];
        ZS_ISSUE_MAIN(0, o0); ZS_ISSUE_MAIN(1, o0); ZS_ISSUE_GATHER(gs_cur, gd_cur);
        const int lp1 = row_of(blockIdx.x + G, 1 < nmine, v1);
        const int o1 = a.rows[lp1];
        ZS_SLICE(0, lds16, v0); ZS_ISSUE_MAIN(0, o1);
        ZS_SLICE(1, lds16, v0); ZS_ISSUE_MAIN(1, o1);
        ZS_SLICE(3, lds16, v0);
        ZS_SLICE(5, lds16, v0);
        valid_cur = v1;
        gs_cur = a.src[lp1]; gd_cur = a.dst[lp1];
        const int lp2 = row_of(blockIdx.x + 2 * G, 2 < nmine, valid_n);
        orow_n = a.rows[lp2];
    }
    __syncthreads();

    for (int it = 0; it < nmine; ++it) {
        const int tile = blockIdx.x + it * G;
        uint16_t* const cur = lds16 + (it & 1) * BUF;
        uint16_t* const nxt = lds16 + ((it & 1) ^ 1) * BUF;
        const int er = a.rows[min(tile * 32 + 16 * role + j16, a.R - 1)];
        const bool el = tile * 32 + 16 * role + j16 < a.R;
        f32x4 accd;
#pragma unroll
        for (int i = 0; i < 4; ++i) accd[i] = 0.f;
#pragma unroll
        for (int s6 = 0; s6 < 6; ++s6) {
            uint4 bd[3];
            const uint16_t* pd;
            {
                const int chunk = s6 < 4 ? 4 * kq + s6 : 4 * (s6 - 4) + kq;
                pd = cur + (s6 >= 4 ? SUB : 0) + rowj + ((chunk ^ swzj) << 3);
            }
            if (s6 < 3) {                                       // dW_ih tile jt0 + s6, K-step `role`
                uint4 aw[3], bt[3];
                {       // (the x operand is read again for each dW tile: held over the three groups it costs a spill)
                    const uint16_t* p0 = cur + offB;
                    const uint16_t* p1 = cur + (offB ^ 8) + 4 * 128;
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc) {
                        const uint2 u0 = lds_read_tr(p0 + pc * PB), u1 = lds_read_tr(p1 + pc * PB);
                        bt[pc] = make_uint4(u0.x, u0.y, u1.x, u1.y);
                    }
                }
                const uint16_t* p0 = cur + offA[s6];
                const uint16_t* p1 = cur + (offA[s6] ^ 8) + 4 * 128;
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) {
                    const uint2 u0 = lds_read_tr(p0 + pc * PA), u1 = lds_read_tr(p1 + pc * PA);
                    aw[pc] = make_uint4(u0.x, u0.y, u1.x, u1.y);
                }
                if constexpr (RC) {
                    if (s6 == 0) {
                        ZS_SLICE(0, nxt, valid_cur); ZS_SLICE(1, nxt, valid_cur);
                        ZS_ISSUE_DH(orow_n);
                    } else if (s6 == 1) {
                        ZS_SLICE(3, nxt, valid_cur);
                        ZS_ISSUE_GATHER(gs_cur, gd_cur);
                    } else {
                        ZS_ISSUE_P(0, pa, pb, sp_n, dp_n);
                    }
                } else {
                    ZS_SLICE(s6, nxt, valid_cur);
                    ZS_ISSUE_MAIN(s6, orow_n);
                }
                acc[s6] = mfma32_c<0>(aw, bt, acc[s6]); acc[s6] = mfma32_c<1>(aw, bt, acc[s6]);
                acc[s6] = mfma32_c<2>(aw, bt, acc[s6]); acc[s6] = mfma32_c<3>(aw, bt, acc[s6]);
                acc[s6] = mfma32_c<4>(aw, bt, acc[s6]); acc[s6] = mfma32_c<5>(aw, bt, acc[s6]);
            } else if constexpr (RC) {
                if (s6 == 3) {
                    ZS_SLICE(5, nxt, valid_cur);
                    ZS_ISSUE_P(1, qa, qb, sp_n, dp_n);
                } else if (s6 == 4) {
                    ZS_ISSUE_P(2, na, nb, sp_n, dp_n);
                    ZS_GATE(0, pa, pb, r);
                } else {
                    ZS_GATE(1, qa, qb, z);
                    ZS_GATE_N();
                }
            } else {
                ZS_SLICE(s6, nxt, valid_cur);
                if (s6 == 3) ZS_ISSUE_GATHER(gs_cur, gd_cur);
            }
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) bd[pc] = *reinterpret_cast<const uint4*>(pd + pc * PA);
            accd = mfma16_c<0>(wq[s6], bd, accd); accd = mfma16_c<1>(wq[s6], bd, accd);
            accd = mfma16_c<2>(wq[s6], bd, accd); accd = mfma16_c<3>(wq[s6], bd, accd);
            accd = mfma16_c<4>(wq[s6], bd, accd); accd = mfma16_c<5>(wq[s6], bd, accd);
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            bool vnn;
            const int lp2 = row_of(tile + 2 * G, it + 2 < nmine, vnn);
            gs_cur = a.src[lp2]; gd_cur = a.dst[lp2];
            valid_cur = valid_n;
            const int lp3 = row_of(tile + 3 * G, it + 3 < nmine, valid_n);
            orow_n = a.rows[lp3];
            if constexpr (RC) { sp_n = gsrc.src_pos[lp3]; dp_n = gsrc.dst_pos[lp3]; }
            (void)vnn;
        }
        // ---- epilogue: lane (j16, kq) holds columns n0 + 4 kq .. + 3 of row 16 role + j16
        int cofs = n0 + 4 * kq;
        asm volatile("" : "+v"(cofs));
        if (el) *reinterpret_cast<float4*>(a.d_msg + ((size_t)er * a.ld_dmsg + cofs)) =
                    make_float4(accd[0], accd[1], accd[2], accd[3]);
        __syncthreads();
    }
#undef ZS_ISSUE_DH
#undef ZS_GATE_N
#undef ZS_GATE
#undef ZS_ISSUE_P
#undef ZS_ISSUE_GATHER
#undef ZS_ISSUE_MAIN
#undef ZS_SLICE
    // ---- one slab per block: [3H][2H] (columns 0..H-1: K-step 0 of dW_ih, H..2H-1: K-step 1), then [2][3H] biases
    float* sw = a.slab_w + (size_t)blockIdx.x * (3 * H) * (2 * H);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int jj = (jt0 + j) * 32 + acc_row(reg, half);
            sw[(size_t)jj * (2 * H) + role * H + tt * 32 + c32] = acc[j][reg];
        }
    // bias sums: the 32 row positions of each column folded in order through the now idle LDS ([32][4][64] floats)
    {
        float* red = lds;
        *reinterpret_cast<float4*>(red + srow * 256 + 0 * 64 + f4) = make_float4(bs_r[0], bs_r[1], bs_r[2], bs_r[3]);
        *reinterpret_cast<float4*>(red + srow * 256 + 1 * 64 + f4) = make_float4(bs_z[0], bs_z[1], bs_z[2], bs_z[3]);
        *reinterpret_cast<float4*>(red + srow * 256 + 2 * 64 + f4) = make_float4(bs_n[0], bs_n[1], bs_n[2], bs_n[3]);
        *reinterpret_cast<float4*>(red + srow * 256 + 3 * 64 + f4) = make_float4(bs_nr[0], bs_nr[1], bs_nr[2], bs_nr[3]);
        __syncthreads();
        if (tid < 256) {
            float s = 0.f;
            for (int r = 0; r < 32; ++r) s += red[r * 256 + tid];
            float* sb = a.slab_b + (size_t)blockIdx.x * 6 * H;
            const int g = tid >> 6, c = tid & 63;          // g: r, z, n, n r
            if (g < 3) sb[g * H + c] = s;                  // db_ih = [dr | dz | dn]
            if (g != 2) sb[3 * H + (g == 3 ? 2 : g) * H + c] = s;     // db_hh = [dr | dz | dn r]
        }
    }
}


// dW_ih[j][k] += sum_rs slab[rs][j][k], k < IN ; dW_hh[j][k-IN] += ... ; biases likewise
__global__ void k_gru_reduce_w(const float* __restrict__ slab_w, const float* __restrict__ slab_b, int n_rs,
                               int IN, int H, float* __restrict__ dW_ih, float* __restrict__ dW_hh,
                               float* __restrict__ db_ih, float* __restrict__ db_hh) {
    const int XH = IN + H;
    const size_t nW = (size_t)3 * H * XH;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nW) {
        float s = 0.f;
        for (int k = 0; k < n_rs; ++k) s += slab_w[(size_t)k * nW + i];
        const int j = (int)(i / XH), col = (int)(i % XH);
        if (col < IN) dW_ih[(size_t)j * IN + col] += s;
        else dW_hh[(size_t)j * H + (col - IN)] += s;
    } else if (i < nW + (size_t)6 * H) {
        const int b = (int)(i - nW);
        float s = 0.f;
        for (int k = 0; k < n_rs; ++k) s += slab_b[(size_t)k * 6 * H + b];
        if (b < 3 * H) db_ih[b] += s;
        else db_hh[b - 3 * H] += s;
    }
}

// the same for one launch of a concat cell (slabs [3H][H | H], IN = H per launch): the W_ih block into the column half
// dW_ih points at (row stride ld_dwih); the W_hh block and the biases only from the launch that computed them (full)
__global__ void k_gru_reduce_w_half(const float* __restrict__ slab_w, const float* __restrict__ slab_b, int n_rs, int H,
                                    float* __restrict__ dW_ih, int ld_dwih, float* __restrict__ dW_hh,
                                    float* __restrict__ db_ih, float* __restrict__ db_hh, int full) {
    const int XH = 2 * H;
    const size_t nW = (size_t)3 * H * XH;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nW) {
        const int j = (int)(i / XH), col = (int)(i % XH);
        if (col >= H && !full) return;
        float s = 0.f;
        for (int k = 0; k < n_rs; ++k) s += slab_w[(size_t)k * nW + i];
        if (col < H) dW_ih[(size_t)j * ld_dwih + col] += s;
        else dW_hh[(size_t)j * H + (col - H)] += s;
    } else if (full && i < nW + (size_t)6 * H) {
        const int b = (int)(i - nW);
        float s = 0.f;
        for (int k = 0; k < n_rs; ++k) s += slab_b[(size_t)k * 6 * H + b];
        if (b < 3 * H) db_ih[b] += s;
        else db_hh[b - 3 * H] += s;
    }
}

__global__ void k_fold_slabs_gru(const float* __restrict__ slabs, size_t stride, int nslab, float* __restrict__ out,
                                 size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k0 = blockIdx.y * 32, k1 = min(nslab, k0 + 32);
    float s = 0.f;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) s += slabs[(size_t)k * stride + i];
    out[(size_t)blockIdx.y * n + i] = s;
}

// k_gru_bwd_zs's slabs: dW_ih[j][k] += sum_rs (slab[rs][j][k] + slab[rs][j][H + k]) (the two K-steps); biases as k_gru_reduce_w
__global__ void k_gru_reduce_w_zs(const float* __restrict__ slab_w, const float* __restrict__ slab_b, int n_rs, int H,
                                  float* __restrict__ dW_ih, float* __restrict__ db_ih, float* __restrict__ db_hh) {
    const size_t nI = (size_t)3 * H * H, nW = 2 * nI;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nI) {
        const size_t o = (i / H) * (2 * H) + (i % H);
        float s = 0.f;
        for (int k = 0; k < n_rs; ++k) s += slab_w[(size_t)k * nW + o] + slab_w[(size_t)k * nW + o + H];
        dW_ih[i] += s;
    } else if (i < nI + (size_t)6 * H) {
        const int b = (int)(i - nI);
        float s = 0.f;
        for (int k = 0; k < n_rs; ++k) s += slab_b[(size_t)k * 6 * H + b];
        if (b < 3 * H) db_ih[b] += s;
        else db_hh[b - 3 * H] += s;
    }
}


// H = 64 weight-gradient kernel: 1 = bf16x6 split products (default), 0 = f32-input MFMA.  A constant of the process,
// read from the environment when the library is loaded (TMPNN_SPLIT_WEIGHTS=0/1; TMPNN_SPLIT=0 implies 0): every
// rank and every run uses the same kernel, so gradients are bitwise reproducible across processes.
static int weights_variant_default() {
    static const int v = [] {
        if (!split_enabled()) return 0;
        const char* e = getenv("TMPNN_SPLIT_WEIGHTS");
        return (e && e[0] == '0') ? 0 : 1;
    }();
    return v;
}
static void plan_weights(int R, int IN, int H, int* n_rs, int* RS, int* NQ, int* NCH) {
    *NQ = 3 * H / 32;
    *NCH = (IN + H + 127) / 128;
    long per = (long)(*NQ) * (*NCH);
    long want = 4096 / per;                  // ~16 waves per CU in flight
    if (want < 1) want = 1;
    long by_rows = (R + 63) / 64;            // at least 64 rows per slab
    long n = by_rows < want ? by_rows : want;
    if (n < 1) n = 1;
    long rs = (R + n - 1) / n;
    rs = (rs + 1) & ~1L;                     // even: one MFMA step eats two rows
    if (rs < 2) rs = 2;
    n = (R + rs - 1) / rs;
    if (n < 1) n = 1;
    *n_rs = (int)n;
    *RS = (int)rs;
}

}  // namespace tmpnn

using namespace tmpnn;

extern "C" {

int tmpnn_gru_bwd_data(const int32_t* rows, int R, int IN, const float* h, int ld_h, int H, const float* w_ih,
                       const float* w_hh, const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout,
                       const float* dy, const float* w_head, float* d_msg, int ld_dmsg, float* d_h, int ld_dh,
                       const int32_t* add_src, const int32_t* add_dst, const float* add_msg, int ld_add,
                       tmpnn_stream stream) {
    TM_REQUIRE(supported_H_cell(H), "gru_bwd_data: unsupported H=%d", H);
    if (R == 0) return TMPNN_OK;
    TM_REQUIRE(R > 0 && IN > 0 && IN % 32 == 0 && (H % 64 != 0 || IN % 64 == 0), "gru_bwd_data: R=%d IN=%d", R, IN);
    TM_REQUIRE(rows && h && w_ih && w_hh && gates && d_msg && d_h, "gru_bwd_data: null pointer");
    TM_REQUIRE(d_hout != nullptr || dy != nullptr, "gru_bwd_data: no upstream gradient (d_hout and dy both null)");
    TM_REQUIRE(dy == nullptr || (w_head != nullptr && aligned16(w_head)), "gru_bwd_data: dy needs a 16-byte aligned w_head");
    TM_REQUIRE((ld_h & 3) == 0 && aligned16(h) && aligned16(gates) && (gate_plane & 3) == 0 &&
                   (d_hout == nullptr || ((ld_dhout & 3) == 0 && aligned16(d_hout) && ld_dhout >= H)),
               "gru_bwd_data: rows must be 16-byte aligned");
    TM_REQUIRE(ld_dmsg >= IN && ld_dh >= H && ld_h >= H, "gru_bwd_data: leading dimension too small");
    TM_REQUIRE(add_msg == nullptr || (add_src && add_dst && ld_add >= H), "gru_bwd_data: fused aggregation adjoint args");
    GruBwdDataArgs a{rows, R, IN, h, ld_h, H, w_ih, w_hh, gates, gate_plane, DhSrc{d_hout, ld_dhout, dy, w_head},
                     d_msg, ld_dmsg, d_h, ld_dh, add_src, add_dst, add_msg, ld_add};
    hipStream_t st = as_stream(stream);
    if (H <= 64 && (IN == H || IN == 2 * H) && aligned16(w_ih) && aligned16(w_hh) && aligned16(d_msg) &&
        (ld_dmsg & 3) == 0 && aligned16(d_h) && (ld_dh & 3) == 0 &&
        (add_msg == nullptr || (aligned16(add_msg) && (ld_add & 3) == 0))) {
        const int ntiles = ceil_div(R, 256);
        dim3 pgrid(ntiles < 256 ? ntiles : 256), pblock(512);
        const size_t shm = sizeof(float) * ((size_t)(IN + H) * 3 * H + 4);
        const int up = (d_hout ? 1 : 0) | (dy ? 2 : 0);
        const bool fuse = add_msg != nullptr;
        if (split_enabled() && IN == H) {
            const size_t shm2 = (size_t)3 * (IN + H) * (3 * H + 8) * 2 + 16 + sizeof(float) * H;
#define S3(HH, UU, FF)                                                                                       \
    do {                                                                                                     \
        TM_SHM_ONCE((k_gru_bwd_data_split<HH, UU, FF>), shm2);                    \
        hipLaunchKernelGGL((k_gru_bwd_data_split<HH, UU, FF>), pgrid, pblock, shm2, st, a, ntiles);          \
    } while (0)
#define SL(HH)                                                                                               \
    do {                                                                                                     \
        if (fuse) { if (up == 1) S3(HH, 1, true); else if (up == 2) S3(HH, 2, true); else S3(HH, 3, true); }      \
        else      { if (up == 1) S3(HH, 1, false); else if (up == 2) S3(HH, 2, false); else S3(HH, 3, false); }   \
    } while (0)
            if (H == 64) SL(64); else SL(32);
#undef SL
#undef S3
            return check_launch("gru_bwd_data_split");
        }
#define L3(HH, II, UU, FF)                                                                                   \
    do {                                                                                                     \
        TM_SHM_ONCE((k_gru_bwd_data_lds<HH, II, UU, FF>), shm);                     \
        hipLaunchKernelGGL((k_gru_bwd_data_lds<HH, II, UU, FF>), pgrid, pblock, shm, st, a, ntiles);         \
    } while (0)
#define LL(HH, II)                                                                                           \
    do {                                                                                                     \
        if (fuse) { if (up == 1) L3(HH, II, 1, true); else if (up == 2) L3(HH, II, 2, true); else L3(HH, II, 3, true); }      \
        else      { if (up == 1) L3(HH, II, 1, false); else if (up == 2) L3(HH, II, 2, false); else L3(HH, II, 3, false); }   \
    } while (0)
        if (H == 64) { if (IN == 64) LL(64, 64); else LL(64, 128); }
        else         { if (IN == 32) LL(32, 32); else LL(32, 64); }
#undef LL
#undef L3
        return check_launch("gru_bwd_data_lds");
    }
    // wider column blocks re-read (and re-derive) the gate planes fewer times
    int NT = (H % 128 == 0 && IN % 128 == 0) ? 4 : (H % 64 == 0) ? 2 : 1;
    if (NT > 1 && (long)ceil_div(R, 128) * ((IN + H) / (32 * NT)) < 128) NT = 1;      // (batch-1 graphs: see tmpnn_gru_fwd)
    dim3 grid(ceil_div(R, 128), (IN + H) / (32 * NT)), block(256);
    if (NT == 4) hipLaunchKernelGGL((k_gru_bwd_data<4>), grid, block, 0, st, a);
    else if (NT == 2) hipLaunchKernelGGL((k_gru_bwd_data<2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_gru_bwd_data<1>), grid, block, 0, st, a);
    return check_launch("gru_bwd_data");
}

static bool weights_use_lds(int IN, int H) { return H == 64 && IN == H; }
static int weights_lds_blocks(int R) {
    const int ntiles = ceil_div(R, 32);
    return ntiles < 512 ? ntiles : 512;          // persistent: <= 2 blocks per CU
}

// output-tiled kernel for the wide cells: (H/64) x ceil((IN+H)/128) output chunks per row slab
static bool weights_use_chunk(int IN, int H) { return H % 64 == 0 && IN % 64 == 0 && !weights_use_lds(IN, H); }
static int weights_chunk_slabs(int R, int IN, int H) {
    const int ntiles = ceil_div(R, 32);
    const int per = (H / 64) * ceil_div(IN + H, 128);
    int want = 1024 / per;
    if (want < 1) want = 1;
    return ntiles < want ? ntiles : want;
}


// the one-pass backward's form: eight 256-register waves per block (k_gru_bwd_two) or four 512-register waves
// (k_gru_bwd_one); a constant of the process (TMPNN_BWD_TWO), never a measurement
#ifdef TMPNN_KEEP_VARIANTS
static bool fused_two_waves() {
    static const bool v = [] { const char* e = getenv("TMPNN_BWD_TWO"); return e == nullptr || e[0] != '0'; }();
    return v;
}
#endif

static int fused_blocks(int R) {
    const int ntiles = ceil_div(R, 32);
    return ntiles < 256 ? ntiles : 256;
}

// the one-pass kernel takes the whole LDS of a CU (two 80 KiB operand-image sets): only offered where a block may have it
static bool device_gives_160k() {
    static std::atomic<int> cache[16];               // 0 unknown, 1 yes, 2 no   (a constant of the device)
    int dev = 0;
    (void)hipGetDevice(&dev);
    int v = cache[dev & 15].load(std::memory_order_relaxed);
    if (v == 0) {
        int bytes = 0;
        if (hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) bytes = 0;
        v = bytes >= 163840 ? 1 : 2;
        cache[dev & 15].store(v, std::memory_order_relaxed);
    }
    return v == 1;
}

int tmpnn_gru_bwd_fused_available(int H, int IN, int xmode) {
#ifdef TMPNN_KEEP_VARIANTS
    if (xmode == 2 && !fused_two_waves()) return 0;          // (the concat halves exist in the eight-wave form only)
#endif
    return (H == 64 && ((IN == 64 && (xmode == 0 || xmode == 1)) || (IN == 128 && xmode == 2)) && device_gives_160k()) ? 1 : 0;
}

size_t tmpnn_gru_bwd_fused_ws(int R, int IN, int H) {
    if (R <= 0) return 0;
    const int n = fused_blocks(R);
    const size_t per = (size_t)3 * H * (IN + H) + (size_t)6 * H;
    return ((size_t)n * per + reduce_slabs_ws_floats(n, per)) * sizeof(float);
}

// The concat cell (xmode 2, IN = 2H): [h[src] | h[dst]] W_ih^T = h[src] W1^T + h[dst] W2^T with W_ih = [W1 | W2], so its backward
// is the single-endpoint cell twice: launch A over (src, W1) does everything a diff cell's launch does (d_h, dW_hh, biases, the
// fused row-F adjoint) and writes d_msg[:, 0:H], dW_ih[:, 0:H]; launch B over (dst, W2) only the W_ih side into the other halves.
static int gru_bwd_fused_concat(GruBwdFusedArgs a, int R, int H, const int32_t* src, const int32_t* dst, const float* w_ih,
                                float* d_msg, float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, float* fold, int up,
                                bool fuse, hipStream_t st) {
    const int n_rs = fused_blocks(R);
    const int ntiles = ceil_div(R, 32);
    const size_t shm = 163840;
    const size_t nW = (size_t)3 * H * 2 * H, nB = (size_t)6 * H;
    int rc;
    for (int half = 0; half < 2; ++half) {
        a.src = half == 0 ? src : dst;
        a.dst = half == 0 ? dst : src;                      // (read by the fused adjoint of launch A only)
        a.w_ih = w_ih + (size_t)half * H;
        a.ld_wih = 2 * H;
        a.d_msg = d_msg + (size_t)half * H;
#define LC(U, F, S)                                                                                          \
    do {                                                                                                     \
        TM_SHM_ONCE((k_gru_bwd_two<2, U, F, S>), shm);                                                       \
        hipLaunchKernelGGL((k_gru_bwd_two<2, U, F, S>), dim3(n_rs), dim3(512), shm, st, a, ntiles);          \
    } while (0)
#define LCU(F, S) do { if (up == 1) LC(1, F, S); else if (up == 2) LC(2, F, S); else LC(3, F, S); } while (0)
        if (half == 0) { if (fuse) LCU(true, true); else LCU(false, true); }
        else LCU(false, false);
#undef LCU
#undef LC
        if ((rc = check_launch("gru_bwd_fused_concat"))) return rc;
        const float* rw = a.slab_w;
        const float* rb = a.slab_b;
        int nred = n_rs;
        if (n_rs > 64) {
            const int ng = ceil_div(n_rs, 32);
            float* fw = fold;
            float* fb = fold + (size_t)ng * nW;
            hipLaunchKernelGGL(k_fold_slabs_gru, dim3(ceil_div((long)nW, 256), ng), dim3(256), 0, st, a.slab_w, nW, n_rs, fw, nW);
            if (half == 0)
                hipLaunchKernelGGL(k_fold_slabs_gru, dim3(ceil_div((long)nB, 256), ng), dim3(256), 0, st, a.slab_b, nB, n_rs, fb, nB);
            if ((rc = check_launch("gru_fold"))) return rc;
            rw = fw; rb = fb; nred = ng;
        }
        hipLaunchKernelGGL(k_gru_reduce_w_half, dim3(ceil_div((long)(nW + nB), 256)), dim3(256), 0, st, rw, rb, nred, H,
                           dW_ih + (size_t)half * H, 2 * H, dW_hh, db_ih, db_hh, half == 0 ? 1 : 0);
        if ((rc = check_launch("gru_reduce_w_half"))) return rc;
    }
    return TMPNN_OK;
}

int tmpnn_gru_bwd_fused(const int32_t* rows, int R, int xmode, const int32_t* src, const int32_t* dst, const float* msg,
                        int ld_msg, int msg_compact, int IN, const float* h, int ld_h, int H, const float* w_ih,
                        const float* w_hh, const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout,
                        const float* dy, const float* w_head, float* d_msg, int ld_dmsg, float* d_h, int ld_dh,
                        const int32_t* add_src, const int32_t* add_dst, const float* add_msg, int ld_add, float* dW_ih,
                        float* dW_hh, float* db_ih, float* db_hh, void* ws, size_t ws_bytes, tmpnn_stream stream) {
    TM_REQUIRE(tmpnn_gru_bwd_fused_available(H, IN, xmode), "gru_bwd_fused: H=%d IN=%d xmode=%d not supported", H, IN, xmode);
    if (R == 0) return TMPNN_OK;
    TM_REQUIRE(R > 0 && rows && h && w_ih && w_hh && gates && d_msg && d_h && dW_ih && dW_hh && db_ih && db_hh,
               "gru_bwd_fused: null pointer");
    TM_REQUIRE(d_hout != nullptr || dy != nullptr, "gru_bwd_fused: no upstream gradient");
    TM_REQUIRE(dy == nullptr || (w_head != nullptr && aligned16(w_head)), "gru_bwd_fused: dy needs a 16-byte aligned w_head");
    TM_REQUIRE(xmode == 0 ? (msg != nullptr && (ld_msg & 3) == 0 && aligned16(msg) && ld_msg >= IN) : (src && dst),
               "gru_bwd_fused: message source");
    TM_REQUIRE((ld_h & 3) == 0 && aligned16(h) && aligned16(gates) && (gate_plane & 3) == 0 && aligned16(w_ih) &&
                   aligned16(w_hh) && (d_hout == nullptr || ((ld_dhout & 3) == 0 && aligned16(d_hout))) &&
                   (ld_dmsg & 3) == 0 && aligned16(d_msg) && (ld_dh & 3) == 0 && aligned16(d_h) &&
                   (add_msg == nullptr || ((ld_add & 3) == 0 && aligned16(add_msg) && add_src && add_dst)),
               "gru_bwd_fused: rows must be 16-byte aligned");
    TM_REQUIRE(xmode == 0 || add_msg == nullptr || (add_src == src && add_dst == dst),
               "gru_bwd_fused: with xmode != 0 the fused adjoint gathers through src / dst (pass the same arrays)");
    const size_t need = tmpnn_gru_bwd_fused_ws(R, IN, H);
    if (ws == nullptr || ws_bytes < need)
        return set_error(TMPNN_EWORKSPACE, "gru_bwd_fused: workspace %zu < %zu bytes", ws_bytes, need);
    const int n_rs = fused_blocks(R);
    const size_t nW = (size_t)3 * H * (IN + H), nB = (size_t)6 * H;
    float* slab_w = reinterpret_cast<float*>(ws);
    float* slab_b = slab_w + (size_t)n_rs * nW;
    float* fold = slab_b + (size_t)n_rs * nB;
    GruBwdFusedArgs a{rows, R, src, dst, msg, ld_msg, msg_compact, h, ld_h, w_ih, w_hh, gates, gate_plane,
                      DhSrc{d_hout, ld_dhout, dy, w_head}, d_msg, ld_dmsg, d_h, ld_dh, add_src, add_dst, add_msg, ld_add,
                      slab_w, slab_b, IN};
    const int ntiles = ceil_div(R, 32);
    const size_t shm = 163840;                               // two 80 KiB operand-image sets: the whole LDS of a CU
    hipStream_t st = as_stream(stream);
    const int up = (d_hout ? 1 : 0) | (dy ? 2 : 0);
    const bool fuse = add_msg != nullptr;
    if (xmode == 2) {
        TM_REQUIRE(ld_dmsg >= 2 * H, "gru_bwd_fused: the concat cell writes d_msg [.., 2H]");
        // (the slab layout of a launch is the IN = H one; the fold area sits behind the larger IN = 2H reservation's slabs)
        float* sb = slab_w + (size_t)n_rs * 3 * H * 2 * H;
        a.slab_b = sb;
        return gru_bwd_fused_concat(a, R, H, src, dst, w_ih, d_msg, dW_ih, dW_hh, db_ih, db_hh, sb + (size_t)n_rs * nB, up,
                                    fuse, st);
    }
#ifdef TMPNN_KEEP_VARIANTS
#define LF(X, U, F)                                                                                          \
    do {                                                                                                     \
        if (fused_two_waves() && !((X) == 0 && (F))) {     /* (message cell + fused adjoint: four-wave form only) */ \
            TM_SHM_ONCE((k_gru_bwd_two<X, U, F>), shm);                                                      \
            hipLaunchKernelGGL((k_gru_bwd_two<X, U, F>), dim3(n_rs), dim3(512), shm, st, a, ntiles);         \
        } else {                                                                                             \
            TM_SHM_ONCE((k_gru_bwd_one<X, U, F>), shm);                                                      \
            hipLaunchKernelGGL((k_gru_bwd_one<X, U, F>), dim3(n_rs), dim3(256), shm, st, a, ntiles);         \
        }                                                                                                    \
    } while (0)
#else
    // (a message cell -- xmode 0 -- with the fused adjoint exists only in the four-wave comparison build; nothing asks for it)
    TM_REQUIRE(!(xmode == 0 && fuse), "gru_bwd_fused: xmode 0 with a fused adjoint needs a TMPNN_KEEP_VARIANTS build");
#define LF(X, U, F)                                                                                          \
    do {                                                                                                     \
        if (!((X) == 0 && (F))) {                                                                            \
            TM_SHM_ONCE((k_gru_bwd_two<X, U, F>), shm);                                                      \
            hipLaunchKernelGGL((k_gru_bwd_two<X, U, F>), dim3(n_rs), dim3(512), shm, st, a, ntiles);         \
        }                                                                                                    \
    } while (0)
#endif
#define LU(X, F) do { if (up == 1) LF(X, 1, F); else if (up == 2) LF(X, 2, F); else LF(X, 3, F); } while (0)
    if (xmode == 0) { if (fuse) LU(0, true); else LU(0, false); }
    else            { if (fuse) LU(1, true); else LU(1, false); }
#undef LU
#undef LF
    int rc = check_launch("gru_bwd_fused");
    if (rc) return rc;
    const float* rw = slab_w;
    const float* rb = slab_b;
    int nred = n_rs;
    if (n_rs > 64) {
        const int ng = ceil_div(n_rs, 32);
        float* fw = fold;
        float* fb = fold + (size_t)ng * nW;
        hipLaunchKernelGGL(k_fold_slabs_gru, dim3(ceil_div((long)nW, 256), ng), dim3(256), 0, st, slab_w, nW, n_rs, fw, nW);
        hipLaunchKernelGGL(k_fold_slabs_gru, dim3(ceil_div((long)nB, 256), ng), dim3(256), 0, st, slab_b, nB, n_rs, fb, nB);
        if ((rc = check_launch("gru_fold"))) return rc;
        rw = fw; rb = fb; nred = ng;
    }
    hipLaunchKernelGGL(k_gru_reduce_w, dim3(ceil_div((long)(nW + nB), 256)), dim3(256), 0, st, rw, rb, nred, IN, H,
                       dW_ih, dW_hh, db_ih, db_hh);
    return check_launch("gru_reduce_w");
}

int tmpnn_gru_bwd_fused_zero_state_available(int H, int IN, int xmode) {
    return (H == 64 && IN == 64 && xmode == 1 && device_gives_160k()) ? 1 : 0;
}

int tmpnn_gru_bwd_fused_zero_state(const int32_t* rows, int R, const int32_t* src, const int32_t* dst, int IN,
                                   const float* h, int ld_h, int H, const float* w_ih, const float* b_hn,
                                   const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout,
                                   const float* dy, const float* w_head, float* d_msg, int ld_dmsg, float* dW_ih,
                                   float* db_ih, float* db_hh, void* ws, size_t ws_bytes, tmpnn_stream stream) {
    TM_REQUIRE(tmpnn_gru_bwd_fused_zero_state_available(H, IN, 1), "gru_bwd_fused_zero_state: H=%d IN=%d not supported", H, IN);
    if (R == 0) return TMPNN_OK;
    TM_REQUIRE(R > 0 && rows && src && dst && h && w_ih && b_hn && gates && d_msg && dW_ih && db_ih && db_hh,
               "gru_bwd_fused_zero_state: null pointer");
    // gate_plane == 0: no planes were saved; `gates` is a host struct naming what the kernel forms r, z, n from
    const bool rc_gates = gate_plane == 0;
    ZsGateSrc gsrc{};
    if (rc_gates) {
        const tmpnn_zs_gate_src* g = reinterpret_cast<const tmpnn_zs_gate_src*>(gates);
        TM_REQUIRE(g->proj && g->src_pos && g->dst_pos && g->b_ih && g->b_hh,
                   "gru_bwd_fused_zero_state: gate_plane = 0 needs proj, src_pos, dst_pos, b_ih and b_hh (struct tmpnn_zs_gate_src)");
        TM_REQUIRE(aligned16(g->proj) && g->ld_proj >= 3 * H && (g->ld_proj & 3) == 0 && aligned16(g->b_ih) && aligned16(g->b_hh),
                   "gru_bwd_fused_zero_state: gate source layout (16-byte alignment, ld_proj=%d)", (int)g->ld_proj);
        TM_REQUIRE(b_hn == g->b_hh + 2 * H, "gru_bwd_fused_zero_state: b_hn is not b_hh + 2H of the gate source");
        gsrc = ZsGateSrc{g->proj, g->ld_proj, g->src_pos, g->dst_pos, g->b_ih, g->b_hh};
        gates = nullptr;
    }
    TM_REQUIRE(d_hout != nullptr || dy != nullptr, "gru_bwd_fused_zero_state: no upstream gradient");
    TM_REQUIRE(dy == nullptr || (w_head != nullptr && aligned16(w_head)),
               "gru_bwd_fused_zero_state: dy needs a 16-byte aligned w_head");
    TM_REQUIRE((ld_h & 3) == 0 && aligned16(h) && aligned16(gates) && (gate_plane & 3) == 0 && aligned16(w_ih) &&
                   aligned16(b_hn) && (d_hout == nullptr || ((ld_dhout & 3) == 0 && aligned16(d_hout))) &&
                   (ld_dmsg & 3) == 0 && aligned16(d_msg) && ld_dmsg >= IN && ld_h >= H,
               "gru_bwd_fused_zero_state: rows must be 16-byte aligned");
    const size_t need = tmpnn_gru_bwd_fused_ws(R, IN, H);
    if (ws == nullptr || ws_bytes < need)
        return set_error(TMPNN_EWORKSPACE, "gru_bwd_fused_zero_state: workspace %zu < %zu bytes", ws_bytes, need);
    const int n_rs = fused_blocks(R);
    const size_t nW = (size_t)3 * H * (IN + H), nB = (size_t)6 * H;
    float* slab_w = reinterpret_cast<float*>(ws);
    float* slab_b = slab_w + (size_t)n_rs * nW;
    float* fold = slab_b + (size_t)n_rs * nB;
    GruBwdFusedArgs a{rows, R, src, dst, nullptr, 0, 0, h, ld_h, w_ih, nullptr, gates, gate_plane,
                      DhSrc{d_hout, ld_dhout, dy, w_head}, d_msg, ld_dmsg, nullptr, 0, nullptr, nullptr, nullptr, 0,
                      slab_w, slab_b, IN};
    if (rc_gates) {      // (the fields k_gru_bwd_zs<., true> reads its gate source from)
        a.msg = gsrc.proj; a.ld_msg = gsrc.ld_proj;
        a.add_src = gsrc.src_pos; a.add_dst = gsrc.dst_pos; a.add_msg = gsrc.b_ih;
    }
    const int ntiles = ceil_div(R, 32);
    const size_t shm = 147456;                               // two 72 KiB operand-image sets
    hipStream_t st = as_stream(stream);
    const int up = (d_hout ? 1 : 0) | (dy ? 2 : 0);
#define LZ(U)                                                                                                \
    do {                                                                                                     \
        TM_SHM_ONCE((k_gru_bwd_zs<U>), shm);                                                                 \
        hipLaunchKernelGGL((k_gru_bwd_zs<U>), dim3(n_rs), dim3(512), shm, st, a, b_hn, ntiles);              \
    } while (0)
#define LZR(U)                                                                                               \
    do {                                                                                                     \
        TM_SHM_ONCE((k_gru_bwd_zs<U, true>), shm + 3 * H * sizeof(float));                                   \
        hipLaunchKernelGGL((k_gru_bwd_zs<U, true>), dim3(n_rs), dim3(512), shm + 3 * H * sizeof(float), st, a, b_hn, ntiles); \
    } while (0)
    if (rc_gates) {
        if (up == 1) LZR(1); else if (up == 2) LZR(2); else LZR(3);
    } else {
        if (up == 1) LZ(1); else if (up == 2) LZ(2); else LZ(3);
    }
#undef LZR
#undef LZ
    int rc = check_launch("gru_bwd_fused_zero_state");
    if (rc) return rc;
    const float* rw = slab_w;
    const float* rb = slab_b;
    int nred = n_rs;
    if (n_rs > 64) {
        const int ng = ceil_div(n_rs, 32);
        float* fw = fold;
        float* fb = fold + (size_t)ng * nW;
        hipLaunchKernelGGL(k_fold_slabs_gru, dim3(ceil_div((long)nW, 256), ng), dim3(256), 0, st, slab_w, nW, n_rs, fw, nW);
        hipLaunchKernelGGL(k_fold_slabs_gru, dim3(ceil_div((long)nB, 256), ng), dim3(256), 0, st, slab_b, nB, n_rs, fb, nB);
        if ((rc = check_launch("gru_fold"))) return rc;
        rw = fw; rb = fb; nred = ng;
    }
    hipLaunchKernelGGL(k_gru_reduce_w_zs, dim3(ceil_div((long)(3 * H * H + nB), 256)), dim3(256), 0, st, rw, rb, nred, H,
                       dW_ih, db_ih, db_hh);
    return check_launch("gru_reduce_w_zs");
}

#ifdef TMPNN_KEEP_VARIANTS
int tmpnn_gru_bwd_weights_choice(void) { return weights_variant_default(); }
#endif  // TMPNN_KEEP_VARIANTS

size_t tmpnn_gru_bwd_weights_ws(int R, int IN, int H) {
    if (R <= 0) return 0;
    int n_rs, RS, NQ, NCH;
    plan_weights(R, IN, H, &n_rs, &RS, &NQ, &NCH);
    // the staged kernels need aligned operands; size for whichever path the call ends up on
    if (weights_use_lds(IN, H)) n_rs = std::max(n_rs, weights_lds_blocks(R));
    if (weights_use_chunk(IN, H)) n_rs = std::max(n_rs, weights_chunk_slabs(R, IN, H));
    const size_t per = (size_t)3 * H * (IN + H) + (size_t)6 * H;
    return ((size_t)n_rs * per + reduce_slabs_ws_floats(n_rs, per)) * sizeof(float);
}

int tmpnn_gru_bwd_weights(const int32_t* rows, int R, int xmode, const int32_t* src, const int32_t* dst,
                          const float* msg, int ld_msg, int msg_compact, int IN, const float* h, int ld_h, int H,
                          const float* gates,
                          size_t gate_plane, const float* d_hout, int ld_dhout, const float* dy, const float* w_head,
                          float* dW_ih, float* dW_hh,
                          float* db_ih, float* db_hh, void* ws, size_t ws_bytes, tmpnn_stream stream) {
    return tmpnn_gru_bwd_weights_variant(rows, R, xmode, src, dst, msg, ld_msg, msg_compact, IN, h, ld_h, H, gates,
                                         gate_plane, d_hout, ld_dhout, dy, w_head, dW_ih, dW_hh, db_ih, db_hh, ws,
                                         ws_bytes, -1, stream);
}

int tmpnn_gru_bwd_weights_variant(const int32_t* rows, int R, int xmode, const int32_t* src, const int32_t* dst,
                                  const float* msg, int ld_msg, int msg_compact, int IN, const float* h, int ld_h, int H,
                                  const float* gates,
                                  size_t gate_plane, const float* d_hout, int ld_dhout, const float* dy,
                                  const float* w_head, float* dW_ih, float* dW_hh,
                                  float* db_ih, float* db_hh, void* ws, size_t ws_bytes, int variant,
                                  tmpnn_stream stream) {
    TM_REQUIRE(variant >= -1 && variant <= 1, "gru_bwd_weights: variant %d (need -1, 0 or 1)", variant);
    TM_REQUIRE(supported_H_cell(H), "gru_bwd_weights: unsupported H=%d", H);
    if (R == 0) return TMPNN_OK;
    TM_REQUIRE(R > 0 && xmode >= 0 && xmode <= 2 && IN % 32 == 0 && IN > 0, "gru_bwd_weights: R=%d xmode=%d IN=%d", R,
               xmode, IN);
    TM_REQUIRE(IN == (xmode == 2 ? 2 * H : (xmode == 1 ? H : IN)), "gru_bwd_weights: IN=%d vs xmode=%d", IN, xmode);
    TM_REQUIRE(rows && h && gates && dW_ih && dW_hh && db_ih && db_hh, "gru_bwd_weights: null pointer");
    TM_REQUIRE(d_hout != nullptr || dy != nullptr, "gru_bwd_weights: no upstream gradient");
    TM_REQUIRE(dy == nullptr || (w_head != nullptr && aligned16(w_head)), "gru_bwd_weights: dy needs a 16-byte aligned w_head");
    TM_REQUIRE(xmode == 0 ? msg != nullptr : (src != nullptr && dst != nullptr), "gru_bwd_weights: message source");
    const size_t need = tmpnn_gru_bwd_weights_ws(R, IN, H);
    if (ws == nullptr || ws_bytes < need)
        return set_error(TMPNN_EWORKSPACE, "gru_bwd_weights: workspace %zu < %zu bytes", ws_bytes, need);
    int n_rs, RS, NQ, NCH;
    plan_weights(R, IN, H, &n_rs, &RS, &NQ, &NCH);
    const bool vec_ok = (ld_h & 3) == 0 && (d_hout == nullptr || ((ld_dhout & 3) == 0 && aligned16(d_hout))) &&
                        aligned16(h) && aligned16(gates) && (gate_plane & 3) == 0 &&
                        (xmode != 0 || ((ld_msg & 3) == 0 && aligned16(msg)));
    const bool use_lds = weights_use_lds(IN, H) && xmode != 2 && vec_ok;
    const bool use_chunk = weights_use_chunk(IN, H) && vec_ok;
    if (use_lds) n_rs = weights_lds_blocks(R);
    if (use_chunk) n_rs = weights_chunk_slabs(R, IN, H);
    const size_t nW = (size_t)3 * H * (IN + H), nB = (size_t)6 * H;
    float* slab_w = reinterpret_cast<float*>(ws);
    float* slab_b = slab_w + (size_t)n_rs * nW;
    float* fold = slab_b + (size_t)n_rs * nB;
    GruBwdWArgs a{rows, R, src, dst, msg, ld_msg, IN, msg_compact, h, ld_h, H, gates, gate_plane,
                  DhSrc{d_hout, ld_dhout, dy, w_head}, slab_w, slab_b,
                  n_rs, RS, NQ, NCH};
    hipStream_t st = as_stream(stream);
    int rc;
    if (use_lds) {
        const int ntiles = ceil_div(R, 32);
        dim3 grid(n_rs), block(256);
        const size_t shm = (size_t)3 * 32 * (256 + 128) * 2 + sizeof(float) * 64;
        const int up = (d_hout ? 1 : 0) | (dy ? 2 : 0);
        auto launch_split = [&]() {
#define SW(X, U)                                                                                             \
    do {                                                                                                     \
        TM_SHM_ONCE((k_gru_bwd_weights_split<X, U>), shm);                     \
        hipLaunchKernelGGL((k_gru_bwd_weights_split<X, U>), grid, block, shm, st, a, ntiles);                \
    } while (0)
            if (xmode == 0) { if (up == 1) SW(0, 1); else if (up == 2) SW(0, 2); else SW(0, 3); }
            else            { if (up == 1) SW(1, 1); else if (up == 2) SW(1, 2); else SW(1, 3); }
#undef SW
        };
        auto launch_f32 = [&]() {
#define LW(X, U) hipLaunchKernelGGL((k_gru_bwd_weights_lds<64, X, U>), grid, block, 0, st, a, ntiles)
            if (xmode == 0) { if (up == 1) LW(0, 1); else if (up == 2) LW(0, 2); else LW(0, 3); }
            else            { if (up == 1) LW(1, 1); else if (up == 2) LW(1, 2); else LW(1, 3); }
#undef LW
        };
        // bf16x6 moves 25 % fewer cycles through the matrix pipe than the f32-input MFMA form; which one is faster
        // differed between MI355X boxes in round 1, so the choice is a process constant (weights_variant_default)
        // or the caller's explicit `variant` -- never a measurement inside the call.
        const int choice = (H == 64 && split_enabled()) ? (variant < 0 ? weights_variant_default() : variant) : 0;
        if (choice != 0) {
            launch_split();
            rc = check_launch("gru_bwd_weights_split");
        } else {
            launch_f32();
            rc = check_launch("gru_bwd_weights_lds");
        }
    } else if (use_chunk) {
        const int ntiles = ceil_div(R, 32);
        const int n_cc = ceil_div(IN + H, 128);
        dim3 grid(n_rs, (H / 64) * n_cc), block(256);
        const int up = (d_hout ? 1 : 0) | (dy ? 2 : 0);
#define LW(X, U) hipLaunchKernelGGL((k_gru_bwd_weights_chunk<X, U>), grid, block, 0, st, a, ntiles, n_cc)
#define LWU(X) do { if (up == 1) LW(X, 1); else if (up == 2) LW(X, 2); else LW(X, 3); } while (0)
        if (xmode == 0) LWU(0); else if (xmode == 1) LWU(1); else LWU(2);
#undef LWU
#undef LW
        rc = check_launch("gru_bwd_weights_chunk");
    } else {
        const long nworkers = (long)n_rs * NQ * NCH;
        dim3 grid(ceil_div(nworkers, 4)), block(256);
        if (xmode == 0) hipLaunchKernelGGL((k_gru_bwd_weights<0>), grid, block, 0, st, a);
        else if (xmode == 1) hipLaunchKernelGGL((k_gru_bwd_weights<1>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_gru_bwd_weights<2>), grid, block, 0, st, a);
        rc = check_launch("gru_bwd_weights");
    }
    if (rc) return rc;
    // fold the slabs 32:1 when there are many, then add into the gradient buffers
    const float* rw = slab_w;
    const float* rb = slab_b;
    int nred = n_rs;
    if (n_rs > 64) {
        const int ng = ceil_div(n_rs, 32);
        float* fw = fold;
        float* fb = fold + (size_t)ng * nW;
        hipLaunchKernelGGL(k_fold_slabs_gru, dim3(ceil_div((long)nW, 256), ng), dim3(256), 0, st, slab_w, nW, n_rs, fw, nW);
        hipLaunchKernelGGL(k_fold_slabs_gru, dim3(ceil_div((long)nB, 256), ng), dim3(256), 0, st, slab_b, nB, n_rs, fb, nB);
        if ((rc = check_launch("gru_fold"))) return rc;
        rw = fw; rb = fb; nred = ng;
    }
    hipLaunchKernelGGL(k_gru_reduce_w, dim3(ceil_div((long)(nW + nB), 256)), dim3(256), 0, st, rw, rb, nred, IN, H,
                       dW_ih, dW_hh, db_ih, db_hh);
    return check_launch("gru_reduce_w");
}

}  // extern "C"
