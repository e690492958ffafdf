// GRU cells of the factor-graph update, BACKWARD in two passes: data and weight gradients as stand-alone
// kernels (generic, LDS-resident f32, bf16x6), the final slab reduction, and their entry points.  The one-pass backward:
// gru_bwd_fused.hip; shared helpers: gru_common.h, gru_bwd_launch.h; the forward: gru_fwd.hip.
#include "gru_bwd_launch.h"

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

// dW_ih[j][k] += sum_rs slab[rs][j][k], k < IN (row stride ld_dwih: a concat cell's launch owns one column half);
// with `full` also dW_hh[j][k-IN] += ... and the biases likewise (the concat cell: only from the launch that computed them)
int launch_gru_reduce_w(const GruSlabs& s, int IN, int H, float* dW_ih, int ld_dwih, float* dW_hh, float* db_ih, float* db_hh,
                        int full, hipStream_t st) {
    SlabSegs t;
    t.add(s.w, s.nW, dW_ih, 3 * H, IN, IN + H, ld_dwih, 1);
    if (full) {
        t.add(s.w + IN, s.nW, dW_hh, 3 * H, H, IN + H, H, 1);
        s.add_bias(t, H, db_ih, db_hh);
    }
    return launch_reduce_segs(t, s.n_rs, slabs_two_level(s.n_rs), st);
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
    // (this entry's own, longer text for a missing upstream gradient comes before check_upstream's)
    TM_REQUIRE(d_hout != nullptr || dy != nullptr, "gru_bwd_data: no upstream gradient (d_hout and dy both null)");
    if (int rc = check_upstream("gru_bwd_data", d_hout, ld_dhout, dy, w_head, H)) return rc;
    TM_REQUIRE((ld_h & 3) == 0 && aligned16(h) && aligned16(gates) && (gate_plane & 3) == 0 &&
                   (d_hout == nullptr || ((ld_dhout & 3) == 0 && aligned16(d_hout))),
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
        const UpSel up = up_sel(d_hout, dy);
        const Flag fuse{add_msg != nullptr};
        if (split_enabled() && IN == H) {
            const size_t shm = (size_t)3 * (IN + H) * (3 * H + 8) * 2 + 16 + sizeof(float) * H;
            dispatch([&](auto HH, auto U, auto F) {
                launch_k<&k_gru_bwd_data_split<HH, U, F>>(pgrid, pblock, shm, st, a, ntiles);
            }, OneOf<64, 32>{H}, up, fuse);
            return check_launch("gru_bwd_data_split");
        }
        const size_t shm = sizeof(float) * ((size_t)(IN + H) * 3 * H + 4);
        dispatch([&](auto HH, auto WIDE, auto U, auto F) {
            launch_k<&k_gru_bwd_data_lds<HH, WIDE ? 2 * HH : HH, U, F>>(pgrid, pblock, shm, st, a, ntiles);
        }, OneOf<64, 32>{H}, Flag{IN == 2 * H}, up, fuse);
        return check_launch("gru_bwd_data_lds");
    }
    // wider column blocks re-read (and re-derive) the gate planes fewer times
    int NT = (H % 128 == 0 && IN % 128 == 0) ? 4 : (H % 64 == 0) ? 2 : 1;
    if (NT > 1 && (long)ceil_div(R, 128) * ((IN + H) / (32 * NT)) < 128) NT = 1;      // (batch-1 graphs: see tmpnn_gru_fwd)
    dim3 grid(ceil_div(R, 128), (IN + H) / (32 * NT)), block(256);
    dispatch([&](auto N) { launch_k<&k_gru_bwd_data<N>>(grid, block, 0, st, a); }, OneOf<4, 2, 1>{NT});
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
    return GruSlabs::bytes(n_rs, IN, H);
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
    if (int rc = check_upstream("gru_bwd_weights", d_hout, ld_dhout, dy, w_head, H)) return rc;
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
    const GruSlabs slabs(ws, n_rs, IN, H);
    GruBwdWArgs a{rows, R, src, dst, msg, ld_msg, IN, msg_compact, h, ld_h, H, gates, gate_plane,
                  DhSrc{d_hout, ld_dhout, dy, w_head}, slabs.w, slabs.b,
                  n_rs, RS, NQ, NCH};
    hipStream_t st = as_stream(stream);
    const UpSel up = up_sel(d_hout, dy);
    const OneOf<0, 1, 2> xm{xmode};
    const int ntiles = ceil_div(R, 32);
    int rc;
    if (use_lds) {
        dim3 grid(n_rs), block(256);
        // bf16x6 moves 25 % fewer cycles through the matrix pipe than the f32-input MFMA form; which one is faster
        // differed between MI355X boxes in round 1, so the choice is a process constant (weights_variant_default)
        // or the caller's explicit `variant` -- never a measurement inside the call.
        const int choice = (H == 64 && split_enabled()) ? (variant < 0 ? weights_variant_default() : variant) : 0;
        if (choice != 0) {
            const size_t shm = (size_t)3 * 32 * (256 + 128) * 2 + sizeof(float) * 64;
            dispatch([&](auto X, auto U) { launch_k<&k_gru_bwd_weights_split<X, U>>(grid, block, shm, st, a, ntiles); },
                     OneOf<0, 1>{xmode}, up);
            rc = check_launch("gru_bwd_weights_split");
        } else {
            dispatch([&](auto X, auto U) { launch_k<&k_gru_bwd_weights_lds<64, X, U>>(grid, block, 0, st, a, ntiles); },
                     OneOf<0, 1>{xmode}, up);
            rc = check_launch("gru_bwd_weights_lds");
        }
    } else if (use_chunk) {
        const int n_cc = ceil_div(IN + H, 128);
        dim3 grid(n_rs, (H / 64) * n_cc), block(256);
        dispatch([&](auto X, auto U) { launch_k<&k_gru_bwd_weights_chunk<X, U>>(grid, block, 0, st, a, ntiles, n_cc); }, xm, up);
        rc = check_launch("gru_bwd_weights_chunk");
    } else {
        const long nworkers = (long)n_rs * NQ * NCH;
        dim3 grid(ceil_div(nworkers, 4)), block(256);
        dispatch([&](auto X) { launch_k<&k_gru_bwd_weights<X>>(grid, block, 0, st, a); }, xm);
        rc = check_launch("gru_bwd_weights");
    }
    if (rc) return rc;
    return launch_gru_reduce_w(slabs, IN, H, dW_ih, IN, dW_hh, db_ih, db_hh, 1, st);
}

}  // extern "C"
