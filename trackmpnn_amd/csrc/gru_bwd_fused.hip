// GRU cells of the factor-graph update, BACKWARD in ONE pass: data and weight gradients from one read of a
// cell's rows (k_gru_bwd_two; k_gru_bwd_zs for rows whose state is zero), their slab reduction and entry points.  The two-pass
// backward and the final reduce: gru_bwd.hip; shared helpers: gru_common.h, gru_bwd_launch.h.
#include "gru_bwd_launch.h"

namespace tmpnn {

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
//     role-1 partials go to the slab's (unused) W_hh columns and the reduction adds the two halves (SlabSeg::pair_off);
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

}  // namespace tmpnn

using namespace tmpnn;

extern "C" {

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
    return GruSlabs::bytes(fused_blocks(R), IN, H);
}

// The concat cell (xmode 2, IN = 2H): [h[src] | h[dst]] W_ih^T = h[src] W1^T + h[dst] W2^T with W_ih = [W1 | W2], so its backward
// is the single-endpoint cell twice: launch A over (src, W1) does everything a diff cell's launch does (d_h, dW_hh, biases, the
// fused row-F adjoint) and writes d_msg[:, 0:H], dW_ih[:, 0:H]; launch B over (dst, W2) only the W_ih side into the other halves.
// `a` describes the whole cell (ld_wih = 2H); `slabs` has the IN = H layout of one launch.
static int gru_bwd_fused_concat(GruBwdFusedArgs a, const GruSlabs& slabs, int H, UpSel up, bool fuse, float* dW_ih,
                                float* dW_hh, float* db_ih, float* db_hh, hipStream_t st) {
    const int ntiles = ceil_div(a.R, 32);
    const int32_t *src = a.src, *dst = a.dst;
    const float* w_ih = a.w_ih;
    float* d_msg = a.d_msg;
    int rc;
    for (int half = 0; half < 2; ++half) {
        a.src = half == 0 ? src : dst;
        a.dst = half == 0 ? dst : src;                      // (read by the fused adjoint of launch A only)
        a.w_ih = w_ih + (size_t)half * H;
        a.d_msg = d_msg + (size_t)half * H;
        dispatch([&](auto U, auto F, auto HHS) {
            if constexpr (HHS || !F)                        // (the fused adjoint belongs to the launch that owns d_h)
                launch_k<&k_gru_bwd_two<2, U, F, HHS>>(dim3(slabs.n_rs), dim3(512), 163840, st, a, ntiles);
        }, up, Flag{fuse && half == 0}, Flag{half == 0});
        if ((rc = check_launch("gru_bwd_fused_concat"))) return rc;
        // (the W_hh block and the bias slabs are added by launch A only)
        if ((rc = launch_gru_reduce_w(slabs, H, H, dW_ih + (size_t)half * H, 2 * H, dW_hh, db_ih, db_hh, half == 0, st))) return rc;
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
    if (int rc = check_upstream("gru_bwd_fused", d_hout, ld_dhout, dy, w_head, H)) return rc;
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
    // (a concat cell's two launches have the IN = H slab layout, inside the larger IN = 2H reservation)
    const GruSlabs slabs(ws, n_rs, xmode == 2 ? H : IN, H);
    GruBwdFusedArgs a{rows, R, src, dst, msg, ld_msg, msg_compact, h, ld_h, w_ih, w_hh, gates, gate_plane,
                      DhSrc{d_hout, ld_dhout, dy, w_head}, d_msg, ld_dmsg, d_h, ld_dh, add_src, add_dst, add_msg, ld_add,
                      slabs.w, slabs.b, IN};
    const int ntiles = ceil_div(R, 32);
    const size_t shm = 163840;                               // two 80 KiB operand-image sets: the whole LDS of a CU
    hipStream_t st = as_stream(stream);
    const UpSel up = up_sel(d_hout, dy);
    const bool fuse = add_msg != nullptr;
    if (xmode == 2) {
        TM_REQUIRE(ld_dmsg >= 2 * H, "gru_bwd_fused: the concat cell writes d_msg [.., 2H]");
        return gru_bwd_fused_concat(a, slabs, H, up, fuse, dW_ih, dW_hh, db_ih, db_hh, st);
    }
#ifndef TMPNN_KEEP_VARIANTS
    // (a message cell -- xmode 0 -- with the fused adjoint exists only in the four-wave comparison build; nothing asks for it)
    TM_REQUIRE(!(xmode == 0 && fuse), "gru_bwd_fused: xmode 0 with a fused adjoint needs a TMPNN_KEEP_VARIANTS build");
#endif
    dispatch([&](auto X, auto U, auto F) {
        constexpr bool one_only = X == 0 && F;               // message cell + fused adjoint: four-wave form only
#ifdef TMPNN_KEEP_VARIANTS
        if (one_only || !fused_two_waves())
            return launch_k<&k_gru_bwd_one<X, U, F>>(dim3(n_rs), dim3(256), shm, st, a, ntiles);
#endif
        // (not `if constexpr`: k_gru_bwd_two<0, U, true> is compiled, as it always was, and never launched)
        if (!one_only) launch_k<&k_gru_bwd_two<X, U, F>>(dim3(n_rs), dim3(512), shm, st, a, ntiles);
    }, OneOf<0, 1>{xmode}, up, Flag{fuse});
    int rc = check_launch("gru_bwd_fused");
    if (rc) return rc;
    return launch_gru_reduce_w(slabs, IN, H, dW_ih, IN, dW_hh, db_ih, db_hh, 1, st);
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
    if (int rc = check_upstream("gru_bwd_fused_zero_state", d_hout, ld_dhout, dy, w_head, H)) return rc;
    TM_REQUIRE((ld_h & 3) == 0 && aligned16(h) && aligned16(gates) && (gate_plane & 3) == 0 && aligned16(w_ih) &&
                   aligned16(b_hn) && (d_hout == nullptr || ((ld_dhout & 3) == 0 && aligned16(d_hout))) &&
                   (ld_dmsg & 3) == 0 && aligned16(d_msg) && ld_dmsg >= IN && ld_h >= H,
               "gru_bwd_fused_zero_state: rows must be 16-byte aligned");
    const size_t need = tmpnn_gru_bwd_fused_ws(R, IN, H);
    if (ws == nullptr || ws_bytes < need)
        return set_error(TMPNN_EWORKSPACE, "gru_bwd_fused_zero_state: workspace %zu < %zu bytes", ws_bytes, need);
    const int n_rs = fused_blocks(R);
    const GruSlabs slabs(ws, n_rs, IN, H);
    GruBwdFusedArgs a{rows, R, src, dst, nullptr, 0, 0, h, ld_h, w_ih, nullptr, gates, gate_plane,
                      DhSrc{d_hout, ld_dhout, dy, w_head}, d_msg, ld_dmsg, nullptr, 0, nullptr, nullptr, nullptr, 0,
                      slabs.w, slabs.b, IN};
    if (rc_gates) {      // (the fields k_gru_bwd_zs<., true> reads its gate source from)
        a.msg = gsrc.proj; a.ld_msg = gsrc.ld_proj;
        a.add_src = gsrc.src_pos; a.add_dst = gsrc.dst_pos; a.add_msg = gsrc.b_ih;
    }
    const int ntiles = ceil_div(R, 32);
    const size_t shm = 147456;                               // two 72 KiB operand-image sets
    hipStream_t st = as_stream(stream);
    dispatch([&](auto U, auto RC) {
        launch_k<&k_gru_bwd_zs<U, RC>>(dim3(n_rs), dim3(512), shm + (RC ? 3 * H * sizeof(float) : 0), st, a, b_hn, ntiles);
    }, up_sel(d_hout, dy), Flag{rc_gates});
    int rc = check_launch("gru_bwd_fused_zero_state");
    if (rc) return rc;
    // dW_ih[j][k] += sum_rs (slab[rs][j][k] + slab[rs][j][H + k]): the slabs' two K-step halves are added by the reduction
    // (more than 64 slabs: the halves of each group of 32 are summed apart and added per group); biases as launch_gru_reduce_w
    SlabSegs t;
    t.add(slabs.w, slabs.nW, dW_ih, 3 * H, H, 2 * H, H, 1, H);
    slabs.add_bias(t, H, db_ih, db_hh);
    return launch_reduce_segs(t, n_rs, slabs_two_level(n_rs), st);
}

}  // extern "C"
