// Frames as decoded -> the CNN's input size, on the device (tmpnn_frames_resize, include/tmpnn.h; host definition:
// trackmpnn_amd.frames.resize_host / prep_host).  The reference resizes every PIL image on the host with
// transforms.Resize((input_h, input_w)) (dataset/kitti_mot.py:367-389, dataset/bdd100k_mot.py:357): an 8-bit bilinear resize in
// two passes, each a sum of bytes times int32 coefficients of a table the host builds in doubles, rounded with
// (2^21 + sum) >> 22 and clamped to a byte.  With the tables given the arithmetic is integer only, so the device equals the host
// byte for byte by construction.
//
// Two launches, any ksize, no LDS for the pixels:
//   k_resize_h    source [n][h][w][3] -> scratch [n][h][W][3], both interleaved.  A thread owns 16 consecutive output pixels of a
//                 row (48 bytes): per pixel its bounds row and, per tap, one coefficient and three source bytes.  Threads run
//                 along W; the 48 bytes leave as three 16-byte stores where rows keep 16-byte alignment (W a multiple of 16),
//                 else, and for the row's tail of fewer than 16 pixels, byte by byte.
//   k_resize_v    scratch (or the source itself when W == w) -> planar [n][3][H][W].  A thread owns 16 consecutive pixels of an
//                 output row in all three channels: per tap one coefficient and 48 bytes of a source row (three 16-byte loads
//                 where aligned), 48 int32 accumulators.  The result leaves as uint8 (one 16-byte store per channel) or, with a
//                 table, as float32 table[c][v] (four 16-byte stores per channel; the table is staged in LDS), single stores
//                 where the alignment or the tail does not allow it.  When H == h there is no vertical pass: the same kernel
//                 runs one tap of weight 2^22, which hands every byte through unchanged -- the copy.
// A bounds row that does not lie inside the source (the host builds the tables; the device cannot trust them) runs no tap and
// gives 0.  Accumulator: at most 255 * (2^22 + ksize) + 2^21 < 2^31 while ksize <= TMPNN_FR_MAX_TAPS.
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PX = 16;                           // pixels a thread owns
constexpr int RS_ROUND = 1 << 21, RS_SHIFT = 22;

// clamp(ss >> 22, 0, 255).  Written as max, unsigned shift, unsigned min on purpose: for pairs of min(max(ss >> 22, 0), 255) that
// are then packed into a word, hipcc emits v_ashr_pk_u8_i32 and ORs further bytes into the upper half of its result as if that
// half were zero -- on the MI355X it held the accumulator's old bits (bytes 6 and 7 of a thread's 48 came out wrong).
__device__ __forceinline__ uint32_t rs_byte(int ss) { return min((uint32_t)max(ss, 0) >> RS_SHIFT, 255u); }

// 48 bytes at p (the first 3 * cnt of them) as 12 words
__device__ __forceinline__ void rs_load48(const uint8_t* p, int cnt, bool vec, uint32_t (&w)[12]) {
    if (vec && cnt == RS_PX) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + 16 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 12; ++q) w[q] = 0;
#pragma unroll
        for (int k = 0; k < 3 * RS_PX; ++k)
            if (k < 3 * cnt) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    }
}

__global__ __launch_bounds__(RS_THREADS) void k_resize_h(tmpnn_frames_resize_args a, uint8_t* __restrict__ ws, int chunks,
                                                         int64_t total, int vec) {
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / chunks;                 // of the n * h rows
    const int xx0 = (int)(i - row * chunks) * RS_PX;
    const int cnt = min(RS_PX, a.W - xx0);
    const uint8_t* s = a.src + row * a.w * 3;
    uint32_t o[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) o[q] = 0;
#pragma unroll
    for (int p = 0; p < RS_PX; ++p) {
        if (p < cnt) {
            const int xx = xx0 + p;
            int xmin = a.bounds_x[2 * xx];
            int nn = min(a.bounds_x[2 * xx + 1], a.kx);
            if (xmin < 0 || nn < 0 || xmin > a.w - nn) xmin = nn = 0;
            const int32_t* cf = a.coef_x + (int64_t)xx * a.kx;
            const uint8_t* q = s + 3 * xmin;
            int s0 = RS_ROUND, s1 = RS_ROUND, s2 = RS_ROUND;
            for (int x = 0; x < nn; ++x) {
                const int c = cf[x];
                s0 += q[3 * x] * c;
                s1 += q[3 * x + 1] * c;
                s2 += q[3 * x + 2] * c;
            }
            o[(3 * p) >> 2] |= rs_byte(s0) << (8 * ((3 * p) & 3));
            o[(3 * p + 1) >> 2] |= rs_byte(s1) << (8 * ((3 * p + 1) & 3));
            o[(3 * p + 2) >> 2] |= rs_byte(s2) << (8 * ((3 * p + 2) & 3));
        }
    }
    uint8_t* d = ws + (row * a.W + xx0) * 3;
    if (vec && cnt == RS_PX) {
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<uint4*>(d + 16 * q) = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3 * RS_PX; ++k)
            if (k < 3 * cnt) d[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
}

template <bool FLOAT_OUT>
__global__ __launch_bounds__(RS_THREADS) void k_resize_v(tmpnn_frames_resize_args a, const uint8_t* __restrict__ in, int vpass,
                                                         int chunks, int64_t total, int vec_in, int vec_out) {
    __shared__ float s_tab[FLOAT_OUT ? 3 * 256 : 1];
    if (FLOAT_OUT) {
        for (int k = threadIdx.x; k < 3 * 256; k += RS_THREADS) s_tab[k] = a.table[k];
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t oy = i / chunks;                  // of the n * H output rows
    const int xx0 = (int)(i - oy * chunks) * RS_PX;
    const int cnt = min(RS_PX, a.W - xx0);
    const int64_t img = oy / a.H;
    const int y = (int)(oy - img * a.H);
    int ymin = y, nn = 1;
    if (vpass) {
        ymin = a.bounds_y[2 * y];
        nn = min(a.bounds_y[2 * y + 1], a.ky);
        if (ymin < 0 || nn < 0 || ymin > a.h - nn) ymin = nn = 0;
    }
    const int32_t* cf = a.coef_y + (int64_t)y * a.ky;
    int acc[3 * RS_PX];
#pragma unroll
    for (int k = 0; k < 3 * RS_PX; ++k) acc[k] = RS_ROUND;
    const uint8_t* p = in + ((img * a.h + ymin) * a.W + xx0) * 3;
    for (int t = 0; t < nn; ++t) {
        const int c = vpass ? cf[t] : (1 << RS_SHIFT);
        uint32_t w[12];
        rs_load48(p + (int64_t)t * a.W * 3, cnt, vec_in != 0, w);
#pragma unroll
        for (int k = 0; k < 3 * RS_PX; ++k) acc[k] += (int)((w[k >> 2] >> (8 * (k & 3))) & 255u) * c;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t o0 = ((img * 3 + c) * a.H + y) * a.W + xx0;
        if (FLOAT_OUT) {
            float* out = static_cast<float*>(a.out) + o0;
            if (vec_out && cnt == RS_PX) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(out + 4 * q) =
                        make_float4(s_tab[c * 256 + rs_byte(acc[3 * (4 * q) + c])], s_tab[c * 256 + rs_byte(acc[3 * (4 * q + 1) + c])],
                                    s_tab[c * 256 + rs_byte(acc[3 * (4 * q + 2) + c])], s_tab[c * 256 + rs_byte(acc[3 * (4 * q + 3) + c])]);
            } else {
#pragma unroll
                for (int px = 0; px < RS_PX; ++px)
                    if (px < cnt) out[px] = s_tab[c * 256 + rs_byte(acc[3 * px + c])];
            }
        } else {
            uint8_t* out = static_cast<uint8_t*>(a.out) + o0;
            if (vec_out && cnt == RS_PX) {
                uint32_t v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    v[q] = rs_byte(acc[3 * (4 * q) + c]) | rs_byte(acc[3 * (4 * q + 1) + c]) << 8 | rs_byte(acc[3 * (4 * q + 2) + c]) << 16
                           | rs_byte(acc[3 * (4 * q + 3) + c]) << 24;
                *reinterpret_cast<uint4*>(out) = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int px = 0; px < RS_PX; ++px)
                    if (px < cnt) out[px] = (uint8_t)rs_byte(acc[3 * px + c]);
            }
        }
    }
}

// bytes of the horizontal pass's result, rounded up to 16; 0 without a horizontal pass; SIZE_MAX for sizes that do not fit
size_t rs_ws_bytes(int n, int h, int w, int W) {
    if (n <= 0 || W == w) return 0;
    const int64_t row = (int64_t)3 * W;
    if ((int64_t)n > INT64_MAX / 16 / row / h) return SIZE_MAX;
    return (size_t)(((int64_t)n * h * row + 15) & ~(int64_t)15);
}

}  // namespace

extern "C" size_t tmpnn_frames_resize_ws(int n, int h, int w, int H, int W) {
    if (n < 0 || h < 1 || w < 1 || H < 1 || W < 1 || W > TMPNN_FR_MAX_W) return 0;
    const size_t b = rs_ws_bytes(n, h, w, W);
    return b == SIZE_MAX ? 0 : b;
}

extern "C" int tmpnn_frames_resize(const tmpnn_frames_resize_args* a, tmpnn_stream stream) {
    TM_REQUIRE(a, "frames_resize: the call struct is null");
    TM_REQUIRE(a->n >= 0 && a->h >= 1 && a->w >= 1 && a->H >= 1 && a->W >= 1 && a->W <= TMPNN_FR_MAX_W && a->h <= (1 << 24)
               && a->w <= (1 << 24) && a->H <= (1 << 24), "frames_resize: n=%d h=%d w=%d H=%d W=%d (n >= 0, sizes 1 .. 2^24, W <= %d)",
               a->n, a->h, a->w, a->H, a->W, TMPNN_FR_MAX_W);
    TM_REQUIRE(a->kx >= 1 && a->kx <= TMPNN_FR_MAX_TAPS && a->ky >= 1 && a->ky <= TMPNN_FR_MAX_TAPS, "frames_resize: kx=%d ky=%d "
               "(1 <= ksize <= %d: the int32 accumulator)", a->kx, a->ky, TMPNN_FR_MAX_TAPS);
    TM_REQUIRE(a->bounds_x && a->coef_x && a->bounds_y && a->coef_y, "frames_resize: null coefficient table");
    if (a->n == 0) return TMPNN_OK;
    const size_t need = rs_ws_bytes(a->n, a->h, a->w, a->W);
    const int64_t per_in = (int64_t)3 * a->h * a->w, per_out = (int64_t)3 * a->H * a->W;
    TM_REQUIRE(need != SIZE_MAX && (int64_t)a->n <= INT64_MAX / per_in && (int64_t)a->n <= INT64_MAX / (4 * per_out),
               "frames_resize: the frames' bytes do not fit in int64");
    TM_REQUIRE(a->src && a->out, "frames_resize: null pointer");
    const bool hpass = a->W != a->w, vpass = a->H != a->h;
    if (hpass) {
        TM_REQUIRE(a->ws && aligned16(a->ws), "frames_resize: the workspace is null or not 16-byte aligned");
        if (a->ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "frames_resize: workspace of %zu bytes, %zu needed", a->ws_bytes, need);
    }
    const int chunks = (a->W + RS_PX - 1) / RS_PX;
    const int64_t total_h = (int64_t)a->n * a->h * chunks, total_v = (int64_t)a->n * a->H * chunks;
    const int64_t blocks_h = (total_h + RS_THREADS - 1) / RS_THREADS, blocks_v = (total_v + RS_THREADS - 1) / RS_THREADS;
    TM_REQUIRE(blocks_h <= INT32_MAX && blocks_v <= INT32_MAX, "frames_resize: %lld workgroups", (long long)(blocks_h > blocks_v ? blocks_h : blocks_v));
    const bool rows16 = a->W % 16 == 0;             // rows of 3 W bytes (interleaved) and of W bytes (planar) keep 16-byte alignment
    hipStream_t st = as_stream(stream);
    const uint8_t* in = a->src;
    if (hpass) {
        uint8_t* ws = static_cast<uint8_t*>(a->ws);
        hipLaunchKernelGGL(k_resize_h, dim3((unsigned)blocks_h), dim3(RS_THREADS), 0, st, *a, ws, chunks, total_h, (int)rows16);
        const int rc = check_launch("frames_resize (horizontal)");
        if (rc != TMPNN_OK) return rc;
        in = ws;
    }
    const int vec_in = rows16 && aligned16(in);
    if (a->table) {
        const int vec_out = a->W % 4 == 0 && aligned16(a->out);
        hipLaunchKernelGGL(k_resize_v<true>, dim3((unsigned)blocks_v), dim3(RS_THREADS), 0, st, *a, in, (int)vpass, chunks, total_v,
                           vec_in, vec_out);
    } else {
        const int vec_out = rows16 && aligned16(a->out);
        hipLaunchKernelGGL(k_resize_v<false>, dim3((unsigned)blocks_v), dim3(RS_THREADS), 0, st, *a, in, (int)vpass, chunks, total_v,
                           vec_in, vec_out);
    }
    return check_launch("frames_resize (vertical)");
}
