// The CNN's input for the frames of a draw (tmpnn_frames_gather, include/tmpnn.h; host definition:
// trackmpnn_amd.frames.FrameStore.frames_host).  The reference opens, flips, resizes, converts and normalises every frame of every
// chunk on the host each time it is drawn (dataset/kitti_mot.py:367-389, :506-511); here the resized frames stay in HBM as
// planar uint8 and one launch writes the float32 images of a frame plan.
//
// The value is selected, not computed: out = table[c][v] with the host's [3][256] table of (v / 255 - mean[c]) / std[c], so the
// output equals the torch ops that built the table bit for bit.
//
// k_frames_gather  one workgroup per run of whole rows of one image (rows are contiguous on both sides: a run of R rows is one
//                  span of R * W bytes in and R * W floats out, R * W <= FR_TILE unless one row is longer).  The span is loaded
//                  into LDS with 16-byte loads from the 16-byte boundary below its first byte (the store's buffer is aligned, and
//                  a 16-byte piece that would pass the buffer's end is loaded byte by byte), the table is staged next to it, and
//                  after one barrier every thread converts four consecutive pixels a step and stores them as one float4:
//                  threads run along W, a wave stores 1 KiB in a row.  The floats in front of the first and behind the last
//                  16-byte boundary of the output span (W * rows not a multiple of 4) are stored one by one.  A mirrored image
//                  reads pixel W - 1 - x of its row in LDS; global loads and stores are the same either way.
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_TILE = 4096;                       // pixels of a workgroup's run of rows (one row when W is larger)
static_assert(FR_TILE <= TMPNN_FR_MAX_W, "the LDS span holds the longer of a tile and a row");

struct FrRun {
    int W, H, row0, shift, mirrored;
};

// the value of element e of the run (row e / W of the run, pixel e % W)
__device__ __forceinline__ float fr_value(const FrRun& u, const uint8_t* s_px, const float* s_tab, int r, int x) {
    const int sx = u.mirrored ? u.W - 1 - x : x;
    const int row = u.row0 + r;                     // row of the image's [3 * H] rows
    const int c = (row >= u.H) + (row >= 2 * u.H);
    return s_tab[c * 256 + s_px[u.shift + r * u.W + sx]];
}

__global__ __launch_bounds__(FR_THREADS) void k_frames_gather(tmpnn_frames_gather_args a, int R, int tiles) {
    __shared__ __attribute__((aligned(16))) uint8_t s_px[TMPNN_FR_MAX_W + 32];
    __shared__ float s_tab[3 * 256];
    const int tid = threadIdx.x;
    const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
    if (img >= a.T) return;
    // the plan row, checked against the store (block-uniform)
    const int64_t s = a.plan[3 * (int64_t)img], f = a.plan[3 * (int64_t)img + 1];
    if (s < 0 || s >= a.nseq || f < 0) return;
    const int64_t g = a.seq_base[s] + f;
    if (g < 0 || g >= a.seq_base[s + 1] || g >= a.nframes) return;
    FrRun u;
    u.W = a.W; u.H = a.H; u.row0 = tile * R;
    u.mirrored = a.plan[3 * (int64_t)img + 2] != 0;
    const int rows = min(R, 3 * a.H - u.row0);
    if (rows <= 0) return;
    const int span = rows * a.W;                    // <= max(FR_TILE, W)
    const int64_t frame_bytes = (int64_t)3 * a.H * a.W, total = a.nframes * frame_bytes;
    const int64_t src = g * frame_bytes + (int64_t)u.row0 * a.W;
    const int64_t src16 = src & ~(int64_t)15;
    u.shift = (int)(src - src16);
    const int pieces = (u.shift + span + 15) >> 4;  // 16 * pieces <= 15 + span + 15 < sizeof(s_px)
    for (int p = tid; p < pieces; p += FR_THREADS) {
        const int64_t off = src16 + 16 * (int64_t)p;
        if (off + 16 <= total) {
            *reinterpret_cast<uint4*>(s_px + 16 * p) = *reinterpret_cast<const uint4*>(a.frames + off);
        } else {
            for (int j = 0; j < 16; ++j) s_px[16 * p + j] = off + j < total ? a.frames[off + j] : (uint8_t)0;
        }
    }
    for (int i = tid; i < 3 * 256; i += FR_THREADS) s_tab[i] = a.table[i];
    __syncthreads();
    const int64_t out0 = ((int64_t)img * 3 * a.H + u.row0) * a.W;       // first float of the run
    float* out = a.out + out0;
    const int head = min(span, (int)((4 - (out0 & 3)) & 3));            // floats in front of the first 16-byte boundary
    const int nvec = (span - head) >> 2, tail = span - head - 4 * nvec;
    if (tid < head) out[tid] = fr_value(u, s_px, s_tab, tid / a.W, tid % a.W);
    if (tid >= 64 && tid - 64 < tail) {
        const int e = head + 4 * nvec + tid - 64;
        out[e] = fr_value(u, s_px, s_tab, e / a.W, e % a.W);
    }
    for (int q = tid; q < nvec; q += FR_THREADS) {
        const int e = head + 4 * q;
        int r = e / a.W, x = e - r * a.W;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = fr_value(u, s_px, s_tab, r, x);
            if (++x == a.W) { x = 0; ++r; }
        }
        *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

}  // namespace

extern "C" int tmpnn_frames_gather(const tmpnn_frames_gather_args* a, tmpnn_stream stream) {
    TM_REQUIRE(a, "frames_gather: the call struct is null");
    TM_REQUIRE(a->T >= 0 && a->H >= 1 && a->W >= 1 && a->W <= TMPNN_FR_MAX_W && a->H <= (1 << 24), "frames_gather: T=%d H=%d W=%d "
               "(T >= 0, 1 <= H <= 2^24, 1 <= W <= %d)", a->T, a->H, a->W, TMPNN_FR_MAX_W);
    TM_REQUIRE(a->nseq >= 1 && a->nframes >= 1, "frames_gather: nseq=%d nframes=%lld", a->nseq, (long long)a->nframes);
    if (a->T == 0) return TMPNN_OK;
    const int64_t frame = (int64_t)3 * a->H * a->W;
    TM_REQUIRE(a->nframes <= INT64_MAX / frame && (int64_t)a->T <= INT64_MAX / (4 * frame), "frames_gather: the store's or the "
               "output's bytes do not fit in int64");
    TM_REQUIRE(a->frames && a->seq_base && a->plan && a->table && a->out, "frames_gather: null pointer");
    TM_REQUIRE(aligned16(a->frames) && aligned16(a->out), "frames_gather: frames or out is not 16-byte aligned");
    const int R = a->W >= FR_TILE ? 1 : FR_TILE / a->W;
    const int64_t tiles = ((int64_t)3 * a->H + R - 1) / R;
    TM_REQUIRE(tiles * a->T <= INT32_MAX, "frames_gather: %lld workgroups", (long long)(tiles * a->T));
    hipLaunchKernelGGL(k_frames_gather, dim3((unsigned)(tiles * a->T)), dim3(FR_THREADS), 0, as_stream(stream), *a, R, (int)tiles);
    return check_launch("frames_gather");
}
