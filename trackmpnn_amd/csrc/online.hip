// Feature rows of a frame's raw detections, written straight into the online tracker's device-resident feature buffer
// (tmpnn_online_features, include/tmpnn.h; host definition: trackmpnn_amd.online.online_features_host).
//
// The arithmetic is the reference's (dataset/kitti_mot.py:545-566) in float32: one-hot category, [score, box centre, box size],
// the temporal pair of t mod fr_range from a table the host built with numpy's sin / cos, the caller's visual columns, and
// every column standardised as (v - mean) / std.  Every operation is a single correctly rounded IEEE operation (no product
// feeds a sum, so nothing can be contracted), hence the rows equal the host definition bit for bit.
//
// D is a few dozen and F at most ~150: the launch is bound by its latency, so one small grid, one element per thread and
// stride, no LDS.
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int OF_THREADS = 256;
constexpr int OF_MAX_BLOCKS = 64;

__global__ __launch_bounds__(OF_THREADS) void k_online_features(int D, int nd, int t_slot, int ncat, int has_temp, int vis_cols,
                                                                const int32_t* __restrict__ raw, const float* __restrict__ vis,
                                                                int ld_vis, const float* __restrict__ mean,
                                                                const float* __restrict__ std_, const float* __restrict__ table,
                                                                float* __restrict__ X, int ld_x, int32_t* __restrict__ y_track,
                                                                int32_t* __restrict__ ids) {
    const int F = ncat + 5 + (has_temp ? 2 : 0) + vis_cols;
    const long total = (long)D * F;
    const long stride = (long)gridDim.x * OF_THREADS;
    for (long i = (long)blockIdx.x * OF_THREADS + threadIdx.x; i < total; i += stride) {
        const int j = (int)(i / F), c = (int)(i % F);
        const int32_t* rw = raw + (size_t)j * 6;
        float v;
        if (c < ncat) {
            v = (rw[0] - 1 == c) ? 1.0f : 0.0f;
        } else if (c < ncat + 5) {
            const int k = c - ncat;
            const float x1 = __int_as_float(rw[2]), y1 = __int_as_float(rw[3]);
            const float x2 = __int_as_float(rw[4]), y2 = __int_as_float(rw[5]);
            v = k == 0   ? __int_as_float(rw[1])
                : k == 1 ? __fadd_rn(x1, x2) * 0.5f
                : k == 2 ? __fadd_rn(y1, y2) * 0.5f
                : k == 3 ? __fsub_rn(x2, x1)
                         : __fsub_rn(y2, y1);
        } else if (has_temp && c < ncat + 7) {
            v = table[(size_t)t_slot * 2 + (c - ncat - 5)];
        } else {
            v = vis[(size_t)j * ld_vis + (c - (F - vis_cols))];
        }
        X[(size_t)(nd + j) * ld_x + c] = __fdiv_rn(__fsub_rn(v, mean[c]), std_[c]);
        if (c == 0) {
            y_track[nd + j] = -1;
            ids[nd + j] = nd + j;
        }
    }
}

}  // namespace

extern "C" int tmpnn_online_features(int D, int nd, int cap, int t_slot, int fr_range, int ncat, int has_temp, int vis_cols,
                                     const int32_t* raw, const float* vis, int ld_vis, const float* mean, const float* std_,
                                     const float* table, float* X, int ld_x, int32_t* y_track, int32_t* ids,
                                     tmpnn_stream stream) {
    TM_REQUIRE(D >= 0 && nd >= 0 && cap >= 0 && (long)nd + D <= cap, "online_features: rows [%d, %d + %d) outside capacity %d", nd,
               nd, D, cap);
    TM_REQUIRE(ncat >= 1 && vis_cols >= 0 && ncat <= 4096 && vis_cols <= 4096, "online_features: ncat=%d vis_cols=%d", ncat, vis_cols);
    const int F = ncat + 5 + (has_temp ? 2 : 0) + vis_cols;
    TM_REQUIRE(ld_x >= F, "online_features: X [cap][ld %d] for F=%d", ld_x, F);
    TM_REQUIRE(!has_temp || (fr_range >= 1 && t_slot >= 0 && t_slot < fr_range), "online_features: t_slot=%d fr_range=%d", t_slot,
               fr_range);
    if (D == 0) return TMPNN_OK;
    TM_REQUIRE(raw && mean && std_ && X && y_track && ids && (!has_temp || table), "online_features: null pointer");
    TM_REQUIRE(vis_cols == 0 || (vis && ld_vis >= vis_cols), "online_features: vis [D][ld %d] for %d columns", ld_vis, vis_cols);
    int blocks = ceil_div((long)D * F, OF_THREADS);
    if (blocks > OF_MAX_BLOCKS) blocks = OF_MAX_BLOCKS;
    hipLaunchKernelGGL(k_online_features, dim3(blocks), dim3(OF_THREADS), 0, as_stream(stream), D, nd, t_slot, ncat, has_temp,
                       vis_cols, raw, vis, ld_vis, mean, std_, table, X, ld_x, y_track, ids);
    return check_launch("online_features");
}
