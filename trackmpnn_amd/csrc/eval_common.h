// What the evaluation kernels share (csrc/moteval.hip, csrc/hota.hip, csrc/evalprep.hip; the flag bits also csrc/results.hip):
// the flag word, the checks of a sequence's slices and of a frame's offsets against the store's totals, the wave helpers of
// the frame loaders, the box arithmetic that must equal the host definitions bit for bit, and the dense hypothesis index.
// These kernels index device memory by counts they read from device memory: every such check has its one definition here.
// Contraction is switched off inside the bodies of the box functions, so that they mean the same in whatever translation
// unit includes them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.h"

namespace tmpnn {

// the low byte of a sequence's flag word (Python: trackmpnn_amd/evalstore.py); the 1-based frame index sits above it
enum { FLAG_LIMIT = 1, FLAG_DUPLICATE = 2, FLAG_STORE = 4, FLAG_SOLVER = 8 };
constexpr double EVAL_EPS = 2.220446049250313e-16;          // np.finfo(np.float64).eps

struct EvalSeq { int64_t gt_base, n_gt, det_base, n_det, off_base, n_frames, obj_base, n_obj; };
// A sequence's slices of the store (row s of seq, against the store's totals); false when one does not lie inside the totals or
// the sequence has max_det detections or more: nothing may be indexed then (the host checked its own copy of the table before
// the launch; this is the table the kernels index by).  OBJ = false: a store without objects -- words 6 and 7 of the row are
// not read, obj_base = n_obj = 0, and a total of 0 makes the object check vacuous.
template <bool OBJ = true>
__device__ __forceinline__ bool eval_seq(const int64_t* seq, int s, int64_t n_gt, int64_t n_det, int64_t n_off, int64_t n_obj, int64_t max_det,
                                         EvalSeq& q) {
    const int64_t* p = seq + (size_t)s * 8;
    q.gt_base = p[0]; q.n_gt = p[1]; q.det_base = p[2]; q.n_det = p[3]; q.off_base = p[4]; q.n_frames = p[5];
    q.obj_base = OBJ ? p[6] : 0; q.n_obj = OBJ ? p[7] : 0;
    return q.gt_base >= 0 && q.n_gt >= 0 && q.gt_base + q.n_gt <= n_gt && q.det_base >= 0 && q.n_det >= 0 &&
           q.det_base + q.n_det <= n_det && q.off_base >= 0 && q.n_frames >= 0 && q.off_base + q.n_frames + 1 <= n_off &&
           q.obj_base >= 0 && q.n_obj >= 0 && q.obj_base + q.n_obj <= n_obj && q.n_gt < 0x7fffffff && q.n_det < max_det &&
           q.n_frames < 0x7fffffff;
}

// The rows [g0, g1) / [d0, d1) of frame f (gt_off, det_off: the sequence's offsets); false when they are not monotone inside
// the sequence's rows (q has passed eval_seq: its row counts are below 2^31).
__device__ __forceinline__ bool eval_frame_rows(const int32_t* gt_off, const int32_t* det_off, int64_t f, const EvalSeq& q, int& g0, int& g1,
                                                int& d0, int& d1) {
    g0 = gt_off[f]; g1 = gt_off[f + 1]; d0 = det_off[f]; d1 = det_off[f + 1];
    return !(g0 < 0 || g1 < g0 || g1 > (int)q.n_gt || d0 < 0 || d1 < d0 || d1 > (int)q.n_det);
}

// the first flag of a sequence stays (frame1: the frame counted from 1, 0 for none)
__device__ __forceinline__ void eval_flag_first(unsigned long long* flag, int bits, int64_t frame1) {
    atomicCAS(flag, 0ull, (unsigned long long)bits | ((unsigned long long)frame1 << 8));
}
// what another workgroup of the launch, or the launch before, wrote with an atomic
__device__ __forceinline__ int eval_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long eval_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// n + the position of this lane among the lanes of the wave with `pred` (of use to those lanes only); n grows by their number
__device__ __forceinline__ int wave_rank(bool pred, int lane, int& n) {
    const unsigned long long bal = __ballot(pred);
    const int at = n + __popcll(bal & ((1ull << lane) - 1ull));
    n += __popcll(bal);
    return at;
}
// whether a value occurs twice in ids[0, n) (the whole wave asks, and gets the same answer)
__device__ __forceinline__ bool wave_has_duplicate(const int* ids, int n, int lane) {
    bool dup = false;
    for (int j = lane; j < n; j += 64) {
        const int id = ids[j];
        for (int j2 = 0; j2 < j; ++j2) dup |= ids[j2] == id;
    }
    return __ballot(dup) != 0;
}

// np.maximum / np.minimum: the first operand where it is larger (smaller) or NaN
__device__ __forceinline__ double box_fmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double box_fmin(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ bool box_finite(double x) { return __builtin_fabs(x) < __builtin_huge_val(); }

// Intersection and areas of two x1 y1 x2 y2 boxes: widths and heights in float32 (reference utils/metrics.py:37,39), the corners
// and everything after in float64, every operation a single correctly rounded one in the order of moteval.mot_dist_host.
__device__ __forceinline__ void box_overlap(float4 o, float4 h, double& inter, double& area_o, double& area_h) {
#pragma clang fp contract(off)
    const float wo = o.z - o.x, ho = o.w - o.y, wh = h.z - h.x, hh = h.w - h.y;
    const double otx = o.x, oty = o.y, htx = h.x, hty = h.y;
    const double obx = otx + (double)wo, oby = oty + (double)ho, hbx = htx + (double)wh, hby = hty + (double)hh;
    const double iw = box_fmax(box_fmin(obx, hbx) - box_fmax(otx, htx), 0.0);
    const double ih = box_fmax(box_fmin(oby, hby) - box_fmax(oty, hty), 0.0);
    inter = iw * ih;
    area_o = (double)wo * (double)ho;
    area_h = (double)wh * (double)hh;
}
// 1 - IoU, NaN above 0.5 (host: moteval.mot_dist_host)
__device__ __forceinline__ double mot_dist(float4 o, float4 h) {
#pragma clang fp contract(off)
    double inter, ao, ah;
    box_overlap(o, h, inter, ao, ah);
    const double uni = (ao + ah) - inter;
    double d = 1.0 - inter / uni;
    if (d > 0.5) d = __builtin_nan("");
    return d;
}
// IoU, 0 where union > 0 is false or the quotient is not finite (host: hota.hota_sim_host)
__device__ __forceinline__ double hota_sim(float4 o, float4 h) {
#pragma clang fp contract(off)
    double inter, ao, ah;
    box_overlap(o, h, inter, ao, ah);
    const double uni = (ao + ah) - inter;
    const double q = inter / uni;
    return (uni > 0.0 && box_finite(q)) ? q : 0.0;
}
// intersection over the detection's own area, 0 where area > eps is false or the quotient is not finite (host:
// evalprep.evalprep_ioa_host)
__device__ __forceinline__ double ep_ioa(float4 d, float4 r) {
#pragma clang fp contract(off)
    double inter, area, ar;
    box_overlap(d, r, inter, area, ar);
    const double q = inter / area;
    return (area > EVAL_EPS && box_finite(q)) ? q : 0.0;
}

// The first entry of sequence s in a workspace of n_pair entries that holds n_obj x n_det per sequence: the entries of the
// sequences before it (saturating at n_pair + 1: a table the host did not check cannot overflow the sum).  Every thread of the
// workgroup of THREADS must call it (one barrier); s_sum: THREADS / 64 words of LDS.
template <int THREADS>
__device__ __forceinline__ long long pair_base(const int64_t* seq, int s, int64_t n_obj_total, int64_t n_det_total, int64_t n_pair,
                                               long long* s_sum) {
    const int tid = threadIdx.x;
    long long part = 0;
    for (int s2 = tid; s2 < s; s2 += THREADS) {
        const int64_t a = seq[(size_t)s2 * 8 + 7], b = seq[(size_t)s2 * 8 + 3];
        const long long e = (a < 0 || b < 0 || a > n_obj_total || b > n_det_total) ? n_pair + 1 : a * b;
        part = (e > n_pair || part + e > n_pair) ? n_pair + 1 : part + e;
    }
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
    if ((tid & 63) == 0) s_sum[tid >> 6] = part;
    __syncthreads();
    long long cbase = 0;
    for (int w = 0; w < THREADS / 64; ++w) cbase += s_sum[w];
    return cbase;
}

// The dense index of every kept row's hypothesis id (ids are arbitrary int32 and change with every evaluation), in order of
// first appearance in the n_det (< 2^28) frame-sorted rows of a sequence: an open-addressing table (key, first, dense: 4 n_det
// slots each; integer CAS on the id, integer min on the first row), a scan over the first rows.  id_of(k): the track of sorted
// row k, negative for none; it is called once per row, by thread k % THREADS.  Out: slot[k] the row's table slot, hidx[k] its
// hypothesis index (-1 without a track), count[h] the rows of hypothesis h, n_hyp their number.  It holds workgroup barriers:
// EVERY thread of the workgroup of THREADS must call it, with the same n_det; s_wave: THREADS / 64 + 1 ints of LDS.
template <int THREADS, typename IdOf>
__device__ __forceinline__ void hyp_index(int n_det, IdOf id_of, int32_t* key, int32_t* first, int32_t* dense, int32_t* slot,
                                          int32_t* hidx, int32_t* count, int* s_wave, int& n_hyp) {
    const int tid = threadIdx.x;
    int cap = 1;
    while (cap < 2 * n_det) cap <<= 1;                       // < 4 n_det: at most half of the slots are ever taken
    if (n_det > 0)
        for (int x = tid; x < cap; x += THREADS) { key[x] = -1; first[x] = 0x7fffffff; }
    for (int k = tid; k < n_det; k += THREADS) count[k] = 0;
    __syncthreads();
    for (int k = tid; k < n_det; k += THREADS) {             // (a row belongs to thread k % THREADS in every pass)
        const int id = id_of(k);
        int at = -1;
        if (id >= 0) {
            uint32_t mix = (uint32_t)id * 2654435761u;
            int h = (int)((mix ^ (mix >> 15)) & (uint32_t)(cap - 1));
            for (int probe = 0; probe < cap && at < 0; ++probe) {
                const int old = atomicCAS(&key[h], -1, id);
                if (old == -1 || old == id) at = h; else h = (h + 1) & (cap - 1);
            }
            if (at >= 0) atomicMin(&first[at], k);
        }
        slot[k] = at;
    }
    __syncthreads();
    n_hyp = 0;
    for (int base = 0; base < n_det; base += THREADS) {
        const int k = base + tid;
        const int at = k < n_det ? slot[k] : -1;
        const int is_first = at >= 0 && eval_load(&first[at]) == k;
        int total;
        const int pre = block_scan<THREADS>(is_first, s_wave, &total);
        if (is_first) dense[at] = n_hyp + pre;
        n_hyp += total;
    }
    __syncthreads();
    for (int k = tid; k < n_det; k += THREADS) {
        const int at = slot[k];
        const int hi = at >= 0 ? dense[at] : -1;
        hidx[k] = (hi >= 0 && hi < n_hyp) ? hi : -1;
        if (hi >= 0 && hi < n_hyp) atomicAdd(&count[hi], 1);
    }
}

}  // namespace tmpnn
