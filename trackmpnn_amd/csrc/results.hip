// The score filter over whole tracks and the order of the result table, on the device (tmpnn_results_apply; include/tmpnn.h;
// host definition: trackmpnn_amd.results.results_host, which restates the reference's store_kitti_results /
// store_bdd100k_results without the file).  Everything is integer work: categories, ids, and the scores as order-preserving
// integer keys (results.score_keys), so that a track's best score is an integer maximum and the comparison with the threshold
// an integer comparison -- the result does not depend on the order in which rows arrive at a table slot, and there is no float
// atomic.  One clear of the workspace's head and four launches, whatever the number of sequences (the sequence is the second
// grid dimension; a workgroup strides over its sequence's rows):
//   k_res_group    a thread per row: the slot of the row's id in the sequence's open-addressed table (>= 2 n_det slots, a power
//                  of two; a slot is claimed by integer CAS on id + 1, 0 = free), then integer max of the category and of the
//                  score key and a count of the rows into the slot; the slot of the row is kept;
//   k_res_filter   a thread per row: -1 where the slot's best key is below the threshold key of the slot's category, else the id;
//   k_res_dups     a thread per frame-sorted position: a kept id that an earlier position of the same frame holds as well is a
//                  duplicate; the smallest such frame wins (integer max of 2^40 - frame);
//   k_res_compact  one workgroup per sequence: the kept rows in frame order by a scan over the frame-sorted permutation in spans
//                  of RS_SPAN positions with a carry (block_scan.h), the tail of `order` filled with -1; then the table's slots
//                  counted into the record.
// Phases that need every row of the phase before are separate launches: nothing waits for another workgroup inside a launch.
// Every index is checked against the store's totals before it is used; a sequence that fails a check is flagged, and leaves the
// others alone.
#include "common.h"
#include "eval_common.h"

using namespace tmpnn;

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_ITEMS = 4;                                 // consecutive positions of one thread of the scan
constexpr int RS_SPAN = RS_THREADS * RS_ITEMS;
constexpr int RS_MAX_BLOCKS = 1024;                         // workgroups per sequence of the row kernels (they stride)
constexpr int RS_MAX_SEQ = 65535;                           // gridDim.y
constexpr int64_t RS_MAX_DET = (int64_t)1 << 28;            // rows of one sequence: its table has at most 2^30 slots
constexpr unsigned long long RS_DUP_TOP = 1ull << 40;

enum { FLAG_NEGATIVE = 16 };                                // (beside FLAG_DUPLICATE and FLAG_STORE of csrc/eval_common.h)

struct ResSeq { int64_t tab_base, n_tab, det_base, n_det, off_base, n_frames; };

// what the host entry point checks of the host copy and the kernels of the device copy
__host__ __device__ inline bool res_seq_ok(const ResSeq& q, int64_t tot_tab, int64_t tot_det, int64_t tot_off) {
    if (q.tab_base < 0 || q.n_tab < 0 || q.tab_base + q.n_tab > tot_tab || q.det_base < 0 || q.n_det < 0 || q.det_base + q.n_det > tot_det ||
        q.off_base < 0 || q.n_frames < 0 || q.n_frames >= 0x7fffffff || q.off_base + q.n_frames + 1 > tot_off || q.n_det >= RS_MAX_DET)
        return false;
    if (q.n_det == 0) return true;
    return q.n_tab >= 2 * q.n_det && q.n_tab <= ((int64_t)1 << 30) && (q.n_tab & (q.n_tab - 1)) == 0 && q.n_frames >= 1;
}
__host__ __device__ inline ResSeq res_seq_of(const int64_t* p) { return ResSeq{p[0], p[1], p[2], p[3], p[4], p[5]}; }

struct ResWs {
    // cleared by every call (one contiguous range)
    unsigned* tab_key;                       // [n_tab] id + 1, 0 = free: a sequence's table at its tab_base
    int* tab_cat;                            // [n_tab] max category of the slot's rows
    unsigned* tab_score;                     // [n_tab] max score key
    int* tab_rows;                           // [n_tab] rows
    unsigned long long* dup;                 // [S] 0, or 2^40 - (1-based frame index of a duplicate): the max is the first frame
    unsigned* bits;                          // [S] flag bits
    // written before it is read
    int* slot;                               // [n_det] the row's slot in its sequence's table, -1 without a track
};

__global__ __launch_bounds__(RS_THREADS) void k_res_group(tmpnn_result_store st, const int32_t* __restrict__ tracks, ResWs W) {
    const int s = blockIdx.y;
    const ResSeq q = res_seq_of(st.seq + (size_t)s * 8);
    if (!res_seq_ok(q, st.n_tab, st.n_det, st.n_off)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&W.bits[s], (unsigned)FLAG_STORE);
        return;
    }
    if (q.n_det == 0) return;
    const unsigned mask = (unsigned)q.n_tab - 1u;
    const int shift = 32 - (63 - __builtin_clzll((unsigned long long)q.n_tab));        // n_tab = 2^k, 1 <= k <= 30
    unsigned* const key = W.tab_key + q.tab_base;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < q.n_det; i += (int64_t)gridDim.x * RS_THREADS) {
        const int id = tracks[q.det_base + i];
        int slot = -1;
        if (id < -1) atomicOr(&W.bits[s], (unsigned)FLAG_NEGATIVE);
        if (id >= 0) {
            const int c = st.det_cat[q.det_base + i];
            if (c < 0 || c >= st.n_cat) {
                atomicOr(&W.bits[s], (unsigned)FLAG_STORE);
            } else {
                const unsigned want = (unsigned)id + 1u;
                unsigned h = (((unsigned)id * 0x9E3779B1u) >> shift) & mask;
                for (int64_t probe = 0; probe < q.n_tab; ++probe) {      // (a table of >= 2 n_det slots always has a free one)
                    const unsigned old = atomicCAS(&key[h], 0u, want);
                    if (old == 0u || old == want) { slot = (int)h; break; }
                    h = (h + 1u) & mask;
                }
                if (slot < 0) {
                    atomicOr(&W.bits[s], (unsigned)FLAG_STORE);
                } else {
                    atomicMax(&W.tab_cat[q.tab_base + slot], c);
                    atomicMax(&W.tab_score[q.tab_base + slot], st.det_key[q.det_base + i]);
                    atomicAdd(&W.tab_rows[q.tab_base + slot], 1);
                }
            }
        }
        W.slot[q.det_base + i] = slot;
    }
}

// whether the filter removes the track of a claimed slot (tab_cat holds categories that k_res_group checked against n_cat)
__device__ __forceinline__ bool res_removed(const tmpnn_result_store& st, const ResWs& W, int64_t at) {
    return W.tab_score[at] < st.thr_key[W.tab_cat[at]];
}

__global__ __launch_bounds__(RS_THREADS) void k_res_filter(tmpnn_result_store st, const int32_t* __restrict__ tracks, ResWs W,
                                                           int32_t* __restrict__ filtered) {
    const int s = blockIdx.y;
    const ResSeq q = res_seq_of(st.seq + (size_t)s * 8);
    if (!res_seq_ok(q, st.n_tab, st.n_det, st.n_off)) return;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < q.n_det; i += (int64_t)gridDim.x * RS_THREADS) {
        const int slot = W.slot[q.det_base + i];
        int id = tracks[q.det_base + i];
        if (slot >= 0 && slot < q.n_tab && res_removed(st, W, q.tab_base + slot)) id = -1;
        filtered[q.det_base + i] = id;
    }
}

__global__ __launch_bounds__(RS_THREADS) void k_res_dups(tmpnn_result_store st, const int32_t* __restrict__ filtered, ResWs W) {
    const int s = blockIdx.y;
    const ResSeq q = res_seq_of(st.seq + (size_t)s * 8);
    if (!res_seq_ok(q, st.n_tab, st.n_det, st.n_off)) return;
    const int32_t* const perm = st.det_perm + q.det_base;
    const int32_t* const ids = filtered + q.det_base;
    for (int64_t p = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; p < q.n_det; p += (int64_t)gridDim.x * RS_THREADS) {
        const int a = perm[p], f = st.det_fidx[q.det_base + p];
        if (a < 0 || a >= q.n_det || f < 0 || f >= q.n_frames) { atomicOr(&W.bits[s], (unsigned)FLAG_STORE); continue; }
        const int lo = st.det_off[q.off_base + f];
        if (lo < 0 || lo > p) { atomicOr(&W.bits[s], (unsigned)FLAG_STORE); continue; }
        const int id = ids[a];
        if (id < 0) continue;
        for (int64_t j = lo; j < p; ++j) {
            const int b = perm[j];
            if (b < 0 || b >= q.n_det) { atomicOr(&W.bits[s], (unsigned)FLAG_STORE); break; }
            if (ids[b] == id) { atomicMax(&W.dup[s], RS_DUP_TOP - (unsigned long long)(f + 1)); break; }
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void k_res_compact(tmpnn_result_store st, const int32_t* __restrict__ filtered, ResWs W,
                                                            tmpnn_result_record* __restrict__ out, int32_t* __restrict__ order) {
    __shared__ int s_wave[RS_WAVES + 1];
    __shared__ long long s_sum[RS_WAVES][3];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ResSeq q = res_seq_of(st.seq + (size_t)s * 8);
    tmpnn_result_record r = {};
    if (!res_seq_ok(q, st.n_tab, st.n_det, st.n_off)) {       // (uniform over the workgroup)
        r.flag = FLAG_STORE;
        if (tid == 0) out[s] = r;
        return;
    }
    const int32_t* const perm = st.det_perm + q.det_base;
    const int32_t* const ids = filtered + q.det_base;
    int32_t* const ord = order + q.det_base;
    int64_t carry = 0;
    for (int64_t base = 0; base < q.n_det; base += RS_SPAN) {
        int a[RS_ITEMS], cnt = 0;
#pragma unroll
        for (int k = 0; k < RS_ITEMS; ++k) {
            const int64_t p = base + (int64_t)tid * RS_ITEMS + k;
            a[k] = -1;
            if (p < q.n_det) {
                const int v = perm[p];
                if (v >= 0 && v < q.n_det && ids[v] != -1) { a[k] = v; ++cnt; }
            }
        }
        int total;
        int64_t at = carry + block_scan<RS_THREADS>(cnt, s_wave, &total);
#pragma unroll
        for (int k = 0; k < RS_ITEMS; ++k)
            if (a[k] >= 0) ord[at++] = a[k];
        carry += total;
    }
    for (int64_t p = carry + tid; p < q.n_det; p += RS_THREADS) ord[p] = -1;
    long long kept_t = 0, rem_t = 0, rem_r = 0;
    for (int64_t j = tid; j < q.n_tab; j += RS_THREADS) {
        const int64_t at = q.tab_base + j;
        if (W.tab_key[at] == 0u) continue;
        if (res_removed(st, W, at)) { ++rem_t; rem_r += W.tab_rows[at]; } else { ++kept_t; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        kept_t += __shfl_down(kept_t, off);
        rem_t += __shfl_down(rem_t, off);
        rem_r += __shfl_down(rem_r, off);
    }
    if (lane == 0) { s_sum[wave][0] = kept_t; s_sum[wave][1] = rem_t; s_sum[wave][2] = rem_r; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < RS_WAVES; ++w) { r.kept_tracks += s_sum[w][0]; r.removed_tracks += s_sum[w][1]; r.removed_rows += s_sum[w][2]; }
        r.kept_rows = carry;
        const unsigned long long d = W.dup[s];
        r.flag = (int64_t)W.bits[s];
        if (d != 0ull) r.flag |= FLAG_DUPLICATE | (int64_t)((RS_DUP_TOP - d) << 8);
        out[s] = r;
    }
}

// carves the workspace; *cleared: the bytes from the start that every call clears
char* res_carve(char* p, int S, int64_t n_det, int64_t n_tab, ResWs& w, size_t* cleared) {
    WsCarver c{p};
    w.tab_key = c.take<unsigned>((size_t)n_tab);
    w.tab_cat = c.take<int>((size_t)n_tab);
    w.tab_score = c.take<unsigned>((size_t)n_tab);
    w.tab_rows = c.take<int>((size_t)n_tab);
    w.dup = c.take<unsigned long long>((size_t)S);
    w.bits = c.take<unsigned>((size_t)S);
    *cleared = (size_t)(c.p - p);
    w.slot = c.take<int>((size_t)n_det);
    return c.p;
}

}  // namespace

extern "C" size_t tmpnn_results_ws(int S, int64_t n_det, int64_t n_tab) {
    if (S < 0 || S > RS_MAX_SEQ || n_det < 0 || n_tab < 0 || n_det >= ((int64_t)1 << 31) || n_tab >= ((int64_t)1 << 34)) return 0;
    ResWs w;
    size_t cleared;
    char* const base = reinterpret_cast<char*>((uintptr_t)16);       // (only the distance is used)
    return (size_t)(res_carve(base, S, n_det, n_tab, w, &cleared) - base);
}

extern "C" int tmpnn_results_apply(const tmpnn_result_store* st, const int64_t* seq_host, const int32_t* tracks, void* ws, size_t ws_bytes,
                                   tmpnn_result_record* out, int32_t* filtered, int32_t* order, tmpnn_stream stream) {
    TM_REQUIRE(st != nullptr, "results_apply: store is null");
    TM_REQUIRE(st->S >= 0 && st->S <= RS_MAX_SEQ && st->n_cat >= 1 && st->n_det >= 0 && st->n_off >= 0 && st->n_tab >= 0,
               "results_apply: S=%d (at most %d) n_cat=%d n_det=%lld n_off=%lld n_tab=%lld", st->S, RS_MAX_SEQ, st->n_cat, (long long)st->n_det,
               (long long)st->n_off, (long long)st->n_tab);
    if (st->S == 0) return TMPNN_OK;
    TM_REQUIRE(seq_host && st->seq && out && st->thr_key, "results_apply: null pointer (seq, seq_host, thr_key or out)");
    TM_REQUIRE(st->n_off == 0 || st->det_off, "results_apply: null offsets");
    TM_REQUIRE(st->n_det == 0 || (st->det_perm && st->det_fidx && st->det_cat && st->det_key && tracks && filtered && order),
               "results_apply: null detection arrays, tracks or outputs");
    int64_t max_det = 0;
    for (int s = 0; s < st->S; ++s) {
        const ResSeq q = res_seq_of(seq_host + (size_t)s * 8);
        TM_REQUIRE(res_seq_ok(q, st->n_tab, st->n_det, st->n_off),
                   "results_apply: sequence %d: table [%lld, +%lld) of %lld, rows [%lld, +%lld) of %lld, offsets [%lld, +%lld + 1) of %lld "
                   "(a table is a power of two of at least twice the rows)", s, (long long)q.tab_base, (long long)q.n_tab, (long long)st->n_tab,
                   (long long)q.det_base, (long long)q.n_det, (long long)st->n_det, (long long)q.off_base, (long long)q.n_frames, (long long)st->n_off);
        max_det = q.n_det > max_det ? q.n_det : max_det;
    }
    const size_t need = tmpnn_results_ws(st->S, st->n_det, st->n_tab);
    TM_REQUIRE(need > 0, "results_apply: the store is beyond the workspace's limits");
    if (ws == nullptr || ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "results_apply: workspace %zu < %zu bytes", ws_bytes, need);
    TM_REQUIRE(aligned16(ws) && (reinterpret_cast<uintptr_t>(out) & 7u) == 0, "results_apply: workspace must be 16-byte, out 8-byte aligned");
    ResWs w;
    size_t cleared;
    res_carve(static_cast<char*>(ws), st->S, st->n_det, st->n_tab, w, &cleared);
    hipStream_t hs = as_stream(stream);
    const hipError_t e = hipMemsetAsync(ws, 0, cleared, hs);
    if (e != hipSuccess) return set_error(TMPNN_ELAUNCH, "results_apply: clearing the workspace: %s", hipGetErrorString(e));
    int gx = ceil_div(max_det, RS_THREADS);
    gx = gx < 1 ? 1 : (gx > RS_MAX_BLOCKS ? RS_MAX_BLOCKS : gx);
    const dim3 rows(gx, st->S);
    hipLaunchKernelGGL(k_res_group, rows, dim3(RS_THREADS), 0, hs, *st, tracks, w);
    if (const int rc = check_launch("results_apply (grouping)")) return rc;
    hipLaunchKernelGGL(k_res_filter, rows, dim3(RS_THREADS), 0, hs, *st, tracks, w, filtered);
    if (const int rc = check_launch("results_apply (filter)")) return rc;
    hipLaunchKernelGGL(k_res_dups, rows, dim3(RS_THREADS), 0, hs, *st, filtered, w);
    if (const int rc = check_launch("results_apply (duplicates)")) return rc;
    hipLaunchKernelGGL(k_res_compact, dim3(st->S), dim3(RS_THREADS), 0, hs, *st, filtered, w, out, order);
    return check_launch("results_apply (compaction)");
}
