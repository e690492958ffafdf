// Validation monitor: the F1 of every forward call of the validation pass, counted on the device in ONE launch per forward
// (reference train.py:207-219 / :241-253: targets = create_targets(labels, node_adj, idx_node), pred = argmax((1 - score, score)),
// f1_score(targets[idx], pred[idx], zero_division=0); train.py:278 logs the mean over the forwards).
//
// The launch does what the training side does in three (k_targets of loss.hip, k_cls_counts and the record fold of monitor.hip):
//   1. targets from the labels: per det, over its CSR run in ascending edge row, the LAST label-positive past edge (sign bit
//      set) and the FIRST label-positive future edge are chosen.  The chosen edge rows are a BITMAP in the LDS -- one bit per
//      row, TMPNN_TRACK_MAX_ROWS bits = 4 KB, set with integer LDS atomics (an edge chosen by both endpoints is one bit) --
//      never an array in HBM.  Row r is bit (r >> 10) of word (r & 1023): the ascending edge rows a wave counts in step 3 sit in
//      consecutive words, i.e. 32 lanes of a half wave on 32 banks, and the rows the dets of a wave choose spread the same way.
//   2. tp / fp / fn with pred = score > 0.5f (strict: argmax's tie goes to class 0) over the edge rows against the bitmap and,
//      with the TP classifier, over the det rows against their labels: a ballot and a popcount per 64 rows, the waves' totals
//      combined in wave order.
//   3. one thread folds the forward into the record: F1 = 2 tp / (2 tp + fp + fn) in fp64, 0 where the denominator is 0.
// E, Dn and the status are read from the graph's meta ON THE DEVICE (the native driver enqueues the launch before any host knows
// them).  Integer counts, one fp64 addition per launch by one thread, no float atomics: exact and repeatable.
#include "common.h"

namespace tmpnn {

static constexpr int VM_THREADS = 1024;                          // one graph: one workgroup of 16 waves
static constexpr int VM_UNROLL = 4;
static constexpr int VM_SHIFT = 10;
static constexpr int VM_WORDS = 1 << VM_SHIFT;                   // bitmap words
static_assert(VM_WORDS * 32 == TMPNN_TRACK_MAX_ROWS, "the bitmap holds one bit per tracker row");
static_assert(VM_WORDS == VM_THREADS, "every thread clears one word");

__device__ inline int vm_clamp_row(int row, int N) { return row < 0 ? 0 : (row < N ? row : N - 1); }

// tp / fp / fn of rows[i], i < R, into the (wave-uniform) c[3]; every lane of the workgroup calls it.  EDGE: the target is the
// row's bit of the bitmap; else the row's label.  VM_UNROLL blocks of 64 rows per trip with clamped indices (monitor.hip
// cc_accumulate): the dependent loads row list -> score / label go out VM_UNROLL at a time, not one memory latency each.
template <bool EDGE>
__device__ inline void vm_accumulate(const int32_t* __restrict__ rows, int R, int N, const float* __restrict__ scores,
                                     const uint8_t* __restrict__ labels, const uint32_t* bm, int c[3]) {
    const int lane = threadIdx.x & 63, first = (threadIdx.x >> 6) * 64;
    for (long base = first; base < R; base += (long)VM_THREADS * VM_UNROLL) {
        int row[VM_UNROLL];
        float s[VM_UNROLL];
        uint8_t t8[VM_UNROLL];
#pragma unroll
        for (int u = 0; u < VM_UNROLL; ++u) {
            const long i = base + (long)u * VM_THREADS + lane;
            row[u] = vm_clamp_row(rows[i < R ? i : R - 1], N);
        }
#pragma unroll
        for (int u = 0; u < VM_UNROLL; ++u) {
            s[u] = scores[row[u]];
            t8[u] = EDGE ? 0 : labels[row[u]];
        }
#pragma unroll
        for (int u = 0; u < VM_UNROLL; ++u) {
            const bool live = base + (long)u * VM_THREADS + lane < R;
            const bool hit = EDGE ? ((bm[row[u] & (VM_WORDS - 1)] >> (row[u] >> VM_SHIFT)) & 1u) != 0 : t8[u] != 0;
            const bool pred = live && s[u] > 0.5f, t = live && hit;
            c[0] += __popcll(__ballot(pred && t));
            c[1] += __popcll(__ballot(pred && !t));
            c[2] += __popcll(__ballot(live && !pred && t));
        }
    }
}

__global__ __launch_bounds__(VM_THREADS) void k_val_f1_count(tmpnn_dgraph g, const uint8_t* __restrict__ labels,
                                                             const float* __restrict__ scores, int tp,
                                                             tmpnn_val_record* __restrict__ rec, int32_t* __restrict__ log,
                                                             int log_cap) {
    __shared__ uint32_t s_bm[VM_WORDS];
    __shared__ int s_c[VM_THREADS / 64][3];
    const int tid = threadIdx.x, N = g.N;
    int E = g.meta[0], Dn = g.meta[1];
    // an invalid graph is presented as empty (tmpnn_dgraph); sizes that are not those of a graph of N rows are treated alike
    if (g.meta[2] != 0 || E < 0 || Dn < 0 || (long)E + Dn > N) E = Dn = 0;
    if (E + Dn == 0) return;                                     // no rows: not a forward
    s_bm[tid] = 0;
    __syncthreads();
    // ---- 1. the chosen edges (create_targets as loss.hip k_targets states it), a thread per det
    const int P = 2 * E;
    for (int d = tid; d < Dn; d += VM_THREADS) {
        int p0 = g.rowptr[d], p1 = g.rowptr[d + 1];
        p0 = p0 < 0 ? 0 : p0;
        p1 = p1 > P ? P : p1;
        int last_past = -1, first_future = -1;
        for (int p = p0; p < p1; p += VM_UNROLL) {
            int v[VM_UNROLL];
            uint8_t l[VM_UNROLL];
#pragma unroll
            for (int u = 0; u < VM_UNROLL; ++u) v[u] = g.inc[p + u < p1 ? p + u : p1 - 1];
#pragma unroll
            for (int u = 0; u < VM_UNROLL; ++u) l[u] = labels[vm_clamp_row(v[u] & 0x7fffffff, N)];
#pragma unroll
            for (int u = 0; u < VM_UNROLL; ++u) {
                if (p + u >= p1 || !l[u]) continue;
                const int row = vm_clamp_row(v[u] & 0x7fffffff, N);
                if (v[u] < 0) last_past = row;
                else if (first_future < 0) first_future = row;
            }
        }
        if (last_past >= 0) atomicOr(&s_bm[last_past & (VM_WORDS - 1)], 1u << (last_past >> VM_SHIFT));
        if (first_future >= 0) atomicOr(&s_bm[first_future & (VM_WORDS - 1)], 1u << (first_future >> VM_SHIFT));
    }
    __syncthreads();
    // ---- 2. the counts
    int c[3] = {0, 0, 0};
    vm_accumulate<true>(g.edge_row, E, N, scores, labels, s_bm, c);
    if (tp) vm_accumulate<false>(g.det_row, Dn, N, scores, labels, s_bm, c);
    if ((tid & 63) == 0)
        for (int k = 0; k < 3; ++k) s_c[tid >> 6][k] = c[k];
    __syncthreads();
    // ---- 3. the forward into the record
    if (tid == 0) {
        long long n[3] = {0, 0, 0};
        for (int w = 0; w < VM_THREADS / 64; ++w)
            for (int k = 0; k < 3; ++k) n[k] += s_c[w][k];
        const long long tp2 = 2 * n[0], den = tp2 + n[1] + n[2];
        const int64_t before = rec->forwards;
        rec->sum_f1 += den > 0 ? (double)tp2 / (double)den : 0.0;   // zero_division = 0
        rec->forwards = before + 1;
        rec->tp += n[0];
        rec->fp += n[1];
        rec->fn += n[2];
        rec->rows += E + Dn;
        if (log != nullptr) {
            int32_t* q = log + 4 * (before < log_cap - 1 ? before : (int64_t)log_cap - 1);
            q[0] = (int32_t)n[0];
            q[1] = (int32_t)n[1];
            q[2] = (int32_t)n[2];
            q[3] = E + Dn;
        }
    }
}

}  // namespace tmpnn

using namespace tmpnn;

extern "C" {

int tmpnn_val_f1_count(const tmpnn_dgraph* g, const uint8_t* labels, const float* scores, int tp_classifier,
                       tmpnn_val_record* rec, int32_t* log, int log_cap, tmpnn_stream stream) {
    TM_REQUIRE(g != nullptr, "val_f1_count: graph is null");
    TM_REQUIRE(rec != nullptr, "val_f1_count: record is null");
    TM_REQUIRE(g->N >= 0 && g->N <= TMPNN_TRACK_MAX_ROWS && g->cap >= g->N, "val_f1_count: N=%d cap=%d (at most %d rows)", g->N,
               g->cap, TMPNN_TRACK_MAX_ROWS);
    TM_REQUIRE(log == nullptr || log_cap >= 1, "val_f1_count: log_cap=%d", log_cap);
    if (g->N == 0) return TMPNN_OK;                              // no rows: not a forward
    TM_REQUIRE(g->meta && g->edge_row && g->det_row && g->rowptr && g->inc, "val_f1_count: the graph's arrays are null");
    TM_REQUIRE(labels && scores, "val_f1_count: labels / scores are null");
    hipLaunchKernelGGL(k_val_f1_count, dim3(1), dim3(VM_THREADS), 0, as_stream(stream), *g, labels, scores,
                       tp_classifier ? 1 : 0, rec, log, log_cap);
    return check_launch("val_f1_count");
}

}  // extern "C"
