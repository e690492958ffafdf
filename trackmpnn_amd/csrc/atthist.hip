// Attention monitor: per head, the histogram of the attention weights detections give to correct and to incorrect associations,
// counted on the device in ONE launch per forward and head group (reference attention_weights.py:84-93 walks the dense [N, N]
// matrices of every stored forward on the host; :99-105 histograms the two lists with bins = 25, range = (0, 1)).
//
// What the dense walk selects, on the CSR form the attention kernels write (alpha [K][stride], position p of det d's run):
//   * a det with incident edges gives each of them its softmax weight alpha[k][p]; every other column of its dense row is an
//     exact 0 and fails the walk's `> 0` test, as does an alpha that underflowed to 0;
//   * a det WITHOUT incident edges has the uniform dense row 1 / N (a softmax over an all-masked row): it gives 1 / N to every
//     edge row of the graph;
//   * the value goes to `tp` where the edge row's label is 1 (equality, not `non-zero`), to `fp` otherwise.
// The launch:
//   1. dets are scanned for empty CSR runs (n_iso) and the edge rows for label 1 (n_pos), once;
//   2. threads stride over the CSR positions p < 2E (coalesced reads of inc and of every head's alpha row), AH_UNROLL blocks of
//      the workgroup per trip with clamped indices; the bin is min(int(v * bins), bins - 1) corrected down / up against the
//      UPLOADED float32 edge table -- np.histogram's own rule, so a value that sits exactly on an edge lands where numpy puts it;
//      the last bin is closed; counts go to an LDS histogram int32 [Kg][2][bins] with integer LDS atomics;
//   3. one thread per head adds n_iso * n_pos / n_iso * (E - n_pos) to the tp / fp cell of the bin of 1.0f / (float)N (IEEE
//      division, numpy's float32(1) / float32(N));
//   4. one thread per cell adds the LDS histogram into the int64 record: a single workgroup, stream-ordered -- plain adds.
// E, Dn and the status are read from the graph's meta ON THE DEVICE, as k_val_f1_count does.  Integer work only: exact and
// repeatable.
#include "common.h"

namespace tmpnn {

static constexpr int AH_THREADS = 1024;                          // one graph: one workgroup of 16 waves
static constexpr int AH_UNROLL = 4;
static constexpr int AH_KMAX = TMPNN_ATT_HIST_KMAX;
static constexpr int AH_BINS = TMPNN_ATT_HIST_MAX_BINS;
static constexpr int AH_HEADER = TMPNN_ATT_HIST_HEADER;
static_assert(sizeof(tmpnn_att_record) == AH_HEADER * sizeof(int64_t), "the histogram follows the header");

__device__ inline int ah_clamp_row(int row, int N) { return row < 0 ? 0 : (row < N ? row : N - 1); }

// the bin of v in (0, e[bins]]: the largest b with e[b] <= v, the last bin closed (np.histogram on a uniform range: an estimate,
// then one step down where v < e[b] and one step up where v >= e[b + 1])
__device__ inline int ah_bin(float v, const float* e, int bins) {
    int b = (int)(v * (float)bins);
    b = b < 0 ? 0 : (b > bins - 1 ? bins - 1 : b);
    while (b > 0 && v < e[b]) --b;
    while (b < bins - 1 && v >= e[b + 1]) ++b;
    return b;
}

__global__ __launch_bounds__(AH_THREADS) void k_att_hist_count(tmpnn_dgraph g, const uint8_t* __restrict__ labels,
                                                               const float* __restrict__ alpha, long stride, int Kg, int k0,
                                                               const float* __restrict__ edges, int bins,
                                                               tmpnn_att_record* __restrict__ rec, int count_forward) {
    __shared__ int s_h[AH_KMAX * 2 * AH_BINS];
    __shared__ float s_e[AH_BINS + 1];
    __shared__ int s_n[3];                                       // isolated dets, label-1 edge rows, values skipped as zero
    const int tid = threadIdx.x, N = g.N;
    int E = g.meta[0], Dn = g.meta[1];
    // an invalid graph is presented as empty (tmpnn_dgraph); sizes that are not those of a graph of N rows are treated alike,
    // and so is an alpha buffer whose rows are shorter than the graph's 2E positions
    if (g.meta[2] != 0 || E < 0 || Dn < 0 || (long)E + Dn > N || 2L * E > stride) E = Dn = 0;
    if (E + Dn == 0) return;                                     // no rows: not a forward
    const int cells = Kg * 2 * bins;
    for (int i = tid; i < cells; i += AH_THREADS) s_h[i] = 0;
    if (tid <= bins) s_e[tid] = edges[tid];
    if (tid < 3) s_n[tid] = 0;
    __syncthreads();
    const int P = 2 * E;
    // ---- 1. isolated dets and label-1 edge rows
    int iso = 0, pos = 0;
    for (int d = tid; d < Dn; d += AH_THREADS) iso += g.rowptr[d] == g.rowptr[d + 1];
    for (int e = tid; e < E; e += AH_THREADS) pos += labels[ah_clamp_row(g.edge_row[e], N)] == 1;
    if (iso) atomicAdd(&s_n[0], iso);
    if (pos) atomicAdd(&s_n[1], pos);
    // ---- 2. the informative weights, a thread per CSR position
    int zeros = 0;
    for (long base = tid; base < P; base += (long)AH_THREADS * AH_UNROLL) {
        long p[AH_UNROLL];
        int row[AH_UNROLL];
        uint8_t lab[AH_UNROLL];
#pragma unroll
        for (int u = 0; u < AH_UNROLL; ++u) {
            const long i = base + (long)u * AH_THREADS;
            p[u] = i < P ? i : P - 1;
            row[u] = ah_clamp_row(g.inc[p[u]] & 0x7fffffff, N);
        }
#pragma unroll
        for (int u = 0; u < AH_UNROLL; ++u) lab[u] = labels[row[u]];
        for (int k = 0; k < Kg; ++k) {
            const float* a = alpha + (long)k * stride;
            float v[AH_UNROLL];
#pragma unroll
            for (int u = 0; u < AH_UNROLL; ++u) v[u] = a[p[u]];
#pragma unroll
            for (int u = 0; u < AH_UNROLL; ++u) {
                if (base + (long)u * AH_THREADS >= P) continue;
                if (!(v[u] > 0.0f)) {
                    ++zeros;
                    continue;
                }
                if (v[u] > s_e[bins]) continue;
                atomicAdd(&s_h[(k * 2 + (lab[u] == 1 ? 0 : 1)) * bins + ah_bin(v[u], s_e, bins)], 1);
            }
        }
    }
    if (zeros) atomicAdd(&s_n[2], zeros);
    __syncthreads();
    // ---- 3. the uniform rows of the isolated dets: 1 / N once for every edge row, split by its label
    const int n_iso = s_n[0], n_pos = s_n[1];
    if (tid < Kg && n_iso > 0 && E > 0) {
        const float u = 1.0f / (float)N;
        if (u <= s_e[bins]) {
            const int b = ah_bin(u, s_e, bins);
            s_h[(tid * 2 + 0) * bins + b] += n_iso * n_pos;       // (n_iso + E <= N <= 32768: the products fit an int32)
            s_h[(tid * 2 + 1) * bins + b] += n_iso * (E - n_pos);
        }
    }
    __syncthreads();
    // ---- 4. into the record
    int64_t* hist = reinterpret_cast<int64_t*>(rec) + AH_HEADER + (long)k0 * 2 * bins;
    for (int i = tid; i < cells; i += AH_THREADS)
        if (s_h[i]) hist[i] += s_h[i];
    if (tid == 0) {
        if (count_forward) {
            rec->forwards += 1;
            rec->dets += Dn;
            rec->isolated += n_iso;
        }
        rec->zeros += s_n[2];
    }
}

}  // namespace tmpnn

using namespace tmpnn;

extern "C" {

int tmpnn_att_hist_count(const tmpnn_dgraph* g, const uint8_t* labels, const float* alpha, int64_t stride, int heads, int first_head,
                         const float* edges, int bins, tmpnn_att_record* rec, int count_forward, tmpnn_stream stream) {
    TM_REQUIRE(g != nullptr, "att_hist_count: graph is null");
    TM_REQUIRE(rec != nullptr, "att_hist_count: record is null");
    TM_REQUIRE(g->N >= 0 && g->N <= TMPNN_TRACK_MAX_ROWS && g->cap >= g->N, "att_hist_count: N=%d cap=%d (at most %d rows)", g->N,
               g->cap, TMPNN_TRACK_MAX_ROWS);
    TM_REQUIRE(heads >= 1 && heads <= AH_KMAX && first_head >= 0, "att_hist_count: heads=%d first_head=%d (1..%d heads per launch)",
               heads, first_head, AH_KMAX);
    TM_REQUIRE(bins >= 1 && bins <= AH_BINS, "att_hist_count: bins=%d (1..%d)", bins, AH_BINS);
    TM_REQUIRE(stride >= 1, "att_hist_count: stride=%lld", (long long)stride);
    if (g->N == 0) return TMPNN_OK;                              // no rows: not a forward
    TM_REQUIRE(g->meta && g->edge_row && g->rowptr && g->inc, "att_hist_count: the graph's arrays are null");
    TM_REQUIRE(labels && alpha && edges, "att_hist_count: labels / alpha / edges are null");
    hipLaunchKernelGGL(k_att_hist_count, dim3(1), dim3(AH_THREADS), 0, as_stream(stream), *g, labels, alpha, (long)stride, heads,
                       first_head, edges, bins, rec, count_forward ? 1 : 0);
    return check_launch("att_hist_count");
}

}  // extern "C"
