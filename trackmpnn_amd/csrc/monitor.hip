// Training monitor: the classification counts of every forward call and the running statistics of an epoch, on the device
// (reference train.py:86-88 / :125-127: pred = argmax(1 - score, score), f1_score(targets[idx], pred[idx], zero_division=0)
// per forward; train.py:157-171: the mean F1 over the forwards and the means of loss_c, loss_f, loss over the chunks).
//
// pred = score > 0.5f (strict: argmax's tie goes to class 0).  Rows S of a forward: its det and edge rows with the TP
// classifier, its edge rows alone without.  A counts record is four int32 -- tp, fp, fn over S, and `rows` = det + edge rows
// of the graph (window) in either mode; rows > 0 is what makes a (call, window) pair a forward.  The counts are integers
// (a ballot and a popcount per 64 rows, the waves' totals combined in wave order); the fold's fp64 sums run in a fixed order
// (each thread its strided terms in sequence, then a fixed tree), with no atomics anywhere: two runs give the same bits.
#include "common.h"

namespace tmpnn {

static constexpr int CC_THREADS = 1024;     // one graph: one workgroup of 16 waves
static constexpr int CCW_THREADS = 64;      // one window: one wave
static constexpr int CC_UNROLL = 4;
static constexpr int FOLD_THREADS = 1024;
static constexpr int FOLD_UNROLL = 8;

// tp / fp / fn of the listed rows rows[list[i]], i < R, accumulated into the (wave-uniform) c[3]; every lane of the wave calls it.
// CC_UNROLL blocks of 64 rows per trip, their indices clamped instead of guarded: the three dependent loads of a row (list,
// row, score / target) go out CC_UNROLL at a time instead of one memory latency each per 64 rows.
template <bool LISTED>
__device__ inline void cc_accumulate(const int32_t* __restrict__ rows, const int32_t* __restrict__ list, int R, int first,
                                     int stride, const float* __restrict__ scores, const uint8_t* __restrict__ targets,
                                     int c[3]) {
    const int lane = threadIdx.x & 63;
    for (long base = first; base < R; base += (long)stride * CC_UNROLL) {
        int idx[CC_UNROLL], row[CC_UNROLL];
        float s[CC_UNROLL];
        uint8_t t8[CC_UNROLL];
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) {
            const long i = base + (long)u * stride + lane;
            idx[u] = (int)(i < R ? i : R - 1);
            if (LISTED) idx[u] = list[idx[u]];
        }
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) row[u] = rows[idx[u]];
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) {
            s[u] = scores[row[u]];
            t8[u] = targets[row[u]];
        }
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) {
            const bool live = base + (long)u * stride + lane < R;
            const bool pred = live && s[u] > 0.5f, t = live && t8[u] != 0;
            c[0] += __popcll(__ballot(pred && t));
            c[1] += __popcll(__ballot(pred && !t));
            c[2] += __popcll(__ballot(live && !pred && t));
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void k_cls_counts(tmpnn_graph g, const float* __restrict__ scores,
                                                           const uint8_t* __restrict__ targets, int tp,
                                                           int32_t* __restrict__ counts) {
    __shared__ int s_c[CC_THREADS / 64][3];
    const int wave = threadIdx.x >> 6;
    int c[3] = {0, 0, 0};
    cc_accumulate<false>(g.edge_row, nullptr, g.E, wave * 64, CC_THREADS, scores, targets, c);
    if (tp) cc_accumulate<false>(g.det_row, nullptr, g.Dn, wave * 64, CC_THREADS, scores, targets, c);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) s_c[wave][k] = c[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        int v = 0;
        for (int w = 0; w < CC_THREADS / 64; ++w) v += s_c[w][threadIdx.x];
        counts[threadIdx.x] = v;
    }
    if (threadIdx.x == 3) counts[3] = g.E + g.Dn;
}

// one wave per window over the lists k_train_losses_win_fwd walks; counts [4][W]
__global__ __launch_bounds__(CCW_THREADS) void k_cls_counts_win(tmpnn_graph g, tmpnn_loss_windows lw,
                                                                const float* __restrict__ scores,
                                                                const uint8_t* __restrict__ targets, int tp,
                                                                int32_t* __restrict__ counts) {
    const int w = blockIdx.x;
    const int d0 = lw.det_ptr[w], Dn = lw.det_ptr[w + 1] - d0;
    const int e0 = lw.edge_ptr[w], E = lw.edge_ptr[w + 1] - e0;
    int c[3] = {0, 0, 0};
    cc_accumulate<true>(g.edge_row, lw.edge_idx + e0, E, 0, CCW_THREADS, scores, targets, c);
    if (tp) cc_accumulate<true>(g.det_row, lw.det_idx + d0, Dn, 0, CCW_THREADS, scores, targets, c);
    if (threadIdx.x < 4) counts[(size_t)threadIdx.x * lw.W + w] = threadIdx.x < 3 ? c[threadIdx.x] : E + Dn;
}

// the sum of every thread's v over the workgroup, by a fixed tree over s [FOLD_THREADS]
template <typename T>
__device__ inline T fold_tree(T v, T* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int half = FOLD_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    const T r = s[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(FOLD_THREADS) void k_train_record_fold(const int32_t* __restrict__ counts, int C, int W,
                                                                    const float* __restrict__ loss_c,
                                                                    const float* __restrict__ loss_f, int B,
                                                                    tmpnn_train_record* __restrict__ rec) {
    __shared__ double s_d[FOLD_THREADS];
    __shared__ long long s_n[FOLD_THREADS];
    const int tid = threadIdx.x;
    double f1 = 0.0;
    long long fwd = 0;
    // (one workgroup: the loads of FOLD_UNROLL records are issued before the first is used -- taken one pair at a time the loop
    //  costs two memory latencies per pair, 118 us at C x W = 6 x 16384; a thread still takes its pairs in ascending (c, w))
    for (int c = 0; c < C; ++c) {
        const int32_t* q = counts + (size_t)c * 4 * W;
        for (long w0 = tid; w0 < W; w0 += FOLD_THREADS * FOLD_UNROLL) {
            int a[FOLD_UNROLL][4];
#pragma unroll
            for (int u = 0; u < FOLD_UNROLL; ++u) {
                const long w = w0 + u * FOLD_THREADS;
                const long wl = w < W ? w : W - 1;                         // (clamped: unconditional loads, back to back)
#pragma unroll
                for (int k = 0; k < 4; ++k) a[u][k] = q[k * (size_t)W + wl];
                if (w >= W) a[u][3] = 0;
            }
#pragma unroll
            for (int u = 0; u < FOLD_UNROLL; ++u) {
                if (a[u][3] <= 0) continue;                                // no rows: not a forward
                const long long tp2 = 2ll * a[u][0];
                const long long den = tp2 + a[u][1] + a[u][2];
                f1 += den > 0 ? (double)tp2 / (double)den : 0.0;           // zero_division = 0
                ++fwd;
            }
        }
    }
    double sc = 0.0, sf = 0.0, sl = 0.0;
    for (long b0 = tid; b0 < B; b0 += FOLD_THREADS * FOLD_UNROLL) {
        float lc[FOLD_UNROLL], lf[FOLD_UNROLL];
#pragma unroll
        for (int u = 0; u < FOLD_UNROLL; ++u) {
            const long b = b0 + u * FOLD_THREADS;
            const long bl = b < B ? b : B - 1;
            lc[u] = loss_c[bl];
            lf[u] = loss_f[bl];
        }
#pragma unroll
        for (int u = 0; u < FOLD_UNROLL; ++u) {
            const bool live = b0 + u * FOLD_THREADS < B;                   // (x + 0.0 == x: a select, no branch around the loads)
            const float l = lc[u] + lf[u];                                 // train.py:132-133 adds the two in fp32
            sc += live ? (double)lc[u] : 0.0;
            sf += live ? (double)lf[u] : 0.0;
            sl += live ? (double)l : 0.0;
        }
    }
    f1 = fold_tree(f1, s_d);
    sc = fold_tree(sc, s_d);
    sf = fold_tree(sf, s_d);
    sl = fold_tree(sl, s_d);
    fwd = fold_tree(fwd, s_n);
    if (tid == 0) {
        rec->sum_f1 += f1;
        rec->forwards += fwd;
        rec->sum_loss_c += sc;
        rec->sum_loss_f += sf;
        rec->sum_loss += sl;
        rec->chunks += B;
    }
}

__global__ __launch_bounds__(FOLD_THREADS) void k_train_embed_fold(const float* __restrict__ loss_d, int n_loss,
                                                                   const int64_t* __restrict__ kept, int n_kept,
                                                                   tmpnn_embed_record* __restrict__ rec) {
    __shared__ double s_d[FOLD_THREADS];
    __shared__ long long s_n[FOLD_THREADS];
    double sd = 0.0;
    long long n = 0, skipped = 0;
    for (long k = threadIdx.x; k < n_kept; k += FOLD_THREADS) {            // a thread takes its chunks in ascending order
        const long long b = kept ? (long long)kept[k] : (long long)k;
        if (b < 0 || b >= n_loss) { ++skipped; continue; }
        sd += (double)loss_d[b];
        ++n;
    }
    sd = fold_tree(sd, s_d);
    n = fold_tree(n, s_n);
    skipped = fold_tree(skipped, s_n);
    if (threadIdx.x == 0) {
        rec->sum_loss_d += sd;
        rec->chunks += n;
        rec->skipped += skipped;
    }
}

}  // namespace tmpnn

using namespace tmpnn;

extern "C" {

int tmpnn_cls_counts(const tmpnn_graph* g, const float* scores, const uint8_t* targets, int tp_classifier, int32_t* counts,
                     tmpnn_stream stream) {
    TM_REQUIRE(g != nullptr, "cls_counts: graph is null");
    TM_REQUIRE(counts != nullptr, "cls_counts: counts is null");
    TM_REQUIRE(g->N >= 0 && g->E >= 0 && g->Dn >= 0 && (long)g->E + g->Dn <= (long)g->N, "cls_counts: N=%d E=%d Dn=%d", g->N, g->E,
               g->Dn);
    TM_REQUIRE(g->E + g->Dn == 0 || (scores && targets), "cls_counts: scores / targets are null");
    TM_REQUIRE((g->E == 0 || g->edge_row) && (g->Dn == 0 || g->det_row), "cls_counts: the graph's row lists are null");
    hipLaunchKernelGGL(k_cls_counts, dim3(1), dim3(CC_THREADS), 0, as_stream(stream), *g, scores, targets, tp_classifier ? 1 : 0,
                       counts);
    return check_launch("cls_counts");
}

int tmpnn_cls_counts_win(const tmpnn_graph* g, const tmpnn_loss_windows* w, const float* scores, const uint8_t* targets,
                         int tp_classifier, int32_t* counts, tmpnn_stream stream) {
    TM_REQUIRE(g != nullptr, "cls_counts_win: graph is null");
    TM_REQUIRE(w != nullptr, "cls_counts_win: windows is null");
    TM_REQUIRE(w->W >= 0 && w->n_det >= 0 && w->n_edge >= 0 && w->n_det <= g->Dn && w->n_edge <= g->E,
               "cls_counts_win: W=%d n_det=%d n_edge=%d against Dn=%d E=%d", w->W, w->n_det, w->n_edge, g->Dn, g->E);
    if (w->W == 0) return TMPNN_OK;
    TM_REQUIRE(counts != nullptr, "cls_counts_win: counts is null");
    TM_REQUIRE(w->det_ptr && w->edge_ptr, "cls_counts_win: window pointers are null");
    TM_REQUIRE((w->n_det == 0 || (w->det_idx && g->det_row)) && (w->n_edge == 0 || (w->edge_idx && g->edge_row)),
               "cls_counts_win: window lists are null");
    TM_REQUIRE(w->n_det + w->n_edge == 0 || (scores && targets), "cls_counts_win: scores / targets are null");
    hipLaunchKernelGGL(k_cls_counts_win, dim3(w->W), dim3(CCW_THREADS), 0, as_stream(stream), *g, *w, scores, targets,
                       tp_classifier ? 1 : 0, counts);
    return check_launch("cls_counts_win");
}

int tmpnn_train_record_fold(const int32_t* counts, int C, int W, const float* loss_c, const float* loss_f, int B,
                            tmpnn_train_record* rec, tmpnn_stream stream) {
    TM_REQUIRE(rec != nullptr, "train_record_fold: record is null");
    TM_REQUIRE(C >= 0 && W >= 0 && B >= 0, "train_record_fold: C=%d W=%d B=%d", C, W, B);
    TM_REQUIRE((long)C * W == 0 || counts, "train_record_fold: counts is null");
    TM_REQUIRE(B == 0 || (loss_c && loss_f), "train_record_fold: loss_c / loss_f are null");
    if ((long)C * W == 0 && B == 0) return TMPNN_OK;
    hipLaunchKernelGGL(k_train_record_fold, dim3(1), dim3(FOLD_THREADS), 0, as_stream(stream), counts, C, W, loss_c, loss_f, B,
                       rec);
    return check_launch("train_record_fold");
}

int tmpnn_train_embed_fold(const float* loss_d, int n_loss, const int64_t* kept, int n_kept, tmpnn_embed_record* rec,
                           tmpnn_stream stream) {
    TM_REQUIRE(rec != nullptr, "train_embed_fold: record is null");
    TM_REQUIRE(n_loss >= 0 && n_kept >= 0, "train_embed_fold: n_loss=%d n_kept=%d", n_loss, n_kept);
    TM_REQUIRE(n_loss == 0 || loss_d, "train_embed_fold: loss_d is null");
    if (n_kept == 0) return TMPNN_OK;
    hipLaunchKernelGGL(k_train_embed_fold, dim3(1), dim3(FOLD_THREADS), 0, as_stream(stream), loss_d, n_loss, kept, n_kept, rec);
    return check_launch("train_embed_fold");
}

}  // extern "C"
