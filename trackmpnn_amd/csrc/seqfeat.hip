// Whole-sequence features from the device-resident detection store (struct tmpnn_seq_features_args, include/tmpnn.h; host
// definition: trackmpnn_amd.seqfeat.sequence_features_host): the reference's `val` / `test` sample of every listed sequence,
// packed one behind the other, in one launch.  A workgroup serves 256 packed rows.
//
// Like a drawn chunk's row (chunkdraw.hip), a feature row is a copy: the static row of the plain box, then the temporal pair of
// the row's frame from the fr_range-entry table.  Rows of 8 .. 143 floats start at any 4-byte boundary, so X is stored in single
// words, threads over (row, column) of the tile: a wave stores 64 consecutive floats whatever F is.
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int SF_THREADS = 256;

struct alignas(16) SfLabel { int64_t t, track; };

__global__ __launch_bounds__(SF_THREADS) void k_seq_features(tmpnn_seq_features_args d) {
    __shared__ int s_det[SF_THREADS];                 // store row of the tile's rows (-1: the row failed a check), its table row
    __shared__ int s_tm[SF_THREADS];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SF_THREADS;
    const int64_t i = row0 + tid;
    const int rows = d.n_rows - row0 < SF_THREADS ? (int)(d.n_rows - row0) : SF_THREADS;
    int det = -1, tm = 0;
    if (i < d.n_rows) {
        // the listed sequence of packed row i: the last k with offsets[k] <= i (k stays inside [0, K) whatever the table holds)
        int lo = 0, hi = d.K - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (d.offsets[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const int64_t o0 = d.offsets[lo], o1 = d.offsets[lo + 1];
        const int s = d.seqs[lo];
        int bad = 0;
        if (o0 < 0 || o0 > i || o1 <= i || o1 > d.n_rows || s < 0 || s >= d.nseq) bad = TMPNN_SF_FLAG_LIST;
        int64_t g0 = 0, g1 = 0, r = 0;
        if (!bad) {
            g0 = d.seq_base[s];
            g1 = d.seq_base[s + 1];
            if (g0 < 0 || g1 <= g0 || g1 > d.nframes) bad = TMPNN_SF_FLAG_RANGE;
        }
        if (!bad) {
            const int64_t r0 = d.first[g0], r1 = d.first[g1];
            r = r0 + (i - o0);
            if (r0 < 0 || r1 < r0 || r1 > d.ndets || r1 - r0 != o1 - o0) bad = TMPNN_SF_FLAG_RANGE;
        }
        int t = 0;
        if (!bad) {
            t = d.frame[r];
            if (t < 0 || t >= g1 - g0) bad = TMPNN_SF_FLAG_FRAME;
            else if (d.first[g0 + t] > r || d.first[g0 + t + 1] <= r) bad = TMPNN_SF_FLAG_FRAME;
        }
        if (bad) {
            atomicOr(d.flag, bad);
        } else {
            det = (int)r;
            tm = t % d.fr_range;
            SfLabel lab;
            lab.t = t;
            lab.track = d.track[r];
            reinterpret_cast<SfLabel*>(d.y)[i] = lab;
            if (d.box) {
                reinterpret_cast<float4*>(d.o_box)[i] = reinterpret_cast<const float4*>(d.box)[r * 2];
                reinterpret_cast<float2*>(d.o_im_hw)[i] = reinterpret_cast<const float2*>(d.seq_hw)[s];
                d.o_map_of[i] = t % d.frames_per_batch;
            }
        }
    }
    s_det[tid] = det;
    s_tm[tid] = tm;
    __syncthreads();
    const int F = d.F, Fs = d.Fs;
    float* xo = d.X + row0 * d.ldx;
    for (int e = tid; e < rows * F; e += SF_THREADS) {
        const int rr = e / F, col = e - rr * F;
        const int dt = s_det[rr];
        if (dt < 0) continue;
        xo[(int64_t)rr * d.ldx + col] = col < Fs ? d.stat[(int64_t)dt * 2 * Fs + col] : d.table[2 * s_tm[rr] + (col - Fs)];
    }
}

}  // namespace

extern "C" {

int tmpnn_seq_features(const tmpnn_seq_features_args* d, tmpnn_stream stream) {
    TM_REQUIRE(d, "seq_features: descriptor is null");
    TM_REQUIRE(d->K >= 1 && d->nseq >= 1 && d->K <= d->nseq, "seq_features: K=%d nseq=%d (1 <= K <= nseq)", d->K, d->nseq);
    TM_REQUIRE(d->Fs >= 1 && (d->F == d->Fs || d->F == d->Fs + 2), "seq_features: F=%d Fs=%d (F = Fs or Fs + 2)", d->F, d->Fs);
    TM_REQUIRE(d->ldx >= d->F, "seq_features: ldx=%d F=%d (>= F)", d->ldx, d->F);
    TM_REQUIRE(d->fr_range >= 1 && d->reserved == 0, "seq_features: fr_range=%d reserved=%d", d->fr_range, d->reserved);
    TM_REQUIRE(d->ndets >= 0 && d->ndets < INT32_MAX && d->nframes >= 1 && d->nframes < INT32_MAX, "seq_features: ndets=%lld nframes=%lld",
               (long long)d->ndets, (long long)d->nframes);
    TM_REQUIRE(d->n_rows >= 0 && d->n_rows <= d->ndets, "seq_features: n_rows=%lld (0 .. ndets = %lld)", (long long)d->n_rows,
               (long long)d->ndets);
    TM_REQUIRE(d->seqs && d->offsets && d->seq_base && d->first && d->flag, "seq_features: null pointer");
    if (d->n_rows == 0) return TMPNN_OK;
    TM_REQUIRE(d->frame && d->track && d->stat && d->X && d->y && (d->F == d->Fs || d->table), "seq_features: null pointer");
    TM_REQUIRE(aligned16(d->y), "seq_features: y is not 16-byte aligned");
    if (d->box) {
        TM_REQUIRE(d->frames_per_batch >= 1, "seq_features: frames_per_batch=%d", d->frames_per_batch);
        TM_REQUIRE(d->seq_hw && d->o_box && d->o_im_hw && d->o_map_of, "seq_features: null pointer (the 'vis' arguments)");
        TM_REQUIRE(aligned16(d->box) && aligned16(d->o_box), "seq_features: box or o_box is not 16-byte aligned");
        TM_REQUIRE((reinterpret_cast<uintptr_t>(d->seq_hw) & 7u) == 0 && (reinterpret_cast<uintptr_t>(d->o_im_hw) & 7u) == 0,
                   "seq_features: seq_hw or o_im_hw is not 8-byte aligned");
    }
    hipLaunchKernelGGL(k_seq_features, dim3(ceil_div(d->n_rows, SF_THREADS)), dim3(SF_THREADS), 0, as_stream(stream), *d);
    return check_launch("seq_features");
}

}  // extern "C"
