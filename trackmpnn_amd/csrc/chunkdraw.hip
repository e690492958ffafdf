// A seeded draw of augmented training chunks from the device-resident detection store (struct tmpnn_chunk_draw,
// include/tmpnn.h; host definition: trackmpnn_amd.chunks.draw_chunks_host).  One workgroup per drawn chunk.
//
// The decisions of a chunk (reversal, flip, per-row dropout) are a function of (seed, step, chunk index, row) through
// Philox4x32-10, so the count pass and the fill pass recompute them and nothing is stored between the two launches.  The
// features were standardised on the host (plain and flipped static rows, the temporal table): a kept row of X is a copy.
#include "block_scan.h"
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int CD_THREADS = 256;
static_assert(TMPNN_CD_MAX_FRAMES <= CD_THREADS, "one thread per frame of a chunk's list");

struct Philox { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al., SC'11): counter c, key k
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Philox o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// u = (word >> 8) * 2^-24 (exact in fp32); the event happens iff u < p
__device__ __forceinline__ bool cd_event(uint32_t word, float p) { return (float)(word >> 8) * 0x1p-24f < p; }

// one drawn chunk: sizes, the ends of its frame list, its decisions
struct CdChunk {
    int n;          // rows before dropout (0: an empty or a rejected chunk)
    int seq;        // sequence of the chunk
    int nfr;        // frames of the list
    int t_lo, t_hi; // first and last frame of the list
    uint32_t ci;    // chunk index = word 1 of the counter
    int flags;
};

struct CdLds {
    int pre[TMPNN_CD_MAX_FRAMES + 1];   // rows of the chunk before frame i of the list
    int first[TMPNN_CD_MAX_FRAMES];     // first detection of frame i in the store
    int frame[TMPNN_CD_MAX_FRAMES];     // frame i of the list
    int wave[CD_THREADS / 64 + 1];
};

// Reads chunk indices[b] of the table into LDS, every index checked against the store's sizes (block-uniform result).
__device__ CdChunk cd_setup(const tmpnn_chunk_draw& d, int b, CdLds& L) {
    const int tid = threadIdx.x;
    CdChunk c;
    c.n = 0; c.seq = 0; c.nfr = 0; c.t_lo = 0; c.t_hi = 0; c.flags = 0;
    const int ci = d.indices[b];
    c.ci = (uint32_t)ci;
    int bad = ci < 0 || ci >= d.nchunks;
    int seq = 0, nfr = 0, n_tab = 0;
    const int32_t* rec = d.chunks;
    if (!bad) {
        rec += (int64_t)ci * (4 + d.L);
        seq = rec[0]; nfr = rec[1]; n_tab = rec[2];
        bad = seq < 0 || seq >= d.nseq || nfr < 1 || nfr > d.L || n_tab < 0 || n_tab > TMPNN_TB_MAX_DETS;
    }
    int cnt = 0, f0 = 0, fr = 0;
    if (!bad && tid < nfr) {
        fr = rec[4 + tid];
        const int64_t g = (int64_t)d.seq_base[seq] + fr;
        if (fr < 0 || g < 0 || g >= d.seq_base[seq + 1] || g >= d.nframes) {
            bad = 1;
        } else {
            const int lo = d.first[g], hi = d.first[g + 1];
            if (lo < 0 || hi < lo || hi > d.ndets) bad = 1;
            else { cnt = hi - lo; f0 = lo; }
        }
    }
    int total;
    const int p = block_scan<CD_THREADS>(bad ? 0 : cnt, L.wave, &total);
    if (tid < TMPNN_CD_MAX_FRAMES) { L.pre[tid] = p; L.first[tid] = f0; L.frame[tid] = fr; }
    if (tid == 0) L.pre[TMPNN_CD_MAX_FRAMES] = total;
    bad = __syncthreads_or(bad);
    if (bad || total != n_tab) {
        c.flags = TMPNN_CD_FLAG_BAD;
        return c;
    }
    c.n = total;
    c.seq = seq;
    c.nfr = nfr;
    c.t_lo = L.frame[0];
    c.t_hi = L.frame[nfr - 1];
    if (d.transforms) {
        const Philox h = philox4x32_10(0u, c.ci, (uint32_t)d.step, (uint32_t)(d.step >> 32), (uint32_t)d.seed,
                                       (uint32_t)(d.seed >> 32));
        if (cd_event(h.w[0], d.p_reverse)) c.flags |= TMPNN_CD_FLAG_REVERSED;
        if (cd_event(h.w[1], d.p_flip)) c.flags |= TMPNN_CD_FLAG_FLIPPED;
    }
    return c;
}

// is row r of the chunk (output order before dropout) kept?
__device__ __forceinline__ bool cd_keep(const tmpnn_chunk_draw& d, const CdChunk& c, int r) {
    if (!d.transforms) return true;
    // (the four rows of a block each run the ten rounds: the pass is bound by its stores, the vector ALU is idle)
    const Philox h = philox4x32_10(1u + ((uint32_t)r >> 2), c.ci, (uint32_t)d.step, (uint32_t)(d.step >> 32), (uint32_t)d.seed,
                                   (uint32_t)(d.seed >> 32));
    const int w = r & 3;                              // (selects, not an indexed array: that would be placed in LDS)
    const uint32_t word = w == 0 ? h.w[0] : w == 1 ? h.w[1] : w == 2 ? h.w[2] : h.w[3];
    return !cd_event(word, d.p_drop);
}

__global__ __launch_bounds__(CD_THREADS) void k_cd_count(tmpnn_chunk_draw d) {
    __shared__ CdLds L;
    __shared__ int s_cnt[CD_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const CdChunk c = cd_setup(d, b, L);
    int kept = 0;                                     // wave-uniform
    for (int base = 0; base < c.n; base += CD_THREADS) {
        const int r = base + tid;
        const bool k = r < c.n && cd_keep(d, c, r);
        kept += __popcll(__ballot(k));
    }
    if ((tid & 63) == 0) s_cnt[tid >> 6] = kept;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < CD_THREADS / 64; ++w) tot += s_cnt[w];
        d.count[b] = tot;
        d.flags[b] = (uint8_t)c.flags;
    }
}

// offsets[0] = 0, offsets[i + 1] = count[0] + .. + count[i]: one workgroup walks the B counts
__global__ __launch_bounds__(CD_THREADS) void k_cd_scan(tmpnn_chunk_draw d) {
    __shared__ int s_wave[CD_THREADS / 64 + 1];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    if (tid == 0) d.offsets[0] = 0;
    for (int base = 0; base < d.B; base += CD_THREADS) {
        const int i = base + tid;
        const int v = i < d.B ? d.count[i] : 0;
        int tot;
        const int p = block_scan<CD_THREADS>(v, s_wave, &tot);
        if (i < d.B) d.offsets[i + 1] = carry + p + v;
        carry += tot;
    }
}

struct alignas(16) CdLabel { int64_t t, track; };

__global__ __launch_bounds__(CD_THREADS) void k_cd_fill(tmpnn_chunk_draw d) {
    __shared__ CdLds L;
    __shared__ int s_det[CD_THREADS];                 // kept rows of the tile: detection, row of the temporal table
    __shared__ int s_tm[CD_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const CdChunk c = cd_setup(d, b, L);
    const int64_t o0 = d.offsets[b], o1 = d.offsets[b + 1];
    if (c.n == 0 || o0 < 0 || o1 < o0 || o1 > d.n_max || o1 - o0 > c.n) return;        // (block-uniform)
    const bool rev = c.flags & TMPNN_CD_FLAG_REVERSED;
    const int flip = (c.flags & TMPNN_CD_FLAG_FLIPPED) ? 1 : 0;
    const int F = d.F, Fs = d.Fs, ld = d.ldx ? d.ldx : d.F;
    CdLabel* yout = reinterpret_cast<CdLabel*>(d.y);
    int64_t row0 = o0;                                // first output row of the tile
    for (int base = 0; base < c.n; base += CD_THREADS) {
        const int r = base + tid;
        bool k = false;
        int det = 0, t = 0;
        if (r < c.n) {
            // frame of row r: the last i with pre[i] <= r
            int lo = 0, hi = c.nfr - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (L.pre[mid] <= r) lo = mid; else hi = mid - 1;
            }
            det = L.first[lo] + (r - L.pre[lo]);
            t = L.frame[lo];
            if (rev) t = c.t_hi - t + c.t_lo;
            k = cd_keep(d, c, r);
        }
        int tot;
        const int p = block_scan<CD_THREADS>(k ? 1 : 0, L.wave, &tot);
        if (row0 + tot > o1) return;                  // (block-uniform: the count pass gave fewer rows than this pass keeps)
        if (k) {
            CdLabel lab;
            lab.t = t;
            lab.track = d.track[det];
            yout[row0 + p] = lab;
            s_det[p] = det;
            const int m = t % d.fr_range;
            s_tm[p] = m < 0 ? m + d.fr_range : m;
        }
        __syncthreads();
        // X: threads over (row, column) of the tile's kept rows, so a wave stores 64 consecutive floats
        float* xo = d.X + row0 * ld;
        for (int e = tid; e < tot * F; e += CD_THREADS) {
            const int rr = e / F, col = e - rr * F;
            xo[(int64_t)rr * ld + col] = col < Fs ? d.stat[((int64_t)s_det[rr] * 2 + flip) * Fs + col] : d.table[2 * s_tm[rr] + (col - Fs)];
        }
        row0 += tot;
        __syncthreads();                              // (s_det / s_tm are rewritten by the next tile)
    }
}

// The rows a vis store adds to a draw (tmpnn_chunk_draw_vis): the decisions are the fill's (cd_setup, cd_keep), so kept row k of
// chunk b lands on row offsets[b] + k here as it does there.  Every thread stores its own row: the box as one 16-byte store.
__global__ __launch_bounds__(CD_THREADS) void k_cd_vis(tmpnn_chunk_draw d, tmpnn_chunk_vis v) {
    __shared__ CdLds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const CdChunk c = cd_setup(d, b, L);
    const int64_t o0 = d.offsets[b], o1 = d.offsets[b + 1];
    if (c.n == 0 || o0 < 0 || o1 < o0 || o1 > d.n_max || o1 - o0 > c.n) return;        // (block-uniform; FLAG_BAD has n = 0)
    const int flip = (c.flags & TMPNN_CD_FLAG_FLIPPED) ? 1 : 0;
    const float2 hw = reinterpret_cast<const float2*>(v.seq_hw)[c.seq];
    const float4* box = reinterpret_cast<const float4*>(v.box);
    float4* o_box = reinterpret_cast<float4*>(v.o_box);
    float2* o_hw = reinterpret_cast<float2*>(v.o_im_hw);
    const int32_t* slot = v.slot + (int64_t)b * d.L;
    int64_t row0 = o0;
    for (int base = 0; base < c.n; base += CD_THREADS) {
        const int r = base + tid;
        bool k = false;
        int det = 0, li = 0;
        if (r < c.n) {
            int lo = 0, hi = c.nfr - 1;                // frame of row r: the last i with pre[i] <= r
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (L.pre[mid] <= r) lo = mid; else hi = mid - 1;
            }
            det = L.first[lo] + (r - L.pre[lo]);
            li = lo;
            k = cd_keep(d, c, r);
        }
        int tot;
        const int p = block_scan<CD_THREADS>(k ? 1 : 0, L.wave, &tot);
        if (row0 + tot > o1) return;                  // (block-uniform, as in the fill)
        if (k) {
            const int64_t o = row0 + p;
            o_box[o] = box[(int64_t)det * 2 + flip];
            o_hw[o] = hw;
            v.o_map_of[o] = slot[li];
            v.o_track[o] = d.track[det];
        }
        row0 += tot;
    }
}

int cd_check(const tmpnn_chunk_draw* d, const char* what) {
    TM_REQUIRE(d, "%s: descriptor is null", what);
    TM_REQUIRE(d->B >= 1 && d->nchunks >= 1 && d->nseq >= 1, "%s: B=%d nchunks=%d nseq=%d", what, d->B, d->nchunks, d->nseq);
    TM_REQUIRE(d->L >= 1 && d->L <= TMPNN_CD_MAX_FRAMES, "%s: L=%d (1 .. %d)", what, d->L, TMPNN_CD_MAX_FRAMES);
    TM_REQUIRE(d->Fs >= 1 && (d->F == d->Fs || d->F == d->Fs + 2), "%s: F=%d Fs=%d (F = Fs or Fs + 2)", what, d->F, d->Fs);
    TM_REQUIRE(d->ldx == 0 || d->ldx >= d->F, "%s: ldx=%d F=%d (0, or >= F)", what, d->ldx, d->F);
    TM_REQUIRE(d->fr_range >= 1, "%s: fr_range=%d", what, d->fr_range);
    TM_REQUIRE(d->ndets >= 0 && d->ndets <= INT32_MAX && d->nframes >= 1 && d->nframes < INT32_MAX, "%s: ndets=%lld nframes=%lld",
               what, (long long)d->ndets, (long long)d->nframes);
    TM_REQUIRE(d->n_max >= 0 && d->n_max <= INT32_MAX, "%s: n_max=%lld (0 .. 2^31 - 1)", what, (long long)d->n_max);
    TM_REQUIRE(d->p_drop >= 0.f && d->p_drop <= 1.f && d->p_reverse >= 0.f && d->p_reverse <= 1.f && d->p_flip >= 0.f &&
                   d->p_flip <= 1.f, "%s: a probability outside [0, 1]", what);
    TM_REQUIRE(d->indices && d->chunks && d->seq_base && d->first && d->count && d->flags && d->offsets, "%s: null pointer", what);
    return TMPNN_OK;
}

}  // namespace

extern "C" {

int tmpnn_chunk_draw_count(const tmpnn_chunk_draw* d, tmpnn_stream stream) {
    if (int rc = cd_check(d, "chunk_draw_count")) return rc;
    hipLaunchKernelGGL(k_cd_count, dim3(d->B), dim3(CD_THREADS), 0, as_stream(stream), *d);
    if (int rc = check_launch("chunk_draw_count")) return rc;
    hipLaunchKernelGGL(k_cd_scan, dim3(1), dim3(CD_THREADS), 0, as_stream(stream), *d);
    return check_launch("chunk_draw_count (scan)");
}

int tmpnn_chunk_draw_fill(const tmpnn_chunk_draw* d, tmpnn_stream stream) {
    if (int rc = cd_check(d, "chunk_draw_fill")) return rc;
    if (d->n_max == 0) return TMPNN_OK;
    TM_REQUIRE(d->track && d->stat && d->X && d->y && (d->F == d->Fs || d->table), "chunk_draw_fill: null pointer");
    TM_REQUIRE(aligned16(d->y), "chunk_draw_fill: y is not 16-byte aligned");
    hipLaunchKernelGGL(k_cd_fill, dim3(d->B), dim3(CD_THREADS), 0, as_stream(stream), *d);
    return check_launch("chunk_draw_fill");
}

int tmpnn_chunk_draw_vis(const tmpnn_chunk_draw* d, const tmpnn_chunk_vis* v, tmpnn_stream stream) {
    if (int rc = cd_check(d, "chunk_draw_vis")) return rc;
    TM_REQUIRE(v, "chunk_draw_vis: the vis struct is null");
    if (d->n_max == 0) return TMPNN_OK;
    TM_REQUIRE(d->track && v->box && v->seq_hw && v->slot && v->o_box && v->o_im_hw && v->o_map_of && v->o_track,
               "chunk_draw_vis: null pointer");
    TM_REQUIRE(aligned16(v->box) && aligned16(v->o_box), "chunk_draw_vis: box or o_box is not 16-byte aligned");
    TM_REQUIRE((reinterpret_cast<uintptr_t>(v->seq_hw) & 7u) == 0 && (reinterpret_cast<uintptr_t>(v->o_im_hw) & 7u) == 0,
               "chunk_draw_vis: seq_hw or o_im_hw is not 8-byte aligned");
    hipLaunchKernelGGL(k_cd_vis, dim3(d->B), dim3(CD_THREADS), 0, as_stream(stream), *d, *v);
    return check_launch("chunk_draw_vis");
}

}  // extern "C"
