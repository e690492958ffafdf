// The training batch of trackmpnn_amd.train_batch.build_train_batch, built on the device (struct tmpnn_train_build,
// include/tmpnn.h).  One workgroup per chunk; the chunk's dets and their per-det state live in LDS.
//
// Slots: slot 0 holds the dets of t0, slot s >= 1 those of timestep t1 + s - 1, so call c appends the dets of slot c + 1 (call 0
// also those of slot 0).  The dets sorted by (slot, row of y) are the chunk's det rows in ascending order ("processing order",
// index k).  The active set of a timestep (utils/graph.py:229-245, 271-274) in closed form: det k is active at the non-empty slot
// s iff slot_k < s <= hi_k, where hi_k is the next slot holding a det of the same track (true positives; the last slot if there
// is none) or the next non-empty slot (false positives).  So a det's out-edges are one run of nt(s) rows at every non-empty slot
// of (slot_k, hi_k], its in-edges one row per det active at its own slot, and its degree at any call is a difference of slot
// offsets -- no edge set is kept.
#include "block_scan.h"
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int TB_THREADS = 256;

__device__ __forceinline__ int tb_block_scan(int v, int* s_wave, int* total) { return block_scan<TB_THREADS>(v, s_wave, total); }

// LDS of one chunk (dynamic: sized by the batch's largest chunk)
struct TbLds {
    uint32_t* key;   // [P]  slot << 12 | row of y, processing order after the sort
    int32_t* trk;    // [P]  track id, processing order
    uint16_t* hi;    // [P]  last slot at which the det is active
    uint16_t* act;   // [P]  active list of the current call
    int32_t* off;    // [max_slots + 1] first det of slot s; off[nslots] = nd
    int32_t* na;     // [max_slots]     dets active at slot s
    int32_t* wave;   // [8]
};

__device__ __forceinline__ TbLds tb_lds(char* smem, int P, int S) {
    TbLds L;
    L.key = reinterpret_cast<uint32_t*>(smem);
    L.trk = reinterpret_cast<int32_t*>(L.key + P);
    L.off = L.trk + P;
    L.na = L.off + S + 1;
    L.wave = L.na + S;
    L.hi = reinterpret_cast<uint16_t*>(L.wave + 8);
    L.act = L.hi + P;
    return L;
}

inline size_t tb_lds_bytes(int P, int S) { return (size_t)P * 12 + (size_t)(2 * S + 1 + 8) * 4; }

// sort the chunk, then slot offsets, track ids, hi and the active counts per slot
__device__ void tb_analyze(const tmpnn_train_build& d, const TbLds& L, int i, int nd, int nslots) {
    const int tid = threadIdx.x;
    const int64_t* y = d.y + 2 * d.offsets[i];
    const int64_t t0 = d.info[4 * i + 2], t1 = d.info[4 * i + 3];
    int P = 1;
    while (P < nd) P <<= 1;
    for (int k = tid; k < P; k += TB_THREADS) {
        uint32_t key = 0xFFFFFFFFu;
        if (k < nd) {
            const int64_t t = y[2 * k];
            const uint32_t s = t == t0 ? 0u : (uint32_t)(t - t1 + 1);
            key = (s << 12) | (uint32_t)k;
        }
        L.key[k] = key;
    }
    for (int s = tid; s < nslots + 1; s += TB_THREADS) L.off[s] = nd;
    for (int s = tid; s < nslots; s += TB_THREADS) L.na[s] = 0;
    __syncthreads();
    // bitonic sort (keys are distinct: the row is in the low bits, so the order within a slot is the order of y)
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int a = tid; a < P; a += TB_THREADS) {
                const int b = a ^ j;
                if (b > a) {
                    const uint32_t ka = L.key[a], kb = L.key[b];
                    const bool up = (a & k) == 0;
                    if ((ka > kb) == up) { L.key[a] = kb; L.key[b] = ka; }
                }
            }
            __syncthreads();
        }
    for (int k = tid; k < nd; k += TB_THREADS) {
        const int s = (int)(L.key[k] >> 12), sp = k == 0 ? -1 : (int)(L.key[k - 1] >> 12);
        for (int q = sp + 1; q <= s; ++q) L.off[q] = k;
        L.trk[k] = (int32_t)y[2 * (L.key[k] & 0xFFFu) + 1];
    }
    __syncthreads();
    for (int k = tid; k < nd; k += TB_THREADS) {
        const int s = (int)(L.key[k] >> 12), tr = L.trk[k], nxt = L.off[s + 1];
        int hi = s;
        if (tr >= 0) {
            hi = nslots - 1;
            for (int j = nxt; j < nd; ++j)
                if (L.trk[j] == tr) { hi = (int)(L.key[j] >> 12); break; }
        } else if (nxt < nd) {
            hi = (int)(L.key[nxt] >> 12);
        }
        L.hi[k] = (uint16_t)hi;
        if (hi > s) {
            atomicAdd(&L.na[s + 1], 1);
            if (hi + 1 < nslots) atomicAdd(&L.na[hi + 1], -1);
        }
    }
    __syncthreads();
    int carry = 0;
    for (int base = 0; base < nslots; base += TB_THREADS) {
        const int s = base + tid;
        const int v = s < nslots ? L.na[s] : 0;
        int tot;
        const int p = tb_block_scan(v, L.wave, &tot);
        if (s < nslots) L.na[s] = carry + p + v;
        carry += tot;
    }
    __syncthreads();
}

// the active list of slot s into L.act (processing order); returns its length
__device__ int tb_active(const TbLds& L, int s) {
    int cnt = 0;
    const int n = L.off[s];
    for (int base = 0; base < n; base += TB_THREADS) {
        const int k = base + threadIdx.x;
        const int f = (k < n && (int)(L.key[k] >> 12) < s && s <= (int)L.hi[k]) ? 1 : 0;
        int tot;
        const int p = tb_block_scan(f, L.wave, &tot);
        if (f) L.act[cnt + p] = (uint16_t)k;
        cnt += tot;
    }
    __syncthreads();
    return cnt;
}

__device__ __forceinline__ int tb_nt(const TbLds& L, int c) { return L.off[c + 2] - L.off[c + 1]; }
__device__ __forceinline__ int tb_edges(const TbLds& L, int c) {
    return c == 0 ? L.off[1] * (L.off[2] - L.off[1]) : L.na[c + 1] * tb_nt(L, c);
}

// global row and det index of det k of batch chunk b
struct TbDet { int row, gd, call; };
__device__ __forceinline__ TbDet tb_det(const tmpnn_train_build& d, const TbLds& L, int b, int k) {
    const int s = (int)(L.key[k] >> 12), c = s > 0 ? s - 1 : 0;
    const int32_t* bl = d.blk + 4 * (d.cptr[b] + c);
    TbDet r;
    r.call = c;
    if (c == 0) {
        const int n0 = L.off[1];
        r.gd = bl[2] + k;
        r.row = bl[0] + (s == 0 ? k : n0 + n0 * (L.off[2] - n0) + (k - n0));
    } else {
        r.gd = bl[2] + (k - L.off[s]);
        r.row = bl[0] + tb_edges(L, c) + (k - L.off[s]);
    }
    return r;
}

// A kept chunk that the descriptor's LDS sizes (max_dets, max_slots) or its C do not cover: the kernel writes nothing for it and
// sets TMPNN_TB_ST_LDS in its status word (the count pass's checks and the Python front never let one through).
__device__ __forceinline__ bool tb_fits(const tmpnn_train_build& d, int i, int64_t nd, int64_t ncalls, int C) {
    if (nd >= 2 && nd <= d.max_dets && ncalls >= 1 && ncalls + 2 <= d.max_slots && ncalls <= C) return true;
    if (threadIdx.x == 0) d.info[4 * i] |= TMPNN_TB_ST_LDS;
    return false;
}

__global__ __launch_bounds__(TB_THREADS) void k_tb_count(tmpnn_train_build d) {
    __shared__ int64_t red[4][TB_THREADS / 64];
    __shared__ int s_st[TB_THREADS / 64];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t o0 = d.offsets[i], o1 = d.offsets[i + 1];
    int st = 0;
    if (o0 < 0 || o1 < o0 || o1 > d.n_feat) st |= TMPNN_TB_ST_OFFSETS;
    const int64_t nd = st ? 0 : o1 - o0;
    const int64_t* y = d.y + 2 * o0;
    int64_t tmin = INT64_MAX, tmax = -1, tp = 0;
    for (int64_t k = tid; k < nd; k += TB_THREADS) {
        const int64_t t = y[2 * k], tr = y[2 * k + 1];
        if (t == TMPNN_TB_NONINT || tr == TMPNN_TB_NONINT) { st |= TMPNN_TB_ST_NONINT; continue; }
        if (t > INT32_MAX || tr > INT32_MAX || tr < INT32_MIN) st |= TMPNN_TB_ST_RANGE;
        if (t < 0) st |= TMPNN_TB_ST_NEGTS;
        tmin = t < tmin ? t : tmin;
        tmax = t > tmax ? t : tmax;
        tp |= tr != -1;
    }
    // (wave reductions, then across the four waves)
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t a = __shfl_xor(tmin, o), b = __shfl_xor(tmax, o), c = __shfl_xor(tp, o);
        const int e = __shfl_xor(st, o);
        tmin = a < tmin ? a : tmin; tmax = b > tmax ? b : tmax; tp |= c; st |= e;
    }
    if (lane == 0) { red[0][wave] = tmin; red[1][wave] = tmax; red[2][wave] = tp; s_st[wave] = st; }
    __syncthreads();
    for (int w = 0; w < TB_THREADS / 64; ++w) {
        tmin = red[0][w] < tmin ? red[0][w] : tmin; tmax = red[1][w] > tmax ? red[1][w] : tmax; tp |= red[2][w]; st |= s_st[w];
    }
    // t1: the smallest timestep above t0
    int64_t t1 = INT64_MAX;
    for (int64_t k = tid; k < nd; k += TB_THREADS) {
        const int64_t t = y[2 * k];
        if (t != TMPNN_TB_NONINT && t > tmin && t < t1) t1 = t;
    }
    for (int o = 32; o > 0; o >>= 1) { const int64_t a = __shfl_xor(t1, o); t1 = a < t1 ? a : t1; }
    __syncthreads();
    if (lane == 0) red[3][wave] = t1;
    __syncthreads();
    for (int w = 0; w < TB_THREADS / 64; ++w) t1 = red[3][w] < t1 ? red[3][w] : t1;
    if (tid == 0) {
        int64_t ncalls = 0;
        if (!st && t1 != INT64_MAX && tp) {                 // kept: two distinct timesteps and a track id other than -1
            ncalls = 1 + tmax - t1;
            if (nd > TMPNN_TB_MAX_DETS) st |= TMPNN_TB_ST_DETS;
            if (ncalls > TMPNN_TB_MAX_CALLS) st |= TMPNN_TB_ST_CALLS;
        }
        int64_t* o = d.info + 4 * (int64_t)i;
        o[0] = st;
        o[1] = st ? 0 : ncalls;
        o[2] = tmin;
        o[3] = t1;
    }
}

__global__ __launch_bounds__(TB_THREADS) void k_tb_calls(tmpnn_train_build d) {
    extern __shared__ __align__(16) char smem[];
    const int b = blockIdx.x, i = d.kept[b];
    if (!tb_fits(d, i, d.offsets[i + 1] - d.offsets[i], d.info[4 * i + 1], TMPNN_TB_MAX_CALLS)) return;
    const int nd = (int)(d.offsets[i + 1] - d.offsets[i]), ncalls = (int)d.info[4 * i + 1];
    const TbLds L = tb_lds(smem, d.max_dets, d.max_slots);
    tb_analyze(d, L, i, nd, ncalls + 1);
    int32_t* out = d.counts + 2 * (int64_t)d.cptr[b];
    for (int c = threadIdx.x; c < ncalls; c += TB_THREADS) {
        out[2 * c] = tb_edges(L, c);
        out[2 * c + 1] = c == 0 ? L.off[2] : tb_nt(L, c);
    }
}

// phase 0: everything but inc
__global__ __launch_bounds__(TB_THREADS) void k_tb_fill(tmpnn_train_build d) {
    extern __shared__ __align__(16) char smem[];
    const int b = blockIdx.x, i = d.kept[b], tid = threadIdx.x;
    if (!tb_fits(d, i, d.offsets[i + 1] - d.offsets[i], d.info[4 * i + 1], d.C)) return;
    const int nd = (int)(d.offsets[i + 1] - d.offsets[i]), ncalls = (int)d.info[4 * i + 1], C = d.C, B = d.B;
    const TbLds L = tb_lds(smem, d.max_dets, d.max_slots);
    tb_analyze(d, L, i, nd, ncalls + 1);
    const int64_t* rowsb = d.call_tab;              // rows before call c
    const int64_t* rp = d.call_tab + C;             // per call: first element in rowptr
    const int64_t* dob = d.call_tab + 3 * C;        // det_order / det_win
    const int64_t* ewb = d.call_tab + 4 * C;        // edge_win
    const int64_t* dib = d.call_tab + 5 * C;        // det_idx
    const int64_t* eib = d.call_tab + 6 * C;        // edge_idx
    const int32_t* GO = d.cb_tab;
    const int32_t* GL = d.cb_tab + (int64_t)C * B;
    const int32_t* GLE = d.cb_tab + 2 * (int64_t)C * B;
    if (b == 0)
        for (int c = tid; c < C; c += TB_THREADS) d.rowptr[rp[c]] = 0;
    // dets
    for (int k = tid; k < nd; k += TB_THREADS) {
        const TbDet t = tb_det(d, L, b, k);
        const int s = (int)(L.key[k] >> 12), hi = L.hi[k], tr = L.trk[k];
        const int seg = d.blk[4 * (d.cptr[b] + t.call) + 3];
        d.det_row[t.gd] = t.row;
        d.pos[t.row] = t.gd;
        d.is_edge[t.row] = 0;
        d.labels[t.row] = tr >= 0 ? 1 : 0;
        d.feat_src[t.row] = d.offsets[i] + (int64_t)(L.key[k] & 0xFFFu);
        d.seg_of_new[t.row] = seg;
        d.new_det_local[t.gd] = (int64_t)t.row - rowsb[t.call];
        d.seg_of_det[t.gd] = seg;
        d.det_group[t.gd] = b;
        const int in = s == 0 ? 0 : L.na[s];
        for (int c = t.call; c < C; ++c) {
            const bool live = c < ncalls;
            const int sc = (live ? c : ncalls - 1) + 1, top = hi < sc ? hi : sc;
            const int out = top > s ? L.off[top + 1] - L.off[s + 1] : 0;
            d.rowptr[rp[c] + 1 + t.gd] = in + out;
            d.det_order[dob[c] + GO[(int64_t)c * B + b] + k] = t.gd;
            d.det_win[dob[c] + t.gd] = live ? b : -1;
            if (live) d.det_idx[dib[c] + GL[(int64_t)c * B + b] + k] = t.gd;
        }
    }
    // edges, call by call: rows [pre + ia * nt + j] of the call's block
    int ebefore = 0;                                  // the chunk's edges of earlier calls
    for (int c = 0; c < ncalls; ++c) {
        const int s = c + 1, nt = tb_nt(L, c);
        const int na = tb_active(L, s), ne = na * nt;
        const int32_t* bl = d.blk + 4 * (d.cptr[b] + c);
        const int row0 = bl[0] + (c == 0 ? L.off[1] : 0), e0 = bl[1], seg = bl[3];
        for (int m = tid; m < ne; m += TB_THREADS) {
            const int ia = m / nt, j = m - ia * nt;
            const int a = L.act[ia], q = L.off[s] + j;
            const TbDet ta = tb_det(d, L, b, a), tq = tb_det(d, L, b, q);
            const int row = row0 + m, ge = e0 + m;
            d.src[ge] = ta.row;
            d.dst[ge] = tq.row;
            d.edge_row[ge] = row;
            d.src_pos[ge] = ta.gd;
            d.dst_pos[ge] = tq.gd;
            d.pos[row] = ge;
            d.is_edge[row] = 1;
            d.labels[row] = (L.trk[a] == L.trk[q] && L.trk[a] >= 0) ? 1 : 0;
            d.feat_src[row] = d.n_feat;
            d.seg_of_new[row] = seg;
            for (int cc = c; cc < C; ++cc) {
                const bool live = cc < ncalls;
                d.edge_win[ewb[cc] + ge] = live ? b : -1;
                if (live) d.edge_idx[eib[cc] + GLE[(int64_t)cc * B + b] + ebefore + m] = ge;
            }
        }
        ebefore += ne;
        __syncthreads();                              // (L.act is rebuilt for the next call)
    }
}

// phase 1: inc, at the offsets the scan of phase 0's degrees gave
__global__ __launch_bounds__(TB_THREADS) void k_tb_inc(tmpnn_train_build d) {
    extern __shared__ __align__(16) char smem[];
    const int b = blockIdx.x, i = d.kept[b], tid = threadIdx.x;
    if (!tb_fits(d, i, d.offsets[i + 1] - d.offsets[i], d.info[4 * i + 1], d.C)) return;
    const int nd = (int)(d.offsets[i + 1] - d.offsets[i]), ncalls = (int)d.info[4 * i + 1], C = d.C;
    const TbLds L = tb_lds(smem, d.max_dets, d.max_slots);
    tb_analyze(d, L, i, nd, ncalls + 1);
    const int64_t* rp = d.call_tab + C;
    const int64_t* ib = d.call_tab + 2 * C;
    // in-edges (the det is the later endpoint: sign bit set), first in its run
    for (int k = tid; k < nd; k += TB_THREADS) {
        const int s = (int)(L.key[k] >> 12);
        if (s == 0) continue;
        const TbDet t = tb_det(d, L, b, k);
        const int na = L.na[s], nt = L.off[s + 1] - L.off[s], j = k - L.off[s];
        const int row0 = d.blk[4 * (d.cptr[b] + t.call)] + (t.call == 0 ? L.off[1] : 0) + j;
        for (int c = t.call; c < C; ++c) {
            const int32_t* r = d.rowptr + rp[c] + t.gd;
            int32_t* o = d.inc + ib[c] + r[0];
            const int n = min(na, r[1] - r[0]);       // (= na: the run's length is phase 0's degree; never past the run)
            for (int ia = 0; ia < n; ++ia) o[ia] = (int32_t)((uint32_t)(row0 + ia * nt) | 0x80000000u);
        }
    }
    // out-edges: a run of nt rows at every call the det is active at, after its in-edges and earlier runs
    for (int c = 0; c < ncalls; ++c) {
        const int s = c + 1, nt = tb_nt(L, c);
        const int na = tb_active(L, s);
        const int row0 = d.blk[4 * (d.cptr[b] + c)] + (c == 0 ? L.off[1] : 0);
        for (int ia = tid; ia < na; ia += TB_THREADS) {
            const int k = L.act[ia], sk = (int)(L.key[k] >> 12);
            const TbDet t = tb_det(d, L, b, k);
            const int skip = (sk == 0 ? 0 : L.na[sk]) + L.off[s] - L.off[sk + 1];
            const int r = row0 + ia * nt;
            for (int cc = c; cc < C; ++cc) {
                const int32_t* rr = d.rowptr + rp[cc] + t.gd;
                int32_t* o = d.inc + ib[cc] + rr[0] + skip;
                const int n = min(nt, rr[1] - rr[0] - skip);
                for (int j = 0; j < n; ++j) o[j] = r + j;
            }
        }
        __syncthreads();
    }
}

int tb_check_batch(const tmpnn_train_build* d, const char* what) {
    TM_REQUIRE(d, "%s: descriptor is null", what);
    TM_REQUIRE(d->n > 0 && d->B > 0 && d->B <= d->n, "%s: B=%d kept chunks of n=%d", what, d->B, d->n);
    TM_REQUIRE(d->y && d->offsets && d->info && d->kept && d->cptr, "%s: null input pointer", what);
    TM_REQUIRE(d->max_dets >= 1 && d->max_dets <= TMPNN_TB_MAX_DETS && (d->max_dets & (d->max_dets - 1)) == 0,
               "%s: max_dets=%d (a power of two <= %d)", what, d->max_dets, TMPNN_TB_MAX_DETS);
    TM_REQUIRE(d->max_slots >= 3 && d->max_slots <= TMPNN_TB_MAX_CALLS + 2, "%s: max_slots=%d (3 .. %d)", what, d->max_slots,
               TMPNN_TB_MAX_CALLS + 2);
    return TMPNN_OK;
}

}  // namespace

extern "C" {

int tmpnn_train_build_count(const tmpnn_train_build* d, tmpnn_stream stream) {
    TM_REQUIRE(d, "train_build_count: descriptor is null");
    TM_REQUIRE(d->n >= 0, "train_build_count: n=%d", d->n);
    TM_REQUIRE(d->n == 0 || (d->y && d->offsets && d->info), "train_build_count: null pointer");
    if (d->n == 0) return TMPNN_OK;
    hipLaunchKernelGGL(k_tb_count, dim3(d->n), dim3(TB_THREADS), 0, as_stream(stream), *d);
    return check_launch("train_build_count");
}

int tmpnn_train_build_calls(const tmpnn_train_build* d, tmpnn_stream stream) {
    if (int rc = tb_check_batch(d, "train_build_calls")) return rc;
    TM_REQUIRE(d->counts, "train_build_calls: counts is null");
    hipLaunchKernelGGL(k_tb_calls, dim3(d->B), dim3(TB_THREADS), tb_lds_bytes(d->max_dets, d->max_slots), as_stream(stream), *d);
    return check_launch("train_build_calls");
}

int tmpnn_train_build_fill(const tmpnn_train_build* d, int phase, tmpnn_stream stream) {
    if (int rc = tb_check_batch(d, "train_build_fill")) return rc;
    TM_REQUIRE(phase == 0 || phase == 1, "train_build_fill: phase=%d (0 or 1)", phase);
    TM_REQUIRE(d->C >= 1 && d->C <= TMPNN_TB_MAX_CALLS, "train_build_fill: C=%d (1 .. %d)", d->C, TMPNN_TB_MAX_CALLS);
    TM_REQUIRE(d->blk && d->call_tab && d->cb_tab && d->rowptr, "train_build_fill: null table");
    if (phase == 0) {
        TM_REQUIRE(d->src && d->dst && d->edge_row && d->src_pos && d->dst_pos && d->det_row && d->seg_of_det && d->new_det_local &&
                       d->det_group && d->is_edge && d->pos && d->labels && d->feat_src && d->seg_of_new && d->det_order &&
                       d->det_win && d->edge_win && d->det_idx && d->edge_idx,
                   "train_build_fill: null output");
        hipLaunchKernelGGL(k_tb_fill, dim3(d->B), dim3(TB_THREADS), tb_lds_bytes(d->max_dets, d->max_slots), as_stream(stream), *d);
    } else {
        TM_REQUIRE(d->inc, "train_build_fill: inc is null");
        hipLaunchKernelGGL(k_tb_inc, dim3(d->B), dim3(TB_THREADS), tb_lds_bytes(d->max_dets, d->max_slots), as_stream(stream), *d);
    }
    return check_launch("train_build_fill");
}

}  // extern "C"
