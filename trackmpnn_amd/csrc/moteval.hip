// CLEAR-MOT events of a set of tracks against the ground truth, on the device (tmpnn_mot_events, tmpnn_mot_dist; include/tmpnn.h;
// host definition: trackmpnn_amd.moteval.mot_events_host), and the rest of the MOT-challenge summary from the same walk plus the
// identity kernels further down (tmpnn_mot_summary; host definition: mot_summary_host).  The reference feeds py-motmetrics one frame at a time on the host
// (utils/metrics.py:7-61); the rule is sequential in the frames of a sequence and independent across sequences, so ONE WAVE per
// sequence walks the frames (one workgroup of 64 threads per sequence: no workgroup barrier anywhere, the wave's lanes share
// LDS behind wave_sync) and writes one record of integer counts.
//
// Per frame t of the sequence's frame range, O = the GT rows of t (row order of the frame-sorted store), H = the detections of
// t whose track is >= 0 (compacted in row order):
//   distance  d[i][j] = 1 - IoU in float64 from float32 widths / heights, NaN above 0.5 -- every operation a single correctly
//             rounded IEEE operation in the host's order (contraction is OFF for this file: hipcc would otherwise fuse
//             w_o h_o + w_h h_h - inter and 1 - inter / union), so the matrix equals the host's bit for bit;
//   step 1    an object matched at t - 1 exactly keeps its hypothesis if that id is in H and the pair's distance is finite;
//   step 2    the rest by optimal assignment: masked / non-finite entries cost L = 2 min(|O|, |H|) (max finite + 1) + 1, the
//             full |O| x |H| matrix goes to the solver, an assigned pair that was finite is a match -- a SWITCH when the object
//             remembers another hypothesis id (however old);
//   counts    unmatched rows of O are misses, unmatched rows of H false positives; dist_sum adds the matched distances in
//             ascending position in O (one lane, in order: bit-equal to the host's sum).
//
// The solver is scipy's linear_sum_assignment INCLUDING its tie rules (csrc/wave_lsap.h, shared with the tracker: which optimum
// comes out decides the switches), the matrix transposed when it has more rows than columns.  Costs are read through the L-fill
// on the fly from the distance matrix, which stays as it was for the counts.
//
// Every loop is bounded by a count read from the store AFTER it was checked against the store's totals: a frame's offsets must be
// monotone inside the sequence's rows, permutation entries and object ids inside their ranges; a violation, a frame beyond
// MOT_MAX rows on either side, or a hypothesis id twice in a frame sets a flag bit in the sequence's record and ends the
// sequence (nothing is read outside the buffers; the other sequences of the launch are not affected).  The flag bits, the
// checks and the distance mot_dist are those of csrc/eval_common.h, shared with csrc/hota.hip and csrc/evalprep.hip.
#pragma clang fp contract(off)
#include "common.h"
#include "eval_common.h"
#include "wave_lsap.h"

using namespace tmpnn;

namespace {

constexpr int MOT_MAX = 256;                 // GT rows / kept hypotheses per frame (the solver's size)
constexpr int MOT_K = MOT_MAX / 64;          // columns per lane
constexpr int MOT_LDS_COST = 2048;           // distance matrices of up to this many entries stay in LDS (16 KiB)
constexpr int MOT_LDS_OBJ = 1024;            // sequences of up to this many objects keep m / last_match in LDS
constexpr size_t MOT_WS_COST = (size_t)MOT_MAX * MOT_MAX;      // doubles per sequence in the workspace
constexpr int MOT_NEVER = -0x7fffffff - 1;   // last_match of an object that was never matched (t - 1 of no frame: see below)

struct MotShared {
    LsapShared<MOT_MAX> L;
    double cost[MOT_LDS_COST];
    float4 obox[MOT_MAX], hbox[MOT_MAX];
    int oid[MOT_MAX], hid[MOT_MAX];
    int omatch[MOT_MAX];                     // position in H an object row was matched with, -1 none
    int m[MOT_LDS_OBJ], last[MOT_LDS_OBJ];
    unsigned char hmask[MOT_MAX];
};

// The cost the solver sees: entry (row, col) of the problem is D[row * sr + col * sc] unless the object / hypothesis of the
// pair was matched in step 1 or the distance is not finite -- then L.  (tr: the problem's rows are hypotheses.)
struct MotCost {
    const double* D;
    const int* omatch;
    const unsigned char* hmask;
    int sr, sc;
    bool tr;
    double L;
    __device__ __forceinline__ double at(int row, int col) const {
        const int i = tr ? col : row, j = tr ? row : col;
        const double d = D[(size_t)row * sr + (size_t)col * sc];
        return (omatch[i] >= 0 || hmask[j] || !box_finite(d)) ? L : d;
    }
};

// a sequence's slices of the store (eval_seq), fewer than max_det detections in it
__device__ __forceinline__ bool mot_seq(const tmpnn_mot_store& st, int s, EvalSeq& q, int64_t max_det = 0x7fffffff) {
    return eval_seq(st.seq, s, st.n_gt, st.n_det, st.n_off, st.n_obj, max_det, q);
}
// IDENT (tmpnn_mot_summary): the walk also keeps, per object, its events (`present`), the tracked ones, the fragmentation
// state (0 never tracked, 1 last event tracked, 2 missed after tracked) and count -- in LDS up to MOT_LDS_OBJ objects, in
// ws_obj (four arrays of obj_stride ints) beyond, as m / last -- and folds them into the (larger) record at the end.
struct MotObjShared { int present[MOT_LDS_OBJ], tracked[MOT_LDS_OBJ], state[MOT_LDS_OBJ], frag[MOT_LDS_OBJ]; };

template <bool IDENT, typename Rec>
__global__ __launch_bounds__(64) void k_mot_events(tmpnn_mot_store st, const int32_t* __restrict__ tracks, double* ws_cost,
                                                   int32_t* ws_m, int32_t* ws_last, int32_t* ws_tracks, int32_t* ws_obj,
                                                   size_t obj_stride, Rec* __restrict__ out) {
    __shared__ MotShared S;
    const int s = blockIdx.x, lane = threadIdx.x;
    EvalSeq q;
    bool ok = mot_seq(st, s, q);
    const int64_t gt_base = q.gt_base, n_gt = q.n_gt, det_base = q.det_base, n_det = q.n_det, off_base = q.off_base,
                  n_frames = q.n_frames, obj_base = q.obj_base, n_obj = q.n_obj;
    int64_t objects = 0, predictions = 0, matches = 0, switches = 0, fps = 0, misses = 0, flag = 0;
    double dist_sum = 0.0;
    if (!ok) flag = FLAG_STORE;
    const int32_t* gt_off = st.gt_off + off_base;
    const int32_t* det_off = st.det_off + off_base;
    const int32_t* gt_id = st.gt_id + gt_base;
    const float4* gt_box = reinterpret_cast<const float4*>(st.gt_box) + gt_base;
    const float4* det_box = reinterpret_cast<const float4*>(st.det_box) + det_base;
    const int32_t* perm = st.det_perm + det_base;
    const int32_t* trk = tracks + det_base;
    int32_t* trs = ws_tracks + det_base;                    // the tracks in frame-sorted order
    double* gcost = ws_cost + (size_t)s * MOT_WS_COST;
    int* m = n_obj <= MOT_LDS_OBJ ? S.m : ws_m + obj_base;
    int* last = n_obj <= MOT_LDS_OBJ ? S.last : ws_last + obj_base;
    int *present = nullptr, *tracked = nullptr, *state = nullptr, *frag = nullptr;
    if constexpr (IDENT) {
        __shared__ MotObjShared T;
        const bool lds = n_obj <= MOT_LDS_OBJ;
        present = lds ? T.present : ws_obj + obj_base;
        tracked = lds ? T.tracked : ws_obj + obj_stride + obj_base;
        state = lds ? T.state : ws_obj + 2 * obj_stride + obj_base;
        frag = lds ? T.frag : ws_obj + 3 * obj_stride + obj_base;
        if (ok)
            for (int64_t o = lane; o < n_obj; o += 64) present[o] = tracked[o] = state[o] = frag[o] = 0;
    }
    const int64_t n_walk = ok ? n_obj : 0;                   // objects whose state was initialised
    if (ok) {
        for (int64_t o = lane; o < n_obj; o += 64) { m[o] = -1; last[o] = MOT_NEVER; }
        bool bad = false;
        for (int64_t k = lane; k < n_det; k += 64) {
            const int p = perm[k];
            if (p < 0 || p >= n_det) { bad = true; trs[k] = -1; } else trs[k] = trk[p];
        }
        if (__ballot(bad)) { flag = FLAG_STORE; ok = false; }
        __threadfence();
        wave_sync();
    }
    const int nF = ok ? (int)n_frames : 0;
    for (int f = 0; f < nF; ++f) {
        int g0, g1, d0, d1;
        if (!eval_frame_rows(gt_off, det_off, f, q, g0, g1, d0, d1)) { flag = FLAG_STORE | ((int64_t)(f + 1) << 8); break; }
        const int nO = g1 - g0;
        // H: the detections of the frame with a track, in row order (ballot compaction, 64 rows a round)
        int nH = 0;
        for (int base = d0; base < d1; base += 64) {
            const int k = base + lane;
            const int id = k < d1 ? trs[k] : -1;
            const int p = wave_rank(id >= 0, lane, nH);
            if (id >= 0 && p < MOT_MAX) { S.hid[p] = id; S.hbox[p] = det_box[k]; S.hmask[p] = 0; }
        }
        objects += nO;
        predictions += nH;
        if (nO > MOT_MAX || nH > MOT_MAX) { flag = FLAG_LIMIT | ((int64_t)(f + 1) << 8); break; }
        bool bad = false;
        for (int i = lane; i < nO; i += 64) {
            const int o = gt_id[g0 + i];
            if (o < 0 || o >= n_obj) bad = true;
            S.oid[i] = o; S.obox[i] = gt_box[g0 + i]; S.omatch[i] = -1;
        }
        if (__ballot(bad)) { flag = FLAG_STORE | ((int64_t)(f + 1) << 8); break; }
        wave_sync();
        // a hypothesis id twice in the frame: the host definition raises
        if (wave_has_duplicate(S.hid, nH, lane)) { flag = FLAG_DUPLICATE | ((int64_t)(f + 1) << 8); break; }
        int nmatch = 0;
        if (nO > 0 && nH > 0) {
            const int t = f;                                  // frames are consecutive: t - 1 is f - 1 (MOT_NEVER is no frame's)
            double* D = nO * nH <= MOT_LDS_COST ? S.cost : gcost;
            double mx = -__builtin_huge_val();
            for (int x = lane; x < nO * nH; x += 64) D[x] = mot_dist(S.obox[x / nH], S.hbox[x % nH]);
            wave_sync();
            // step 1: hypothesis ids are unique in the frame and so are the remembered ids of the objects matched at t - 1, so
            // the rows are independent and a lane per row gives the sequential result
            for (int i = lane; i < nO; i += 64) {
                const int o = S.oid[i];
                if (last[o] == t - 1 && m[o] >= 0) {
                    const int want = m[o];
                    int j = -1;
                    for (int j2 = 0; j2 < nH; ++j2) if (j < 0 && S.hid[j2] == want) j = j2;
                    if (j >= 0 && box_finite(D[i * nH + j])) { S.omatch[i] = j; S.hmask[j] = 1; last[o] = t; }
                }
            }
            wave_sync();
            // step 2: the largest finite distance that is left, then the assignment over the L-filled matrix
            for (int x = lane; x < nO * nH; x += 64) {
                const double d = D[x];
                if (S.omatch[x / nH] < 0 && !S.hmask[x % nH] && box_finite(d)) mx = d > mx ? d : mx;
            }
            const uint64_t mxk = ~wave_min64(~key_f64(mx));
            if (mxk != key_f64(-__builtin_huge_val())) {
                // (undo the key map: the maximum itself, bit for bit)
                const uint64_t b = (mxk >> 63) ? (mxk & 0x7fffffffffffffffull) : ~mxk;
                mx = __longlong_as_double((long long)b);
                const bool tr = nH < nO;                          // (scipy transposes a tall matrix)
                MotCost C;
                C.D = D; C.omatch = S.omatch; C.hmask = S.hmask; C.tr = tr;
                C.sr = tr ? 1 : nH; C.sc = tr ? nH : 1;
                C.L = (double)(2 * (tr ? nH : nO)) * (mx + 1.0) + 1.0;
                const int nr = tr ? nH : nO, nc = tr ? nO : nH;
                // the solver must see the masks of step 1 only: its matches are collected first and applied afterwards
                if (!wave_lsap_solve(S.L, C, nr, nc, lane)) { flag = FLAG_SOLVER | ((int64_t)(f + 1) << 8); break; }
                wave_sync();
                int sw = 0;
                int newj[MOT_K];
#pragma unroll
                for (int k = 0; k < MOT_K; ++k) {
                    newj[k] = -1;
                    const int r = lane + 64 * k;
                    if (r < nr) {
                        const int c = S.L.col4row[r];
                        const int i = tr ? c : r, j = tr ? r : c;
                        if (c >= 0 && c < nc && S.omatch[i] < 0 && !S.hmask[j] && box_finite(D[i * nH + j])) newj[k] = (i << 16) | j;
                    }
                }
                wave_sync();
#pragma unroll
                for (int k = 0; k < MOT_K; ++k)
                    if (newj[k] >= 0) {
                        const int i = newj[k] >> 16, j = newj[k] & 0xffff, o = S.oid[i], h = S.hid[j];
                        if (m[o] >= 0 && m[o] != h) ++sw;
                        m[o] = h; last[o] = t;
                        S.omatch[i] = j; S.hmask[j] = 1;
                    }
                wave_sync();
                for (int d = 32; d >= 1; d >>= 1) sw += __shfl_xor(sw, d);
                switches += sw;
            }
            // the matched distances in ascending position in O: one running sum, every lane computes the same one
            for (int i = 0; i < nO; ++i) {
                const int j = S.omatch[i];
                if (j >= 0) { dist_sum += D[i * nH + j]; ++nmatch; }
            }
        }
        matches += nmatch;
        misses += nO - nmatch;
        fps += nH - nmatch;
        if constexpr (IDENT) {
            // one event per object of the frame (ids are unique in a frame: a lane per row)
            for (int i = lane; i < nO; i += 64) {
                const int o = S.oid[i];
                ++present[o];
                if (S.omatch[i] >= 0) {
                    ++tracked[o];
                    if (state[o] == 2) ++frag[o];
                    state[o] = 1;
                } else if (state[o] == 1) state[o] = 2;
            }
        }
        wave_sync();
    }
    int64_t mt = 0, pt = 0, ml = 0, fr = 0;
    if constexpr (IDENT) {
        wave_sync();
        for (int64_t o = lane; o < n_walk; o += 64) {
            const int p = present[o];
            if (p > 0) {
                const double ratio = (double)tracked[o] / (double)p;
                if (ratio >= 0.8) ++mt; else if (ratio < 0.2) ++ml; else ++pt;
            }
            fr += frag[o];
        }
        for (int d = 32; d >= 1; d >>= 1) {
            mt += __shfl_xor(mt, d); pt += __shfl_xor(pt, d); ml += __shfl_xor(ml, d); fr += __shfl_xor(fr, d);
        }
    }
    if (lane == 0) {
        Rec r;
        r.objects = objects; r.predictions = predictions; r.matches = matches; r.switches = switches;
        r.false_positives = fps; r.misses = misses; r.frames = n_frames; r.flag = flag; r.dist_sum = dist_sum;
        if constexpr (IDENT) {
            r.unique_objects = n_walk; r.mostly_tracked = mt; r.partially_tracked = pt; r.mostly_lost = ml; r.fragmentations = fr;
            r.idtp = -1; r.hypotheses = 0;                    // (k_mot_hyp, k_mot_idtp)
        }
        out[s] = r;
    }
}

constexpr int MD_THREADS = 256;
__global__ __launch_bounds__(MD_THREADS) void k_mot_dist(const float4* __restrict__ a, int na, const float4* __restrict__ b, int nb,
                                                         double* __restrict__ out) {
    const long total = (long)na * nb, stride = (long)gridDim.x * MD_THREADS;
    for (long x = (long)blockIdx.x * MD_THREADS + threadIdx.x; x < total; x += stride) out[x] = mot_dist(a[x / nb], b[x % nb]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Identity figures (tmpnn_mot_summary; host definition: trackmpnn_amd.moteval.mot_summary_host).  After the walk, three kernels:
//   k_mot_hyp    one workgroup per sequence: the dense index of every kept detection's hypothesis id (ids are arbitrary int32
//                and change with every evaluation), in order of first appearance in the frame-sorted rows -- an open-addressing
//                table in the workspace (integer CAS on the id, integer min on the first row), a scan over the first rows
//                (hyp_index, csrc/eval_common.h, shared with k_hota_prep);
//   k_mot_pairs  parallel over sequences and frames, a wave per frame: n[o][h] += 1 for every pair of the frame at a finite
//                mot_dist (the walk's function and predicate; integer atomics: the result does not depend on their order).
//                No per-frame limit: rows are read where they lie;
//   k_mot_idtp   one workgroup per sequence: the largest sum of n over one-to-one matchings, by shortest augmenting paths over
//                the integer costs wmax - n (every row of the smaller side is assigned, so the minimum is nr wmax - idtp).  The
//                value does not depend on which optimum is found, so no tie rule is restated here.
// A sequence the walk flagged takes no part (idtp = -1).  Every index is checked against the store's totals before it is used.
constexpr int MI_THREADS = 256;
constexpr int MI_WAVES = MI_THREADS / 64;
constexpr int MI_LDS_COL = 2048;             // the solver's column state stays in LDS up to this many columns (56 KiB)
constexpr int MI_FRAMES = 8;                 // frames of one workgroup of k_mot_pairs (two per wave)
constexpr int64_t MI_MAX_PAIR = (int64_t)1 << 40;
constexpr int64_t MI_MAX_DET = (int64_t)1 << 28;            // (table slots are int32: 4 n_det of them)

struct MotIdentWs {
    int32_t *tab_key, *tab_first, *tab_dense;               // [4 n_det]: a sequence's table starts at 4 det_base
    int32_t *slot, *hidx, *hcount;                          // [n_det]: table slot / dense hypothesis index of a sorted row; rows per hypothesis
    int64_t* cbase;                                         // [S]: first entry of the sequence's count matrix, -1 none
    int32_t* cnt;                                           // [n_pair]: n[o][h] at cbase + o * n_det + h
    long long *u, *v, *spc;                                 // solver: rows at obj_base, columns at obj_base + det_base
    int32_t *col4row, *SR, *path, *row4col, *done;
};

__global__ __launch_bounds__(MI_THREADS) void k_mot_hyp(tmpnn_mot_store st, const int32_t* __restrict__ ws_tracks, MotIdentWs W,
                                                        int64_t n_pair, tmpnn_mot_summary_record* out) {
    __shared__ int s_wave[MI_WAVES + 1];
    __shared__ long long s_sum[MI_WAVES];
    const int s = blockIdx.x, tid = threadIdx.x;
    EvalSeq q;
    const bool ok = mot_seq(st, s, q, MI_MAX_DET) && out[s].flag == 0;
    const long long cbase = pair_base<MI_THREADS>(st.seq, s, st.n_obj, st.n_det, n_pair, s_sum);      // of the count matrix
    const bool fits = ok && cbase <= n_pair && q.n_obj * q.n_det <= n_pair - cbase;      // (n_obj, n_det < 2^31: no overflow)
    int n_hyp = 0;
    if (fits) {                                              // (uniform over the workgroup)
        const int32_t* trs = ws_tracks + q.det_base;
        hyp_index<MI_THREADS>((int)q.n_det, [trs](int k) { return trs[k]; }, W.tab_key + 4 * q.det_base, W.tab_first + 4 * q.det_base,
                              W.tab_dense + 4 * q.det_base, W.slot + q.det_base, W.hidx + q.det_base, W.hcount + q.det_base, s_wave, n_hyp);
    }
    if (tid == 0) {
        W.cbase[s] = fits ? cbase : -1;
        out[s].hypotheses = n_hyp;
        if (ok && !fits) out[s].flag = FLAG_STORE;
    }
}

__global__ __launch_bounds__(MI_THREADS) void k_mot_pairs(tmpnn_mot_store st, const int32_t* __restrict__ ws_tracks, MotIdentWs W,
                                                          int frame_groups, const tmpnn_mot_summary_record* __restrict__ out) {
    const int s = blockIdx.x / frame_groups, group = blockIdx.x % frame_groups;      // (the grid is S x frame_groups blocks)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    EvalSeq q;
    if (!mot_seq(st, s, q) || out[s].flag != 0) return;
    const int64_t cbase = W.cbase[s];
    if (cbase < 0) return;
    const int32_t* gt_off = st.gt_off + q.off_base;
    const int32_t* det_off = st.det_off + q.off_base;
    const int32_t* gt_id = st.gt_id + q.gt_base;
    const float4* gt_box = reinterpret_cast<const float4*>(st.gt_box) + q.gt_base;
    const float4* det_box = reinterpret_cast<const float4*>(st.det_box) + q.det_base;
    const int32_t* trs = ws_tracks + q.det_base;
    const int32_t* hidx = W.hidx + q.det_base;
    int32_t* cnt = W.cnt + cbase;
    for (int r = 0; r < MI_FRAMES / MI_WAVES; ++r) {
        const int64_t f = (int64_t)group * MI_FRAMES + r * MI_WAVES + wave;
        if (f >= q.n_frames) return;
        int g0, g1, d0, d1;
        if (!eval_frame_rows(gt_off, det_off, f, q, g0, g1, d0, d1)) continue;                     // (the walk flags it)
        const int nD = d1 - d0;
        const int64_t total = (int64_t)(g1 - g0) * nD;
        for (int64_t x = lane; x < total; x += 64) {
            const int i = g0 + (int)(x / nD), k = d0 + (int)(x % nD);
            const int o = gt_id[i], h = trs[k] >= 0 ? hidx[k] : -1;
            if (o < 0 || o >= q.n_obj || h < 0 || h >= q.n_det) continue;
            if (box_finite(mot_dist(gt_box[i], det_box[k]))) atomicAdd(&cnt[(int64_t)o * q.n_det + h], 1);
        }
    }
}

struct MiKey { long long c; unsigned t; };                  // reduced cost, then (assigned << 31 | column): the smallest wins
__device__ __forceinline__ MiKey mi_min(MiKey a, MiKey b) { return (b.c < a.c || (b.c == a.c && b.t < a.t)) ? b : a; }

__global__ __launch_bounds__(MI_THREADS) void k_mot_idtp(tmpnn_mot_store st, MotIdentWs W, tmpnn_mot_summary_record* out) {
    __shared__ long long s_v[MI_LDS_COL], s_spc[MI_LDS_COL];
    __shared__ int s_path[MI_LDS_COL], s_row4col[MI_LDS_COL], s_done[MI_LDS_COL];
    __shared__ MiKey s_key[2][MI_WAVES];
    __shared__ int s_fail;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    EvalSeq q;
    const bool ok = mot_seq(st, s, q) && out[s].flag == 0 && W.cbase[s] >= 0;
    const int n_hyp = ok ? (int)out[s].hypotheses : 0;
    if (!ok || n_hyp < 0 || n_hyp > q.n_det) return;         // (idtp stays -1: no identity figures)
    if (q.n_obj == 0 || n_hyp == 0) { if (tid == 0) out[s].idtp = 0; return; }
    const int32_t* N = W.cnt + W.cbase[s];
    const bool tr = n_hyp < q.n_obj;                         // the smaller side is the rows
    const int nr = tr ? n_hyp : (int)q.n_obj, nc = tr ? (int)q.n_obj : n_hyp;
    const int64_t sr = tr ? 1 : q.n_det, sc = tr ? q.n_det : 1;
    long long* u = W.u + q.obj_base;
    int* col4row = W.col4row + q.obj_base;
    int* SR = W.SR + q.obj_base;
    const bool lds = nc <= MI_LDS_COL;
    const int64_t cb = q.obj_base + q.det_base;              // (nc <= max(n_obj, n_det) <= n_obj + n_det of the sequence)
    long long* v = lds ? s_v : W.v + cb;
    long long* spc = lds ? s_spc : W.spc + cb;
    int* path = lds ? s_path : W.path + cb;
    int* row4col = lds ? s_row4col : W.row4col + cb;
    int* done = lds ? s_done : W.done + cb;
    constexpr long long INF = 0x3fffffffffffffffll;
    int phase = 0;
    auto block_min = [&](MiKey k) {                          // (every thread; one barrier: the two buffers alternate)
        for (int d = 32; d >= 1; d >>= 1) {
            MiKey o;
            o.c = __shfl_xor(k.c, d); o.t = __shfl_xor(k.t, d);
            k = mi_min(k, o);
        }
        if (lane == 0) s_key[phase][wave] = k;
        __syncthreads();
        k = s_key[phase][0];
        for (int w = 1; w < MI_WAVES; ++w) k = mi_min(k, s_key[phase][w]);
        phase ^= 1;
        return k;
    };
    // wmax: the largest count (costs wmax - n are >= 0)
    MiKey mk = {0, 0};
    for (int64_t x = tid; x < (int64_t)nr * nc; x += MI_THREADS) {
        const long long c = -(long long)N[(x / nc) * sr + (x % nc) * sc];
        mk.c = c < mk.c ? c : mk.c;
    }
    const long long wmax = -block_min(mk).c;
    for (int i = tid; i < nr; i += MI_THREADS) { u[i] = 0; col4row[i] = -1; }
    for (int j = tid; j < nc; j += MI_THREADS) { v[j] = 0; row4col[j] = -1; }
    if (tid == 0) s_fail = 0;
    __syncthreads();
    for (int cur = 0; cur < nr; ++cur) {
        for (int j = tid; j < nc; j += MI_THREADS) { spc[j] = INF; path[j] = -1; done[j] = 0; }      // (column j: thread j % MI_THREADS)
        for (int i = tid; i < nr; i += MI_THREADS) SR[i] = 0;
        __syncthreads();
        int i = cur, sink = -1;
        long long min_val = 0;
        for (int it = 0; it < nc && sink < 0; ++it) {
            if (tid == 0) SR[i] = 1;
            const long long ui = u[i];
            MiKey best = {INF, 0xffffffffu};
            for (int j = tid; j < nc; j += MI_THREADS) {
                if (done[j]) continue;
                const long long r = min_val + (wmax - (long long)N[i * sr + j * sc]) - ui - v[j];
                if (r < spc[j]) { spc[j] = r; path[j] = i; }
                const MiKey k = {spc[j], (row4col[j] >= 0 ? 0x80000000u : 0u) | (unsigned)j};
                best = mi_min(best, k);
            }
            best = block_min(best);
            if (best.t == 0xffffffffu) break;                // (no column left: never spin)
            const int j = (int)(best.t & 0x7fffffffu);
            min_val = best.c;
            if ((j & (MI_THREADS - 1)) == tid) done[j] = 1;
            if (best.t & 0x80000000u) {
                i = row4col[j];
                if (i < 0 || i >= nr) break;
            } else sink = j;
        }
        if (sink < 0) { if (tid == 0) { out[s].flag = FLAG_SOLVER; } return; }       // (uniform: every thread holds the same sink)
        __syncthreads();
        // dual variables (with col4row as it was BEFORE the augmentation), then the augmentation along `path`
        for (int i2 = tid; i2 < nr; i2 += MI_THREADS)
            if (SR[i2]) u[i2] += (i2 == cur) ? min_val : (min_val - spc[col4row[i2]]);
        for (int j = tid; j < nc; j += MI_THREADS)
            if (done[j]) v[j] -= min_val - spc[j];
        __syncthreads();
        if (tid == 0) {
            int j = sink;
            for (int step = 0;; ++step) {
                const int ip = step <= nr ? path[j] : -1;     // (a path visits a row once: never spin)
                if (ip < 0 || ip >= nr) { s_fail = 1; break; }
                row4col[j] = ip;
                const int old = col4row[ip];
                col4row[ip] = j;
                j = old;
                if (ip == cur) break;
                if (j < 0 || j >= nc) { s_fail = 1; break; }
            }
        }
        __syncthreads();
        if (s_fail) { if (tid == 0) { out[s].flag = FLAG_SOLVER; } return; }
    }
    MiKey sum = {0, 0};
    for (int i = tid; i < nr; i += MI_THREADS) {
        const int j = col4row[i];
        if (j >= 0 && j < nc) sum.c += N[i * sr + j * sc];
    }
    for (int d = 32; d >= 1; d >>= 1) sum.c += __shfl_xor(sum.c, d);
    if (lane == 0) s_key[phase][wave] = sum;
    __syncthreads();
    if (tid == 0) {
        long long idtp = 0;
        for (int w = 0; w < MI_WAVES; ++w) idtp += s_key[phase][w].c;
        out[s].idtp = idtp;
    }
}

// the arguments tmpnn_mot_events and tmpnn_mot_summary share: the store, the host copy of its sequence table, the tracks
int mot_check_args(const char* fn, const tmpnn_mot_store* st, const int64_t* seq_host, const int32_t* tracks, const void* out) {
    TM_REQUIRE(st != nullptr, "%s: store is null", fn);
    return eval_check_store(fn, st->S, st->n_gt, st->n_det, st->n_off, &st->n_obj, seq_host, seq_host && st->seq && out,
                            "seq, seq_host or out", st->gt_off && st->det_off, st->gt_id && st->gt_box,
                            st->det_box && st->det_perm && tracks, st->gt_box, st->det_box, 0x7fffffff, EVAL_NO_LIMIT);
}

struct MotWalkWs { double* cost; int32_t *m, *last, *tracks; };
char* mot_carve_walk(char* p, int S, int64_t n_obj, int64_t n_det, MotWalkWs& w) {
    WsCarver c{p};
    w.cost = c.take<double>((size_t)S * MOT_WS_COST);
    w.m = c.take<int32_t>((size_t)n_obj);
    w.last = c.take<int32_t>((size_t)n_obj);
    w.tracks = c.take<int32_t>((size_t)n_det);
    return c.p;
}

// the workspace of tmpnn_mot_summary behind the walk's: per-object state, hypothesis tables, solver state, count matrices
char* mot_carve_ident(char* p, int S, int64_t n_obj, int64_t n_det, int64_t n_pair, int32_t*& obj, MotIdentWs& w) {
    WsCarver c{p};
    const size_t no = (size_t)n_obj, nd = (size_t)n_det, ncol = no + nd;
    obj = c.take<int32_t>(4 * (align16(no * 4) / 4));
    w.tab_key = c.take<int32_t>(4 * nd);
    w.tab_first = c.take<int32_t>(4 * nd);
    w.tab_dense = c.take<int32_t>(4 * nd);
    w.slot = c.take<int32_t>(nd);
    w.hidx = c.take<int32_t>(nd);
    w.hcount = c.take<int32_t>(nd);
    w.cbase = c.take<int64_t>((size_t)S);
    w.u = c.take<long long>(no);
    w.v = c.take<long long>(ncol);
    w.spc = c.take<long long>(ncol);
    w.col4row = c.take<int32_t>(no);
    w.SR = c.take<int32_t>(no);
    w.path = c.take<int32_t>(ncol);
    w.row4col = c.take<int32_t>(ncol);
    w.done = c.take<int32_t>(ncol);
    w.cnt = c.take<int32_t>((size_t)n_pair);
    return c.p;
}

}  // namespace

extern "C" size_t tmpnn_mot_events_ws(int S, int64_t n_obj, int64_t n_det) {
    if (S < 0 || n_obj < 0 || n_det < 0) return 0;
    return (size_t)S * MOT_WS_COST * sizeof(double) + 2 * align16((size_t)n_obj * 4) + align16((size_t)n_det * 4);
}

extern "C" int tmpnn_mot_max_per_frame(void) { return MOT_MAX; }

extern "C" int tmpnn_mot_events(const tmpnn_mot_store* st, const int64_t* seq_host, const int32_t* tracks, void* ws, size_t ws_bytes,
                                tmpnn_mot_record* out, tmpnn_stream stream) {
    if (const int rc = mot_check_args("mot_events", st, seq_host, tracks, out)) return rc;
    if (st->S == 0) return TMPNN_OK;
    const size_t need = tmpnn_mot_events_ws(st->S, st->n_obj, st->n_det);
    if (ws == nullptr || ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "mot_events: workspace %zu < %zu bytes", ws_bytes, need);
    TM_REQUIRE(aligned16(ws), "mot_events: workspace must be 16-byte aligned");
    MotWalkWs w;
    mot_carve_walk(static_cast<char*>(ws), st->S, st->n_obj, st->n_det, w);
    hipLaunchKernelGGL((k_mot_events<false, tmpnn_mot_record>), dim3(st->S), dim3(64), 0, as_stream(stream), *st, tracks, w.cost, w.m,
                       w.last, w.tracks, (int32_t*)nullptr, (size_t)0, out);
    return check_launch("mot_events");
}

extern "C" int tmpnn_mot_summary_limit(int which) {
    return which == 0 ? MOT_LDS_OBJ : which == 1 ? MI_LDS_COL : which == 2 ? MI_FRAMES : -1;
}

extern "C" size_t tmpnn_mot_summary_ws(int S, int64_t n_obj, int64_t n_det, int64_t n_pair) {
    if (S < 0 || n_obj < 0 || n_det < 0 || n_pair < 0 || n_det >= MI_MAX_DET || n_pair >= MI_MAX_PAIR) return 0;
    MotWalkWs w;
    MotIdentWs wi;
    int32_t* obj;
    char* const base = reinterpret_cast<char*>((uintptr_t)16);       // (only the distance is used)
    return (size_t)(mot_carve_ident(mot_carve_walk(base, S, n_obj, n_det, w), S, n_obj, n_det, n_pair, obj, wi) - base);
}

extern "C" int tmpnn_mot_summary(const tmpnn_mot_store* st, const int64_t* seq_host, const int32_t* tracks, void* ws, size_t ws_bytes,
                                 tmpnn_mot_summary_record* out, tmpnn_stream stream) {
    if (const int rc = mot_check_args("mot_summary", st, seq_host, tracks, out)) return rc;
    if (st->S == 0) return TMPNN_OK;
    TM_REQUIRE(st->n_det < MI_MAX_DET, "mot_summary: %lld detections (fewer than %lld expected)", (long long)st->n_det, (long long)MI_MAX_DET);
    int64_t n_pair = 0, max_frames = 0;
    for (int s = 0; s < st->S; ++s) {
        const int64_t* q = seq_host + (size_t)s * 8;
        n_pair += q[7] * q[3];                                // (n_obj and n_det of a sequence are below 2^31 and 2^28)
        TM_REQUIRE(n_pair < MI_MAX_PAIR, "mot_summary: the count matrices (n_obj x n_det per sequence) pass %lld entries", (long long)MI_MAX_PAIR);
        max_frames = q[5] > max_frames ? q[5] : max_frames;
    }
    const int frame_groups = max_frames > 0 ? ceil_div(max_frames, MI_FRAMES) : 1;
    TM_REQUIRE((int64_t)st->S * frame_groups < 0x7fffffff, "mot_summary: %d sequences x %d groups of %d frames pass the grid", st->S, frame_groups,
               MI_FRAMES);
    const size_t need = tmpnn_mot_summary_ws(st->S, st->n_obj, st->n_det, n_pair);
    if (ws == nullptr || ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "mot_summary: workspace %zu < %zu bytes", ws_bytes, need);
    TM_REQUIRE(aligned16(ws), "mot_summary: workspace must be 16-byte aligned");
    MotWalkWs w;
    MotIdentWs wi;
    int32_t* obj;
    mot_carve_ident(mot_carve_walk(static_cast<char*>(ws), st->S, st->n_obj, st->n_det, w), st->S, st->n_obj, st->n_det, n_pair, obj, wi);
    hipStream_t hs = as_stream(stream);
    if (n_pair > 0) {
        const hipError_t e = hipMemsetAsync(wi.cnt, 0, (size_t)n_pair * 4, hs);
        if (e != hipSuccess) return set_error(TMPNN_ELAUNCH, "mot_summary: clearing the count matrices: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL((k_mot_events<true, tmpnn_mot_summary_record>), dim3(st->S), dim3(64), 0, hs, *st, tracks, w.cost, w.m, w.last,
                       w.tracks, obj, align16((size_t)st->n_obj * 4) / 4, out);
    if (const int rc = check_launch("mot_summary (walk)")) return rc;
    hipLaunchKernelGGL(k_mot_hyp, dim3(st->S), dim3(MI_THREADS), 0, hs, *st, w.tracks, wi, n_pair, out);
    if (const int rc = check_launch("mot_summary (hypothesis index)")) return rc;
    hipLaunchKernelGGL(k_mot_pairs, dim3(st->S * frame_groups), dim3(MI_THREADS), 0, hs, *st, w.tracks, wi, frame_groups, out);
    if (const int rc = check_launch("mot_summary (pair counts)")) return rc;
    hipLaunchKernelGGL(k_mot_idtp, dim3(st->S), dim3(MI_THREADS), 0, hs, *st, wi, out);
    return check_launch("mot_summary (assignment)");
}

extern "C" int tmpnn_mot_dist(const float* box_a, int na, const float* box_b, int nb, double* out, tmpnn_stream stream) {
    TM_REQUIRE(na >= 0 && nb >= 0, "mot_dist: na=%d nb=%d", na, nb);
    if (na == 0 || nb == 0) return TMPNN_OK;
    TM_REQUIRE(box_a && box_b && out, "mot_dist: null pointer");
    TM_REQUIRE(aligned16(box_a) && aligned16(box_b), "mot_dist: boxes must be 16-byte aligned");
    int blocks = ceil_div((long)na * nb, MD_THREADS);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_mot_dist, dim3(blocks), dim3(MD_THREADS), 0, as_stream(stream), reinterpret_cast<const float4*>(box_a), na,
                       reinterpret_cast<const float4*>(box_b), nb, out);
    return check_launch("mot_dist");
}
