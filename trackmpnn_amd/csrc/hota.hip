// HOTA of a set of tracks against the ground truth, on the device (tmpnn_hota; include/tmpnn.h; host definition:
// trackmpnn_amd.hota.hota_host, which restates TrackEval's metrics/hota.py with a stated order for every float sum).  The record
// equals the host's: integers exactly, every double bit for bit -- both sides are the same IEEE operations in the same order
// (contraction is OFF for this file), and there is no float atomic anywhere.  One clear of the workspace and four launches,
// whatever the number of sequences:
//   k_hota_prep    one workgroup per sequence: the tracks in frame-sorted order, the dense index of every kept detection's
//                  hypothesis id in order of first appearance (hyp_index, csrc/eval_common.h, as k_mot_hyp of csrc/moteval.hip:
//                  an open-addressing table, integer CAS / min, a scan over the first rows), tc[h] = rows per hypothesis, gc[o] =
//                  rows per object;
//   k_hota_align   pass A, one wave per sequence walks the frames in order: row and column sums of the frame's similarity
//                  matrix sequentially per lane, then a lane per pair adds sim / (colsum + rowsum - sim) into pm[o][h] (ids
//                  are unique in a frame: no two lanes meet; across frames the order is the walk's).  It also checks every frame
//                  (offsets, the per-frame limit, ids in range, a hypothesis id twice) and flags the sequence;
//   k_hota_match   pass B, parallel over sequences and frames, one wave per frame: the assignment of -(gas sim) by the wave
//                  solver (csrc/wave_lsap.h: scipy's linear_sum_assignment with its tie rules; the matrix transposed when it has
//                  more rows than columns), gas = pm / (gc + tc - pm) by the one division.  Scores of frames up to
//                  HOTA_LDS_SCORE pairs are formed once into LDS; beyond, the cost functor recomputes them.  Then the matched
//                  pairs in ascending GT position: lane a holds alpha index a, counts the pair iff sim >= thresholds[a], adds sim
//                  to its partial loc sum, and adds 1 to mc[o][h][a] and (once per frame) to tp[a] with integer atomics.  The
//                  frame's 19 partial sums go to the frame's slot;
//   k_hota_fold    one workgroup per sequence: the slots added in frame order, the three association sums per (alpha, object)
//                  over the hypotheses in ascending index and then, by one thread per alpha, over the objects; the record.
// The similarity is recomputed wherever it is needed (one function, the same inputs: the same bits).  Every index is checked
// against the store's totals before it is used; a sequence that fails a check is flagged, stops, and leaves the others alone.
#pragma clang fp contract(off)
#include "common.h"
#include "eval_common.h"
#include "wave_lsap.h"

using namespace tmpnn;

namespace {

constexpr int HOTA_MAX = 256;                // GT rows / kept hypotheses per frame (the solver's size)
constexpr int HOTA_NA = 19;                  // alphas
constexpr int HOTA_LDS_SCORE = 1024;         // frames of up to this many pairs keep the solver's scores in LDS (8 KiB a wave)
constexpr int HP_THREADS = 256;
constexpr int HP_WAVES = HP_THREADS / 64;
constexpr int HM_WAVES = 2;                  // waves of one workgroup of k_hota_match
constexpr int HM_FRAMES = 8;                 // frames of one workgroup of k_hota_match (four per wave)
constexpr int64_t HOTA_MAX_DET = (int64_t)1 << 28;          // (table slots are int32: 4 n_det of them)
constexpr int64_t HOTA_MAX_PAIR = ((int64_t)1 << 31) / (8 + 4 * HOTA_NA);

// a sequence's slices of the store (eval_seq)
__device__ __forceinline__ bool hota_seq(const tmpnn_mot_store& st, int s, EvalSeq& q) {
    return eval_seq(st.seq, s, st.n_gt, st.n_det, st.n_off, st.n_obj, HOTA_MAX_DET, q);
}

struct HotaThr { double v[HOTA_NA]; };       // ALPHAS - EPS, by value in the kernel arguments

struct HotaWs {
    // cleared by every call (one contiguous range)
    double* pm;                              // [n_pair]: a sequence's matrix at cbase, entry o * n_det + h
    int32_t* mc;                             // [n_pair][19]
    double* loc;                             // [n_off][19]: frame f of a sequence at off_base + f
    unsigned long long* tp;                  // [S][19]
    unsigned long long* flag;                // [S]: tmpnn_hota_record::flag
    // written before they are read
    int32_t* trs;                            // [n_det]: the tracks in frame-sorted order
    int32_t *tab_key, *tab_first, *tab_dense;               // [4 n_det]: a sequence's table starts at 4 det_base
    int32_t *slot, *hidx, *tc;               // [n_det]: table slot / dense hypothesis index of a sorted row; rows per hypothesis
    int32_t* gc;                             // [n_obj]: rows per object
    int64_t* cbase;                          // [S]: first entry of the sequence's pair matrices, -1 none
    int32_t* n_hyp;                          // [S]
    int64_t* n_trk;                          // [S]: kept detections
    double* part;                            // [3][n_obj * 19]: the association sums of (object, alpha), at obj_base * 19
};

__global__ __launch_bounds__(HP_THREADS) void k_hota_prep(tmpnn_mot_store st, const int32_t* __restrict__ tracks, HotaWs W, int64_t n_pair) {
    __shared__ int s_wave[HP_WAVES + 1];
    __shared__ long long s_sum[HP_WAVES];
    __shared__ int s_bad;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    EvalSeq q;
    const bool ok = hota_seq(st, s, q);
    if (tid == 0) s_bad = 0;
    const long long cbase = pair_base<HP_THREADS>(st.seq, s, st.n_obj, st.n_det, n_pair, s_sum);       // of the pair matrices
    const bool fits = ok && cbase <= n_pair && q.n_obj * q.n_det <= n_pair - cbase;      // (n_obj < 2^31, n_det < 2^28: no overflow)
    int n_hyp = 0;
    long long n_trk = 0;
    if (fits) {                                              // (uniform over the workgroup)
        const int n_det = (int)q.n_det;
        int32_t* trs = W.trs + q.det_base;
        int32_t* gc = W.gc + q.obj_base;
        const int32_t* perm = st.det_perm + q.det_base;
        const int32_t* trk = tracks + q.det_base;
        const int32_t* gt_id = st.gt_id + q.gt_base;
        bool bad = false;
        for (int64_t o = tid; o < q.n_obj; o += HP_THREADS) gc[o] = 0;
        // the track of a sorted row, on the way the tracks in frame-sorted order and their number
        auto id_of = [&](int k) {
            const int p = perm[k];
            int id = -1;
            if (p < 0 || p >= n_det) bad = true; else id = trk[p];
            trs[k] = id;
            n_trk += id >= 0;
            return id;
        };
        hyp_index<HP_THREADS>(n_det, id_of, W.tab_key + 4 * q.det_base, W.tab_first + 4 * q.det_base, W.tab_dense + 4 * q.det_base,
                              W.slot + q.det_base, W.hidx + q.det_base, W.tc + q.det_base, s_wave, n_hyp);
        for (int64_t i = tid; i < q.n_gt; i += HP_THREADS) {      // (gc was cleared before the barriers of hyp_index)
            const int o = gt_id[i];
            if (o < 0 || o >= q.n_obj) bad = true; else atomicAdd(&gc[o], 1);
        }
        if (bad) s_bad = 1;
    }
    for (int d = 32; d >= 1; d >>= 1) n_trk += __shfl_xor(n_trk, d);
    __syncthreads();                                         // (s_sum was read by every thread before the first barrier inside)
    if (lane == 0) s_sum[wave] = n_trk;
    __syncthreads();
    if (tid == 0) {
        long long t = 0;
        for (int w = 0; w < HP_WAVES; ++w) t += s_sum[w];
        W.cbase[s] = fits ? cbase : -1;
        W.n_hyp[s] = n_hyp;
        W.n_trk[s] = t;
        if (!fits || s_bad) eval_flag_first(&W.flag[s], FLAG_STORE, 0);
    }
}

// what a wave holds of one frame: the GT rows, and the kept detections (a track >= 0) compacted in row order
struct HotaFrame {
    float4 obox[HOTA_MAX], hbox[HOTA_MAX];
    int oid[HOTA_MAX], hh[HOTA_MAX];
};

// Loads frame f into F; nO / nH: the rows on both sides.  Returns 0, or the flag bits of the frame (FLAG_STORE: an offset or an
// id out of range; FLAG_LIMIT: more than HOTA_MAX rows on a side) -- then F is not to be used.  One wave.
__device__ __forceinline__ int hota_load_frame(const tmpnn_mot_store& st, const EvalSeq& q, const HotaWs& W, int64_t f, int lane,
                                               HotaFrame& F, int& nO, int& nH) {
    const int32_t* gt_off = st.gt_off + q.off_base;
    const int32_t* det_off = st.det_off + q.off_base;
    const int32_t* gt_id = st.gt_id + q.gt_base;
    const float4* gt_box = reinterpret_cast<const float4*>(st.gt_box) + q.gt_base;
    const float4* det_box = reinterpret_cast<const float4*>(st.det_box) + q.det_base;
    const int32_t* trs = W.trs + q.det_base;
    const int32_t* hidx = W.hidx + q.det_base;
    nO = nH = 0;
    int g0, g1, d0, d1;
    if (!eval_frame_rows(gt_off, det_off, f, q, g0, g1, d0, d1)) return FLAG_STORE;
    nO = g1 - g0;
    bool bad = false;
    for (int base = d0; base < d1; base += 64) {
        const int k = base + lane;
        const int id = k < d1 ? trs[k] : -1;
        const int p = wave_rank(id >= 0, lane, nH);
        if (id >= 0) {
            const int h = hidx[k];
            if (h < 0 || h >= q.n_det) bad = true;
            if (p < HOTA_MAX) { F.hh[p] = h; F.hbox[p] = det_box[k]; }
        }
    }
    if (nO > HOTA_MAX || nH > HOTA_MAX) return FLAG_LIMIT;
    for (int i = lane; i < nO; i += 64) {
        const int o = gt_id[g0 + i];
        if (o < 0 || o >= q.n_obj) bad = true;
        F.oid[i] = o; F.obox[i] = gt_box[g0 + i];
    }
    if (__ballot(bad)) return FLAG_STORE;
    wave_sync();
    return 0;
}

__global__ __launch_bounds__(64) void k_hota_align(tmpnn_mot_store st, HotaWs W) {
    __shared__ HotaFrame F;
    __shared__ double s_rs[HOTA_MAX], s_cs[HOTA_MAX];
    const int s = blockIdx.x, lane = threadIdx.x;
    EvalSeq q;
    if (!hota_seq(st, s, q) || eval_load(&W.flag[s]) != 0) return;
    const int64_t cbase = W.cbase[s];
    if (cbase < 0) return;
    double* pm = W.pm + cbase;
    for (int64_t f = 0; f < q.n_frames; ++f) {
        int nO, nH;
        const int bits = hota_load_frame(st, q, W, f, lane, F, nO, nH);
        if (bits) { if (lane == 0) eval_flag_first(&W.flag[s], bits, f + 1); return; }
        // a hypothesis id twice in the frame: the host definition raises
        if (wave_has_duplicate(F.hh, nH, lane)) { if (lane == 0) eval_flag_first(&W.flag[s], FLAG_DUPLICATE, f + 1); return; }
        if (nO > 0 && nH > 0) {
            for (int i = lane; i < nO; i += 64) {            // row sums, in ascending column
                double a = 0.0;
                for (int j = 0; j < nH; ++j) a += hota_sim(F.obox[i], F.hbox[j]);
                s_rs[i] = a;
            }
            for (int j = lane; j < nH; j += 64) {            // column sums, in ascending row
                double a = 0.0;
                for (int i = 0; i < nO; ++i) a += hota_sim(F.obox[i], F.hbox[j]);
                s_cs[j] = a;
            }
            wave_sync();
            for (int x = lane; x < nO * nH; x += 64) {
                const int i = x / nH, j = x % nH;
                const double sim = hota_sim(F.obox[i], F.hbox[j]);
                const double den = (s_cs[j] + s_rs[i]) - sim;
                if (den > 0.0 + EVAL_EPS) {
                    double* at = pm + (int64_t)F.oid[i] * q.n_det + F.hh[j];
                    *at = *at + sim / den;
                }
            }
        }
        // another lane takes the pair in a later frame: the wave's stores are complete and visible to its lanes behind this (one
        // compute unit, one write-through L1: workgroup scope is enough, as for the walk's per-object state in csrc/moteval.hip)
        wave_sync();
    }
}

// The cost the solver sees: entry (row, col) of the problem is -(gas sim) of the pair (tr: the problem's rows are hypotheses),
// from LDS where the frame's scores were formed there, recomputed otherwise.
struct HotaCost {
    const HotaFrame* F;
    const double* score;                     // [nO * nH] in LDS, or null
    const double* pm;
    const int32_t *gc, *tc;
    int64_t n_det;
    int nH;
    bool tr;
    __device__ __forceinline__ double pair(int i, int j) const {
        const int o = F->oid[i], h = F->hh[j];
        const double p = pm[(int64_t)o * n_det + h];
        const double gas = p / ((double)(gc[o] + tc[h]) - p);
        return -(gas * hota_sim(F->obox[i], F->hbox[j]));
    }
    __device__ __forceinline__ double at(int row, int col) const {
        const int i = tr ? col : row, j = tr ? row : col;
        return score ? score[i * nH + j] : pair(i, j);
    }
};

struct HotaMatchShared {
    LsapShared<HOTA_MAX> L;
    HotaFrame F;
    double score[HOTA_LDS_SCORE];
    int omatch[HOTA_MAX];                    // position in H an object row was matched with, -1 none
};

__global__ __launch_bounds__(64 * HM_WAVES) void k_hota_match(tmpnn_mot_store st, HotaWs W, HotaThr thr, int frame_groups) {
    __shared__ HotaMatchShared s_all[HM_WAVES];
    const int s = blockIdx.x / frame_groups, group = blockIdx.x % frame_groups;      // (the grid is S x frame_groups blocks)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    HotaMatchShared& S = s_all[wave];
    EvalSeq q;
    if (!hota_seq(st, s, q) || eval_load(&W.flag[s]) != 0) return;                    // (k_hota_align flagged it)
    const int64_t cbase = W.cbase[s];
    if (cbase < 0) return;
    HotaCost C;
    C.F = &S.F; C.pm = W.pm + cbase; C.gc = W.gc + q.obj_base; C.tc = W.tc + q.det_base; C.n_det = q.n_det;
    int32_t* mc = W.mc + cbase * HOTA_NA;
    const double my_thr = thr.v[lane < HOTA_NA ? lane : 0];
    for (int r = 0; r < HM_FRAMES / HM_WAVES; ++r) {
        const int64_t f = (int64_t)group * HM_FRAMES + r * HM_WAVES + wave;
        if (f >= q.n_frames) return;
        int nO, nH;
        if (hota_load_frame(st, q, W, f, lane, S.F, nO, nH) || nO == 0 || nH == 0) { wave_sync(); continue; }
        const bool lds = nO * nH <= HOTA_LDS_SCORE;
        C.nH = nH; C.tr = nH < nO;                           // (scipy transposes a tall matrix)
        C.score = nullptr;
        if (lds) {
            for (int x = lane; x < nO * nH; x += 64) S.score[x] = C.pair(x / nH, x % nH);
            C.score = S.score;
        }
        for (int i = lane; i < nO; i += 64) S.omatch[i] = -1;
        wave_sync();
        const int nr = C.tr ? nH : nO, nc = C.tr ? nO : nH;
        if (!wave_lsap_solve(S.L, C, nr, nc, lane)) { if (lane == 0) eval_flag_first(&W.flag[s], FLAG_SOLVER, f + 1); return; }
        wave_sync();
        for (int row = lane; row < nr; row += 64) {
            const int c = S.L.col4row[row];
            if (c >= 0 && c < nc) S.omatch[C.tr ? c : row] = C.tr ? row : c;
        }
        wave_sync();
        // the matched pairs in ascending GT position; lane a is alpha index a: one running sum per lane, in order
        double loc = 0.0;
        int cnt = 0;
        for (int i = 0; i < nO; ++i) {
            const int j = S.omatch[i];
            if (j < 0) continue;                             // (uniform over the wave)
            const double sim = hota_sim(S.F.obox[i], S.F.hbox[j]);
            if (lane < HOTA_NA && sim >= my_thr) {
                loc += sim;
                ++cnt;
                atomicAdd(&mc[((int64_t)S.F.oid[i] * q.n_det + S.F.hh[j]) * HOTA_NA + lane], 1);
            }
        }
        if (lane < HOTA_NA) {
            W.loc[(q.off_base + f) * HOTA_NA + lane] = loc;
            if (cnt) atomicAdd(&W.tp[(size_t)s * HOTA_NA + lane], (unsigned long long)cnt);
        }
        wave_sync();
    }
}

__global__ __launch_bounds__(HP_THREADS) void k_hota_fold(tmpnn_mot_store st, HotaWs W, tmpnn_hota_record* __restrict__ out) {
    const int s = blockIdx.x, tid = threadIdx.x;
    EvalSeq q;
    const bool ok = hota_seq(st, s, q);
    const int64_t cbase = ok ? W.cbase[s] : -1;
    const unsigned long long flag = eval_load(&W.flag[s]);
    int n_hyp = ok ? W.n_hyp[s] : 0;
    if (n_hyp < 0 || n_hyp > q.n_det) n_hyp = 0;
    const bool live = ok && cbase >= 0 && flag == 0;
    const int64_t n_part = (int64_t)st.n_obj * HOTA_NA;      // (the stride of the three planes of `part`)
    double* part = W.part + q.obj_base * HOTA_NA;
    if (live) {
        const int32_t* mc = W.mc + cbase * HOTA_NA;
        const int32_t* gc = W.gc + q.obj_base;
        const int32_t* tc = W.tc + q.det_base;
        for (int64_t x = tid; x < q.n_obj * HOTA_NA; x += HP_THREADS) {        // x = o * 19 + a: neighbours read neighbours
            const int64_t o = x / HOTA_NA;
            const int a = (int)(x % HOTA_NA);
            const int g = gc[o];
            double sa = 0.0, sre = 0.0, spr = 0.0;
            for (int h = 0; h < n_hyp; ++h) {
                const int m = mc[(o * q.n_det + h) * HOTA_NA + a];
                if (m == 0) continue;                        // (the host adds 0.0 there: no bit changes)
                const int t = tc[h];
                const double md = (double)m;
                const int da = g + t - m;
                sa += md * (md / (double)(da > 1 ? da : 1));
                sre += md * (md / (double)(g > 1 ? g : 1));
                spr += md * (md / (double)(t > 1 ? t : 1));
            }
            part[x] = sa; part[n_part + x] = sre; part[2 * n_part + x] = spr;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (tid < HOTA_NA) {
        tmpnn_hota_record& r = out[s];
        double loc = 0.0, sa = 0.0, sre = 0.0, spr = 0.0;
        if (live) {
            const double* slots = W.loc + q.off_base * HOTA_NA;
            for (int64_t f = 0; f < q.n_frames; ++f) loc += slots[f * HOTA_NA + tid];
            for (int64_t o = 0; o < q.n_obj; ++o) {
                const int64_t x = o * HOTA_NA + tid;
                sa += part[x]; sre += part[n_part + x]; spr += part[2 * n_part + x];
            }
        }
        r.tp[tid] = live ? (int64_t)W.tp[(size_t)s * HOTA_NA + tid] : 0;
        r.loc_sum[tid] = loc; r.ass_a_num[tid] = sa; r.ass_re_num[tid] = sre; r.ass_pr_num[tid] = spr;
        if (tid == 0) {
            r.gt_dets = ok ? q.n_gt : 0;
            r.tracker_dets = ok ? W.n_trk[s] : 0;
            r.objects = ok ? q.n_obj : 0;
            r.hypotheses = n_hyp;
            r.flag = (int64_t)flag;
        }
    }
}

// carves the workspace; *cleared: the bytes from the start that every call clears
char* hota_carve(char* p, int S, int64_t n_obj, int64_t n_det, int64_t n_off, int64_t n_pair, HotaWs& w, size_t* cleared) {
    WsCarver c{p};
    const size_t no = (size_t)n_obj, nd = (size_t)n_det, np = (size_t)n_pair;
    w.pm = c.take<double>(np);
    w.mc = c.take<int32_t>(np * HOTA_NA);
    w.loc = c.take<double>((size_t)n_off * HOTA_NA);
    w.tp = c.take<unsigned long long>((size_t)S * HOTA_NA);
    w.flag = c.take<unsigned long long>((size_t)S);
    *cleared = (size_t)(c.p - p);
    w.trs = c.take<int32_t>(nd);
    w.tab_key = c.take<int32_t>(4 * nd);
    w.tab_first = c.take<int32_t>(4 * nd);
    w.tab_dense = c.take<int32_t>(4 * nd);
    w.slot = c.take<int32_t>(nd);
    w.hidx = c.take<int32_t>(nd);
    w.tc = c.take<int32_t>(nd);
    w.gc = c.take<int32_t>(no);
    w.cbase = c.take<int64_t>((size_t)S);
    w.n_hyp = c.take<int32_t>((size_t)S);
    w.n_trk = c.take<int64_t>((size_t)S);
    w.part = c.take<double>(3 * no * HOTA_NA);
    return c.p;
}

}  // namespace

extern "C" size_t tmpnn_hota_ws(int S, int64_t n_obj, int64_t n_det, int64_t n_off, int64_t n_pair) {
    if (S < 0 || n_obj < 0 || n_det < 0 || n_off < 0 || n_pair < 0 || n_det >= HOTA_MAX_DET || n_pair > HOTA_MAX_PAIR ||
        n_obj >= 0x7fffffff || n_off >= ((int64_t)1 << 40))
        return 0;
    HotaWs w;
    size_t cleared;
    char* const base = reinterpret_cast<char*>((uintptr_t)16);       // (only the distance is used)
    return (size_t)(hota_carve(base, S, n_obj, n_det, n_off, n_pair, w, &cleared) - base);
}

extern "C" int tmpnn_hota(const tmpnn_mot_store* st, const int64_t* seq_host, const int32_t* tracks, const double* thresholds, void* ws,
                          size_t ws_bytes, tmpnn_hota_record* out, tmpnn_stream stream) {
    TM_REQUIRE(st != nullptr, "hota: store is null");
    if (const int rc = eval_check_store("hota", st->S, st->n_gt, st->n_det, st->n_off, &st->n_obj, seq_host,
                                        seq_host && st->seq && out && thresholds, "seq, seq_host, thresholds or out",
                                        st->gt_off && st->det_off, st->gt_id && st->gt_box, st->det_box && st->det_perm && tracks,
                                        st->gt_box, st->det_box, EVAL_NO_LIMIT, 0x7fffffff))
        return rc;
    if (st->S == 0) return TMPNN_OK;
    TM_REQUIRE(st->n_det < HOTA_MAX_DET, "hota: %lld detections (fewer than %lld expected)", (long long)st->n_det, (long long)HOTA_MAX_DET);
    HotaThr thr;
    for (int a = 0; a < HOTA_NA; ++a) {
        thr.v[a] = thresholds[a];
        TM_REQUIRE(thr.v[a] == thr.v[a] && (a == 0 || thr.v[a] > thr.v[a - 1]), "hota: thresholds must ascend (index %d)", a);
    }
    int64_t n_pair = 0, max_frames = 0;
    for (int s = 0; s < st->S; ++s) {
        const int64_t* q = seq_host + (size_t)s * 8;
        TM_REQUIRE(q[7] == 0 || q[3] <= HOTA_MAX_PAIR / q[7], "hota: sequence %d: the pair workspace (n_obj x n_det) passes %lld entries", s,
                   (long long)HOTA_MAX_PAIR);
        n_pair += q[7] * q[3];
        TM_REQUIRE(n_pair <= HOTA_MAX_PAIR, "hota: the pair workspace (n_obj x n_det per sequence) passes %lld entries", (long long)HOTA_MAX_PAIR);
        max_frames = q[5] > max_frames ? q[5] : max_frames;
    }
    const int frame_groups = max_frames > 0 ? ceil_div(max_frames, HM_FRAMES) : 1;
    TM_REQUIRE((int64_t)st->S * frame_groups < 0x7fffffff, "hota: %d sequences x %d groups of %d frames pass the grid", st->S, frame_groups, HM_FRAMES);
    const size_t need = tmpnn_hota_ws(st->S, st->n_obj, st->n_det, st->n_off, n_pair);
    TM_REQUIRE(need > 0, "hota: the store is beyond the workspace's limits");
    if (ws == nullptr || ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "hota: workspace %zu < %zu bytes", ws_bytes, need);
    TM_REQUIRE(aligned16(ws), "hota: workspace must be 16-byte aligned");
    HotaWs w;
    size_t cleared;
    hota_carve(static_cast<char*>(ws), st->S, st->n_obj, st->n_det, st->n_off, n_pair, w, &cleared);
    hipStream_t hs = as_stream(stream);
    const hipError_t e = hipMemsetAsync(ws, 0, cleared, hs);
    if (e != hipSuccess) return set_error(TMPNN_ELAUNCH, "hota: clearing the workspace: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_hota_prep, dim3(st->S), dim3(HP_THREADS), 0, hs, *st, tracks, w, n_pair);
    if (const int rc = check_launch("hota (hypothesis index)")) return rc;
    hipLaunchKernelGGL(k_hota_align, dim3(st->S), dim3(64), 0, hs, *st, w);
    if (const int rc = check_launch("hota (alignment)")) return rc;
    hipLaunchKernelGGL(k_hota_match, dim3(st->S * frame_groups), dim3(64 * HM_WAVES), 0, hs, *st, w, thr, frame_groups);
    if (const int rc = check_launch("hota (matching)")) return rc;
    hipLaunchKernelGGL(k_hota_fold, dim3(st->S), dim3(HP_THREADS), 0, hs, *st, w, out);
    return check_launch("hota (fold)");
}
