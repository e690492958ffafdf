// CLEAR-MOT events of a set of tracks against the ground truth, on the device (tmpnn_mot_events, tmpnn_mot_dist; include/tmpnn.h;
// host definition: trackmpnn_amd.moteval.mot_events_host).  The reference feeds py-motmetrics one frame at a time on the host
// (utils/metrics.py:7-61); the rule is sequential in the frames of a sequence and independent across sequences, so ONE WAVE per
// sequence walks the frames (one workgroup of 64 threads per sequence: no workgroup barrier anywhere, the wave's lanes share
// LDS behind mot_wave_sync) and writes one record of integer counts.
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
// The solver is scipy's linear_sum_assignment (rectangular_lsap.cpp: shortest augmenting paths in fp64, the matrix transposed
// when it has more rows than columns) restated step for step INCLUDING its tie rules, as csrc/trackops.hip restates it for the
// tracker's float costs (see the top of that file): the scan over `remaining` keeps the first column of minimal reduced cost
// unless a later one of equal cost is unassigned (then the last such); `remaining` is filled in reverse and compacted by moving
// its last entry into the hole.  Which optimum comes out decides the switches.  Lane l owns columns l, l + 64, l + 128, l + 192
// (reduced costs, duals, path, position in `remaining` in registers); the row state lives in LDS.  Costs are read through the
// L-fill on the fly from the distance matrix, which stays as it was for the counts.
//
// Every loop is bounded by a count read from the store AFTER it was checked against the store's totals: a frame's offsets must be
// monotone inside the sequence's rows, permutation entries and object ids inside their ranges; a violation, a frame beyond
// MOT_MAX rows on either side, or a hypothesis id twice in a frame sets a flag bit in the sequence's record and ends the
// sequence (nothing is read outside the buffers; the other sequences of the launch are not affected).
#pragma clang fp contract(off)
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int MOT_MAX = 256;                 // GT rows / kept hypotheses per frame (the solver's size)
constexpr int MOT_K = MOT_MAX / 64;          // columns per lane
constexpr int MOT_LDS_COST = 2048;           // distance matrices of up to this many entries stay in LDS (16 KiB)
constexpr int MOT_LDS_OBJ = 1024;            // sequences of up to this many objects keep m / last_match in LDS
constexpr size_t MOT_WS_COST = (size_t)MOT_MAX * MOT_MAX;      // doubles per sequence in the workspace
constexpr int MOT_NEVER = -0x7fffffff - 1;   // last_match of an object that was never matched (t - 1 of no frame: see below)

enum { FLAG_LIMIT = 1, FLAG_DUPLICATE = 2, FLAG_STORE = 4, FLAG_SOLVER = 8 };

struct MotShared {
    double u[MOT_MAX], spc[MOT_MAX];
    double cost[MOT_LDS_COST];
    float4 obox[MOT_MAX], hbox[MOT_MAX];
    int col4row[MOT_MAX], path[MOT_MAX];
    int oid[MOT_MAX], hid[MOT_MAX];
    int omatch[MOT_MAX];                     // position in H an object row was matched with, -1 none
    int m[MOT_LDS_OBJ], last[MOT_LDS_OBJ];
    unsigned char SR[MOT_MAX], hmask[MOT_MAX];
};

__device__ __forceinline__ void mot_wave_sync() {          // LDS writes of this wave visible to its other lanes (one wave only)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// np.maximum / np.minimum: the first operand where it is larger (smaller) or NaN
__device__ __forceinline__ double mot_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double mot_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ bool mot_finite(double x) { return __builtin_fabs(x) < __builtin_huge_val(); }

// 1 - IoU of two x1 y1 x2 y2 boxes, NaN above 0.5 (host: moteval.mot_dist_host, the same operations in the same order)
__device__ __forceinline__ double mot_dist(float4 o, float4 h) {
    const float wo = o.z - o.x, ho = o.w - o.y, wh = h.z - h.x, hh = h.w - h.y;      // float32, as metrics.py:37,39
    const double otx = o.x, oty = o.y, htx = h.x, hty = h.y;
    const double obx = otx + (double)wo, oby = oty + (double)ho, hbx = htx + (double)wh, hby = hty + (double)hh;
    const double iw = mot_max(mot_min(obx, hbx) - mot_max(otx, htx), 0.0);
    const double ih = mot_max(mot_min(oby, hby) - mot_max(oty, hty), 0.0);
    const double inter = iw * ih;
    const double uni = ((double)wo * (double)ho + (double)wh * (double)hh) - inter;
    double d = 1.0 - inter / uni;
    if (d > 0.5) d = __builtin_nan("");
    return d;
}

__device__ __forceinline__ uint64_t mot_key(double x) {        // order-preserving: a < b  <=>  key(a) < key(b)   (no NaNs here)
    const uint64_t b = (uint64_t)__double_as_longlong(x + 0.0);           // (-0.0 -> +0.0: scipy compares with ==)
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// Wave-wide minima of unsigned keys: four DPP exchange steps inside each row of 16 lanes (quad_perm xor 1, xor 2,
// row_half_mirror, row_mirror), then the four rows through v_readlane -- no LDS crossbar on the solver's scan.
template <int CTRL>
__device__ __forceinline__ uint32_t mot_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t mot_min_step64(uint64_t x) {
    const uint64_t y = ((uint64_t)mot_dpp<CTRL>((uint32_t)(x >> 32)) << 32) | mot_dpp<CTRL>((uint32_t)x);
    return y < x ? y : x;
}
template <int CTRL>
__device__ __forceinline__ uint32_t mot_min_step32(uint32_t x) { const uint32_t y = mot_dpp<CTRL>(x); return y < x ? y : x; }
__device__ __forceinline__ uint64_t mot_wave_min64(uint64_t x) {
    x = mot_min_step64<0xB1>(x);          // quad_perm [1,0,3,2]
    x = mot_min_step64<0x4E>(x);          // quad_perm [2,3,0,1]
    x = mot_min_step64<0x141>(x);         // row_half_mirror
    x = mot_min_step64<0x140>(x);         // row_mirror: every lane of a row of 16 holds the row's minimum
    uint64_t m = ~0ull;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t y = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(x >> 32), 16 * r) << 32) | (uint32_t)__builtin_amdgcn_readlane((uint32_t)x, 16 * r);
        m = y < m ? y : m;
    }
    return m;
}
__device__ __forceinline__ uint32_t mot_wave_min32(uint32_t x) {
    x = mot_min_step32<0xB1>(x);
    x = mot_min_step32<0x4E>(x);
    x = mot_min_step32<0x141>(x);
    x = mot_min_step32<0x140>(x);
    uint32_t m = ~0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const uint32_t y = (uint32_t)__builtin_amdgcn_readlane(x, 16 * r); m = y < m ? y : m; }
    return m;
}
__device__ __forceinline__ double mot_readlane_f64(double x, int l) {
    const long long b = __double_as_longlong(x);
    return __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(b >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)b, l));
}

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
        return (omatch[i] >= 0 || hmask[j] || !mot_finite(d)) ? L : d;
    }
};

// rows i < nr <= nc columns; result in S.col4row[0..nr); false when no augmenting path was found (cannot happen with finite costs)
__device__ bool mot_wave_solve(MotShared& S, const MotCost& C, int nr, int nc, int lane) {
    double v[MOT_K];
    int r4c[MOT_K];
#pragma unroll
    for (int k = 0; k < MOT_K; ++k) { v[k] = 0.0; r4c[k] = -1; }
    for (int i = lane; i < nr; i += 64) { S.u[i] = 0.0; S.col4row[i] = -1; }
    mot_wave_sync();
    const int KU = (nc + 63) >> 6;                        // column groups in use
    for (int cur = 0; cur < nr; ++cur) {
        double spc[MOT_K];
        int path[MOT_K], pos[MOT_K];
        bool alive[MOT_K], scj[MOT_K];
#pragma unroll
        for (int k = 0; k < MOT_K; ++k) {
            const int j = lane + 64 * k;
            spc[k] = __builtin_huge_val(); path[k] = -1; pos[k] = nc - 1 - j; alive[k] = j < nc; scj[k] = false;
        }
        for (int i = lane; i < nr; i += 64) S.SR[i] = 0;
        mot_wave_sync();
        int i = cur, sink = -1, num_rem = nc;
        double min_val = 0.0;
        while (sink < 0 && num_rem > 0) {
            if (lane == 0) S.SR[i] = 1;
            const double ui = S.u[i];
            double m = __builtin_huge_val();
#pragma unroll
            for (int k = 0; k < MOT_K; ++k) {
                if (k < KU && alive[k]) {
                    const double r = min_val + C.at(i, lane + 64 * k) - ui - v[k];
                    if (r < spc[k]) { path[k] = i; spc[k] = r; }
                    m = spc[k] < m ? spc[k] : m;
                }
            }
            // the minimum, then the scan's choice among the columns that attain it: an unassigned one if there is any (the one at
            // the HIGHEST position of `remaining`), else the one at the lowest position -- one key: unassigned first
            const uint64_t mk = mot_wave_min64(mot_key(m));
            uint32_t sel = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < MOT_K; ++k)
                if (k < KU && alive[k] && mot_key(spc[k]) == mk) {
                    const uint32_t q = r4c[k] == -1 ? (uint32_t)(MOT_MAX - 1 - pos[k]) : (uint32_t)(MOT_MAX + pos[k]);
                    sel = q < sel ? q : sel;
                }
            sel = mot_wave_min32(sel);
            if (sel == 0xFFFFFFFFu) return false;                // (no live column attains the minimum: never spin)
            const int ipos = sel < (uint32_t)MOT_MAX ? MOT_MAX - 1 - (int)sel : (int)sel - MOT_MAX;
            int jsel = -1, r4sel = -2;
#pragma unroll
            for (int k = 0; k < MOT_K; ++k) {
                const bool mine = k < KU && alive[k] && pos[k] == ipos;
                const unsigned long long bal = __ballot(mine);
                if (bal) {                                       // (exactly one column sits at a position)
                    const int src = __ffsll((long long)bal) - 1;
                    jsel = src + 64 * k;
                    r4sel = __builtin_amdgcn_readlane(r4c[k], src);
                    m = mot_readlane_f64(spc[k], src);
                }
            }
            if (jsel < 0) return false;
            min_val = m;
            if (r4sel == -1) sink = jsel; else i = r4sel;
#pragma unroll
            for (int k = 0; k < MOT_K; ++k) {
                if (lane + 64 * k == jsel) { scj[k] = true; alive[k] = false; }
                else if (alive[k] && pos[k] == num_rem - 1) pos[k] = ipos;
            }
            --num_rem;
        }
        if (sink < 0) return false;
        // dual variables (with col4row as it was BEFORE the augmentation), then the augmentation along `path`
#pragma unroll
        for (int k = 0; k < MOT_K; ++k)
            if (lane + 64 * k < nc) { S.spc[lane + 64 * k] = spc[k]; S.path[lane + 64 * k] = path[k]; }
        mot_wave_sync();
        for (int i2 = lane; i2 < nr; i2 += 64)
            if (S.SR[i2]) S.u[i2] += (i2 == cur) ? min_val : (min_val - S.spc[S.col4row[i2]]);
#pragma unroll
        for (int k = 0; k < MOT_K; ++k)
            if (scj[k]) v[k] -= min_val - spc[k];
        mot_wave_sync();
        int j = sink;
        for (int step = 0;; ++step) {
            if (step > nr) return false;                          // (a path visits a row once: never spin)
            const int ip = S.path[j];
            if (ip < 0 || ip >= nr) return false;
#pragma unroll
            for (int k = 0; k < MOT_K; ++k)
                if (lane + 64 * k == j) r4c[k] = ip;
            const int old = S.col4row[ip];
            mot_wave_sync();
            if (lane == 0) S.col4row[ip] = j;
            mot_wave_sync();
            j = old;
            if (ip == cur) break;
            if (j < 0 || j >= nc) return false;
        }
    }
    return true;
}

__global__ __launch_bounds__(64) void k_mot_events(tmpnn_mot_store st, const int32_t* __restrict__ tracks, double* ws_cost,
                                                   int32_t* ws_m, int32_t* ws_last, int32_t* ws_tracks,
                                                   tmpnn_mot_record* __restrict__ out) {
    __shared__ MotShared S;
    const int s = blockIdx.x, lane = threadIdx.x;
    const int64_t* q = st.seq + (size_t)s * 8;
    const int64_t gt_base = q[0], n_gt = q[1], det_base = q[2], n_det = q[3], off_base = q[4], n_frames = q[5], obj_base = q[6],
                  n_obj = q[7];
    int64_t objects = 0, predictions = 0, matches = 0, switches = 0, fps = 0, misses = 0, flag = 0;
    double dist_sum = 0.0;
    // the sequence's slices must lie inside the store (the host checked its own copy of the table before the launch; this is
    // the table the kernel indexes by)
    bool ok = gt_base >= 0 && n_gt >= 0 && gt_base + n_gt <= st.n_gt && det_base >= 0 && n_det >= 0 && det_base + n_det <= st.n_det &&
              off_base >= 0 && n_frames >= 0 && off_base + n_frames + 1 <= st.n_off && obj_base >= 0 && n_obj >= 0 &&
              obj_base + n_obj <= st.n_obj && n_gt < 0x7fffffff && n_det < 0x7fffffff && n_frames < 0x7fffffff;
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
    if (ok) {
        for (int64_t o = lane; o < n_obj; o += 64) { m[o] = -1; last[o] = MOT_NEVER; }
        bool bad = false;
        for (int64_t k = lane; k < n_det; k += 64) {
            const int p = perm[k];
            if (p < 0 || p >= n_det) { bad = true; trs[k] = -1; } else trs[k] = trk[p];
        }
        if (__ballot(bad)) { flag = FLAG_STORE; ok = false; }
        __threadfence();
        mot_wave_sync();
    }
    const int nF = ok ? (int)n_frames : 0;
    for (int f = 0; f < nF; ++f) {
        const int g0 = gt_off[f], g1 = gt_off[f + 1], d0 = det_off[f], d1 = det_off[f + 1];
        if (g0 < 0 || g1 < g0 || g1 > n_gt || d0 < 0 || d1 < d0 || d1 > n_det) { flag = FLAG_STORE | ((int64_t)(f + 1) << 8); break; }
        const int nO = g1 - g0;
        // H: the detections of the frame with a track, in row order (ballot compaction, 64 rows a round)
        int nH = 0;
        for (int base = d0; base < d1; base += 64) {
            const int k = base + lane;
            const int id = k < d1 ? trs[k] : -1;
            const unsigned long long bal = __ballot(id >= 0);
            if (id >= 0) {
                const int p = nH + __popcll(bal & ((1ull << lane) - 1ull));
                if (p < MOT_MAX) { S.hid[p] = id; S.hbox[p] = det_box[k]; S.hmask[p] = 0; }
            }
            nH += __popcll(bal);
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
        mot_wave_sync();
        // a hypothesis id twice in the frame: the host definition raises
        bool dup = false;
        for (int j = lane; j < nH; j += 64) {
            const int id = S.hid[j];
            for (int j2 = 0; j2 < j; ++j2) dup |= S.hid[j2] == id;
        }
        if (__ballot(dup)) { flag = FLAG_DUPLICATE | ((int64_t)(f + 1) << 8); break; }
        int nmatch = 0;
        if (nO > 0 && nH > 0) {
            const int t = f;                                  // frames are consecutive: t - 1 is f - 1 (MOT_NEVER is no frame's)
            double* D = nO * nH <= MOT_LDS_COST ? S.cost : gcost;
            double mx = -__builtin_huge_val();
            for (int x = lane; x < nO * nH; x += 64) D[x] = mot_dist(S.obox[x / nH], S.hbox[x % nH]);
            mot_wave_sync();
            // step 1: hypothesis ids are unique in the frame and so are the remembered ids of the objects matched at t - 1, so
            // the rows are independent and a lane per row gives the sequential result
            for (int i = lane; i < nO; i += 64) {
                const int o = S.oid[i];
                if (last[o] == t - 1 && m[o] >= 0) {
                    const int want = m[o];
                    int j = -1;
                    for (int j2 = 0; j2 < nH; ++j2) if (j < 0 && S.hid[j2] == want) j = j2;
                    if (j >= 0 && mot_finite(D[i * nH + j])) { S.omatch[i] = j; S.hmask[j] = 1; last[o] = t; }
                }
            }
            mot_wave_sync();
            // step 2: the largest finite distance that is left, then the assignment over the L-filled matrix
            for (int x = lane; x < nO * nH; x += 64) {
                const double d = D[x];
                if (S.omatch[x / nH] < 0 && !S.hmask[x % nH] && mot_finite(d)) mx = d > mx ? d : mx;
            }
            const uint64_t mxk = ~mot_wave_min64(~mot_key(mx));
            if (mxk != mot_key(-__builtin_huge_val())) {
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
                if (!mot_wave_solve(S, C, nr, nc, lane)) { flag = FLAG_SOLVER | ((int64_t)(f + 1) << 8); break; }
                mot_wave_sync();
                int sw = 0;
                int newj[MOT_K];
#pragma unroll
                for (int k = 0; k < MOT_K; ++k) {
                    newj[k] = -1;
                    const int r = lane + 64 * k;
                    if (r < nr) {
                        const int c = S.col4row[r];
                        const int i = tr ? c : r, j = tr ? r : c;
                        if (c >= 0 && c < nc && S.omatch[i] < 0 && !S.hmask[j] && mot_finite(D[i * nH + j])) newj[k] = (i << 16) | j;
                    }
                }
                mot_wave_sync();
#pragma unroll
                for (int k = 0; k < MOT_K; ++k)
                    if (newj[k] >= 0) {
                        const int i = newj[k] >> 16, j = newj[k] & 0xffff, o = S.oid[i], h = S.hid[j];
                        if (m[o] >= 0 && m[o] != h) ++sw;
                        m[o] = h; last[o] = t;
                        S.omatch[i] = j; S.hmask[j] = 1;
                    }
                mot_wave_sync();
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
        mot_wave_sync();
    }
    if (lane == 0) {
        tmpnn_mot_record r;
        r.objects = objects; r.predictions = predictions; r.matches = matches; r.switches = switches;
        r.false_positives = fps; r.misses = misses; r.frames = n_frames; r.flag = flag; r.dist_sum = dist_sum;
        out[s] = r;
    }
}

constexpr int MD_THREADS = 256;
__global__ __launch_bounds__(MD_THREADS) void k_mot_dist(const float4* __restrict__ a, int na, const float4* __restrict__ b, int nb,
                                                         double* __restrict__ out) {
    const long total = (long)na * nb, stride = (long)gridDim.x * MD_THREADS;
    for (long x = (long)blockIdx.x * MD_THREADS + threadIdx.x; x < total; x += stride) out[x] = mot_dist(a[x / nb], b[x % nb]);
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t tmpnn_mot_events_ws(int S, int64_t n_obj, int64_t n_det) {
    if (S < 0 || n_obj < 0 || n_det < 0) return 0;
    return (size_t)S * MOT_WS_COST * sizeof(double) + 2 * align16((size_t)n_obj * 4) + align16((size_t)n_det * 4);
}

extern "C" int tmpnn_mot_max_per_frame(void) { return MOT_MAX; }

extern "C" int tmpnn_mot_events(const tmpnn_mot_store* st, const int64_t* seq_host, const int32_t* tracks, void* ws, size_t ws_bytes,
                                tmpnn_mot_record* out, tmpnn_stream stream) {
    TM_REQUIRE(st != nullptr, "mot_events: store is null");
    TM_REQUIRE(st->S >= 0 && st->n_gt >= 0 && st->n_det >= 0 && st->n_off >= 0 && st->n_obj >= 0,
               "mot_events: S=%d n_gt=%lld n_det=%lld n_off=%lld n_obj=%lld", st->S, (long long)st->n_gt, (long long)st->n_det,
               (long long)st->n_off, (long long)st->n_obj);
    if (st->S == 0) return TMPNN_OK;
    TM_REQUIRE(seq_host && st->seq && out, "mot_events: null pointer (seq, seq_host or out)");
    TM_REQUIRE(st->n_off == 0 || (st->gt_off && st->det_off), "mot_events: null offsets");
    TM_REQUIRE(st->n_gt == 0 || (st->gt_id && st->gt_box), "mot_events: null GT arrays");
    TM_REQUIRE(st->n_det == 0 || (st->det_box && st->det_perm && tracks), "mot_events: null detection arrays or tracks");
    TM_REQUIRE(aligned16(st->gt_box) && aligned16(st->det_box), "mot_events: boxes must be 16-byte aligned");
    for (int s = 0; s < st->S; ++s) {
        const int64_t* q = seq_host + (size_t)s * 8;
        TM_REQUIRE(q[0] >= 0 && q[1] >= 0 && q[1] < 0x7fffffff && q[0] + q[1] <= st->n_gt, "mot_events: sequence %d: GT rows [%lld, +%lld) of %lld", s,
                   (long long)q[0], (long long)q[1], (long long)st->n_gt);
        TM_REQUIRE(q[2] >= 0 && q[3] >= 0 && q[3] < 0x7fffffff && q[2] + q[3] <= st->n_det, "mot_events: sequence %d: detection rows [%lld, +%lld) of %lld",
                   s, (long long)q[2], (long long)q[3], (long long)st->n_det);
        TM_REQUIRE(q[4] >= 0 && q[5] >= 0 && q[5] < 0x7fffffff && q[4] + q[5] + 1 <= st->n_off, "mot_events: sequence %d: offsets [%lld, +%lld + 1) of %lld",
                   s, (long long)q[4], (long long)q[5], (long long)st->n_off);
        TM_REQUIRE(q[6] >= 0 && q[7] >= 0 && q[6] + q[7] <= st->n_obj, "mot_events: sequence %d: objects [%lld, +%lld) of %lld", s,
                   (long long)q[6], (long long)q[7], (long long)st->n_obj);
    }
    const size_t need = tmpnn_mot_events_ws(st->S, st->n_obj, st->n_det);
    if (ws == nullptr || ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "mot_events: workspace %zu < %zu bytes", ws_bytes, need);
    TM_REQUIRE(aligned16(ws), "mot_events: workspace must be 16-byte aligned");
    char* p = static_cast<char*>(ws);
    double* ws_cost = reinterpret_cast<double*>(p);
    p += (size_t)st->S * MOT_WS_COST * sizeof(double);
    int32_t* ws_m = reinterpret_cast<int32_t*>(p);
    p += align16((size_t)st->n_obj * 4);
    int32_t* ws_last = reinterpret_cast<int32_t*>(p);
    p += align16((size_t)st->n_obj * 4);
    int32_t* ws_tracks = reinterpret_cast<int32_t*>(p);
    hipLaunchKernelGGL(k_mot_events, dim3(st->S), dim3(64), 0, as_stream(stream), *st, tracks, ws_cost, ws_m, ws_last, ws_tracks, out);
    return check_launch("mot_events");
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
