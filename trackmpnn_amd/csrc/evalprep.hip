// The KITTI benchmark's preprocessing of a set of tracks, on the device (tmpnn_evalprep; include/tmpnn.h; host definition:
// trackmpnn_amd.evalprep.evalprep_frame_host, which restates TrackEval's datasets/kitti_2d_box.py:get_preprocessed_seq_data):
// per frame the tracker rows of the class are assigned to the GT rows of the class and its distractors, rows matched to a
// distractor or to an occluded / truncated object are removed, and so are unmatched rows that are too small or lie in an
// ignore region.  The host resolved the rules into one code byte per row (struct tmpnn_evalprep_store): no rule logic here.
// One clear of the records and one launch, whatever the number of sequences:
//   k_evalprep     parallel over sequences and frames, one wave per frame (EP_WAVES waves and EP_FRAMES frames a workgroup, as
//                  k_hota_match): the tracker rows (track >= 0, code 1) and the matching GT rows (codes 1 .. 3) compacted into
//                  LDS by ballots, in row order; the scores (hota_sim, entries below 0.5 - eps set to 0) into LDS for frames up
//                  to EP_LDS_SCORE pairs, recomputed by the cost functor beyond; the assignment of -score by the wave solver
//                  (csrc/wave_lsap.h, the matrix transposed when it has more rows than columns); a pair is matched iff its score
//                  exceeds eps.  Then a lane per tracker row: the fate of a matched row from the code of its GT row, of an
//                  unmatched one from its height and from the intersection-over-own-area with every ignore region of the
//                  frame.  tracks_out of every detection row of the frame is written, and the seven counts go into the
//                  sequence's record with integer atomics (one add a count per wave).
// The scores are the same IEEE operations in the same order as the host's (contraction is OFF for this file).  No float atomic,
// no wait on another workgroup.  Every index is checked against the store's totals before it is used; a failed check, a frame
// beyond the limit or a solver that gives up sets the sequence's flag word (the first flag stays) and leaves the others alone.
// The flag bits, the checks, hota_sim and ep_ioa are those of csrc/eval_common.h, shared with csrc/moteval.hip and csrc/hota.hip.
#pragma clang fp contract(off)
#include "common.h"
#include "eval_common.h"
#include "wave_lsap.h"

using namespace tmpnn;

namespace {

constexpr int EP_MAX = 256;                  // detection rows / GT rows per frame, all categories (the solver's size)
constexpr int EP_LDS_SCORE = 1024;           // frames of up to this many pairs keep the solver's scores in LDS (8 KiB a wave)
constexpr int EP_WAVES = 2;                  // waves of one workgroup
constexpr int EP_FRAMES = 8;                 // frames of one workgroup (four per wave)
constexpr int NCOUNT = 7;                    // rows_in, other_class, removed_distractor / occluded / small / ignored, kept

enum { GT_OUT = 0, GT_SCORED = 1, GT_HARD = 2, GT_DISTRACTOR = 3, GT_REGION = 4 };
enum { C_ROWS = 0, C_OTHER = 1, C_DISTRACTOR = 2, C_OCCLUDED = 3, C_SMALL = 4, C_IGNORED = 5, C_KEPT = 6 };

// what a wave holds of one frame: the matching GT rows and the tracker rows, both compacted in row order
struct EpFrame {
    float4 gbox[EP_MAX], tbox[EP_MAX];
    int tarr[EP_MAX];                        // arrival index of a tracker row, relative to det_base
    int tmatch[EP_MAX];                      // position among the matching GT rows a tracker row was matched with, -1 none
    unsigned char gcode[EP_MAX];
};

// The cost the solver sees: entry (row, col) of the problem is -score of the pair (tr: the problem's rows are tracker rows),
// from LDS where the frame's scores were formed there, recomputed otherwise.
struct EpCost {
    const EpFrame* F;
    const double* score;                     // [nG * nT] in LDS, or null
    int nT;
    bool tr;
    __device__ __forceinline__ double pair(int i, int j) const {
        const double s = hota_sim(F->gbox[i], F->tbox[j]);
        return s < 0.5 - EVAL_EPS ? 0.0 : s;
    }
    __device__ __forceinline__ double at(int row, int col) const {
        const int i = tr ? col : row, j = tr ? row : col;
        return -(score ? score[i * nT + j] : pair(i, j));
    }
};

struct EpShared {
    LsapShared<EP_MAX> L;
    EpFrame F;
    double score[EP_LDS_SCORE];
};

__device__ __forceinline__ int ep_count(bool p) { return __popcll(__ballot(p)); }
__device__ __forceinline__ void ep_flag(tmpnn_evalprep_record* rec, int bits, int64_t frame1) {     // (the record's flag word)
    eval_flag_first(reinterpret_cast<unsigned long long*>(&rec->flag), bits, frame1);
}

__global__ __launch_bounds__(64 * EP_WAVES) void k_evalprep(tmpnn_evalprep_store st, const int32_t* __restrict__ tracks,
                                                            int32_t* __restrict__ tracks_out, tmpnn_evalprep_record* __restrict__ out,
                                                            int frame_groups) {
    __shared__ EpShared s_all[EP_WAVES];
    const int s = blockIdx.x / frame_groups, group = blockIdx.x % frame_groups;      // (the grid is S x frame_groups blocks)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    EpShared& S = s_all[wave];
    EvalSeq q;
    if (!eval_seq<false>(st.seq, s, st.n_gt, st.n_det, st.n_off, 0, 0x7fffffff, q)) {
        if (group == 0 && threadIdx.x == 0) ep_flag(&out[s], FLAG_STORE, 0);
        return;
    }
    const int32_t* gt_off = st.gt_off + q.off_base;
    const int32_t* det_off = st.det_off + q.off_base;
    const unsigned char* gt_code = st.gt_code + q.gt_base;
    const unsigned char* det_code = st.det_code + q.det_base;
    const float4* gt_box = reinterpret_cast<const float4*>(st.gt_box) + q.gt_base;
    const float4* det_box = reinterpret_cast<const float4*>(st.det_box) + q.det_base;
    const int32_t* perm = st.det_perm + q.det_base;
    const int32_t* trk = tracks + q.det_base;
    int32_t* trk_out = tracks_out + q.det_base;
    const int n_det = (int)q.n_det;
    EpCost C;
    C.F = &S.F;
    int cnt[NCOUNT];                         // (uniform over the wave)
#pragma unroll
    for (int c = 0; c < NCOUNT; ++c) cnt[c] = 0;
    for (int r = 0; r < EP_FRAMES / EP_WAVES; ++r) {
        const int64_t f = (int64_t)group * EP_FRAMES + r * EP_WAVES + wave;
        if (f >= q.n_frames) break;
        int g0, g1, d0, d1;
        if (!eval_frame_rows(gt_off, det_off, f, q, g0, g1, d0, d1)) {
            if (lane == 0) ep_flag(&out[s], FLAG_STORE, f + 1);
            continue;
        }
        if (g1 - g0 > EP_MAX || d1 - d0 > EP_MAX) {
            if (lane == 0) ep_flag(&out[s], FLAG_LIMIT, f + 1);
            continue;
        }
        // the tracker rows of the frame, in row order; every other detection row is done at once
        int nT = 0, rows_in = 0;
        bool bad = false;
        for (int base = d0; base < d1; base += 64) {
            const int k = base + lane;
            int p = -1, id = -1;
            bool cls = false;
            if (k < d1) {
                p = perm[k];
                if (p < 0 || p >= n_det) { bad = true; p = -1; } else { id = trk[p]; cls = det_code[k] == 1; }
            }
            const bool is_trk = id >= 0 && cls;
            const int at = wave_rank(is_trk, lane, nT);              // (< EP_MAX: the frame has at most EP_MAX rows)
            rows_in += ep_count(id >= 0);
            if (is_trk) {
                S.F.tarr[at] = p; S.F.tbox[at] = det_box[k]; S.F.tmatch[at] = -1;
            } else if (p >= 0) {
                trk_out[p] = -1;
            }
        }
        if (__ballot(bad)) {
            if (lane == 0) ep_flag(&out[s], FLAG_STORE, f + 1);
            wave_sync();
            continue;
        }
        // the GT rows of the matching (the class, scored or not, and its distractors), in row order
        int nG = 0;
        for (int base = g0; base < g1; base += 64) {
            const int k = base + lane;
            const int code = k < g1 ? gt_code[k] : GT_OUT;
            const bool part = code >= GT_SCORED && code <= GT_DISTRACTOR;
            const int at = wave_rank(part, lane, nG);
            if (part) { S.F.gbox[at] = gt_box[k]; S.F.gcode[at] = (unsigned char)code; }
        }
        wave_sync();
        if (nT > 0 && nG > 0) {
            C.nT = nT; C.tr = nT < nG;                           // (scipy transposes a tall matrix)
            C.score = nullptr;
            if (nG * nT <= EP_LDS_SCORE) {
                for (int x = lane; x < nG * nT; x += 64) S.score[x] = C.pair(x / nT, x % nT);
                C.score = S.score;
                wave_sync();
            }
            const int nr = C.tr ? nT : nG, nc = C.tr ? nG : nT;
            if (!wave_lsap_solve(S.L, C, nr, nc, lane)) {
                if (lane == 0) ep_flag(&out[s], FLAG_SOLVER, f + 1);
                wave_sync();
                continue;
            }
            wave_sync();
            for (int row = lane; row < nr; row += 64) {
                const int c = S.L.col4row[row];
                if (c < 0 || c >= nc) continue;
                const int i = C.tr ? c : row, j = C.tr ? row : c;
                if (-C.at(row, c) > 0.0 + EVAL_EPS) S.F.tmatch[j] = i;
            }
            wave_sync();
        }
        // the fate of every tracker row: a lane per row
        for (int base = 0; base < nT; base += 64) {
            const int j = base + lane;
            int fate = -1;
            if (j < nT) {
                const float4 b = S.F.tbox[j];
                const int i = S.F.tmatch[j];
                if (i >= 0) {
                    const int code = S.F.gcode[i];
                    fate = code == GT_DISTRACTOR ? C_DISTRACTOR : code == GT_HARD ? C_OCCLUDED : C_KEPT;
                } else if ((double)(b.w - b.y) <= st.height_thr) {
                    fate = C_SMALL;
                } else {
                    fate = C_KEPT;
                    for (int k = g0; k < g1; ++k)
                        if (gt_code[k] == GT_REGION && ep_ioa(b, gt_box[k]) > 0.5 + EVAL_EPS) fate = C_IGNORED;
                }
                const int p = S.F.tarr[j];
                trk_out[p] = fate == C_KEPT ? trk[p] : -1;
            }
#pragma unroll
            for (int c = C_DISTRACTOR; c <= C_KEPT; ++c) cnt[c] += ep_count(fate == c);
        }
        cnt[C_ROWS] += rows_in;
        cnt[C_OTHER] += rows_in - nT;
        wave_sync();                                             // (the next frame overwrites the wave's LDS)
    }
    if (lane < NCOUNT) {
        int mine = 0;
#pragma unroll
        for (int c = 0; c < NCOUNT; ++c) mine = lane == c ? cnt[c] : mine;
        if (mine) atomicAdd(reinterpret_cast<unsigned long long*>(&out[s].count[lane]), (unsigned long long)mine);
    }
}

}  // namespace

extern "C" int tmpnn_evalprep_max_per_frame(void) { return EP_MAX; }

extern "C" int tmpnn_evalprep(const tmpnn_evalprep_store* st, const int64_t* seq_host, const int32_t* tracks, int32_t* tracks_out,
                              tmpnn_evalprep_record* out, tmpnn_stream stream) {
    TM_REQUIRE(st != nullptr, "evalprep: store is null");
    if (const int rc = eval_check_store("evalprep", st->S, st->n_gt, st->n_det, st->n_off, nullptr, seq_host, seq_host && st->seq && out,
                                        "seq, seq_host or out", st->gt_off && st->det_off, st->gt_code && st->gt_box,
                                        st->det_code && st->det_box && st->det_perm && tracks && tracks_out, st->gt_box, st->det_box,
                                        0x7fffffff, EVAL_NO_LIMIT))
        return rc;
    if (st->S == 0) return TMPNN_OK;
    TM_REQUIRE(st->height_thr == st->height_thr, "evalprep: the height threshold is NaN");
    int64_t max_frames = 0;
    for (int s = 0; s < st->S; ++s) max_frames = seq_host[(size_t)s * 8 + 5] > max_frames ? seq_host[(size_t)s * 8 + 5] : max_frames;
    const int frame_groups = max_frames > 0 ? ceil_div(max_frames, EP_FRAMES) : 1;
    TM_REQUIRE((int64_t)st->S * frame_groups < 0x7fffffff, "evalprep: %d sequences x %d groups of %d frames pass the grid", st->S, frame_groups, EP_FRAMES);
    hipStream_t hs = as_stream(stream);
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)st->S * sizeof(tmpnn_evalprep_record), hs);
    if (e != hipSuccess) return set_error(TMPNN_ELAUNCH, "evalprep: clearing the records: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_evalprep, dim3(st->S * frame_groups), dim3(64 * EP_WAVES), 0, hs, *st, tracks, tracks_out, out, frame_groups);
    return check_launch("evalprep");
}
