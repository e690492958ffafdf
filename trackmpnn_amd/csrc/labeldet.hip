// GT track ids for detections, on the device (tmpnn_label_dets, tmpnn_label_compact; include/tmpnn.h; host definition:
// trackmpnn_amd.labeling.label_frame_host).  The reference does this per frame in Python every time a chunk is handed out
// (dataset/kitti_mot.py:422-486, dataset/bdd100k_mot.py:407-470): a greedy matching of the frame's detections to its GT boxes in
// descending IoU, then the removal of unassigned detections in ignore regions (by IoM) and on ignore objects (by IoU).
//
// k_label<NT>   one workgroup of NT threads per frame; thread t is detection t of the frame AND GT row t of the frame (both sides
//               hold at most NT rows).  NT = 64 (one wave) for the frames of at most 64 x 64, NT = 256 for the others: the host
//               routes the frames into two lists, one launch each.  The frame's boxes, categories and free marks are staged in LDS (60
//               bytes a row, 15 KB at NT = 256); the P x G overlap matrix is never stored, an overlap is recomputed where it is needed.
//               The sorted greedy matching equals rounds of MUTUAL BEST picks under the same strict order (IoU descending, then
//               the flat index p * G' + g ascending): every free detection picks its best free eligible GT row (first maximum over
//               ascending g), every free GT row its best free detection (first maximum over ascending p); a pair that picked each
//               other is accepted; the rounds end when none is.  The best pair of all free pairs is always mutual, so every
//               round but the last accepts one; a mutual pair is preceded in the order by no free pair that shares an end with
//               it, so the sorted walk accepts it too.  A pick is kept from round to round and searched again only when its
//               partner was taken.  Three barriers a round.
// k_label_scan  ONE workgroup: the exclusive prefix sums of the per-frame kept counts of both sides in tiles of 256 frames with a
//               running carry (block_scan.h), the totals and the flags of the frames into the record.
// k_label_pack  one wave per frame: the kept rows of both sides, packed in input order at the frame's offset (ballot ranks);
//               the per-sequence offsets.
// Four launches whatever the size, no host wait between them, nothing atomic, plain vector stores only.
//
// Overlaps are the float32 "+1" forms of utils/misc.py:4-42 in numpy's operation order: contraction is OFF for this file, every
// +, -, * is one correctly rounded float32 operation, minimum and maximum hand a NaN on as numpy's do, and the quotient is formed
// in float64 and rounded to float32 (for float32 operands that is the correctly rounded float32 quotient, 53 >= 2 * 24 + 2, and
// the compiler is free to emit the IEEE float32 division for it), so that every decision equals the host's.
//
// Every offset read from the store is checked against the store's totals before it is used; a frame whose offsets are out of
// range sets the frame's flag and nothing is read or written outside the arrays.
#pragma clang fp contract(off)
#include "block_scan.h"
#include "common.h"

using namespace tmpnn;

namespace {

constexpr int LB_MAX = 256;                  // rows of one side of a frame
constexpr int LB_WAVE = 64;                  // frames up to LB_WAVE x LB_WAVE take one wave
constexpr int LB_FLAG_LIMIT = 1, LB_FLAG_STORE = 2;
constexpr int LS_THREADS = 256;              // k_label_scan: frames per tile
constexpr int LP_THREADS = 256;              // k_label_pack: four frames per workgroup

__device__ __forceinline__ float np_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ float np_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ float np_div(float a, float b) { return (float)((double)a / (double)b); }

// intersection and the two areas of x1 y1 x2 y2 boxes a (a detection) and b (a GT row)
__device__ __forceinline__ void lb_parts(float4 a, float4 b, float& inter, float& area_a, float& area_b) {
    const float xA = np_max(a.x, b.x), yA = np_max(a.y, b.y), xB = np_min(a.z, b.z), yB = np_min(a.w, b.w);
    inter = np_max((xB - xA) + 1.0f, 0.0f) * np_max((yB - yA) + 1.0f, 0.0f);
    area_a = ((a.z - a.x) + 1.0f) * ((a.w - a.y) + 1.0f);
    area_b = ((b.z - b.x) + 1.0f) * ((b.w - b.y) + 1.0f);
}
__device__ __forceinline__ float lb_iou(float4 a, float4 b) {
    float inter, aa, ab;
    lb_parts(a, b, inter, aa, ab);
    return np_div(inter, (aa + ab) - inter);
}
__device__ __forceinline__ float lb_iom(float4 a, float4 b) {
    float inter, aa, ab;
    lb_parts(a, b, inter, aa, ab);
    return np_div(inter, np_min(aa, ab));
}

template <int NT>
struct LabelShared {
    float4 dbox[NT], gbox[NT];
    int dcat[NT], gcat[NT];
    int gcls[NT];                            // 0 matchable, 1 iom-ignore, 2 iou-ignore
    int dpick[NT], gpick[NT];                // this round's pick of a free row (-1: none / not free)
    int dfree[NT], gfree[NT];
    int wave[NT / 64 + 1];
};

template <int NT>
__global__ __launch_bounds__(NT) void k_label(tmpnn_label_store st, tmpnn_label_out out, const int32_t* __restrict__ list,
                                              int64_t n_list) {
    __shared__ LabelShared<NT> S;
    const int t = threadIdx.x;
    if ((int64_t)blockIdx.x >= n_list) return;
    const int64_t f = list[blockIdx.x];
    if (f < 0 || f >= st.n_frames) return;
    const int64_t d0 = st.det_first[f], d1 = st.det_first[f + 1], g0 = st.gt_first[f], g1 = st.gt_first[f + 1];
    if (d0 < 0 || d1 < d0 || d1 > st.n_det || g0 < 0 || g1 < g0 || g1 > st.n_gt) {
        if (t == 0) { out.det_cnt[f] = 0; out.gt_cnt[f] = 0; out.fflag[f] = LB_FLAG_STORE; }
        return;
    }
    const int64_t P64 = d1 - d0, G64 = g1 - g0;
    if (P64 > NT || G64 > NT) {                                   // over the limit (NT = 256), or routed to the wrong list
        for (int64_t i = t; i < P64; i += NT) { out.track[d0 + i] = -1; out.keep[d0 + i] = 0; }
        for (int64_t i = t; i < G64; i += NT) out.gt_keep[g0 + i] = 0;
        if (t == 0) { out.det_cnt[f] = 0; out.gt_cnt[f] = 0; out.fflag[f] = (P64 > LB_MAX || G64 > LB_MAX) ? LB_FLAG_LIMIT : LB_FLAG_STORE; }
        return;
    }
    const int P = (int)P64, G = (int)G64;
    const bool is_d = t < P, is_g = t < G;
    float4 mybox = make_float4(0.f, 0.f, 0.f, 0.f), mygbox = mybox;
    int mycat = 0, mygcat = 0, mycls = 1;
    if (is_d) {
        mybox = reinterpret_cast<const float4*>(st.det_box)[d0 + t];
        mycat = st.det_cat[d0 + t];
        S.dbox[t] = mybox; S.dcat[t] = mycat;
    }
    if (is_g) {
        mygbox = reinterpret_cast<const float4*>(st.gt_box)[g0 + t];
        mygcat = st.gt_cat[g0 + t];
        mycls = mygcat == st.iom_ignore_cat ? 1 : (mygcat == st.iou_ignore_cat ? 2 : 0);
        S.gbox[t] = mygbox; S.gcat[t] = mygcat; S.gcls[t] = mycls;
    }
    const bool matchable = is_g && mycls == 0;
    S.dfree[t] = is_d ? 1 : 0;
    S.gfree[t] = matchable ? 1 : 0;
    __syncthreads();

    // ---- the matching: rounds of mutual best picks
    const float iou_t = st.iou_thresh;
    bool dfree = is_d, gfree = matchable;
    int dbest = -2, gbest = -2;                                   // -2: to be searched, -1: no eligible free partner is left
    int track = -1;
    if (P > 0 && G > 0) {
        for (int round = 0; round <= NT; ++round) {               // (every round but the last accepts a pair: at most min(P, G) + 1)
            if (dfree && (dbest == -2 || (dbest >= 0 && !S.gfree[dbest]))) {
                float bv = 0.f;
                dbest = -1;
                for (int g = 0; g < G; ++g) {
                    if (!S.gfree[g] || S.gcat[g] != mycat) continue;
                    const float v = lb_iou(mybox, S.gbox[g]);
                    if (v >= iou_t && (dbest < 0 || v > bv)) { bv = v; dbest = g; }
                }
            }
            if (gfree && (gbest == -2 || (gbest >= 0 && !S.dfree[gbest]))) {
                float bv = 0.f;
                gbest = -1;
                for (int p = 0; p < P; ++p) {
                    if (!S.dfree[p] || S.dcat[p] != mygcat) continue;
                    const float v = lb_iou(S.dbox[p], mygbox);
                    if (v >= iou_t && (gbest < 0 || v > bv)) { bv = v; gbest = p; }
                }
            }
            S.dpick[t] = dfree ? dbest : -1;
            S.gpick[t] = gfree ? gbest : -1;
            __syncthreads();
            int accepted = 0;
            if (dfree && dbest >= 0 && S.gpick[dbest] == t) {
                track = st.gt_track[g0 + dbest];
                dfree = false;
                accepted = 1;
            }
            if (gfree && gbest >= 0 && S.dpick[gbest] == t) gfree = false;
            const int any = __syncthreads_or(accepted);           // (the picks were read before it, the free marks change after it)
            if (!any) break;
            if (is_d) S.dfree[t] = dfree ? 1 : 0;
            if (matchable) S.gfree[t] = gfree ? 1 : 0;
            __syncthreads();
        }
    }

    // ---- the removal: an unassigned detection in an ignore region (IoM) or on an ignore object (IoU)
    int keep = 0;
    if (is_d) {
        keep = 1;
        if (dfree) {
            bool any1 = false, nan1 = false, any2 = false, nan2 = false;
            float m1 = 0.f, m2 = 0.f;
            for (int g = 0; g < G; ++g) {
                const int c = S.gcls[g];
                if (c == 1) {
                    const float v = lb_iom(mybox, S.gbox[g]);
                    if (v != v) nan1 = true;
                    else if (!any1 || v > m1) m1 = v;
                    any1 = true;
                } else if (c == 2) {
                    const float v = lb_iou(mybox, S.gbox[g]);
                    if (v != v) nan2 = true;
                    else if (!any2 || v > m2) m2 = v;
                    any2 = true;
                }
            }
            // np.amax hands a NaN on, and a NaN passes no >=
            if ((any1 && !nan1 && m1 >= st.iom_thresh) || (any2 && !nan2 && m2 >= iou_t)) keep = 0;
        }
        out.track[d0 + t] = dfree ? -1 : track;
        out.keep[d0 + t] = (uint8_t)keep;
    }
    if (is_g) out.gt_keep[g0 + t] = matchable ? 1 : 0;
    int total;
    block_scan<NT>(keep, S.wave, &total);
    int gtotal;
    block_scan<NT>(matchable ? 1 : 0, S.wave, &gtotal);
    if (t == 0) { out.det_cnt[f] = total; out.gt_cnt[f] = gtotal; out.fflag[f] = 0; }
}

__global__ __launch_bounds__(LS_THREADS) void k_label_scan(tmpnn_label_store st, tmpnn_label_out out) {
    __shared__ int s_wave[LS_THREADS / 64 + 1];
    __shared__ int s_first;
    const int t = threadIdx.x;
    int64_t run_d = 0, run_g = 0;
    int flag = 0;
    int64_t bad_frame = -1;                                       // the first flagged frame
    for (int64_t f0 = 0; f0 < st.n_frames; f0 += LS_THREADS) {
        const int64_t f = f0 + t;
        int cd = 0, cg = 0, fl = 0;
        if (f < st.n_frames) {
            const int64_t d0 = st.det_first[f], d1 = st.det_first[f + 1], g0 = st.gt_first[f], g1 = st.gt_first[f + 1];
            cd = out.det_cnt[f]; cg = out.gt_cnt[f]; fl = out.fflag[f];
            // a count the frame cannot have (its offsets are wrong, or no list named the frame)
            if (d0 < 0 || d1 < d0 || d1 > st.n_det || g0 < 0 || g1 < g0 || g1 > st.n_gt || cd < 0 || cd > d1 - d0 || cg < 0 || cg > g1 - g0)
                fl |= LB_FLAG_STORE;
            if (fl) { cd = cg = 0; }                              // (nothing is packed for a flagged frame)
        }
        int tot_d, tot_g, n_bad, n_kind;
        const int ex_d = block_scan<LS_THREADS>(cd, s_wave, &tot_d);
        const int ex_g = block_scan<LS_THREADS>(cg, s_wave, &tot_g);
        if (f < st.n_frames) {
            out.det_off[f] = (int32_t)(run_d + ex_d);
            out.gt_off[f] = (int32_t)(run_g + ex_g);
            out.fflag[f] = (uint8_t)fl;
        }
        run_d += tot_d; run_g += tot_g;
        const int before = block_scan<LS_THREADS>(fl ? 1 : 0, s_wave, &n_bad);
        if (n_bad && bad_frame < 0) {                             // (uniform over the workgroup; taken once at the most)
            if (fl && before == 0) s_first = t;
            __syncthreads();
            bad_frame = f0 + s_first;
        }
        // how many frames of the tile carry which flag: the limit in the low half, the store in the high half (<= 256 each)
        block_scan<LS_THREADS>(((fl & LB_FLAG_LIMIT) ? 1 : 0) | ((fl & LB_FLAG_STORE) ? 1 << 16 : 0), s_wave, &n_kind);
        if (n_kind & 0xffff) flag |= LB_FLAG_LIMIT;
        if (n_kind >> 16) flag |= LB_FLAG_STORE;
    }
    if (t == 0) {
        out.det_off[st.n_frames] = (int32_t)run_d;
        out.gt_off[st.n_frames] = (int32_t)run_g;
        tmpnn_label_record r;
        r.flag = flag; r.frame = bad_frame; r.kept_det = run_d; r.kept_gt = run_g;
        *out.record = r;
    }
}

// the rows [a0, a1) with a non-zero mark, packed from position `o` on: one wave, `n_out` = the capacity of the packed arrays
template <typename Row>
__device__ __forceinline__ void lb_pack_side(int64_t a0, int64_t a1, const uint8_t* __restrict__ mark, int64_t o, int64_t n_out,
                                             int lane, Row row) {
    for (int64_t base = a0; base < a1; base += 64) {
        const int64_t i = base + lane;
        const int k = (i < a1 && mark[i] != 0) ? 1 : 0;
        const unsigned long long m = __ballot(k);
        const int64_t pos = o + __popcll(m & ((1ull << lane) - 1ull));
        if (k && pos >= 0 && pos < n_out) row(i, pos);
        o += __popcll(m);
    }
}

__global__ __launch_bounds__(LP_THREADS) void k_label_pack(tmpnn_label_store st, tmpnn_label_out out) {
    const int lane = threadIdx.x & 63;
    const int64_t gid = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (gid <= st.S) {                                            // the per-sequence offsets
        const int64_t b = st.seq_base[gid];
        const bool ok = b >= 0 && b <= st.n_frames;
        out.seq_det_off[gid] = ok ? out.det_off[b] : 0;
        out.seq_gt_off[gid] = ok ? out.gt_off[b] : 0;
    }
    const int64_t f = gid >> 6;                                   // (wave-uniform)
    if (f >= st.n_frames) return;
    if (out.fflag[f] != 0) return;
    const int64_t d0 = st.det_first[f], d1 = st.det_first[f + 1], g0 = st.gt_first[f], g1 = st.gt_first[f + 1];
    if (d0 < 0 || d1 < d0 || d1 > st.n_det || g0 < 0 || g1 < g0 || g1 > st.n_gt) return;
    const float4* det_box = reinterpret_cast<const float4*>(st.det_box);
    const float4* gt_box = reinterpret_cast<const float4*>(st.gt_box);
    float4* o_det_box = reinterpret_cast<float4*>(out.o_det_box);
    float4* o_gt_box = reinterpret_cast<float4*>(out.o_gt_box);
    lb_pack_side(d0, d1, out.keep, out.det_off[f], st.n_det, lane, [&](int64_t i, int64_t pos) {
        out.o_det_frame[pos] = st.det_frame[i];
        out.o_det_track[pos] = out.track[i];
        out.o_det_cat[pos] = st.det_cat[i];
        o_det_box[pos] = det_box[i];
        out.o_det_score[pos] = st.det_score[i];
    });
    lb_pack_side(g0, g1, out.gt_keep, out.gt_off[f], st.n_gt, lane, [&](int64_t i, int64_t pos) {
        out.o_gt_frame[pos] = st.gt_frame[i];
        out.o_gt_track[pos] = st.gt_track[i];
        out.o_gt_cat[pos] = st.gt_cat[i];
        o_gt_box[pos] = gt_box[i];
    });
}

int check_args(const tmpnn_label_store* st, const tmpnn_label_out* out, const char* who) {
    TM_REQUIRE(st != nullptr && out != nullptr, "%s: store or out is null", who);
    TM_REQUIRE(st->S >= 0 && st->n_frames >= 0 && st->n_det >= 0 && st->n_gt >= 0 && st->n_small >= 0 && st->n_big >= 0,
               "%s: S=%d n_frames=%lld n_det=%lld n_gt=%lld n_small=%lld n_big=%lld", who, st->S, (long long)st->n_frames,
               (long long)st->n_det, (long long)st->n_gt, (long long)st->n_small, (long long)st->n_big);
    TM_REQUIRE(st->n_frames < 0x7fffffff && st->n_det < 0x7fffffff && st->n_gt < 0x7fffffff, "%s: the store is indexed by int32", who);
    TM_REQUIRE(st->n_small + st->n_big == st->n_frames, "%s: the two frame lists hold %lld + %lld of %lld frames", who,
               (long long)st->n_small, (long long)st->n_big, (long long)st->n_frames);
    TM_REQUIRE(st->iou_thresh == st->iou_thresh && st->iom_thresh == st->iom_thresh, "%s: a threshold is NaN", who);
    TM_REQUIRE(st->seq_base && st->det_first && st->gt_first, "%s: null frame tables", who);
    TM_REQUIRE((st->n_small == 0 || st->small_frames) && (st->n_big == 0 || st->big_frames), "%s: null frame lists", who);
    TM_REQUIRE(st->n_det == 0 || (st->det_frame && st->det_cat && st->det_box && st->det_score), "%s: null detection arrays", who);
    TM_REQUIRE(st->n_gt == 0 || (st->gt_frame && st->gt_track && st->gt_cat && st->gt_box), "%s: null GT arrays", who);
    TM_REQUIRE(aligned16(st->det_box) && aligned16(st->gt_box), "%s: boxes must be 16-byte aligned", who);
    TM_REQUIRE(out->record && out->det_off && out->gt_off && out->seq_det_off && out->seq_gt_off, "%s: null record or offsets", who);
    TM_REQUIRE(st->n_frames == 0 || (out->det_cnt && out->gt_cnt && out->fflag), "%s: null per-frame outputs", who);
    TM_REQUIRE(st->n_det == 0 || (out->track && out->keep && out->o_det_frame && out->o_det_track && out->o_det_cat && out->o_det_box &&
                                  out->o_det_score), "%s: null detection outputs", who);
    TM_REQUIRE(st->n_gt == 0 || (out->gt_keep && out->o_gt_frame && out->o_gt_track && out->o_gt_cat && out->o_gt_box),
               "%s: null GT outputs", who);
    TM_REQUIRE(aligned16(out->o_det_box) && aligned16(out->o_gt_box) && (reinterpret_cast<uintptr_t>(out->record) & 7u) == 0,
               "%s: packed boxes must be 16-byte aligned, the record 8-byte aligned", who);
    return TMPNN_OK;
}

}  // namespace

extern "C" int tmpnn_label_max_per_frame(void) { return LB_MAX; }

extern "C" int tmpnn_label_wave_frame(void) { return LB_WAVE; }

extern "C" int tmpnn_label_dets(const tmpnn_label_store* st, const tmpnn_label_out* out, tmpnn_stream stream) {
    if (int rc = check_args(st, out, "label_dets")) return rc;
    if (st->n_small > 0) {
        hipLaunchKernelGGL(k_label<LB_WAVE>, dim3((unsigned)st->n_small), dim3(LB_WAVE), 0, as_stream(stream), *st, *out,
                           st->small_frames, st->n_small);
        if (int rc = check_launch("label_dets (wave frames)")) return rc;
    }
    if (st->n_big > 0) {
        hipLaunchKernelGGL(k_label<LB_MAX>, dim3((unsigned)st->n_big), dim3(LB_MAX), 0, as_stream(stream), *st, *out, st->big_frames,
                           st->n_big);
        if (int rc = check_launch("label_dets (workgroup frames)")) return rc;
    }
    return TMPNN_OK;
}

extern "C" int tmpnn_label_compact(const tmpnn_label_store* st, const tmpnn_label_out* out, tmpnn_stream stream) {
    if (int rc = check_args(st, out, "label_compact")) return rc;
    hipLaunchKernelGGL(k_label_scan, dim3(1), dim3(LS_THREADS), 0, as_stream(stream), *st, *out);
    if (int rc = check_launch("label_compact (scan)")) return rc;
    const int64_t threads = (st->n_frames * 64 > (int64_t)st->S + 1) ? st->n_frames * 64 : (int64_t)st->S + 1;
    hipLaunchKernelGGL(k_label_pack, dim3((unsigned)ceil_div(threads, LP_THREADS)), dim3(LP_THREADS), 0, as_stream(stream), *st, *out);
    return check_launch("label_compact (pack)");
}
