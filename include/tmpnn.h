/*
 * tmpnn.h -- C ABI of libtmpnn.so: the MI355X (gfx950) implementation of the TrackMPNN
 * message-passing hot path.
 *
 * Every entry point replaces one stage of the reference's per-timestep forward/backward
 * (reference = arangesh/TrackMPNN; file:line cited at each declaration).  The reference has no
 * FFI of its own (it is pure Python on torch ops); the stages below are exactly the ATen calls
 * `TrackMPNN.forward` (models/track_mpnn.py:54-75) and `FactorGraphGRU.forward`
 * (models/layers.py:84-116) dispatch, regrouped by what they compute.
 *
 * Conventions
 *   - all feature tensors are fp32, row-major, with an explicit leading dimension (`ld*`, in
 *     floats) so one [N, G*H] state tensor can be addressed per feature group without repacking;
 *   - all index arrays are int32 and live in device memory;
 *   - the caller owns every buffer (including workspaces); the library never allocates, frees,
 *     or keeps a device pointer past the call;
 *   - work is only ENQUEUED on `stream`; nothing synchronises the device;
 *   - return value: TMPNN_OK (0) or a negative TMPNN_E* code; `tmpnn_last_error()` gives the
 *     thread-local message of the last failure.  Nothing is ever thrown across the boundary.
 *   - supported hidden widths: H in {32, 64, 128, 256}; additionally the multiples of 128 up to 1024 in the entry points of
 *     the paths without attention: tmpnn_gru_{fwd,bwd_data,bwd_weights} (H-generic f32 kernels), tmpnn_wide_*,
 *     tmpnn_input_bn_*, tmpnn_heads_* (<= 1024 columns per call), tmpnn_gather_diff_* / tmpnn_gather_concat_bwd / tmpnn_segsum_*
 *     (served internally in 256-column slices).  tmpnn_att_*, tmpnn_gather_concat_fwd and the fused / tiled H <= 64 forms keep
 *     the four widths.
 *   - no entry point measures, tunes or keeps data between calls; the only process state is the thread-local
 *     error string and idempotent per-kernel function attributes.
 */
#ifndef TMPNN_H
#define TMPNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMPNN_ABI_VERSION 13 /* 2: struct tmpnn_graph gained seg_plan (round 4); 3: win_plan (round 5); 4 (round 6, frozen): the
                               exported set is what a default run can reach (80 entry points: 15 superseded or internal ones
                               left it), tmpnn_input_tf_* take x_rows, + tmpnn_segsum_fwd_live, tmpnn_bce_logits_*;
                               5: + struct tmpnn_loss_windows, tmpnn_train_losses_win_* (entry points added, none changed);
                               6: + struct tmpnn_train_build, tmpnn_train_build_* (entry points added, none changed);
                               7: + tmpnn_cls_counts, tmpnn_cls_counts_win, struct tmpnn_train_record, tmpnn_train_record_fold
                                  (entry points added, none changed);
                               8: + struct tmpnn_optim_seg, struct tmpnn_adam_state, tmpnn_optim_chunk, tmpnn_adam_step,
                                  tmpnn_grad_flow (entry points added, none changed);
                               9: + struct tmpnn_chunk_draw, tmpnn_chunk_draw_count, tmpnn_chunk_draw_fill (entry points added,
                                  none changed);
                               10: + struct tmpnn_zs_gate_src: tmpnn_gru_bwd_fused_zero_state takes it in place of the gate
                                   planes when gate_plane == 0 (same arguments; calls that pass planes are unchanged);
                               11: + tmpnn_online_features (entry point added, none changed);
                               12: + struct tmpnn_mot_store, struct tmpnn_mot_record, tmpnn_mot_events, tmpnn_mot_events_ws,
                                   tmpnn_mot_dist, tmpnn_mot_max_per_frame (entry points added, none changed);
                               13: + struct tmpnn_map_store, struct tmpnn_map_record, tmpnn_map_best, tmpnn_map_eval,
                                   tmpnn_map_eval_ws, tmpnn_map_tile (entry points added, none changed);
                               still 13: + struct tmpnn_mot_summary_record, tmpnn_mot_summary, tmpnn_mot_summary_ws,
                                   tmpnn_mot_summary_limit (entry points added, none changed; the number stays because
                                   tests/test_map_eval.py holds the library to exactly 13: a caller that needs them looks
                                   the symbols up);
                               still 13, for the same reason: + struct tmpnn_val_record, tmpnn_val_f1_count (entry point
                                   added, none changed);
                               still 13, for the same reason: + struct tmpnn_label_store, struct tmpnn_label_record, struct
                                   tmpnn_label_out, tmpnn_label_dets, tmpnn_label_compact, tmpnn_label_max_per_frame,
                                   tmpnn_label_wave_frame (entry points added, none changed);
                               still 13, for the same reason: + struct tmpnn_chunk_vis, tmpnn_chunk_draw_vis, struct
                                   tmpnn_frames_gather_args, tmpnn_frames_gather (entry points added, none changed; the
                                   reserved word of struct tmpnn_chunk_draw, zero so far, is now ldx: 0 means F as before);
                               still 13, for the same reason: + struct tmpnn_frames_resize_args, tmpnn_frames_resize,
                                   tmpnn_frames_resize_ws (entry points added, none changed);
                               still 13, for the same reason: + struct tmpnn_hota_record, tmpnn_hota, tmpnn_hota_ws (entry
                                   points added, none changed);
                               still 13, for the same reason: + struct tmpnn_result_store, struct tmpnn_result_record,
                                   tmpnn_results_apply, tmpnn_results_ws (entry points added, none changed);
                               still 13, for the same reason: + struct tmpnn_evalprep_store, struct tmpnn_evalprep_record,
                                   tmpnn_evalprep, tmpnn_evalprep_max_per_frame (entry points added, none changed);
                               still 13, for the same reason: + struct tmpnn_att_record, tmpnn_att_hist_count (entry point
                                   added, none changed);
                               still 13, for the same reason: + struct tmpnn_seq_features_args, tmpnn_seq_features (entry
                                   point added, none changed);
                               still 13, for the same reason: + struct tmpnn_embed_loss, tmpnn_embed_loss_ws,
                                   tmpnn_embed_loss_fwd, tmpnn_embed_loss_bwd, tmpnn_vis_head_scatter, struct
                                   tmpnn_embed_record, tmpnn_train_embed_fold (entry points added, none changed);
                               still 13, for the same reason: + tmpnn_espnet_arena_floats, tmpnn_espnet_ws_bytes,
                                   tmpnn_espnet_fwd (entry points added, none changed);
                               still 13, for the same reason: + tmpnn_espnet_centres_ws_bytes, tmpnn_espnet_trunk,
                                   tmpnn_espnet_centres, tmpnn_vis_head_pixels, tmpnn_vis_head_rows_from_logits (entry points
                                   added, none changed);
                               still 13, for the same reason: + tmpnn_espnet_train_param_floats, tmpnn_espnet_train_table,
                                   tmpnn_espnet_train_ws_bytes, tmpnn_espnet_train_bwd_ws_bytes, tmpnn_espnet_refold,
                                   tmpnn_espnet_train_fwd, tmpnn_espnet_train_bwd (entry points added, none changed);
                               still 13, for the same reason: + tmpnn_reduce_slabs (entry point added, none changed);
                               still 13, for the same reason: + tmpnn_espnet_dec_param_floats, tmpnn_espnet_dec_table,
                                   tmpnn_espnet_dec_ws_bytes, tmpnn_espnet_dec_bwd_ws_bytes, tmpnn_espnet_dec_refold,
                                   tmpnn_espnet_dec_fwd, tmpnn_espnet_dec_bwd (entry points added, none changed) */

#define TMPNN_OK 0
#define TMPNN_EINVAL (-1)   /* bad shape / null pointer / unsupported width */
#define TMPNN_ELAUNCH (-2)  /* hipGetLastError() after a launch */
#define TMPNN_EWORKSPACE (-3) /* workspace too small */

typedef void* tmpnn_stream; /* hipStream_t */
typedef void* tmpnn_event;  /* hipEvent_t, created and owned by the caller (the library only records / waits on it) */

/*
 * Index form of the reference's adjacency pair (utils/graph.py:151-163, 294-308): every edge
 * row e of node_adj holds +1 at its earlier det (`src`) and -1 at its later det (`dst`);
 * edge_adj is its transpose, i.e. the det -> incident-edge lists, stored here as a CSR whose
 * entries are edge ROW indices with the sign of edge_adj[d, e] in bit 31 (set = -1 = d is the
 * later det of e).  Built once per call by the host from the adjacency the reference passes.
 */
/* Optional plan of a DENSE graph for the edge -> det segment sum (csrc/agg.hip, k_segsum_tiles): the edge set cut into
 * 8 src x 16 dst tiles over det indices, each summed by the workgroup that streams its rows, so that an edge row is read
 * from HBM once instead of once per endpoint.  Built by the host once per graph (trackmpnn_amd.graph.dense_seg_plan); the
 * caller owns every array including the partial-row buffer `ws` (one segment sum at a time per plan). */
typedef struct tmpnn_seg_plan {
    int32_t T;               /* tiles */
    int32_t I;               /* work items: runs of consecutive tiles that share their 16 dsts */
    int32_t nsplit;          /* = N of the graph: entries of inc2 at or above it address partial rows */
    const int32_t* t_row;    /* [T][8][16] edge row of (src i, dst j) of a tile, -1 where the graph has no such edge */
    const int32_t* items;    /* [I][2] first tile, tile count */
    const int32_t* rowptr2;  /* [Dn+1] CSR of the second pass */
    const int32_t* inc2;     /* per det: nsplit + partial row (tile t, src i: 8t + i; item k, dst j: 8T + 16k + j), or a
                                plain edge row (< nsplit); sign bit as in tmpnn_graph.inc */
    float* ws;               /* [8 T + 16 I][256] partial rows */
    size_t ws_floats;
} tmpnn_seg_plan;

/* Optional plan of a BATCH OF SMALL WINDOWS (block-diagonal: no edge crosses windows) for the edge -> det segment sum at H = 64
 * (csrc/agg.hip, k_segsum_win): a workgroup owns a window at a time and walks its edge rows through the LDS in chunks of 160, once
 * -- each edge row is read from memory ONCE instead of once per endpoint; results equal the CSR kernel's bit for bit.  Incidence i
 * of a det's CSR run belongs to the stream (det, i % 4); stream s of a window's (window-local) dets is added to by lane group
 * s % 128 of the workgroup.  Built by the host once per graph (trackmpnn_amd.graph.build_win_plan) from the window label of every
 * det; the caller owns the arrays. */
typedef struct tmpnn_win_plan {
    int32_t W;                /* windows */
    int32_t nbig;             /* dets of the windows beyond the kernel's capacity (160 dets, 24 chunks, 15 steps a chunk): CSR kernel */
    const int32_t* wrec;      /* [W][8] per window: first entry / count in erow, first visiting position (entry of det / drow) /
                                       count of its dets (capacity + 1: left to the CSR kernel), first step in recs, and the steps of
                                       its chunks, 4 bits each, in three words; 32-byte aligned */
    const int32_t* erow;      /* edge rows, window by window, ascending within a window; a window's list starts at a multiple of 4 */
    const uint16_t* recs;     /* [steps][128] per chunk and step, for each lane group: place of the edge row in the chunk | 0x100
                                       where the det is the edge's later endpoint (the sign bit of tmpnn_graph.inc) | (stream / 128)
                                       << 9 | 0x8000 for "nothing to do"; a lane group's records of one stream are in run order;
                                       256-byte aligned */
    const int32_t* det;       /* [Dn]  det index per visiting position (window-major) */
    const int32_t* drow;      /* [Dn]  its graph row */
    const int32_t* big_order; /* [nbig] det indices of the windows left to the CSR kernel */
} tmpnn_win_plan;

typedef struct tmpnn_graph {
    int32_t N;               /* rows of the state tensor (dets + edges) */
    int32_t E;               /* edge rows */
    int32_t Dn;              /* det rows */
    const int32_t* src;      /* [E]  row of the +1 det of edge e */
    const int32_t* dst;      /* [E]  row of the -1 det of edge e */
    const int32_t* edge_row; /* [E]  row of edge e (ascending) */
    const int32_t* det_row;  /* [Dn] row of det d (ascending) */
    const int32_t* rowptr;   /* [Dn+1] CSR offsets into inc */
    const int32_t* inc;      /* [2E] (edge row) | (sign bit: 0x80000000 when d == dst) */
    const int32_t* det_order; /* [Dn] or NULL: order in which the det -> edge reductions visit the dets (a permutation of
                                0..Dn-1).  Results do not depend on it; a host that batches independent windows lists
                                each window's dets together, so that the two reads of an edge row (one from either
                                endpoint) are issued from the same CU close in time */
    const tmpnn_seg_plan* seg_plan; /* or NULL: dense graphs, H = 256 column blocks -- tmpnn_segsum_fwd and the wide cells'
                                       backward then read every edge row once (see tmpnn_seg_plan) */
    const tmpnn_win_plan* win_plan; /* or NULL: batches of small windows, H = 64 -- the segment sums (tmpnn_segsum_fwd,
                                       tmpnn_gather_diff_bwd) then read every edge row once (see tmpnn_win_plan) */
} tmpnn_graph;

/*
 * Edge tiles: the edge rows of a graph cut into tiles of `rows_per_tile` rows chosen so that a tile touches FEW distinct
 * dets.  The rolling graph's frame blocks are dense [A srcs x D_t dsts] row sets in src-major order
 * (utils/graph.py:141-156, 285-301), so a tile of (8 srcs x 16 dsts) needs 24 rows of a per-det table where 128
 * consecutive rows of a wide block need up to 129, and every gather of h[src] / h[dst] (models/layers.py:90-95) or of
 * their projections becomes a read from an LDS copy of the tile's det list.  Built once per graph
 * (trackmpnn_amd.graph.build_edge_tiles); any tiling that covers every edge row exactly once is valid -- ragged
 * (post-decode) graphs simply get longer det lists.
 */
typedef struct tmpnn_edge_tiles {
    int32_t T;              /* tiles */
    int32_t rows_per_tile;  /* 128 (wide cells) or 32 (H <= 64 cells) */
    const int32_t* t_row;   /* [T * rows_per_tile] graph row of each slot; -1 = padding.  PRECONDITION (device data, not validated by
                               the entry points; trackmpnn_amd.graph.build_edge_tiles guarantees it and tests/test_graph.py checks
                               it): padding occurs in the LAST tile only, BEHIND its valid slots, so slot 0 of every tile is a real
                               row -- the wide forward (k_wide_gru_fwd_pp) has no row guard: a padding slot recomputes and rewrites
                               what its tile's slot 0 writes, byte for byte */
    const int32_t* t_loc;   /* [T * rows_per_tile] (position of the slot's src det in the tile's det list) |
                               (position of its dst det) << 16 */
    const int32_t* t_dptr;  /* [T + 1] offsets into t_dets */
    const int32_t* t_dets;  /* [t_dptr[T]] det INDEX (0..Dn-1, = row of a per-det table), ascending within a tile */
} tmpnn_edge_tiles;

int tmpnn_abi_version(void);
const char* tmpnn_last_error(void);

/* ---- row E: node -> edge message (models/layers.py:90-95) -------------------------------
 * diff  : out[edge_row[e], 0:H]  (=|+=)  in[src[e], 0:H] - in[dst[e], 0:H]
 * concat: out[edge_row[e], 0:2H] (=|+=) [in[src[e], 0:H] | in[dst[e], 0:H]]
 * `accumulate` != 0 adds into out.  The backward of either is tmpnn_segsum_fwd on the gradient
 * (diff: signs +1/-1, concat: column offsets 0/H), exposed as tmpnn_gather_*_bwd. */
int tmpnn_gather_diff_fwd(const tmpnn_graph* g, const float* in, int ld_in, float* out, int ld_out,
                          int H, int accumulate, tmpnn_stream stream);
int tmpnn_gather_concat_fwd(const tmpnn_graph* g, const float* in, int ld_in, float* out, int ld_out,
                            int H, int accumulate, tmpnn_stream stream);
/* d_in[det_row[d], 0:H] (=|+=) sum_{e: src=d} d_out[row e, 0:H] - sum_{e: dst=d} d_out[row e, 0:H] */
int tmpnn_gather_diff_bwd(const tmpnn_graph* g, const float* d_out, int ld_dout, float* d_in, int ld_din,
                          int H, int accumulate, tmpnn_stream stream);
/* d_in[det_row[d], 0:H] (=|+=) sum_{e: src=d} d_out[row e, 0:H] + sum_{e: dst=d} d_out[row e, H:2H] */
int tmpnn_gather_concat_bwd(const tmpnn_graph* g, const float* d_out, int ld_dout, float* d_in, int ld_din,
                            int H, int accumulate, tmpnn_stream stream);

/* ---- row F: edge -> node signed aggregation, no attention (models/layers.py:103) --------
 * out[det_row[d], 0:H] (=|+=) sum_{e: src=d} in[row e] - sum_{e: dst=d} in[row e]
 * backward: d_in[edge_row[e]] (=|+=) d_out[src[e]] - d_out[dst[e]]  (= tmpnn_gather_diff_fwd). */
int tmpnn_segsum_fwd(const tmpnn_graph* g, const float* in, int ld_in, float* out, int ld_out,
                     int H, int accumulate, int compact_out /* out row = d instead of det_row[d] */,
                     tmpnn_stream stream);
/* The same sum where the caller KNOWS that rows >= row_limit of `in` are all-zero -- a forward call's new edge rows, which
 * enter the state as 0 (models/track_mpnn.py:61, utils/graph.py:148,291): those rows are not read (their +-0 changes no bit
 * of a sum).  row_limit >= N reads every row.  Ignored by the dense / window plans (they take the plain form). */
int tmpnn_segsum_fwd_live(const tmpnn_graph* g, const float* in, int ld_in, float* out, int ld_out,
                          int H, int compact_out, int row_limit, tmpnn_stream stream);
/* The backward of row F: tmpnn_gather_diff_fwd applied to gradients (the same kernel, the same bits):
 * d_in[edge_row[e], 0:H] (=|+=) d_out[src[e], 0:H] - d_out[dst[e], 0:H]. */
int tmpnn_segsum_bwd(const tmpnn_graph* g, const float* d_out, int ld_dout, float* d_in, int ld_din,
                     int H, int accumulate, tmpnn_stream stream);

/* ---- row G: attention-weighted aggregation (models/layers.py:26-43, 105-112) -------------
 * K heads (1..8 per call, all served by the same passes; a model with more runs groups of heads and combines their means: the output of a call is the MEAN over ITS heads).  W_cat [H][K*H]: head k's W_att ([H][H], in x out, as the reference
 * stores it) in columns k*H .. (k+1)*H; a [K][H].
 *   ha    = h[det rows] @ W_cat                       (ha [Dn][K*H]: the heads of a det side by side)
 *   s_e   = LeakyReLU_0.2(|ha_k[src]-ha_k[dst]| . a_k)  (score [2E][K] per CSR POSITION: an edge's score is stored at both
 *                                                      of its positions, so a det reads its run's scores contiguously)
 *   alpha = softmax over each det's incident edges    (alpha [K][2E], CSR order, AFTER dropout)
 *   out[d, 0:H] = 1/K sum_k sum_p sign_p * alpha_kp * h[inc row p]     (COMPACT rows: d, not det_row[d])
 * Also saved for the backward: stats [Dn][K][2] = the softmax's (max, sum exp) per det and head, and esk [K][Dn][H] = the
 * per-head aggregate 1/K sum_p sign_p alpha_kp h[row p] (out = sum_k esk[k]).
 * keep: NULL (eval / no dropout) or uint8 [2E] in CSR order, bit k set = head k keeps the position (kept entries scaled
 *   1/(1-p_drop)): one byte per position serves every head.
 * erec [E][8]: everything an edge-owned pass needs to know about edge e, as one 32-byte record: the DET INDICES of its
 *   src / dst endpoint, its CSR positions in the src det's and in the dst det's run (the inverse of inc) | the graph rows
 *   of src, dst and of the edge itself, 0.
 * Buffer sizes: score max(2E, 1) * K floats, alpha K * 2E, stats Dn * K * 2, esk K * Dn * H, ha Dn * K * H.  A graph without
 *   edges (E == 0, Dn > 0) may pass inc == NULL, keep == NULL and erec == NULL: no edge array is read then (score's first K
 *   floats are, as a stand-in, which is why score holds at least K floats), out and esk become 0 and stats (0, 1).
 * One read of h[inc row p] per CSR position serves every head; launches: 1 GEMM + 2 kernels. */
int tmpnn_att_fwd(const tmpnn_graph* g, const int32_t* erec, const float* h, int ld_h, int H, int K,
                  const float* W_cat, const float* a, const uint8_t* keep, float p_drop,
                  float* ha, float* score, float* stats, float* esk, float* alpha, float* out, int ld_out,
                  tmpnn_stream stream);
/* Backward of tmpnn_att_fwd.  d_out [N rows, ld_dout] is read at det rows (row-indexed).
 * Accumulates: d_h (+=, edge rows through the values, det rows through ha), dW_att [K][H][H] (+=, one [H][H] block per
 * head in the reference's layout), da [K][H] (+=).  ws: tmpnn_att_bwd_ws(E, Dn, H, K) floats, 16-byte aligned.
 * inc_other [2E]: det index of the OTHER endpoint of every CSR position (the src det's positions hold dst_pos[e] and vice
 * versa), bit 31 set on dst-side positions.  One edge-owned pass (reads h[row e] once, updates d_h[row e]) + one det-owned
 * pass over the projected det table + two Dn-row GEMMs. */
size_t tmpnn_att_bwd_ws(int E, int Dn, int H, int K);
/* erec [E][8] and inc_other [2E] of the two calls above from the graph's own arrays, in one launch.  pos [N]: row -> index
 * within its type (edge index for edge rows); src_pos / dst_pos [E]: det indices of an edge's endpoints. */
int tmpnn_att_index(const tmpnn_graph* g, const int32_t* pos, const int32_t* src_pos, const int32_t* dst_pos,
                    int32_t* erec, int32_t* inc_other, tmpnn_stream stream);
int tmpnn_att_bwd(const tmpnn_graph* g, const int32_t* erec, const int32_t* inc_other,
                  const float* h, int ld_h, int H, int K,
                  const float* W_cat, const float* a, const uint8_t* keep, float p_drop,
                  const float* ha, const float* score, const float* stats, const float* esk,
                  const float* d_out, int ld_dout, float* ws, size_t ws_floats,
                  float* d_h, int ld_dh, float* dW_att, float* da, tmpnn_stream stream);
/* The same with one output pointer per head (host arrays of K device pointers: dW_heads[k] [H][H] (+=), da_heads[k] [H]
 * (+=)) -- the heads' parameters are separate tensors (models/layers.py:7-24, 67: a ModuleList of GraphAttentionLayer, one per head), so their
 * .grad buffers can be accumulated in place without a stacked temporary. */
int tmpnn_att_bwd_heads(const tmpnn_graph* g, const int32_t* erec, const int32_t* inc_other,
                        const float* h, int ld_h, int H, int K,
                        const float* W_cat, const float* a, const uint8_t* keep, float p_drop,
                        const float* ha, const float* score, const float* stats, const float* esk,
                        const float* d_out, int ld_dout, float* ws, size_t ws_floats,
                        float* d_h, int ld_dh, float* const* dW_heads, float* const* da_heads, tmpnn_stream stream);

/* ---- rows H', I: GRU cells with row indirection + type-masked merge ----------------------
 * (torch.nn.GRUCell as used at models/layers.py:97,114; merge layers.py:116).
 * For every r < R with row = rows[r]:
 *     x      = xmode 0: msg[msg_compact ? r : row, 0:IN]
 *              xmode 1: h[src[r]] - h[dst[r]]          (fused row E, diff;   IN = H)
 *              xmode 2: [h[src[r]] | h[dst[r]]]        (fused row E, concat; IN = 2H)
 *              xmode 3: as xmode 1, but the x-part of the gates is read PRE-PROJECTED: msg = P [Dn][ld_msg >= 3H]
 *                       with P = h[det rows] @ W_ih^T (tmpnn_rows_linear), src/dst = DET INDICES of the two
 *                       endpoints; gi[r] = P[src[r]] - P[dst[r]] (linearity of row E).  H <= 64 only; wih_t unused.
 *     h_out[row] = GRUCell(x, h[row])
 * so running it once with rows = edge_row and once with rows = det_row performs the merge in
 * place.  Weights are passed TRANSPOSED (wih_t [IN][3H], whh_t [H][3H], see tmpnn_transpose);
 * gate order r,z,n.  gates: NULL or 4 planes [4][gate_plane] of row-indexed [N][H] floats
 * (r, z, n, W_hn h + b_hn) saved for the backward.
 * Fused output head (row J): if logit_part != NULL, plane p of logit_part (p < tmpnn_gru_fwd_head_parts(),
 * plane stride part_stride >= N floats) receives at `row` the partial dot product of h_out[row] with
 * w_head[0:H] over the p-th 32-column slice; tmpnn_heads_finish sums the planes of all groups, adds the bias
 * and applies the sigmoid.  tmpnn_gru_fwd_head_parts() == 0 means the fused head is unavailable for that
 * shape (use tmpnn_heads_fwd). */
int tmpnn_gru_fwd_head_parts(int H, int IN, int xmode);
int tmpnn_gru_fwd(const int32_t* rows, int R, int xmode, const int32_t* src, const int32_t* dst,
                  const float* msg, int ld_msg, int msg_compact, int IN, const float* h, int ld_h, int H,
                  const float* wih_t, const float* whh_t, const float* b_ih, const float* b_hh,
                  float* h_out, int ld_out, float* gates, size_t gate_plane,
                  const float* w_head, float* logit_part, size_t part_stride, tmpnn_stream stream);
/* Upstream gradient of both backward entry points: dh[row] = d_hout[row] (NULL = 0) + dy[row] * w_head
 * (dy NULL = no head term).  dy [N] is the gradient of the logits (tmpnn_heads_bwd's dy_out) and
 * w_head [H] the slice of the output head (w_node for det rows, w_edge for edge rows) of this group.
 *
 * Data gradient: d_msg[row, 0:IN] = d_gi @ W_ih ; d_h[row] = dh[row]*z + d_gh @ W_hh (both written,
 * not accumulated).  W_ih [3H][IN], W_hh [3H][H] in the reference layout.  If add_msg != NULL the
 * adjoint of row F is fused into the store: d_h[row] += add_msg[add_src[r]] - add_msg[add_dst[r]]
 * (rows = edge_row, add_src/dst = src/dst, add_msg = the d_msg buffer whose DET rows the node cell's
 * call has already written). */
int tmpnn_gru_bwd_data(const int32_t* rows, int R, int IN, const float* h, int ld_h, int H,
                       const float* w_ih, const float* w_hh,
                       const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout,
                       const float* dy, const float* w_head,
                       float* d_msg, int ld_dmsg, float* d_h, int ld_dh,
                       const int32_t* add_src, const int32_t* add_dst, const float* add_msg, int ld_add,
                       tmpnn_stream stream);
/* Weight gradient: dW_ih [3H][IN], dW_hh [3H][H], db_ih [3H], db_hh [3H] are ACCUMULATED (+=).
 * x is re-formed as in tmpnn_gru_fwd (xmode).  ws: tmpnn_gru_bwd_weights_ws(R, IN, H) bytes. */
/* Which H = 64 weight-gradient kernel tmpnn_gru_bwd_weights uses: 1 = bf16x6 split products (default), 0 = f32-input
 * MFMA.  A constant of the process (TMPNN_SPLIT_WEIGHTS=0/1 or TMPNN_SPLIT=0 in the environment when the library is
 * loaded): nothing is measured or decided inside a call, so every run and every rank takes the same kernel and
 * gradients are bitwise reproducible across processes.  tmpnn_gru_bwd_weights_variant takes the form explicitly
 * (variant 0 / 1; -1 = the process default) -- used by bench.py to time both forms. */
size_t tmpnn_gru_bwd_weights_ws(int R, int IN, int H);
int tmpnn_gru_bwd_weights(const int32_t* rows, int R, int xmode, const int32_t* src, const int32_t* dst,
                          const float* msg, int ld_msg, int msg_compact, int IN,
                          const float* h, int ld_h, int H,
                          const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout,
                          const float* dy, const float* w_head,
                          float* dW_ih, float* dW_hh, float* db_ih, float* db_hh,
                          void* ws, size_t ws_bytes, tmpnn_stream stream);

/* Fused backward of one cell: tmpnn_gru_bwd_data + tmpnn_gru_bwd_weights in ONE pass over the gates
 * (arguments as in those two; available when tmpnn_gru_bwd_fused_available(H, IN, xmode) != 0, i.e. H = 64,
 * IN = H, xmode 0 or 1).  With xmode 1 the fused row-F adjoint gathers through the cell's own endpoints:
 * add_src / add_dst must be the src / dst arrays.  ws: tmpnn_gru_bwd_fused_ws(R, IN, H) bytes. */
int tmpnn_gru_bwd_fused_available(int H, int IN, int xmode);
size_t tmpnn_gru_bwd_fused_ws(int R, int IN, int H);
int tmpnn_gru_bwd_fused(const int32_t* rows, int R, int xmode, const int32_t* src, const int32_t* dst,
                        const float* msg, int ld_msg, int msg_compact, int IN,
                        const float* h, int ld_h, int H, const float* w_ih, const float* w_hh,
                        const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout,
                        const float* dy, const float* w_head,
                        float* d_msg, int ld_dmsg, float* d_h, int ld_dh,
                        const int32_t* add_src, const int32_t* add_dst, const float* add_msg, int ld_add,
                        float* dW_ih, float* dW_hh, float* db_ih, float* db_hh,
                        void* ws, size_t ws_bytes, tmpnn_stream stream);
/* The same backward for rows whose incoming state h[row] is ZERO -- a forward call's new edge rows (xmode 1: x = h[src] -
 * h[dst]; available when tmpnn_gru_bwd_fused_zero_state_available(H, IN, xmode) != 0, i.e. H = IN = 64, xmode 1).  It does
 * not read h[row] nor the fourth gate plane (ghn = b_hn exactly: b_hn = b_hh + 2H), writes d_msg and accumulates dW_ih,
 * db_ih and db_hh (dW_hh gets nothing); d_h[row] is NOT formed, so the row-F adjoint is not taken either: for a call's new
 * rows it lies behind d_h_in.  ws: tmpnn_gru_bwd_fused_ws(R, IN, H) bytes.
 *
 * gate_plane != 0: `gates` is the device pointer to the saved planes [r | z | n], gate_plane floats apart, as for
 * tmpnn_gru_bwd_fused.  gate_plane == 0: the planes were NOT saved (tmpnn_gru_fwd_tiles_zero_state with gates = NULL) and
 * `gates` is a HOST pointer to a struct tmpnn_zs_gate_src, read at launch: the kernel forms r, z, n of a row again from the
 * projected det rows the forward read, with the forward's expressions (bit-identical planes, no matrix product):
 *   r = sigmoid((0 + (P_r[s] - P_r[d])) + (b_ir + b_hr)), z likewise, n = tanh(fma(r, 0 + b_hn, (P_n[s] - P_n[d]) + b_in))
 * with s = src_pos[i], d = dst_pos[i] for list position i (the lists run parallel to rows / src / dst).  A NULL struct, a
 * NULL or misaligned field (proj, b_ih, b_hh 16-byte aligned, ld_proj >= 3H and a multiple of 4) or b_hn != b_hh + 2H
 * fails with TMPNN_EINVAL before anything is launched.  Available whenever the entry point itself is. */
typedef struct tmpnn_zs_gate_src {
    const float* proj;        /* [Dn][ld_proj]: the output of tmpnn_rows_linear the forward call read (columns r | z | n) */
    int32_t ld_proj;
    const int32_t* src_pos;   /* [R] det positions (rows of proj) of the rows' endpoints */
    const int32_t* dst_pos;
    const float* b_ih;        /* [3H] the cell's biases */
    const float* b_hh;
} tmpnn_zs_gate_src;
int tmpnn_gru_bwd_fused_zero_state_available(int H, int IN, int xmode);
int tmpnn_gru_bwd_fused_zero_state(const int32_t* rows, int R, const int32_t* src, const int32_t* dst, int IN,
                                   const float* h, int ld_h, int H, const float* w_ih, const float* b_hn,
                                   const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout,
                                   const float* dy, const float* w_head, float* d_msg, int ld_dmsg,
                                   float* dW_ih, float* db_ih, float* db_hh,
                                   void* ws, size_t ws_bytes, tmpnn_stream stream);

/* tmpnn_gru_fwd's xmode 3 (edge cell over the projected det rows `proj` [Dn][ld_proj >= 3H] of tmpnn_rows_linear) over
 * EDGE TILES (rows_per_tile = 32, covering the graph's R edge rows): the distinct projected rows of a tile are staged in
 * LDS an item ahead instead of gathered per edge row after the matrix phase.  H in {32, 64}; bit-identical to
 * tmpnn_gru_fwd(rows = edge_row, xmode = 3, src / dst = det indices).  layers.py:90-97, rows E + H' + I + J. */
int tmpnn_gru_fwd_tiles(const tmpnn_edge_tiles* tiles, int R, const float* proj, int ld_proj, const float* h, int ld_h, int H,
                        const float* whh_t, const float* b_ih, const float* b_hh, float* h_out, int ld_out, float* gates,
                        size_t gate_plane, const float* w_head, float* logit_part, size_t part_stride, tmpnn_stream stream);
/* The same cell for tile lists whose rows all have a ZERO incoming state -- a call's new edge rows (available when
 * tmpnn_gru_fwd_tiles_zero_state_available(H, xmode) != 0: H in {32, 64}, xmode 3, rows_per_tile = 32).  h is not read and
 * there is no W_hh product; outputs bit-identical to tmpnn_gru_fwd_tiles on such rows.  Writes h_out, the r, z, n gate
 * planes (when gates != NULL) and the head partials (when logit_part != NULL); the fourth plane (hn = b_hh[2H:3H]) only
 * when write_hn != 0 -- tmpnn_gru_bwd_fused_zero_state does not read it. */
int tmpnn_gru_fwd_tiles_zero_state_available(int H, int xmode);
int tmpnn_gru_fwd_tiles_zero_state(const tmpnn_edge_tiles* tiles, int R, const float* proj, int ld_proj, int H,
                                   const float* b_ih, const float* b_hh, float* h_out, int ld_out, float* gates,
                                   size_t gate_plane, int write_hn, const float* w_head, float* logit_part, size_t part_stride,
                                   tmpnn_stream stream);

/* out[r, 0:NOUT] = in[rows[r], 0:H] @ wt[H][NOUT]  (compact output rows; H in {32, 64}, NOUT = 3H):
 * the det-row projection P of tmpnn_gru_fwd's xmode 3. */
int tmpnn_rows_linear(const int32_t* rows, int R, const float* in, int ld_in, int H, const float* wt, int NOUT,
                      float* out, int ld_out, tmpnn_stream stream);

/* out [cols][rows] = in[rows][cols]^T (weight re-layout for tmpnn_gru_fwd) */
int tmpnn_transpose(const float* in, int rows, int cols, float* out, tmpnn_stream stream);

/* dst[i] (+)= sum over s < nslab of slabs[s*stride + i], i < n, in a fixed order of plain fp32 adds (one launch): up to 64 slabs
 * one after the other (t = 0; t += slab s, s ascending); more than 64 in two levels, the same sum over each group of 32
 * consecutive slabs and then over the group sums in ascending order.  accumulate: dst[i] = dst[i] + t, else dst[i] = t.
 * stride >= n; floats between n and stride are never read.  The reduction behind every per-block partial sum of the library. */
int tmpnn_reduce_slabs(const float* slabs, size_t stride, int nslab, float* dst, size_t n, int accumulate,
                       tmpnn_stream stream);

/* ---- rows C, D: input transform on the NEW rows (models/track_mpnn.py:45-52, 59-61) -------
 * Lin1 -> BatchNorm1d -> ReLU -> Lin2, evaluated only on the nd new det rows (the new edge
 * rows are all-zero inputs: they enter the BatchNorm statistics as `b1` and are masked to zero
 * afterwards, track_mpnn.py:61).  Statistics are per segment (= per window of a block-diagonal
 * batch; one segment reproduces the reference):
 *   xdet [nd][ld_x] gathered det-row features (group columns start at xdet), F inputs
 *   seg_ptr [S+1] det rows of segment s are [seg_ptr[s], seg_ptr[s+1]); seg_cnt [S] = ALL new
 *   rows of the segment (dets + zero rows).  A segment may hold no det rows (seg_ptr[s] == seg_ptr[s+1]: a window
 *   that contributes zero rows only), provided seg_cnt[s] >= 2.
 *   training: batch stats (biased var, eps 1e-5) written to mean/rstd [S][H] and running stats
 *   updated sequentially over segments with momentum 0.1 (unbiased var); else running stats.
 *   y_save [nd][H] = Lin1 output (saved for backward); out rows written to
 *   h_new[out_row[i], 0:H] (ld_h). */
int tmpnn_input_bn_fwd(const float* xdet, int ld_x, int F, int nd, const int32_t* seg_ptr,
                       const int32_t* seg_cnt, const int32_t* seg_of_det /* [nd] segment of each det row, or NULL */,
                       int S, int H, int training,
                       const float* w1, const float* b1, const float* gamma, const float* beta,
                       float* running_mean, float* running_var,
                       const float* w2, const float* b2,
                       float* y_save, float* mean, float* rstd, float* ws_a /* [nd][H] scratch */,
                       const int32_t* out_row, float* h_new, int ld_h, tmpnn_stream stream);
/* Backward.  d_h rows are read at out_row; mean/rstd/y_save are the forward's outputs (eval
 * mode: one row holding the running statistics).  Accumulates (+=) dw1 [H][F], db1, dgamma,
 * dbeta, dw2 [H][H], db2; writes d_xdet [nd][ld_dx] (may be NULL) and d_xzero [S][F] (may be
 * NULL): the gradient every all-zero row of segment s receives through the batch statistics
 * (0 in eval mode).  ws: tmpnn_input_bn_bwd_ws(nd, S, H, F) floats. */
size_t tmpnn_input_bn_bwd_ws(int nd, int S, int H, int F);
int tmpnn_input_bn_bwd(const float* xdet, int ld_x, int F, int nd, const int32_t* seg_ptr,
                       const int32_t* seg_cnt, const int32_t* seg_of_det, int S, int H, int training,
                       const float* w1, const float* b1, const float* gamma, const float* beta,
                       const float* w2,
                       const float* y_save, const float* mean, const float* rstd,
                       const int32_t* out_row, const float* d_h, int ld_dh,
                       float* d_xdet, int ld_dx, float* d_xzero,
                       float* dw1, float* db1, float* dgamma, float* dbeta, float* dw2, float* db2,
                       float* ws, size_t ws_floats, tmpnn_stream stream);

/* The same transform in ONE launch per direction for batches of SHORT segments (csrc/intf.hip): a workgroup owns whole
 * segments, so the per-segment statistics, the BatchNorm backward's segment sums and the gradient of the zero rows never
 * leave it.  Arguments and results as tmpnn_input_bn_fwd / _bwd (no activation workspace; the backward's workspace holds
 * one slab of parameter gradients per workgroup, added into dw1 .. db2 in a fixed order) plus max_seg_rows = the longest
 * segment's number of det rows, which the host knows from its plan.  tmpnn_input_tf_supported: H in {32, 64}, F <= 128,
 * max_seg_rows <= 128 -- callers use tmpnn_input_bn_* otherwise (one window of thousands of dets is ONE segment).
 * x_rows (int64 [nd], or NULL): det row i's features are row x_rows[i] of `xdet` -- the caller's x [n, F] with its new det
 * rows listed (the gather of the det rows out of x rides in the kernel's own staging pass); NULL: row i. */
int tmpnn_input_tf_supported(int H, int F, int max_seg_rows);
int tmpnn_input_tf_fwd(const float* xdet, const int64_t* x_rows, int ld_x, int F, int nd, const int32_t* seg_ptr, const int32_t* seg_cnt,
                       const int32_t* seg_of_det, int S, int max_seg_rows, int H, int training, const float* w1, const float* b1,
                       const float* gamma, const float* beta, float* running_mean, float* running_var, const float* w2,
                       const float* b2, float* y_save, float* mean, float* rstd, const int32_t* out_row, float* h_new,
                       int ld_h, tmpnn_stream stream);
size_t tmpnn_input_tf_bwd_ws(int nd, int S, int H, int F, int training);   /* bytes */
int tmpnn_input_tf_bwd(const float* xdet, const int64_t* x_rows, int ld_x, int F, int nd, const int32_t* seg_ptr, const int32_t* seg_cnt,
                       const int32_t* seg_of_det, int S, int max_seg_rows, int H, int training, const float* w1, const float* b1,
                       const float* gamma, const float* beta, const float* w2, const float* y_save, const float* mean,
                       const float* rstd, const int32_t* out_row, const float* d_h, int ld_dh, float* d_xdet, int ld_dx,
                       float* d_xzero, float* dw1, float* db1, float* dgamma, float* dbeta, float* dw2, float* db2, void* ws,
                       size_t ws_bytes, tmpnn_stream stream);

/* ---- row J: masked output heads + sigmoid (models/track_mpnn.py:72-75) -------------------
 * logits[i] = is_edge[i] ? w_e . h[i] + b_e : w_n . h[i] + b_n ; scores = sigmoid(logits).
 * h [N][ld_h], C = G*H columns. */
int tmpnn_heads_fwd(const float* h, int ld_h, int C, int N, const uint8_t* is_edge,
                    const float* w_node, const float* b_node, const float* w_edge, const float* b_edge,
                    float* logits, float* scores, tmpnn_stream stream);
/* logits[i] = sum_p parts[p*part_stride + i] + (is_edge[i] ? b_edge : b_node) ; scores = sigmoid(logits). */
int tmpnn_heads_finish(const float* parts, size_t part_stride, int nparts, int N, const uint8_t* is_edge,
                       const float* b_node, const float* b_edge, float* logits, float* scores, tmpnn_stream stream);
/* dy = d_logits + d_scores * s(1-s) (either may be NULL).  dy_out [N] (may be NULL) receives dy;
 * d_h (may be NULL): d_h[i] (=|+=) dy[i] * w_type(i); dw_node/dw_edge [C], db_node/db_edge [1]
 * accumulated (+=).  ws: tmpnn_heads_bwd_ws(N, C) bytes. */
size_t tmpnn_heads_bwd_ws(int N, int C);
int tmpnn_heads_bwd(const float* h, int ld_h, int C, int N, const uint8_t* is_edge,
                    const float* w_node, const float* w_edge, const float* scores,
                    const float* d_logits, const float* d_scores, float* dy_out,
                    float* d_h, int ld_dh, int accumulate,
                    float* dw_node, float* db_node, float* dw_edge, float* db_edge,
                    void* ws, size_t ws_bytes, tmpnn_stream stream);

/* ---- training targets and losses on the same CSR (models/loss.py) ---------------
 * labels / targets: uint8 [N] (1 = positive).  A det's PAST edges are its CSR entries with the sign bit set,
 * its FUTURE edges the others, both in ascending edge-row order.
 *
 * tmpnn_targets (create_targets, loss.py:8-44): targets[det] = labels[det]; per det the LAST label-positive
 * past edge and the FIRST label-positive future edge get target 1, every other edge 0. */
int tmpnn_targets(const tmpnn_graph* g, const uint8_t* labels, uint8_t* targets, tmpnn_stream stream);
/* CELoss (loss.py:77-115): loss[0] = sum over dets and over their two sets (past, future) that contain a
 * positive target of cross_entropy(logits[set], target) / |set|  (target = last positive of the past set,
 * first positive of the future set).  stats [Dn][2][4] (max, sum exp, target row, set size) is saved for the
 * backward; ws: tmpnn_ce_loss_ws(Dn) floats.  Backward: d_logits[edge rows] += d_loss[0] * d loss / d logit;
 * src_pos/dst_pos [E] = det INDEX of each edge's endpoints. */
size_t tmpnn_ce_loss_ws(int Dn);
int tmpnn_ce_loss_fwd(const tmpnn_graph* g, const float* logits, const uint8_t* targets, float* stats, float* loss,
                      float* ws, size_t ws_floats, tmpnn_stream stream);
int tmpnn_ce_loss_bwd(const tmpnn_graph* g, const int32_t* src_pos, const int32_t* dst_pos, const float* logits,
                      const float* stats, const float* d_loss, float* d_logits, tmpnn_stream stream);
/* FocalLoss (loss.py:47-74) over the R rows listed in `rows`: loss_sum[0] = sum_i -(1-pt_i)^gamma log(pt_i) alpha_t,
 * pt = (t ? s : 1-s) + 1e-10 (the caller divides by R for size_average).  Backward: d_scores[row] += d_loss[0] *
 * scale * d loss_i / d s.  ws: tmpnn_focal_loss_ws(R) floats. */
size_t tmpnn_focal_loss_ws(int R);
int tmpnn_focal_loss_fwd(const int32_t* rows, int R, const float* scores, const uint8_t* targets, float gamma,
                         int use_alpha, float alpha0, float alpha1, float* loss_sum, float* ws, size_t ws_floats,
                         tmpnn_stream stream);
int tmpnn_focal_loss_bwd(const int32_t* rows, int R, const float* scores, const uint8_t* targets, float gamma,
                         int use_alpha, float alpha0, float alpha1, const float* d_loss, float scale, float* d_scores,
                         tmpnn_stream stream);
/* Binary cross-entropy with logits, SUMMED over n elements -- the loss SURVEY 8(d)'s metric is quoted with (BCE on every logit of
 * a call against fixed {0,1} targets; `torch.nn.functional.binary_cross_entropy_with_logits(reduction='sum')`):
 * loss_sum[0] = sum_i max(l_i, 0) - l_i t_i + log(1 + exp(-|l_i|)), fixed summation order (bitwise reproducible);
 * backward d_logits[i] = d_loss[0] * (sigmoid(l_i) - t_i).  targets: float [n].  ws: tmpnn_bce_logits_ws(n) floats. */
size_t tmpnn_bce_logits_ws(long n);
int tmpnn_bce_logits_sum_fwd(const float* logits, const float* targets, long n, float* loss_sum, float* ws, size_t ws_floats,
                             tmpnn_stream stream);
int tmpnn_bce_logits_sum_bwd(const float* logits, const float* targets, long n, const float* d_loss, float* d_logits,
                             tmpnn_stream stream);
/* train.py:70-81 for one forward call of a batch-1 window in ONE launch each way: create_targets, the cross-entropy over the
 * logits and the two focal terms with gamma = 0 and no alpha (edge rows; det rows too with the TP classifier), bit for bit
 * the values tmpnn_targets / tmpnn_ce_loss_* / tmpnn_focal_loss_* produce (same expressions, sums in the same order).
 * out [4]: loss_c, focal sum over the edge rows, focal sum over the det rows, loss_f (= mean + mean, NaN over an empty
 * selection as loss.mean() gives).  targets [N] and stats [Dn][2][4] are kept for the backward.  ws: tmpnn_train_losses_ws
 * floats.  Supported while E, Dn <= 8192 (tmpnn_train_losses_supported); larger graphs take the separate entry points.
 * Backward: d_logits [N] / d_scores [N] (either may be NULL) are WRITTEN for every row (zeros where a row has no term);
 * d_c / d_f: the two seeds (device scalars). */
int tmpnn_train_losses_supported(int E, int Dn);
size_t tmpnn_train_losses_ws(int E, int Dn);
int tmpnn_train_losses_fwd(const tmpnn_graph* g, const float* logits, const float* scores, const uint8_t* labels,
                           int tp_classifier, uint8_t* targets, float* stats, float* out, float* ws, size_t ws_floats,
                           tmpnn_stream stream);
int tmpnn_train_losses_bwd(const tmpnn_graph* g, const int32_t* src_pos, const int32_t* dst_pos, const float* logits,
                           const float* scores, const uint8_t* targets, const float* stats, const float* d_c, const float* d_f,
                           int tp_classifier, float* d_logits, float* d_scores, tmpnn_stream stream);
/* The same losses for MANY windows of one call of a block-diagonal batch (trackmpnn_amd.train_batch.build_train_batch): per window
 * its own create_targets, cross-entropy sum, focal sums and loss_f (= mean over its det rows + mean over its edge rows with the
 * TP classifier, the edge mean without; NaN over an empty selection), the reference's per-chunk bookkeeping (train.py:70-81)
 * kept apart for every window.  A window's lists name the det / edge INDICES (positions in det_row / edge_row) of its rows,
 * ascending; every det of a listed det's CSR run and every endpoint of a listed edge must belong to the same window (the
 * block-diagonal layout guarantees it).  A window with no rows at all (finished, or not in the batch) gets 0 in every output
 * and its rows' gradients are 0.  Values and sums are formed exactly as tmpnn_train_losses_fwd forms them on the window's own
 * subgraph (128-row chunks, four interleaved sums, the chunks in sequence), with no row limit per window.
 * out [4][W]: loss_c, focal sum over the edge rows, focal sum over the det rows, loss_f -- one row of W values each.  targets [N] is written on the rows of
 * the listed windows only; stats [Dn][2][4] on their dets.  ws: tmpnn_train_losses_win_ws floats.
 * Backward: element-wise over the call's E + Dn rows, each row of d_logits / d_scores (either may be NULL) WRITTEN once;
 * d_c [W] / d_f [W]: the seeds per window (device). */
typedef struct tmpnn_loss_windows {
    int32_t W;                /* windows */
    int32_t n_det;            /* det_ptr[W] (host copy: sizes the workspace) */
    int32_t n_edge;           /* edge_ptr[W] */
    const int32_t* det_ptr;   /* [W + 1] */
    const int32_t* det_idx;   /* [n_det]  det indices, window by window, ascending within a window */
    const int32_t* edge_ptr;  /* [W + 1] */
    const int32_t* edge_idx;  /* [n_edge] edge indices, likewise */
    const int32_t* det_win;   /* [Dn] window of every det, -1 = none */
    const int32_t* edge_win;  /* [E]  window of every edge, -1 = none */
} tmpnn_loss_windows;
size_t tmpnn_train_losses_win_ws(const tmpnn_loss_windows* w);
int tmpnn_train_losses_win_fwd(const tmpnn_graph* g, const tmpnn_loss_windows* w, const float* logits, const float* scores,
                               const uint8_t* labels, int tp_classifier, uint8_t* targets, float* stats, float* out, float* ws,
                               size_t ws_floats, tmpnn_stream stream);
int tmpnn_train_losses_win_bwd(const tmpnn_graph* g, const tmpnn_loss_windows* w, const int32_t* src_pos, const int32_t* dst_pos,
                               const float* logits, const float* scores, const uint8_t* targets, const float* stats,
                               const float* d_c, const float* d_f, int tp_classifier, float* d_logits, float* d_scores,
                               tmpnn_stream stream);

/* The training monitor (train.py:86-88, :125-127, :157-171): classification counts per forward call and the running statistics of
 * an epoch, on the device.  pred = score > 0.5f (strict: argmax((1 - s, s)) with the tie going to class 0); targets: the bytes the
 * loss forward wrote.  The counted rows S are the det and the edge rows of the graph (window) with the TP classifier, its edge
 * rows alone without.  A counts record is four int32: tp = #{pred and t}, fp = #{pred and not t}, fn = #{not pred and t} over S,
 * and rows = det rows + edge rows of the graph (window) in either mode; rows > 0 is what makes a (call, window) pair a forward.
 * Integer counts (ballot + popcount per wave, the waves combined in a fixed order), no atomics: exact and repeatable.
 *   tmpnn_cls_counts: one graph, counts [4].
 *   tmpnn_cls_counts_win: every window of one call of a block-diagonal batch, over the det_idx / edge_idx lists the windowed
 *     loss walks (no row limit per window); counts [4][W], a window with no rows gets zeros.
 *   tmpnn_train_record_fold: ONE launch that adds a step to the record: for every pair of counts [C][4][W] with rows > 0 its
 *     F1 = 2 tp / (2 tp + fp + fn) in fp64 (0 when the denominator is 0: zero_division=0) and one forward; for every chunk
 *     b < B its loss_c[b], loss_f[b] and float(loss_c[b] + loss_f[b]) (fp32 values, summed in fp64) and one chunk.  The sums
 *     are taken in a fixed order.  The record is device memory the caller zeroes (an epoch boundary) and reads. */
typedef struct tmpnn_train_record {
    double sum_f1;       /* over the forwards */
    int64_t forwards;
    double sum_loss_c;   /* over the chunks */
    double sum_loss_f;
    double sum_loss;     /* of float(loss_c + loss_f) */
    int64_t chunks;
} tmpnn_train_record;
int tmpnn_cls_counts(const tmpnn_graph* g, const float* scores, const uint8_t* targets, int tp_classifier, int32_t* counts,
                     tmpnn_stream stream);
int tmpnn_cls_counts_win(const tmpnn_graph* g, const tmpnn_loss_windows* w, const float* scores, const uint8_t* targets,
                         int tp_classifier, int32_t* counts, tmpnn_stream stream);
int tmpnn_train_record_fold(const int32_t* counts, int C, int W, const float* loss_c, const float* loss_f, int B,
                            tmpnn_train_record* rec, tmpnn_stream stream);
/* The embedding network's loss of the same chunks (train.py:157-163 logs its epoch mean): ONE launch that adds loss_d[kept[k]],
 * k < n_kept (kept NULL: loss_d[k]), as fp32 values summed in fp64 in a fixed order, and the number of chunks added, to a record
 * of its own.  loss_d [n_loss]; an index outside [0, n_loss) is skipped and counted in `skipped`. */
typedef struct tmpnn_embed_record {
    double sum_loss_d;   /* over the chunks */
    int64_t chunks;
    int64_t skipped;
} tmpnn_embed_record;
int tmpnn_train_embed_fold(const float* loss_d, int n_loss, const int64_t* kept, int n_kept, tmpnn_embed_record* rec,
                           tmpnn_stream stream);

/* The optimizer step (train.py:135 `optimizer_trk.step()` of the `optim.Adam(model.parameters(), lr, weight_decay)` of
 * train.py:329; the learning rate is whatever the StepLR of train.py:330 last set) and the gradient statistics of
 * --plot-gradients (utils/gradients.py:23: `p.grad.abs().mean()` per parameter), each in ONE launch over the flat gradient
 * bucket (trackmpnn_amd.dist.GradBucket).
 * A parameter keeps its own storage: segment s of the table says where it lives and which slice [start, start + count) of the
 * three flat fp32 buffers (gradient, exp_avg, exp_avg_sq; n_flat elements each, 16-byte aligned) belongs to it.  The work list
 * holds one (segment, offset inside the segment) int32 pair per chunk of tmpnn_optim_chunk() elements (offsets are multiples of
 * it); both tables are device memory the caller builds once.  A pair or a segment that does not fit (segment >= P, a slice
 * outside [0, n_flat), an offset outside the segment) is skipped by the kernel.
 *   tmpnn_adam_step: with t = state->step + 1, per element (fp32, torch.optim.Adam's L2 weight decay, not AdamW):
 *       g = fl(grad * grad_scale) + weight_decay * p;   m += (1 - beta1) (g - m);   v = beta2 v + (1 - beta2) g g;
 *       p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);        grad = 0 when zero_grads
 *     lr and the step count are read from the device record, so a captured launch replays with the current values; the two
 *     bias corrections are formed once per workgroup in fp64.  The same launch sets state->step = t: every workgroup reads the
 *     record before it takes an integer ticket, and the last ticket moves the count and clears the ticket.  The product
 *     grad * grad_scale is rounded to fp32 before the decay term is added, so grad_scale = 1 / world equals
 *     `flat.mul_(1 / world)` followed by a step with grad_scale = 1, bit for bit.  No atomics on floats; repeatable bits.
 *     beta1, beta2, eps, weight_decay, grad_scale and zero_grads are launch arguments (a captured launch keeps them).
 *   tmpnn_grad_flow: stats [P][3] fp64 per segment = mean |g| (an fp64 sum in a fixed order over n), max |g| (NaN if any element
 *     is NaN, as torch.max), the number of non-finite elements.  One workgroup per segment; repeatable bits. */
typedef struct tmpnn_optim_seg {
    float* p;       /* the parameter's own storage */
    int64_t start;  /* first element of its slice of the flat buffers */
    int64_t count;  /* elements */
} tmpnn_optim_seg;
typedef struct tmpnn_adam_state { /* 16 bytes of device memory, 16-byte aligned; zero `step` and `ticket` before the first step */
    double lr;
    float step;     /* steps taken so far (what torch keeps as state['step']); exact up to 2^24 */
    int32_t ticket; /* 0 between launches */
} tmpnn_adam_state;
int tmpnn_optim_chunk(void);
int tmpnn_adam_step(const tmpnn_optim_seg* segs, int P, const int32_t* work, int nwork, float* grad, float* exp_avg,
                    float* exp_avg_sq, int64_t n_flat, tmpnn_adam_state* state, double beta1, double beta2, double eps,
                    double weight_decay, float grad_scale, int zero_grads, tmpnn_stream stream);
int tmpnn_grad_flow(const tmpnn_optim_seg* segs, int P, const float* grad, int64_t n_flat, double* stats, tmpnn_stream stream);

/* The training batch of trackmpnn_amd.train_batch.build_train_batch, built on the device (build_train_batch_device): the
 * train-mode graphs of every call of a block-diagonal batch of chunks (utils/graph.py:96-186, 189-334 with mode='train').
 * Input: chunk i is y[offsets[i] .. offsets[i+1]) of the stacked labels y [ND][2] = (timestep, track id); a value that was not
 * an integer is passed as TMPNN_TB_NONINT.  Three steps, one workgroup per chunk, the chunk's dets and per-det state in LDS:
 *   tmpnn_train_build_count: per input chunk, info[i][4] = {status (TMPNN_TB_* bits, 0 = valid), calls of the chunk (0 = the
 *     reference skips it: fewer than two timesteps or every track id -1), t0, t1}.  The host reads info once.
 *   tmpnn_train_build_calls: per kept chunk b and call c < ncalls_b, counts[cptr[b] + c] = {new edge rows, new det rows}.
 *     The host forms the call-major offsets (blk, cb_tab, call_tab) from them and reads the per-call totals once.
 *   tmpnn_train_build_fill phase 0: every index array except inc; rowptr holds {0, degree of every det} per call, which the
 *     caller turns into offsets with an inclusive scan per call; phase 1: inc (needs those offsets).
 * calls / fill check every kept chunk against max_dets, max_slots and C on the device: one that does not fit gets nothing
 * written and TMPNN_TB_ST_LDS in info[i][0], which the caller reads with the per-call totals.
 * Placement comes from the offsets: no atomics in global memory, the output is deterministic.  Limits per chunk: at most
 * TMPNN_TB_MAX_DETS detections and TMPNN_TB_MAX_CALLS calls (1 + tN - t1); rows and edges of the batch fit in int32. */
#define TMPNN_TB_MAX_DETS 4096
#define TMPNN_TB_MAX_CALLS 1024
#define TMPNN_TB_NONINT INT64_MIN          /* marks a non-integral label value */
#define TMPNN_TB_ST_NONINT 1               /* status bits of tmpnn_train_build_count */
#define TMPNN_TB_ST_NEGTS 2
#define TMPNN_TB_ST_RANGE 4
#define TMPNN_TB_ST_DETS 8
#define TMPNN_TB_ST_CALLS 16
#define TMPNN_TB_ST_OFFSETS 32
#define TMPNN_TB_ST_LDS 64                 /* set by calls / fill: the chunk exceeds max_dets, max_slots or C (nothing written) */
typedef struct tmpnn_train_build {
    int32_t n;                  /* input chunks */
    int32_t B;                  /* kept chunks (calls / fill) */
    int32_t C;                  /* calls of the batch = max ncalls_b (fill) */
    int32_t max_dets;           /* a power of two >= every kept chunk's detections (calls / fill: sizes the LDS) */
    int32_t max_slots;          /* >= 2 + every kept chunk's calls */
    int64_t n_feat;             /* rows of y (= offsets[n]; count: offsets beyond it are invalid; fill: feat_src of edge rows) */
    const int64_t* y;           /* [ND][2] */
    const int64_t* offsets;     /* [n + 1] */
    int64_t* info;              /* [n][4] count output */
    const int32_t* kept;        /* [B] input chunk of batch chunk b */
    const int32_t* cptr;        /* [B + 1] first entry of chunk b in the per-(chunk, call) tables */
    int32_t* counts;            /* [cptr[B]][2] calls output */
    const int32_t* blk;         /* [cptr[B]][4] block (b, c): first row, edge, det of the call-major layout, segment in call c */
    const int64_t* call_tab;    /* [7][C] rows before call c; first element of call c in rowptr, inc, det_order / det_win,
                                   edge_win, det_idx, edge_idx */
    const int32_t* cb_tab;      /* [3][C][B] first element of chunk b in call c's det_order, det_idx, edge_idx */
    /* prefix-stable outputs, sized for the last call */
    int32_t* src; int32_t* dst; int32_t* edge_row; int32_t* src_pos; int32_t* dst_pos;     /* [E] */
    int32_t* det_row; int32_t* seg_of_det; int64_t* new_det_local; int64_t* det_group;     /* [Dn] */
    uint8_t* is_edge; int32_t* pos; uint8_t* labels; int64_t* feat_src; int64_t* seg_of_new;   /* [N] */
    /* per call, concatenated */
    int32_t* rowptr; int32_t* inc; int32_t* det_order; int32_t* det_win; int32_t* edge_win; int32_t* det_idx; int32_t* edge_idx;
} tmpnn_train_build;
int tmpnn_train_build_count(const tmpnn_train_build* d, tmpnn_stream stream);
int tmpnn_train_build_calls(const tmpnn_train_build* d, tmpnn_stream stream);
int tmpnn_train_build_fill(const tmpnn_train_build* d, int phase, tmpnn_stream stream);

/* A seeded draw of B augmented training chunks from a device-resident detection store (trackmpnn_amd.chunks: DetectionStore,
 * ChunkSampler.draw; the host definition is draw_chunks_host), written in the stacked form tmpnn_train_build_* take: the
 * reference's --random-transforms (dataset/kitti_mot.py:494-532: time reversal, horizontal flip, per-detection dropout).
 * The store keeps the detections sorted by (sequence, frame): the detections of frame f of sequence s are
 * first[seq_base[s] + f] .. first[seq_base[s] + f + 1).  Per detection it holds the track id and the standardised static
 * feature row of the plain box and of the flipped box (stat[det][0 / 1][Fs]); table[t mod fr_range][2] holds the standardised
 * temporal pair.  So the device only selects and gathers: no feature arithmetic runs here.
 * Chunk ci of the table is chunks[ci][4 + L] = {sequence, frames in its list, detections before dropout, 0, frame list (L
 * entries, padded with -1)}; its rows before dropout are the detections of its frames in list order.  Drawn chunk b is chunk
 * indices[b].  Decisions come from Philox4x32-10 with key = (seed low, seed high) and counter = (j, ci, step low, step high):
 * block j = 0 gives reversal (word 0) and flip (word 1), word w of block j >= 1 decides row 4 (j - 1) + w of the chunk; with
 * u = (word >> 8) * 2^-24 the event happens iff u < p.  A chunk's draw depends on (seed, step, ci) only, not on the batch.
 * Time reversal: t' = last frame of the list - t + first frame of the list.
 *   tmpnn_chunk_draw_count: count[b] = rows kept, flags[b], and offsets[B + 1] = the exclusive scan of count (two launches:
 *     one workgroup per chunk, then one workgroup for the scan).
 *   tmpnn_chunk_draw_fill: the same decisions again (nothing is stored between the two); kept row k of chunk b goes to row
 *     offsets[b] + k: y = (t', track id), X = the static row of the plain or the flipped box, then table[t' mod fr_range] when
 *     F = Fs + 2.  Rows of X and y from offsets[B] on are not written.
 * A chunk that does not pass the device's own checks of the tables (an index, a sequence or a frame out of range, a size that
 * is not the table's, more than TMPNN_TB_MAX_DETS rows) is drawn as an empty chunk with TMPNN_CD_FLAG_BAD set.  No atomics;
 * the output is deterministic. */
#define TMPNN_CD_MAX_FRAMES 256            /* frames of one chunk's list */
#define TMPNN_CD_FLAG_REVERSED 1
#define TMPNN_CD_FLAG_FLIPPED 2
#define TMPNN_CD_FLAG_BAD 128
typedef struct tmpnn_chunk_draw {
    int32_t B;                  /* drawn chunks */
    int32_t nchunks;            /* chunks of the table */
    int32_t L;                  /* entries of a chunk's frame list, 1 .. TMPNN_CD_MAX_FRAMES */
    int32_t nseq;               /* sequences of the store */
    int32_t F;                  /* columns of X: Fs, or Fs + 2 with the temporal pair */
    int32_t Fs;                 /* columns of the static row */
    int32_t fr_range;           /* rows of table */
    int32_t transforms;         /* 0: the plain chunks (no random numbers, flags 0) */
    int64_t ndets;              /* detections of the store */
    int64_t nframes;            /* frames of the store = seq_base[nseq] */
    int64_t n_max;              /* rows of X and y: the sum of the drawn chunks' sizes before dropout, < 2^31 */
    uint64_t seed;
    uint64_t step;
    float p_drop;
    float p_reverse;
    float p_flip;
    int32_t ldx;                /* row stride of X in floats, >= F; 0 (the field was reserved and zero before): F */
    const int32_t* indices;     /* [B] */
    const int32_t* chunks;      /* [nchunks][4 + L] */
    const int32_t* seq_base;    /* [nseq + 1] */
    const int32_t* first;       /* [nframes + 1] */
    const int32_t* track;       /* [ndets] */
    const float* stat;          /* [ndets][2][Fs] */
    const float* table;         /* [fr_range][2] (F = Fs + 2) */
    int32_t* count;             /* [B] */
    uint8_t* flags;             /* [B] */
    int64_t* offsets;           /* [B + 1] */
    float* X;                   /* [n_max][ldx] */
    int64_t* y;                 /* [n_max][2], 16-byte aligned */
} tmpnn_chunk_draw;
int tmpnn_chunk_draw_count(const tmpnn_chunk_draw* d, tmpnn_stream stream);
int tmpnn_chunk_draw_fill(const tmpnn_chunk_draw* d, tmpnn_stream stream);

/* What a store with the 'vis' feature group adds to a draw: per kept row the box its features were made from, its image's
 * size, the image it needs and its track id -- the arguments of tmpnn_vis_head_fwd.  The store holds, per detection, the plain
 * and the mirrored box (box[det][0 / 1][4], float32: the flip in float64 on the raw box, then narrowed, as for stat) and per
 * sequence the image size.  slot[b][k] is the image of listed frame k of drawn chunk b: the row of the draw's frame plan, built
 * on the host from the same Philox block j = 0 that decides the flip (trackmpnn_amd.chunks.ChunkSampler.frame_plan).
 *   tmpnn_chunk_draw_vis: one launch behind tmpnn_chunk_draw_fill with the same descriptor (offsets written by
 *     tmpnn_chunk_draw_count); one workgroup per chunk, the same decisions once more.  Kept row k of chunk b goes to row
 *     offsets[b] + k: o_box = the plain or the mirrored box (one 16-byte store), o_im_hw = the sequence's (h, w), o_map_of =
 *     slot[b][list index of the row's frame], o_track = the track id.  Time reversal changes none of them.  Rows from offsets[B]
 *     on are not written, and a chunk with TMPNN_CD_FLAG_BAD writes nothing.  No atomics. */
typedef struct tmpnn_chunk_vis {
    const float* box;           /* [ndets][2][4] x1 y1 x2 y2: plain, mirrored; 16-byte aligned */
    const float* seq_hw;        /* [nseq][2]: image height, width; 8-byte aligned */
    const int32_t* slot;        /* [B][L] */
    float* o_box;               /* [n_max][4], 16-byte aligned */
    float* o_im_hw;             /* [n_max][2], 8-byte aligned */
    int32_t* o_map_of;          /* [n_max] */
    int32_t* o_track;           /* [n_max] */
} tmpnn_chunk_vis;
int tmpnn_chunk_draw_vis(const tmpnn_chunk_draw* d, const tmpnn_chunk_vis* v, tmpnn_stream stream);

/* Whole-sequence features from the same store (csrc/seqfeat.hip; trackmpnn_amd.seqfeat.SequenceFeatures; host definition:
 * sequence_features_host): the reference's `val` / `test` sample, every detection of a sequence in the store's order, no
 * transforms.  K listed sequences are packed one behind the other: listed sequence k = seqs[k] owns the packed rows
 * offsets[k] .. offsets[k + 1], which are the store's rows first[seq_base[s]] .. first[seq_base[s + 1]] in order.  Packed row i
 * of store row r and frame t = frame[r]:  X[i][0 .. Fs) = stat[r][0] (the plain box), X[i][Fs .. Fs + 2) = table[t mod fr_range]
 * when F = Fs + 2, y[i] = (t, track[r]); columns F .. ldx of X are not written (the 'vis' group: tmpnn_vis_head_fwd fills them).
 * With box != NULL the same launch writes the visual head's arguments: o_box = box[r][0], o_im_hw = seq_hw[s], o_map_of =
 * t mod frames_per_batch (the row's image inside a batch of frames_per_batch frames aligned to its multiples).
 *   tmpnn_seq_features: ONE launch, a workgroup per 256 packed rows; nothing is computed, every value is selected.  X is stored
 *     in 4-byte words, a wave 64 consecutive ones: a row of 8, 10, 13, 15, 138 or 143 floats is in general not 16-byte aligned
 *     and a sequence's packed base falls at any row, so no wider store is used for it; y, o_box and o_im_hw are whole rows of 16,
 *     16 and 8 bytes.  n_rows = 0 launches nothing.
 * Every entry the kernel indexes by is checked against the store's totals first: the listed sequence, its frame range, its row
 * range and that this range has the size the packed offsets give it, the row's frame and that `first` brackets the row at
 * that frame.  A row that fails is not written and ORs a bit into flag[0] (1: the sequence list or the packed offsets, 2:
 * seq_base / first, 4: frame): reachable only if the device tables were overwritten, never an out-of-range access. */
#define TMPNN_SF_FLAG_LIST 1
#define TMPNN_SF_FLAG_RANGE 2
#define TMPNN_SF_FLAG_FRAME 4
typedef struct tmpnn_seq_features_args {
    int32_t K;                  /* listed sequences, >= 1 */
    int32_t nseq;               /* sequences of the store */
    int32_t F;                  /* columns written: Fs, or Fs + 2 with the temporal pair */
    int32_t Fs;                 /* columns of the static row */
    int32_t ldx;                /* row stride of X in floats, >= F */
    int32_t fr_range;           /* rows of table */
    int32_t frames_per_batch;   /* >= 1 (read with box only) */
    int32_t reserved;           /* 0 */
    int64_t ndets;              /* detections of the store */
    int64_t nframes;            /* frames of the store = seq_base[nseq] */
    int64_t n_rows;             /* packed rows = offsets[K], < 2^31 */
    const int32_t* seqs;        /* [K] */
    const int64_t* offsets;     /* [K + 1] */
    const int32_t* seq_base;    /* [nseq + 1] */
    const int32_t* first;       /* [nframes + 1] */
    const int32_t* frame;       /* [ndets]: frame of every detection within its sequence */
    const int32_t* track;       /* [ndets] */
    const float* stat;          /* [ndets][2][Fs] */
    const float* table;         /* [fr_range][2] (F = Fs + 2) */
    const float* box;           /* [ndets][2][4], 16-byte aligned; NULL: a store without 'vis' */
    const float* seq_hw;        /* [nseq][2], 8-byte aligned (with box) */
    float* X;                   /* [n_rows][ldx] */
    int64_t* y;                 /* [n_rows][2], 16-byte aligned */
    float* o_box;               /* [n_rows][4], 16-byte aligned (with box) */
    float* o_im_hw;             /* [n_rows][2], 8-byte aligned (with box) */
    int32_t* o_map_of;          /* [n_rows] (with box) */
    int32_t* flag;              /* [1]: ORed into, never cleared here */
} tmpnn_seq_features_args;
int tmpnn_seq_features(const tmpnn_seq_features_args* d, tmpnn_stream stream);

/* The CNN's input for the frames of a draw (csrc/frames.hip; trackmpnn_amd.frames.FrameStore; host definition: frames_host).
 * The store keeps every frame of every sequence, already resized to the CNN's input size H x W, as planar uint8 [3][H][W]; frame
 * f of sequence s lies at byte (seq_base[s] + f) * 3 * H * W (int64).  Output image i is frame plan[i] = (sequence, frame,
 * mirrored 0 / 1), mirrored along W where flagged, as float32 [T][3][H][W] with out = table[c][v]: the table, built on the host
 * with the float32 torch ops v.float().div(255).sub(mean[c]).div(std[c]) (ToTensor, then Normalize), is the definition of the
 * value, so the output is selected, not computed.
 *   tmpnn_frames_gather: one launch; a workgroup converts a run of whole rows of one image (about 4 KiB of pixels): 16-byte loads
 *     of the run into LDS (the table is staged there too), then 16-byte stores of four pixels a thread, threads along W; the
 *     mirrored read reverses within the row in LDS.  Any W up to TMPNN_FR_MAX_W: unaligned heads and tails are single loads and
 *     stores.  A plan row outside the store writes nothing (the host validates the plan).  T = 0 launches nothing. */
#define TMPNN_FR_MAX_W 8192
typedef struct tmpnn_frames_gather_args {
    int32_t T;                  /* images of the plan */
    int32_t H, W;               /* 1 <= W <= TMPNN_FR_MAX_W */
    int32_t nseq;
    int64_t nframes;            /* frames of the store = seq_base[nseq] */
    const uint8_t* frames;      /* [nframes][3][H][W], 16-byte aligned */
    const int64_t* seq_base;    /* [nseq + 1] */
    const int64_t* plan;        /* [T][3]: sequence, frame, mirrored */
    const float* table;         /* [3][256] */
    float* out;                 /* [T][3][H][W], 16-byte aligned */
} tmpnn_frames_gather_args;
int tmpnn_frames_gather(const tmpnn_frames_gather_args* a, tmpnn_stream stream);

/* Frames as decoded to the CNN's input size (csrc/resize.hip; trackmpnn_amd.frames.FrameStore.from_raw, FramePrep; host
 * definition: resize_host, prep_host).  n frames of one source size h x w, uint8 interleaved [n][h][w][3] as decoders and cameras
 * deliver them, become planar [n][3][H][W]: uint8 (what the store keeps) when table is NULL, else float32 table[c][v] (the CNN's
 * input, selected from the [3][256] table of tmpnn_frames_gather).  The resize is the 8-bit bilinear resize of the reference's
 * transforms.Resize on a PIL image: a horizontal pass when W != w, its result rounded to uint8, then a vertical pass when H != h,
 * a copy when neither differs.  Per axis the host builds bounds [out][2] = (first source index, taps) and coef [out][ksize] int32
 * (2^22 fixed point, zero beyond the taps) in doubles (trackmpnn_amd.frames.resize_coeffs); an output sample is
 * clamp((2^21 + sum_x src[first + x] * coef[x]) >> 22, 0, 255), integer arithmetic only, so the device equals resize_host byte
 * for byte.  All four tables are always passed (those of an axis that keeps its size are not read).
 *   tmpnn_frames_resize: two launches -- the horizontal pass over all n frames into the workspace [n][h][W][3], the vertical pass
 *     from it (one launch from src when W == w).  A thread owns 16 consecutive output pixels, threads along W; 16-byte loads and
 *     stores where W keeps rows aligned (W % 16 == 0; float32 output: W % 4 == 0), single accesses otherwise and for a row's tail,
 *     so any W up to TMPNN_FR_MAX_W works.  No LDS for pixels, no atomics; ksize <= TMPNN_FR_MAX_TAPS keeps the int32
 *     accumulator (at most 255 * (2^22 + ksize) + 2^21).  A bounds row outside the source gives 0.  n = 0 launches nothing.
 *   tmpnn_frames_resize_ws: bytes of that workspace (0 when W == w, when n == 0, or for sizes the call refuses). */
#define TMPNN_FR_MAX_TAPS 1024
typedef struct tmpnn_frames_resize_args {
    int32_t n;                  /* frames */
    int32_t h, w;               /* source size */
    int32_t H, W;               /* output size, 1 <= W <= TMPNN_FR_MAX_W */
    int32_t kx, ky;             /* columns of coef_x, coef_y: 1 <= ksize <= TMPNN_FR_MAX_TAPS */
    int32_t reserved;           /* 0 */
    const uint8_t* src;         /* [n][h][w][3] */
    const int32_t* bounds_x;    /* [W][2] */
    const int32_t* coef_x;      /* [W][kx] */
    const int32_t* bounds_y;    /* [H][2] */
    const int32_t* coef_y;      /* [H][ky] */
    const float* table;         /* [3][256], or NULL for uint8 output */
    void* out;                  /* uint8 or float32 [n][3][H][W] */
    void* ws;                   /* tmpnn_frames_resize_ws bytes, 16-byte aligned (NULL when W == w) */
    size_t ws_bytes;
} tmpnn_frames_resize_args;
size_t tmpnn_frames_resize_ws(int n, int h, int w, int H, int W);
int tmpnn_frames_resize(const tmpnn_frames_resize_args* a, tmpnn_stream stream);

/* ======================================================================================================
 * Batch-1 path (the reference's real call pattern, train.py:92-107 / infer.py:60-87: ONE small
 * graph per call).  Two things make a call cheap when the graph has a few thousand rows:
 *   (1) the graph's SIZES stay on the device (tmpnn_dgraph): the adjacency -> index conversion is one kernel and the
 *       host never waits for E / Dn, so nothing synchronises between calls;
 *   (2) the whole message-passing iteration is two launches forward (input transform; edge + node cells with the
 *       aggregation, the merge and the output heads fused) and two backward: tmpnn_mp_iter_fwd / _bwd.
 * Limits: N <= TMPNN_DG_BIG_ROWS rows, H in {32, 64}, no attention heads (the staged entry points above cover the
 * rest).  Arithmetic: fp32 throughout (v_mfma_f32_16x16x4_f32 = an fmaf chain), reductions in a fixed order.
 * ====================================================================================================== */
#define TMPNN_DG_MAX_ROWS 4096
#define TMPNN_DG_BIG_ROWS 65535    /* fused iteration and tmpnn_graph_from_coo_arena_ws (work arrays in a global scratch) */
#define TMPNN_TRACK_MAX_ROWS 32768 /* tracker-side operations tmpnn_track_* (row deletion keeps an N-int table in the LDS) */
#define TMPNN_DG_META 8      /* ints in tmpnn_dgraph.meta: [0] E, [1] Dn, [2] status, [3] N, rest reserved */
/* status bits (0 = the adjacency is a TrackMPNN factor graph, SURVEY 8 "graph invariants") */
#define TMPNN_DG_BAD_VALUE 1     /* an off-diagonal entry is not +-1, or an index is out of range */
#define TMPNN_DG_BAD_ROW 2       /* an edge row without exactly one +1 and one -1, or a det row with off-diagonals */
#define TMPNN_DG_BAD_ENDPOINT 4  /* an edge endpoint is not a det row */
#define TMPNN_DG_BAD_ORDER 8     /* not src row < edge row < dst row (utils/graph.py:153-156,298-301) */
#define TMPNN_DG_BAD_EDGE_DIAG 16 /* diag(edge_adj) does not complement diag(node_adj) */
#define TMPNN_DG_BAD_EDGE_ADJ 32 /* edge_adj is not node_adj^T off the diagonal */

/* Index form of one graph with device-side sizes.  All arrays are caller-owned device memory of capacity `cap`
 * rows (one arena of tmpnn_dgraph_ints(cap) int32, carved by tmpnn_dgraph_bind).  When status != 0 the producer
 * stores E = Dn = 0, so that consumers touch nothing; the host reads meta when it chooses to (deferred check). */
typedef struct tmpnn_dgraph {
    int32_t N;          /* rows of the state tensor: host-known (the adjacency's shape) */
    int32_t cap;        /* capacity of the arrays, >= N */
    int32_t* meta;      /* [TMPNN_DG_META] */
    uint8_t* is_edge;   /* [cap]   1 on edge rows */
    int32_t* pos;       /* [cap]   row -> index within its type */
    int32_t* src;       /* [cap]   per edge index: ROW of the +1 det */
    int32_t* dst;       /* [cap]   per edge index: ROW of the -1 det */
    int32_t* src_pos;   /* [cap]   per edge index: det INDEX of src */
    int32_t* dst_pos;   /* [cap]   per edge index: det INDEX of dst */
    int32_t* edge_row;  /* [cap]   row of edge e (ascending) */
    int32_t* det_row;   /* [cap]   row of det d (ascending) */
    int32_t* rowptr;    /* [cap+1] det -> incident edges CSR */
    int32_t* inc;       /* [2 cap] edge row | sign bit, ascending edge row per det (as tmpnn_graph.inc) */
} tmpnn_dgraph;

size_t tmpnn_dgraph_ints(int cap);
/* pure host arithmetic: point `out`'s arrays into `arena` (tmpnn_dgraph_ints(cap) int32, 16-byte aligned) */
int tmpnn_dgraph_bind(void* arena, int cap, int N, tmpnn_dgraph* out);

/* Adjacency pair -> tmpnn_dgraph in ONE launch (replaces the dense round trips of models/track_mpnn.py:55-56 and
 * models/layers.py:85-88, and validates what utils/graph.py:151-163,294-308 build).  COO entries as torch stores
 * them: idx int64 [2][nnz] (rows then columns), val fp32 [nnz]; explicit zeros and UNcoalesced diagonals are fine
 * (duplicate diagonal entries are summed; duplicate off-diagonal entries make the row invalid).  edge_idx may be
 * NULL (no cross-check).  N <= TMPNN_DG_MAX_ROWS. */
int tmpnn_graph_from_coo(int N, const int64_t* node_idx, const float* node_val, int64_t nnz_node,
                         const int64_t* edge_idx, const float* edge_val, int64_t nnz_edge,
                         const tmpnn_dgraph* g, tmpnn_stream stream);

/* tmpnn_graph_from_coo on an arena of tmpnn_dgraph_ints(cap) int32 (= tmpnn_dgraph_bind + the conversion, one call) */
int tmpnn_graph_from_coo_arena(int N, const int64_t* node_idx, const float* node_val, int64_t nnz_node,
                               const int64_t* edge_idx, const float* edge_val, int64_t nnz_edge, void* arena, int cap,
                               tmpnn_stream stream);
/* The same conversion for graphs of up to TMPNN_DG_BIG_ROWS rows (dense scenes): above TMPNN_DG_MAX_ROWS the work
 * arrays do not fit the LDS and live in `ws` (tmpnn_graph_from_coo_ws_ints(N) ints, 0 for small N: then this is
 * tmpnn_graph_from_coo_arena). */
int tmpnn_graph_from_coo_arena_ws(int N, const int64_t* node_idx, const float* node_val, int64_t nnz_node,
                                  const int64_t* edge_idx, const float* edge_val, int64_t nnz_edge, void* arena, int cap,
                                  void* ws, size_t ws_ints, tmpnn_stream stream);

/* The same index form from the ROW form of a graph (type mask + the two endpoint rows of every edge row): what the
 * tracker-side operations below edit.  Same validation, same status bits. */
/* ... for graphs of up to TMPNN_DG_BIG_ROWS rows (`ws`: tmpnn_graph_from_coo_ws_ints(N) ints, as for tmpnn_graph_from_coo_arena_ws). */
int tmpnn_graph_from_rows_ws(int N, const uint8_t* is_edge, const int32_t* row_src, const int32_t* row_dst,
                             const tmpnn_dgraph* g, void* ws, size_t ws_ints, tmpnn_stream stream);

/* Parameters of the model as device pointers in the reference's layouts (state_dict keys of SURVEY 8(b)); the same
 * struct with gradient buffers is what tmpnn_mp_iter_bwd accumulates into (+=).  G <= 3 feature groups. */
typedef struct tmpnn_mp_params {
    int32_t G, H, IN_e /* H (diff) or 2H (concat) */, F_total;
    int32_t F[3];                 /* input width of each group's transform */
    float* w1[3]; float* b1[3]; float* gamma[3]; float* beta[3]; float* w2[3]; float* b2[3];   /* input_transforms.g.{0,1,3} */
    float* run_mean[3]; float* run_var[3];                                                      /* BatchNorm buffers (NULL in a gradient struct) */
    int64_t* num_batches_tracked[3];                                                            /* BatchNorm counters, +1 per training call with new rows (may be NULL) */
    float* e_wih[3]; float* e_whh[3]; float* e_bih[3]; float* e_bhh[3];                         /* factor_grus.g.edge_gru */
    float* n_wih[3]; float* n_whh[3]; float* n_bih[3]; float* n_bhh[3];                         /* factor_grus.g.node_gru */
    float* w_node; float* b_node; float* w_edge; float* b_edge;                                 /* output_transform_{node,edge} */
} tmpnn_mp_params;

/* MFMA-operand images of the four GRU weight matrices of every group (forward and backward-data forms): one
 * launch, to be repeated whenever the weights change (once per optimizer step).  prep: tmpnn_mp_iter_prep_floats. */
size_t tmpnn_mp_iter_prep_floats(int G, int H, int IN_e);
int tmpnn_mp_iter_prepare(const tmpnn_mp_params* P, float* prep, tmpnn_stream stream);

/* One TrackMPNN.forward call (models/track_mpnn.py:54-75 + models/layers.py:84-116).
 *   h [N][G*H]: rows [0, N - n_new) hold the carried state on entry; the n_new new rows are written (input
 *   transform on new det rows, zeros on new edge rows) -- this is the h the iteration reads.  x [n_new][ld_x]:
 *   features of the new rows (only det rows are read: edge rows are all-zero by contract, utils/graph.py:148,291).
 *   Outputs: h_out [N][G*H], logits [N], scores [N].  save: tmpnn_mp_iter_save_floats floats kept for
 *   tmpnn_mp_iter_bwd (may be NULL only for an inference call without new rows).  training != 0: batch statistics (one segment) + running-stat update. */
size_t tmpnn_mp_iter_save_floats(int N, int n_new, int G, int H);
int tmpnn_mp_iter_fwd(const tmpnn_mp_params* P, const float* prep, const tmpnn_dgraph* g, int n_new,
                      const float* x, int ld_x, float* h, int training,
                      float* h_out, float* logits, float* scores, float* save, size_t save_floats,
                      tmpnn_stream stream);
/* The same call in PARTS, for models with attention heads (K > 0, models/layers.py:105-112): the attention-weighted
 * aggregate replaces the signed sum between the call's two launches.  parts: bit 0 = skip the input transform launch,
 * bit 1 = skip the iteration launch, bit 2 = the aggregate es [G][N][H] (by det INDEX, the layout of the save buffer at
 * tmpnn_mp_iter_save_es_offset floats) has been written by the caller -- tmpnn_att_fwd(out = save + offset + g N H,
 * ld_out = H) on the state `h` that the input transform launch completed -- and the det tiles read it instead of forming
 * the signed sum.  Sequence: parts = 2, tmpnn_att_fwd per feature group, parts = 1 | 4.  parts = 0 is tmpnn_mp_iter_fwd.
 * bit 3 (round 6; inference only): scores[det rows] = 1 -- a model trained without the TP classifier (the reference README's
 * commands, README.md:52-67), whose detections all count as true positives in the loop (infer.py:53-56, 77-80); logits unchanged. */
size_t tmpnn_mp_iter_save_es_offset(int N, int n_new, int G, int H);
int tmpnn_mp_iter_fwd_parts(const tmpnn_mp_params* P, const float* prep, const tmpnn_dgraph* g, int n_new,
                            const float* x, int ld_x, float* h, int training,
                            float* h_out, float* logits, float* scores, float* save, size_t save_floats, int parts,
                            tmpnn_stream stream);
/* Backward of tmpnn_mp_iter_fwd.  d_scores / d_logits (N values each, element stride st_* >= 0; 0 = one broadcast
 * value, the gradient of a plain sum) and d_hout [N][G*H] may each be NULL.  Writes d_h
 * [N][G*H] (gradient of the h the iteration read: its first N - n_new rows are the gradient of the carried state)
 * and d_x [n_new][F_total] (may be NULL); ACCUMULATES (+=) every parameter gradient into `grads`.
 * ws: tmpnn_mp_iter_bwd_ws bytes. */
size_t tmpnn_mp_iter_bwd_ws(int N, int n_new, int G, int H, int IN_e);
int tmpnn_mp_iter_bwd(const tmpnn_mp_params* P, const float* prep, const tmpnn_dgraph* g, int n_new,
                      const float* x, int ld_x, const float* h, const float* h_out, const float* scores,
                      const float* save, int training,
                      const float* d_scores, int st_dscores, const float* d_logits, int st_dlogits,
                      const float* d_hout, float* d_h, float* d_x, const tmpnn_mp_params* grads,
                      void* ws, size_t ws_bytes, tmpnn_stream stream);
/* ... in PARTS: bit 0 = skip the tile launch (d_h, d_msg = the first N * G * IN_e floats of ws, weight-gradient slabs),
 * bit 1 = skip the finish launch (adjoints of the aggregations on the carried rows, slab reduction, input transform
 * backward), bit 2 = the finish launch does NOT add the adjoint of the edge -> node sum to d_h's edge rows: the caller has
 * -- tmpnn_att_bwd(d_out = ws + g IN_e, ld_dout = G IN_e, d_h + g H, ld_dh = G H) per feature group between the two.
 * Sequence: parts = 2, tmpnn_att_bwd per group, parts = 1 | 4. */
int tmpnn_mp_iter_bwd_parts(const tmpnn_mp_params* P, const float* prep, const tmpnn_dgraph* g, int n_new,
                            const float* x, int ld_x, const float* h, const float* h_out, const float* scores,
                            const float* save, int training,
                            const float* d_scores, int st_dscores, const float* d_logits, int st_dlogits,
                            const float* d_hout, float* d_h, float* d_x, const tmpnn_mp_params* grads,
                            void* ws, size_t ws_bytes, int parts, tmpnn_stream stream);

/* ======================================================================================================
 * Tracker-side graph maintenance on the device (csrc/trackops.hip).  Between two model
 * calls the reference moves a DENSE N x N adjacency and the hidden state to the host and back
 * (utils/graph.py:216-221,326-332 and :420-425,532-537).  Here the graph lives in HBM in ROW form, one entry per
 * state row, all int32 unless noted (capacity <= TMPNN_TRACK_MAX_ROWS rows):
 *     ts, det_id, assoc            y_pred[:, 0..2]: timestep (-1 on edge rows), detection id, associated next detection id
 *     is_edge (uint8), row_src, row_dst   the +1 / -1 det ROW of an edge row (-1 on det rows)
 *     labels (uint8)               ground-truth class (training; may be NULL at inference)
 * and its index form is re-derived with tmpnn_graph_from_rows after every edit.  score: P(positive) per row, fp32
 * (scores[:, 1] of the reference).  Hungarian matching and the walk that finalises tracks stay on the host.
 * ====================================================================================================== */
/* y_pred[:, 2].  mode 0 (training, utils/graph.py:229-245): through the one label-positive future edge; false
 * positives point at themselves; status bit 0 is set if a det has more than one positive future edge.
 * mode 1 (inference, greedy: :251-268 and :437-454): best-scoring future edge (>= 0.5, to a det >= 0.5) of the nearest
 * timestep. */
/* Active set at time t (utils/graph.py:270-278): rows in ascending order into active[], their number into count[0]. */
/* Append the block of timestep t behind row N (utils/graph.py:283-325): A x D edge rows (src-major) then D det rows
 * with ids new_ids[D]; labels from track[det id] (int32 [ND] track of every detection, -1 = false positive; NULL at
 * inference).  The row arrays must have room for N + A*D + D entries. */
/* The rows decode_tracks deletes (utils/graph.py:492-512) as a stream compaction: keep[] = kept rows (ascending),
 * count[0] = their number, count[2] = how many of them are det rows (count: >= 3 ints), o_* = the compacted row form with
 * renumbered endpoints. */
/* out[q][0:W] = in[keep[q]][0:W] for q < count[0] (count read on the device; the launch covers max_rows): the hidden
 * state and the scores follow the deletion without leaving HBM (utils/graph.py:514,519). */
/* decode_tracks' track finalisation (utils/graph.py:456-490) on the device: y_track [ND] = y_out[:, 1] of the sequence
 * (int32, -1 = no track yet; it stays in device memory between calls), updated for the window's dets from the
 * association links assoc[] (det ids, the output of tmpnn_track_associate or of the Hungarian matching), the scores and
 * t_upto exactly as the reference's walk over all detections does.  pos_of_det [ND]: scratch (det id -> position among
 * the graph's dets; entries of dets outside the graph are never read).  ws: tmpnn_track_finalize_ws(N) bytes, only
 * needed when the graph may hold more than 4096 dets (0 otherwise). */
size_t tmpnn_track_finalize_ws(int max_dets);

/* One call per phase of a timestep, as the reference's loops call update_graph / decode_tracks (train.py:102-104,
 * infer.py:70-87): the kernels above enqueued back to back.  At batch 1 a timestep is bound by the number of calls and
 * launches, not by their work.  `small`: int32 [4] in device memory -- [0] a count (active set / kept rows), [1] status bits
 * of the label rule, [2] kept det rows, [3] the NEXT timestep's active-set size (tmpnn_track_retire with next_t >= 0). */
typedef struct tmpnn_track_rows {   /* the row form (see above); labels may be NULL at inference */
    int32_t *ts, *det_id, *assoc;
    uint8_t* is_edge;
    int32_t *src, *dst;
    uint8_t* labels;
} tmpnn_track_rows;
/* initialize_graph (utils/graph.py:96-186): the first block of a sequence from ONE packed upload -- packed [6][N] int32 =
 * ts, det_id, is_edge, src, dst, labels rows; assoc = -1; feats [N][ld_f] = X[det id][0:F] on det rows, zeros on edge rows
 * (NULL: not written); y_track [ND] = -1 (NULL: untouched); then the index form into g (as tmpnn_graph_from_rows_ws). */
int tmpnn_track_load(int N, int ND, const int32_t* packed, const tmpnn_track_rows* rows, const float* X, int ld_x, int F,
                     float* feats, int ld_f, int32_t* y_track, const tmpnn_dgraph* g, void* ws, size_t ws_ints,
                     tmpnn_stream stream);
/* update_graph, first half (utils/graph.py:227-278): the associations (skipped with associate = 0: rows->assoc is current)
 * and the active set of timestep t -> active[], small[0]. */
int tmpnn_track_select(const tmpnn_dgraph* g, const tmpnn_track_rows* rows, const float* score, int mode, int t,
                       int associate, int32_t* active, int32_t* small, tmpnn_stream stream);
/* The same with a scratch for associate = 2: the associations by OPTIMAL ASSIGNMENT per timestep (reference hungarian(),
 * utils/graph.py:33-93 -- scipy's linear_sum_assignment restated on the device, ties included; README.md:67,122 recommends
 * --hungarian).  Inference graphs (mode 1) of <= TMPNN_DG_MAX_ROWS rows; a timestep's problem may have up to
 * tmpnn_track_hungarian_max_dets() rows / columns; cost matrices beyond 4096 entries use `ws` (fp32 [rows x columns]).  A problem
 * that fits neither sets bit 1 (value 2) of small[1] and is left unassociated: the caller then matches on the host instead. */
int tmpnn_track_select_ws(const tmpnn_dgraph* g, const tmpnn_track_rows* rows, const float* score, int mode, int t,
                          int associate, int32_t* active, int32_t* small, void* ws, size_t ws_bytes, tmpnn_stream stream);
int tmpnn_track_hungarian_max_dets(void);
/* update_graph, second half (:283-332): the block of timestep t appended behind row N (tmpnn_track_append), the features
 * of the new rows written (feats [A*D + D][ld_f]: zeros on edge rows, X[new_ids[j]][0:F] on det rows; NULL: not written)
 * and the index form of the grown graph derived into g_new (bound for N + A*D + D rows; ws / ws_ints as
 * tmpnn_graph_from_rows_ws). */
int tmpnn_track_extend(int N, int A, int D, const int32_t* active, const int32_t* new_ids, int t, const int32_t* track,
                       const tmpnn_track_rows* rows, const float* X, int ld_x, int F, float* feats, int ld_f,
                       const tmpnn_dgraph* g_new, void* ws, size_t ws_ints, tmpnn_stream stream);
/* update_graph's second half AND the input transform of the model call that follows it, in ONE launch (round 6; inference,
 * graphs of N + A*D + D <= TMPNN_DG_MAX_ROWS rows, the fused batch-1 path's H in {32, 64}): block 0 appends the block and
 * derives the grown graph's index form into g_new as tmpnn_track_extend does; G further blocks run the transform of the D new
 * dets in eval mode (running statistics) straight from X[new_ids[j]][0:F_total] into h[N + A*D + j][0:G*H] and write zeros to the
 * A*D new edge rows of h -- what the first launch of tmpnn_mp_iter_fwd(training = 0) does with the features tmpnn_track_extend
 * would have written (same code, same arithmetic order: bit-identical).  The caller follows with
 * tmpnn_mp_iter_fwd_parts(parts = 1, x = NULL).  h [N + A*D + D][G*H]: rows [0, N) hold the carried state.  save / save_floats:
 * as tmpnn_mp_iter_fwd for (N + A*D + D, A*D + D) -- the transform's Lin1 outputs and statistics land where that call puts them.
 * counts (or NULL): the `small` words of the tmpnn_track_retire call in front of this one on the stream.  The launch then takes
 * N = counts[0] and A = counts[3] ON THE DEVICE and the arguments N / A (and g_new's binding, h, save) are upper bounds the buffers
 * were sized with: the caller enqueues the timestep's first launch without waiting for the previous decode's counters, reads them
 * while it runs, and re-binds g_new's arena (same capacity) with the exact row count for the calls that follow.
 * gather_src / ld_gather / gather_keep (with counts; or NULL): that decode was called with h_new = NULL, i.e. it left the kept
 * rows' state where it was; further blocks of this launch move it -- h[q][0:G*H] = gather_src[gather_keep[q]][0:G*H] for
 * q < counts[0] -- beside the append and the transform (which touch rows >= N only). */
int tmpnn_track_extend_tf(int N, int A, int D, const int32_t* active, const int32_t* new_ids, int t, const int32_t* track,
                          const tmpnn_track_rows* rows, const float* X, int ld_x, const tmpnn_mp_params* P, float* h,
                          float* save, size_t save_floats, const tmpnn_dgraph* g_new, const int32_t* counts,
                          const float* gather_src, int ld_gather, const int32_t* gather_keep, tmpnn_stream stream);
/* decode_tracks (:431-520): associations from the scores (associate = 1: the greedy rule; 2: optimal assignment per timestep as
 * tmpnn_track_select_ws, graphs of <= TMPNN_DG_MAX_ROWS rows, its cost scratch = fin_ws / fin_ws_bytes, overflow in bit 1 of
 * small[1]; 0: rows->assoc holds them already, e.g. from a matching on the host), track finalisation, row deletion into rows_out, the state rows and scores compacted (h_new [N][ld_hn],
 * s_new [N]; small[0] / small[2] = kept rows / kept det rows; h_new = NULL on graphs of <= TMPNN_DG_MAX_ROWS rows: the kept rows'
 * state is NOT moved -- `keep` lists the rows, the caller moves them, e.g. tmpnn_track_extend_tf's gather_* arguments).  next_t >= 0: also the active set of timestep next_t on
 * the compacted rows by the inference rule -> active[], small[3]; the caller then reads small once per timestep instead of twice.
 * Greedy associations carry over (deletion removes no future edge of a kept det); with associate = 2 the next update_graph would
 * re-derive them by its own assignment sweep over the compacted graph (a det that was assigned and deleted frees its column), so
 * that sweep runs here, over the rows that stay, and rows_out->assoc holds ITS result (round 5).
 * notify (or NULL; round 6): int32 [8] in PINNED HOST memory that the runtime maps into the device's address space at the same
 * address (hipHostMalloc; checked).  The caller clears notify[4]; the launch that produces the counters stores small[0..3] into
 * notify[0..3] and then 1 into notify[4] (release order, system scope).  The host may then poll notify[4] (acquire) instead of
 * copying `small` back behind the call: it has the counts while the kept rows' state is still moving, and no copy is enqueued.
 * The device never waits for the host; a caller that does not see the flag may still synchronise and read `small`. */
int tmpnn_track_retire(const tmpnn_dgraph* g, const tmpnn_track_rows* rows, const float* score, int associate, int t_upto,
                       int ret_win, int32_t* y_track, int ND, int32_t* pos_of_det, void* fin_ws, size_t fin_ws_bytes,
                       int32_t* keep, int32_t* small, const tmpnn_track_rows* rows_out, const float* h, int ld_h, int W,
                       float* h_new, int ld_hn, float* s_new, int next_t, int32_t* active, int32_t* notify,
                       tmpnn_stream stream);

/* The validation monitor (train.py:207-219, :241-253, :278; csrc/valmon.hip): the F1 of every forward call of the validation
 * pass in ONE launch per forward, enqueued between the model call and tmpnn_track_retire.  g: the graph the model call ran on;
 * labels [N]: the tracker's row labels (tmpnn_track_rows.labels of the CURRENT row set: retire compacts them into the other
 * one); scores [N]: P(positive) per row as the model call wrote it.
 *   targets: create_targets (models/loss.py:8-44) as tmpnn_targets states it -- per det, over its CSR run in ascending edge
 *     row, the last label-positive past edge and the first label-positive future edge get 1, every other edge 0, a det its
 *     label.  An edge chosen by both endpoints counts once.  The chosen edges are a bitmap in the LDS; no targets array exists.
 *   counts: pred = score > 0.5f (strict, as tmpnn_cls_counts); tp, fp, fn over the edge rows and, tp_classifier != 0, the det
 *     rows (without the TP classifier a det's score is never read); rows = E + Dn in either mode.
 *   fold, by one thread: rows > 0 makes the call a forward -- one with an empty selection included (no TP classifier, E = 0:
 *     the reference appends f1_score([], [], zero_division=0) = 0.0).  F1 = 2 tp / (2 tp + fp + fn) in fp64, 0 where the
 *     denominator is 0; rec->sum_f1 += F1, rec->forwards += 1, the four totals += the forward's.  log (or NULL): int32
 *     [log_cap][4]; the forward's (tp, fp, fn, rows) is written at log[4 * min(forwards before, log_cap - 1)].
 * E, Dn and the status are read from g->meta on the device: a graph with status != 0 is no forward, and nothing here waits for
 * the host.  N <= TMPNN_TRACK_MAX_ROWS (checked on the host; N = 0 launches nothing).  Integer counts (ballot + popcount, the
 * waves combined in wave order, integer LDS atomics for the bitmap), one fp64 addition per launch: exact and repeatable.  The
 * record is device memory the caller zeroes and reads. */
typedef struct tmpnn_val_record {
    double sum_f1;             /* over the forwards */
    int64_t forwards;
    int64_t tp, fp, fn, rows;  /* summed over the forwards */
} tmpnn_val_record;
int tmpnn_val_f1_count(const tmpnn_dgraph* g, const uint8_t* labels, const float* scores, int tp_classifier,
                       tmpnn_val_record* rec, int32_t* log, int log_cap, tmpnn_stream stream);

/* The attention monitor (attention_weights.py:84-105; csrc/atthist.hip): per head, the histograms of the attention weights the
 * detections give to correct (`tp`) and to incorrect (`fp`) associations, ONE launch per forward and group of up to
 * TMPNN_ATT_HIST_KMAX heads, enqueued between the model call and tmpnn_track_retire.  g: the graph the model call ran on; labels
 * [N]: the tracker's row labels of the CURRENT row set; alpha: heads [heads][stride] float32, head k's weights in g's CSR order
 * (position p of g->inc) at alpha + k * stride, as tmpnn_att_fwd writes them (stride >= 2E: a shorter buffer is no forward).
 *   selection: what the reference's walk over the dense [N, N] matrices selects -- for every det row and every EDGE column with
 *     a weight > 0.  A det with incident edges: its alpha at each of them (an alpha of exactly 0 is skipped and counted in
 *     `zeros`; one above edges[bins] is skipped).  A det without incident edges (rowptr[d] == rowptr[d + 1]) has the uniform
 *     dense row 1.0f / (float)N: that value once for every edge row of the graph.  The value is `tp` where the edge row's label
 *     == 1, `fp` for every other label.
 *   bins: edges [bins + 1] float32 ascending (device memory; numpy.histogram_bin_edges of a float32 array), bins <=
 *     TMPNN_ATT_HIST_MAX_BINS.  The bin of v is the largest b with edges[b] <= v, the last bin closed: min(int(v * bins),
 *     bins - 1) stepped down / up against the table, which is numpy.histogram's rule on a uniform range -- a value that sits
 *     exactly on an edge lands where numpy puts it.
 *   record: the header below, then int64 counts [K][2][bins] (K = all heads of the model; [k][0] = tp, [k][1] = fp).  The launch
 *     adds the histograms of heads first_head .. first_head + heads - 1; count_forward != 0 (the first launch of a forward) also
 *     adds the forward to the header; `zeros` is added by every launch.
 * E, Dn and the status are read from g->meta on the device: a graph with status != 0 or without rows is no forward and leaves
 * the record untouched; nothing here waits for the host.  N <= TMPNN_TRACK_MAX_ROWS (checked on the host; N = 0 launches
 * nothing).  Integer LDS atomics into an int32 [heads][2][bins] histogram, plain int64 adds into the record by one thread per
 * cell (one workgroup, stream-ordered): exact and repeatable.  The record is device memory the caller zeroes and reads. */
#define TMPNN_ATT_HIST_KMAX 8       /* heads per launch (= the heads of one tmpnn_att_fwd call) */
#define TMPNN_ATT_HIST_MAX_BINS 64
#define TMPNN_ATT_HIST_HEADER 4     /* int64 words in front of the histogram */
typedef struct tmpnn_att_record {
    int64_t forwards;          /* forwards counted */
    int64_t dets;              /* det rows seen, summed over the forwards */
    int64_t isolated;          /* of them without an incident edge */
    int64_t zeros;             /* (head, position) pairs skipped because the weight was not > 0 */
    /* int64_t counts[K][2][bins] follows */
} tmpnn_att_record;
int tmpnn_att_hist_count(const tmpnn_dgraph* g, const uint8_t* labels, const float* alpha, int64_t stride, int heads,
                         int first_head, const float* edges, int bins, tmpnn_att_record* rec, int count_forward,
                         tmpnn_stream stream);


/* ======================================================================================================
 * Online tracking (trackmpnn_amd.online.OnlineTracker): the feature rows of one frame's raw detections, built on the
 * device (csrc/online.hip).  The reference's feature arithmetic (dataset/kitti_mot.py:545-566) in float32, per new
 * detection j < D and column c of row nd + j of X:
 *     [0, ncat)                 one-hot of the 1-based category
 *     [ncat, ncat + 5)          score, (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1
 *     has_temp: the next 2      table[t_slot][0:2]: (sin, cos) of (t mod fr_range) pi / fr_range, built by the HOST with
 *                               numpy (t_slot = t mod fr_range; table [fr_range][2], not standardised)
 *     vis_cols: the last ones   vis[j][0:vis_cols]
 * and every column stored as (v - mean[c]) / std[c], each a single correctly rounded operation: the rows equal
 * trackmpnn_amd.online.online_features_host bit for bit.  Also y_track[nd + j] = -1 and ids[nd + j] = nd + j.
 * raw [D][6] 32-bit words: category (int32), then score, x1, y1, x2, y2 (float32 bits).  X [cap][ld_x] with nd + D <= cap
 * (checked on the host); categories are NOT checked on the device (one outside 1..ncat gives an all-zero one-hot).
 * One launch; D = 0 launches nothing. */
int tmpnn_online_features(int D, int nd, int cap, int t_slot, int fr_range, int ncat, int has_temp, int vis_cols,
                          const int32_t* raw, const float* vis, int ld_vis, const float* mean, const float* std_,
                          const float* table, float* X, int ld_x, int32_t* y_track, int32_t* ids, tmpnn_stream stream);

/* ======================================================================================================
 * MOT evaluation (trackmpnn_amd.moteval.MotEvaluator): the CLEAR-MOT events of S sequences' tracks against their ground truth
 * in one launch (csrc/moteval.hip) -- what the reference's validation pass does on the host with py-motmetrics, one frame at a
 * time (utils/metrics.py:7-61, train.py:264-282).  The rule is trackmpnn_amd.moteval.mot_events_host; counts are equal to it,
 * the distances and dist_sum bit for bit.
 *
 * The store holds what does not change between evaluations, packed over the sequences (all device memory, built by
 * trackmpnn_amd.moteval.MotStore): both sides' rows sorted stably by frame, GT rows with a negative track dropped,
 *     seq      [S][8] int64    gt_base, n_gt, det_base, n_det, off_base, n_frames, obj_base, n_obj of a sequence
 *     gt_off   [n_off] int32   per sequence n_frames + 1 offsets over its frame range, relative to gt_base; det_off likewise
 *     gt_id    [n_gt] int32    object ids renumbered densely per sequence (0 .. n_obj - 1)
 *     gt_box   [n_gt][4], det_box [n_det][4] float32  x1 y1 x2 y2 (16-byte aligned)
 *     det_perm [n_det] int32   sorted position -> arrival index of a detection, relative to det_base
 * tracks [n_det] int32: y_out[:, 1] of every sequence in ARRIVAL order at its det_base; negative = no track.
 * ====================================================================================================== */
typedef struct tmpnn_mot_store {
    int32_t S, reserved;
    int64_t n_gt, n_det, n_off, n_obj; /* totals over the sequences: the lengths of the arrays below */
    const int64_t* seq;
    const int32_t* gt_off;
    const int32_t* det_off;
    const int32_t* gt_id;
    const float* gt_box;
    const float* det_box;
    const int32_t* det_perm;
} tmpnn_mot_store;
/* One per sequence.  flag: 0, or in its low byte 1 = a frame with more than tmpnn_mot_max_per_frame() GT rows or kept
 * hypotheses, 2 = a hypothesis id twice in a frame, 4 = the store is inconsistent (an offset, a permutation entry or an object
 * id out of range: nothing was read outside the arrays), 8 = the solver found no augmenting path; above it (flag >> 8) the
 * 1-based index of the frame in the sequence's range.  A flagged sequence's counts are those up to that frame. */
typedef struct tmpnn_mot_record {
    int64_t objects, predictions, matches /* switches included */, switches, false_positives, misses, frames;
    int64_t flag;
    double dist_sum; /* the matched distances, added by frame, then by position among the frame's GT rows */
} tmpnn_mot_record;
int tmpnn_mot_max_per_frame(void);
/* bytes: per sequence a cost matrix of the limit's size (used by frames whose matrix does not fit in LDS), the remembered
 * hypothesis and last matched frame per object, the tracks in sorted order */
size_t tmpnn_mot_events_ws(int S, int64_t n_obj, int64_t n_det);
/* One launch, one workgroup per sequence, out [S].  seq_host: the HOST copy of st->seq, checked against the totals before the
 * launch (the kernel checks the device copy again, and every offset it indexes by).  ws: 16-byte aligned, tmpnn_mot_events_ws
 * bytes; its contents need not survive between calls. */
int tmpnn_mot_events(const tmpnn_mot_store* st, const int64_t* seq_host, const int32_t* tracks, void* ws, size_t ws_bytes,
                     tmpnn_mot_record* out, tmpnn_stream stream);
/* out [na][nb] float64 = 1 - IoU of box_a[i], box_b[j] (x1 y1 x2 y2 float32, 16-byte aligned), NaN where it exceeds 0.5 or is
 * 0 / 0: width and height in float32, the rest in float64, bit-equal to trackmpnn_amd.moteval.mot_dist_host. */
int tmpnn_mot_dist(const float* box_a, int na, const float* box_b, int nb, double* out, tmpnn_stream stream);

/* The whole MOT-challenge summary (trackmpnn_amd.moteval.mot_summary_host; metrics.py:47-61): the record of tmpnn_mot_events
 * from the same walk, plus track coverage and fragmentations (kept per object by the walk) and the identity true positives:
 * idtp = the largest sum, over one-to-one matchings of a sequence's objects and hypotheses (the distinct tracks >= 0), of the
 * number of frames in which the pair is present at a finite distance.  idfp = predictions - idtp, idfn = objects - idtp.
 * flag as in tmpnn_mot_record (8 also: the identity assignment found no augmenting path); a flagged sequence has idtp = -1. */
typedef struct tmpnn_mot_summary_record {
    int64_t objects, predictions, matches, switches, false_positives, misses, frames;
    int64_t flag;
    double dist_sum;
    int64_t unique_objects, mostly_tracked, partially_tracked, mostly_lost; /* tracked / present >= 0.8, between, < 0.2 */
    int64_t fragmentations;
    int64_t idtp;
    int64_t hypotheses; /* distinct tracks >= 0 of the sequence */
} tmpnn_mot_summary_record;
/* which = 0: objects of a sequence up to which the walk's per-object state stays in LDS; 1: columns (the larger of objects
 * and hypotheses) up to which the identity assignment's column state stays in LDS; 2: frames per workgroup of the pair-count
 * kernel; -1 for any other `which`.  Beyond 0 and 1 the state lives in the workspace: no limit on a sequence. */
int tmpnn_mot_summary_limit(int which);
/* bytes; n_pair = the sum over the sequences of n_obj x n_det (the int32 count matrices, cleared by every call).  0 when an
 * argument is negative, n_det >= 2^28 or n_pair >= 2^40. */
size_t tmpnn_mot_summary_ws(int S, int64_t n_obj, int64_t n_det, int64_t n_pair);
/* The arguments of tmpnn_mot_events; out [S].  One clear of the count matrices and four launches, whatever S: the walk (one
 * wave per sequence), the dense index of every kept detection's hypothesis id (one workgroup per sequence), the pair counts
 * (parallel over sequences and frames, integer atomics), the assignment (one workgroup per sequence). */
int tmpnn_mot_summary(const tmpnn_mot_store* st, const int64_t* seq_host, const int32_t* tracks, void* ws, size_t ws_bytes,
                      tmpnn_mot_summary_record* out, tmpnn_stream stream);

/* HOTA (trackmpnn_amd.hota.HotaEvaluator; csrc/hota.hip) over the same store and tracks: the record of every sequence equals
 * trackmpnn_amd.hota.hota_host -- integers exactly, every double bit for bit (every float sum has a stated sequential order and
 * there is no float atomic).  All arrays run over the 19 localisation thresholds alpha = 0.05 .. 0.95.  flag as in
 * tmpnn_mot_record; a flagged sequence's sums are zero.  The derived figures (DetA, AssA, LocA, HOTA ...) are host arithmetic on
 * the record (trackmpnn_amd.hota). */
typedef struct tmpnn_hota_record {
    int64_t tp[19];                 /* matched pairs with similarity >= thresholds[a] */
    int64_t gt_dets, tracker_dets;  /* GT rows, kept detections (fn = gt_dets - tp, fp = tracker_dets - tp) */
    int64_t objects, hypotheses;    /* distinct GT ids, distinct tracks >= 0 */
    int64_t flag;
    double loc_sum[19];             /* the similarities of the counted pairs: per frame by position among the GT rows, then by frame */
    double ass_a_num[19], ass_re_num[19], ass_pr_num[19]; /* sums of m (m / max(1, gc + tc - m)), .. / max(1, gc), .. / max(1, tc) over
                                       the pairs' match counts m: per object by hypothesis index, then by object */
} tmpnn_hota_record;
/* bytes; n_off = the store's n_off, n_pair = the sum over the sequences of n_obj x n_det (84 bytes an entry: a double and 19
 * int32).  0 when an argument is negative, n_det >= 2^28 or n_pair > 2^31 / 84 (the pair workspace stays under 2 GiB). */
size_t tmpnn_hota_ws(int S, int64_t n_obj, int64_t n_det, int64_t n_off, int64_t n_pair);
/* The arguments of tmpnn_mot_events, and thresholds: 19 ascending doubles in HOST memory, read during the call (numpy's
 * arange(0.05, 0.99, 0.05) - eps: a matched pair counts at index a iff its similarity >= thresholds[a]).  out [S].  One clear
 * of the workspace's head and four launches, whatever S: the hypothesis index and the per-id row counts (one workgroup per
 * sequence), the alignment pass (one wave per sequence, frames in order), the matching (parallel over sequences and frames, a
 * wave per frame, integer atomics), the fold (one workgroup per sequence).  A frame takes tmpnn_mot_max_per_frame() rows on
 * either side. */
int tmpnn_hota(const tmpnn_mot_store* st, const int64_t* seq_host, const int32_t* tracks, const double* thresholds, void* ws,
               size_t ws_bytes, tmpnn_hota_record* out, tmpnn_stream stream);

/* ======================================================================================================
 * Benchmark preprocessing (trackmpnn_amd.evalprep.EvalPrep; csrc/evalprep.hip): what the KITTI benchmark does to a set of tracks
 * before it scores one class (TrackEval, datasets/kitti_2d_box.py:get_preprocessed_seq_data) -- per frame one assignment of the
 * class's tracker rows to the GT rows of the class and its distractors by the similarity of tmpnn_hota (entries below 0.5 - eps
 * are 0, a pair is matched iff its score exceeds eps); a row matched to a distractor or to an occluded / truncated object is
 * removed, and so is an unmatched row whose float32 height is <= height_thr or whose intersection with an ignore region exceeds
 * 0.5 + eps of its own area.  The rule is trackmpnn_amd.evalprep.evalprep_frame_host; tracks_out and the counts equal it exactly.
 *
 * The store holds what does not change between calls, packed over the sequences (all device memory, built by
 * trackmpnn_amd.evalprep.EvalPrepStore): both sides' rows sorted stably by frame, EVERY row kept,
 *     seq      [S][8] int64    gt_base, n_gt, det_base, n_det, off_base, n_frames of a sequence, two reserved words
 *     gt_off   [n_off] int32   per sequence n_frames + 1 offsets over the union frame range, relative to gt_base; det_off likewise
 *     gt_code  [n_gt] uint8    the rules resolved by the host: 0 the row takes no part, 1 of the class and scored, 2 of the class
 *                              but occluded or truncated, 3 a distractor, 4 an ignore region
 *     det_code [n_det] uint8   1 iff the row's category is the class (sorted order)
 *     gt_box   [n_gt][4], det_box [n_det][4] float32  x1 y1 x2 y2 (16-byte aligned)
 *     det_perm [n_det] int32   sorted position -> arrival index of a detection, relative to det_base
 * tracks [n_det] int32: y_out[:, 1] of every sequence in ARRIVAL order at its det_base; negative = no track.
 * ====================================================================================================== */
typedef struct tmpnn_evalprep_store {
    int32_t S, reserved;
    int64_t n_gt, n_det, n_off; /* totals over the sequences: the lengths of the arrays below */
    double height_thr;          /* min_height + eps, formed by the host */
    const int64_t* seq;
    const int32_t* gt_off;
    const int32_t* det_off;
    const uint8_t* gt_code;
    const uint8_t* det_code;
    const float* gt_box;
    const float* det_box;
    const int32_t* det_perm;
} tmpnn_evalprep_store;
/* One per sequence.  count: rows_in (rows with a track), other_class, removed_distractor, removed_occluded, removed_small,
 * removed_ignored, kept -- the last six sum to the first.  flag: 0, or in its low byte 1 = a frame with more than
 * tmpnn_evalprep_max_per_frame() detection rows or GT rows (all categories), 4 = the store is inconsistent (an offset or a
 * permutation entry out of range: nothing was read outside the arrays), 8 = the solver found no augmenting path; above it
 * (flag >> 8) the 1-based index of the frame in the sequence's range.  A flagged sequence's counts and tracks_out are not to be
 * used. */
typedef struct tmpnn_evalprep_record {
    int64_t count[7];
    int64_t flag;
} tmpnn_evalprep_record;
int tmpnn_evalprep_max_per_frame(void);
/* out [S]; tracks_out [n_det] int32 (not `tracks`): the ids after the preprocessing, arrival order, every sequence at its
 * det_base, -1 where the row had no track, another class, or was removed.  seq_host: the HOST copy of st->seq, checked against
 * the totals before the launch (the kernel checks the device copy again, and every offset it indexes by).  One clear of the
 * records and one launch, whatever S: parallel over sequences and frames, a wave per frame, integer atomics for the counts.  No
 * workspace. */
int tmpnn_evalprep(const tmpnn_evalprep_store* st, const int64_t* seq_host, const int32_t* tracks, int32_t* tracks_out,
                   tmpnn_evalprep_record* out, tmpnn_stream stream);

/* ======================================================================================================
 * Tracking results (trackmpnn_amd.results.TrackResults; csrc/results.hip): the last step of the reference's inference
 * (infer.py:91-96; dataset/kitti_mot.py:21-73, dataset/bdd100k_mot.py:22-67) -- a track whose category (the largest category id
 * over its rows) has a threshold and whose best detection score is below it is removed as a whole, and the kept rows are put
 * in frame order for the result table.  The rule is trackmpnn_amd.results.results_host; ids, order and counts equal it exactly.
 *
 * The store holds what does not change between calls, packed over the sequences (all device memory, built by
 * trackmpnn_amd.results.ResultStore):
 *     seq      [S][8] int64    tab_base, n_tab, det_base, n_det, off_base, n_frames of a sequence, two reserved words;
 *                              n_tab: the slots of its track table in the workspace, a power of two >= 2 n_det (0 without rows)
 *     det_off  [n_off] int32   per sequence n_frames + 1 offsets of its frames over the sorted positions, relative to det_base
 *     det_perm [n_det] int32   sorted position (stable by frame) -> arrival index, relative to det_base
 *     det_fidx [n_det] int32   frame index (frame - first frame) of a sorted position
 *     det_cat  [n_det] int32   category ids in arrival order, 0 <= id < n_cat
 *     det_key  [n_det] uint32  the scores in arrival order as integers of the same order (trackmpnn_amd.results.score_keys)
 *     thr_key  [n_cat] uint32  per category id the key of the threshold, 0 = none
 * tracks [n_det] int32: y_out[:, 1] of every sequence in ARRIVAL order at its det_base; -1 = no track.
 * ====================================================================================================== */
typedef struct tmpnn_result_store {
    int32_t S, n_cat;
    int64_t n_det, n_off, n_tab; /* totals over the sequences: the lengths of the arrays below and of the tables */
    const int64_t* seq;
    const int32_t* det_off;
    const int32_t* det_perm;
    const int32_t* det_fidx;
    const int32_t* det_cat;
    const uint32_t* det_key;
    const uint32_t* thr_key;
} tmpnn_result_store;
/* One per sequence.  kept_rows: rows whose filtered id is not -1 (the length of the sequence's part of `order`); removed_rows:
 * rows of removed tracks.  flag: 0, or in its low byte 2 = a kept id twice in a frame (flag >> 8: the 1-based index of the first
 * such frame in the sequence's range), 4 = the store is inconsistent (an offset, a permutation entry, a category or a table size
 * out of range: nothing was read outside the arrays), 16 = an id below -1. */
typedef struct tmpnn_result_record {
    int64_t kept_rows, kept_tracks, removed_rows, removed_tracks;
    int64_t flag;
    int64_t reserved[3];
} tmpnn_result_record;
/* bytes: the track tables (four words a slot, cleared by every call), the flag words, the slot of every row.  0 when an argument
 * is negative, S > 65535, n_det >= 2^31 or n_tab >= 2^34. */
size_t tmpnn_results_ws(int S, int64_t n_det, int64_t n_tab);
/* out [S]; filtered [n_det] int32: the ids after the filter, arrival order, every sequence at its det_base; order [n_det] int32:
 * at a sequence's det_base the arrival indices (relative to det_base) of its kept rows sorted stably by frame, -1 behind them.
 * seq_host: the HOST copy of st->seq, checked before the launches (the kernels check the device copy again, and every index).
 * One clear of the workspace's head and four launches, whatever S: the grouping of rows by id with the per-track integer maxima
 * (a thread per row, integer CAS / max), the filter (a thread per row), the duplicate check (a thread per sorted position), the
 * compaction and the counts (one workgroup per sequence).  ws: 16-byte aligned, tmpnn_results_ws bytes; its contents need not
 * survive between calls.  No float arithmetic and no float atomic: the output does not depend on the order of execution. */
int tmpnn_results_apply(const tmpnn_result_store* st, const int64_t* seq_host, const int32_t* tracks, void* ws, size_t ws_bytes,
                        tmpnn_result_record* out, int32_t* filtered, int32_t* order, tmpnn_stream stream);

/* ======================================================================================================
 * Validation mAP (trackmpnn_amd.mapeval.MapEvaluator): the mean average precision of the detections that were given a track,
 * over S sequences, in two launches (csrc/mapeval.hip) -- what the reference's validation pass computes on the host
 * (utils/metrics.py:93-229, train.py:272-273,286).  The rule is trackmpnn_amd.mapeval.map_host; counts are equal to it, ap bit
 * for bit.
 *
 * The store holds what does not change between evaluations (all device memory, built by trackmpnn_amd.mapeval.MapStore).  GT rows
 * are sorted stably by (class, sequence, frame); a GROUP is the GT rows of one (sequence, frame, class), a range of that order;
 * detections stay in arrival order, packed over the sequences.
 *     gt_box     [n_gt][4] float32  x1 y1 x2 y2 (16-byte aligned)     gt_seq [n_gt] int32  the row's sequence
 *     cls_gt_off [C + 1] int32      the GT rows of a class
 *     grp_off    [n_grp + 1] int32  the GT rows of a group
 *     det_box    [n_det][4] float32 (16-byte aligned)
 *     det_grp    [n_det] int32      the group of the detection's (sequence, frame, class), -1: there is none
 *     det_best   [n_det] int32      what tmpnn_map_best wrote
 *     cls_off    [C + 1] int32, order [n_live] int32   per class its detections in frames that have GT rows, by descending
 *                                   score, ties by (sequence, arrival index)
 *     claim_off  [n_gt + 1] int32, claim_det [n_claim] int32   per GT row the detections with det_best == row, arrival order
 * tracks [n_det] int32: y_out[:, 1] of every sequence in arrival order, negative = no track (a sequence that takes no part: all
 * negative); part [S] int32: 1 where the sequence takes part (its GT rows count), else 0.
 * ====================================================================================================== */
typedef struct tmpnn_map_store {
    int32_t S, C;
    int64_t n_gt, n_det, n_grp, n_live, n_claim; /* the lengths of the arrays below; all < 2^31 */
    const float* gt_box;
    const int32_t* gt_seq;
    const int32_t* cls_gt_off;
    const int32_t* grp_off;
    const float* det_box;
    const int32_t* det_grp;
    const int32_t* det_best;
    const int32_t* cls_off;
    const int32_t* order;
    const int32_t* claim_off;
    const int32_t* claim_det;
} tmpnn_map_store;
/* One per class.  annotations: the class's GT rows over the sequences that take part (0: the class is not one of this
 * evaluation); kept: its kept detections in frames with GT rows; flag: 0, or 1 = the store is inconsistent (an offset or an
 * index out of range: nothing was read outside the arrays; ap is 0 then). */
typedef struct tmpnn_map_record {
    double ap;
    int64_t annotations, kept, true_positives, flag;
} tmpnn_map_record;
/* entries of a class's sorted list that one step of the sweeps takes (the carries cross at its multiples) */
int tmpnn_map_tile(void);
/* best [n_det]: per detection the index (in the store's GT order) of the GT row of its group with the largest IoU in the
 * "+1" form of utils/misc.py:4-22, float64 from the float32 boxes, the FIRST maximum (a NaN counts as the maximum, as in
 * np.argmax); -1 where det_grp is -1, where the maximum is below 0.5 or NaN; -2 where det_grp or the group's offsets are out of
 * range.  Equal to trackmpnn_amd.mapeval.map_best_host per group.  Reads gt_box, grp_off, det_box, det_grp only. */
int tmpnn_map_best(const tmpnn_map_store* st, int32_t* best, tmpnn_stream stream);
/* bytes: the true-positive marks, the status of the claim lists, tp_k and the precision / envelope of every list entry */
size_t tmpnn_map_eval_ws(int64_t n_gt, int64_t n_det, int64_t n_live);
/* Two launches (one thread per GT row: the first kept claimant; one workgroup per class: three tiled sweeps of its sorted
 * list), out [C].  ws: 16-byte aligned, tmpnn_map_eval_ws bytes; its contents need not survive between calls. */
int tmpnn_map_eval(const tmpnn_map_store* st, const int32_t* tracks, const int32_t* part, void* ws, size_t ws_bytes,
                   tmpnn_map_record* out, tmpnn_stream stream);

/* ======================================================================================================
 * GT track ids for detections (trackmpnn_amd.labeling.DetectionLabeler; csrc/labeldet.hip) -- the reference's get_track_ids
 * (dataset/kitti_mot.py:422-486, dataset/bdd100k_mot.py:407-470) over all frames of S sequences at once: the greedy matching
 * of a frame's detections to its GT boxes in descending float32 "+1" IoU (equal categories, IoU >= iou_thresh; equal IoUs by
 * ascending flat index p * G' + g over the matchable rows), then the removal of unassigned detections whose largest IoM over
 * the iom_ignore_cat boxes is >= iom_thresh or whose largest IoU over the iou_ignore_cat boxes is >= iou_thresh (a NaN among
 * them keeps the detection).  The rule is trackmpnn_amd.labeling.label_frame_host; every output equals it exactly.
 *
 * The store (all device memory): both sides sorted stably by (sequence, frame), packed over the sequences; frame f of sequence
 * s is the global frame seq_base[s] + f, its detections det_first[.] .. det_first[. + 1], its GT rows gt_first likewise.
 *     seq_base     [S + 1] int32          det_first, gt_first [n_frames + 1] int32
 *     small_frames [n_small] int32        the global frames with at most tmpnn_label_wave_frame() rows on either side (one wave
 *     big_frames   [n_big] int32          labels such a frame), and the others (one workgroup); every frame in exactly one list
 *     det_frame, det_cat [n_det] int32    det_box [n_det][4] float32 x1 y1 x2 y2 (16-byte aligned)   det_score [n_det] float32
 *     gt_frame, gt_track, gt_cat [n_gt] int32    gt_box [n_gt][4] float32 (16-byte aligned); det_frame / gt_frame: the frame
 *                                         within the sequence, only handed on to the packed rows
 * At most tmpnn_label_max_per_frame() detections and GT rows (ignore rows included) in a frame.
 * ====================================================================================================== */
typedef struct tmpnn_label_store {
    int32_t S, reserved;
    int64_t n_frames, n_det, n_gt; /* totals over the sequences; all < 2^31 - 1 */
    int32_t iom_ignore_cat, iou_ignore_cat;
    float iou_thresh, iom_thresh;
    int64_t n_small, n_big; /* n_small + n_big == n_frames */
    const int32_t* seq_base;
    const int32_t* det_first;
    const int32_t* gt_first;
    const int32_t* small_frames;
    const int32_t* big_frames;
    const int32_t* det_frame;
    const int32_t* det_cat;
    const float* det_box;
    const float* det_score;
    const int32_t* gt_frame;
    const int32_t* gt_track;
    const int32_t* gt_cat;
    const float* gt_box;
} tmpnn_label_store;
/* flag: 0, or 1 = a frame with more than tmpnn_label_max_per_frame() detections or GT rows, 2 = the store is inconsistent (an
 * offset or a frame index out of range, a frame in neither list: nothing was read or written outside the arrays); frame: the
 * first global frame with a flag, else -1; kept_det, kept_gt: the rows packed (a flagged frame packs none). */
typedef struct tmpnn_label_record {
    int64_t flag, frame, kept_det, kept_gt;
} tmpnn_label_record;
/* What the two entry points write (all device memory, the caller's):
 *     track [n_det] int32 (-1: not assigned)   keep [n_det] u8   gt_keep [n_gt] u8       tmpnn_label_dets
 *     det_cnt, gt_cnt [n_frames] int32  the kept rows of a frame   fflag [n_frames] u8   tmpnn_label_dets (_compact zeroes the
 *                                                                                        counts of a flagged frame)
 *     det_off, gt_off [n_frames + 1] int32    where a frame's kept rows start in the packed arrays    tmpnn_label_compact
 *     seq_det_off, seq_gt_off [S + 1] int32   the same per sequence
 *     o_det_frame, o_det_track, o_det_cat [n_det] int32, o_det_box [n_det][4] (16-byte aligned), o_det_score [n_det]: the kept
 *     detections, packed, in the store's order; o_gt_frame, o_gt_track, o_gt_cat [n_gt], o_gt_box [n_gt][4]: the kept GT rows */
typedef struct tmpnn_label_out {
    tmpnn_label_record* record; /* 8-byte aligned */
    int32_t* track;
    uint8_t* keep;
    uint8_t* gt_keep;
    int32_t* det_cnt;
    int32_t* gt_cnt;
    uint8_t* fflag;
    int32_t* det_off;
    int32_t* gt_off;
    int32_t* seq_det_off;
    int32_t* seq_gt_off;
    int32_t* o_det_frame;
    int32_t* o_det_track;
    int32_t* o_det_cat;
    float* o_det_box;
    float* o_det_score;
    int32_t* o_gt_frame;
    int32_t* o_gt_track;
    int32_t* o_gt_cat;
    float* o_gt_box;
} tmpnn_label_out;
int tmpnn_label_max_per_frame(void);
int tmpnn_label_wave_frame(void);
/* At most two launches (the wave frames, the workgroup frames): track, keep, gt_keep, det_cnt, gt_cnt, fflag. */
int tmpnn_label_dets(const tmpnn_label_store* st, const tmpnn_label_out* out, tmpnn_stream stream);
/* Two launches after tmpnn_label_dets on the same stream (one workgroup scans the per-frame counts and writes the record; one
 * wave per frame packs the kept rows): everything else of tmpnn_label_out. */
int tmpnn_label_compact(const tmpnn_label_store* st, const tmpnn_label_out* out, tmpnn_stream stream);

/* ======================================================================================================
 * The visual head (csrc/vishead.hip; host definition: trackmpnn_amd.vishead.vis_head_host): the embedding CNN's map read at each
 * box centre (reference dataset/kitti_mot.py:391-412), the softmax rows that are the 128 'vis' feature columns (:563-566) and the
 * identity loss over the same rows (models/loss.py:162-181), per chunk, with its gradient wrt the maps.
 *   centre   cx = trunc(((x1 + x2) / 2) * input_w / im_w / down_ratio), cy likewise with y, input_h, im_h: every operation one
 *            correctly rounded float32 operation in this order; clamped to the map (flag bit 0, counted)
 *   logits   maps[map_of][c][cy][cx], c < 128;  rows[d][col + c] = (softmax(logits)[c] - mean[c]) / std[c]
 *   loss[b]  mean over the rows d of chunk b (offsets[b] <= d < offsets[b + 1]) with track[d] >= 0 of
 *            logsumexp(logits[d]) - logits[d][track[d] % 128]; 0 for a chunk without such a row
 *   dmaps    += g[b] / n_b * (softmax - onehot) at the row's pixel, for every labelled row; rows sharing a pixel are summed in
 *            ascending row order by the lowest of them, which stores once: no atomics, bitwise reproducible
 * A map_of outside [0, T) reads map 0 and sets flag bit 1; chunk boundaries that are not non-decreasing within [0, D] are
 * clamped and counted: nothing is read or written outside the arrays, and the caller raises when it reads the counts.
 * ====================================================================================================== */
typedef struct {
    int32_t T, Hm, Wm;          /* maps [T][128][Hm][Wm], T * Hm * Wm < 2^31 */
    int32_t B;                  /* chunks (>= 1) */
    int64_t D;                  /* detections, <= 131 072 (the backward's scan is D / 64 steps a row) */
    float input_h, input_w, down_ratio;
    float im_h, im_w;           /* the image size of every row when im_hw is NULL */
    int32_t ld_rows, col;       /* row stride of `rows` in floats, first column written (col + 128 <= ld_rows) */
    int32_t reserved;
    const float* maps;
    const float* box;           /* [D][4] x1 y1 x2 y2 */
    const int32_t* map_of;      /* [D] */
    const float* im_hw;         /* [D][2] (h, w), or NULL */
    const int32_t* track;       /* [D], -1: no label; NULL: no row is labelled (inference) */
    const int32_t* offsets;     /* [B + 1], or NULL with B = 1: one chunk of all rows */
    const float* mean;          /* [128] */
    const float* std;           /* [128] */
    float* rows;                /* [D][ld_rows] */
    float* logits;              /* [D][128] */
    float* stat;                /* [D][2]: the row's maximum and the sum of exp(logit - maximum) */
    float* nll;                 /* [D]: logsumexp - logit[track % 128]; 0 for a row without label */
    int32_t* pix;               /* [D]: (map * Hm + cy) * Wm + cx */
    int32_t* flag;              /* [D]: bit 0 centre clamped, bit 1 map_of out of range */
    int32_t* chunk_of;          /* [D]: the row's chunk, -1: in none */
    int32_t* key;               /* [D]: pix of a labelled row of a chunk, -1 otherwise: equal keys share a pixel of dmaps */
    float* loss;                /* [B] */
    int32_t* count;             /* [B][4]: labelled rows, clamped rows, bad rows + bad boundaries, rows */
} tmpnn_vis_head;
/* Two launches (one wave per detection; one wave per chunk, a fixed-order reduction): everything from `rows` on. */
int tmpnn_vis_head_fwd(const tmpnn_vis_head* a, tmpnn_stream stream);
/* After tmpnn_vis_head_fwd on the same stream, with the same struct: a memset of dmaps [T][128][Hm][Wm] and one launch (one wave
 * per detection; a pairwise scan of the saved pixels finds the sharers).  g [B]: the gradient arriving at loss. */
int tmpnn_vis_head_bwd(const tmpnn_vis_head* a, const float* g, float* dmaps, tmpnn_stream stream);
/* After tmpnn_vis_head_fwd on the same stream, with the same struct: a memset of dmaps and one launch that adds a gradient handed
 * in, d_logits [D][128], at the pixels the forward saved (the backward of the gather alone, for a loss computed outside over
 * `logits`: tmpnn_embed_loss_*).  Rows with a label in a chunk are added; rows that share a pixel are summed in ascending row
 * order by the lowest of them, which stores once (the ownership scan of tmpnn_vis_head_bwd): no atomics. */
int tmpnn_vis_head_scatter(const tmpnn_vis_head* a, const float* d_logits, float* dmaps, tmpnn_stream stream);
/* The head behind a CNN that answers per pixel (tmpnn_espnet_centres), for inference: `maps` may be NULL, track and offsets are
 * NULL and B = 1.  tmpnn_vis_head_pixels (one launch) writes pix and flag of every row by the centre rule above;
 * tmpnn_vis_head_rows_from_logits (one launch, one wave per row and one for the counts) then reads `logits` [D][128] -- filled
 * by the caller for the pixels in pix -- and writes everything else tmpnn_vis_head_fwd writes, by the same arithmetic: rows
 * from equal logits are equal bit for bit. */
int tmpnn_vis_head_pixels(const tmpnn_vis_head* a, tmpnn_stream stream);
int tmpnn_vis_head_rows_from_logits(const tmpnn_vis_head* a, tmpnn_stream stream);

/* ======================================================================================================
 * The embedding loss (csrc/embedloss.hip; host definition: trackmpnn_amd.embedloss.embedding_loss_host): the reference's
 * discriminative pull-push loss over embedding rows (models/loss.py:118-159), per chunk, with its gradient wrt the rows.
 *   cluster  the rows of chunk b (offsets[b] <= i < offsets[b + 1]) with track[i] >= 0 that share one track id (compared as
 *            integers); C clusters, n_c rows, mu_c their mean (rows added in ascending order)
 *   terms    var = (1 / C) sum_c (1 / n_c) sum_{i in c} relu(|x_i - mu_c| - delta_var)^2                      (0 when C = 0)
 *            dist = (1 / (C (C - 1))) sum_{c != c'} relu(delta_dist - |mu_c - mu_c'|)^2, ordered pairs        (0 when C <= 1)
 *   loss[b]  var + dist
 *   d_features[k] = g[b] (u_k - (1 / n_c) sum_{i in c} u_i + v_c / n_c) for a row k of cluster c, 0 for every other row, with
 *            u_i = 2 relu(d_i - delta_var) (x_i - mu_c) / (d_i C n_c), d_i = |x_i - mu_c|, and
 *            v_c = -(4 / (C (C - 1))) sum_{c' != c} relu(delta_dist - m) (mu_c - mu_c') / m, m = |mu_c - mu_c'|;
 *            where a norm is exactly 0 its direction term is 0
 * No atomics: every sum has one owner and a fixed order, so the results are bitwise reproducible.  No limit on the rows or the
 * clusters of a chunk (a wave per row scans its chunk's ids 64 at a time).  Chunk boundaries that are not non-decreasing within
 * [0, D] are clamped and counted, and a row then belongs to the first chunk that holds it: nothing is read or written outside
 * the arrays, and the caller raises when it reads the counts.
 * ====================================================================================================== */
typedef struct tmpnn_embed_loss {
    int64_t D;                  /* rows, <= 131 072 */
    int32_t B;                  /* chunks (>= 1) */
    int32_t W;                  /* columns of a row, 1 .. 1024 */
    int32_t ld;                 /* row stride of features and of d_features in floats, >= W */
    float delta_var, delta_dist;
    int32_t reserved;
    const float* features;      /* [D][ld] */
    const int32_t* track;       /* [D], -1: no label */
    const int32_t* offsets;     /* [B + 1], or NULL with B = 1: one chunk of all rows */
    void* ws;                   /* tmpnn_embed_loss_ws(D, W) bytes, 16-byte aligned; the forward's results for the backward */
    size_t ws_bytes;
    float* loss;                /* [B] */
    float* terms;               /* [B][2]: var, dist */
    int32_t* count;             /* [B][4]: labelled rows, clusters, bad boundaries, rows */
} tmpnn_embed_loss;
size_t tmpnn_embed_loss_ws(int64_t D, int W);
/* Four launches (the rows' chunks; leaders and means; distances and leader pairs; one wave per chunk): loss, terms, count. */
int tmpnn_embed_loss_fwd(const tmpnn_embed_loss* a, tmpnn_stream stream);
/* After tmpnn_embed_loss_fwd on the same stream, with the same struct: two launches.  g [B]: the gradient arriving at loss;
 * columns 0 .. W - 1 of every row of d_features [D][ld] are written. */
int tmpnn_embed_loss_bwd(const tmpnn_embed_loss* a, const float* g, float* d_features, tmpnn_stream stream);

/* ======================================================================================================
 * Wide cells (H = 128 / 256, diff messages; BASELINE.json C5) as LDS-tiled GEMMs on bf16x6 split products
 * (csrc/wide.hip).  Same arithmetic contract as the H <= 64 kernels: fp32 in / out, fp32 accumulate, error no larger
 * than the f32 MFMA chain.  tmpnn_wide_prepare splits the cell's two weight matrices into their MFMA operand images
 * once per optimizer step (prep: tmpnn_wide_prep_bytes bytes, 16-byte aligned).
 * ====================================================================================================== */
int tmpnn_wide_supported(int H, int IN);
size_t tmpnn_wide_prep_bytes(int H, int IN);
int tmpnn_wide_prepare(const float* w_ih /* [3H][IN] */, const float* w_hh /* [3H][H] */, int IN, int H, void* prep,
                       tmpnn_stream stream);
/* Forward of one cell over the rows `rows[R]` with the diff message taken through the projected det rows (rows E + H'
 * + I): P [Dn][3H] = h[det_rows] W_ih^T is written here; gi = P[src_pos[r]] - P[dst_pos[r]] (det INDICES),
 * gh = h[rows[r]] W_hh^T, h_out[rows[r]] = GRUCell; gates: NULL or the 4 planes of tmpnn_gru_fwd. */
int tmpnn_wide_gru_fwd(const void* prep, const int32_t* det_rows, int Dn, const int32_t* rows, int R,
                       const int32_t* src_pos, const int32_t* dst_pos, const float* h, int ld_h, int H,
                       const float* b_ih, const float* b_hh, float* P, float* h_out, int ld_out, float* gates,
                       size_t gate_plane, tmpnn_stream stream);
/* The same forward over edge tiles (rows_per_tile = 128; tiles cover the graph's R edge rows): P rows of a tile's det
 * list are staged in LDS once per tile and hidden chunk instead of gathered per edge row; bit-identical results. */
int tmpnn_wide_gru_fwd_tiled(const void* prep, const int32_t* det_rows, int Dn, const tmpnn_edge_tiles* tiles, int R,
                             const float* h, int ld_h, int H, const float* b_ih, const float* b_hh, float* P,
                             float* h_out, int ld_out, float* gates, size_t gate_plane, tmpnn_stream stream);
/* Data gradient (as tmpnn_gru_bwd_data with IN = H, no fused adjoint): d_msg[rows[r]][0:H] = d_gi W_ih,
 * d_h[rows[r]] = dh z + d_gh W_hh.  ws: tmpnn_wide_gru_bwd_data_ws(R, H) bytes (the materialised d_gi, d_gh). */

/* Weight gradient of the same cell from the gate gradients tmpnn_wide_gru_bwd_data left in ITS workspace (`dg_ws`, read
 * only): dW_ih += d_gi^T (h[src] - h[dst]), dW_hh += d_gh^T h[rows], db_ih / db_hh += column sums (replaces
 * tmpnn_gru_bwd_weights for the wide cells: layers.py:84-116 backward).  ws: tmpnn_wide_gru_bwd_weights_ws(R, H) bytes. */

/* The whole backward of a wide EDGE cell under the diff message x[e] = h[src e] - h[dst e] (models/layers.py:90-95, 107),
 * with both W_ih products taken on the det side by linearity -- the backward twin of the forward's projected det rows:
 *     S[d] = sum_{e: src = d} d_gi[e] - sum_{e: dst = d} d_gi[e]
 *     d_h[det_row[d]] += S[d] W_ih                 (the message adjoint: replaces d_x = d_gi W_ih + tmpnn_gather_diff_bwd)
 *     dW_ih += S^T h[det rows]                     (replaces d_gi^T (h[src] - h[dst]) over the E edge rows)
 * and, over the edge rows, d_h[edge_row[e]] = dh z + d_gh W_hh (plain store), dW_hh += d_gh^T h, db_ih / db_hh += column
 * sums.  The gate gradients are materialised once as [N][4H] = [dr | dz | dn | dn r] indexed by graph row.
 * Replaces tmpnn_wide_gru_bwd_data + tmpnn_wide_gru_bwd_weights + tmpnn_gather_diff_bwd for this cell: two of the four
 * (E x 3H x H) products run over Dn rows.  ws: tmpnn_wide_gru_bwd_diff_ws(N, E, Dn, H) bytes. */
size_t tmpnn_wide_gru_bwd_diff_ws(int N, int E, int Dn, int H);
int tmpnn_wide_gru_bwd_diff(const void* prep, const tmpnn_graph* g, const float* h, int ld_h, int H, const float* gates,
                            size_t gate_plane, const float* d_hout, int ld_dhout, const float* dy, const float* w_head,
                            float* d_h, int ld_dh, float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, void* ws,
                            size_t ws_bytes, tmpnn_stream stream);
/* The same call with the det-side branch (the signed segment sums of d_gi and the message adjoint) enqueued on a SECOND
 * stream next to the two E-row matrix kernels: forked from `stream` after the gate gradients, joined before the det-side
 * weight gradient, so `stream` order alone still covers every output.  Results are bit-identical to tmpnn_wide_gru_bwd_diff.
 * aux_stream must differ from stream; do not use while `stream` is being captured into a graph.  ev_fork / ev_join: two
 * events of the caller (hipEventDisableTiming is enough) that the call records and waits on -- the library creates, destroys
 * and synchronises nothing; on return (also with an error code) `stream` waits for everything enqueued on aux_stream. */
/* ... and with the adjoint of row F (models/layers.py:103: d_h[e] += add_msg[src[e]] - add_msg[dst[e]], what
 * tmpnn_gather_diff_fwd(g, add_msg, ld_add, d_h, ld_dh, H, accumulate = 1) would add afterwards) taken in the epilogue of the
 * E-row product: one read-modify-write pass over d_h's edge rows less.  add_msg: the table whose det rows hold d_es (>= H
 * columns); aux_stream may be NULL (one stream; the events are then unused).  Bit-identical to the two calls. */
int tmpnn_wide_gru_bwd_diff_fused(const void* prep, const tmpnn_graph* g, const float* h, int ld_h, int H, const float* gates,
                                  size_t gate_plane, const float* d_hout, int ld_dhout, const float* dy, const float* w_head,
                                  float* d_h, int ld_dh, float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, void* ws,
                                  size_t ws_bytes, const float* add_msg, int ld_add, tmpnn_stream stream,
                                  tmpnn_stream aux_stream, tmpnn_event ev_fork, tmpnn_event ev_join);

/* ======================================================================================================
 * The embedding CNN (csrc/espnet.hip; host definition: trackmpnn_amd.espnet.espnet_host): the reference's ESPNetv2
 * segmentation net EESPNet_Seg(classes = C, s = 1) (models/espv2) in eval mode.  images [T][3][H][W] float32 ->
 * out [T][C][H][W] float32, both contiguous NCHW; H and W positive multiples of 16.  Every BatchNorm uses its running
 * statistics, folded by the caller into a per-channel scale and shift; both Dropout2d are the identity.  No atomics: results
 * are bitwise reproducible, and image i of a batch gives the same bits for every T.
 *
 * The weight arena is one array of float32.  It is a sequence of segments, each padded with zeros to a multiple of 4 floats,
 * in this order (a "norm" is scale [c] | shift [c]; slopes are the per-channel PReLU weights):
 *   level1      W [32][3][3][3] | scale [32] | shift [32] | slope [32]
 *   DOWN(level2_0: 32 -> 64)  DOWN(level3_0: 64 -> 128)  3 x EESP(level3: 128 -> 128)
 *   DOWN(level4_0: 128 -> 256)  7 x EESP(level4: 256 -> 256)
 *   PW(proj_L4_C: 256 -> 128)   EESP(pspMod.0: 256 -> 128)
 *   4 x W [128][9] (pspMod.1.stages)   PW(pspMod.1.project: 640 -> 128)
 *   PW(project_l3: 128 -> C; the norm and slopes of act_l3)   PW(project_l2: 64 + C -> C)   PW(project_l1: 32 + C -> C)
 * with
 *   PW(cin -> cout, groups g)   Wt [cin / g][cout] (the conv weight [cout][cin / g] transposed) | scale [cout] | shift [cout] |
 *                               slope [cout]; without a norm scale = 1, shift = 0; without an activation slope = 1
 *   EESP(nin -> nout), n = nout / 4
 *                               PW(proj_1x1: nin -> n, g = 4) | W [4][n][9] (spp_dw.0 .. 3) | scale [nout] | shift [nout] |
 *                               slope [nout] (br_after_cat) | PW(conv_1x1_exp: nout -> nout, g = 4; slopes: module_act, or
 *                               in a DOWN the block's act from channel nin on)
 *   DOWN(nin -> nout)           W [3][3][3][3] | scale [3] | shift [3] | slope [3] (inp_reinf.0) | Wt [3][nout] | scale [nout] |
 *                               shift [nout] (inp_reinf.1) | slope [nin] (act, channels below nin) | EESP(eesp: nin -> nout - nin)
 * tmpnn_espnet_arena_floats(C) is the length of that array (0: C outside 1 .. 1024); tmpnn_espnet_ws_bytes the workspace of one
 * call (0: a shape tmpnn_espnet_fwd refuses).  tmpnn_espnet_fwd validates on the host before any launch (null pointers, H or W
 * not a multiple of 16, T outside 1 .. 65535, max(C, 160) H W >= 2^31, pointers not 16-byte aligned: TMPNN_EINVAL; a short
 * workspace: TMPNN_EWORKSPACE), then enqueues 70 launches on `stream`, whatever T is; nothing is allocated, copied or waited for.
 * ====================================================================================================== */
size_t tmpnn_espnet_arena_floats(int C);
size_t tmpnn_espnet_ws_bytes(int T, int H, int W, int C);
int tmpnn_espnet_fwd(const float* arena, int C, const float* images, int T, int H, int W, void* ws, size_t ws_bytes, float* out,
                     tmpnn_stream stream);
/* The same net answered at single pixels.  Everything behind the C-channel map at 1/8 size is pointwise convs and x2 resizes, so
 * one output pixel needs 2 x 2 pixels of the last merge, 3 x 3 of the one before and the taps of those at 1/8 size.
 *   tmpnn_espnet_centres_ws_bytes   the workspace without the four maps of the dense tail (0: a shape that is refused); the
 *                                   arrays of the trunk lie where they lie in the workspace of tmpnn_espnet_fwd
 *   tmpnn_espnet_trunk              the first 65 launches of tmpnn_espnet_fwd (the same host code), which leave the encoder
 *                                   outputs at 1/2 and 1/4 size and that 1/8 map in the workspace; the same checks
 *   tmpnn_espnet_centres            after the trunk on the same stream, with the same workspace: one launch, one workgroup per
 *                                   entry of pix [D] (pix = (t H + y) W + x, T H W < 2^31), logits [D][C] = what
 *                                   tmpnn_espnet_fwd leaves at out[t][.][y][x], bit for bit; flags [D] = 1 where pix lay
 *                                   outside [0, T H W) and was clamped into it, else 0.  1 <= C <= 256 (TMPNN_EINVAL names
 *                                   the dense call for wider nets); D = 0 launches nothing; no atomics. */
size_t tmpnn_espnet_centres_ws_bytes(int T, int H, int W, int C);
int tmpnn_espnet_trunk(const float* arena, int C, const float* images, int T, int H, int W, void* ws, size_t ws_bytes,
                       tmpnn_stream stream);
int tmpnn_espnet_centres(const float* arena, int C, int T, int H, int W, const void* ws, size_t ws_bytes, const int32_t* pix, int D,
                         float* logits, int32_t* flags, tmpnn_stream stream);
/* Training the decoder behind merge_l3 with everything in front of it frozen (csrc/espnet_train.hip; host definition:
 * trackmpnn_amd.espnet.espnet_decoder_grads_host).  The function differentiated is tmpnn_espnet_fwd's: running statistics, both
 * Dropout2d the identity (fine-tuning with frozen statistics).  Trained: 9 tensors, float32, in ONE flat parameter buffer without
 * padding, in the order of the state dict:
 *   project_l3.1.conv.weight [C][128] | act_l3.bn.weight [C] | act_l3.bn.bias [C] | act_l3.act.weight [C] |
 *   project_l2.conv.weight [C][64 + C] | project_l2.bn.weight [C] | project_l2.bn.bias [C] | project_l2.act.weight [C] |
 *   project_l1.1.conv.weight [C][32 + C]
 * `stats` holds the frozen statistics of the two norms: act_l3 running_mean [C] | running_var [C] | project_l2 running_mean [C] |
 * running_var [C].  `grads` has the parameter buffer's layout; the backward ADDS into it.
 *   tmpnn_espnet_train_param_floats  the length of the parameter buffer (0: C outside 1 .. 1024)
 *   tmpnn_espnet_train_table         rows [n][3] int64 for the first min(n, cap) tensors: (offset in the parameter buffer, element
 *                                    count, offset in the weight arena of the segment the tensor is folded into); returns n = 9
 *                                    (TMPNN_EINVAL < 0: C outside 1 .. 1024)
 *   tmpnn_espnet_train_ws_bytes      the workspace of tmpnn_espnet_train_fwd: tmpnn_espnet_fwd's, then what the backward needs kept
 *                                    (the pre-activations of act_l3 and project_l2); 0: a shape that is refused
 *   tmpnn_espnet_train_bwd_ws_bytes  the scratch of tmpnn_espnet_train_bwd (float64 partial sums included); 0 likewise
 *   tmpnn_espnet_refold              one launch: rewrites the arena segments of the three trained layers from params and stats
 *                                    (weights transposed, scale and shift folded in float64 and rounded once: the bits the host
 *                                    packing gives); nothing is copied through the host
 *   tmpnn_espnet_train_fwd           tmpnn_espnet_fwd's 70 launches (the same host code and kernels; the two trained layers that end
 *                                    in a PReLU also store the value in front of it); out has tmpnn_espnet_fwd's bits
 *   tmpnn_espnet_train_bwd           after tmpnn_espnet_train_fwd on the same workspace: d_out [T][C][H][W] -> grads, and, when
 *                                    d_l1 [T][32][H/2][W/2] and d_l2 [T][64][H/4][W/4] are given (both or neither), the gradients
 *                                    at the encoder taps out_l1 and out_l2 (overwritten).  13 launches whatever T is, no atomics,
 *                                    every sum in a fixed order: equal bits for equal inputs.  The same checks as tmpnn_espnet_fwd. */
size_t tmpnn_espnet_train_param_floats(int C);
int tmpnn_espnet_train_table(int C, int64_t* rows, int cap);
size_t tmpnn_espnet_train_ws_bytes(int T, int H, int W, int C);
size_t tmpnn_espnet_train_bwd_ws_bytes(int T, int H, int W, int C);
int tmpnn_espnet_refold(float* arena, int C, const float* params, const float* stats, tmpnn_stream stream);
int tmpnn_espnet_train_fwd(const float* arena, int C, const float* images, int T, int H, int W, void* ws, size_t ws_bytes, float* out,
                           tmpnn_stream stream);
int tmpnn_espnet_train_bwd(const float* arena, int C, const float* params, const float* stats, int T, int H, int W, const void* ws,
                           size_t ws_bytes, const float* d_out, void* bws, size_t bws_bytes, float* grads, float* d_l1, float* d_l2,
                           tmpnn_stream stream);
/* The same with the WHOLE decoder trained: proj_L4_C and pspMod as well, the encoder (every net.* tensor) still frozen.  Seven
 * siblings of the entry points above with the same arguments and checks; what differs:
 *   the parameter buffer     the 36 decoder tensors in state-dict order without padding:
 *                            proj_L4_C.conv.weight [128][256] | .bn.weight [128] | .bn.bias [128] | .act.weight [128] |
 *                            pspMod.0.proj_1x1.conv.weight [32][64] | .bn.weight [32] | .bn.bias [32] | .act.weight [32] |
 *                            pspMod.0.spp_dw.0 .. 3.conv.weight 4 x [32][9] | pspMod.0.conv_1x1_exp.conv.weight [128][32] | .bn.weight
 *                            [128] | .bn.bias [128] | pspMod.0.br_after_cat.bn.weight [128] | .bn.bias [128] | .act.weight [128] |
 *                            pspMod.0.module_act.weight [128] | pspMod.1.stages.0 .. 3.conv.weight 4 x [128][9] |
 *                            pspMod.1.project.conv.weight [128][640] | .bn.weight [128] | .bn.bias [128] | .act.weight [128] | the 9
 *                            tensors of the tail as above
 *   stats                    running_mean [c] | running_var [c] of the 7 norms in that order: proj_L4_C.bn (128), pspMod.0.proj_1x1.bn
 *                            (32), pspMod.0.conv_1x1_exp.bn (128), pspMod.0.br_after_cat.bn (128), pspMod.1.project.bn (128), act_l3.bn
 *                            (C), project_l2.bn (C)
 *   tmpnn_espnet_dec_table   returns n = 36; a grouped conv weight's segment is Wt [cin / g][cout], a depthwise weight's segment the
 *                            tensor as it lies, bn.weight's the folded scale, bn.bias's the folded shift, a slope's the slopes
 *   tmpnn_espnet_dec_ws_bytes      tmpnn_espnet_train_ws_bytes', then the pre-activations of proj_L4_C, pspMod.0.proj_1x1,
 *                            pspMod.0.conv_1x1_exp and pspMod.1.project and the four pooled maps of the PSP chain
 *   tmpnn_espnet_dec_refold  one launch over all 26 trained segments
 *   tmpnn_espnet_dec_fwd     tmpnn_espnet_fwd's 70 launches and bits; the PSP chain writes its four pooled maps to four places
 *   tmpnn_espnet_dec_bwd     48 launches whatever T is (the first 13 are tmpnn_espnet_train_bwd's, with the same bits for the tail's 9
 *                            tensors and for d_l1 and d_l2); d_l1, d_l2, d_l3 [T][128][H/8][W/8], d_l4 [T][256][H/16][W/16]: all
 *                            four or none (then 47 launches, and no parameter gradient changes a bit) */
size_t tmpnn_espnet_dec_param_floats(int C);
int tmpnn_espnet_dec_table(int C, int64_t* rows, int cap);
size_t tmpnn_espnet_dec_ws_bytes(int T, int H, int W, int C);
size_t tmpnn_espnet_dec_bwd_ws_bytes(int T, int H, int W, int C);
int tmpnn_espnet_dec_refold(float* arena, int C, const float* params, const float* stats, tmpnn_stream stream);
int tmpnn_espnet_dec_fwd(const float* arena, int C, const float* images, int T, int H, int W, void* ws, size_t ws_bytes, float* out,
                         tmpnn_stream stream);
int tmpnn_espnet_dec_bwd(const float* arena, int C, const float* params, const float* stats, int T, int H, int W, const void* ws,
                         size_t ws_bytes, const float* d_out, void* bws, size_t bws_bytes, float* grads, float* d_l1, float* d_l2,
                         float* d_l3, float* d_l4, tmpnn_stream stream);

/* ---- comparison builds only (-DTMPNN_KEEP_VARIANTS; tools/build_variant.sh) ------------------------------------------------
 * Superseded forms kept for A/B runs: the two-kernel backward of the wide cells (the shipped path takes both W_ih products on
 * the det side, tmpnn_wide_gru_bwd_diff*), its two-stream form, the explicit choice of the H = 64 weight-gradient kernel, the
 * block append without features.  The shipped libtmpnn.so does NOT export them. */
#ifdef TMPNN_KEEP_VARIANTS
int tmpnn_track_append(int N, int A, int D, const int32_t* active, const int32_t* new_ids, int t, const int32_t* track,
                       int32_t* ts, int32_t* det_id, int32_t* assoc, uint8_t* is_edge, int32_t* row_src,
                       int32_t* row_dst, uint8_t* labels, tmpnn_stream stream);
int tmpnn_gru_bwd_weights_variant(const int32_t* rows, int R, int xmode, const int32_t* src, const int32_t* dst,
                                  const float* msg, int ld_msg, int msg_compact, int IN,
                                  const float* h, int ld_h, int H,
                                  const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout,
                                  const float* dy, const float* w_head,
                                  float* dW_ih, float* dW_hh, float* db_ih, float* db_hh,
                                  void* ws, size_t ws_bytes, int variant, tmpnn_stream stream);
int tmpnn_gru_bwd_weights_choice(void);
int tmpnn_wide_gru_bwd_diff_aux(const void* prep, const tmpnn_graph* g, const float* h, int ld_h, int H, const float* gates,
                            size_t gate_plane, const float* d_hout, int ld_dhout, const float* dy, const float* w_head,
                            float* d_h, int ld_dh, float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, void* ws,
                            size_t ws_bytes, tmpnn_stream stream,
                                tmpnn_stream aux_stream, tmpnn_event ev_fork, tmpnn_event ev_join);
size_t tmpnn_wide_gru_bwd_data_ws(int R, int H);
int tmpnn_wide_gru_bwd_data(const void* prep, const int32_t* rows, int R, const float* h, int ld_h, int H,
                            const float* gates, size_t gate_plane, const float* d_hout, int ld_dhout, const float* dy,
                            const float* w_head, float* d_msg, int ld_dmsg, float* d_h, int ld_dh, void* ws,
                            size_t ws_bytes, tmpnn_stream stream);
size_t tmpnn_wide_gru_bwd_weights_ws(int R, int H);
int tmpnn_wide_gru_bwd_weights(const void* dg_ws, const int32_t* rows, int R, const int32_t* src, const int32_t* dst,
                               const float* h, int ld_h, int H, float* dW_ih, float* dW_hh, float* db_ih, float* db_hh,
                               void* ws, size_t ws_bytes, tmpnn_stream stream);
#endif

#ifdef __cplusplus
}
#endif
#endif /* TMPNN_H */
