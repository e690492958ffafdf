"""ctypes binding of libtmpnn.so (the C ABI declared in include/tmpnn.h).

The library is the product: there is NO fallback.  If the shared object is missing or a call
fails, a RuntimeError is raised -- nothing silently reroutes through torch ops or the oracle.
"""
from __future__ import annotations

import ctypes as C

import torch
import os
import re
from typing import Dict, List, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# TMPNN_LIB_PATH: load another build of the SAME library (kernel experiments of tools/build_variant.sh); never a fallback
LIB_PATH = os.environ.get('TMPNN_LIB_PATH') or os.path.join(_HERE, 'lib', 'libtmpnn.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'tmpnn.h')

ABI_VERSION = 13

c_int = C.c_int
c_void_p = C.c_void_p
c_size_t = C.c_size_t
c_float = C.c_float


class CSegPlan(C.Structure):
    """struct tmpnn_seg_plan (include/tmpnn.h): the single-read segment sum of a dense graph."""
    _fields_ = [('T', C.c_int32), ('I', C.c_int32), ('nsplit', C.c_int32), ('t_row', c_void_p), ('items', c_void_p),
                ('rowptr2', c_void_p), ('inc2', c_void_p), ('ws', c_void_p), ('ws_floats', c_size_t)]


class CWinPlan(C.Structure):
    """struct tmpnn_win_plan (include/tmpnn.h): the single-read segment sum of a batch of small windows."""
    _fields_ = [('W', C.c_int32), ('nbig', C.c_int32), ('wrec', c_void_p), ('erow', c_void_p), ('recs', c_void_p),
                ('det', c_void_p), ('drow', c_void_p), ('big_order', c_void_p)]


class CGraph(C.Structure):
    """struct tmpnn_graph (include/tmpnn.h)."""
    _fields_ = [('N', C.c_int32), ('E', C.c_int32), ('Dn', C.c_int32),
                ('src', c_void_p), ('dst', c_void_p), ('edge_row', c_void_p), ('det_row', c_void_p),
                ('rowptr', c_void_p), ('inc', c_void_p), ('det_order', c_void_p), ('seg_plan', c_void_p),
                ('win_plan', c_void_p)]


_GP = C.POINTER(CGraph)


class CZsGateSrc(C.Structure):
    """struct tmpnn_zs_gate_src (include/tmpnn.h): what tmpnn_gru_bwd_fused_zero_state forms r, z, n from when the forward
    saved no gate planes (passed by address as `gates`, with gate_plane = 0)."""
    _fields_ = [('proj', c_void_p), ('ld_proj', C.c_int32), ('src_pos', c_void_p), ('dst_pos', c_void_p),
                ('b_ih', c_void_p), ('b_hh', c_void_p)]


class CEdgeTiles(C.Structure):
    """struct tmpnn_edge_tiles (include/tmpnn.h)."""
    _fields_ = [('T', C.c_int32), ('rows_per_tile', C.c_int32), ('t_row', c_void_p), ('t_loc', c_void_p),
                ('t_dptr', c_void_p), ('t_dets', c_void_p)]


_TP = C.POINTER(CEdgeTiles)


class CDGraph(C.Structure):
    """struct tmpnn_dgraph (include/tmpnn.h): index-form graph whose sizes live on the device."""
    _fields_ = [('N', C.c_int32), ('cap', C.c_int32), ('meta', c_void_p), ('is_edge', c_void_p), ('pos', c_void_p),
                ('src', c_void_p), ('dst', c_void_p), ('src_pos', c_void_p), ('dst_pos', c_void_p),
                ('edge_row', c_void_p), ('det_row', c_void_p), ('rowptr', c_void_p), ('inc', c_void_p)]


_P3 = c_void_p * 3


class CMpParams(C.Structure):
    """struct tmpnn_mp_params (include/tmpnn.h): every parameter (or its gradient buffer) as a device pointer."""
    _fields_ = [('G', C.c_int32), ('H', C.c_int32), ('IN_e', C.c_int32), ('F_total', C.c_int32), ('F', C.c_int32 * 3),
                ('w1', _P3), ('b1', _P3), ('gamma', _P3), ('beta', _P3), ('w2', _P3), ('b2', _P3),
                ('run_mean', _P3), ('run_var', _P3), ('num_batches_tracked', _P3),
                ('e_wih', _P3), ('e_whh', _P3), ('e_bih', _P3), ('e_bhh', _P3),
                ('n_wih', _P3), ('n_whh', _P3), ('n_bih', _P3), ('n_bhh', _P3),
                ('w_node', c_void_p), ('b_node', c_void_p), ('w_edge', c_void_p), ('b_edge', c_void_p)]


class CTrackRows(C.Structure):
    """struct tmpnn_track_rows (include/tmpnn.h): the row form of the rolling tracking graph."""
    _fields_ = [('ts', c_void_p), ('det_id', c_void_p), ('assoc', c_void_p), ('is_edge', c_void_p), ('src', c_void_p),
                ('dst', c_void_p), ('labels', c_void_p)]


class CLossWindows(C.Structure):
    """struct tmpnn_loss_windows (include/tmpnn.h): the loss windows of one call of a block-diagonal training batch."""
    _fields_ = [('W', C.c_int32), ('n_det', C.c_int32), ('n_edge', C.c_int32), ('det_ptr', c_void_p), ('det_idx', c_void_p),
                ('edge_ptr', c_void_p), ('edge_idx', c_void_p), ('det_win', c_void_p), ('edge_win', c_void_p)]


class CTrainBuild(C.Structure):
    """struct tmpnn_train_build (include/tmpnn.h): the device build of a training batch."""
    _fields_ = [('n', C.c_int32), ('B', C.c_int32), ('C', C.c_int32), ('max_dets', C.c_int32), ('max_slots', C.c_int32),
                ('n_feat', C.c_int64)] + [(f, c_void_p) for f in (
                    'y', 'offsets', 'info', 'kept', 'cptr', 'counts', 'blk', 'call_tab', 'cb_tab',
                    'src', 'dst', 'edge_row', 'src_pos', 'dst_pos', 'det_row', 'seg_of_det', 'new_det_local', 'det_group',
                    'is_edge', 'pos', 'labels', 'feat_src', 'seg_of_new',
                    'rowptr', 'inc', 'det_order', 'det_win', 'edge_win', 'det_idx', 'edge_idx')]


class CChunkDraw(C.Structure):
    """struct tmpnn_chunk_draw (include/tmpnn.h): a seeded draw of augmented training chunks from the detection store."""
    _fields_ = ([(f, C.c_int32) for f in ('B', 'nchunks', 'L', 'nseq', 'F', 'Fs', 'fr_range', 'transforms')]
                + [(f, C.c_int64) for f in ('ndets', 'nframes', 'n_max')] + [('seed', C.c_uint64), ('step', C.c_uint64)]
                + [(f, c_float) for f in ('p_drop', 'p_reverse', 'p_flip')] + [('ldx', C.c_int32)]
                + [(f, c_void_p) for f in ('indices', 'chunks', 'seq_base', 'first', 'track', 'stat', 'table',
                                           'count', 'flags', 'offsets', 'X', 'y')])


class CChunkDrawVis(C.Structure):
    """struct tmpnn_chunk_vis (include/tmpnn.h): what a store with the 'vis' feature group adds to a draw."""
    _fields_ = [(f, c_void_p) for f in ('box', 'seq_hw', 'slot', 'o_box', 'o_im_hw', 'o_map_of', 'o_track')]


class CSeqFeatures(C.Structure):
    """struct tmpnn_seq_features_args (include/tmpnn.h): the whole-sequence features of listed sequences from the detection store."""
    _fields_ = ([(f, C.c_int32) for f in ('K', 'nseq', 'F', 'Fs', 'ldx', 'fr_range', 'frames_per_batch', 'reserved')]
                + [(f, C.c_int64) for f in ('ndets', 'nframes', 'n_rows')]
                + [(f, c_void_p) for f in ('seqs', 'offsets', 'seq_base', 'first', 'frame', 'track', 'stat', 'table', 'box', 'seq_hw',
                                           'X', 'y', 'o_box', 'o_im_hw', 'o_map_of', 'flag')])


class CFramesGather(C.Structure):
    """struct tmpnn_frames_gather_args (include/tmpnn.h): the CNN's input images of a frame plan from the resident uint8 frames."""
    _fields_ = ([(f, C.c_int32) for f in ('T', 'H', 'W', 'nseq')] + [('nframes', C.c_int64)]
                + [(f, c_void_p) for f in ('frames', 'seq_base', 'plan', 'table', 'out')])


class CFramesResize(C.Structure):
    """struct tmpnn_frames_resize_args (include/tmpnn.h): raw interleaved frames to the CNN's input size, planar uint8 or float32."""
    _fields_ = ([(f, C.c_int32) for f in ('n', 'h', 'w', 'H', 'W', 'kx', 'ky', 'reserved')]
                + [(f, c_void_p) for f in ('src', 'bounds_x', 'coef_x', 'bounds_y', 'coef_y', 'table', 'out', 'ws')]
                + [('ws_bytes', c_size_t)])


class CMotStore(C.Structure):
    """struct tmpnn_mot_store (include/tmpnn.h): both sides of S sequences sorted by frame, for the MOT evaluation."""
    _fields_ = ([('S', C.c_int32), ('reserved', C.c_int32)] + [(f, C.c_int64) for f in ('n_gt', 'n_det', 'n_off', 'n_obj')]
                + [(f, c_void_p) for f in ('seq', 'gt_off', 'det_off', 'gt_id', 'gt_box', 'det_box', 'det_perm')])


class CEvalPrepStore(C.Structure):
    """struct tmpnn_evalprep_store (include/tmpnn.h): both sides of S sequences sorted by frame, the rules as one code byte a row."""
    _fields_ = ([('S', C.c_int32), ('reserved', C.c_int32)] + [(f, C.c_int64) for f in ('n_gt', 'n_det', 'n_off')]
                + [('height_thr', C.c_double)]
                + [(f, c_void_p) for f in ('seq', 'gt_off', 'det_off', 'gt_code', 'det_code', 'gt_box', 'det_box', 'det_perm')])


class CResultStore(C.Structure):
    """struct tmpnn_result_store (include/tmpnn.h): the detections of S sequences sorted by frame, for the result filter."""
    _fields_ = ([('S', C.c_int32), ('n_cat', C.c_int32)] + [(f, C.c_int64) for f in ('n_det', 'n_off', 'n_tab')]
                + [(f, c_void_p) for f in ('seq', 'det_off', 'det_perm', 'det_fidx', 'det_cat', 'det_key', 'thr_key')])


class CMapStore(C.Structure):
    """struct tmpnn_map_store (include/tmpnn.h): GT rows by (class, sequence, frame), claim lists and per-class order, for mAP."""
    _fields_ = ([('S', C.c_int32), ('C', C.c_int32)] + [(f, C.c_int64) for f in ('n_gt', 'n_det', 'n_grp', 'n_live', 'n_claim')]
                + [(f, c_void_p) for f in ('gt_box', 'gt_seq', 'cls_gt_off', 'grp_off', 'det_box', 'det_grp', 'det_best', 'cls_off',
                                           'order', 'claim_off', 'claim_det')])


class CLabelStore(C.Structure):
    """struct tmpnn_label_store (include/tmpnn.h): both sides of S sequences sorted by frame, for the GT track-id labelling."""
    _fields_ = ([('S', C.c_int32), ('reserved', C.c_int32)] + [(f, C.c_int64) for f in ('n_frames', 'n_det', 'n_gt')]
                + [('iom_ignore_cat', C.c_int32), ('iou_ignore_cat', C.c_int32), ('iou_thresh', c_float), ('iom_thresh', c_float)]
                + [(f, C.c_int64) for f in ('n_small', 'n_big')]
                + [(f, c_void_p) for f in ('seq_base', 'det_first', 'gt_first', 'small_frames', 'big_frames', 'det_frame', 'det_cat',
                                           'det_box', 'det_score', 'gt_frame', 'gt_track', 'gt_cat', 'gt_box')])


class CLabelOut(C.Structure):
    """struct tmpnn_label_out (include/tmpnn.h): what tmpnn_label_dets and tmpnn_label_compact write."""
    _fields_ = [(f, c_void_p) for f in ('record', 'track', 'keep', 'gt_keep', 'det_cnt', 'gt_cnt', 'fflag', 'det_off', 'gt_off',
                                        'seq_det_off', 'seq_gt_off', 'o_det_frame', 'o_det_track', 'o_det_cat', 'o_det_box',
                                        'o_det_score', 'o_gt_frame', 'o_gt_track', 'o_gt_cat', 'o_gt_box')]


class CVisHead(C.Structure):
    """struct tmpnn_vis_head (include/tmpnn.h): one call of the visual head (box-centre gather, softmax rows, identity loss)."""
    _fields_ = ([(f, C.c_int32) for f in ('T', 'Hm', 'Wm', 'B')] + [('D', C.c_int64)]
                + [(f, c_float) for f in ('input_h', 'input_w', 'down_ratio', 'im_h', 'im_w')]
                + [(f, C.c_int32) for f in ('ld_rows', 'col', 'reserved')]
                + [(f, c_void_p) for f in ('maps', 'box', 'map_of', 'im_hw', 'track', 'offsets', 'mean', 'std', 'rows', 'logits',
                                           'stat', 'nll', 'pix', 'flag', 'chunk_of', 'key', 'loss', 'count')])


class CEmbedLoss(C.Structure):
    """struct tmpnn_embed_loss (include/tmpnn.h): one call of the embedding (pull-push) loss over D rows in B chunks."""
    _fields_ = ([('D', C.c_int64)] + [(f, C.c_int32) for f in ('B', 'W', 'ld')] + [('delta_var', c_float), ('delta_dist', c_float),
                ('reserved', C.c_int32)] + [(f, c_void_p) for f in ('features', 'track', 'offsets', 'ws')]
                + [('ws_bytes', c_size_t)] + [(f, c_void_p) for f in ('loss', 'terms', 'count')])


_DGP = C.POINTER(CDGraph)
_MPP = C.POINTER(CMpParams)
_TRP = C.POINTER(CTrackRows)
_LWP = C.POINTER(CLossWindows)
_TBP = C.POINTER(CTrainBuild)
_CDP = C.POINTER(CChunkDraw)
_CVP = C.POINTER(CChunkDrawVis)
_FGP = C.POINTER(CFramesGather)
_FRP = C.POINTER(CFramesResize)
_MSP = C.POINTER(CMotStore)
_MAP = C.POINTER(CMapStore)
_RSP = C.POINTER(CResultStore)
_LSP = C.POINTER(CLabelStore)
_LOP = C.POINTER(CLabelOut)
_VHP = C.POINTER(CVisHead)

# name -> (restype, argtypes); must mirror include/tmpnn.h (tests/test_abi.py cross-checks the names)
_SIGNATURES = {
    'tmpnn_abi_version': (c_int, []),
    'tmpnn_last_error': (C.c_char_p, []),
    'tmpnn_gather_diff_fwd': (c_int, [_GP, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    'tmpnn_gather_concat_fwd': (c_int, [_GP, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    'tmpnn_gather_diff_bwd': (c_int, [_GP, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    'tmpnn_gather_concat_bwd': (c_int, [_GP, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    'tmpnn_segsum_fwd': (c_int, [_GP, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'tmpnn_segsum_fwd_live': (c_int, [_GP, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'tmpnn_segsum_bwd': (c_int, [_GP, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    'tmpnn_att_fwd': (c_int, [_GP, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'tmpnn_att_bwd_ws': (c_size_t, [c_int, c_int, c_int, c_int]),
    'tmpnn_att_index': (c_int, [_GP, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_att_bwd': (c_int, [_GP, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                              c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t,
                              c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'tmpnn_att_bwd_heads': (c_int, [_GP, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                    c_size_t, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'tmpnn_gru_fwd': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                              c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    'tmpnn_gru_fwd_head_parts': (c_int, [c_int, c_int, c_int]),
    'tmpnn_gru_fwd_tiles': (c_int, [_TP, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    'tmpnn_gru_fwd_tiles_zero_state_available': (c_int, [c_int, c_int]),
    'tmpnn_gru_fwd_tiles_zero_state': (c_int, [_TP, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                               c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'tmpnn_heads_finish': (c_int, [c_void_p, c_size_t, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_gru_bwd_data': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p,
                                   c_void_p, c_int, c_void_p, c_int,
                                   c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'tmpnn_gru_bwd_weights_ws': (c_size_t, [c_int, c_int, c_int]),
    'tmpnn_gru_bwd_weights': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'tmpnn_gru_bwd_fused_available': (c_int, [c_int, c_int, c_int]),
    'tmpnn_gru_bwd_fused_ws': (c_size_t, [c_int, c_int, c_int]),
    'tmpnn_gru_bwd_fused': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int,
                                    c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                    c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    'tmpnn_gru_bwd_fused_zero_state_available': (c_int, [c_int, c_int, c_int]),
    'tmpnn_gru_bwd_fused_zero_state': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                               c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int, c_void_p,
                                               c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_size_t, c_void_p]),
    'tmpnn_rows_linear': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    'tmpnn_transpose': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'tmpnn_reduce_slabs': (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p]),
    'tmpnn_input_bn_fwd': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'tmpnn_input_bn_bwd_ws': (c_size_t, [c_int, c_int, c_int, c_int]),
    'tmpnn_input_bn_bwd': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                   c_void_p, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_size_t, c_void_p]),
    'tmpnn_input_tf_supported': (c_int, [c_int, c_int, c_int]),
    'tmpnn_input_tf_fwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'tmpnn_input_tf_bwd_ws': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'tmpnn_input_tf_bwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                   c_void_p, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_size_t, c_void_p]),
    'tmpnn_heads_fwd': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    'tmpnn_heads_bwd_ws': (c_size_t, [c_int, c_int]),
    'tmpnn_heads_bwd': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    'tmpnn_targets': (c_int, [_GP, c_void_p, c_void_p, c_void_p]),
    'tmpnn_ce_loss_ws': (c_size_t, [c_int]),
    'tmpnn_ce_loss_fwd': (c_int, [_GP, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'tmpnn_ce_loss_bwd': (c_int, [_GP, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_focal_loss_ws': (c_size_t, [c_int]),
    'tmpnn_focal_loss_fwd': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_float, c_float, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    'tmpnn_focal_loss_bwd': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_float, c_float, c_void_p,
                                     c_float, c_void_p, c_void_p]),
    'tmpnn_bce_logits_ws': (c_size_t, [C.c_long]),
    'tmpnn_bce_logits_sum_fwd': (c_int, [c_void_p, c_void_p, C.c_long, c_void_p, c_void_p, c_size_t, c_void_p]),
    'tmpnn_bce_logits_sum_bwd': (c_int, [c_void_p, c_void_p, C.c_long, c_void_p, c_void_p, c_void_p]),
    'tmpnn_train_losses_supported': (c_int, [c_int, c_int]),
    'tmpnn_train_losses_ws': (c_size_t, [c_int, c_int]),
    'tmpnn_train_losses_fwd': (c_int, [_GP, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_void_p]),
    'tmpnn_train_losses_bwd': (c_int, [_GP, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_void_p, c_void_p, c_void_p]),
    'tmpnn_train_losses_win_ws': (c_size_t, [_LWP]),
    'tmpnn_train_losses_win_fwd': (c_int, [_GP, _LWP, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_size_t, c_void_p]),
    'tmpnn_train_losses_win_bwd': (c_int, [_GP, _LWP, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'tmpnn_cls_counts': (c_int, [_GP, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'tmpnn_cls_counts_win': (c_int, [_GP, _LWP, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'tmpnn_train_record_fold': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'tmpnn_optim_chunk': (c_int, []),
    'tmpnn_adam_step': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, C.c_int64, c_void_p,
                                C.c_double, C.c_double, C.c_double, C.c_double, c_float, c_int, c_void_p]),
    'tmpnn_grad_flow': (c_int, [c_void_p, c_int, c_void_p, C.c_int64, c_void_p, c_void_p]),
    'tmpnn_train_build_count': (c_int, [_TBP, c_void_p]),
    'tmpnn_train_build_calls': (c_int, [_TBP, c_void_p]),
    'tmpnn_train_build_fill': (c_int, [_TBP, c_int, c_void_p]),
    'tmpnn_chunk_draw_count': (c_int, [_CDP, c_void_p]),
    'tmpnn_chunk_draw_fill': (c_int, [_CDP, c_void_p]),
    'tmpnn_chunk_draw_vis': (c_int, [_CDP, _CVP, c_void_p]),
    'tmpnn_seq_features': (c_int, [C.POINTER(CSeqFeatures), c_void_p]),
    'tmpnn_frames_gather': (c_int, [_FGP, c_void_p]),
    'tmpnn_frames_resize_ws': (c_size_t, [c_int] * 5),
    'tmpnn_frames_resize': (c_int, [_FRP, c_void_p]),
    'tmpnn_online_features': (c_int, [c_int] * 8 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                      c_void_p, c_void_p, c_void_p]),
    'tmpnn_mot_max_per_frame': (c_int, []),
    'tmpnn_mot_events_ws': (c_size_t, [c_int, C.c_int64, C.c_int64]),
    'tmpnn_mot_events': (c_int, [_MSP, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'tmpnn_mot_dist': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'tmpnn_mot_summary_limit': (c_int, [c_int]),
    'tmpnn_mot_summary_ws': (c_size_t, [c_int, C.c_int64, C.c_int64, C.c_int64]),
    'tmpnn_mot_summary': (c_int, [_MSP, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'tmpnn_hota_ws': (c_size_t, [c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    'tmpnn_hota': (c_int, [_MSP, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'tmpnn_evalprep_max_per_frame': (c_int, []),
    'tmpnn_evalprep': (c_int, [C.POINTER(CEvalPrepStore), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_results_ws': (c_size_t, [c_int, C.c_int64, C.c_int64]),
    'tmpnn_results_apply': (c_int, [_RSP, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_map_tile': (c_int, []),
    'tmpnn_map_best': (c_int, [_MAP, c_void_p, c_void_p]),
    'tmpnn_map_eval_ws': (c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    'tmpnn_map_eval': (c_int, [_MAP, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    'tmpnn_label_max_per_frame': (c_int, []),
    'tmpnn_label_wave_frame': (c_int, []),
    'tmpnn_label_dets': (c_int, [_LSP, _LOP, c_void_p]),
    'tmpnn_label_compact': (c_int, [_LSP, _LOP, c_void_p]),
    'tmpnn_vis_head_fwd': (c_int, [_VHP, c_void_p]),
    'tmpnn_vis_head_bwd': (c_int, [_VHP, c_void_p, c_void_p, c_void_p]),
    'tmpnn_vis_head_scatter': (c_int, [_VHP, c_void_p, c_void_p, c_void_p]),
    'tmpnn_vis_head_pixels': (c_int, [_VHP, c_void_p]),
    'tmpnn_vis_head_rows_from_logits': (c_int, [_VHP, c_void_p]),
    'tmpnn_embed_loss_ws': (c_size_t, [C.c_int64, c_int]),
    'tmpnn_embed_loss_fwd': (c_int, [C.POINTER(CEmbedLoss), c_void_p]),
    'tmpnn_embed_loss_bwd': (c_int, [C.POINTER(CEmbedLoss), c_void_p, c_void_p, c_void_p]),
    'tmpnn_train_embed_fold': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'tmpnn_espnet_arena_floats': (c_size_t, [c_int]),
    'tmpnn_espnet_ws_bytes': (c_size_t, [c_int] * 4),
    'tmpnn_espnet_fwd': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    'tmpnn_espnet_centres_ws_bytes': (c_size_t, [c_int] * 4),
    'tmpnn_espnet_trunk': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    'tmpnn_espnet_centres': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p,
                                     c_void_p]),
    'tmpnn_espnet_train_param_floats': (c_size_t, [c_int]),
    'tmpnn_espnet_train_table': (c_int, [c_int, c_void_p, c_int]),
    'tmpnn_espnet_train_ws_bytes': (c_size_t, [c_int] * 4),
    'tmpnn_espnet_train_bwd_ws_bytes': (c_size_t, [c_int] * 4),
    'tmpnn_espnet_refold': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'tmpnn_espnet_train_fwd': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    'tmpnn_espnet_train_bwd': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                       c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_espnet_dec_param_floats': (c_size_t, [c_int]),
    'tmpnn_espnet_dec_table': (c_int, [c_int, c_void_p, c_int]),
    'tmpnn_espnet_dec_ws_bytes': (c_size_t, [c_int] * 4),
    'tmpnn_espnet_dec_bwd_ws_bytes': (c_size_t, [c_int] * 4),
    'tmpnn_espnet_dec_refold': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'tmpnn_espnet_dec_fwd': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    'tmpnn_espnet_dec_bwd': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                     c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_dgraph_ints': (c_size_t, [c_int]),
    'tmpnn_dgraph_bind': (c_int, [c_void_p, c_int, c_int, _DGP]),
    'tmpnn_graph_from_coo': (c_int, [c_int, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, C.c_int64, _DGP, c_void_p]),
    'tmpnn_graph_from_coo_arena': (c_int, [c_int, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, C.c_int64, c_void_p, c_int, c_void_p]),
    'tmpnn_graph_from_coo_arena_ws': (c_int, [c_int, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, C.c_int64, c_void_p, c_int,
                                              c_void_p, c_size_t, c_void_p]),
    'tmpnn_graph_from_rows_ws': (c_int, [c_int, c_void_p, c_void_p, c_void_p, _DGP, c_void_p, c_size_t, c_void_p]),
    'tmpnn_track_finalize_ws': (c_size_t, [c_int]),
    'tmpnn_track_load': (c_int, [c_int, c_int, c_void_p, _TRP, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, _DGP, c_void_p,
                                 c_size_t, c_void_p]),
    'tmpnn_track_select': (c_int, [_DGP, _TRP, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'tmpnn_track_select_ws': (c_int, [_DGP, _TRP, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'tmpnn_track_hungarian_max_dets': (c_int, []),
    'tmpnn_track_extend': (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, _TRP, c_void_p, c_int, c_int,
                                   c_void_p, c_int, _DGP, c_void_p, c_size_t, c_void_p]),
    'tmpnn_track_extend_tf': (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, _TRP, c_void_p, c_int, c_void_p,
                                      c_void_p, c_void_p, c_size_t, _DGP, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'tmpnn_track_retire': (c_int, [_DGP, _TRP, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                   c_void_p, c_void_p, _TRP, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                   c_void_p, c_void_p, c_void_p]),
    'tmpnn_val_f1_count': (c_int, [_DGP, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    'tmpnn_att_hist_count': (c_int, [_DGP, c_void_p, c_void_p, C.c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                     c_void_p]),
    'tmpnn_wide_supported': (c_int, [c_int, c_int]),
    'tmpnn_wide_prep_bytes': (c_size_t, [c_int, c_int]),
    'tmpnn_wide_prepare': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'tmpnn_wide_gru_fwd': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    'tmpnn_wide_gru_fwd_tiled': (c_int, [c_void_p, c_void_p, c_int, _TP, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    'tmpnn_wide_gru_bwd_diff_ws': (c_size_t, [c_int, c_int, c_int, c_int]),
    'tmpnn_wide_gru_bwd_diff': (c_int, [c_void_p, _GP, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int,
                                        c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_size_t, c_void_p]),
    'tmpnn_wide_gru_bwd_diff_fused': (c_int, [c_void_p, _GP, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int,
                                              c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_mp_iter_prep_floats': (c_size_t, [c_int, c_int, c_int]),
    'tmpnn_mp_iter_prepare': (c_int, [_MPP, c_void_p, c_void_p]),
    'tmpnn_mp_iter_save_floats': (c_size_t, [c_int, c_int, c_int, c_int]),
    'tmpnn_mp_iter_fwd': (c_int, [_MPP, c_void_p, _DGP, c_int, c_void_p, c_int, c_void_p, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'tmpnn_mp_iter_save_es_offset': (c_size_t, [c_int, c_int, c_int, c_int]),
    'tmpnn_mp_iter_fwd_parts': (c_int, [_MPP, c_void_p, _DGP, c_int, c_void_p, c_int, c_void_p, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    'tmpnn_mp_iter_bwd_parts': (c_int, [_MPP, c_void_p, _DGP, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, _MPP, c_void_p,
                                        c_size_t, c_int, c_void_p]),
    'tmpnn_mp_iter_bwd_ws': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'tmpnn_mp_iter_bwd': (c_int, [_MPP, c_void_p, _DGP, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, _MPP, c_void_p,
                                  c_size_t, c_void_p]),
}

_lib: Optional[C.CDLL] = None


# entry points only a comparison build (-DTMPNN_KEEP_VARIANTS, tools/build_variant.sh) exports: bound when the loaded library
# has them (TMPNN_LIB_PATH pointing at such a build), absent from the shipped one
_VARIANT_SIGNATURES = {
    'tmpnn_track_append': (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_gru_bwd_weights_variant': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                              c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    'tmpnn_gru_bwd_weights_choice': (c_int, []),
    'tmpnn_wide_gru_bwd_diff_aux': (c_int, [c_void_p, _GP, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int,
                                            c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    'tmpnn_wide_gru_bwd_data_ws': (c_size_t, [c_int, c_int]),
    'tmpnn_wide_gru_bwd_data': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_int,
                                        c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    'tmpnn_wide_gru_bwd_weights_ws': (c_size_t, [c_int, c_int]),
    'tmpnn_wide_gru_bwd_weights': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}


def header_symbols(variants: bool = False) -> List[str]:
    """Every function name include/tmpnn.h declares for the shipped library (variants=True: also the comparison-build
    entry points of its `#ifdef TMPNN_KEEP_VARIANTS` section)."""
    with open(HEADER_PATH) as f:
        txt = f.read()
    if not variants:
        txt = re.sub(r'#ifdef TMPNN_KEEP_VARIANTS.*?#endif', '', txt, flags=re.S)
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(tmpnn_[a-z0-9_]+)\s*\(', txt)))


def load() -> C.CDLL:
    """Load libtmpnn.so (once).  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  trackmpnn_amd has no CPU or torch fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f'libtmpnn.so does not export {name}; rebuild it') from e
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in _VARIANT_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    v = lib.tmpnn_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f'libtmpnn.so ABI version {v} != expected {ABI_VERSION}; rebuild it')
    _lib = lib
    return lib


def last_error() -> str:
    return load().tmpnn_last_error().decode('utf-8', 'replace')


def call(name: str, *args) -> None:
    """Invoke an int-returning entry point; raise RuntimeError(tmpnn_last_error()) on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f'{name} failed (code {rc}): {last_error()}')


def fn(name: str):
    """The bound ctypes function (for hot paths that call it many times; the caller checks the return code)."""
    return getattr(load(), name)


def ptr(t) -> Optional[int]:
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def raw_stream(device=None) -> int:
    """hipStream_t of torch's current stream on `device` (default: the current device) as an integer.  The public
    torch.cuda.current_stream() builds a Stream object per call (~7 us: twice per batch-1 forward call it was a seventh
    of the host time); the raw accessor is a plain C call."""
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    return torch._C._cuda_getCurrentRawStream(idx)
