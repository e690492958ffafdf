"""The host definition of the MOT evaluation (trackmpnn_amd.moteval.mot_events_host), the store the device evaluator is fed
from, and the argument checks of the new entry points -- no GPU.  tests/test_mot_eval_gpu.py holds the device kernel to this
definition."""
import ctypes as C
import math

import numpy as np
import pytest

from trackmpnn_amd import _lib
from trackmpnn_amd.moteval import (COUNT_KEYS, MAX_PER_FRAME, MotEvaluator, MotStore, mot_dist_host, mot_events_host, mot_overall,
                                   synth_mot_sequence)


def B(x, y, w=10, h=10):
    return [x, y, x + w, y + h]


def run(det, gt):
    """det: rows (frame, track, box); gt: rows (frame, id, box)."""
    return mot_events_host([d[0] for d in det], [d[2] for d in det], [d[1] for d in det],
                           [g[0] for g in gt], [g[1] for g in gt], [g[2] for g in gt])


def counts(r):
    return tuple(r[k] for k in COUNT_KEYS)


def test_hand_case():
    """Two objects; their hypothesis ids swap at frame 1; at frame 2 one object is gone and a stray hypothesis appears."""
    gt = [(0, 1, B(0, 0)), (0, 2, B(100, 0)), (1, 1, B(0, 0)), (1, 2, B(100, 0)), (2, 1, B(0, 0))]
    det = [(0, 10, B(0, 0)), (0, 20, B(100, 0)), (1, 20, B(0, 0)), (1, 10, B(100, 0)), (2, 20, B(1, 0)), (2, 30, B(500, 500))]
    r = run(det, gt)
    assert counts(r) == (5, 6, 5, 2, 1, 0, 3)
    assert r['dist_sum'] == 0.18181818181818177
    assert r['mota'] == 1 - 3 / 5 and r['motp'] == r['dist_sum'] / 5 and r['recall'] == 1.0 and r['precision'] == 5 / 6


def test_kept_correspondence_wins_over_a_cheaper_alternative():
    """Step 1 runs before the assignment: object 1 keeps hypothesis 10 although hypothesis 20 now fits it better (and is
    taken by nobody else); an optimal assignment alone would pick 20."""
    gt = [(0, 1, B(0, 0)), (1, 1, B(0, 0))]
    det = [(0, 10, B(0, 0)), (1, 10, B(3, 0)), (1, 20, B(0, 0))]
    r = run(det, gt)
    assert counts(r) == (2, 3, 2, 0, 1, 0, 2)
    assert r['dist_sum'] == mot_dist_host([B(0, 0)], [B(3, 0)])[0, 0]


def test_correspondence_is_not_kept_across_an_unmatched_frame():
    """Object 1 is matched at frame 0 and unmatched at frame 1.  At frame 2 the assignment decides: the better hypothesis 20
    wins over the remembered 10 and counts as a switch; with only the same id left it is a plain match."""
    gt = [(0, 1, B(0, 0)), (1, 1, B(0, 0)), (2, 1, B(0, 0))]
    r = run([(0, 10, B(0, 0)), (2, 10, B(3, 0)), (2, 20, B(0, 0))], gt)
    assert counts(r) == (3, 3, 2, 1, 1, 1, 3) and r['dist_sum'] == 0.0
    r = run([(0, 10, B(0, 0)), (2, 10, B(3, 0))], gt)
    assert counts(r) == (3, 2, 2, 0, 0, 1, 3)
    # a switch is counted however long ago the other id was remembered
    r = run([(0, 10, B(0, 0)), (2, 20, B(0, 0))], gt)
    assert counts(r) == (3, 2, 2, 1, 0, 1, 3)


def test_negative_tracks_are_ignored_on_both_sides():
    gt = [(0, 1, B(0, 0)), (0, -1, B(50, 0)), (1, 1, B(0, 0))]
    det = [(0, 10, B(0, 0)), (0, -1, B(50, 0)), (1, -1, B(0, 0))]
    assert counts(run(det, gt)) == (2, 1, 1, 0, 0, 1, 2)
    # ... but their frames still span the range (metrics.py:19-22 sorts every row's frame)
    assert run(det + [(5, -1, B(0, 0))], gt)['frames'] == 6


def test_frames_empty_on_one_side_or_both():
    gt = [(0, 1, B(0, 0)), (3, 1, B(0, 0))]
    det = [(1, 10, B(0, 0)), (3, 10, B(0, 0))]
    assert counts(run(det, gt)) == (2, 2, 1, 0, 1, 1, 4)          # frame 0: GT only, 1: hypotheses only, 2: neither


def test_no_hypotheses_and_no_ground_truth():
    gt = [(0, 1, B(0, 0)), (1, 1, B(0, 0))]
    r = run([], gt)
    assert counts(r) == (2, 0, 0, 0, 0, 2, 2) and r['mota'] == 0.0 and math.isnan(r['motp']) and math.isnan(r['precision'])
    r = run([(4, 10, B(0, 0))], [])
    assert counts(r) == (0, 1, 0, 0, 1, 0, 1) and math.isnan(r['mota']) and math.isnan(r['recall'])
    r = run([], [])
    assert counts(r) == (0, 0, 0, 0, 0, 0, 0) and math.isnan(r['mota'])


def test_zero_area_boxes_cannot_be_matched():
    z = [5, 5, 5, 5]
    d = mot_dist_host([z, B(0, 0)], [z, B(0, 0)])
    assert math.isnan(d[0, 0]) and d[1, 1] == 0.0                  # 0 / 0 stays NaN
    assert counts(run([(0, 10, z)], [(0, 1, z)])) == (1, 1, 0, 0, 1, 1, 1)


def test_distance_special_pairs():
    a = B(0, 0)
    d = mot_dist_host([a], [B(50, 50), a, B(10, 0), B(2, 2, 4, 4), B(0, 0, 5, 10), B(0, 0, 4, 10)])[0]
    assert math.isnan(d[0]) and d[1] == 0.0 and math.isnan(d[2])   # disjoint, identical, touching at an edge
    assert math.isnan(d[3])                                        # a 4 x 4 box inside a 10 x 10 one: IoU 0.16
    assert d[4] == 0.5                                             # IoU exactly 0.5 stays finite
    assert math.isnan(d[5])
    assert d.dtype == np.float64


def test_overall_is_the_ratio_of_summed_counts():
    a = run([(0, 10, B(0, 0))], [(0, 1, B(0, 0))])                                     # mota 1
    b = run([], [(t, 1, B(0, 0)) for t in range(9)])                                   # mota 0
    o = mot_overall([a, b])
    assert o['objects'] == 10 and o['misses'] == 9 and o['mota'] == 1 - 9 / 10         # not the mean of the ratios (0.5)
    assert o['mota'] != (a['mota'] + b['mota']) / 2
    assert math.isnan(mot_overall([])['mota'])


def test_duplicate_id_in_a_frame_raises():
    with pytest.raises(ValueError, match='GT id occurs twice in frame 0'):
        run([], [(0, 1, B(0, 0)), (0, 1, B(50, 0))])
    with pytest.raises(ValueError, match='hypothesis id occurs twice in frame 2'):
        run([(2, 7, B(0, 0)), (2, 7, B(50, 0))], [(2, 1, B(0, 0))])
    run([(2, -1, B(0, 0)), (2, -1, B(50, 0))], [(2, -1, B(0, 0)), (2, -1, B(9, 9))])   # -1 is no id


def test_store_construction_on_unsorted_input():
    q0 = {'det_frame': [7, 5, 7, 6, 5], 'det_box': [B(i, 0) for i in range(5)],
          'gt_frame': [6, 4, 6, 4, 9, 5], 'gt_track': [40, 7, 7, -1, 40, 300], 'gt_box': [B(0, i) for i in range(6)]}
    q1 = {'det_frame': [2], 'det_box': [B(9, 9)], 'gt_frame': [], 'gt_track': [], 'gt_box': []}
    st = MotStore([q0, q1])
    assert st.S == 2 and st.t0 == [4, 2] and st.empty == [False, True]
    # sequence 0: frames 4 .. 9; GT row 3 (track -1) dropped; stable in the frame
    assert st.seq[0].tolist() == [0, 5, 0, 5, 0, 6, 0, 3] and st.seq[1].tolist() == [5, 0, 5, 1, 7, 1, 3, 0]
    assert st.gt_off.tolist() == [0, 1, 2, 4, 4, 4, 5] + [0, 0]
    assert st.det_off.tolist() == [0, 0, 2, 3, 5, 5, 5] + [0, 1]
    assert st.det_perm.tolist() == [1, 4, 3, 0, 2] + [0]
    assert st.gt_ids[0].tolist() == [7, 40, 300]
    assert st.gt_id.tolist() == [0, 2, 1, 0, 1]                    # rows 1 (t4, id 7), 5 (t5, 300), 0 (t6, 40), 2 (t6, 7), 4 (t9, 40)
    assert st.gt_box[:, 1].tolist() == [1, 5, 0, 2, 4] and st.det_box[:, 0].tolist() == [1, 4, 3, 0, 2, 9]
    assert st.gt_box.dtype == np.float32 and st.det_box.dtype == np.float32 and st.gt_off.dtype == np.int32
    assert (st.n_gt, st.n_det, st.n_off, st.n_obj) == (5, 6, 9, 3)
    with pytest.raises(ValueError, match='sequence 1: a GT id occurs twice in frame 3'):
        MotStore([q0, {'det_frame': [], 'det_box': [], 'gt_frame': [3, 3], 'gt_track': [5, 5], 'gt_box': [B(0, 0), B(1, 1)]}])


def test_synthetic_generator_exercises_every_count():
    q = synth_mot_sequence(3, 40)
    r = mot_events_host(q['det_frame'], q['det_box'], q['tracks'], q['gt_frame'], q['gt_track'], q['gt_box'])
    assert r['switches'] > 0 and r['false_positives'] > 0 and r['misses'] > 0 and r['matches'] > 100
    assert r['matches'] + r['misses'] == r['objects'] and r['matches'] + r['false_positives'] == r['predictions']


def test_evaluator_needs_a_device():
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        MotEvaluator([], device='cpu')


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    assert lib.tmpnn_mot_max_per_frame() == MAX_PER_FRAME
    assert lib.tmpnn_mot_events(None, None, None, None, 0, None, None) == -1 and b'store is null' in lib.tmpnn_last_error()
    seq = np.array([[0, 2, 0, 3, 0, 4, 0, 2]], np.int64)
    one = C.c_void_p(256)                                          # (never dereferenced: every call below fails its checks)

    def store(**kw):
        f = dict(S=1, reserved=0, n_gt=2, n_det=3, n_off=5, n_obj=2, seq=one, gt_off=one, det_off=one, gt_id=one, gt_box=one,
                 det_box=one, det_perm=one)
        f.update(kw)
        return _lib.CMotStore(**f)

    def call(st, seq_host=seq, ws=one, ws_bytes=1 << 30):
        return lib.tmpnn_mot_events(C.byref(st), seq_host.ctypes.data if seq_host is not None else None, one, ws, ws_bytes, one, None)
    assert call(store(S=-1)) == -1
    assert call(store(), seq_host=None) == -1 and b'null pointer' in lib.tmpnn_last_error()
    assert call(store(gt_box=None)) == -1 and b'null GT arrays' in lib.tmpnn_last_error()
    assert call(store(det_perm=None)) == -1
    assert call(store(gt_box=C.c_void_p(260))) == -1 and b'16-byte aligned' in lib.tmpnn_last_error()
    assert call(store(n_gt=1)) == -1 and b'sequence 0: GT rows' in lib.tmpnn_last_error()
    assert call(store(n_det=2)) == -1 and b'detection rows' in lib.tmpnn_last_error()
    assert call(store(n_off=4)) == -1 and b'offsets' in lib.tmpnn_last_error()
    assert call(store(n_obj=1)) == -1 and b'objects' in lib.tmpnn_last_error()
    bad = seq.copy()
    bad[0, 5] = -1
    assert call(store(), seq_host=bad) == -1
    need = lib.tmpnn_mot_events_ws(1, 2, 3)
    assert need >= MAX_PER_FRAME * MAX_PER_FRAME * 8 + 4 * (2 + 2 + 3)
    assert call(store(), ws_bytes=need - 1) == -3 and b'workspace' in lib.tmpnn_last_error()
    assert call(store(), ws=None) == -3
    assert lib.tmpnn_mot_events_ws(-1, 0, 0) == 0
    assert lib.tmpnn_mot_events(C.byref(store(S=0)), None, None, None, 0, None, None) == 0      # nothing to do, nothing launched
    # tmpnn_mot_dist
    assert lib.tmpnn_mot_dist(None, -1, None, 0, None, None) == -1
    assert lib.tmpnn_mot_dist(None, 2, None, 2, None, None) == -1 and b'null pointer' in lib.tmpnn_last_error()
    assert lib.tmpnn_mot_dist(C.c_void_p(260), 2, one, 2, one, None) == -1 and b'16-byte aligned' in lib.tmpnn_last_error()
    assert lib.tmpnn_mot_dist(None, 0, None, 5, None, None) == 0
