"""The benchmark preprocessing rule on the host (trackmpnn_amd.evalprep): hand-computed frames, one per branch, and the
properties of the rule.  prep_set() is the set of synthetic sequences tests/test_evalprep_gpu.py runs on the device."""
import numpy as np
import pytest

from trackmpnn_amd.evalprep import (COUNT_KEYS, KITTI_CAR, KITTI_PEDESTRIAN, PrepRules, evalprep_frame_host, evalprep_host,
                                    evalprep_ioa_host, prep_eval_sequences, synth_prep_sequence)
from trackmpnn_amd.hota import hota_sim_host

CAR, VAN, CYC, DONTCARE = 2, 4, 3, 9
REMOVALS = ('removed_distractor', 'removed_occluded', 'removed_small', 'removed_ignored')


def box(x, y, w, h):
    return [x, y, x + w, y + h]


def frame(dets, gts, rules=KITTI_CAR):
    """dets: (category, box, track); gts: (category, box, occlusion, truncation)."""
    d = list(zip(*dets)) if dets else ([], [], [])
    g = list(zip(*gts)) if gts else ([], [], [], [])
    out, keep, c = evalprep_frame_host(np.asarray(d[0], np.int64), np.asarray(d[1], np.float32).reshape(-1, 4), np.asarray(d[2], np.int64),
                                       np.asarray(g[0], np.int64), np.asarray(g[1], np.float32).reshape(-1, 4), np.asarray(g[2], np.int64),
                                       np.asarray(g[3], np.int64), rules)
    assert sum(c[k] for k in COUNT_KEYS[1:]) == c['rows_in']
    return out.tolist(), keep.tolist(), c


def counts(**kw):
    c = {k: 0 for k in COUNT_KEYS}
    c.update(kw)
    return c


def test_a_box_on_a_van_is_removed_and_the_same_box_on_a_car_stays():
    b = box(100, 100, 50, 50)
    assert frame([(CAR, b, 5)], [(VAN, b, 0, 0)]) == ([-1], [False], counts(rows_in=1, removed_distractor=1))
    assert frame([(CAR, b, 5)], [(CAR, b, 0, 0)]) == ([5], [True], counts(rows_in=1, kept=1))
    # the pedestrian rules: Person_sitting (6) is the distractor, a Van is nothing
    assert frame([(1, b, 5)], [(6, b, 0, 0)], KITTI_PEDESTRIAN) == ([-1], [False], counts(rows_in=1, removed_distractor=1))
    assert frame([(1, b, 5)], [(VAN, b, 0, 0)], KITTI_PEDESTRIAN) == ([5], [False], counts(rows_in=1, kept=1))


def test_a_box_on_an_occluded_or_truncated_car_is_removed_and_that_gt_row_is_not_kept():
    b = box(100, 100, 50, 50)
    assert frame([(CAR, b, 5)], [(CAR, b, 3, 0)]) == ([-1], [False], counts(rows_in=1, removed_occluded=1))
    assert frame([(CAR, b, 5)], [(CAR, b, 0, 1)]) == ([-1], [False], counts(rows_in=1, removed_occluded=1))
    assert frame([(CAR, b, 5)], [(CAR, b, 2, 0)]) == ([5], [True], counts(rows_in=1, kept=1))


def test_an_unmatched_25_px_box_is_removed_and_a_25_5_px_one_stays():
    out, _, c = frame([(CAR, box(100, 100, 50, 25), 5), (CAR, box(300, 100, 50, 25.5), 6)], [])
    assert out == [-1, 6] and c == counts(rows_in=2, removed_small=1, kept=1)


def test_a_small_matched_box_stays():
    b = box(100, 100, 40, 20)
    assert frame([(CAR, b, 5)], [(CAR, b, 0, 0)]) == ([5], [True], counts(rows_in=1, kept=1))


def test_an_unmatched_box_more_than_half_inside_a_region_is_removed_and_one_exactly_half_inside_stays():
    region = (DONTCARE, box(0, 0, 100, 100), -1, -1)
    inside, half = box(40, 10, 80, 50), box(50, 10, 100, 50)         # 60 of 80 px, 50 of 100 px of the width lie inside
    assert evalprep_ioa_host([inside, half], [region[1]]).ravel().tolist() == [0.75, 0.5]
    out, keep, c = frame([(CAR, inside, 5), (CAR, half, 6)], [region])
    assert out == [-1, 6] and keep == [False] and c == counts(rows_in=2, removed_ignored=1, kept=1)


def test_a_matched_box_inside_a_region_stays():
    b = box(20, 20, 50, 50)
    out, keep, c = frame([(CAR, b, 5)], [(DONTCARE, box(0, 0, 100, 100), -1, -1), (CAR, b, 0, 0)])
    assert out == [5] and keep == [False, True] and c == counts(rows_in=1, kept=1)


def test_equal_iou_to_a_car_and_a_van_goes_the_way_of_scipys_assignment():
    from scipy.optimize import linear_sum_assignment
    d, left, right = box(100, 100, 50, 50), box(90, 100, 50, 50), box(110, 100, 50, 50)
    s = hota_sim_host([left, right], [d])
    assert s[0, 0] == s[1, 0] == 2000.0 / 3000.0
    row = int(linear_sum_assignment(-s)[0][0])                      # the GT row scipy gives the one hypothesis
    for cats in ((CAR, VAN), (VAN, CAR)):
        out, _, c = frame([(CAR, d, 5)], [(cats[0], left, 0, 0), (cats[1], right, 0, 0)])
        if cats[row] == VAN:
            assert out == [-1] and c == counts(rows_in=1, removed_distractor=1)
        else:
            assert out == [5] and c == counts(rows_in=1, kept=1)


def test_a_tall_frame_and_a_wide_frame():
    # tall: three GT rows, one hypothesis, on the Van
    gts = [(CAR, box(100, 100, 50, 50), 0, 0), (VAN, box(300, 100, 50, 50), 0, 0), (CAR, box(500, 100, 50, 50), 3, 0)]
    out, keep, c = frame([(CAR, box(302, 100, 50, 50), 5)], gts)
    assert out == [-1] and keep == [True, False, False] and c == counts(rows_in=1, removed_distractor=1)
    # wide: one low Car; the identical box takes it, the shifted one (IoU 36 / 44) is left unmatched and is too low, the third is far
    g = box(100, 100, 40, 24)
    out, keep, c = frame([(CAR, box(104, 100, 40, 24), 5), (CAR, g, 6), (CAR, box(500, 100, 50, 50), 7)], [(CAR, g, 0, 0)])
    assert out == [-1, 6, 7] and keep == [True] and c == counts(rows_in=3, removed_small=1, kept=2)


def test_an_empty_side():
    out, keep, c = frame([(CAR, box(100, 100, 50, 50), 5), (CAR, box(300, 100, 50, 10), 6)], [])
    assert out == [5, -1] and keep == [] and c == counts(rows_in=2, removed_small=1, kept=1)
    out, keep, c = frame([], [(CAR, box(100, 100, 50, 50), 0, 0), (CAR, box(300, 100, 50, 50), 3, 0), (VAN, box(500, 100, 50, 50), 0, 0)])
    assert out == [] and keep == [True, False, False] and c == counts()
    assert frame([], []) == ([], [], counts())


def test_rows_of_another_class_and_rows_without_a_track_come_out_minus_one():
    b = box(100, 100, 50, 50)
    out, _, c = frame([(CYC, b, 5), (CAR, b, -1), (CAR, b, 7), (CYC, b, -1)], [(CAR, b, 0, 0)])
    assert out == [-1, -1, 7, -1] and c == counts(rows_in=2, other_class=1, kept=1)


def test_a_score_below_one_half_is_no_match():
    # IoU 24 / 76 < 0.5: the hypothesis is unmatched, so the Van does not remove it
    out, _, c = frame([(CAR, box(126, 100, 50, 50), 5)], [(VAN, box(100, 100, 50, 50), 0, 0)])
    assert out == [5] and c == counts(rows_in=1, kept=1)


def test_rules_are_checked():
    with pytest.raises(ValueError, match='must differ'):
        PrepRules(2, (2,), 9)
    with pytest.raises(ValueError, match='must differ'):
        PrepRules(2, (4,), 4)


def prep_set():
    """The sequences of the device tests: random ones (shuffled arrival, a late first frame, gaps in the frames) and shaped ones
    -- per frame (matching GT rows, hypotheses): 0 and 1 rows on either side, the lane boundary, tall and wide frames, both sides
    of 1024 pairs, and a frame at the limit of 256 rows."""
    gap = synth_prep_sequence(3, 30, objects=5, t0=3)
    for side in ('det', 'gt'):                                      # frames 10 .. 14 without detections, 12 .. 17 without ground truth
        lo, hi = (10, 14) if side == 'det' else (12, 17)
        keep = (gap[f'{side}_frame'] < lo) | (gap[f'{side}_frame'] > hi)
        for k in list(gap):
            if k.startswith(side) or (side == 'det' and k == 'tracks'):
                gap[k] = gap[k][keep]
    exact = dict(p_untracked=0.0, p_wrong=0.0)
    return [synth_prep_sequence(1, 40, shuffle=True),
            synth_prep_sequence(2, 25, objects=10, distractors=3, regions=3, t0=7, shuffle=True),
            gap,
            synth_prep_sequence(4, 0, objects=4, distractors=2, sizes=[(0, 0), (0, 1), (1, 0), (1, 1), (0, 3), (3, 0), (2, 5), (5, 2)], **exact),
            synth_prep_sequence(5, 0, objects=50, distractors=20, sizes=[(5, 63), (5, 64), (5, 65), (66, 5), (64, 64), (65, 63), (32, 32), (33, 32),
                                                                         (31, 33), (32, 33), (70, 9), (9, 70)], shuffle=True, **exact),
            synth_prep_sequence(6, 0, objects=200, distractors=56, others=0, regions=0, sizes=[(256, 256), (3, 4)], **exact),
            synth_prep_sequence(7, 0, objects=40, distractors=10, sizes=[(50, 90), (20, 20), (50, 37)], shuffle=True)]


@pytest.fixture(scope='module')
def prep_host():
    qs = prep_set()
    return qs, [evalprep_host(q, q['tracks'], KITTI_CAR) for q in qs]


def test_the_device_set_shows_every_branch_on_the_host(prep_host):
    qs, ref = prep_host
    total = {k: sum(r[2][k] for r in ref) for k in COUNT_KEYS}
    for k in REMOVALS + ('other_class', 'kept'):
        assert total[k] > 0, k
    for q, (out, keep, c) in zip(qs, ref):
        assert sum(c[k] for k in COUNT_KEYS[1:]) == c['rows_in'] == int((q['tracks'] >= 0).sum())
        assert c['kept'] == int((out >= 0).sum()) and np.array_equal(out[out >= 0], q['tracks'][out >= 0])
        assert np.array_equal(keep, (q['gt_cat'] == CAR) & (q['gt_occ'] <= 2) & (q['gt_trunc'] <= 0))
    # the shaped frames are what their names say: tracker rows x matching GT rows per frame
    q = qs[4]
    shape = [(int(((q['det_frame'] == t) & (q['tracks'] >= 0) & (q['det_cat'] == CAR)).sum()),
              int(((q['gt_frame'] == t) & np.isin(q['gt_cat'], (CAR, VAN))).sum())) for t in range(12)]
    assert shape[:3] == [(63, 5), (64, 5), (65, 5)] and shape[6:10] == [(32, 32), (32, 33), (33, 31), (33, 32)]
    q = qs[5]
    assert int((q['det_frame'] == 0).sum()) == 256 == int((q['gt_frame'] == 0).sum())


def test_rules_that_switch_everything_off_change_nothing():
    off = PrepRules(CAR, (), None, max_occlusion=10 ** 9, max_truncation=10 ** 9, min_height=-np.inf)
    q = synth_prep_sequence(11, 30, others=0, p_wrong=0.0, shuffle=True)
    out, keep, c = evalprep_host(q, q['tracks'], off)
    assert np.array_equal(out, np.where(q['tracks'] >= 0, q['tracks'], -1)) and c['kept'] == c['rows_in'] > 0
    assert np.array_equal(keep, q['gt_cat'] == CAR)
    out, _, c = evalprep_host(q, q['tracks'], KITTI_CAR)
    assert c['kept'] < c['rows_in']


def test_eval_sequences_drops_exactly_the_rows_outside_gt_keep(prep_host):
    qs, ref = prep_host
    for q, r, (_, keep, _) in zip(qs, prep_eval_sequences(qs, KITTI_CAR), ref):
        assert 0 < keep.sum() < keep.shape[0]
        for k in q:
            assert np.array_equal(r[k], q[k][keep] if k.startswith('gt_') else q[k]), k


def test_evalprep_needs_the_device():
    from trackmpnn_amd import EvalPrep
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        EvalPrep(prep_set()[:1], KITTI_CAR, 'cpu')
