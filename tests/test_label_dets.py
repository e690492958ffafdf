"""GT track ids for detections: the host definition (trackmpnn_amd.labeling.label_frame_host, label_detections_host) against
the recorded results of the reference's get_track_ids (tests/golden/label, tools/gen_label_golden.py), against a brute-force
restatement, and on the cases the reference leaves open or that sit at an edge.  No GPU here; the device is held to the host
definition in tests/test_label_dets_gpu.py."""
import os

import numpy as np
import pytest

from trackmpnn_amd import DetectionStore, _lib
from trackmpnn_amd.labeling import (BDD_RULES, KITTI_RULES, DetectionLabeler, LabelRules, label_detections_host, label_frame_host,
                                    label_overlaps_host, synth_label_sequence)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'label')
FIXTURES = ('label_kitti_a', 'label_kitti_b', 'label_bdd')
RULE_SETS = {'kitti': KITTI_RULES, 'bdd': BDD_RULES}
KEYS = ('det_frame', 'det_cat', 'det_box', 'det_score', 'gt_frame', 'gt_track', 'gt_cat', 'gt_box')
Z = [5, 5, 4, 4]                                                  # zero area in the "+1" form: every overlap with it is 0 / 0


def load_fixture(name):
    """(the sequence, its rules, the reference's results)"""
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    q = {k: z[k] for k in KEYS}
    q.update(num_frames=int(z['num_frames']), width=int(z['width']))
    return q, RULE_SETS[str(z['rules'])], {k: z['ref_' + k] for k in ('keep', 'track', 'gt_keep')}


def frame(det, gt, num_frames=1, width=1242):
    """A one-frame sequence from rows (cat, box) and (track, cat, box)."""
    return {'det_frame': np.zeros(len(det), np.int64), 'det_cat': np.asarray([c for c, _ in det], np.int64),
            'det_box': np.asarray([b for _, b in det], np.float32).reshape(-1, 4), 'det_score': np.linspace(0.1, 0.9, len(det)),
            'gt_frame': np.zeros(len(gt), np.int64), 'gt_track': np.asarray([t for t, _, _ in gt], np.int64),
            'gt_cat': np.asarray([c for _, c, _ in gt], np.int64), 'gt_box': np.asarray([b for _, _, b in gt], np.float32).reshape(-1, 4),
            'num_frames': num_frames, 'width': width}


def label1(q, rules=KITTI_RULES):
    return label_frame_host(q['det_cat'], q['det_box'], q['gt_track'], q['gt_cat'], q['gt_box'], rules)


def brute_force(det_cat, det_box, gt_track, gt_cat, gt_box, rules):
    """The rule once more, pair by pair in Python: every eligible pair in a list, sorted by (-IoU, flat index), walked."""
    P, G = len(det_cat), len(gt_cat)
    real = [g for g in range(G) if gt_cat[g] not in (rules.iom_ignore_cat, rules.iou_ignore_cat)]
    gt_keep = np.asarray([g in real for g in range(G)], bool)
    track, keep = np.full(P, -1, np.int64), np.ones(P, bool)
    iou, iom = label_overlaps_host(det_box, gt_box)
    pairs = [(-float(iou[p, g]), p * len(real) + k, p, g) for p in range(P) for k, g in enumerate(real)
             if iou[p, g] >= np.float32(rules.iou_thresh) and det_cat[p] == gt_cat[g]]
    used = set()
    for _, _, p, g in sorted(pairs):
        if track[p] < 0 and g not in used:
            track[p] = gt_track[g]
            used.add(g)
    for p in range(P):
        if track[p] >= 0:
            continue
        a = [iom[p, g] for g in range(G) if gt_cat[g] == rules.iom_ignore_cat]
        b = [iou[p, g] for g in range(G) if gt_cat[g] == rules.iou_ignore_cat and gt_cat[g] != rules.iom_ignore_cat]
        if (a and not np.isnan(a).any() and max(a) >= np.float32(rules.iom_thresh)) or \
                (b and not np.isnan(b).any() and max(b) >= np.float32(rules.iou_thresh)):
            keep[p] = False
    return track, keep, gt_keep


# ---- frames shared with the device tests: name -> (sequence, rules)
def tie_frame():
    """Duplicate detection boxes and duplicate GT boxes: every IoU of the matching is 1."""
    b = [100, 100, 149, 179]
    return frame([(1, b), (1, b), (1, b), (2, b)], [(7, 1, b), (8, 1, b), (9, 2, b), (10, 2, b)])


def nan_frame():
    return frame([(1, Z), (1, [10, 10, 59, 59]), (1, [12, 10, 61, 59]), (1, [300, 10, 349, 59])],
                 [(-1, 9, Z), (-1, 9, [0, 0, 99, 99]), (5, 4, [300, 10, 349, 59]), (6, 4, Z), (3, 1, Z)])


def chain_frame(n=30):
    """2 n - 1 boxes of width 100 in a row, GT rows and detections alternating, the gap to the next box shrinking towards the
    right (from 26 to 18 pixels: neighbours overlap by more than half, boxes two apart by less).  So every box's best partner
    is its right neighbour and only the rightmost pair is mutual: the rounds of the device accept one pair each, from the right.
    The sorted walk takes every second edge: detection i gets the GT row to its right."""
    x = np.concatenate([[0.0], np.cumsum(np.linspace(26.0, 18.0, 2 * n - 2))])
    box = [[v, 0, v + 99, 99] for v in x]
    return frame([(1, b) for b in box[1::2]], [(i, 1, b) for i, b in enumerate(box[0::2])])


def special_frames():
    return {'tie': tie_frame(), 'nan': nan_frame(), 'chain_wave': chain_frame(30), 'chain_workgroup': chain_frame(70)}


def test_chain_frame_is_what_it_says():
    for n in (30, 70):
        q = chain_frame(n)
        iou = label_overlaps_host(q['det_box'], q['gt_box'])[0]
        right, left = iou[np.arange(n - 1), np.arange(1, n)], iou[np.arange(n - 1), np.arange(n - 1)]
        assert (np.diff(np.stack([left, right], 1).ravel()) > 0).all() and left.min() >= 0.5       # strictly rising to the right
        assert ((iou >= 0.5).sum(1) == 2).all()
        track, keep, gt_keep = label1(q)
        assert track.tolist() == list(range(1, n)) and keep.all() and gt_keep.all()


@pytest.mark.parametrize('name', FIXTURES)
def test_host_equals_the_reference(name):
    q, rules, ref = load_fixture(name)
    out = label_detections_host([q], rules)[0]
    assert np.array_equal(out['keep'], ref['keep'])
    assert np.array_equal(out['gt_keep'], ref['gt_keep'])
    assert np.array_equal(out['track'][ref['keep']], ref['track'][ref['keep']])
    n = ref['keep'].shape[0]                                      # all three outcomes in number
    for share in ((ref['track'] >= 0).sum() / n, (ref['keep'] & (ref['track'] < 0)).sum() / n, (~ref['keep']).sum() / n):
        assert 0.1 < share < 0.9


@pytest.mark.parametrize('rules', [KITTI_RULES, BDD_RULES, LabelRules(9, 4, 0.3, 0.6)])
def test_host_equals_brute_force(rules):
    q = synth_label_sequence(5, 30, rules, max_det=20, max_gt=14)
    q['det_box'], q['gt_box'] = np.round(q['det_box'] / 8) * 8, np.round(q['gt_box'] / 8) * 8      # (a coarse grid: ties occur)
    ties = 0
    for t in range(q['num_frames']):
        d, g = q['det_frame'] == t, q['gt_frame'] == t
        args = (q['det_cat'][d], q['det_box'][d], q['gt_track'][g], q['gt_cat'][g], q['gt_box'][g], rules)
        for a, b in zip(label_frame_host(*args), brute_force(*args)):
            assert np.array_equal(a, b)
        v = label_overlaps_host(q['det_box'][d], q['gt_box'][g])[0].ravel()
        v = v[v >= rules.iou_thresh]
        ties += v.shape[0] - np.unique(v).shape[0]
    assert ties > 0


def test_stated_tie_order():
    track, keep, gt_keep = label1(tie_frame())
    # flat index p * G' + g ascending: detection 0 takes the first row of its class, detection 1 the second, detection 2 none
    assert track.tolist() == [7, 8, -1, 9] and keep.all() and gt_keep.all()
    b = [0, 0, 9, 9]
    # one GT row, two identical detections: the first gets it
    assert label1(frame([(1, b), (1, b)], [(4, 1, b)]))[0].tolist() == [4, -1]
    # one detection, two identical GT rows: the first is taken
    assert label1(frame([(1, b)], [(4, 1, b), (5, 1, b)]))[0].tolist() == [4]


def test_threshold_edges():
    iou = label_overlaps_host([[1000, 0, 1009, 9]], [[1000, 0, 1004, 9], [1000, 0, 1004, 8]])[0][0]
    assert iou[0] == np.float32(0.5) and iou[1] < np.float32(0.5)
    q = frame([(1, [1000, 0, 1009, 9])], [(3, 1, [1000, 0, 1004, 9])])
    assert label1(q)[0].tolist() == [3]                           # exactly 0.5 passes
    q = frame([(1, [1000, 0, 1009, 9])], [(3, 1, [1000, 0, 1004, 8])])
    assert label1(q)[0].tolist() == [-1]                          # just below does not
    # the same edge for the removal by IoU (a Van) and a removal by IoM: [0,0,9,9] in [0,0,99,99] has IoM 1, a quarter inside 0.25
    assert label1(frame([(1, [1000, 0, 1009, 9])], [(3, 4, [1000, 0, 1004, 9])]))[1].tolist() == [False]
    assert label1(frame([(1, [1000, 0, 1009, 9])], [(3, 4, [1000, 0, 1004, 8])]))[1].tolist() == [True]
    assert label1(frame([(1, [0, 0, 9, 9]), (1, [95, 95, 104, 104])], [(-1, 9, [0, 0, 99, 99])]))[1].tolist() == [False, True]
    # IoM exactly at 0.8: 8 of 10 columns inside
    assert label_overlaps_host([[92, 0, 101, 9]], [[0, 0, 99, 99]])[1][0, 0] == np.float32(0.8)
    assert label1(frame([(1, [92, 0, 101, 9]), (1, [93, 0, 102, 9])], [(-1, 9, [0, 0, 99, 99])]))[1].tolist() == [False, True]


def test_nan_rows_keep_the_detection():
    q = nan_frame()
    iou, iom = label_overlaps_host(q['det_box'], q['gt_box'])
    assert np.isnan(iom[:, 0]).all() and np.isnan(iom[:, 3]).all() and np.isnan(iou[0, [0, 3, 4]]).all()
    track, keep, gt_keep = label1(q)
    # detections 1 and 2 lie inside the DontCare box [0,0,99,99], but the zero-area DontCare row makes every IoM row's maximum
    # NaN, which passes no >=: they stay, as in the reference.  Detection 0 (zero area) has a NaN in its Van row too and stays;
    # detection 3 sits on the Van with a NaN-free IoU row and goes.  A NaN IoU matches nobody.
    assert track.tolist() == [-1, -1, -1, -1] and keep.tolist() == [True, True, True, False]
    assert gt_keep.tolist() == [False, False, False, False, True]
    # without the zero-area rows the same detections go
    q2 = frame([(1, [10, 10, 59, 59]), (1, [300, 10, 349, 59])], [(-1, 9, [0, 0, 99, 99]), (5, 4, [300, 10, 349, 59])])
    assert label1(q2)[1].tolist() == [False, False]
    # a NaN overlap never matches
    assert label1(frame([(1, Z)], [(3, 1, Z)]))[0].tolist() == [-1]


def test_empty_sides():
    b = [0, 0, 9, 9]
    track, keep, gt_keep = label1(frame([(1, b), (2, b)], []))
    assert track.tolist() == [-1, -1] and keep.all() and gt_keep.shape == (0,)
    track, keep, gt_keep = label1(frame([], [(1, 1, b), (-1, 9, b), (2, 4, b)]))
    assert track.shape == (0,) and keep.shape == (0,) and gt_keep.tolist() == [True, False, False]
    out = label_detections_host([frame([], [])], KITTI_RULES)[0]
    assert out['track'].shape == out['keep'].shape == out['gt_keep'].shape == (0,)
    assert label1(frame([(1, b)], [(3, 1, b)]), BDD_RULES)[0].tolist() == [3]
    assert label1(frame([(1, b)], [(3, 9, b)]), BDD_RULES)[1].tolist() == [False]       # (9 is the distractor there)


def test_wrong_class_pair_does_not_consume_its_gt():
    a, b = [0, 0, 99, 99], [0, 0, 99, 89]
    # detection 0 (class 2) overlaps the class-1 row perfectly, detection 1 (class 1) a little less: the row goes to detection 1
    track, keep, _ = label1(frame([(2, a), (1, b)], [(11, 1, a)]))
    assert track.tolist() == [-1, 11] and keep.all()


def test_assigned_detection_in_an_ignore_region_stays():
    a = [10, 10, 59, 59]
    track, keep, gt_keep = label1(frame([(1, a), (1, [12, 10, 61, 59])], [(-1, 9, [0, 0, 99, 99]), (4, 1, a), (8, 4, a)]))
    assert track.tolist() == [4, -1] and keep.tolist() == [True, False] and gt_keep.tolist() == [False, True, False]


def test_sequences_in_any_row_order():
    q, rules, _ = load_fixture('label_kitti_a')
    rng = np.random.default_rng(3)
    # the frames in a random order; within a frame the rows keep their order (the tie order depends on it)
    pd = np.concatenate([np.where(q['det_frame'] == t)[0] for t in rng.permutation(q['num_frames'])])
    pg = np.concatenate([np.where(q['gt_frame'] == t)[0] for t in rng.permutation(q['num_frames'])])
    q2 = dict(q)
    for k in KEYS:
        q2[k] = q[k][pd] if k.startswith('det') else q[k][pg]
    a, b = label_detections_host([q], rules)[0], label_detections_host([q2], rules)[0]
    assert np.array_equal(a['track'][pd], b['track']) and np.array_equal(a['keep'][pd], b['keep'])
    assert np.array_equal(a['gt_keep'][pg], b['gt_keep'])


def test_constructor_value_errors():
    b = [0, 0, 9, 9]
    good = frame([(1, b)], [(3, 1, b)])
    DetectionLabeler([good], KITTI_RULES, device=None)

    def bad(**kw):
        q = dict(good)
        q.update(kw)
        with pytest.raises(ValueError):
            DetectionLabeler([q], KITTI_RULES, device=None)
    bad(det_frame=np.zeros(1, np.float32))                        # integer frames and categories
    bad(det_cat=np.ones(1, np.float64))
    bad(gt_cat=np.ones(1, np.float32))
    bad(gt_frame=np.zeros(1, np.float64))
    bad(gt_track=np.zeros(1, np.float64))
    bad(det_box=np.float32([[0, 0, np.inf, 9]]))                  # finite boxes and scores
    bad(gt_box=np.float32([[0, np.nan, 9, 9]]))
    bad(det_score=np.float32([np.nan]))
    bad(det_frame=np.ones(1, np.int64))                           # frames inside [0, num_frames)
    bad(gt_frame=-np.ones(1, np.int64))
    bad(num_frames=0)
    bad(det_cat=np.ones(2, np.int64))                             # equal lengths
    bad(det_score=np.zeros(2))
    bad(gt_track=np.zeros(2, np.int64))
    bad(gt_box=np.zeros((2, 4), np.float32))
    bad(gt_track=-np.ones(1, np.int64))                           # a matchable row needs an id
    with pytest.raises(ValueError):
        DetectionLabeler([], KITTI_RULES, device=None)
    with pytest.raises(ValueError):
        DetectionLabeler([good], (9, 4), device=None)
    with pytest.raises(ValueError):
        label_detections_host([dict(good, gt_track=-np.ones(1, np.int64))], KITTI_RULES)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        DetectionLabeler([good], KITTI_RULES, device='cpu')
    with pytest.raises(RuntimeError, match='no labelling'):
        DetectionLabeler([good], KITTI_RULES, device=None).read()


def test_store_sequences_feed_the_detection_store():
    (q, rules, ref), (q2, _, ref2) = load_fixture('label_kitti_a'), load_fixture('label_kitti_b')
    q = dict(q, det_box=q['det_box'].astype(np.float64) + 0.001)  # (float64 boxes are handed on as they are)
    lb = DetectionLabeler([q, q2], rules, device=None)
    lb.label()
    host = label_detections_host([q, q2], rules)
    for a, b in zip(lb.read(), host):
        assert all(np.array_equal(a[k], b[k]) for k in ('track', 'keep', 'gt_keep'))
    ss, es = lb.store_sequences(), lb.eval_sequences()
    for s, e, src, h in zip(ss, es, (q, q2), host):
        k = h['keep']
        assert np.array_equal(s['frame'], src['det_frame'][k]) and np.array_equal(s['track'], h['track'][k])
        assert np.array_equal(s['cat'], src['det_cat'][k]) and np.array_equal(s['box'], src['det_box'][k])
        assert s['box'].dtype == src['det_box'].dtype and np.array_equal(s['score'], src['det_score'][k])
        assert s['num_frames'] == src['num_frames'] and s['width'] == src['width']
        assert np.array_equal(e['det_box'], src['det_box'][k].astype(np.float32)) and np.array_equal(e['det_frame'], s['frame'])
        g = h['gt_keep']
        assert np.array_equal(e['gt_track'], src['gt_track'][g]) and np.array_equal(e['gt_box'], src['gt_box'][g])
        assert np.array_equal(e['gt_cat'], src['gt_cat'][g]) and np.array_equal(e['gt_frame'], src['gt_frame'][g])
        assert not np.isin(e['gt_cat'], (rules.iom_ignore_cat, rules.iou_ignore_cat)).any()
    store = DetectionStore(ss, 3, '2d+temp', np.zeros(10), np.ones(10), device=None)
    assert store.ndets == sum(int(h['keep'].sum()) for h in host) and store.nseq == 2
    assert np.array_equal(store.track, np.concatenate([s['track'] for s in ss]).astype(np.int32))


def test_argument_validation_needs_no_gpu():
    """Bad arguments are rejected on the host before any launch."""
    import ctypes as C
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.tmpnn_label_max_per_frame() == 256 and lib.tmpnn_label_wave_frame() == 64
    for fn in (lib.tmpnn_label_dets, lib.tmpnn_label_compact):
        assert fn(None, None, None) == -1 and b'null' in lib.tmpnn_last_error()
        out = _lib.CLabelOut()
        st = _lib.CLabelStore(1, 0, 3, 0, 0, 9, 4, 0.5, 0.8, 1, 1)                  # the lists hold 2 of 3 frames
        assert fn(C.byref(st), C.byref(out), None) == -1 and b'frame lists' in lib.tmpnn_last_error()
        st = _lib.CLabelStore(1, 0, 3, 0, 0, 9, 4, 0.5, 0.8, 3, 0)                  # no tables
        assert fn(C.byref(st), C.byref(out), None) == -1 and b'null frame tables' in lib.tmpnn_last_error()
        st = _lib.CLabelStore(1, 0, 2 ** 31, 0, 0, 9, 4, 0.5, 0.8, 2 ** 31, 0)
        assert fn(C.byref(st), C.byref(out), None) == -1 and b'int32' in lib.tmpnn_last_error()
        st = _lib.CLabelStore(1, 0, 3, 0, 0, 9, 4, float('nan'), 0.8, 3, 0)
        assert fn(C.byref(st), C.byref(out), None) == -1 and b'NaN' in lib.tmpnn_last_error()
