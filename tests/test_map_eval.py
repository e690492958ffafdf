"""The validation mAP on the host (trackmpnn_amd.mapeval: map_host, map_best_host, MapStore): the recorded results of the
reference's compute_map (tests/golden/map/map_*.npz, tools/gen_map_golden.py), one hand-made case per quirk of the rule, the
store's route (fixed best rows, claim lists, per-class order: what the device runs) against the definition, input errors."""
import glob
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN_DIR
from trackmpnn_amd import _lib
from trackmpnn_amd.mapeval import MapEvaluator, MapStore, map_best_host, map_host, map_iou_host, synth_map_sequence

KEYS = ('det_frame', 'det_box', 'det_cat', 'det_score', 'gt_frame', 'gt_box', 'gt_cat', 'gt_track', 'tracks')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'map', 'map_*.npz')))


def load_fixture(path):
    """(sequences, tracks with None for the sequence left out, reference mAP, largest per-class true-positive count)"""
    d = np.load(path)
    seqs = [{k: d[f's{s}_{k}'] for k in KEYS} for s in range(int(d['n_seq']))]
    tracks = [None if s == int(d['left_out']) else q['tracks'] for s, q in enumerate(seqs)]
    return seqs, tracks, float(d['map_ref']), int(d['max_tp'])


def fixture_bound(max_tp, classes):
    """Two different summation orders over non-negative terms that sum to at most 1: per class at most max_tp terms (the
    reference adds them pairwise, the rule one at a time), then the classes (the reference adds them in the order of their
    names as strings); each order is within (terms) * 2^-53 of the exact sum."""
    return 2 * (max_tp + classes) * 2.0 ** -53


def seq(det, gt):
    """det: rows (frame, cat, score, x1, y1, x2, y2), gt: rows (frame, cat, x1, y1, x2, y2)"""
    det, gt = np.asarray(det, np.float64).reshape(-1, 7), np.asarray(gt, np.float64).reshape(-1, 6)
    return {'det_frame': det[:, 0].astype(np.int64), 'det_cat': det[:, 1].astype(np.int64), 'det_score': det[:, 2].astype(np.float32),
            'det_box': det[:, 3:].astype(np.float32), 'gt_frame': gt[:, 0].astype(np.int64), 'gt_cat': gt[:, 1].astype(np.int64),
            'gt_box': gt[:, 2:].astype(np.float32), 'gt_track': np.arange(gt.shape[0], dtype=np.int64)}


def all_tracked(q):
    return np.arange(q['det_frame'].shape[0], dtype=np.int64)


def store_route(seqs, tracks):
    """What the device computes, restated on the store's arrays: first kept claimant per GT row, then per class the counts,
    the envelope and the ordered sum."""
    from trackmpnn_amd.mapeval import _average_precision, _mean
    st = MapStore(seqs)
    st.set_best(st.best_host())
    tr = np.full(st.n_det, -1, np.int64)
    for s, t in enumerate(tracks):
        if t is not None:
            tr[st.det_base[s]:st.det_base[s + 1]] = t
    mark = np.zeros(st.n_det, bool)
    for g in range(st.n_gt):
        for d in st.claim_det[st.claim_off[g]:st.claim_off[g + 1]]:
            if tr[d] >= 0:
                mark[d] = True
                break
    out = {'classes': [], 'ap': [], 'annotations': [], 'kept': [], 'true_positives': []}
    for c in range(st.C):
        rows = st.gt_seq[st.cls_gt_off[c]:st.cls_gt_off[c + 1]]
        n = int(sum(tracks[s] is not None for s in rows))
        if n == 0:
            continue
        lst = st.order[st.cls_off[c]:st.cls_off[c + 1]]
        lst = lst[tr[lst] >= 0]
        tp = (mark[lst] & (st.det_best[lst] >= 0)).astype(np.int64)
        for k, v in zip(('classes', 'ap', 'annotations', 'kept', 'true_positives'),
                        (st.classes[c], _average_precision(tp, n), n, int(lst.shape[0]), int(tp.sum()))):
            out[k].append(v)
    out['map'] = _mean(out['ap'])
    return out


def same(a, b):
    return (all(a[k] == b[k] for k in ('classes', 'annotations', 'kept', 'true_positives'))
            and [np.float64(x).view(np.int64) for x in a['ap']] == [np.float64(x).view(np.int64) for x in b['ap']]
            and (np.float64(a['map']).view(np.int64) == np.float64(b['map']).view(np.int64)))


def test_fixtures_exist():
    assert 2 <= len(FIXTURES) <= 3 and all(os.path.getsize(p) < 100_000 for p in FIXTURES)


@pytest.mark.parametrize('path', FIXTURES, ids=os.path.basename)
def test_map_host_reproduces_the_reference(path):
    seqs, tracks, ref, max_tp = load_fixture(path)
    r = map_host(seqs, tracks)
    assert max(r['true_positives']) == max_tp
    bound = fixture_bound(max_tp, len(r['classes']))
    print(f'{os.path.basename(path)}: map_host {r["map"]!r}, reference {ref!r}, |diff| {abs(r["map"] - ref):.3e}, bound {bound:.3e}')
    assert abs(r['map'] - ref) <= bound


@pytest.mark.parametrize('path', FIXTURES, ids=os.path.basename)
def test_fixture_content(path):
    seqs, tracks, _, _ = load_fixture(path)
    r = map_host(seqs, tracks)
    assert len(r['classes']) == 3
    for tp, kept in zip(r['true_positives'], r['kept']):
        assert 0.2 < tp / kept < 0.9
    dup = no_gt_frame = alien = untracked = 0
    for q, tr in zip(seqs, tracks):
        if tr is None:
            continue
        untracked += int((tr < 0).sum())
        alien += int((~np.isin(q['det_cat'], r['classes']) & (tr >= 0)).sum())
        no_gt_frame += int((~np.isin(q['det_frame'], q['gt_frame']) & (tr >= 0)).sum())
        claimed = []
        for i in np.where(tr >= 0)[0]:
            g = np.where((q['gt_frame'] == q['det_frame'][i]) & (q['gt_cat'] == q['det_cat'][i]))[0]
            j = int(map_best_host(q['det_box'][i:i + 1], q['gt_box'][g])[0])
            if j >= 0:
                claimed.append(int(g[j]))
        dup += len(claimed) - len(set(claimed))
    assert dup >= 1 and no_gt_frame >= 1 and alien >= 1 and untracked >= 1


@pytest.mark.parametrize('path', FIXTURES, ids=os.path.basename)
def test_store_route_equals_the_definition_on_the_fixtures(path):
    seqs, tracks, _, _ = load_fixture(path)
    assert same(store_route(seqs, tracks), map_host(seqs, tracks))


@pytest.mark.parametrize('ties', [False, True])
def test_store_route_equals_the_definition(ties):
    seqs = [synth_map_sequence(300 + i, L, ties=ties) for i, L in enumerate((1, 2, 3, 40, 65))]
    tracks = [q['tracks'] for q in seqs]
    ref = map_host(seqs, tracks)
    assert same(store_route(seqs, tracks), ref) and sum(ref['true_positives']) > 100
    tracks[3] = None                                              # a sequence left out, other tracks in another
    tracks[4] = np.where(np.arange(tracks[4].shape[0]) % 3 == 0, -1, tracks[4])
    ref2 = map_host(seqs, tracks)
    assert same(store_route(seqs, tracks), ref2) and ref2['annotations'] != ref['annotations']


# ---- one hand-made case per quirk ------------------------------------------------------------------------------------------------

def test_iou_of_exactly_one_half_is_a_true_positive():
    # "+1" form: (0, 0, 9, 9) is 10 x 10, (0, 0, 4, 9) is 5 x 10: 50 / (100 + 50 - 50)
    assert map_iou_host([[0, 0, 9, 9]], [[0, 0, 4, 9]])[0, 0] == 0.5
    q = seq([(0, 1, 0.9, 0, 0, 9, 9)], [(0, 1, 0, 0, 4, 9)])
    r = map_host([q], [all_tracked(q)])
    assert r['true_positives'] == [1] and r['ap'] == [1.0] and r['map'] == 1.0
    q = seq([(0, 1, 0.9, 0, 0, 9, 9)], [(0, 1, 0, 0, 4, 8)])        # just below: 45 / 100
    r = map_host([q], [all_tracked(q)])
    assert r['true_positives'] == [0] and r['ap'] == [0.0]


def test_a_second_claimant_is_a_false_positive_and_never_tries_the_second_best_box():
    # both detections overlap GT row 0 most; the second also overlaps GT row 1 by more than one half
    gt = [(0, 1, 0, 0, 99, 99), (0, 1, 20, 0, 119, 99)]
    det = [(0, 1, 0.9, 0, 0, 99, 99), (0, 1, 0.8, 9, 0, 108, 99)]
    q = seq(det, gt)
    iou = map_iou_host(q['det_box'][1:], q['gt_box'])[0]
    assert iou[0] > iou[1] >= 0.5
    r = map_host([q], [all_tracked(q)])
    assert r['kept'] == [2] and r['true_positives'] == [1] and r['annotations'] == [2]
    assert r['ap'] == [0.5]                                       # recall 1/2 at precision 1
    # with the first claimant untracked the second is the first KEPT claimant
    r = map_host([q], [np.array([-1, 5])])
    assert r['kept'] == [1] and r['true_positives'] == [1]
    assert same(store_route([q], [np.array([-1, 5])]), r)


def test_a_class_mismatch_does_not_match():
    q = seq([(0, 2, 0.9, 0, 0, 9, 9)], [(0, 1, 0, 0, 9, 9), (1, 2, 0, 0, 9, 9)])
    r = map_host([q], [all_tracked(q)])
    assert r['classes'] == [1, 2] and r['kept'] == [0, 1] and r['true_positives'] == [0, 0] and r['map'] == 0.0


def test_a_detection_in_a_frame_without_gt_or_of_a_class_without_gt_is_ignored():
    q = seq([(0, 1, 0.9, 0, 0, 9, 9), (5, 1, 0.95, 0, 0, 9, 9), (0, 7, 0.99, 0, 0, 9, 9)], [(0, 1, 0, 0, 9, 9)])
    r = map_host([q], [all_tracked(q)])
    assert r['classes'] == [1] and r['kept'] == [1] and r['ap'] == [1.0]


def test_the_gt_of_a_sequence_left_out_is_not_counted():
    a = seq([(0, 1, 0.9, 0, 0, 9, 9)], [(0, 1, 0, 0, 9, 9)])
    b = seq([(0, 1, 0.8, 0, 0, 9, 9)], [(0, 1, 50, 50, 59, 59), (0, 2, 0, 0, 9, 9), (1, 1, 0, 0, 9, 9)])
    both = map_host([a, b], [all_tracked(a), all_tracked(b)])
    assert both['classes'] == [1, 2] and both['annotations'] == [3, 1] and both['ap'][0] == 1.0 / 3.0
    one = map_host([a, b], [all_tracked(a), None])
    assert one['classes'] == [1] and one['annotations'] == [1] and one['map'] == 1.0
    assert same(store_route([a, b], [all_tracked(a), None]), one)


def test_ties_in_score_keep_the_natural_order():
    # equal scores: a false positive that ARRIVES first ranks first, in the first sequence before the second
    fp, tp = (0, 1, 0.5, 500, 500, 509, 509), (0, 1, 0.5, 0, 0, 9, 9)
    gt = [(0, 1, 0, 0, 9, 9)]
    q1, q2 = seq([fp, tp], gt), seq([tp, fp], gt)
    assert map_host([q1], [all_tracked(q1)])['ap'] == [0.5]       # ranks: FP, TP -> precision 1/2 at recall 1
    assert map_host([q2], [all_tracked(q2)])['ap'] == [1.0]
    a, b = seq([fp], gt), seq([tp], gt)
    assert map_host([a, b], [all_tracked(a), all_tracked(b)])['ap'] == [0.25]      # FP, TP of two annotations
    assert map_host([b, a], [all_tracked(b), all_tracked(a)])['ap'] == [0.5]
    for s in ([q1], [q2], [a, b], [b, a]):
        t = [all_tracked(q) for q in s]
        assert same(store_route(s, t), map_host(s, t))


def test_a_class_without_a_kept_detection_has_ap_zero():
    q = seq([(0, 1, 0.9, 0, 0, 9, 9), (0, 2, 0.9, 30, 30, 39, 39)], [(0, 1, 0, 0, 9, 9), (0, 2, 30, 30, 39, 39)])
    r = map_host([q], [np.array([4, -1])])
    assert r['classes'] == [1, 2] and r['kept'] == [1, 0] and r['ap'] == [1.0, 0.0] and r['map'] == 0.5
    assert same(store_route([q], [np.array([4, -1])]), r)


def test_no_gt_gives_nan():
    q = seq([(0, 1, 0.9, 0, 0, 9, 9)], [])
    r = map_host([q], [all_tracked(q)])
    assert r['classes'] == [] and np.isnan(r['map'])
    q2 = seq([(0, 1, 0.9, 0, 0, 9, 9)], [(0, 1, 0, 0, 9, 9)])
    assert np.isnan(map_host([q2], [None])['map'])


def test_best_row_is_the_first_maximum_and_nan_counts_as_one():
    det = np.float32([[0, 0, 9, 9]])
    assert list(map_best_host(det, np.float32([[0, 0, 9, 8], [0, 0, 9, 9], [0, 0, 9, 9]]))) == [1]
    assert list(map_best_host(det, np.zeros((0, 4), np.float32))) == [-1]
    # zero area in the "+1" form on both sides: 0 / 0 = NaN wins the argmax and fails the test
    z = np.float32([[5, 5, 4, 4]])
    assert np.isnan(map_iou_host(z, z)[0, 0])
    assert list(map_best_host(z, np.float32([[5, 5, 4, 4], [5, 5, 4, 4]]))) == [-1]


# ---- errors, ABI -------------------------------------------------------------------------------------------------------------------

def test_bad_input_raises_value_error():
    q = seq([(0, 1, 0.9, 0, 0, 9, 9)], [(0, 1, 0, 0, 9, 9)])
    for key, val in (('det_cat', np.array([1.0])), ('gt_cat', np.array([1.5])), ('det_score', np.array([np.nan], np.float32)),
                     ('det_score', np.array([np.inf], np.float32)), ('det_box', np.float32([[0, 0, np.inf, 9]])),
                     ('gt_box', np.float32([[0, np.nan, 9, 9]])), ('det_score', np.zeros(2, np.float32)),
                     ('det_cat', np.array([1, 2])), ('gt_box', np.zeros((2, 4), np.float32))):
        bad = dict(q, **{key: val})
        with pytest.raises(ValueError):
            MapStore([bad])
        with pytest.raises(ValueError):
            map_host([bad], [all_tracked(q)])
    with pytest.raises(ValueError):
        map_host([q], [])
    with pytest.raises(ValueError):
        map_host([q], [np.array([1, 2])])
    with pytest.raises(ValueError):
        map_host([q], [np.array([0.5])])
    st = MapStore([q])
    with pytest.raises(ValueError):
        st.set_best(np.array([1]))                                # (one GT row: index 1 is out of range)


def test_a_host_device_is_refused():
    q = seq([(0, 1, 0.9, 0, 0, 9, 9)], [(0, 1, 0, 0, 9, 9)])
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        MapEvaluator([q], 'cpu')


def test_abi_version_and_entry_points():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 13 and lib.tmpnn_abi_version() == 13
    assert lib.tmpnn_map_tile() >= 64
    assert lib.tmpnn_map_eval_ws(10, 20, 15) >= 20 + 10 + 15 * 12 and lib.tmpnn_map_eval_ws(-1, 0, 0) == 0
    assert lib.tmpnn_map_best(None, None, None) == -1 and b'store is null' in lib.tmpnn_last_error()
    st = _lib.CMapStore(1, 1, 1, 1, 1, 1, 1)                      # null arrays: rejected on the host before any launch
    assert lib.tmpnn_map_eval(st, None, None, None, 0, None, None) == -1
