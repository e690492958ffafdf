"""The host definition of the result filter and the result tables (trackmpnn_amd.results: results_host, kitti_lines_host,
bdd_document_host) against what the reference's store_kitti_results / store_bdd100k_results recorded
(tests/golden/results, tools/gen_results_golden.py), and the rule's edges by hand.  No GPU."""
import glob
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN_DIR
from trackmpnn_amd.results import (BDD_RESULT_RULES, COUNT_KEYS, KITTI_RESULT_RULES, ResultRules, ResultStore, bbox_pred_of,
                                   bdd_document_host, kitti_lines_host, results_host, score_keys, synth_result_sequence)

RULE_SETS = {'kitti': KITTI_RESULT_RULES, 'bdd': BDD_RESULT_RULES}
SEQ_KEYS = ('det_frame', 'det_cat', 'det_score', 'det_box', 'det_alpha', 'det_dim', 'det_loc', 'det_rot')
SEVEN = np.float32(0.7)
BELOW = np.nextafter(SEVEN, np.float32(0))


def fixture_names():
    return sorted(os.path.basename(f)[len('results_'):-4] for f in glob.glob(os.path.join(GOLDEN_DIR, 'results', 'results_*.npz')))


def load_fixture(name):
    """(sequence dict with 'tracks' = the ids before the filter, rules, the npz)"""
    z = np.load(os.path.join(GOLDEN_DIR, 'results', f'results_{name}.npz'))
    q = {k: z[k] for k in SEQ_KEYS if k in z.files}
    q['tracks'] = z['y_in'][:, 1]
    return q, RULE_SETS[str(z['rules'])], z


def sequence(frame, cat, score, **kw):
    n = len(frame)
    return dict(det_frame=np.asarray(frame, np.int64), det_cat=np.asarray(cat, np.int64), det_score=np.asarray(score, np.float32),
                det_box=np.arange(4 * n, dtype=np.float32).reshape(n, 4), **kw)


def test_the_fixtures_are_what_the_issue_asks_for():
    names = fixture_names()
    assert {'kitti_mixed', 'kitti_boundary', 'kitti_gaps', 'bdd'} <= set(names) and len(names) >= 4
    for name in names:
        q, rules, z = load_fixture(name)
        assert 0 < q['det_frame'].shape[0] <= 200 and z['bbox_pred'].shape == (q['det_frame'].shape[0], 14)
        assert z['bbox_pred'].dtype == np.float32 and np.array_equal(z['bbox_pred'], bbox_pred_of(q, rules))
    q, _, z = load_fixture('kitti_mixed')                           # tracks whose rows mix categories: the maximum decides
    sets = {tuple(sorted(set(q['det_cat'][q['tracks'] == t].tolist()))) for t in np.unique(q['tracks'][q['tracks'] >= 0])}
    assert {(1, 2), (2, 3)} <= sets
    q, _, z = load_fixture('kitti_boundary')                        # Car tracks at, just below and above the threshold
    best = {}
    for t in np.unique(q['tracks'][q['tracks'] >= 0]):
        rows = q['tracks'] == t
        if q['det_cat'][rows].max() == 2:
            best.setdefault(q['det_score'][rows].max(), []).append(bool((z['y_out'][rows, 1] == -1).all()))
    assert best[SEVEN] and not any(best[SEVEN]) and best[BELOW] and all(best[BELOW])
    assert any(s > SEVEN for s in best) and any(s < BELOW for s in best)
    q, _, _ = load_fixture('kitti_gaps')                            # unsorted arrival, gaps, a first frame that is not 0
    fr = q['det_frame']
    assert fr.min() > 0 and (np.diff(fr) < 0).any() and np.unique(fr).shape[0] < fr.max() - fr.min() + 1


@pytest.mark.parametrize('name', fixture_names())
def test_host_functions_reproduce_the_reference(name):
    q, rules, z = load_fixture(name)
    res = results_host(q, q['tracks'], rules)
    assert np.array_equal(res['tracks'], z['y_out'][:, 1])          # the mutated y_out, exactly
    assert res['t_range'] == (int(z['y_in'][:, 0].min()), int(z['y_in'][:, 0].max()))
    kept = z['y_out'][:, 1] != -1
    assert res['order'].dtype == np.int32 and res['kept_rows'] == int(kept.sum()) == res['order'].shape[0]
    assert np.array_equal(np.sort(res['order']), np.where(kept)[0]) and (np.diff(q['det_frame'][res['order']]) >= 0).all()
    gone = (q['tracks'] >= 0) & ~kept
    assert res['removed_rows'] == int(gone.sum()) and res['removed_tracks'] == np.unique(q['tracks'][gone]).shape[0]
    assert res['kept_tracks'] == np.unique(z['y_out'][kept, 1]).shape[0]
    if 'kitti_bytes' in z.files:
        assert kitti_lines_host(q, res, rules) == z['kitti_bytes'].tobytes()
        assert res['removed_tracks'] > 0
    else:
        assert bdd_document_host(q, res, rules, str(z['bdd_name'])) == json.loads(str(z['bdd_json']))
        assert res['removed_tracks'] == 0
        json.dumps(bdd_document_host(q, res, rules, 'x'))           # plain ints and floats: json takes it


def test_float32_boundary():
    """np.amax(float32 scores) < 0.7 compares in float32 under NumPy 2: exactly float32(0.7) stays, the next float32 below goes."""
    assert float(SEVEN) < 0.7 and BELOW < SEVEN
    q = sequence([0, 1, 0, 1, 2], [2, 2, 2, 2, 2], [SEVEN, 0.1, BELOW, 0.1, 0.9])
    res = results_host(q, [5, 5, 6, 6, 7])
    assert res['tracks'].tolist() == [5, 5, -1, -1, 7]
    assert [res[k] for k in COUNT_KEYS] == [3, 2, 2, 1]
    assert res['order'].tolist() == [0, 1, 4]


def test_the_maximum_category_decides():
    q = sequence([0, 1, 0, 1, 0, 1], [1, 2, 2, 3, 1, 1], [0.5] * 6)
    res = results_host(q, [1, 1, 2, 2, 3, 3])
    assert res['tracks'].tolist() == [-1, -1, 2, 2, 3, 3]           # {1, 2}: a Car, removed; {2, 3}: a Cyclist; a Pedestrian
    assert results_host(q, [1, 1, 2, 2, 3, 3], BDD_RESULT_RULES)['removed_tracks'] == 0
    res = results_host(q, [1, 1, 2, 2, 3, 3], ResultRules(KITTI_RESULT_RULES.names, {3: 0.6, 1: 0.5}))
    assert res['tracks'].tolist() == [1, 1, -1, -1, 3, 3]           # 0.5 < 0.5 is false


def test_order_range_and_rows_without_a_track():
    q = sequence([9, 4, 9, 4, 6, 2], [1, 1, 1, 2, 1, 2], [0.9, 0.9, 0.9, 0.2, 0.9, 0.3])
    res = results_host(q, [3, 3, -1, 8, 1, 9])
    assert res['tracks'].tolist() == [3, 3, -1, -1, 1, -1] and res['order'].tolist() == [1, 4, 0]
    assert res['t_range'] == (2, 9)                                 # over all rows, removed ones included
    assert [res[k] for k in COUNT_KEYS] == [3, 2, 2, 2]
    lines = kitti_lines_host(q, res).decode().splitlines()
    assert lines[0] == '4 3 Pedestrian -1 -1 -10.00 4.00 5.00 6.00 7.00 -1.00 -1.00 -1.00 -1000.00 -1000.00 -1000.00 -10.00 0.90'
    assert [ln.split()[:2] for ln in lines] == [['4', '3'], ['6', '1'], ['9', '3']]
    doc = bdd_document_host(q, res, KITTI_RESULT_RULES, '0003.json')
    assert [d['frameIndex'] for d in doc] == list(range(2, 10)) and [len(d['labels']) for d in doc] == [0, 0, 1, 0, 1, 0, 0, 1]
    assert doc[2] == {'name': '0003.json', 'videoName': '0003.json', 'frameIndex': 4,
                      'labels': [{'id': 3, 'category': 'Pedestrian', 'box2d': {'x1': 4.0, 'y1': 5.0, 'x2': 6.0, 'y2': 7.0}}]}
    empty = results_host(sequence([], [], []), [])
    assert empty['t_range'] is None and empty['kept_rows'] == 0 and kitti_lines_host(sequence([], [], []), empty) == b''


def test_duplicates_negative_ids_and_unknown_categories():
    q = synth_result_sequence(3, 20, duplicate='kept')
    with pytest.raises(ValueError, match=rf'occurs twice in frame {q["dup_frame"]}$'):
        results_host(q, q['tracks'])
    q = synth_result_sequence(3, 20, duplicate='removed')           # the reference filters first: no error
    res = results_host(q, q['tracks'])
    rows = (q['det_frame'] == q['dup_frame']) & (q['tracks'] >= 0)
    ids, cnt = np.unique(q['tracks'][rows], return_counts=True)
    assert cnt.max() == 2 and (res['tracks'][q['tracks'] == ids[cnt.argmax()]] == -1).all()
    q = sequence([0, 0], [1, 1], [0.9, 0.9])
    with pytest.raises(ValueError, match='track id -2'):
        results_host(q, [-2, 4])
    with pytest.raises(ValueError, match=r'categories \[4\] are not among'):
        results_host(sequence([0], [4], [0.9]), [1])
    with pytest.raises(ValueError, match=r'sequence 1: categories \[9\]'):
        ResultStore([q, sequence([0], [9], [0.9])], BDD_RESULT_RULES)
    with pytest.raises(ValueError, match='det_score must be float32'):
        results_host(dict(q, det_score=np.array([0.9, 0.9])), [1, 2])


def test_score_keys_keep_the_order_of_the_floats():
    rng = np.random.default_rng(0)
    s = np.concatenate([rng.normal(0, 1, 500), [0.0, -0.0, np.inf, -np.inf, 0.7, 1e-45, -1e-45], [SEVEN, BELOW]]).astype(np.float32)
    k = score_keys(s)
    assert k.dtype == np.uint32
    i, j = np.meshgrid(np.arange(s.shape[0]), np.arange(s.shape[0]))
    assert np.array_equal(s[i] < s[j], k[i] < k[j]) and np.array_equal(s[i] == s[j], k[i] == k[j])
    nan = score_keys(np.array([np.nan, -np.nan], np.float32))
    assert (nan == 0xFFFFFFFF).all() and k.max() < 0xFFFFFFFF and k.min() > 0     # NaN: the maximum; 0 is free for "no threshold"
    q = sequence([0, 1], [2, 2], [np.nan, 0.1])                    # a NaN best score compares false: kept, as in the reference
    assert results_host(q, [1, 1])['removed_tracks'] == 0


def test_store_layout():
    seqs = [synth_result_sequence(5, 9), synth_result_sequence(6, 0), synth_result_sequence(7, 30, n_tracks=200, max_len=3)]
    st = ResultStore(seqs, KITTI_RESULT_RULES)
    assert st.seq[1, 1] == st.seq[1, 3] == st.seq[1, 5] == 0 and st.t_range[1] is None
    for s, q in enumerate(seqs):
        tb, nt, db, n, ob, nf = (int(v) for v in st.seq[s, :6])
        assert n == q['det_frame'].shape[0]
        if n == 0:
            continue
        assert nt >= max(256, 2 * n) and nt & (nt - 1) == 0 and nt < 4 * max(n, 128)
        perm, off = st.det_perm[db:db + n], st.det_off[ob:ob + nf + 1]
        fr = q['det_frame'][perm]
        assert np.array_equal(np.sort(perm), np.arange(n)) and (np.diff(fr) >= 0).all() and off[0] == 0 and off[-1] == n
        assert np.array_equal(st.det_fidx[db:db + n], fr - fr[0])
        for f in range(nf):
            assert (fr[off[f]:off[f + 1]] == fr[0] + f).all()
    assert st.thr_key.tolist() == [0, 0, int(score_keys(np.array([0.7], np.float32))[0]), 0]
