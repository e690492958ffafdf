"""The result filter on the device (csrc/results.hip: tmpnn_results_apply; TrackResults) against the host definition
results_host.  Every comparison is exact: the filtered ids, the order of the kept rows, the counts.  Shapes are the smallest at
which the kernels can go wrong: several sequences of different sizes in one store, an empty one, one left out, and one sequence
beyond a workgroup's span of the scan whose sparse ids collide in the table."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_track_results import fixture_names, load_fixture, sequence
from trackmpnn_amd.moteval import FLAG_DUPLICATE, MotEvaluator, mot_events_host, synth_mot_sequence
from trackmpnn_amd.results import (BDD_RESULT_RULES, COUNT_KEYS, FLAG_NEGATIVE, KITTI_RESULT_RULES, TrackResults, kitti_lines_host,
                                   bdd_document_host, results_host, results_overall, synth_result_sequence)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def same(dev, ref):
    return (set(dev) == set(ref) and np.array_equal(dev['tracks'], ref['tracks']) and dev['tracks'].dtype == ref['tracks'].dtype
            and np.array_equal(dev['order'], ref['order']) and dev['order'].dtype == ref['order'].dtype == np.int32
            and all(dev[k] == ref[k] for k in COUNT_KEYS + ('t_range',)))


def host_tracks(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def assert_equal_host(seqs, rules=KITTI_RESULT_RULES, tracks=None, tr=None):
    tr = TrackResults(seqs, rules, DEV) if tr is None else tr
    tracks = [q['tracks'] for q in seqs] if tracks is None else tracks
    tr.apply(tracks)
    per = tr.read()
    refs = [None if t is None else results_host(q, host_tracks(t), rules) for q, t in zip(seqs, tracks)]
    for s, (d, r) in enumerate(zip(per, refs)):
        assert (d is None and r is None) or same(d, r), f'sequence {s}: device != host'
    return refs, tr


@pytest.fixture(scope='module')
def big():
    """about 5000 rows, 3500 distinct sparse ids up to 2^31 - 1: five spans of the scan, and 3500 ids in 16384 slots collide"""
    q = synth_result_sequence(2, 60, n_tracks=3500, max_len=2, sparse_ids=True)
    return q, results_host(q, q['tracks'])


@pytest.mark.parametrize('name', fixture_names())
def test_fixtures(name, tmp_path):
    q, rules, z = load_fixture(name)
    refs, tr = assert_equal_host([q], rules)
    assert np.array_equal(refs[0]['tracks'], z['y_out'][:, 1])
    if 'kitti_bytes' in z.files:
        paths = tr.write_kitti(str(tmp_path))
        assert [os.path.basename(p) for p in paths] == ['0000.txt']
        assert open(paths[0], 'rb').read() == z['kitti_bytes'].tobytes()         # byte-equal to what the reference wrote
    else:
        paths = tr.write_bdd(str(tmp_path))
        doc = json.load(open(paths[0]))
        assert doc == bdd_document_host(q, refs[0], rules, '0000.json')
        ref = json.loads(str(z['bdd_json']))
        assert [d['labels'] for d in doc] == [d['labels'] for d in ref] and [d['frameIndex'] for d in doc] == [d['frameIndex'] for d in ref]


def test_three_sequences_one_empty_one_left_out(tmp_path):
    seqs = [synth_result_sequence(21, 25, n_tracks=30), synth_result_sequence(22, 0), synth_result_sequence(23, 7, n_tracks=9, with_3d=True),
            synth_result_sequence(24, 40, n_tracks=60, max_len=5)]
    assert [q['det_frame'].shape[0] for q in seqs][1] == 0 and len({q['det_frame'].shape[0] for q in seqs}) == 4
    tracks = [seqs[0]['tracks'], seqs[1]['tracks'], None, torch.from_numpy(seqs[3]['tracks']).to(DEV)]    # host, host, left out, device
    refs, tr = assert_equal_host(seqs, tracks=tracks)
    assert refs[2] is None and refs[1]['t_range'] is None and all(refs[s]['removed_tracks'] > 0 and refs[s]['kept_tracks'] > 0 for s in (0, 3))
    ft = tr.filtered_tracks()
    assert [f.shape[0] for f in ft] == [q['det_frame'].shape[0] for q in seqs] and all(f.dtype == torch.int32 and f.is_cuda for f in ft)
    assert np.array_equal(ft[3].cpu().numpy(), refs[3]['tracks']) and (ft[2].cpu().numpy() == -1).all()
    paths = tr.write_kitti(str(tmp_path))                           # no detections / left out: no file
    assert paths[1] is None and paths[2] is None and sorted(os.listdir(tmp_path)) == ['0000.txt', '0003.txt']
    assert open(paths[3], 'rb').read() == kitti_lines_host(seqs[3], refs[3])
    # the other way round: device int32 / device int64 / host, everything taking part
    tracks = [torch.from_numpy(seqs[0]['tracks']).to(DEV).int(), seqs[1]['tracks'], torch.from_numpy(seqs[2]['tracks']).to(DEV), seqs[3]['tracks']]
    refs2, _ = assert_equal_host(seqs, tracks=tracks, tr=tr)
    assert same(refs2[0], refs[0]) and refs2[2] is not None


def test_beyond_one_span_with_sparse_ids(big):
    q, ref = big
    n = q['det_frame'].shape[0]
    assert 4500 < n < 5500 and n > 4 * 1024                         # RS_SPAN = 1024 positions a pass of the scan
    ids = np.unique(q['tracks'][q['tracks'] >= 0])
    assert ids.shape[0] >= 3000 and ids.min() == 0 and ids.max() == 2 ** 31 - 1
    slots = (ids.astype(np.uint64) * 0x9E3779B1 % 2 ** 32 >> 18).astype(np.int64)      # the table's hash: 2^14 slots for 2 n <= 16384
    assert np.unique(slots).shape[0] < ids.shape[0]                 # ids collide
    small = synth_result_sequence(31, 12)
    refs, tr = assert_equal_host([small, q, small])
    assert same(refs[1], ref) and ref['removed_tracks'] > 300 and ref['kept_tracks'] > 1000
    rec = tr._out.cpu().numpy().copy()
    tr.apply([small['tracks'], torch.from_numpy(q['tracks']).to(DEV), small['tracks']])
    assert np.array_equal(tr._out.cpu().numpy(), rec)               # a second run, device tracks: the same bytes


def test_two_applies_leak_nothing(big):
    q, ref = big
    small = synth_result_sequence(32, 15, n_tracks=25)
    tr = TrackResults([q, small], KITTI_RESULT_RULES, DEV)
    other = []                                                      # every track split in two by the parity of the frame
    for x in (q, small):
        dense = np.unique(x['tracks'], return_inverse=True)[1].reshape(-1)
        other.append(np.where(x['tracks'] >= 0, 2 * dense + x['det_frame'] % 2, -1))
    first, _ = assert_equal_host([q, small], tr=tr)
    second, _ = assert_equal_host([q, small], tracks=other, tr=tr)
    assert first[0]['kept_rows'] != second[0]['kept_rows'] and first[0]['kept_tracks'] != second[0]['kept_tracks']
    third, _ = assert_equal_host([q, small], tracks=[None, small['tracks']], tr=tr)         # fewer kept rows: the tail of order is -1
    assert third[0] is None and same(third[1], first[1])
    st = tr.store
    order = tr._out.cpu().numpy()[tr._rec_ints + st.n_det:]
    assert (order[:q['det_frame'].shape[0]] == -1).all() and (order[int(st.seq[1, 2]) + third[1]['kept_rows']:] == -1).all()
    again, _ = assert_equal_host([q, small], tr=tr)
    assert same(again[0], first[0]) and same(again[1], first[1])


def test_a_planted_duplicate_is_flagged():
    dup, clean, gone = synth_result_sequence(3, 20, duplicate='kept'), synth_result_sequence(4, 20), synth_result_sequence(3, 20, duplicate='removed')
    seqs = [clean, dup, gone]
    tr = TrackResults(seqs, KITTI_RESULT_RULES, DEV)
    tr.apply([q['tracks'] for q in seqs])
    with pytest.raises(RuntimeError, match=rf'^TrackResults.read: sequence 1, frame {dup["dup_frame"]}: a kept track id occurs twice in one frame$'):
        tr.read()
    with pytest.raises(ValueError, match=rf'twice in frame {dup["dup_frame"]}$'):
        results_host(dup, dup['tracks'])
    per = tr.read(check=False)
    assert per[1]['flag'] & FLAG_DUPLICATE and (per[1]['flag'] >> 8) - 1 + int(dup['det_frame'].min()) == dup['dup_frame']
    for s in (0, 2):                                               # the others are unaffected; a duplicate in a removed track is none
        assert per[s].pop('flag') == 0 and same(per[s], results_host(seqs[s], seqs[s]['tracks']))
    # two duplicates: the first frame is the one named
    q = sequence([5, 5, 3, 3, 4], [1, 1, 1, 1, 1], [0.9] * 5)
    tr = TrackResults([q], KITTI_RESULT_RULES, DEV)
    tr.apply([np.array([7, 7, 8, 8, 9])])
    with pytest.raises(RuntimeError, match='sequence 0, frame 3: a kept'):
        tr.read()
    tr.apply([np.array([7, -2, 8, 1, 9])])
    with pytest.raises(RuntimeError, match='sequence 0: a track id below -1'):
        tr.read()
    assert tr.read(check=False)[0]['flag'] == FLAG_NEGATIVE
    with pytest.raises(ValueError, match='track id -2'):
        results_host(q, [7, -2, 8, 1, 9])


def test_filtered_tracks_feed_the_evaluators():
    seqs = []
    for i in range(2):
        q = synth_mot_sequence(50 + i, 30, objects=7)
        n = q['det_frame'].shape[0]
        rng = np.random.default_rng(60 + i)
        q['det_cat'] = np.where(q['tracks'] >= 0, 1 + q['tracks'] % 3, rng.integers(1, 4, n))       # one category a track
        q['det_score'] = rng.uniform(0.2, 0.71, n).astype(np.float32)
        seqs.append(q)
    tr = TrackResults(seqs, KITTI_RESULT_RULES, DEV)                 # (GT keys are ignored)
    tr.apply([q['tracks'] for q in seqs])
    ev = MotEvaluator(seqs, DEV)
    ev.evaluate(tr.filtered_tracks())
    rec = ev._out.cpu().numpy().copy()
    per, _ = ev.read()
    refs = [results_host(q, q['tracks']) for q in seqs]
    assert all(0 < r['removed_rows'] < r['kept_rows'] for r in refs)
    ev.evaluate([r['tracks'] for r in refs])                        # the host-filtered ids: the same record
    assert np.array_equal(ev._out.cpu().numpy(), rec)
    for p, q, r in zip(per, seqs, refs):
        h = mot_events_host(q['det_frame'], q['det_box'], r['tracks'], q['gt_frame'], q['gt_track'], q['gt_box'])
        assert all(p[k] == h[k] for k in ('objects', 'predictions', 'matches', 'switches', 'false_positives', 'misses'))
        assert p['predictions'] == r['kept_rows']


def test_calling_behaviour():
    seqs = [synth_result_sequence(41, 6), synth_result_sequence(42, 9)]
    tr = TrackResults(seqs, KITTI_RESULT_RULES, DEV)
    with pytest.raises(RuntimeError, match='no apply has been enqueued'):
        tr.read()
    with pytest.raises(RuntimeError, match='no apply has been enqueued'):
        tr.filtered_tracks()
    with pytest.raises(ValueError, match='1 track arrays for 2 sequences'):
        tr.apply([seqs[0]['tracks']])
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        TrackResults(seqs, KITTI_RESULT_RULES, 'cpu')
    with pytest.raises(ValueError, match=r'categories \[4, 5, 6, 7, 8\]'):
        TrackResults([synth_result_sequence(43, 6, rules=BDD_RESULT_RULES)], KITTI_RESULT_RULES, DEV)
    assert TrackResults([], KITTI_RESULT_RULES, DEV).store.S == 0
    refs, _ = assert_equal_host([synth_result_sequence(43, 6, rules=BDD_RESULT_RULES)], BDD_RESULT_RULES)
    assert refs[0]['removed_tracks'] == 0 and refs[0]['kept_tracks'] == 20


def infer_fixture(name='infer_greedy_w3_r0'):
    from tests.golden_util import Golden
    from tests.test_parity_gpu import build_model
    gold = Golden(name)
    m = gold.meta
    X, y = gold.t('X'), gold.t('y')
    n = int(y.shape[1])
    rng = np.random.default_rng(8)
    seq = {'X': X, 'y': y, 'det_frame': y[0, :, 0].numpy().astype(np.int64), 'det_cat': rng.integers(1, 4, n),
           'det_score': rng.uniform(0.2, 0.74, n).astype(np.float32)}
    c, wh = rng.uniform(100, 900, (n, 2)), rng.uniform(30, 80, (n, 2))
    seq['det_box'] = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    return gold, m, build_model(m, gold.params()), seq


def test_infer_dataset_on_a_reference_sequence():
    from trackmpnn_amd.loops import infer_dataset
    gold, m, model, seq = infer_fixture()
    empty = dict(sequence([], [], []), X=torch.zeros(1, 0, seq['X'].shape[2]), y=torch.zeros(1, 0, 2, dtype=torch.int64))
    tr = TrackResults([empty, seq], KITTI_RESULT_RULES, DEV)
    per = infer_dataset(model, [empty, seq], tr, m['cur_win_size'], m['ret_win_size'], m['hungarian'], m.get('tp_classifier', True))
    y_out = gold.d[f'd{gold.ncalls - 1}/y_out']                     # the reference's tracks of this sequence
    ref = results_host(seq, y_out[:, 1])
    assert per[0] is None and same(per[1], ref) and ref['removed_tracks'] > 0 and ref['kept_tracks'] > 0
    assert not model.training
    with pytest.raises(ValueError, match='1 sequences, the results hold 2'):
        infer_dataset(model, [seq], tr)


def test_validate_scores_the_filtered_tracks():
    from trackmpnn_amd import validate
    from trackmpnn_amd.loops import infer_sequence
    gold, m, model, seq = infer_fixture()
    rng = np.random.default_rng(9)
    n = seq['det_frame'].shape[0]
    y_ref = gold.d[f'd{gold.ncalls - 1}/y_out']
    gt = y_ref[:, 1] >= 0                                          # a ground truth: the reference's tracks, jittered boxes
    seq.update(gt_frame=seq['det_frame'][gt], gt_track=y_ref[gt, 1], gt_box=(seq['det_box'][gt] + rng.normal(0, 1, (int(gt.sum()), 4))).astype(np.float32))
    args = (m['cur_win_size'], m['ret_win_size'], m['hungarian'], m.get('tp_classifier', True))
    tr = TrackResults([seq], KITTI_RESULT_RULES, DEV)
    plain = validate(model, [seq], MotEvaluator([seq], DEV), *args)
    out = validate(model, [seq], MotEvaluator([seq], DEV), *args, results=tr)
    y_out = infer_sequence(model, seq['X'], seq['y'], args[0], args[1], args[2], DEV, args[3])[0]
    ref = results_host(seq, y_out[:, 1])
    ev = MotEvaluator([seq], DEV)
    ev.evaluate([ref['tracks']])                                   # validate of the host-filtered tracks
    per, overall = ev.read()
    assert out['results'] == results_overall([ref]) and ref['removed_rows'] > 0
    assert set(out) - set(plain) == {'results'}
    for k, v in overall.items():
        assert np.array_equal(np.asarray(out[k], np.float64).view(np.int64), np.asarray(v, np.float64).view(np.int64)), k
    assert out['predictions'] == ref['kept_rows'] < plain['predictions']
    with pytest.raises(ValueError, match='results was not built over the sequences'):
        validate(model, [seq], MotEvaluator([seq], DEV), *args, results=TrackResults([sequence([0], [1], [0.5])], KITTI_RESULT_RULES, DEV))
