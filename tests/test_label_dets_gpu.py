"""GT track ids for detections on the device (csrc/labeldet.hip: tmpnn_label_dets, tmpnn_label_compact;
trackmpnn_amd.labeling.DetectionLabeler) against the host definition label_detections_host: equal, no tolerance."""
import functools

import numpy as np
import pytest

from tests.test_label_dets import FIXTURES, frame, load_fixture, special_frames
from trackmpnn_amd import DetectionStore, MotEvaluator, _lib
from trackmpnn_amd.labeling import BDD_RULES, KITTI_RULES, MAX_PER_FRAME, WAVE_FRAME, DetectionLabeler, synth_label_sequence

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def assert_equal_host(seqs, rules):
    """Labels on the device and on the host: track, keep, gt_keep, and the packed lists of both kinds.  Returns the labeler and
    the host's labels."""
    lb = DetectionLabeler(seqs, rules, DEV)
    lb.label()
    out = lb.read()
    host = DetectionLabeler(seqs, rules, device=None)
    host.label()
    ref = host.read()
    assert len(out) == len(ref) == len(seqs)
    for s, (o, h) in enumerate(zip(out, ref)):
        for k in ('track', 'keep', 'gt_keep'):
            assert o[k].dtype == h[k].dtype and np.array_equal(o[k], h[k]), f'sequence {s}: {k} differs'
    for mine, theirs in ((lb.store_sequences(), host.store_sequences()), (lb.eval_sequences(), host.eval_sequences())):
        for s, (a, b) in enumerate(zip(mine, theirs)):
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(a[k], b[k]) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype, f'sequence {s}: {k} differs'
    return lb, ref


@functools.lru_cache(maxsize=None)
def sized(seed, sizes, rules=KITTI_RULES):
    return synth_label_sequence(seed, 0, rules, sigma=4.0, sizes=sizes)


def test_limits_agree_with_the_library():
    lib = _lib.load()
    assert lib.tmpnn_label_max_per_frame() == MAX_PER_FRAME and lib.tmpnn_label_wave_frame() == WAVE_FRAME


@pytest.mark.parametrize('name', FIXTURES)
def test_fixtures(name):
    q, rules, ref = load_fixture(name)
    _, host = assert_equal_host([q], rules)
    assert np.array_equal(host[0]['keep'], ref['keep']) and np.array_equal(host[0]['gt_keep'], ref['gt_keep'])


def test_all_fixtures_in_one_store():
    (a, rules, _), (b, _, _) = load_fixture('label_kitti_a'), load_fixture('label_kitti_b')
    assert_equal_host([a, b, a], rules)


def test_sizes_across_the_wave_boundary():
    edge = (0, 1, 63, 64, 65)
    sizes = tuple((p, g) for p in edge for g in edge)
    q = sized(31, sizes)
    lb, host = assert_equal_host([q], KITTI_RULES)
    assert lb.n_small == 16 and lb.n_big == 9                     # (both kernels ran)
    assert 0.1 < (host[0]['track'] >= 0).mean() < 0.9 and 0.1 < (~host[0]['keep']).mean() < 0.9
    assert_equal_host([sized(32, sizes, BDD_RULES)], BDD_RULES)


def test_full_frame():
    q = sized(41, ((MAX_PER_FRAME, MAX_PER_FRAME), (3, 2)))
    _, host = assert_equal_host([q], KITTI_RULES)
    assert (host[0]['track'] >= 0).sum() > 40 and (~host[0]['keep']).sum() > 40


def test_over_the_limit_raises():
    q = sized(43, ((2, 2), (MAX_PER_FRAME + 1, 5), (4, 4)))
    lb = DetectionLabeler([sized(44, ((2, 2),)), q], KITTI_RULES, DEV)
    lb.label()
    with pytest.raises(RuntimeError, match='sequence 1, frame 1 has more than 256'):
        lb.read()
    q = sized(45, ((5, MAX_PER_FRAME + 1),))
    lb = DetectionLabeler([q], KITTI_RULES, DEV)
    lb.label()
    with pytest.raises(RuntimeError, match='sequence 0, frame 0 has more than 256'):
        lb.read()


@pytest.mark.parametrize('name', sorted(special_frames()))
def test_special_frames(name):
    q = special_frames()[name]
    lb, host = assert_equal_host([q], KITTI_RULES)
    if name.startswith('chain'):
        n = q['gt_frame'].shape[0]
        assert host[0]['track'].tolist() == list(range(1, n))
        assert (lb.n_small, lb.n_big) == ((1, 0) if n <= WAVE_FRAME else (0, 1))


def test_label_twice_and_rows_in_any_order():
    q, rules, _ = load_fixture('label_bdd')
    rng = np.random.default_rng(5)
    pd = np.concatenate([np.where(q['det_frame'] == t)[0] for t in rng.permutation(q['num_frames'])])
    pg = np.concatenate([np.where(q['gt_frame'] == t)[0] for t in rng.permutation(q['num_frames'])])
    q2 = {k: (v[pd] if k.startswith('det') else v[pg]) if isinstance(v, np.ndarray) else v for k, v in q.items()}
    lb, host = assert_equal_host([q2], rules)
    lb.label()                                                    # (a second labelling overwrites the first)
    again = lb.read()
    assert all(np.array_equal(again[0][k], host[0][k]) for k in ('track', 'keep', 'gt_keep'))


def test_many_small_frames_cross_the_scan_tile():
    seqs = [synth_label_sequence(900 + i, 600, KITTI_RULES, max_det=3, max_gt=3, sigma=3.0) for i in range(5)]
    empty_i, empty_f = np.zeros(0, np.int64), np.zeros((0, 4), np.float32)
    seqs[1].update(det_frame=empty_i, det_cat=empty_i, det_box=empty_f, det_score=np.zeros(0, np.float32))      # no detections
    seqs[3].update(gt_frame=empty_i, gt_track=empty_i, gt_cat=empty_i, gt_box=empty_f)                          # no GT
    lb, host = assert_equal_host(seqs, KITTI_RULES)
    assert lb.F == 3000 and lb.n_big == 0
    assert host[3]['keep'].all() and (host[3]['track'] < 0).all() and host[1]['keep'].shape == (0,)
    kept = sum(int(h['keep'].sum()) for h in host)
    assert 0.1 < kept / lb.n_det < 0.95 and sum(int((h['track'] >= 0).sum()) for h in host) > 300


def test_lists_are_accepted_downstream():
    q, rules, _ = load_fixture('label_kitti_a')
    lb = DetectionLabeler([q, load_fixture('label_kitti_b')[0]], rules, DEV)
    lb.label()
    es, ss = lb.eval_sequences(), lb.store_sequences()
    ev = MotEvaluator(es, DEV)
    ev.evaluate([s['track'] for s in ss])                         # the labels themselves as tracks
    per, overall = ev.read()
    for r, e, t in zip(per, es, ss):
        assert r['objects'] == e['gt_frame'].shape[0] and r['predictions'] == int((t['track'] >= 0).sum())
    # an assigned detection overlaps its GT row by half in the "+1" form; the evaluator's own overlap has no "+1", so a few
    # pairs at the edge may fall out, but not many
    assert 0.9 * overall['predictions'] < overall['matches'] <= overall['predictions']
    store = DetectionStore(ss, 3, '2d+temp', np.zeros(10), np.ones(10), device=DEV)
    assert store.ndets == sum(s['frame'].shape[0] for s in ss)
    assert np.array_equal(store.track_d.cpu().numpy(), np.concatenate([s['track'] for s in ss]).astype(np.int32))


def test_empty_store():
    lb, host = assert_equal_host([frame([], [], num_frames=3)], KITTI_RULES)
    assert host[0]['keep'].shape == (0,) and lb.store_sequences()[0]['frame'].shape == (0,)
