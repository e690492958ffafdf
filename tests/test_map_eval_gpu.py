"""The validation mAP on the device (csrc/mapeval.hip: tmpnn_map_best, tmpnn_map_eval; trackmpnn_amd.mapeval.MapEvaluator;
trackmpnn_amd.loops.validate(map_evaluator=)) against the host definition map_host: counts equal, ap and map bit for bit.  No
tolerance, except against the recorded results of the reference (the bound of tests/test_map_eval.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_map_eval import FIXTURES, fixture_bound, load_fixture, same, seq
from trackmpnn_amd import _lib
from trackmpnn_amd.mapeval import MapEvaluator, map_best_host, map_host, synth_map_sequence

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def device(seqs, tracks):
    ev = MapEvaluator(seqs, DEV)
    ev.evaluate(tracks)
    return ev.read()


def assert_equal_host(seqs, tracks):
    d, h = device(seqs, tracks), map_host(seqs, tracks)
    assert same(d, h), f'device {d} != host {h}'
    return h


def test_map_best_equals_the_host():
    rng = np.random.default_rng(11)
    c = rng.uniform(0, 400, (2, 2))[rng.integers(0, 2, 64)]       # 64 x 64 boxes around 2 centres: many pairs overlap by half

    def boxes():
        tl = c + rng.normal(0, 14, (64, 2))
        return np.concatenate([tl, tl + rng.uniform(40, 60, (64, 2))], 1).astype(np.float32)
    z = [5, 5, 4, 4]                                              # zero area in the "+1" form
    special = [([1000, 0, 1009, 9], [[1000, 0, 1004, 9]], 0),                     # exactly 0.5
               ([0, 0, 9, 9], [[0, 0, 4, 8]], -1),                                # just below
               ([0, 0, 9, 9], [[0, 0, 9, 8], [0, 0, 9, 9], [0, 0, 9, 9]], 1),     # two equal maxima: the first
               (z, [z, z], -1),                                                   # 0 / 0: NaN is the maximum and fails
               (z, [[0, 0, 9, 9], z], -1),                                        # ... also behind a finite value
               ([0, 0, 9, 9], [z, [0, 0, 9, 9]], 1)]                              # a degenerate GT box is no obstacle
    gt = [boxes()] + [np.float32(g) for _, g, _ in special]
    det_box = np.concatenate([boxes(), np.float32([d for d, _, _ in special]), np.float32([[0, 0, 9, 9]])])
    det_grp = np.concatenate([np.zeros(64), 1 + np.arange(len(special)), [-1]]).astype(np.int32)
    grp_off = np.concatenate([[0], np.cumsum([g.shape[0] for g in gt])]).astype(np.int32)
    gt_box = np.concatenate(gt)
    ref = np.full(det_box.shape[0], -1, np.int64)
    for d, g in enumerate(det_grp):
        if g >= 0:
            j = map_best_host(det_box[d:d + 1], gt_box[grp_off[g]:grp_off[g + 1]])[0]
            ref[d] = grp_off[g] + j if j >= 0 else -1
    for k, (_, _, want) in enumerate(special):                    # the host definition itself on the special pairs
        assert ref[64 + k] == (grp_off[1 + k] + want if want >= 0 else -1)
    assert 0.2 < (ref[:64] >= 0).mean() < 0.9                      # both outcomes in number
    t = {k: torch.from_numpy(v).to(DEV) for k, v in dict(gt_box=gt_box, grp_off=grp_off, det_box=det_box, det_grp=det_grp).items()}
    out = torch.full((det_box.shape[0],), -7, dtype=torch.int32, device=DEV)
    st = _lib.CMapStore(1, 1, gt_box.shape[0], det_box.shape[0], grp_off.shape[0] - 1, 0, 0, t['gt_box'].data_ptr(), None, None,
                        t['grp_off'].data_ptr(), t['det_box'].data_ptr(), t['det_grp'].data_ptr())
    _lib.call('tmpnn_map_best', C.byref(st), out.data_ptr(), _lib.raw_stream(torch.device(DEV)))
    assert np.array_equal(out.cpu().numpy().astype(np.int64), ref)


@pytest.fixture(scope='module')
def five():
    """Sequences of 1, 2, 3, 40 and 65 frames, three classes; without and with ties in score."""
    return {ties: [synth_map_sequence(300 + i, L, ties=ties) for i, L in enumerate((1, 2, 3, 40, 65))] for ties in (False, True)}


@pytest.mark.parametrize('ties', [False, True])
def test_evaluate_equals_the_host(five, ties):
    seqs = five[ties]
    h = assert_equal_host(seqs, [q['tracks'] for q in seqs])
    assert h['classes'] == [0, 1, 2] and all(0 < t < k for t, k in zip(h['true_positives'], h['kept']))
    if ties:
        assert np.unique(np.concatenate([q['det_score'] for q in seqs])).shape[0] <= 11


def one_class(n, seed):
    """One class with exactly n detections, all in frames with GT: per frame six GT boxes on a grid, per box a detection
    most of the time and sometimes a duplicate, stray detections in between."""
    rng = np.random.default_rng(seed)
    det, gt, t = [], [], 0
    while len(det) < n:
        for o in range(6):
            x, y = 150.0 * o, 20.0 * (t % 7)
            gt.append((t, 1, x, y, x + 60, y + 60))
            for _ in range(int(rng.random() < 0.85) + int(rng.random() < 0.15)):
                j = rng.normal(0, 4, 4)
                det.append((t, 1, 0, x + j[0], y + j[1], x + 60 + j[2], y + 60 + j[3]))
            if rng.random() < 0.2:
                det.append((t, 1, 0, x + 75, y + 300, x + 135, y + 360))
        t += 1
    q = seq(det[:n], gt)
    q['det_score'] = ((rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    return q


@pytest.mark.parametrize('which', ['tile', 'tile + 1', '2 * tile + 1'])
def test_tile_boundaries(which):
    """The carries of the three sweeps (counts, envelope, ordered sum) cross from tile to tile at multiples of the tile."""
    tile = _lib.load().tmpnn_map_tile()
    n = {'tile': tile, 'tile + 1': tile + 1, '2 * tile + 1': 2 * tile + 1}[which]
    q = one_class(n, 40 + n)
    ev = MapEvaluator([q], DEV)
    assert ev.store.C == 1 and ev.store.n_live == n
    tr = np.arange(n, dtype=np.int64)
    ev.evaluate([tr])
    d, h = ev.read(), map_host([q], [tr])
    assert same(d, h), f'device {d} != host {h}'
    assert h['kept'] == [n] and 0.5 * n < h['true_positives'][0] < 0.95 * n and 0.3 < h['ap'][0] < 0.999
    # the list as long as before, fewer kept: the ranks k no longer coincide with the positions in the list
    tr2 = np.where(np.arange(n) % 5 == 2, -1, tr)
    ev.evaluate([tr2])
    d, h2 = ev.read(), map_host([q], [tr2])
    assert same(d, h2) and h2['kept'][0] == int((tr2 >= 0).sum()) < n


def test_the_same_evaluator_twice_keeps_no_stale_marks(five):
    seqs = five[False]
    ev = MapEvaluator(seqs, DEV)
    t1 = [q['tracks'] for q in seqs]
    # other tracks: the first claimant of many GT rows loses its track, so the mark moves to a duplicate or goes away
    t2 = [np.where(np.arange(t.shape[0]) % 2 == 0, -1, t) for t in t1]
    h1, h2 = map_host(seqs, t1), map_host(seqs, t2)
    assert h1['true_positives'] != h2['true_positives']
    for tracks, h in ((t1, h1), (t2, h2), (t1, h1), ([np.full_like(t, -1) for t in t1], None), (t2, h2)):
        ev.evaluate(tracks)
        d = ev.read()
        if h is None:
            assert d['kept'] == [0, 0, 0] and d['ap'] == [0.0, 0.0, 0.0] and d['annotations'] == h1['annotations']
        else:
            assert same(d, h)


def test_sequences_left_out_and_device_tensors(five):
    seqs = five[True]
    ev = MapEvaluator(seqs, DEV)
    tracks = [q['tracks'] for q in seqs]
    full = map_host(seqs, tracks)
    as_dev = [torch.from_numpy(t).to(DEV) for t in tracks]
    ev.evaluate(as_dev)                                           # every sequence on the device: no track upload at all
    assert same(ev.read(), full)
    ev.evaluate([as_dev[0].int(), tracks[1], torch.from_numpy(tracks[2]), as_dev[3], tracks[4]])
    assert same(ev.read(), full)
    for left in ([3], [0, 4], [0, 1, 2, 4]):
        t = [None if s in left else (as_dev[s] if s % 2 else tracks[s]) for s in range(5)]
        ev.evaluate(t)
        h = map_host(seqs, t)
        assert same(ev.read(), h) and h['annotations'] != full['annotations']
    t = [None, None, None, as_dev[3], None]                       # only device tensors and a changed participation
    ev.evaluate(t)
    assert same(ev.read(), map_host(seqs, t))
    ev.evaluate(as_dev)
    assert same(ev.read(), full)
    ev.evaluate([None] * 5)
    r = ev.read()
    assert r['classes'] == [] and np.isnan(r['map'])
    with pytest.raises(ValueError):
        ev.evaluate(tracks[:2])
    with pytest.raises(ValueError):
        ev.evaluate([tracks[0][:-1]] + tracks[1:])
    with pytest.raises(RuntimeError, match='no evaluation'):
        MapEvaluator(seqs[:1], DEV).read()


def test_hand_made_cases_on_the_device():
    gt = [(0, 1, 0, 0, 99, 99), (0, 1, 20, 0, 119, 99), (0, 2, 0, 0, 4, 9)]
    det = [(0, 1, 0.9, 0, 0, 99, 99), (0, 1, 0.8, 9, 0, 108, 99), (0, 2, 0.7, 0, 0, 9, 9), (3, 1, 0.95, 0, 0, 9, 9), (0, 7, 0.99, 0, 0, 9, 9)]
    q = seq(det, gt)
    empty = seq([(0, 1, 0.5, 0, 0, 9, 9)], [])
    for tracks in ([np.arange(5), np.arange(1)], [np.array([-1, 3, 4, 5, 6]), None], [np.array([0, -1, -1, 1, 2]), np.arange(1)]):
        assert_equal_host([q, empty], tracks)
    r = device([empty], [np.arange(1)])
    assert r['classes'] == [] and np.isnan(r['map'])


@pytest.mark.parametrize('path', FIXTURES, ids=os.path.basename)
def test_reference_fixtures_through_the_device(path):
    seqs, tracks, ref, max_tp = load_fixture(path)
    d = device(seqs, tracks)
    assert same(d, map_host(seqs, tracks))
    assert abs(d['map'] - ref) <= fixture_bound(max_tp, len(d['classes']))


@pytest.mark.parametrize('use_hungarian', [False, True])
def test_validate_end_to_end(use_hungarian):
    from trackmpnn_amd import MotEvaluator, TrackMPNN, validate
    from trackmpnn_amd.loops import infer_sequence
    seqs = []
    for i in range(3):
        q = synth_map_sequence(70 + i, 30, objects=4)
        y = np.stack([q['det_frame'], q['tracks']], 1)
        q['y'] = torch.from_numpy(y)[None]
        q['X'] = torch.randn(1, y.shape[0], 8, generator=torch.Generator().manual_seed(700 + i))
        seqs.append(q)
    no_gt = dict(seqs[0], gt_frame=np.zeros(0, np.int64), gt_track=np.zeros(0, np.int64), gt_box=np.zeros((0, 4), np.float32),
                 gt_cat=np.zeros(0, np.int64))                     # skipped (train.py:190-192): left out of the mAP too
    seqs = [seqs[0], no_gt, seqs[1], seqs[2]]
    torch.manual_seed(9)
    model = TrackMPNN('2d', 3, 32, 0, 'diff').to(DEV)
    gp = torch.Generator().manual_seed(17)
    with torch.no_grad():                                          # scores on both sides of 0.5
        for k, prm in model.named_parameters():
            prm.add_((0.1 * torch.randn(prm.shape, generator=gp)).to(DEV))
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_((0.5 * torch.randn(prm.shape, generator=gp)).to(DEV))
    model.eval()
    ev, mev = MotEvaluator(seqs, DEV), MapEvaluator(seqs, DEV)
    plain = validate(model, seqs, ev, cur_win_size=3, use_hungarian=use_hungarian)
    out = validate(model, seqs, ev, cur_win_size=3, use_hungarian=use_hungarian, map_evaluator=mev)
    from trackmpnn_amd.moteval import COUNT_KEYS
    assert set(plain) == set(COUNT_KEYS) | {'dist_sum', 'mota', 'motp', 'recall', 'precision', 'motas', 'per_sequence'}
    assert set(out) == set(plain) | {'map', 'aps'}
    assert all(out[k] == plain[k] or (out[k] != out[k] and plain[k] != plain[k]) for k in plain if k != 'per_sequence')
    tracks = []
    for s, q in enumerate(seqs):
        if s == 1:
            tracks.append(None)
            continue
        y_out, ncalls, _ = infer_sequence(model, q['X'], q['y'], 3, 0, use_hungarian, DEV)
        assert ncalls > 0
        tracks.append(y_out[:, 1])
    h = map_host(seqs, tracks)
    assert np.float64(out['map']).view(np.int64) == np.float64(h['map']).view(np.int64)
    assert out['aps'] == dict(zip(h['classes'], h['ap'])) and sum(h['kept']) > 0 and sum(h['true_positives']) > 0
    with pytest.raises(ValueError, match='map_evaluator'):
        validate(model, seqs, ev, cur_win_size=3, map_evaluator=MapEvaluator(seqs[:3], DEV))
