"""The host definition of HOTA (trackmpnn_amd.hota.hota_host, hota_overall), pinned by hand-computed cases: TrackEval is not a
dependency and no fixture holds its output, so the figures below are worked out from the metric's definition."""
import numpy as np
import pytest

from trackmpnn_amd.hota import ALPHAS, EPS, FIGURES, NA, hota_host, hota_overall, hota_sim_host, synth_hota_sequence

ARGS = ('det_frame', 'det_box', 'tracks', 'gt_frame', 'gt_track', 'gt_box')


def host(q):
    return hota_host(*[q[k] for k in ARGS])


def grid_boxes(ids):
    ids = np.asarray(ids, np.float32)
    return np.stack([100 * ids, 0 * ids, 100 * ids + 40, 0 * ids + 30], 1).astype(np.float32)


def perfect_sequence(objects=4, frames=30):
    f = np.repeat(np.arange(frames), objects)
    o = np.tile(np.arange(objects), frames)
    return {'det_frame': f, 'det_box': grid_boxes(o), 'tracks': o + 10, 'gt_frame': f.copy(), 'gt_track': 3 * o + 2, 'gt_box': grid_boxes(o)}


def swap_sequence():
    """two objects, 10 frames, exact boxes; the two hypothesis ids swap at frame 5"""
    q = perfect_sequence(2, 10)
    q['tracks'] = np.where(q['det_frame'] < 5, q['tracks'], 21 - q['tracks'])
    return q


def edge_sequence():
    """GT (0, 0, 2, 1) against detection (0, 0, 1, 1): IoU exactly 0.5"""
    return {'det_frame': np.array([0]), 'det_box': np.float32([[0, 0, 1, 1]]), 'tracks': np.array([7]), 'gt_frame': np.array([0]),
            'gt_track': np.array([1]), 'gt_box': np.float32([[0, 0, 2, 1]])}


def grid_frame(nO, nH, seed, frames=1):
    """`frames` identical frames of nO GT boxes and nH detections on a grid of 60 x 60 cells (boxes 40 x 40): most pairs do not
    overlap (scores exactly 0); GT boxes repeat every 3 nO / 4 cells and detections draw their cell and one of three offsets
    at random, so boxes are duplicated and positive scores tie exactly."""
    rng = np.random.default_rng(seed)
    cells = max(1, 3 * nO // 4)
    oc = np.arange(nO) % cells
    hc = rng.integers(0, cells + 2, nH)
    off = rng.choice(np.float32([0, 5, 10]), nH)

    def box(c, d):
        x, y = 60.0 * (c % 32) + d, 60.0 * (c // 32)
        return np.stack([x, y, x + 40, y + 40], 1).astype(np.float32)
    rep = lambda a: np.concatenate([a] * frames)
    return {'gt_frame': np.repeat(np.arange(frames), nO), 'gt_track': rep(rng.permutation(nO) * 2 + 1), 'gt_box': rep(box(oc, 0 * oc)),
            'det_frame': np.repeat(np.arange(frames), nH), 'tracks': rep(rng.permutation(nH) + 50), 'det_box': rep(box(hc, off))}


def lds_switch_sequences(shapes):
    """three grid frames per shape; in the last one the detections carry other ids and are shifted, so gas differs from pair to pair"""
    seqs = []
    for i, (nO, nH) in enumerate(shapes):
        q = grid_frame(nO, nH, 50 + i, frames=3)
        last = q['det_frame'] == 2
        q['tracks'] = np.where(last, q['tracks'][::-1], q['tracks'])
        q['det_box'] = np.where(last[:, None], q['det_box'] + np.float32([3, 0, 3, 0]), q['det_box'])
        seqs.append(q)
    return seqs


def test_constants():
    assert ALPHAS.shape == (NA,) == (19,) and ALPHAS.dtype == np.float64 and EPS == 2.0 ** -52
    assert ALPHAS[9] == 0.5                                        # (numpy's arange lands on 0.5 exactly: the threshold edge below)


def test_perfect_tracking():
    r = host(perfect_sequence())
    for k in FIGURES:
        assert np.array_equal(r[k], np.ones(NA)), k
        assert r[k.lower()] == 1.0
    assert r['HOTA(0)'] == r['LocA(0)'] == r['HOTALocA(0)'] == 1.0
    assert np.array_equal(r['tp'], np.full(NA, 120)) and r['gt_dets'] == r['tracker_dets'] == 120
    assert (r['objects'], r['hypotheses']) == (4, 4) and not r['fn'].any() and not r['fp'].any()
    assert np.array_equal(r['loc_sum'], np.full(NA, 120.0)) and np.array_equal(r['ass_a_num'], np.full(NA, 120.0))


def test_identity_swap():
    r = host(swap_sequence())
    assert np.array_equal(r['DetA'], np.ones(NA)) and np.array_equal(r['LocA'], np.ones(NA))
    assert np.array_equal(r['tp'], np.full(NA, 20))
    # every TP has TPA = 5, FNA = 5, FPA = 5: 20 x 5 / 15 summed as 4 pairs of m = 5 -> 4 x 5 x (5 / 15)
    assert np.allclose(r['AssA'], 1 / 3, rtol=0, atol=1e-15) and np.allclose(r['AssRe'], 0.5) and np.allclose(r['AssPr'], 0.5)
    assert np.allclose(r['HOTA'], np.sqrt(1 / 3), rtol=0, atol=1e-15)
    assert abs(r['hota'] - 0.5773502691896257) < 1e-15 and r['deta'] == 1.0 and r['loca'] == 1.0


def test_threshold_edge():
    q = edge_sequence()
    assert hota_sim_host(q['gt_box'], q['det_box'])[0, 0] == 0.5
    r = host(q)
    assert r['tp'].tolist() == [1] * 10 + [0] * 9                 # sim >= alpha - EPS: ALPHAS[9] is exactly 0.5
    assert r['fn'].tolist() == r['fp'].tolist() == [0] * 10 + [1] * 9
    assert np.array_equal(r['loc_sum'], np.array([0.5] * 10 + [0.0] * 9))
    assert np.array_equal(r['LocA'], np.array([0.5] * 10 + [1.0] * 9))


def test_sim_has_no_cut_and_no_nan():
    sim = hota_sim_host(np.float32([[0, 0, 10, 10], [0, 0, 0, 0]]), np.float32([[9, 9, 19, 19], [50, 50, 60, 60], [0, 0, 0, 0]]))
    assert sim[0, 0] == 1.0 / 199.0 and sim[0, 1] == 0.0 and not sim[1].any() and np.isfinite(sim).all()


def test_empty_sides():
    q = perfect_sequence(3, 6)
    none_kept = dict(q, tracks=np.full_like(q['tracks'], -1))
    r = host(none_kept)
    assert r['gt_dets'] == 18 and r['tracker_dets'] == 0 and r['hypotheses'] == 0 and r['fn'].tolist() == [18] * NA and not r['fp'].any()
    assert np.array_equal(r['LocA'], np.ones(NA)) and r['loca'] == 1.0
    assert all(not r[k].any() for k in FIGURES if k != 'LocA') and r['hota'] == r['deta'] == r['assa'] == 0.0
    no_gt = dict(q, gt_frame=q['gt_frame'][:0], gt_track=q['gt_track'][:0], gt_box=q['gt_box'][:0])
    r = host(no_gt)
    assert r['gt_dets'] == 0 and r['tracker_dets'] == 18 and r['objects'] == 0 and r['fp'].tolist() == [18] * NA and not r['fn'].any()
    assert np.array_equal(r['LocA'], np.ones(NA)) and all(not r[k].any() for k in FIGURES if k != 'LocA')
    r = host({k: v[:0] for k, v in q.items()})
    assert r['gt_dets'] == r['tracker_dets'] == 0 and np.array_equal(r['LocA'], np.ones(NA)) and r['hota'] == 0.0


def test_frames_with_one_side_only():
    """frames 0-1: GT only; 2-3: both; 4-5: detections only -- the one-sided frames count in gc / tc, fn and fp and are not assigned"""
    q = perfect_sequence(1, 6)
    keep_gt, keep_det = q['gt_frame'] < 4, q['det_frame'] >= 2
    q = {k: v[keep_det] if k in ('det_frame', 'det_box', 'tracks') else v[keep_gt] for k, v in q.items()}
    r = host(q)
    assert r['gt_dets'] == r['tracker_dets'] == 4 and r['tp'].tolist() == [2] * NA
    assert r['fn'].tolist() == r['fp'].tolist() == [2] * NA
    assert np.array_equal(r['DetA'], np.full(NA, 2 / 6)) and np.array_equal(r['LocA'], np.ones(NA))
    assert np.array_equal(r['ass_a_num'], np.full(NA, 2 * (2 / 6))) and np.array_equal(r['AssA'], np.full(NA, 2 * (2 / 6) / 2))
    assert np.array_equal(r['AssRe'], np.full(NA, 0.5)) and np.array_equal(r['AssPr'], np.full(NA, 0.5))


def test_overall():
    a, b = host(synth_hota_sequence(1, 12, objects=3)), host(synth_hota_sequence(2, 40, objects=5))
    assert a['tp'][0] != b['tp'][0] and a['tp'][0] > 0
    o = hota_overall([a, b])
    assert np.array_equal(o['tp'], a['tp'] + b['tp'])
    for k in ('gt_dets', 'tracker_dets', 'objects', 'hypotheses'):
        assert o[k] == a[k] + b[k]
    assert np.array_equal(o['fn'], a['fn'] + b['fn']) and np.array_equal(o['fp'], a['fp'] + b['fp'])
    tp = (a['tp'] + b['tp']).astype(np.float64)
    for k in ('AssA', 'AssRe', 'AssPr'):
        assert np.array_equal(o[k], (a[k] * a['tp'] + b[k] * b['tp']) / np.maximum(1, tp))
    assert np.array_equal(o['LocA'], np.maximum(1e-10, a['LocA'] * a['tp'] + b['LocA'] * b['tp']) / np.maximum(1e-10, tp))
    assert np.array_equal(o['DetA'], tp / np.maximum(1, tp + o['fn'] + o['fp']))
    assert np.array_equal(o['DetRe'], tp / np.maximum(1, o['gt_dets'])) and np.array_equal(o['DetPr'], tp / np.maximum(1, o['tracker_dets']))
    assert np.array_equal(o['HOTA'], np.sqrt(o['DetA'] * o['AssA'])) and np.array_equal(o['RHOTA'], np.sqrt(o['DetRe'] * o['AssA']))
    assert o['hota'] == float(np.cumsum(o['HOTA'])[-1] / NA) and o['HOTA(0)'] == o['HOTA'][0]
    one = hota_overall([a])                                        # a single sequence: its own figures up to the weighting's rounding
    assert np.allclose(one['HOTA'], a['HOTA'], rtol=1e-15, atol=0) and np.array_equal(one['DetA'], a['DetA'])
    empty = hota_overall([])
    assert empty['hota'] == 0.0 and np.array_equal(empty['LocA'], np.ones(NA))


def test_alpha_coverage():
    """the wide-jitter generator the device tests use has matched pairs between every two thresholds"""
    r = host(synth_hota_sequence(3, 60))
    assert (np.diff(r['tp']) < 0).all(), r['tp']
    assert r['tp'][0] > 300 and r['tp'][-1] > 0


def test_tied_scores_make_the_tie_rule_matter(monkeypatch):
    """The grid cases of the device tests have exact ties among positive scores: another optimal assignment (the solver run
    over the mirrored columns) gives another record, so a device solver without scipy's tie rules would not pass them."""
    import scipy.optimize
    plain = scipy.optimize.linear_sum_assignment

    def mirrored(cost):
        rows, cols = plain(np.asarray(cost)[:, ::-1])
        return rows, np.asarray(cost).shape[1] - 1 - cols
    seqs = [grid_frame(65, 64, 35)] + lds_switch_sequences(((31, 33), (32, 32), (33, 32)))
    refs = [host(q) for q in seqs]
    monkeypatch.setattr(scipy.optimize, 'linear_sum_assignment', mirrored)
    other = [host(q) for q in seqs]
    changed = [any(not np.array_equal(r[k], o[k]) for k in ('tp', 'loc_sum', 'ass_a_num')) for r, o in zip(refs, other)]
    assert sum(changed) >= 2, changed


def test_argument_errors():
    q = perfect_sequence(2, 3)
    with pytest.raises(ValueError, match='a hypothesis id occurs twice in frame 1'):
        host(dict(q, tracks=np.array([10, 11, 10, 10, 10, 11])))
    with pytest.raises(ValueError, match='a GT id occurs twice in frame 0'):
        host(dict(q, gt_track=np.array([2, 2, 2, 5, 2, 5])))
    with pytest.raises(ValueError, match='tracks: 5 entries for 6 rows'):
        host(dict(q, tracks=q['tracks'][:5]))
    with pytest.raises(ValueError, match='one box per row'):
        host(dict(q, gt_box=q['gt_box'][:5]))
    with pytest.raises(ValueError, match='integer values expected'):
        host(dict(q, tracks=q['tracks'].astype(np.float32)))
