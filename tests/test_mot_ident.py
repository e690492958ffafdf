"""The host definition of the rest of the MOT-challenge summary (trackmpnn_amd.moteval.mot_summary_host: track coverage,
fragmentations, the identity figures) and the argument checks of tmpnn_mot_summary -- no GPU.  tests/test_mot_ident_gpu.py
holds the device kernels to this definition."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import trackmpnn_amd
from trackmpnn_amd import _lib
from trackmpnn_amd.moteval import (MAX_PAIR_COUNTS, SUMMARY_KEYS, MotEvaluator, mot_dist_host, mot_events_host, mot_overall,
                                   mot_summary_host, sequence_from_counts, synth_mot_sequence)

ARGS = ('det_frame', 'det_box', 'tracks', 'gt_frame', 'gt_track', 'gt_box')
IDENT_KEYS = ('idtp', 'idfp', 'idfn', 'idp', 'idr', 'idf1')


def B(x, y, w=10, h=10):
    return [x, y, x + w, y + h]


def run(det, gt):
    """det: rows (frame, track, box); gt: rows (frame, id, box)."""
    return mot_summary_host([d[0] for d in det], [d[2] for d in det], [d[1] for d in det],
                            [g[0] for g in gt], [g[1] for g in gt], [g[2] for g in gt])


def events(pattern, first=0):
    """One object with one event per character: 'T' a frame with a hypothesis on it (tracked), 'm' a frame without one (miss),
    '-' a frame in which the object is absent from the GT (a second object keeps the frame range going)."""
    gt, det = [], []
    for t, ch in enumerate(pattern, first):
        gt.append((t, 9, B(500, 500)))
        det.append((t, 90, B(500, 500)))
        if ch != '-':
            gt.append((t, 1, B(0, 0)))
        if ch == 'T':
            det.append((t, 10, B(0, 0)))
    return run(det, gt)


def coverage(r):
    return tuple(r[k] for k in SUMMARY_KEYS)


def test_exported():
    assert trackmpnn_amd.mot_summary_host is mot_summary_host and 'mot_summary_host' in trackmpnn_amd.__all__


def test_fragmentation_hand_cases():
    # (object 9 is tracked in every frame: mostly tracked, no fragmentation)
    assert events('TTmT')['fragmentations'] == 1
    assert events('TT-T')['fragmentations'] == 0                   # absent from the GT in the gap: no event, no break
    r = events('mmmm')
    assert r['fragmentations'] == 0 and coverage(r) == (2, 1, 0, 1, 0)          # never tracked: mostly lost
    assert events('mmTT')['fragmentations'] == 0                   # a miss before the first tracked event does not count
    assert events('TTmm')['fragmentations'] == 0                   # ... nor one after the last
    assert events('TmTmmTm')['fragmentations'] == 2
    assert events('Tm-mT-T')['fragmentations'] == 1


def test_a_switch_is_a_tracked_event():
    gt = [(t, 1, B(0, 0)) for t in range(3)]
    det = [(0, 10, B(0, 0)), (1, 20, B(0, 0)), (2, 20, B(0, 0))]
    r = run(det, gt)
    assert r['switches'] == 1 and r['fragmentations'] == 0 and coverage(r) == (1, 1, 0, 0, 0)
    assert (r['idtp'], r['idfp'], r['idfn']) == (2, 1, 1)


@pytest.mark.parametrize('tracked,present,expect', [(4, 5, 'mostly_tracked'), (12, 15, 'mostly_tracked'), (1, 5, 'partially_tracked'),
                                                    (1, 10, 'mostly_lost'), (3, 5, 'partially_tracked'), (0, 3, 'mostly_lost'),
                                                    (5, 5, 'mostly_tracked')])
def test_coverage_thresholds(tracked, present, expect):
    """tracked / present in float64 against 0.8 and 0.2: 4 / 5 and 12 / 15 are >= 0.8, 1 / 5 is >= 0.2, 1 / 10 is below."""
    r = events('T' * tracked + 'm' * (present - tracked))
    want = {k: 0 for k in SUMMARY_KEYS[1:4]}
    want[expect] += 1
    want['mostly_tracked'] += 1                                    # (object 9)
    assert {k: r[k] for k in want} == want and r['unique_objects'] == 2


def brute_idtp(n):
    """The largest sum of n over injective maps of the smaller side into the larger (n >= 0: leaving a pair out never helps)."""
    n = n if n.shape[0] <= n.shape[1] else n.T
    best = 0
    for cols in itertools.permutations(range(n.shape[1]), n.shape[0]):
        best = max(best, int(sum(n[i, j] for i, j in enumerate(cols))))
    return best


def pair_counts(q):
    """n[o][h] and the per-object / per-hypothesis frame counts, straight from the definition."""
    gt_ok, tr_ok = q['gt_track'] >= 0, q['tracks'] >= 0
    oids, hids = np.unique(q['gt_track'][gt_ok]), np.unique(q['tracks'][tr_ok])
    n = np.zeros((oids.shape[0], hids.shape[0]), np.int64)
    for t in np.unique(np.concatenate([q['gt_frame'], q['det_frame']])):
        go, dh = np.where((q['gt_frame'] == t) & gt_ok)[0], np.where((q['det_frame'] == t) & tr_ok)[0]
        if go.size and dh.size:
            fin = np.isfinite(mot_dist_host(q['gt_box'][go], q['det_box'][dh]))
            for i, j in zip(*np.nonzero(fin)):
                n[np.searchsorted(oids, q['gt_track'][go[i]]), np.searchsorted(hids, q['tracks'][dh[j]])] += 1
    no = np.array([(q['gt_track'][gt_ok] == o).sum() for o in oids], np.int64)
    nh = np.array([(q['tracks'][tr_ok] == h).sum() for h in hids], np.int64)
    return n, no, nh


def padded_identity(n, no, nh):
    """idtp, idfp, idfn as py-motmetrics' id_global_assignment forms them: a min-cost assignment on the (|O| + |H|)^2 matrix of
    false-positive and false-negative counts, with dummy rows / columns for the unmatched and a forbidden rest."""
    from scipy.optimize import linear_sum_assignment
    O, H = n.shape
    big = 1e9                                                      # (stands for the NaN blocks)
    fp, fn = np.full((O + H, O + H), big), np.full((O + H, O + H), big)
    fp[:O, :H] = nh[None, :] - n
    fn[:O, :H] = no[:, None] - n
    fp[O:, :H] = np.where(np.eye(H, dtype=bool), nh[None, :], big)
    fn[O:, :H] = np.where(np.eye(H, dtype=bool), 0, big)
    fn[:O, H:] = np.where(np.eye(O, dtype=bool), no[:, None], big)
    fp[:O, H:] = np.where(np.eye(O, dtype=bool), 0, big)
    fp[O:, H:] = fn[O:, H:] = 0
    r, c = linear_sum_assignment(fp + fn)
    idfp, idfn = int(fp[r, c].sum()), int(fn[r, c].sum())
    return int(no.sum()) - idfn, idfp, idfn


def test_identity_against_an_independent_restatement():
    """>= 100 seeded sequences of <= 5 objects and <= 6 hypotheses: idtp by brute force over all injective maps, idfp / idfn
    through the padded assignment of py-motmetrics."""
    done = hard = 0
    for seed in range(400):
        rng = np.random.default_rng(seed)
        q = synth_mot_sequence(2000 + seed, int(rng.integers(3, 13)), objects=int(rng.integers(1, 6)), p_swap=0.35, stray_rate=0.1)
        n, no, nh = pair_counts(q)
        if n.shape[1] > 6 or n.size == 0:
            continue
        r = mot_summary_host(*[q[k] for k in ARGS])
        idtp = brute_idtp(n)
        assert r['idtp'] == idtp, f'seed {seed}'
        assert (r['idtp'], r['idfp'], r['idfn']) == padded_identity(n, no, nh), f'seed {seed}'
        assert r['idfp'] == r['predictions'] - idtp and r['idfn'] == r['objects'] - idtp
        assert r['idf1'] == 2 * idtp / (r['objects'] + r['predictions'])
        done += 1
        hard += int(n.max(1).sum() > idtp)                         # (the best column of every row is not a matching)
    assert done >= 100 and hard >= 10


def test_sequence_from_counts():
    cnt = np.array([[5, 4], [4, 0]])
    q = sequence_from_counts(cnt)
    assert np.array_equal(pair_counts(q)[0], cnt)
    r = mot_summary_host(*[q[k] for k in ARGS])
    assert r['idtp'] == 8 and r['objects'] == r['predictions'] == 13 and (r['idfp'], r['idfn']) == (5, 5)      # greedy: 5
    assert r['idp'] == r['idr'] == r['idf1'] == 8 / 13
    cnt = np.array([[1, 0, 2], [0, 3, 0], [2, 2, 2], [0, 0, 1]])
    q = sequence_from_counts(cnt, hyp_ids=[2 ** 31 - 1, 7, 0], t0=-3)
    assert np.array_equal(pair_counts(q)[0], cnt[:, [2, 1, 0]])   # (columns in ascending id)
    assert mot_summary_host(*[q[k] for k in ARGS])['idtp'] == brute_idtp(cnt) == 7


def test_degenerate_cases():
    gt = [(0, 1, B(0, 0)), (1, 1, B(0, 0))]
    r = run([], gt)                                                # no hypothesis at all
    assert (r['idtp'], r['idfp'], r['idfn'], r['idf1'], r['idr']) == (0, 0, 2, 0.0, 0.0) and math.isnan(r['idp'])
    assert coverage(r) == (1, 0, 0, 1, 0)
    r = run([(0, -1, B(0, 0)), (1, -1, B(0, 0))], gt)              # all tracks -1: the same
    assert (r['idtp'], r['idfp'], r['idfn'], r['idf1']) == (0, 0, 2, 0.0) and math.isnan(r['idp']) and coverage(r) == (1, 0, 0, 1, 0)
    r = run([(0, 10, B(0, 0)), (1, 10, B(0, 0))], [])              # no GT
    assert (r['idtp'], r['idfp'], r['idfn'], r['idf1'], r['idp']) == (0, 2, 0, 0.0, 0.0) and math.isnan(r['idr'])
    assert coverage(r) == (0, 0, 0, 0, 0)
    r = run([], [])
    assert r['idtp'] == 0 and all(math.isnan(r[k]) for k in ('idp', 'idr', 'idf1'))
    r = run([(0, 10, B(300, 300))], [(0, 1, B(0, 0))])             # both sides, no pair within reach
    assert (r['idtp'], r['idfp'], r['idfn'], r['idf1']) == (0, 1, 1, 0.0)


def test_events_are_unchanged_and_overall_sums():
    qs = [synth_mot_sequence(60 + i, 25, p_swap=0.2) for i in range(3)]
    full = [mot_summary_host(*[q[k] for k in ARGS]) for q in qs]
    for q, r in zip(qs, full):
        e = mot_events_host(*[q[k] for k in ARGS])
        assert list(e) == ['objects', 'predictions', 'matches', 'switches', 'false_positives', 'misses', 'frames', 'dist_sum', 'mota',
                           'motp', 'recall', 'precision']
        assert all(e[k] == r[k] for k in e)
        assert set(r) == set(e) | set(SUMMARY_KEYS) | set(IDENT_KEYS)
        assert r['mostly_tracked'] + r['partially_tracked'] + r['mostly_lost'] == r['unique_objects'] == 6
    o = mot_overall(full)
    for k in SUMMARY_KEYS + ('idtp', 'idfp', 'idfn', 'objects'):
        assert o[k] == sum(r[k] for r in full)
    assert o['idf1'] == 2 * o['idtp'] / (o['objects'] + o['predictions']) and o['idp'] == o['idtp'] / o['predictions']
    assert o['idr'] == o['idtp'] / o['objects'] and sum(r['fragmentations'] for r in full) > 0
    # dicts without the new keys (mot_events_host, or a flagged sequence without identity figures) are summed as before
    plain = mot_overall([mot_events_host(*[q[k] for k in ARGS]) for q in qs])
    assert set(plain) == set(mot_events_host(*[qs[0][k] for k in ARGS])) and all(plain[k] == o[k] for k in plain)
    mixed = mot_overall([full[0], {k: v for k, v in full[1].items() if k not in IDENT_KEYS}])
    assert 'idtp' not in mixed and 'idf1' not in mixed and mixed['fragmentations'] == full[0]['fragmentations'] + full[1]['fragmentations']


def test_constructor_cap_names_the_host_definition(monkeypatch):
    """The identity count matrices take objects x detections entries per sequence: beyond MAX_PAIR_COUNTS the constructor
    refuses (before anything touches the device)."""
    q = sequence_from_counts(np.ones((3, 4), np.int64))           # 3 objects x 12 detections
    monkeypatch.setattr('trackmpnn_amd.moteval.MAX_PAIR_COUNTS', 35)
    with pytest.raises(ValueError, match='MAX_PAIR_COUNTS.*mot_summary_host'):
        MotEvaluator([q], 'cuda:0', identity=True)
    assert MAX_PAIR_COUNTS == 2 ** 27
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        MotEvaluator([q], 'cpu', identity=True)


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    assert [lib.tmpnn_mot_summary_limit(w) for w in (-1, 3)] == [-1, -1]
    lds_obj, lds_col, frames = [lib.tmpnn_mot_summary_limit(w) for w in (0, 1, 2)]
    assert lds_obj >= 64 and lds_col >= 64 and frames >= 1
    assert lib.tmpnn_mot_summary(None, None, None, None, 0, None, None) == -1 and b'mot_summary: store is null' in lib.tmpnn_last_error()
    seq = np.array([[0, 2, 0, 3, 0, 4, 0, 2]], np.int64)
    one = C.c_void_p(256)                                          # (never dereferenced: every call below fails its checks)

    def store(**kw):
        f = dict(S=1, reserved=0, n_gt=2, n_det=3, n_off=5, n_obj=2, seq=one, gt_off=one, det_off=one, gt_id=one, gt_box=one,
                 det_box=one, det_perm=one)
        f.update(kw)
        return _lib.CMotStore(**f)

    def call(st, seq_host=seq, ws=one, ws_bytes=1 << 30):
        return lib.tmpnn_mot_summary(C.byref(st), seq_host.ctypes.data if seq_host is not None else None, one, ws, ws_bytes, one, None)
    assert call(store(S=-1)) == -1
    assert call(store(), seq_host=None) == -1 and b'null pointer' in lib.tmpnn_last_error()
    assert call(store(gt_box=None)) == -1 and b'null GT arrays' in lib.tmpnn_last_error()
    assert call(store(gt_box=C.c_void_p(260))) == -1 and b'16-byte aligned' in lib.tmpnn_last_error()
    assert call(store(n_det=2)) == -1 and b'detection rows' in lib.tmpnn_last_error()
    assert call(store(n_obj=1)) == -1 and b'objects' in lib.tmpnn_last_error()
    assert call(store(n_det=1 << 28), seq_host=seq) == -1 and b'detections' in lib.tmpnn_last_error()
    need = lib.tmpnn_mot_summary_ws(1, 2, 3, 6)
    assert need >= lib.tmpnn_mot_events_ws(1, 2, 3) + 4 * 6 + 4 * 4 * 2 + 4 * 3 * 4 * 3
    assert lib.tmpnn_mot_summary_ws(1, 2, 3, 7) > need - 16        # the count matrices are part of it
    assert call(store(), ws_bytes=need - 1) == -3 and b'workspace' in lib.tmpnn_last_error()
    assert call(store(), ws=None) == -3
    assert call(store(), ws=C.c_void_p(264)) == -1 and b'16-byte aligned' in lib.tmpnn_last_error()
    assert lib.tmpnn_mot_summary_ws(-1, 0, 0, 0) == 0 and lib.tmpnn_mot_summary_ws(1, 1, 1, -1) == 0
    assert lib.tmpnn_mot_summary_ws(1, 1, 1 << 28, 1) == 0 and lib.tmpnn_mot_summary_ws(1, 1, 1, 1 << 40) == 0
    assert lib.tmpnn_mot_summary(C.byref(store(S=0)), None, None, None, 0, None, None) == 0     # nothing to do, nothing launched
