"""The MOT-challenge summary on the device (csrc/moteval.hip: tmpnn_mot_summary; MotEvaluator(identity=True)) against the host
definition mot_summary_host.  Every comparison is exact: the integer fields are equal, and the ratios are equal as floats
because they are the same divisions of the same integers.  Shapes are the smallest at which the kernels can go wrong."""
import numpy as np
import pytest
import torch

from trackmpnn_amd import _lib
from trackmpnn_amd.moteval import (COUNT_KEYS, FLAG_LIMIT, SUMMARY_KEYS, MotEvaluator, mot_overall, mot_summary_host,
                                   sequence_from_counts, synth_mot_sequence)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARGS = ('det_frame', 'det_box', 'tracks', 'gt_frame', 'gt_track', 'gt_box')
IDENT_KEYS = ('idtp', 'idfp', 'idfn', 'idp', 'idr', 'idf1')


def host(q, tracks=None):
    return mot_summary_host(*[q[k] if k != 'tracks' or tracks is None else tracks for k in ARGS])


def bits(x):
    return np.float64(x).view(np.int64)


def same(dev, ref):
    """Every key of the host dict: integers equal, floats bit for bit (NaN included)."""
    return set(dev) == set(ref) and all(bits(dev[k]) == bits(ref[k]) if isinstance(ref[k], float) else dev[k] == ref[k] for k in ref)


def limits():
    lib = _lib.load()
    return [lib.tmpnn_mot_summary_limit(w) for w in (0, 1, 2)]     # objects in LDS, solver columns in LDS, frames per workgroup


def assert_equal_host(seqs, tracks=None):
    ev = MotEvaluator(seqs, DEV, identity=True)
    tracks = [q['tracks'] for q in seqs] if tracks is None else tracks
    ev.evaluate(tracks)
    per, overall = ev.read()
    refs = [None if t is None else host(q, t) for q, t in zip(seqs, tracks)]
    for s, (d, r) in enumerate(zip(per, refs)):
        assert (d is None and r is None) or same(d, r), f'sequence {s}: device {d} != host {r}'
    assert same(overall, mot_overall([r for r in refs if r is not None]))
    return refs, ev


def test_one_launch_over_eight_sequences():
    seqs = [synth_mot_sequence(300 + i, L, t0=(0, 3, -2)[i % 3], p_swap=0.15) for i, L in enumerate((1, 2, 17, 40, 41, 60, 33, 59))]
    seqs[2] = {k: v[:0] for k, v in seqs[2].items()}               # an empty sequence
    tracks = [q['tracks'] for q in seqs]
    tracks[4] = None                                               # one left out
    tracks[6] = np.full_like(tracks[6], -1)                        # one without a kept hypothesis
    refs, ev = assert_equal_host(seqs, tracks)
    live = [r for r in refs if r is not None]
    assert sum(r['fragmentations'] for r in live) > 0 and sum(r['idtp'] for r in live) > 100
    assert sum(r['idtp'] < r['matches'] for r in live) >= 3        # identities really change
    assert len({k for r in live for k in SUMMARY_KEYS[1:4] if r[k]}) >= 2
    assert refs[6]['idtp'] == 0 and refs[6]['mostly_lost'] == 6
    plain = MotEvaluator(seqs, DEV)                                # identity=False over the same tracks: the same CLEAR figures
    plain.evaluate(tracks)
    per_plain, overall_plain = plain.read()
    per, overall = ev.read()
    for d, p in zip(per + [overall], per_plain + [overall_plain]):
        assert (d is None and p is None) or (all(bits(d[k]) == bits(p[k]) for k in p) and 'idtp' not in p)


def test_arbitrary_hypothesis_ids():
    q0, q1 = synth_mot_sequence(21, 30, p_swap=0.2), synth_mot_sequence(22, 30, p_swap=0.2)

    def remap(tr, table):
        return np.where(tr >= 0, table[np.clip(tr, 0, None) % table.shape[0]], tr)
    rng = np.random.default_rng(4)
    big = 2 ** 31 - 1 - rng.permutation(997)                       # ids near 2^31 - 1 (997 is prime: one id per residue, none merged)
    sparse = rng.permutation(997).astype(np.int64) * 2000003 % (2 ** 31 - 1)
    assert np.unique(big).shape[0] == np.unique(sparse).shape[0] == 997
    t0, t1 = remap(q0['tracks'], big), remap(q1['tracks'], sparse)
    t1[::7] = -5                                                   # negative tracks take no part
    refs, ev = assert_equal_host([q0, q1, q0], [t0, t1, t0])       # the same ids in sequences 0 and 2: never merged
    assert same(refs[0], refs[2]) and refs[0]['idtp'] == host(q0)['idtp'] > 0
    rec = ev._out.cpu().numpy().copy()
    assert [int(x) for x in rec[:, 15]] == [np.unique(t[t >= 0]).shape[0] for t in (t0, t1, t0)]
    ev.evaluate([torch.from_numpy(t0).to(DEV), torch.from_numpy(t1).to(DEV).int(), torch.from_numpy(t0)])
    assert np.array_equal(ev._out.cpu().numpy(), rec)              # device tensors and host arrays: the same records


def lsa_sum(cnt):
    from scipy.optimize import linear_sum_assignment
    cnt = np.asarray(cnt)
    return int(cnt[linear_sum_assignment(cnt, maximize=True)].sum())


def test_solver_shapes():
    """Hypothesis counts around the wave and the workgroup (a thread owns columns t, t + 256, ...), both orientations, the
    greedy trap, all-equal counts (every optimum ties), and both sides of the LDS cap of the column state."""
    rng = np.random.default_rng(8)
    lds_col = limits()[1]
    cases = [np.array([[5, 4], [4, 0]]), np.ones((4, 6), np.int64), np.ones((6, 4), np.int64), np.full((5, 5), 2)]
    for n_hyp in (1, 63, 64, 65, 257):
        c = rng.integers(0, 3, (3, n_hyp))
        c[rng.integers(0, 3, n_hyp), np.arange(n_hyp)] |= 1        # every hypothesis exists
        c[:, 0] |= 1                                               # ... and every object
        cases.append(c)
    cases.append(rng.integers(1, 4, (9, 2)))                       # more objects than hypotheses: hypotheses are the rows
    cases.append(rng.integers(0, 4, (40, 37)) + np.eye(40, 37, dtype=np.int64))
    cases.append(rng.integers(0, 4, (37, 40)) + np.eye(37, 40, dtype=np.int64))
    for n_hyp in (lds_col, lds_col + 1):                           # column state in LDS / in the workspace
        c = np.zeros((3, n_hyp), np.int64)
        c[rng.integers(0, 3, n_hyp), np.arange(n_hyp)] = 1
        c[:, :3] += np.array([[1, 2, 0], [2, 1, 1], [0, 1, 2]])
        cases.append(c)
    seqs = [sequence_from_counts(c, hyp_ids=rng.permutation(c.shape[1]) * 3 + 5) for c in cases]
    refs, _ = assert_equal_host(seqs)
    assert [r['idtp'] for r in refs] == [lsa_sum(c) for c in cases]
    assert refs[0]['idtp'] == 8 and refs[1]['idtp'] == 4 and refs[2]['idtp'] == 4 and refs[3]['idtp'] == 10


def many_objects(n_obj, frames=10):
    """n_obj objects over `frames` frames, each present in two consecutive frames where the range allows; hypothesis ids swap
    between neighbours in odd frames and every third detection of frame 1 is missing (misses, fragment-free coverage)."""
    per = -(-n_obj // (frames - 1))
    q = {k: [] for k in ARGS}
    for t in range(frames):
        ids = np.concatenate([np.arange((t - 1) * per, min(t * per, n_obj)) if t else np.zeros(0, np.int64),
                              np.arange(t * per, min((t + 1) * per, n_obj)) if t < frames - 1 else np.zeros(0, np.int64)]).astype(np.int64)
        box = np.stack([150.0 * (ids % per), 200.0 * (ids // per % 2), 150.0 * (ids % per) + 100, 200.0 * (ids // per % 2) + 100], 1)
        keep = np.ones(ids.shape[0], bool) if t != 1 else np.arange(ids.shape[0]) % 3 != 0
        q['gt_frame'] += [t] * ids.shape[0]
        q['gt_track'] += list(ids)
        q['gt_box'].append(box.astype(np.float32))
        q['det_frame'] += [t] * int(keep.sum())
        q['tracks'] += list((ids ^ 1 if t % 2 else ids)[keep] * 2)
        q['det_box'].append(box[keep].astype(np.float32))
    return {k: np.concatenate(v) if k.endswith('box') else np.asarray(v, np.int64) for k, v in q.items()}


def test_object_state_on_both_sides_of_the_lds_table():
    lds_obj = limits()[0]
    seqs = [many_objects(lds_obj), many_objects(lds_obj + 1), synth_mot_sequence(5, 6)]
    assert [np.unique(q['gt_track']).shape[0] for q in seqs[:2]] == [lds_obj, lds_obj + 1]
    assert max(np.bincount(q['gt_frame']).max() for q in seqs[:2]) <= _lib.load().tmpnn_mot_max_per_frame()
    refs, _ = assert_equal_host(seqs)
    for r in refs[:2]:
        assert r['mostly_tracked'] > 0 and r['partially_tracked'] > 0 and r['switches'] > 0 and 0 < r['idtp'] < r['matches']


def test_frames_the_pair_kernel_splits_on():
    fpw = limits()[2]
    lens = (1, fpw - 1, fpw, fpw + 1, 3 * fpw + fpw // 2)
    seqs = [synth_mot_sequence(80 + i, L, p_swap=0.2, p_absent=0.0, p_miss=0.0) for i, L in enumerate(lens)]
    refs, _ = assert_equal_host(seqs)
    assert [r['frames'] for r in refs] == list(lens) and all(r['idtp'] > 0 for r in refs)


def test_fragmentations_and_coverage_by_hand():
    """tracked, tracked, miss, tracked -> 1 fragmentation; the same with the object absent from the GT in the gap -> 0."""
    def one(pattern):
        gt = [(t, 1) for t, ch in enumerate(pattern) if ch != '-'] + [(t, 9) for t in range(len(pattern))]
        det = [(t, 10, 1) for t, ch in enumerate(pattern) if ch == 'T'] + [(t, 90, 9) for t in range(len(pattern))]
        box = lambda o: [50.0 * o, 0, 50.0 * o + 10, 10]
        return {'gt_frame': np.array([g[0] for g in gt]), 'gt_track': np.array([g[1] for g in gt]),
                'gt_box': np.float32([box(g[1]) for g in gt]), 'det_frame': np.array([d[0] for d in det]),
                'tracks': np.array([d[1] for d in det]), 'det_box': np.float32([box(d[2]) for d in det])}
    pats = ['TTmT', 'TT-T', 'mmmm', 'mmTT', 'TmTmmTm', 'TTTTm', 'Tmmmm', 'Tmmmmmmmmm', 'TTTTTTTTTTTTmmm']
    refs, _ = assert_equal_host([one(p) for p in pats])
    assert [r['fragmentations'] for r in refs] == [1, 0, 0, 0, 2, 0, 0, 0, 0]
    assert [(r['mostly_tracked'] - 1, r['partially_tracked'], r['mostly_lost']) for r in refs[5:]] == [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0)]


def test_calling_behaviour():
    seqs = [synth_mot_sequence(40 + i, L, p_swap=0.2) for i, L in enumerate((9, 17, 30))]
    ev = MotEvaluator(seqs, DEV, identity=True)
    tracks = [q['tracks'] for q in seqs]
    other = [np.where(t >= 0, t % 3 + 5 * np.arange(t.shape[0]), -1) for t in tracks]
    ev.evaluate(tracks)
    rec1 = ev._out.cpu().numpy().copy()
    per1, _ = ev.read()
    ev.evaluate(other)                                             # other tracks: their own result, nothing stale in the counts
    per2, _ = ev.read()
    ev.evaluate(tracks)
    assert np.array_equal(ev._out.cpu().numpy(), rec1)             # the same tracks again: identical records
    for d1, d2, q, o in zip(per1, per2, seqs, other):
        assert same(d1, host(q)) and same(d2, host(q, o)) and d1['idtp'] != d2['idtp']


def test_a_flagged_sequence_has_no_identity_figures():
    cap = _lib.load().tmpnn_mot_max_per_frame()
    ok = synth_mot_sequence(7, 12)
    n = cap + 1                                                    # one frame with cap + 1 kept hypotheses
    box = np.stack([150.0 * np.arange(n), np.zeros(n), 150.0 * np.arange(n) + 100, np.full(n, 100.0)], 1).astype(np.float32)
    over = {'det_frame': np.zeros(n, np.int64), 'det_box': box, 'tracks': np.arange(n), 'gt_frame': np.zeros(3, np.int64),
            'gt_track': np.arange(3), 'gt_box': box[:3]}
    seqs = [ok, over, synth_mot_sequence(8, 5)]
    ev = MotEvaluator(seqs, DEV, identity=True)
    ev.evaluate([q['tracks'] for q in seqs])
    with pytest.raises(RuntimeError, match=rf'sequence 1, frame 0: a frame has more than {cap}'):
        ev.read()
    per, overall = ev.read(check=False)
    assert per[1]['flag'] & FLAG_LIMIT and not any(k in per[1] for k in IDENT_KEYS) and 'idtp' not in overall
    for s in (0, 2):                                               # the other sequences of the launch are unaffected
        assert per[s].pop('flag') == 0 and same(per[s], host(seqs[s]))
    tr = over['tracks'].copy()                                     # one hypothesis fewer with a track: the frame passes
    tr[100] = -1
    ev.evaluate([ok['tracks'], tr, seqs[2]['tracks']])
    per, _ = ev.read()
    assert same(per[1], host(over, tr)) and per[1]['idtp'] == 3


def test_validate_end_to_end():
    from trackmpnn_amd import TrackMPNN, validate
    from trackmpnn_amd.loops import infer_sequence
    seqs = []
    for i in range(2):
        q = synth_mot_sequence(70 + i, 24, objects=4)
        y = np.stack([q['det_frame'], q['tracks']], 1)
        q['y'] = torch.from_numpy(y)[None]
        q['X'] = torch.randn(1, y.shape[0], 8, generator=torch.Generator().manual_seed(700 + i))
        seqs.append(q)
    torch.manual_seed(9)
    model = TrackMPNN('2d', 3, 32, 0, 'diff').to(DEV).eval()
    gp = torch.Generator().manual_seed(17)
    with torch.no_grad():                                          # scores on both sides of 0.5
        for k, prm in model.named_parameters():
            prm.add_((0.1 * torch.randn(prm.shape, generator=gp)).to(DEV))
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_((0.5 * torch.randn(prm.shape, generator=gp)).to(DEV))
    out = validate(model, seqs, MotEvaluator(seqs, DEV, identity=True), cur_win_size=3)
    refs = [host(q, infer_sequence(model, q['X'], q['y'], 3, 0, False, DEV)[0][:, 1]) for q in seqs]
    for d, r in zip(out['per_sequence'], refs):
        assert same(d, r)
    ro = mot_overall(refs)
    assert all(bits(out[k]) == bits(ro[k]) for k in ro) and all(k in out for k in SUMMARY_KEYS + IDENT_KEYS)
    assert ro['predictions'] > 0 and ro['unique_objects'] == 8
