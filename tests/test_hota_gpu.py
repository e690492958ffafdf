"""HOTA on the device (csrc/hota.hip: tmpnn_hota; HotaEvaluator) against the host definition hota_host.  Every comparison is exact:
integers equal, every float64 of the record bit for bit (both sides are the same IEEE operations in the same order), and so are
the derived figures, which are host arithmetic on the record.  Shapes are the smallest at which the kernels can go wrong."""
import numpy as np
import pytest
import torch

from tests.test_hota import edge_sequence, grid_frame, lds_switch_sequences, perfect_sequence, swap_sequence
from trackmpnn_amd.hota import (FIGURES, FRAMES_PER_GROUP, LDS_SCORE, MAX_HOTA_PAIRS, NA, HotaEvaluator, hota_host, hota_overall,
                                synth_hota_sequence)
from trackmpnn_amd.moteval import FLAG_LIMIT, MAX_PER_FRAME, MotEvaluator

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARGS = ('det_frame', 'det_box', 'tracks', 'gt_frame', 'gt_track', 'gt_box')


def host(q, tracks=None):
    return hota_host(*[q[k] if k != 'tracks' or tracks is None else tracks for k in ARGS])


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


def same(dev, ref):
    """Every key of the host dict: integers equal, floats bit for bit."""
    if set(dev) != set(ref):
        return False
    for k, v in ref.items():
        d = dev[k]
        if isinstance(v, np.ndarray) and v.dtype == np.float64 or isinstance(v, float):
            if not np.array_equal(bits(d), bits(v)):
                return False
        elif not np.array_equal(d, v):
            return False
    return True


def diff(dev, ref):
    return {k: (dev.get(k), ref[k]) for k in ref if not same({k: dev.get(k)}, {k: ref[k]})}


def assert_equal_host(seqs, tracks=None):
    ev = HotaEvaluator(seqs, DEV)
    tracks = [q['tracks'] for q in seqs] if tracks is None else tracks
    ev.evaluate(tracks)
    per, overall = ev.read()
    refs = [None if t is None else host(q, t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for q, t in zip(seqs, tracks)]
    for s, (d, r) in enumerate(zip(per, refs)):
        assert (d is None and r is None) or same(d, r), f'sequence {s}: device != host in {diff(d, r)}'
    assert same(overall, hota_overall([r for r in refs if r is not None]))
    return refs, ev


def test_one_launch_over_eight_sequences():
    """lengths on both sides of the matching kernel's frame groups; an empty sequence, one left out, host and device tracks"""
    lens = (0, 1, 2, FRAMES_PER_GROUP - 1, FRAMES_PER_GROUP, FRAMES_PER_GROUP + 1, 40, 60)
    assert lens == (0, 1, 2, 7, 8, 9, 40, 60)
    seqs = [synth_hota_sequence(i, L) for i, L in enumerate(lens)]
    assert seqs[0]['det_frame'].size == 0
    tracks = [q['tracks'] for q in seqs]
    tracks[4] = None                                               # one left out
    for s in (2, 5, 7):
        tracks[s] = torch.from_numpy(tracks[s]).to(DEV)            # device int64
    tracks[6] = torch.from_numpy(tracks[6]).to(DEV).int()          # device int32
    refs, _ = assert_equal_host(seqs, tracks)
    assert (np.diff(refs[7]['tp']) < 0).all() and refs[7]['tp'][-1] > 0          # every threshold separates some pairs
    assert refs[0]['gt_dets'] == 0 and np.array_equal(refs[0]['LocA'], np.ones(NA))
    assert all(0 < refs[s]['hota'] < 1 and refs[s]['assa'] < 1 for s in (3, 5, 6, 7))


def test_arbitrary_hypothesis_ids():
    q0, q1 = synth_hota_sequence(21, 30, p_swap=0.2), synth_hota_sequence(22, 30, p_swap=0.2)

    def remap(tr, table):
        return np.where(tr >= 0, table[np.clip(tr, 0, None) % table.shape[0]], tr)
    rng = np.random.default_rng(4)
    big = 2 ** 31 - 2 - rng.permutation(997)                       # ids near 2^31 - 1 (997 is prime: one id per residue, none merged)
    big[np.unique(q0['tracks'][q0['tracks'] >= 0] % 997)[:2]] = (0, 2 ** 31 - 1)          # ... and the two ends of the range
    sparse = rng.permutation(997).astype(np.int64) * 2000003 % (2 ** 31 - 1)
    assert np.unique(big).shape[0] == np.unique(sparse).shape[0] == 997
    t0, t1 = remap(q0['tracks'], big), remap(q1['tracks'], sparse)
    assert t0.min() == -1 and 0 in t0 and t0.max() == 2 ** 31 - 1
    t1[::7] = -5                                                   # negative tracks take no part
    refs, ev = assert_equal_host([q0, q1, q0], [t0, t1, t0])       # the same ids in sequences 0 and 2: never merged
    assert same(refs[0], refs[2]) and same(refs[0], host(q0))      # the ids' values do not matter, their order of appearance does
    assert [r['hypotheses'] for r in refs] == [np.unique(t[t >= 0]).shape[0] for t in (t0, t1, t0)]
    rec = ev._out.cpu().numpy().copy()
    ev.evaluate([torch.from_numpy(t0).to(DEV), torch.from_numpy(t1).to(DEV).int(), torch.from_numpy(t0)])
    assert np.array_equal(ev._out.cpu().numpy(), rec)              # device tensors and host arrays: the same records


def test_solver_shapes():
    """single frames up to the per-frame limit, both orientations (the matrix is transposed when it has more rows than columns)"""
    shapes = ((1, 1), (1, 5), (5, 1), (3, 64), (64, 3), (65, 64), (MAX_PER_FRAME, MAX_PER_FRAME))
    assert MAX_PER_FRAME == 256
    seqs = [grid_frame(nO, nH, 30 + i) for i, (nO, nH) in enumerate(shapes)]
    refs, _ = assert_equal_host(seqs)
    assert [(r['gt_dets'], r['tracker_dets']) for r in refs] == list(shapes)
    assert all(r['tp'][0] > 0 for r in refs[3:]) and refs[6]['tp'][0] < MAX_PER_FRAME
    assert len({int(t) for r in refs for t in r['tp']}) > 6        # partial overlaps: the thresholds separate pairs


def test_scores_on_both_sides_of_the_lds_switch():
    """The one LDS / recompute switch of the kernels: a frame of up to LDS_SCORE = 1024 pairs keeps the solver's scores in LDS,
    a larger one recomputes them in the cost functor.  There is no switch on the number of objects or hypotheses of a sequence:
    pm, mc, gc and tc live in the workspace at every size (the 256 x 256 case of test_solver_shapes has 256 of each).  Three
    frames each, so that gas differs from pair to pair; tests/test_hota.py shows that the tie rule decides these records."""
    assert LDS_SCORE == 1024
    shapes = ((31, 33), (32, 32), (33, 32), (32, 33), (16, 64), (17, 64), (64, 17))
    assert sorted(a * b for a, b in shapes) == [1023, 1024, 1024, 1056, 1056, 1088, 1088]
    seqs = lds_switch_sequences(shapes)
    refs, _ = assert_equal_host(seqs)
    assert all(r['tp'][0] > 0 and 0 < r['assa'] < 1 for r in refs)


def test_a_frame_beyond_the_limit_flags_its_sequence_only():
    n = MAX_PER_FRAME + 1                                          # one frame with 257 GT rows
    box = np.stack([150.0 * np.arange(n), np.zeros(n), 150.0 * np.arange(n) + 100, np.full(n, 100.0)], 1).astype(np.float32)
    over = {'gt_frame': np.r_[0, np.ones(n, np.int64)], 'gt_track': np.r_[0, np.arange(n)], 'gt_box': np.r_[box[:1], box],
            'det_frame': np.array([0, 1, 1, 1]), 'tracks': np.arange(4), 'det_box': box[[0, 0, 1, 2]]}
    seqs = [synth_hota_sequence(7, 12), over, synth_hota_sequence(8, 5)]
    ev = HotaEvaluator(seqs, DEV)
    ev.evaluate([q['tracks'] for q in seqs])
    with pytest.raises(RuntimeError, match=rf'sequence 1, frame 1: a frame has more than {MAX_PER_FRAME}'):
        ev.read()
    per, _ = ev.read(check=False)
    assert per[1]['flag'] & FLAG_LIMIT and per[1]['flag'] >> 8 == 2
    for s in (0, 2):                                               # the other sequences of the launch are unaffected
        assert per[s].pop('flag') == 0 and same(per[s], host(seqs[s]))
    keep = np.r_[True, np.arange(n) != 100]                        # one GT row fewer: the frame passes
    ok = dict(over, gt_frame=over['gt_frame'][keep], gt_track=over['gt_track'][keep], gt_box=over['gt_box'][keep])
    refs, _ = assert_equal_host([ok])
    assert refs[0]['tp'][0] == 4 and refs[0]['gt_dets'] == MAX_PER_FRAME + 1


def test_a_duplicate_hypothesis_is_flagged():
    q = perfect_sequence(2, 3)
    ev = HotaEvaluator([q, q], DEV)
    ev.evaluate([q['tracks'], np.array([10, 11, 10, 10, 10, 11])])
    with pytest.raises(RuntimeError, match='sequence 1, frame 1: a hypothesis id occurs twice in one frame'):
        ev.read()
    with pytest.raises(ValueError, match='occurs twice in frame 1'):
        host(q, np.array([10, 11, 10, 10, 10, 11]))


def test_hand_cases_on_the_device():
    refs, _ = assert_equal_host([perfect_sequence(), swap_sequence(), edge_sequence()])
    for k in FIGURES:
        assert np.array_equal(refs[0][k], np.ones(NA))
    assert np.array_equal(refs[1]['DetA'], np.ones(NA)) and np.allclose(refs[1]['AssA'], 1 / 3, rtol=0, atol=1e-15)
    assert abs(refs[1]['hota'] - 0.5773502691896257) < 1e-15
    assert refs[2]['tp'].tolist() == [1] * 10 + [0] * 9


def test_empty_sides_on_the_device():
    q = perfect_sequence(3, 6)
    no_gt = dict(q, gt_frame=q['gt_frame'][:0], gt_track=q['gt_track'][:0], gt_box=q['gt_box'][:0])
    one_sided = {k: v[q['det_frame'] >= 2] if k in ('det_frame', 'det_box', 'tracks') else v[q['gt_frame'] < 4] for k, v in q.items()}
    refs, _ = assert_equal_host([q, no_gt, one_sided], [np.full_like(q['tracks'], -1), q['tracks'], one_sided['tracks']])
    assert refs[0]['fn'].tolist() == [18] * NA and refs[1]['fp'].tolist() == [18] * NA and refs[2]['tp'].tolist() == [6] * NA
    assert refs[2]['fn'].tolist() == refs[2]['fp'].tolist() == [6] * NA


def test_calling_behaviour():
    seqs = [synth_hota_sequence(40 + i, L, p_swap=0.2) for i, L in enumerate((9, 17, 30))]
    ev = HotaEvaluator(seqs, DEV)
    with pytest.raises(RuntimeError, match='no evaluation has been enqueued'):
        ev.read()
    with pytest.raises(ValueError, match='2 track arrays for 3 sequences'):
        ev.evaluate([q['tracks'] for q in seqs[:2]])
    tracks = [q['tracks'] for q in seqs]
    other = [np.where(t >= 0, t % 3 + 5 * np.arange(t.shape[0]), -1) for t in tracks]
    ev.evaluate(tracks)
    rec1 = ev._out.cpu().numpy().copy()
    per1, _ = ev.read()
    ev.evaluate(other)                                             # other tracks: their own result, the workspace is cleared
    per2, _ = ev.read()
    ev.evaluate(tracks)
    assert np.array_equal(ev._out.cpu().numpy(), rec1)             # the same tracks again: identical records
    for d1, d2, q, o in zip(per1, per2, seqs, other):
        assert same(d1, host(q)) and same(d2, host(q, o)) and d1['hypotheses'] != d2['hypotheses']
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        HotaEvaluator(seqs, 'cpu')


def test_pair_workspace_cap():
    n = 5100                                                       # 5100 objects x 5100 detections in one sequence
    assert n * n > MAX_HOTA_PAIRS == 2 ** 31 // 84
    q = {'gt_frame': np.arange(n) // 255, 'gt_track': np.arange(n), 'gt_box': np.zeros((n, 4), np.float32),
         'det_frame': np.arange(n) // 255, 'tracks': np.arange(n), 'det_box': np.zeros((n, 4), np.float32)}
    with pytest.raises(ValueError, match='MAX_HOTA_PAIRS.*hota_host'):
        HotaEvaluator([q], DEV)


def test_validate_end_to_end():
    from trackmpnn_amd import TrackMPNN, validate
    from trackmpnn_amd.loops import infer_sequence
    seqs = []
    for i in range(2):
        q = synth_hota_sequence(70 + i, 24, objects=4)
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
    before = validate(model, seqs, MotEvaluator(seqs, DEV, identity=True), cur_win_size=3)
    out = validate(model, seqs, MotEvaluator(seqs, DEV, identity=True), cur_win_size=3, hota_evaluator=HotaEvaluator(seqs, DEV))
    refs = [host(q, infer_sequence(model, q['X'], q['y'], 3, 0, False, DEV)[0][:, 1]) for q in seqs]
    ro = hota_overall(refs)
    assert ro['tracker_dets'] > 0 and ro['tp'][0] > 0
    for k in ('hota', 'deta', 'assa', 'loca', 'detre', 'detpr', 'assre', 'asspr'):
        assert bits(out[k]) == bits(ro[k]) and k not in before
    assert all(same(d, r) for d, r in zip(out['hota_per_sequence'], refs))
    assert set(out) - set(before) == {'hota', 'deta', 'assa', 'loca', 'detre', 'detpr', 'assre', 'asspr', 'hota_per_sequence'}
    for k, v in before.items():                                    # every key validate returned before is unchanged
        if k == 'per_sequence':
            assert all(set(a) == set(b) and all(np.array_equal(bits(a[x]), bits(b[x])) for x in a) for a, b in zip(v, out[k]))
        else:
            assert np.array_equal(bits(v), bits(out[k])), k
    with pytest.raises(ValueError, match='hota_evaluator was not built over the sequences'):
        validate(model, seqs, MotEvaluator(seqs, DEV), cur_win_size=3, hota_evaluator=HotaEvaluator(seqs[:1] * 2, DEV))
