"""The MOT evaluation on the device (csrc/moteval.hip: tmpnn_mot_events, tmpnn_mot_dist; trackmpnn_amd.moteval.MotEvaluator;
trackmpnn_amd.loops.validate) against the host definition mot_events_host: counts equal, distances and dist_sum bit for bit.
No tolerance anywhere."""
import numpy as np
import pytest
import torch

from trackmpnn_amd import _lib
from trackmpnn_amd.moteval import (COUNT_KEYS, FLAG_DUPLICATE, FLAG_LIMIT, MotEvaluator, mot_dist_host, mot_events_host, mot_overall,
                                   synth_mot_sequence)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def host(q, tracks=None):
    return mot_events_host(q['det_frame'], q['det_box'], q['tracks'] if tracks is None else tracks, q['gt_frame'], q['gt_track'],
                           q['gt_box'])


def bits(x):
    return np.float64(x).view(np.int64)


def same_record(dev, ref):
    return all(dev[k] == ref[k] for k in COUNT_KEYS) and bits(dev['dist_sum']) == bits(ref['dist_sum'])


def evaluate(seqs, tracks=None, check=True):
    ev = MotEvaluator(seqs, DEV)
    ev.evaluate([q['tracks'] for q in seqs] if tracks is None else tracks)
    return ev.read(check=check)


def assert_equal_host(seqs):
    per, overall = evaluate(seqs)
    refs = [host(q) for q in seqs]
    for s, (d, r) in enumerate(zip(per, refs)):
        assert same_record(d, r), f'sequence {s}: device {d} != host {r}'
    ro = mot_overall(refs)
    assert same_record(overall, ro) and bits(overall['mota']) == bits(ro['mota'])
    return refs


def B(x, y, w=10, h=10):
    return [x, y, x + w, y + h]


def test_mot_dist_equals_the_host_matrix():
    rng = np.random.default_rng(11)
    # 64 x 64 random boxes around 2 centres (so that a good part of the pairs overlap by more than half) + the special pairs
    c = rng.uniform(0, 400, (2, 2))[rng.integers(0, 2, 64)]

    def boxes():
        tl = c + rng.normal(0, 6, (64, 2))
        return np.concatenate([tl, tl + rng.uniform(40, 60, (64, 2))], 1).astype(np.float32)
    special = np.array([B(0, 0), B(50, 50), B(10, 0), B(2, 2, 4, 4), [5, 5, 5, 5], B(0, 0, 5, 10), B(0, 0, 4, 10), [7, 7, 7, 9]], np.float32)
    a, b = np.concatenate([boxes(), special]), np.concatenate([boxes(), special])
    ref = mot_dist_host(a, b)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    out = torch.full((a.shape[0], b.shape[0]), -7.0, dtype=torch.float64, device=DEV)
    _lib.call('tmpnn_mot_dist', ta.data_ptr(), a.shape[0], tb.data_ptr(), b.shape[0], out.data_ptr(), _lib.raw_stream(torch.device(DEV)))
    dev = out.cpu().numpy()
    nan = np.isnan(ref)
    assert 0.2 < (~nan[:64, :64]).mean() < 0.9                     # both kinds of entry in number
    assert np.array_equal(np.isnan(dev), nan)
    assert np.array_equal(dev[~nan].view(np.int64), ref[~nan].view(np.int64))
    s = 64                                                         # the special pairs, row box (0, 0, 10, 10)
    assert dev[s, s] == 0.0 and np.isnan(dev[s, s + 1]) and np.isnan(dev[s, s + 2]) and np.isnan(dev[s, s + 3])
    assert np.isnan(dev[s + 4, s + 4]) and np.isnan(dev[s + 7, s + 7])          # zero area: 0 / 0
    assert dev[s, s + 5] == 0.5 and np.isnan(dev[s, s + 6])        # IoU exactly 0.5 stays finite


def test_one_launch_over_eight_sequences():
    seqs = [synth_mot_sequence(100 + i, L, t0=(0, 3, -2)[i % 3]) for i, L in enumerate((1, 2, 3, 40, 40, 41, 64, 65))]
    refs = assert_equal_host(seqs)
    assert sum(r['switches'] for r in refs) > 0 and sum(r['false_positives'] for r in refs) > 0
    assert sum(r['misses'] for r in refs) > 0 and sum(r['matches'] for r in refs) > 1000
    assert [r['frames'] for r in refs] == [1, 2, 3, 40, 40, 41, 64, 65]


def crowd(seed, nO, nH, frames=2, spread=12.0, clusters=1):
    """Frames of nO GT boxes and nH hypotheses crowded into `clusters` places, so that most pairs of a place are finite: the
    assignment has real work.  Hypothesis ids are permuted from frame to frame (kept correspondences, switches)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 2000, (clusters, 2))

    def boxes(n):
        tl = centres[rng.integers(0, clusters, n)] + rng.normal(0, spread, (n, 2))
        return np.concatenate([tl, tl + 100 + rng.normal(0, 4, (n, 2))], 1).astype(np.float32)
    q = {k: [] for k in ('det_frame', 'det_box', 'tracks', 'gt_frame', 'gt_track', 'gt_box')}
    for t in range(frames):
        q['gt_frame'] += [t] * nO
        q['gt_track'] += list(range(nO))
        q['gt_box'].append(boxes(nO))
        q['det_frame'] += [t] * nH
        q['tracks'] += list(rng.permutation(nH) if t else np.arange(nH))
        q['det_box'].append(boxes(nH))
    return {k: np.concatenate(v) if k.endswith('box') else np.asarray(v, np.int64) for k, v in q.items()}


def test_solver_shapes():
    """1 x 1, the transposed 5 x 1, 63 / 64 / 65 columns (a lane owns columns l, l + 64, ...), the limit, and matrices on both
    sides of the LDS cap of 2048 entries (32 x 64 fits, 33 x 64 and everything larger lives in the workspace)."""
    shapes = [(1, 1), (1, 5), (5, 1), (40, 63), (40, 64), (40, 65), (63, 40), (65, 40), (64, 64), (32, 64), (33, 64), (130, 129),
              (256, 256)]
    seqs = [crowd(500 + i, nO, nH, clusters=1 if max(nO, nH) < 100 else 3) for i, (nO, nH) in enumerate(shapes)]
    refs = assert_equal_host(seqs)
    assert all(r['matches'] > 0 for r in refs) and sum(r['switches'] for r in refs) > 100


def tie_case(seed, nO, nH):
    """Frames 0 and 2: every box the same, so every cost is equal and the solver's tie rules alone choose the pairs.  Frame 1
    tells which pairs frame 0 chose: the objects stand apart and the hypothesis with id j stands on object perm[j], so an
    object keeps its hypothesis only where frame 0 gave it that one and is switched otherwise."""
    q = crowd(seed, nO, nH, frames=3)
    perm = np.random.default_rng(seed).permutation(max(nO, nH))
    q['gt_box'][:] = np.float32(B(10, 10, 50, 50))
    q['det_box'][:] = np.float32(B(12, 10, 50, 50))
    q['gt_box'][nO:2 * nO] = np.float32([B(200 * i, 0, 50, 50) for i in range(nO)])
    ids = q['tracks'][nH:2 * nH]
    q['det_box'][nH:2 * nH] = np.float32([B(200 * perm[j], 0 if perm[j] < nO else 5000, 50, 50) for j in ids])
    return q


def test_ties():
    """Duplicated boxes on both sides, equal costs everywhere: the device makes scipy's choice."""
    seqs = [tie_case(900 + i, nO, nH) for i, (nO, nH) in enumerate([(5, 7), (7, 5), (6, 6), (70, 66), (66, 70), (1, 3)])]
    q = crowd(950, 6, 9, frames=3)                                 # two groups of duplicates: two levels of cost
    q['gt_box'][:] = np.float32(B(10, 10, 50, 50))
    q['det_box'][::2] = np.float32(B(12, 10, 50, 50))
    q['det_box'][1::2] = np.float32(B(10, 13, 50, 50))
    seqs.append(q)
    refs = assert_equal_host(seqs)
    assert all(0 < r['switches'] for r in refs[:5]) and sum(r['matches'] - r['switches'] for r in refs[:5]) > 100


def test_limits():
    ok = synth_mot_sequence(7, 12)
    over = crowd(21, 3, 257, frames=1)
    at = crowd(22, 3, 256, frames=2)
    seqs = [ok, over, at, synth_mot_sequence(8, 5)]
    ev = MotEvaluator(seqs, DEV)
    ev.evaluate([q['tracks'] for q in seqs])
    with pytest.raises(RuntimeError, match=r'sequence 1, frame 0: a frame has more than 256'):
        ev.read()
    per, _ = ev.read(check=False)
    assert per[1]['flag'] & FLAG_LIMIT and [p['flag'] for i, p in enumerate(per) if i != 1] == [0, 0, 0]
    for s in (0, 2, 3):                                            # the other sequences of the launch are still correct
        assert same_record(per[s], host(seqs[s]))
    # one hypothesis fewer with a track: the frame passes
    tr = over['tracks'].copy()
    tr[100] = -1
    ev.evaluate([ok['tracks'], tr, at['tracks'], seqs[3]['tracks']])
    per, _ = ev.read()
    assert same_record(per[1], host(over, tr)) and per[1]['predictions'] == 256
    # a hypothesis id twice in a frame
    dup = ok['tracks'].copy()
    f = ok['det_frame']
    frames, n = np.unique(f[dup >= 0], return_counts=True)
    ft = int(frames[n >= 2][-1])
    i = np.where((f == ft) & (dup >= 0))[0]
    dup[i[1]] = dup[i[0]]
    with pytest.raises(ValueError, match=f'twice in frame {ft}'):
        host(ok, dup)
    ev.evaluate([dup, tr, at['tracks'], seqs[3]['tracks']])
    with pytest.raises(RuntimeError, match=rf'sequence 0, frame {ft}: a hypothesis id occurs twice'):
        ev.read()
    assert ev.read(check=False)[0][0]['flag'] & FLAG_DUPLICATE


def test_calling_behaviour():
    seqs = [synth_mot_sequence(40 + i, L) for i, L in enumerate((9, 17, 30))]
    ev = MotEvaluator(seqs, DEV)
    tracks = [q['tracks'] for q in seqs]
    ev.evaluate(tracks)
    rec1 = ev._out.cpu().numpy().copy()
    per1, _ = ev.read()
    ev.evaluate(tracks)
    assert np.array_equal(ev._out.cpu().numpy(), rec1)             # bit-identical records, dist_sum included
    # device tensors (int64 and int32), and a mix of device and host
    ev.evaluate([torch.from_numpy(t).to(DEV) for t in tracks])
    assert np.array_equal(ev._out.cpu().numpy(), rec1)
    ev.evaluate([torch.from_numpy(tracks[0]).to(DEV).int(), tracks[1], torch.from_numpy(tracks[2])])
    assert np.array_equal(ev._out.cpu().numpy(), rec1)
    # other tracks, then the first ones again: nothing is carried over from one evaluation to the next
    ev.evaluate([np.where(t >= 0, t % 3 + 5 * np.arange(t.shape[0]), -1) for t in tracks])
    assert not np.array_equal(ev._out.cpu().numpy(), rec1)
    ev.evaluate(tracks)
    assert np.array_equal(ev._out.cpu().numpy(), rec1)
    for d, q in zip(per1, seqs):
        assert same_record(d, host(q))
    # a sequence left out of an evaluation
    ev.evaluate([tracks[0], None, tracks[2]])
    per, overall = ev.read()
    assert per[1] is None and same_record(overall, mot_overall([per1[0], per1[2]]))
    with pytest.raises(ValueError):
        ev.evaluate(tracks[:2])
    with pytest.raises(ValueError):
        ev.evaluate([tracks[0][:-1], tracks[1], tracks[2]])


def test_many_objects_keep_their_state_in_the_workspace():
    """More objects than the LDS table holds (1024): the remembered hypothesis and last matched frame live in the workspace."""
    rng = np.random.default_rng(5)
    T, n = 20, 110                                                 # 110 objects per frame, new ids every other frame: 1100 in all
    q = {k: [] for k in ('det_frame', 'det_box', 'tracks', 'gt_frame', 'gt_track', 'gt_box')}
    tl = np.stack([np.arange(n) * 150.0, np.zeros(n)], 1)
    for t in range(T):
        box = np.concatenate([tl + t, tl + t + 100], 1).astype(np.float32)
        q['gt_frame'] += [t] * n
        q['gt_track'] += list(t // 2 * n + np.arange(n))
        q['gt_box'].append(box)
        q['det_frame'] += [t] * n
        # from frame 6 on the ids of neighbours swap in every odd frame: the kept correspondence is 150 px away, the
        # assignment takes the box at hand and counts a switch
        q['tracks'] += list(2 * (np.arange(n) ^ 1 if t >= 6 and t % 2 else np.arange(n)))
        q['det_box'].append(box + rng.normal(0, 2, (n, 4)).astype(np.float32))
    q = {k: np.concatenate(v) if k.endswith('box') else np.asarray(v, np.int64) for k, v in q.items()}
    assert np.unique(q['gt_track']).shape[0] > 1024
    r = assert_equal_host([q, synth_mot_sequence(1, 6)])[0]
    assert r['matches'] == T * n and r['switches'] > 0


@pytest.mark.parametrize('use_hungarian', [False, True])
def test_validate_end_to_end(use_hungarian):
    from trackmpnn_amd import TrackMPNN, validate
    from trackmpnn_amd.loops import infer_sequence
    seqs = []
    for i in range(3):
        q = synth_mot_sequence(70 + i, 30, objects=4)
        y = np.stack([q['det_frame'], q['tracks']], 1)
        q['y'] = torch.from_numpy(y)[None]
        q['X'] = torch.randn(1, y.shape[0], 8, generator=torch.Generator().manual_seed(700 + i))
        seqs.append(q)
    # a sequence without ground truth and one without detections: skipped (train.py:190-192)
    no_gt = dict(seqs[0], gt_frame=np.zeros(0, np.int64), gt_track=np.zeros(0, np.int64), gt_box=np.zeros((0, 4), np.float32))
    no_det = dict(seqs[1], det_frame=np.zeros(0, np.int64), det_box=np.zeros((0, 4), np.float32), tracks=np.zeros(0, np.int64),
                  y=torch.zeros(1, 0, 2, dtype=torch.int64), X=torch.zeros(1, 0, 8))
    seqs = [seqs[0], no_gt, seqs[1], no_det, seqs[2]]
    torch.manual_seed(9)
    model = TrackMPNN('2d', 3, 32, 0, 'diff').to(DEV)
    gp = torch.Generator().manual_seed(17)
    with torch.no_grad():                                          # scores on both sides of 0.5
        for k, prm in model.named_parameters():
            prm.add_((0.1 * torch.randn(prm.shape, generator=gp)).to(DEV))
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_((0.5 * torch.randn(prm.shape, generator=gp)).to(DEV))
    ev = MotEvaluator(seqs, DEV)
    model.train()
    out = validate(model, seqs, ev, cur_win_size=3, use_hungarian=use_hungarian)
    assert model.training                                          # the mode is restored ...
    model.eval()
    out2 = validate(model, seqs, ev, cur_win_size=3, use_hungarian=use_hungarian)
    assert not model.training                                      # ... whichever it was
    refs = []
    for q in (seqs[0], seqs[2], seqs[4]):
        y_out, ncalls, _ = infer_sequence(model, q['X'], q['y'], 3, 0, use_hungarian, DEV)
        assert ncalls > 0
        refs.append(host(q, y_out[:, 1]))
    per = out['per_sequence']
    assert per[1] is None and per[3] is None and len(out['motas']) == 3
    for d, r in zip((per[0], per[2], per[4]), refs):
        assert same_record(d, r)
    ro = mot_overall(refs)
    assert same_record(out, ro) and bits(out['mota']) == bits(ro['mota']) and bits(out['motp']) == bits(ro['motp'])
    assert [bits(a) for a in out['motas']] == [bits(r['mota']) for r in refs]
    assert ro['predictions'] > 0 and ro['objects'] > 0
    assert same_record(out2, ro)                                   # the same pass again: the same figures
