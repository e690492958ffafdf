"""The benchmark preprocessing on the device (csrc/evalprep.hip: tmpnn_evalprep; EvalPrep) against the host definition
evalprep_host.  Every comparison is exact: tracks_out, every count, every flag.  The sequences are tests/test_evalprep.py's
prep_set(): the smallest shapes at which the kernel can go wrong (0 and 1 rows on either side, the lane boundary, tall and wide
frames, both sides of the LDS score limit, the per-frame limit)."""
import numpy as np
import pytest
import torch

from tests.test_evalprep import prep_set
from trackmpnn_amd import _lib
from trackmpnn_amd.evalprep import (COUNT_KEYS, FRAMES_PER_GROUP, KITTI_CAR, KITTI_PEDESTRIAN, LDS_SCORE, MAX_PER_FRAME, EvalPrep,
                                    PrepRules, evalprep_host, prep_overall, synth_prep_sequence)
from trackmpnn_amd.hota import HotaEvaluator, hota_host, hota_overall
from trackmpnn_amd.moteval import FLAG_LIMIT, MotEvaluator, mot_overall, mot_summary_host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


def same(dev, ref):
    """Every key of the host dict: integers equal, floats bit for bit."""
    if set(dev) != set(ref):
        return False
    for k, v in ref.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float64 or isinstance(v, float):
            if not np.array_equal(bits(dev[k]), bits(v)):
                return False
        elif not np.array_equal(dev[k], v):
            return False
    return True


@pytest.fixture(scope='module')
def prep_ref():
    """The set and the host definition over it, computed once and left unchanged."""
    qs = prep_set()
    return qs, [evalprep_host(q, q['tracks'], KITTI_CAR) for q in qs]


def assert_equal_host(ep, seqs, refs, tracks=None):
    tracks = [q['tracks'] for q in seqs] if tracks is None else tracks
    ep.apply(tracks)
    filt = [f.cpu().numpy() for f in ep.filtered_tracks()]
    per, overall = ep.read()
    for s, (f, c, r, t) in enumerate(zip(filt, per, refs, tracks)):
        assert f.dtype == np.int32 and f.shape == seqs[s]['tracks'].shape
        if t is None:
            assert c is None and (f == -1).all(), f'sequence {s}'
        else:
            assert np.array_equal(f, r[0]), f'sequence {s}: {int((f != r[0]).sum())} rows of tracks_out differ from the host'
            assert c == r[2], f'sequence {s}: {c} != {r[2]}'
    assert overall == prep_overall([r[2] for r, t in zip(refs, tracks) if t is not None])


def test_the_library_and_the_module_agree_on_the_limits():
    assert _lib.load().tmpnn_evalprep_max_per_frame() == MAX_PER_FRAME == 256 and LDS_SCORE == 1024 and FRAMES_PER_GROUP == 8


def test_equal_to_the_host_on_every_shape(prep_ref):
    """one launch over the whole set: different frame ranges, gaps, shuffled arrival, every shaped frame, 256 rows accepted"""
    seqs, refs = prep_ref
    ep = EvalPrep(seqs, KITTI_CAR, DEV)
    assert_equal_host(ep, seqs, refs)
    assert sum(r[2]['kept'] for r in refs) > 0


def test_none_device_and_host_tracks_and_two_applies(prep_ref):
    seqs, refs = prep_ref
    seqs, refs = seqs[:4], list(refs[:4])
    ep = EvalPrep(seqs, KITTI_CAR, DEV)
    # the first call: other tracks (every id shifted, every third row without a track)
    first = [np.where(np.arange(q['tracks'].shape[0]) % 3 == 0, -1, q['tracks'] + 5) for q in seqs]
    assert_equal_host(ep, seqs, [evalprep_host(q, t, KITTI_CAR) for q, t in zip(seqs, first)], first)
    # the second call on the same object gives the second call's result: one left out, one device tensor (int64), host arrays
    tracks = [None, torch.from_numpy(seqs[1]['tracks']).to(DEV), seqs[2]['tracks'], seqs[3]['tracks'].astype(np.int32)]
    assert_equal_host(ep, seqs, refs, tracks)
    assert_equal_host(ep, seqs, refs)


def test_an_empty_store_and_an_empty_sequence():
    ep = EvalPrep([], KITTI_CAR, DEV)
    ep.apply([])
    assert ep.read() == ([], prep_overall([])) and ep.filtered_tracks() == []
    seqs = [synth_prep_sequence(1, 0), synth_prep_sequence(2, 3)]
    assert seqs[0]['tracks'].shape[0] == 0
    assert_equal_host(EvalPrep(seqs, KITTI_CAR, DEV), seqs, [evalprep_host(q, q['tracks'], KITTI_CAR) for q in seqs])
    with pytest.raises(RuntimeError, match='no apply has been enqueued'):
        EvalPrep(seqs, KITTI_CAR, DEV).read()
    with pytest.raises(ValueError, match='1 track arrays for 2 sequences'):
        EvalPrep(seqs, KITTI_CAR, DEV).apply([None])


def test_other_rules(prep_ref):
    seqs = prep_ref[0][:3]
    off = PrepRules(2, (), None, max_occlusion=10 ** 9, max_truncation=10 ** 9, min_height=-np.inf)
    for rules in (off, PrepRules(2, (4, 3), 9, max_occlusion=0, max_truncation=5, min_height=40.0)):
        assert_equal_host(EvalPrep(seqs, rules, DEV), seqs, [evalprep_host(q, q['tracks'], rules) for q in seqs])
    ped = [synth_prep_sequence(9, 12, rules=KITTI_PEDESTRIAN, shuffle=True)]
    ref = [evalprep_host(q, q['tracks'], KITTI_PEDESTRIAN) for q in ped]
    assert ref[0][2]['removed_distractor'] > 0
    assert_equal_host(EvalPrep(ped, KITTI_PEDESTRIAN, DEV), ped, ref)


def test_a_frame_beyond_the_limit_flags_its_sequence_only():
    exact = dict(p_untracked=0.0, p_wrong=0.0, others=0)
    seqs = [synth_prep_sequence(1, 6),
            synth_prep_sequence(2, 0, objects=4, distractors=2, regions=0, sizes=[(3, 3), (2, 2), (6, MAX_PER_FRAME + 1), (1, 1)], t0=4, **exact),
            synth_prep_sequence(3, 0, objects=200, distractors=56, regions=1, sizes=[(2, 2), (MAX_PER_FRAME, 5)], **exact),
            synth_prep_sequence(4, 9, shuffle=True)]
    assert int((seqs[1]['det_frame'] == 6).sum()) == 257 and int((seqs[2]['gt_frame'] == 1).sum()) == 257
    refs = [evalprep_host(q, q['tracks'], KITTI_CAR) for q in seqs]               # (the host definition has no limit)
    ep = EvalPrep(seqs, KITTI_CAR, DEV)
    ep.apply([q['tracks'] for q in seqs])
    with pytest.raises(RuntimeError, match=r'sequence 1, frame 6: a frame has more than 256 detection rows or GT rows; sequence 2, frame 1: a frame'):
        ep.read()
    per, _ = ep.read(check=False)
    assert [p['flag'] for p in per] == [0, FLAG_LIMIT | (3 << 8), FLAG_LIMIT | (2 << 8), 0]
    filt = ep.filtered_tracks()
    for s in (0, 3):
        assert np.array_equal(filt[s].cpu().numpy(), refs[s][0])
        assert {k: per[s][k] for k in COUNT_KEYS} == refs[s][2]


def test_through_to_the_figures(prep_ref):
    """HotaEvaluator / MotEvaluator(identity=True) over eval_sequences(), scoring filtered_tracks() on the device, equal the host
    definitions on the host-filtered rows bit for bit"""
    seqs, refs = prep_ref
    pick = (0, 1, 2, 6)
    seqs, refs = [seqs[i] for i in pick], [refs[i] for i in pick]
    ep = EvalPrep(seqs, KITTI_CAR, DEV)
    es = ep.eval_sequences()
    for q, e, r in zip(seqs, es, refs):
        assert e['gt_frame'].shape[0] == int(r[1].sum()) < q['gt_frame'].shape[0]
    hev, mev = HotaEvaluator(es, DEV), MotEvaluator(es, DEV, identity=True)
    ep.apply([q['tracks'] for q in seqs])
    hev.evaluate(ep.filtered_tracks())
    mev.evaluate(ep.filtered_tracks())
    hper, hall = hev.read()
    mper, mall = mev.read()
    args = lambda e, r: (e['det_frame'], e['det_box'], r[0], e['gt_frame'], e['gt_track'], e['gt_box'])
    href = [hota_host(*args(e, r)) for e, r in zip(es, refs)]
    mref = [mot_summary_host(*args(e, r)) for e, r in zip(es, refs)]
    for s in range(len(seqs)):
        assert same(hper[s], href[s]) and same(mper[s], mref[s]), f'sequence {s}'
    assert same(hall, hota_overall(href)) and same(mall, mot_overall(mref))
    # the stage matters: the rows as they are given score otherwise
    plain = MotEvaluator(es, DEV)
    plain.evaluate([q['tracks'] for q in seqs])
    assert plain.read()[1]['predictions'] > mall['predictions'] == sum(r[2]['kept'] for r in refs)


def test_validate_with_prep_equals_the_composition_by_hand():
    from tests.test_track_results_gpu import infer_fixture
    from trackmpnn_amd import validate
    from trackmpnn_amd.loops import infer_sequence
    gold, m, model, seq = infer_fixture()
    rng = np.random.default_rng(9)
    y_ref = gold.d[f'd{gold.ncalls - 1}/y_out']
    gt = np.where(y_ref[:, 1] >= 0)[0]                              # a ground truth: the reference's tracks, jittered boxes
    ng = gt.shape[0]
    seq['det_cat'] = np.where(rng.random(seq['det_cat'].shape[0]) < 0.8, 2, 3)
    seq.update(gt_frame=seq['det_frame'][gt], gt_track=y_ref[gt, 1], gt_box=(seq['det_box'][gt] + rng.normal(0, 1, (ng, 4))).astype(np.float32),
               gt_cat=rng.choice([2, 2, 2, 4, 3], ng), gt_occ=rng.integers(0, 4, ng), gt_trunc=(rng.random(ng) < 0.1).astype(np.int64))
    args = (m['cur_win_size'], m['ret_win_size'], m['hungarian'], m.get('tp_classifier', True))
    ep = EvalPrep([seq], KITTI_CAR, DEV)
    es = ep.eval_sequences()
    plain = validate(model, es, MotEvaluator(es, DEV), *args)
    out = validate(model, es, MotEvaluator(es, DEV), *args, hota_evaluator=HotaEvaluator(es, DEV), prep=ep)
    y_out = infer_sequence(model, seq['X'], seq['y'], args[0], args[1], args[2], DEV, args[3])[0]
    ref = evalprep_host(seq, y_out[:, 1], KITTI_CAR)
    ev, hev = MotEvaluator(es, DEV), HotaEvaluator(es, DEV)
    ev.evaluate([ref[0]])                                            # validate of the host-filtered tracks
    hev.evaluate([ref[0]])
    overall, hall = ev.read()[1], hev.read()[1]
    assert out['prep'] == ref[2] and 0 < ref[2]['kept'] < ref[2]['rows_in']
    assert min(ref[2][k] for k in ('other_class', 'removed_distractor', 'removed_occluded')) > 0
    assert set(out) - set(plain) == {'prep', 'hota', 'deta', 'assa', 'loca', 'detre', 'detpr', 'assre', 'asspr', 'hota_per_sequence'}
    for k, v in overall.items():
        assert np.array_equal(bits(out[k]), bits(v)), k
    for k in ('hota', 'deta', 'assa', 'loca'):
        assert np.array_equal(bits(out[k]), bits(hall[k])), k
    assert out['predictions'] == ref[2]['kept'] < plain['predictions']
    # without prep nothing changes: the plain pass scores the rows as they are
    ev.evaluate([y_out[:, 1]])
    for k, v in ev.read()[1].items():
        assert np.array_equal(bits(plain[k]), bits(v)), k
    with pytest.raises(ValueError, match='prep was not built over the sequences'):
        validate(model, es, MotEvaluator(es, DEV), *args, prep=EvalPrep([synth_prep_sequence(1, 3)], KITTI_CAR, DEV))
