"""The frame-sorted packing under MotStore, EvalPrepStore and ResultStore (trackmpnn_amd/evalstore.py), host only.

One fixed set per store class: two seeded sequences (one starting at frame 3), a sequence with GT rows only, one with detection
rows only, one without rows, one whose frames arrive unsorted with two rows of one frame apart from each other, and one with
GT tracks of -1.  Two checks over it:

    the definition   stated here, without the code under test: for every frame of a sequence's range the sorted positions
                     off[f] : off[f + 1] are exactly the arrival indices of that frame, ascending (the GT side without a
                     permutation in the store is checked through the rows it carries); offsets run from 0 to the row count;
                     the bases in `seq` are the running sums
    the bytes        the SHA-256 of every packed array, recorded from the commit before the packing was moved into one module

and the five refusals of a CPU device, whose texts are literals recorded from that commit as well.
"""
import hashlib

import numpy as np
import pytest

from trackmpnn_amd.evalprep import GT_SCORED, KITTI_CAR, EvalPrep, EvalPrepStore, _gt_codes, synth_prep_sequence
from trackmpnn_amd.hota import HotaEvaluator
from trackmpnn_amd.mapeval import MapEvaluator
from trackmpnn_amd.moteval import MotEvaluator, MotStore, synth_mot_sequence
from trackmpnn_amd.results import KITTI_RESULT_RULES, ResultStore, TrackResults, score_keys, synth_result_sequence

MOT_ARRAYS = ('seq', 'gt_off', 'det_off', 'gt_id', 'gt_box', 'det_box', 'det_perm')
PREP_ARRAYS = ('seq', 'gt_off', 'det_off', 'gt_code', 'det_code', 'gt_box', 'det_box', 'det_perm')
RESULT_ARRAYS = ('seq', 'det_off', 'det_perm', 'det_fidx', 'det_cat', 'det_key', 'thr_key')

# recorded at e57d715 (the parent of the commit that added this file) by running these sets through its modules
SHA256 = {
    'MotStore': {
        'seq': '06150cb2a34a99d8dea3828f4e252f773b931ef177f48274e2c0cd28b40ec917',
        'gt_off': '8f268b6cf7501cfcb526cfaa41e334b75847ecb6f90531415d323a5ceebe9cb4',
        'det_off': '49a0d0112cdce05700d3e6855ec44e16977b6ca5cceb5fd7b599998cca1deeec',
        'gt_id': 'f4dc9615de7ce49fa3f7be73962c318f6012023930a70d08403a287972baa642',
        'gt_box': '758a0a7d4aabe5aac8f9ccd27c0cd2043dfb736ffda2080f17314359dd27c66f',
        'det_box': '1eaab02df0a4576bd2cfc2c01be7a14401dcd7408d5abce5f4db9224b965684f',
        'det_perm': '86129bc7dd4f25460abbca63475bbb1aa6c58c46da4d5d1f94683945fae3ea4e',
    },
    'EvalPrepStore': {
        'seq': 'b8fb2ab0041a2fc8b13bd7505dffb750c2b46117f3f3e91277e0efc26eaa1844',
        'gt_off': '240ea35d2b9d1ac24af5ab7a6dbf4cee83b35d2d117c1d4fa24a6603c5bb53a9',
        'det_off': '97142f38e2304b3b3bd0548e466b1a3e39995df4a5f5b1b89e532dbeddc41096',
        'gt_code': 'c021590d41dfd71eb654b21cb97a612e34cca400c24cdf6b6b89f84d90d6a3ee',
        'det_code': '4a7f1cca6f96e2c8d2ea2918b622e07518e354aea5dbab6263276e3902c2ac77',
        'gt_box': 'b72f6877608a4632f77ee123d5cab2df88e143d8477913b15ef94426ad994017',
        'det_box': 'a6c0e76b58c29abc0e4049f7e2712eecfc259c38ec78d151dfa61fb357fc9b4d',
        'det_perm': '8885778df02c99e548ada3a096cb32d0b137644ba5f5520e95349745a02fb587',
    },
    'ResultStore': {
        'seq': '340e5c3d47edc7f80794b0874f0c0de2014251f2d974e3fe8d1bb8f35b6a2dc9',
        'det_off': 'c4ac07655bcfc3bd202dc65e075603f6ac70a420f7f3619819dbe1de85e09c95',
        'det_perm': '2865378b6d7644280ffa1df01be47fd544d82df99abda1b796db9b24a1fbf677',
        'det_fidx': '74fccf695e02dcc8f5751aa66ca3340cc59dfec19316c65bd43a9c664135b049',
        'det_cat': '11f118d53a2c5884a3329713ae84c685aff9c0c391c2e8b1e830f039714af224',
        'det_key': 'b0a92c11f6df3b1fc466e3ce27b982a432ef0ed70190ba9417b188fd690a2922',
        'thr_key': '8aeaa42d6aae7dd2a7f600444b016de9ecf770914d9ada06f4bd22c81f53af5c',
    },
}


def boxes(n, first):
    """n distinct boxes: row i is recognisable by its x1 = first + i."""
    x = first + np.arange(n, dtype=np.float32)
    return np.stack([x, x + 1, x + 20, x + 30], 1).astype(np.float32)


def hand_sequence(det_frame, gt_frame, gt_track=None):
    """A sequence with the given frames, every row with a box of its own and every column the three stores read."""
    det_frame, gt_frame = np.asarray(det_frame, np.int64), np.asarray(gt_frame, np.int64)
    nd, ng = det_frame.shape[0], gt_frame.shape[0]
    return {'det_frame': det_frame, 'det_box': boxes(nd, 100), 'tracks': np.arange(nd, dtype=np.int64) + 50,
            'det_cat': np.asarray([2, 1, 3] * nd, np.int64)[:nd], 'det_score': (np.arange(nd) / 8 + 0.25).astype(np.float32),
            'gt_frame': gt_frame, 'gt_track': np.arange(ng, dtype=np.int64) * 2 + 1 if gt_track is None else np.asarray(gt_track, np.int64),
            'gt_box': boxes(ng, 500), 'gt_cat': np.asarray([2, 4, 9, 1] * ng, np.int64)[:ng],
            'gt_occ': np.asarray([0, 3, 1] * ng, np.int64)[:ng], 'gt_trunc': np.asarray([0, 0, 0, 1, 0] * ng, np.int64)[:ng]}


def hand_sequences():
    return [hand_sequence([], [4, 4, 6, 5]),                                           # rows on the GT side only
            hand_sequence([7, 9, 9, 8], []),                                           # rows on the detection side only
            hand_sequence([], []),                                                     # no rows at all
            hand_sequence([12, 10, 11, 10, 13, 12, 10], [11, 13, 10, 11, 10, 12, 11]),  # unsorted, the rows of a frame apart
            hand_sequence([2, 2, 3, 4, 4], [2, 3, 3, 2, 4, 4], gt_track=[5, -1, 7, -1, 5, -1])]


@pytest.fixture(scope='module')
def sets():
    """The sequences of every store class and the stores over them, built once and left unchanged."""
    seeded = dict(objects=3)
    mot = [synth_mot_sequence(11, 6, t0=3, **seeded), synth_mot_sequence(12, 6, **seeded)] + hand_sequences()
    prep = [synth_prep_sequence(11, 6, t0=3, **seeded), synth_prep_sequence(12, 6, **seeded)] + hand_sequences()
    res = [synth_result_sequence(11, 6)] + hand_sequences()
    return {'MotStore': (mot, MotStore(mot)), 'EvalPrepStore': (prep, EvalPrepStore(prep, KITTI_CAR)),
            'ResultStore': (res, ResultStore(res, KITTI_RESULT_RULES))}


def digests(store, names):
    """name -> SHA-256 over dtype, shape and bytes of the array."""
    out = {}
    for k in names:
        a = getattr(store, k)
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous, k
        out[k] = hashlib.sha256(f'{a.dtype.str}{a.shape}'.encode() + a.tobytes()).hexdigest()
    return out


def frames_of(frame, t0, nf, keep=None):
    """Per frame of the range the arrival indices of its rows, ascending -- the definition, by a scan per frame."""
    rows = np.arange(frame.shape[0]) if keep is None else np.where(keep)[0]
    return [rows[frame[rows] == t] for t in range(t0, t0 + nf)]


def union_range(q, sides):
    both = np.concatenate([q[k] for k in sides])
    return (int(both.min()), int(both.max()) - int(both.min()) + 1) if both.size else (0, 0)


def check_side(off, want, n_rows):
    """The offsets of one side of one sequence against the per-frame row lists `want`; returns the sorted order they imply."""
    assert off.dtype == np.int32 and off.shape[0] == len(want) + 1
    assert off[0] == 0 and off[-1] == n_rows == sum(w.shape[0] for w in want)
    assert [int(b - a) for a, b in zip(off[:-1], off[1:])] == [w.shape[0] for w in want]
    return np.concatenate(want + [np.zeros(0, np.int64)]).astype(np.int64)


def check_bases(seq, advance):
    """Columns 0, 2, 4, 6 are the running sums of what each sequence takes (`advance`: [S, 4])."""
    assert seq.dtype == np.int64 and seq.shape == (advance.shape[0], 8)
    run = np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(advance, 0)])
    assert np.array_equal(seq[:, 0::2], run[:-1])
    return run[-1]


def test_mot_store_is_the_frame_sorted_packing(sets):
    seqs, st = sets['MotStore']
    assert st.S == len(seqs)
    totals = check_bases(st.seq, np.stack([st.seq[:, 1], st.seq[:, 3], st.seq[:, 5] + 1, st.seq[:, 7]], 1))
    assert [st.n_gt, st.n_det, st.n_off, st.n_obj] == totals.tolist()
    assert [a.shape[0] for a in (st.gt_id, st.gt_box, st.det_box, st.det_perm, st.gt_off, st.det_off)] == [
        st.n_gt, st.n_gt, st.n_det, st.n_det, st.n_off, st.n_off]
    for s, q in enumerate(seqs):
        gb, ng, db, nd, ob, nf, _, n_obj = (int(v) for v in st.seq[s])
        assert (st.t0[s], nf) == union_range(q, ('det_frame', 'gt_frame'))
        do = check_side(st.det_off[ob:ob + nf + 1], frames_of(q['det_frame'], st.t0[s], nf), nd)
        assert nd == q['det_frame'].shape[0] and np.array_equal(st.det_perm[db:db + nd], do)
        assert np.array_equal(st.det_box[db:db + nd], q['det_box'][do])
        go = check_side(st.gt_off[ob:ob + nf + 1], frames_of(q['gt_frame'], st.t0[s], nf, q['gt_track'] >= 0), ng)
        assert ng == int((q['gt_track'] >= 0).sum())                  # (the dropped rows are absent)
        assert np.array_equal(st.gt_box[gb:gb + ng], q['gt_box'][go])
        assert n_obj == st.gt_ids[s].shape[0] and np.array_equal(st.gt_ids[s][st.gt_id[gb:gb + ng]], q['gt_track'][go])
    assert st.seq[6, 1] == 3 and st.seq[5].tolist()[1::2] == [7, 7, 4, 7]      # (the -1 rows went; the unsorted one as counted)


def test_evalprep_store_is_the_frame_sorted_packing(sets):
    seqs, st = sets['EvalPrepStore']
    assert st.S == len(seqs) and not st.seq[:, 6:].any()
    totals = check_bases(st.seq, np.stack([st.seq[:, 1], st.seq[:, 3], st.seq[:, 5] + 1, st.seq[:, 7]], 1))
    assert [st.n_gt, st.n_det, st.n_off, 0] == totals.tolist()
    assert [a.shape[0] for a in (st.gt_code, st.gt_box, st.det_code, st.det_box, st.det_perm, st.gt_off, st.det_off)] == [
        st.n_gt, st.n_gt, st.n_det, st.n_det, st.n_det, st.n_off, st.n_off]
    for s, q in enumerate(seqs):
        gb, ng, db, nd, ob, nf = (int(v) for v in st.seq[s, :6])
        assert (st.t0[s], nf) == union_range(q, ('det_frame', 'gt_frame'))
        do = check_side(st.det_off[ob:ob + nf + 1], frames_of(q['det_frame'], st.t0[s], nf), nd)
        assert nd == q['det_frame'].shape[0] and np.array_equal(st.det_perm[db:db + nd], do)
        assert np.array_equal(st.det_box[db:db + nd], q['det_box'][do])
        assert np.array_equal(st.det_code[db:db + nd], (q['det_cat'][do] == KITTI_CAR.cls).astype(np.uint8))
        go = check_side(st.gt_off[ob:ob + nf + 1], frames_of(q['gt_frame'], st.t0[s], nf), ng)
        assert ng == q['gt_frame'].shape[0]                           # (every row kept, a track of -1 included)
        code = _gt_codes(q['gt_cat'], q['gt_occ'], q['gt_trunc'], KITTI_CAR)
        assert np.array_equal(st.gt_box[gb:gb + ng], q['gt_box'][go]) and np.array_equal(st.gt_code[gb:gb + ng], code[go])
        assert np.array_equal(st.gt_keep[s], code == GT_SCORED)


def test_result_store_is_the_frame_sorted_packing(sets):
    seqs, st = sets['ResultStore']
    assert st.S == len(seqs) and not st.seq[:, 6:].any()
    totals = check_bases(st.seq, np.stack([st.seq[:, 1], st.seq[:, 3], st.seq[:, 5] + 1, st.seq[:, 7]], 1))
    assert [st.n_tab, st.n_det, st.n_off, 0] == totals.tolist()
    assert [a.shape[0] for a in (st.det_perm, st.det_fidx, st.det_cat, st.det_key, st.det_off)] == [st.n_det] * 4 + [st.n_off]
    for s, q in enumerate(seqs):
        _, n_tab, db, nd, ob, nf = (int(v) for v in st.seq[s, :6])
        t0, nf_want = union_range(q, ('det_frame',))
        assert nf == nf_want and st.t_range[s] == ((t0, t0 + nf - 1) if nd else None)
        assert n_tab == (0 if nd == 0 else max(256, 1 << int(2 * nd - 1).bit_length()))
        want = frames_of(q['det_frame'], t0, nf)
        do = check_side(st.det_off[ob:ob + nf + 1], want, nd)
        assert nd == q['det_frame'].shape[0] and np.array_equal(st.det_perm[db:db + nd], do)
        assert np.array_equal(st.det_fidx[db:db + nd], np.repeat(np.arange(nf), [w.shape[0] for w in want]))
        assert np.array_equal(st.det_cat[db:db + nd], q['det_cat']) and np.array_equal(st.det_key[db:db + nd], score_keys(q['det_score']))
        assert st.arrays[s]['det_frame'] is not None and np.array_equal(st.arrays[s]['det_box'], q['det_box'])


@pytest.mark.parametrize('cls,names', [('MotStore', MOT_ARRAYS), ('EvalPrepStore', PREP_ARRAYS), ('ResultStore', RESULT_ARRAYS)])
def test_packed_bytes_are_those_of_the_commit_before(sets, cls, names):
    got = digests(sets[cls][1], names)
    for k in names:
        print(f"        '{k}': '{got[k]}',")
    assert got == SHA256[cls]


NO_CPU = ' on cpu: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path): pass a cuda device, or '
REFUSALS = [                                                       # (the full texts of the same commit)
    (lambda q: MotEvaluator(q, 'cpu'), 'MotEvaluator' + NO_CPU + 'score on the host with mot_events_host'),
    (lambda q: HotaEvaluator(q, 'cpu'), 'HotaEvaluator' + NO_CPU + 'score on the host with hota_host'),
    (lambda q: EvalPrep(q, KITTI_CAR, 'cpu'), 'EvalPrep' + NO_CPU + 'filter on the host with evalprep_host'),
    (lambda q: TrackResults(q, KITTI_RESULT_RULES, 'cpu'), 'TrackResults' + NO_CPU + 'filter on the host with results_host'),
    (lambda q: MapEvaluator(q, 'cpu'), 'MapEvaluator' + NO_CPU + 'score on the host with map_host'),
]


@pytest.mark.parametrize('make,text', REFUSALS, ids=['MotEvaluator', 'HotaEvaluator', 'EvalPrep', 'TrackResults', 'MapEvaluator'])
def test_a_cpu_device_is_refused_before_anything_is_built(make, text):
    with pytest.raises(RuntimeError) as e:
        make([])
    print(repr(str(e.value)))
    assert str(e.value) == text
