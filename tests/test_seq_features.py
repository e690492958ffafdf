"""The whole-sequence sample on the host (trackmpnn_amd.seqfeat.sequence_features_host): against what the reference's dataset
classes hand out as `val` samples (tests/golden/seqfeat, tools/gen_seqfeat_golden.py), against draw_chunks_host on
whole-sequence chunks (an independent path to the same bits), and at the edges.  No device."""
import ctypes
import os

import numpy as np
import pytest

from tests.seqfeat_cases import FIXTURES, NCAT_KITTI, feature_stats, fixture_sequences, load_fixture, synth_store
from trackmpnn_amd import _lib
from trackmpnn_amd.chunks import DetectionStore, draw_chunks_host
from trackmpnn_amd.seqfeat import SequenceFeatures, listed_features_host, sequence_features_host


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize('name', FIXTURES)
def test_host_equals_the_references_val_sample(name):
    fx = load_fixture(name)
    seqs = fixture_sequences(fx)
    store = DetectionStore(seqs, int(fx['ncat']), str(fx['feats']), fx['mean'], fx['std'], fr_range=int(fx['fr_range']), device=None)
    assert store.F == fx['mean'].size
    for i, q in enumerate(seqs):
        ref_X, ref_y = fx[f's{i}_ref_features'], fx[f's{i}_ref_y']
        out = sequence_features_host(store, i)
        assert out.X.dtype == np.float32 and out.y.dtype == np.int64 and out.X.shape == ref_X.shape
        assert np.array_equal(bits(out.X), bits(ref_X)), f'sequence {i}: features differ from the reference'
        assert np.array_equal(out.y, ref_y.astype(np.int64))
    # the fixtures hold what the issue asks of them
    nf = [int(q['num_frames']) for q in seqs]
    assert max(nf) > int(fx['fr_range'])
    q = seqs[0]
    have = np.zeros(nf[0], bool)
    have[q['frame']] = True
    assert not have[0] and not have[-1] and (~have[1:-1]).any() and have.any()         # empty frames at the start, inside, at the end
    if name.startswith('kitti'):
        assert max(nf) > 256 and any(q['frame'].size == 1 for q in seqs)
        assert (np.diff(seqs[1]['frame']) < 0).any()                                    # (handed over unsorted)


@pytest.mark.parametrize('feats', ['2d', '2d+temp', '2d+temp+vis'])
def test_host_equals_the_plain_draw_of_a_whole_sequence_chunk(feats):
    store, seqs = synth_store(3, (1, 3, 40, 256), NCAT_KITTI, feats, empty=(0,))
    chunks = [(s, list(range(int(q['num_frames'])))) for s, q in enumerate(seqs)]
    for s in range(len(seqs)):
        hd = draw_chunks_host(store, chunks, [s], step=0, seed=0, random_transforms=False)
        out = sequence_features_host(store, s)
        assert hd.kept.all() and np.array_equal(bits(out.X), bits(hd.X)) and np.array_equal(out.y, hd.y)
        if store.vis:
            assert np.array_equal(bits(out.box), bits(hd.box)) and np.array_equal(bits(out.im_hw), bits(hd.im_hw))
            assert np.array_equal(out.frame, hd.map_of)            # (the plan's row of a whole-sequence chunk is the frame itself)
            assert not out.X[:, -128:].any()
        else:
            assert out.box is None and out.im_hw is None and out.frame is None
    assert sequence_features_host(store, 3).X.shape[0] > 256


def test_sequences_with_no_and_with_one_detection():
    mean, std = feature_stats(NCAT_KITTI, '2d+temp')
    none = dict(frame=np.zeros(0, np.int64), track=np.zeros(0, np.int64), cat=np.zeros(0, np.int64), box=np.zeros((0, 4)),
                score=np.zeros(0), width=1242, num_frames=5)
    one = dict(frame=np.asarray([4]), track=np.asarray([17]), cat=np.asarray([2]), box=np.asarray([[10.25, 20.5, 110.75, 90.0]]),
               score=np.asarray([0.9]), width=1242, num_frames=6)
    store = DetectionStore([none, one, none], NCAT_KITTI, '2d+temp', mean, std, device=None)
    for s in (0, 2):
        out = sequence_features_host(store, s)
        assert out.X.shape == (0, 10) and out.y.shape == (0, 2) and out.y.dtype == np.int64
    out = sequence_features_host(store, 1)
    raw = np.asarray([0, 1, 0, 0.9, (10.25 + 110.75) / 2, (20.5 + 90.0) / 2, 110.75 - 10.25, 90.0 - 20.5], np.float32)
    a = np.mod(np.asarray([4], np.float32), 30) * np.pi / 30
    pair = np.concatenate((np.sin(a), np.cos(a))).astype(np.float32)
    assert np.array_equal(bits(out.X), bits((np.concatenate([raw, pair])[None] - mean) / std))
    assert out.y.tolist() == [[4, 17]]
    assert [o.X.shape[0] for o in listed_features_host(store)] == [0, 1, 0]


def test_the_temporal_pair_wraps_at_fr_range():
    store, seqs = synth_store(5, (20,), NCAT_KITTI, '2d+temp', dets=(1, 3), fr_range=7)
    mean, std = feature_stats(NCAT_KITTI, '2d+temp')
    out = sequence_features_host(store, 0)
    fr = out.y[:, 0]
    assert fr.max() == 19 and (np.diff(fr) >= 0).all()
    # the reference's arithmetic on its float32 frame column (kitti_mot.py:414-420), row by row and without a table
    a = np.mod(fr.astype(np.float32)[:, None], 7) * np.pi / 7
    pair = np.concatenate((np.sin(a), np.cos(a)), axis=1).astype(np.float32)
    assert np.array_equal(bits(out.X[:, 8:]), bits((pair - mean[None, 8:]) / std[None, 8:]))
    first = {int(t): i for i, t in reversed(list(enumerate(fr)))}
    for t in (7, 14, 19):
        assert np.array_equal(bits(out.X[first[t], 8:]), bits(out.X[first[t % 7], 8:]))


def test_malformed_arguments_raise():
    store, seqs = synth_store(1, (4, 5, 6), NCAT_KITTI, '2d')
    for bad in (3, -1):
        with pytest.raises(IndexError, match='of 3'):
            sequence_features_host(store, bad)
    with pytest.raises(IndexError, match='sequence 7 of 3'):
        listed_features_host(store, [0, 7])
    with pytest.raises(ValueError, match='listed twice'):
        listed_features_host(store, [2, 0, 2])
    for bad in ([], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match='non-empty 1-d list of integers'):
            listed_features_host(store, bad)
    assert [o.y[:, 0].max(initial=-1) < n for o, n in zip(listed_features_host(store, [2, 0]), (6, 4))] == [True, True]
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        SequenceFeatures(store)                                        # (a host-only store: no CPU path)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        DetectionStore(seqs, 3, '2d', *feature_stats(NCAT_KITTI, '2d'), device='cpu')


def test_the_entry_point_validates_on_the_host():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.tmpnn_seq_features(None, None) == -1 and b'descriptor is null' in lib.tmpnn_last_error()
    d = _lib.CSeqFeatures()
    call = lambda: lib.tmpnn_seq_features(ctypes.byref(d), None)
    d.K, d.nseq, d.F, d.Fs, d.ldx, d.fr_range, d.nframes = 2, 1, 8, 8, 8, 30, 4
    assert call() == -1 and b'K=2 nseq=1' in lib.tmpnn_last_error()
    d.K, d.F = 1, 9
    assert call() == -1 and b'F = Fs or Fs + 2' in lib.tmpnn_last_error()
    d.F, d.ldx = 10, 9
    assert call() == -1 and b'ldx=9' in lib.tmpnn_last_error()
    d.ldx, d.ndets, d.n_rows = 138, 5, 6
    assert call() == -1 and b'n_rows=6' in lib.tmpnn_last_error()
    d.n_rows = 5
    assert call() == -1 and b'null pointer' in lib.tmpnn_last_error()
    # (every table present, an output missing; then y off its 16-byte boundary, a box off its own: still no launch)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p += p % 16
    for f in ('seqs', 'offsets', 'seq_base', 'first', 'frame', 'track', 'stat', 'table', 'flag'):
        setattr(d, f, p)
    assert call() == -1 and b'null pointer' in lib.tmpnn_last_error()
    d.X, d.y = p, p + 8
    assert call() == -1 and b'y is not 16-byte aligned' in lib.tmpnn_last_error()
    d.y, d.box = p, p + 4
    assert call() == -1 and b'frames_per_batch=0' in lib.tmpnn_last_error()
    d.frames_per_batch = 8
    assert call() == -1 and b"the 'vis' arguments" in lib.tmpnn_last_error()
    d.seq_hw, d.o_box, d.o_im_hw, d.o_map_of = p, p, p, p
    assert call() == -1 and b'box or o_box is not 16-byte aligned' in lib.tmpnn_last_error()
