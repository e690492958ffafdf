"""The online tracker's host side (no GPU): the host definition of the feature rows against the detection store's tables and
against the reference's arithmetic restated literally, and the argument validation of FeatureSpec / OnlineTracker."""
import numpy as np
import pytest
import torch

from trackmpnn_amd import DetectionStore, FeatureSpec, OnlineTracker, TrackMPNN, online_features_host

FR_RANGE = 30


def _mantissa_f32(rng, n, scale):
    """float32 values with full 24-bit mantissas (random bit patterns in [1, 2), scaled by a non-power-of-two)."""
    bits = (rng.integers(0, 1 << 23, size=n, dtype=np.int64) | (127 << 23)).astype(np.uint32)
    return (bits.view(np.float32) - np.float32(1.0)) * np.float32(scale)


def _detections(seed, ncat, frames=41, per_frame=3):
    rng = np.random.default_rng(seed)
    frame = np.repeat(np.arange(frames), per_frame)            # (sorted: the store's stable sort keeps this order)
    n = frame.size
    x1, y1 = _mantissa_f32(rng, n, 1100.7), _mantissa_f32(rng, n, 330.3)
    w, h = _mantissa_f32(rng, n, 141.9) + np.float32(1.0), _mantissa_f32(rng, n, 93.1) + np.float32(1.0)
    box = np.stack([x1, y1, (x1 + w).astype(np.float32), (y1 + h).astype(np.float32)], 1).astype(np.float32)
    score = _mantissa_f32(rng, n, 0.999)
    cat = rng.integers(1, ncat + 1, size=n)
    return frame, cat, score, box


def _stats(seed, F):
    rng = np.random.default_rng(seed)
    return _mantissa_f32(rng, F, 3.3) - np.float32(1.1), _mantissa_f32(rng, F, 2.7) + np.float32(0.3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('feats', ['2d', '2d+temp'])
@pytest.mark.parametrize('ncat', [1, 8])
def test_host_rows_equal_the_detection_store_bit_for_bit(feats, ncat):
    """online_features_host == DetectionStore.stat[:, 0] (static columns) and DetectionStore.table[t mod fr_range] (temporal
    pair): the store's tables are the reference's arithmetic already; boxes and scores carry full float32 mantissas."""
    frame, cat, score, box = _detections(11 + ncat, ncat)
    F = ncat + 5 + (2 if 'temp' in feats else 0)
    mean, std = _stats(5 + ncat, F)
    seq = dict(frame=frame, track=np.full(frame.size, -1), cat=cat, box=box.astype(np.float64), score=score.astype(np.float64),
               width=1242, num_frames=int(frame.max()) + 1)
    store = DetectionStore([seq], ncat, feats, mean, std, fr_range=FR_RANGE, device=None)
    spec = FeatureSpec(ncat, feats, mean, std, fr_range=FR_RANGE)
    assert spec.F == F
    for t in range(int(frame.max()) + 1):                       # (41 frames: t mod fr_range wraps)
        sel = frame == t
        rows = online_features_host(spec, cat[sel], score[sel], box[sel], t)
        assert rows.dtype == np.float32 and rows.shape == (int(sel.sum()), F)
        assert np.array_equal(_bits(rows[:, :ncat + 5]), _bits(store.stat[sel, 0]))
        if 'temp' in feats:
            assert np.array_equal(_bits(rows[:, ncat + 5:]), _bits(np.broadcast_to(store.table[t % FR_RANGE], (rows.shape[0], 2))))


@pytest.mark.parametrize('feats', ['2d', '2d+temp', '2d+temp+vis'])
def test_host_rows_equal_the_reference_arithmetic_restated(feats):
    """dataset/kitti_mot.py:545-566 (and :414-420 for the temporal pair) written out on the reference's own bbox_pred layout
    [fr, -1, cat, -10, x1, y1, x2, y2, ..., score] in float32, frame by frame."""
    ncat = 8
    frame, cat, score, box = _detections(23, ncat, frames=35, per_frame=2)
    n = frame.size
    vis = _mantissa_f32(np.random.default_rng(4), n * 128, 0.01).reshape(n, 128) if 'vis' in feats else None
    spec_F = ncat + 5 + (2 if 'temp' in feats else 0) + (128 if 'vis' in feats else 0)
    mean, std = _stats(31, spec_F)
    bbox_pred = np.zeros((n, 16), dtype=np.float32)
    bbox_pred[:, 0], bbox_pred[:, 2], bbox_pred[:, 4:8], bbox_pred[:, 15] = frame, cat, box, score
    features = np.eye(ncat, dtype=np.float32)[bbox_pred[:, 2].astype('int64') - 1]
    two_d_feats = np.stack((bbox_pred[:, 15], (bbox_pred[:, 4] + bbox_pred[:, 6]) / 2.0, (bbox_pred[:, 5] + bbox_pred[:, 7]) / 2.0,
                            bbox_pred[:, 6] - bbox_pred[:, 4], bbox_pred[:, 7] - bbox_pred[:, 5]), axis=1)
    features = np.concatenate((features, two_d_feats), 1)
    if 'temp' in feats:
        tf = np.mod(bbox_pred[:, 0:1], FR_RANGE) * np.pi / FR_RANGE
        features = np.concatenate((features, np.concatenate((np.sin(tf), np.cos(tf)), axis=1)), 1)
    if 'vis' in feats:
        features = np.concatenate((features, vis), 1)
    assert features.dtype == np.float32
    want = (features - mean) / std
    spec = FeatureSpec(ncat, feats, mean, std, fr_range=FR_RANGE)
    got = np.concatenate([online_features_host(spec, cat[frame == t], score[frame == t], box[frame == t], t,
                                               None if vis is None else vis[frame == t]) for t in range(35)])
    assert np.array_equal(_bits(got), _bits(want))
    if vis is not None:                                         # the 'vis' columns are (v - m) / s in float32
        assert np.array_equal(_bits(got[:, -128:]), _bits((vis - mean[-128:]) / std[-128:]))


def test_empty_frame_gives_no_rows():
    spec = FeatureSpec(3, '2d+temp', np.zeros(10), np.ones(10))
    rows = online_features_host(spec, np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 4)), 7)
    assert rows.shape == (0, 10) and rows.dtype == np.float32


def test_feature_spec_validation():
    with pytest.raises(ValueError, match='mean / std of length'):
        FeatureSpec(3, '2d', np.zeros(9), np.ones(8))
    with pytest.raises(ValueError, match='mean / std of length'):
        FeatureSpec(3, '2d+temp', np.zeros(8), np.ones(8))
    with pytest.raises(ValueError, match='feats='):
        FeatureSpec(3, 'temp', np.zeros(2), np.ones(2))
    with pytest.raises(ValueError, match='std non-zero'):
        FeatureSpec(3, '2d', np.zeros(8), np.zeros(8))
    spec = FeatureSpec(3, '2d', np.zeros(8), np.ones(8))
    ok = dict(score=[0.5], box=[[0.0, 0.0, 1.0, 1.0]], t=0)
    for bad in (0, 4):
        with pytest.raises(ValueError, match='cat outside'):
            online_features_host(spec, [bad], **ok)
    with pytest.raises(ValueError, match='not finite'):
        online_features_host(spec, [1], [0.5], [[0.0, np.inf, 1.0, 1.0]], 0)
    with pytest.raises(ValueError, match='not finite'):
        online_features_host(spec, [1], [np.nan], [[0.0, 0.0, 1.0, 1.0]], 0)
    with pytest.raises(ValueError, match='vis given'):
        online_features_host(spec, [1], [0.5], [[0.0, 0.0, 1.0, 1.0]], 0, vis=np.zeros((1, 128)))


def test_online_tracker_validation_needs_no_gpu():
    model = TrackMPNN('2d', 3, 32, 0, 'diff').eval()
    spec = FeatureSpec(3, '2d', np.zeros(8), np.ones(8))
    with pytest.raises(ValueError, match='cur_win_size'):
        OnlineTracker(model, cur_win_size=1)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        OnlineTracker(model, device='cpu')
    with pytest.raises(ValueError, match='feature columns'):
        OnlineTracker(model, spec=FeatureSpec(3, '2d+temp', np.zeros(10), np.ones(10)))
    with pytest.raises(ValueError, match='eval mode'):
        OnlineTracker(TrackMPNN('2d', 3, 32, 0, 'diff'))
    trk = OnlineTracker(model)
    with pytest.raises(ValueError, match='FeatureSpec'):
        trk.push([1], [0.5], [[0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match='float32 expected'):
        trk.push_features(torch.zeros(2, 9))
    trk = OnlineTracker(model, spec=spec)
    with pytest.raises(ValueError, match='cat outside'):
        trk.push([4], [0.5], [[0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match='not finite'):
        trk.push([1], [0.5], [[0.0, 0.0, np.nan, 1.0]])
    assert (trk.frames, trk.ndets, trk.finalised_upto) == (0, 0, 0) and trk.tracks().shape == (0,)
    # the model is on the host: the first push that would touch the device refuses it
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        trk.push([1], [0.5], [[0.0, 0.0, 1.0, 1.0]])


def test_package_exports_the_online_api():
    import trackmpnn_amd
    from trackmpnn_amd import _lib
    for name in ('OnlineTracker', 'FeatureSpec', 'online_features_host'):
        assert name in trackmpnn_amd.__all__ and hasattr(trackmpnn_amd, name)
    assert 'tmpnn_online_features' in _lib._SIGNATURES and 'tmpnn_online_features' in _lib.header_symbols()
