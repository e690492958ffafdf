"""The frame resize without a GPU: the host definition (trackmpnn_amd.frames.resize_coeffs / resize_host / prep_host) against
Pillow's recorded output (tests/golden/resize, tools/gen_resize_golden.py) and, where Pillow imports, against Pillow itself at the
KITTI sizes; the host twin of FrameStore.from_raw; the argument checks of tmpnn_frames_resize; and the new ValueErrors of
OnlineVis / OnlineTracker."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from trackmpnn_amd import (FeatureSpec, FramePrep, FrameStore, OnlineTracker, OnlineVis, TrackMPNN, prep_host, resize_coeffs,
                           resize_host)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resize')
KITTI = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
KITTI_IN = (384, 1280)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def fixtures():
    paths = sorted(glob.glob(os.path.join(GOLDEN, '*.npz')))
    assert len(paths) == 8, f'{len(paths)} fixtures under {GOLDEN}'
    return paths


@pytest.fixture(scope='module')
def kitti_frames():
    rng = np.random.default_rng(42)
    return {hw: rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in KITTI}


@pytest.fixture(scope='module')
def kitti_resized(kitti_frames):
    return {hw: resize_host(a, KITTI_IN) for hw, a in kitti_frames.items()}


def test_resize_host_equals_every_fixture():
    for path in fixtures():
        d = np.load(path)
        got = resize_host(d['src'], d['out'].shape[1:3])
        assert got.dtype == np.uint8 and got.shape == d['out'].shape
        assert np.array_equal(got, d['out']), os.path.basename(path)
        # one frame alone equals its slice of the batch
        assert np.array_equal(resize_host(d['src'][0], d['out'].shape[1:3]), d['out'][0])


@pytest.mark.parametrize('hw', KITTI)
def test_resize_host_equals_pillow_at_the_kitti_sizes(hw, kitti_frames, kitti_resized):
    Image = pytest.importorskip('PIL.Image')
    want = np.asarray(Image.fromarray(kitti_frames[hw]).resize((KITTI_IN[1], KITTI_IN[0]), Image.BILINEAR))
    assert np.array_equal(kitti_resized[hw], want)


@pytest.mark.parametrize('hw', KITTI)
def test_mirror_before_equals_mirror_after_at_the_kitti_sizes(hw, kitti_frames, kitti_resized):
    """The sentence of the STATED DEVIATION of trackmpnn_amd.frames: at the data set's sizes the two orders give equal bytes."""
    assert np.array_equal(resize_host(kitti_frames[hw][:, ::-1], KITTI_IN), kitti_resized[hw][:, ::-1])


@pytest.mark.parametrize('hw,HW', [((64, 64), (64, 64)), ((9, 9), (9, 17)), ((9, 17), (5, 17)), ((31, 47), (31, 20)),
                                   ((31, 47), (50, 47))])
def test_copy_and_single_axis_routes_equal_pillow(hw, HW, monkeypatch):
    """Neither axis differs: a copy, no pass; one axis differs: one pass -- and the result is still Pillow's."""
    from trackmpnn_amd import frames
    Image = pytest.importorskip('PIL.Image')
    a = np.random.default_rng(sum(hw) + sum(HW)).integers(0, 256, hw + (3,), dtype=np.uint8)
    axes = []
    orig = frames._pass_host
    monkeypatch.setattr(frames, '_pass_host', lambda src, axis, *t: (axes.append(axis - src.ndim), orig(src, axis, *t))[1])
    got = resize_host(a, HW)
    assert axes == ([-2] if HW[1] != hw[1] else []) + ([-3] if HW[0] != hw[0] else [])
    assert got is not a and np.array_equal(got, np.asarray(Image.fromarray(a).resize((HW[1], HW[0]), Image.BILINEAR)))


@pytest.mark.parametrize('sizes', [(1242, 1280), (375, 384), (720, 384), (300, 7), (2, 5), (3, 11), (45, 7), (64, 64), (1, 1), (1, 9),
                                   (9, 1), (5000, 3)])
def test_resize_coeffs_rows_stay_inside_the_source_and_sum_to_one(sizes):
    in_size, out_size = sizes
    bounds, coef = resize_coeffs(in_size, out_size)
    ksize = coef.shape[1]
    assert bounds.dtype == coef.dtype == np.int32 and bounds.shape == (out_size, 2) and coef.shape[0] == out_size
    assert ksize == int(np.ceil(max(in_size / out_size, 1.0))) * 2 + 1
    xmin, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (n >= 1).all() and (n <= ksize).all() and (xmin >= 0).all() and (xmin + n <= in_size).all()
    assert (coef >= 0).all()                                       # bilinear has no negative weight
    assert (np.abs(coef.astype(np.int64).sum(axis=1) - (1 << 22)) <= ksize).all()
    assert all((coef[i, n[i]:] == 0).all() for i in range(out_size))


def test_prep_host_is_resize_then_the_table():
    from trackmpnn_amd.frames import norm_table
    _, _, table = norm_table(MEAN, STD)
    a = np.random.default_rng(3).integers(0, 256, (2, 23, 45, 3), dtype=np.uint8)
    got = prep_host(a, (33, 7), table)
    r = resize_host(a, (33, 7))
    assert got.dtype == np.float32 and got.shape == (2, 3, 33, 7)
    want = torch.from_numpy(r).permute(0, 3, 1, 2).float().div(255)
    want = (want - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)    # ToTensor, then Normalize
    assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    assert np.array_equal(prep_host(a[1], (33, 7), table), got[1:2])


def test_from_raw_host_store_equals_the_store_of_host_resized_frames():
    rng = np.random.default_rng(8)
    raw = [rng.integers(0, 256, (3, 37, 61, 3), dtype=np.uint8), rng.integers(0, 256, (2, 50, 70, 3), dtype=np.uint8)]
    hw = (20, 33)
    a = FrameStore.from_raw(raw, hw, MEAN, STD, device=None)
    b = FrameStore([resize_host(s, hw) for s in raw], MEAN, STD, device=None)
    assert (a.H, a.W) == hw and np.array_equal(a.planar, b.planar) and np.array_equal(a.seq_base, b.seq_base)
    assert np.array_equal(a.raw_hw, [[37, 61], [50, 70]]) and np.array_equal(b.raw_hw, [[20, 33], [20, 33]])
    plan = np.array([[1, 1, 1], [0, 2, 0], [0, 0, 1], [1, 0, 0]])
    fa, fb = a.frames_host(plan), b.frames_host(plan)
    assert fa.shape == (4, 3, 20, 33) and np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert np.array_equal(fa[2].view(np.uint32), prep_host(raw[0][0], hw, a.table)[0][:, :, ::-1].view(np.uint32))
    with pytest.raises(ValueError, match='uint8 expected'):
        FrameStore.from_raw([raw[0].astype(np.int32)], hw, MEAN, STD, device=None)
    with pytest.raises(ValueError, match='output size'):
        FrameStore.from_raw(raw, (20, 8193), MEAN, STD, device=None)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        FrameStore.from_raw(raw, hw, MEAN, STD, device='cpu')


def test_entry_point_argument_errors_need_no_gpu():
    from trackmpnn_amd import _lib
    lib = _lib.load()
    assert {'tmpnn_frames_resize', 'tmpnn_frames_resize_ws'} <= set(_lib._SIGNATURES) & set(_lib.header_symbols())
    R = _lib.CFramesResize
    one = 16                                                    # (any non-null address: nothing is launched, nothing is read)
    assert lib.tmpnn_frames_resize(None, None) == -1 and b'call struct is null' in lib.tmpnn_last_error()
    for bad, msg in ((R(-1, 4, 4, 8, 8, 3, 3, 0, one, one, one, one, one), b'n=-1'),
                     (R(1, 0, 4, 8, 8, 3, 3, 0, one, one, one, one, one), b'h=0'),
                     (R(1, 4, 4, 8, 8193, 3, 3, 0, one, one, one, one, one), b'W=8193'),
                     (R(1, 4, 4, 8, 8, 1025, 3, 0, one, one, one, one, one), b'kx=1025'),
                     (R(1, 4, 4, 8, 8, 3, 0, 0, one, one, one, one, one), b'ky=0'),
                     (R(1, 4, 4, 8, 8, 3, 3, 0, one, one, None, one, one), b'null coefficient table'),
                     (R(1, 4, 4, 8, 8, 3, 3, 0, None, one, one, one, one, None, one), b'null pointer'),
                     (R(1, 4, 4, 8, 8, 3, 3, 0, one, one, one, one, one, None, one, None, 0), b'workspace is null'),
                     (R(1, 4, 4, 8, 8, 3, 3, 0, one, one, one, one, one, None, one, 24, 1 << 20), b'16-byte aligned')):
        assert lib.tmpnn_frames_resize(ctypes.byref(bad), None) == -1 and msg in lib.tmpnn_last_error(), msg
    short = R(2, 4, 4, 8, 8, 3, 3, 0, one, one, one, one, one, None, one, 32, 16)
    assert lib.tmpnn_frames_resize(ctypes.byref(short), None) == -3 and b'workspace of 16 bytes' in lib.tmpnn_last_error()
    assert lib.tmpnn_frames_resize(ctypes.byref(R(0, 4, 4, 8, 8, 3, 3, 0, None, one, one, one, one)), None) == 0   # n = 0: no launch
    # the workspace: the horizontal pass's result [n][h][W][3], rounded up to 16; none without a horizontal pass
    assert lib.tmpnn_frames_resize_ws(2, 4, 4, 8, 8) == 2 * 4 * 8 * 3 and lib.tmpnn_frames_resize_ws(1, 3, 2, 11, 5) == 48
    assert lib.tmpnn_frames_resize_ws(5, 9, 17, 5, 17) == 0 and lib.tmpnn_frames_resize_ws(0, 4, 4, 8, 8) == 0
    assert lib.tmpnn_frames_resize_ws(1, 4, 4, 8, 8193) == 0


def test_frame_prep_validation_needs_no_gpu():
    prep = FramePrep((48, 80), MEAN, STD)
    assert prep.input_hw == (48, 80) and prep.table.shape == (3, 256)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        FramePrep((48, 80), MEAN, STD, device='cpu')
    with pytest.raises(ValueError, match='output size'):
        FramePrep((0, 80), MEAN, STD)
    with pytest.raises(ValueError, match='mean / std of length'):
        FramePrep((48, 80), (0.5, 0.5), STD)
    with pytest.raises(ValueError, match='uint8 expected'):
        prep.prep(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match=r'\[h, w, 3\] or frames'):
        prep.prep(np.zeros((2, 2, 4, 4, 3), np.uint8))


class _Head:
    """What OnlineVis and OnlineTracker read of a VisHead (a VisHead itself needs a device)."""

    def __init__(self, input_hw, mean, std):
        self.input_h, self.input_w = float(input_hw[0]), float(input_hw[1])
        self.mean, self.std = np.asarray(mean, np.float32), np.asarray(std, np.float32)

    def rows(self, *a, **k):
        raise AssertionError('no launch expected')


def test_online_vis_and_tracker_value_errors():
    ncat = 3
    F = ncat + 5 + 2 + 128
    rng = np.random.default_rng(1)
    mean, std = rng.normal(size=F).astype(np.float32), (rng.random(F) + 0.5).astype(np.float32)
    spec = FeatureSpec(ncat, '2d+temp+vis', mean, std)
    prep = FramePrep((48, 80), MEAN, STD)
    net = lambda x: x
    vis = OnlineVis(_Head((48, 80), mean[-128:], std[-128:]), prep, net)
    with pytest.raises(ValueError, match="head's input size"):
        OnlineVis(_Head((48, 96), mean[-128:], std[-128:]), prep, net)
    with pytest.raises(ValueError, match='a VisHead expected'):
        OnlineVis(object(), prep, net)
    with pytest.raises(ValueError, match='a FramePrep expected'):
        OnlineVis(_Head((48, 80), mean[-128:], std[-128:]), object(), net)
    with pytest.raises(ValueError, match='callable'):
        OnlineVis(_Head((48, 80), mean[-128:], std[-128:]), prep, None)

    model = TrackMPNN('2d+temp+vis', ncat, 32, 0, 'diff').eval()
    plain = TrackMPNN('2d+temp', ncat, 32, 0, 'diff').eval()
    with pytest.raises(ValueError, match="'vis' columns"):                   # a spec without 'vis'
        OnlineTracker(plain, spec=FeatureSpec(ncat, '2d+temp', mean[:10], std[:10]), vis=vis)
    with pytest.raises(ValueError, match="'vis' columns"):                   # no spec at all
        OnlineTracker(model, vis=vis)
    with pytest.raises(ValueError, match='must be an OnlineVis'):
        OnlineTracker(model, spec=spec, vis=prep)
    other = std[-128:].copy()
    other[5] += 1.0
    with pytest.raises(ValueError, match='mean / std values differ'):
        OnlineTracker(model, spec=spec, vis=OnlineVis(_Head((48, 80), mean[-128:], other), prep, net))

    det = ([1], [0.5], [[1.0, 2.0, 9.0, 8.0]])
    frame = np.zeros((37, 61, 3), np.uint8)
    trk = OnlineTracker(model, spec=spec, vis=vis)
    with pytest.raises(ValueError, match='frame= and vis= together'):
        trk.push(*det, vis=np.zeros((1, 128), np.float32), frame=frame)
    with pytest.raises(ValueError, match=r'frame \[h, w, 3\] uint8'):
        trk.push(*det, frame=frame.astype(np.float32))
    with pytest.raises(ValueError, match=r'frame \[h, w, 3\] uint8'):
        trk.push(*det, frame=frame[None])
    with pytest.raises(ValueError, match='pass vis'):                        # neither: the old rule of a 'vis' spec
        trk.push(*det)
    with pytest.raises(ValueError, match='needs a tracker built with vis=OnlineVis'):
        OnlineTracker(model, spec=spec).push(*det, frame=frame)
    assert (trk.frames, trk.ndets) == (0, 0)
    # a frame without detections runs no CNN and no launch, on any machine
    trk.vis.embed_net = lambda x: (_ for _ in ()).throw(AssertionError('no CNN expected'))
    trk.push([], [], np.zeros((0, 4)), frame=frame)
    assert (trk.frames, trk.ndets) == (1, 0)


def test_package_exports_the_resize_api():
    import trackmpnn_amd
    for name in ('FramePrep', 'OnlineVis', 'resize_coeffs', 'resize_host', 'prep_host'):
        assert name in trackmpnn_amd.__all__ and hasattr(trackmpnn_amd, name)
    assert hasattr(FrameStore, 'from_raw')
