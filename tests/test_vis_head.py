"""The visual head: the host definition (trackmpnn_amd.vishead.vis_centres_host, vis_head_host) against the recorded results of
the reference's get_vis_feats, F.softmax and FairMOTLoss (tests/golden/vis, tools/gen_vis_golden.py), and on the cases the
library states for itself.  No GPU here; the device is held to the host definition in tests/test_vis_head_gpu.py.

Tolerances.  The indices are integers: exact.  The float32 softmax and loss against the reference's float32 ones: rtol 1e-5,
which is the rounding of a 128-term float32 sum in any order (127 * 2^-24 = 7.6e-6) plus that of the exponent's argument.  The
standardised rows (softmax - mean) / std cancel against the mean, so the same error of the softmax is an absolute one there:
|err| <= 1e-5 * (1 + |value|) / std."""
import os

import numpy as np
import pytest

from trackmpnn_amd import _lib
from trackmpnn_amd.vishead import MAX_DETS, VIS_COLS, VisHead, vis_centres_host, vis_head_host, vis_pixels_host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis')
FIXTURES = ('vis_kitti_375_d4', 'vis_kitti_375_d1', 'vis_kitti_370_d4', 'vis_kitti_370_d1', 'vis_bdd_d4')
SHAPES = {'vis_kitti_375_d4': ((375, 1242), (384, 1280), 4), 'vis_kitti_375_d1': ((375, 1242), (384, 1280), 1),
          'vis_kitti_370_d4': ((370, 1224), (384, 1280), 4), 'vis_kitti_370_d1': ((370, 1224), (384, 1280), 1),
          'vis_bdd_d4': ((720, 1280), (720, 1280), 4)}
HALF = np.full(VIS_COLS, 0.5, np.float32)                          # the reference's mean and std of the 'vis' columns
ZERO, ONE = np.zeros(VIS_COLS, np.float32), np.ones(VIS_COLS, np.float32)


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    return {k: z[k] for k in z.files}


def head_args(z, dtype=np.float32):
    """(positional arguments up to offsets, (input_hw, down_ratio)) of vis_head_host for a fixture's head part"""
    return ((z['head_maps'].astype(dtype), z['head_box'], z['head_map_of'], tuple(z['im_hw']), z['head_track'], z['head_offsets']),
            (tuple(z['head_input_hw']), int(z['head_down_ratio'])))


def small_case(D, seed=0, T=2, Hm=6, Wm=10, B=3, p_fp=0.3):
    """A seeded head problem on T maps of 128 x Hm x Wm: image (8 Hm, 8 Wm), input (2 Hm, 2 Wm), down_ratio 2, so a map pixel is
    8 x 8 image pixels and in-image boxes stay on the map; B chunks with random boundaries, ids up to 399, a share p_fp of -1."""
    rng = np.random.default_rng([seed, D, 9])
    im_hw = (8 * Hm, 8 * Wm)
    maps = (2.0 * rng.standard_normal((T, VIS_COLS, Hm, Wm))).astype(np.float32)
    x = np.sort(rng.uniform(0, im_hw[1] - 1, (D, 2)), axis=1)
    y = np.sort(rng.uniform(0, im_hw[0] - 1, (D, 2)), axis=1)
    box = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)
    map_of = np.sort(rng.integers(0, T, D)).astype(np.int64)
    track = rng.integers(0, 400, D)
    track[rng.random(D) < p_fp] = -1
    offsets = np.concatenate([[0], np.sort(rng.integers(0, D + 1, B - 1)), [D]]).astype(np.int64)
    return {'maps': maps, 'box': box, 'map_of': map_of, 'im_hw': im_hw, 'track': track.astype(np.int64), 'offsets': offsets,
            'input_hw': (2 * Hm, 2 * Wm), 'down_ratio': 2}


def host(c, dtype=np.float64, mean=HALF, std=HALF, g=None):
    return vis_head_host(c['maps'].astype(dtype), c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'], mean, std,
                         c['input_hw'], c['down_ratio'], g=g)


# ---- the centre index ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_centres_equal_the_reference(name):
    z = load_fixture(name)
    im_hw, input_hw, down = SHAPES[name]
    assert (tuple(z['im_hw']), tuple(z['input_hw']), int(z['down_ratio'])) == (im_hw, input_hw, down)
    assert z['box'].dtype == np.float32 and z['box'].shape[0] >= 1500
    cy, cx = vis_centres_host(z['box'], im_hw, input_hw, down)
    assert cy.dtype == np.int64 and np.array_equal(cy, z['ref_cy']) and np.array_equal(cx, z['ref_cx'])
    # the same sizes given per row
    cy2, cx2 = vis_centres_host(z['box'], np.tile(np.asarray(im_hw, np.float32), (z['box'].shape[0], 1)), input_hw, down)
    assert np.array_equal(cy2, cy) and np.array_equal(cx2, cx)
    # in-image boxes stay on the map: nothing is clamped
    assert not vis_pixels_host(cy, cx, np.zeros_like(cy), input_hw[0] // down, input_hw[1] // down)[2].any()


def test_a_fixture_holds_a_box_whose_float64_centre_differs():
    found = 0
    for name in FIXTURES:
        z = load_fixture(name)
        k = np.where(z['fp64_differs'])[0]
        if not k.size:
            continue
        (ih, iw), (h, w), down = z['input_hw'], z['im_hw'], int(z['down_ratio'])
        b = z['box'][k].astype(np.float64)
        cx64 = np.trunc(((b[:, 0] + b[:, 2]) / 2.0) * iw / w / down).astype(np.int64)
        cy64 = np.trunc(((b[:, 1] + b[:, 3]) / 2.0) * ih / h / down).astype(np.int64)
        differs = (cx64 != z['ref_cx'][k]) | (cy64 != z['ref_cy'][k])
        assert differs.all()                                       # float64 disagrees with the reference on every one of them
        found += int(differs.sum())
    assert found >= 1


def test_centres_truncate_toward_zero_and_clamp():
    # centres at x = -6, 3, 79.9 -> -1.5, 0.75, 19.97 map pixels -> -1, 0, 19 (truncation, not floor: -0.4 -> 0)
    box = np.asarray([[-8, 0, -4, 2], [2, 0, 4, 2], [79.8, 0, 80.0, 2], [-2, 0, -1.2, 2], [100, 90, 120, 100]], np.float32)
    cy, cx = vis_centres_host(box, (48, 80), (12, 20), 1)
    assert cx.tolist() == [-1, 0, 19, 0, 27] and cy.tolist() == [0, 0, 0, 0, 23]
    y, x, clamped, pix = vis_pixels_host(cy, cx, [0, 0, 0, 1, 1], 12, 20)
    assert x.tolist() == [0, 0, 19, 0, 19] and y.tolist() == [0, 0, 0, 0, 11] and clamped.tolist() == [True, False, False, False, True]
    assert pix.tolist() == [0, 0, 19, 240, 240 + 11 * 20 + 19]


def test_centres_reject_bad_input():
    with pytest.raises(ValueError, match='not finite'):
        vis_centres_host(np.asarray([[0, 0, np.nan, 1]], np.float32), (10, 10), (10, 10), 1)
    with pytest.raises(ValueError, match='im_hw'):
        vis_centres_host(np.zeros((3, 4), np.float32), np.ones((2, 2)), (10, 10), 1)
    with pytest.raises(ValueError, match='positive'):
        vis_centres_host(np.zeros((1, 4), np.float32), (10, 10), (10, 10), 0)


# ---- softmax rows and identity loss -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_head_equals_the_reference(name):
    z = load_fixture(name)
    args, geo = head_args(z)
    logits, soft, loss, _ = vis_head_host(*args, ZERO, ONE, *geo)
    assert logits.dtype == np.float32 and np.array_equal(logits, z['ref_logits'])      # a gather
    np.testing.assert_allclose(soft, z['ref_softmax'], rtol=1e-5, atol=0)
    np.testing.assert_allclose(loss, z['ref_loss'], rtol=1e-5, atol=0)
    _, rows, loss2, _ = vis_head_host(*args, HALF, HALF, *geo)
    assert np.array_equal(loss2, loss)
    err = np.abs(rows - z['ref_rows'])
    assert (err <= 1e-5 * (1 + np.abs(z['ref_rows'])) / 0.5).all(), err.max()
    assert (z['head_track'] >= VIS_COLS).any() and (z['head_track'] < 0).any()         # ids >= 128 and false positives occur


def test_float64_and_float32_hosts_agree():
    c = small_case(65)
    a, b = host(c, np.float64), host(c, np.float32)
    assert a[0].dtype == np.float64 and b[3].dtype == np.float32
    np.testing.assert_allclose(b[1], a[1], rtol=0, atol=4e-5)
    np.testing.assert_allclose(b[2], a[2], rtol=1e-5)
    np.testing.assert_allclose(b[3], a[3], rtol=0, atol=1e-6)


def test_gradient_is_the_derivative_of_the_loss():
    """dmaps against central differences of sum(g * loss) in float64."""
    c = small_case(12, seed=3, Hm=3, Wm=4)
    g = np.asarray([0.7, -1.3, 2.0])
    _, _, _, dmaps = host(c, g=g)
    rng = np.random.default_rng(1)
    nz = np.argwhere(dmaps != 0)
    picks = [tuple(nz[i]) for i in rng.integers(0, nz.shape[0], 12)] + [(0, 0, 0, 0)]
    for idx in picks:
        vals = []
        for eps in (1e-6, -1e-6):
            m = c['maps'].astype(np.float64)
            m[idx] += eps
            vals.append(float((g * vis_head_host(m, c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'], HALF, HALF, c['input_hw'],
                                                 c['down_ratio'])[2]).sum()))
        assert abs((vals[0] - vals[1]) / 2e-6 - dmaps[idx]) < 1e-7


# ---- the pinned cases --------------------------------------------------------------------------------------------------------
def test_chunk_without_a_labelled_row_and_empty_chunk():
    c = small_case(20, seed=5)
    c['offsets'] = np.asarray([0, 6, 6, 13, 20], np.int64)          # chunk 1 is empty
    c['track'][6:13] = -1                                           # chunk 2 has rows, none labelled
    c['track'][[0, 14]] = [3, 4]
    logits, rows, loss, dmaps = host(c)
    assert loss.shape == (4,) and loss[1] == 0 and loss[2] == 0 and loss[0] > 0 and loss[3] > 0
    assert np.isfinite(rows).all() and rows.shape == (20, VIS_COLS)                     # rows of unlabelled detections are still features
    cy, cx, _, _ = vis_pixels_host(*vis_centres_host(c['box'], c['im_hw'], c['input_hw'], c['down_ratio']), c['map_of'], 6, 10)
    touched = np.zeros(dmaps.shape, bool)
    for i in np.where(c['track'] >= 0)[0]:
        touched[c['map_of'][i], :, cy[i], cx[i]] = True
    assert (dmaps[~touched] == 0).all() and (dmaps[touched] != 0).any()
    only = dict(c, offsets=np.asarray([6, 13], np.int64))           # that chunk alone: loss 0, gradient exactly 0
    _, _, l1, d1 = host(only)
    assert l1.tolist() == [0.0] and not d1.any()


def test_track_ids_wrap_at_128():
    c = small_case(9, seed=7, p_fp=0.0)
    a = host(c)
    b = host(dict(c, track=c['track'] % VIS_COLS + VIS_COLS * np.arange(9)))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_clamped_centres_read_the_border():
    c = small_case(4, seed=8, T=1)
    c['box'] = np.asarray([[-30, -30, -10, -10], [200, 100, 220, 130], [-19, 20, -5, 24], [30, 10, 34, 14]], np.float32)
    c['map_of'], c['track'], c['offsets'] = np.zeros(4, np.int64), np.asarray([1, 2, 3, 4]), np.asarray([0, 4])
    logits = host(c)[0]
    m = c['maps'].astype(np.float64)[0]
    assert np.array_equal(logits[0], m[:, 0, 0]) and np.array_equal(logits[1], m[:, 5, 9]) and np.array_equal(logits[2], m[:, 2, 0])
    assert np.array_equal(logits[3], m[:, 1, 4])
    cy, cx = vis_centres_host(c['box'], c['im_hw'], c['input_hw'], c['down_ratio'])
    assert vis_pixels_host(cy, cx, c['map_of'], 6, 10)[2].tolist() == [True, True, True, False]


def test_sharers_of_a_pixel_add_in_row_order():
    c = small_case(5, seed=9, T=1, p_fp=0.0)
    c['box'] = np.tile(np.asarray([[30, 10, 34, 14]], np.float32), (5, 1))
    c['map_of'], c['offsets'] = np.zeros(5, np.int64), np.asarray([0, 2, 5])
    g = np.asarray([1.5, -0.5])
    logits, _, _, dmaps = host(c, np.float32, g=g)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    acc = np.zeros(VIS_COLS, np.float32)
    for i in range(5):
        d = p[i].copy()
        d[c['track'][i] % VIS_COLS] -= np.float32(1)
        acc = acc + (g.astype(np.float32)[0 if i < 2 else 1] / np.float32(2 if i < 2 else 3)) * d
    assert np.array_equal(dmaps[0, :, 1, 4], acc) and np.count_nonzero(dmaps) <= VIS_COLS


def test_host_rejects_bad_input():
    c = small_case(6)
    with pytest.raises(ValueError, match='map_of outside'):
        host(dict(c, map_of=np.full(6, 2)))
    with pytest.raises(ValueError, match='offsets'):
        host(dict(c, offsets=np.asarray([0, 4, 3, 6])))
    with pytest.raises(ValueError, match='offsets'):
        host(dict(c, offsets=np.asarray([0, 7])))
    with pytest.raises(ValueError, match='maps'):
        vis_head_host(np.zeros((1, 64, 2, 2)), c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'], HALF, HALF, (4, 4), 1)


# ---- the boundary ------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_fail_loudly():
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        VisHead((12, 20), 2, HALF, HALF, device='cpu')


def test_entry_points_validate_on_the_host():
    import ctypes as C
    lib = _lib.load()
    assert lib.tmpnn_vis_head_fwd(None, None) == -1 and b'vis_head_fwd' in lib.tmpnn_last_error()
    a = _lib.CVisHead()
    a.T, a.Hm, a.Wm, a.B, a.D = 1, 65536, 65536, 1, 0
    assert lib.tmpnn_vis_head_fwd(C.byref(a), None) == -1 and b'int32' in lib.tmpnn_last_error()
    a.Hm, a.Wm, a.D = 6, 10, MAX_DETS + 1
    assert lib.tmpnn_vis_head_fwd(C.byref(a), None) == -1 and b'D=131073' in lib.tmpnn_last_error()
    a.D, a.input_h, a.input_w, a.down_ratio, a.im_h, a.im_w = 0, 12.0, 20.0, 0.0, 48.0, 80.0
    assert lib.tmpnn_vis_head_fwd(C.byref(a), None) == -1 and b'down_ratio' in lib.tmpnn_last_error()
    a.down_ratio, a.ld_rows, a.col = 2.0, 130, 3
    assert lib.tmpnn_vis_head_fwd(C.byref(a), None) == -1 and b'col=3' in lib.tmpnn_last_error()
    a.col = 2
    assert lib.tmpnn_vis_head_fwd(C.byref(a), None) == -1 and b'null maps' in lib.tmpnn_last_error()
    assert lib.tmpnn_vis_head_bwd(C.byref(a), None, None, None) == -1
