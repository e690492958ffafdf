"""The visual head on the device (-m gpu; csrc/vishead.hip: tmpnn_vis_head_fwd, tmpnn_vis_head_bwd; trackmpnn_amd.vishead.VisHead)
against the host definition vis_head_host in float64.

Bounds.  Centres, pixels, counts: integers, exact.  Logits: a gather, bit for bit.  Rows: |err| <= 1e-5 (1 + |value|) / std -- the
softmax is a 128-term float32 sum (127 * 2^-24 = 7.6e-6 in any order, plus the rounding of the exponent's argument), and the
standardisation divides its error by std.  Loss: rtol 1e-5.  dmaps: 1e-5 (1 + |value|) times the number of rows that share the
pixel (each adds one softmax with that error).  Weight gradients of a convolution in front of the head: 1e-5 (1 + |value|) on
the gradient itself, plus the rounding of the convolution's own float32 backward sum.

Measured maxima are printed by every test that compares (profiles/vis_head.md records them)."""
import functools

import numpy as np
import pytest
import torch

from tests.test_vis_head import FIXTURES, load_fixture, small_case
from trackmpnn_amd.vishead import VIS_COLS, VisHead, vis_centres_host, vis_head_host, vis_pixels_host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_rng = np.random.default_rng(123)
MEAN = (0.02 * _rng.random(VIS_COLS)).astype(np.float32)
STD = (0.3 + 1.7 * _rng.random(VIS_COLS)).astype(np.float32)


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def reference(c, g=None):
    """The float64 host results of a case and what the device is compared with besides: clamped centres, pixels, counts, and
    per pixel of dmaps the number of labelled rows on it."""
    T, _, Hm, Wm = c['maps'].shape
    logits, rows, loss, dmaps = vis_head_host(c['maps'].astype(np.float64), c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'],
                                              MEAN, STD, c['input_hw'], c['down_ratio'], g=g)
    cy, cx, clamped, pix = vis_pixels_host(*vis_centres_host(c['box'], c['im_hw'], c['input_hw'], c['down_ratio']), c['map_of'], Hm, Wm)
    off, lab = c['offsets'], c['track'] >= 0
    B = off.shape[0] - 1
    sharers = np.zeros((T, Hm, Wm), np.int64)
    in_chunk = np.zeros(lab.shape[0], bool)
    for b in range(B):
        in_chunk[off[b]:off[b + 1]] = True
    np.add.at(sharers, (c['map_of'][lab & in_chunk], cy[lab & in_chunk], cx[lab & in_chunk]), 1)
    return {'logits': logits, 'rows': rows, 'loss': loss, 'dmaps': dmaps, 'cy': cy, 'cx': cx, 'clamped': clamped, 'pix': pix,
            'labelled': np.asarray([lab[off[b]:off[b + 1]].sum() for b in range(B)]),
            'n_clamped': np.asarray([clamped[off[b]:off[b + 1]].sum() for b in range(B)]), 'rows_of': np.diff(off), 'sharers': sharers}


@functools.lru_cache(maxsize=None)
def case(D):
    """small_case(D) with every seventh box pushed off the image (clamped centres), and its reference (computed once)."""
    c = small_case(D, seed=2)
    c['box'][::7] += np.float32(100)
    c['g'] = np.asarray([0.75, -1.25, 2.0])
    return c, reference(c, c['g'])


def run_device(c, g=None, head=None):
    """(rows, loss, dmaps, logits as numpy; the record) of one forward + backward on the device."""
    head = head or VisHead(c['input_hw'], c['down_ratio'], MEAN, STD, DEV)
    maps = torch.from_numpy(c['maps']).to(DEV).requires_grad_()
    rows, loss = head.forward(maps, c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'])
    assert not rows.requires_grad and loss.requires_grad
    logits, rec = head.last_logits().cpu().numpy(), head.record()
    w = torch.ones_like(loss) if g is None else torch.from_numpy(np.asarray(g, np.float32)).to(DEV)
    (loss * w).sum().backward()
    return rows.cpu().numpy(), loss.detach().cpu().numpy(), maps.grad.cpu().numpy(), logits, rec


def check(c, ref, out, what):
    rows, loss, dmaps, logits, rec = out
    assert np.array_equal(rec['cy'], ref['cy']) and np.array_equal(rec['cx'], ref['cx']) and np.array_equal(rec['pix'], ref['pix'])
    assert np.array_equal(rec['row_clamped'], ref['clamped'])
    assert np.array_equal(rec['labelled'], ref['labelled']) and np.array_equal(rec['clamped'], ref['n_clamped'])
    assert np.array_equal(rec['rows'], ref['rows_of'])
    assert logits.dtype == np.float32 and np.array_equal(logits.astype(np.float64), ref['logits'])              # bit for bit
    e_rows = np.abs(rows - ref['rows']) / ((1 + np.abs(ref['rows'])) / STD[None, :])
    e_loss = np.abs(loss - ref['loss']) / np.maximum(np.abs(ref['loss']), 1e-300)
    e_loss[ref['loss'] == 0] = np.abs(loss[ref['loss'] == 0])                                                   # (exactly 0 expected)
    e_d = np.abs(dmaps - ref['dmaps']) / ((1 + np.abs(ref['dmaps'])) * np.maximum(ref['sharers'], 1)[:, None])
    print(f'{what}: max rows err / bound unit {e_rows.max(initial=0):.3g}, loss rel {e_loss.max(initial=0):.3g}, '
          f'dmaps err / bound unit {e_d.max(initial=0):.3g} (each must be <= 1e-5)')
    assert e_rows.max(initial=0) <= 1e-5 and e_loss.max(initial=0) <= 1e-5 and e_d.max(initial=0) <= 1e-5
    assert (dmaps[np.broadcast_to((ref['sharers'] == 0)[:, None], dmaps.shape)] == 0).all()                     # untouched pixels: exactly 0


@pytest.mark.parametrize('D', [0, 1, 63, 64, 65, 130])
def test_device_equals_the_host(D):
    c, ref = case(D)
    if D >= 63:
        assert ref['clamped'].sum() >= D // 7 and (ref['sharers'] > 1).any() and (ref['labelled'] > 0).any()
    check(c, ref, run_device(c, c['g']), f'D={D}')


@pytest.mark.parametrize('name', FIXTURES)
def test_centres_equal_the_reference_at_the_real_sizes(name):
    """The recorded boxes of the reference (those whose float64 centre differs among them) on a map of the real size: the
    device's centres equal the reference's indices, and nothing is clamped."""
    z = load_fixture(name)
    (h, w), (ih, iw), down = (int(v) for v in z['im_hw']), (int(v) for v in z['input_hw']), int(z['down_ratio'])
    n = z['box'].shape[0]
    head = VisHead((ih, iw), down, MEAN, STD, DEV)
    head.rows(torch.zeros((1, VIS_COLS, ih // down, iw // down), device=DEV), z['box'], np.zeros(n, np.int64), (h, w))
    rec = head.record()
    assert np.array_equal(rec['cy'], z['ref_cy']) and np.array_equal(rec['cx'], z['ref_cx'])
    assert rec['clamped'].tolist() == [0] and rec['rows'].tolist() == [n]


def special_case():
    """12 rows on T = 2 maps.  Rows 0-4: one box on map 0 (five sharers); row 5 elsewhere; chunk 0 = rows 0-5.  Rows 6, 7: one box,
    maps 0 and 1 (the same (cy, cx), different pixels); row 8 elsewhere; chunk 1 = rows 6-8.  Chunk 2 = rows 9-11, none
    labelled, each on a pixel of its own."""
    c = small_case(12, seed=4, p_fp=0.0)
    px = lambda x, y: [8 * x + 1, 8 * y + 1, 8 * x + 5, 8 * y + 5]                                             # a box centred in map pixel (y, x)
    c['box'] = np.asarray([px(3, 2)] * 5 + [px(0, 0)] + [px(7, 4)] * 2 + [px(9, 5)] + [px(1, 1), px(2, 1), px(3, 1)], np.float32)
    c['map_of'] = np.asarray([0] * 6 + [0, 1, 1] + [0, 1, 0], np.int64)
    c['track'] = np.asarray([7, 135, 7, 300, 2, 9, 11, 11, 12, -1, -1, -1], np.int64)
    c['offsets'] = np.asarray([0, 6, 9, 12], np.int64)
    return c


def test_sharers_maps_and_the_unlabelled_chunk():
    c = special_case()
    ref = reference(c)
    assert ref['sharers'][0, 2, 3] == 5 and ref['sharers'][0, 4, 7] == 1 and ref['sharers'][1, 4, 7] == 1
    assert ref['labelled'].tolist() == [6, 3, 0] and ref['loss'][2] == 0
    out = run_device(c)
    check(c, ref, out, 'special')
    rows, loss, dmaps, _, _ = out
    assert loss[2] == 0.0                                                                                       # exactly
    for y, x, m in ((1, 1, 0), (1, 2, 1), (1, 3, 0)):
        assert not dmaps[m, :, y, x].any()                                                                      # exactly 0
    assert dmaps[0, :, 4, 7].any() and dmaps[1, :, 4, 7].any() and not np.array_equal(dmaps[0, :, 4, 7], dmaps[1, :, 4, 7])
    assert np.isfinite(rows[9:]).all()
    again = run_device(c)
    assert np.array_equal(again[2].view(np.int32), dmaps.view(np.int32))                                        # two backwards: the same bits
    assert np.array_equal(again[1].view(np.int32), loss.view(np.int32))
    c65, _ = case(65)
    a, b = run_device(c65, c65['g']), run_device(c65, c65['g'])
    assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32))


def test_rows_into_a_strided_feature_tensor():
    c, ref = case(65)
    F = 10 + VIS_COLS
    head = VisHead(c['input_hw'], c['down_ratio'], MEAN, STD, DEV)
    maps = torch.from_numpy(c['maps']).to(DEV)
    plain = head.rows(maps, c['box'], c['map_of'], c['im_hw'])
    assert plain.shape == (65, VIS_COLS) and not plain.requires_grad
    big = torch.full((65, F + 7), -7.5, device=DEV)
    X = big[:, :F]                                                                                              # row stride F + 7
    assert not X.is_contiguous()
    with torch.no_grad():
        got = head.rows(maps, torch.from_numpy(c['box']).to(DEV), torch.from_numpy(c['map_of']).to(DEV),
                        np.tile(np.asarray(c['im_hw'], np.float32), (65, 1)), out=X, col=F - VIS_COLS)
    assert got is X
    assert torch.equal(X[:, F - VIS_COLS:].contiguous().view(torch.int32), plain.view(torch.int32))
    assert (big[:, :F - VIS_COLS] == -7.5).all() and (big[:, F:] == -7.5).all()
    rec = head.record()
    assert rec['labelled'].tolist() == [0] and rec['clamped'].tolist() == [int(ref['clamped'].sum())] and rec['rows'].tolist() == [65]
    e = np.abs(plain.cpu().numpy() - ref['rows']) / ((1 + np.abs(ref['rows'])) / STD[None, :])
    assert e.max() <= 1e-5
    with pytest.raises(ValueError, match='out'):
        head.rows(maps, c['box'], c['map_of'], c['im_hw'], out=X, col=F - VIS_COLS + 1)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        head.rows(maps.cpu(), c['box'], c['map_of'], c['im_hw'])


def test_bad_map_and_bad_offsets_are_reported_not_read():
    c, _ = case(65)
    head = VisHead(c['input_hw'], c['down_ratio'], MEAN, STD, DEV)
    maps = torch.from_numpy(c['maps']).to(DEV)
    mo = c['map_of'].copy()
    mo[3] = 2
    head.rows(maps, c['box'], mo, c['im_hw'])
    with pytest.raises(RuntimeError, match='map_of outside'):
        head.record()
    bad = torch.tensor([0, 40, 30, 99], dtype=torch.int32, device=DEV)                                          # device offsets: the kernel clamps
    head.forward(maps, c['box'], c['map_of'], c['im_hw'], c['track'], bad)
    with pytest.raises(RuntimeError, match='offsets'):
        head.record()
    with pytest.raises(ValueError, match='offsets'):
        head.forward(maps, c['box'], c['map_of'], c['im_hw'], c['track'], [0, 40, 30, 65])
    wide = c['track'].copy()
    wide[5] = 2 ** 31                                                                                           # would wrap to a negative id
    with pytest.raises(ValueError, match='track outside int32'):
        head.forward(maps, c['box'], c['map_of'], c['im_hw'], wide, c['offsets'])
    with pytest.raises(ValueError, match='at most 131072'):
        head.rows(maps, np.zeros((2 ** 17 + 1, 4), np.float32), np.zeros(2 ** 17 + 1, np.int64), c['im_hw'])


def test_backward_is_differentiable_once():
    """A second differentiation through the backward raises; it does not take dmaps for a constant."""
    c, _ = case(65)
    head = VisHead(c['input_hw'], c['down_ratio'], MEAN, STD, DEV)
    maps = torch.from_numpy(c['maps']).to(DEV).requires_grad_()
    _, loss = head.forward(maps, c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'])
    w = torch.ones_like(loss).requires_grad_()                                                                  # dmaps depends on the weights of the losses
    (d,) = torch.autograd.grad((loss * w).sum(), maps, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        d.sum().backward()


def test_autograd_through_a_convolution():
    """A one-layer convolution as the CNN: loss.sum().backward() through VisHead against the same graph from torch indexing and
    F.cross_entropy in float64.  (The float32 convolution in front of the head rounds its 27-term sums: about 1e-6 on a logit,
    twice that relative to a softmax value -- a fifth of the bound's unit at most.)"""
    T, Hm, Wm = 2, 12, 20
    c = small_case(24, seed=6, T=T, Hm=Hm, Wm=Wm)
    c['input_hw'], c['down_ratio'] = (Hm, Wm), 1                                                                # image 96 x 160 -> input 12 x 20
    c['offsets'] = np.asarray([0, 9, 24], np.int64)
    c['track'][[0, 10]] = [5, 200]
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(3, VIS_COLS, 3, padding=1)
    img = torch.randn(T, 3, Hm, Wm)
    # float64 on the host
    c64 = torch.nn.Conv2d(3, VIS_COLS, 3, padding=1).double()
    c64.load_state_dict({k: v.double() for k, v in conv.state_dict().items()})
    m64 = c64(img.double())
    m64.retain_grad()
    cy, cx, _, _ = vis_pixels_host(*vis_centres_host(c['box'], c['im_hw'], c['input_hw'], 1), c['map_of'], Hm, Wm)
    lg = m64[torch.from_numpy(c['map_of']), :, torch.from_numpy(cy), torch.from_numpy(cx)]
    lab = torch.from_numpy(np.where(c['track'] >= 0, c['track'] % VIS_COLS, -100))
    off = c['offsets']
    ref_loss = torch.stack([torch.nn.functional.cross_entropy(lg[off[b]:off[b + 1]], lab[off[b]:off[b + 1]], ignore_index=-100)
                            for b in range(2)])
    ref_loss.sum().backward()
    # the device
    conv = conv.to(DEV)
    head = VisHead(c['input_hw'], 1, MEAN, STD, DEV)
    rows, loss = head.forward(conv(img.to(DEV)), c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'])
    loss.sum().backward()
    np.testing.assert_allclose(loss.detach().cpu().numpy(), ref_loss.detach().numpy(), rtol=1e-5)
    # the bound: the one of the rows and of dmaps applied to the gradient itself, 1e-5 (1 + |value|), plus the float32 rounding
    # of the convolution's own backward, a sum over at most D touched pixels: D 2^-24 of the sum of the terms' magnitudes
    dm = m64.grad
    E = c['box'].shape[0] * 2.0 ** -24 * dm.abs()
    bound_w = 1e-5 * (1 + c64.weight.grad.abs()) + torch.nn.grad.conv2d_weight(img.double().abs(), tuple(c64.weight.shape), E, padding=1)
    bound_b = 1e-5 * (1 + c64.bias.grad.abs()) + E.sum((0, 2, 3))
    ew = (conv.weight.grad.cpu().double() - c64.weight.grad).abs()
    eb = (conv.bias.grad.cpu().double() - c64.bias.grad).abs()
    print(f'autograd: max weight-gradient err / bound {(ew / bound_w).max():.3g}, bias {(eb / bound_b).max():.3g} (<= 1); '
          f'max |dW| {c64.weight.grad.abs().max():.3g}, max err {ew.max():.3g}')
    assert c64.weight.grad.abs().max() > 1e-2
    assert (ew <= bound_w).all() and (eb <= bound_b).all()


def test_rows_drive_the_online_tracker():
    """VisHead.rows joined with the 2d + temp columns and pushed as features == push(..., vis = the host's softmax rows)."""
    from trackmpnn_amd import FeatureSpec, OnlineTracker, TrackMPNN, online_features_host
    from trackmpnn_amd.graph import synth_window
    ncat, Hm, Wm, frames = 3, 6, 10, 12
    im_hw, input_hw, down = (8 * Hm, 8 * Wm), (2 * Hm, 2 * Wm), 2
    F = ncat + 5 + 2 + VIS_COLS
    mean = np.concatenate([np.full(ncat, 0.5), [0.5, 40, 24, 20, 12], [0.5, 0.5], np.full(VIS_COLS, 0.5)]).astype(np.float32)
    std = np.concatenate([np.full(ncat, 0.5), [0.2, 25, 14, 12, 8], [0.5, 0.5], np.full(VIS_COLS, 0.5)]).astype(np.float32)
    sp = FeatureSpec(ncat, '2d+temp+vis', mean, std)
    sp_flat = FeatureSpec(ncat, '2d+temp', mean[:F - VIS_COLS], std[:F - VIS_COLS])
    yy = synth_window(81, frames, 5.0, 12)
    torch.manual_seed(22)
    model = TrackMPNN('2d+temp+vis', 3, 32, 0, 'diff').to(DEV).eval()
    with torch.no_grad():
        for k, prm in model.named_parameters():
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(2)).to(DEV))
    rng = np.random.default_rng(8)
    maps = (2.0 * rng.standard_normal((frames, VIS_COLS, Hm, Wm))).astype(np.float32)
    maps_d = torch.from_numpy(maps).to(DEV)
    head = VisHead(input_hw, down, mean, std, DEV)                                                              # (takes the last 128 entries)
    a = OnlineTracker(model, 3, 1, False, True, spec=sp, device=DEV, max_dets=16)
    b = OnlineTracker(model, 3, 1, False, True, device=DEV, max_dets=16)
    zero, one = np.zeros(VIS_COLS, np.float32), np.ones(VIS_COLS, np.float32)
    last = int(yy[-1, 0])                                                                                       # the last frame with detections
    for t in range(last + 1):
        D = int((yy[:, 0] == t).sum())
        x = np.sort(rng.uniform(0, im_hw[1] - 1, (D, 2)), axis=1)
        y = np.sort(rng.uniform(0, im_hw[0] - 1, (D, 2)), axis=1)
        box = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)
        cat, score = rng.integers(1, ncat + 1, D), rng.random(D).astype(np.float32)
        soft = vis_head_host(maps, box, np.full(D, t), im_hw, np.full(D, -1), [0, D], zero, one, input_hw, down)[1]
        a.push(cat, score, box, vis=soft, last=t == last)
        X = torch.empty((D, F), dtype=torch.float32, device=DEV)
        X[:, :F - VIS_COLS] = torch.from_numpy(online_features_host(sp_flat, cat, score, box, t)).to(DEV)
        head.rows(maps_d, box, np.full(D, t), im_hw, out=X, col=F - VIS_COLS)
        b.push_features(X, last=t == last)
    assert a.ndets == b.ndets == yy.shape[0]
    xa, xb = a._X[:a.ndets].cpu().numpy(), b._X[:b.ndets].cpu().numpy()
    assert np.array_equal(xa[:, :F - VIS_COLS], xb[:, :F - VIS_COLS])
    e = np.abs(xa - xb) / ((1 + np.abs(xa)) / std[None, :])
    print(f'online: max feature difference / bound unit {e.max():.3g} (<= 1e-5)')
    assert e.max() <= 1e-5
    ta, tb = a.tracks(), b.tracks()
    assert np.array_equal(ta, tb) and (ta >= 0).any()
