"""The embedding CNN answered at the box centres on the device (-m gpu; csrc/espnet.hip: tmpnn_espnet_trunk, tmpnn_espnet_centres;
csrc/vishead.hip: tmpnn_vis_head_pixels, tmpnn_vis_head_rows_from_logits; EspEmbedNet.centres, EspCentres, VisHead.rows).

The yardstick is the dense call of the same net: logits_at(pix) must equal net(images)[t, :, cy, cx] as int32 words at EVERY pixel
of a fixture.  Every pixel is the smallest input that reaches every place the kernel can go wrong: the four corners and all
borders (the clamps of esp_axis and min(i0 + 1, n - 1)), coordinates with zero and non-zero blend weights on each of the three
levels, all four columns of the dense resize's four-column threads, the switch between the two sources of both convs, and the
image offset with T > 1.  Against the reference the bound is the one of tests/test_espnet_gpu.py: 8 e_ref."""
import functools

import numpy as np
import pytest
import torch

from tests.espnet_cases import CASES, espnet_weights, load_case
from tests.seqfeat_cases import NCAT_KITTI, feature_stats, synth_sequence

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def words(t):
    return t.contiguous().view(torch.int32)


def all_pixels(T, H, W, seed):
    """Every pixel of a [T, ., H, W] map in a seeded shuffled order, a sixteenth of them listed twice: int32 on the device."""
    rng = np.random.default_rng(seed)
    n = T * H * W
    pix = np.concatenate([np.arange(n), rng.choice(n, max(1, n // 16), replace=False)])
    rng.shuffle(pix)
    return torch.from_numpy(pix.astype(np.int32)).to(DEV)


def gather(maps, pix):
    """maps[t, :, cy, cx] for pix = (t H + cy) W + cx: [D, C]."""
    T, C, H, W = maps.shape
    p = pix.long()
    t, rem = p // (H * W), p % (H * W)
    return maps[t, :, rem // W, rem % W]


@functools.lru_cache(maxsize=None)
def device_case(name):
    """(net, images on the device, the dense maps, all pixels, the logits at them, their flags) of a fixture, computed once."""
    from trackmpnn_amd import EspEmbedNet
    fx, sd = load_case(name)
    T, C, H, W, seed = CASES[name]
    net = EspEmbedNet.from_state_dict(sd, DEV)
    images = torch.from_numpy(fx['images']).to(DEV)
    dense = net(images)
    pix = all_pixels(T, H, W, seed)
    logits, flags = net.centres(images).logits_at(pix)
    return net, images, dense, pix, logits, flags


@pytest.mark.parametrize('name', ['c1_16x16', 'c4_batch3', 'c5_c128', 'c3_48x80'])
def test_every_pixel_equals_the_dense_map_bit_for_bit(name):
    T, C, H, W, _ = CASES[name]
    net, images, dense, pix, logits, flags = device_case(name)
    assert pix.numel() > T * H * W and set(pix.tolist()) == set(range(T * H * W))
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (pix.numel(), C) and logits.is_contiguous()
    assert flags.dtype == torch.int32 and tuple(flags.shape) == (pix.numel(),) and not flags.any()
    want = gather(dense, pix)
    diff = (words(logits) != words(want)).any(dim=1)
    assert not diff.any(), f'{int(diff.sum())} of {pix.numel()} pixels differ, the first: pix {int(pix[diff][0])}'


@pytest.mark.parametrize('name', ['c1_16x16', 'c4_batch3', 'c5_c128'])
def test_logits_within_eight_times_the_references_own_float32_error(name):
    fx, _ = load_case(name)
    _, _, _, pix, logits, _ = device_case(name)
    ref = fx['ref_out64']
    e_ref = np.abs(fx['ref_out32'].astype(np.float64) - ref).max()
    want = gather(torch.from_numpy(ref), pix.cpu()).numpy()
    err = np.abs(logits.cpu().numpy().astype(np.float64) - want).max()
    print(f'{name}: e_ref = {e_ref:.3e}, centres err = {err:.3e}, ratio = {err / e_ref:.2f} (<= 8)')
    assert np.isfinite(err) and err <= 8 * e_ref


def test_the_upper_end_of_the_supported_channel_count():
    """C = 256: one lane group per conv, the LDS arrays full."""
    from trackmpnn_amd import EspEmbedNet
    net = EspEmbedNet.from_state_dict(espnet_weights(256, 108), DEV)
    images = torch.from_numpy(np.random.default_rng(6).standard_normal((1, 3, 16, 32)).astype(np.float32)).to(DEV)
    pix = all_pixels(1, 16, 32, 7)
    logits, flags = net.centres(images).logits_at(pix)
    assert tuple(logits.shape) == (pix.numel(), 256) and not flags.any()
    assert torch.equal(words(logits), words(gather(net(images), pix)))


def test_a_wider_net_is_sent_to_the_dense_call():
    from trackmpnn_amd import EspEmbedNet
    net = EspEmbedNet.from_state_dict(espnet_weights(260, 11), DEV, centres=True)
    with pytest.raises(ValueError, match='dense call'):
        net(torch.zeros(1, 3, 16, 16, device=DEV))


# ---- through the visual head ---------------------------------------------------------------------------------------------------
def head_case():
    """The head over c5_c128's 16 x 32 map (down_ratio 1, images of 16 x 32), 40 seeded boxes, a quarter of them with the centre
    outside the image on one side or another, and two of them on the same pixel."""
    from trackmpnn_amd import VisHead
    rng = np.random.default_rng(31)
    mean = (0.02 * rng.random(128)).astype(np.float32)
    std = (0.3 + 1.7 * rng.random(128)).astype(np.float32)
    head = VisHead((16, 32), 1, mean, std, DEV)
    D = 40
    cx, cy = rng.uniform(0, 32, D), rng.uniform(0, 16, D)
    cx[:5], cy[5:10] = rng.uniform(-9, -1, 5), rng.uniform(16.5, 30, 5)
    cx[10:12], cy[12] = rng.uniform(33, 50, 2), -3.0
    cx[20], cy[20] = cx[21], cy[21]
    w, h = rng.uniform(1, 6, D), rng.uniform(1, 6, D)
    box = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
    return head, box, np.zeros(D, np.int32), (16, 32)


def test_rows_through_the_head_equal_the_dense_rows_bit_for_bit():
    net, images, dense, _, _, _ = device_case('c5_c128')
    head, box, map_of, im_hw = head_case()
    D, k = box.shape[0], 5
    X0 = torch.from_numpy(np.random.default_rng(2).standard_normal((D, 140)).astype(np.float32)).to(DEV)
    Xd, Xs = X0.clone(), X0.clone()
    assert head.rows(dense, box, map_of, im_hw, out=Xd, col=k) is Xd
    rec_d, log_d = head.record(), head.last_logits().clone()
    assert head.rows(net.centres(images), box, map_of, im_hw, out=Xs, col=k) is Xs
    rec_s, log_s = head.record(), head.last_logits()
    assert rec_d['row_clamped'].sum() >= 10 and not rec_d['row_clamped'].all()
    assert torch.equal(words(Xs[:, k:k + 128]), words(Xd[:, k:k + 128]))
    assert torch.equal(words(Xs[:, :k]), words(X0[:, :k])) and torch.equal(words(Xs[:, k + 128:]), words(X0[:, k + 128:]))
    assert torch.equal(words(log_s), words(log_d))
    assert set(rec_s) == set(rec_d)
    for key in rec_d:
        assert np.array_equal(rec_s[key], rec_d[key]), key
    # a new tensor instead of `out`, and per-row image sizes on the device
    hw = torch.tensor([im_hw] * D, dtype=torch.float32, device=DEV)
    got = head.rows(net.centres(images), torch.from_numpy(box).to(DEV), torch.from_numpy(map_of).to(DEV), hw)
    assert tuple(got.shape) == (D, 128) and torch.equal(words(got), words(Xd[:, k:k + 128]))


def test_the_head_refuses_what_the_handle_cannot_serve():
    net, images, _, _, _, _ = device_case('c5_c128')
    head, box, map_of, im_hw = head_case()
    D = box.shape[0]
    with pytest.raises(ValueError, match='dense call'):
        head.forward(net.centres(images), box, map_of, im_hw, np.arange(D), [0, D])
    net8, images8, _, _, _, _ = device_case('c1_16x16')
    with pytest.raises(ValueError, match='C = 128'):
        head.rows(net8.centres(images8), box, map_of, im_hw)
    # no detection at all
    got = head.rows(net.centres(images), np.zeros((0, 4), np.float32), np.zeros(0, np.int32), im_hw)
    assert tuple(got.shape) == (0, 128) and head.record()['rows'].tolist() == [0]


# ---- drop-in: the whole-sequence pass and one online push, dense net against centres=True ------------------------------------------
INPUT_HW, RAW_HW, N_FRAMES, FPB = (32, 80), (16, 40), 5, 3
PIX_MEAN, PIX_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@functools.lru_cache(maxsize=None)
def vis_case():
    """The two-sequence 'vis' store of tests/test_espnet_gpu.py (5 frames of 16 x 40 resized to 32 x 80, batches of 3 frames), with
    the seeded C = 128 net twice: dense and centres=True."""
    from trackmpnn_amd import DetectionStore, EspEmbedNet, FrameStore, VisHead
    rng = np.random.default_rng(78)
    mean, std = feature_stats(NCAT_KITTI, '2d+temp+vis')
    mean[-128:] = (0.02 * rng.random(128)).astype(np.float32)
    std[-128:] = (0.3 + 1.7 * rng.random(128)).astype(np.float32)
    seqs = [synth_sequence(rng, N_FRAMES, NCAT_KITTI, dets=(1, 3), im_hw=RAW_HW) for _ in range(2)]
    store = DetectionStore(seqs, NCAT_KITTI, '2d+temp+vis', mean, std, device=DEV)
    raw = [rng.integers(0, 256, (N_FRAMES,) + RAW_HW + (3,), dtype=np.uint8) for _ in seqs]
    frames = FrameStore.from_raw(raw, INPUT_HW, PIX_MEAN, PIX_STD, DEV)
    sd = espnet_weights(128, 9)
    return dict(store=store, seqs=seqs, raw=raw, frames=frames, mean=mean, std=std, head=VisHead(INPUT_HW, 1, mean, std, DEV),
                dense=EspEmbedNet.from_state_dict(sd, DEV), sparse=EspEmbedNet.from_state_dict(sd, DEV, centres=True))


def test_attach_vis_with_a_centres_net_fills_the_same_bits():
    from trackmpnn_amd import EspCentres, SequenceFeatures
    c = vis_case()
    X = {}
    for kind in ('dense', 'sparse'):
        sf = SequenceFeatures(c['store'])
        sf.build(frames_per_batch=FPB)
        sf.attach_vis(c['head'], c['frames'], c[kind], frames_per_batch=FPB)
        sf.check()
        X[kind] = sf.X.clone()
    assert X['dense'].shape[0] > 0 and torch.equal(words(X['sparse']), words(X['dense']))
    assert isinstance(c['sparse'](c['frames'].gather(np.array([[0, 0, 0]], np.int64))), EspCentres)
    assert {(2, 32, 80), (3, 32, 80)} <= set(c['sparse']._cws) and not c['sparse']._ws         # no dense workspace was made


def test_an_online_push_with_a_centres_net_lands_on_the_same_bits():
    from trackmpnn_amd import FeatureSpec, FramePrep, OnlineTracker, OnlineVis, TrackMPNN
    c = vis_case()
    seq = c['seqs'][1]
    idx = np.flatnonzero(seq['frame'] == 0)
    assert idx.size >= 1
    rows = {}
    for kind in ('dense', 'sparse'):
        torch.manual_seed(3)
        model = TrackMPNN('2d+temp+vis', NCAT_KITTI, 32, 0, 'diff').to(DEV).eval()
        spec = FeatureSpec(NCAT_KITTI, '2d+temp+vis', c['mean'], c['std'])
        prep = FramePrep(INPUT_HW, PIX_MEAN, PIX_STD, device=DEV)
        trk = OnlineTracker(model, 3, 0, False, True, spec=spec, device=DEV, max_dets=8, vis=OnlineVis(c['head'], prep, c[kind]))
        trk.push(seq['cat'][idx], seq['score'][idx].astype(np.float32), seq['box'][idx].astype(np.float32), frame=c['raw'][1][0],
                 last=True)
        assert trk.ndets == idx.size
        rows[kind] = trk._X[:trk.ndets].clone()
    assert torch.equal(words(rows['sparse']), words(rows['dense']))


# ---- behaviour -----------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_second_allocates_nothing():
    net, images, _, pix, logits, _ = device_case('c3_48x80')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    h = net.centres(images)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before                          # the workspace of this shape exists already
    assert h.shape == (1, 8, 48, 80) and (h.T, h.C, h.H, h.W) == h.shape
    again, _ = h.logits_at(pix)
    assert torch.equal(words(again), words(logits))
    mine = torch.full_like(logits, float('nan'))
    got, _ = h.logits_at(pix, out=mine)
    assert got is mine and torch.equal(words(mine), words(logits))


def test_a_handle_is_refused_once_its_workspace_has_been_overwritten():
    net, images, _, pix, _, _ = device_case('c1_16x16')
    old = net.centres(images)
    new = net.centres(images)
    with pytest.raises(RuntimeError, match='overwritten'):
        old.logits_at(pix)
    new.logits_at(pix)


def test_launches_go_on_the_current_stream():
    net, images, _, pix, logits, _ = device_case('c4_batch3')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, _ = net.centres(images).logits_at(pix)
    side.synchronize()
    assert torch.equal(words(got), words(logits))


def test_no_pixel_and_pixels_outside_the_map():
    net, images, dense, _, _, _ = device_case('c4_batch3')
    T, C, H, W, _ = CASES['c4_batch3']
    h = net.centres(images)
    logits, flags = h.logits_at(torch.zeros(0, dtype=torch.int32, device=DEV))
    assert tuple(logits.shape) == (0, C) and logits.dtype == torch.float32 and tuple(flags.shape) == (0,)
    n = T * H * W
    pix = torch.tensor([5, -1, n - 7, n, 2 * n, -n, 77], dtype=torch.int32, device=DEV)
    logits, flags = h.logits_at(pix)
    assert flags.tolist() == [0, 1, 0, 1, 1, 1, 0]
    clamped = torch.tensor([5, 0, n - 7, n - 1, n - 1, 0, 77], dtype=torch.int32, device=DEV)
    assert torch.equal(words(logits), words(gather(dense, clamped)))
    for bad in (pix.long(), pix.cpu(), pix.view(1, -1), torch.arange(0, 14, device=DEV, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match='pix '):
            h.logits_at(bad)
