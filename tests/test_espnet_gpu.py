"""The embedding CNN on the device (-m gpu; csrc/espnet.hip: tmpnn_espnet_fwd; trackmpnn_amd.espnet.EspEmbedNet) against the
fixtures the reference's EESPNet_Seg left under tests/golden/espnet.

The yardstick of a fixture is the reference's own float32 error on it, e_ref = max|ref_out32 - ref_out64|: the device's
max|out - ref_out64| must stay within 8 e_ref.  Two correct float32 implementations that sum in different orders through some 40
layers differ by a small multiple of either one's error; a wrong tap, border, slope or BatchNorm channel is off by three or more
orders of magnitude.  Measured ratios: profiles/espnet.md."""
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


@functools.lru_cache(maxsize=None)
def device_case(name):
    """(net, images on the device, the net's maps) of a fixture, computed once."""
    from trackmpnn_amd import EspEmbedNet
    fx, sd = load_case(name)
    net = EspEmbedNet.from_state_dict(sd, DEV)
    images = torch.from_numpy(fx['images']).to(DEV)
    return net, images, net(images)


@pytest.mark.parametrize('name', list(CASES))
def test_maps_within_eight_times_the_references_own_float32_error(name):
    fx, _ = load_case(name)
    net, images, out = device_case(name)
    T, C, H, W, _ = CASES[name]
    assert net.C == C and out.dtype == torch.float32 and tuple(out.shape) == (T, C, H, W) and out.is_contiguous()
    assert not out.requires_grad
    ref = fx['ref_out64']
    e_ref = np.abs(fx['ref_out32'].astype(np.float64) - ref).max()
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print(f'{name}: e_ref = {e_ref:.3e}, device err = {err:.3e}, ratio = {err / e_ref:.2f} (<= 8), max|ref| = {np.abs(ref).max():.3f}')
    assert np.isfinite(err) and err <= 8 * e_ref


def test_the_wide_channel_tile_at_its_threshold():
    """csrc/espnet.hip gives a pointwise conv 32 output channels a lane once that fills every CU (pw_wide: 256 workgroups), 8
    otherwise, and the fixtures are too small to reach it.  144 x 240 with C = 256 is the smallest multiple-of-16 shape whose
    project_l1 (72 x 120 pixels: 34 workgroups, the last one partly idle, x 8 channel tiles) takes the wide tile while
    project_l2 (9 x 8) keeps the narrow one; levels 3 and 4 are 18 x 30 and 9 x 15.  No fixture of that size is stored: the
    yardstick is espnet_host in float32 against float64 on the CPU, which is the reference's own pair bit for bit
    (tests/test_espnet.py pins the float64 one, and the float32 one runs the same torch ops)."""
    from trackmpnn_amd import EspEmbedNet, espnet_host
    sd = espnet_weights(256, 108)
    images = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 3, 144, 240)).astype(np.float32))
    ref = espnet_host(sd, images, torch.float64).numpy()
    e_ref = np.abs(espnet_host(sd, images, torch.float32).numpy().astype(np.float64) - ref).max()
    net = EspEmbedNet.from_state_dict(sd, DEV)
    out = net(images.to(DEV))
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print(f'144x240 C=256: e_ref = {e_ref:.3e}, device err = {err:.3e}, ratio = {err / e_ref:.2f} (<= 8), max|ref| = {np.abs(ref).max():.3f}')
    assert np.isfinite(err) and err <= 8 * e_ref
    assert torch.equal(net(images.to(DEV)).view(torch.int32), out.view(torch.int32))


def test_an_image_of_a_batch_equals_the_same_image_alone_bit_for_bit():
    net, images, out = device_case('c4_batch3')
    for i in range(images.shape[0]):
        alone = net(images[i:i + 1].contiguous())
        assert torch.equal(alone[0].view(torch.int32), out[i].view(torch.int32)), f'image {i}'
    pair = net(images[1:3].contiguous())
    assert torch.equal(pair.view(torch.int32), out[1:3].view(torch.int32))


@pytest.mark.parametrize('name', ['c3_48x80', 'c5_c128'])
def test_two_calls_give_the_same_bits(name):
    net, images, out = device_case(name)
    assert torch.equal(net(images).view(torch.int32), out.view(torch.int32))


def test_out_is_written_and_a_second_call_allocates_nothing():
    net, images, out = device_case('c2_32x64')
    mine = torch.full_like(out, float('nan'))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = net(images, out=mine)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before                          # the workspace of this shape exists already
    assert got is mine and torch.equal(mine.view(torch.int32), out.view(torch.int32))
    for bad in (mine[:, :4], mine.double(), mine.cpu(), mine.permute(0, 1, 3, 2)):
        with pytest.raises(ValueError, match='out '):
            net(images, out=bad)


def test_launches_go_on_the_current_stream():
    net, images, out = device_case('c2_32x64')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = net(images)
    side.synchronize()
    assert torch.equal(got.view(torch.int32), out.view(torch.int32))


def test_what_the_call_refuses():
    net, images, _ = device_case('c1_16x16')
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        net(images.cpu())
    for H, W in ((24, 40), (20, 36), (16, 8)):
        with pytest.raises(ValueError, match='multiples of 16'):
            net(torch.zeros(1, 3, H, W, device=DEV))
    with pytest.raises(ValueError, match=r'images \[T, 3, H, W\] float32'):
        net(torch.zeros(1, 3, 16, 16, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='contiguous'):
        net(torch.zeros(1, 3, 16, 32, device=DEV).transpose(2, 3)[:, :, :16, :16].transpose(2, 3))
    with pytest.raises(ValueError, match='empty batch'):
        net(torch.zeros(0, 3, 16, 16, device=DEV))


def test_state_dict_round_trips_and_the_net_is_in_eval_mode():
    from trackmpnn_amd import EspEmbedNet
    net, images, out = device_case('c1_16x16')
    _, sd = load_case('c1_16x16')
    back = net.state_dict()
    assert list(back) == list(sd) and all(back[k] is sd[k] for k in sd)
    again = EspEmbedNet.from_state_dict(back, DEV)
    assert torch.equal(again(images).view(torch.int32), out.view(torch.int32))
    assert net.training is False and net.eval() is net and net.train(False) is net
    with pytest.raises(NotImplementedError, match='eval-mode network'):
        net.train(True)


# ---- behind the visual head: a tiny 'vis' store, the whole-sequence pass and one online push -----------------------------------
INPUT_HW, RAW_HW, N_FRAMES, FPB = (32, 80), (16, 40), 5, 3
PIX_MEAN, PIX_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@functools.lru_cache(maxsize=None)
def vis_case():
    """Two sequences of 5 frames of 16 x 40 pixels resized to the CNN's 32 x 80, batches of 3 frames (so a batch of 3 and one of
    2 per sequence), the seeded net with C = 128.  The reference (computed once): sequence_vis_host -- vis_head_host in float64 --
    over espnet_host(float64) maps."""
    from trackmpnn_amd import DetectionStore, EspEmbedNet, FrameStore, VisHead, espnet_host, sequence_features_host, sequence_vis_host
    rng = np.random.default_rng(78)
    mean, std = feature_stats(NCAT_KITTI, '2d+temp+vis')
    mean[-128:] = (0.02 * rng.random(128)).astype(np.float32)
    std[-128:] = (0.3 + 1.7 * rng.random(128)).astype(np.float32)
    seqs = [synth_sequence(rng, N_FRAMES, NCAT_KITTI, dets=(1, 3), im_hw=RAW_HW) for _ in range(2)]
    store = DetectionStore(seqs, NCAT_KITTI, '2d+temp+vis', mean, std, device=DEV)
    raw = [rng.integers(0, 256, (N_FRAMES,) + RAW_HW + (3,), dtype=np.uint8) for _ in seqs]
    frames = FrameStore.from_raw(raw, INPUT_HW, PIX_MEAN, PIX_STD, DEV)
    sd = espnet_weights(128, 9)
    net = EspEmbedNet.from_state_dict(sd, DEV)
    head = VisHead(INPUT_HW, 1, mean, std, DEV)
    embed = lambda images: espnet_host(sd, torch.from_numpy(images), torch.float64).numpy()
    ref = []
    for s in range(2):
        sample = sequence_features_host(store, s)
        sample.X = sample.X.astype(np.float64)
        ref.append(sequence_vis_host(store, s, sample, frames, embed, mean, std, INPUT_HW, 1, frames_per_batch=FPB)[:, -128:])
    return dict(store=store, seqs=seqs, raw=raw, frames=frames, net=net, head=head, mean=mean, std=std, ref=ref)


def rows_err(got, ref, std):
    """max |err| in units of the bound tests/test_chunk_vis_gpu.py holds the head's rows to: 1e-5 (1 + |v|) / std."""
    return (np.abs(got - ref) / ((1 + np.abs(ref)) / std[None, -128:])).max(initial=0)


def test_attach_vis_fills_the_visual_columns_from_the_device_net():
    from trackmpnn_amd import SequenceFeatures
    c = vis_case()
    sf = SequenceFeatures(c['store'])
    plain = [d['X'].clone() for d in sf.build(frames_per_batch=FPB)]
    sf.attach_vis(c['head'], c['frames'], c['net'], frames_per_batch=FPB)
    sf.check()
    assert {(2, 32, 80), (3, 32, 80)} <= set(c['net']._ws)                   # one workspace per batch size, reused
    for k in range(2):
        a, b = int(sf.offsets[k]), int(sf.offsets[k + 1])
        X = sf.X[a:b].cpu().numpy()
        assert b > a and np.array_equal(X[:, :-128].view(np.int32), plain[k][0, :, :-128].cpu().numpy().view(np.int32))
        err = rows_err(X[:, -128:].astype(np.float64), c['ref'][k], c['std'])
        print(f'sequence {k}: {b - a} rows, max rows err / bound unit {err:.3g} (<= 1e-5)')
        assert err <= 1e-5


def test_an_online_push_lands_on_the_same_rows():
    from trackmpnn_amd import FeatureSpec, FramePrep, OnlineTracker, OnlineVis, TrackMPNN
    c = vis_case()
    seq = c['seqs'][1]
    idx = np.flatnonzero(seq['frame'] == 0)                                    # the store sorts stably by frame: this order
    assert idx.size >= 1
    torch.manual_seed(3)
    model = TrackMPNN('2d+temp+vis', NCAT_KITTI, 32, 0, 'diff').to(DEV).eval()
    spec = FeatureSpec(NCAT_KITTI, '2d+temp+vis', c['mean'], c['std'])
    prep = FramePrep(INPUT_HW, PIX_MEAN, PIX_STD, device=DEV)
    trk = OnlineTracker(model, 3, 0, False, True, spec=spec, device=DEV, max_dets=8, vis=OnlineVis(c['head'], prep, c['net']))
    trk.push(seq['cat'][idx], seq['score'][idx].astype(np.float32), seq['box'][idx].astype(np.float32), frame=c['raw'][1][0], last=True)
    assert trk.ndets == idx.size
    got = trk._X[:trk.ndets, -128:].cpu().numpy().astype(np.float64)
    err = rows_err(got, c['ref'][1][:idx.size], c['std'])
    print(f'online push: {idx.size} rows, max rows err / bound unit {err:.3g} (<= 1e-5)')
    assert err <= 1e-5
