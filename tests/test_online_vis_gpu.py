"""The online tracker's default-mode path on the device (-m gpu): push(cat, score, box, frame=img) under OnlineVis -- resize,
CNN, visual head, all on the device -- leaves the tracker's feature rows bit-equal to the rows assembled offline (resize_host,
FrameStore.gather, the same CNN, VisHead.rows, online_features_host) and gives infer_sequence's tracks on them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RAW_HW, INPUT_HW, NCAT, WIN = (37, 61), (48, 80), 3, 3
DETS = [2, 3, 0, 4, 1, 3, 2, 4]                                   # per frame; one frame without detections
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


class _Net(torch.nn.Module):
    """128 channels of element-wise ops only, maps[:, c] = x[:, c % 3] * a[c] + b[c]: no dependence on the batch size or on a
    library's choice of algorithm, so a frame alone and a frame in a batch give the same bits."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(17)
        self.register_buffer('a', (torch.rand(128, generator=g) * 2 + 0.5).view(1, 128, 1, 1))
        self.register_buffer('b', torch.randn(128, generator=g).view(1, 128, 1, 1))
        self.register_buffer('idx', torch.arange(128) % 3)

    def forward(self, x):
        return x[:, self.idx] * self.a + self.b


@pytest.fixture(scope='module')
def scene():
    """The stream, the parts shared by both solvers, and the feature rows X assembled offline (computed once)."""
    from trackmpnn_amd import FeatureSpec, FramePrep, FrameStore, TrackMPNN, VisHead, online_features_host, resize_host
    rng = np.random.default_rng(23)
    F = NCAT + 5 + 2 + 128
    mean = rng.normal(size=F).astype(np.float32)
    std = (rng.random(F) + 0.5).astype(np.float32)
    mean[-128:], std[-128:] = (rng.random(128) * 0.01).astype(np.float32), (rng.random(128) * 0.02 + 0.005).astype(np.float32)
    spec = FeatureSpec(NCAT, '2d+temp+vis', mean, std)
    frames = rng.integers(0, 256, (len(DETS),) + RAW_HW + (3,), dtype=np.uint8)
    dets = []
    for D in DETS:
        x1, y1 = rng.random(D) * 40, rng.random(D) * 22
        box = np.stack([x1, y1, x1 + 2 + rng.random(D) * 18, y1 + 2 + rng.random(D) * 12], 1).astype(np.float32)
        dets.append((rng.integers(1, NCAT + 1, size=D), rng.random(D).astype(np.float32), box))
    torch.manual_seed(31)
    model = TrackMPNN('2d+temp+vis', NCAT, 32, 0, 'diff').to(DEV).eval()
    with torch.no_grad():                                          # (as tests/test_online_gpu.py: biases that let edges win)
        for k, prm in model.named_parameters():
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(2)).to(DEV))
    net = _Net().to(DEV).eval()
    head = VisHead(INPUT_HW, 1, mean, std, device=DEV)
    prep = FramePrep(INPUT_HW, MEAN, STD, device=DEV)
    # offline: host resize -> the existing store and gather -> the CNN on all frames at once -> the head -> the other columns
    store = FrameStore([resize_host(frames, INPUT_HW)], MEAN, STD, device=DEV)
    plan = np.array([[0, t, 0] for t in range(len(DETS))])
    with torch.no_grad():
        maps = net(store.gather(plan))
    box_all = np.concatenate([d[2] for d in dets])
    map_of = np.repeat(np.arange(len(DETS)), DETS)
    vis_rows = head.rows(maps, box_all, map_of, RAW_HW).cpu().numpy()
    other = np.concatenate([online_features_host(spec, c, s, b, t, vis=np.zeros((len(c), 128), np.float32))[:, :F - 128]
                            for t, (c, s, b) in enumerate(dets)])
    X = np.ascontiguousarray(np.concatenate([other, vis_rows], axis=1), dtype=np.float32)
    y = np.stack([map_of, np.full(map_of.size, -1)], 1).astype(np.int64)
    assert X.shape == (sum(DETS), F) and np.isfinite(X).all()
    return dict(spec=spec, frames=frames, dets=dets, model=model, net=net, head=head, prep=prep, X=X, y=y, F=F)


@pytest.mark.parametrize('hungarian', [False, True], ids=['greedy', 'hungarian'])
def test_pushing_frames_equals_the_offline_rows_and_tracks(scene, hungarian):
    from trackmpnn_amd import OnlineTracker, OnlineVis
    from trackmpnn_amd.loops import infer_sequence
    s = scene
    trk = OnlineTracker(s['model'], WIN, 0, hungarian, True, spec=s['spec'], device=DEV, max_dets=8,
                        vis=OnlineVis(s['head'], s['prep'], s['net']))
    frames_t = torch.from_numpy(s['frames'])
    for t, (cat, score, box) in enumerate(s['dets']):
        frame = s['frames'][t] if t % 2 else frames_t[t]          # a numpy frame and a tensor frame alike
        trk.push(cat, score, box, frame=frame, last=t == len(DETS) - 1)
    assert trk.ndets == s['X'].shape[0] and trk.frames == len(DETS) and trk.growths >= 1
    got = trk._X[:trk.ndets].cpu().numpy()
    F = s['F']
    assert np.array_equal(got[:, :F - 128].view(np.uint32), s['X'][:, :F - 128].view(np.uint32))
    assert np.array_equal(got[:, F - 128:].view(np.uint32), s['X'][:, F - 128:].view(np.uint32))
    y1, calls, _ = infer_sequence(s['model'], torch.from_numpy(s['X'])[None], torch.from_numpy(s['y'])[None], WIN, 0, hungarian,
                                  DEV, True)
    tracks = trk.tracks()
    print(f'hungarian={hungarian}: {calls} forward calls, tracks {tracks.tolist()}')
    assert calls > 0 and np.array_equal(tracks, y1[:, 1])


def test_host_vis_pushes_keep_working_beside_frame_pushes(scene):
    """push(..., vis=host_array) on a tracker that has an OnlineVis, and push_features: unchanged, the same rows."""
    from trackmpnn_amd import OnlineTracker, OnlineVis
    s = scene
    F = s['F']
    trk = OnlineTracker(s['model'], WIN, 0, False, True, spec=s['spec'], device=DEV, vis=OnlineVis(s['head'], s['prep'], s['net']))
    ref = OnlineTracker(s['model'], WIN, 0, False, True, device=DEV)
    lo = 0
    for t, (cat, score, box) in enumerate(s['dets']):
        rows = s['X'][lo:lo + len(cat)]
        lo += len(cat)
        raw_vis = (rows[:, F - 128:] * s['spec'].std[-128:] + s['spec'].mean[-128:]).astype(np.float32)
        trk.push(cat, score, box, vis=raw_vis, last=t == len(DETS) - 1)
        ref.push_features(rows, last=t == len(DETS) - 1)
    a, b = trk._X[:trk.ndets].cpu().numpy(), ref._X[:ref.ndets].cpu().numpy()
    assert np.array_equal(a[:, :F - 128].view(np.uint32), b[:, :F - 128].view(np.uint32))
    assert np.array_equal(b.view(np.uint32), s['X'].view(np.uint32))
