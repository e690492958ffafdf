"""Training chunks drawn with the visual feature group on the MI355X (-m gpu): the device draw of a 'vis' store against
draw_host bit for bit in every field, FrameStore.gather against frames_host bit for bit, DrawnChunks.attach_vis against
vis_head_host in float64 (the bounds of tests/test_vis_head_gpu.py), the launch / wait budget, and train_epoch(vis=...) against
the pieces it composes.  The definitions themselves are checked without a GPU in tests/test_chunk_vis.py."""
import functools
import random

import numpy as np
import pytest
import torch

from tests.test_chunk_draw import NCAT, synth_sequences
from tests.test_chunk_vis import (IMG_MEAN, IMG_STD, VIS_MEAN, VIS_STD, plain_store, vis_rule_cases, vis_stats, vis_store,
                                  with_height)
from tests.test_optim_gpu import _sync_warnings
from trackmpnn_amd.vishead import VIS_COLS, vis_centres_host, vis_head_host, vis_pixels_host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _bits(t):
    return t.contiguous().view(torch.int32)


def assert_device_equals_host(sampler, idx, step, plain_sampler=None):
    """Every field of the device draw of a 'vis' store equals draw_host bit for bit (rows [0, offsets[B])); with
    `plain_sampler` (the same chunks over the store without 'vis') the non-vis fields equal its DEVICE draw too."""
    st = sampler.store
    dr, hd = sampler.draw(idx, step), sampler.draw_host(idx, step)
    nd, Fp = int(hd.offsets[-1]), st.F - VIS_COLS
    assert dr.n_max == hd.n_max and tuple(dr.X.shape) == (hd.n_max, st.F) and tuple(dr.y.shape) == (hd.n_max, 2)
    assert tuple(dr.box.shape) == (hd.n_max, 4) and tuple(dr.im_hw.shape) == (hd.n_max, 2)
    assert tuple(dr.map_of.shape) == (hd.n_max,) and tuple(dr.track.shape) == (hd.n_max,)
    assert (dr.box.dtype, dr.im_hw.dtype, dr.map_of.dtype, dr.track.dtype) == (torch.float32, torch.float32, torch.int32, torch.int32)
    assert torch.equal(dr.offsets.cpu(), torch.from_numpy(hd.offsets)) and torch.equal(dr.flags.cpu(), torch.from_numpy(hd.flags))
    assert torch.equal(dr.y[:nd].cpu(), torch.from_numpy(hd.y))
    assert torch.equal(_bits(dr.X[:nd, :Fp].cpu()), _bits(torch.from_numpy(hd.X[:, :Fp].copy())))
    assert torch.equal(_bits(dr.box[:nd].cpu()), _bits(torch.from_numpy(hd.box)))
    assert torch.equal(_bits(dr.im_hw[:nd].cpu()), _bits(torch.from_numpy(hd.im_hw)))
    assert torch.equal(dr.map_of[:nd].cpu(), torch.from_numpy(hd.map_of)) and torch.equal(dr.track[:nd].cpu(), torch.from_numpy(hd.track))
    assert np.array_equal(dr.plan.frames, hd.plan.frames) and np.array_equal(dr.plan.slot, hd.plan.slot)
    if plain_sampler is not None:
        dp = plain_sampler.draw(idx, step)
        assert dp.box is None and dp.plan is None and dp.n_max == dr.n_max
        assert torch.equal(dp.offsets, dr.offsets) and torch.equal(dp.flags, dr.flags) and torch.equal(dp.y[:nd], dr.y[:nd])
        assert torch.equal(_bits(dp.X[:nd]), _bits(dr.X[:nd, :Fp]))
    return dr, hd


# ---- 1. device draw == host definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('feats', ['2d+vis', '2d+temp+vis'])
def test_mixed_sequences(feats):
    from trackmpnn_amd import ChunkSampler
    seqs, chunks = vis_rule_cases()                    # several widths and heights, false positives, empty frames, a one-frame sequence
    store, plain = vis_store(seqs, feats, DEV), plain_store(seqs, feats, DEV)
    sampler, psampler = ChunkSampler(store, chunks, seed=2024), ChunkSampler(plain, chunks, seed=2024)
    rng = np.random.RandomState(1)
    flags = []
    for step in (0, 1, 2 ** 40 + 3):
        idx = rng.randint(0, len(chunks), 3 * len(chunks))                   # (repeats and any order)
        _, hd = assert_device_equals_host(sampler, idx, step, psampler)
        flags.append(hd.flags)
        assert not hd.kept.all()
    assert set(np.concatenate(flags)) == {0, 1, 2, 3}
    assert_device_equals_host(sampler, [5], 0, psampler)
    # dropout 0 and 1, and no transforms at all
    for kw in (dict(dropout=0.0), dict(dropout=1.0), dict(random_transforms=False)):
        s2, p2 = ChunkSampler(store, chunks, seed=7, **kw), ChunkSampler(plain, chunks, seed=7, **kw)
        _, hd = assert_device_equals_host(s2, np.arange(len(chunks)), 9, p2)
        if kw.get('dropout') == 1.0:
            assert hd.offsets[-1] == 0 and not hd.kept.any() and hd.box.shape == (0, 4) and hd.plan.frames.shape[0] > 0
        else:
            assert hd.kept.all()
        if 'random_transforms' in kw:
            assert not hd.flags.any() and not hd.plan.frames[:, 2].any()


def test_an_empty_chunk_two_tiles_and_a_one_frame_list():
    from trackmpnn_amd import ChunkSampler
    rng = np.random.RandomState(3)
    z = np.zeros(0, np.int64)
    empty = dict(frame=z, track=z, cat=z, box=np.zeros((0, 4)), score=np.zeros(0), width=1242, height=375, num_frames=4)
    n, T = 700, 50                                                          # 14 detections a frame: 40 listed frames = 560 rows
    x1 = np.round(rng.uniform(0, 1000, n), 2)
    big = dict(frame=np.repeat(np.arange(T), n // T), track=rng.randint(-1, 300, n), cat=rng.randint(1, NCAT + 1, n),
               box=np.stack([x1, x1 * 0 + 150.5, x1 + np.round(rng.uniform(5, 150, n), 2), x1 * 0 + 200.25], 1),
               score=rng.uniform(0, 1, n), width=1238, height=374, num_frames=T)
    small = with_height(synth_sequences(seed=5, lengths=(9,)))[0]
    longest = list(range(3, 43))
    chunks = [(1, [7]), (1, longest), (0, [0, 1, 2, 3]), (2, [0, 1, 2, 3, 4]), (1, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18])]
    for feats in ('2d+vis', '2d+temp+vis'):
        store, plain = vis_store([empty, big, small], feats, DEV), plain_store([empty, big, small], feats, DEV)
        sampler, psampler = ChunkSampler(store, chunks, seed=12), ChunkSampler(plain, chunks, seed=12)
        assert sampler.size.tolist()[:3] == [14, 560, 0] and sampler.size[4] == 266 and sampler.L == 40
        for step in (0, 1):
            dr, hd = assert_device_equals_host(sampler, [0, 1, 2, 3, 4, 2, 1], step, psampler)
            assert hd.offsets[2] == hd.offsets[3] and hd.offsets[2] - hd.offsets[1] > 256       # the empty chunk; two tiles kept
            assert (hd.plan.slot[0, 1:] == -1).all() and (hd.plan.slot[1] >= 0).all()
        dr, hd = assert_device_equals_host(sampler, [2], 0, psampler)                            # a draw of nothing
        assert dr.n_max == 0 and dr.box.shape == (0, 4) and hd.plan.frames.shape == (4, 3)


# ---- 2. the frames -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H, W', [(2, 3), (5, 17), (8, 64), (7, 130), (40, 130), (48, 160), (2, 4100)])
def test_gather_equals_frames_host(H, W):
    """The issue's sizes (a workgroup holds the whole image), then sizes with several workgroups an image whose runs of rows
    start off a 16-byte boundary (40 x 130), on one (48 x 160), and a row longer than a run (2 x 4100)."""
    from trackmpnn_amd import FrameStore
    rng = np.random.default_rng(H * 1000 + W)
    seqs = [rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8) for nf in (3, 1, 2)]
    fs = FrameStore(seqs, IMG_MEAN, IMG_STD, DEV)
    host = FrameStore(seqs, IMG_MEAN, IMG_STD, device=None)
    # a repeated row, one frame both plain and mirrored, the store's first and last frame (the last bytes of the buffer)
    plan = np.asarray([[2, 1, 1], [0, 0, 0], [0, 2, 1], [0, 2, 0], [1, 0, 1], [2, 1, 1], [2, 1, 0], [0, 1, 1]])
    for p in (plan, plan[:1], plan[3:4]):                                   # T = 8, and T = 1 mirrored / plain
        got, want = fs.gather(p), host.frames_host(p)
        assert got.dtype == torch.float32 and tuple(got.shape) == (p.shape[0], 3, H, W)
        assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(want)))
    assert np.array_equal(fs.frames_host(plan[:2]), host.frames_host(plan[:2]))                  # (a device store's host definition)
    assert tuple(fs.gather(np.zeros((0, 3), np.int64)).shape) == (0, 3, H, W)
    with pytest.raises(ValueError, match='frame 3 of sequence 0'):
        fs.gather(np.asarray([[0, 3, 0]]))


# ---- 3. the head on a draw ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attach_case():
    from trackmpnn_amd import ChunkSampler
    seqs, chunks = vis_rule_cases()
    sampler = ChunkSampler(vis_store(seqs, '2d+temp+vis', DEV), chunks, seed=11)
    idx = np.arange(len(chunks))[::2]
    hd = sampler.draw_host(idx, 4)
    Hm, Wm, input_hw, down = 12, 40, (48, 160), 4
    maps = np.random.default_rng(5).standard_normal((hd.plan.frames.shape[0], VIS_COLS, Hm, Wm)).astype(np.float32)
    g = np.random.default_rng(6).uniform(-2, 2, idx.size)
    _, rows, loss, dmaps = vis_head_host(maps.astype(np.float64), hd.box, hd.map_of, hd.im_hw, hd.track, hd.offsets, VIS_MEAN, VIS_STD,
                                         input_hw, down, g=g)
    cy, cx, _, _ = vis_pixels_host(*vis_centres_host(hd.box, hd.im_hw, input_hw, down), hd.map_of, Hm, Wm)
    sharers = np.zeros((maps.shape[0], Hm, Wm), np.int64)
    lab = hd.track >= 0
    np.add.at(sharers, (hd.map_of[lab], cy[lab], cx[lab]), 1)
    return sampler, idx, hd, maps, g, (input_hw, down), dict(rows=rows, loss=loss, dmaps=dmaps, sharers=sharers)


def _run_attach(junk_tail):
    from trackmpnn_amd import VisHead
    sampler, idx, hd, maps, g, (input_hw, down), _ = _attach_case()
    mean, std = vis_stats('2d+temp+vis')
    head = VisHead(input_hw, down, mean, std, DEV)
    dr = sampler.draw(idx, 4)
    nd = int(hd.offsets[-1])
    assert 0 < nd < dr.n_max
    dr.X[:, sampler.store.F - VIS_COLS:] = -7.5
    if junk_tail:                                                           # rows at and beyond offsets[B]: anything at all
        dr.box[nd:] = torch.tensor([float('nan'), -1e30, 1e30, float('inf')], device=DEV)
        dr.im_hw[nd:] = 0.0
        dr.map_of[nd:] = torch.tensor([-5, 2 ** 31 - 1], dtype=torch.int32, device=DEV).repeat(dr.n_max)[:dr.n_max - nd]
        dr.track[nd:] = 77
    before = dr.X.clone()
    m = torch.from_numpy(maps).to(DEV).requires_grad_()
    loss = dr.attach_vis(head, m)
    assert loss.requires_grad and tuple(loss.shape) == (idx.size,) and not dr.X.requires_grad
    (loss * torch.from_numpy(g.astype(np.float32)).to(DEV)).sum().backward()
    return dr, before, loss.detach().cpu().numpy(), m.grad.cpu().numpy(), nd


def test_attach_vis_equals_the_host_in_float64():
    """Rows: |err| <= 1e-5 (1 + |value|) / std; loss: rtol 1e-5; dmaps: 1e-5 (1 + |value|) times the rows that share the pixel
    (the bounds tests/test_vis_head_gpu.py states and uses).  The other columns of X keep their bits."""
    sampler, idx, hd, maps, g, _, ref = _attach_case()
    dr, before, loss, dmaps, nd = _run_attach(junk_tail=False)
    Fp = sampler.store.F - VIS_COLS
    assert torch.equal(_bits(dr.X[:, :Fp]), _bits(before[:, :Fp]))
    rows = dr.X[:nd, Fp:].cpu().numpy()
    e_rows = np.abs(rows - ref['rows']) / ((1 + np.abs(ref['rows'])) / VIS_STD[None, :])
    e_loss = np.abs(loss - ref['loss']) / np.maximum(np.abs(ref['loss']), 1e-300)
    e_loss[ref['loss'] == 0] = np.abs(loss[ref['loss'] == 0])
    e_d = np.abs(dmaps - ref['dmaps']) / ((1 + np.abs(ref['dmaps'])) * np.maximum(ref['sharers'], 1)[:, None])
    print(f'attach_vis: max rows err / bound unit {e_rows.max():.3g}, loss rel {e_loss.max():.3g}, dmaps err / bound unit '
          f'{e_d.max():.3g} (each must be <= 1e-5); {nd} rows, {int((ref["sharers"] > 1).sum())} shared pixels')
    assert (ref['loss'] > 0).any() and (ref['sharers'] > 0).any()
    assert e_rows.max() <= 1e-5 and e_loss.max() <= 1e-5 and e_d.max() <= 1e-5
    assert (dmaps[np.broadcast_to((ref['sharers'] == 0)[:, None], dmaps.shape)] == 0).all()
    # without the loss: the same rows, nothing to differentiate
    from trackmpnn_amd import VisHead
    mean, std = vis_stats('2d+temp+vis')
    dr2 = sampler.draw(idx, 4)
    assert dr2.attach_vis(VisHead((48, 160), 4, mean, std, DEV), torch.from_numpy(maps).to(DEV), loss=False) is None
    assert torch.equal(_bits(dr2.X[:nd]), _bits(dr.X[:nd]))


def test_rows_beyond_the_kept_total_change_nothing():
    sampler = _attach_case()[0]
    a, _, loss_a, dmaps_a, nd = _run_attach(junk_tail=False)
    b, before_b, loss_b, dmaps_b, _ = _run_attach(junk_tail=True)
    assert np.array_equal(loss_a.view(np.int32), loss_b.view(np.int32)) and np.array_equal(dmaps_a.view(np.int32), dmaps_b.view(np.int32))
    assert torch.equal(_bits(a.X[:nd]), _bits(b.X[:nd]))
    Fp = sampler.store.F - VIS_COLS
    assert torch.equal(_bits(b.X[:, :Fp]), _bits(before_b[:, :Fp]))


# ---- 4. launches and waits ---------------------------------------------------------------------------------------------------
def test_draw_plan_and_gather_never_wait_for_the_device():
    from trackmpnn_amd import ChunkSampler, FrameStore
    seqs, chunks = vis_rule_cases()
    sampler = ChunkSampler(vis_store(seqs, '2d+temp+vis', DEV), chunks, seed=15)
    rng = np.random.default_rng(2)
    fs = FrameStore([rng.integers(0, 256, (q['num_frames'], 12, 40, 3), dtype=np.uint8) for q in seqs], IMG_MEAN, IMG_STD, DEV)
    idx = sampler.epoch_order(0)
    fs.gather(sampler.draw(idx, 0).plan)                                    # warm: code objects, caching allocators
    torch.cuda.synchronize()
    keep = []

    def go():
        for s in range(3):
            dr = sampler.draw(idx[:5 + 4 * s], s)
            keep.append((dr, fs.gather(sampler.frame_plan(idx[:5 + 4 * s], s)), fs.gather(dr.plan)))

    assert _sync_warnings(go) == []
    assert len(_sync_warnings(lambda: int(keep[0][0].offsets[-1]))) >= 1    # (the detector works)
    assert torch.equal(keep[0][1], keep[0][2])


# ---- 5. train_epoch ----------------------------------------------------------------------------------------------------------
class _CountingNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, VIS_COLS, 3, padding=1)
        self.calls = 0

    def forward(self, x):
        self.calls += 1
        return self.conv(x)


def _vis_training_set():
    from trackmpnn_amd import ChunkSampler, FrameStore, make_chunks
    seqs = with_height(synth_sequences(seed=21, lengths=(12, 9, 1, 14)))
    chunks = make_chunks([s['num_frames'] for s in seqs], 5, 3, rng=random.Random(22))
    sampler = ChunkSampler(vis_store(seqs, '2d+vis', DEV), chunks, seed=23)
    rng = np.random.default_rng(4)
    H, W = 12, 40
    fs = FrameStore([rng.integers(0, 256, (q['num_frames'], H, W, 3), dtype=np.uint8) for q in seqs], IMG_MEAN, IMG_STD, DEV)
    return sampler, fs, (H, W)


def _fresh(input_hw):
    from trackmpnn_amd import BucketAdam, TrackMPNN, VisHead
    from trackmpnn_amd.dist import GradBucket
    torch.manual_seed(9)
    model = TrackMPNN('2d+vis', NCAT, 32, 0, 'diff')
    gp = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for k, prm in model.named_parameters():
            prm.add_(0.1 * torch.randn(prm.shape, generator=gp))
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=gp))
    model = model.to(DEV).train()
    torch.manual_seed(3)
    net = _CountingNet().to(DEV)
    bucket = GradBucket(model)
    opt = BucketAdam(model, bucket, lr=1e-3, weight_decay=0)
    net_opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    mean, std = vis_stats('2d+vis')
    head = VisHead(input_hw, 1, mean, std, DEV)
    return model, net, opt, net_opt, head


def _state(model, net):
    return ([p.detach().clone() for p in model.parameters()] + [b.detach().clone() for b in model.buffers()],
            [p.detach().clone() for p in net.parameters()])


def test_train_epoch_with_vis_equals_the_composition(monkeypatch):
    """train_epoch(batch_size=1, vis=...) against the steps written out: draw, batch, gather, CNN, head.forward into X,
    zero_grad twice, the tracker's chunk step (train_chunks on the one-chunk batch: the same launches train_epoch issues, so
    the comparison is bit for bit), the identity loss's backward, two steps.  Every parameter and buffer of the tracker and
    every parameter of the CNN equal bit for bit; two runs of train_epoch equal each other; the slices whose one chunk is
    skipped take no step and call the CNN zero times."""
    from trackmpnn_amd import AllChunksSkipped, VisTraining
    from trackmpnn_amd.loops import train_chunks, train_epoch
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    sampler, fs, hw = _vis_training_set()
    epoch = 2
    order = sampler.epoch_order(epoch)
    Fp = sampler.store.F - VIS_COLS

    # the composition
    model, net, opt, net_opt, head = _fresh(hw)
    k = 0
    for ci in order:
        drawn = sampler.draw([ci], epoch)
        try:
            batch = drawn.batch()
        except AllChunksSkipped:
            continue
        maps = net(fs.gather(drawn.plan))
        rows, loss_d = head.forward(maps, drawn.box, drawn.map_of, drawn.im_hw, drawn.track, drawn.offsets, out=drawn.X, col=Fp)
        assert rows is drawn.X and not rows.requires_grad
        net_opt.zero_grad()
        opt.zero_grad()
        train_chunks(model, batch, drawn.features(batch), True)
        loss_d.sum().backward()
        net_opt.step()
        opt.step()
        k += 1
    want = _state(model, net)
    assert 5 <= k < len(order) and net.calls == k                           # several steps, and chunks the reference skips
    p0 = _state(*_fresh(hw)[:2])
    assert not all(torch.equal(a, b) for a, b in zip(want[1], p0[1])) and not all(torch.equal(a, b) for a, b in zip(want[0], p0[0]))

    # train_epoch, twice
    for run in range(2):
        model2, net2, opt2, net_opt2, head2 = _fresh(hw)
        steps = train_epoch(model2, sampler, opt2, 1, epoch, vis=VisTraining(head2, fs, net2, net_opt2))
        assert steps == k and net2.calls == k
        got = _state(model2, net2)
        for a, b in zip(got[0] + got[1], want[0] + want[1]):
            assert torch.equal(_bits(a.float()), _bits(b.float())), run
    # a vis store without vis= is refused before anything is drawn
    with pytest.raises(ValueError, match='vis=VisTraining'):
        train_epoch(model2, sampler, opt2, 1, epoch)


def test_a_slice_of_skipped_chunks_runs_no_cnn():
    from trackmpnn_amd import ChunkSampler, VisTraining
    from trackmpnn_amd.loops import train_epoch
    sampler, fs, hw = _vis_training_set()
    skipping = ChunkSampler(sampler.store, [(2, [0]), (0, [3]), (1, [8])], seed=1)          # one timestep each: the reference skips them
    model, net, opt, net_opt, head = _fresh(hw)
    before = _state(model, net)
    assert train_epoch(model, skipping, opt, 2, 0, vis=VisTraining(head, fs, net, net_opt)) == 0
    assert net.calls == 0
    after = _state(model, net)
    assert all(torch.equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1]))
