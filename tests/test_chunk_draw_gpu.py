"""The device draw of augmented training chunks on the MI355X (-m gpu): ChunkSampler.draw against draw_chunks_host bit for bit,
the batch built from a draw (padded labels), the draw's launch / wait budget, and train_epoch against the pieces it composes.
The rules themselves (draw_chunks_host against the reference's arithmetic) are checked without a GPU in test_chunk_draw.py."""
import random

import numpy as np
import pytest
import torch

from tests.test_chunk_draw import FR_RANGE, KITTI_MEAN, KITTI_STD, NCAT, _rule_cases, synth_sequences
from tests.test_optim_gpu import _sync_warnings
from tests.test_train_batch_gpu import _perturbed_model
from tests.test_train_build_gpu import assert_same_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _store(seqs, feats, device=DEV):
    from trackmpnn_amd import DetectionStore
    return DetectionStore(seqs, NCAT, feats, KITTI_MEAN[feats], KITTI_STD[feats], fr_range=FR_RANGE, device=device)


def _assert_device_equals_host(sampler, idx, step):
    dr = sampler.draw(idx, step)
    hd = sampler.draw_host(idx, step)
    nd = int(hd.offsets[-1])
    assert dr.n_max == hd.n_max and tuple(dr.X.shape) == (hd.n_max, sampler.store.F) and tuple(dr.y.shape) == (hd.n_max, 2)
    assert (dr.X.dtype, dr.y.dtype, dr.offsets.dtype, dr.flags.dtype) == (torch.float32, torch.int64, torch.int64, torch.uint8)
    assert torch.equal(dr.offsets.cpu(), torch.from_numpy(hd.offsets))
    assert torch.equal(dr.flags.cpu(), torch.from_numpy(hd.flags))
    assert torch.equal(dr.y[:nd].cpu(), torch.from_numpy(hd.y))
    assert torch.equal(dr.X[:nd].cpu().view(torch.int32), torch.from_numpy(hd.X).view(torch.int32))      # bits, not values
    return dr, hd


def _c2_set(n, seed):
    """n sequences shaped like the C2 training chunks (synth_window: 7 frames, about 6 detections each) with random boxes,
    one chunk per sequence."""
    from trackmpnn_amd import synth_window
    rng = np.random.RandomState(seed)
    seqs = []
    for s in range(n):
        y = synth_window(1000 + s, 7, 6.0, 20)
        m = y.shape[0]
        x1, y1 = np.round(rng.uniform(0, 1080, m), 2), np.round(rng.uniform(100, 250, m), 2)
        box = np.stack([x1, y1, x1 + np.round(rng.uniform(5, 150, m), 2), y1 + np.round(rng.uniform(5, 120, m), 2)], 1)
        seqs.append(dict(frame=y[:, 0], track=y[:, 1], cat=rng.randint(1, NCAT + 1, m), box=box,
                         score=np.round(rng.uniform(0.3, 1, m), 4), width=1242, num_frames=int(y[:, 0].max()) + 1))
    return seqs, [(s, list(range(q['num_frames']))) for s, q in enumerate(seqs)]


# ---- 1. device draw == host definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('feats', ['2d', '2d+temp'])
def test_mixed_sequences(feats):
    from trackmpnn_amd import ChunkSampler
    seqs, chunks = _rule_cases()                       # several widths, false positives, empty frames, a one-frame sequence
    sampler = ChunkSampler(_store(seqs, feats), chunks, seed=2024)
    rng = np.random.RandomState(1)
    flags = []
    for step in (0, 1, 7, 2 ** 40 + 3):
        idx = rng.randint(0, len(chunks), 3 * len(chunks))                   # (repeats and any order)
        _, hd = _assert_device_equals_host(sampler, idx, step)
        flags.append(hd.flags)
        assert not hd.kept.all()
    assert set(np.concatenate(flags)) == {0, 1, 2, 3}
    _assert_device_equals_host(sampler, [5], 0)
    plain = ChunkSampler(sampler.store, chunks, seed=2024, random_transforms=False)
    _, hd = _assert_device_equals_host(plain, np.arange(len(chunks)), 9)
    assert hd.kept.all() and not hd.flags.any()
    other = ChunkSampler(sampler.store, chunks, seed=7, dropout=0.5, p_reverse=1.0, p_flip=0.0)
    _, hd = _assert_device_equals_host(other, np.arange(len(chunks)), 9)
    assert (hd.flags == 1).all()


@pytest.mark.parametrize('feats', ['2d', '2d+temp'])
def test_c2_sized_set(feats):
    from trackmpnn_amd import ChunkSampler
    seqs, chunks = _c2_set(1024, seed=2)
    sampler = ChunkSampler(_store(seqs, feats), chunks, seed=11)
    for epoch in (0, 1):
        dr, hd = _assert_device_equals_host(sampler, sampler.epoch_order(epoch), epoch)
        assert dr.offsets.numel() == 1025 and 0.7 * hd.n_max < hd.offsets[-1] < 0.9 * hd.n_max


@pytest.mark.parametrize('feats', ['2d', '2d+temp'])
def test_a_chunk_at_the_limit(feats):
    from trackmpnn_amd import ChunkSampler
    from trackmpnn_amd.train_batch import TB_MAX_DETS
    rng = np.random.RandomState(3)
    n, T = TB_MAX_DETS, 64
    x1 = rng.uniform(0, 1000, n)
    big = dict(frame=np.repeat(np.arange(T), n // T), track=rng.randint(-1, 80, n), cat=rng.randint(1, NCAT + 1, n),
               box=np.stack([x1, x1 * 0 + 150.5, x1 + rng.uniform(5, 150, n), x1 * 0 + 200.25], 1), score=rng.uniform(0, 1, n),
               width=1242, num_frames=T)
    small = synth_sequences(seed=5, lengths=(9,))[0]
    chunks = [(1, [0, 1, 2, 3, 4]), (0, list(range(T))), (1, [4, 5, 6, 7, 8]), (0, list(range(T)))]
    sampler = ChunkSampler(_store([big, small], feats), chunks, seed=12)
    assert sampler.size[1] == TB_MAX_DETS
    for step in (0, 1):
        _assert_device_equals_host(sampler, [0, 1, 2, 3], step)


def test_a_draw_of_nothing():
    from trackmpnn_amd import ChunkSampler
    z = np.zeros(0, np.int64)
    empty = dict(frame=z, track=z, cat=z, box=np.zeros((0, 4)), score=np.zeros(0), width=1242, num_frames=4)
    sampler = ChunkSampler(_store([empty, synth_sequences(seed=5, lengths=(9,))[0]], '2d+temp'), [(0, [0, 1, 2, 3]), (1, [0, 1, 2])],
                           seed=3)
    dr, _ = _assert_device_equals_host(sampler, [0], 0)
    assert dr.n_max == 0 and dr.offsets.tolist() == [0, 0]
    from trackmpnn_amd import AllChunksSkipped
    with pytest.raises(AllChunksSkipped, match='every chunk is skipped'):
        dr.batch()
    _assert_device_equals_host(sampler, [0, 1, 0], 0)


# ---- 2. the batch of a draw --------------------------------------------------------------------------------------------------
def test_batch_of_a_draw_and_padded_labels():
    from trackmpnn_amd import ChunkSampler, build_train_batch, build_train_batch_device, make_chunks
    seqs = synth_sequences(seed=6, lengths=(40, 57, 3, 25))
    chunks = make_chunks([s['num_frames'] for s in seqs], 5, 3, rng=random.Random(4))
    sampler = ChunkSampler(_store(seqs, '2d'), chunks, seed=13)
    idx = sampler.epoch_order(0)
    dr = sampler.draw(idx, 0)
    off = dr.offsets.cpu().numpy()
    nd = int(off[-1])
    assert 0 < nd < dr.n_max
    batch = dr.batch()
    exact = build_train_batch_device(dr.y[:nd].clone(), DEV, offsets=dr.offsets)
    assert_same_batch(batch, exact)
    yh = dr.y[:nd].cpu().numpy()
    assert_same_batch(batch, build_train_batch([yh[off[i]:off[i + 1]] for i in range(len(idx))], DEV))
    assert batch.n_feat == nd and tuple(dr.features(batch).shape) == (nd, 8) and len(batch.skipped) >= 1
    assert dr.features(batch).data_ptr() == dr.X.data_ptr()
    # trailing garbage rows (random, NaN-free) are ignored with padded=True and refused without it
    gen = torch.Generator().manual_seed(14)
    junk = torch.randint(-2 ** 40, 2 ** 40, (517, 2), generator=gen).to(DEV)
    y_pad = torch.cat([dr.y[:nd], junk])
    assert_same_batch(build_train_batch_device(y_pad, DEV, offsets=dr.offsets, padded=True), exact)
    assert_same_batch(build_train_batch_device(y_pad.double(), DEV, offsets=off, padded=True), exact)
    with pytest.raises(ValueError, match='offsets must run from 0 to ND'):
        build_train_batch_device(y_pad, DEV, offsets=dr.offsets)
    with pytest.raises(ValueError, match='offsets must run from 0 to ND'):
        build_train_batch_device(y_pad, DEV, offsets=dr.offsets, padded=False)
    with pytest.raises(ValueError, match='offsets do not ascend within'):
        build_train_batch_device(dr.y[:nd - 1].clone(), DEV, offsets=dr.offsets, padded=True)      # (too few rows: refused)


def test_a_chunk_the_kernels_refuse_does_not_train_as_an_empty_one():
    """The kernels check every table entry they index by; a chunk that fails is drawn empty with bit 7 of its flag set.  The host
    validates the tables, so this takes an overwritten device copy: here the chunk table claims one detection fewer than the
    chunk's frames hold.  batch() reads the flags' maximum along with the build's first read and raises."""
    from trackmpnn_amd import ChunkSampler, build_train_batch_device
    seqs, chunks = _rule_cases()
    sampler = ChunkSampler(_store(seqs, '2d+temp'), chunks, seed=5)
    big = int(np.argmax(sampler.size))
    others = [i for i in np.argsort(-sampler.size)[1:3]]
    sampler.table_d.view(len(chunks), 4 + sampler.L)[big, 2] -= 1
    dr = sampler.draw([others[0], big, others[1]], 0)
    flags, off = dr.flags.cpu().numpy(), dr.offsets.cpu().numpy()
    assert flags[1] == 128 and not (flags[[0, 2]] & 128).any()
    assert off[1] == off[2] and off[0] < off[1] and off[2] < off[3]
    with pytest.raises(RuntimeError, match='refused a chunk'):
        dr.batch()
    with pytest.raises(ValueError, match='draw_flags'):
        build_train_batch_device(dr.y, DEV, offsets=dr.offsets, padded=True, draw_flags=dr.flags[:2])
    sampler.table_d.view(len(chunks), 4 + sampler.L)[big, 2] += 1
    dr = sampler.draw([others[0], big, others[1]], 0)
    assert len(_sync_warnings(lambda: dr.batch())) == 2                     # (the flags ride along: still the build's two reads)


# ---- 3. launches and waits ---------------------------------------------------------------------------------------------------
def test_a_draw_never_waits_for_the_device():
    from trackmpnn_amd import ChunkSampler
    seqs, chunks = _c2_set(256, seed=7)
    sampler = ChunkSampler(_store(seqs, '2d+temp'), chunks, seed=15)
    idx = sampler.epoch_order(0)
    sampler.draw(idx, 0).batch()                                            # warm: code objects, caching allocators
    torch.cuda.synchronize()
    keep = []
    assert _sync_warnings(lambda: keep.extend(sampler.draw(idx[:100 + 50 * s], s) for s in range(3))) == []
    assert len(_sync_warnings(lambda: sampler.draw(idx, 1).batch())) == 2   # draw + build: the build's two reads
    assert len(_sync_warnings(lambda: int(keep[0].offsets[-1]))) >= 1       # (the detector works)


# ---- 4. train_epoch ----------------------------------------------------------------------------------------------------------
class _RecordingOpt:
    """The optimizer handed to train_epoch, keeping a copy of every step's gradient bucket."""

    def __init__(self, opt, bucket):
        self.opt, self.bucket, self.grads = opt, bucket, []

    def zero_grad(self):
        self.opt.zero_grad()

    def step(self):
        self.grads.append(self.bucket.flat.detach().double().cpu())
        self.opt.step()


def _flat_params(bucket):
    return torch.cat([p.detach().reshape(-1) for p in bucket.params]).double().cpu()


def test_train_epoch_batch_of_one_equals_train_chunk_and_step(monkeypatch):
    """train_epoch(batch_size=1, no transforms) against train_chunk + opt.step() over the same chunks in the same order.

    Losses: 1e-4 relative per step, gradients: tau_t = 2e-4 max|g_t| per step (the tolerances of tests/test_train_batch_gpu.py
    for train_chunks against train_chunk).  Parameters after k steps, per element, from the gradient tolerance through Adam
    (weight_decay = 0, so the parameters enter the update through the gradients only):
      Adam moves an element by lr r_t, r_t = mh_t / (sqrt(vh_t) + eps), mh_t = sum_i a_i g_i, vh_t = sum_i b_i g_i^2 with
      weights a_i = (1 - b1) b1^(t-i) / (1 - b1^t) and b_i = (1 - b2) b2^(t-i) / (1 - b2^t), each summing to 1.
      (a) Cauchy-Schwarz: |r_t| <= C_t = (1 - b1) / sqrt(1 - b2) sqrt(sum_{j<t} (b1^2 / b2)^j) sqrt(1 - b2^t) / (1 - b1^t),
          so two runs never differ by more than 2 C_t in r_t, whatever their gradients.
      (b) Let the other run's gradients be g_i + d_i, |d_i| <= tau = max_t tau_t.  d r_t / d g_i = a_i / (sqrt(vh) + eps)
          - mh b_i g_i / (sqrt(vh) (sqrt(vh) + eps)^2), so |sum_i d_i d r_t / d g_i| <= tau (1 + |r_t|) / sqrt(vh)
          (sum a_i = 1; sum b_i |g_i| <= sqrt(vh)).  Along the segment between the two histories sqrt(vh) >= sqrt(vh_t) - tau
          (triangle inequality of the b-weighted norm) and |r_t| <= C_t, so by the mean value theorem
          |r_t' - r_t| <= tau (1 + C_t) / (sqrt(vh_t) - tau) wherever sqrt(vh_t) > tau.
      Hence |p' - p| <= lr sum_t min(2 C_t, tau (1 + C_t) / (sqrt(vh_t) - tau)) + k 2^-21 max(|p|, lr): the last term is the
      fp32 rounding of the k updates themselves (the kernel's update is within a few ulp of the exact one per step)."""
    from trackmpnn_amd import BucketAdam, ChunkSampler, loops, make_chunks
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.loops import train_chunk, train_epoch
    lr, b1, b2, epoch = 1e-3, 0.9, 0.999, 2
    seqs = synth_sequences(seed=21, lengths=(12, 9, 3, 14))
    chunks = make_chunks([s['num_frames'] for s in seqs], 5, 3, rng=random.Random(22))
    sampler = ChunkSampler(_store(seqs, '2d'), chunks, seed=23, random_transforms=False)
    order = sampler.epoch_order(epoch)

    # sequential: one chunk, one step
    model = _perturbed_model(seed=9)
    bucket = GradBucket(model)
    opt = BucketAdam(model, bucket, lr=lr, weight_decay=0)
    seq_loss, seq_grads = [], []
    for ci in order:
        hd = sampler.draw_host([ci], epoch)
        opt.zero_grad()
        r = train_chunk(model, torch.from_numpy(hd.X)[None], torch.from_numpy(hd.y)[None], DEV, True)
        if r is None:
            continue
        seq_loss.append(float(r[0].detach()))
        seq_grads.append(bucket.flat.detach().double().cpu())
        opt.step()
    p_seq = _flat_params(bucket)
    k = len(seq_loss)
    assert 5 <= k < len(order)                                             # several steps, and a chunk the reference skips

    # train_epoch
    model2 = _perturbed_model(seed=9)
    bucket2 = GradBucket(model2)
    p0 = _flat_params(bucket2)
    rec = _RecordingOpt(BucketAdam(model2, bucket2, lr=lr, weight_decay=0), bucket2)
    ep_loss = []
    orig = loops.train_chunks

    def recording(*a, **kw):
        out = orig(*a, **kw)
        ep_loss.append(float(out[0].detach()))
        return out

    monkeypatch.setattr(loops, 'train_chunks', recording)
    assert train_epoch(model2, sampler, rec, 1, epoch) == k
    monkeypatch.setattr(loops, 'train_chunks', orig)
    p_ep = _flat_params(bucket2)

    assert len(ep_loss) == k
    tau = 0.0
    for t in range(k):
        print(f'step {t}: loss {ep_loss[t]:.6f} / {seq_loss[t]:.6f}, max |dg| {float((rec.grads[t] - seq_grads[t]).abs().max()):.3e}'
              f' of max |g| {float(seq_grads[t].abs().max()):.3e}')
        assert abs(ep_loss[t] - seq_loss[t]) <= 1e-4 * abs(seq_loss[t]), t
        tau_t = 2e-4 * float(seq_grads[t].abs().max())
        assert float((rec.grads[t] - seq_grads[t]).abs().max()) <= tau_t, t
        tau = max(tau, tau_t)
    bound = torch.zeros_like(p_seq)
    vh = torch.zeros_like(p_seq)
    for t in range(1, k + 1):
        vh = b2 * vh + (1 - b2) * seq_grads[t - 1] ** 2
        root = (vh / (1 - b2 ** t)).sqrt()
        C = ((1 - b1) / np.sqrt(1 - b2) * np.sqrt(sum((b1 * b1 / b2) ** j for j in range(t))) * np.sqrt(1 - b2 ** t)
             / (1 - b1 ** t))
        smooth = torch.where(root > tau, tau * (1 + C) / (root - tau).clamp_min(1e-300), torch.full_like(root, np.inf))
        bound += lr * torch.minimum(smooth, torch.full_like(root, 2 * C))
    bound += k * 2.0 ** -21 * torch.maximum(p_seq.abs(), torch.full_like(p_seq, lr))
    err = (p_ep - p_seq).abs()
    moved = (p_seq - p0).abs()
    print(f'{k} steps: max |dp| {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, median bound '
          f'{float(bound.median()):.3e}, max moved {float(moved.max()):.3e}, worst err / bound {float((err / bound).max()):.3e}')
    assert float(moved.max()) > 2 * lr                                      # (the runs are not no-ops)
    assert bool((err <= bound).all()), float((err / bound).max())


def test_train_epoch_with_transforms_is_repeatable():
    from trackmpnn_amd import BucketAdam, ChunkSampler, TrainMonitor
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.loops import train_epoch
    seqs, chunks = _c2_set(160, seed=31)
    runs = []
    for _ in range(2):
        sampler = ChunkSampler(_store(seqs, '2d'), chunks, seed=32)
        model = _perturbed_model(seed=9)
        bucket = GradBucket(model)
        opt = BucketAdam(model, bucket, lr=1e-3, weight_decay=5e-4)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.2)
        mon = TrainMonitor(DEV)
        steps = [train_epoch(model, sampler, opt, 64, e, monitor=mon, scheduler=sched) for e in (0, 1)]
        assert steps == [3, 3]                                             # 160 chunks in slices of 64, 64, 32
        assert opt.param_groups[0]['lr'] == pytest.approx(1e-3 * 0.2 ** 2)
        runs.append((_flat_params(bucket), {k: b.detach().clone() for k, b in model.named_buffers()}))
    assert torch.equal(runs[0][0], runs[1][0]) and bool(torch.isfinite(runs[0][0]).all())
    for k, b in runs[0][1].items():
        assert torch.equal(b, runs[1][1][k]), k
    p0 = _flat_params(GradBucket(_perturbed_model(seed=9)))
    assert not torch.equal(runs[0][0], p0)


# ---- 5. refusals before any launch -------------------------------------------------------------------------------------------
def test_malformed_inputs_raise_before_any_launch():
    from trackmpnn_amd import ChunkSampler, DetectionStore
    seqs, chunks = _rule_cases()
    m, s = KITTI_MEAN['2d'], KITTI_STD['2d']
    with pytest.raises(ValueError, match='vis'):
        DetectionStore(seqs, NCAT, '2d+vis', m, s, device=DEV)
    with pytest.raises(ValueError, match='mean / std of length'):
        DetectionStore(seqs, NCAT, '2d', m[:-1], s, device=DEV)
    with pytest.raises(ValueError, match='mean / std of length'):
        DetectionStore(seqs, NCAT, '2d+temp', KITTI_MEAN['2d+temp'], s, device=DEV)
    bad = [dict(q) for q in seqs]
    bad[4]['cat'] = np.zeros_like(bad[4]['cat'])
    with pytest.raises(ValueError, match='cat outside'):
        DetectionStore(bad, NCAT, '2d', m, s, device=DEV)
    store = _store(seqs, '2d')
    with pytest.raises(ValueError, match='num_frames'):
        ChunkSampler(store, chunks + [(2, [9, 10, 11])], seed=0)           # sequence 2 has eleven frames
    sampler = ChunkSampler(store, chunks, seed=0)
    torch.cuda.synchronize()
    for bad_idx, exc in (([0, len(chunks)], IndexError), ([-1], IndexError), ([], ValueError), ([0.5], ValueError)):
        with pytest.raises(exc):
            assert _sync_warnings(lambda: sampler.draw(bad_idx, 0)) == []
    with pytest.raises(ValueError, match='step'):
        sampler.draw([0], -1)
    dr = sampler.draw([0, 1], 0)
    assert not bool((dr.flags & 128).any())
