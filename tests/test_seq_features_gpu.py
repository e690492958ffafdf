"""Whole-sequence features on the device (-m gpu; csrc/seqfeat.hip: tmpnn_seq_features; trackmpnn_amd.seqfeat.SequenceFeatures)
against the host definition: bit for bit in everything the build's launch writes (every value is selected, not computed), the
visual columns at the bound tests/test_vis_head_gpu.py holds VisHead.rows to against vis_head_host in float64:
|err| <= 1e-5 (1 + |value|) / std."""
import functools

import numpy as np
import pytest
import torch

from tests.seqfeat_cases import NCAT_KITTI, WIDTHS, feature_stats, synth_sequence, synth_store
from trackmpnn_amd.chunks import DetectionStore
from trackmpnn_amd.frames import FrameStore
from trackmpnn_amd.seqfeat import SequenceFeatures, listed_features_host, sequence_features_host, sequence_vis_host
from trackmpnn_amd.vishead import VIS_COLS, VisHead

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_build_equals_host(sf, sequences=None, frames_per_batch=8):
    """sf.build(sequences) against listed_features_host: shapes, dtypes, every bit the launch writes.  Returns the dicts."""
    st = sf.store
    out = sf.build(sequences, frames_per_batch)
    ref = listed_features_host(st, sequences)
    assert len(out) == len(ref)
    for k, (d, r) in enumerate(zip(out, ref)):
        n = r.X.shape[0]
        assert d['X'].dtype == torch.float32 and d['y'].dtype == torch.int64 and d['X'].device == st.device
        assert tuple(d['X'].shape) == (1, n, st.F) and tuple(d['y'].shape) == (1, n, 2)
        assert d['X'][0].is_contiguous() and d['y'][0].is_contiguous()
        assert np.array_equal(bits(d['X'][0, :, :st.Fv]), bits(r.X[:, :st.Fv])), f'listed sequence {k}: X differs'
        assert np.array_equal(d['y'][0].cpu().numpy(), r.y), f'listed sequence {k}: y differs'
        a, b = int(sf.offsets[k]), int(sf.offsets[k + 1])
        assert b - a == n
        if st.vis:
            assert np.array_equal(bits(sf.box[a:b]), bits(r.box)) and np.array_equal(bits(sf.im_hw[a:b]), bits(r.im_hw))
            assert sf.map_of.dtype == torch.int32 and np.array_equal(sf.map_of[a:b].cpu().numpy(), r.frame % frames_per_batch)
    assert int(sf.offsets[-1]) == sum(r.X.shape[0] for r in ref) == sf.X.shape[0]
    sf.check()
    return out


@pytest.mark.parametrize('ncat, feats', WIDTHS)
def test_every_row_width(ncat, feats):
    """F = 8, 10, 138, 13, 15, 143: rows that are not 16-byte aligned, sequences whose packed base falls at any row (the odd
    detection counts see to that), more than one workgroup of 256 rows."""
    store, _ = synth_store(11, (1, 3, 7, 40, 57, 33), ncat, feats, DEV, dets=(0, 5))
    assert store.F == {('2d', 3): 8, ('2d+temp', 3): 10, ('2d+temp+vis', 3): 138, ('2d', 8): 13, ('2d+temp', 8): 15,
                       ('2d+temp+vis', 8): 143}[(feats, ncat)]
    sf = SequenceFeatures(store)
    assert_build_equals_host(sf)
    assert sf.X.shape[0] > 256 and len({int(o) % 4 for o in sf.offsets}) > 1
    assert_build_equals_host(sf, [4, 0, 5, 2], frames_per_batch=3)          # a listed subset, not ascending


@pytest.mark.parametrize('nseq', [1, 3, 70])
def test_stores_of_one_three_and_seventy_sequences(nseq):
    rng = np.random.default_rng(nseq)
    lengths = [int(v) for v in rng.integers(1, 12, nseq)]
    empty = (0, nseq - 1) if nseq > 1 else ()                                # empty sequences first and last
    store, _ = synth_store(20 + nseq, lengths, NCAT_KITTI, '2d+temp+vis', DEV, dets=(0, 4), empty=empty)
    sf = SequenceFeatures(store)
    out = assert_build_equals_host(sf)
    if nseq > 1:
        assert tuple(out[0]['X'].shape) == (1, 0, 138) and tuple(out[-1]['y'].shape) == (1, 0, 2)
        order = [int(v) for v in rng.permutation(nseq)[:max(2, nseq // 2)]]
        assert_build_equals_host(sf, order)
        out = sf.build([0, nseq - 1])                                       # nothing to write: no launch, empty views
        assert sf.X.shape[0] == 0 and [tuple(d['X'].shape) for d in out] == [(1, 0, 138)] * 2
        sf.check()


def test_a_long_sequence_and_a_crowded_frame():
    """300 frames with 1 - 3 detections each (beyond a training chunk's 256 listed frames), and a frame with 65 detections."""
    rng = np.random.default_rng(8)
    mean, std = feature_stats(NCAT_KITTI, '2d+temp')
    long = synth_sequence(rng, 300, NCAT_KITTI, dets=(1, 3))
    crowd = synth_sequence(rng, 9, NCAT_KITTI, dets=lambda f: np.where(f == 4, 65, 2))
    store = DetectionStore([long, crowd], NCAT_KITTI, '2d+temp', mean, std, device=DEV)
    assert int(np.diff(store.first).max()) == 65
    sf = SequenceFeatures(store)
    out = assert_build_equals_host(sf)
    assert out[0]['y'][0, -1, 0].item() == 299 and out[0]['X'].shape[1] >= 300


def test_build_twice_gives_identical_bytes():
    store, _ = synth_store(31, (5, 40, 12), NCAT_KITTI, '2d+temp', DEV)
    sf = SequenceFeatures(store)
    sf.build()
    X1, y1 = sf.X.clone(), sf.y.clone()
    sf.X.fill_(float('nan'))
    sf2 = SequenceFeatures(store)
    sf2.build()
    sf.build()
    for X, y in ((sf.X, sf.y), (sf2.X, sf2.y)):
        assert torch.equal(X.view(torch.int32), X1.view(torch.int32)) and torch.equal(y, y1)


def test_malformed_lists_raise_before_any_launch():
    store, _ = synth_store(1, (4, 5, 6), NCAT_KITTI, '2d', DEV)
    sf = SequenceFeatures(store)
    with pytest.raises(IndexError, match='sequence 3 of 3'):
        sf.build([0, 3])
    with pytest.raises(ValueError, match='listed twice'):
        sf.build([1, 1])
    with pytest.raises(ValueError, match='frames_per_batch=0'):
        sf.build(frames_per_batch=0)
    with pytest.raises(ValueError, match="without 'vis'"):
        sf.attach_vis(None, None, None)


def test_a_row_the_kernel_refuses_raises_the_flag_and_is_not_written():
    """A device table overwritten behind the host's back (a frame outside the row's sequence): the kernel checks the entry
    before it indexes by it, so the row is skipped, the flag word reports it on the next host read, and the other rows are
    served."""
    store, _ = synth_store(2, (6, 9), NCAT_KITTI, '2d+temp', DEV, dets=(1, 3))
    sf = SequenceFeatures(store)
    good = sf.build()[0]['X'].clone()
    sf.check()
    sf.frame_d[1] = 5000
    out = sf.build()
    with pytest.raises(RuntimeError, match="a row's frame"):
        sf.check()
    X = out[0]['X'][0]
    assert torch.equal(X[0].view(torch.int32), good[0, 0].view(torch.int32)) and torch.equal(X[2:].view(torch.int32), good[0, 2:].view(torch.int32))


# ---- the visual pass ---------------------------------------------------------------------------------------------------------
INPUT_HW, RAW_HW, N_FRAMES = (24, 80), (12, 40), 10


class Counted(torch.nn.Module):
    """The embedding net with a count of its calls and of the images they held."""

    def __init__(self, net):
        super().__init__()
        self.net, self.calls, self.images = net, 0, 0

    def forward(self, x):
        self.calls += 1
        self.images += int(x.shape[0])
        assert not self.training and not torch.is_grad_enabled()
        return self.net(x)


@functools.lru_cache(maxsize=None)
def vis_case():
    """Two sequences of 10 frames of 12 x 40 pixels resized to the CNN's 24 x 80; sequence 0 has no detection in frames 3 - 5
    (an empty batch at frames_per_batch = 3) and 8 - 9; a fixed-seed conv as the embedding net.  The reference (computed once):
    sequence_vis_host in float64 on the device conv's own maps."""
    rng = np.random.default_rng(77)
    mean, std = feature_stats(NCAT_KITTI, '2d+temp+vis')
    mean[-VIS_COLS:] = (0.02 * rng.random(VIS_COLS)).astype(np.float32)
    std[-VIS_COLS:] = (0.3 + 1.7 * rng.random(VIS_COLS)).astype(np.float32)
    seqs = [synth_sequence(rng, N_FRAMES, NCAT_KITTI, dets=lambda f: np.where(((f >= 3) & (f <= 5)) | (f >= 8), 0, 3), im_hw=RAW_HW),
            synth_sequence(rng, N_FRAMES, NCAT_KITTI, dets=(1, 4), im_hw=RAW_HW)]
    store = DetectionStore(seqs, NCAT_KITTI, '2d+temp+vis', mean, std, device=DEV)
    raw = [rng.integers(0, 256, (N_FRAMES,) + RAW_HW + (3,), dtype=np.uint8) for _ in seqs]
    frames = FrameStore.from_raw(raw, INPUT_HW, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], DEV)
    torch.manual_seed(4)
    net = torch.nn.Conv2d(3, VIS_COLS, 3, padding=1).to(DEV)
    head = VisHead(INPUT_HW, 1, mean, std, DEV)
    embed = lambda images: net(torch.from_numpy(images).to(DEV)).double().cpu().numpy()
    ref = []
    with torch.no_grad():
        for s in range(2):
            sample = sequence_features_host(store, s)
            sample.X = sample.X.astype(np.float64)
            ref.append(sequence_vis_host(store, s, sample, frames, embed, mean, std, INPUT_HW, 1, frames_per_batch=8)[:, -VIS_COLS:])
    return store, frames, net, head, std[-VIS_COLS:], ref


@functools.lru_cache(maxsize=None)
def vis_run(fpb):
    store, frames, net, head, _, _ = vis_case()
    sf = SequenceFeatures(store)
    plain = [d['X'].clone() for d in sf.build(frames_per_batch=fpb)]
    counted = Counted(net).train()
    sf.attach_vis(head, frames, counted, frames_per_batch=fpb)
    sf.check()
    return sf, plain, counted


@pytest.mark.parametrize('fpb', [1, 3, 8])
def test_the_visual_pass(fpb):
    store, frames, net, head, std, ref = vis_case()
    sf, plain, counted = vis_run(fpb)
    assert counted.training                                                 # the mode is restored
    err = 0.0
    for k in range(2):
        a, b = int(sf.offsets[k]), int(sf.offsets[k + 1])
        X = sf.X[a:b].cpu().numpy()
        e = np.abs(X[:, -VIS_COLS:] - ref[k]) / ((1 + np.abs(ref[k])) / std[None, :])
        err = max(err, e.max(initial=0))
        assert np.array_equal(bits(X[:, :-VIS_COLS]), bits(plain[k][0, :, :-VIS_COLS]))         # the other columns: untouched
    print(f'frames_per_batch={fpb}: max rows err / bound unit {err:.3g} (<= 1e-5), {counted.calls} calls of the net on {counted.images} images')
    assert err <= 1e-5
    # batches with a detection, per sequence: sequence 0 has none in frames 3 - 5 and 8 - 9, sequence 1 in every frame
    have = [np.bincount(sequence_features_host(store, s).frame, minlength=N_FRAMES) > 0 for s in range(2)]
    batches = [(f0, min(f0 + fpb, N_FRAMES)) for f0 in range(0, N_FRAMES, fpb)]
    live = [[(f0, f1) for f0, f1 in batches if h[f0:f1].any()] for h in have]
    assert counted.calls == len(live[0]) + len(live[1]) and counted.images == sum(f1 - f0 for l in live for f0, f1 in l)
    assert len(live[0]) < len(batches) if fpb in (1, 3) else N_FRAMES % fpb                    # an empty batch, a short last one
    assert torch.equal(sf.X.view(torch.int32), vis_run(1)[0].X.view(torch.int32))               # the same bits at every batch size


def test_attach_vis_with_another_batch_size_than_the_build():
    store, frames, net, head, _, _ = vis_case()
    sf = SequenceFeatures(store)
    sf.build()                                                              # frames_per_batch = 8
    sf.attach_vis(head, frames, net, frames_per_batch=3)                    # map_of is made anew first
    assert np.array_equal(sf.map_of.cpu().numpy(), sf.y[:, 0].cpu().numpy() % 3)
    assert torch.equal(sf.X.view(torch.int32), vis_run(3)[0].X.view(torch.int32))
    with pytest.raises(ValueError, match='does not hold the frames'):
        sf.attach_vis(head, FrameStore([np.zeros((3, 24, 80, 3), np.uint8)], [0.5] * 3, [0.5] * 3, DEV), net)


# ---- the loops ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) if a is not None and b is not None else a is b


def small_model(features):
    from trackmpnn_amd import TrackMPNN
    torch.manual_seed(9)
    model = TrackMPNN(features, 3, 32, 0, 'diff').to(DEV)
    gp = torch.Generator().manual_seed(17)
    with torch.no_grad():                                                   # scores on both sides of 0.5
        for k, prm in model.named_parameters():
            prm.add_((0.1 * torch.randn(prm.shape, generator=gp)).to(DEV))
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_((0.5 * torch.randn(prm.shape, generator=gp)).to(DEV))
    return model


def test_validate_store_equals_validate_on_hand_built_dicts():
    from trackmpnn_amd import MotEvaluator, validate
    from trackmpnn_amd.loops import VisInference, infer_store, validate_store
    from trackmpnn_amd.moteval import synth_mot_sequence
    mot = [synth_mot_sequence(70 + i, 30, objects=4) for i in range(3)]
    mean, std = feature_stats(NCAT_KITTI, '2d')
    rng = np.random.default_rng(3)
    seqs = [dict(frame=q['det_frame'], track=q['tracks'], cat=rng.integers(1, 4, q['det_frame'].size), box=q['det_box'],
                 score=np.round(rng.uniform(0.3, 1, q['det_frame'].size), 2), width=1000, num_frames=30) for q in mot]
    assert all((np.diff(q['det_frame']) >= 0).all() for q in mot)            # (the store's order is the evaluator's)
    store = DetectionStore(seqs, NCAT_KITTI, '2d', mean, std, device=DEV)
    sf = SequenceFeatures(store)
    model = small_model('2d').train()
    ev = MotEvaluator(mot, DEV)
    out = validate_store(model, sf, ev, cur_win_size=3)
    assert model.training
    by_hand = [{'X': torch.from_numpy(r.X)[None], 'y': torch.from_numpy(r.y)[None]} for r in listed_features_host(store)]
    ref = validate(model, by_hand, ev, cur_win_size=3)
    assert ref['predictions'] > 0 and ref['matches'] > 0 and same(out, ref)
    # the two mismatch errors, as train_epoch raises them
    vstore, frames, net, head, _, _ = vis_case()
    with pytest.raises(ValueError, match="holds 'vis' features"):
        validate_store(model, SequenceFeatures(vstore), ev)
    with pytest.raises(ValueError, match="without 'vis' features"):
        validate_store(model, sf, ev, vis=VisInference(head, frames, net))
    with pytest.raises(ValueError, match="without 'vis' features"):
        infer_store(model, sf, None, vis=VisInference(head, frames, net))


def test_validate_store_with_the_visual_pass():
    """The 'vis' store through validate_store: what validate gives on the features build + attach_vis leave behind."""
    from trackmpnn_amd import MotEvaluator, validate
    from trackmpnn_amd.loops import VisInference, validate_store
    vstore, frames, net, head, _, _ = vis_case()
    model = small_model('2d-temp-vis').eval()
    mot = []
    for s in range(2):
        r = sequence_features_host(vstore, s)
        mot.append(dict(det_frame=r.frame, det_box=r.box, gt_frame=r.frame, gt_track=np.maximum(r.y[:, 1], 0) + np.arange(r.frame.size) * 1000,
                        gt_box=r.box))
    ev = MotEvaluator(mot, DEV)
    counted = Counted(net)
    sf = SequenceFeatures(vstore)
    out = validate_store(model, sf, ev, vis=VisInference(head, frames, counted, frames_per_batch=3), cur_win_size=3)
    assert counted.calls == vis_run(3)[2].calls and torch.equal(sf.X.view(torch.int32), vis_run(3)[0].X.view(torch.int32))
    sf3 = vis_run(3)[0]
    dicts = [{'X': sf3.X[int(a):int(b)][None], 'y': sf3.y[int(a):int(b)][None]} for a, b in zip(sf3.offsets[:-1], sf3.offsets[1:])]
    assert same(out, validate(model, dicts, ev, cur_win_size=3))
