"""Training chunks drawn with the visual feature group, host side (no GPU): what a 'vis' DetectionStore adds to a draw (the
box the features were made from, the image size, the image every row needs: ChunkSampler.frame_plan), the value table of
FrameStore and frames_host, the host attach of the visual head, and the refusals.  tests/test_chunk_vis_gpu.py holds the
device to these definitions."""
import random

import numpy as np
import pytest
import torch

from tests.test_chunk_draw import FR_RANGE, KITTI_MEAN, KITTI_STD, NCAT, _rule_cases, synth_sequences
from trackmpnn_amd.chunks import FLAG_FLIPPED, FLAG_REVERSED, ChunkSampler, DetectionStore, FramePlan, make_chunks
from trackmpnn_amd.frames import FrameStore
from trackmpnn_amd.vishead import VIS_COLS, vis_head_host

_rng = np.random.default_rng(77)
VIS_MEAN = (0.02 * _rng.random(VIS_COLS)).astype(np.float32)
VIS_STD = (0.3 + 1.7 * _rng.random(VIS_COLS)).astype(np.float32)
HEIGHTS = (375, 370, 374, 376)
IMG_MEAN, IMG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)             # the ImageNet values the reference normalises with


def plain_feats(feats):
    return feats.replace('+vis', '')


def vis_stats(feats):
    base = plain_feats(feats)
    return (np.concatenate([np.asarray(KITTI_MEAN[base], np.float32), VIS_MEAN]),
            np.concatenate([np.asarray(KITTI_STD[base], np.float32), VIS_STD]))


def with_height(seqs):
    return [dict(q, height=HEIGHTS[i % len(HEIGHTS)]) for i, q in enumerate(seqs)]


def vis_store(seqs, feats, device=None):
    m, s = vis_stats(feats)
    return DetectionStore(seqs, NCAT, feats, m, s, fr_range=FR_RANGE, device=device)


def plain_store(seqs, feats, device=None):
    base = plain_feats(feats)
    return DetectionStore(seqs, NCAT, base, KITTI_MEAN[base], KITTI_STD[base], fr_range=FR_RANGE, device=device)


def vis_rule_cases():
    seqs, chunks = _rule_cases()
    return with_height(seqs), chunks


def assert_vis_fields_follow_the_rules(hd, seqs, chunks, indices):
    """box, im_hw, map_of, track and the plan of a HostDraw, restated from the indices: per chunk the detections of its listed
    frames in list order, those that `kept` marks; the box mirrored in float64 and then narrowed iff the chunk is flipped; the
    image of a row is (sequence, LISTED frame, flip decision) whatever time reversal does to t'."""
    pos = 0
    first_use = {}
    for b, ci in enumerate(indices):
        s, frames = chunks[ci]
        q = seqs[s]
        fr_of = np.asarray(q['frame'])
        visited = np.concatenate([np.flatnonzero(fr_of == f) for f in frames] + [np.zeros(0, np.int64)]).astype(np.int64)
        list_pos = np.concatenate([np.full(int((fr_of == f).sum()), k) for k, f in enumerate(frames)] + [np.zeros(0, np.int64)])
        keep = hd.kept[pos:pos + visited.size]
        pos += visited.size
        pick, k_of = visited[keep], list_pos[keep].astype(np.int64)
        flip = int(bool(hd.flags[b] & FLAG_FLIPPED))
        box = np.asarray(q['box'], np.float64)[pick].copy()
        if flip:
            box[:, 0], box[:, 2] = q['width'] - box[:, 2] - 1, q['width'] - box[:, 0].copy() - 1
        o0, o1 = hd.offsets[b], hd.offsets[b + 1]
        assert o1 - o0 == pick.size
        assert hd.box.dtype == np.float32 and np.array_equal(hd.box[o0:o1].view(np.uint32), box.astype(np.float32).view(np.uint32))
        assert np.array_equal(hd.im_hw[o0:o1], np.tile(np.asarray([[q['height'], q['width']]], np.float32), (pick.size, 1)))
        assert hd.track.dtype == np.int32 and np.array_equal(hd.track[o0:o1], np.asarray(q['track'])[pick])
        assert np.array_equal(hd.track[o0:o1], hd.y[o0:o1, 1])
        want = np.stack([np.full(pick.size, s), np.asarray(frames, np.int64)[k_of], np.full(pick.size, flip)], 1).reshape(-1, 3)
        assert hd.map_of.dtype == np.int32 and np.array_equal(hd.plan.frames[hd.map_of[o0:o1]], want)
        assert np.array_equal(hd.map_of[o0:o1], hd.plan.slot[b, k_of])
        # the plan: one row per (sequence, listed frame, flip), whether or not a detection of that frame was kept
        for k, f in enumerate(frames):
            first_use.setdefault((s, f, flip), len(first_use))
            assert hd.plan.slot[b, k] == first_use[(s, f, flip)]
        assert (hd.plan.slot[b, len(frames):] == -1).all()
    assert pos == hd.n_max
    assert [tuple(r) for r in hd.plan.frames] == sorted(first_use, key=first_use.get)
    assert hd.plan.frames.dtype == np.int64 and hd.plan.slot.dtype == np.int32


# ---- 1. the rules ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feats', ['2d+vis', '2d+temp+vis'])
def test_a_vis_draw_follows_the_rules_and_leaves_the_rest_alone(feats):
    seqs, chunks = vis_rule_cases()
    store, plain = vis_store(seqs, feats), plain_store(seqs, feats)
    assert store.vis and not plain.vis and store.F == plain.F + VIS_COLS
    assert store.box.shape == (store.ndets, 2, 4) and store.box.dtype == np.float32
    assert store.im_hw.shape == (len(seqs), 2) and store.im_hw.dtype == np.float32
    sv, sp = ChunkSampler(store, chunks, seed=2024), ChunkSampler(plain, chunks, seed=2024)
    idx = np.arange(len(chunks))
    seen = dict(reversed_and_flipped=False, flipped=False, plain=False)
    for step in range(40):
        hd, hp = sv.draw_host(idx, step), sp.draw_host(idx, step)
        assert_vis_fields_follow_the_rules(hd, seqs, chunks, idx)
        Fp = plain.F
        assert hd.X.shape == (hp.X.shape[0], Fp + VIS_COLS)
        assert np.array_equal(hd.X[:, :Fp].view(np.uint32), hp.X.view(np.uint32))             # bits
        assert np.array_equal(hd.y, hp.y) and np.array_equal(hd.offsets, hp.offsets)
        assert np.array_equal(hd.flags, hp.flags) and np.array_equal(hd.kept, hp.kept) and hd.n_max == hp.n_max
        assert hp.box is None and hp.plan is None and hp.map_of is None and hp.im_hw is None and hp.track is None
        both = (hd.flags & (FLAG_REVERSED | FLAG_FLIPPED)) == (FLAG_REVERSED | FLAG_FLIPPED)
        nonempty = np.diff(hd.offsets) > 0
        seen['reversed_and_flipped'] |= bool((both & nonempty).any())
        seen['flipped'] |= bool(((hd.flags & FLAG_FLIPPED) != 0).any())
        seen['plain'] |= bool((hd.flags == 0).any())
    assert all(seen.values()), seen


def test_the_spellings_and_the_feature_width():
    seqs, _ = vis_rule_cases()
    m, s = vis_stats('2d+temp+vis')
    a = DetectionStore(seqs, NCAT, '2d-temp-vis', m, s, fr_range=FR_RANGE, device=None)
    assert a.vis and a.temp and a.F == NCAT + 5 + 2 + 128
    m, s = vis_stats('2d+vis')
    b = DetectionStore(seqs, NCAT, '2d-vis', m, s, fr_range=FR_RANGE, device=None)
    assert b.vis and not b.temp and b.F == NCAT + 5 + 128
    assert not plain_store(seqs, '2d+temp').vis


# ---- 2. the plan -------------------------------------------------------------------------------------------------------------
def test_the_plan_shares_a_frame_only_under_one_flip_decision():
    """Two overlapping chunks of one sequence (frames 0-4 and 2-6 and a skip pair): over the steps their flip decisions agree
    and differ; shared (frame, flip) pairs share a slot, differing flips do not; rows are in order of first use; -1 pads."""
    seqs = with_height(synth_sequences(seed=9, lengths=(12,)))
    chunks = [(0, [0, 1, 2, 3, 4]), (0, [2, 3, 4, 5, 6, 9, 10])]
    sampler = ChunkSampler(vis_store(seqs, '2d+temp+vis'), chunks, seed=5)
    seen = dict(same=False, differ=False, reversed_and_flipped=False)
    for step in range(40):
        plan = sampler.frame_plan([0, 1], step)
        hd = sampler.draw_host([0, 1], step)
        assert isinstance(plan, FramePlan) and np.array_equal(plan.frames, hd.plan.frames) and np.array_equal(plan.slot, hd.plan.slot)
        f0, f1 = (int(bool(f & FLAG_FLIPPED)) for f in hd.flags)
        assert plan.slot.shape == (2, 7) and plan.slot[0, :5].tolist() == [0, 1, 2, 3, 4] and (plan.slot[0, 5:] == -1).all()
        assert [tuple(r) for r in plan.frames[:5]] == [(0, f, f0) for f in range(5)]
        if f0 == f1:
            seen['same'] = True
            assert plan.slot[1].tolist() == [2, 3, 4, 5, 6, 7, 8] and plan.frames.shape == (9, 3)
            assert [tuple(r) for r in plan.frames[5:]] == [(0, f, f1) for f in (5, 6, 9, 10)]
        else:
            seen['differ'] = True
            assert plan.slot[1].tolist() == [5, 6, 7, 8, 9, 10, 11] and plan.frames.shape == (12, 3)
            assert [tuple(r) for r in plan.frames[5:]] == [(0, f, f1) for f in (2, 3, 4, 5, 6, 9, 10)]
        if hd.flags[1] == (FLAG_REVERSED | FLAG_FLIPPED) and hd.offsets[2] > hd.offsets[1]:
            seen['reversed_and_flipped'] = True
            # time reversal relabels t' only: the image of a row is still its LISTED frame
            o0, o1 = hd.offsets[1], hd.offsets[2]
            listed = plan.frames[hd.map_of[o0:o1], 1]
            assert np.array_equal(hd.y[o0:o1, 0], 10 - listed + 2) and (plan.frames[hd.map_of[o0:o1], 2] == 1).all()
    assert all(seen.values()), seen
    # the same chunk twice in a draw: one decision, every slot shared
    plan = sampler.frame_plan([1, 1], 3)
    assert np.array_equal(plan.slot[0], plan.slot[1]) and plan.frames.shape == (7, 3)
    # without transforms nothing is mirrored
    plain = ChunkSampler(sampler.store, chunks, seed=5, random_transforms=False)
    assert not plain.frame_plan([0, 1], 0).frames[:, 2].any() and plain.frame_plan([0, 1], 0).frames.shape == (9, 3)


# ---- 3. the frames -----------------------------------------------------------------------------------------------------------
def test_the_value_table_is_the_torch_statement():
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8)]
    fs = FrameStore(frames, IMG_MEAN, IMG_STD, device=None)
    assert fs.table.shape == (3, 256) and fs.table.dtype == np.float32
    v = torch.arange(256, dtype=torch.uint8)
    for c in range(3):
        want = v.float().div(255).sub(IMG_MEAN[c]).div(IMG_STD[c])
        assert want.dtype == torch.float32
        assert np.array_equal(fs.table[c].view(np.uint32), want.numpy().view(np.uint32))
    # ToTensor + Normalize on a whole frame, in torch, is the same selection
    img = torch.from_numpy(frames[0][1]).permute(2, 0, 1)
    want = img.float().div(255).sub(torch.tensor(IMG_MEAN)[:, None, None]).div(torch.tensor(IMG_STD)[:, None, None])
    got = fs.frames_host(np.asarray([[0, 1, 0]]))
    assert got.dtype == np.float32 and np.array_equal(got[0].view(np.uint32), want.numpy().view(np.uint32))


def test_frames_host_is_the_table_applied_plain_and_mirrored():
    # hand-built frames: pixel (y, x) of channel c of frame g holds a value that names its place
    H, W = 3, 5
    seq_a = np.zeros((2, H, W, 3), np.uint8)
    seq_b = np.zeros((1, H, W, 3), np.uint8)
    for g, fr in enumerate([seq_a[0], seq_a[1], seq_b[0]]):
        for c in range(3):
            fr[:, :, c] = 60 * g + 20 * c + 5 * np.arange(H)[:, None] + np.arange(W)[None, :]
    fs = FrameStore([seq_a, seq_b], IMG_MEAN, IMG_STD, device=None)
    assert fs.seq_base.tolist() == [0, 2, 3] and (fs.H, fs.W) == (H, W)
    plan = np.asarray([[1, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 1]])                # a repeat; one frame plain and mirrored
    out = fs.frames_host(plan)
    assert out.shape == (4, 3, H, W) and out.dtype == np.float32
    for i, (s, f, m) in enumerate(plan):
        g = (0, 2)[s] + f
        for c in range(3):
            for y in range(H):
                for x in range(W):
                    v = 60 * g + 20 * c + 5 * y + (W - 1 - x if m else x)
                    assert out[i, c, y, x] == fs.table[c, v]
    assert np.array_equal(out[0], out[3]) and np.array_equal(out[1], out[2][:, :, ::-1])
    assert fs.frames_host(np.zeros((0, 3), np.int64)).shape == (0, 3, H, W)
    assert np.array_equal(fs.frames_host(FramePlan(plan.astype(np.int64), np.zeros((1, 1), np.int32))), out)


# ---- 4. the composition ------------------------------------------------------------------------------------------------------
def test_a_host_attach_is_the_visual_head_on_the_drawn_boxes():
    seqs, chunks = vis_rule_cases()
    store = vis_store(seqs, '2d+temp+vis')
    sampler = ChunkSampler(store, chunks, seed=11)
    idx = np.arange(len(chunks))[::2]
    hd = sampler.draw_host(idx, 4)
    T = hd.plan.frames.shape[0]
    Hm, Wm, input_hw, down = 12, 40, (48, 160), 4
    maps = np.random.default_rng(5).standard_normal((T, VIS_COLS, Hm, Wm))
    before = hd.X.copy()
    assert not before[:, store.F - VIS_COLS:].any()
    mean, std = vis_stats('2d+temp+vis')
    loss = hd.attach_vis(maps, mean, std, input_hw, down)
    _, rows, want_loss, _ = vis_head_host(maps, hd.box, hd.map_of, hd.im_hw, hd.track, hd.offsets, VIS_MEAN, VIS_STD, input_hw, down)
    assert np.array_equal(hd.X[:, store.F - VIS_COLS:], rows.astype(np.float32)) and np.array_equal(loss, want_loss)
    assert np.array_equal(hd.X[:, :store.F - VIS_COLS], before[:, :store.F - VIS_COLS])
    assert loss.shape == (idx.size,) and (loss > 0).any() and np.isfinite(hd.X).all()


# ---- 5. refusals (host checks: nothing is launched) --------------------------------------------------------------------------
def test_malformed_inputs_raise():
    seqs, chunks = vis_rule_cases()
    m, s = vis_stats('2d+temp+vis')
    bad = [dict(q) for q in seqs]
    del bad[3]['height']
    with pytest.raises(ValueError, match='sequence 3.*height'):
        DetectionStore(bad, NCAT, '2d+temp+vis', m, s, device=None)
    with pytest.raises(ValueError, match='mean / std of length'):
        DetectionStore(seqs, NCAT, '2d+temp+vis', m[:-1], s[:-1], device=None)
    with pytest.raises(ValueError, match='mean / std of length'):
        DetectionStore(seqs, NCAT, '2d+vis', m, s, device=None)                       # (the 2d+temp+vis statistics: two too many)
    with pytest.raises(ValueError, match='feats'):
        DetectionStore(seqs, NCAT, 'vis', m, s, device=None)
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8), rng.integers(0, 256, (3, 4, 7, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match='one size'):
        FrameStore([a, b], IMG_MEAN, IMG_STD, device=None)
    with pytest.raises(ValueError, match='mean / std of length'):
        FrameStore([a], IMG_MEAN[:2], IMG_STD, device=None)
    with pytest.raises(ValueError, match='uint8'):
        FrameStore([a.astype(np.float32)], IMG_MEAN, IMG_STD, device=None)
    with pytest.raises(ValueError, match='uint8'):
        FrameStore([a[0]], IMG_MEAN, IMG_STD, device=None)                            # (one frame, not a sequence of frames)
    fs = FrameStore([a, a[:1]], IMG_MEAN, IMG_STD, device=None)
    for plan, what in (([[2, 0, 0]], 'sequence'), ([[1, 1, 0]], 'frame 1 of sequence 1'), ([[0, -1, 0]], 'frame'),
                       ([[0, 0, 2]], 'mirrored'), ([[0, 0]], r'\[T, 3\]')):
        with pytest.raises(ValueError, match=what):
            fs.frames_host(np.asarray(plan))
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        fs.gather(np.asarray([[0, 0, 0]]))                                            # a host-only store has no device gather
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        FrameStore([a], IMG_MEAN, IMG_STD, device='cpu')
    # train_epoch: a vis store without vis=, and vis= without a vis store -- before anything is drawn
    from trackmpnn_amd.loops import VisTraining, train_epoch
    sampler = ChunkSampler(vis_store(seqs, '2d+temp+vis'), chunks, seed=0)
    with pytest.raises(ValueError, match='vis=VisTraining'):
        train_epoch(None, sampler, None, 4, 0)
    plain = ChunkSampler(plain_store(seqs, '2d+temp'), chunks, seed=0)
    with pytest.raises(ValueError, match="without 'vis'"):
        train_epoch(None, plain, None, 4, 0, vis=VisTraining(None, None, None, None))
    with pytest.raises(ValueError, match="without 'vis'"):
        plain.draw_host([0], 0).attach_vis(np.zeros((1, VIS_COLS, 2, 2)), m, s, (8, 8), 4)


def test_entry_points_validate_on_the_host():
    import ctypes
    import os
    from trackmpnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.tmpnn_frames_gather(None, None) == -1 and b'call struct is null' in lib.tmpnn_last_error()
    a = _lib.CFramesGather(1, 4, 8193, 1, 1, None, None, None, None, None)
    assert lib.tmpnn_frames_gather(ctypes.byref(a), None) == -1 and b'W=8193' in lib.tmpnn_last_error()
    a.W = 8
    assert lib.tmpnn_frames_gather(ctypes.byref(a), None) == -1 and b'null pointer' in lib.tmpnn_last_error()
    a.T = 0
    assert lib.tmpnn_frames_gather(ctypes.byref(a), None) == 0                         # nothing to do: nothing is launched
    d = _lib.CChunkDraw()
    d.B, d.nchunks, d.nseq, d.L, d.F, d.Fs, d.fr_range, d.nframes = 1, 1, 1, 7, 10, 8, 30, 1
    v = _lib.CChunkDrawVis()
    assert lib.tmpnn_chunk_draw_vis(ctypes.byref(d), ctypes.byref(v), None) == -1 and b'null pointer' in lib.tmpnn_last_error()
    d.ldx = 9
    assert lib.tmpnn_chunk_draw_vis(ctypes.byref(d), ctypes.byref(v), None) == -1 and b'ldx=9' in lib.tmpnn_last_error()
    d.ldx = 138
    assert lib.tmpnn_chunk_draw_vis(ctypes.byref(d), None, None) == -1 and b'null pointer' in lib.tmpnn_last_error()
