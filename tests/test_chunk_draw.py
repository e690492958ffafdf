"""Training chunks drawn with the reference's random transforms, host side (no GPU): the Philox generator, make_chunks, the
rules of a draw (draw_chunks_host against the rules of dataset/kitti_mot.py's __getitem__ written out independently, from
their statement), the rates of the three decisions and how a draw is keyed.  tests/test_chunk_draw_gpu.py holds the device draw to draw_chunks_host."""
import random

import numpy as np
import pytest
import torch

from trackmpnn_amd.chunks import (FLAG_FLIPPED, FLAG_REVERSED, ChunkSampler, DetectionStore, draw_chunks_host, make_chunks,
                                  philox4x32)

# dataset/kitti_mot.py:155-177, detections == 'centertrack': three categories, [score, xc, yc, w, h], the temporal pair
NCAT = 3
KITTI_MEAN = {'2d': [0.5] * 3 + [0.78, 544.57, 171.58, 71.54, 61.50]}
KITTI_STD = {'2d': [0.5] * 3 + [0.14, 285.65, 13.94, 69.92, 47.39]}
KITTI_MEAN['2d+temp'] = KITTI_MEAN['2d'] + [0.0, 0.0]
KITTI_STD['2d+temp'] = KITTI_STD['2d'] + [1.0, 1.0]
FR_RANGE = 30


def synth_sequence(rng, num_frames, width, mean_dets=4.0, p_empty=0.15, p_fp=0.25, ntracks=16):
    """One sequence of random detections: some frames empty, some detections false positives (track -1), boxes with decimals
    that float32 cannot hold (as parsed from a detection file); a track appears at most once per frame."""
    n_f = np.minimum(rng.poisson(mean_dets, num_frames), ntracks)
    n_f[rng.rand(num_frames) < p_empty] = 0
    frame = np.repeat(np.arange(num_frames), n_f)
    track = np.concatenate([rng.permutation(ntracks)[:k] for k in n_f] + [np.zeros(0, np.int64)]).astype(np.int64)
    if frame.size and rng.rand() < 0.5:                                   # (files need not be sorted)
        order = rng.permutation(frame.size)
        frame, track = frame[order], track[order]
    n = frame.size
    x1 = np.round(rng.uniform(0, width - 160, n), 2)
    y1 = np.round(rng.uniform(100, 250, n), 2)
    box = np.stack([x1, y1, x1 + np.round(rng.uniform(5, 150, n), 2), y1 + np.round(rng.uniform(5, 120, n), 2)], 1)
    track[rng.rand(n) < p_fp] = -1
    return dict(frame=frame, track=track, cat=rng.randint(1, NCAT + 1, n), box=box, score=np.round(rng.uniform(0.3, 1, n), 4),
                width=width, num_frames=num_frames)


def synth_sequences(seed, lengths=(1, 3, 11, 12, 40, 57), widths=(1242, 1224, 1238, 1241), **kw):
    rng = np.random.RandomState(seed)
    return [synth_sequence(rng, nf, widths[i % len(widths)], **kw) for i, nf in enumerate(lengths)]


def rules_of_a_draw(seq, frames, time_reversed, flipped, keep, feats, fr_range=FR_RANGE):
    """The rules of a draw for one chunk, written out from their statement (module docstring of trackmpnn_amd.chunks), with the
    decisions given: `time_reversed`, `flipped`, and `keep` per detection of the chunk in visiting order (True = it stays).
    Index-based and independent of the store: nothing here is precomputed.  Returns (X float32 [n, F], y int64 [n, 2])."""
    f32 = np.float32
    frame_of = np.asarray(seq['frame'])
    # which detections, in which order: the listed frames one after the other, each frame's detections as they were loaded
    visited = np.concatenate([np.flatnonzero(frame_of == f) for f in frames] + [np.zeros(0, np.int64)]).astype(np.int64)
    assert visited.size == len(keep)
    pick = visited[np.asarray(keep, dtype=bool)]
    n = pick.size
    # time: mirrored about the two ends of the frame list (not about the detections' own extremes)
    t = frame_of[pick].astype(np.int64)
    if time_reversed:
        t = frames[0] + frames[-1] - t
    # box: mirrored in double precision on the raw coordinates, only then narrowed to single precision
    left, top, right, bottom = np.asarray(seq['box'], dtype=np.float64)[pick].T
    if flipped:
        left, right = seq['width'] - right - 1, seq['width'] - left - 1
    left, top, right, bottom = (v.astype(f32) for v in (left, top, right, bottom))
    # columns, every operation in single precision: category indicator, score, centre, size, (phase of t)
    X = np.zeros((n, NCAT + 5 + (2 if 'temp' in feats else 0)), f32)
    X[np.arange(n), np.asarray(seq['cat'])[pick] - 1] = 1
    X[:, NCAT] = np.asarray(seq['score'])[pick].astype(f32)
    X[:, NCAT + 1] = (left + right) / f32(2)
    X[:, NCAT + 2] = (top + bottom) / f32(2)
    X[:, NCAT + 3] = right - left
    X[:, NCAT + 4] = bottom - top
    if 'temp' in feats:
        angle = (t % fr_range).astype(f32) * f32(np.pi) / f32(fr_range)
        X[:, NCAT + 5] = np.sin(angle)
        X[:, NCAT + 6] = np.cos(angle)
    X = (X - np.asarray(KITTI_MEAN[feats], f32)) / np.asarray(KITTI_STD[feats], f32)
    assert X.dtype == f32
    return X, np.stack([t, np.asarray(seq['track'])[pick].astype(np.int64)], 1)


def host_store(seqs, feats):
    return DetectionStore(seqs, NCAT, feats, KITTI_MEAN[feats], KITTI_STD[feats], fr_range=FR_RANGE, device=None)


def assert_draw_follows_the_rules(hd, seqs, chunks, indices, feats):
    """Every chunk of the HostDraw equals rules_of_a_draw under the decisions read back from its flags and kept mask."""
    pos = 0
    for b, ci in enumerate(indices):
        s, frames = chunks[ci]
        n = int(sum((seqs[s]['frame'] == f).sum() for f in frames))
        keep = hd.kept[pos:pos + n]
        pos += n
        X, y = rules_of_a_draw(seqs[s], frames, bool(hd.flags[b] & FLAG_REVERSED), bool(hd.flags[b] & FLAG_FLIPPED), keep, feats)
        o0, o1 = hd.offsets[b], hd.offsets[b + 1]
        assert o1 - o0 == keep.sum() == X.shape[0], (b, ci)
        assert np.array_equal(hd.y[o0:o1], y), (b, ci)
        assert hd.X[o0:o1].dtype == np.float32 and np.array_equal(hd.X[o0:o1].view(np.uint32), X.view(np.uint32)), (b, ci)
    assert pos == hd.n_max == hd.kept.size and hd.offsets[-1] == hd.X.shape[0] == hd.y.shape[0]


# ---- 1. the generator --------------------------------------------------------------------------------------------------------
def test_philox4x32_10_known_answers():
    assert [int(w) for w in philox4x32([0, 0, 0, 0], [0, 0])] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    out = philox4x32([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])
    assert [int(w) for w in out] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # vectorised over counters, one key
    both = philox4x32([[0, 0, 0, 0], [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], [[0, 0], [0xa4093822, 0x299f31d0]])
    assert both.dtype == np.uint32 and int(both[0, 0]) == 0x6627e8d5 and int(both[1, 3]) == 0x24126ea1


# ---- 2. the chunk list -------------------------------------------------------------------------------------------------------
def _chunks_by_the_rule(lengths, window, reach):
    """The chunk list from the rule's statement: windows of `window` frames every window // 2 frames, clipped at the sequence's
    end; one random.randint per window, from its end up to `reach` frames further, names a frame that is appended together
    with its successor if both exist."""
    out = []
    for s, n in enumerate(lengths):
        start = 0
        while start < n:
            frames = list(range(start, min(start + window, n)))
            jump = random.randint(start + window, start + window + reach)
            if jump + 1 < n:
                frames.extend((jump, jump + 1))
            out.append((s, frames))
            start += window // 2
    return out


@pytest.mark.parametrize('cw, rw', [(5, 0), (5, 3), (4, 2), (10, 5)])
def test_make_chunks_is_the_references_list(cw, rw):
    num_frames = [3, 11, 12, 1, 154, 2 * cw, 2 * cw + 1]                  # shorter than a window; not a multiple of the stride
    random.seed(17)
    want = _chunks_by_the_rule(num_frames, cw, rw)
    random.seed(17)
    got = make_chunks(num_frames, cw, rw)
    assert got == want
    assert make_chunks(num_frames, cw, rw, rng=random.Random(17)) == want       # (a generator of one's own: same calls)
    assert [fr for s, fr in got if s == 0][0] == [0, 1, 2]


def test_make_chunks_skip_pair_edge():
    # ret_win_size = 0: skip_fr = st + 5.  11 frames: st = 4 gives 9 < 10, the pair (9, 10) is appended; 12 frames: st = 6 gives
    # 11 < 11, false, nothing is appended, while st = 4 gives 9 < 11
    c11 = dict((fr[0], fr) for _, fr in make_chunks([11], 5, 0))
    assert c11[4] == [4, 5, 6, 7, 8, 9, 10] and c11[6] == [6, 7, 8, 9, 10]
    c12 = dict((fr[0], fr) for _, fr in make_chunks([12], 5, 0))
    assert c12[6] == [6, 7, 8, 9, 10] and c12[4] == [4, 5, 6, 7, 8, 9, 10] and c12[5 - 5] == [0, 1, 2, 3, 4, 5, 6]
    with pytest.raises(ValueError):
        make_chunks([10], 1, 0)


# ---- 3. the rules ------------------------------------------------------------------------------------------------------------
def _rule_cases():
    seqs = synth_sequences(seed=3)
    tiny = dict(frame=np.array([0, 2]), track=np.array([5, -1]), cat=np.array([2, 1]),
                box=np.array([[100.37, 150.11, 180.93, 210.77], [640.49, 160.03, 700.21, 222.9]]), score=np.array([0.91, 0.55]),
                width=1242, num_frames=3)
    seqs.append(tiny)
    random.seed(5)
    chunks = make_chunks([s['num_frames'] for s in seqs], 5, 3)
    chunks.append((4, [10, 11, 12, 13, 14, 20, 21]))                     # a skip pair by hand
    return seqs, chunks


@pytest.mark.parametrize('feats', ['2d', '2d+temp'])
def test_a_draw_is_the_references_arithmetic(feats):
    seqs, chunks = _rule_cases()
    store = host_store(seqs, feats)
    idx = np.arange(len(chunks))
    seen = dict(skip_reversed=False, empty_frame=False, empty_chunk=False, flipped_rounding=False, all_four=set())
    for step in range(40):
        hd = draw_chunks_host(store, chunks, idx, step, seed=2024)
        assert_draw_follows_the_rules(hd, seqs, chunks, idx, feats)
        pos = 0
        for b, (s, frames) in enumerate(chunks):
            per_frame = [int((seqs[s]['frame'] == f).sum()) for f in frames]
            keep = hd.kept[pos:pos + sum(per_frame)]
            rev, flip = bool(hd.flags[b] & FLAG_REVERSED), bool(hd.flags[b] & FLAG_FLIPPED)
            seen['all_four'].add((rev, flip))
            skip_pair = len(frames) > 2 and frames[-2] != frames[-3] + 1
            if rev and skip_pair and keep.any():
                seen['skip_reversed'] = True
                y = hd.y[hd.offsets[b]:hd.offsets[b + 1]]
                assert set(y[:, 0]) <= {frames[-1] - f + frames[0] for f in frames}       # about the LIST's ends
                assert (np.diff(y[:, 0]) <= 0).all()                                      # rows keep their order
            k = 0
            for nf in per_frame:
                if nf and not keep[k:k + nf].any() and keep.any():
                    seen['empty_frame'] = True
                k += nf
            if keep.size and not keep.any():
                seen['empty_chunk'] = True
                assert hd.offsets[b] == hd.offsets[b + 1]
            if flip and keep.any():
                # boxes whose flipped x1 rounds differently when W - x2 - 1 is formed in float32 instead of float64
                W, f32 = seqs[s]['width'], np.float32
                x2 = np.concatenate([seqs[s]['box'][seqs[s]['frame'] == f, 2] for f in frames])[keep]
                if ((W - x2 - 1).astype(f32) != f32(W) - x2.astype(f32) - f32(1)).any():
                    seen['flipped_rounding'] = True
            pos += sum(per_frame)
    assert seen['skip_reversed'] and seen['empty_frame'] and seen['empty_chunk'] and seen['flipped_rounding'], seen
    assert len(seen['all_four']) == 4


def test_the_flip_is_not_one_column_in_float32():
    """Why the store keeps the whole static row of the flipped box: x1' and x2' are rounded to float32 one by one, so the width
    x2' - x1' of a flipped box can differ from the plain width in the last bit (the heights and the rest never do)."""
    store = host_store(synth_sequences(seed=4, lengths=(60,)), '2d')
    plain, flipped = store.stat[:, 0], store.stat[:, 1]
    xc, w = NCAT + 1, NCAT + 3
    other = [c for c in range(store.Fs) if c not in (xc, w)]
    assert np.array_equal(plain[:, other], flipped[:, other])
    assert (plain[:, xc] != flipped[:, xc]).mean() > 0.9
    assert (plain[:, w] != flipped[:, w]).any() and np.abs(plain[:, w] - flipped[:, w]).max() < 1e-5


# ---- 4. the rates ------------------------------------------------------------------------------------------------------------
def test_rates_of_the_three_decisions():
    seqs = synth_sequences(seed=6, lengths=(60,) * 20, p_empty=0.1)
    store = host_store(seqs, '2d')
    chunks = make_chunks([60] * 20, 5, 3, rng=random.Random(7))
    sampler = ChunkSampler(store, chunks, seed=0xC0FFEE123456789)
    idx = np.arange(len(chunks))
    flags, kept = [], []
    for step in range(1 + 20000 // len(chunks)):
        hd = sampler.draw_host(idx, step)
        flags.append(hd.flags)
        kept.append(hd.kept)
    flags, kept = np.concatenate(flags), np.concatenate(kept)
    n_c, n_d = flags.size, kept.size
    assert n_c >= 2 * 10 ** 4 and n_d >= 2 * 10 ** 5
    bound = lambda p, n: 5 * np.sqrt(p * (1 - p) / n)
    rev, flip = (flags & FLAG_REVERSED) != 0, (flags & FLAG_FLIPPED) != 0
    print(f'dropout {1 - kept.mean():.5f} of {n_d}; reversed {rev.mean():.5f}, flipped {flip.mean():.5f}, both '
          f'{(rev & flip).mean():.5f} of {n_c}')
    assert abs((1 - kept.mean()) - 0.2) <= bound(0.2, n_d)
    assert abs(rev.mean() - 0.5) <= bound(0.5, n_c)
    assert abs(flip.mean() - 0.5) <= bound(0.5, n_c)
    assert abs((rev & flip).mean() - 0.25) <= bound(0.25, n_c)               # independent decisions


# ---- 5. keying ---------------------------------------------------------------------------------------------------------------
def _segment(hd, b):
    o0, o1 = hd.offsets[b], hd.offsets[b + 1]
    return hd.X[o0:o1].tobytes(), hd.y[o0:o1].tobytes(), int(hd.flags[b])


def test_a_draw_is_keyed_by_chunk_and_step_not_by_the_batch():
    seqs, chunks = _rule_cases()
    store = host_store(seqs, '2d+temp')
    sampler = ChunkSampler(store, chunks, seed=99)
    big = int(np.argmax(sampler.size))
    others = [i for i in range(len(chunks)) if i != big]
    alone = sampler.draw_host([big], 5)
    assert _segment(alone, 0) == _segment(sampler.draw_host(others[:6] + [big], 5), 6)
    assert _segment(alone, 0) == _segment(sampler.draw_host([others[9], big] + others[20:23], 5), 1)
    assert _segment(alone, 0) == _segment(sampler.draw_host([big, big], 5), 1)
    per_step = [sampler.draw_host([big], s).kept.tobytes() for s in range(8)]
    assert len(set(per_step)) > 1                                          # the steps differ
    assert sampler.draw_host([big], 5).kept.tobytes() == per_step[5]        # and a step repeats
    assert ChunkSampler(store, chunks, seed=100).draw_host([big], 5).kept.tobytes() != per_step[5] or \
        ChunkSampler(store, chunks, seed=100).draw_host([big], 6).kept.tobytes() != per_step[6]
    # the epoch order: a permutation, seeded, different from epoch to epoch
    o0, o1 = sampler.epoch_order(0), sampler.epoch_order(1)
    assert sorted(o0) == list(range(len(chunks))) and np.array_equal(o0, sampler.epoch_order(0)) and not np.array_equal(o0, o1)


@pytest.mark.parametrize('feats', ['2d', '2d+temp'])
def test_without_transforms_a_draw_is_the_plain_chunk(feats):
    seqs, chunks = _rule_cases()
    store = host_store(seqs, feats)
    idx = np.arange(len(chunks))[::-1].copy()
    a = draw_chunks_host(store, chunks, idx, 3, seed=1, random_transforms=False)
    assert not a.flags.any() and a.kept.all() and a.offsets[-1] == a.n_max
    assert_draw_follows_the_rules(a, seqs, chunks, idx, feats)
    b = draw_chunks_host(store, chunks, idx, 4, seed=2, random_transforms=False)
    assert np.array_equal(a.X, b.X) and np.array_equal(a.y, b.y)           # no random number is involved


# ---- 6. refusals (host checks: nothing is launched) --------------------------------------------------------------------------
def test_malformed_inputs_raise():
    seqs, chunks = _rule_cases()
    m, s = KITTI_MEAN['2d'], KITTI_STD['2d']
    with pytest.raises(ValueError, match='vis'):
        DetectionStore(seqs, NCAT, '2d+temp+vis', m, s, device=None)
    with pytest.raises(ValueError, match='mean / std of length'):
        DetectionStore(seqs, NCAT, '2d+temp', m, s, device=None)
    with pytest.raises(ValueError, match='mean / std of length'):
        DetectionStore(seqs, NCAT, '2d', m, s + [1.0], device=None)
    bad = [dict(q) for q in seqs]
    bad[2]['cat'] = bad[2]['cat'].copy()
    bad[2]['cat'][0] = NCAT + 1
    with pytest.raises(ValueError, match='cat outside'):
        DetectionStore(bad, NCAT, '2d', m, s, device=None)
    store = host_store(seqs, '2d')
    with pytest.raises(ValueError, match='num_frames'):
        ChunkSampler(store, chunks + [(1, [1, 2, 3])], seed=0)               # sequence 1 has three frames: 0, 1, 2
    sampler = ChunkSampler(store, chunks, seed=0)
    with pytest.raises(IndexError):
        sampler.draw_host([0, len(chunks)], 0)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        sampler.draw([0], 0)                                               # a host-only store has no device draw
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        DetectionStore(seqs, NCAT, '2d', m, s, device='cpu')


def test_every_chunk_skipped_is_an_exception_of_its_own():
    from trackmpnn_amd import AllChunksSkipped, build_train_batch
    assert issubclass(AllChunksSkipped, ValueError)
    one_timestep, only_false_positives = np.array([[3, 1], [3, 2]]), np.array([[0, -1], [1, -1]])
    with pytest.raises(AllChunksSkipped, match='every chunk is skipped'):
        build_train_batch([one_timestep, only_false_positives])
    with pytest.raises(AllChunksSkipped):
        build_train_batch([])


def test_a_chunk_above_the_builders_limit_is_refused():
    from trackmpnn_amd.train_batch import TB_MAX_DETS
    n = TB_MAX_DETS + 1
    rng = np.random.RandomState(8)
    seq = dict(frame=np.arange(n) % 4, track=np.arange(n), cat=np.ones(n, np.int64), box=rng.uniform(0, 300, (n, 4)),
               score=np.ones(n), width=1242, num_frames=4)
    store = host_store([seq], '2d')
    with pytest.raises(ValueError, match='TB_MAX_DETS'):
        ChunkSampler(store, [(0, [0, 1, 2, 3])], seed=0)
    ChunkSampler(store, [(0, [0, 1, 2])], seed=0)


def test_entry_points_validate_on_the_host():
    import ctypes
    import os
    from trackmpnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.tmpnn_chunk_draw_count(None, None) == -1 and b'descriptor is null' in lib.tmpnn_last_error()
    d = _lib.CChunkDraw()
    d.B, d.nchunks, d.nseq, d.L, d.F, d.Fs, d.fr_range, d.nframes = 1, 1, 1, 257, 8, 8, 30, 1
    assert lib.tmpnn_chunk_draw_count(ctypes.byref(d), None) == -1 and b'L=257' in lib.tmpnn_last_error()
    d.L, d.F = 7, 9
    assert lib.tmpnn_chunk_draw_fill(ctypes.byref(d), None) == -1 and b'F = Fs or Fs + 2' in lib.tmpnn_last_error()
    d.F = 10
    assert lib.tmpnn_chunk_draw_count(ctypes.byref(d), None) == -1 and b'null pointer' in lib.tmpnn_last_error()
