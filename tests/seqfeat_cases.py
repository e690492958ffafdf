"""Shared inputs of tests/test_seq_features.py and tests/test_seq_features_gpu.py: seeded synthetic sequences and the feature
statistics of the two data sets (read from tests/golden/seqfeat, where the reference's dataset classes left them)."""
import os

import numpy as np

from trackmpnn_amd.chunks import DetectionStore

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'seqfeat')
FIXTURES = ('kitti_2d', 'kitti_2d_temp', 'bdd_2d_temp')
NCAT_KITTI, NCAT_BDD = 3, 8
# F = 8, 10, 138 (KITTI) and 13, 15, 143 (BDD)
WIDTHS = [(NCAT_KITTI, '2d'), (NCAT_KITTI, '2d+temp'), (NCAT_KITTI, '2d+temp+vis'), (NCAT_BDD, '2d'), (NCAT_BDD, '2d+temp'),
          (NCAT_BDD, '2d+temp+vis')]


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f'seqfeat_{name}.npz')) as z:
        return {k: z[k] for k in z.files}


def fixture_sequences(fx):
    """The store's input of a fixture: one dict per sequence, the track ids the reference assigned."""
    return [{k: fx[f's{i}_{k}'] for k in ('frame', 'track', 'cat', 'box', 'score', 'width', 'height', 'num_frames')}
            for i in range(int(fx['nseq']))]


def feature_stats(ncat, feats):
    """(mean, std) of `feats` for the data set with `ncat` categories: the reference's values for the static and temporal
    columns, 0.5 / 0.5 for the visual ones (kitti_mot.py:155-177)."""
    fx = load_fixture('kitti_2d_temp' if ncat == NCAT_KITTI else 'bdd_2d_temp')
    assert int(fx['ncat']) == ncat
    out = []
    for v in (fx['mean'], fx['std']):
        a = list(v[:ncat + 5]) + (list(v[ncat + 5:ncat + 7]) if 'temp' in feats else []) + ([0.5] * 128 if 'vis' in feats else [])
        out.append(np.asarray(a, np.float32))
    return out


def synth_sequence(rng, num_frames, ncat, dets=(0, 4), im_hw=(375, 1242), shuffle=True):
    """One sequence of random detections: dets[0] .. dets[1] per frame (an int per frame: that many), some false positives
    (track -1), boxes with decimals float32 cannot hold; the rows are handed over unsorted (the store sorts stably by frame)."""
    n_f = (np.asarray(dets(np.arange(num_frames))) if callable(dets) else rng.integers(dets[0], dets[1] + 1, num_frames)).astype(np.int64)
    frame = np.repeat(np.arange(num_frames), n_f)
    n = frame.size
    if shuffle and n:
        frame = frame[rng.permutation(n)]
    h, w = im_hw
    x1 = np.round(rng.uniform(0, 0.85 * w, n), 2)                          # (inside the image, whatever its size)
    y1 = np.round(rng.uniform(0, 0.65 * h, n), 2)
    box = np.stack([x1, y1, x1 + np.round(rng.uniform(0.01 * w, 0.12 * w, n), 2), y1 + np.round(rng.uniform(0.02 * h, 0.3 * h, n), 2)], 1)
    track = rng.integers(0, 300, n)
    track[rng.random(n) < 0.25] = -1
    return dict(frame=frame, track=track, cat=rng.integers(1, ncat + 1, n), box=box, score=np.round(rng.uniform(0.3, 1, n), 4),
                width=w, height=h, num_frames=num_frames)


def synth_store(seed, lengths, ncat, feats, device=None, dets=(0, 4), fr_range=30, empty=()):
    """(store, sequences): sequences of `lengths` frames; those whose index is in `empty` hold no detection."""
    rng = np.random.default_rng([seed, 7])
    sizes = [(375, 1242), (370, 1224), (720, 1280)]
    seqs = [synth_sequence(rng, nf, ncat, (0, 0) if i in empty else dets, sizes[i % 3]) for i, nf in enumerate(lengths)]
    mean, std = feature_stats(ncat, feats)
    return DetectionStore(seqs, ncat, feats, mean, std, fr_range=fr_range, device=device), seqs
