"""Record what the reference's compute_map (utils/metrics.py:126-229) gives on a few small tie-free cases.

    python tools/gen_map_golden.py --reference-path DIR --out tests/golden/map

DIR is a checkout of the reference.  Its utils.metrics is imported as it is, under two shims: `np.str = str` (the function
uses the alias numpy removed) and a stub module `motmetrics` (imported at the top of the file, not used by compute_map).  Each
case is fed the way train.py:265-273 feeds it -- float32 rows (cat, alpha, x1, y1, x2, y2, ..., score), only the detections with
a track, every GT row -- and written as map_<name>.npz: the inputs per sequence (s<i>_det_frame ...), the tracks, which
sequences were left out, the reference's mAP and the largest per-class true-positive count (the tests' error bound).

The fixtures live in a directory of their own: tests/conftest.py takes every .npz directly under tests/golden for a model
fixture.  They are data; nothing of the reference's text is copied here."""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYS = ('det_frame', 'det_box', 'det_cat', 'det_score', 'gt_frame', 'gt_box', 'gt_cat', 'gt_track', 'tracks')
# name -> ([(seed, frames)], index of a sequence that is left out or None)
CASES = {'single': ([(3, 40)], None), 'three': ([(11, 30), (12, 45), (13, 25)], None), 'left_out': ([(21, 35), (22, 30), (23, 35)], 1)}


def reference_compute_map(path):
    if 'str' not in vars(np):
        np.str = str
    sys.modules.setdefault('motmetrics', types.ModuleType('motmetrics'))
    sys.path.insert(0, path)
    from utils.metrics import compute_map
    return compute_map


def rows14(cat, box, score):
    r = np.zeros((cat.shape[0], 14), np.float32)
    r[:, 0], r[:, 2:6], r[:, 13] = cat, box, score
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join('tests', 'golden', 'map'))
    a = ap.parse_args()
    from trackmpnn_amd.mapeval import map_host, synth_map_sequence
    compute_map = reference_compute_map(a.reference_path)
    os.makedirs(a.out, exist_ok=True)
    for name, (specs, left) in CASES.items():
        seqs = [synth_map_sequence(seed, frames) for seed, frames in specs]
        pred, gt = {}, {}
        for s, q in enumerate(seqs):
            if s == left:
                continue
            kept = q['tracks'] >= 0
            y_out = np.stack([q['det_frame'], q['tracks']], 1).astype(np.int64)
            pred[str(s)] = (y_out[kept], rows14(q['det_cat'], q['det_box'], q['det_score'])[kept])
            gt[str(s)] = (np.stack([q['gt_frame'], q['gt_track']], 1).astype(np.int64),
                          rows14(q['gt_cat'], q['gt_box'], np.zeros(q['gt_cat'].shape[0])))
        ref = float(compute_map(pred, gt))
        ours = map_host(seqs, [None if s == left else q['tracks'] for s, q in enumerate(seqs)])
        out = {f's{s}_{k}': q[k] for s, q in enumerate(seqs) for k in KEYS}
        out.update(n_seq=np.int64(len(seqs)), left_out=np.int64(-1 if left is None else left), map_ref=np.float64(ref),
                   max_tp=np.int64(max(ours['true_positives'])))
        path = os.path.join(a.out, f'map_{name}.npz')
        np.savez_compressed(path, **out)
        share = [t / k for t, k in zip(ours['true_positives'], ours['kept'])]
        print(f'{path}: {os.path.getsize(path)} bytes, reference mAP {ref!r}, map_host {ours["map"]!r} (diff {abs(ref - ours["map"]):.2e}), '
              f'true-positive share per class {[round(x, 3) for x in share]}')


if __name__ == '__main__':
    main()
