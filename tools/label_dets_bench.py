"""Wall time of the GT track-id labelling on the device next to the host definition, on the same sequences in the same run.

    python tools/label_dets_bench.py --out profiles/label_dets_run.md

Two sets of synthetic sequences (labeling.synth_label_sequence; tools/gen_label_golden.py --time runs the reference's own function
over the same frames on the CPU):

    kitti   21 sequences of 237 to 528 frames (8258 in all), 0 .. 16 detections and GT rows a frame, KITTI_RULES
    bdd     200 sequences of 200 frames, 0 .. 24 detections and GT rows a frame, BDD_RULES

In ONE process, per set:

  (a) label_detections_host over the sequences (numpy)               wall time of the call, once
  (b) DetectionLabeler.label + read (four launches, one device ->    wall time from the call to the returned list; the store
      host copy)                                                     was built and uploaded before

and (b) taken apart: label() up to its return (launches enqueued), the wait for the device, the copy and the lists.  The two
must agree exactly (checked on every repetition).  Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (rule set, sequences, frames per sequence (mean; +-40 % where spread), spread, max boxes a side, seed)
SETS = {'kitti': ('kitti', 21, 380, True, 16, 7000), 'bdd': ('bdd', 200, 200, False, 24, 9000)}


def build_set(name):
    """(rule set name, the sequences) of one of SETS, from its seeds."""
    from trackmpnn_amd.labeling import BDD_RULES, KITTI_RULES, synth_label_sequence
    rs, n, frames, spread, boxes, seed = SETS[name]
    rules = {'kitti': KITTI_RULES, 'bdd': BDD_RULES}[rs]
    rng = np.random.default_rng(seed)
    return rs, [synth_label_sequence(seed + i, int(frames * rng.uniform(0.6, 1.4)) if spread else frames, rules, max_det=boxes,
                                     max_gt=boxes) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sets', default='kitti,bdd')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('label_dets_bench needs the MI355X: no timing is taken without it')
    from trackmpnn_amd.labeling import BDD_RULES, KITTI_RULES, DetectionLabeler, label_detections_host
    dev = 'cuda:0'
    text = []
    for name in a.sets.split(','):
        rs, seqs = build_set(name)
        rules = {'kitti': KITTI_RULES, 'bdd': BDD_RULES}[rs]
        t0 = time.perf_counter()
        ref = label_detections_host(seqs, rules)
        host_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        lb = DetectionLabeler(seqs, rules, dev)
        torch.cuda.synchronize()
        build_ms = 1e3 * (time.perf_counter() - t0)
        dev_ms = []
        for r in range(a.reps + 1):                               # (repetition 0 warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lb.label()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            out = lb.read()
            t3 = time.perf_counter()
            for o, h in zip(out, ref):
                for k in ('track', 'keep', 'gt_keep'):
                    assert np.array_equal(o[k], h[k]), f'{name}: {k} differ'
            if r:
                dev_ms.append([1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)])
        d = min(dev_ms, key=lambda v: v[0])
        keep, track = np.concatenate([o['keep'] for o in out]), np.concatenate([o['track'] for o in out])
        text += [f'### {name}', '',
                 f'{len(seqs)} sequences, {lb.F} frames, {lb.n_det} detections, {lb.n_gt} GT rows ({lb.n_small} frames by one wave, '
                 f'{lb.n_big} by a workgroup); {int((track >= 0).sum())} assigned, {int(keep.sum())} kept; best of {a.reps} repetitions '
                 f'after one warm-up; the store is checked, sorted and uploaded once ({build_ms:.1f} ms, not in the figures); '
                 f'device and host results equal on every repetition.', '',
                 '| path | ms | us per frame |', '|---|---|---|',
                 f'| (a) `label_detections_host` (one run) | {host_ms:.1f} | {1e3 * host_ms / lb.F:.2f} |',
                 f'| (b) `label` + `read` | {d[0]:.3f} | {1e3 * d[0] / lb.F:.3f} |',
                 f'| (b) of which: `label` returns after | {d[1]:.3f} | |',
                 f'| (b) of which: wait for the device | {d[2]:.3f} | |',
                 f'| (b) of which: copy + lists | {d[3]:.3f} | |', '', f'host / device: {host_ms / d[0]:.0f}x', '']
        print(json.dumps(dict(tool='label_dets_bench', set=name, device=torch.cuda.get_device_name(0), frames=lb.F, detections=lb.n_det,
                              host_ms=host_ms, device_ms=d[0], enqueue_ms=d[1], wait_ms=d[2], read_ms=d[3], store_build_ms=build_ms)))
    text = '\n'.join(text)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
