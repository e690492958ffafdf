"""Wall time of the MOT evaluation on the device next to the host definition, on the same tracks in the same run.

    python tools/mot_eval_bench.py --out profiles/mot_eval_run.md

A KITTI-val-shaped set from synthetic sequences (moteval.synth_mot_sequence: about 10 sequences of about 800 frames and about 8
objects, with misses, stray hypotheses, id swaps).  In ONE process:

  (a) mot_events_host over every sequence (numpy + scipy)          wall time of the loop
  (b) MotEvaluator.evaluate + read (one upload, one launch, one     wall time from the call to the returned dicts
      device -> host copy; the store was uploaded before)

and, with --split, (b) taken apart: evaluate() up to its return (upload + launch enqueued), the wait for the device, the
copy and the dicts.  The two must agree: counts equal, dist_sum bit for bit (checked on every repetition).  Not bench.py:
nothing here gates a change."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sequences', type=int, default=10)
    ap.add_argument('--frames', type=int, default=800)
    ap.add_argument('--objects', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='write the table (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mot_eval_bench needs the MI355X: no timing is taken without it')
    from trackmpnn_amd.moteval import COUNT_KEYS, MotEvaluator, mot_events_host, synth_mot_sequence
    dev = 'cuda:0'
    rng = np.random.default_rng(3)
    seqs = [synth_mot_sequence(8100 + i, int(a.frames * rng.uniform(0.6, 1.4)), objects=a.objects) for i in range(a.sequences)]
    tracks = [q['tracks'] for q in seqs]
    t0 = time.perf_counter()
    ev = MotEvaluator(seqs, dev)
    torch.cuda.synchronize()
    build_ms = 1e3 * (time.perf_counter() - t0)

    def on_host():
        t0 = time.perf_counter()
        out = [mot_events_host(q['det_frame'], q['det_box'], q['tracks'], q['gt_frame'], q['gt_track'], q['gt_box']) for q in seqs]
        return out, 1e3 * (time.perf_counter() - t0)

    def on_device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate(tracks)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        per, overall = ev.read()
        t3 = time.perf_counter()
        return per, overall, [1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)]

    host_ms, dev_ms = [], []
    for r in range(a.reps + 1):                                   # (repetition 0 warms up)
        ref, hm = on_host()
        per, overall, dm = on_device()
        for s, (d, h) in enumerate(zip(per, ref)):
            assert all(d[k] == h[k] for k in COUNT_KEYS), f'sequence {s}: counts differ: {d} != {h}'
            assert np.float64(d['dist_sum']).view(np.int64) == np.float64(h['dist_sum']).view(np.int64), f'sequence {s}: dist_sum'
        if r:
            host_ms.append(hm)
            dev_ms.append(dm)
    h = min(host_ms)
    d = min(dev_ms, key=lambda v: v[0])
    nf = sum(int(x) for x in ev.store.seq[:, 5])
    lines = [f'{len(seqs)} sequences, {nf} frames, {ev.store.n_gt} GT rows, {ev.store.n_det} detections, {ev.store.n_obj} objects; '
             f'overall MOTA {overall["mota"]:.4f}, {overall["switches"]} switches, {overall["false_positives"]} false positives, '
             f'{overall["misses"]} misses; best of {a.reps} repetitions after one warm-up; the store is built and uploaded once '
             f'({build_ms:.1f} ms, not in the figures).', '',
             '| path | ms per evaluation | us per frame |', '|---|---|---|',
             f'| (a) `mot_events_host` over the sequences | {h:.3f} | {1e3 * h / nf:.2f} |',
             f'| (b) `evaluate` + `read` | {d[0]:.3f} | {1e3 * d[0] / nf:.2f} |',
             f'| (b) of which: `evaluate` returns after | {d[1]:.3f} | |',
             f'| (b) of which: wait for the device | {d[2]:.3f} | {1e3 * d[2] / max(int(ev.store.seq[:, 5].max()), 1):.2f} (per frame of the longest sequence) |',
             f'| (b) of which: copy + dicts | {d[3]:.3f} | |',
             '', f'host / device: {h / d[0]:.1f}x']
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(dict(tool='mot_eval_bench', device=torch.cuda.get_device_name(0), sequences=len(seqs), frames=nf,
                          host_ms=h, device_ms=d[0], enqueue_ms=d[1], wait_ms=d[2], read_ms=d[3], store_build_ms=build_ms)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
