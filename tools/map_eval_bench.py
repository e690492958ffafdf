"""Wall time of the validation mAP on the device next to the host definition, on the same tracks in the same run.

    python tools/map_eval_bench.py --out profiles/map_eval_run.md

A KITTI-val-shaped set from synthetic sequences (mapeval.synth_map_sequence: 10 sequences of 480 to 1120 frames, about 8
objects, three classes, duplicates, strays, frames without GT).  In ONE process:

  (a) map_host over the sequences (numpy)                           wall time of the call
  (b) MapEvaluator.evaluate + read (one upload, two launches, one   wall time from the call to the returned dict
      device -> host copy; the store was built and uploaded before)

and (b) taken apart: evaluate() up to its return (upload + launches enqueued), the wait for the device, the copy and the dict.
The two must agree: counts equal, ap and map bit for bit (checked on every repetition).  Not bench.py: nothing here gates a
change."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bits(x):
    return np.float64(x).view(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sequences', type=int, default=10)
    ap.add_argument('--frames', type=int, default=800)
    ap.add_argument('--objects', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='write the table (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('map_eval_bench needs the MI355X: no timing is taken without it')
    from trackmpnn_amd.mapeval import MapEvaluator, map_host, synth_map_sequence
    dev = 'cuda:0'
    rng = np.random.default_rng(3)
    seqs = [synth_map_sequence(8100 + i, int(a.frames * rng.uniform(0.6, 1.4)), objects=a.objects) for i in range(a.sequences)]
    tracks = [q['tracks'] for q in seqs]
    t0 = time.perf_counter()
    ev = MapEvaluator(seqs, dev)
    torch.cuda.synchronize()
    build_ms = 1e3 * (time.perf_counter() - t0)

    def on_host():
        t0 = time.perf_counter()
        out = map_host(seqs, tracks)
        return out, 1e3 * (time.perf_counter() - t0)

    def on_device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate(tracks)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out = ev.read()
        t3 = time.perf_counter()
        return out, [1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)]

    host_ms, dev_ms = [], []
    for r in range(a.reps + 1):                                   # (repetition 0 warms up)
        ref, hm = on_host()
        out, dm = on_device()
        for k in ('classes', 'annotations', 'kept', 'true_positives'):
            assert out[k] == ref[k], f'{k} differ: {out[k]} != {ref[k]}'
        assert [bits(x) for x in out['ap']] == [bits(x) for x in ref['ap']] and bits(out['map']) == bits(ref['map']), 'ap / map differ'
        if r:
            host_ms.append(hm)
            dev_ms.append(dm)
    h = min(host_ms)
    d = min(dev_ms, key=lambda v: v[0])
    st = ev.store
    lines = [f'{len(seqs)} sequences, {st.n_gt} GT rows, {st.n_det} detections ({st.n_live} in frames with GT, {st.n_claim} with a best '
             f'GT row), {st.C} classes; mAP {out["map"]:.4f}, kept {out["kept"]}, true positives {out["true_positives"]}; best of '
             f'{a.reps} repetitions after one warm-up; the store is built and uploaded once ({build_ms:.1f} ms with the launch of '
             f'`tmpnn_map_best` and its read-back, not in the figures).', '',
             '| path | ms per evaluation | ns per detection |', '|---|---|---|',
             f'| (a) `map_host` over the sequences | {h:.3f} | {1e6 * h / max(st.n_det, 1):.1f} |',
             f'| (b) `evaluate` + `read` | {d[0]:.3f} | {1e6 * d[0] / max(st.n_det, 1):.1f} |',
             f'| (b) of which: `evaluate` returns after | {d[1]:.3f} | |',
             f'| (b) of which: wait for the device | {d[2]:.3f} | |',
             f'| (b) of which: copy + dict | {d[3]:.3f} | |',
             '', f'host / device: {h / d[0]:.1f}x']
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(dict(tool='map_eval_bench', device=torch.cuda.get_device_name(0), sequences=len(seqs), detections=st.n_det,
                          host_ms=h, device_ms=d[0], enqueue_ms=d[1], wait_ms=d[2], read_ms=d[3], store_build_ms=build_ms)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
