"""Wall time of the HOTA evaluation on the device next to the host definition, on the same tracks in the same run.

    python tools/hota_eval_bench.py --out profiles/hota_eval_run.md
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/hota_eval_bench.py --trace 20

Two sets of synthetic sequences (hota.synth_hota_sequence: moteval.synth_mot_sequence -- misses, stray hypotheses, id swaps,
untracked detections -- with the detection jitter widened so that every threshold separates pairs); nothing outside the tree is
read:

  kitti   a KITTI-validation-sized set: 3 sequences of about 300 to 800 frames, about 10 objects per frame
  bdd     a BDD-validation-sized set: 200 sequences of 200 frames

For each, in ONE process:

  (a) hota_host over every sequence (numpy + scipy)                 wall time of the loop (--host-reps repetitions)
  (b) HotaEvaluator.evaluate + read (one packed upload, one clear   wall time from the call to the returned dicts, which
      and four launches, one device -> host copy; the store was      ends in the copy's synchronise: --reps repetitions
      uploaded before)                                               after --warmup, median and spread

and (b) taken apart: evaluate() up to its return, the wait for the device, the copy and the dicts.  (a) and (b) must agree
in every record field, integers equal and float64 bit for bit (checked against the first host result on every repetition).
--trace N: N evaluations of the chosen --set and nothing else (the program to put under rocprofv3 for the per-kernel times).
Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_set(name):
    from trackmpnn_amd.hota import synth_hota_sequence
    if name == 'kitti':
        return [synth_hota_sequence(9100 + i, L, objects=10) for i, L in enumerate((300, 550, 800))]
    return [synth_hota_sequence(9200 + i, 200, objects=8) for i in range(200)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--set', choices=('kitti', 'bdd', 'both'), default='both')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--trace', type=int, default=0, help='run this many evaluations and nothing else')
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hota_eval_bench needs the MI355X: no timing is taken without it')
    from trackmpnn_amd.hota import INT_KEYS, PAIR_BYTES, SUM_KEYS, HotaEvaluator, hota_host, hota_overall
    dev = 'cuda:0'
    text, rows = [], []
    for name in (('kitti', 'bdd') if a.set == 'both' else (a.set,)):
        seqs = make_set(name)
        tracks = [q['tracks'] for q in seqs]
        t0 = time.perf_counter()
        ev = HotaEvaluator(seqs, dev)
        torch.cuda.synchronize()
        build_ms = 1e3 * (time.perf_counter() - t0)
        if a.trace:
            for _ in range(a.trace):
                ev.evaluate(tracks)
                ev.read()
            continue

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

        host_ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            ref = [hota_host(q['det_frame'], q['det_box'], q['tracks'], q['gt_frame'], q['gt_track'], q['gt_box']) for q in seqs]
            host_ms.append(1e3 * (time.perf_counter() - t0))
        dev_ms = []
        for r in range(a.warmup + a.reps):
            per, overall, dm = on_device()
            for s, (d, h) in enumerate(zip(per, ref)):
                assert np.array_equal(d['tp'], h['tp']) and all(d[k] == h[k] for k in INT_KEYS), f'{name}: sequence {s}: counts differ'
                assert all(np.array_equal(d[k].view(np.int64), h[k].view(np.int64)) for k in SUM_KEYS), f'{name}: sequence {s}: float sums differ'
            if r >= a.warmup:
                dev_ms.append(dm)
        dm = np.array(dev_ms)
        med = np.median(dm, axis=0)
        h = float(np.median(host_ms))
        st = ev.store
        nf = sum(int(x) for x in st.seq[:, 5])
        ro = hota_overall(ref)
        text += [f'### {name}', '',
                 f'{len(seqs)} sequences, {nf} frames, {st.n_gt} GT rows, {st.n_det} detections, {st.n_obj} objects, {ro["hypotheses"]} hypotheses; '
                 f'pair workspace {ev._n_pair} entries x {PAIR_BYTES} bytes, workspace {ev._ws_bytes} bytes; overall HOTA {ro["hota"]:.4f}, '
                 f'DetA {ro["deta"]:.4f}, AssA {ro["assa"]:.4f}, LocA {ro["loca"]:.4f}, tp {int(ro["tp"][0])} .. {int(ro["tp"][-1])}; '
                 f'{a.reps} repetitions after {a.warmup} warm-ups, host {a.host_reps} repetitions; every repetition equal to the host in '
                 f'every record field; the store is built and uploaded once ({build_ms:.1f} ms, not in the figures).', '',
                 '| path | median ms | min | max | us per frame |', '|---|---|---|---|---|',
                 f'| (a) `hota_host` over the sequences | {h:.1f} | {min(host_ms):.1f} | {max(host_ms):.1f} | {1e3 * h / nf:.2f} |',
                 f'| (b) `evaluate` + `read` | {med[0]:.3f} | {dm[:, 0].min():.3f} | {dm[:, 0].max():.3f} | {1e3 * med[0] / nf:.2f} |',
                 f'| (b) of which: `evaluate` returns after | {med[1]:.3f} | {dm[:, 1].min():.3f} | {dm[:, 1].max():.3f} | |',
                 f'| (b) of which: wait for the device | {med[2]:.3f} | {dm[:, 2].min():.3f} | {dm[:, 2].max():.3f} | |',
                 f'| (b) of which: copy + dicts | {med[3]:.3f} | {dm[:, 3].min():.3f} | {dm[:, 3].max():.3f} | |',
                 '', f'host / device: {h / med[0]:.0f}x', '']
        rows.append(dict(set=name, sequences=len(seqs), frames=nf, pairs=ev._n_pair, ws_bytes=ev._ws_bytes, host_ms=h, device_ms=float(med[0]),
                         device_min_ms=float(dm[:, 0].min()), device_max_ms=float(dm[:, 0].max()), enqueue_ms=float(med[1]),
                         wait_ms=float(med[2]), read_ms=float(med[3]), store_build_ms=build_ms))
    if a.trace:
        return
    out = '\n'.join(text)
    print(out)
    print(json.dumps(dict(tool='hota_eval_bench', device=torch.cuda.get_device_name(0), sets=rows)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
