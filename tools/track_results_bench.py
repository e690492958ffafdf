"""Wall time of the result filter on the device next to the host definition, on the same tracks in the same run.

    python tools/track_results_bench.py --out profiles/track_results_run.md
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/track_results_bench.py --set test --trace 20

Two sets of synthetic sequences (results.synth_result_sequence); nothing outside the tree is read:

  val    a KITTI-validation-sized store: 3 sequences of 300 / 550 / 800 frames, about 10 rows a frame
  test   a KITTI-test-sized store: 29 sequences of about 10^4 rows each (about 700 frames, 14 rows a frame)

For each, in ONE process:

  (a) results_host over every sequence (numpy)                      wall time of the loop (--host-reps repetitions)
  (b) TrackResults.apply + read (one packed upload, one clear and    wall time from the call to the returned dicts, which
      four launches, one device -> host copy; the store was           ends in the copy's synchronise: --reps repetitions
      uploaded before)                                                after --warmup, median and spread

and (b) taken apart: apply() up to its return, the wait for the device, the copy and the dicts.  (a) and (b) must agree in the
filtered ids, the order and the counts (checked on every repetition).  --trace N: N applies + reads of the chosen --set and
nothing else (the program to put under rocprofv3 for the per-kernel times).  Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_set(name):
    from trackmpnn_amd.results import synth_result_sequence
    if name == 'val':
        return [synth_result_sequence(9300 + i, L, n_tracks=L // 3, max_len=40, p_gap=0.0, t0=0) for i, L in enumerate((300, 550, 800))]
    return [synth_result_sequence(9400 + i, 700, n_tracks=430, max_len=60, p_gap=0.0, t0=0) for i in range(29)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--set', choices=('val', 'test', 'both'), default='both')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--trace', type=int, default=0, help='run this many applies + reads and nothing else')
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('track_results_bench needs the MI355X: no timing is taken without it')
    from trackmpnn_amd.results import COUNT_KEYS, KITTI_RESULT_RULES, TrackResults, results_host, results_overall
    dev = 'cuda:0'
    text, rows = [], []
    for name in (('val', 'test') if a.set == 'both' else (a.set,)):
        seqs = make_set(name)
        tracks = [q['tracks'] for q in seqs]
        t0 = time.perf_counter()
        tr = TrackResults(seqs, KITTI_RESULT_RULES, dev)
        torch.cuda.synchronize()
        build_ms = 1e3 * (time.perf_counter() - t0)
        if a.trace:
            for _ in range(a.trace):
                tr.apply(tracks)
                tr.read()
            continue

        def on_device():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.apply(tracks)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            per = tr.read()
            t3 = time.perf_counter()
            return per, [1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)]

        host_ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            ref = [results_host(q, q['tracks'], KITTI_RESULT_RULES) for q in seqs]
            host_ms.append(1e3 * (time.perf_counter() - t0))
        dev_ms = []
        for r in range(a.warmup + a.reps):
            per, dm = on_device()
            for s, (d, h) in enumerate(zip(per, ref)):
                assert np.array_equal(d['tracks'], h['tracks']) and np.array_equal(d['order'], h['order']), f'{name}: sequence {s}: ids or order differ'
                assert all(d[k] == h[k] for k in COUNT_KEYS), f'{name}: sequence {s}: counts differ'
            if r >= a.warmup:
                dev_ms.append(dm)
        dm = np.array(dev_ms)
        med = np.median(dm, axis=0)
        h = float(np.median(host_ms))
        st = tr.store
        nf = sum(int(x) for x in st.seq[:, 5])
        ro = results_overall(ref)
        ntr = ro['kept_tracks'] + ro['removed_tracks']
        text += [f'### {name}', '',
                 f'{len(seqs)} sequences, {nf} frames, {st.n_det} rows, {ntr} tracks ({ro["removed_tracks"]} removed with {ro["removed_rows"]} rows; '
                 f'{ro["kept_rows"]} rows kept), {st.n_tab} table slots, workspace {tr._ws_bytes} bytes; {a.reps} repetitions after {a.warmup} '
                 f'warm-ups, host {a.host_reps} repetitions; every repetition equal to the host in ids, order and counts; the store is built '
                 f'and uploaded once ({build_ms:.1f} ms, not in the figures).', '',
                 '| path | median ms | min | max | us per row |', '|---|---|---|---|---|',
                 f'| (a) `results_host` over the sequences | {h:.1f} | {min(host_ms):.1f} | {max(host_ms):.1f} | {1e3 * h / st.n_det:.3f} |',
                 f'| (b) `apply` + `read` | {med[0]:.3f} | {dm[:, 0].min():.3f} | {dm[:, 0].max():.3f} | {1e3 * med[0] / st.n_det:.4f} |',
                 f'| (b) of which: `apply` returns after | {med[1]:.3f} | {dm[:, 1].min():.3f} | {dm[:, 1].max():.3f} | |',
                 f'| (b) of which: wait for the device | {med[2]:.3f} | {dm[:, 2].min():.3f} | {dm[:, 2].max():.3f} | |',
                 f'| (b) of which: copy + dicts | {med[3]:.3f} | {dm[:, 3].min():.3f} | {dm[:, 3].max():.3f} | |',
                 '', f'host / device: {h / med[0]:.0f}x', '']
        rows.append(dict(set=name, sequences=len(seqs), frames=nf, rows=int(st.n_det), tracks=ntr, ws_bytes=tr._ws_bytes, host_ms=h,
                         host_min_ms=min(host_ms), host_max_ms=max(host_ms), device_ms=float(med[0]), device_min_ms=float(dm[:, 0].min()),
                         device_max_ms=float(dm[:, 0].max()), enqueue_ms=float(med[1]), wait_ms=float(med[2]), read_ms=float(med[3]),
                         store_build_ms=build_ms))
    if a.trace:
        return
    out = '\n'.join(text)
    print(out)
    print(json.dumps(dict(tool='track_results_bench', device=torch.cuda.get_device_name(0), sets=rows)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
