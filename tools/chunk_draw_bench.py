"""The draw of a training step: ChunkSampler.draw on the device against the host route to the same step.

    python tools/chunk_draw_bench.py --B 1024 16384 --reps 20 --out OUT.md

Workload: a C2-shaped set (B sequences of synth_window(7 frames, about 6 detections each) with random boxes, one chunk per
sequence, '2d' features), one draw of all B chunks with the reference's transforms.  Per B, device events around each stage
(the host's own work lies between the two events, so it is part of the figure), warm-up excluded, median and min .. max:

  (a) ChunkSampler.draw                                     the device draw (three launches, no wait)
  (b) ChunkSampler.draw_host + the upload of X and y        the only route to the same step without the device draw
  (c) DrawnChunks.batch()                                   build_train_batch_device on the drawn labels
  (d) train_chunks (forward calls, losses, one backward)    the step the draw feeds, H = 64

and the bytes a draw moves, from the shapes.  Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NCAT = 3
MEAN = [0.5] * 3 + [0.5, 600.0, 175.0, 75.0, 60.0]             # round stand-ins for a detector's statistics: the draw copies
STD = [0.5] * 3 + [0.25, 300.0, 25.0, 75.0, 50.0]              # standardised rows, so any mean / std times the same


def c2_set(n, seed):
    from trackmpnn_amd import synth_window
    rng = np.random.RandomState(seed)
    seqs = []
    for s in range(n):
        y = synth_window(1000 + s, 7, 6.0, 20)
        m = y.shape[0]
        x1, y1 = np.round(rng.uniform(0, 1080, m), 2), np.round(rng.uniform(100, 250, m), 2)
        box = np.stack([x1, y1, x1 + np.round(rng.uniform(5, 150, m), 2), y1 + np.round(rng.uniform(5, 120, m), 2)], 1)
        seqs.append(dict(frame=y[:, 0], track=y[:, 1], cat=rng.randint(1, NCAT + 1, m), box=box,
                         score=np.round(rng.uniform(0.3, 1, m), 4), width=1242, num_frames=int(y[:, 0].max()) + 1))
    return seqs, [(s, list(range(q['num_frames']))) for s, q in enumerate(seqs)]


def timed(fn, reps, warmup):
    """Milliseconds between two device events around fn(), per repetition."""
    out = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(r)
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1))
    return np.asarray(out)


def fmt(ms):
    return f'{np.median(ms):.3f} ({ms.min():.3f} .. {ms.max():.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, nargs='+', default=[1024, 16384])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--step-reps', type=int, default=5, help='repetitions of the train_chunks step (d)')
    ap.add_argument('--step-max-B', type=int, default=16384, help='largest B for which (d) is run')
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('chunk_draw_bench needs the MI355X: no timing is taken without it')
    import __graft_entry__
    __graft_entry__.build()
    from trackmpnn_amd import ChunkSampler, DetectionStore, TrackMPNN
    from trackmpnn_amd.loops import train_chunks
    dev = torch.device('cuda:0')
    lines = ['| B | rows before / after dropout | (a) device draw ms | (b) host draw + upload ms | (b) / (a) | (c) build ms | '
             '(d) train_chunks ms | MB moved by (a) |', '|---|---|---|---|---|---|---|---|']
    results = []
    for B in a.B:
        t0 = time.perf_counter()
        seqs, chunks = c2_set(B, seed=2)
        store = DetectionStore(seqs, NCAT, '2d', MEAN, STD, device=dev)
        sampler = ChunkSampler(store, chunks, seed=11)
        order = sampler.epoch_order(0)
        print(f'[chunk_draw_bench] B={B}: set built in {time.perf_counter() - t0:.1f} s, {store.ndets} detections', flush=True)
        keep = {}

        def dev_draw(r):
            keep['d'] = sampler.draw(order, r)

        def host_draw(r):
            hd = sampler.draw_host(order, r)
            keep['h'] = (torch.from_numpy(hd.X).to(dev), torch.from_numpy(hd.y).to(dev), torch.from_numpy(hd.offsets).to(dev))

        def build(r):
            keep['b'] = keep['d'].batch()

        ta = timed(dev_draw, a.reps, a.warmup)
        tb = timed(host_draw, max(3, a.reps // 4), 1)
        tc = timed(build, max(3, a.reps // 4), 1)
        drawn = keep['d']
        nd = int(drawn.offsets[-1])
        # same draw, same bits (the last repetition of either route used another step: compare one step directly)
        d1, h1 = sampler.draw(order, 1), sampler.draw_host(order, 1)
        n1 = int(h1.offsets[-1])
        assert torch.equal(d1.X[:n1].cpu(), torch.from_numpy(h1.X)) and torch.equal(d1.y[:n1].cpu(), torch.from_numpy(h1.y))
        td = None
        if B <= a.step_max_B:
            torch.manual_seed(5)
            model = TrackMPNN('2d', 3, 64, 0, 'diff').to(dev).train()
            batch = keep['b']
            X = drawn.features(batch)

            def step(r):
                model.zero_grad(set_to_none=True)
                train_chunks(model, batch, X)

            try:
                td = timed(step, a.step_reps, 1)
            except torch.cuda.OutOfMemoryError:
                print(f'[chunk_draw_bench] B={B}: train_chunks does not fit in device memory; (d) not run', flush=True)
                model.zero_grad(set_to_none=True)
        F, Fs = store.F, store.Fs
        # per kept row: the static row and the track id read, the X row and the (t', track) pair written; per chunk its table row,
        # the frame index (two passes), count / flags / offsets
        moved = nd * (4 * Fs + 4 + 4 * F + 16) + B * (2 * (4 * (4 + sampler.L) + 8 * sampler.L) + 4 + 1 + 8 + 4 + 16)
        lines.append(f'| {B} | {drawn.n_max} / {nd} | {fmt(ta)} | {fmt(tb)} | {np.median(tb) / np.median(ta):.0f} | {fmt(tc)} | '
                     f'{fmt(td) if td is not None else "not run"} | {moved / 1e6:.2f} |')
        results.append(dict(B=B, n_max=drawn.n_max, nd=nd, draw_ms=float(np.median(ta)), host_ms=float(np.median(tb)),
                            build_ms=float(np.median(tc)), step_ms=None if td is None else float(np.median(td)),
                            bytes_moved=int(moved)))
        print(lines[-1], flush=True)
        del keep, store, sampler
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(dict(tool='chunk_draw_bench', device=torch.cuda.get_device_name(0), reps=a.reps, results=results)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
