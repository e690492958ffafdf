"""Batched chunk training with the reference's losses against the headline step, on the batch bench.py builds (C2: B = 16384
windows, 64 distinct seeds tiled).

    (a) bench.step: every call of the batch, BCE with logits over all logits against fixed targets, one backward, Adam
    (b) trackmpnn_amd.loops.train_chunks + Adam: the same calls with create_targets + CELoss + FocalLoss per chunk and call
        (one windowed loss launch per call each way), one backward -- the losses inside the timed region
    (b') (b) with a TrainMonitor (trackmpnn_amd.monitor): one counting launch per call and one fold per step more, no host read.
        (b) and (b') are timed in the same process, alternating step by step, so both see the same clocks and allocator state;
        R = sum over the calls of (listed det rows + listed edge rows) is what the counting launches read.  Also one C2 chunk
        through train_chunk (batch 1, where a launch per call shows) with and without a monitor, alternating likewise
    (c) the host build of (b)'s batch (build_train_batch: graphs, labels, loss windows, feature sources; once per set of chunks)
    (d) the device build of the same batch (build_train_batch_device) from one stacked [ND, 2] device tensor + offsets, and
        separately from the list of per-chunk host arrays
    (e) a fresh-batch step: build_train_batch_device + train_chunks + Adam on labels never used before -- K label sets drawn up
        front with the reference's transforms (time reversal p = 0.5, detection dropout p = 0.2), cycled after warm-up draws;
        reported with its split: the build, the plans the first forward builds on every new graph (edge_tiles / win_plan /
        dense_seg_plan: the first step on a batch minus a second step on it) and the step with those plans cached

Each step is timed on its own (device synchronised on both sides) after `--warmup` untimed steps; the line reports the median and
the spread over `--steps` steps, graph-edges/s and the ratio (b) / (a).

    python tools/train_batch_bench.py --steps 10 --warmup 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return np.asarray(ms)


def timed_pair(fn_a, fn_b, steps, warmup):
    """fn_a and fn_b alternating step by step, each step timed on its own."""
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(steps):
        for k, fn in enumerate((fn_a, fn_b)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return np.asarray(ms[0]), np.asarray(ms[1])


def summary(ms, edges):
    med = float(np.median(ms))
    return dict(ms_median=round(med, 3), ms_min=round(float(ms.min()), 3), ms_max=round(float(ms.max()), 3),
                graph_edges_per_s=round(edges / med * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=None)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-tp-classifier', action='store_true')
    ap.add_argument('--draws', type=int, default=6, help='(e): label sets drawn up front')
    ap.add_argument('--skip-host-build', action='store_true', help='(c) is not run: (b) trains the device-built batch')
    args = ap.parse_args()
    import bench
    from trackmpnn_amd import TrackMPNN, TrainMonitor, build_train_batch, build_train_batch_device, synth_window
    from trackmpnn_amd.loops import train_chunk, train_chunks
    dev = torch.device('cuda', 0)
    w = bench.WORKLOADS['c2']
    B = int(args.windows or w['windows'])
    wl = bench.make_workload('c2', 0, dev, windows=B)                   # (a): rank 0 draws seed 1
    ms_a = timed(wl['step'], args.steps, args.warmup)
    edges_a = wl['edge_iters']
    # (b): the same chunks (bench.build_batch's windows: seeds 1000 + s, tiled)
    distinct = min(B, 64)
    ys = [synth_window(1000 + s, w['frames'], w['mean_dets'], w['max_dets']) for s in range(distinct)]
    ys = (ys * ((B + distinct - 1) // distinct))[:B]
    build_s = None
    if not args.skip_host_build:
        t0 = time.perf_counter()
        batch = build_train_batch(ys, dev)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
    # (d): the same chunks built on the device, from the stacked form (what a collate gives) and from the list form
    off = np.concatenate([[0], np.cumsum([y.shape[0] for y in ys])])
    y_d, off_d = torch.from_numpy(np.concatenate(ys)).to(dev), torch.from_numpy(off).to(dev)
    built = {}

    def build_d():
        built['b'] = build_train_batch_device(y_d, dev, offsets=off_d)

    ms_d = timed(build_d, args.steps, args.warmup)
    ms_d_list = timed(lambda: build_train_batch_device(ys, dev), max(args.steps // 2, 1), 1)
    if args.skip_host_build:
        batch = built['b']
    F = w['ncat'] + 5
    Xs = torch.randn(batch.n_feat, F, generator=torch.Generator().manual_seed(1)).to(dev)
    torch.manual_seed(5)
    model = TrackMPNN('2d', w['ncat'], w['H'], 0, 'diff').to(dev).train()
    opt = bench.make_adam(model)
    tp = not args.no_tp_classifier
    out = {}

    def step_b():
        opt.zero_grad(set_to_none=False)
        out['r'] = train_chunks(model, batch, Xs, tp)
        opt.step()

    mon = TrainMonitor(dev)

    def step_bm():
        opt.zero_grad(set_to_none=False)
        train_chunks(model, batch, Xs, tp, monitor=mon)
        opt.step()

    ms_b, ms_bm = timed_pair(step_b, step_bm, args.steps, args.warmup)
    loss, per_chunk, ncalls, edges_b = out['r']
    stats = mon.read()
    listed_rows = int(sum(w.n_det + w.n_edge for w in batch.windows))
    # batch 1: one C2 chunk through train_chunk, with and without a monitor
    y1 = torch.from_numpy(ys[0])[None]
    X1 = Xs[:ys[0].shape[0]][None].cpu()
    mon1 = TrainMonitor(dev)

    def chunk(m):
        opt.zero_grad(set_to_none=False)
        train_chunk(model, X1, y1, dev, tp, monitor=m)

    ms_c, ms_cm = timed_pair(lambda: chunk(None), lambda: chunk(mon1), max(args.steps, 20), max(args.warmup, 5))
    # (e): fresh batches -- K transformed label sets drawn up front (device-resident, as a collate hands them over)
    rng = np.random.RandomState(7)

    def draw():
        out_ys = []
        for y in ys:
            y = y.copy()
            if rng.rand() < 0.5:
                y[:, 0] = y[:, 0].max() - y[:, 0] + y[:, 0].min()
            out_ys.append(y[rng.rand(y.shape[0]) >= 0.2])
        o = np.concatenate([[0], np.cumsum([y.shape[0] for y in out_ys])])
        X = torch.randn(int(o[-1]), F, generator=torch.Generator().manual_seed(len(o))).to(dev)
        return torch.from_numpy(np.concatenate(out_ys)).to(dev), torch.from_numpy(o).to(dev), X

    sets = [draw() for _ in range(max(args.draws, 2))]
    split = {'build': [], 'plans': [], 'step': []}
    cyc = {'i': 0}

    def step_e(record=False):
        yy, oo, X = sets[cyc['i'] % len(sets)]
        cyc['i'] += 1
        t0 = time.perf_counter()
        fb = build_train_batch_device(yy, dev, offsets=oo)
        if record:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        opt.zero_grad(set_to_none=False)
        train_chunks(model, fb, X, tp)
        opt.step()
        if record:
            # the same step again on the same batch: its graphs' plans are cached now, so the difference is their first build
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            opt.zero_grad(set_to_none=False)
            train_chunks(model, fb, X, tp)
            opt.step()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            split['build'].append((t1 - t0) * 1e3)
            split['plans'].append(((t2 - t1) - (t3 - t2)) * 1e3)
            split['step'].append((t3 - t2) * 1e3)

    ms_e = timed(step_e, args.steps, max(args.warmup, len(sets)))
    for _ in range(len(sets)):
        step_e(record=True)
    a, b = summary(ms_a, edges_a), summary(ms_b, edges_b)
    bm = summary(ms_bm, edges_b)
    rng_b = round(float(ms_b.max() - ms_b.min()), 3)
    delta = round(bm['ms_median'] - b['ms_median'], 3)
    med = lambda v: round(float(np.median(v)), 4)
    print(json.dumps(dict(
        workload=f"C2: {B} windows (64 distinct seeds tiled), {w['frames']} frames, H={w['H']}, K=0, diff",
        steps=args.steps, warmup=args.warmup, tp_classifier=tp,
        a_headline_bce_step=a, b_train_chunks_real_losses_step=b,
        b_prime_with_monitor_step=bm | dict(
            listed_rows_R=listed_rows, counted_bytes_9R=9 * listed_rows, delta_median_ms=delta, range_of_b_ms=rng_b,
            verdict='not resolvable, <= range of (b)' if abs(delta) <= rng_b else 'outside the range of (b)',
            monitor={k: (round(v, 6) if isinstance(v, float) else v) for k, v in stats.items()}),
        train_chunk_c2_ms=dict(plain_median=med(ms_c), plain_min=round(float(ms_c.min()), 4), plain_max=round(float(ms_c.max()), 4),
                               monitor_median=med(ms_cm), monitor_min=round(float(ms_cm.min()), 4),
                               monitor_max=round(float(ms_cm.max()), 4)),
        c_host_build_s=None if build_s is None else round(build_s, 3),
        d_device_build_ms=summary(ms_d, 0) | dict(list_form_ms_median=round(float(np.median(ms_d_list)), 3)),
        e_fresh_batch_step=summary(ms_e, edges_b) | dict(draws=len(sets), split_ms_median={
            k: round(float(np.median(v)), 3) for k, v in split.items()}),
        ratio_b_over_a=round(b['ms_median'] / a['ms_median'], 4),
        edge_iterations=dict(a=int(edges_a), b=int(edges_b)), chunks=batch.B, calls=len(batch.plans), chunk_calls=int(ncalls),
        loss_per_chunk_mean=round(float(loss.detach()) / batch.B, 4), finite=bool(torch.isfinite(per_chunk).all()),
        device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
