"""Batched chunk training with the reference's losses against the headline step, on the batch bench.py builds (C2: B = 16384
windows, 64 distinct seeds tiled).

    (a) bench.step: every call of the batch, BCE with logits over all logits against fixed targets, one backward, Adam
    (b) trackmpnn_amd.loops.train_chunks + Adam: the same calls with create_targets + CELoss + FocalLoss per chunk and call
        (one windowed loss launch per call each way), one backward -- the losses inside the timed region
    (c) the host build of (b)'s batch (build_train_batch: graphs, labels, loss windows, feature sources; once per set of chunks)

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
    args = ap.parse_args()
    import bench
    from trackmpnn_amd import TrackMPNN, build_train_batch, synth_window
    from trackmpnn_amd.loops import train_chunks
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
    t0 = time.perf_counter()
    batch = build_train_batch(ys, dev)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
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

    ms_b = timed(step_b, args.steps, args.warmup)
    loss, per_chunk, ncalls, edges_b = out['r']
    a, b = summary(ms_a, edges_a), summary(ms_b, edges_b)
    print(json.dumps(dict(
        workload=f"C2: {B} windows (64 distinct seeds tiled), {w['frames']} frames, H={w['H']}, K=0, diff",
        steps=args.steps, warmup=args.warmup, tp_classifier=tp,
        a_headline_bce_step=a, b_train_chunks_real_losses_step=b,
        c_host_build_s=round(build_s, 3),
        ratio_b_over_a=round(b['ms_median'] / a['ms_median'], 4),
        edge_iterations=dict(a=int(edges_a), b=int(edges_b)), chunks=batch.B, calls=len(batch.plans), chunk_calls=int(ncalls),
        loss_per_chunk_mean=round(float(loss.detach()) / batch.B, 4), finite=bool(torch.isfinite(per_chunk).all()),
        device=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
