"""The end of a training step, timed on the MI355X: torch's Adam + `bucket.zero()` against `BucketAdam.step(zero_grads=True)`.

One process, the variants alternating, device events around `--steps` steps each after a warm-up, `--reps` repetitions, median
and spread (min .. max) per variant; for the H = 64, K = 0 diff model (~55 k parameters) and an H = 256 model (~860 k):
  (a) torch.optim.Adam(fused=True) where this torch offers it (bench.make_adam's choice) + bucket.zero()
  (b) torch.optim.Adam, default form + bucket.zero()
  (c) BucketAdam.step(zero_grads=True)                      -- one launch (tmpnn_adam_step)
and the replay of one captured C2 window (fixture roll_c2_kitti_car_w5: forward calls + loss + backward + optimizer in one
hipGraph, as tools/c1_latency.py builds it) with a capturable torch Adam against BucketAdam.
A step's time here is what a loop of steps costs per step (host enqueue or device, whichever is longer); `host` is the time to
enqueue alone.  (a) measured in the same run is the yardstick for (c).

    python tools/optim_bench.py [--steps 1000] [--reps 5] [--out profiles/optim_step.md]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/optim_bench.py --trace-steps 100      # one kernel per step

Needs a GPU (there is no CPU path)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

DEV = 'cuda:0'


def _model(nhidden):
    from trackmpnn_amd import TrackMPNN
    from trackmpnn_amd.dist import GradBucket
    torch.manual_seed(5)
    model = TrackMPNN('2d', 3, nhidden, 0, 'diff').to(DEV).train()
    bucket = GradBucket(model)
    bucket.flat.copy_(1e-3 * torch.randn(bucket.flat.numel(), device=DEV))
    return model, bucket


def _variants(nhidden):
    """[(label, step end)] -- each on its own model and bucket."""
    import bench
    from trackmpnn_amd import BucketAdam
    out = []
    model, bucket = _model(nhidden)
    opt_a = bench.make_adam(model)
    fused = bool(opt_a.param_groups[0].get('fused'))

    def end_a(opt=opt_a, bucket=bucket):
        opt.step()
        bucket.zero()

    out.append((f'(a) torch Adam{" (fused=True)" if fused else ", default form (no fused form here)"} + bucket.zero()', end_a))
    model, bucket = _model(nhidden)
    opt_b = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-4)

    def end_b(opt=opt_b, bucket=bucket):
        opt.step()
        bucket.zero()

    out.append(('(b) torch Adam, default form + bucket.zero()', end_b))
    model, bucket = _model(nhidden)
    opt_c = BucketAdam(model, bucket, lr=1e-4, weight_decay=5e-4)
    out.append(('(c) BucketAdam.step(zero_grads=True)', lambda opt=opt_c: opt.step(zero_grads=True)))
    return out, bucket.flat.numel()


def _time(fn, steps):
    """(ms per step by device events around `steps` calls, ms per step of host enqueue)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, host * 1e3 / steps


def _alternate(variants, steps, reps, warmup):
    res = {label: ([], []) for label, _ in variants}
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    for _ in range(reps):
        for label, fn in variants:
            dev, host = _time(fn, steps)
            res[label][0].append(dev)
            res[label][1].append(host)
    return res


def _row(label, dev, host):
    return (f'| {label} | {statistics.median(dev) * 1e3:.1f} | {min(dev) * 1e3:.1f} .. {max(dev) * 1e3:.1f} | '
            f'{statistics.median(host) * 1e3:.1f} |')


def _captured(steps, reps):
    from tests.golden_util import Golden
    from tests.test_parity_gpu import build_model
    from trackmpnn_amd import BucketAdam, CapturedWindow
    from trackmpnn_amd.dist import GradBucket
    gold = Golden('roll_c2_kitti_car_w5')
    loss_fn = lambda outs, h: torch.cat([l for _, l in outs]).sum()      # noqa: E731
    variants = []
    keep = []
    for kind in ('torch', 'bucket'):
        model = build_model(gold.meta, gold.params())
        bucket = GradBucket(model)
        calls = []
        for c in range(gold.ncalls):
            na, ea = gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV)
            if not na.is_sparse:
                na, ea = na.to_sparse(), ea.to_sparse()
            calls.append((gold.t(f'c{c}/x').to(DEV), na, ea))
        if kind == 'torch':
            opt = torch.optim.Adam(model.parameters(), lr=1e-5, weight_decay=5e-4, capturable=True)
            label = 'captured C2 window, torch Adam (capturable=True)'
        else:
            opt = BucketAdam(model, bucket, lr=1e-5, weight_decay=5e-4)
            label = 'captured C2 window, BucketAdam'
        win = CapturedWindow(model, calls, loss_fn, optimizer=opt, bucket=bucket)
        keep.append((model, bucket, opt, win))
        variants.append((label, win.replay))
    return _alternate(variants, steps, reps, warmup=10)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--out', default=None, help='also write the tables to this file')
    ap.add_argument('--trace-steps', type=int, default=0,
                    help='run only this many BucketAdam steps after ONE warm-up step (for a kernel trace) and exit')
    ap.add_argument('--no-captured', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/optim_bench.py needs a GPU: trackmpnn_amd has no CPU path and nothing is timed without one')
    import __graft_entry__
    __graft_entry__.build()
    if args.trace_steps:
        from trackmpnn_amd import BucketAdam
        model, bucket = _model(64)
        opt = BucketAdam(model, bucket, lr=1e-4, weight_decay=5e-4)
        for _ in range(1 + args.trace_steps):
            opt.step(zero_grads=True)
        torch.cuda.synchronize()
        print(f'[optim_bench] {1 + args.trace_steps} BucketAdam steps issued (expect as many k_adam_step dispatches)')
        return
    lines = [f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.steps} steps per measurement, '
             f'{args.reps} repetitions, variants alternating; times in microseconds per step', '']
    for nhidden in (64, 256):
        variants, n = _variants(nhidden)
        res = _alternate(variants, args.steps, args.reps, args.warmup)
        lines += [f'H = {nhidden}, {n} parameters', '',
                  '| step end | median us | min .. max us | host enqueue us (median) |', '|---|---|---|---|']
        lines += [_row(label, *res[label]) for label, _ in variants]
        lines.append('')
    if not args.no_captured:
        res = _captured(max(args.steps // 2, 1), args.reps)
        lines += ['captured window (whole step: forward calls + loss + backward + optimizer, one hipGraph launch)', '',
                  '| replay | median us | min .. max us | host enqueue us (median) |', '|---|---|---|---|']
        lines += [_row(label, *v) for label, v in res.items()]
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
