#!/usr/bin/env python
"""Time of the embedding CNN on the device against the path a user had before it: the same forward as torch eager ops.

    python tools/espnet_bench.py [--T 1 8] [--H 384 --W 1280 --C 128] [--steps 30 --warmup 5] [--json PATH]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/espnet_bench.py --trace --T 1

device      EspEmbedNet(images): 70 launches of csrc/espnet.hip on the current stream
eager       espnet_host(sd, images, torch.float32) with the state dict on the device: torch ops, convolutions through MIOpen,
            timed after its own warm-up (MIOpen searches an algorithm per shape in the first calls)
Both are timed with device events around `steps` back-to-back calls, after `warmup` calls of the same shape, and the two outputs
are compared at the size that is timed (--check64: each also with the float64 forward on the CPU).  Weights:
tests/espnet_cases.espnet_weights(C, 1).  --trace runs the device path alone (3 warm-up calls, `steps` timed ones) for a kernel
trace: the launch count per call is the trace's dispatches over the calls.
Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.espnet_cases import espnet_weights          # noqa: E402
from trackmpnn_amd import EspEmbedNet, espnet_host     # noqa: E402

LAUNCHES = 70


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--H', type=int, default=384)
    ap.add_argument('--W', type=int, default=1280)
    ap.add_argument('--C', type=int, default=128)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trace', action='store_true', help='the device path alone, for rocprofv3')
    ap.add_argument('--check64', action='store_true', help='also compare both paths with espnet_host in float64 on the CPU (first T)')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('espnet_bench: no GPU (a timing needs the MI355X)')
    dev = torch.device('cuda:0')
    sd = espnet_weights(args.C, 1)
    net = EspEmbedNet.from_state_dict(sd, dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    rows = []
    for T in args.T:
        images = torch.randn((T, 3, args.H, args.W), generator=torch.Generator().manual_seed(T)).to(dev)
        out = torch.empty((T, args.C, args.H, args.W), dtype=torch.float32, device=dev)
        if args.trace:
            ms = timed(lambda: net(images, out=out), args.steps, 3)
            print(f'T={T}: device {ms:.3f} ms per call under the tracer, {args.steps + 3} calls of {LAUNCHES} launches')
            continue
        up_bytes = T * args.C * args.H * args.W * 4 * (1 + 0.25)              # the final x2: one read of the half-size map, one write
        ms_dev = timed(lambda: net(images, out=out), args.steps, args.warmup)
        with torch.no_grad():
            ref = espnet_host(sd_dev, images, torch.float32)
            diff = float((out - ref).abs().max())
            peak = float(ref.abs().max())
            err64 = None
            if args.check64 and T == args.T[0]:
                ref64 = espnet_host(sd, images.cpu(), torch.float64)
                err64 = dict(device=float((out.cpu().double() - ref64).abs().max()), eager=float((ref.cpu().double() - ref64).abs().max()))
                del ref64
            del ref
            ms_eager = timed(lambda: espnet_host(sd_dev, images, torch.float32), max(3, args.steps // 3), max(3, args.warmup))
        row = dict(T=T, C=args.C, H=args.H, W=args.W, device_ms=round(ms_dev, 4), eager_ms=round(ms_eager, 4),
                   speedup=round(ms_eager / ms_dev, 2), launches=LAUNCHES, max_abs_diff=diff, max_abs_out=peak,
                   final_upsample_bytes=int(up_bytes), steps=args.steps, warmup=args.warmup)
        if err64 is not None:
            row['max_abs_err_vs_float64'] = err64
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
