#!/usr/bin/env python
"""Time one training step of the embedding CNN's decoder: forward + backward + Adam step (run by hand; nothing asserts a time).

    python tools/espnet_train_bench.py [--C 128] [--hw 384 1280] [--T 1 8] [--steps 10] [--repeats 5] [--scope tail [decoder]]
                                       [--only device|torch]

device      EspTrainNet + GradBucket + BucketAdam: the library's path (70 forward launches, 1 refold, 13 backward launches -- 48
            with scope='decoder' --, 1 Adam launch and the bucket's zero fill per step, whatever T is); one path per --scope
            given, named `device` for the tail and `device/decoder` for the whole decoder
torch       the path a user had before: espnet_host's ops in float32 on the device with autograd on the trained tensors of the
            last --scope given and torch.optim.Adam (the encoder runs without a graph in all)
d_maps is what VisHead's backward hands over: 16 centres per frame, every other pixel zero.  Seeded weights (tests/espnet_cases.py),
random images.  Per T the paths alternate `repeats` times; each measurement is device events around `steps` back-to-back steps
after a warm-up of 3.  Prints one line per measurement and a JSON summary (median and range in ms per step).  --only runs one path
alone (for a kernel trace of its own).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.espnet_cases import espnet_weights                                   # noqa: E402
from trackmpnn_amd import BucketAdam, EspTrainNet                                # noqa: E402
from trackmpnn_amd.dist import GradBucket                                        # noqa: E402
from trackmpnn_amd.espnet import _host_forward, trained_param_names              # noqa: E402

LR, WD = 5e-4, 5e-4           # the reference's embedding optimizer


def sparse_d_maps(T, C, H, W, dev, seed=0):
    rng = np.random.default_rng(seed)
    d = torch.zeros((T, C, H, W), dtype=torch.float32)
    for t in range(T):
        for p in rng.choice(H * W, 16, replace=False):
            d[t, :, p // W, p % W] = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    return d.to(dev)


def device_step(sd, images, d, dev, scope='tail'):
    net = EspTrainNet.from_state_dict(sd, dev, scope=scope)
    bucket = GradBucket(net)
    opt = BucketAdam(net, bucket, lr=LR, weight_decay=WD)

    def step():
        opt.zero_grad()
        net(images).backward(d)
        opt.step()
    return step


def torch_step(sd, images, d, dev, scope='tail'):
    names = trained_param_names(int(sd['project_l3.1.conv.weight'].shape[0]), scope)
    frozen = {k: v.to(dev) for k, v in sd.items() if k not in names and v.dtype.is_floating_point}
    leaves = {k: torch.nn.Parameter(sd[k].to(dev)) for k in names}
    opt = torch.optim.Adam(list(leaves.values()), LR, weight_decay=WD)

    def g(k):
        return leaves[k] if k in leaves else frozen[k]

    def step():
        opt.zero_grad()
        out, _ = _host_forward(g, images)
        out.backward(d)
        opt.step()
    return step


def measure(step, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--C', type=int, default=128)
    ap.add_argument('--hw', type=int, nargs=2, default=(384, 1280))
    ap.add_argument('--T', type=int, nargs='+', default=(1, 8))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--scope', nargs='+', choices=('tail', 'decoder'), default=('tail',))
    ap.add_argument('--only', choices=('device', 'torch'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    H, W = args.hw
    sd = espnet_weights(args.C, 107)
    summary = {}
    for T in args.T:
        images = torch.randn((T, 3, H, W), generator=torch.Generator().manual_seed(T)).to(dev)
        d = sparse_d_maps(T, args.C, H, W, dev)
        paths = {}
        if args.only in (None, 'device'):
            for scope in args.scope:
                paths['device' if scope == 'tail' else 'device/' + scope] = device_step(sd, images, d, dev, scope)
        if args.only in (None, 'torch'):
            paths['torch'] = torch_step(sd, images, d, dev, args.scope[-1])
        for step in paths.values():
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for r in range(args.repeats):
            for k, step in paths.items():
                ms = measure(step, args.steps)
                times[k].append(ms)
                print(f'T={T} {k} repeat {r}: {ms:.3f} ms / step', flush=True)
        summary[f'T={T}'] = {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in times.items()}
        del paths
        torch.cuda.empty_cache()
    print(json.dumps(dict(C=args.C, H=H, W=W, steps=args.steps, repeats=args.repeats, scope=list(args.scope), ms_per_step=summary)))


if __name__ == '__main__':
    main()
