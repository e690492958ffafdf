#!/usr/bin/env python
"""Time of the embedding CNN on the device against the path a user had before it: the same forward as torch eager ops.

    python tools/espnet_bench.py [--T 1 8] [--H 384 --W 1280 --C 128] [--steps 30 --warmup 5] [--json PATH]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/espnet_bench.py --trace --T 1
    python tools/espnet_bench.py --centres [--T 1 8] [--dets-per-image 16] [--json PATH]
    python tools/espnet_bench.py --hashes

device      EspEmbedNet(images): 70 launches of csrc/espnet.hip on the current stream
eager       espnet_host(sd, images, torch.float32) with the state dict on the device: torch ops, convolutions through MIOpen,
            timed after its own warm-up (MIOpen searches an algorithm per shape in the first calls)
Both are timed with device events around `steps` back-to-back calls, after `warmup` calls of the same shape, and the two outputs
are compared at the size that is timed (--check64: each also with the float64 forward on the CPU).  Weights:
tests/espnet_cases.espnet_weights(C, 1).  --trace runs the device path alone (3 warm-up calls, `steps` timed ones) for a kernel
trace: the launch count per call is the trace's dispatches over the calls.
--centres   the inference pair behind the visual head, per T with D = T x dets-per-image seeded boxes: net(images) +
            head.rows(maps, ...) (70 + 2 launches) against net.centres(images) + head.rows(handle, ...) (65 + 3), the rows
            compared bit for bit, with the workspace and result bytes of both paths; then, for the fixtures under
            tests/golden/espnet, the error of logits_at at every pixel over the reference's own float32 error
--hashes    sha256 of net(images) for those fixtures: the record that the dense maps keep their bits across a change
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


def fixture_hashes(dev):
    """name -> sha256 of the dense maps' bytes, for the five recorded fixtures."""
    import hashlib
    from tests.espnet_cases import CASES, load_case
    out = {}
    for name in CASES:
        fx, sd = load_case(name)
        maps = EspEmbedNet.from_state_dict(sd, dev)(torch.from_numpy(fx['images']).to(dev))
        out[name] = hashlib.sha256(maps.cpu().numpy().tobytes()).hexdigest()
    return out


def centres_rows(args, dev):
    import numpy as np
    from tests.espnet_cases import CASES, load_case
    from trackmpnn_amd import VisHead, _lib
    sd = espnet_weights(args.C, 1)
    net = EspEmbedNet.from_state_dict(sd, dev)
    rng = np.random.default_rng(0)
    head = VisHead((args.H, args.W), 1, np.zeros(128, np.float32), np.ones(128, np.float32), dev)
    rows = []
    for T in args.T:
        D = T * args.dets_per_image
        images = torch.randn((T, 3, args.H, args.W), generator=torch.Generator().manual_seed(T)).to(dev)
        cx, cy = rng.uniform(0, args.W, D), rng.uniform(0, args.H, D)
        box = torch.from_numpy(np.stack([cx - 20, cy - 30, cx + 20, cy + 30], 1).astype(np.float32)).to(dev)
        map_of = torch.from_numpy(np.repeat(np.arange(T), args.dets_per_image).astype(np.int32)).to(dev)
        im_hw = (args.H, args.W)
        out = torch.empty((T, args.C, args.H, args.W), dtype=torch.float32, device=dev)
        x_dense = torch.zeros((D, 128), dtype=torch.float32, device=dev)
        x_sparse = torch.zeros_like(x_dense)

        def dense():
            head.rows(net(images, out=out), box, map_of, im_hw, out=x_dense)

        def sparse():
            head.rows(net.centres(images), box, map_of, im_hw, out=x_sparse)

        ms_dense = timed(dense, args.steps, args.warmup)
        ms_sparse = timed(sparse, args.steps, args.warmup)
        ms_net = timed(lambda: net(images, out=out), args.steps, args.warmup)
        ms_trunk = timed(lambda: net.centres(images), args.steps, args.warmup)
        same = bool(torch.equal(x_dense.view(torch.int32), x_sparse.view(torch.int32)))
        ws_d = int(_lib.fn('tmpnn_espnet_ws_bytes')(T, args.H, args.W, args.C))
        ws_s = int(_lib.fn('tmpnn_espnet_centres_ws_bytes')(T, args.H, args.W, args.C))
        row = dict(T=T, D=D, C=args.C, H=args.H, W=args.W, dense_ms=round(ms_dense, 4), centres_ms=round(ms_sparse, 4),
                   saved_us=round(1e3 * (ms_dense - ms_sparse), 1), net_ms=round(ms_net, 4), trunk_ms=round(ms_trunk, 4),
                   rows_equal_bitwise=same, dense_bytes=dict(workspace=ws_d, result=out.numel() * 4),
                   centres_bytes=dict(workspace=ws_s, result=D * args.C * 4), steps=args.steps, warmup=args.warmup)
        rows.append(row)
        print(json.dumps(row), flush=True)
        head.release()
        del out, images
    for name, (T, C, H, W, _) in CASES.items():
        fx, fsd = load_case(name)
        fnet = EspEmbedNet.from_state_dict(fsd, dev)
        pix = torch.arange(T * H * W, dtype=torch.int32, device=dev)
        logits, _ = fnet.centres(torch.from_numpy(fx['images']).to(dev)).logits_at(pix)
        ref = fx['ref_out64'].transpose(0, 2, 3, 1).reshape(T * H * W, C)
        e_ref = float(np.abs(fx['ref_out32'].astype(np.float64) - fx['ref_out64']).max())
        err = float(np.abs(logits.cpu().numpy().astype(np.float64) - ref).max())
        row = dict(fixture=name, e_ref=e_ref, centres_err=err, ratio=round(err / e_ref, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


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
    ap.add_argument('--centres', action='store_true', help='net + head.rows against net.centres + head.rows')
    ap.add_argument('--dets-per-image', type=int, default=16)
    ap.add_argument('--hashes', action='store_true', help='sha256 of the dense maps of the recorded fixtures')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('espnet_bench: no GPU (a timing needs the MI355X)')
    dev = torch.device('cuda:0')
    if args.hashes or args.centres:
        rows = []
        if args.centres:
            rows += centres_rows(args, dev)
        if args.hashes:
            rows.append(dict(hashes=fixture_hashes(dev)))
            print(json.dumps(rows[-1]), flush=True)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, 'w') as f:
                json.dump(rows, f, indent=1)
        return
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
