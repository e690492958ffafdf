"""Time of the embedding loss behind the visual head next to the identity loss, on the same device and inputs.

    python tools/embed_loss_bench.py --out profiles/embed_loss_run.md
    python tools/embed_loss_bench.py --trace 50        # loss='embedding' steps alone: the program to put under rocprofv3 --kernel-trace --stats

Shape: the batch of tools/vis_head_bench.py -- KITTI chunks of 7 frames with 8 .. 16 detections a frame (about 84 rows a chunk),
one map of 128 x 96 x 320 per frame, 64 chunks (448 maps, about 5 400 rows) -- and one chunk.  A quarter of the detections are false
positives (-1); a chunk holds 16 track ids, so a cluster has about 4 rows.

In ONE process, per shape, alternating:

  (identity)   VisHead.forward(...) and loss.sum().backward(): 2 launches forward, a memset and 1 launch backward.  This path is
               untouched by the embedding loss (tests/test_vis_embed_gpu.py holds it to tmpnn_vis_head_bwd bit for bit), so it
               is also the figure of the code before the embedding loss existed.
  (embedding)  VisHead.forward(..., loss='embedding') and loss.sum().backward(): the head's 2 launches and the loss's 4 forward;
               the loss's 2 launches, a memset and the scatter's 1 launch backward.
  (loss alone) EmbeddingLoss()(logits, track, offsets) over the logits the head saved, and its backward: 4 + 2 launches.

Forward and backward are timed apart with device events.  A timed window holds --inner calls; the figures are ms per call:
the median, the minimum and the maximum over --reps windows after one warm-up window.  Not bench.py: nothing here gates a
change, and there is no threshold to meet: the identity head is the yardstick."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LAUNCHES = {'identity': '2 / memset + 1', 'embedding': '2 + 4 / 2 + memset + 1', 'loss alone': '4 / 2'}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chunks', default='1,64')
    ap.add_argument('--reps', type=int, default=15, help='timed windows per figure')
    ap.add_argument('--inner', type=int, default=20, help='calls per timed window')
    ap.add_argument('--trace', type=int, default=0, help="run this many loss='embedding' steps per shape and nothing else")
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('embed_loss_bench needs the MI355X: no timing is taken without it')
    from vis_head_bench import FRAMES, IM_HW, INPUT_HW, DOWN, MAP_HW, build
    from trackmpnn_amd import EmbeddingLoss, VisHead
    dev = 'cuda:0'
    half = np.full(128, 0.5, np.float32)
    head, crit = VisHead(INPUT_HW, DOWN, half, half, dev), EmbeddingLoss()
    text = []
    for B in [int(v) for v in a.chunks.split(',')]:
        box, map_of, track, offsets, _ = build(B)
        D, T = box.shape[0], B * FRAMES
        rng = np.random.default_rng(B)
        ids = rng.integers(0, 16, D) + 400 * np.repeat(np.arange(B), np.diff(offsets))
        track = np.where(track >= 0, ids, -1)
        gen = torch.Generator(device=dev).manual_seed(B)
        maps = (0.5 * torch.randn((T, 128) + MAP_HW, generator=gen, device=dev)).requires_grad_()
        box_d, map_d = torch.from_numpy(box).to(dev), torch.from_numpy(map_of).to(dev).to(torch.int32)
        track_d, off_d = torch.from_numpy(track).to(dev).to(torch.int32), torch.from_numpy(offsets).to(dev).to(torch.int32)
        head.forward(maps, box_d, map_d, IM_HW, track_d, off_d)
        logits = head.last_logits().clone().requires_grad_()

        def fwd(kind):
            if kind == 'loss alone':
                return crit(logits, track_d, off_d)
            return head.forward(maps, box_d, map_d, IM_HW, track_d, off_d, loss=kind)[1]

        def bwd(loss):
            maps.grad, logits.grad = None, None
            loss.sum().backward()

        if a.trace:
            for _ in range(a.trace):
                bwd(fwd('embedding'))
            torch.cuda.synchronize()
            print(json.dumps(dict(tool='embed_loss_bench', mode='trace', steps=a.trace, chunks=B, rows=D, maps=T)))
            del maps
            torch.cuda.empty_cache()
            continue
        t = {(k, s): [] for k in LAUNCHES for s in ('fwd', 'bwd')}
        for r in range(a.reps + 1):                               # (window 0 warms up; the forms alternate)
            for kind in LAUNCHES:
                outs, f_ms = timed(torch, lambda: [fwd(kind) for _ in range(a.inner)])
                _, b_ms = timed(torch, lambda: [bwd(o) for o in outs])
                del outs
                if r:
                    t[(kind, 'fwd')].append(f_ms / a.inner)
                    t[(kind, 'bwd')].append(b_ms / a.inner)
        rec = head.embed_record()
        stat = {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}
        cell = lambda k: '{:.3f} ({:.3f} .. {:.3f})'.format(*stat[k])
        text += [f'### {B} chunk{"s" if B > 1 else ""}', '',
                 f'{T} maps of 128 x {MAP_HW[0]} x {MAP_HW[1]} ({maps.numel() * 4 / 2 ** 20:.0f} MiB), {D} rows ({int(rec["labelled"].sum())} labelled, '
                 f'{int(rec["clusters"].sum())} clusters, largest chunk {int(rec["rows"].max())} rows); ms per call: median (minimum .. maximum) of '
                 f'{a.reps} windows of {a.inner} calls after one warm-up window, device events.', '',
                 '| | launches forward / backward | forward, ms | backward, ms |', '|---|---|---|---|']
        text += [f"| {kind} | {LAUNCHES[kind]} | {cell((kind, 'fwd'))} | {cell((kind, 'bwd'))} |" for kind in LAUNCHES] + ['']
        print(json.dumps(dict(tool='embed_loss_bench', chunks=B, rows=D, maps=T, device=torch.cuda.get_device_name(0),
                              ms={f'{k} {s}': v for (k, s), v in stat.items()})))
        del maps, logits
        torch.cuda.empty_cache()
    text = '\n'.join(text)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
