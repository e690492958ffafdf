"""Time of the visual head on the device next to the reference's own form of the same step, on the same device and inputs.

    python tools/vis_head_bench.py --out profiles/vis_head_run.md
    python tools/vis_head_bench.py --trace 50          # VisHead steps alone, per shape: the program to put under rocprofv3 --kernel-trace --stats

Shapes: KITTI chunks of 7 frames with 8 .. 16 detections a frame (about 12), one map of 128 x 96 x 320 per frame (384 x 1280 input
at down_ratio 4, images of 375 x 1242); (a) one chunk, (b) a batch of 64 chunks (448 maps).  A quarter of the detections are false
positives (-1), ids go up to 399.

In ONE process, per shape, alternating:

  (ref)   the reference's form restated with torch ops: one `map[:, :, cy, cx]` per detection (the pixels from vis_centres_host,
          all at once: the reference's per-box index arithmetic in Python is NOT charged to it), torch.cat, per chunk a cross
          entropy over the labels `id % 128` with -1 ignored, softmax and the standardisation; backward = the losses' sum
          .backward() into the per-frame maps (each frame's map is a tensor of its own, as the CNN hands them out)
  (dev)   VisHead.forward (two launches) and loss.sum().backward() (a memset of dmaps and one launch)

Forward and backward are timed apart with device events (the reference's loop is bound by its launches, so its device-timeline
time is its wall time).  A timed window holds --inner calls of VisHead (20: a single call is under 0.1 ms) and --inner / 4 of
the reference form on one chunk, one on the batch; the figures are ms per call, medians over the windows after a warm-up.  The two forms' losses and map gradients are compared on
every shape.  Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IM_HW, INPUT_HW, DOWN, MAP_HW = (375, 1242), (384, 1280), 4, (96, 320)
FRAMES = 7


def build(chunks, seed=5):
    """box [D, 4], map_of [D], track [D], offsets [chunks + 1] of `chunks` chunks of FRAMES frames."""
    rng = np.random.default_rng(seed)
    per_frame = rng.integers(8, 17, chunks * FRAMES)
    D = int(per_frame.sum())
    x = np.sort(rng.uniform(0, IM_HW[1] - 1, (D, 2)), axis=1)
    y = np.sort(rng.uniform(0, IM_HW[0] - 1, (D, 2)), axis=1)
    box = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)
    map_of = np.repeat(np.arange(chunks * FRAMES), per_frame).astype(np.int64)
    track = rng.integers(0, 400, D)
    track[rng.random(D) < 0.25] = -1
    first = np.concatenate([[0], np.cumsum(per_frame)])
    return box, map_of, track.astype(np.int64), first[::FRAMES].astype(np.int64), first


def reference_step(torch, frame_maps, box, first, track, offsets, mean, std):
    """The per-detection form: (rows, losses [B]) with autograd into frame_maps.  The pixel of every detection comes from
    vis_centres_host (pinned equal to the reference's index by tests/test_vis_head.py); what is kept of the reference's form is
    what costs the time: one indexing kernel per detection, one concatenation, one cross entropy per chunk."""
    from trackmpnn_amd.vishead import vis_centres_host
    cy, cx = vis_centres_host(box, IM_HW, INPUT_HW, DOWN)
    frame_of = np.repeat(np.arange(len(frame_maps)), np.diff(first))
    vis = torch.cat([frame_maps[t][:, :, y, x] for t, y, x in zip(frame_of.tolist(), cy.tolist(), cx.tolist())], 0)
    labels = torch.from_numpy(np.where(track >= 0, track % 128, -100)).to(vis.device)
    bounds = offsets.tolist()
    losses = [torch.nn.functional.cross_entropy(vis[lo:hi], labels[lo:hi], ignore_index=-100) for lo, hi in zip(bounds[:-1], bounds[1:])]
    rows = ((torch.softmax(vis, dim=1) - mean) / std).detach()
    return rows, torch.stack(losses)


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
    ap.add_argument('--reps', type=int, default=7, help='timed windows per figure')
    ap.add_argument('--inner', type=int, default=20, help='VisHead calls per timed window')
    ap.add_argument('--trace', type=int, default=0, help='run this many VisHead steps per shape and nothing else')
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('vis_head_bench needs the MI355X: no timing is taken without it')
    from trackmpnn_amd import VisHead
    dev = 'cuda:0'
    mean, std = np.full(128, 0.5, np.float32), np.full(128, 0.5, np.float32)
    mean_d, std_d = torch.from_numpy(mean).to(dev), torch.from_numpy(std).to(dev)
    head = VisHead(INPUT_HW, DOWN, mean, std, dev)
    text = []
    for B in [int(v) for v in a.chunks.split(',')]:
        box, map_of, track, offsets, first = build(B)
        D, T = box.shape[0], B * FRAMES
        gen = torch.Generator(device=dev).manual_seed(B)
        maps = (2.0 * torch.randn((T, 128) + MAP_HW, generator=gen, device=dev)).requires_grad_()
        box_d, map_d = torch.from_numpy(box).to(dev), torch.from_numpy(map_of).to(dev).to(torch.int32)
        track_d, off_d = torch.from_numpy(track).to(dev).to(torch.int32), torch.from_numpy(offsets).to(dev).to(torch.int32)

        def dev_fwd():
            return head.forward(maps, box_d, map_d, IM_HW, track_d, off_d)

        def dev_bwd(loss):
            maps.grad = None
            loss.sum().backward()

        if a.trace:
            for _ in range(a.trace):
                dev_bwd(dev_fwd()[1])
            torch.cuda.synchronize()
            print(json.dumps(dict(tool='vis_head_bench', mode='trace', steps=a.trace, chunks=B, detections=D, maps=T)))
            del maps
            torch.cuda.empty_cache()
            continue
        frame_maps = [maps[t:t + 1].detach().clone().requires_grad_() for t in range(T)]

        def ref_fwd():
            return reference_step(torch, frame_maps, box, first, track, offsets, mean_d, std_d)

        def ref_bwd(loss):
            for fm in frame_maps:
                fm.grad = None
            loss.sum().backward()

        t = {'dev_fwd': [], 'dev_bwd': [], 'ref_fwd': [], 'ref_bwd': []}
        n_dev, n_ref = a.inner, (max(1, a.inner // 4) if B == 1 else 1)
        for r in range(a.reps + 1):                               # (window 0 warms up; the two forms alternate)
            outs, f_ms = timed(torch, lambda: [dev_fwd() for _ in range(n_dev)])
            _, b_ms = timed(torch, lambda: [dev_bwd(o[1]) for o in outs])
            routs, rf_ms = timed(torch, lambda: [ref_fwd() for _ in range(n_ref)])
            _, rb_ms = timed(torch, lambda: [ref_bwd(o[1]) for o in routs])
            if r:
                for k, v in zip(('dev_fwd', 'dev_bwd', 'ref_fwd', 'ref_bwd'), (f_ms / n_dev, b_ms / n_dev, rf_ms / n_ref, rb_ms / n_ref)):
                    t[k].append(v)
        (rows, loss), (rrows, rloss) = outs[-1], routs[-1]
        del outs, routs
        # the two forms agree (float32 both; a chunk always has a labelled row here)
        d_loss = float(((loss.detach() - rloss.detach()).abs() / rloss.detach().abs()).max())
        d_rows = float((rows - rrows).abs().max())
        d_grad = max(float((maps.grad[i] - fm.grad[0]).abs().max()) for i, fm in enumerate(frame_maps) if fm.grad is not None)
        assert d_loss < 1e-5 and d_rows < 1e-5 and d_grad < 1e-6, (d_loss, d_rows, d_grad)
        rec = head.record()
        m = {k: float(np.median(v)) for k, v in t.items()}
        text += [f'### {B} chunk{"s" if B > 1 else ""}', '',
                 f'{T} maps of 128 x {MAP_HW[0]} x {MAP_HW[1]} ({maps.numel() * 4 / 2 ** 20:.0f} MiB), {D} detections '
                 f'({int(rec["labelled"].sum())} labelled, {int(rec["clamped"].sum())} clamped); ms per call, medians of {a.reps} windows of {n_dev} calls (reference form: {n_ref}) after '
                 f'one warm-up window, device events; agreement of the two forms: loss rel {d_loss:.2g}, rows abs {d_rows:.2g}, map gradient abs '
                 f'{d_grad:.2g}.', '',
                 '| | reference form, ms | VisHead, ms | ratio |', '|---|---|---|---|',
                 f'| forward (rows + loss) | {m["ref_fwd"]:.3f} | {m["dev_fwd"]:.3f} | {m["ref_fwd"] / m["dev_fwd"]:.0f}x |',
                 f'| backward (d loss / d maps) | {m["ref_bwd"]:.3f} | {m["dev_bwd"]:.3f} | {m["ref_bwd"] / m["dev_bwd"]:.0f}x |',
                 f'| both | {m["ref_fwd"] + m["ref_bwd"]:.3f} | {m["dev_fwd"] + m["dev_bwd"]:.3f} | '
                 f'{(m["ref_fwd"] + m["ref_bwd"]) / (m["dev_fwd"] + m["dev_bwd"]):.0f}x |', '']
        print(json.dumps(dict(tool='vis_head_bench', chunks=B, detections=D, maps=T, device=torch.cuda.get_device_name(0), **m,
                              min_ms={k: float(min(v)) for k, v in t.items()}, max_ms={k: float(max(v)) for k, v in t.items()})))
        del frame_maps, maps
        torch.cuda.empty_cache()
    text = '\n'.join(text)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
