"""The draw of a training step with the visual feature group, and the CNN's input for its frames.

    python tools/chunk_vis_bench.py --B 1024 --reps 20 --out OUT.md

Workload: the C2-shaped set of tools/chunk_draw_bench.py (B sequences of synth_window(7 frames, about 6 detections each), one
chunk per sequence), the reference's transforms.  Device events around each stage (the host's own work lies between the two
events, so it is part of the figure), warm-up excluded, median and min .. max:

  (a) ChunkSampler.draw, '2d+temp'          the plain draw (three launches)
  (b) ChunkSampler.draw, '2d+temp+vis'      the same plus the frame plan on the host, its upload and tmpnn_chunk_draw_vis
  (c) FrameStore.gather                     T images of H x W (KITTI's CNN input: 384 x 1280) from a store of --frames frames, half
                                            of them mirrored: bytes read (uint8) + written (float32) per second
  (d) a device copy of the same float32     out.copy_(other): reads and writes 4 bytes a value, the rate the device gives a
      tensor                                plain streaming kernel of that size

Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.chunk_draw_bench import MEAN, NCAT, STD, c2_set, fmt, timed      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, nargs='+', default=[1024])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=256, help='frames of the FrameStore')
    ap.add_argument('--T', type=int, nargs='+', default=[64, 448], help='images of a gather (64 chunks of 7 frames: 448)')
    ap.add_argument('--hw', type=int, nargs=2, default=[384, 1280])
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('chunk_vis_bench needs the MI355X: no timing is taken without it')
    import __graft_entry__
    __graft_entry__.build()
    from trackmpnn_amd import ChunkSampler, DetectionStore, FrameStore
    dev = torch.device('cuda:0')
    lines = ['| B | rows before dropout | (a) plain draw ms | (b) vis draw ms | (b) - (a) ms | images of the plan |', '|---|---|---|---|---|---|']
    results = []
    for B in a.B:
        seqs, chunks = c2_set(B, seed=2)
        for q in seqs:
            q['height'] = 375
        tm, ts = MEAN + [0.0, 0.0], STD + [1.0, 1.0]
        plain = ChunkSampler(DetectionStore(seqs, NCAT, '2d+temp', tm, ts, device=dev), chunks, seed=11)
        vis = ChunkSampler(DetectionStore(seqs, NCAT, '2d+temp+vis', tm + [0.0] * 128, ts + [1.0] * 128, device=dev), chunks, seed=11)
        order = plain.epoch_order(0)
        keep = {}
        ta = timed(lambda r: keep.__setitem__('p', plain.draw(order, r)), a.reps, a.warmup)
        tb = timed(lambda r: keep.__setitem__('v', vis.draw(order, r)), a.reps, a.warmup)
        dv, hv = vis.draw(order, 1), vis.draw_host(order, 1)
        n1 = int(hv.offsets[-1])
        assert torch.equal(dv.box[:n1].cpu(), torch.from_numpy(hv.box)) and torch.equal(dv.map_of[:n1].cpu(), torch.from_numpy(hv.map_of))
        lines.append(f'| {B} | {dv.n_max} | {fmt(ta)} | {fmt(tb)} | {np.median(tb) - np.median(ta):.3f} | {hv.plan.frames.shape[0]} |')
        results.append(dict(B=B, n_max=dv.n_max, plain_ms=float(np.median(ta)), vis_ms=float(np.median(tb))))
        print(lines[-1], flush=True)
    H, W = a.hw
    rng = np.random.default_rng(0)
    fs = FrameStore([torch.from_numpy(rng.integers(0, 256, (a.frames, H, W, 3), dtype=np.uint8))], (0.485, 0.456, 0.406),
                    (0.229, 0.224, 0.225), dev)
    lines += ['', f'| T images of {H} x {W} | (c) gather ms | GB/s (1 + 4 bytes a value) | (d) copy ms | GB/s (4 + 4 bytes a value) | '
              '(c) / (d) time |', '|---|---|---|---|---|---|']
    for T in a.T:
        plan = np.stack([np.zeros(T, np.int64), rng.integers(0, a.frames, T), np.arange(T) % 2], 1)
        keep = {}
        tc = timed(lambda r: keep.__setitem__('g', fs.gather(plan)), a.reps, a.warmup)
        got = keep['g']
        assert torch.equal(got[:2].cpu(), torch.from_numpy(fs.frames_host(plan[:2])))
        other = torch.empty_like(got)
        td = timed(lambda r: other.copy_(got), a.reps, a.warmup)
        vals = T * 3 * H * W
        lines.append(f'| {T} | {fmt(tc)} | {5 * vals / np.median(tc) / 1e6:.0f} | {fmt(td)} | {8 * vals / np.median(td) / 1e6:.0f} | '
                     f'{np.median(tc) / np.median(td):.2f} |')
        results.append(dict(T=T, H=H, W=W, gather_ms=float(np.median(tc)), copy_ms=float(np.median(td))))
        print(lines[-1], flush=True)
        del other, got, keep
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(dict(tool='chunk_vis_bench', device=torch.cuda.get_device_name(0), reps=a.reps, results=results)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
