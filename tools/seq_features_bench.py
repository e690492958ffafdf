"""The whole-sequence features of a validation pass: SequenceFeatures against what a user did without it.

    python tools/seq_features_bench.py --reps 20 --vis-reps 5 --out OUT.md

Workload: a KITTI-val-shaped store -- three sequences of 209, 339 and 837 frames (the lengths of the reference's validation
sequences 16, 18 and 20), about 10 detections a frame, frames at the CNN's input size 384 x 1280 --, with and without 'vis'.
Device events around each item (the host's own work lies between the two events, so it is part of the figure), warm-up
excluded, median and min .. max:

  (a) SequenceFeatures.build, '2d+temp'               one launch and one small upload
  (b) the same by hand                                sequence_features_host per sequence, then one upload of X and y each
  (c) build + attach_vis, '2d+temp+vis'               per batch of --frames-per-batch frames: gather, net, VisHead.rows
  (d) the same by hand                                (b) for the static columns and the head's arguments, then the per-frame loop
                                                      FrameStore.gather -> net -> VisHead.rows(out=X[rows])

The embedding net is a stand-in, one Conv2d(3, 128, 3, stride=4, padding=1) (down_ratio 4), so that the CNN does not swamp the
figure; (c) and (d) run the same net on the same frames.  Launch counts are those of the library's entry points (tmpnn_seq_features
1, tmpnn_frames_gather 1, tmpnn_vis_head_fwd 2 a call) plus the calls of the net; uploads are counted apart.

Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.chunk_draw_bench import MEAN, NCAT, STD, fmt, timed      # noqa: E402

LENGTHS = (209, 339, 837)
IM_HW = (375, 1242)


def val_set(seed, lengths, per_frame):
    rng = np.random.default_rng(seed)
    seqs = []
    for nf in lengths:
        n_f = rng.poisson(per_frame, nf)
        frame = np.repeat(np.arange(nf), n_f)
        n = frame.size
        x1, y1 = np.round(rng.uniform(0, IM_HW[1] - 160, n), 2), np.round(rng.uniform(100, 250, n), 2)
        box = np.stack([x1, y1, x1 + np.round(rng.uniform(5, 150, n), 2), y1 + np.round(rng.uniform(5, 120, n), 2)], 1)
        seqs.append(dict(frame=frame, track=rng.integers(-1, 200, n), cat=rng.integers(1, NCAT + 1, n), box=box,
                         score=np.round(rng.uniform(0.3, 1, n), 4), width=IM_HW[1], height=IM_HW[0], num_frames=nf))
    return seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--vis-reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--per-frame', type=float, default=10.0)
    ap.add_argument('--lengths', type=int, nargs='+', default=list(LENGTHS))
    ap.add_argument('--hw', type=int, nargs=2, default=[384, 1280])
    ap.add_argument('--frames-per-batch', type=int, nargs='+', default=[8])
    ap.add_argument('--out', default=None, help='write the table (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('seq_features_bench needs the MI355X: no timing is taken without it')
    import __graft_entry__
    __graft_entry__.build()
    from trackmpnn_amd import DetectionStore, FrameStore, SequenceFeatures, VisHead, listed_features_host
    dev = torch.device('cuda:0')
    seqs = val_set(5, a.lengths, a.per_frame)
    tm, ts = MEAN + [0.0, 0.0], STD + [1.0, 1.0]
    keep = {}

    def by_hand(store):
        """The parent commit's way to the static columns: the host definition per sequence, uploaded."""
        out = []
        for r in listed_features_host(store):
            d = {'X': torch.from_numpy(r.X).to(dev)[None], 'y': torch.from_numpy(r.y).to(dev)[None]}
            if store.vis:
                d['box'], d['im_hw'] = torch.from_numpy(r.box).to(dev), torch.from_numpy(r.im_hw).to(dev)
            out.append(d)
        return out

    # ---- without 'vis'
    plain = DetectionStore(seqs, NCAT, '2d+temp', tm, ts, device=dev)
    sf = SequenceFeatures(plain)
    ta = timed(lambda r: keep.__setitem__('a', sf.build()), a.reps, a.warmup)
    tb = timed(lambda r: keep.__setitem__('b', by_hand(plain)), a.reps, a.warmup)
    for d, h in zip(keep['a'], keep['b']):
        assert torch.equal(d['X'].view(torch.int32), h['X'].view(torch.int32)) and torch.equal(d['y'], h['y'])
    sf.check()
    nseq, rows = len(seqs), plain.ndets
    lines = [f'{nseq} sequences of {a.lengths} frames, {rows} detections; frames of {a.hw[0]} x {a.hw[1]}; device events, '
             f'median (min .. max) of {a.reps} ({a.vis_reps} for the visual pass) after {a.warmup} warm-up runs.', '',
             '| item | ms | library launches + net calls | uploads |', '|---|---|---|---|',
             f"| (a) `SequenceFeatures.build`, '2d+temp' | {fmt(ta)} | 1 | 1 |",
             f'| (b) `sequence_features_host` per sequence + upload | {fmt(tb)} | 0 | {2 * nseq} |']
    results = [dict(item='build', ms=float(np.median(ta))), dict(item='host+upload', ms=float(np.median(tb)))]
    print('\n'.join(lines[-2:]), flush=True)

    # ---- with 'vis'
    vis = DetectionStore(seqs, NCAT, '2d+temp+vis', tm + [0.5] * 128, ts + [0.5] * 128, device=dev)
    H, W = a.hw
    gen = torch.Generator(device=dev).manual_seed(1)
    frames = FrameStore([torch.randint(0, 256, (nf, H, W, 3), dtype=torch.uint8, device=dev, generator=gen) for nf in a.lengths],
                        (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dev)
    torch.manual_seed(2)
    net = torch.nn.Conv2d(3, 128, 3, stride=4, padding=1).to(dev).eval()
    head = VisHead((H, W), 4, tm + [0.5] * 128, ts + [0.5] * 128, dev)
    svf = SequenceFeatures(vis)
    col = vis.F - 128
    zeros = torch.zeros(int(np.diff(vis.first).max()), dtype=torch.int32, device=dev)        # map_of of a one-image call
    live = [[f for f in range(nf) if vis.first[vis.seq_base[s] + f + 1] > vis.first[vis.seq_base[s] + f]] for s, nf in enumerate(a.lengths)]

    def per_frame_loop():
        out = by_hand(vis)
        with torch.no_grad():
            for s, d in enumerate(out):
                X, base = d['X'][0], int(vis.first[vis.seq_base[s]])
                for f in live[s]:
                    r0, r1 = int(vis.first[vis.seq_base[s] + f]) - base, int(vis.first[vis.seq_base[s] + f + 1]) - base
                    maps = net(frames.gather(np.asarray([[s, f, 0]], np.int64)))
                    head.rows(maps, d['box'][r0:r1], zeros[:r1 - r0], d['im_hw'][r0:r1],
                              out=X[r0:r1], col=col)
        return out

    td = timed(lambda r: keep.__setitem__('d', per_frame_loop()), a.vis_reps, 1)
    n_live = sum(len(l) for l in live)
    for fpb in a.frames_per_batch:
        def device_pass():
            out = svf.build(frames_per_batch=fpb)
            svf.attach_vis(head, frames, net, frames_per_batch=fpb)
            return out
        tc = timed(lambda r: keep.__setitem__('c', device_pass()), a.vis_reps, 1)
        svf.check()
        worst = 0.0
        for d, h in zip(keep['c'], keep['d']):
            assert torch.equal(d['X'][0, :, :col].contiguous().view(torch.int32), h['X'][0, :, :col].contiguous().view(torch.int32))
            assert torch.equal(d['y'], h['y'])
            worst = max(worst, float((d['X'][0, :, col:] - h['X'][0, :, col:]).abs().max()))
        batches = sum(sum(1 for f0 in range(0, nf, fpb) if any(f0 <= f < f0 + fpb for f in live[s])) for s, nf in enumerate(a.lengths))
        lines.append(f"| (c) `build` + `attach_vis`, '2d+temp+vis', {fpb} frames a batch | {fmt(tc)} | 1 + {batches} x (1 + 1 + 2) = "
                     f'{1 + 4 * batches} | 1 + {batches} plans |')
        results.append(dict(item='build+attach_vis', frames_per_batch=fpb, ms=float(np.median(tc)), batches=batches, max_abs_diff_vs_loop=worst))
        print(lines[-1], flush=True)
    lines.append(f'| (d) host columns + upload, then per frame `gather` -> net -> `rows` | {fmt(td)} | {n_live} x (1 + 1 + 2) = {4 * n_live} | '
                 f'{4 * nseq} + {n_live} plans |')
    results.append(dict(item='per-frame loop', ms=float(np.median(td)), frames=n_live))
    print(lines[-1], flush=True)
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(dict(tool='seq_features_bench', device=torch.cuda.get_device_name(0), rows=rows, results=results)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
