"""N monitored train_chunks steps on the C2 batch, and nothing else: the program to put under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o r -- python tools/train_monitor_trace.py --steps 8

for the per-launch time of the monitor's kernels (k_cls_counts_win: one launch per call; k_train_record_fold: one per step)
next to the windowed loss they follow.  Prints the number of listed rows R the counting launches read per step."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=None)
    ap.add_argument('--steps', type=int, default=8)
    args = ap.parse_args()
    import bench
    from trackmpnn_amd import TrackMPNN, TrainMonitor, build_train_batch_device, synth_window
    from trackmpnn_amd.loops import train_chunks
    dev = torch.device('cuda', 0)
    w = bench.WORKLOADS['c2']
    B = int(args.windows or w['windows'])
    distinct = min(B, 64)
    ys = [synth_window(1000 + s, w['frames'], w['mean_dets'], w['max_dets']) for s in range(distinct)]
    ys = (ys * ((B + distinct - 1) // distinct))[:B]
    off = np.concatenate([[0], np.cumsum([y.shape[0] for y in ys])])
    batch = build_train_batch_device(torch.from_numpy(np.concatenate(ys)).to(dev), dev, offsets=torch.from_numpy(off).to(dev))
    Xs = torch.randn(batch.n_feat, w['ncat'] + 5, generator=torch.Generator().manual_seed(1)).to(dev)
    torch.manual_seed(5)
    model = TrackMPNN('2d', w['ncat'], w['H'], 0, 'diff').to(dev).train()
    opt = bench.make_adam(model)
    m = TrainMonitor(dev)
    for _ in range(args.steps):
        opt.zero_grad(set_to_none=False)
        train_chunks(model, batch, Xs, monitor=m)
        opt.step()
    torch.cuda.synchronize()
    print(json.dumps(dict(steps=args.steps, calls=len(batch.plans), chunks=batch.B,
                          listed_rows_R=int(sum(x.n_det + x.n_edge for x in batch.windows)), monitor=m.read())))


if __name__ == '__main__':
    main()
