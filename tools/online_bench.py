"""Wall time of a steady-state push of the online tracker next to infer_sequence's time per timestep.

    python tools/online_bench.py --frames 2000 --out profiles/online_tracker.md

Shape C2: a KITTI-like stream (synth_window: about 8 detections per frame, misses and false positives), '2d' features, H = 64,
cur_win_size 5, greedy association.  In ONE process, on the same detections:

  (a) loops.infer_sequence on the recorded sequence           wall time of the call / timesteps
  (b) OnlineTracker.push_features, one host frame per push    wall time of every push (each ends with the timestep's polled read)
  (c) OnlineTracker.push, raw detections                      the same + one packed copy and the feature launch

(b) and (c) report p50 / p99 / max over the steady-state pushes (the first `--skip` pushes are left out) and the whole stream's
wall time per push up to a final synchronisation, which is what (a) measures.  The three runs must give the same tracks.  Not
bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NCAT = 3
MEAN = [0.5] * 3 + [0.5, 600.0, 175.0, 75.0, 60.0]             # round stand-ins for a detector's statistics
STD = [0.5] * 3 + [0.25, 300.0, 25.0, 75.0, 50.0]


def stream_of(frames, mean_dets, seed):
    """(y [ND, 2] time-sorted, per frame (cat, score, box))."""
    from trackmpnn_amd import synth_window
    y = synth_window(seed, frames, mean_dets, int(3 * mean_dets))
    rng = np.random.RandomState(seed + 1)
    per = []
    for t in range(int(y[-1, 0]) + 1):
        m = int((y[:, 0] == t).sum())
        x1, y1 = rng.uniform(0, 1080, m), rng.uniform(100, 250, m)
        box = np.stack([x1, y1, x1 + rng.uniform(5, 150, m), y1 + rng.uniform(5, 120, m)], 1).astype(np.float32)
        per.append((rng.randint(1, NCAT + 1, m), rng.uniform(0.3, 1, m).astype(np.float32), box))
    return y, per


def pct(ms):
    ms = np.asarray(ms)
    return f'{np.percentile(ms, 50):.4f} / {np.percentile(ms, 99):.4f} / {ms.max():.4f}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--dets', type=float, default=8.0)
    ap.add_argument('--win', type=int, default=5)
    ap.add_argument('--skip', type=int, default=10, help='leading pushes left out of the percentiles')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None, help='write the table (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('online_bench needs the MI355X: no timing is taken without it')
    import __graft_entry__
    __graft_entry__.build()
    from trackmpnn_amd import FeatureSpec, OnlineTracker, TrackMPNN, online_features_host
    from trackmpnn_amd.loops import infer_sequence
    dev = 'cuda:0'
    spec = FeatureSpec(NCAT, '2d', MEAN, STD)
    yy, per = stream_of(a.frames, a.dets, 4100)
    rows = [online_features_host(spec, c, s, b, t) for t, (c, s, b) in enumerate(per)]
    X = torch.from_numpy(np.concatenate(rows))[None]
    y = torch.from_numpy(yy)[None]
    xs = [torch.from_numpy(r) for r in rows]
    T = len(per)
    torch.manual_seed(9)
    model = TrackMPNN('2d', NCAT, 64, 0, 'diff').to(dev)
    gp = torch.Generator().manual_seed(17)
    with torch.no_grad():                                       # scores on both sides of 0.5 (as bench.py's loop block)
        for k, prm in model.named_parameters():
            prm.add_((0.1 * torch.randn(prm.shape, generator=gp)).to(dev))
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_((0.5 * torch.randn(prm.shape, generator=gp)).to(dev))
    model.eval()

    def offline():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = infer_sequence(model, X, y, a.win, 0, False, dev, True)
        torch.cuda.synchronize()
        return out[0][:, 1], 1e3 * (time.perf_counter() - t0) / T

    def online(raw):
        trk = OnlineTracker(model, a.win, 0, False, True, spec=spec, device=dev)
        ms = []
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        for t in range(T):
            t0 = time.perf_counter()
            if raw:
                trk.push(*per[t], last=t == T - 1)
            else:
                trk.push_features(xs[t], last=t == T - 1)
            ms.append(1e3 * (time.perf_counter() - t0))
        torch.cuda.synchronize()
        return trk.tracks(), 1e3 * (time.perf_counter() - t_all) / T, ms[a.skip:], trk.native_steps

    res = dict(offline=[], feat=[], raw=[])
    ref = None
    for r in range(a.reps + 1):                                 # (repetition 0 warms up: library load, allocator, pinned pool)
        tr_o, ms_o = offline()
        tr_f, ms_f, pf, nat_f = online(False)
        tr_r, ms_r, pr, nat_r = online(True)
        ref = tr_o if ref is None else ref
        assert np.array_equal(tr_o, ref) and np.array_equal(tr_f, ref) and np.array_equal(tr_r, ref), 'the tracks differ'
        if r:
            res['offline'].append(ms_o)
            res['feat'].append((ms_f, pf))
            res['raw'].append((ms_r, pr))
    best = lambda k: min(res[k], key=lambda v: v[0])
    o = min(res['offline'])
    (f_all, f_ms), (r_all, r_ms) = best('feat'), best('raw')
    lines = [f'{T} frames, {yy.shape[0]} detections ({yy.shape[0] / T:.1f} per frame), cur_win_size {a.win}, H = 64, greedy; '
             f'{nat_f} of {T} pushes through the native driver; best of {a.reps} repetitions after one warm-up.', '',
             '| path | ms per timestep (whole stream, synchronised at the end) | steady-state push p50 / p99 / max ms | '
             'difference per push to infer_sequence ms |', '|---|---|---|---|',
             f'| (a) `infer_sequence` | {o:.4f} | - | - |',
             f'| (b) `push_features` (host rows) | {f_all:.4f} | {pct(f_ms)} | {f_all - o:+.4f} |',
             f'| (c) `push` (raw detections) | {r_all:.4f} | {pct(r_ms)} | {r_all - o:+.4f} |']
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(dict(tool='online_bench', device=torch.cuda.get_device_name(0), frames=T, ndets=int(yy.shape[0]),
                          offline_ms=o, push_features_ms=f_all, push_ms=r_all, native=nat_f,
                          push_features_p50_p99_max=[float(np.percentile(f_ms, 50)), float(np.percentile(f_ms, 99)), float(max(f_ms))],
                          push_p50_p99_max=[float(np.percentile(r_ms, 50)), float(np.percentile(r_ms, 99)), float(max(r_ms))])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
