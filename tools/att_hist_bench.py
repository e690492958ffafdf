"""What the attention histograms cost per timestep of infer_sequence, next to the dense route they replace.

    python tools/att_hist_bench.py --out profiles/att_hist.md

A model with K = 2 heads ('2d' features, H = 64) on the KITTI-like sequence of tools/val_f1_bench.py (synth_window: about 6
detections per frame, misses and false positives, cur_win_size 5), 40 frames, and on its first --short-frames frames.  In ONE
process, on the same sequence, greedy association:

  off       infer_sequence(...)                                the loop as it is without a monitor (models with heads run the
                                                               composed timesteps: there is no native driver to lose)
  on        infer_sequence(..., att_monitor=AttentionMonitor)  + one counting launch per model call inside the loop, no host read
  dense     what a user had before, the reference's way: after every such call every head's dense [N, N] matrix through
            SparseAttention.numpy(), the labels and row types copied to the host, and the walk over N x N x K entries in Python
            (the short sequence only: it takes seconds)
  dense_np  the same copies with the walk as one numpy expression per head: the copies' share of `dense`

Every figure: wall time of the call up to a device synchronisation / timesteps, the calls repeated for --budget seconds after
three warm-up calls (one warm-up and at least one call for `dense`), the variants taken in turn --reps times; reported as the
median of the repetitions with their range.  `on`, `dense` and `dense_np` must give the same histograms.  Also: count() alone,
back to back on one graph, per call.  Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DenseWalk:
    """The pass an AttentionMonitor replaces.  python=True: the entry-by-entry walk; else one numpy expression per head."""

    def __init__(self, K, bins, python):
        self.K, self.bins, self.python = K, bins, python
        self.lists = [([], []) for _ in range(K)]
        self.forwards = 0

    def count(self, tg, attention):
        N = tg.N
        r = tg.rows
        packed = torch.stack([r['is_edge'][:N], r['labels'][:N]]).cpu().numpy()
        is_edge, lab = packed[0] != 0, packed[1]
        self.forwards += 1
        for k, att in enumerate(attention[0]):
            a = att.numpy()                                             # dense [N, N], built on the device and copied
            tp, fp = self.lists[k]
            if self.python:
                for row in range(N):
                    if is_edge[row]:
                        continue
                    for col in range(N):
                        if a[row][col] > 0 and is_edge[col]:
                            (tp if lab[col] == 1 else fp).append(a[row][col])
            else:
                sel = (~is_edge)[:, None] & (a > 0) & is_edge[None, :]
                rr, cc = np.nonzero(sel)
                v, t = a[rr, cc], lab[cc] == 1
                tp.extend(v[t])
                fp.extend(v[~t])

    def counts(self):
        out = np.zeros((self.K, 2, self.bins), np.int64)
        for k, pair in enumerate(self.lists):
            for s, vals in enumerate(pair):
                out[k, s] = np.histogram(np.asarray(vals, np.float32), self.bins, (0.0, 1.0))[0]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--short-frames', type=int, default=10)
    ap.add_argument('--dets', type=float, default=6.0)
    ap.add_argument('--win', type=int, default=5)
    ap.add_argument('--heads', type=int, default=2)
    ap.add_argument('--node-bias', type=float, default=1.5, help='added to the det head\'s bias: most detections score above 0.5 and '
                    'stay active, so the window keeps its edges (a trained tracker\'s graphs, not rows of isolated dets)')
    ap.add_argument('--budget', type=float, default=1.0, help='seconds of calls per figure and repetition')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    if not torch.cuda.is_available():
        raise SystemExit('att_hist_bench needs the MI355X: no timing is taken without it')
    from trackmpnn_amd import AttentionMonitor, TrackMPNN, synth_window
    from trackmpnn_amd.loops import infer_sequence
    from trackmpnn_amd.tracking import TrackGraph
    dev = 'cuda:0'
    K = a.heads
    yy = synth_window(2001, a.frames, a.dets, int(3 * a.dets) + 2)
    Xall = torch.randn(1, yy.shape[0], 8, generator=torch.Generator().manual_seed(3001))
    seqs = {}
    for name, frames in (('long', a.frames), ('short', a.short_frames)):
        keep = yy[:, 0] < frames
        seqs[name] = (Xall[:, torch.from_numpy(keep)].contiguous(), torch.from_numpy(yy[keep])[None], int(yy[keep][:, 0].max()) + 1,
                      int(keep.sum()))
    torch.manual_seed(5)
    model = TrackMPNN('2d', 3, 64, K, 'diff')
    gp = torch.Generator().manual_seed(4242)
    with torch.no_grad():                                       # scores on both sides of 0.5 (as bench.py's loop block)
        for k, prm in model.named_parameters():
            prm.add_(0.1 * torch.randn(prm.shape, generator=gp))
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=gp) + (a.node_bias if '_node' in k else 0.0))
    model = model.to(dev).eval()
    am = AttentionMonitor(dev, K)

    def timed(fn, T, warm, least):
        for _ in range(warm):
            r = fn()
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < a.budget or n < least:
            r = fn()
            n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3 / T, r

    def run(seq, mon):
        X, y, _, _ = seqs[seq]
        return infer_sequence(model, X, y, a.win, 0, False, dev, att_monitor=mon)

    def on(seq):
        am.reset()
        return run(seq, am) + (None,)

    def dense(seq, python):
        w = DenseWalk(K, 25, python)
        return run(seq, w) + (w,)

    plan = [('long', 'off', lambda: run('long', None) + (None,), 3, 3), ('long', 'on', lambda: on('long'), 3, 3),
            ('short', 'off', lambda: run('short', None) + (None,), 3, 3), ('short', 'on', lambda: on('short'), 3, 3),
            ('short', 'dense_np', lambda: dense('short', False), 3, 3), ('short', 'dense', lambda: dense('short', True), 1, 1)]
    ms = {(s, v): [] for s, v, _, _, _ in plan}
    hist, tracks, calls, edges = {}, {}, {}, {}
    for rep in range(a.reps):
        for s, v, fn, warm, least in plan:
            t, r = timed(fn, seqs[s][2], warm, least)
            ms[(s, v)].append(t)
            assert np.array_equal(tracks.setdefault(s, r[0]), r[0]), 'the tracks differ'
            calls[s], edges[s] = r[1], r[2]
            if v == 'on':
                hist[(s, v)] = am.read()
            elif r[3] is not None:
                hist[(s, v)] = dict(counts=r[3].counts(), forwards=r[3].forwards)
    for v in ('dense', 'dense_np'):
        assert np.array_equal(hist[('short', 'on')]['counts'], hist[('short', v)]['counts']), v
        assert hist[('short', 'on')]['forwards'] == hist[('short', v)]['forwards'] == calls['short'] - 1
    assert hist[('long', 'on')]['forwards'] == calls['long'] - 1
    # count() alone: back to back on the graph of the sequence's first call
    X, y, _, _ = seqs['long']
    with torch.no_grad():
        tg, feats, _, _ = TrackGraph.initialize(X, y, 0, 'test', dev)
        _, _, _, att = model.forward_dgraph(feats, None, tg.graph)
    alone = []
    for rep in range(a.reps):
        for _ in range(50):
            am.count(tg, att)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2000):
            am.count(tg, att)
        torch.cuda.synchronize()
        alone.append((time.perf_counter() - t0) / 2000 * 1e6)
    med = lambda k: float(np.median(ms[k]))
    cell = lambda k: f'{med(k):.4f} ({min(ms[k]):.4f} .. {max(ms[k]):.4f})'
    names = dict(off='`infer_sequence`, no monitor', on='`infer_sequence(..., att_monitor=AttentionMonitor)`',
                 dense_np='dense route: `SparseAttention.numpy()` per head + host copies, walk in numpy',
                 dense='dense route: `SparseAttention.numpy()` per head + host copies, walk in Python (the reference\'s)')
    lines = [f'K = {K} heads, H = 64, cur_win_size {a.win}, greedy; ms per timestep, median of {a.reps} repetitions (range), '
             f'{a.budget:g} s of calls each (`dense`: one warm-up call, then at least one call).', '']
    for s in ('long', 'short'):
        _, _, T, nd = seqs[s]
        lines += [f'**{s}**: {T} timesteps, {nd} detections ({nd / T:.1f} per frame), {calls[s]} forward calls of which '
                  f'{calls[s] - 1} are counted (E = {edges[s] / calls[s]:.0f} edges per call on average, {hist[(s, "on")]["dets"]} det rows '
                  f'of which {hist[(s, "on")]["isolated"]} without an edge), {int(hist[(s, "on")]["counts"].sum())} values in the histograms.', '',
                  '| path | ms per timestep |', '|---|---|']
        lines += [f'| {names[v]} | {cell((s, v))} |' for ss, v, _, _, _ in plan if ss == s]
        per_fwd = (med((s, 'on')) - med((s, 'off'))) * T / (calls[s] - 1) * 1e3
        lines += ['', f'Cost of the counting launch: {med((s, "on")) - med((s, "off")):+.4f} ms per timestep = {per_fwd:+.1f} us per '
                      f'counted forward ({(med((s, "on")) / med((s, "off")) - 1) * 100:+.1f} % of the loop).', '']
    lines += [f'Dense route against the monitored loop (short): Python walk {med(("short", "dense")) / med(("short", "on")):.0f}x, numpy walk '
              f'{med(("short", "dense_np")) / med(("short", "on")):.1f}x.',
              f'`AttentionMonitor.count` alone, 2000 calls back to back on one graph (N = {tg.N}, E = {tg.E}): '
              f'{float(np.median(alone)):.2f} us per call ({min(alone):.2f} .. {max(alone):.2f}).']
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(dict(tool='att_hist_bench', device=torch.cuda.get_device_name(0), heads=K,
                          ms_per_timestep={f'{s}/{v}': [round(x, 5) for x in t] for (s, v), t in ms.items()},
                          count_alone_us=[round(x, 3) for x in alone])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(text + '\n\n')


if __name__ == '__main__':
    main()
