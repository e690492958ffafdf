"""Wall time of the whole MOT-challenge summary on the device next to the host definition, and of the CLEAR-only evaluator at
this commit next to an earlier one.

    python tools/mot_ident_bench.py --out profiles/mot_ident_run.md [--parent DIR]

The KITTI-val-shaped synthetic set of tools/mot_eval_bench.py (moteval.synth_mot_sequence: about 10 sequences of about 800 frames
and about 8 objects).  In ONE process:

  (a) mot_summary_host over every sequence (numpy + scipy)                 wall time of the loop
  (b) MotEvaluator(identity=True).evaluate + read (one upload, one clear   wall time from the call to the returned dicts
      + four launches, one device -> host copy; the store uploaded before)
  (c) MotEvaluator(identity=False).evaluate + read                         the same, the evaluator as it was

(a) and (b) must agree in every key (integers equal, ratios bit for bit): checked on every repetition.  With --parent DIR (a
checkout of the commit to compare with, its library built) the tool also runs (c) in child processes, alternating between
this tree and DIR, `--rounds` times each, and reports every process's median and the spread of DIR's own repetitions: the
existing path must not be slower than that spread allows.  --trace N: N identity evaluations and nothing else (the program to
put under `rocprofv3 --kernel-trace --stats` for the per-kernel times).  Not bench.py: nothing here gates a change."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_set(moteval, a):
    rng = np.random.default_rng(3)
    return [moteval.synth_mot_sequence(8100 + i, int(a.frames * rng.uniform(0.6, 1.4)), objects=a.objects) for i in range(a.sequences)]


def timed(ev, tracks):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.evaluate(tracks)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    per, overall = ev.read()
    t3 = time.perf_counter()
    return per, overall, [1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)]


def plain_child(a):
    """(c) alone, with the package of --tree: one JSON line of the repetitions' times."""
    sys.path.insert(0, a.tree)
    from trackmpnn_amd import moteval
    assert os.path.dirname(os.path.dirname(os.path.abspath(moteval.__file__))) == os.path.abspath(a.tree)
    seqs = make_set(moteval, a)
    tracks = [q['tracks'] for q in seqs]
    ev = moteval.MotEvaluator(seqs, 'cuda:0')
    ms = [timed(ev, tracks)[2][0] for _ in range(a.reps + 3)][3:]
    print(json.dumps(dict(plain_ms=ms)))


def same(d, h):
    return set(d) == set(h) and all(np.float64(d[k]).view(np.int64) == np.float64(h[k]).view(np.int64) if isinstance(h[k], float)
                                    else d[k] == h[k] for k in h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sequences', type=int, default=10)
    ap.add_argument('--frames', type=int, default=800)
    ap.add_argument('--objects', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2, help='child processes per tree for the comparison with --parent')
    ap.add_argument('--parent', default=None, help='a checkout of the commit to compare identity=False with (library built)')
    ap.add_argument('--out', default=None, help='write the table (markdown) here as well')
    ap.add_argument('--trace', type=int, default=0, help='run this many identity evaluations and nothing else')
    ap.add_argument('--plain-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mot_ident_bench needs the MI355X: no timing is taken without it')
    if a.plain_child:
        return plain_child(a)
    sys.path.insert(0, ROOT)
    from trackmpnn_amd import moteval
    seqs = make_set(moteval, a)
    tracks = [q['tracks'] for q in seqs]
    ev = moteval.MotEvaluator(seqs, 'cuda:0', identity=True)
    if a.trace:
        for _ in range(a.trace):
            ev.evaluate(tracks)
        ev.read()
        return
    plain = moteval.MotEvaluator(seqs, 'cuda:0')
    host_ms, dev_ms, plain_ms = [], [], []
    for r in range(a.reps + 1):                                   # (repetition 0 warms up)
        t0 = time.perf_counter()
        ref = [moteval.mot_summary_host(q['det_frame'], q['det_box'], q['tracks'], q['gt_frame'], q['gt_track'], q['gt_box']) for q in seqs]
        hm = 1e3 * (time.perf_counter() - t0)
        per, overall, dm = timed(ev, tracks)
        _, _, pm = timed(plain, tracks)
        for s, (d, h) in enumerate(zip(per, ref)):
            assert same(d, h), f'sequence {s}: device {d} != host {h}'
        assert same(overall, moteval.mot_overall(ref))
        if r:
            host_ms.append(hm)
            dev_ms.append(dm)
            plain_ms.append(pm)
    h = min(host_ms)
    d = min(dev_ms, key=lambda v: v[0])
    p = min(plain_ms, key=lambda v: v[0])
    st = ev.store
    nf = sum(int(x) for x in st.seq[:, 5])
    lines = [f'{len(seqs)} sequences, {nf} frames, {st.n_gt} GT rows, {st.n_det} detections, {st.n_obj} objects, count matrices of '
             f'{ev._n_pair} entries; overall MOTA {overall["mota"]:.4f}, IDF1 {overall["idf1"]:.4f} (idtp {overall["idtp"]}), '
             f'{overall["mostly_tracked"]} / {overall["partially_tracked"]} / {overall["mostly_lost"]} mostly tracked / partially / '
             f'mostly lost, {overall["fragmentations"]} fragmentations; best of {a.reps} repetitions after one warm-up; (a) and (b) '
             'agreed in every key on every repetition.', '',
             '| path | ms per evaluation | us per frame |', '|---|---|---|',
             f'| (a) `mot_summary_host` over the sequences | {h:.3f} | {1e3 * h / nf:.2f} |',
             f'| (b) `identity=True`: `evaluate` + `read` | {d[0]:.3f} | {1e3 * d[0] / nf:.2f} |',
             f'| (b) of which: `evaluate` returns after | {d[1]:.3f} | |',
             f'| (b) of which: wait for the device | {d[2]:.3f} | |',
             f'| (b) of which: copy + dicts | {d[3]:.3f} | |',
             f'| (c) `identity=False`: `evaluate` + `read` (same process) | {p[0]:.3f} | {1e3 * p[0] / nf:.2f} |',
             '', f'host / device (a) / (b): {h / d[0]:.1f}x; identity figures on top of the CLEAR walk (b) - (c): {d[0] - p[0]:.3f} ms']
    result = dict(tool='mot_ident_bench', device=torch.cuda.get_device_name(0), sequences=len(seqs), frames=nf, host_ms=h,
                  identity_ms=d[0], plain_ms=p[0])
    if a.parent:
        runs = {'this': [], 'parent': []}
        for _ in range(a.rounds):
            for name, tree in (('this', ROOT), ('parent', os.path.abspath(a.parent))):
                cmd = [sys.executable, os.path.abspath(__file__), '--plain-child', '--tree', tree, '--reps', str(max(a.reps, 20)),
                       '--sequences', str(a.sequences), '--frames', str(a.frames), '--objects', str(a.objects)]
                out = subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=tree).stdout
                runs[name].append(json.loads(out.strip().splitlines()[-1])['plain_ms'])
        lines += ['', f'`identity=False` in processes of their own, alternating this tree and the parent ({max(a.reps, 20)} repetitions '
                  'after 3 warm-ups each):', '', '| tree, process | median ms | min | max |', '|---|---|---|---|']
        for name in ('parent', 'this'):
            for i, ms in enumerate(runs[name]):
                lines.append(f'| {name}, {i + 1} | {statistics.median(ms):.3f} | {min(ms):.3f} | {max(ms):.3f} |')
        pm, tm = [statistics.median(ms) for ms in runs['parent']], [statistics.median(ms) for ms in runs['this']]
        allp = [x for ms in runs['parent'] for x in ms]
        lines += ['', f'parent: medians {min(pm):.3f} to {max(pm):.3f} ms between processes, single repetitions {min(allp):.3f} to '
                  f'{max(allp):.3f} ms; this tree: medians {min(tm):.3f} to {max(tm):.3f} ms -- '
                  + ('inside the spread of the parent\'s own repetitions' if max(tm) <= max(allp) else 'OUTSIDE the spread of the parent\'s own repetitions')]
        result.update(parent_median_ms=pm, this_median_ms=tm, parent_min_ms=min(allp), parent_max_ms=max(allp))
    text = '\n'.join(lines)
    print(text)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
