"""Launches, kernel time and idle time between consecutive kernels, per step, from a rocprofv3 --kernel-trace CSV of a bench run.

    python tools/kernel_gaps.py TRACE_DIR_OR_CSV [--anchor SUBSTR] [--last K] [--top N] [--match SUBSTR]

A step is the span from one launch of the anchor kernel (one that runs once per step; default: the last call's full edge
backward) to the next.  The last K such spans are used (default 20: the timed steps of `bench.py --steps 20`), and every
figure is the mean over them.  The idle time of a boundary is start(next) - end(previous) of two kernels that follow each other
on the device, clamped at zero; a negative difference (the next kernel was already running) is counted as overlap.
Boundaries are grouped by (previous kernel, next kernel); --match keeps the groups in which either name contains SUBSTR and
prints their share.  Collect the trace in a run of its own (no counters in the same run).
"""
import argparse
import collections
import csv
import glob
import os
import re


def short(name):
    name = re.sub(r'^void ', '', name)
    name = re.sub(r'\(.*$', '', name)          # drop the argument list
    return name.replace('tmpnn::', '')[:70]


def load(path):
    if os.path.isdir(path):
        fs = sorted(glob.glob(os.path.join(path, '**', '*kernel_trace.csv'), recursive=True))
        if not fs:
            raise SystemExit('no *kernel_trace.csv under ' + path)
        path = fs[0]
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])))
    rows.sort()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('trace')
    ap.add_argument('--anchor', default='k_gru_bwd_two<1, 2,')
    ap.add_argument('--last', type=int, default=20)
    ap.add_argument('--top', type=int, default=15)
    ap.add_argument('--match', default=None)
    a = ap.parse_args()
    rows = load(a.trace)
    marks = [i for i, r in enumerate(rows) if a.anchor in r[2]]
    if len(marks) < 2:
        raise SystemExit(f'anchor {a.anchor!r} matches {len(marks)} launches: need one launch per step')
    marks = marks[-(a.last + 1):]
    steps = len(marks) - 1
    lo, hi = marks[0], marks[-1]
    span = (rows[hi][0] - rows[lo][0]) / 1e6
    ktime = sum(e - s for s, e, _ in rows[lo:hi]) / 1e6
    idle = overlap = 0.0
    groups = collections.defaultdict(lambda: [0, 0.0])
    end = rows[lo][1]
    prev = rows[lo][2]
    for s, e, n in rows[lo + 1:hi + 1]:
        d = s - end
        if d >= 0:
            idle += d
        else:
            overlap -= d
        g = groups[(prev, n)]
        g[0] += 1
        g[1] += max(d, 0)
        if e > end:
            end, prev = e, n
    print(f'{steps} steps: {span / steps:.3f} ms/step on the device, {(hi - lo) / steps:.1f} launches/step, '
          f'kernel time {ktime / steps:.3f} ms/step, idle between kernels {idle / 1e6 / steps:.3f} ms/step, '
          f'overlap {overlap / 1e6 / steps:.3f} ms/step')
    if a.match:
        sel = {k: v for k, v in groups.items() if a.match in k[0] or a.match in k[1]}
        print(f'boundaries touching {a.match!r}: {sum(v[0] for v in sel.values()) / steps:.1f} per step, '
              f'idle {sum(v[1] for v in sel.values()) / 1e6 / steps:.4f} ms/step')
        groups = sel
    print(f'{"idle ms/step":>12s} {"per step":>8s} {"us each":>8s}  previous -> next')
    for (p, n), (c, t) in sorted(groups.items(), key=lambda kv: -kv[1][1])[:a.top]:
        print(f'{t / 1e6 / steps:12.4f} {c / steps:8.1f} {t / 1e3 / c:8.2f}  {p} -> {n}')


if __name__ == '__main__':
    main()
