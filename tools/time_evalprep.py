"""Time of the benchmark preprocessing on the device (EvalPrep.apply) next to the host definition, next to tmpnn_hota on the same
set, and inside a validation pass.

    python tools/time_evalprep.py --out profiles/evalprep_run.md

A KITTI-validation-shaped set made by evalprep.synth_prep_sequence (nothing outside the tree is read): 10 sequences of 150 to
600 frames, about 10 rows a frame on either side (objects of the class, distractors, other classes, ignore regions; stray
hypotheses in regions and below 25 px).  In ONE process:

  (a) evalprep_host over every sequence (numpy + scipy)            wall time of the loop (--host-reps repetitions)
  (b) EvalPrep.apply + read (one packed upload, one clear and one   wall time from the call to the returned dicts, which ends
      launch, one device -> host copy; the store was uploaded       in the copy's synchronise: --reps repetitions after --warmup,
      before)                                                       median and spread
  (c) HotaEvaluator.evaluate + read over eval_sequences(), scoring  the same, in the same loop, alternating with (b)
      the filtered tracks handed over on the device
  (d) device events around the launches of (b) and of (c) alone     the device time of tmpnn_evalprep next to tmpnn_hota
  (e) validate(...) over the first --val-seqs sequences of the set  wall time of the pass without `prep` (the pass as it was
      with a small random model, MotEvaluator + HotaEvaluator       before this stage existed) and with it, alternating

(a) and (b) must agree in every row of tracks_out and every count (checked on every repetition).  Not bench.py: nothing here
gates a change."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_set():
    from trackmpnn_amd.evalprep import synth_prep_sequence
    lens = (150, 200, 250, 300, 350, 400, 450, 500, 550, 600)
    return [synth_prep_sequence(9300 + i, L, objects=7, distractors=2, others=2, regions=2, shuffle=bool(i % 2)) for i, L in enumerate(lens)]


def stats(v):
    v = np.asarray(v, np.float64)
    return f'{np.median(v):.3f} | {v.min():.3f} | {v.max():.3f}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--val-seqs', type=int, default=2, help='sequences of the validation pass of (e); 0: skip it')
    ap.add_argument('--val-reps', type=int, default=3)
    ap.add_argument('--out', default=None, help='write the tables (markdown) here as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_evalprep needs the MI355X: no timing is taken without it')
    from trackmpnn_amd import TrackMPNN, validate
    from trackmpnn_amd.evalprep import COUNT_KEYS, KITTI_CAR, EvalPrep, evalprep_host, prep_overall
    from trackmpnn_amd.hota import HotaEvaluator
    from trackmpnn_amd.moteval import MotEvaluator
    dev = 'cuda:0'
    seqs = make_set()
    tracks = [q['tracks'] for q in seqs]
    host_ms = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ref = [evalprep_host(q, q['tracks'], KITTI_CAR) for q in seqs]
        host_ms.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    ep = EvalPrep(seqs, KITTI_CAR, dev)
    torch.cuda.synchronize()
    build_ms = 1e3 * (time.perf_counter() - t0)
    hev = HotaEvaluator(ep.eval_sequences(), dev)
    prep_ms, hota_ms, prep_ev, hota_ev = [], [], [], []
    for r in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ep.apply(tracks)
        per, overall = ep.read()
        t1 = time.perf_counter()
        filt = ep.filtered_tracks()
        for s, (f, c, h) in enumerate(zip(filt, per, ref)):
            assert np.array_equal(f.cpu().numpy(), h[0]) and c == h[2], f'sequence {s}: the device differs from the host'
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        hev.evaluate(filt)
        hev.read()
        t3 = time.perf_counter()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        dtracks = [f.clone() for f in filt]
        torch.cuda.synchronize()
        e[0].record()
        ep.apply(dtracks)
        e[1].record()
        e[2].record()
        hev.evaluate(dtracks)
        e[3].record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            prep_ms.append(1e3 * (t1 - t0))
            hota_ms.append(1e3 * (t3 - t2))
            prep_ev.append(e[0].elapsed_time(e[1]))
            hota_ev.append(e[2].elapsed_time(e[3]))
    st = ep.store
    nf = sum(int(x) for x in st.seq[:, 5])
    tot = prep_overall([h[2] for h in ref])
    h = float(np.median(host_ms))
    text = ['### KITTI-validation-shaped set', '',
            f'{len(seqs)} sequences, {nf} frames, {st.n_gt} GT rows, {st.n_det} detection rows; counts ' + ', '.join(f'{k} {tot[k]}' for k in COUNT_KEYS)
            + f'; {a.reps} repetitions after {a.warmup} warm-ups, host {a.host_reps} repetitions; every repetition equal to the host in every row '
            f'and count; the store is built and uploaded once ({build_ms:.1f} ms, not in the figures).', '',
            '| path | median ms | min | max |', '|---|---|---|---|',
            f'| (a) `evalprep_host` over the sequences | {stats(host_ms)} |',
            f'| (b) `EvalPrep.apply` + `read`, wall | {stats(prep_ms)} |',
            f'| (c) `HotaEvaluator.evaluate` + `read` on the filtered tracks, wall | {stats(hota_ms)} |',
            f'| (d) `tmpnn_evalprep` (device tracks; clear + launch), device events | {stats(prep_ev)} |',
            f'| (d) `tmpnn_hota` (device tracks; clear + four launches), device events | {stats(hota_ev)} |',
            '', f'host / device (a) / (b): {h / np.median(prep_ms):.0f}x; evalprep / hota by device events: {np.median(prep_ev) / np.median(hota_ev):.3f}', '']
    row = dict(sequences=len(seqs), frames=nf, host_ms=h, prep_wall_ms=float(np.median(prep_ms)), hota_wall_ms=float(np.median(hota_ms)),
               prep_event_ms=float(np.median(prep_ev)), hota_event_ms=float(np.median(hota_ev)), store_build_ms=build_ms)
    if a.val_seqs > 0:
        vs = []
        for i, q in enumerate(seqs[:a.val_seqs]):
            q = dict(q)
            q['y'] = torch.from_numpy(np.stack([q['det_frame'], q['tracks']], 1))[None]
            q['X'] = torch.randn(1, q['y'].shape[1], 8, generator=torch.Generator().manual_seed(700 + i))
            vs.append(q)
        torch.manual_seed(9)
        model = TrackMPNN('2d', 3, 32, 0, 'diff').to(dev).eval()
        gp = torch.Generator().manual_seed(17)
        with torch.no_grad():                                          # scores on both sides of 0.5
            for k, prm in model.named_parameters():
                prm.add_((0.1 * torch.randn(prm.shape, generator=gp)).to(dev))
                if k.startswith('output_transform') and k.endswith('bias'):
                    prm.copy_((0.5 * torch.randn(prm.shape, generator=gp)).to(dev))
        vp = EvalPrep(vs, KITTI_CAR, dev)
        es = vp.eval_sequences()
        mev, hev2 = MotEvaluator(es, dev, identity=True), HotaEvaluator(es, dev)
        without, with_ = [], []
        for r in range(1 + a.val_reps):
            for use, acc in ((None, without), (vp, with_)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = validate(model, es, mev, cur_win_size=3, hota_evaluator=hev2, prep=use)
                dt = 1e3 * (time.perf_counter() - t0)
                if r > 0:
                    acc.append(dt)
        vf = sum(int(x) for x in vp.store.seq[:, 5])
        text += ['### A validation pass', '',
                 f'`validate` over {len(vs)} sequences ({vf} frames) with a small random model (hidden size 32, window 3), `MotEvaluator(identity=True)` '
                 f'and `HotaEvaluator`; {a.val_reps} repetitions after one warm-up, the two alternating; the pass ends in the evaluators\' reads.', '',
                 '| pass | median ms | min | max |', '|---|---|---|---|',
                 f'| without `prep` (the pass as before) | {stats(without)} |', f'| with `prep=ep` | {stats(with_)} |', '']
        row.update(validate_ms=float(np.median(without)), validate_prep_ms=float(np.median(with_)), validate_frames=vf, kept=out['prep']['kept'])
    out = '\n'.join(text)
    print(out)
    print(json.dumps(dict(tool='time_evalprep', device=torch.cuda.get_device_name(0), **row)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
