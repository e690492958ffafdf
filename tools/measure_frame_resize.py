#!/usr/bin/env python
"""Time the frame resize on the MI355X and write the report (profiles/frame_resize.md).

    python tools/measure_frame_resize.py --out profiles/frame_resize.md

For one KITTI frame (375 x 1242 -> 384 x 1280) and for a batch of 64: the device time per call of tmpnn_frames_resize (device
events around a run of calls, both output forms) and the bytes it moves against the HBM peak; the end-to-end time of
FramePrep.prep from a host frame (host clock, ending in a synchronise); and, where Pillow is installed, the host path it
replaces (Image.resize + ToTensor + Normalize).  Every figure is the median (and the minimum) of ROUNDS rounds; the rounds of
the arms alternate.  The outputs are compared with the host definition before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H_IN, W_IN, H_OUT, W_OUT = 375, 1242, 384, 1280
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PEAK_TBS = 8.0                                  # HBM peak of the MI355X, TB/s (data sheet)
ROUNDS = 7


def moved_bytes(n: int, float_out: bool) -> int:
    """What the two launches must read and write: the source, the horizontal pass's result written and read back, the output."""
    return n * (H_IN * W_IN * 3 + 2 * H_IN * W_OUT * 3 + 3 * H_OUT * W_OUT * (4 if float_out else 1))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='profiles/frame_resize.md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('measure_frame_resize: needs the GPU (nothing is timed without one)')
    import __graft_entry__
    __graft_entry__.build()
    from trackmpnn_amd import FramePrep, prep_host, resize_host
    from trackmpnn_amd.frames import _DeviceResize
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    prep = FramePrep((H_OUT, W_OUT), MEAN, STD, device=dev)
    lines = ['# Frame resize on the device (`tmpnn_frames_resize`, `csrc/resize.hip`)', '',
             f'`python tools/measure_frame_resize.py` on {torch.cuda.get_device_name(0)}; KITTI frames {H_IN} x {W_IN} -> '
             f'{H_OUT} x {W_OUT}, random bytes; median (minimum) of {ROUNDS} alternating rounds.', '']

    # ---- correctness at the sizes timed
    one = rng.integers(0, 256, (1, H_IN, W_IN, 3), dtype=np.uint8)
    got = prep.prep(one[0]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), prep_host(one, (H_OUT, W_OUT), prep.table).view(np.uint32))
    rs = _DeviceResize((H_OUT, W_OUT), dev)
    table_d = torch.from_numpy(prep.table).to(dev)

    # ---- device time per call
    lines += ['## Device time per call (device events around a run of back-to-back calls)', '',
              '| frames | output | calls per round | time per call | bytes moved | rate | of the 8 TB/s peak |', '|---|---|---|---|---|---|---|']
    arms = []
    for n, calls in ((1, 400), (64, 25)):
        src = torch.from_numpy(rng.integers(0, 256, (n, H_IN, W_IN, 3), dtype=np.uint8)).to(dev)
        if n == 64:
            u8 = torch.empty((n, 3, H_OUT, W_OUT), dtype=torch.uint8, device=dev)
            rs.run(src, u8, None)
            assert np.array_equal(u8[-1].cpu().numpy(), resize_host(src[-1].cpu().numpy(), (H_OUT, W_OUT)).transpose(2, 0, 1))
        for float_out in (False, True):
            out = torch.empty((n, 3, H_OUT, W_OUT), dtype=torch.float32 if float_out else torch.uint8, device=dev)
            arms.append((n, calls, float_out, src, out, []))
    for r in range(ROUNDS + 1):                                 # (round 0 warms every shape up)
        for n, calls, float_out, src, out, ts in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                rs.run(src, out, table_d if float_out else None)
            e1.record()
            torch.cuda.synchronize()
            if r:
                ts.append(e0.elapsed_time(e1) * 1e3 / calls)    # us per call
    for n, calls, float_out, src, out, ts in arms:
        med, mn = statistics.median(ts), min(ts)
        b = moved_bytes(n, float_out)
        rate = b / (med * 1e-6) / 1e12
        lines.append(f'| {n} | {"float32" if float_out else "uint8"} | {calls} | {med:.1f} us ({mn:.1f}) | {b / 1e6:.1f} MB | '
                     f'{rate:.2f} TB/s | {100 * rate / PEAK_TBS:.1f} % |')
    lines += ['', 'A call is two launches (horizontal pass into the uint8 workspace, vertical pass from it) plus the workspace\'s '
              'allocation from torch\'s caching allocator.  The time per call above includes the host\'s enqueue wherever the device '
              'outruns it.', '']

    # ---- end to end from a host frame
    lines += ['## `FramePrep.prep` from a host frame (host clock; pinned upload, two launches, one synchronise at the end)', '',
              '| frames | calls per round | time per call | per frame |', '|---|---|---|---|']
    e2e = []
    for n, calls in ((1, 200), (64, 10)):
        host = rng.integers(0, 256, (n, H_IN, W_IN, 3), dtype=np.uint8)
        e2e.append((n, calls, host[0] if n == 1 else host, []))
    for r in range(ROUNDS + 1):
        for n, calls, host, ts in e2e:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                x = prep.prep(host)
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) * 1e6 / calls)
    for n, calls, host, ts in e2e:
        med, mn = statistics.median(ts), min(ts)
        lines.append(f'| {n} | {calls} | {med:.0f} us ({mn:.0f}) | {med / n:.0f} us |')
    lines.append('')

    # ---- the host path it replaces
    lines += ['## The host path it replaces (Pillow resize + ToTensor + Normalize of one frame, on this machine\'s CPU)', '']
    try:
        import PIL
        from PIL import Image
    except ImportError:
        lines += ['Pillow is not installed on the GPU machine: not measured here.', '']
    else:
        img = Image.fromarray(one[0])
        m, s = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
        ts_r, ts_n = [], []
        for r in range(ROUNDS + 1):
            t0 = time.perf_counter()
            for _ in range(20):
                res = img.resize((W_OUT, H_OUT), Image.BILINEAR)
            t1 = time.perf_counter()
            for _ in range(20):
                x = torch.from_numpy(np.asarray(res)).permute(2, 0, 1).float().div(255).sub(m).div(s)
            t2 = time.perf_counter()
            if r:
                ts_r.append((t1 - t0) * 1e6 / 20)
                ts_n.append((t2 - t1) * 1e6 / 20)
        lines += [f'Pillow {PIL.__version__}, torch with {torch.get_num_threads()} threads: resize {statistics.median(ts_r):.0f} us '
                  f'({min(ts_r):.0f}), ToTensor + Normalize {statistics.median(ts_n):.0f} us ({min(ts_n):.0f}) per frame.', '']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
