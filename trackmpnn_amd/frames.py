"""The CNN's input, from frames as decoded: the resize, and the images of a draw from frames resident on the device.

The reference opens every frame of every chunk with PIL each time the chunk is drawn, mirrors it where the chunk is flipped,
resizes it to the CNN's input size, and runs ToTensor and Normalize on the host (dataset/kitti_mot.py:367-389, :506-511).  The
resized KITTI training set is about 12 GB as uint8 and fits in HBM many times over, so here the frames are uploaded and resized
once (`FrameStore.from_raw`; `FrameStore(...)` takes frames already at the input size) and one launch (`FrameStore.gather`,
tmpnn_frames_gather, csrc/frames.hip) writes the float32 images of a draw's frame plan (`ChunkSampler.frame_plan`):

    frames = FrameStore.from_raw([seq0_frames, seq1_frames, ...], (384, 1280), mean, std)   # [num_frames, h_s, w_s, 3] uint8 each
    drawn = sampler.draw(idx, step)                                                       # a DetectionStore with 'vis'
    images = frames.gather(drawn.plan)                                                    # [T, 3, H, W] float32, no wait
    loss_d = drawn.attach_vis(head, embed_net(images))                                    # rows into X, identity loss [B]

(`trackmpnn_amd.loops.train_epoch(..., vis=VisTraining(...))` is that loop.)  A live frame goes through `FramePrep`:

    prep = FramePrep((384, 1280), mean, std)
    images = prep.prep(frame)                            # [h, w, 3] uint8 as decoded -> [1, 3, H, W] float32 on the device, no wait

(`trackmpnn_amd.online.OnlineVis` hands it to the online tracker.)  Decoding the images stays the user's job.

The resize.  transforms.Resize on a PIL image is Pillow's 8-bit bilinear resize: a horizontal pass (when the width changes)
whose result is rounded to uint8, then a vertical pass (when the height changes), a copy when neither changes.  Each pass is
integer arithmetic over a per-axis table of int32 coefficients that `resize_coeffs` builds in Python floats; `resize_host` is
the definition in numpy (byte-equal to Pillow 12.2.0 at every size tried, tests/test_frame_resize.py), and the device
(tmpnn_frames_resize, csrc/resize.hip) runs the same integer sums on the same tables, so it equals `resize_host` byte for byte.

The value is selected, not computed: `table` [3, 256] float32 holds, for channel c and byte v, the float32 torch ops
`v.float().div(255).sub(mean[c]).div(std[c])` -- ToTensor followed by Normalize -- and the kernels look every pixel up in it,
so the device output equals `frames_host` / `prep_host` bit for bit by construction.

STATED DEVIATION.  The reference mirrors the image before it resizes it; this mirrors the resized frame.  A mirrored bilinear
resize samples the mirrored positions, but the coefficient tables are built in doubles from one end of the axis, so the two
orders are not proven equal in general.  They are checked equal byte for byte at the data sets' sizes (the four KITTI sizes
375 x 1242, 370 x 1224, 374 x 1238, 376 x 1241 and 720 x 1280, to 384 x 1280; tests/test_frame_resize.py holds the KITTI ones).

Limits: every frame of a store has one (H, W), W <= MAX_W = 8192 (a workgroup of the gather stages whole rows in LDS); frame
offsets are int64, so the store is bounded by the device's memory only.  A resize call takes frames of one source size, and a
coefficient row has at most MAX_TAPS = 1024 taps (source over output size up to 511), which keeps the int32 accumulator.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from .train_batch import _to_device

MAX_W = 8192                         # TMPNN_FR_MAX_W
MAX_TAPS = 1024                      # TMPNN_FR_MAX_TAPS
RESIZE_BATCH = 256                   # frames per resize call of from_raw (bounds the workspace)
_PRECISION_BITS = 22
_I63 = 2 ** 63


def _plan_frames(plan) -> np.ndarray:
    fr = np.asarray(plan.frames if hasattr(plan, 'frames') else plan)
    if fr.ndim != 2 or fr.shape[1] != 3 or (fr.size and not np.issubdtype(fr.dtype, np.integer)):
        raise ValueError(f'FrameStore: a frame plan [T, 3] of integers (sequence, frame, mirrored) expected, got {fr.shape} {fr.dtype}')
    return np.ascontiguousarray(fr.astype(np.int64))


# ---- the resize: host definition ---------------------------------------------------------------------------------------------
def resize_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out_size, 2], coef int32 [out_size, ksize]): the bilinear table of one axis, in Python floats (C doubles).
    Output index xx reads the source samples bounds[xx, 0] .. bounds[xx, 0] + bounds[xx, 1] - 1 with the weights coef[xx]
    (2^22 fixed point, zero beyond the taps)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f'resize_coeffs: in_size={in_size}, out_size={out_size}; >= 1 expected')
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    one = float(1 << _PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = []
        ww = 0.0
        for x in range(n):
            a = abs((x + xmin - center + 0.5) / fs)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
        bounds[xx] = (xmin, n)
    return bounds, coef


def _pass_host(src: np.ndarray, axis: int, bounds: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """One pass along `axis` of src uint8: clamp((2^21 + sum_x src[xmin + x] * coef[xx][x]) >> 22, 0, 255) in int32."""
    in_size = src.shape[axis]
    acc = np.full(src.shape[:axis] + (bounds.shape[0],) + src.shape[axis + 1:], 1 << (_PRECISION_BITS - 1), np.int32)
    shape = [1] * src.ndim
    shape[axis] = bounds.shape[0]
    for x in range(coef.shape[1]):
        c = coef[:, x]
        if not c.any():
            continue
        idx = np.minimum(bounds[:, 0] + x, in_size - 1)              # (beyond the taps the coefficient is zero)
        acc += np.take(src, idx, axis=axis).astype(np.int32) * c.reshape(shape)
    return np.clip(acc >> _PRECISION_BITS, 0, 255).astype(np.uint8)


def _check_raw(a, what: str):
    """(tensor or array, shape) of frames [h, w, 3] or [..., h, w, 3] uint8."""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
    shape = tuple(a.shape)
    if len(shape) < 3 or shape[-1] != 3 or a.dtype not in (torch.uint8, np.dtype(np.uint8)) or min(shape[-3:-1]) < 1:
        raise ValueError(f'{what}: frames [..., h, w, 3] uint8 expected, got {shape} {a.dtype}')
    return a, shape


def _check_hw(hw, what: str) -> Tuple[int, int]:
    try:
        H, W = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: the output size (H, W) expected, got {hw!r}') from None
    if H < 1 or W < 1 or W > MAX_W or H > 2 ** 24:
        raise ValueError(f'{what}: an output size of {H} x {W} (1 <= H <= 2^24, 1 <= W <= {MAX_W})')
    return H, W


def resize_host(frames, hw) -> np.ndarray:
    """uint8 [..., h, w, 3] -> uint8 [..., H, W, 3]: the reference's transforms.Resize((H, W)) on a PIL image (module docstring),
    in numpy.  The definition the device is compared with."""
    a, _ = _check_raw(frames, 'resize_host')
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    H, W = _check_hw(hw, 'resize_host')
    h, w = a.shape[-3], a.shape[-2]
    if W != w:
        a = _pass_host(a, a.ndim - 2, *resize_coeffs(w, W))
    if H != h:
        a = _pass_host(a, a.ndim - 3, *resize_coeffs(h, H))
    return np.ascontiguousarray(a) if (W != w or H != h) else a.copy()


def norm_table(mean, std, what: str = 'FrameStore') -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(mean [3], std [3], table float32 [3, 256]): the definition of every output value, ToTensor then Normalize in float32
    torch ops."""
    mean, std = np.asarray(mean, dtype=np.float32).ravel(), np.asarray(std, dtype=np.float32).ravel()
    if mean.size != 3 or std.size != 3:
        raise ValueError(f'{what}: mean / std of length {mean.size} / {std.size}; one value per colour channel (3) expected')
    if not (np.isfinite(mean).all() and np.isfinite(std).all() and (std != 0).all()):
        raise ValueError(f'{what}: mean / std must be finite and std non-zero')
    v = torch.arange(256, dtype=torch.uint8)
    table = torch.stack([v.float().div(255).sub(float(mean[c])).div(float(std[c])) for c in range(3)]).numpy()
    return mean.copy(), std.copy(), table


def prep_host(frames, hw, table) -> np.ndarray:
    """uint8 [h, w, 3] or [n, h, w, 3] -> float32 [n, 3, H, W]: resize_host, then table[c][v] (ToTensor + Normalize; `table`
    [3, 256] as `norm_table` builds it).  The definition of FramePrep.prep."""
    table = np.asarray(table, np.float32)
    if table.shape != (3, 256):
        raise ValueError(f'prep_host: table [3, 256] expected, got {table.shape}')
    r = resize_host(frames, hw)
    if r.ndim == 3:
        r = r[None]
    if r.ndim != 4:
        raise ValueError(f'prep_host: frames [h, w, 3] or [n, h, w, 3] expected, got {r.shape}')
    return table[np.arange(3)[None, :, None, None], r.transpose(0, 3, 1, 2)]


# ---- the resize: device -----------------------------------------------------------------------------------------------------
def _cuda_device(device, what: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != 'cuda':
        if what == 'FrameStore':
            raise RuntimeError('FrameStore: the gather runs on the MI355X HIP kernels only; pass a cuda device, or device=None for '
                               'a host-only store (frames_host)')
        raise RuntimeError(f'{what}: the resize runs on the MI355X HIP kernels only (no CPU path): pass a cuda device '
                           '(prep_host is the host definition)')
    return dev


class _DeviceResize:
    """tmpnn_frames_resize to one output size on one device; the coefficient tables are cached per source size (one upload
    each)."""

    def __init__(self, hw, device: torch.device):
        self.H, self.W = hw
        self.device = device
        self._tables: Dict[Tuple[int, int], tuple] = {}

    def tables(self, h: int, w: int):
        t = self._tables.get((h, w))
        if t is None:
            (bx, cx), (by, cy) = resize_coeffs(w, self.W), resize_coeffs(h, self.H)
            if cx.shape[1] > MAX_TAPS or cy.shape[1] > MAX_TAPS:
                raise ValueError(f'resize: {h} x {w} -> {self.H} x {self.W} needs {max(cx.shape[1], cy.shape[1])} taps; at most '
                                 f'{MAX_TAPS}')
            words = np.concatenate([bx.ravel(), cx.ravel(), by.ravel(), cy.ravel()])
            d = _to_device(words, self.device)
            o = np.cumsum([0, bx.size, cx.size, by.size]) * 4
            t = (d, int(cx.shape[1]), int(cy.shape[1]), tuple(int(d.data_ptr() + v) for v in o))
            self._tables[(h, w)] = t
        return t

    def run(self, src: torch.Tensor, out: torch.Tensor, table_d) -> None:
        """src uint8 [n, h, w, 3] contiguous on the device -> out [n, 3, H, W] contiguous: uint8 (table_d None) or float32 through
        table_d.  Two launches; nothing waits for the device."""
        n, h, w, _ = (int(v) for v in src.shape)
        if n == 0:
            return
        _, kx, ky, (pbx, pcx, pby, pcy) = self.tables(h, w)
        need = int(_lib.fn('tmpnn_frames_resize_ws')(n, h, w, self.H, self.W))
        ws = torch.empty(need, dtype=torch.uint8, device=self.device) if need else None
        a = _lib.CFramesResize(n, h, w, self.H, self.W, kx, ky, 0, src.data_ptr(), pbx, pcx, pby, pcy, _lib.ptr(table_d),
                               out.data_ptr(), _lib.ptr(ws), need)
        _lib.call('tmpnn_frames_resize', C.byref(a), _lib.raw_stream(self.device))


class FramePrep:
    """A live frame to the CNN's input on the device: resize to `input_hw`, ToTensor, Normalize (module docstring).

    input_hw     (input_h, input_w) of the CNN
    mean, std    the three per-channel values of Normalize (after ToTensor's division by 255)
    device       a cuda device (first used by the first `prep`)

        prep.prep(frame)   -> [n, 3, H, W] float32 on the device; `prep_host(frame, input_hw, prep.table)` bit for bit

    frame: [h, w, 3] or [n, h, w, 3] uint8 as decoded, numpy or tensor, on the host or on the device.  A host frame takes one
    pinned, non-blocking upload; the two resize launches follow on the current stream and nothing waits for the device.  The
    coefficient tables are built and uploaded once per source size."""

    def __init__(self, input_hw, mean, std, device='cuda:0'):
        self.H, self.W = _check_hw(input_hw, 'FramePrep')
        self.mean, self.std, self.table = norm_table(mean, std, 'FramePrep')
        self.device = _cuda_device(device, 'FramePrep')
        self._rs = self._table_d = None

    @property
    def input_hw(self) -> Tuple[int, int]:
        return self.H, self.W

    def prep(self, frame) -> torch.Tensor:
        a, shape = _check_raw(frame, 'FramePrep.prep')
        if len(shape) not in (3, 4):
            raise ValueError(f'FramePrep.prep: a frame [h, w, 3] or frames [n, h, w, 3] expected, got {shape}')
        if self._rs is None:
            if self.device.index is None:
                self.device = torch.device('cuda', torch.cuda.current_device())
            self._rs = _DeviceResize((self.H, self.W), self.device)
            self._table_d = torch.from_numpy(self.table).to(self.device)
        if isinstance(a, torch.Tensor) and a.device.type == 'cuda':
            if a.device != self.device:
                raise ValueError(f'FramePrep.prep: the frame is on {a.device}, the prep on {self.device}')
            src = a.detach().contiguous()
        else:
            src = _to_device(a.detach() if isinstance(a, torch.Tensor) else a, self.device)     # pinned staging, asynchronous copy
        src = src.reshape((-1,) + shape[-3:])
        out = torch.empty((src.shape[0], 3, self.H, self.W), dtype=torch.float32, device=self.device)
        self._rs.run(src, out, self._table_d)
        return out


class FrameStore:
    """The resized frames of a set of sequences, resident on `device` (None: host only, for `frames_host`).

    sequences_of_frames   per sequence an array (or tensor) [num_frames, H, W, 3] uint8: the frames as the CNN sees them, already
                          resized to its input size; all of one (H, W).  Kept planar ([3][H][W] per frame) in one buffer.
                          (`FrameStore.from_raw` takes the frames as decoded and resizes them on the device.)
    mean, std             the three per-channel values of Normalize (after ToTensor's division by 255)

        store.gather(plan)        -> [T, 3, H, W] float32 on the device, one launch, no wait for the device
        store.frames_host(plan)   -> the same in numpy: the definition

    Host tables: `num_frames`, `seq_base` int64 [nseq + 1] (frame f of sequence s is frame seq_base[s] + f of the buffer),
    `table` float32 [3, 256], and, for a host-only store, `planar` uint8 [frames, 3, H, W]; `raw_hw` int64 [nseq, 2]: the
    (h, w) the frames of every sequence were decoded at -- the `im_hw` of the VisHead call (the store's own size unless the
    store was built by `from_raw`)."""

    def __init__(self, sequences_of_frames, mean, std, device='cuda:0'):
        seqs = self._setup(sequences_of_frames, None, mean, std)
        self.device, self.planar, self.planar_d = None, None, None
        if device is None:
            self.planar = np.concatenate([np.ascontiguousarray(torch.as_tensor(a).numpy().transpose(0, 3, 1, 2)) for a in seqs])
            return
        self._alloc(device)
        for i, a in enumerate(seqs):
            self.planar_d[int(self.seq_base[i]):int(self.seq_base[i + 1])].copy_(torch.as_tensor(a).to(self.device).permute(0, 3, 1, 2))

    def _setup(self, sequences_of_frames, input_hw, mean, std) -> list:
        """The host tables from the sequences' shapes.  input_hw None: frames at the store's size, all of one (H, W); else the
        store's size, and every sequence has a size of its own."""
        mean, std, table = norm_table(mean, std)
        seqs = list(sequences_of_frames)
        if not seqs:
            raise ValueError('FrameStore: no sequences')
        hw, nf, raw = (None if input_hw is None else _check_hw(input_hw, 'FrameStore.from_raw')), [], []
        for i, a in enumerate(seqs):
            shape, dtype = tuple(a.shape), (a.dtype if isinstance(a, torch.Tensor) else np.asarray(a).dtype)
            if len(shape) != 4 or shape[3] != 3 or dtype not in (torch.uint8, np.dtype(np.uint8)):
                raise ValueError(f'FrameStore: sequence {i}: frames [num_frames, H, W, 3] uint8 expected, got {shape} {dtype}')
            if shape[0] < 1 or shape[1] < 1 or shape[2] < 1:
                raise ValueError(f'FrameStore: sequence {i}: frames of shape {shape}')
            if hw is None:
                hw = shape[1:3]
            if input_hw is None and shape[1:3] != hw:
                raise ValueError(f'FrameStore: sequence {i}: frames of {shape[1]} x {shape[2]}, those before of {hw[0]} x {hw[1]}: '
                                 'every frame of a store has one size (the CNN\'s input size)')
            nf.append(shape[0])
            raw.append(shape[1:3])
        self.H, self.W = int(hw[0]), int(hw[1])
        if self.W > MAX_W or self.H > 2 ** 24:
            raise ValueError(f'FrameStore: frames of {self.H} x {self.W} (H <= 2^24, W <= {MAX_W})')
        self.nseq = len(seqs)
        self.num_frames = np.asarray(nf, np.int64)
        self.raw_hw = np.asarray(raw, np.int64).reshape(self.nseq, 2)
        self.seq_base = np.concatenate([[0], np.cumsum(self.num_frames)]).astype(np.int64)
        self.nframes = int(self.seq_base[-1])
        self.frame_bytes = 3 * self.H * self.W
        if self.nframes * self.frame_bytes >= _I63:
            raise ValueError('FrameStore: the frames do not fit in int64 bytes')
        self.mean, self.std, self.table = mean, std, table
        return seqs

    def _alloc(self, device) -> None:
        """One buffer for every frame, and the two small tables, on the device."""
        dev = _cuda_device(device, 'FrameStore')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        # one buffer, one sequence uploaded at a time (the host never holds a second copy of the whole set)
        self.planar_d = torch.empty((self.nframes, 3, self.H, self.W), dtype=torch.uint8, device=dev)
        self.seq_base_d = torch.from_numpy(self.seq_base).to(dev)
        self.table_d = torch.from_numpy(self.table).to(dev)

    @classmethod
    def from_raw(cls, sequences_of_frames, input_hw, mean, std, device='cuda:0') -> 'FrameStore':
        """A store of frames as decoded: per sequence [num_frames, h_s, w_s, 3] uint8, one size per sequence (sizes may differ
        between sequences).  One sequence at a time is uploaded and resized on the device to `input_hw` (tmpnn_frames_resize,
        bytes equal to `resize_host`) into the store's planar buffer; `gather` and `frames_host` then behave as for any store.
        device=None fills `planar` through `resize_host`.  `raw_hw` records the sequences' (h_s, w_s)."""
        self = cls.__new__(cls)
        seqs = self._setup(sequences_of_frames, input_hw, mean, std)
        self.device, self.planar, self.planar_d = None, None, None
        if device is None:
            self.planar = np.concatenate([np.ascontiguousarray(resize_host(a, (self.H, self.W)).transpose(0, 3, 1, 2)) for a in seqs])
            return self
        self._alloc(device)
        rs = _DeviceResize((self.H, self.W), self.device)
        for i, a in enumerate(seqs):
            src = torch.as_tensor(a).to(self.device).contiguous()
            base = int(self.seq_base[i])
            for k in range(0, int(src.shape[0]), RESIZE_BATCH):
                part = src[k:k + RESIZE_BATCH]
                rs.run(part, self.planar_d[base + k:base + k + int(part.shape[0])], None)
        return self

    def _check(self, plan) -> np.ndarray:
        """The plan's rows, validated on the host: nothing is launched for a plan outside the store."""
        fr = _plan_frames(plan)
        if fr.shape[0] == 0:
            return fr
        s, f, m = fr[:, 0], fr[:, 1], fr[:, 2]
        if s.min() < 0 or s.max() >= self.nseq:
            raise ValueError(f'FrameStore: the plan names sequence {int(s.max() if s.min() >= 0 else s.min())} of {self.nseq}')
        bad = np.nonzero((f < 0) | (f >= self.num_frames[s]))[0]
        if bad.size:
            i = int(bad[0])
            raise ValueError(f'FrameStore: the plan names frame {int(f[i])} of sequence {int(s[i])}, which has '
                             f'{int(self.num_frames[s[i]])} frames')
        if ((m != 0) & (m != 1)).any():
            raise ValueError('FrameStore: the mirrored flag of a plan row is 0 or 1')
        if fr.shape[0] * self.frame_bytes * 4 >= _I63 or fr.shape[0] >= 2 ** 31:
            raise ValueError(f'FrameStore: {fr.shape[0]} images of {self.frame_bytes} values do not fit in int64 bytes')
        return fr

    def frames_host(self, plan) -> np.ndarray:
        """The definition of gather(plan) in numpy: [T, 3, H, W] float32, image i = frame plan.frames[i] (mirrored along W where
        flagged), every value table[c][v]."""
        fr = self._check(plan)
        out = np.empty((fr.shape[0], 3, self.H, self.W), np.float32)
        ch = np.arange(3)[:, None, None]
        for i, (s, f, m) in enumerate(fr):
            g = int(self.seq_base[s] + f)
            img = self.planar[g] if self.planar is not None else self.planar_d[g].cpu().numpy()
            out[i] = self.table[ch, img[:, :, ::-1] if m else img]
        return out

    def gather(self, plan) -> torch.Tensor:
        """[T, 3, H, W] float32 on the device: the CNN's input for the images of a frame plan (a FramePlan, or its `frames`
        [T, 3] array), in one launch; the plan is the one small upload, and nothing waits for the device.  Bit for bit
        frames_host(plan).  T = 0 launches nothing."""
        if self.device is None:
            raise RuntimeError('FrameStore.gather runs on the MI355X HIP kernels only (no CPU path): build the FrameStore on a cuda '
                               'device (frames_host is the host definition)')
        fr = self._check(plan)
        T = int(fr.shape[0])
        out = torch.empty((T, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        if T == 0:
            return out
        plan_d = _to_device(fr.ravel(), self.device)
        a = _lib.CFramesGather(T, self.H, self.W, self.nseq, self.nframes, self.planar_d.data_ptr(), self.seq_base_d.data_ptr(),
                               plan_d.data_ptr(), self.table_d.data_ptr(), out.data_ptr())
        _lib.call('tmpnn_frames_gather', C.byref(a), _lib.raw_stream(self.device))
        return out
