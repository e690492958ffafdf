"""The CNN's input for the frames of a draw, from frames resident on the device.

The reference opens every frame of every chunk with PIL each time the chunk is drawn, mirrors it where the chunk is flipped,
resizes it to the CNN's input size, and runs ToTensor and Normalize on the host (dataset/kitti_mot.py:367-389, :506-511).  The
resized KITTI training set is about 12 GB as uint8 and fits in HBM many times over, so here the resized frames are uploaded
once (`FrameStore`) and one launch (`FrameStore.gather`, tmpnn_frames_gather, csrc/frames.hip) writes the float32 images of a
draw's frame plan (`ChunkSampler.frame_plan`):

    frames = FrameStore([seq0_frames, seq1_frames, ...], mean, std, device='cuda:0')     # [num_frames, H, W, 3] uint8 each
    drawn = sampler.draw(idx, step)                                                       # a DetectionStore with 'vis'
    images = frames.gather(drawn.plan)                                                    # [T, 3, H, W] float32, no wait
    loss_d = drawn.attach_vis(head, embed_net(images))                                    # rows into X, identity loss [B]

(`trackmpnn_amd.loops.train_epoch(..., vis=VisTraining(...))` is that loop.)  Decoding and resizing the images stay the user's job.

The value is selected, not computed: `table` [3, 256] float32 holds, for channel c and byte v, the float32 torch ops
`v.float().div(255).sub(mean[c]).div(std[c])` -- ToTensor followed by Normalize -- and the kernel looks every pixel up in it,
so the device output equals `frames_host` bit for bit by construction.

STATED DEVIATION.  The reference mirrors the image before it resizes it; this mirrors the resized frame.  The two agree up to
the resize's own uint8 rounding (a mirrored bilinear resize samples the mirrored positions; the rounding of the interpolated
values to uint8 need not be symmetric).

Limits: every frame of a store has one (H, W), W <= MAX_W = 8192 (a workgroup stages whole rows in LDS); frame offsets are
int64, so the store is bounded by the device's memory only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .train_batch import _to_device

MAX_W = 8192                         # TMPNN_FR_MAX_W
_I63 = 2 ** 63


def _plan_frames(plan) -> np.ndarray:
    fr = np.asarray(plan.frames if hasattr(plan, 'frames') else plan)
    if fr.ndim != 2 or fr.shape[1] != 3 or (fr.size and not np.issubdtype(fr.dtype, np.integer)):
        raise ValueError(f'FrameStore: a frame plan [T, 3] of integers (sequence, frame, mirrored) expected, got {fr.shape} {fr.dtype}')
    return np.ascontiguousarray(fr.astype(np.int64))


class FrameStore:
    """The resized frames of a set of sequences, resident on `device` (None: host only, for `frames_host`).

    sequences_of_frames   per sequence an array (or tensor) [num_frames, H, W, 3] uint8: the frames as the CNN sees them, already
                          resized to its input size; all of one (H, W).  Kept planar ([3][H][W] per frame) in one buffer.
    mean, std             the three per-channel values of Normalize (after ToTensor's division by 255)

        store.gather(plan)        -> [T, 3, H, W] float32 on the device, one launch, no wait for the device
        store.frames_host(plan)   -> the same in numpy: the definition

    Host tables: `num_frames`, `seq_base` int64 [nseq + 1] (frame f of sequence s is frame seq_base[s] + f of the buffer),
    `table` float32 [3, 256], and, for a host-only store, `planar` uint8 [frames, 3, H, W]."""

    def __init__(self, sequences_of_frames, mean, std, device='cuda:0'):
        mean, std = np.asarray(mean, dtype=np.float32).ravel(), np.asarray(std, dtype=np.float32).ravel()
        if mean.size != 3 or std.size != 3:
            raise ValueError(f'FrameStore: mean / std of length {mean.size} / {std.size}; one value per colour channel (3) expected')
        if not (np.isfinite(mean).all() and np.isfinite(std).all() and (std != 0).all()):
            raise ValueError('FrameStore: mean / std must be finite and std non-zero')
        seqs = list(sequences_of_frames)
        if not seqs:
            raise ValueError('FrameStore: no sequences')
        hw, nf = None, []
        for i, a in enumerate(seqs):
            shape, dtype = tuple(a.shape), (a.dtype if isinstance(a, torch.Tensor) else np.asarray(a).dtype)
            if len(shape) != 4 or shape[3] != 3 or dtype not in (torch.uint8, np.dtype(np.uint8)):
                raise ValueError(f'FrameStore: sequence {i}: frames [num_frames, H, W, 3] uint8 expected, got {shape} {dtype}')
            if shape[0] < 1 or shape[1] < 1 or shape[2] < 1:
                raise ValueError(f'FrameStore: sequence {i}: frames of shape {shape}')
            if hw is None:
                hw = shape[1:3]
            if shape[1:3] != hw:
                raise ValueError(f'FrameStore: sequence {i}: frames of {shape[1]} x {shape[2]}, those before of {hw[0]} x {hw[1]}: '
                                 'every frame of a store has one size (the CNN\'s input size)')
            nf.append(shape[0])
        self.H, self.W = int(hw[0]), int(hw[1])
        if self.W > MAX_W or self.H > 2 ** 24:
            raise ValueError(f'FrameStore: frames of {self.H} x {self.W} (H <= 2^24, W <= {MAX_W})')
        self.nseq = len(seqs)
        self.num_frames = np.asarray(nf, np.int64)
        self.seq_base = np.concatenate([[0], np.cumsum(self.num_frames)]).astype(np.int64)
        self.nframes = int(self.seq_base[-1])
        self.frame_bytes = 3 * self.H * self.W
        if self.nframes * self.frame_bytes >= _I63:
            raise ValueError('FrameStore: the frames do not fit in int64 bytes')
        self.mean, self.std = mean.copy(), std.copy()
        # the definition of every output value: ToTensor, then Normalize, in float32 torch ops
        v = torch.arange(256, dtype=torch.uint8)
        self.table = torch.stack([v.float().div(255).sub(float(mean[c])).div(float(std[c])) for c in range(3)]).numpy()
        self.device, self.planar, self.planar_d = None, None, None
        if device is None:
            self.planar = np.concatenate([np.ascontiguousarray(torch.as_tensor(a).numpy().transpose(0, 3, 1, 2)) for a in seqs])
            return
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError('FrameStore: the gather runs on the MI355X HIP kernels only; pass a cuda device, or device=None for '
                               'a host-only store (frames_host)')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        # one buffer, one sequence uploaded at a time (the host never holds a second copy of the whole set)
        self.planar_d = torch.empty((self.nframes, 3, self.H, self.W), dtype=torch.uint8, device=dev)
        for i, a in enumerate(seqs):
            self.planar_d[int(self.seq_base[i]):int(self.seq_base[i + 1])].copy_(torch.as_tensor(a).to(dev).permute(0, 3, 1, 2))
        self.seq_base_d = torch.from_numpy(self.seq_base).to(dev)
        self.table_d = torch.from_numpy(self.table).to(dev)

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
