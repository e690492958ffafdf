"""The visual head: the embedding CNN's feature map read at each box centre, softmaxed into the 128 'vis' feature columns, and
the identity loss over the same rows (reference dataset/kitti_mot.py:391-412, 558-566; models/loss.py:162-181 FairMOTLoss).

    vis_centres_host    the box-centre pixel of every detection on the feature map, in numpy.  The DEFINITION of the index.
    vis_pixels_host     those centres clamped to the map, the flag of the clamped ones, the pixel index the device saves
    vis_head_host       logits, standardised softmax rows, per-chunk identity loss and its gradient wrt the maps, in numpy, in the
                        dtype of `maps` (float64: the yardstick of the device tests)
    VisHead             the same on the device (tmpnn_vis_head_fwd, tmpnn_vis_head_bwd; csrc/vishead.hip): `rows()` for inference,
                        `forward()` a torch.autograd.Function whose backward hands d(loss)/d(maps) to the user's CNN, `record()`;
                        `forward(loss='embedding')` puts the reference's EmbeddingLoss (embedloss.py) in the identity loss's place

The rule.  A detection with box x1 y1 x2 y2 in an image of im_h x im_w pixels that the CNN sees resized to input_h x input_w and
answers with a map of 1 / down_ratio that size reads the pixel

    cx = trunc(((x1 + x2) / 2) * input_w / im_w / down_ratio),   cy = trunc(((y1 + y2) / 2) * input_h / im_h / down_ratio)

with EVERY operation in float32, in this order, and truncation toward zero.  That is the reference's arithmetic on its float32
boxes; the same formula in float64 truncates differently for about one box in 60 000, so the float32 order is the definition.
`logits` [D, 128] are maps[map_of, :, cy, cx]; the feature columns are rows = (softmax(logits) - mean) / std.  Per chunk b (rows
offsets[b] .. offsets[b + 1]) the identity loss is the mean over the rows with track >= 0 of logsumexp(logits) -
logits[track % 128]: nn.CrossEntropyLoss over the labels the reference maps with `id % 128`, -1 ignored.  For an upstream
gradient g [B], every labelled row adds g[b] / n_b * (softmax - onehot) at its pixel of dmaps; rows that share a pixel are summed
in ascending row order.

STATED DEVIATIONS.  (1) A centre outside the map is clamped to [0, Hm - 1] x [0, Wm - 1] and counted (`record()`); the reference
raises IndexError for an index that is too large and wraps a negative one to the other side of the map.  (2) A chunk without a
labelled row has loss 0 and a zero gradient; the reference returns 0 for a chunk without rows but NaN (with a zero gradient) for
a chunk whose rows are all false positives.

Out of scope: the CNN itself (the user's torch module) and image loading.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

VIS_COLS = 128                 # channels of the embedding map = width of the 'vis' feature group
FLAG_CLAMPED, FLAG_MAP = 1, 2  # per-row flags of the device (csrc/vishead.hip): centre clamped, map_of outside [0, T)
COUNT_WORDS = 4                # per chunk: labelled rows, clamped rows, rows with a flag the device cannot serve, rows
MAX_DETS = 2 ** 17             # detections per call (csrc/vishead.hip VH_MAX_D): the backward's pairwise scan grows with D * D
_I32 = 2 ** 31


def _box32(box) -> np.ndarray:
    if isinstance(box, torch.Tensor):
        box = box.detach().cpu().numpy()
    b = np.ascontiguousarray(np.asarray(box, dtype=np.float32).reshape(-1, 4))
    if not np.isfinite(b).all():
        raise ValueError('vis head: a box is not finite')
    return b


def _im_hw32(im_hw, D: int) -> np.ndarray:
    """[D, 2] float32 (h, w) from one pair or one pair per row."""
    if isinstance(im_hw, torch.Tensor):
        im_hw = im_hw.detach().cpu().numpy()
    a = np.asarray(im_hw, dtype=np.float32)
    if a.shape == (2,):
        a = np.broadcast_to(a[None, :], (D, 2))
    if a.shape != (D, 2):
        raise ValueError(f'vis head: im_hw of shape {a.shape}; (h, w) or [{D}, 2] expected')
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError('vis head: image sizes must be finite and positive')
    return a


def _geometry(input_hw, down_ratio) -> Tuple[np.float32, np.float32, np.float32]:
    ih, iw, dr = np.float32(input_hw[0]), np.float32(input_hw[1]), np.float32(down_ratio)
    if not (np.isfinite([ih, iw, dr]).all() and ih > 0 and iw > 0 and dr > 0):
        raise ValueError(f'vis head: input_hw={tuple(input_hw)}, down_ratio={down_ratio}; finite and positive expected')
    return ih, iw, dr


def vis_centres_host(box, im_hw, input_hw, down_ratio) -> Tuple[np.ndarray, np.ndarray]:
    """(cy, cx) int64 [D]: the map pixel under every box centre (module docstring), not clamped.  box float32 [D, 4] x1 y1 x2 y2;
    im_hw [D, 2] or (h, w); input_hw (input_h, input_w); every operation float32."""
    b = _box32(box)
    im = _im_hw32(im_hw, b.shape[0])
    ih, iw, dr = _geometry(input_hw, down_ratio)
    two = np.float32(2)
    with np.errstate(over='ignore'):
        cx = ((b[:, 0] + b[:, 2]) / two) * iw / im[:, 1] / dr
        cy = ((b[:, 1] + b[:, 3]) / two) * ih / im[:, 0] / dr
    assert cx.dtype == np.float32 and cy.dtype == np.float32
    lim = np.float32(2.0 ** 62)                                     # (an overflowed centre stays a huge index of its sign)
    tr = lambda c: np.clip(np.trunc(c), -lim, lim).astype(np.int64)
    return tr(cy), tr(cx)


def vis_pixels_host(cy, cx, map_of, Hm: int, Wm: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(cy, cx, clamped, pix): the centres clamped to the Hm x Wm map, which rows were clamped, and the pixel index
    (map_of * Hm + cy) * Wm + cx that the device saves per row."""
    cy, cx = np.asarray(cy, np.int64), np.asarray(cx, np.int64)
    y, x = np.clip(cy, 0, Hm - 1), np.clip(cx, 0, Wm - 1)
    return y, x, (y != cy) | (x != cx), (np.asarray(map_of, np.int64) * Hm + y) * Wm + x


def _chunks(offsets, D: int) -> np.ndarray:
    o = np.asarray(offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).ravel()
    if o.size < 2 or o[0] < 0 or o[-1] > D or (np.diff(o) < 0).any():
        raise ValueError(f'vis head: offsets must be [B + 1] non-decreasing chunk boundaries within [0, {D}]')
    return o


def vis_head_host(maps, box, map_of, im_hw, track, offsets, mean, std, input_hw, down_ratio, g=None):
    """(logits [D, 128], rows [D, 128], loss [B], dmaps like maps) in the dtype of `maps` (module docstring).

    maps [T, 128, Hm, Wm] float32 or float64; box [D, 4]; map_of [D] in [0, T); im_hw [D, 2] or (h, w); track [D] (-1: a false
    positive); offsets [B + 1]; mean, std [128]; g [B]: the gradient arriving at `loss` (default: ones, loss.sum())."""
    maps = np.asarray(maps)
    if maps.ndim != 4 or maps.shape[1] != VIS_COLS or maps.dtype not in (np.float32, np.float64):
        raise ValueError(f'vis_head_host: maps [T, {VIS_COLS}, Hm, Wm] float32 / float64 expected, got {maps.shape} {maps.dtype}')
    dt = maps.dtype
    T, _, Hm, Wm = maps.shape
    b = _box32(box)
    D = b.shape[0]
    map_of, track = np.asarray(map_of, np.int64).ravel(), np.asarray(track, np.int64).ravel()
    if map_of.shape[0] != D or track.shape[0] != D:
        raise ValueError('vis_head_host: one map_of and one track per box expected')
    if D and (map_of.min() < 0 or map_of.max() >= T):
        raise ValueError(f'vis_head_host: a map_of outside [0, {T})')
    off = _chunks(offsets, D)
    B = off.size - 1
    mean, std = np.asarray(mean, dt).ravel(), np.asarray(std, dt).ravel()
    if mean.size != VIS_COLS or std.size != VIS_COLS:
        raise ValueError(f'vis_head_host: mean, std of {VIS_COLS} entries expected')
    cy, cx, _, _ = vis_pixels_host(*vis_centres_host(b, im_hw, input_hw, down_ratio), map_of, Hm, Wm)
    logits = np.ascontiguousarray(maps[map_of, :, cy, cx]).reshape(D, VIS_COLS)
    mx = logits.max(axis=1, keepdims=True) if D else np.zeros((0, 1), dt)
    e = np.exp(logits - mx)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    rows = (p - mean[None, :]) / std[None, :]
    lab = track >= 0
    cls = np.where(lab, track % VIS_COLS, 0)
    nll = (mx[:, 0] + np.log(s[:, 0])) - logits[np.arange(D), cls]
    g = np.ones(B, dt) if g is None else np.asarray(g, dt).ravel()
    loss, dmaps = np.zeros(B, dt), np.zeros_like(maps)
    for c in range(B):
        r = np.arange(off[c], off[c + 1])
        r = r[lab[r]]
        if r.size == 0:
            continue
        acc = dt.type(0)
        for i in r:                                                 # ascending rows
            acc = acc + nll[i]
        loss[c] = acc / dt.type(r.size)
        coef = g[c] / dt.type(r.size)
        for i in r:                                                 # ascending rows, so sharers of a pixel add in that order
            d = p[i].copy()
            d[cls[i]] -= dt.type(1)
            dmaps[map_of[i], :, cy[i], cx[i]] += coef * d
    return logits, rows.astype(dt, copy=False), loss, dmaps


# ---- the device ------------------------------------------------------------------------------------------------------------
def _dev_tensor(x, dtype, dev, what: str) -> torch.Tensor:
    """A contiguous tensor of `dtype` on `dev` from a device tensor, a host tensor or an array (hosts are uploaded)."""
    if isinstance(x, torch.Tensor) and x.device.type == 'cuda':
        if x.device != dev:
            raise ValueError(f'VisHead: {what} is on {x.device}, the head on {dev}')
        return x.detach().to(dtype=dtype).contiguous()             # (a device tensor is not read here: int32 range is the caller's)
    a = np.ascontiguousarray(x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x))
    if dtype == torch.int32:
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f'VisHead: {what} must be integers, got {a.dtype}')
        if a.size and (a.min() < -_I32 or a.max() >= _I32):
            raise ValueError(f'VisHead: a {what} outside int32')
    return torch.from_numpy(a).to(device=dev, dtype=dtype).contiguous()


class _VisCall:
    """The buffers of one forward (kept for the backward and for record())."""
    __slots__ = ('c', 'keep', 'fbuf', 'ibuf', 'D', 'B', 'maps_shape', 'rows', 'loss', 'logits')


class _VisFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, maps, head, box, map_of, im_hw, track, offsets, dest):
        # dest = (out, col): a tuple, so that `out` is not an input of the node (it is written in place and carries no gradient)
        call = head._launch(maps, box, map_of, im_hw, track, offsets, dest[0], dest[1])
        ctx.call, ctx.head = call, head
        if dest[0] is not None:
            return call.loss
        ctx.mark_non_differentiable(call.rows)
        return call.rows, call.loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        call, head = ctx.call, ctx.head
        d_loss = grads[-1]
        g = d_loss.detach().to(torch.float32).contiguous()
        dmaps = torch.empty(call.maps_shape, dtype=torch.float32, device=head.device)
        _lib.call('tmpnn_vis_head_bwd', C.byref(call.c), g.data_ptr(), dmaps.data_ptr(), _lib.raw_stream(head.device))
        return dmaps, None, None, None, None, None, None, None


class _VisEmbedFn(torch.autograd.Function):
    """VisHead.forward(loss='embedding'): the forward launches write rows, logits and pixels, the embedding loss
    (embedloss.EmbeddingLoss) runs over the saved logits; backward: its gradient wrt the logits, then tmpnn_vis_head_scatter."""

    @staticmethod
    def forward(ctx, maps, head, crit, box, map_of, im_hw, track, offsets, dest):
        call = head._launch(maps, box, map_of, im_hw, track, offsets, dest[0], dest[1])
        ecall = crit._launch(call.logits, call.keep[4], call.keep[5])           # (the head's own device track and offsets)
        ctx.call, ctx.ecall, ctx.head, ctx.crit = call, ecall, head, crit
        if dest[0] is not None:
            return ecall.loss
        ctx.mark_non_differentiable(call.rows)
        return call.rows, ecall.loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        call, head = ctx.call, ctx.head
        d_logits = ctx.crit._backward(ctx.ecall, grads[-1]).contiguous()
        dmaps = torch.empty(call.maps_shape, dtype=torch.float32, device=head.device)
        _lib.call('tmpnn_vis_head_scatter', C.byref(call.c), d_logits.data_ptr(), dmaps.data_ptr(), _lib.raw_stream(head.device))
        return dmaps, None, None, None, None, None, None, None, None


class VisHead:
    """The visual head on the device (module docstring).

    input_hw     (input_h, input_w): the size the CNN sees every image resized to (KITTI 384 x 1280, BDD 720 x 1280)
    down_ratio   input size over map size (dla34: 4, espv2: 1)
    mean, std    the 128 'vis' entries of the feature statistics; a longer vector (a FeatureSpec's mean / std) gives its last 128
    device       a cuda device

        head.rows(maps, box, map_of, im_hw, out=None, col=0)        -> rows [D, 128], or `out` with columns col .. col + 127 written
        head.forward(maps, box, map_of, im_hw, track, offsets, out=None, col=0)
                                                                    -> (rows [D, 128] detached, loss [B]); loss.sum().backward()
                                                                        reaches the CNN through `maps`
        head.record()                                               -> the counts of the last call (one host read)

    maps [T, 128, Hm, Wm] float32 on the device (rows() also takes an espnet.EspCentres); box [D, 4], map_of [D], im_hw [D, 2] or (h, w), track [D], offsets [B + 1];
    D <= MAX_DETS = 131 072 per call; map_of, track and offsets are int32 on the device (host arrays outside int32 raise):
    device tensors are used as they are and nothing then waits for the device; host tensors and arrays are uploaded."""

    def __init__(self, input_hw, down_ratio, mean, std, device='cuda:0'):
        self.input_h, self.input_w, self.down_ratio = (float(v) for v in _geometry(input_hw, down_ratio))
        m, s = np.asarray(mean, np.float32).ravel(), np.asarray(std, np.float32).ravel()
        if m.size < VIS_COLS or s.size < VIS_COLS:
            raise ValueError(f'VisHead: mean / std of at least {VIS_COLS} entries expected')
        m, s = m[-VIS_COLS:], s[-VIS_COLS:]
        if not (np.isfinite(m).all() and np.isfinite(s).all() and (s != 0).all()):
            raise ValueError('VisHead: mean / std must be finite and std non-zero')
        self.mean, self.std = m.copy(), s.copy()
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'VisHead on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path): pass a cuda device')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        self._stats = torch.from_numpy(np.concatenate([self.mean, self.std])).to(dev)
        self._last: Optional[_VisCall] = None

    # ---- one forward: two launches over a map; three (pixels, the CNN's tail at them, rows) over an EspCentres
    def _launch(self, maps, box, map_of, im_hw, track, offsets, out, col) -> _VisCall:
        dev = self.device
        from .espnet import EspCentres
        sparse = isinstance(maps, EspCentres)
        if sparse:
            if track is not None or offsets is not None:
                raise ValueError('VisHead.forward: an EspCentres carries no map for the backward to fill: train over the dense '
                                 'call, net(images) of a net built with centres=False (rows() takes the handle)')
            if maps.device != dev or maps.C != VIS_COLS:
                raise ValueError(f'VisHead: an EspCentres with C = {VIS_COLS} on {dev} expected, got C = {maps.C} on {maps.device}')
            mp, (T, _, Hm, Wm) = maps, maps.shape
        else:
            if not isinstance(maps, torch.Tensor) or maps.device.type != 'cuda':
                raise RuntimeError('VisHead: maps on the host: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path)')
            if maps.device != dev or maps.dim() != 4 or maps.shape[1] != VIS_COLS or maps.dtype != torch.float32:
                raise ValueError(f'VisHead: maps [T, {VIS_COLS}, Hm, Wm] float32 on {dev} expected, got {tuple(maps.shape)} '
                                 f'{maps.dtype} on {maps.device}')
            mp = maps.detach().contiguous()
            T, _, Hm, Wm = (int(v) for v in mp.shape)
        if T < 1 or Hm < 1 or Wm < 1 or T * Hm * Wm >= _I32:
            raise ValueError(f'VisHead: maps of {T} x {Hm} x {Wm} pixels (1 .. 2^31 - 1 expected)')
        bx = _dev_tensor(box, torch.float32, dev, 'box')
        if bx.numel() % 4:
            raise ValueError(f'VisHead: box of shape {tuple(bx.shape)}; [D, 4] expected')
        bx = bx.reshape(bx.numel() // 4, 4)
        D = int(bx.shape[0])
        if D > MAX_DETS:
            raise ValueError(f'VisHead: {D} detections in one call; at most {MAX_DETS} (split the batch)')
        mo = _dev_tensor(map_of, torch.int32, dev, 'map_of').reshape(-1)
        hw, im_h, im_w = None, 0.0, 0.0
        if isinstance(im_hw, (tuple, list)) and len(im_hw) == 2 and not isinstance(im_hw[0], (tuple, list, np.ndarray, torch.Tensor)):
            im_h, im_w = float(np.float32(im_hw[0])), float(np.float32(im_hw[1]))       # one size for every row: no upload
            if not (np.isfinite([im_h, im_w]).all() and im_h > 0 and im_w > 0):
                raise ValueError('VisHead: image sizes must be finite and positive')
        else:
            hw = _dev_tensor(im_hw, torch.float32, dev, 'im_hw')
            if hw.numel() != 2 * D:
                raise ValueError(f'VisHead: im_hw of shape {tuple(hw.shape)}; (h, w) or [{D}, 2] expected')
        if mo.shape[0] != D:
            raise ValueError(f'VisHead: {D} boxes, {mo.shape[0]} map_of')
        tr = None
        if track is not None:
            tr = _dev_tensor(track, torch.int32, dev, 'track').reshape(-1)
            if tr.shape[0] != D:
                raise ValueError(f'VisHead: {D} boxes, {tr.shape[0]} track ids')
        of, B = None, 1
        if offsets is not None:
            if not (isinstance(offsets, torch.Tensor) and offsets.device.type == 'cuda'):
                offsets = _chunks(offsets, D)                       # (host boundaries are checked here; device ones by the kernel)
            of = _dev_tensor(offsets, torch.int32, dev, 'offsets').reshape(-1)
            B = int(of.shape[0]) - 1
            if B < 1:
                raise ValueError('VisHead: offsets [B + 1] with B >= 1 expected')
        if out is None:
            rows, ld, col = torch.empty((D, VIS_COLS), dtype=torch.float32, device=dev), VIS_COLS, 0
        else:
            col = int(col)
            if (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or out.dim() != 2
                    or out.shape[0] != D or col < 0 or col + VIS_COLS > out.shape[1] or (D > 1 and out.stride(1) != 1)
                    or (D > 1 and out.stride(0) < out.shape[1])):
                raise ValueError(f'VisHead.rows: out [{D}, >= col + {VIS_COLS}] float32 on {dev} with unit column stride expected')
            rows, ld = out, (int(out.stride(0)) if D > 1 else int(out.shape[1]))
        # float results: logits | stat (max, sum) | nll | loss; int results: pix | flag | chunk_of | key | count
        fbuf = torch.empty(D * (VIS_COLS + 3) + B, dtype=torch.float32, device=dev)
        ibuf = torch.empty(D * 4 + B * COUNT_WORDS, dtype=torch.int32, device=dev)
        fp, ip = fbuf.data_ptr(), ibuf.data_ptr()
        call = _VisCall()
        call.D, call.B, call.maps_shape, call.fbuf, call.ibuf = D, B, tuple(mp.shape), fbuf, ibuf
        call.keep = (mp, bx, mo, hw, tr, of, rows, self._stats)
        call.c = _lib.CVisHead(T, Hm, Wm, B, D, self.input_h, self.input_w, self.down_ratio, im_h, im_w, ld, col, 0,
                               None if sparse else mp.data_ptr(), bx.data_ptr(), mo.data_ptr(), _lib.ptr(hw), _lib.ptr(tr), _lib.ptr(of),
                               self._stats.data_ptr(), self._stats.data_ptr() + 4 * VIS_COLS, rows.data_ptr(),
                               fp, fp + 4 * D * VIS_COLS, fp + 4 * D * (VIS_COLS + 2), ip, ip + 4 * D, ip + 8 * D, ip + 12 * D,
                               fp + 4 * D * (VIS_COLS + 3), ip + 16 * D)
        call.rows, call.logits = rows, fbuf[:D * VIS_COLS].view(D, VIS_COLS)
        if sparse:
            _lib.call('tmpnn_vis_head_pixels', C.byref(call.c), _lib.raw_stream(dev))
            _, esp_flags = mp.logits_at(ibuf[:D], out=call.logits)          # (every pix is inside the map: the flags stay 0)
            call.keep += (esp_flags,)
            _lib.call('tmpnn_vis_head_rows_from_logits', C.byref(call.c), _lib.raw_stream(dev))
        else:
            _lib.call('tmpnn_vis_head_fwd', C.byref(call.c), _lib.raw_stream(dev))
        call.loss = fbuf[D * (VIS_COLS + 3):]
        self._last = call
        return call

    def rows(self, maps, box, map_of, im_hw, out: Optional[torch.Tensor] = None, col: int = 0) -> torch.Tensor:
        """The standardised 'vis' columns of D detections: a new [D, 128] tensor, or `out` [D, F] (any row stride) with its
        columns col .. col + 127 written and the others untouched.  No autograd graph is built.

        `maps` may be an espnet.EspCentres (EspEmbedNet.centres, C = 128) in the tensor's place: the head then computes the
        pixels, asks the handle for the logits at them and forms the rows from those -- three launches, no host wait, the same
        bits in rows, last_logits() and record() as over the dense map."""
        with torch.no_grad():
            return self._launch(maps, box, map_of, im_hw, None, None, out, col).rows

    def forward(self, maps, box, map_of, im_hw, track, offsets, out: Optional[torch.Tensor] = None, col: int = 0, loss='identity'):
        """(rows [D, 128], loss [B]): the feature columns (detached, as the reference's features.detach()) and the identity loss
        of every chunk, differentiable wrt `maps`.  With `out` [D, F] the rows are written into its columns col .. col + 127 as
        rows() writes them, and `out` itself is returned in their place.

        loss: 'identity' (FairMOTLoss, the default), 'embedding' (the reference's EmbeddingLoss over the gathered logits with its
        default deltas; module docstring of trackmpnn_amd.embedloss) or an embedloss.EmbeddingLoss instance for other deltas.
        `embed_record()` then gives the embedding loss's counts of the call."""
        if track is None or offsets is None:
            raise ValueError('VisHead.forward: track and offsets are needed (rows() is the call without a loss)')
        from .espnet import EspCentres
        if isinstance(maps, EspCentres):
            raise ValueError('VisHead.forward: an EspCentres carries no map for the backward to fill: train over the dense call, '
                             'net(images) of a net built with centres=False (rows() takes the handle)')
        if not (isinstance(loss, str) and loss == 'identity'):
            crit = self._embedding(loss)
            got = _VisEmbedFn.apply(maps, self, crit, box, map_of, im_hw, track, offsets, (out, col if out is not None else 0))
            self._last_embed = crit
            return (out, got) if out is not None else got
        if out is None:
            return _VisFn.apply(maps, self, box, map_of, im_hw, track, offsets, (None, 0))
        return out, _VisFn.apply(maps, self, box, map_of, im_hw, track, offsets, (out, col))

    def _embedding(self, loss):
        """The EmbeddingLoss behind forward(loss=...): the instance handed in, or one with the reference's deltas for 'embedding'."""
        from .embedloss import EmbeddingLoss
        if isinstance(loss, EmbeddingLoss):
            return loss
        if isinstance(loss, str) and loss == 'embedding':
            if getattr(self, '_embed_default', None) is None:
                self._embed_default = EmbeddingLoss()
            return self._embed_default
        raise ValueError(f"VisHead.forward: loss={loss!r}; 'identity', 'embedding' or an EmbeddingLoss expected")

    def embed_record(self) -> dict:
        """EmbeddingLoss.record() of the last forward(loss='embedding') (one host read)."""
        crit = getattr(self, '_last_embed', None)
        if crit is None:
            raise RuntimeError("VisHead.embed_record: no forward(loss='embedding') has been made")
        return crit.record()

    def last_logits(self) -> torch.Tensor:
        """The gathered logits [D, 128] of the last call (a view of its buffer)."""
        if self._last is None:
            raise RuntimeError('VisHead: no call has been made')
        return self._last.logits

    def release(self) -> None:
        """Forget the last call: its buffers (the maps among them) are kept for last_logits() and record() until the next call
        or this.  A loop over many batches of maps calls it to hold one batch at a time."""
        self._last = None

    def record(self) -> dict:
        """The counts of the last call (the one device -> host read): per chunk `labelled` (rows with track >= 0), `clamped` (rows
        whose centre lay outside the map) and `rows`; per row `pix` = (map_of * Hm + cy) * Wm + cx, `cy`, `cx` and `clamped`.
        RuntimeError when a map_of lay outside [0, T) or the chunk boundaries were not non-decreasing within [0, D]."""
        call = self._last
        if call is None:
            raise RuntimeError('VisHead.record: no call has been made')
        D, B = call.D, call.B
        raw = call.ibuf.cpu().numpy()
        pix, flag = raw[:D].astype(np.int64), raw[D:2 * D]
        cnt = raw[4 * D:].reshape(B, COUNT_WORDS).astype(np.int64)
        if cnt[:, 2].any() or (flag & FLAG_MAP).any():
            raise RuntimeError('VisHead.record: a map_of outside [0, T), or chunk offsets that are not non-decreasing within [0, D]')
        _, _, Hm, Wm = call.maps_shape
        return {'labelled': cnt[:, 0], 'clamped': cnt[:, 1], 'rows': cnt[:, 3], 'pix': pix, 'cy': (pix // Wm) % Hm, 'cx': pix % Wm,
                'row_clamped': (flag & FLAG_CLAMPED) != 0}
