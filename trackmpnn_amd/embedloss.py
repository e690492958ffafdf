"""The embedding loss: the reference's discriminative pull-push loss over embedding rows (models/loss.py:118-159 EmbeddingLoss),
which it keeps next to FairMOTLoss as the other way to train the embedding CNN (dataset/kitti_mot.py:131-132).

    embedding_loss_host   per-chunk loss, its two terms and the gradient wrt the rows, in numpy, in the dtype of `features`
                          (float64: the yardstick of the device tests).  The DEFINITION, the order of every sum included.
    EmbeddingLoss         the same on the device (tmpnn_embed_loss_fwd, tmpnn_embed_loss_bwd; csrc/embedloss.hip): an nn.Module
                          whose forward is a torch.autograd.Function wrt `features`, `record()`
    VisHead.forward(..., loss='embedding')   (vishead.py) the loss over the logits the visual head gathered, its gradient
                          scattered into the maps (tmpnn_vis_head_scatter)

The rule.  One loss per chunk, no state across chunks.  Chunk b is rows offsets[b] .. offsets[b + 1] of features [D, W]; row i has
track id track[i], -1 marking a false positive.  A CLUSTER is the labelled rows (track >= 0) of the chunk that share one id; ids
are compared as integers (5 and 133 are two clusters), and the same id in two chunks gives two clusters.  With C clusters, n_c
rows in cluster c and mu_c their mean:

    var  = (1 / C) sum_c (1 / n_c) sum_{i in c} relu(|x_i - mu_c| - delta_var)^2                            0 when C = 0
    dist = (1 / (C (C - 1))) sum_{c != c'} relu(delta_dist - |mu_c - mu_c'|)^2   (ordered pairs)            0 when C <= 1
    loss[b] = var + dist

A chunk without a labelled row has loss 0 and a zero gradient (so does the reference: 0.0 for an all-false-positive chunk and for
an empty one).  This is the reference's rule in full; there are no deviations.

Gradient.  For g [B] arriving at loss and a row k of cluster c of chunk b

    d_features[k] = g[b] (u_k - (1 / n_c) sum_{i in c} u_i + v_c / n_c)
    u_i = 2 relu(d_i - delta_var) (x_i - mu_c) / (d_i C n_c),                                               d_i = |x_i - mu_c|
    v_c = -(4 / (C (C - 1))) sum_{c' != c} relu(delta_dist - m) (mu_c - mu_c') / m,                         m = |mu_c - mu_c'|

and where a norm is exactly 0 its direction term is 0 (torch's subgradient of `norm` at 0).  Unlabelled rows and rows outside
every chunk get zeros.

The order of the sums.  A cluster's LEADER is its lowest row; clusters are ordered by their leaders.  mu_c adds the cluster's rows
in ascending order and divides by n_c.  The variance term adds relu(d_i - delta_var)^2 / n_c over the labelled rows of the chunk
in ascending order and divides by C.  The distance term adds, per cluster in leader order, relu(delta_dist - m)^2 over the other
clusters in leader order, then these sums in leader order, and divides by C (C - 1).  sum u_i and v_c add in the same orders, and
t_c = (v_c - sum u_i) / n_c.  The W channels of a norm are added by np.sum.  The device kernels add rows and clusters in these
orders, and use a butterfly over the 64 lanes where a sum runs over channels or over the rows of a whole chunk.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _lib

MAX_ROWS = 2 ** 17             # rows per call (csrc/embedloss.hip EL_MAX_D)
MAX_COLS = 1024                # columns of a row (EL_MAX_W)
COUNT_WORDS = 4                # per chunk: labelled rows, clusters, bad boundaries, rows
_I32 = 2 ** 31


def _host_chunks(offsets, D: int) -> np.ndarray:
    o = np.asarray(offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).ravel()
    if o.size < 2 or o[0] < 0 or o[-1] > D or (np.diff(o) < 0).any():
        raise ValueError(f'embedding loss: offsets must be [B + 1] non-decreasing chunk boundaries within [0, {D}]')
    return o


def embedding_loss_host(features, track, offsets, delta_var: float = 0.5, delta_dist: float = 10.0, g=None,
                        norms: Optional[List[float]] = None):
    """(loss [B], terms [B, 2] = (var, dist), d_features like features) in the dtype of `features` (module docstring).

    features [D, W] float32 or float64; track [D] integers (-1: a false positive); offsets [B + 1], or None: one chunk of all
    rows; g [B]: the gradient arriving at `loss` (default: ones, loss.sum()).  norms: a list that receives every norm the
    gradient divides by or finds zero (every d_i, every m of an ordered pair)."""
    x = np.asarray(features)
    if x.ndim != 2 or x.dtype not in (np.float32, np.float64):
        raise ValueError(f'embedding_loss_host: features [D, W] float32 / float64 expected, got {x.shape} {x.dtype}')
    dt = x.dtype
    D, W = x.shape
    track = np.asarray(track).ravel()
    if track.size and not np.issubdtype(track.dtype, np.integer):
        raise ValueError(f'embedding_loss_host: track must be integers, got {track.dtype}')
    track = track.astype(np.int64)
    if track.shape[0] != D:
        raise ValueError(f'embedding_loss_host: {D} rows, {track.shape[0]} track ids')
    off = np.asarray([0, D], np.int64) if offsets is None else _host_chunks(offsets, D)
    B = off.size - 1
    g = np.ones(B, dt) if g is None else np.asarray(g, dt).ravel()
    if g.size != B:
        raise ValueError(f'embedding_loss_host: {B} chunks, {g.size} entries of g')
    dv, dd, zero = dt.type(delta_var), dt.type(delta_dist), dt.type(0)
    loss, terms, dx = np.zeros(B, dt), np.zeros((B, 2), dt), np.zeros_like(x)
    for b in range(B):
        rows = [i for i in range(int(off[b]), int(off[b + 1])) if track[i] >= 0]
        members = {}                                            # id -> rows ascending; insertion order = leader order
        for i in rows:
            members.setdefault(int(track[i]), []).append(i)
        clusters = list(members.values())
        Cn = len(clusters)
        if Cn == 0:
            continue
        Cf = dt.type(Cn)
        mus, dist = [], {}
        var = zero
        for c in clusters:
            acc = np.zeros(W, dt)
            for i in c:                                         # ascending rows
                acc = acc + x[i]
            mus.append(acc / dt.type(len(c)))
        cl_of = {i: k for k, c in enumerate(clusters) for i in c}
        for i in rows:                                          # ascending rows
            k = cl_of[i]
            df = x[i] - mus[k]
            dist[i] = np.sqrt(np.sum(df * df))
            h = max(dist[i] - dv, zero)
            var = var + (h * h) / dt.type(len(clusters[k]))
            if norms is not None:
                norms.append(float(dist[i]))
        var = var / Cf
        dst = zero
        vs = [np.zeros(W, dt) for _ in clusters]
        if Cn > 1:
            pairs = Cf * dt.type(Cn - 1)
            for k in range(Cn):                                 # leader order
                s = zero
                for k2 in range(Cn):                            # leader order
                    if k2 == k:
                        continue
                    df = mus[k] - mus[k2]
                    m = np.sqrt(np.sum(df * df))
                    hd = max(dd - m, zero)
                    s = s + hd * hd
                    if norms is not None:
                        norms.append(float(m))
                    if m > 0 and hd > 0:
                        vs[k] = vs[k] + (hd * df) / m
                dst = dst + s
                vs[k] = (dt.type(-4) / pairs) * vs[k]
            dst = dst / pairs
        loss[b], terms[b, 0], terms[b, 1] = var + dst, var, dst

        def ucoef(i, n):
            h = max(dist[i] - dv, zero)
            return (dt.type(2) * h) / (dist[i] * (Cf * dt.type(n))) if (h > 0 and dist[i] > 0) else zero
        for k, c in enumerate(clusters):
            n = len(c)
            su = np.zeros(W, dt)
            for i in c:                                         # ascending rows
                uc = ucoef(i, n)
                if uc != 0:
                    su = su + uc * (x[i] - mus[k])
            t = (vs[k] - su) / dt.type(n)
            for i in c:
                dx[i] = g[b] * (ucoef(i, n) * (x[i] - mus[k]) + t)
    return loss, terms, dx


# ---- the device ------------------------------------------------------------------------------------------------------------
def _int_tensor(x, dev, what: str) -> torch.Tensor:
    """A contiguous int32 tensor on `dev` from a device tensor (used as it is), a host tensor or an array (checked, uploaded)."""
    if isinstance(x, torch.Tensor) and x.device.type == 'cuda':
        if x.device != dev:
            raise ValueError(f'EmbeddingLoss: {what} is on {x.device}, the features on {dev}')
        return x.detach().to(dtype=torch.int32).contiguous().reshape(-1)
    a = np.ascontiguousarray(x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).ravel()
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f'EmbeddingLoss: {what} must be integers, got {a.dtype}')
    if a.size and (a.min() < -_I32 or a.max() >= _I32):
        raise ValueError(f'EmbeddingLoss: a {what} outside int32')
    return torch.from_numpy(a.astype(np.int64)).to(device=dev, dtype=torch.int32).contiguous()


class _EmbedCall:
    """The buffers of one forward (kept for the backward and for record())."""
    __slots__ = ('c', 'keep', 'D', 'B', 'W', 'ld', 'loss', 'terms', 'count', 'device')


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, mod, track, offsets):
        ctx.call = mod._launch(features, track, offsets)
        return ctx.call.loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss):
        return EmbeddingLoss._backward(ctx.call, d_loss), None, None, None


class EmbeddingLoss(torch.nn.Module):
    """The embedding loss on the device (module docstring); delta_var, delta_dist as the reference's constructor.

        crit = EmbeddingLoss()
        loss = crit(features, track)                 # [1]: the loss of one chunk, the reference's call shape
        loss = crit(features, track, offsets)        # [B]: one loss per chunk; loss.sum().backward() reaches `features`
        crit.record()                                # the counts of the last call (one host read)

    features [D, W] float32 on the device, 1 <= W <= 1024, unit column stride (any row stride >= W is used as it is),
    D <= MAX_ROWS = 131 072 per call; track [D] and offsets [B + 1] are int32 on the device (host arrays outside int32 raise):
    device tensors are used as they are and nothing then waits for the device; host tensors and arrays are uploaded.  The
    gradient wrt `features` is differentiable once."""

    def __init__(self, delta_var: float = 0.5, delta_dist: float = 10.0):
        super().__init__()
        dv, dd = float(np.float32(delta_var)), float(np.float32(delta_dist))
        if not (np.isfinite([dv, dd]).all() and dv >= 0 and dd >= 0):
            raise ValueError(f'EmbeddingLoss: delta_var={delta_var}, delta_dist={delta_dist}; finite and not negative expected')
        self.delta_var, self.delta_dist = dv, dd
        self._last: Optional[_EmbedCall] = None

    # ---- one forward: four launches
    def _launch(self, features, track, offsets) -> _EmbedCall:
        if not isinstance(features, torch.Tensor) or features.device.type != 'cuda':
            raise RuntimeError('EmbeddingLoss: features on the host: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path)')
        if features.dim() != 2 or features.dtype != torch.float32 or not 1 <= int(features.shape[1]) <= MAX_COLS:
            raise ValueError(f'EmbeddingLoss: features [D, W] float32 with 1 <= W <= {MAX_COLS} expected, got {tuple(features.shape)} '
                             f'{features.dtype}')
        dev = features.device
        x = features.detach()
        D, W = int(x.shape[0]), int(x.shape[1])
        if D > MAX_ROWS:
            raise ValueError(f'EmbeddingLoss: {D} rows in one call; at most {MAX_ROWS} (split the batch)')
        if D > 1 and (x.stride(1) != 1 or x.stride(0) < W) or (D <= 1 and not x.is_contiguous()):
            x = x.contiguous()
        ld = int(x.stride(0)) if D > 1 else W
        tr = _int_tensor(track, dev, 'track')
        if tr.shape[0] != D:
            raise ValueError(f'EmbeddingLoss: {D} rows, {tr.shape[0]} track ids')
        of, B = None, 1
        if offsets is not None:
            if not (isinstance(offsets, torch.Tensor) and offsets.device.type == 'cuda'):
                offsets = _host_chunks(offsets, D)                   # (host boundaries are checked here; device ones by the kernel)
            of = _int_tensor(offsets, dev, 'offsets')
            B = int(of.shape[0]) - 1
            if B < 1:
                raise ValueError('EmbeddingLoss: offsets [B + 1] with B >= 1 expected')
        ws_bytes = int(_lib.fn('tmpnn_embed_loss_ws')(D, W)) if D else 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        fbuf = torch.empty(3 * B, dtype=torch.float32, device=dev)              # loss | terms
        count = torch.empty((B, COUNT_WORDS), dtype=torch.int32, device=dev)
        call = _EmbedCall()
        call.D, call.B, call.W, call.ld, call.device = D, B, W, ld, dev
        call.keep = (x, tr, of, ws, fbuf)
        call.c = _lib.CEmbedLoss(D, B, W, ld, self.delta_var, self.delta_dist, 0, x.data_ptr() if D else None, _lib.ptr(tr) if D else None,
                                 _lib.ptr(of), _lib.ptr(ws), ws_bytes, fbuf.data_ptr(), fbuf.data_ptr() + 4 * B, count.data_ptr())
        _lib.call('tmpnn_embed_loss_fwd', C.byref(call.c), _lib.raw_stream(dev))
        call.loss, call.terms, call.count = fbuf[:B], fbuf[B:].view(B, 2), count
        self._last = call
        return call

    @staticmethod
    def _backward(call: _EmbedCall, d_loss: torch.Tensor) -> torch.Tensor:
        """d_features [D, W] (row stride = the features') for the gradient d_loss [B] arriving at the call's loss: two launches."""
        g = d_loss.detach().to(torch.float32).contiguous()
        buf = torch.empty(max(call.D * call.ld, 1), dtype=torch.float32, device=call.device)
        _lib.call('tmpnn_embed_loss_bwd', C.byref(call.c), g.data_ptr(), buf.data_ptr(), _lib.raw_stream(call.device))
        return buf.as_strided((call.D, call.W), (call.ld, 1))

    def forward(self, features, track, offsets=None) -> torch.Tensor:
        """loss [B] (one chunk of all rows, [1], without `offsets`), differentiable wrt `features`.  No wait for the device."""
        if not isinstance(features, torch.Tensor) or features.device.type != 'cuda':
            raise RuntimeError('EmbeddingLoss: features on the host: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path)')
        return _EmbedFn.apply(features, self, track, offsets)

    def last_terms(self) -> torch.Tensor:
        """(var, dist) [B, 2] of the last call (a view of its buffer)."""
        if self._last is None:
            raise RuntimeError('EmbeddingLoss: no call has been made')
        return self._last.terms

    def release(self) -> None:
        """Forget the last call (its buffers are kept for last_terms() and record() until the next call or this)."""
        self._last = None

    def record(self) -> dict:
        """The counts of the last call (the one device -> host read): per chunk `labelled` (rows with track >= 0), `clusters`
        and `rows`.  RuntimeError when the chunk boundaries were not non-decreasing within [0, D]."""
        call = self._last
        if call is None:
            raise RuntimeError('EmbeddingLoss.record: no call has been made')
        cnt = call.count.cpu().numpy().astype(np.int64)
        if cnt[:, 2].any():
            raise RuntimeError('EmbeddingLoss.record: chunk offsets that are not non-decreasing within [0, D]')
        return {'labelled': cnt[:, 0], 'clusters': cnt[:, 1], 'rows': cnt[:, 3]}
