"""Batched chunk training: many chunks of train.py:54-135 in one block-diagonal batch, with the reference's own losses.

A train-mode graph depends on the labels only (utils/graph.py:229-245, 271-274 read `labels`, never `scores`, when
mode == 'train'), so a set of chunks' whole sequences of graphs is built before the first forward call.  `build_train_batch`
is the host definition; `build_train_batch_device` builds the same batch with HIP kernels, fast enough to build one per step
(the reference's --random-transforms redraw every chunk's labels each time it is drawn):

    batch = build_train_batch_device(ys, device)   # ys: B chunks y_b [ND_b, 2] = [timestep, track id]
    loss, per_chunk, ncalls, edge_iters = train_chunks(model, batch, Xs)     # trackmpnn_amd.loops

`build_train_batch` lays the kept chunks out as `batch_windows` does (call-major, append-only: one `CallPlan` per call) and adds
what the losses need: the row labels, per call the loss windows (`LossWindows`: which det / edge indices belong to which live
chunk) and the source of every new det row's features.  Chunk semantics are `train_chunk`'s (= train.py):

  * a chunk that initialize_graph(mode='train') rejects (fewer than two non-empty timesteps, or every det a false positive,
    utils/graph.py:132) is dropped and listed in `skipped`;
  * a chunk's calls are the first call plus one for EVERY timestep in range(t1 + 1, tN + 1); a timestep without detections is
    a call with no new rows, on which the model still runs and whose losses are added again;
  * labels: det row = track >= 0; edge row = track(src) == track(dst) >= 0 (utils/graph.py:165-176, 310-325);
  * a chunk is live at call c while c < ncalls_b; finished chunks carry no loss terms and their rows get zero gradient.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .graph import CallPlan, FrameGraph, WindowBuilder, WindowCall, batch_windows


@dataclass
class LossWindows:
    """struct tmpnn_loss_windows (include/tmpnn.h) of one call: per window of the batch its det / edge indices (positions in the
    call graph's det_row / edge_row), ascending; the window of every det / edge (-1: the chunk is not live at this call)."""
    W: int
    n_det: int
    n_edge: int
    det_ptr: torch.Tensor     # int32 [W + 1]
    det_idx: torch.Tensor     # int32 [n_det]
    edge_ptr: torch.Tensor    # int32 [W + 1]
    edge_idx: torch.Tensor    # int32 [n_edge]
    det_win: torch.Tensor     # int32 [Dn]
    edge_win: torch.Tensor    # int32 [E]
    _c: Optional[_lib.CLossWindows] = field(default=None, repr=False, compare=False)

    def to(self, device) -> 'LossWindows':
        mv = lambda t: t.to(device)
        return LossWindows(self.W, self.n_det, self.n_edge, mv(self.det_ptr), mv(self.det_idx), mv(self.edge_ptr),
                           mv(self.edge_idx), mv(self.det_win), mv(self.edge_win))

    def cref(self):
        if self._c is None:
            self._c = _lib.CLossWindows(self.W, self.n_det, self.n_edge, self.det_ptr.data_ptr(), self.det_idx.data_ptr(),
                                        self.edge_ptr.data_ptr(), self.edge_idx.data_ptr(), self.det_win.data_ptr(),
                                        self.edge_win.data_ptr())
        return C.byref(self._c)


@dataclass
class TrainBatch:
    """What `build_train_batch` returns (see the module docstring).  Chunk b of the batch is chunk kept[b] of the `ys` given."""
    plans: List[CallPlan]             # one per call of the batch
    windows: List[LossWindows]        # one per call
    labels: torch.Tensor              # uint8 [N of the last call]; call c reads labels[:plans[c].graph.N] (rows never move)
    feat_src: List[torch.Tensor]      # int64 [n_new] per call: row of the stacked features of every new row (edge rows: n_feat)
    kept: np.ndarray                  # int64 [B]  index into ys of every chunk of the batch
    skipped: List[int]                # indices into ys of the chunks the reference skips
    ncalls_b: np.ndarray              # int64 [B]  calls of every chunk (train_chunk's count)
    edges_b: np.ndarray               # int64 [B]  sum of E over its calls (train_chunk's edge iterations)
    det_offset: np.ndarray            # int64 [len(ys) + 1]  first row of chunk i in the stacked features
    chunk_calls: List[List[WindowCall]] = field(default_factory=list, repr=False)   # every chunk's calls, batch order
    #                                                                    (empty on a batch of build_train_batch_device)

    @property
    def B(self) -> int:
        return int(self.kept.size)

    @property
    def ncalls(self) -> int:
        return int(self.ncalls_b.sum())

    @property
    def edge_iters(self) -> int:
        return int(self.edges_b.sum())

    @property
    def n_feat(self) -> int:
        return int(self.det_offset[-1])

    def call_labels(self, c: int) -> torch.Tensor:
        return self.labels[:self.plans[c].graph.N]

    def stacked_features(self, Xs) -> torch.Tensor:
        """[n_feat + 1, F]: the chunks' features stacked in the order of ys, then one zero row (the features of edge rows).
        Xs: one [n_feat, F] tensor stacked that way, or a sequence of [ND_i, F] / [1, ND_i, F] tensors (skipped chunks
        included)."""
        if isinstance(Xs, torch.Tensor):
            X = Xs.reshape(-1, Xs.shape[-1])
        else:
            X = torch.cat([x.reshape(-1, x.shape[-1]) for x in Xs])
        if X.shape[0] != self.n_feat:
            raise ValueError(f'features: {X.shape[0]} rows for {self.n_feat} detections')
        X = X.to(self.labels.device)                      # (host features are moved once per step, as train_chunk takes them)
        return torch.cat([X, X.new_zeros((1, X.shape[1]))])


class AllChunksSkipped(ValueError):
    """Every chunk handed to a batch build is skipped (fewer than two timesteps, or only false positives): there is no batch.
    A ValueError, as the builds have always raised for this case; loops that redraw their chunks catch it and move on."""


def _as_y(y) -> np.ndarray:
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.asarray(y, dtype=np.int64)
    return y.reshape(-1, 2)


def build_train_batch(ys: Sequence, device='cpu') -> TrainBatch:
    """The block-diagonal training batch of the chunks `ys` (each y [ND, 2] or [1, ND, 2], host or device), resident on
    `device`.  Host index plumbing, once per set of chunks (the graphs do not depend on the model's outputs)."""
    ys = [_as_y(y) for y in ys]
    det_offset = np.zeros(len(ys) + 1, np.int64)
    det_offset[1:] = np.cumsum([y.shape[0] for y in ys])
    kept, skipped, wins = [], [], []
    for i, y in enumerate(ys):
        # initialize_graph(mode='train') returns None (utils/graph.py:132): t0 == t1, or no true positive at all
        if np.unique(y[:, 0]).size < 2 or (y[:, 1] == -1).all():
            skipped.append(i)
            continue
        kept.append(i)
        wins.append(WindowBuilder(y).calls(empty_calls=True))
    if not wins:
        raise AllChunksSkipped('build_train_batch: every chunk is skipped (fewer than two timesteps, or only false positives)')
    plans, refs = batch_windows(wins, device='cpu')
    kept = np.asarray(kept, np.int64)
    B, ncalls = len(wins), len(plans)
    ncalls_b = np.asarray([len(w) for w in wins], np.int64)
    n_new = np.zeros((ncalls, B), np.int64)
    for b, w in enumerate(wins):
        n_new[:len(w), b] = [wc.n_new for wc in w]
    row_win = np.repeat(np.tile(np.arange(B), ncalls), n_new.ravel())          # window of every row, call-major
    # track id of every det row, then the labels of the final graph (a row's label never changes: rows only append)
    trk_all = np.concatenate([y[:, 1] for y in ys])
    N = plans[-1].graph.N
    track = np.full(N, -1, np.int64)
    for plan, ref in zip(plans, refs):
        if ref.shape[0]:
            track[plan.new_det_row.numpy()] = trk_all[det_offset[kept[ref[:, 0]]] + ref[:, 1]]
    fg = plans[-1].graph
    labels = np.zeros(N, np.uint8)
    det_rows = fg.det_row.numpy()
    labels[det_rows] = track[det_rows] >= 0
    ts, td = track[fg.src.numpy()], track[fg.dst.numpy()]
    labels[fg.edge_row.numpy()] = (ts == td) & (ts >= 0)
    live = np.arange(ncalls)[:, None] < ncalls_b[None, :]                      # [calls, B]
    windows, feat_src = [], []
    edges_b = np.zeros(B, np.int64)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))

    def lists(rows, c):
        win = row_win[rows]
        win = np.where(live[c][win], win, -1)
        order = np.argsort(win, kind='stable')            # (call blocks are ascending by window: a merge of sorted runs)
        order = order[win[order] >= 0]
        cnt = np.bincount(win[win >= 0], minlength=B)
        ptr = np.zeros(B + 1, np.int64)
        ptr[1:] = np.cumsum(cnt)
        return win, order, ptr, cnt

    for c, (plan, ref) in enumerate(zip(plans, refs)):
        g = plan.graph
        dwin, didx, dptr, _ = lists(g.det_row.numpy(), c)
        ewin, eidx, eptr, ecnt = lists(g.edge_row.numpy(), c)
        edges_b += ecnt
        windows.append(LossWindows(B, int(didx.size), int(eidx.size), i32(dptr), i32(didx), i32(eptr), i32(eidx), i32(dwin),
                                   i32(ewin)))
        fs = np.full(plan.n_new, det_offset[-1], np.int64)
        if ref.shape[0]:
            fs[plan.new_det_local.numpy()] = det_offset[kept[ref[:, 0]]] + ref[:, 1]
        feat_src.append(torch.from_numpy(fs))
    dev = torch.device(device)
    return TrainBatch(plans=[p.to(dev) for p in plans], windows=[w.to(dev) for w in windows],
                      labels=torch.from_numpy(labels).to(dev), feat_src=[f.to(dev) for f in feat_src], kept=kept,
                      skipped=skipped, ncalls_b=ncalls_b, edges_b=edges_b, det_offset=det_offset, chunk_calls=wins)


# ----------------------------------------------------------------------------------------------
# the same batch built on the device (csrc/trainbuild.hip, struct tmpnn_train_build)
# ----------------------------------------------------------------------------------------------
TB_MAX_DETS, TB_MAX_CALLS = 4096, 1024       # TMPNN_TB_MAX_DETS / TMPNN_TB_MAX_CALLS: per chunk
_TB_NONINT = -2 ** 63                        # TMPNN_TB_NONINT
_TB_STATUS = ((32, 'offsets do not ascend within [0, ND]'), (1, 'a label is not an integer'),
              (2, 'a timestep is negative'), (4, 'a label is outside int32'),
              (8, f'more than {TB_MAX_DETS} detections, beyond the device builder\'s limits (build_train_batch takes it)'),
              (16, f'more than {TB_MAX_CALLS} calls (1 + tN - t1), beyond the device builder\'s limits (build_train_batch '
                   'takes it)'))


def _check_labels(y):
    """ValueError unless y (array or tensor) is [ND, 2] or [1, ND, 2] of a real dtype."""
    shape = tuple(y.shape)
    cplx = y.dtype.is_complex if isinstance(y, torch.Tensor) else np.iscomplexobj(y)
    if cplx or not (len(shape) == 2 or (len(shape) == 3 and shape[0] == 1)) or shape[-1] != 2:
        raise ValueError(f'build_train_batch_device: labels [ND, 2] or [1, ND, 2] of integers expected, got {shape} {y.dtype}')


def _label_tensor(y) -> torch.Tensor:
    """y as a [ND, 2] tensor (no copy, same device)."""
    t = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
    _check_labels(t)
    return t.reshape(-1, 2)


def _to_device(t, dev) -> torch.Tensor:
    """A host tensor / array on `dev` without waiting for work already queued there: staged in pinned memory, copied
    asynchronously on the current stream (a copy from pageable memory synchronises the stream).  Device tensors move as usual."""
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    if t.device.type != 'cpu':
        return t.to(dev)
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


def _stacked_labels(ys, offsets, dev):
    """(y int64 [ND, 2], offsets int64 [n + 1]) on `dev`: the list form is stacked with one copy."""
    if offsets is not None:
        y = _label_tensor(ys)
        off = offsets if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets))
        if off.dim() != 1 or off.numel() < 1 or off.is_floating_point() or off.dtype.is_complex:
            raise ValueError('build_train_batch_device: offsets [n + 1] of integers expected')
        off = _to_device(off.to(torch.int64) if off.device.type == 'cpu' else off, dev).to(torch.int64)
    elif all(isinstance(y, np.ndarray) for y in ys):                 # (host arrays: one concatenation, one copy)
        lens = np.zeros(len(ys) + 1, np.int64)
        lens[1:] = np.cumsum([y.size // 2 for y in ys])
        y = torch.from_numpy(np.concatenate([y.reshape(-1, 2) for y in ys]) if ys else np.zeros((0, 2), np.int64))
        off = _to_device(lens, dev)
    else:
        parts = [_label_tensor(y) for y in ys]
        lens = np.zeros(len(parts) + 1, np.int64)
        lens[1:] = np.cumsum([p.shape[0] for p in parts])
        dt = torch.float64 if any(p.is_floating_point() for p in parts) else torch.int64
        if all(p.device.type == 'cpu' for p in parts):
            y = torch.cat([p.to(dt) for p in parts]) if parts else torch.zeros((0, 2), dtype=dt)
        else:
            y = torch.cat([_to_device(p, dev).to(dt) for p in parts])
        off = _to_device(lens, dev)
    y = _to_device(y, dev)
    if y.is_floating_point():
        y = y.to(torch.float64)
        bad = y != torch.trunc(y)                                   # (NaN included)
        y = torch.where(bad, torch.full_like(y, 0), y.clamp(-2.0 ** 40, 2.0 ** 40)).to(torch.int64)
        y = torch.where(bad, torch.full_like(y, _TB_NONINT), y)
    else:
        y = y.to(torch.int64)
    return y.contiguous(), off.contiguous()


def build_train_batch_device(ys, device='cuda:0', offsets=None, padded: bool = False, draw_flags=None) -> TrainBatch:
    """The TrainBatch of `build_train_batch(ys)`, built by HIP kernels on `device` (csrc/trainbuild.hip): equal in every field,
    except that `chunk_calls` stays empty.  Two device-to-host reads (the per-chunk counts, then the per-call totals), the only
    points where the host waits for the device: host-side tables go up through pinned memory, asynchronously.  No loop over
    chunks on the host, so a fresh batch can be built every step.

    ys: a list of per-chunk labels y_b [ND_b, 2] / [1, ND_b, 2] (host or device), or, with `offsets` [n + 1], one stacked
    [ND, 2] tensor whose chunk i is rows offsets[i] .. offsets[i+1].  Integer dtypes, or floating ones holding integers.
    padded (with `offsets`): the stacked tensor may hold more rows than offsets[-1]; the rows beyond it are ignored (a draw of
    `trackmpnn_amd.chunks.ChunkSampler`, whose kept total only the device knows).  Otherwise offsets must run from 0 to ND.
    draw_flags: the uint8 `flags` [n] of the ChunkSampler draw the labels come from (device).  Their maximum rides along with
    host read 1 (no further wait), and a chunk the draw kernels refused (bit 7, TMPNN_CD_FLAG_BAD: the store's or the sampler's
    device tables failed the kernels' checks) raises RuntimeError here, where it would otherwise train as an empty chunk.
    Limits per chunk: TB_MAX_DETS detections and TB_MAX_CALLS calls (build_train_batch serves larger chunks); rows and edges of
    the batch in int32.  Raises ValueError on malformed labels and AllChunksSkipped (a ValueError) when every chunk is skipped."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('build_train_batch_device runs on the MI355X HIP kernels only (no CPU path): pass a cuda device')
    if offsets is None:                                     # (shapes are checked before anything touches the device)
        ys = [y if isinstance(y, (np.ndarray, torch.Tensor)) else np.asarray(y) for y in ys]
        for y in ys:
            _check_labels(y)
    else:
        _label_tensor(ys)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    y, off = _stacked_labels(ys, offsets, dev)
    n, ND = off.numel() - 1, int(y.shape[0])
    if n <= 0:
        raise AllChunksSkipped('build_train_batch_device: every chunk is skipped (fewer than two timesteps, or only false positives)')
    stream = _lib.raw_stream(dev)
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    d = _lib.CTrainBuild()
    d.n, d.n_feat, d.y, d.offsets = n, ND, y.data_ptr(), off.data_ptr()
    if draw_flags is not None and not (isinstance(draw_flags, torch.Tensor) and draw_flags.dtype == torch.uint8 and
                                       draw_flags.numel() == n):
        raise ValueError(f'build_train_batch_device: draw_flags must be a uint8 tensor of {n} entries')
    buf = torch.empty(5 * n + 1 + (draw_flags is not None), **i64)           # info [n, 4], offsets [n + 1], (the draw's flags)
    buf[4 * n:5 * n + 1].copy_(off)
    if draw_flags is not None:
        buf[5 * n + 1:].copy_(draw_flags.to(dev).amax().reshape(1))
    d.info = buf.data_ptr()
    _lib.call('tmpnn_train_build_count', C.byref(d), stream)
    h = buf.cpu().numpy()                                                    # host read 1: the per-chunk counts
    if draw_flags is not None and h[5 * n + 1] & 128:                       # TMPNN_CD_FLAG_BAD
        raise RuntimeError('build_train_batch_device: the draw kernels refused a chunk (flags bit 7): the device tables of '
                           'the DetectionStore or of the ChunkSampler do not pass the kernels\' checks')
    info, det_offset = h[:4 * n].reshape(n, 4), h[4 * n:5 * n + 1].copy()
    bad = np.nonzero(info[:, 0])[0]
    if bad.size:
        i = int(bad[0])
        msg = next(m for bit, m in _TB_STATUS if info[i, 0] & bit)
        raise ValueError(f'build_train_batch_device: chunk {i}: {msg}')
    if padded and offsets is not None:
        if det_offset[0] != 0:
            raise ValueError(f'build_train_batch_device: offsets must start at 0 (and end within ND = {ND})')
    elif det_offset[0] != 0 or det_offset[-1] != ND:
        raise ValueError(f'build_train_batch_device: offsets must run from 0 to ND = {ND}')
    kept = np.nonzero(info[:, 1] > 0)[0].astype(np.int64)
    skipped = np.nonzero(info[:, 1] == 0)[0].tolist()
    if kept.size == 0:
        raise AllChunksSkipped('build_train_batch_device: every chunk is skipped (fewer than two timesteps, or only false positives)')
    ncalls_b = info[kept, 1].astype(np.int64)
    B, Cn = int(kept.size), int(ncalls_b.max())
    cptr = np.zeros(B + 1, np.int64)
    cptr[1:] = np.cumsum(ncalls_b)
    T0 = int(cptr[-1])
    P = 1 << int(max(int((det_offset[kept + 1] - det_offset[kept]).max()) - 1, 0)).bit_length()
    Lc = (ncalls_b[None, :] > np.arange(Cn)[:, None]).sum(1)               # blocks of call c (host: from the counts)
    hb = _to_device(np.concatenate([kept, cptr, ncalls_b, np.cumsum(Lc) - 1]), dev)
    kept_d, cptr_d, ncb_d, ends_d = hb[:B], hb[B:2 * B + 1], hb[2 * B + 1:3 * B + 1], hb[3 * B + 1:]
    k32 = hb[:2 * B + 1].to(torch.int32)
    counts = torch.empty((T0, 2), **i32)
    d.B, d.C, d.max_dets, d.max_slots = B, Cn, P, Cn + 2
    d.kept, d.cptr, d.counts = k32.data_ptr(), k32[B:].data_ptr(), counts.data_ptr()
    _lib.call('tmpnn_train_build_calls', C.byref(d), stream)

    # call-major layout of the blocks (b, c), c < ncalls_b: index plumbing on the device, no host round trip
    ar = lambda k: torch.arange(k, device=dev)
    excl = lambda x, dim=0: torch.cumsum(x, dim) - x
    b_of = torch.repeat_interleave(ar(B), ncb_d, output_size=T0)
    c_of = ar(T0) - cptr_d[b_of]
    ne, ndt = counts[:, 0].long(), counts[:, 1].long()
    nr = ne + ndt
    perm = torch.argsort(c_of * B + b_of)
    c_p, nr_p, nd_p = c_of[perm], nr[perm], ndt[perm]
    full = nr_p > 0                                                          # a segment: the block has new rows
    cnt = torch.stack([nr_p, ne[perm], nd_p, full.long()])
    cs = torch.cumsum(cnt, 1)                                               # [4, T0], call-major
    tot = cs[:, ends_d]                                                      # [4, C] rows / edges / dets / segments up to call c
    N_c, E_c, D_c = tot[0], tot[1], tot[2]
    S_c = tot[3] - torch.cat([tot[3, :1] * 0, tot[3, :-1]])
    segg = cs[3] - 1
    blk = torch.empty((T0, 4), **i64)
    blk[perm] = torch.cat([(cs[:3] - cnt[:3]).T, (segg - excl(S_c)[c_p])[:, None]], 1)
    blk = blk.to(torch.int32)
    D_prev = torch.cat([D_c[:1] * 0, D_c[:-1]])
    # min_seg_cnt / max_seg_nd per call: a running min / max over the call-major blocks, each call lifted by a step of 2^41
    # above the one before (values < 2^40; an empty block counts as 2^40), read at the call's last block
    lift = c_p << 41
    min_cnt = torch.cummin(torch.where(full, nr_p, torch.full_like(nr_p, 2 ** 40)) - lift, 0).values[ends_d]
    min_cnt = min_cnt + (ar(Cn) << 41)
    min_cnt = torch.where(min_cnt >= 2 ** 40, 0, min_cnt)
    max_nd = torch.cummax(nd_p + lift, 0).values[ends_d] - (ar(Cn) << 41)
    # per (call, chunk): the chunk's dets / edges so far, and where they start in det_order, det_idx, edge_idx.  These tables are
    # [C, B] for every chunk, finished ones included: a finished chunk's dets stay in every later call's det_order, and
    # LossWindows has W = B, so the outputs det_order (sum_c Dn_c >= 2 C B entries), det_ptr and edge_ptr are that large already.
    # int32 (a batch whose counts overflow it is refused after read 2); the int64 index is dropped once used.
    cs_d, cs_e = torch.cumsum(ndt, 0), torch.cumsum(ne, 0)
    cum_d = (cs_d - (cs_d - ndt)[cptr_d[:-1]][b_of]).to(torch.int32)
    cum_e = (cs_e - (cs_e - ne)[cptr_d[:-1]][b_of]).to(torch.int32)
    idx = torch.minimum(cptr_d[:-1][None, :] + ar(Cn)[:, None], cptr_d[1:][None, :] - 1)
    CD, CE = cum_d[idx], cum_e[idx]
    del idx
    live = ar(Cn)[:, None] < ncb_d[None, :]
    CDl, CEl = CD * live, CE * live
    del live, CE
    ex32 = lambda x: torch.cumsum(x, 1, dtype=torch.int32) - x
    n_det_c, n_edge_c, edges_d = CDl.sum(1), CEl.sum(1), CEl.sum(0)
    cb_tab = torch.stack([ex32(CD), ex32(CDl), ex32(CEl)])
    del CD
    det_ptr = torch.cat([cb_tab[1], n_det_c[:, None].to(torch.int32)], 1)
    edge_ptr = torch.cat([cb_tab[2], n_edge_c[:, None].to(torch.int32)], 1)
    del CDl, CEl
    status = buf[:4 * n].view(n, 4)[:, 0].amax()[None]                       # (TMPNN_TB_ST_LDS from the calls kernel)
    tot = torch.cat([N_c, E_c, D_c, S_c, min_cnt, max_nd, n_det_c, n_edge_c, edges_d, status]).cpu().numpy()   # host read 2
    if tot[-1]:
        raise RuntimeError(f'build_train_batch_device: status {int(tot[-1])} from the calls kernel (LDS sizes of the descriptor)')
    N_c, E_c, D_c, S_c, min_cnt, max_nd, n_det_c, n_edge_c = tot[:8 * Cn].reshape(8, Cn)
    edges_b = tot[8 * Cn:-1].copy()
    N, E, Dn = int(N_c[-1]), int(E_c[-1]), int(D_c[-1])
    if N >= 2 ** 31 or 2 * E >= 2 ** 31:
        raise ValueError(f'build_train_batch_device: {N} rows / {E} edges do not fit the int32 rows of the device builder '
                         '(build the batch with build_train_batch, or in smaller batches)')
    ex = lambda a: np.concatenate([[0], np.cumsum(a)[:-1]]).astype(np.int64)
    rp_len = D_c + 1
    # per call: rows before it, first element in rowptr, inc, det_order / det_win, edge_win, det_idx, edge_idx (call_tab)
    bases = np.stack([np.concatenate([[0], N_c[:-1]]), ex(rp_len), ex(2 * E_c), ex(D_c), ex(E_c), ex(n_det_c),
                      ex(n_edge_c)]).astype(np.int64)
    call_tab = _to_device(np.concatenate([bases.ravel(), rp_len]), dev)
    rp_len_d = call_tab[7 * Cn:]
    e32 = lambda k: torch.empty(int(k), **i32)
    e64 = lambda k: torch.empty(int(k), **i64)
    o = dict(src=e32(E), dst=e32(E), edge_row=e32(E), src_pos=e32(E), dst_pos=e32(E), det_row=e32(Dn), seg_of_det=e32(Dn),
             new_det_local=e64(Dn), det_group=e64(Dn), is_edge=torch.empty(N, dtype=torch.uint8, device=dev), pos=e32(N),
             labels=torch.empty(N, dtype=torch.uint8, device=dev), feat_src=e64(N), seg_of_new=e64(N),
             rowptr=e32(rp_len.sum()), inc=e32(2 * E_c.sum()), det_order=e32(D_c.sum()), det_win=e32(D_c.sum()),
             edge_win=e32(E_c.sum()), det_idx=e32(n_det_c.sum()), edge_idx=e32(n_edge_c.sum()))
    for k, t in o.items():
        setattr(d, k, t.data_ptr())
    d.n_feat = int(det_offset[-1])
    d.blk, d.call_tab, d.cb_tab = blk.data_ptr(), call_tab.data_ptr(), cb_tab.data_ptr()
    _lib.call('tmpnn_train_build_fill', C.byref(d), 0, stream)
    # rowptr: {0, degrees} per call -> offsets (an inclusive scan per call)
    rcs = torch.cumsum(o['rowptr'], 0)
    rowptr = (rcs - torch.repeat_interleave(rcs[call_tab[Cn:2 * Cn]], rp_len_d, output_size=int(rp_len.sum()))).to(torch.int32)
    o['rowptr'] = rowptr
    d.rowptr = rowptr.data_ptr()
    _lib.call('tmpnn_train_build_fill', C.byref(d), 1, stream)
    # segments of every call: seg_cnt, and seg_ptr = {0, new det rows so far} per call
    nS = int(S_c.sum())
    seg_cnt = torch.zeros(nS + 1, **i32).index_copy_(0, torch.where(full, segg, torch.full_like(segg, nS)),
                                                    nr_p.to(torch.int32))[:nS]
    seg_ptr = torch.zeros(nS + Cn + 1, **i32)
    seg_ptr.index_copy_(0, torch.where(full, segg + c_p + 1, torch.full_like(segg, nS + Cn)),
                        (cs[2] - D_prev[c_p]).to(torch.int32))
    seg_ptr = seg_ptr[:nS + Cn]

    plans, windows, feat_src = [], [], []
    sb = ex(S_c)
    for c in range(Cn):
        n1, e1, d1 = int(N_c[c]), int(E_c[c]), int(D_c[c])
        n0, d0 = (int(N_c[c - 1]), int(D_c[c - 1])) if c else (0, 0)
        r0, i0, q0 = int(bases[1, c]), int(bases[2, c]), int(bases[3, c])
        g = FrameGraph(N=n1, E=e1, Dn=d1, src=o['src'][:e1], dst=o['dst'][:e1], edge_row=o['edge_row'][:e1],
                       det_row=o['det_row'][:d1], rowptr=rowptr[r0:r0 + d1 + 1], inc=o['inc'][i0:i0 + 2 * e1],
                       is_edge=o['is_edge'][:n1], pos=o['pos'][:n1], src_pos=o['src_pos'][:e1], dst_pos=o['dst_pos'][:e1])
        if B > 1:
            g.det_order = o['det_order'][q0:q0 + d1]
            g.__dict__['_det_group'] = o['det_group'][:d1]
        s0, S = int(sb[c]), int(S_c[c])
        plans.append(CallPlan(graph=g, n_new=n1 - n0, new_det_local=o['new_det_local'][d0:d1],
                              new_det_row=o['det_row'][d0:d1], seg_ptr=seg_ptr[s0 + c:s0 + c + S + 1],
                              seg_cnt=seg_cnt[s0:s0 + S], seg_of_new=o['seg_of_new'][n0:n1], min_seg_cnt=int(min_cnt[c]),
                              seg_of_det=o['seg_of_det'][d0:d1], max_seg_nd=int(max_nd[c])))
        a, m = int(bases[5, c]), int(bases[6, c])
        w0 = int(bases[4, c])
        windows.append(LossWindows(B, int(n_det_c[c]), int(n_edge_c[c]), det_ptr[c], o['det_idx'][a:a + int(n_det_c[c])],
                                   edge_ptr[c], o['edge_idx'][m:m + int(n_edge_c[c])], o['det_win'][q0:q0 + d1],
                                   o['edge_win'][w0:w0 + e1]))
        feat_src.append(o['feat_src'][n0:n1])
    return TrainBatch(plans=plans, windows=windows, labels=o['labels'], feat_src=feat_src, kept=kept, skipped=skipped,
                      ncalls_b=ncalls_b, edges_b=edges_b, det_offset=det_offset)
