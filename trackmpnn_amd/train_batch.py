"""Batched chunk training: many chunks of train.py:54-135 in one block-diagonal batch, with the reference's own losses.

A train-mode graph depends on the labels only (utils/graph.py:229-245, 271-274 read `labels`, never `scores`, when
mode == 'train'), so a set of chunks' whole sequences of graphs is built once, on the host, and reused in every epoch:

    batch = build_train_batch(ys, device)          # ys: B chunks y_b [ND_b, 2] = [timestep, track id]
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
from .graph import CallPlan, WindowBuilder, WindowCall, batch_windows


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
        raise ValueError('build_train_batch: every chunk is skipped (fewer than two timesteps, or only false positives)')
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
