"""The reference's training-quality signal on the device: F1 per forward call and the epoch's loss means.

After every forward call the reference (train.py:86-88, :125-127) takes `pred = argmax((1 - score, score))`, selects the det and
edge rows (the edge rows alone with --no-tp-classifier) and appends `f1_score(targets[idx], pred[idx], zero_division=0)` to
`epoch_f1`; at the end of the epoch (train.py:157-171) it logs the mean F1 over the forwards and the means of `loss_c`, `loss_f`
and `loss` over the chunks.  A `TrainMonitor` keeps the same five numbers in a small device record
(struct tmpnn_train_record): `train_chunk` / `train_chunks` count tp / fp / fn after every forward
(`classification_counts`, `classification_counts_windows`: integer counts, no host read) and fold the chunk / the step into
the record with one launch.  The host waits for the device in `read()` only:

    m = TrainMonitor(device)
    for ys, Xs in epoch:                                   # one optimizer step per B chunks
        batch = build_train_batch_device(ys, device)
        opt.zero_grad()
        loss, per_chunk, _, _ = train_chunks(model, batch, Xs, monitor=m)
        opt.step()
    stats = m.read()                                       # avg_f1, avg_loss_c, avg_loss_f, avg_loss, forwards, chunks
    m.reset()

Every (call, chunk) pair of a batch in which the chunk has rows is one forward, so a batched epoch averages over the same
forwards as the reference's chunk-by-chunk loop.  Under `trackmpnn_amd.dist` each rank's monitor covers its own shard.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .loss import classification_counts, classification_counts_windows

_FIELDS = ('sum_f1', 'forwards', 'sum_loss_c', 'sum_loss_f', 'sum_loss', 'chunks')       # struct tmpnn_train_record


class TrainMonitor:
    """Running F1 / loss statistics of an epoch in device memory (module docstring).

    record       int64 [6] device tensor holding struct tmpnn_train_record bit for bit (the fp64 sums as their bit patterns)
    last_counts  int32 [C, 4, W] device tensor of the last batched step: tp, fp, fn, rows of every (call, chunk); zeros on
                 pairs that are not forwards.  None before the first `train_chunks(..., monitor=...)`."""

    def __init__(self, device='cuda:0'):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'TrainMonitor on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only '
                               '(no CPU or torch fallback exists)')
        self.device = dev
        self.record = torch.zeros(len(_FIELDS), dtype=torch.int64, device=dev)
        self.last_counts: Optional[torch.Tensor] = None

    def reset(self) -> None:
        """Zero the record (an epoch boundary).  No host read."""
        self.record.zero_()

    def new_counts(self, C: int, W: int, zero: bool) -> torch.Tensor:
        """int32 [C, 4, W] for the counts of a step (zero: rows no call will write must read as `no forward`)."""
        mk = torch.zeros if zero else torch.empty
        return mk((C, 4, W), dtype=torch.int32, device=self.device)

    def count(self, counts: torch.Tensor, c: int, scores, targets, graph, tp_classifier: bool) -> None:
        """Batch 1: the counts of forward call c of a chunk into counts[c, :, 0]."""
        classification_counts(scores, targets, graph, tp_classifier, out=counts[c])

    def count_windows(self, counts: torch.Tensor, c: int, scores, targets, plan, windows, tp_classifier: bool) -> None:
        """A batch: the counts of every window of call c into counts[c]."""
        classification_counts_windows(scores, targets, plan, windows, tp_classifier, out=counts[c])

    def fold(self, counts: torch.Tensor, loss_c: torch.Tensor, loss_f: torch.Tensor) -> None:
        """One launch: every forward of counts [C, 4, W] and every chunk's (loss_c, loss_f) into the record."""
        C, _, W = counts.shape
        lc = loss_c.detach().reshape(-1)
        lf = loss_f.detach().reshape(-1)
        lc = lc if (lc.dtype == torch.float32 and lc.is_contiguous()) else lc.float().contiguous()
        lf = lf if (lf.dtype == torch.float32 and lf.is_contiguous()) else lf.float().contiguous()
        if lc.numel() != lf.numel():
            raise ValueError(f'TrainMonitor.fold: {lc.numel()} loss_c, {lf.numel()} loss_f')
        _lib.call('tmpnn_train_record_fold', counts.data_ptr(), int(C), int(W), lc.data_ptr(), lf.data_ptr(), int(lc.numel()),
                  self.record.data_ptr(), _lib.raw_stream(self.device))

    def read(self) -> Dict[str, float]:
        """The one device -> host copy: what train.py:157-171 logs, and the two divisors.  A mean over nothing (no forward /
        no chunk since the last reset) is NaN, as the reference's np.mean of an empty list."""
        raw = self.record.cpu().numpy()
        f = raw.view(np.float64)
        forwards, chunks = int(raw[1]), int(raw[5])
        nan = float('nan')
        return dict(avg_f1=float(f[0]) / forwards if forwards else nan,
                    avg_loss_c=float(f[2]) / chunks if chunks else nan,
                    avg_loss_f=float(f[3]) / chunks if chunks else nan,
                    avg_loss=float(f[4]) / chunks if chunks else nan,
                    forwards=forwards, chunks=chunks)
