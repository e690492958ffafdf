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

The validation pass computes the same F1 after every forward call of every sequence (train.py:207-219, :241-253) and logs the
mean (train.py:278).  A `ValMonitor` keeps it in a device record of its own (struct tmpnn_val_record): one launch per forward
(`tmpnn_val_f1_count`: targets from the tracker's label rows, counts, the fold) that `infer_sequence(..., monitor=vm)` issues
behind the model call on either of its paths -- the native driver included -- and `validate(..., monitor=vm)` reads once.
`val_counts_host` / `val_f1_host` are its definition in numpy (tests/test_val_f1.py pins them against the reference).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

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


_VAL_FIELDS = ('sum_f1', 'forwards', 'tp', 'fp', 'fn', 'rows')                            # struct tmpnn_val_record


def val_counts_host(is_edge, src, dst, labels, scores, tp_classifier: bool = True) -> Tuple[int, int, int, int]:
    """(tp, fp, fn, rows) of one forward call as the validation pass counts it (train.py:207-219), in numpy.

    Row form of the graph: is_edge [N], src / dst [N] = the ROWS of an edge row's earlier / later det (ignored on det rows),
    labels [N], scores [N] or [N, 1] = P(positive).  Targets (models/loss.py:8-44): a det's target is its label; per det the
    LAST label-positive edge that ends in it (a past edge: such rows lie above the det's) and the FIRST label-positive edge that
    starts from it (a future edge) get 1, every other edge 0 -- an edge chosen from both ends is one row.  pred = score > 0.5
    in float32 (argmax((1 - s, s)): the tie goes to class 0).  Counted over the edge rows and, with the TP classifier, the det
    rows; rows = N in either mode."""
    is_edge = np.asarray(is_edge).reshape(-1) != 0
    N = int(is_edge.size)
    src, dst = np.asarray(src).reshape(-1).astype(np.int64), np.asarray(dst).reshape(-1).astype(np.int64)
    lab = np.asarray(labels).reshape(-1) != 0
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    if not (src.size == dst.size == lab.size == s.size == N):
        raise ValueError(f'val_counts_host: {N} rows, {src.size} src, {dst.size} dst, {lab.size} labels, {s.size} scores')
    targets = lab & ~is_edge
    pos = np.flatnonzero(is_edge & lab)                                   # label-positive edge rows, ascending
    last_past = np.full(N, -1, np.int64)
    first_future = np.full(N, N, np.int64)
    np.maximum.at(last_past, dst[pos], pos)
    np.minimum.at(first_future, src[pos], pos)
    targets[last_past[last_past >= 0]] = True
    targets[first_future[first_future < N]] = True
    pred = s > np.float32(0.5)
    sel = is_edge if not tp_classifier else np.ones(N, bool)
    return (int((pred & targets & sel).sum()), int((pred & ~targets & sel).sum()), int((~pred & targets & sel).sum()), N)


def val_f1_host(counts: Sequence[Sequence[int]]) -> Dict:
    """What train.py:278 logs, from the (tp, fp, fn, rows) of every forward call in order: each call with rows > 0 is a forward
    of F1 = 2 tp / (2 tp + fp + fn) in float64, 0 where the denominator is 0 (f1_score(..., zero_division=0) -- an empty
    selection included); 'f1' their mean, the sum taken left to right (NaN over no forward), 'per_forward' the values."""
    per: List[float] = []
    tot = [0, 0, 0, 0]
    total = 0.0
    for tp, fp, fn, rows in counts:
        if rows <= 0:
            continue
        den = 2 * int(tp) + int(fp) + int(fn)
        f1 = float(2 * int(tp)) / float(den) if den > 0 else 0.0
        per.append(f1)
        total += f1
        tot = [a + int(b) for a, b in zip(tot, (tp, fp, fn, rows))]
    return dict(f1=total / len(per) if per else float('nan'), forwards=len(per), tp=tot[0], fp=tot[1], fn=tot[2], rows=tot[3],
                per_forward=per)


class ValMonitor:
    """The validation pass's F1 in device memory (module docstring).

    record  int64 [6] device tensor holding struct tmpnn_val_record bit for bit (sum_f1 as its bit pattern)
    log_forwards > 0: an int32 [log_forwards, 4] device log of every forward's (tp, fp, fn, rows); forwards beyond its end
    overwrite the last entry."""

    def __init__(self, device='cuda:0', log_forwards: int = 0):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'ValMonitor on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only '
                               '(no CPU or torch fallback exists)')
        if int(log_forwards) < 0:
            raise ValueError(f'ValMonitor: log_forwards={log_forwards}')
        self.device = dev
        self.record = torch.zeros(len(_VAL_FIELDS), dtype=torch.int64, device=dev)
        self.log_cap = int(log_forwards)
        self._log = torch.zeros((self.log_cap, 4), dtype=torch.int32, device=dev) if self.log_cap else None

    def reset(self) -> None:
        """Zero the record (and the log).  No host read."""
        self.record.zero_()
        if self._log is not None:
            self._log.zero_()

    def native_args(self) -> Tuple[int, int, int, int]:
        """(address of tmpnn_val_f1_count, record, log or 0, log capacity) for the native inference driver."""
        import ctypes as C
        return (C.cast(_lib.fn('tmpnn_val_f1_count'), C.c_void_p).value, self.record.data_ptr(),
                0 if self._log is None else self._log.data_ptr(), self.log_cap)

    def count(self, tg, scores: torch.Tensor, tp_classifier: bool = True) -> None:
        """One launch: the forward call that just ran on `tg.graph` (a tracking.TrackGraph BEFORE its decode: the label rows
        are the current row set's), scores [N] or [N, 1] as the model call returned them.  tp_classifier false: det rows are not
        counted (whether their scores were overwritten with 1 makes no difference).  No host read."""
        N = int(tg.N)
        sc = scores.detach().reshape(-1)
        if sc.numel() != N:
            raise ValueError(f'ValMonitor.count: {sc.numel()} scores for a graph of {N} rows')
        if N == 0:
            return
        sc = sc if (sc.dtype == torch.float32 and sc.is_contiguous()) else sc.float().contiguous()
        _lib.call('tmpnn_val_f1_count', tg.graph.cref(), tg.rows['labels'].data_ptr(), sc.data_ptr(), 1 if tp_classifier else 0,
                  self.record.data_ptr(), _lib.ptr(self._log), self.log_cap, _lib.raw_stream(self.device))

    def read(self) -> Dict:
        """The one device -> host copy: 'f1' = the mean over the forwards (train.py:278, a fraction; NaN over no forward),
        'forwards' and the summed 'tp', 'fp', 'fn', 'rows'."""
        raw = self.record.cpu().numpy()
        forwards = int(raw[1])
        return dict(f1=float(raw.view(np.float64)[0]) / forwards if forwards else float('nan'), forwards=forwards,
                    tp=int(raw[2]), fp=int(raw[3]), fn=int(raw[4]), rows=int(raw[5]))

    def log(self) -> np.ndarray:
        """int32 [forwards, 4] on the host: (tp, fp, fn, rows) of every forward since the last reset (log_forwards > 0 only;
        at most log_forwards rows)."""
        if self._log is None:
            raise RuntimeError('ValMonitor.log: built with log_forwards = 0')
        forwards = int(self.record[1].item())
        return self._log[:min(forwards, self.log_cap)].cpu().numpy()
