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

With visual features the reference also logs the embedding network's loss ("Average embedding loss for epoch", train.py:157-163):
`train_epoch(vis=..., monitor=m)` hands the kept chunks' `loss_d` to `m.fold_embed` (one launch, a record of its own: struct
tmpnn_embed_record), and `read()` then also carries `avg_loss_d` and `avg_loss_total`.

Every (call, chunk) pair of a batch in which the chunk has rows is one forward, so a batched epoch averages over the same
forwards as the reference's chunk-by-chunk loop.  Under `trackmpnn_amd.dist` each rank's monitor covers its own shard.

The validation pass computes the same F1 after every forward call of every sequence (train.py:207-219, :241-253) and logs the
mean (train.py:278).  A `ValMonitor` keeps it in a device record of its own (struct tmpnn_val_record): one launch per forward
(`tmpnn_val_f1_count`: targets from the tracker's label rows, counts, the fold) that `infer_sequence(..., monitor=vm)` issues
behind the model call on either of its paths -- the native driver included -- and `validate(..., monitor=vm)` reads once.
`val_counts_host` / `val_f1_host` are its definition in numpy (tests/test_val_f1.py pins them against the reference).

The reference's third program, attention_weights.py, produces the paper's attention figure: per head, the distribution of the
attention weights detections give to correct and to incorrect associations.  It stores every head's dense [N, N] matrix after
every model call inside the timestep loop and walks N^2 x K entries on the host.  An `AttentionMonitor` keeps the two histograms
of every head in a device record (struct tmpnn_att_record + int64 [K][2][bins]): one launch per forward and group of up to 8
heads (`tmpnn_att_hist_count`, csrc/atthist.hip) over the [2E] CSR-ordered `alpha` the attention kernels wrote, issued by
`infer_sequence(..., att_monitor=am)` behind each of those model calls and read once by `validate(..., att_monitor=am)`;
`att_hist_host` is its definition in numpy (tests/test_att_hist.py pins it against the reference's dense walk).
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
        self.embed_record: Optional[torch.Tensor] = None      # int64 [3]: struct tmpnn_embed_record, made by the first fold_embed

    def reset(self) -> None:
        """Zero the record (an epoch boundary).  No host read."""
        self.record.zero_()
        self.embed_record = None

    def fold_embed(self, loss_d: torch.Tensor, kept: Optional[torch.Tensor] = None) -> None:
        """One launch: the embedding network's loss of the chunks `kept` (int64 indices on the device into loss_d [n]; None: every
        chunk) into a record of its own: an fp64 sum in a fixed order and the number of chunks.  `read()` then also gives
        'avg_loss_d' and 'avg_loss_total' (train.py:157-163).  No host read."""
        ld = loss_d.detach().reshape(-1)
        ld = ld if (ld.dtype == torch.float32 and ld.is_contiguous()) else ld.float().contiguous()
        if ld.device != self.record.device:
            raise ValueError(f'TrainMonitor.fold_embed: loss_d on {ld.device}, the monitor on {self.record.device}')
        if kept is not None:
            if kept.device != ld.device or kept.dtype != torch.int64:
                raise ValueError('TrainMonitor.fold_embed: kept must be an int64 tensor on the device of loss_d')
            kept = kept.reshape(-1).contiguous()
        if self.embed_record is None:
            self.embed_record = torch.zeros(3, dtype=torch.int64, device=self.record.device)
        n_kept = int(ld.numel() if kept is None else kept.numel())
        _lib.call('tmpnn_train_embed_fold', ld.data_ptr() if ld.numel() else None, int(ld.numel()), _lib.ptr(kept) if n_kept else None,
                  n_kept, self.embed_record.data_ptr(), _lib.raw_stream(self.device))

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
        no chunk since the last reset) is NaN, as the reference's np.mean of an empty list.  If fold_embed ran since the last
        reset(), also 'avg_loss_d' = the mean of loss_d over the chunks it took and 'avg_loss_total' = the mean of
        loss_d + loss_c + loss_f over the chunks = avg_loss_d + avg_loss (both folds take the kept chunks of every step); the
        copy then carries both records."""
        if self.embed_record is None:
            raw = self.record.cpu().numpy()
        else:
            both = torch.cat([self.record, self.embed_record]).cpu().numpy()
            raw, eraw = both[:len(_FIELDS)], both[len(_FIELDS):]
        f = raw.view(np.float64)
        forwards, chunks = int(raw[1]), int(raw[5])
        nan = float('nan')
        out = dict(avg_f1=float(f[0]) / forwards if forwards else nan,
                   avg_loss_c=float(f[2]) / chunks if chunks else nan,
                   avg_loss_f=float(f[3]) / chunks if chunks else nan,
                   avg_loss=float(f[4]) / chunks if chunks else nan,
                   forwards=forwards, chunks=chunks)
        if self.embed_record is not None:
            if int(eraw[2]):
                raise RuntimeError(f'TrainMonitor.read: fold_embed was handed {int(eraw[2])} chunk indices outside loss_d')
            n_d = int(eraw[1])
            out['avg_loss_d'] = float(eraw.view(np.float64)[0]) / n_d if n_d else nan
            out['avg_loss_total'] = out['avg_loss_d'] + out['avg_loss']
        return out


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


ATT_HIST_KMAX = 8            # TMPNN_ATT_HIST_KMAX: heads per counting launch
ATT_HIST_MAX_BINS = 64       # TMPNN_ATT_HIST_MAX_BINS
ATT_HIST_HEADER = 4          # TMPNN_ATT_HIST_HEADER: forwards, dets, isolated, zeros (struct tmpnn_att_record)


def att_hist_edges(bins: int = 25) -> np.ndarray:
    """The float32 edge table np.histogram uses for float32 values with `bins` and range (0, 1): [bins + 1]."""
    return np.histogram_bin_edges(np.zeros(0, np.float32), int(bins), (0.0, 1.0)).astype(np.float32)


def att_csr_host(is_edge, src, dst):
    """(det rows ascending, rowptr [Dn + 1], inc [2E]) of a graph in row form (src / dst [N]: the ROWS of an edge row's earlier /
    later det): per det its incident edge rows ascending, the sign bit set where the det is the edge's LATER end -- the CSR
    order of tmpnn_dgraph.inc, i.e. the order of a head's `alpha`."""
    is_edge = np.asarray(is_edge).reshape(-1) != 0
    src, dst = np.asarray(src).reshape(-1).astype(np.int64), np.asarray(dst).reshape(-1).astype(np.int64)
    er = np.flatnonzero(is_edge)
    dets = np.flatnonzero(~is_edge)
    end = np.concatenate([src[er], dst[er]])                      # the det of every (edge, side)
    val = np.concatenate([er, er | 0x80000000])
    order = np.lexsort((np.concatenate([er, er]), end))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(dets, end), minlength=dets.size))]).astype(np.int64)
    return dets, rowptr, val[order].astype(np.int64)


def att_hist_host(is_edge, labels, alphas, N: Optional[int] = None, bins: int = 25, rowptr=None, inc=None, src=None, dst=None) -> Dict:
    """The attention histograms of ONE forward call as the reference's head study counts them (attention_weights.py:84-105), in
    numpy, on the CSR form.

    is_edge [N], labels [N]; the graph either as rowptr [Dn + 1] / inc [2E] (edge row | sign bit, as tmpnn_dgraph) or in row
    form src / dst [N] (att_csr_host derives the CSR); alphas [K, 2E] float32: head k's weight at CSR position p, i.e. what
    the det that owns p gives the edge row inc[p]; N: the call's row count (default is_edge.size).

    Selection: the reference looks at every det ROW of a head's dense [N, N] matrix and every EDGE column whose entry is > 0.
    In eval mode a det with incident edges holds its softmax over them and exact zeros elsewhere, so it contributes its alphas
    -- one that underflowed to exactly 0 is skipped by the `> 0` test ('zeros' counts them).  A det with NO incident edge
    holds the uniform value float32(1) / float32(N) in every column (an all-masked softmax): it contributes that value once
    for every edge row of the graph.  A value is `tp` where the edge row's label == 1 and `fp` for every other label.  Each
    list is binned with np.histogram(values.astype(np.float32), bins, (0.0, 1.0)): half-open bins, the last one closed.

    Returns counts int64 [K, 2, bins] ([k, 0] = tp, [k, 1] = fp), edges float32 [bins + 1], forwards (1 if the graph has
    rows), dets, isolated, zeros."""
    is_edge = np.asarray(is_edge).reshape(-1) != 0
    lab = np.asarray(labels).reshape(-1)
    N = int(is_edge.size if N is None else N)
    if rowptr is None:
        _, rowptr, inc = att_csr_host(is_edge, src, dst)
    rowptr, inc = np.asarray(rowptr).reshape(-1).astype(np.int64), np.asarray(inc).reshape(-1).astype(np.int64)
    a = np.asarray(alphas, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    K, P = a.shape[0], int(inc.size)
    Dn, E = int(rowptr.size) - 1, P // 2
    if a.shape[1] != P or lab.size != is_edge.size or P != 2 * int(is_edge.sum()) or Dn != int((~is_edge).sum()):
        raise ValueError(f'att_hist_host: alphas {a.shape}, {P} CSR positions, {lab.size} labels, {is_edge.size} rows')
    edge_tp = lab[inc & 0x7FFFFFFF] == 1                            # per CSR position: the edge row's label is 1
    n_iso = int((rowptr[1:] == rowptr[:-1]).sum())
    edge_lab = lab[is_edge] == 1
    uniform = np.float32(1.0) / np.float32(max(N, 1))
    counts = np.zeros((K, 2, int(bins)), np.int64)
    zeros = 0
    for k in range(K):
        live = a[k] > 0
        zeros += int((~live).sum())
        for side, sel in ((0, edge_tp), (1, ~edge_tp)):
            vals = a[k][live & sel]
            iso = np.full(n_iso * int((edge_lab if side == 0 else ~edge_lab).sum()), uniform, np.float32)
            counts[k, side] = np.histogram(np.concatenate([vals, iso]).astype(np.float32), int(bins), (0.0, 1.0))[0]
    return dict(counts=counts, edges=att_hist_edges(bins), forwards=int(E + Dn > 0), dets=Dn, isolated=n_iso, zeros=zeros)


class AttentionMonitor:
    """The head study's histograms in device memory (module docstring).

    record  int64 [4 + K * 2 * bins] device tensor: struct tmpnn_att_record (forwards, dets, isolated, zeros), then the counts
            [K][2][bins] ([k][0] = tp: the edge's label is 1, [k][1] = fp)
    edges   float32 [bins + 1] device tensor: np.histogram's edge table for float32 values, bins, range (0, 1)
    feature_set: which feature group's heads are counted (attention_weights.py:60 stores group 0)."""

    def __init__(self, device='cuda:0', nattheads: int = 0, bins: int = 25, feature_set: int = 0):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'AttentionMonitor on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only '
                               '(no CPU or torch fallback exists)')
        if int(nattheads) < 1:
            raise ValueError(f'AttentionMonitor: nattheads={nattheads}: a model without attention heads has no weights to count')
        if not 1 <= int(bins) <= ATT_HIST_MAX_BINS:
            raise ValueError(f'AttentionMonitor: bins={bins} (1 .. {ATT_HIST_MAX_BINS})')
        if int(feature_set) < 0:
            raise ValueError(f'AttentionMonitor: feature_set={feature_set}')
        self.device = dev
        self.K, self.bins, self.feature_set = int(nattheads), int(bins), int(feature_set)
        self.edges_host = att_hist_edges(self.bins)
        self.edges = torch.from_numpy(self.edges_host).to(dev)
        self.record = torch.zeros(ATT_HIST_HEADER + self.K * 2 * self.bins, dtype=torch.int64, device=dev)

    def reset(self) -> None:
        """Zero the record.  No host read."""
        self.record.zero_()

    @staticmethod
    def _one_buffer(grp: List[torch.Tensor]) -> Optional[Tuple[int, int]]:
        """(address, stride in floats) where the heads' alphas are rows of ONE buffer (as the attention stage returns them:
        slices alpha[k, :2E] of a [Kg, max(2E, 1)] tensor), else None."""
        a0 = grp[0]
        n = int(a0.numel())
        if n == 0:                                   # (no edges: an empty tensor has no address; count() hands over zeros)
            return None
        if any(a.dtype != torch.float32 or a.dim() != 1 or int(a.numel()) != n or (n > 1 and a.stride(0) != 1) for a in grp):
            return None
        if len(grp) == 1:
            return a0.data_ptr(), max(n, 1)
        step = grp[1].data_ptr() - a0.data_ptr()
        if step < 4 * max(n, 1) or step % 4:
            return None
        st = a0.untyped_storage().data_ptr()
        if any(a.untyped_storage().data_ptr() != st or a.data_ptr() - a0.data_ptr() != k * step for k, a in enumerate(grp)):
            return None
        return a0.data_ptr(), step // 4

    def count(self, tg, attention) -> None:
        """The launches of ONE forward: `tg` the tracking.TrackGraph the model call just ran on (BEFORE its decode: the label
        rows are the current row set's), `attention` the call's fourth output -- per feature group a list of SparseAttention.
        One launch per group of up to 8 heads (the first one counts the forward).  No host read."""
        if attention is None or self.feature_set >= len(attention) or attention[self.feature_set] is None:
            raise ValueError(f'AttentionMonitor.count: the call returned no attention for feature group {self.feature_set} '
                             f'(a model without heads?); the monitor was built for {self.K} heads')
        heads = attention[self.feature_set]
        if len(heads) != self.K:
            raise ValueError(f'AttentionMonitor.count: {len(heads)} heads handed in, the monitor was built for {self.K}')
        N = int(tg.N)
        if N == 0:
            return
        alphas = [h.alpha.detach() for h in heads]
        n = int(alphas[0].numel())
        st = _lib.raw_stream(self.device)
        for k0 in range(0, self.K, ATT_HIST_KMAX):
            grp = alphas[k0:k0 + ATT_HIST_KMAX]
            one = self._one_buffer(grp)
            if one is None:
                if any(int(a.numel()) != n for a in grp):
                    raise ValueError('AttentionMonitor.count: the heads hold different numbers of weights')
                buf = torch.zeros((len(grp), max(n, 1)), dtype=torch.float32, device=self.device)
                if n:
                    torch.stack([a.reshape(-1).float() for a in grp], out=buf)
                one = (buf.data_ptr(), max(n, 1))
            _lib.call('tmpnn_att_hist_count', tg.graph.cref(), tg.rows['labels'].data_ptr(), one[0], one[1], len(grp), k0,
                      self.edges.data_ptr(), self.bins, self.record.data_ptr(), 1 if k0 == 0 else 0, st)

    def read(self) -> Dict:
        """The one device -> host copy: 'counts' int64 [K, 2, bins] (tp = 0, fp = 1), 'edges' float32 [bins + 1], 'forwards',
        and the header's 'dets', 'isolated', 'zeros'."""
        raw = self.record.cpu().numpy()
        return dict(counts=raw[ATT_HIST_HEADER:].reshape(self.K, 2, self.bins).copy(), edges=self.edges_host.copy(),
                    forwards=int(raw[0]), dets=int(raw[1]), isolated=int(raw[2]), zeros=int(raw[3]))

    def normalized(self, result: Optional[Dict] = None) -> np.ndarray:
        """float64 [K, 2, bins]: every histogram divided by its total, as the figure plots it (attention_weights.py:99-105:
        weights = 1 / len); a histogram without values is NaN.  result: a dict of read() (default: read now)."""
        counts = (self.read() if result is None else result)['counts'].astype(np.float64)
        total = counts.sum(-1, keepdims=True)
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(total > 0, counts / total, np.nan)
