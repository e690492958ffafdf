"""What the device evaluators over per-sequence stores share (moteval.py, hota.py, evalprep.py, results.py; mapeval.py takes the
device refusal and `cat`): one definition of each piece, nothing that belongs to one metric.

    FLAG_*                the low byte of a sequence's flag word (csrc/eval_common.h); the 1-based frame index sits above it
    _ints, _boxes         the checked integer / float32 box arrays of an argument;  _frame_range: the frame range of both sides
    cat                   the one concatenation of per-sequence parts, with a dtype and the shape of the empty case
    frame_sort            one side of one sequence: the stable order by frame and the per-frame offsets over a frame range
    SeqTable              the `seq` table of a store while it is built: running bases, the [S, 8] rows, the parts by name
    pack_tracks           the tracks of an evaluation into the device buffer, one packed upload at the most
    flag_message          the text of a read() that met flag words
    upload                a store's arrays on the device, by name, and their pointers
    cuda_device           the refusal of a device that is not the GPU
    SequenceEvaluator     the skeleton of MotEvaluator, HotaEvaluator, EvalPrep and TrackResults: the store on the device, the
                          enqueue step, the read step with its flag check, the per-sequence loop, the filtered-track views
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib

FLAG_LIMIT, FLAG_DUPLICATE, FLAG_STORE, FLAG_SOLVER = 1, 2, 4, 8


def _boxes(b, what: str) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float32)).reshape(-1, 4) if np.size(b) else np.zeros((0, 4), np.float32)
    return b


def _ints(a, what: str, n: Optional[int] = None) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f'{what}: integer values expected, got {a.dtype}')
    a = a.astype(np.int64).reshape(-1)
    if n is not None and a.shape[0] != n:
        raise ValueError(f'{what}: {a.shape[0]} entries for {n} rows')
    return a


def _frame_range(det_frame: np.ndarray, gt_frame: np.ndarray):
    """(first frame, number of frames) of both sides together, every row counted (metrics.py:19-27); (0, 0) without rows."""
    both = np.concatenate([det_frame, gt_frame])
    if both.size == 0:
        return 0, 0
    return int(both.min()), int(both.max()) - int(both.min()) + 1


def cat(parts, dtype, tail=()):
    return np.ascontiguousarray(np.concatenate(parts).astype(dtype)) if parts else np.zeros((0,) + tail, dtype)


def frame_sort(frame: np.ndarray, t0: int, nf: int, keep: Optional[np.ndarray] = None):
    """One side of one sequence, sorted STABLY by frame: (order, off).  order: sorted position -> arrival index, over the rows
    `keep` (ascending arrival indices; default: every row); off: int32 [nf + 1], the first sorted position of every frame of
    t0 .. t0 + nf - 1 and, last, the number of rows."""
    order = np.argsort(frame if keep is None else frame[keep], kind='stable')
    if keep is not None:
        order = keep[order]
    return order, np.searchsorted(frame[order], np.arange(t0, t0 + nf + 1), side='left').astype(np.int32)


class SeqTable:
    """The `seq` table of a store while its constructor walks the sequences: int64 [S, 8], four (base, count) pairs a row -- two
    kinds of rows the store names, the per-frame offsets (count n_frames, n_frames + 1 entries), and a fourth kind -- with the
    running bases, and the parts of every packed array by name.  The limits are the store's: `max_rows` rows of one side of a
    sequence (and 2^31 - 1 frames) with `beyond` as the message's end, `max_sequences` in one store."""

    def __init__(self, who: str, S: int, max_rows: int = 2 ** 31 - 1, beyond: str = 'is beyond int32', max_sequences: Optional[int] = None):
        if max_sequences is not None and S > max_sequences:
            raise ValueError(f'{who}: {S} sequences, at most {max_sequences} in one store')
        self.who, self.max_rows, self.beyond = who, max_rows, beyond
        self.seq = np.zeros((S, 8), np.int64)
        self.totals = [0, 0, 0, 0]
        self.parts: Dict[str, List[np.ndarray]] = {}

    def check(self, s: int, nf: int, rows: int) -> None:
        if nf >= 2 ** 31 - 1 or rows >= self.max_rows:
            raise ValueError(f'{self.who}: sequence {s} {self.beyond}')

    def add(self, s: int, n_a: int, n_b: int, nf: int, n_c: int = 0, **parts) -> None:
        """Row s: n_a and n_b rows of the two kinds, nf frames, n_c of the fourth kind; parts: this sequence's piece of every array."""
        a, b, f, c = self.totals
        self.seq[s] = (a, n_a, b, n_b, f, nf, c, n_c)
        self.totals = [a + n_a, b + n_b, f + nf + 1, c + n_c]
        for k, v in parts.items():
            self.parts.setdefault(k, []).append(v)

    def pack(self, name: str, dtype, tail=()) -> np.ndarray:
        return cat(self.parts.get(name, []), dtype, tail)


def pack_tracks(det: Sequence, n_det: int, tracks: Sequence, buf: torch.Tensor, who: str) -> List[bool]:
    """The tracks of an evaluation into `buf` (int32 [n_det] on the device, sequence s at det[s] = (base, n)): host arrays go up in
    one packed copy at the most (-1 for a sequence given as None), device tensors are copied on the device.  Returns, per
    sequence, whether it was left out."""
    if len(tracks) != len(det):
        raise ValueError(f'{who}: {len(tracks)} track arrays for {len(det)} sequences')
    host = np.full(n_det, -1, np.int32)
    on_device = []
    left_out = []
    host_used = False
    for s, tr in enumerate(tracks):
        base, n = det[s]
        left_out.append(tr is None)
        if tr is None:
            host_used |= n > 0                                  # (its slice is filled with -1)
            continue
        if isinstance(tr, torch.Tensor) and tr.is_cuda:
            if tr.dtype.is_floating_point or tr.numel() != n:
                raise ValueError(f'{who}: sequence {s}: an int tensor of {n} tracks expected')
            on_device.append((base, n, tr))
        else:
            a = _ints(tr, f'{who}: sequence {s}: tracks', n)
            if a.size and (a.max() >= 2 ** 31 or a.min() < -2 ** 31):
                raise ValueError(f'{who}: sequence {s}: track ids are int32')
            host[base:base + n] = a
            host_used |= n > 0
    if host_used:
        buf[:n_det].copy_(torch.from_numpy(host), non_blocking=True)          # the one packed upload
    for base, n, tr in on_device:
        buf[base:base + n].copy_(tr.reshape(-1))
    return left_out


def flag_message(who: str, flags, t0_of, texts: Dict[int, str]) -> str:
    """The text of a read() that met flag words.  flags: (sequence, word) pairs; t0_of(s): the frame at which the frame count in
    the words of sequence s starts; texts: bit -> text."""
    return f'{who}: ' + '; '.join(f'sequence {s}' + (f', frame {t0_of(s) + (f >> 8) - 1}: ' if f >> 8 else ': ')
                                  + ', '.join(txt for bit, txt in texts.items() if f & bit) for s, f in flags)


def upload(store, names: Sequence[str], dev):
    """The store's arrays `names` on the device: (tensors by name, their addresses in that order, None for an empty one).  A
    uint32 array goes up as the int32 tensor of the same bytes."""
    t = {}
    for k in names:
        a = getattr(store, k)
        t[k] = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
    return t, [t[k].data_ptr() or None for k in names]


def cuda_device(device, who: str, otherwise: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(f'{who} on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path): pass a cuda device, '
                           f'or {otherwise}')
    return dev


class SequenceEvaluator:
    """The skeleton of an evaluator over a per-sequence store (`seq[:, 2:4]` = det_base, n_det; `S`, `n_det`).  A subclass sets
    STEP, FLAG_WORD and FLAG_TEXT, builds its store and its struct over `_attach`, allocates `_out`, enqueues through `_enqueue`
    and reads through `_read`, for which it supplies `_row`: record -> dict."""
    STEP = ('evaluate', 'evaluation')          # the enqueueing method, and what read() misses without it
    FLAG_WORD: int                             # the column of the flag word in a record
    FLAG_TEXT: Dict[int, str]

    def __init__(self, device, otherwise: str):
        self.device = cuda_device(device, type(self).__name__, otherwise)

    def _attach(self, st, names: Sequence[str]) -> List:
        """Take the store: its arrays `names` go up (`_t`), the track buffer is allocated.  Returns the arrays' addresses."""
        self.store = st
        self._seq_host = np.ascontiguousarray(st.seq)
        self._det = [(int(b), int(n)) for b, n in st.seq[:, 2:4]]
        self._t, ptrs = upload(st, names, self.device)
        self._tracks = torch.empty(max(st.n_det, 1), dtype=torch.int32, device=self.device)
        self._left_out = [False] * st.S
        self._pending = False
        return ptrs

    def _workspace(self, nbytes: int) -> None:
        self._ws_bytes = int(nbytes)
        self._ws = torch.empty(max(self._ws_bytes, 16), dtype=torch.uint8, device=self.device)

    def _enqueue(self, entry: str, tracks: Sequence, *args) -> None:
        """Pack the tracks and call `entry`(store, seq_host, tracks, *args, stream); the evaluation counts once the call returned."""
        left_out = pack_tracks(self._det, self.store.n_det, tracks, self._tracks, f'{type(self).__name__}.{self.STEP[0]}')
        _lib.call(entry, C.byref(self._c), self._seq_host.ctypes.data, self._tracks.data_ptr(), *args, _lib.raw_stream(self.device))
        self._left_out = left_out
        self._pending = True

    def _need_pending(self, method: str) -> None:
        if not self._pending:
            raise RuntimeError(f'{type(self).__name__}.{method}: no {self.STEP[1]} has been enqueued')

    def _views(self, buf: torch.Tensor, first: int = 0) -> List[torch.Tensor]:
        """filtered_tracks(): per sequence the view of its ids in `buf`, whose element `first` is the id of row 0."""
        self._need_pending('filtered_tracks')
        return [buf[first + b:first + b + n] for b, n in self._det]

    def _read(self, check: bool, records=None, t0_of=None) -> List:
        """Per sequence the dict of `_row(s, rec, fl, out)` (rec: the records, fl: their words as float64, out: everything that was
        copied), None for one left out; 'flag' in every dict under check=False.  records: the int64 [S, words] records in what
        was copied (default: all of it); t0_of(s): first frame (default: store.t0[s])."""
        self._need_pending('read')
        out = self._out.cpu().numpy()                               # (the one device -> host copy; it waits for the launches)
        rec = out if records is None else records(out)
        flag, fl = rec[:, self.FLAG_WORD], rec.view(np.float64)
        bad = [(s, int(flag[s])) for s in range(self.store.S) if flag[s] != 0 and not self._left_out[s]]
        if bad and check:
            raise RuntimeError(flag_message(f'{type(self).__name__}.read', bad, t0_of or self.store.t0.__getitem__, self.FLAG_TEXT))
        per: List = []
        for s in range(self.store.S):
            if self._left_out[s]:
                per.append(None)
                continue
            r = self._row(s, rec, fl, out)
            if not check:
                r['flag'] = int(flag[s])
            per.append(r)
        return per
