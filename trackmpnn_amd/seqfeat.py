"""Whole-sequence features on the device: the `{'X': [1, ND, F], 'y': [1, ND, 2]}` that validation and inference take.

In the reference these are the `val` / `test` samples of the dataset class (dataset/kitti_mot.py:488-568; bdd100k_mot.py follows
the same rules): the chunk of such a split lists every frame of a sequence (kitti_mot.py:228-230), no transform is drawn, and a
row holds the one-hot category, [score, xc, yc, w, h], with 'temp' the temporal pair of the row's frame, with 'vis' the 128
softmax columns read from the embedding CNN's map at the box centre; the whole row is standardised.  Training has the device path
`DetectionStore` -> `ChunkSampler.draw` -> `attach_vis` (chunks.py) and the stream has `OnlineTracker.push(..., frame=)`; this
module is the recorded-sequence pass, from the same `DetectionStore`:

    store = DetectionStore(sequences, ncategories, '2d+temp+vis', mean, std, device='cuda:0')
    sf = SequenceFeatures(store)
    seqs = sf.build()                                       # one launch: every sequence's X (static and temporal columns) and y
    sf.attach_vis(head, frames, embed_net)                  # per batch of frames: gather -> CNN -> VisHead.rows into X
    validate(model, seqs, evaluator)

(`trackmpnn_amd.loops.validate_store` / `infer_store` are that composition.)  A `ChunkSampler` cannot stand in: a chunk lists at
most 256 frames and 4096 detections, and a draw leaves a tail of unspecified rows.

    sequence_features_host   the DEFINITION, in numpy, from a host-only store: the store's rows of the sequence in the store's own
                             order (stable by frame, load order within a frame: the reference's order), X[:, :Fs] = stat[row, 0],
                             the temporal columns table[frame % fr_range], y = [frame, track]; with 'vis' the last 128 columns
                             are zero and the visual head's per-row arguments ride along.  By construction it equals
                             draw_chunks_host(..., random_transforms=False) on a chunk that lists every frame of the sequence,
                             wherever such a chunk is within the draw's limits (tests/test_seq_features.py: an independent path to
                             the same bits).
    listed_features_host     the definition of `build(sequences)`: the samples of a validated list of sequences, in its order.
    sequence_vis_host        the definition of the visual columns, by composition of functions the project has pinned already:
                             per batch of frames FrameStore.frames_host -> the caller's maps -> vis_head_host rows.
    SequenceFeatures         the device: tmpnn_seq_features (csrc/seqfeat.hip), one launch for any list of sequences; every value
                             is selected from the store's tables, not computed, so the device equals the definition bit for bit.

The reference's `__getitem__` with 'vis' needs torchvision.transforms, which the fixtures' generator (tools/gen_seqfeat_golden.py)
does not have: tests/golden/seqfeat pins the static and temporal columns and the labels against the reference's own dataset
classes, and the visual columns are pinned through sequence_vis_host's parts (tests/golden/vis, tests/golden/resize).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch

from . import _lib
from .chunks import DetectionStore
from .train_batch import _to_device
from .vishead import VIS_COLS, vis_head_host

FLAG_LIST, FLAG_RANGE, FLAG_FRAME = 1, 2, 4          # TMPNN_SF_FLAG_*


@dataclass
class SequenceSample:
    """What `sequence_features_host` returns (numpy).  The fields from `box` on are those of a store with 'vis' (None otherwise);
    X's last 128 columns are then zero until `sequence_vis_host`."""
    X: np.ndarray                           # float32 [ND, F]
    y: np.ndarray                           # int64 [ND, 2] = [frame, track id]
    box: Optional[np.ndarray] = None        # float32 [ND, 4]: the plain box
    im_hw: Optional[np.ndarray] = None      # float32 [ND, 2]
    frame: Optional[np.ndarray] = None      # int64 [ND] = y[:, 0]


def _sequence_list(store: DetectionStore, sequences, what: str) -> np.ndarray:
    """The listed sequences as int64 [K]: distinct indices of the store, in the caller's order (None: all of them)."""
    if sequences is None:
        return np.arange(store.nseq, dtype=np.int64)
    idx = np.asarray(sequences)
    if idx.ndim != 1 or idx.size == 0 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f'{what}: sequences must be a non-empty 1-d list of integers')
    if idx.min() < 0 or idx.max() >= store.nseq:
        raise IndexError(f'{what}: sequence {int(idx.max() if idx.min() >= 0 else idx.min())} of {store.nseq}')
    if np.unique(idx).size != idx.size:
        raise ValueError(f'{what}: a sequence is listed twice')
    return idx.astype(np.int64)


def _row_range(store: DetectionStore, s: int, f0: int = 0, f1: Optional[int] = None):
    """The store's rows of frames f0 .. f1 - 1 of sequence s (contiguous; default: the whole sequence)."""
    g = int(store.seq_base[s])
    f1 = int(store.num_frames[s]) if f1 is None else f1
    return int(store.first[g + f0]), int(store.first[g + f1])


def sequence_features_host(store: DetectionStore, s: int) -> SequenceSample:
    """The definition of the whole-sequence sample of sequence `s` (module docstring), in numpy; `store` may be host-only."""
    s = int(_sequence_list(store, [s], 'sequence_features_host')[0])
    r0, r1 = _row_range(store, s)
    rows = np.arange(r0, r1)
    fr = store.frame[rows].astype(np.int64)
    X = np.zeros((rows.size, store.F), np.float32)
    X[:, :store.Fs] = store.stat[rows, 0]
    if store.temp:
        X[:, store.Fs:store.Fv] = store.table[np.mod(fr, store.fr_range)]
    out = SequenceSample(X, np.stack([fr, store.track[rows].astype(np.int64)], 1))
    if store.vis:
        out.box, out.im_hw, out.frame = store.box[rows, 0], np.broadcast_to(store.im_hw[s], (rows.size, 2)).copy(), fr
    return out


def listed_features_host(store: DetectionStore, sequences=None) -> List[SequenceSample]:
    """The definition of SequenceFeatures.build(sequences): sequence_features_host of every listed sequence (distinct indices in
    any order; default: all), in the order of the list.  IndexError for an index outside the store, ValueError for a repeated
    one."""
    return [sequence_features_host(store, int(s)) for s in _sequence_list(store, sequences, 'listed_features_host')]


def _frame_batches(store: DetectionStore, s: int, frames_per_batch: int):
    """(f0, f1, r0, r1) of every batch of frames_per_batch frames of sequence s that holds a detection: frames f0 .. f1 - 1
    (aligned to multiples of frames_per_batch; the last one may be short), the store's rows r0 .. r1 - 1."""
    nf = int(store.num_frames[s])
    for f0 in range(0, nf, frames_per_batch):
        f1 = min(f0 + frames_per_batch, nf)
        r0, r1 = _row_range(store, s, f0, f1)
        if r1 > r0:
            yield f0, f1, r0, r1


def _check_vis_args(store: DetectionStore, frames, frames_per_batch, what: str) -> int:
    if not store.vis:
        raise ValueError(f"{what}: the store was built without 'vis'")
    fpb = int(frames_per_batch)
    if fpb < 1:
        raise ValueError(f'{what}: frames_per_batch={frames_per_batch}')
    if frames.nseq != store.nseq or not np.array_equal(frames.num_frames, store.num_frames):
        raise ValueError(f'{what}: the FrameStore does not hold the frames of the store\'s sequences')
    return fpb


def sequence_vis_host(store: DetectionStore, s: int, sample: SequenceSample, frames, embed: Callable, mean, std, input_hw,
                      down_ratio, frames_per_batch: int = 8) -> np.ndarray:
    """The definition of the visual columns of sequence `s`: per batch of frames (`_frame_batches`) images =
    frames.frames_host of the unmirrored frames (s, f, 0), maps = embed(images) (the caller's CNN on numpy [T, 3, H, W] ->
    [T, 128, Hm, Wm], float32 or float64), rows = vis_head_host(maps, box, frame - f0, im_hw, ...) written into the last 128
    columns of sample.X (in X's dtype: float32 as sequence_features_host made it; a test that wants the float64 rows hands over
    X.astype(float64)).  A batch without detections is not handed to `embed`.  Returns sample.X."""
    fpb = _check_vis_args(store, frames, frames_per_batch, 'sequence_vis_host')
    s = int(_sequence_list(store, [s], 'sequence_vis_host')[0])
    base = _row_range(store, s)[0]
    m, sd = np.asarray(mean).ravel()[-VIS_COLS:], np.asarray(std).ravel()[-VIS_COLS:]
    for f0, f1, r0, r1 in _frame_batches(store, s, fpb):
        a, b = r0 - base, r1 - base
        plan = np.stack([np.full(f1 - f0, s), np.arange(f0, f1), np.zeros(f1 - f0, np.int64)], 1).astype(np.int64)
        maps = np.asarray(embed(frames.frames_host(plan)))
        _, rows, _, _ = vis_head_host(maps, sample.box[a:b], sample.frame[a:b] - f0, sample.im_hw[a:b], np.full(b - a, -1),
                                      np.asarray([0, b - a]), m, sd, input_hw, down_ratio)
        sample.X[a:b, sample.X.shape[1] - VIS_COLS:] = rows
    return sample.X


class SequenceFeatures:
    """The whole-sequence samples of a DetectionStore on its device (module docstring).

        sf.build(sequences=None, frames_per_batch=8)   -> per listed sequence {'X': [1, ND, F] float32, 'y': [1, ND, 2] int64}
        sf.attach_vis(head, frames, embed_net, frames_per_batch=8)      the last 128 columns of a 'vis' store's X
        sf.check()                                     the one host read: RuntimeError if a launch refused a row

    After `build` the packed buffers are `X` [N, F], `y` [N, 2] and, with 'vis', `box` [N, 4], `im_hw` [N, 2], `map_of` [N]
    (int32); listed sequence k owns rows offsets[k] .. offsets[k + 1] (`offsets`: host int64 [K + 1]), `sequences` the list."""

    def __init__(self, store: DetectionStore):
        if store.device is None:
            raise RuntimeError('SequenceFeatures runs on the MI355X HIP kernels only (no CPU path): build the DetectionStore on a '
                               'cuda device (sequence_features_host is the host definition)')
        self.store = store
        self.device = store.device
        self.frame_d = _to_device(store.frame, self.device)           # the one table the training draw does not need
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.sequences = self.offsets = self.X = self.y = self.box = self.im_hw = self.map_of = None
        self.frames_per_batch = 0
        self._list_d = None

    def _launch(self, frames_per_batch: int) -> None:
        st, K, n = self.store, int(self.sequences.size), int(self.offsets[-1])
        self.frames_per_batch = frames_per_batch
        d = _lib.CSeqFeatures()
        d.K, d.nseq, d.F, d.Fs, d.ldx, d.fr_range, d.frames_per_batch = K, st.nseq, st.Fv, st.Fs, st.F, st.fr_range, frames_per_batch
        d.ndets, d.nframes, d.n_rows = st.ndets, int(st.seq_base[-1]), n
        d.offsets, d.seqs = self._list_d.data_ptr(), self._list_d.data_ptr() + 8 * (K + 1)
        d.seq_base, d.first, d.track = st.seq_base_d.data_ptr(), st.first_d.data_ptr(), st.track_d.data_ptr()
        d.frame, d.stat, d.table = self.frame_d.data_ptr(), st.stat_d.data_ptr(), st.table_d.data_ptr()
        d.X, d.y, d.flag = self.X.data_ptr(), self.y.data_ptr(), self.flag.data_ptr()
        if st.vis:
            d.box, d.seq_hw = st.box_d.data_ptr(), st.im_hw_d.data_ptr()
            d.o_box, d.o_im_hw, d.o_map_of = self.box.data_ptr(), self.im_hw.data_ptr(), self.map_of.data_ptr()
        _lib.call('tmpnn_seq_features', C.byref(d), _lib.raw_stream(self.device))

    def build(self, sequences=None, frames_per_batch: int = 8) -> List[dict]:
        """The packed X and y of the listed sequences (distinct indices in any order; default: all, in the store's order) in ONE
        launch, with no wait for the device; with 'vis' the same launch writes the packed box, im_hw and map_of (the row's frame
        index inside its batch of `frames_per_batch` frames aligned to multiples of it: frame % frames_per_batch), and the last
        128 columns of X are left unwritten (`attach_vis` fills them).  Returns per listed sequence the dict `validate` /
        `infer_dataset` take: views of the packed buffers; a sequence without detections gives X [1, 0, F].  The list and its
        packed offsets are the call's one small upload.  The kernel checks every table entry it indexes by; a row that fails is
        not written and raises the flag word `check()` reads (reachable only if the device tables were overwritten)."""
        st, dev = self.store, self.device
        idx = _sequence_list(st, sequences, 'SequenceFeatures.build')
        fpb = int(frames_per_batch)
        if fpb < 1:
            raise ValueError(f'SequenceFeatures.build: frames_per_batch={frames_per_batch}')
        K = int(idx.size)
        g0, g1 = st.seq_base[idx], st.seq_base[idx + 1]
        off = np.zeros(K + 1, np.int64)
        off[1:] = np.cumsum(st.first[g1].astype(np.int64) - st.first[g0])
        n = int(off[-1])
        words = np.empty(3 * K + 2, np.int32)                      # offsets int64 [K + 1] | seqs int32 [K]: one upload
        words[:2 * K + 2], words[2 * K + 2:] = off.view(np.int32), idx
        self._list_d = _to_device(words, dev)
        self.sequences, self.offsets = idx, off
        self.X = torch.empty((n, st.F), dtype=torch.float32, device=dev)
        self.y = torch.empty((n, 2), dtype=torch.int64, device=dev)
        self.box = self.im_hw = self.map_of = None
        if st.vis:
            fl = torch.empty(6 * n, dtype=torch.float32, device=dev)             # box [n, 4] | im_hw [n, 2]
            self.box, self.im_hw = fl[:4 * n].view(n, 4), fl[4 * n:].view(n, 2)
            self.map_of = torch.empty(n, dtype=torch.int32, device=dev)
        self._launch(fpb)
        return [{'X': self.X[off[k]:off[k + 1]].unsqueeze(0), 'y': self.y[off[k]:off[k + 1]].unsqueeze(0)} for k in range(K)]

    def attach_vis(self, head, frames, embed_net, frames_per_batch: int = 8) -> None:
        """The visual pass over the sequences of the last `build`: for each, its frames in batches of `frames_per_batch` (aligned
        to its multiples; the last one may be short); per batch images = frames.gather of the unmirrored frames (s, f, 0), maps =
        embed_net(images) under torch.no_grad() with the net in eval mode (its mode is restored afterwards), and
        head.rows(maps, box[rows], map_of[rows], im_hw[rows], out=X[rows], col=F - 128).  The rows of a frame range are
        contiguous in the store and every range is known on the host, so the pass issues no host read; columns [0, F - 128) of X
        stay untouched, and at most one batch of images and maps is alive at a time (`head.release()` after every batch).
        A batch whose frames hold no detection runs no CNN: in eval mode a net keeps no state from one call to the next, so
        leaving a call out changes nothing.  If `frames_per_batch` is not the one `build` was given, the build's launch runs
        once more with it first (map_of depends on it; every other value is rewritten as it was)."""
        st = self.store
        fpb = _check_vis_args(st, frames, frames_per_batch, 'SequenceFeatures.attach_vis')
        if self.sequences is None:
            raise RuntimeError('SequenceFeatures.attach_vis: build() first')
        if frames.device != self.device or head.device != self.device:
            raise ValueError(f'SequenceFeatures.attach_vis: the store is on {self.device}, the frames on {frames.device}, the head '
                             f'on {head.device}')
        if fpb != self.frames_per_batch and int(self.offsets[-1]):
            self._launch(fpb)
        col = st.F - VIS_COLS
        was_training = getattr(embed_net, 'training', None)
        if was_training is not None:
            embed_net.eval()
        try:
            with torch.no_grad():
                for k, s in enumerate(self.sequences):
                    shift = int(self.offsets[k]) - _row_range(st, int(s))[0]
                    nf = int(st.num_frames[s])
                    plan = np.stack([np.full(nf, s), np.arange(nf), np.zeros(nf, np.int64)], 1).astype(np.int64)
                    for f0, f1, r0, r1 in _frame_batches(st, int(s), fpb):
                        a, b = r0 + shift, r1 + shift
                        images = frames.gather(plan[f0:f1])
                        maps = embed_net(images)
                        head.rows(maps, self.box[a:b], self.map_of[a:b], self.im_hw[a:b], out=self.X[a:b], col=col)
                        head.release()
                        del images, maps
        finally:
            if was_training is not None:
                embed_net.train(was_training)

    def check(self) -> None:
        """The host read of the flag word every launch of this object ORs into (one wait for the device).  The word is never
        cleared: once a launch has refused a row the device tables are not to be trusted, and every later check() raises."""
        flag = int(self.flag.item())
        if flag:
            what = [w for bit, w in ((FLAG_LIST, 'the sequence list or its packed offsets'), (FLAG_RANGE, 'seq_base / first'),
                                     (FLAG_FRAME, 'a row\'s frame')) if flag & bit]
            raise RuntimeError(f'SequenceFeatures: the kernel refused rows (flag {flag}: {", ".join(what)} inconsistent with the '
                               "store's totals): the device tables were overwritten")
