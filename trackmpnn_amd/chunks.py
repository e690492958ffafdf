"""Training chunks drawn on the device: the reference's --random-transforms (time reversal, horizontal flip, detection dropout).

The reference redraws every chunk each time its dataset hands it out (dataset/kitti_mot.py:488-568; bdd100k_mot.py follows the
same rules): two decisions per chunk (reverse time, flip horizontally, p = 0.5 each), then every detection is dropped with
p = dropout_ratio = 0.2, and the features are computed from what is left.  Here the sequences are kept on the device once
(`DetectionStore`), and a seeded draw of B chunks (`ChunkSampler.draw`, csrc/chunkdraw.hip) is written in the stacked form
`build_train_batch_device(y, offsets=...)` and `train_chunks(model, batch, X)` take, without the host waiting for the device:

    chunks = make_chunks(num_frames, cur_win_size, ret_win_size)            # the reference's chunk list (its call order on `random`)
    store = DetectionStore(sequences, ncategories, '2d+temp', mean, std, device='cuda:0')
    sampler = ChunkSampler(store, chunks, seed)
    for idx in batches(sampler.epoch_order(epoch)):
        drawn = sampler.draw(idx, step)                                     # DrawnChunks: X, y, offsets, flags on the device
        batch = drawn.batch()                                               # build_train_batch_device(..., padded=True)
        train_chunks(model, batch, drawn.features(batch))

(`trackmpnn_amd.loops.train_epoch` is that loop with the optimizer step.)  Reading detection files stays outside the library:
the store is built from arrays
(where only a detector's output and the labels are at hand, `trackmpnn_amd.labeling.DetectionLabeler.store_sequences()` gives the
`track` ids: the reference's get_track_ids, on the plain boxes).

The rules (kitti_mot.py, `t` = frame, W = image width, `frames` = the chunk's frame list):
  * rows of a chunk: the detections of its frames in list order, in load order within a frame (also under time reversal, so
    reversed timestamps descend);
  * flip acts on the raw box in Python floats, x1' = W - x2 - 1, x2' = W - x1 - 1, and is then stored as float32 (:350-353);
  * time reversal: t' = frames[-1] - t + frames[0], the ends of the LIST (:522-524); track ids do not change;
  * features, float32 (:545-566): one-hot category, [score, (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], with 'temp' the
    pair sin a, cos a of a = mod(t', fr_range) * pi / fr_range; then (features - mean) / std;  y = [t', track id].

A drawn feature row is selected, not computed: the store holds, per detection, the standardised static row of the plain box
and of the flipped box, both in the reference's own arithmetic on the host, and a `fr_range`-entry table of the standardised
temporal pair.  Flip changes the centre column and, because x1' and x2' are rounded to float32 on their own, for most boxes
the last bit of the width column as well; time reversal changes the two table columns.  So the device features equal the reference's
arithmetic bit for bit by construction.

The visual group ('2d+vis', '2d+temp+vis': the reference's default).  Its 128 columns come from the embedding CNN's map at the box
centre, so a draw cannot select them; it carries what the visual head (vishead.py) needs instead: per kept row `box` (the box the
row's features were made from, mirrored iff the chunk is flipped), `im_hw`, `map_of` (the image the row needs) and `track`, written
by one more launch with the fill's decisions.  The images of a draw are known on the host before any launch
(`ChunkSampler.frame_plan`): the image of a row is that of its LISTED frame -- time reversal relabels t' only -- mirrored iff its
chunk is flipped, and the flip is Philox block j = 0, which the host computes as the device does.  `FrameStore.gather(plan)`
(frames.py) gives the CNN's input, `DrawnChunks.attach_vis(head, maps)` writes the rows into the last 128 columns of X and returns
the per-chunk identity loss; everything else of the draw is bit for bit that of the same store without 'vis'.

Random numbers: Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and counter = (j, chunk index in the dataset,
step & 0xffffffff, step >> 32).  Block j = 0: word 0 decides reversal, word 1 flip.  Block j >= 1: word w decides row
4 (j - 1) + w of the chunk, rows counted in output order before dropout.  u = (word >> 8) * 2^-24 (exact in float32), and the
event happens iff u < float32(p).  A chunk's draw is keyed by its index in the dataset, so it does not depend on the batch it
lands in or on its position there.  This is the same DISTRIBUTION as the reference's `random.random()` decisions, not the same
stream: a run here does not reproduce the reference's individual draws, only their statistics.
"""
from __future__ import annotations

import ctypes as C
import random
import re
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .embedloss import embedding_loss_host
from .train_batch import TB_MAX_DETS, AllChunksSkipped, _to_device, build_train_batch_device
from .vishead import VIS_COLS, vis_head_host

CD_MAX_FRAMES = 256                  # TMPNN_CD_MAX_FRAMES: frames of one chunk's list
FLAG_REVERSED, FLAG_FLIPPED, FLAG_BAD = 1, 2, 128            # TMPNN_CD_FLAG_*
_ORDER_STREAM = 0xFFFFFFFF           # counter word 1 of epoch_order (no chunk index reaches it)

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32 (Salmon et al., SC'11; 10 rounds by default) of counters [..., 4] under keys [..., 2] (broadcast against each
    other), as uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    m0, m1 = np.uint64(_M0), np.uint64(_M1)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                                    # (32 x 32 -> 64 bits: no overflow in uint64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _MASK, (p0 >> s32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def _uniform(words: np.ndarray) -> np.ndarray:
    """u = (word >> 8) * 2^-24 in float32 (exact)."""
    return (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _split64(v: int, what: str) -> Tuple[int, int]:
    v = int(v)
    if not 0 <= v < 2 ** 64:
        raise ValueError(f'{what}={v} is outside [0, 2^64)')
    return v & 0xFFFFFFFF, v >> 32


def make_chunks(num_frames: Sequence[int], cur_win_size: int, ret_win_size: int, rng=random) -> List[Tuple[int, List[int]]]:
    """The reference's training chunks (kitti_mot.py:218-227) as [(sequence index, [frames])]: for every sequence and every
    st in range(0, num_frames, cur_win_size // 2) the frames st .. min(st + cur_win_size, num_frames) - 1; one
    rng.randint(st + cur_win_size, st + cur_win_size + ret_win_size) gives skip_fr, and where skip_fr < num_frames - 1 the
    frames skip_fr and skip_fr + 1 are appended.  The calls on `rng` are the reference's in its order: after random.seed(s)
    this is the chunk list the reference draws after random.seed(s)."""
    cw, rw = int(cur_win_size), int(ret_win_size)
    if cw < 2 or rw < 0:
        raise ValueError(f'make_chunks: cur_win_size={cur_win_size} (>= 2), ret_win_size={ret_win_size} (>= 0)')
    chunks = []
    for i, nf in enumerate(num_frames):
        nf = int(nf)
        for st in range(0, nf, cw // 2):
            frames = list(range(st, min(st + cw, nf)))
            skip = rng.randint(st + cw, st + cw + rw)
            if skip < nf - 1:
                frames += [skip, skip + 1]
            chunks.append((i, frames))
    return chunks


def _parse_feats(feats: str) -> Tuple[bool, bool]:
    """(with the temporal pair, with the visual group).  '2d', '2d+temp', '2d+vis' or '2d+temp+vis' ('2d-temp-vis', the
    spelling of the model's `feats`, is taken too)."""
    names = re.split(r'[+-]', feats) if isinstance(feats, str) else None
    if names not in (['2d'], ['2d', 'temp'], ['2d', 'vis'], ['2d', 'temp', 'vis']):
        raise ValueError(f"DetectionStore: feats={feats!r}; '2d', '2d+temp', '2d+vis' or '2d+temp+vis' expected")
    return 'temp' in names, 'vis' in names


class DetectionStore:
    """The detections of a set of sequences, resident on `device` (None: host only, for `draw_chunks_host`).

    sequences   per sequence a mapping with `frame` [n] int, `track` [n] int (-1: false positive), `cat` [n] int
                (1-based), `box` [n, 4] x1 y1 x2 y2 (float64 accepted: the flip is computed in it, as the reference computes it
                in Python floats), `score` [n], the image `width` and `num_frames`.
    ncategories one-hot width;  feats '2d', '2d+temp', '2d+vis' or '2d+temp+vis';  mean, std: [F] with F = ncategories + 5 (+ 2)
                (+ 128), the reference's values for the detector at hand (kitti_mot.py:155-177; the library carries no presets).
                With 'vis' (`store.vis`) every sequence also carries the image `height`, and the store keeps what the visual head
                needs per row: `box` float32 [n, 2, 4] (the plain and the mirrored box: the flip in float64 on the raw box, then
                narrowed, as for `stat`) and `im_hw` float32 [nseq, 2].  A draw then leaves the last 128 columns of X to
                `DrawnChunks.attach_vis` (module docstring of trackmpnn_amd.frames for the images).

    Host tables (numpy; the device copies carry the same names with `_d`): the detections sorted stably by (sequence, frame),
    `frame`, `track` int32 [n], `stat` float32 [n, 2, Fs] (the standardised static row of the plain / the flipped box),
    `seq_base` int32 [nseq + 1] and `first` int32 [frames + 1] (detections of frame f of sequence s:
    first[seq_base[s] + f] .. first[seq_base[s] + f + 1]), `table` float32 [fr_range, 2]."""

    def __init__(self, sequences, ncategories: int, feats, mean, std, fr_range: int = 30, device='cuda:0'):
        self.temp, self.vis = _parse_feats(feats)
        self.ncat, self.fr_range = int(ncategories), int(fr_range)
        if self.ncat < 1 or self.fr_range < 1:
            raise ValueError(f'DetectionStore: ncategories={ncategories}, fr_range={fr_range}')
        self.Fs = self.ncat + 5
        self.Fv = self.Fs + (2 if self.temp else 0)                       # columns a draw writes
        self.F = self.Fv + (VIS_COLS if self.vis else 0)
        mean, std = np.asarray(mean, dtype=np.float32).ravel(), np.asarray(std, dtype=np.float32).ravel()
        if mean.size != self.F or std.size != self.F:
            raise ValueError(f'DetectionStore: mean / std of length {mean.size} / {std.size} for {self.F} feature columns '
                             f'({self.ncat} categories + 5{" + 2" if self.temp else ""}{" + 128 vis" if self.vis else ""})')
        if not (np.isfinite(mean).all() and np.isfinite(std).all() and (std != 0).all()):
            raise ValueError('DetectionStore: mean / std must be finite and std non-zero')
        sequences = list(sequences)
        if not sequences:
            raise ValueError('DetectionStore: no sequences')
        nf = np.zeros(len(sequences), np.int64)
        frames, tracks, stats, firsts, boxes = [], [], [], [], []
        im_hw = np.zeros((len(sequences), 2), np.float32)
        eye = np.eye(self.ncat, dtype=np.float32)
        m, s = mean[None, :self.Fs], std[None, :self.Fs]
        for i, sq in enumerate(sequences):
            nf[i] = int(sq['num_frames'])
            fr = np.asarray(sq['frame']).ravel()
            n = fr.size
            tr, cat = np.asarray(sq['track']).ravel(), np.asarray(sq['cat']).ravel()
            box = np.asarray(sq['box'], dtype=np.float64).reshape(-1, 4)
            score = np.asarray(sq['score'], dtype=np.float64).ravel()
            width = sq['width']
            if self.vis:
                if 'height' not in sq:
                    raise ValueError(f"DetectionStore: sequence {i}: 'vis' features need the image `height` next to `width`")
                im_hw[i] = (sq['height'], width)
                if not (np.isfinite(im_hw[i]).all() and (im_hw[i] > 0).all()):
                    raise ValueError(f'DetectionStore: sequence {i}: height, width must be finite and positive')
            if nf[i] < 1 or nf[i] >= 2 ** 24:
                raise ValueError(f'DetectionStore: sequence {i}: num_frames={nf[i]} (1 .. 2^24 - 1)')
            if not (tr.size == cat.size == score.size == box.shape[0] == n):
                raise ValueError(f'DetectionStore: sequence {i}: frame, track, cat, box, score differ in length')
            for a, nm in ((fr, 'frame'), (tr, 'track'), (cat, 'cat')):
                if n and not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f'DetectionStore: sequence {i}: {nm} must be integers, got {a.dtype}')
            if n and (fr.min() < 0 or fr.max() >= nf[i]):
                raise ValueError(f'DetectionStore: sequence {i}: a frame outside [0, num_frames = {nf[i]})')
            if n and (cat.min() < 1 or cat.max() > self.ncat):
                raise ValueError(f'DetectionStore: sequence {i}: a cat outside 1 .. {self.ncat}')
            if n and (tr.min() < -1 or tr.max() >= 2 ** 31):
                raise ValueError(f'DetectionStore: sequence {i}: a track id outside -1 .. 2^31 - 1')
            if not (np.isfinite(box).all() and np.isfinite(score).all()):
                raise ValueError(f'DetectionStore: sequence {i}: a box or score is not finite')
            order = np.argsort(fr, kind='stable')                 # (load order is kept within a frame)
            fr, tr, cat, box, score = fr[order], tr[order], cat[order], box[order], score[order]
            # the flipped box: Python-float arithmetic on the raw box (kitti_mot.py:350-353), then float32 like the plain one
            fbox = box.copy()
            fbox[:, 0] = width - box[:, 2] - 1
            fbox[:, 2] = width - box[:, 0] - 1
            st = np.empty((n, 2, self.Fs), np.float32)
            for v, bx in enumerate((box, fbox)):
                b32, s32 = bx.astype(np.float32), score.astype(np.float32)
                two_d = np.stack((s32, (b32[:, 0] + b32[:, 2]) / 2.0, (b32[:, 1] + b32[:, 3]) / 2.0, b32[:, 2] - b32[:, 0],
                                  b32[:, 3] - b32[:, 1]), axis=1).astype(np.float32)
                st[:, v] = (np.concatenate((eye[cat.astype(np.int64) - 1].reshape(n, self.ncat), two_d), axis=1) - m) / s
            if self.vis:
                boxes.append(np.stack((box.astype(np.float32), fbox.astype(np.float32)), axis=1))
            frames.append(fr.astype(np.int32))
            tracks.append(tr.astype(np.int32))
            stats.append(st)
            firsts.append(np.searchsorted(fr, np.arange(nf[i])))
        self.num_frames = nf
        self.nseq = len(sequences)
        self.seq_base = np.concatenate([[0], np.cumsum(nf)])
        self.frame, self.track, self.stat = np.concatenate(frames), np.concatenate(tracks), np.concatenate(stats)
        self.ndets = int(self.frame.size)
        base = np.concatenate([[0], np.cumsum([f.size for f in frames])])
        self.first = np.concatenate([f + b for f, b in zip(firsts, base[:-1])] + [[self.ndets]])
        if self.seq_base[-1] >= 2 ** 31 - 1 or self.ndets >= 2 ** 31 - 1:
            raise ValueError('DetectionStore: frames and detections must fit in int32')
        self.seq_base, self.first = self.seq_base.astype(np.int32), self.first.astype(np.int32)
        # the temporal pair of t mod fr_range (kitti_mot.py:414-420 on a float32 column), standardised
        a = np.mod(np.arange(self.fr_range, dtype=np.float32)[:, None], self.fr_range) * np.pi / self.fr_range
        pair = np.concatenate((np.sin(a), np.cos(a)), axis=1).astype(np.float32)
        self.table = ((pair - mean[None, self.Fs:self.Fv]) / std[None, self.Fs:self.Fv]).astype(np.float32) if self.temp else pair
        self.box = np.ascontiguousarray(np.concatenate(boxes)) if self.vis else None
        self.im_hw = im_hw if self.vis else None
        self.device = None
        if device is not None:
            dev = torch.device(device)
            if dev.type != 'cuda':
                raise RuntimeError('DetectionStore: the device draw runs on the MI355X HIP kernels only; pass a cuda device, or '
                                   'device=None for a host-only store (draw_chunks_host)')
            if dev.index is None:
                dev = torch.device('cuda', torch.cuda.current_device())
            self.device = dev
            # one upload: the int32 tables in one buffer, the float32 tables in another
            ints = [self.seq_base, self.first, self.track]
            flts = [self.stat.ravel(), self.table.ravel()]
            if self.vis:                                          # (box first: 16-byte aligned in the buffer, then im_hw: 8)
                flts = [self.box.ravel(), self.im_hw.ravel()] + flts
            ibuf, fbuf = _to_device(np.concatenate(ints), dev), _to_device(np.concatenate(flts), dev)
            io, fo = np.cumsum([0] + [a.size for a in ints]), np.cumsum([0] + [a.size for a in flts])
            self.seq_base_d, self.first_d, self.track_d = (ibuf[io[k]:io[k + 1]] for k in range(3))
            self.stat_d, self.table_d = (fbuf[fo[k]:fo[k + 1]] for k in range(len(flts) - 2, len(flts)))
            self.box_d, self.im_hw_d = (fbuf[fo[0]:fo[1]], fbuf[fo[1]:fo[2]]) if self.vis else (None, None)


@dataclass
class FramePlan:
    """The images a draw needs (`ChunkSampler.frame_plan`; host arrays, known before any launch)."""
    frames: np.ndarray      # int64 [T, 3]: (sequence, frame, mirrored 0 / 1), unique rows in order of first use
    slot: np.ndarray        # int32 [B, L]: the row of `frames` of listed frame k of drawn chunk b; -1 in the padding


@dataclass
class HostDraw:
    """What `draw_chunks_host` returns (numpy).  `kept` marks, over the n_max rows of the drawn chunks before dropout (chunks in
    the order of `indices`, rows in output order), the rows that survived: X and y hold exactly those.  The fields from `box`
    on are those of a store with 'vis' (None otherwise), one entry per kept row; X's last 128 columns are then zero until
    `attach_vis`."""
    X: np.ndarray           # float32 [ND, F]
    y: np.ndarray           # int64 [ND, 2]
    offsets: np.ndarray     # int64 [B + 1]
    flags: np.ndarray       # uint8 [B]
    kept: np.ndarray        # bool [n_max]
    n_max: int
    box: Optional[np.ndarray] = None        # float32 [ND, 4]: the box the row's features were made from (mirrored iff flipped)
    im_hw: Optional[np.ndarray] = None      # float32 [ND, 2]
    map_of: Optional[np.ndarray] = None     # int32 [ND]: plan.slot[chunk, list index of the row's frame]
    track: Optional[np.ndarray] = None      # int32 [ND] = y[:, 1]
    plan: Optional[FramePlan] = None

    def attach_vis(self, maps, mean, std, input_hw, down_ratio, embed_loss='identity') -> np.ndarray:
        """The host definition of DrawnChunks.attach_vis: vis_head_host on the drawn rows, its rows written into the last 128
        columns of X (in float32); returns the per-chunk identity loss [B] in the dtype of `maps`.  embed_loss='embedding' (or
        an object with delta_var / delta_dist, such as an EmbeddingLoss): embedding_loss_host over the gathered logits instead."""
        if self.plan is None:
            raise ValueError("HostDraw.attach_vis: the store was built without 'vis'")
        logits, rows, loss, _ = vis_head_host(maps, self.box, self.map_of, self.im_hw, self.track, self.offsets,
                                              np.asarray(mean).ravel()[-VIS_COLS:], np.asarray(std).ravel()[-VIS_COLS:], input_hw, down_ratio)
        self.X[:, self.X.shape[1] - VIS_COLS:] = rows
        if isinstance(embed_loss, str) and embed_loss == 'identity':
            return loss
        if isinstance(embed_loss, str) and embed_loss != 'embedding':
            raise ValueError(f"HostDraw.attach_vis: embed_loss={embed_loss!r}; 'identity', 'embedding' or an EmbeddingLoss expected")
        deltas = (0.5, 10.0) if isinstance(embed_loss, str) else (embed_loss.delta_var, embed_loss.delta_dist)
        return embedding_loss_host(logits, self.track, self.offsets, *deltas)[0]


@dataclass
class DrawnChunks:
    """What `ChunkSampler.draw` returns, all on the device.  Chunk b of the draw is rows offsets[b] .. offsets[b + 1]; only the
    device knows the kept total offsets[B], so X and y have n_max rows (the chunks' sizes before dropout) and the rows from
    offsets[B] on are unspecified.

    With a 'vis' store the draw also carries the visual head's arguments per row (`box`, `im_hw`, `map_of`, `track`, all
    [n_max, ...] with the same unspecified tail) and the frame `plan`; columns [0, F - 128) of X are those of the same store
    without 'vis' and the last 128 are left unwritten until `attach_vis`.  VisHead serves the unspecified rows safely: they
    belong to no chunk (no loss, no gradient), and every centre and map index is clamped before anything is read
    (csrc/vishead.hip), so they produce finite or garbage feature rows that nothing reads -- never a fault."""
    X: torch.Tensor         # float32 [n_max, F]
    y: torch.Tensor         # int64 [n_max, 2] = [t', track id]
    offsets: torch.Tensor   # int64 [B + 1]
    flags: torch.Tensor     # uint8 [B]: bit 0 = time reversed, bit 1 = flipped (bit 7: refused by the kernel's table checks)
    n_max: int
    box: Optional[torch.Tensor] = None      # float32 [n_max, 4]: the box the row's features were made from (mirrored iff flipped)
    im_hw: Optional[torch.Tensor] = None    # float32 [n_max, 2]
    map_of: Optional[torch.Tensor] = None   # int32 [n_max]: plan.slot[chunk, list index of the row's frame]
    track: Optional[torch.Tensor] = None    # int32 [n_max] = y[:, 1]
    plan: Optional[FramePlan] = None

    def attach_vis(self, head, maps, loss: bool = True, embed_loss='identity'):
        """The visual head on the draw: maps [T, 128, Hm, Wm] = the CNN's answer to the images of `plan` (FrameStore.gather).  The
        standardised softmax rows go into the last 128 columns of X; with `loss` the per-chunk identity loss [B] is returned,
        differentiable wrt `maps` (VisHead.forward), otherwise None (VisHead.rows).  embed_loss: which loss that is --
        'identity', 'embedding' or an EmbeddingLoss (VisHead.forward's `loss`).  No wait for the device."""
        if self.plan is None:
            raise ValueError("DrawnChunks.attach_vis: the store was built without 'vis'")
        col = int(self.X.shape[1]) - VIS_COLS
        if not loss:
            head.rows(maps, self.box, self.map_of, self.im_hw, out=self.X, col=col)
            return None
        return head.forward(maps, self.box, self.map_of, self.im_hw, self.track, self.offsets, out=self.X, col=col, loss=embed_loss)[1]

    def batch(self):
        """The TrainBatch of the drawn chunks (build_train_batch_device; its two host reads are the only waits).  The maximum of
        `flags` rides along with the first read: a chunk the kernels refused (bit 7) raises RuntimeError here."""
        if self.n_max == 0:                               # (nothing was there to draw: known without asking the device)
            raise AllChunksSkipped('DrawnChunks.batch: every chunk is skipped (the drawn chunks hold no detections)')
        return build_train_batch_device(self.y, self.y.device, offsets=self.offsets, padded=True, draw_flags=self.flags)

    def features(self, batch) -> torch.Tensor:
        """The stacked features train_chunks(model, batch, X) takes: the rows the batch was built from."""
        return self.X[:batch.n_feat]


class ChunkSampler:
    """Seeded draws of augmented chunks from a DetectionStore (module docstring).

    chunks              [(sequence index, [frames])], e.g. from make_chunks; uploaded once as one table (sequence, frame list
                        padded to the longest list, size before dropout).  A chunk above TB_MAX_DETS detections is refused.
    seed                key of every random number of this sampler (0 .. 2^64 - 1)
    random_transforms   False: a draw is the plain chunk, no random numbers involved
    dropout, p_reverse, p_flip   the reference's 0.2, 0.5, 0.5"""

    def __init__(self, store: DetectionStore, chunks, seed: int, random_transforms: bool = True, dropout: float = 0.2,
                 p_reverse: float = 0.5, p_flip: float = 0.5):
        self.store = store
        self.seed = int(seed)
        self._key = _split64(seed, 'seed')
        self.random_transforms = bool(random_transforms)
        for p, nm in ((dropout, 'dropout'), (p_reverse, 'p_reverse'), (p_flip, 'p_flip')):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f'ChunkSampler: {nm}={p} is not a probability')
        self.dropout, self.p_reverse, self.p_flip = float(dropout), float(p_reverse), float(p_flip)
        chunks = [(int(s), [int(f) for f in fr]) for s, fr in chunks]
        if not chunks:
            raise ValueError('ChunkSampler: no chunks')
        self.nchunks = len(chunks)
        self.L = L = max(len(fr) for _, fr in chunks)
        if L > CD_MAX_FRAMES:
            raise ValueError(f'ChunkSampler: a chunk lists {L} frames, more than {CD_MAX_FRAMES}')
        tab = np.full((self.nchunks, 4 + L), -1, np.int32)
        tab[:, 3] = 0
        rows, t_rows, k_rows = [], [], []
        for ci, (s, fr) in enumerate(chunks):
            if not 0 <= s < store.nseq:
                raise ValueError(f'ChunkSampler: chunk {ci} names sequence {s} of {store.nseq}')
            if not fr:
                raise ValueError(f'ChunkSampler: chunk {ci} lists no frame')
            f = np.asarray(fr, np.int64)
            if f.min() < 0 or f.max() >= store.num_frames[s]:
                raise ValueError(f'ChunkSampler: chunk {ci} names frame {int(f.max() if f.min() >= 0 else f.min())} of sequence '
                                 f'{s}, which has num_frames = {int(store.num_frames[s])}')
            if (f[-1] - f + f[0]).min() < 0:
                raise ValueError(f'ChunkSampler: chunk {ci}: time reversal about the ends of its list ({fr[0]}, {fr[-1]}) gives a '
                                 'negative timestep')
            g = store.seq_base[s] + f
            lo, hi = store.first[g].astype(np.int64), store.first[g + 1].astype(np.int64)
            r = np.repeat(lo - np.concatenate([[0], np.cumsum(hi - lo)[:-1]]), hi - lo) + np.arange(int((hi - lo).sum()))
            if r.size > TB_MAX_DETS:
                raise ValueError(f'ChunkSampler: chunk {ci} holds {r.size} detections, more than TB_MAX_DETS = {TB_MAX_DETS} '
                                 '(the device builder\'s limit per chunk)')
            tab[ci, :3] = (s, len(fr), r.size)
            tab[ci, 4:4 + len(fr)] = f
            rows.append(r)
            t_rows.append(np.repeat(f, hi - lo))
            k_rows.append(np.repeat(np.arange(f.size), hi - lo))
        self.table = tab
        self.size = tab[:, 2].astype(np.int64)                                   # detections before dropout
        self._ptr = np.concatenate([[0], np.cumsum(self.size)])
        self._rows = np.concatenate(rows).astype(np.int64)                       # store row of every chunk row before dropout
        self._t_row = np.concatenate(t_rows).astype(np.int64)                    # frame of every such row
        self._k_row = np.concatenate(k_rows).astype(np.int64)                    # its position in the chunk's list
        self._ends = np.asarray([(fr[0], fr[-1]) for _, fr in chunks], np.int64)
        self.table_d = _to_device(tab.ravel(), store.device) if store.device is not None else None

    def __len__(self) -> int:
        return self.nchunks

    def epoch_order(self, epoch: int) -> np.ndarray:
        """A seeded permutation of the chunk indices (the reference's DataLoader(shuffle=True)): chunk i is ranked by the first
        two Philox words of counter (i, 0xffffffff, epoch low, epoch high) under the sampler's key.  Host side."""
        lo, hi = _split64(epoch, 'epoch')
        ctr = np.zeros((self.nchunks, 4), np.uint64)
        ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(self.nchunks), _ORDER_STREAM, lo, hi
        w = philox4x32(ctr, np.asarray(self._key, np.uint64)).astype(np.uint64)
        return np.argsort((w[:, 0] << np.uint64(32)) | w[:, 1], kind='stable').astype(np.int64)

    def _indices(self, indices) -> np.ndarray:
        idx = np.asarray(indices)
        if idx.ndim != 1 or idx.size == 0 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError('ChunkSampler: indices must be a non-empty 1-d sequence of integers')
        if idx.min() < 0 or idx.max() >= self.nchunks:
            raise IndexError(f'ChunkSampler: index {int(idx.max() if idx.min() >= 0 else idx.min())} for {self.nchunks} chunks')
        return idx.astype(np.int64)

    def _chunk_flags(self, idx: np.ndarray, slo: int, shi: int) -> np.ndarray:
        """The two decisions of every drawn chunk (Philox block j = 0) as uint8 [B]."""
        flags = np.zeros(idx.size, np.uint8)
        if self.random_transforms:
            ctr = np.zeros((idx.size, 4), np.uint64)
            ctr[:, 1], ctr[:, 2], ctr[:, 3] = idx, slo, shi
            u = _uniform(philox4x32(ctr, np.asarray(self._key, np.uint64)))
            flags |= np.where(u[:, 0] < np.float32(self.p_reverse), FLAG_REVERSED, 0).astype(np.uint8)
            flags |= np.where(u[:, 1] < np.float32(self.p_flip), FLAG_FLIPPED, 0).astype(np.uint8)
        return flags

    def frame_plan(self, indices, step: int) -> FramePlan:
        """The images draw(indices, step) needs, on the host and before any launch: one row (sequence, frame, mirrored) per
        distinct image, in order of first use (drawn chunks in the order of `indices`, then list order within a chunk), and per
        drawn chunk the row of each listed frame.  The image of a detection is that of its LISTED frame (time reversal relabels
        t' only, kitti_mot.py:506-524), mirrored iff its chunk is flipped: the chunk's flip decision, computed here from Philox
        block j = 0 exactly as draw_host computes `flags`.  Two drawn chunks that list the same frame of the same sequence with
        the same decision share a row."""
        idx = self._indices(indices)
        slo, shi = _split64(step, 'step')
        flip = ((self._chunk_flags(idx, slo, shi) & FLAG_FLIPPED) != 0).astype(np.int64)
        tab = self.table[idx].astype(np.int64)
        valid = np.arange(self.L)[None, :] < tab[:, 1:2]
        g = (self.store.seq_base.astype(np.int64)[tab[:, 0]][:, None] + tab[:, 4:]) * 2 + flip[:, None]     # (global frame, flip)
        keys = g[valid]                                                          # (chunk-major, then list order)
        uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
        order = np.argsort(first, kind='stable')                                 # unique keys by first use
        rank = np.empty(order.size, np.int64)
        rank[order] = np.arange(order.size)
        slot = np.full((idx.size, self.L), -1, np.int32)
        slot[valid] = rank[inv.ravel()]
        at = first[order]
        seq = np.broadcast_to(tab[:, 0:1], g.shape)[valid][at]
        frames = np.stack([seq, tab[:, 4:][valid][at], np.broadcast_to(flip[:, None], g.shape)[valid][at]], 1).astype(np.int64)
        return FramePlan(frames, slot)

    def draw_host(self, indices, step: int) -> HostDraw:
        """The host definition of draw(indices, step), in numpy (module docstring)."""
        st, idx = self.store, self._indices(indices)
        slo, shi = _split64(step, 'step')
        B = idx.size
        n_b = self.size[idx]
        n_max = int(n_b.sum())
        start = np.concatenate([[0], np.cumsum(n_b)[:-1]])
        b_of = np.repeat(np.arange(B), n_b)
        r = np.arange(n_max) - start[b_of]                                      # row of the chunk, output order before dropout
        src = self._ptr[idx][b_of] + r
        det, t = self._rows[src], self._t_row[src]
        flags = self._chunk_flags(idx, slo, shi)
        kept = np.ones(n_max, bool)
        if self.random_transforms:
            key = np.asarray(self._key, np.uint64)
            ctr = np.zeros((n_max, 4), np.uint64)
            ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = 1 + r // 4, idx[b_of], slo, shi
            u = _uniform(philox4x32(ctr, key)[np.arange(n_max), r % 4])
            kept = ~(u < np.float32(self.dropout))
        rev = (flags[b_of] & FLAG_REVERSED) != 0
        flip = ((flags[b_of] & FLAG_FLIPPED) != 0).astype(np.int64)
        lo, hi = self._ends[idx, 0][b_of], self._ends[idx, 1][b_of]
        t = np.where(rev, hi - t + lo, t)
        X = np.zeros((n_max, st.F), np.float32) if st.vis else np.empty((n_max, st.F), np.float32)
        X[:, :st.Fs] = st.stat[det, flip]
        if st.temp:
            X[:, st.Fs:st.Fv] = st.table[np.mod(t, st.fr_range)]
        y = np.stack([t, st.track[det].astype(np.int64)], 1)
        offsets = np.zeros(B + 1, np.int64)
        offsets[1:] = np.cumsum(np.bincount(b_of[kept], minlength=B))
        hd = HostDraw(X[kept], y[kept], offsets, flags, kept, n_max)
        if st.vis:
            hd.plan = self.frame_plan(idx, step)
            hd.box, hd.im_hw = st.box[det, flip][kept], st.im_hw[self.table[idx, 0]][b_of][kept]
            hd.map_of = hd.plan.slot[b_of, self._k_row[src]][kept]
            hd.track = st.track[det][kept]
        return hd

    def draw(self, indices, step: int) -> DrawnChunks:
        """B = len(indices) chunks drawn on the device (csrc/chunkdraw.hip): three launches (count, the scan of the counts into
        offsets, fill), no wait for the device.  Equal to draw_host(indices, step) in X[:ND], y[:ND], offsets and flags.
        With a 'vis' store one more launch (tmpnn_chunk_draw_vis) writes box, im_hw, map_of and track of every kept row, equal
        to draw_host's; the frame plan is computed on the host first and its `slot` is the draw's one more small upload.  The
        last 128 columns of X are left unwritten (DrawnChunks.attach_vis fills them).
        The kernels check every table entry they index by and draw a chunk that fails as empty with bit 7 of its flag set
        (reachable only if the device tables were overwritten: the host validated them); `DrawnChunks.batch()` raises on it,
        a caller that consumes X / y some other way must look at `flags` itself."""
        st = self.store
        if st.device is None:
            raise RuntimeError('ChunkSampler.draw runs on the MI355X HIP kernels only (no CPU path): build the DetectionStore on '
                               'a cuda device (draw_host is the host definition)')
        idx = self._indices(indices)
        slo, shi = _split64(step, 'step')
        dev = st.device
        B, n_max = int(idx.size), int(self.size[idx].sum())
        if n_max >= 2 ** 31:
            raise ValueError(f'ChunkSampler.draw: {n_max} rows in one draw (2^31 - 1 at the most); draw smaller batches')
        idx_d = _to_device(idx.astype(np.int32), dev)
        plan = self.frame_plan(idx, step) if st.vis else None
        X = torch.empty((n_max, st.F), dtype=torch.float32, device=dev)
        y = torch.empty((n_max, 2), dtype=torch.int64, device=dev)
        offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        flags = torch.empty(B, dtype=torch.uint8, device=dev)
        d = _lib.CChunkDraw()
        d.B, d.nchunks, d.L, d.nseq, d.F, d.Fs, d.fr_range = B, self.nchunks, self.L, st.nseq, st.F, st.Fs, st.fr_range
        d.F, d.ldx = st.Fv, st.F                                                 # (a 'vis' store: the fill leaves the last 128 columns)
        d.transforms = 1 if self.random_transforms else 0
        d.ndets, d.nframes, d.n_max = st.ndets, int(st.seq_base[-1]), n_max
        d.seed, d.step = self.seed, int(step)
        d.p_drop, d.p_reverse, d.p_flip = self.dropout, self.p_reverse, self.p_flip
        d.indices, d.chunks = idx_d.data_ptr(), self.table_d.data_ptr()
        d.seq_base, d.first, d.track = st.seq_base_d.data_ptr(), st.first_d.data_ptr(), st.track_d.data_ptr()
        d.stat, d.table = st.stat_d.data_ptr(), st.table_d.data_ptr()
        d.count, d.flags, d.offsets = count.data_ptr(), flags.data_ptr(), offsets.data_ptr()
        d.X, d.y = X.data_ptr(), y.data_ptr()
        stream = _lib.raw_stream(dev)
        _lib.call('tmpnn_chunk_draw_count', C.byref(d), stream)
        _lib.call('tmpnn_chunk_draw_fill', C.byref(d), stream)
        if not st.vis:
            return DrawnChunks(X, y, offsets, flags, n_max)
        slot_d = _to_device(plan.slot.ravel(), dev)
        fl = torch.empty((n_max, 6), dtype=torch.float32, device=dev)             # box [n_max, 4] | im_hw [n_max, 2]
        it = torch.empty((2, n_max), dtype=torch.int32, device=dev)               # map_of | track
        box, im_hw = fl.view(-1)[:4 * n_max].view(n_max, 4), fl.view(-1)[4 * n_max:].view(n_max, 2)
        v = _lib.CChunkDrawVis(st.box_d.data_ptr(), st.im_hw_d.data_ptr(), slot_d.data_ptr(), box.data_ptr(), im_hw.data_ptr(),
                               it[0].data_ptr(), it[1].data_ptr())
        _lib.call('tmpnn_chunk_draw_vis', C.byref(d), C.byref(v), stream)
        return DrawnChunks(X, y, offsets, flags, n_max, box, im_hw, it[0], it[1], plan)


def draw_chunks_host(store: DetectionStore, chunks, indices, step: int, seed: int, random_transforms: bool = True,
                     dropout: float = 0.2, p_reverse: float = 0.5, p_flip: float = 0.5) -> HostDraw:
    """The host definition of a draw, in numpy: what ChunkSampler(store, chunks, seed, ...).draw(indices, step) writes on the
    device, from the same inputs (to the device draw what build_train_batch is to build_train_batch_device).  `store` may be a
    host-only DetectionStore (device=None).  The decisions are Philox draws with the reference's probabilities: the same
    distribution as the reference's `random.random()`, not its stream (module docstring)."""
    host = store
    if store.device is not None:                      # (the sampler's table is not uploaded for a host draw)
        host = object.__new__(DetectionStore)
        host.__dict__.update(store.__dict__)
        host.device = None
    return ChunkSampler(host, chunks, seed, random_transforms, dropout, p_reverse, p_flip).draw_host(indices, step)
