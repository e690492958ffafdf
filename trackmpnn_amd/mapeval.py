"""Validation mAP: the mean average precision of the detections that were given a track (reference utils/metrics.py:93-229,
train.py:272-273,286).

    map_iou_host        the float64 "+1" IoU matrix of two float32 box lists (utils/misc.py:4-22)
    map_best_host       per detection the first GT box of largest IoU, -1 below 0.5: what the device's tmpnn_map_best must equal
    map_host            the rule, in numpy: the sequences and their tracks in, mAP and the per-class figures out.  It is the
                        DEFINITION the device must equal (counts exactly, ap and map bit for bit).
    MapStore            what does not change between epochs, packed over the sequences: GT rows by (class, sequence, frame), the
                        groups of one image and class, per class the detections by descending score, per GT row its claimants
    MapEvaluator        the store on the device + `evaluate(tracks)` (two launches of tmpnn_map_eval, csrc/mapeval.hip) +
                        `read()` (the one device -> host copy)
    synth_map_sequence  synth_mot_sequence + classes, scores, duplicates, a class without GT, frames without GT

The rule keeps the reference's quirks: a sequence left out (tracks None) brings neither detections nor GT; only detections with
a track take part, every GT row counts; an image is a (sequence, frame) with at least one GT row and a detection in any other
frame is ignored (it is NOT a false positive); classes are those of the GT that takes part; within an image and class the kept
detections are walked in arrival order, each takes the FIRST GT box of largest IoU (a NaN counts as the largest), and is a true
positive iff that IoU is >= 0.5 and the box was not taken before -- the second-best box is never tried.  Where the reference
leaves the outcome open it is pinned: ties in score keep the natural order (sequence, arrival index; the reference's argsort is
unstable), AP is added one term at a time in ascending rank (np.sum is pairwise), no GT at all gives NaN.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .evalstore import _boxes, _ints, cat, cuda_device
from .moteval import synth_mot_sequence

FLAG_STORE = 1
RECORD_WORDS = 5               # struct tmpnn_map_record: ap (double), annotations, kept, true_positives, flag (int64)
IOU_THRESHOLD = 0.5


def map_iou_host(det_box, gt_box) -> np.ndarray:
    """[len(det_box), len(gt_box)] float64: intersection over union of x1 y1 x2 y2 boxes with the reference's "+1" on every
    width and height, computed in float64 from the float32 coordinates (metrics.py:171,180)."""
    a, b = _boxes(det_box, 'det_box').astype(np.float64), _boxes(gt_box, 'gt_box').astype(np.float64)
    x11, y11, x12, y12 = (a[:, i:i + 1] for i in range(4))
    x21, y21, x22, y22 = (b[:, i][None, :] for i in range(4))
    with np.errstate(invalid='ignore', divide='ignore'):
        w = np.maximum((np.minimum(x12, x22) - np.maximum(x11, x21)) + 1.0, 0.0)
        h = np.maximum((np.minimum(y12, y22) - np.maximum(y11, y21)) + 1.0, 0.0)
        inter = w * h
        area_a = ((x12 - x11) + 1.0) * ((y12 - y11) + 1.0)
        area_b = ((x22 - x21) + 1.0) * ((y22 - y21) + 1.0)
        return inter / ((area_a + area_b) - inter)


def map_best_host(det_box, gt_box) -> np.ndarray:
    """int64 [len(det_box)]: per detection the index of the first GT box of largest IoU (np.argmax: a NaN counts as the
    largest), -1 where that IoU is below 0.5 or NaN, or where there is no GT box (metrics.py:180-184)."""
    iou = map_iou_host(det_box, gt_box)
    if iou.shape[1] == 0:
        return np.full(iou.shape[0], -1, np.int64)
    j = np.argmax(iou, axis=1)
    return np.where(iou[np.arange(iou.shape[0]), j] >= IOU_THRESHOLD, j, -1).astype(np.int64)


def _average_precision(tp: np.ndarray, n_gt: int) -> float:
    """tp: 0 / 1 per kept detection in rank order.  Recall tp_k / N, precision tp_k / k, the envelope, and the area added one
    term at a time in ascending k (metrics.py:64-90,206-214)."""
    n = tp.shape[0]
    if n == 0:
        return 0.0
    tpk = np.cumsum(tp.astype(np.int64))
    rec = tpk / float(n_gt)
    prec = tpk / np.arange(1, n + 1, dtype=np.float64)
    env = np.maximum.accumulate(prec[::-1])[::-1]
    ap, prev = 0.0, 0.0
    for k in range(n):
        if rec[k] != prev:
            ap += (rec[k] - prev) * env[k]
            prev = rec[k]
    return float(ap)


def _mean(aps: Sequence[float]) -> float:
    tot = 0.0
    for a in aps:                                                 # ascending class
        tot += a
    return tot / len(aps) if len(aps) else float('nan')


def _fields(q: Dict, s: int):
    """The arrays of one sequence, checked: (det_frame, det_cat, det_score, det_box, gt_frame, gt_cat, gt_box)."""
    det_frame, gt_frame = _ints(q['det_frame'], 'det_frame'), _ints(q['gt_frame'], 'gt_frame')
    nd, ng = det_frame.shape[0], gt_frame.shape[0]
    det_cat, gt_cat = _ints(q['det_cat'], 'det_cat', nd), _ints(q['gt_cat'], 'gt_cat', ng)
    sc = q['det_score']
    if isinstance(sc, torch.Tensor):
        sc = sc.detach().cpu().numpy()
    score = np.asarray(sc, dtype=np.float32).reshape(-1)          # (train.py:265: the reference scores the float32 rows)
    db, gb = _boxes(q['det_box'], 'det_box'), _boxes(q['gt_box'], 'gt_box')
    if db.shape[0] != nd or gb.shape[0] != ng or score.shape[0] != nd:
        raise ValueError(f'mAP: sequence {s}: one box and one score per detection, one box per GT row expected')
    if not (np.isfinite(db).all() and np.isfinite(gb).all() and np.isfinite(score).all()):
        raise ValueError(f'mAP: sequence {s}: boxes and scores must be finite')
    return det_frame, det_cat, score, db, gt_frame, gt_cat, gb


def map_host(sequences: Sequence[Dict], tracks: Sequence) -> Dict:
    """The validation mAP of `tracks` (per sequence y_out[:, 1] in arrival order, None: the sequence takes no part).
    sequences: dicts with det_frame, det_cat, det_score, det_box, gt_frame, gt_cat, gt_box.  Returns {'map', 'classes',
    'ap', 'annotations', 'kept', 'true_positives'}: the lists run over the classes of the GT that takes part, ascending."""
    if len(tracks) != len(sequences):
        raise ValueError(f'map_host: {len(tracks)} track arrays for {len(sequences)} sequences')
    data = []
    for s, (q, tr) in enumerate(zip(sequences, tracks)):
        if tr is None:
            continue
        f = _fields(q, s)
        data.append(f + (_ints(tr, f'map_host: sequence {s}: tracks', f[0].shape[0]),))
    classes = sorted(set(int(c) for f in data for c in f[5]))
    n_gt = {c: 0 for c in classes}
    scores: Dict[int, List[float]] = {c: [] for c in classes}
    tps: Dict[int, List[int]] = {c: [] for c in classes}
    for det_frame, det_cat, score, db, gt_frame, gt_cat, gb, tr in data:
        rows: Dict = {}                                           # (frame, class) -> GT rows in arrival order
        for g in range(gt_frame.shape[0]):
            rows.setdefault((int(gt_frame[g]), int(gt_cat[g])), []).append(g)
            n_gt[int(gt_cat[g])] += 1
        images = set(int(t) for t in gt_frame)
        taken = set()
        for i in np.where(tr >= 0)[0]:                            # arrival order
            t, c = int(det_frame[i]), int(det_cat[i])
            if t not in images or c not in scores:
                continue
            r = rows.get((t, c), [])
            j = int(map_best_host(db[i:i + 1], gb[r])[0])
            tp = j >= 0 and r[j] not in taken
            if tp:
                taken.add(r[j])
            scores[c].append(score[i])
            tps[c].append(int(tp))
    out = {'classes': classes, 'ap': [], 'annotations': [], 'kept': [], 'true_positives': []}
    for c in classes:
        sc, tp = np.asarray(scores[c], np.float32), np.asarray(tps[c], np.int64)
        order = np.argsort(-sc, kind='stable')
        out['ap'].append(_average_precision(tp[order], n_gt[c]))
        out['annotations'].append(n_gt[c])
        out['kept'].append(int(tp.shape[0]))
        out['true_positives'].append(int(tp.sum()))
    out['map'] = _mean(out['ap'])
    return out


def synth_map_sequence(seed: int, frames: int, classes: int = 3, ties: bool = False, p_dup: float = 0.12, p_alien: float = 0.04,
                       p_empty: float = 0.06, p_wrong: float = 0.04, **kw) -> Dict:
    """synth_mot_sequence(seed, frames, **kw) made into a detection problem: every GT row gets the class of its object
    (object index mod `classes`), every detection the class of the GT box of its frame it overlaps most (a random one where it
    overlaps none, and with p_wrong a wrong one); with p_dup a detection is followed by a jittered duplicate with a fresh track
    id (a second claimant of the same GT box); with p_alien per frame a detection of class `classes` + 4, which no GT row has;
    with p_empty a frame loses all its GT rows.  Scores are distinct (ties=False) or rounded to one decimal.  Detections stay
    sorted by frame.  Returns the dict of synth_mot_sequence plus det_cat, det_score, gt_cat."""
    from .moteval import mot_dist_host
    q = synth_mot_sequence(seed, frames, **kw)
    rng = np.random.default_rng([seed, 77])
    gt_cat = ((q['gt_track'] - 1) // 3) % classes
    empty = np.unique(q['gt_frame'])
    empty = empty[rng.random(empty.shape[0]) < p_empty]
    keep = ~np.isin(q['gt_frame'], empty)
    gt_frame, gt_track, gt_box, gt_cat = q['gt_frame'][keep], q['gt_track'][keep], q['gt_box'][keep], gt_cat[keep]
    frame, box, track, cat = list(q['det_frame']), list(q['det_box']), list(q['tracks']), []
    for i in range(len(frame)):
        g = np.where(q['gt_frame'] == frame[i])[0]
        c = int(rng.integers(classes))
        if g.size:
            d = mot_dist_host(q['det_box'][i:i + 1], q['gt_box'][g])[0]
            if np.isfinite(d).any():
                c = int(((q['gt_track'][g[int(np.nanargmin(d))]] - 1) // 3) % classes)
        if rng.random() < p_wrong:
            c = (c + 1) % classes
        cat.append(c)
    fresh = 1_000_000
    for i in range(len(frame)):
        if rng.random() < p_dup:
            frame.append(frame[i]); box.append(box[i] + rng.normal(0, 1, 4).astype(np.float32)); cat.append(cat[i])
            track.append(fresh if rng.random() >= 0.05 else -1)
            fresh += 1
    for t in np.unique(q['det_frame']):
        if rng.random() < p_alien:
            c, sz = rng.uniform(100, 900, 2), rng.uniform(30, 80, 2)
            frame.append(int(t)); box.append(np.concatenate([c - sz / 2, c + sz / 2]).astype(np.float32)); cat.append(classes + 4)
            track.append(fresh)
            fresh += 1
    frame, track, cat = np.asarray(frame, np.int64), np.asarray(track, np.int64), np.asarray(cat, np.int64)
    box = np.asarray(box, np.float32).reshape(-1, 4)
    o = np.argsort(frame, kind='stable')
    n = o.shape[0]
    score = np.round(rng.random(n), 1) if ties else (rng.permutation(n) + 1.0) / (n + 1.0)
    return {'det_frame': frame[o], 'det_box': box[o], 'tracks': track[o], 'det_cat': cat[o], 'det_score': score.astype(np.float32),
            'gt_frame': gt_frame, 'gt_track': gt_track, 'gt_box': gt_box, 'gt_cat': gt_cat}


class MapStore:
    """What the evaluator keeps of S sequences (dicts with det_frame, det_cat, det_score, det_box, gt_frame, gt_cat, gt_box;
    categories integers, boxes and scores finite, else ValueError).  GT rows sorted stably by (class, sequence, frame), so that
    the rows of a class, and inside them the rows of a GROUP (one sequence, frame and class), are ranges that keep the arrival
    order; detections in arrival order, packed over the sequences.  All host numpy arrays, as struct tmpnn_map_store names them:

        classes     the classes of the GT, ascending (class index c <-> classes[c])
        gt_box      float32 [n_gt, 4]   gt_seq int32 [n_gt]   cls_gt_off int32 [C + 1]   grp_off int32 [n_grp + 1]
        det_box     float32 [n_det, 4]  det_grp int32 [n_det] (-1: no GT row of that sequence, frame and class)
        det_base    int64 [S + 1]       the detections of sequence s are det_base[s] : det_base[s + 1]
        cls_off     int32 [C + 1], order int32 [n_live]: per class its detections in frames with GT rows, by descending
                    float32 score, ties by (sequence, arrival index)
        claim_off   int32 [n_gt + 1], claim_det int32 [n_claim]: after set_best(best), per GT row the detections whose best
                    row it is, in arrival order
    """

    def __init__(self, sequences: Sequence[Dict]):
        S = len(sequences)
        fields = [_fields(q, s) for s, q in enumerate(sequences)]
        self.S = S
        self.classes = sorted(set(int(c) for f in fields for c in f[5]))
        cls_index = {c: i for i, c in enumerate(self.classes)}
        self.C = len(self.classes)
        self.det_base = np.zeros(S + 1, np.int64)
        self.det_base[1:] = np.cumsum([f[0].shape[0] for f in fields])
        self.n_det = int(self.det_base[-1])
        g_seq = cat([np.full(f[4].shape[0], s) for s, f in enumerate(fields)], np.int64)
        g_frame = cat([f[4] for f in fields], np.int64)
        g_cls = cat([[cls_index[int(c)] for c in f[5]] for f in fields], np.int64)
        g_box = cat([f[6] for f in fields], np.float32, (4,)).reshape(-1, 4)
        self.n_gt = int(g_seq.shape[0])
        if max(self.n_gt, self.n_det) >= 2 ** 31 - 1:
            raise ValueError('MapStore: the store is indexed by int32')
        o = np.lexsort((g_frame, g_seq, g_cls))                   # (stable: rows of one key keep their arrival order)
        g_seq, g_frame, g_cls = g_seq[o], g_frame[o], g_cls[o]
        self.gt_box = np.ascontiguousarray(g_box[o])
        self.gt_seq = g_seq.astype(np.int32)
        self.gt_cls = g_cls.astype(np.int32)
        self.cls_gt_off = np.searchsorted(g_cls, np.arange(self.C + 1), side='left').astype(np.int32)
        new = np.ones(self.n_gt, bool)
        new[1:] = (g_cls[1:] != g_cls[:-1]) | (g_seq[1:] != g_seq[:-1]) | (g_frame[1:] != g_frame[:-1])
        starts = np.where(new)[0]
        self.n_grp = int(starts.shape[0])
        self.grp_off = np.concatenate([starts, [self.n_gt]]).astype(np.int32)
        group = {(int(g_seq[a]), int(g_frame[a]), int(g_cls[a])): i for i, a in enumerate(starts)}
        images = set((int(s), int(t)) for s, t in zip(g_seq, g_frame))
        det_grp = np.full(self.n_det, -1, np.int32)
        d_cls = np.full(self.n_det, -1, np.int64)                 # class index of a LIVE detection, else -1
        for s, f in enumerate(fields):
            base = int(self.det_base[s])
            for i in range(f[0].shape[0]):
                t, c = int(f[0][i]), cls_index.get(int(f[1][i]), -1)
                if c >= 0 and (s, t) in images:
                    d_cls[base + i] = c
                    det_grp[base + i] = group.get((s, t, c), -1)
        self.det_grp = det_grp
        self.det_box = cat([f[3] for f in fields], np.float32, (4,)).reshape(-1, 4)
        self.det_score = cat([f[2] for f in fields], np.float32)
        live = np.where(d_cls >= 0)[0]
        order = live[np.lexsort((live, -self.det_score[live], d_cls[live]))]
        self.order = order.astype(np.int32)
        self.n_live = int(order.shape[0])
        self.cls_off = np.searchsorted(d_cls[order], np.arange(self.C + 1), side='left').astype(np.int32)
        self.det_best: Optional[np.ndarray] = None
        self.claim_off = np.zeros(self.n_gt + 1, np.int32)
        self.claim_det = np.zeros(0, np.int32)
        self.n_claim = 0

    def best_host(self) -> np.ndarray:
        """det_best by the host definition: map_best_host over every group (what tmpnn_map_best computes on the device)."""
        best = np.full(self.n_det, -1, np.int32)
        for d in np.where(self.det_grp >= 0)[0]:
            a, b = int(self.grp_off[self.det_grp[d]]), int(self.grp_off[self.det_grp[d] + 1])
            j = int(map_best_host(self.det_box[d:d + 1], self.gt_box[a:b])[0])
            best[d] = a + j if j >= 0 else -1
        return best

    def set_best(self, best) -> None:
        """Take det_best [n_det] (int32, the store's GT order, -1 none) and build the claim lists from it."""
        best = np.asarray(best).astype(np.int32).reshape(-1)
        if best.shape[0] != self.n_det or (best.size and (best.min() < -1 or best.max() >= self.n_gt)):
            raise ValueError('MapStore.set_best: one entry in -1 .. n_gt - 1 per detection expected')
        self.det_best = best
        claim = np.where(best >= 0)[0]
        claim = claim[np.argsort(best[claim], kind='stable')]     # (by GT row, arrival order kept)
        self.claim_det = claim.astype(np.int32)
        self.n_claim = int(claim.shape[0])
        self.claim_off = np.searchsorted(best[claim], np.arange(self.n_gt + 1), side='left').astype(np.int32)


class MapEvaluator:
    """The validation mAP of S sequences on the device.  sequences: the dicts MotEvaluator takes plus det_cat, det_score, gt_cat
    (host arrays or tensors; they are the same in every epoch -- only the tracks change).  The store is built on the host and
    uploaded once; tmpnn_map_best runs once here and its result is read back once for the claim lists.

        ev.evaluate(tracks)   tracks: per sequence an int tensor / array [n_det] in arrival order, host or device (None: the
                              sequence takes no part in this evaluation).  One packed upload at the most, two launches, no host
                              wait.
        ev.read()             the one device -> host copy: the dict of map_host ('map', 'classes', 'ap', 'annotations', 'kept',
                              'true_positives' over the classes of the GT that took part).  RuntimeError when a class's flag
                              is set (the store is inconsistent).
    """

    def __init__(self, sequences: Sequence[Dict], device='cuda:0'):
        self.device = dev = cuda_device(device, 'MapEvaluator', 'score on the host with map_host')
        self.store = st = MapStore(sequences)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self._t = {k: up(getattr(st, k)) for k in ('gt_box', 'gt_seq', 'cls_gt_off', 'grp_off', 'det_box', 'det_grp', 'cls_off',
                                                   'order')}
        self._t['det_best'] = torch.empty(max(st.n_det, 1), dtype=torch.int32, device=dev)
        self._c = self._c_store()
        _lib.call('tmpnn_map_best', C.byref(self._c), self._t['det_best'].data_ptr(), _lib.raw_stream(dev))
        best = self._t['det_best'][:st.n_det].cpu().numpy()       # (the one read-back of the construction)
        if best.size and best.min() < -1:
            raise RuntimeError('MapEvaluator: tmpnn_map_best found a group out of range (the store is inconsistent)')
        st.set_best(best)
        self._t['claim_off'], self._t['claim_det'] = up(st.claim_off), up(st.claim_det)
        self._c = self._c_store()
        lib = _lib.load()
        self._ws_bytes = int(lib.tmpnn_map_eval_ws(st.n_gt, st.n_det, st.n_live))
        self._ws = torch.empty(max(self._ws_bytes, 16), dtype=torch.uint8, device=dev)
        # tracks [n_det] and, behind them, the S participation words: one buffer, so that one copy brings both
        self._in = torch.full((st.n_det + st.S + 1,), -1, dtype=torch.int32, device=dev)
        self._part_dev: Optional[List[bool]] = None                 # what the device's participation words say
        self._out = torch.zeros(max(st.C, 1), RECORD_WORDS, dtype=torch.int64, device=dev)
        self._pending = False

    def _c_store(self):
        st, t = self.store, self._t
        p = lambda k: (t[k].data_ptr() or None) if k in t else None
        return _lib.CMapStore(st.S, st.C, st.n_gt, st.n_det, st.n_grp, st.n_live, st.n_claim, *[p(k) for k in (
            'gt_box', 'gt_seq', 'cls_gt_off', 'grp_off', 'det_box', 'det_grp', 'det_best', 'cls_off', 'order', 'claim_off',
            'claim_det')])

    def evaluate(self, tracks: Sequence) -> None:
        st = self.store
        if len(tracks) != st.S:
            raise ValueError(f'MapEvaluator.evaluate: {len(tracks)} track arrays for {st.S} sequences')
        nd = st.n_det
        host = np.full(nd + st.S, -1, np.int32)
        on_device = []
        part = []
        host_used = False
        for s, tr in enumerate(tracks):
            base, n = int(st.det_base[s]), int(st.det_base[s + 1] - st.det_base[s])
            part.append(tr is not None)
            if tr is None:
                host_used |= n > 0                                  # (its slice is filled with -1)
                continue
            if isinstance(tr, torch.Tensor) and tr.is_cuda:
                if tr.dtype.is_floating_point or tr.numel() != n:
                    raise ValueError(f'MapEvaluator.evaluate: sequence {s}: an int tensor of {n} tracks expected')
                on_device.append((base, n, tr))
            else:
                a = _ints(tr, f'MapEvaluator.evaluate: sequence {s}: tracks', n)
                host[base:base + n] = np.clip(a, -1, 2 ** 31 - 1)   # (only the sign is read)
                host_used |= n > 0
        host[nd:] = part
        if host_used:
            self._in[:nd + st.S].copy_(torch.from_numpy(host), non_blocking=True)          # the one packed upload
        elif part != self._part_dev and st.S:
            self._in[nd:nd + st.S].copy_(torch.from_numpy(host[nd:]), non_blocking=True)   # (the participation words alone)
        self._part_dev = part
        for base, n, tr in on_device:
            self._in[base:base + n].copy_(tr.reshape(-1).clamp(-1, 2 ** 31 - 1))
        p = self._in.data_ptr()
        _lib.call('tmpnn_map_eval', C.byref(self._c), p, p + 4 * nd, self._ws.data_ptr(), self._ws_bytes, self._out.data_ptr(),
                  _lib.raw_stream(self.device))
        self._pending = True

    def read(self) -> Dict:
        if not self._pending:
            raise RuntimeError('MapEvaluator.read: no evaluation has been enqueued')
        st = self.store
        rec = self._out.cpu().numpy()                               # (the one device -> host copy; it waits for the launches)
        ap = rec.view(np.float64)[:, 0]
        bad = [st.classes[c] for c in range(st.C) if rec[c, 4] != 0]
        if bad:
            raise RuntimeError(f'MapEvaluator.read: classes {bad}: the store is inconsistent (an offset or an index out of range)')
        out = {'classes': [], 'ap': [], 'annotations': [], 'kept': [], 'true_positives': []}
        for c in range(st.C):
            if rec[c, 1] == 0:                                      # (none of its GT takes part: not a class of this evaluation)
                continue
            out['classes'].append(st.classes[c])
            out['ap'].append(float(ap[c]))
            out['annotations'].append(int(rec[c, 1]))
            out['kept'].append(int(rec[c, 2]))
            out['true_positives'].append(int(rec[c, 3]))
        out['map'] = _mean(out['ap'])
        return out
