"""GT track ids for detections: the reference's get_track_ids (dataset/kitti_mot.py:422-486, dataset/bdd100k_mot.py:407-470),
once per data set instead of once per chunk.

    LabelRules             the two ignore categories and the two thresholds; KITTI_RULES (DontCare 9, Van 4), BDD_RULES (crowd -1,
                           distractor 9)
    label_overlaps_host    the float32 "+1" IoU and IoM matrices of two float32 box lists (utils/misc.py:4-42, numpy's order)
    label_frame_host       the rule for one frame, in numpy.  It is the DEFINITION the device must equal, exactly.
    label_detections_host  the rule over the frames of every sequence
    DetectionLabeler       the sequences on the device + `label()` (tmpnn_label_dets, tmpnn_label_compact; csrc/labeldet.hip: four
                           launches, no host wait) + `read()` (the one device -> host copy) + `store_sequences()` (what
                           DetectionStore takes) + `eval_sequences()` (what MotEvaluator / MapEvaluator take)

The rule, per frame.  GT rows of the two ignore categories are no ground truth (gt_keep False); the others are the MATCHABLE rows,
in input order.  A pair (detection p, matchable row g) is eligible when the categories are equal and iou >= iou_thresh.  The
eligible pairs are walked in descending IoU; a pair is accepted when both its ends are still free, and the detection then takes
the row's track id.  A detection that was not assigned is dropped when the maximum of its IoM over the `iom_ignore_cat` boxes is
>= iom_thresh or the maximum of its IoU over the `iou_ignore_cat` boxes is >= iou_thresh (np.amax: one NaN in the row makes
the maximum NaN, which passes no `>=`, so the detection stays -- as in the reference).  An assigned detection always stays.  A
frame without any GT row keeps every detection unassigned; a frame without detections still filters its GT.

Overlaps are float32, every operation in numpy's order on the float32 boxes; the thresholds are compared as float32.  A NaN
never passes a `>=`.

THE TIE ORDER IS THE LIBRARY'S CHOICE.  The reference orders the pairs with numpy's unstable argsort, so among exactly equal
IoUs its order is whatever that sort gives.  Here, among equal IoUs, the pair with the smaller flat index p * G' + g goes first
(G' = the number of matchable rows, g counted among them).

STATED DEVIATION.  The reference labels every chunk after its horizontal flip, on the flipped float32 boxes; here the plain boxes
are labelled once (the assignment does not depend on time reversal or dropout).  A flip preserves overlaps in exact
arithmetic; in float32 a pair lying exactly at a threshold could fall the other way.  This stands next to the other stated
deviation of the training data: ChunkSampler's draws match the reference in distribution, not in stream (trackmpnn_amd.chunks).

The device takes at most 256 detections and at most 256 GT rows (ignore rows included) per frame, as MotEvaluator does; a larger
frame sets a flag and `read()` raises.  The host definition has no limit.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .evalstore import _boxes, _ints

MAX_PER_FRAME = 256            # detections / GT rows of one frame the device takes (csrc/labeldet.hip LB_MAX)
WAVE_FRAME = 64                # frames with at most this many rows on either side are labelled by one wave
FLAG_LIMIT, FLAG_STORE = 1, 2
RECORD_WORDS = 4               # struct tmpnn_label_record: flag, frame, kept_det, kept_gt (int64)
_I32 = 2 ** 31


@dataclass(frozen=True)
class LabelRules:
    """iom_ignore_cat: regions (DontCare, crowd) whose unassigned detections are dropped by intersection over minimum;
    iou_ignore_cat: objects (Van, distractor) whose unassigned detections are dropped by IoU.  Both are no ground truth."""
    iom_ignore_cat: int
    iou_ignore_cat: int
    iou_thresh: float = 0.5
    iom_thresh: float = 0.8


KITTI_RULES = LabelRules(9, 4)
BDD_RULES = LabelRules(-1, 9)


def label_overlaps_host(box_a, box_b) -> Tuple[np.ndarray, np.ndarray]:
    """(iou, iom), both float32 [len(box_a), len(box_b)]: vectorized_iou / vectorized_iom of utils/misc.py with the "+1" on every
    width and height, every operation in float32 in numpy's order."""
    a, b = _boxes(box_a, 'box_a'), _boxes(box_b, 'box_b')
    x11, y11, x12, y12 = (a[:, i:i + 1] for i in range(4))
    x21, y21, x22, y22 = (b[:, i][None, :] for i in range(4))
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        xA, yA = np.maximum(x11, x21), np.maximum(y11, y21)
        xB, yB = np.minimum(x12, x22), np.minimum(y12, y22)
        inter = np.maximum((xB - xA) + one, zero) * np.maximum((yB - yA) + one, zero)
        area_a = ((x12 - x11) + one) * ((y12 - y11) + one)
        area_b = ((x22 - x21) + one) * ((y22 - y21) + one)
        iou = inter / ((area_a + area_b) - inter)
        iom = inter / np.minimum(area_a, area_b)
    return iou.astype(np.float32, copy=False), iom.astype(np.float32, copy=False)


def _gt_class(gt_cat: np.ndarray, rules: LabelRules) -> np.ndarray:
    """0: matchable, 1: an iom_ignore_cat row, 2: an iou_ignore_cat row (1 wins where the two categories are the same)."""
    return np.where(gt_cat == int(rules.iom_ignore_cat), 1, np.where(gt_cat == int(rules.iou_ignore_cat), 2, 0))


def label_frame_host(det_cat, det_box, gt_track, gt_cat, gt_box, rules: LabelRules):
    """One frame: (track int64 [P] (-1: not assigned), keep bool [P], gt_keep bool [G]).  The definition (module docstring).
    Matchable GT rows carry track ids >= 0 (ValueError otherwise: -1 means "not assigned")."""
    det_cat, gt_cat = _ints(det_cat, 'det_cat'), _ints(gt_cat, 'gt_cat')
    P, G = det_cat.shape[0], gt_cat.shape[0]
    gt_track = _ints(gt_track, 'gt_track', G)
    det_box, gt_box = _boxes(det_box, 'det_box'), _boxes(gt_box, 'gt_box')
    if det_box.shape[0] != P or gt_box.shape[0] != G:
        raise ValueError('label_frame_host: one box per row expected')
    cls = _gt_class(gt_cat, rules)
    gt_keep = cls == 0
    if (gt_track[gt_keep] < 0).any():
        raise ValueError('label_frame_host: a matchable GT row has a negative track id')
    track, keep = np.full(P, -1, np.int64), np.ones(P, bool)
    if P == 0 or G == 0:
        return track, keep, gt_keep
    iou_t, iom_t = np.float32(rules.iou_thresh), np.float32(rules.iom_thresh)
    rows = np.where(gt_keep)[0]
    if rows.size:
        iou = label_overlaps_host(det_box, gt_box[rows])[0]
        with np.errstate(invalid='ignore'):
            ok = (iou >= iou_t) & (det_cat[:, None] == gt_cat[rows][None, :])
        flat = np.where(ok.ravel())[0]
        v = iou.ravel()[flat]
        taken = np.zeros(rows.size, bool)
        for k in flat[np.lexsort((flat, -v))]:                    # descending IoU, equal IoUs by ascending flat index
            p, g = divmod(int(k), rows.size)
            if track[p] < 0 and not taken[g]:
                track[p], taken[g] = gt_track[rows[g]], True
    free = track < 0
    with np.errstate(invalid='ignore'):
        for c, which, thr in ((1, 1, iom_t), (2, 0, iou_t)):
            rows = np.where(cls == c)[0]
            if rows.size:
                keep &= ~(free & (np.amax(label_overlaps_host(det_box, gt_box[rows])[which], axis=1) >= thr))
    return track, keep, gt_keep


def _fields(q: Dict, s: int) -> Dict:
    """The arrays of one sequence, checked (ValueError) and sorted stably by frame.  Returns a dict with num_frames, width, the
    sorted det_* / gt_* columns, the permutations det_order / gt_order (sorted position -> input index) and the per-frame
    offsets det_first / gt_first [num_frames + 1]."""
    who = f'DetectionLabeler: sequence {s}'
    nf = int(q['num_frames'])
    if nf < 1 or nf >= 2 ** 24:
        raise ValueError(f'{who}: num_frames={nf} (1 .. 2^24 - 1)')
    width = q['width']
    if not np.isfinite(float(width)):
        raise ValueError(f'{who}: width={width}')
    det_frame, gt_frame = _ints(q['det_frame'], f'{who}: det_frame'), _ints(q['gt_frame'], f'{who}: gt_frame')
    nd, ng = det_frame.shape[0], gt_frame.shape[0]
    det_cat, gt_cat = _ints(q['det_cat'], f'{who}: det_cat', nd), _ints(q['gt_cat'], f'{who}: gt_cat', ng)
    gt_track = _ints(q['gt_track'], f'{who}: gt_track', ng)
    sc = q['det_score']
    if isinstance(sc, torch.Tensor):
        sc = sc.detach().cpu().numpy()
    score = np.asarray(sc).reshape(-1)
    db, gb = _boxes(q['det_box'], 'det_box'), _boxes(q['gt_box'], 'gt_box')
    if db.shape[0] != nd or gb.shape[0] != ng or score.shape[0] != nd:
        raise ValueError(f'{who}: frame, cat, box, score (detections) or frame, track, cat, box (GT) differ in length')
    if not (np.isfinite(db).all() and np.isfinite(gb).all() and np.isfinite(score.astype(np.float64)).all()):
        raise ValueError(f'{who}: a box or score is not finite')
    for a, nm in ((det_frame, 'det_frame'), (gt_frame, 'gt_frame')):
        if a.size and (a.min() < 0 or a.max() >= nf):
            raise ValueError(f'{who}: a {nm} outside [0, num_frames = {nf})')
    for a, nm in ((det_cat, 'det_cat'), (gt_cat, 'gt_cat'), (gt_track, 'gt_track')):
        if a.size and (a.min() < -_I32 or a.max() >= _I32):
            raise ValueError(f'{who}: a {nm} outside int32')
    do, go = np.argsort(det_frame, kind='stable'), np.argsort(gt_frame, kind='stable')
    f = {'num_frames': nf, 'width': width, 'det_order': do, 'gt_order': go, 'det_box_in': np.asarray(q['det_box']).reshape(-1, 4),
         'det_score_in': score,
         'det_frame': det_frame[do], 'det_cat': det_cat[do], 'det_box': db[do], 'det_score': score[do].astype(np.float32),
         'gt_frame': gt_frame[go], 'gt_track': gt_track[go], 'gt_cat': gt_cat[go], 'gt_box': gb[go]}
    f['det_first'] = np.searchsorted(f['det_frame'], np.arange(nf + 1))
    f['gt_first'] = np.searchsorted(f['gt_frame'], np.arange(nf + 1))
    return f


def _check_matchable(fields: Sequence[Dict], rules: LabelRules) -> None:
    for s, f in enumerate(fields):
        if (f['gt_track'][_gt_class(f['gt_cat'], rules) == 0] < 0).any():
            raise ValueError(f'DetectionLabeler: sequence {s}: a GT row outside the ignore categories has a negative track id')


def _label_sorted_host(f: Dict, rules: LabelRules):
    """(track, keep, gt_keep) of one checked sequence, in its frame-sorted order."""
    nd, ng = f['det_frame'].shape[0], f['gt_frame'].shape[0]
    track, keep, gt_keep = np.full(nd, -1, np.int64), np.ones(nd, bool), np.ones(ng, bool)
    for t in range(f['num_frames']):
        d0, d1, g0, g1 = f['det_first'][t], f['det_first'][t + 1], f['gt_first'][t], f['gt_first'][t + 1]
        if d0 == d1 and g0 == g1:
            continue
        track[d0:d1], keep[d0:d1], gt_keep[g0:g1] = label_frame_host(f['det_cat'][d0:d1], f['det_box'][d0:d1], f['gt_track'][g0:g1],
                                                                     f['gt_cat'][g0:g1], f['gt_box'][g0:g1], rules)
    return track, keep, gt_keep


def _unsort(f: Dict, track, keep, gt_keep) -> Dict:
    out = {'track': np.empty_like(track), 'keep': np.empty_like(keep), 'gt_keep': np.empty_like(gt_keep)}
    out['track'][f['det_order']], out['keep'][f['det_order']], out['gt_keep'][f['gt_order']] = track, keep, gt_keep
    return out


def label_detections_host(sequences: Sequence[Dict], rules: LabelRules) -> List[Dict]:
    """label_frame_host over the frames of every sequence (the dicts DetectionLabeler takes).  Per sequence a dict with `track`
    int64 [n] (-1: not assigned), `keep` bool [n], `gt_keep` bool [m], in the order of the input rows."""
    fields = [_fields(q, s) for s, q in enumerate(sequences)]
    _check_matchable(fields, rules)
    return [_unsort(f, *_label_sorted_host(f, rules)) for f in fields]


def _al16(n: int) -> int:
    return (int(n) + 15) & ~15


class DetectionLabeler:
    """Labels the detections of S sequences against their ground truth on the device.

    sequences   per sequence a mapping with det_frame [n] int, det_cat [n] int, det_box [n, 4] x1 y1 x2 y2, det_score [n],
                gt_frame [m] int, gt_track [m] int, gt_cat [m] int, gt_box [m, 4], num_frames and the image width: the
                evaluators' field names plus what DetectionStore needs.  Frames lie in [0, num_frames), boxes and scores are
                finite, GT rows outside the two ignore categories have track ids >= 0; ValueError otherwise.
    rules       LabelRules (KITTI_RULES, BDD_RULES)
    device      a cuda device; None: a host-only labeler whose label() runs label_detections_host (as DetectionStore's
                device=None is a host-only store)

        lb.label()             enqueues the launches (tmpnn_label_dets, tmpnn_label_compact); no host wait
        lb.read()              the one device -> host copy: per sequence `track`, `keep`, `gt_keep` in input order.  RuntimeError
                               when a frame has more than 256 detections or GT rows
        lb.store_sequences()   what DetectionStore takes: the kept detections (frame, track, cat, box, score, width, num_frames)
        lb.eval_sequences()    what MotEvaluator / MapEvaluator take: the kept detections and the kept GT rows

    The kept rows of both lists are sorted stably by frame (input order within a frame), which is the order DetectionStore and
    the evaluators give them anyway.  store_sequences() hands on the boxes and scores as they were passed in (DetectionStore
    computes the flip from them in float64); eval_sequences() the float32 rows that were labelled."""

    def __init__(self, sequences: Sequence[Dict], rules: LabelRules, device='cuda:0'):
        if not isinstance(rules, LabelRules):
            raise ValueError('DetectionLabeler: rules must be a LabelRules')
        for c in (rules.iom_ignore_cat, rules.iou_ignore_cat):
            if int(c) != c or not -_I32 <= int(c) < _I32:
                raise ValueError(f'DetectionLabeler: ignore category {c!r}')
        if not (np.isfinite(rules.iou_thresh) and np.isfinite(rules.iom_thresh)):
            raise ValueError('DetectionLabeler: thresholds must be finite')
        sequences = list(sequences)
        if not sequences:
            raise ValueError('DetectionLabeler: no sequences')
        self.rules = rules
        self.fields = fl = [_fields(q, s) for s, q in enumerate(sequences)]
        _check_matchable(fl, rules)
        self.S = S = len(fl)
        self.seq_base = np.concatenate([[0], np.cumsum([f['num_frames'] for f in fl])]).astype(np.int64)
        self.det_base = np.concatenate([[0], np.cumsum([f['det_frame'].shape[0] for f in fl])]).astype(np.int64)
        self.gt_base = np.concatenate([[0], np.cumsum([f['gt_frame'].shape[0] for f in fl])]).astype(np.int64)
        self.F, self.n_det, self.n_gt = int(self.seq_base[-1]), int(self.det_base[-1]), int(self.gt_base[-1])
        if max(self.F, self.n_det, self.n_gt) >= _I32 - 1:
            raise ValueError('DetectionLabeler: frames, detections and GT rows must fit in int32')
        self._host: Optional[List[Dict]] = None       # what read() returned
        self._packed = None                           # per sequence the kept rows (dicts of sorted-order arrays)
        self._pending = False
        F, n, m = self.F, self.n_det, self.n_gt
        det_first = np.concatenate([f['det_first'][:-1] + b for f, b in zip(fl, self.det_base[:-1])] + [[n]])
        gt_first = np.concatenate([f['gt_first'][:-1] + b for f, b in zip(fl, self.gt_base[:-1])] + [[m]])
        # the routing of the device: a frame of at most WAVE_FRAME rows on either side is labelled by one wave
        size = np.maximum(np.diff(det_first), np.diff(gt_first))
        small, big = np.where(size <= WAVE_FRAME)[0], np.where(size > WAVE_FRAME)[0]
        self.n_small, self.n_big = int(small.shape[0]), int(big.shape[0])
        self.device = None
        if device is None:
            return
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'DetectionLabeler on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only: pass a cuda device, '
                               'or device=None for a host-only labeler (label_detections_host)')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        cat = lambda k: np.concatenate([f[k] for f in fl])
        ints = [self.seq_base, det_first, gt_first, small, big, cat('det_frame'), cat('det_cat'), cat('gt_frame'), cat('gt_track'),
                cat('gt_cat')]
        # one upload per type; every section starts on a 16-byte boundary
        io = np.cumsum([0] + [_al16(4 * a.shape[0]) // 4 for a in ints])
        ibuf = np.zeros(max(int(io[-1]), 4), np.int32)
        for a, o in zip(ints, io[:-1]):
            ibuf[o:o + a.shape[0]] = a
        flts = [cat('det_box').reshape(-1), cat('gt_box').reshape(-1), cat('det_score')]
        fo = np.cumsum([0] + [_al16(4 * a.shape[0]) // 4 for a in flts])
        fbuf = np.zeros(max(int(fo[-1]), 4), np.float32)
        for a, o in zip(flts, fo[:-1]):
            fbuf[o:o + a.shape[0]] = a
        self._ibuf, self._fbuf = torch.from_numpy(ibuf).to(dev), torch.from_numpy(fbuf).to(dev)
        ip = lambda k: self._ibuf.data_ptr() + 4 * int(io[k])
        fp = lambda k: self._fbuf.data_ptr() + 4 * int(fo[k])
        self._c_store = _lib.CLabelStore(S, 0, F, n, m, int(rules.iom_ignore_cat), int(rules.iou_ignore_cat),
                                         float(np.float32(rules.iou_thresh)), float(np.float32(rules.iom_thresh)),
                                         self.n_small, self.n_big, ip(0), ip(1), ip(2), ip(3), ip(4), ip(5), ip(6), fp(0), fp(2),
                                         ip(7), ip(8), ip(9), fp(1))
        # the results: one buffer, so that one copy brings everything (sections in the order of struct tmpnn_label_out)
        secs = [('record', 8 * RECORD_WORDS), ('track', 4 * n), ('keep', n), ('gt_keep', m), ('det_cnt', 4 * F), ('gt_cnt', 4 * F),
                ('fflag', F), ('det_off', 4 * (F + 1)), ('gt_off', 4 * (F + 1)), ('seq_det_off', 4 * (S + 1)),
                ('seq_gt_off', 4 * (S + 1)), ('o_det_frame', 4 * n), ('o_det_track', 4 * n), ('o_det_cat', 4 * n),
                ('o_det_box', 16 * n), ('o_det_score', 4 * n), ('o_gt_frame', 4 * m), ('o_gt_track', 4 * m), ('o_gt_cat', 4 * m),
                ('o_gt_box', 16 * m)]
        self._sec, off = {}, 0
        for k, b in secs:
            self._sec[k] = (off, b)
            off += _al16(b)
        self._out = torch.zeros(max(off, 16), dtype=torch.uint8, device=dev)
        self._c_out = _lib.CLabelOut(*[self._out.data_ptr() + self._sec[k][0] for k, _ in secs])

    # ---- the launches
    def label(self) -> None:
        self._host = self._packed = None
        if self.device is None:
            res = [_label_sorted_host(f, self.rules) for f in self.fields]
            self._host = [_unsort(f, *r) for f, r in zip(self.fields, res)]
            self._packed = [self._pack_host(f, *r) for f, r in zip(self.fields, res)]
            return
        st = _lib.raw_stream(self.device)
        _lib.call('tmpnn_label_dets', C.byref(self._c_store), C.byref(self._c_out), st)
        _lib.call('tmpnn_label_compact', C.byref(self._c_store), C.byref(self._c_out), st)
        self._pending = True

    @staticmethod
    def _pack_host(f: Dict, track, keep, gt_keep) -> Dict:
        return {'det_idx': np.where(keep)[0], 'det_frame': f['det_frame'][keep], 'det_track': track[keep], 'det_cat': f['det_cat'][keep],
                'det_box': f['det_box'][keep], 'det_score': f['det_score'][keep], 'gt_frame': f['gt_frame'][gt_keep],
                'gt_track': f['gt_track'][gt_keep], 'gt_cat': f['gt_cat'][gt_keep], 'gt_box': f['gt_box'][gt_keep]}

    def read(self) -> List[Dict]:
        if self._host is not None:
            return self._host
        if not self._pending:
            raise RuntimeError('DetectionLabeler.read: no labelling has been enqueued')
        raw = self._out.cpu().numpy()                               # (the one device -> host copy; it waits for the launches)

        def sec(k, dtype, tail=()):
            o, b = self._sec[k]
            return raw[o:o + b].view(dtype).reshape((-1,) + tail)
        rec = sec('record', np.int64)
        if rec[0] & FLAG_LIMIT:
            t = int(rec[1])
            s = int(np.searchsorted(self.seq_base, t, side='right') - 1)
            raise RuntimeError(f'DetectionLabeler.read: sequence {s}, frame {t - int(self.seq_base[s])} has more than '
                               f'{MAX_PER_FRAME} detections or GT rows')
        if rec[0]:
            raise RuntimeError('DetectionLabeler.read: the store is inconsistent (an offset or a frame index out of range)')
        track, keep, gt_keep = sec('track', np.int32).astype(np.int64), sec('keep', np.uint8) != 0, sec('gt_keep', np.uint8) != 0
        sdo, sgo = sec('seq_det_off', np.int32), sec('seq_gt_off', np.int32)
        if int(rec[2]) != int(keep.sum()) or int(rec[3]) != int(gt_keep.sum()) or sdo[-1] != rec[2] or sgo[-1] != rec[3]:
            raise RuntimeError('DetectionLabeler.read: the compaction disagrees with the keep flags')
        cols = {k: sec('o_' + k, np.float32 if k in ('det_box', 'gt_box', 'det_score') else np.int32, (4,) if k.endswith('box') else ())
                for k in ('det_frame', 'det_track', 'det_cat', 'det_box', 'det_score', 'gt_frame', 'gt_track', 'gt_cat', 'gt_box')}
        host, packed = [], []
        for s, f in enumerate(self.fields):
            d0, d1, g0, g1 = (int(x) for x in (self.det_base[s], self.det_base[s + 1], self.gt_base[s], self.gt_base[s + 1]))
            host.append(_unsort(f, track[d0:d1], keep[d0:d1], gt_keep[g0:g1]))
            p = {k: (v[sdo[s]:sdo[s + 1]] if k.startswith('det') else v[sgo[s]:sgo[s + 1]]) for k, v in cols.items()}
            p = {k: (v.astype(np.int64) if v.dtype == np.int32 else v.copy()) for k, v in p.items()}
            p['det_idx'] = np.where(keep[d0:d1])[0]
            packed.append(p)
        self._host, self._packed, self._pending = host, packed, False
        return host

    def _need(self) -> List[Dict]:
        if self._packed is None:
            self.read()
        return self._packed

    def store_sequences(self) -> List[Dict]:
        out = []
        for f, p in zip(self.fields, self._need()):
            src = f['det_order'][p['det_idx']]                      # input index of every kept detection
            out.append({'frame': p['det_frame'], 'track': p['det_track'], 'cat': p['det_cat'], 'box': f['det_box_in'][src],
                        'score': f['det_score_in'][src], 'width': f['width'], 'num_frames': f['num_frames']})
        return out

    def eval_sequences(self) -> List[Dict]:
        keys = ('det_frame', 'det_cat', 'det_box', 'det_score', 'gt_frame', 'gt_track', 'gt_cat', 'gt_box')
        return [{k: p[k] for k in keys} for p in self._need()]


def synth_label_sequence(seed: int, frames: int, rules: LabelRules = KITTI_RULES, max_det: int = 39, max_gt: int = 29,
                         classes: Sequence[int] = (1, 2, 3), sigma: float = 6.0, p_wrong: float = 0.2, width: int = 1242,
                         height: int = 375, sizes: Optional[Sequence[Tuple[int, int]]] = None) -> Dict:
    """A seeded synthetic sequence for the labeller (a DetectionLabeler dict): per frame 0 .. max_gt GT rows whose categories are
    drawn evenly from `classes` and the two ignore categories of `rules`, and 0 .. max_det detections, each a jittered copy
    (normal, `sigma` pixels a coordinate) of a random GT box of its frame with that box's class -- with p_wrong another of
    `classes`, and a random one for a copy of an ignore row; a frame without GT gets random boxes.  Track ids are distinct
    within a frame; rows of iom_ignore_cat carry -1.  So assigned, unassigned and removed detections all occur in number.
    sizes: per frame (detections, GT rows) in place of the random counts (`frames` is then their number)."""
    rng = np.random.default_rng([int(seed), 4242])
    cats = list(classes) + [int(rules.iom_ignore_cat), int(rules.iou_ignore_cat)]
    cols: Dict[str, list] = {k: [] for k in ('det_frame', 'det_cat', 'det_box', 'det_score', 'gt_frame', 'gt_track', 'gt_cat', 'gt_box')}

    def boxes(n):
        c = np.stack([rng.uniform(0, width, n), rng.uniform(0, height, n)], 1)
        wh = rng.uniform(30, 140, (n, 2))
        return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    if sizes is not None:
        frames = len(sizes)
    for t in range(int(frames)):
        if sizes is None:
            G, P = int(rng.integers(0, max_gt + 1)), int(rng.integers(0, max_det + 1))
        else:
            P, G = (int(v) for v in sizes[t])
        g_box, g_cat = boxes(G), np.asarray([cats[i] for i in rng.integers(0, len(cats), G)], np.int64)
        g_track = np.where(g_cat == int(rules.iom_ignore_cat), -1, rng.permutation(1000)[:G])
        if G:
            src = rng.integers(0, G, P)
            d_box = (g_box[src] + rng.normal(0, sigma, (P, 4))).astype(np.float32)
            d_cat = g_cat[src].copy()
            for i in range(P):
                if d_cat[i] not in classes:
                    d_cat[i] = classes[int(rng.integers(len(classes)))]
                elif rng.random() < p_wrong:
                    d_cat[i] = [c for c in classes if c != d_cat[i]][int(rng.integers(len(classes) - 1))]
        else:
            d_box, d_cat = boxes(P), np.asarray([classes[i] for i in rng.integers(0, len(classes), P)], np.int64)
        for k, v in (('det_frame', np.full(P, t)), ('det_cat', d_cat), ('det_box', d_box), ('det_score', rng.random(P).astype(np.float32)),
                     ('gt_frame', np.full(G, t)), ('gt_track', g_track), ('gt_cat', g_cat), ('gt_box', g_box)):
            cols[k].append(v)
    q = {k: (np.concatenate(v).astype(np.float32).reshape(-1, 4) if k.endswith('box') else
             np.concatenate(v).astype(np.float32 if k == 'det_score' else np.int64)) for k, v in cols.items()}
    q.update(num_frames=int(frames), width=int(width))
    return q
