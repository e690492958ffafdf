"""CLEAR-MOT counts of a set of tracks against the ground truth (reference utils/metrics.py:7-61, train.py:264-282).

    mot_events_host     the rule, in numpy + scipy: one sequence in, the counts out.  It is the DEFINITION the device kernel
                        must equal (counts exactly, distances and their sum bit for bit).
    mot_dist_host       the float64 distance matrix of two box lists (1 - IoU, NaN above 0.5)
    mot_overall         the figures of several sequences: ratios of the summed counts
    MotStore            the per-sequence data that do not change between epochs (frames, boxes, GT ids), sorted by frame,
                        packed over the sequences
    MotEvaluator        the store on the device + `evaluate(tracks)` (one launch of tmpnn_mot_events, csrc/moteval.hip, one
                        workgroup per sequence) + `read()` (the one device -> host copy)
    mot_summary_host    the rule of the rest of the MOT-challenge summary (track coverage, fragmentations, the identity
                        figures IDF1 / IDP / IDR), built on the same walk; MotEvaluator(identity=True) equals it (tmpnn_mot_summary)

The reference scores with py-motmetrics (a pandas accumulator fed one frame at a time).  That package is not a dependency
of this library and is not pinned by any fixture: the rule below restates MOTAccumulator.update and iou_matrix as they are
in py-motmetrics >= 1.2 and as metrics.py calls them ("unpinnable").
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _lib
from .evalstore import (FLAG_DUPLICATE, FLAG_LIMIT, FLAG_SOLVER, FLAG_STORE, SeqTable, SequenceEvaluator, _boxes, _frame_range, _ints,
                        frame_sort)

MAX_PER_FRAME = 256            # GT rows / kept hypotheses of one frame the device solver takes (csrc/moteval.hip MOT_MAX)
COUNT_KEYS = ('objects', 'predictions', 'matches', 'switches', 'false_positives', 'misses', 'frames')
SUMMARY_KEYS = ('unique_objects', 'mostly_tracked', 'partially_tracked', 'mostly_lost', 'fragmentations')
MAX_PAIR_COUNTS = 2 ** 27      # entries (int32) of the identity count matrices of one store: sum over sequences of n_obj x n_det
_FLAG_TEXT = {FLAG_LIMIT: f'a frame has more than {MAX_PER_FRAME} GT rows or kept hypotheses',
              FLAG_DUPLICATE: 'a hypothesis id occurs twice in one frame',
              FLAG_STORE: 'the store is inconsistent (an offset, a permutation entry or an object id out of range)',
              FLAG_SOLVER: 'the assignment solver found no augmenting path'}


def mot_dist_host(box_o, box_h) -> np.ndarray:
    """[len(box_o), len(box_h)] float64: 1 - IoU of x1 y1 x2 y2 boxes, NaN where it exceeds 0.5 (and where it is 0 / 0).
    Width and height are formed in float32, everything after that in float64 -- metrics.py:36-40 hands float32
    (x, y, w, h) rows to iou_matrix(max_iou=0.5), which works in float64."""
    bo, bh = _boxes(box_o, 'box_o'), _boxes(box_h, 'box_h')
    tl_o, tl_h = bo[:, :2].astype(np.float64), bh[:, :2].astype(np.float64)
    wh_o, wh_h = (bo[:, 2:] - bo[:, :2]).astype(np.float64), (bh[:, 2:] - bh[:, :2]).astype(np.float64)
    br_o, br_h = tl_o + wh_o, tl_h + wh_h
    with np.errstate(invalid='ignore', divide='ignore'):
        iwh = np.maximum(np.minimum(br_o[:, None, :], br_h[None, :, :]) - np.maximum(tl_o[:, None, :], tl_h[None, :, :]), 0)
        inter = iwh[..., 0] * iwh[..., 1]
        union = ((wh_o[:, 0] * wh_o[:, 1])[:, None] + (wh_h[:, 0] * wh_h[:, 1])[None, :]) - inter
        d = 1.0 - inter / union
        d[d > 0.5] = np.nan
    return d


def _derived(c: Dict) -> Dict:
    def ratio(a, b):
        return float(a) / float(b) if b else float('nan')
    c['mota'] = 1.0 - ratio(c['misses'] + c['false_positives'] + c['switches'], c['objects'])
    c['motp'] = ratio(c['dist_sum'], c['matches'])
    c['recall'] = ratio(c['matches'], c['objects'])
    c['precision'] = ratio(c['matches'], c['predictions'])
    if 'idtp' in c:                                               # (mot_summary_host: the identity figures)
        c['idfp'], c['idfn'] = c['predictions'] - c['idtp'], c['objects'] - c['idtp']
        c['idp'] = ratio(c['idtp'], c['idtp'] + c['idfp'])
        c['idr'] = ratio(c['idtp'], c['idtp'] + c['idfn'])
        c['idf1'] = ratio(2 * c['idtp'], c['objects'] + c['predictions'])
    return c


def mot_overall(per_sequence: Sequence[Dict]) -> Dict:
    """The figures over several sequences: ratios of the SUMMED counts (compute_many(..., generate_overall=True),
    train.py:281-282), dist_sum added in the order of the list.  Where every dict has them (mot_summary_host) the coverage
    counts, the fragmentations and idtp are summed as well, and the identity ratios formed from the sums."""
    keys = COUNT_KEYS + tuple(k for k in SUMMARY_KEYS + ('idtp',) if per_sequence and all(k in r for r in per_sequence))
    c = {k: 0 for k in keys}
    c['dist_sum'] = 0.0
    for r in per_sequence:
        for k in keys:
            c[k] += int(r[k])
        c['dist_sum'] += float(r['dist_sum'])
    return _derived(c)


def _check_unique(ids: np.ndarray, t: int, what: str):
    if np.unique(ids).shape[0] != ids.shape[0]:
        raise ValueError(f'mot_events: {what} id occurs twice in frame {t}')


def _mot_walk(det_frame, det_box, tracks, gt_frame, gt_track, gt_box, on_frame=None):
    """The frame walk behind mot_events_host and mot_summary_host: the counts (before _derived), and the checked arrays
    (det_frame, det_box, tracks, gt_frame, gt_track, gt_box, t0, nframes).  on_frame(t, oids, tracked): the GT ids of frame t
    and, per id, whether the walk matched it there (step 1 or step 2, a switch included)."""
    from scipy.optimize import linear_sum_assignment
    det_frame, gt_frame = _ints(det_frame, 'det_frame'), _ints(gt_frame, 'gt_frame')
    tracks, gt_track = _ints(tracks, 'tracks', det_frame.shape[0]), _ints(gt_track, 'gt_track', gt_frame.shape[0])
    det_box, gt_box = _boxes(det_box, 'det_box'), _boxes(gt_box, 'gt_box')
    if det_box.shape[0] != det_frame.shape[0] or gt_box.shape[0] != gt_frame.shape[0]:
        raise ValueError('mot_events: one box per row expected')
    t0, nframes = _frame_range(det_frame, gt_frame)
    c = {k: 0 for k in COUNT_KEYS}
    c['frames'] = nframes
    dist_sum = 0.0
    m: Dict[int, int] = {}
    last_match: Dict[int, int] = {}
    for t in range(t0, t0 + nframes):
        orow = np.where((gt_frame == t) & (gt_track >= 0))[0]
        hrow = np.where((det_frame == t) & (tracks >= 0))[0]
        oids, hids = gt_track[orow], tracks[hrow]
        _check_unique(oids, t, 'a GT')
        _check_unique(hids, t, 'a hypothesis')
        nO, nH = oids.shape[0], hids.shape[0]
        c['objects'] += nO
        c['predictions'] += nH
        matched_d = [None] * nO
        hmask = np.zeros(nH, dtype=bool)
        if nO and nH:
            d = mot_dist_host(gt_box[orow], det_box[hrow])
            omask = np.zeros(nO, dtype=bool)
            for i in range(nO):                                   # step 1
                o = int(oids[i])
                if o not in m or last_match.get(o) != t - 1:
                    continue
                js = np.where(~hmask & (hids == m[o]))[0]
                if js.shape[0] == 0:
                    continue
                j = int(js[0])
                if np.isfinite(d[i, j]):
                    omask[i] = hmask[j] = True
                    matched_d[i] = float(d[i, j])
                    last_match[o] = t
                    c['matches'] += 1
            d2 = d.copy()                                         # step 2
            d2[omask, :] = np.nan
            d2[:, hmask] = np.nan
            fin = np.isfinite(d2)
            if fin.any():
                L = 2 * min(nO, nH) * (d2[fin].max() + 1) + 1
                cost = np.where(fin, d2, L)
                for i, j in zip(*linear_sum_assignment(cost)):
                    if not fin[i, j]:
                        continue
                    o, h = int(oids[i]), int(hids[j])
                    if o in m and m[o] != h:
                        c['switches'] += 1
                    c['matches'] += 1
                    matched_d[i] = float(d2[i, j])
                    hmask[j] = True
                    m[o] = h
                    last_match[o] = t
        for i in range(nO):
            if matched_d[i] is None:
                c['misses'] += 1
            else:
                dist_sum += matched_d[i]
        c['false_positives'] += int(nH - hmask.sum())
        if on_frame is not None:
            on_frame(t, oids, [md is not None for md in matched_d])
    c['dist_sum'] = float(dist_sum)
    return c, (det_frame, det_box, tracks, gt_frame, gt_track, gt_box, t0, nframes)


def mot_events_host(det_frame, det_box, tracks, gt_frame, gt_track, gt_box) -> Dict:
    """The CLEAR-MOT events of one sequence.  det_box / gt_box float32 [n, 4] (x1 y1 x2 y2); tracks = y_out[:, 1] in arrival
    order; rows with tracks < 0 or gt_track < 0 take no part (metrics.py:28,32).  Per frame of the common range: keep the
    correspondences of the previous frame (step 1), assign the rest optimally (step 2), count."""
    return _derived(_mot_walk(det_frame, det_box, tracks, gt_frame, gt_track, gt_box)[0])


def mot_summary_host(det_frame, det_box, tracks, gt_frame, gt_track, gt_box) -> Dict:
    """Everything mot_events_host returns plus the rest of the MOT-challenge summary (metrics.py:47-61), as py-motmetrics
    >= 1.2 defines it.  Over the objects O = the GT ids >= 0 and the hypotheses = the distinct tracks >= 0:

        coverage        an object has one event per frame it is in the GT, tracked (matched by the walk) or miss;
                        mostly_tracked: tracked / present >= 0.8 (float64), mostly_lost: < 0.2, partially_tracked: the rest
        fragmentations  per object the transitions tracked -> miss between its first and its last tracked event (= maximal
                        tracked runs - 1; frames without the object are no events), summed
        identity        n[o][h] = the frames in which both are present at a finite mot_dist, whatever the walk matched;
                        idtp = the largest sum of n over one-to-one matchings of objects and hypotheses, idfn = objects - idtp,
                        idfp = predictions - idtp, idp, idr, idf1 = 2 idtp / (objects + predictions)
    """
    from scipy.optimize import linear_sum_assignment
    present: Dict[int, int] = {}
    tracked: Dict[int, int] = {}
    state: Dict[int, int] = {}                                    # 0 never tracked, 1 last event tracked, 2 missed after tracked
    frag = [0]

    def on_frame(t, oids, hit):
        for o, h in zip(oids.tolist(), hit):
            present[o] = present.get(o, 0) + 1
            st = state.get(o, 0)
            if h:
                tracked[o] = tracked.get(o, 0) + 1
                frag[0] += st == 2
                state[o] = 1
            else:
                state[o] = 2 if st == 1 else st
    c, (det_frame, det_box, tracks, gt_frame, gt_track, gt_box, t0, nframes) = _mot_walk(
        det_frame, det_box, tracks, gt_frame, gt_track, gt_box, on_frame)
    ratio = [np.float64(tracked.get(o, 0)) / np.float64(n) for o, n in present.items()]
    c['unique_objects'] = len(present)
    c['mostly_tracked'] = sum(1 for r in ratio if r >= 0.8)
    c['partially_tracked'] = sum(1 for r in ratio if 0.2 <= r < 0.8)
    c['mostly_lost'] = sum(1 for r in ratio if r < 0.2)
    c['fragmentations'] = int(frag[0])
    oid = {o: i for i, o in enumerate(sorted(present))}
    hid = {h: j for j, h in enumerate(np.unique(tracks[tracks >= 0]).tolist())}
    n = np.zeros((len(oid), len(hid)), np.int64)
    for t in range(t0, t0 + nframes):
        orow = np.where((gt_frame == t) & (gt_track >= 0))[0]
        hrow = np.where((det_frame == t) & (tracks >= 0))[0]
        if orow.size and hrow.size:
            fin = np.isfinite(mot_dist_host(gt_box[orow], det_box[hrow]))
            for i, j in zip(*np.nonzero(fin)):
                n[oid[int(gt_track[orow[i]])], hid[int(tracks[hrow[j]])]] += 1
    idtp = int(n[linear_sum_assignment(n, maximize=True)].sum()) if n.size else 0
    c['idtp'] = idtp
    return _derived(c)


def synth_mot_sequence(seed: int, frames: int, objects: int = 6, p_absent: float = 0.05, p_miss: float = 0.15,
                       stray_rate: float = 0.18, p_swap: float = 0.06, p_untracked: float = 0.05, t0: int = 0,
                       shuffle_gt: bool = True) -> Dict:
    """A synthetic sequence for the tests and tools/mot_eval_bench.py: `objects` boxes drifting over a 1000 x 1000 field,
    every one absent from the ground truth of a frame with p_absent and undetected with p_miss; detections are jittered
    boxes that carry the object's hypothesis id (two ids swap or one is renewed with p_swap per frame; -1 with
    p_untracked); stray detections with fresh ids at `stray_rate` per frame.  GT ids are not dense and the GT rows come
    in shuffled order.  Returns the dict MotEvaluator takes plus 'tracks'."""
    rng = np.random.default_rng(seed)
    pos, vel = rng.uniform(100, 900, (objects, 2)), rng.uniform(-4, 4, (objects, 2))
    size = rng.uniform(30, 80, (objects, 2))
    hyp = np.arange(objects) + 100
    nxt = 100 + objects
    gt, det = [], []
    for t in range(frames):
        if objects >= 2 and rng.random() < p_swap:
            a, b = rng.choice(objects, 2, replace=False)
            hyp[a], hyp[b] = hyp[b], hyp[a]
        if objects and rng.random() < p_swap:
            hyp[rng.integers(objects)] = nxt
            nxt += 1
        for o in range(objects):
            c = pos[o] + vel[o] * t
            box = np.concatenate([c - size[o] / 2, c + size[o] / 2])
            if rng.random() >= p_absent:
                gt.append((t0 + t, 3 * o + 1, *box))
            if rng.random() >= p_miss:
                det.append((t0 + t, hyp[o] if rng.random() >= p_untracked else -1, *(box + rng.normal(0, 2, 4))))
        for _ in range(rng.poisson(stray_rate)):
            c, sz = rng.uniform(100, 900, 2), rng.uniform(30, 80, 2)
            det.append((t0 + t, nxt, *np.concatenate([c - sz / 2, c + sz / 2])))
            nxt += 1
    gt = np.asarray(gt, np.float64).reshape(-1, 6)
    det = np.asarray(det, np.float64).reshape(-1, 6)
    if shuffle_gt:
        gt = gt[rng.permutation(gt.shape[0])]
    return {'det_frame': det[:, 0].astype(np.int64), 'det_box': det[:, 2:].astype(np.float32), 'tracks': det[:, 1].astype(np.int64),
            'gt_frame': gt[:, 0].astype(np.int64), 'gt_track': gt[:, 1].astype(np.int64), 'gt_box': gt[:, 2:].astype(np.float32)}


def sequence_from_counts(counts, hyp_ids=None, t0: int = 0) -> Dict:
    """A sequence whose identity count matrix is `counts` [objects, hypotheses], for the tests: object o stands at a fixed box far
    from the others; for every pair with counts[o][h] = c > 0 there are c dedicated frames whose GT holds only o and whose
    detections hold only h, at o's box.  So n[o][h] = counts[o][h] and idtp is the maximum-weight matching of `counts`.  Frames run
    from t0 in row-major order of the pairs; hyp_ids: the track id of every column (default 100 + h).  The dict MotEvaluator
    takes plus 'tracks'."""
    counts = np.asarray(counts, np.int64)
    hyp_ids = np.arange(counts.shape[1]) + 100 if hyp_ids is None else np.asarray(hyp_ids, np.int64)
    o, h = np.nonzero(counts)
    rep = counts[o, h]
    o, h = np.repeat(o, rep), np.repeat(h, rep)
    frame = t0 + np.arange(o.shape[0], dtype=np.int64)
    box = np.stack([200.0 * o, np.zeros(o.shape[0]), 200.0 * o + 50, np.full(o.shape[0], 50.0)], 1).astype(np.float32)
    return {'det_frame': frame, 'det_box': box, 'tracks': hyp_ids[h], 'gt_frame': frame.copy(), 'gt_track': 3 * o + 1, 'gt_box': box.copy()}


class MotStore:
    """What the evaluator keeps of S sequences, packed: rows of both sides sorted STABLY by frame, per-frame offsets over the
    common frame range (relative to the sequence's first row), GT ids renumbered densely per sequence (ascending original
    id), the permutation sorted position -> arrival index of the detections, float32 boxes.  GT rows with a negative track
    are dropped; a GT id twice in a frame raises ValueError.  All host numpy arrays:

        seq      int64 [S, 8]   gt_base, n_gt, det_base, n_det, off_base, n_frames, obj_base, n_obj
        gt_off   int32 [n_off]  per sequence n_frames + 1 entries; det_off likewise
        gt_id    int32 [n_gt]   gt_box float32 [n_gt, 4]   det_box float32 [n_det, 4]   det_perm int32 [n_det]
        t0       first frame of each sequence's range (host only)
    """

    def __init__(self, sequences: Sequence[Dict]):
        self.S = len(sequences)
        self.t0: List[int] = []
        self.empty: List[bool] = []
        self.gt_ids: List[np.ndarray] = []                        # dense id -> original id, per sequence
        tab = SeqTable('MotStore', self.S)
        for s, q in enumerate(sequences):
            det_frame, gt_frame = _ints(q['det_frame'], 'det_frame'), _ints(q['gt_frame'], 'gt_frame')
            gt_track = _ints(q['gt_track'], 'gt_track', gt_frame.shape[0])
            db, gb = _boxes(q['det_box'], 'det_box'), _boxes(q['gt_box'], 'gt_box')
            if db.shape[0] != det_frame.shape[0] or gb.shape[0] != gt_frame.shape[0]:
                raise ValueError(f'MotStore: sequence {s}: one box per row expected')
            t0, nf = _frame_range(det_frame, gt_frame)
            self.empty.append(det_frame.shape[0] == 0 or gt_frame.shape[0] == 0)
            tab.check(s, nf, max(det_frame.shape[0], gt_frame.shape[0]))
            go, g_off = frame_sort(gt_frame, t0, nf, np.where(gt_track >= 0)[0])
            do, d_off = frame_sort(det_frame, t0, nf)
            uniq, dense = np.unique(gt_track[go], return_inverse=True)
            if uniq.size and uniq.max() >= 2 ** 31:
                raise ValueError(f'MotStore: sequence {s}: ids are int32')
            key = gt_frame[go] * (int(uniq.shape[0]) + 1) + dense.reshape(-1)
            if np.unique(key).shape[0] != key.shape[0]:
                k, cnt = np.unique(key, return_counts=True)
                raise ValueError(f'MotStore: sequence {s}: a GT id occurs twice in frame {int(k[cnt > 1][0] // (uniq.shape[0] + 1))}')
            tab.add(s, go.shape[0], do.shape[0], nf, uniq.shape[0], gt_off=g_off, det_off=d_off, gt_id=dense.reshape(-1),
                    gt_box=gb[go], det_box=db[do], det_perm=do)
            self.t0.append(t0)
            self.gt_ids.append(uniq)
        self.seq = tab.seq
        for k in ('gt_off', 'det_off', 'gt_id', 'det_perm'):
            setattr(self, k, tab.pack(k, np.int32))
        self.gt_box, self.det_box = tab.pack('gt_box', np.float32, (4,)), tab.pack('det_box', np.float32, (4,))
        self.n_gt, self.n_det, self.n_off, self.n_obj = tab.totals


def _attach_mot_store(ev: SequenceEvaluator, st: MotStore) -> None:
    """The store on the device for `ev` (MotEvaluator, HotaEvaluator), with the struct tmpnn_mot_store over it."""
    names = ('seq', 'gt_off', 'det_off', 'gt_id', 'gt_box', 'det_box', 'det_perm')
    ev._c = _lib.CMotStore(st.S, 0, st.n_gt, st.n_det, st.n_off, st.n_obj, *ev._attach(st, names))


RECORD_WORDS = 9               # struct tmpnn_mot_record: seven int64 counts, the flag word, dist_sum (double)
SUMMARY_WORDS = 16             # struct tmpnn_mot_summary_record: the same, then SUMMARY_KEYS, idtp, hypotheses


class MotEvaluator(SequenceEvaluator):
    """The MOT evaluation of S sequences on the device.  sequences: one dict per sequence with det_frame, det_box, gt_frame,
    gt_track, gt_box (host arrays or tensors; they are the same in every epoch -- only the tracks change).  The store is
    built on the host and uploaded once.

        ev.evaluate(tracks)   tracks: per sequence an int tensor / array [n_det] in arrival order, host or device (None:
                              the sequence takes no part in this evaluation).  One packed upload at the most, one launch, no
                              host wait.
        ev.read()             the one device -> host copy: (per_sequence, overall); per_sequence[i] is the dict of
                              mot_events_host (None for a sequence left out), overall the ratios of the summed counts.
                              RuntimeError when a sequence's flag word is set (check=False: no error, every dict has
                              the sequence's 'flag' word instead; a flagged sequence's counts stop at the flagged frame).

    identity=True: the whole MOT-challenge summary.  evaluate enqueues tmpnn_mot_summary (one clear and four launches, whatever
    the number of sequences; still one packed upload and no host wait) and the dicts are those of mot_summary_host: track
    coverage, fragmentations, idtp / idfp / idfn / idp / idr / idf1 as well (a flagged sequence read with check=False has no
    identity figures, and then neither has the overall dict).  The count matrices take objects x detections int32 per sequence
    in the workspace: a store beyond MAX_PAIR_COUNTS entries raises ValueError (score it with mot_summary_host).
    """
    FLAG_WORD, FLAG_TEXT = 7, _FLAG_TEXT

    def __init__(self, sequences: Sequence[Dict], device='cuda:0', identity: bool = False):
        super().__init__(device, 'score on the host with mot_events_host')
        self.identity = bool(identity)
        st = MotStore(sequences)
        self._n_pair = int((st.seq[:, 7] * st.seq[:, 3]).sum())
        if self.identity and self._n_pair > MAX_PAIR_COUNTS:
            raise ValueError(f'MotEvaluator(identity=True): the identity count matrices (objects x detections per sequence) have '
                             f'{self._n_pair} entries, more than MAX_PAIR_COUNTS = {MAX_PAIR_COUNTS}: score such a set on the host '
                             'with mot_summary_host')
        _attach_mot_store(self, st)
        lib = _lib.load()
        self._workspace(lib.tmpnn_mot_summary_ws(st.S, st.n_obj, st.n_det, self._n_pair) if self.identity else
                        lib.tmpnn_mot_events_ws(st.S, st.n_obj, st.n_det))
        self._out = torch.zeros(max(st.S, 1), SUMMARY_WORDS if self.identity else RECORD_WORDS, dtype=torch.int64, device=self.device)

    def evaluate(self, tracks: Sequence) -> None:
        self._enqueue('tmpnn_mot_summary' if self.identity else 'tmpnn_mot_events', tracks, self._ws.data_ptr(), self._ws_bytes,
                      self._out.data_ptr())

    def _row(self, s, rec, fl, out) -> Dict:
        c = {k: int(rec[s, i]) for i, k in enumerate(COUNT_KEYS)}
        c['dist_sum'] = float(fl[s, 8])
        if self.identity:
            c.update({k: int(rec[s, 9 + i]) for i, k in enumerate(SUMMARY_KEYS)})
            if rec[s, 14] >= 0:                                     # (a flagged sequence has no identity figures)
                c['idtp'] = int(rec[s, 14])
        return _derived(c)

    def read(self, check: bool = True):
        per = self._read(check)
        return per, mot_overall([p for p in per if p is not None])

