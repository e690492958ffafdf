"""The KITTI benchmark's preprocessing of a set of tracks, in front of HOTA and the MOT summary.

    PrepRules             the class that is scored, its distractor classes, the ignore category and the thresholds
    evalprep_frame_host   the rule for one frame, in numpy + scipy.  It is the DEFINITION the device kernel must equal exactly.
    evalprep_ioa_host     the float64 intersection-over-own-area of detections against regions
    evalprep_host         the rule over the frames of one sequence
    prep_eval_sequences   the sequences without the ground truth that is not scored (host only)
    synth_prep_sequence   seeded test data: every branch of the rule, and frames of a given shape
    EvalPrepStore         the per-sequence data that do not change between evaluations, frame-sorted, the rules resolved into one
                          code byte a row
    EvalPrep              the store on the device + `apply(tracks)` (tmpnn_evalprep, csrc/evalprep.hip: one clear and one launch
                          whatever the number of sequences) + `filtered_tracks()` + `read()` (the one device -> host copy) +
                          `eval_sequences()` (the ground truth the evaluators are to be built over)

The benchmark does not score the rows it is given.  Before it scores a class, TrackEval's datasets/kitti_2d_box.py
(get_preprocessed_seq_data) matches the tracker's boxes of the class against the ground truth of the class and its distractor
class, removes the boxes matched to a distractor or to a heavily occluded or truncated object, removes the unmatched boxes that
are too small or lie in a DontCare region, and drops the ground truth that is not scored.  The rule below restates that
function.  TrackEval is not a dependency of this library and no fixture pins it: parity with its numbers is by restatement, and
tests/test_evalprep.py pins the rule by hand-computed frames.

The rule, for one frame (evalprep_frame_host):
    tracker rows     the rows with tracks >= 0 and det_cat == cls, in input order.  Every other row gets -1 in tracks_out; a row
                     with a track and another class counts as `other_class`.
    GT rows          of the matching: the rows with gt_cat == cls or gt_cat in distractors, in input order, occluded and
                     truncated ones included.  The ignore regions are the boxes of the rows with gt_cat == ignore_cat.
    scores           score = hota_sim_host(gt_box[rows], det_box[trk]) -- the similarity HotaEvaluator scores with, so the two
                     stages agree on every bit; entries with score < 0.5 - EPS are set to 0; the assignment is
                     linear_sum_assignment(-score) (scipy's own transposition of a tall matrix applies); a pair is matched iff
                     its score is > 0 + EPS.  Only when both sides are non-empty.
    matched rows     a matched tracker row is removed when its GT row is a distractor (`removed_distractor`), else when its GT
                     row has gt_occ > max_occlusion or gt_trunc > max_truncation (`removed_occluded`; integer comparisons).  A
                     matched row that stays is not looked at again.
    unmatched rows   an unmatched tracker row is removed when its height is <= min_height + EPS (`removed_small`; the height is
                     the float32 difference y2 - y1, widened to float64, as hota_sim forms it), else when any ignore region has
                     ioa > 0.5 + EPS (`removed_ignored`).  ioa = evalprep_ioa_host: the intersection by the operations of
                     hota_sim_host in their order, divided by the detection's area (the float64 product of its float32 width
                     and height); 0 where area > EPS is false or the quotient is not finite.
    GT kept          gt_keep = (gt_cat == cls) & (gt_occ <= max_occlusion) & (gt_trunc <= max_truncation).  It does not depend on
                     the tracks.
    counts           rows_in (rows with a track), other_class, the four removal counts and kept: the six parts sum to rows_in.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .evalstore import FLAG_LIMIT, FLAG_SOLVER, FLAG_STORE, SeqTable, SequenceEvaluator, _boxes, _frame_range, _ints, frame_sort
from .hota import EPS, hota_sim_host

MAX_PER_FRAME = 256            # detection rows / GT rows of one frame, all categories, the device kernel takes (csrc/evalprep.hip EP_MAX)
LDS_SCORE = 1024               # frames of up to this many pairs keep the solver's scores in LDS (csrc/evalprep.hip)
FRAMES_PER_GROUP = 8           # frames of one workgroup
COUNT_KEYS = ('rows_in', 'other_class', 'removed_distractor', 'removed_occluded', 'removed_small', 'removed_ignored', 'kept')
RECORD_WORDS = 8               # struct tmpnn_evalprep_record: the seven counts, the flag word
GT_OUT, GT_SCORED, GT_HARD, GT_DISTRACTOR, GT_REGION = 0, 1, 2, 3, 4        # the code byte of a GT row
_FLAG_TEXT = {FLAG_LIMIT: f'a frame has more than {MAX_PER_FRAME} detection rows or GT rows',
              FLAG_STORE: 'the store is inconsistent (an offset or a permutation entry out of range)',
              FLAG_SOLVER: 'the assignment solver found no augmenting path'}
_GT_KEYS = ('gt_frame', 'gt_track', 'gt_cat', 'gt_box', 'gt_occ', 'gt_trunc')


@dataclass(frozen=True)
class PrepRules:
    """cls: the category that is scored; distractors: the categories whose ground truth takes part in the matching and removes
    what it is matched with; ignore_cat: the category of the ignore regions (None: there are none); a GT row of the class with
    gt_occ > max_occlusion or gt_trunc > max_truncation is not scored and removes what it is matched with; an unmatched box of
    height <= min_height (+ eps) is removed."""
    cls: int
    distractors: Tuple[int, ...] = ()
    ignore_cat: Optional[int] = None
    max_occlusion: int = 2
    max_truncation: int = 0
    min_height: float = 25.0

    def __post_init__(self):
        object.__setattr__(self, 'distractors', tuple(int(c) for c in self.distractors))
        if int(self.cls) in self.distractors or (self.ignore_cat is not None and int(self.ignore_cat) in self.distractors + (int(self.cls),)):
            raise ValueError('PrepRules: the class, its distractors and the ignore category must differ')
        if np.isnan(float(self.min_height)):
            raise ValueError('PrepRules: min_height is NaN')


# the reference's GT category ids (dataset/kitti_mot.py:263): Pedestrian 1, Car 2, Cyclist 3, Van 4, Truck 5, Person 6, Tram 7,
# Misc 8, DontCare 9
KITTI_CAR = PrepRules(2, (4,), 9)
KITTI_PEDESTRIAN = PrepRules(1, (6,), 9)


def evalprep_ioa_host(det_box, region_box) -> np.ndarray:
    """[len(det_box), len(region_box)] float64: intersection over the detection's own area -- the intersection by the operations
    of hota_sim_host in their order (widths and heights in float32, everything after in float64), the area the float64 product
    of the detection's float32 width and height; 0.0 where area > EPS is false or the quotient is not finite."""
    bd, br = _boxes(det_box, 'det_box'), _boxes(region_box, 'region_box')
    tl_d, tl_r = bd[:, :2].astype(np.float64), br[:, :2].astype(np.float64)
    wh_d, wh_r = (bd[:, 2:] - bd[:, :2]).astype(np.float64), (br[:, 2:] - br[:, :2]).astype(np.float64)
    br_d, br_r = tl_d + wh_d, tl_r + wh_r
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        iwh = np.maximum(np.minimum(br_d[:, None, :], br_r[None, :, :]) - np.maximum(tl_d[:, None, :], tl_r[None, :, :]), 0)
        inter = iwh[..., 0] * iwh[..., 1]
        area = np.broadcast_to((wh_d[:, 0] * wh_d[:, 1])[:, None], inter.shape)
        ioa = inter / area
        ioa[~(area > EPS) | ~np.isfinite(ioa)] = 0.0
    return ioa


def _gt_codes(gt_cat: np.ndarray, gt_occ: np.ndarray, gt_trunc: np.ndarray, rules: PrepRules) -> np.ndarray:
    """The code byte of every GT row (GT_OUT .. GT_REGION): the rules, resolved."""
    code = np.zeros(gt_cat.shape[0], np.uint8)
    is_cls = gt_cat == int(rules.cls)
    hard = (gt_occ > int(rules.max_occlusion)) | (gt_trunc > int(rules.max_truncation))
    code[is_cls & ~hard] = GT_SCORED
    code[is_cls & hard] = GT_HARD
    code[np.isin(gt_cat, np.asarray(rules.distractors, np.int64))] = GT_DISTRACTOR
    if rules.ignore_cat is not None:
        code[gt_cat == int(rules.ignore_cat)] = GT_REGION
    return code


def evalprep_frame_host(det_cat, det_box, tracks, gt_cat, gt_box, gt_occ, gt_trunc, rules: PrepRules):
    """The rule for one frame (see the module text).  det_cat [n], det_box float32 [n, 4] (x1 y1 x2 y2), tracks [n] (negative:
    no track); gt_cat, gt_occ, gt_trunc [m] integers, gt_box float32 [m, 4].  Returns (tracks_out int64 [n], gt_keep bool [m],
    counts: a dict over COUNT_KEYS).  No limit on the size of a frame."""
    from scipy.optimize import linear_sum_assignment
    det_cat = _ints(det_cat, 'det_cat')
    tracks = _ints(tracks, 'tracks', det_cat.shape[0])
    gt_cat = _ints(gt_cat, 'gt_cat')
    gt_occ, gt_trunc = _ints(gt_occ, 'gt_occ', gt_cat.shape[0]), _ints(gt_trunc, 'gt_trunc', gt_cat.shape[0])
    det_box, gt_box = _boxes(det_box, 'det_box'), _boxes(gt_box, 'gt_box')
    if det_box.shape[0] != det_cat.shape[0] or gt_box.shape[0] != gt_cat.shape[0]:
        raise ValueError('evalprep_frame_host: one box per row expected')
    code = _gt_codes(gt_cat, gt_occ, gt_trunc, rules)
    trk = np.where((tracks >= 0) & (det_cat == int(rules.cls)))[0]
    rows = np.where((code >= GT_SCORED) & (code <= GT_DISTRACTOR))[0]
    regions = gt_box[code == GT_REGION]
    counts = {k: 0 for k in COUNT_KEYS}
    counts['rows_in'] = int((tracks >= 0).sum())
    counts['other_class'] = counts['rows_in'] - int(trk.shape[0])
    tracks_out = np.full(tracks.shape[0], -1, np.int64)
    match = np.full(trk.shape[0], -1, np.int64)                       # the GT row (position in `rows`) of a tracker row
    if rows.size and trk.size:
        score = hota_sim_host(gt_box[rows], det_box[trk])
        score[score < 0.5 - EPS] = 0
        ri, ci = linear_sum_assignment(-score)
        ok = score[ri, ci] > 0 + EPS
        match[ci[ok]] = ri[ok]
    height = (det_box[trk, 3] - det_box[trk, 1]).astype(np.float64)   # (a float32 difference, widened)
    ioa = evalprep_ioa_host(det_box[trk], regions)
    for j in range(trk.shape[0]):
        if match[j] >= 0:
            c = code[rows[match[j]]]
            fate = 'removed_distractor' if c == GT_DISTRACTOR else 'removed_occluded' if c == GT_HARD else 'kept'
        elif height[j] <= float(rules.min_height) + EPS:
            fate = 'removed_small'
        elif bool((ioa[j] > 0.5 + EPS).any()):
            fate = 'removed_ignored'
        else:
            fate = 'kept'
        counts[fate] += 1
        if fate == 'kept':
            tracks_out[trk[j]] = tracks[trk[j]]
    return tracks_out, code == GT_SCORED, counts


def _sequence_arrays(q: Dict, who: str) -> Dict:
    a = {'det_frame': _ints(q['det_frame'], 'det_frame'), 'gt_frame': _ints(q['gt_frame'], 'gt_frame')}
    nd, ng = a['det_frame'].shape[0], a['gt_frame'].shape[0]
    a['det_cat'] = _ints(q['det_cat'], 'det_cat', nd)
    for k in ('gt_cat', 'gt_occ', 'gt_trunc'):
        a[k] = _ints(q[k], k, ng)
    a['det_box'], a['gt_box'] = _boxes(q['det_box'], 'det_box'), _boxes(q['gt_box'], 'gt_box')
    if a['det_box'].shape[0] != nd or a['gt_box'].shape[0] != ng:
        raise ValueError(f'{who}: one box per row expected')
    return a


def evalprep_host(seq: Dict, tracks, rules: PrepRules):
    """evalprep_frame_host over the frames of one sequence.  seq: a dict with det_frame, det_cat, det_box, gt_frame, gt_track,
    gt_cat, gt_box, gt_occ, gt_trunc; tracks [n_det] in arrival order.  The frame range is the union of both sides' frames.
    Returns (tracks_out int64 [n_det], gt_keep bool [n_gt], counts), rows in arrival order, the counts summed over the frames."""
    a = _sequence_arrays(seq, 'evalprep_host')
    tracks = _ints(tracks, 'tracks', a['det_frame'].shape[0])
    t0, nframes = _frame_range(a['det_frame'], a['gt_frame'])
    tracks_out = np.full(tracks.shape[0], -1, np.int64)
    gt_keep = np.zeros(a['gt_frame'].shape[0], bool)
    counts = {k: 0 for k in COUNT_KEYS}
    for t in range(t0, t0 + nframes):
        d, g = np.where(a['det_frame'] == t)[0], np.where(a['gt_frame'] == t)[0]
        out, keep, c = evalprep_frame_host(a['det_cat'][d], a['det_box'][d], tracks[d], a['gt_cat'][g], a['gt_box'][g], a['gt_occ'][g],
                                           a['gt_trunc'][g], rules)
        tracks_out[d], gt_keep[g] = out, keep
        for k in COUNT_KEYS:
            counts[k] += c[k]
    return tracks_out, gt_keep, counts


def prep_eval_sequences(sequences: Sequence[Dict], rules: PrepRules) -> List[Dict]:
    """The sequences with the GT rows outside gt_keep dropped (every gt_* column; the other entries as they are): the ground
    truth the benchmark scores for the class, what MotEvaluator / HotaEvaluator are to be built over.  Host only."""
    out = []
    for q in sequences:
        r = dict(q)
        v = {k: (q[k].detach().cpu().numpy() if isinstance(q[k], torch.Tensor) else np.asarray(q[k])) for k in _GT_KEYS}
        keep = _gt_codes(_ints(v['gt_cat'], 'gt_cat'), _ints(v['gt_occ'], 'gt_occ'), _ints(v['gt_trunc'], 'gt_trunc'), rules) == GT_SCORED
        for k in _GT_KEYS:
            r[k] = v[k].reshape(-1, 4)[keep] if k == 'gt_box' else v[k].reshape(-1)[keep]
        out.append(r)
    return out


def prep_overall(per_sequence: Sequence[Optional[Dict]]) -> Dict:
    """The counts summed over the sequences that took part."""
    return {k: sum(int(p[k]) for p in per_sequence if p is not None) for k in COUNT_KEYS}


def synth_prep_sequence(seed: int, frames: int, objects: int = 6, distractors: int = 2, others: int = 2, regions: int = 2,
                        rules: PrepRules = KITTI_CAR, other_cat: int = 3, p_absent: float = 0.05, p_miss: float = 0.1,
                        p_hard: float = 0.2, p_untracked: float = 0.08, p_wrong: float = 0.08, stray_rate: float = 0.9,
                        sigma: float = 2.0, t0: int = 0, shuffle: bool = False, sizes: Optional[Sequence[Tuple[int, int]]] = None) -> Dict:
    """A seeded synthetic sequence for the tests and tools/time_evalprep.py (an EvalPrep dict plus 'tracks'): `objects` boxes of
    the class, `distractors` of the distractor classes and `others` of other_cat drift over a 1000 x 1000 field, every one
    absent from a frame's ground truth with p_absent; a row is heavily occluded (gt_occ 3) or truncated (gt_trunc 1) with
    p_hard; `regions` fixed ignore regions have a GT row in every frame (track -1, flags -1).  Every present box is detected
    unless p_miss: a copy jittered by `sigma` pixels that carries the object's hypothesis id (-1 with p_untracked) and the class
    (other_cat for the others; with p_wrong the other of the two).  Stray hypotheses at `stray_rate` per frame with fresh ids:
    in turn inside a region, lower than 25 px, and anywhere.  shuffle: both sides in shuffled arrival order.
    sizes: per frame (matching GT rows, hypotheses) in place of the random presence (`frames` is then their number): the first
    boxes of the class and the distractors are present, hypothesis k copies box k modulo their number (anywhere, without one)
    under the id 100 + k, and there are no strays."""
    rng = np.random.default_rng([int(seed), 2718])
    if sizes is not None:
        frames = len(sizes)
        if max([0] + [int(g) for g, _ in sizes]) > objects + distractors:
            raise ValueError('synth_prep_sequence: sizes asks for more matching GT rows than objects + distractors')
    dis = rules.distractors or (int(rules.cls),)
    cat = np.asarray([int(rules.cls)] * objects + [int(dis[i % len(dis)]) for i in range(distractors)] + [int(other_cat)] * others, np.int64)
    if sizes is not None:                                             # (the class and its distractors interleaved: both in every prefix)
        head = np.argsort(np.concatenate([np.arange(objects) * max(distractors, 1), np.arange(distractors) * max(objects, 1) + 0.5]), kind='stable')
        cat[:objects + distractors] = cat[:objects + distractors][head]
    E = cat.shape[0]
    pos, vel = rng.uniform(100, 900, (E, 2)), rng.uniform(-3, 3, (E, 2))
    size = rng.uniform(30, 90, (E, 2))
    reg = np.zeros((regions, 4))
    if regions:
        c, wh = rng.uniform(150, 850, (regions, 2)), rng.uniform(100, 200, (regions, 2))
        reg = np.concatenate([c - wh / 2, c + wh / 2], 1)
    nxt, n_stray = 100000, 0
    gt, det = [], []                                                  # (frame, track, cat, occ, trunc, box) / (frame, track, cat, box)
    flip = lambda c: int(other_cat) if c == int(rules.cls) else int(rules.cls)
    for t in range(int(frames)):
        centre = pos + vel * t
        box = np.concatenate([centre - size / 2, centre + size / 2], 1)
        if sizes is None:
            present = [e for e in range(E) if rng.random() >= p_absent]
        else:
            present = list(range(int(sizes[t][0]))) + list(range(objects + distractors, E))
        for e in present:
            hard = rng.random() < p_hard
            occ, trunc = (3, 0) if hard and rng.random() < 0.5 else (int(rng.integers(0, 3)), 1 if hard else 0)
            gt.append((t0 + t, 3 * e + 1, cat[e], occ, trunc, *box[e]))
        for k in range(regions):
            gt.append((t0 + t, -1, int(rules.ignore_cat) if rules.ignore_cat is not None else int(other_cat), -1, -1, *reg[k]))
        if sizes is None:
            for e in present:
                if rng.random() < p_miss:
                    continue
                c = int(other_cat) if cat[e] == int(other_cat) else int(rules.cls)
                det.append((t0 + t, 100 + e if rng.random() >= p_untracked else -1, flip(c) if rng.random() < p_wrong else c,
                            *(box[e] + rng.normal(0, sigma, 4))))
            for _ in range(rng.poisson(stray_rate)):
                kind = n_stray % 3
                n_stray += 1
                if kind == 0 and regions:
                    r = reg[int(rng.integers(regions))]
                    wh = rng.uniform(30, 60, 2)
                    c = rng.uniform(r[:2] + wh / 2 - 10, r[2:] - wh / 2 + 10)
                elif kind == 1:
                    c, wh = rng.uniform(100, 900, 2), np.asarray([rng.uniform(30, 80), rng.uniform(8, 25)])
                else:
                    c, wh = rng.uniform(100, 900, 2), rng.uniform(30, 80, 2)
                det.append((t0 + t, nxt, int(rules.cls), *np.concatenate([c - wh / 2, c + wh / 2])))
                nxt += 1
        else:
            G = int(sizes[t][0])
            for k in range(int(sizes[t][1])):
                if G:
                    b = box[k % G] + rng.normal(0, sigma, 4)
                else:
                    c, wh = rng.uniform(100, 900, 2), rng.uniform(30, 80, 2)
                    b = np.concatenate([c - wh / 2, c + wh / 2])
                det.append((t0 + t, 100 + k if rng.random() >= p_untracked else -1, flip(int(rules.cls)) if rng.random() < p_wrong else int(rules.cls), *b))
    gt = np.asarray(gt, np.float64).reshape(-1, 9)
    det = np.asarray(det, np.float64).reshape(-1, 7)
    if shuffle:
        gt, det = gt[rng.permutation(gt.shape[0])], det[rng.permutation(det.shape[0])]
    i64 = lambda a: a.astype(np.int64)
    return {'det_frame': i64(det[:, 0]), 'tracks': i64(det[:, 1]), 'det_cat': i64(det[:, 2]), 'det_box': det[:, 3:].astype(np.float32),
            'gt_frame': i64(gt[:, 0]), 'gt_track': i64(gt[:, 1]), 'gt_cat': i64(gt[:, 2]), 'gt_occ': i64(gt[:, 3]), 'gt_trunc': i64(gt[:, 4]),
            'gt_box': gt[:, 5:].astype(np.float32)}


class EvalPrepStore:
    """What EvalPrep keeps of S sequences, packed (host numpy arrays; struct tmpnn_evalprep_store, include/tmpnn.h): rows of both
    sides sorted STABLY by frame, EVERY row kept, per-frame offsets over the union frame range, the rules resolved into a byte:

        seq       int64 [S, 8]   gt_base, n_gt, det_base, n_det, off_base, n_frames, 0, 0
        gt_off    int32 [n_off]  per sequence n_frames + 1 entries, relative to the sequence's first row; det_off likewise
        gt_code   uint8 [n_gt]   GT_OUT / GT_SCORED / GT_HARD / GT_DISTRACTOR / GT_REGION     det_code uint8 [n_det]  1 iff det_cat == cls
        gt_box    float32 [n_gt, 4]   det_box float32 [n_det, 4]   det_perm int32 [n_det]  sorted position -> arrival index
        gt_keep   per sequence, bool in arrival order: the GT rows that are scored (host only); t0: first frame (host only)
    """

    def __init__(self, sequences: Sequence[Dict], rules: PrepRules):
        self.S, self.rules = len(sequences), rules
        self.t0: List[int] = []
        self.gt_keep: List[np.ndarray] = []
        tab = SeqTable('EvalPrepStore', self.S)
        for s, q in enumerate(sequences):
            a = _sequence_arrays(q, f'EvalPrepStore: sequence {s}')
            t0, nf = _frame_range(a['det_frame'], a['gt_frame'])
            nd, ng = a['det_frame'].shape[0], a['gt_frame'].shape[0]
            tab.check(s, nf, max(nd, ng))
            code = _gt_codes(a['gt_cat'], a['gt_occ'], a['gt_trunc'], rules)
            go, g_off = frame_sort(a['gt_frame'], t0, nf)
            do, d_off = frame_sort(a['det_frame'], t0, nf)
            tab.add(s, ng, nd, nf, gt_off=g_off, det_off=d_off, gt_code=code[go], det_code=a['det_cat'][do] == int(rules.cls),
                    gt_box=a['gt_box'][go], det_box=a['det_box'][do], det_perm=do)
            self.t0.append(t0)
            self.gt_keep.append(code == GT_SCORED)
        self.seq = tab.seq
        self.gt_off, self.det_off, self.det_perm = (tab.pack(k, np.int32) for k in ('gt_off', 'det_off', 'det_perm'))
        self.gt_code, self.det_code = tab.pack('gt_code', np.uint8), tab.pack('det_code', np.uint8)
        self.gt_box, self.det_box = tab.pack('gt_box', np.float32, (4,)), tab.pack('det_box', np.float32, (4,))
        self.n_gt, self.n_det, self.n_off, _ = tab.totals


class EvalPrep(SequenceEvaluator):
    """The benchmark's preprocessing of S sequences on the device.  sequences: one dict per sequence with det_frame, det_cat,
    det_box, gt_frame, gt_track, gt_cat, gt_box, gt_occ, gt_trunc (the same in every epoch -- only the tracks change); rules: a
    PrepRules (KITTI_CAR, KITTI_PEDESTRIAN).  The store is built on the host and uploaded once.

        ep.apply(tracks)        tracks: per sequence an int tensor / array [n_det] in arrival order, host or device (None: the
                                sequence is left out).  One packed upload at the most, one clear and one launch whatever the
                                number of sequences, no host wait.
        ep.filtered_tracks()    per sequence a device view, int32 [n_det] in arrival order: the ids after the preprocessing (-1
                                where the row had no track, another class, or was removed), for MotEvaluator / HotaEvaluator
                                .evaluate without a host trip (valid until the next apply)
        ep.read()               the one device -> host copy: (per_sequence, overall); per_sequence[i] is the count dict of
                                evalprep_host (None for a sequence left out), overall their sum.  RuntimeError naming sequence
                                and frame when a flag word is set (check=False: no error, every dict has the sequence's 'flag'
                                word instead; a flagged sequence's counts and tracks are not to be used).
        ep.eval_sequences()     host only: the sequences with the GT rows outside gt_keep dropped -- what MotEvaluator /
                                HotaEvaluator are to be built over, so that they score what the benchmark scores.

    tracks_out and every count equal evalprep_host.  A frame takes at most MAX_PER_FRAME detection rows and as many GT rows, all
    categories (beyond: FLAG_LIMIT for that sequence only; the host definition has no limit)."""

    STEP, FLAG_WORD, FLAG_TEXT = ('apply', 'apply'), 7, _FLAG_TEXT

    def __init__(self, sequences: Sequence[Dict], rules: PrepRules = KITTI_CAR, device='cuda:0'):
        super().__init__(device, 'filter on the host with evalprep_host')
        self.rules = rules
        self._sequences = list(sequences)
        st = EvalPrepStore(sequences, rules)
        names = ('seq', 'gt_off', 'det_off', 'gt_code', 'det_code', 'gt_box', 'det_box', 'det_perm')
        self._c = _lib.CEvalPrepStore(st.S, 0, st.n_gt, st.n_det, st.n_off, float(rules.min_height) + EPS, *self._attach(st, names))
        self._filtered = torch.full((max(st.n_det, 1),), -1, dtype=torch.int32, device=self.device)
        self._out = torch.zeros(max(st.S, 1), RECORD_WORDS, dtype=torch.int64, device=self.device)

    def apply(self, tracks: Sequence) -> None:
        self._enqueue('tmpnn_evalprep', tracks, self._filtered.data_ptr(), self._out.data_ptr())

    def filtered_tracks(self) -> List[torch.Tensor]:
        return self._views(self._filtered)

    def _row(self, s, rec, fl, out) -> Dict:
        return {k: int(rec[s, i]) for i, k in enumerate(COUNT_KEYS)}

    def read(self, check: bool = True):
        per = self._read(check)
        return per, prep_overall(per)

    def eval_sequences(self) -> List[Dict]:
        return prep_eval_sequences(self._sequences, self.rules)
