"""HOTA of a set of tracks against the ground truth (Luiten et al., IJCV 2021; the figure the KITTI tracking benchmark ranks by).

    hota_host           the rule, in numpy + scipy: one sequence in, the record and the derived figures out.  It is the DEFINITION
                        the device kernels must equal: integers exactly, every float64 of the record bit for bit.
    hota_sim_host       the float64 similarity matrix of two box lists (IoU, no cut)
    hota_overall        the figures of several sequences (TrackEval's combine_sequences)
    HotaEvaluator       a MotStore on the device + `evaluate(tracks)` (tmpnn_hota, csrc/hota.hip: one clear and four launches
                        whatever the number of sequences) + `read()` (the one device -> host copy)

The rule restates TrackEval's metrics/hota.py (eval_sequence, combine_sequences, _compute_final_fields).  TrackEval is not a
dependency of this library and no fixture pins it: parity with its numbers is by restatement, and tests/test_hota.py pins the
rule by hand-computed cases.  TrackEval sums floats with np.sum (pairwise, in an order numpy chooses); the rule fixes a
sequential order for every float sum instead, so that a device can equal it exactly.

The rows that are given are scored, as MotEvaluator scores them.  TrackEval's KITTI preprocessing (the class, its distractor
class, occluded and truncated objects, small boxes, DontCare regions) is evalprep.EvalPrep: build the evaluator over
`EvalPrep.eval_sequences()` and hand `EvalPrep.filtered_tracks()` to `evaluate` (or pass `validate(..., prep=ep)`) to score
what the benchmark scores.  It uses hota_sim_host, so the two stages agree on every bit.
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch

from . import _lib
from .evalstore import SequenceEvaluator, _boxes, _frame_range, _ints
from .moteval import _FLAG_TEXT, MotStore, _attach_mot_store, _check_unique

ALPHAS = np.arange(0.05, 0.99, 0.05)           # the 19 localisation thresholds, as numpy produces them
EPS = np.finfo(np.float64).eps
NA = 19
INT_KEYS = ('gt_dets', 'tracker_dets', 'objects', 'hypotheses')
SUM_KEYS = ('loc_sum', 'ass_a_num', 'ass_re_num', 'ass_pr_num')
FIGURES = ('HOTA', 'DetA', 'AssA', 'LocA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'RHOTA')
PAIR_BYTES = 8 + 4 * NA                        # workspace per entry of objects x detections: pm (float64) + mc (19 int32)
MAX_HOTA_PAIRS = 2 ** 31 // PAIR_BYTES         # 25 565 281 entries: the pair workspace alone stays under 2 GiB
MAX_WS_BYTES = 2 ** 31
LDS_SCORE = 1024                               # frames of up to this many pairs keep the solver's scores in LDS (csrc/hota.hip)
FRAMES_PER_GROUP = 8                           # frames of one workgroup of the matching kernel
RECORD_WORDS = 24 + 4 * NA                     # struct tmpnn_hota_record


def hota_sim_host(box_o, box_h) -> np.ndarray:
    """[len(box_o), len(box_h)] float64: IoU of x1 y1 x2 y2 boxes -- inter / union by the operations of mot_dist_host in its
    order (widths and heights in float32, everything after in float64), without a cut; 0.0 where union > 0 is false or the
    quotient is not finite."""
    bo, bh = _boxes(box_o, 'box_o'), _boxes(box_h, 'box_h')
    tl_o, tl_h = bo[:, :2].astype(np.float64), bh[:, :2].astype(np.float64)
    wh_o, wh_h = (bo[:, 2:] - bo[:, :2]).astype(np.float64), (bh[:, 2:] - bh[:, :2]).astype(np.float64)
    br_o, br_h = tl_o + wh_o, tl_h + wh_h
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        iwh = np.maximum(np.minimum(br_o[:, None, :], br_h[None, :, :]) - np.maximum(tl_o[:, None, :], tl_h[None, :, :]), 0)
        inter = iwh[..., 0] * iwh[..., 1]
        union = ((wh_o[:, 0] * wh_o[:, 1])[:, None] + (wh_h[:, 0] * wh_h[:, 1])[None, :]) - inter
        sim = inter / union
        sim[~(union > 0) | ~np.isfinite(sim)] = 0.0
    return sim


def _seq_sum(a: np.ndarray, axis: int) -> np.ndarray:
    """The sum along `axis` in ascending position, one addition after the other (np.sum adds pairwise)."""
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), np.float64)
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def _final_fields(r: Dict) -> Dict:
    """TrackEval's _compute_final_fields on a record that holds tp, gt_dets, tracker_dets, the AssA / AssRe / AssPr and LocA
    arrays: the detection figures, HOTA, RHOTA, the values at alpha = 0.05, and every figure's mean over the alphas."""
    tp = r['tp'].astype(np.float64)
    fn, fp = (r['gt_dets'] - r['tp']).astype(np.float64), (r['tracker_dets'] - r['tp']).astype(np.float64)
    r['fn'], r['fp'] = r['gt_dets'] - r['tp'], r['tracker_dets'] - r['tp']
    r['DetRe'] = tp / np.maximum(1.0, tp + fn)
    r['DetPr'] = tp / np.maximum(1.0, tp + fp)
    r['DetA'] = tp / np.maximum(1.0, tp + fn + fp)
    r['HOTA'] = np.sqrt(r['DetA'] * r['AssA'])
    r['RHOTA'] = np.sqrt(r['DetRe'] * r['AssA'])
    r['HOTA(0)'], r['LocA(0)'] = float(r['HOTA'][0]), float(r['LocA'][0])
    r['HOTALocA(0)'] = r['HOTA(0)'] * r['LocA(0)']
    for k in FIGURES:
        r[k.lower()] = float(np.cumsum(r[k])[-1] / NA)
    return r


def _derived(r: Dict) -> Dict:
    """The figures of one sequence's record (tp, the four float sums, the counts)."""
    tp = r['tp'].astype(np.float64)
    for k, num in (('AssA', 'ass_a_num'), ('AssRe', 'ass_re_num'), ('AssPr', 'ass_pr_num')):
        r[k] = r[num] / np.maximum(1.0, tp)
    r['LocA'] = np.maximum(1e-10, r['loc_sum']) / np.maximum(1e-10, tp)
    return _final_fields(r)


def hota_overall(per_sequence: Sequence[Dict]) -> Dict:
    """The figures over several sequences, as TrackEval's combine_sequences: the integer fields summed, AssA / AssRe / AssPr
    weighted by tp (sum AssA_s tp_s / max(1, sum tp_s)), LocA = max(1e-10, sum LocA_s tp_s) / max(1e-10, sum tp_s), then the
    derived figures.  Host arithmetic on the records, in the order of the list."""
    r = {'tp': np.zeros(NA, np.int64)}
    r.update({k: 0 for k in INT_KEYS})
    w = {k: np.zeros(NA, np.float64) for k in ('AssA', 'AssRe', 'AssPr', 'LocA')}
    for q in per_sequence:
        r['tp'] = r['tp'] + q['tp']
        for k in INT_KEYS:
            r[k] += int(q[k])
        for k in w:
            w[k] = w[k] + q[k] * q['tp'].astype(np.float64)
    tp = r['tp'].astype(np.float64)
    for k in ('AssA', 'AssRe', 'AssPr'):
        r[k] = w[k] / np.maximum(1.0, tp)
    r['LocA'] = np.maximum(1e-10, w['LocA']) / np.maximum(1e-10, tp)
    return _final_fields(r)


def hota_host(det_frame, det_box, tracks, gt_frame, gt_track, gt_box) -> Dict:
    """HOTA of one sequence.  Inputs and row filtering are mot_events_host's: det_box / gt_box float32 [n, 4] (x1 y1 x2 y2),
    tracks = y_out[:, 1] in arrival order, rows with tracks < 0 or gt_track < 0 take no part, the frame range is the common
    one, an id twice in a frame raises ValueError.  No class filtering and no DontCare removal (see the module text).

    Objects are numbered densely by ascending GT id, hypotheses by first appearance in the stably frame-sorted detection rows.
        pass A   per frame, gc[o] += 1 and tc[h] += 1 for everything present; where both sides are present, with sim the
                 similarity matrix of the frame, pm[o, h] += sim / (colsum + rowsum - sim) where that denominator exceeds EPS;
                 afterwards gas = pm / (gc + tc - pm)
        pass B   per frame with both sides one assignment, linear_sum_assignment(-(gas * sim)), whatever the alpha; a matched
                 pair counts at alpha index a iff sim >= ALPHAS[a] - EPS: tp[a] += 1, loc[a] += sim, mc[a][o, h] += 1
        sums     ass_a_num[a] = sum m (m / max(1, gc + tc - m)), ass_re_num with max(1, gc), ass_pr_num with max(1, tc), m = mc[a]
    Every float sum runs in a stated order: row and column sums of sim in ascending position; pm frame by frame; loc per frame
    over the counted pairs in ascending GT position, then over the frames; the association sums per object over the hypotheses
    in ascending index, then over the objects.

    Returns the record -- int64 tp[19], gt_dets, tracker_dets, objects, hypotheses; float64 loc_sum[19], ass_a_num[19],
    ass_re_num[19], ass_pr_num[19] -- and the derived figures: the arrays 'HOTA', 'DetA', 'AssA', 'LocA', 'DetRe', 'DetPr',
    'AssRe', 'AssPr', 'RHOTA' over the alphas, their means under the lower-case names, 'HOTA(0)', 'LocA(0)', 'HOTALocA(0)',
    and fn / fp."""
    from scipy.optimize import linear_sum_assignment
    det_frame, gt_frame = _ints(det_frame, 'det_frame'), _ints(gt_frame, 'gt_frame')
    tracks, gt_track = _ints(tracks, 'tracks', det_frame.shape[0]), _ints(gt_track, 'gt_track', gt_frame.shape[0])
    det_box, gt_box = _boxes(det_box, 'det_box'), _boxes(gt_box, 'gt_box')
    if det_box.shape[0] != det_frame.shape[0] or gt_box.shape[0] != gt_frame.shape[0]:
        raise ValueError('hota_host: one box per row expected')
    t0, nframes = _frame_range(det_frame, gt_frame)
    oid = {o: i for i, o in enumerate(np.unique(gt_track[gt_track >= 0]).tolist())}
    hid: Dict[int, int] = {}
    for k in np.argsort(det_frame, kind='stable'):
        if tracks[k] >= 0:
            hid.setdefault(int(tracks[k]), len(hid))
    nO, nH = len(oid), len(hid)
    gc, tc = np.zeros(nO, np.int64), np.zeros(nH, np.int64)
    pm = np.zeros((nO, nH), np.float64)
    frames = []
    for t in range(t0, t0 + nframes):                                 # pass A
        orow = np.where((gt_frame == t) & (gt_track >= 0))[0]
        hrow = np.where((det_frame == t) & (tracks >= 0))[0]
        _check_unique(gt_track[orow], t, 'a GT')
        _check_unique(tracks[hrow], t, 'a hypothesis')
        o = np.array([oid[int(x)] for x in gt_track[orow]], np.int64)
        h = np.array([hid[int(x)] for x in tracks[hrow]], np.int64)
        gc[o] += 1
        tc[h] += 1
        if o.size == 0 or h.size == 0:
            continue
        sim = hota_sim_host(gt_box[orow], det_box[hrow])
        den = (_seq_sum(sim, 0)[None, :] + _seq_sum(sim, 1)[:, None]) - sim
        sim_iou = np.zeros_like(sim)
        mask = den > 0 + EPS
        sim_iou[mask] = sim[mask] / den[mask]
        pm[o[:, None], h[None, :]] += sim_iou
        frames.append((o, h, sim))
    gas = pm / ((gc[:, None] + tc[None, :]).astype(np.float64) - pm) if pm.size else pm
    tp = np.zeros(NA, np.int64)
    loc = np.zeros(NA, np.float64)
    mc = np.zeros((NA, nO, nH), np.int64)
    for o, h, sim in frames:                                          # pass B
        rows, cols = linear_sum_assignment(-(gas[o[:, None], h[None, :]] * sim))
        order = np.argsort(rows, kind='stable')                       # (ascending GT position)
        for a in range(NA):
            part = 0.0
            for i, j in zip(rows[order], cols[order]):
                if sim[i, j] >= ALPHAS[a] - EPS:
                    tp[a] += 1
                    part += sim[i, j]
                    mc[a, o[i], h[j]] += 1
            loc[a] += part
    r = {'tp': tp, 'gt_dets': int(gc.sum()), 'tracker_dets': int(tc.sum()), 'objects': nO, 'hypotheses': nH, 'loc_sum': loc}
    m = mc.astype(np.float64)
    gcf, tcf = gc.astype(np.float64), tc.astype(np.float64)
    for key, den in (('ass_a_num', (gc[:, None] + tc[None, :]).astype(np.float64)[None] - m), ('ass_re_num', gcf[None, :, None]),
                     ('ass_pr_num', tcf[None, None, :])):
        term = m * (m / np.maximum(1.0, den))
        r[key] = _seq_sum(_seq_sum(term, 2), 1)                       # over the hypotheses of an object, then over the objects
    return _derived(r)


def synth_hota_sequence(seed: int, frames: int, objects: int = 8, **kw) -> Dict:
    """synth_mot_sequence with the detection jitter scaled by a per-row factor in [0, 25] (a fixed generator, whatever the
    seed of the sequence), for the tests and tools/hota_eval_bench.py: matched pairs at every similarity level, so that every one
    of the 19 thresholds separates some of them."""
    from .moteval import synth_mot_sequence
    q = synth_mot_sequence(seed, frames, objects=objects, **kw)
    rng = np.random.default_rng(0)
    n = q['det_box'].shape[0]
    q['det_box'] = (q['det_box'] + rng.normal(0, 1, (n, 4)) * rng.uniform(0, 25, (n, 1))).astype(np.float32)
    return q


class HotaEvaluator(SequenceEvaluator):
    """HOTA of S sequences on the device.  sequences: the dicts MotEvaluator takes (det_frame, det_box, gt_frame, gt_track,
    gt_box; the same in every epoch); the evaluator builds its own MotStore and uploads it once.  The calling contract is
    MotEvaluator's:

        ev.evaluate(tracks)   tracks: per sequence an int tensor / array [n_det] in arrival order, host or device (None: the
                              sequence takes no part).  One packed upload at the most, one clear and four launches whatever
                              the number of sequences, no host wait.
        ev.read()             the one device -> host copy: (per_sequence, overall); per_sequence[i] is the dict of hota_host
                              (None for a sequence left out), overall that of hota_overall.  RuntimeError when a sequence's
                              flag word is set, with the bits of evalstore.py and the messages of moteval.py (check=False:
                              no error, every dict has the sequence's 'flag' word instead).

    Every record field equals hota_host: integers exactly, float64 bit for bit.  A frame takes at most moteval.MAX_PER_FRAME rows on
    either side (beyond: FLAG_LIMIT for that sequence only).  The workspace holds objects x detections entries of PAIR_BYTES per
    sequence: a store beyond MAX_HOTA_PAIRS entries (or a workspace beyond 2 GiB) raises ValueError -- score it with hota_host.
    No class filtering and no DontCare removal here: evalprep.EvalPrep is the benchmark's preprocessing in front of this."""
    FLAG_WORD, FLAG_TEXT = 23, _FLAG_TEXT

    def __init__(self, sequences: Sequence[Dict], device='cuda:0'):
        super().__init__(device, 'score on the host with hota_host')
        st = MotStore(sequences)
        self._n_pair = int((st.seq[:, 7] * st.seq[:, 3]).sum())
        ws_bytes = int(_lib.load().tmpnn_hota_ws(st.S, st.n_obj, st.n_det, st.n_off, self._n_pair)) if self._n_pair <= MAX_HOTA_PAIRS else 0
        if self._n_pair > MAX_HOTA_PAIRS or ws_bytes > MAX_WS_BYTES:
            raise ValueError(f'HotaEvaluator: the pair workspace (objects x detections per sequence) has {self._n_pair} entries, more '
                             f'than MAX_HOTA_PAIRS = {MAX_HOTA_PAIRS}, or the workspace passes 2 GiB: score such a set on the host '
                             'with hota_host')
        self._thr = np.ascontiguousarray(ALPHAS - EPS)
        _attach_mot_store(self, st)
        self._workspace(ws_bytes)
        self._out = torch.zeros(max(st.S, 1), RECORD_WORDS, dtype=torch.int64, device=self.device)

    def evaluate(self, tracks: Sequence) -> None:
        self._enqueue('tmpnn_hota', tracks, self._thr.ctypes.data, self._ws.data_ptr(), self._ws_bytes, self._out.data_ptr())

    def _row(self, s, rec, fl, out) -> Dict:
        r = {'tp': rec[s, :NA].copy()}
        r.update({k: int(rec[s, NA + i]) for i, k in enumerate(INT_KEYS)})
        r.update({k: fl[s, 24 + NA * i:24 + NA * (i + 1)].copy() for i, k in enumerate(SUM_KEYS)})
        return _derived(r)

    def read(self, check: bool = True):
        per = self._read(check)
        return per, hota_overall([p for p in per if p is not None])

