"""The last step of the reference's inference: the score filter over whole tracks and the KITTI / BDD100K result tables
(reference infer.py:91-96, ablation.py:137; dataset/kitti_mot.py:21-73 store_kitti_results, dataset/bdd100k_mot.py:22-67
store_bdd100k_results).

    ResultRules           category names and the per-category least best score of a track (KITTI: Car tracks below 0.7 go)
    results_host          the rule, in numpy: one sequence and its tracks in, the filtered tracks, the kept rows in frame order
                          and the counts out.  It is the DEFINITION the device kernels must equal exactly.
    kitti_lines_host      the bytes store_kitti_results writes for that result
    bdd_document_host     the list store_bdd100k_results hands to json.dump
    synth_result_sequence a seeded generator for the tests and tools/gen_results_golden.py
    TrackResults          the store on the device + `apply(tracks)` (tmpnn_results_apply, csrc/results.hip: one clear and four
                          launches whatever the number of sequences) + `filtered_tracks()` (device views for the evaluators) +
                          `read()` (the one device -> host copy) + `write_kitti` / `write_bdd`

tests/golden/results pins the three host functions to the reference's own output (tools/gen_results_golden.py).  The BDD
document is pinned by the `data` argument the reference hands to json.dump, not by a file: its labels hold numpy scalars, on
which json.dump raises TypeError for every frame that is not empty, so the reference writes no BDD file as it stands.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .evalstore import FLAG_DUPLICATE, FLAG_STORE, SeqTable, SequenceEvaluator, _boxes, _ints, frame_sort


@dataclass(frozen=True)
class ResultRules:
    """names: category id -> the name written into the result table; min_track_score: category id -> threshold: a track whose
    category (the maximum category id over its rows) is listed and whose best detection score is below the threshold is
    removed as a whole."""
    names: Dict[int, str]
    min_track_score: Dict[int, float] = field(default_factory=dict)


KITTI_RESULT_RULES = ResultRules({1: 'Pedestrian', 2: 'Car', 3: 'Cyclist'}, {2: 0.7})
BDD_RESULT_RULES = ResultRules({1: 'pedestrian', 2: 'rider', 3: 'car', 4: 'bus', 5: 'truck', 6: 'train', 7: 'motorcycle', 8: 'bicycle'}, {})

COUNT_KEYS = ('kept_rows', 'kept_tracks', 'removed_rows', 'removed_tracks')
FLAG_NEGATIVE = 16             # an id below -1 (csrc/results.hip; bits 2 and 4 are evalstore's FLAG_DUPLICATE and FLAG_STORE)
_FLAG_TEXT = {FLAG_DUPLICATE: 'a kept track id occurs twice in one frame',
              FLAG_STORE: 'the store is inconsistent (an offset, a permutation entry, a category or a table size out of range)',
              FLAG_NEGATIVE: 'a track id below -1'}
RECORD_WORDS = 8               # struct tmpnn_result_record: the four counts, the flag word, three reserved
MAX_CATEGORY = 2 ** 15         # category ids are small non-negative integers (the threshold table is indexed by them)
MAX_SEQUENCES = 65535          # the sequence is the second grid dimension of the kernels
# the values load_detections fills in where a detector gives no 3D estimate (kitti_mot.py:360-363)
_OPTIONAL = (('det_alpha', (), -10.0), ('det_dim', (3,), -1.0), ('det_loc', (3,), -1000.0), ('det_rot', (), -10.0))


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _sequence_arrays(seq: Dict, rules: ResultRules, who: str) -> Dict:
    """The checked arrays of a sequence: det_frame / det_cat int64 [n], det_score float32 [n], det_box float32 [n, 4], and the
    optional columns with their defaults.  GT keys are ignored."""
    frame = _ints(seq['det_frame'], f'{who}: det_frame')
    n = frame.shape[0]
    q = {'det_frame': frame, 'det_cat': _ints(seq['det_cat'], f'{who}: det_cat', n), 'det_box': _boxes(_host(seq['det_box']), 'det_box')}
    score = _host(seq['det_score'])
    if score.size and score.dtype != np.float32:
        raise ValueError(f'{who}: det_score must be float32 (the filter compares in float32), got {score.dtype}')
    q['det_score'] = np.ascontiguousarray(score, np.float32).reshape(-1)
    if q['det_score'].shape[0] != n or q['det_box'].shape[0] != n:
        raise ValueError(f'{who}: one score and one box per row expected')
    for k, tail, default in _OPTIONAL:
        v = seq.get(k)
        q[k] = np.full((n,) + tail, default, np.float32) if v is None else np.ascontiguousarray(_host(v), np.float32).reshape((n,) + tail)
    bad = sorted(set(np.unique(q['det_cat']).tolist()) - set(rules.names))
    if bad:
        raise ValueError(f'{who}: categories {bad} are not among the rules\' names {sorted(rules.names)}')
    return q


def _check_rules(rules: ResultRules):
    for c in list(rules.names) + list(rules.min_track_score):
        if not (isinstance(c, (int, np.integer)) and 0 <= int(c) < MAX_CATEGORY):
            raise ValueError(f'ResultRules: category id {c!r}: integers in [0, {MAX_CATEGORY}) expected')


def results_host(seq: Dict, tracks, rules: ResultRules = KITTI_RESULT_RULES) -> Dict:
    """store_kitti_results / store_bdd100k_results without the file.  seq: det_frame, det_cat, det_score (float32), det_box
    and optionally det_alpha, det_dim, det_loc, det_rot; tracks = y_out[:, 1] in arrival order.

    For every id >= 0: c = max(det_cat) and s = max(det_score) over its rows; where c is in rules.min_track_score and
    s < np.float32(threshold), every row of the id becomes -1 (kitti_mot.py:36-45).  The comparison is made IN FLOAT32: that
    is what `np.amax(float32 array) < 0.7` does under NumPy 2 (NEP 50: the Python float takes the array's type), so a best score
    of exactly float32(0.7) = 0.699999988... is kept.  NumPy 1.x compared in double, where that value is below 0.7, and removed
    such a track.  (A NaN best score compares false and keeps the track, as in the reference.)

    Returns 'tracks' (int64 [n], filtered), 'order' (int32: the arrival indices of the rows whose filtered id is not -1, sorted
    stably by frame -- the order of the result table), kept_rows, kept_tracks, removed_rows, removed_tracks, and 't_range' =
    (min, max) of det_frame over ALL rows, as the reference takes it (None without rows).  ValueError: an id below -1 (the
    reference would write such rows into the table, by accident); a frame in which two kept rows share an id, named by its
    frame (the reference asserts there) -- a duplicate inside a removed track is no error: the reference filters first."""
    _check_rules(rules)
    q = _sequence_arrays(seq, rules, 'results_host')
    frame, cat, score = q['det_frame'], q['det_cat'], q['det_score']
    tr = _ints(tracks, 'results_host: tracks', frame.shape[0]).copy()
    if tr.size and tr.min() < -1:
        raise ValueError(f'results_host: track id {int(tr.min())}: ids are >= 0, or -1 for no track')
    kept_tracks = removed_tracks = removed_rows = 0
    for trk in np.unique(tr):
        if trk < 0:
            continue
        rows = np.where(tr == trk)[0]
        c, s = int(np.amax(cat[rows])), np.amax(score[rows])
        if c in rules.min_track_score and s < np.float32(rules.min_track_score[c]):
            tr[rows] = -1
            removed_tracks += 1
            removed_rows += rows.shape[0]
        else:
            kept_tracks += 1
    kept = np.where(tr != -1)[0]
    order = kept[np.argsort(frame[kept], kind='stable')].astype(np.int32)
    key = np.stack([frame[order], tr[order]], 1)
    if key.shape[0] and np.unique(key, axis=0).shape[0] != key.shape[0]:
        k, cnt = np.unique(key, axis=0, return_counts=True)
        raise ValueError(f'results_host: a track id occurs twice in frame {int(k[cnt > 1][0, 0])}')
    return {'tracks': tr, 'order': order, 'kept_rows': int(order.shape[0]), 'kept_tracks': kept_tracks,
            'removed_rows': removed_rows, 'removed_tracks': removed_tracks,
            't_range': (int(frame.min()), int(frame.max())) if frame.size else None}


def kitti_lines_host(seq: Dict, res: Dict, rules: ResultRules = KITTI_RESULT_RULES) -> bytes:
    """The bytes store_kitti_results writes for `res` = results_host(seq, ...): one line per kept row in `order` -- frame, id,
    category name, -1 -1, then alpha, the box, height width length, x y z, rotation_y and the score, each float32 value through
    '%.2f' (kitti_mot.py:71)."""
    q = _sequence_arrays(seq, rules, 'kitti_lines_host')
    out = []
    for i in res['order'].tolist():
        b, d, l = q['det_box'][i], q['det_dim'][i], q['det_loc'][i]
        out.append('%d %d %s -1 -1 %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n' % (
            q['det_frame'][i], res['tracks'][i], rules.names[int(q['det_cat'][i])], q['det_alpha'][i], b[0], b[1], b[2], b[3],
            d[0], d[1], d[2], l[0], l[1], l[2], q['det_rot'][i], q['det_score'][i]))
    return ''.join(out).encode('ascii')


def bdd_document_host(seq: Dict, res: Dict, rules: ResultRules, name: str) -> List:
    """The list store_bdd100k_results hands to json.dump for `res` (bdd100k_mot.py:41-64): one entry per frame of t_range, a
    frame without kept rows included, `name` (the file's base name) as 'name' and 'videoName'; every number an int / a float
    (the float32 coordinates exactly), so that json.dump takes it."""
    q = _sequence_arrays(seq, rules, 'bdd_document_host')
    if res['t_range'] is None:
        return []
    t0, t1 = res['t_range']
    doc = [{'name': name, 'videoName': name, 'frameIndex': t, 'labels': []} for t in range(t0, t1 + 1)]
    for i in res['order'].tolist():
        b = q['det_box'][i]
        doc[int(q['det_frame'][i]) - t0]['labels'].append({
            'id': int(res['tracks'][i]), 'category': rules.names[int(q['det_cat'][i])],
            'box2d': {'x1': float(b[0]), 'y1': float(b[1]), 'x2': float(b[2]), 'y2': float(b[3])}})
    return doc


def bbox_pred_of(seq: Dict, rules: ResultRules) -> np.ndarray:
    """float32 [n, 14]: the rows the reference's two functions take (category, alpha, x1 y1 x2 y2, h w l, x y z, rotation_y,
    score), as infer.py:92 cuts them out of the loader's rows."""
    q = _sequence_arrays(seq, rules, 'bbox_pred_of')
    return np.concatenate([q['det_cat'][:, None].astype(np.float32), q['det_alpha'][:, None], q['det_box'], q['det_dim'], q['det_loc'],
                           q['det_rot'][:, None], q['det_score'][:, None]], 1).astype(np.float32).reshape(-1, 14)


def synth_result_sequence(seed: int, frames: int, n_tracks: int = 20, rules: ResultRules = KITTI_RESULT_RULES, t0: int = 3,
                          p_gap: float = 0.15, max_len: Optional[int] = None, p_present: float = 0.7, stray_rate: float = 1.0,
                          sparse_ids: bool = False, duplicate: Optional[str] = None, with_3d: bool = False) -> Dict:
    """A seeded sequence and its tracks for the tests and tools/gen_results_golden.py: the dict results_host takes plus 'tracks'.
    Frames start at t0 and skip one to three numbers with p_gap; the rows arrive shuffled.  Track k lives for up to max_len of
    the `frames` frames (default: all) from a random first one, present in each with p_present (in its first always).  Its
    category set cycles over the single categories of `rules` and the pairs of neighbouring ones, each row drawing from the set
    and the largest one occurring at least once -- for KITTI {1, 2} makes a Car and {2, 3} a Cyclist.  Its best score cycles,
    with another period, over float32(0.7), the float32 next below it, a value in [0.75, 1) and one in [0.2, 0.65); the other
    rows score below the best.  Stray rows without a track (-1) at `stray_rate` a frame.  sparse_ids: the ids are distinct
    values over [0, 2^31 - 1], both ends included; otherwise 0 .. n_tracks - 1 in shuffled order.  duplicate: 'kept' / 'removed'
    plants a second row in one frame of a track that results_host keeps / removes ('dup_frame' names the frame).  with_3d:
    det_alpha, det_dim, det_loc, det_rot are random values instead of absent."""
    rng = np.random.default_rng([int(seed), 9191])
    cats = sorted(rules.names)
    sets = [(c,) for c in cats] + [(a, b) for a, b in zip(cats[:-1], cats[1:])]
    seven = np.float32(0.7)
    steps = np.where(rng.random(frames) < p_gap, rng.integers(2, 5, frames), 1)
    fr = t0 + np.concatenate([[0], np.cumsum(steps[1:])]).astype(np.int64) if frames else np.zeros(0, np.int64)
    ids = np.arange(n_tracks, dtype=np.int64)
    if sparse_ids:
        pool = np.unique(rng.integers(1, 2 ** 31 - 1, 2 * n_tracks + 8))
        ids = np.concatenate([[0, 2 ** 31 - 1], rng.permutation(pool)])[:n_tracks]
        if ids.shape[0] != n_tracks:
            raise ValueError('synth_result_sequence: too few distinct sparse ids: change the seed')
    ids = rng.permutation(ids)
    rows = []                                                       # (frame, track, category, score)
    for k in range(n_tracks if frames else 0):
        cset = sets[k % len(sets)]
        L = frames if max_len is None else min(frames, int(rng.integers(1, max_len + 1)))
        first = int(rng.integers(0, frames - L + 1))
        at = [first] + [f for f in range(first + 1, first + L) if rng.random() < p_present]
        best = (seven, np.nextafter(seven, np.float32(0)), np.float32(rng.uniform(0.75, 1.0)), np.float32(rng.uniform(0.2, 0.65)))[(k // len(sets)) % 4]
        sc = (best * rng.uniform(0.3, 0.99, len(at))).astype(np.float32)
        sc[int(rng.integers(len(at)))] = best
        cc = rng.choice(cset, len(at))
        cc[int(rng.integers(len(at)))] = max(cset)
        rows += [(fr[f], ids[k], c, s) for f, c, s in zip(at, cc, sc)]
    for f in range(frames):
        rows += [(fr[f], -1, rng.choice(cats), np.float32(rng.uniform(0.05, 1.0))) for _ in range(rng.poisson(stray_rate))]
    frame = np.asarray([r[0] for r in rows], np.int64)
    tracks = np.asarray([r[1] for r in rows], np.int64)
    cat = np.asarray([r[2] for r in rows], np.int64)
    score = np.asarray([r[3] for r in rows], np.float32)
    n = frame.shape[0]

    def table(box):
        q = {'det_frame': frame, 'det_cat': cat, 'det_score': score, 'det_box': box}
        if with_3d:
            g = np.random.default_rng([int(seed), 7])
            q.update(det_alpha=g.uniform(-3.2, 3.2, n).astype(np.float32), det_dim=g.uniform(0.5, 4.0, (n, 3)).astype(np.float32),
                     det_loc=g.uniform(-40, 80, (n, 3)).astype(np.float32), det_rot=g.uniform(-3.2, 3.2, n).astype(np.float32))
        return q
    dup_frame = None
    if duplicate is not None:
        if duplicate not in ('kept', 'removed'):
            raise ValueError(f"synth_result_sequence: duplicate={duplicate!r}: 'kept' or 'removed' expected")
        res = results_host(table(np.zeros((n, 4), np.float32)), tracks, rules)
        want = (res['tracks'] != -1) if duplicate == 'kept' else ((tracks >= 0) & (res['tracks'] == -1))
        cand = np.where(want)[0]
        if cand.size == 0:
            raise ValueError(f'synth_result_sequence: no {duplicate} track to duplicate a row of: change the seed')
        i = int(cand[rng.integers(cand.size)])
        dup_frame = int(frame[i])
        frame, tracks, cat = np.append(frame, frame[i]), np.append(tracks, tracks[i]), np.append(cat, cat[i])
        score = np.append(score, np.float32(0.5 * score[i])).astype(np.float32)
        n += 1
    p = rng.permutation(n)
    frame, tracks, cat, score = frame[p], tracks[p], cat[p], score[p]
    c = np.stack([rng.uniform(0, 1242, n), rng.uniform(0, 375, n)], 1)
    wh = rng.uniform(20, 160, (n, 2))
    q = table(np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32))
    q['tracks'] = tracks
    if dup_frame is not None:
        q['dup_frame'] = dup_frame
    return q


def score_keys(score: np.ndarray) -> np.ndarray:
    """uint32 per float32: an integer whose unsigned order is the floats' order (-0 counted as +0); every NaN maps to the largest
    key, so that a maximum over keys propagates it as np.amax does, and compares false against every threshold."""
    s = np.ascontiguousarray(score, np.float32) + np.float32(0)     # (-0 + 0 = +0)
    u = s.view(np.uint32)
    key = np.where(u >> 31 == 0, u | np.uint32(0x80000000), ~u).astype(np.uint32)
    key[np.isnan(s)] = np.uint32(0xFFFFFFFF)
    return key


class ResultStore:
    """What TrackResults keeps of S sequences, packed (host numpy arrays; struct tmpnn_result_store, include/tmpnn.h):

        seq       int64 [S, 8]   tab_base, n_tab, det_base, n_det, off_base, n_frames, 0, 0
        det_perm  int32 [n_det]  sorted position (stable by frame) -> arrival index, relative to det_base
        det_fidx  int32 [n_det]  frame index (frame - first frame) of a sorted position
        det_off   int32 [n_off]  per sequence n_frames + 1 offsets of its frames over the sorted positions
        det_cat   int32 [n_det]  categories, arrival order           det_key  uint32 [n_det]  score_keys of the scores
        thr_key   uint32 [n_cat] per category id the key of float32(threshold), 0 = no threshold
    n_tab: slots of the sequence's track table, a power of two >= max(256, 2 n_det) (0 without rows)."""

    def __init__(self, sequences: Sequence[Dict], rules: ResultRules):
        _check_rules(rules)
        tab = SeqTable('ResultStore', len(sequences), max_rows=2 ** 28, beyond='is beyond int32 (frames) or 2^28 rows',
                       max_sequences=MAX_SEQUENCES)
        self.S, self.rules = len(sequences), rules
        self.arrays: List[Dict] = []
        self.t_range: List = []
        for s, q in enumerate(sequences):
            a = _sequence_arrays(q, rules, f'ResultStore: sequence {s}')
            frame = a['det_frame']
            n = frame.shape[0]
            t0, t1 = (int(frame.min()), int(frame.max())) if n else (0, -1)
            nf = t1 - t0 + 1
            tab.check(s, nf, n)
            o, off = frame_sort(frame, t0, nf)
            n_tab = 0 if n == 0 else max(256, 1 << int(2 * n - 1).bit_length())
            tab.add(s, n_tab, n, nf, det_perm=o, det_fidx=frame[o] - t0, det_off=off, det_cat=a['det_cat'], det_key=score_keys(a['det_score']))
            self.arrays.append(a)
            self.t_range.append((t0, t1) if n else None)
        self.seq = tab.seq
        for k in ('det_perm', 'det_fidx', 'det_off', 'det_cat'):
            setattr(self, k, tab.pack(k, np.int32))
        self.det_key = tab.pack('det_key', np.uint32)
        self.n_cat = max(list(rules.names) + list(rules.min_track_score) + [0]) + 1
        thr = np.zeros(self.n_cat, np.uint32)
        for c, v in rules.min_track_score.items():
            if not np.isnan(np.float32(v)):                          # (nothing is below NaN: no threshold)
                thr[int(c)] = score_keys(np.asarray([v], np.float32))[0]
        self.thr_key = thr
        self.n_tab, self.n_det, self.n_off, _ = tab.totals


class TrackResults(SequenceEvaluator):
    """The score filter and the result table of S sequences on the device.  sequences: the evaluators' dicts (det_frame,
    det_cat, det_score float32, det_box; optionally det_alpha, det_dim, det_loc, det_rot; GT keys are ignored) -- what
    DetectionLabeler.eval_sequences() gives; a category outside rules.names raises ValueError.  The store is built on the host
    and uploaded once.

        tr.apply(tracks)       tracks: per sequence an int tensor / array [n_det] in arrival order, host or device (None: the
                               sequence is left out).  One packed upload at the most, one clear and four launches whatever
                               the number of sequences, no host wait.
        tr.filtered_tracks()   per sequence a device view, int32 [n_det] in arrival order: the ids after the filter, for
                               MotEvaluator / MapEvaluator / HotaEvaluator.evaluate without a host trip (valid until the next apply)
        tr.read()              the one device -> host copy: per sequence the dict of results_host (None where left out).
                               RuntimeError naming sequence and frame when a flag word is set (check=False: no error, every
                               dict has the sequence's 'flag' word instead)
        tr.write_kitti(dir)    '%.4d.txt' per sequence, the bytes of kitti_lines_host; write_bdd: '%.4d.json', bdd_document_host
                               through json.dump.  A sequence without detections, or left out, writes no file (infer.py:38-40).
    Everything read() returns equals results_host exactly; two applies of the same tracks give the same bytes."""

    STEP, FLAG_WORD, FLAG_TEXT = ('apply', 'apply'), 4, _FLAG_TEXT

    def __init__(self, sequences: Sequence[Dict], rules: ResultRules = KITTI_RESULT_RULES, device='cuda:0'):
        super().__init__(device, 'filter on the host with results_host')
        self.rules = rules
        st = ResultStore(sequences, rules)
        names = ('seq', 'det_off', 'det_perm', 'det_fidx', 'det_cat', 'det_key', 'thr_key')
        self._c = _lib.CResultStore(st.S, st.n_cat, st.n_det, st.n_off, st.n_tab, *self._attach(st, names))
        self._workspace(_lib.load().tmpnn_results_ws(st.S, st.n_det, st.n_tab))
        if self._ws_bytes == 0 and st.S:
            raise ValueError(f'TrackResults: a store of {st.S} sequences, {st.n_det} rows is beyond the workspace\'s limits')
        # one buffer for everything read() copies: the records (int64 words as int32 pairs), the filtered ids, the order
        self._rec_ints = 2 * RECORD_WORDS * max(st.S, 1)
        self._out = torch.zeros(self._rec_ints + 2 * st.n_det, dtype=torch.int32, device=self.device)

    def apply(self, tracks: Sequence) -> None:
        base = self._out.data_ptr()
        self._enqueue('tmpnn_results_apply', tracks, self._ws.data_ptr(), self._ws_bytes, base, base + 4 * self._rec_ints,
                      base + 4 * (self._rec_ints + self.store.n_det))

    def filtered_tracks(self) -> List[torch.Tensor]:
        return self._views(self._out, self._rec_ints)

    def _row(self, s, rec, fl, out) -> Dict:
        st = self.store
        b, n = self._det[s]
        ids, order = self._rec_ints + b, self._rec_ints + st.n_det + b          # (its filtered ids, its part of the order)
        r = {'tracks': out[ids:ids + n].astype(np.int64), 'order': out[order:order + int(rec[s, 0])].copy()}
        r.update({k: int(rec[s, i]) for i, k in enumerate(COUNT_KEYS)})
        r['t_range'] = st.t_range[s]
        return r

    def read(self, check: bool = True) -> List:
        return self._read(check, lambda out: out[:self._rec_ints].view(np.int64).reshape(-1, RECORD_WORDS),
                          lambda s: self.store.t_range[s][0])

    def _write(self, out_dir: str, ext: str, per: Optional[List]) -> List[Optional[str]]:
        per = self.read() if per is None else per
        os.makedirs(out_dir, exist_ok=True)
        paths: List[Optional[str]] = []
        for s, r in enumerate(per):
            if r is None or r['t_range'] is None:
                paths.append(None)
                continue
            name = '%.4d.%s' % (s, ext)
            path = os.path.join(out_dir, name)
            if ext == 'txt':
                with open(path, 'wb') as f:
                    f.write(kitti_lines_host(self.store.arrays[s], r, self.rules))
            else:
                with open(path, 'w') as f:
                    json.dump(bdd_document_host(self.store.arrays[s], r, self.rules, name), f)
            paths.append(path)
        return paths

    def write_kitti(self, out_dir: str, per: Optional[List] = None) -> List[Optional[str]]:
        """'%.4d.txt' per sequence in out_dir (created if missing) from the read record (`per`: what read() returned, to spare a
        second copy).  Returns the paths, None for a sequence that wrote no file."""
        return self._write(out_dir, 'txt', per)

    def write_bdd(self, out_dir: str, per: Optional[List] = None) -> List[Optional[str]]:
        """'%.4d.json' per sequence, as write_kitti."""
        return self._write(out_dir, 'json', per)


def results_overall(per_sequence: Sequence[Optional[Dict]]) -> Dict:
    """The four counts summed over the sequences that took part."""
    return {k: sum(int(r[k]) for r in per_sequence if r is not None) for k in COUNT_KEYS}
