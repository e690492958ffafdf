"""Online tracking: detections arrive one frame at a time, track ids come out a few frames later.

`OnlineTracker` runs the loop of reference infer.py:35-87 -- the one `loops.infer_sequence` runs over a recorded sequence --
incrementally: push k is timestep k, and after every push the tracker has done exactly what the offline loop does at that
timestep (update_graph -> model -> decode_tracks, or the look-ahead of initialize_graph while fewer than two non-empty frames
have arrived), through the same `TrackGraph` calls and the same native driver.  Fed the frames of a time-sorted sequence with
`last=True` on its last non-empty frame, `tracks()` equals `infer_sequence`'s `y_out[:, 1]` exactly.

    spec = FeatureSpec(ncategories=8, feats='2d+temp', mean=mean, std=std)
    trk = OnlineTracker(model, cur_win_size=5, spec=spec)
    for cat, score, box in detector:                   # every frame, also the ones without detections
        trk.push(cat, score, box)
        ids = trk.tracks()                             # -1: not finalised yet

With a 'vis' model the 128 visual columns come from the live frame, on the device (`OnlineVis`: resize + ToTensor + Normalize by
`frames.FramePrep`, the user's CNN, `VisHead.rows` writing straight into the feature buffer; no host round trip):

    spec = FeatureSpec(ncategories=8, feats='2d+temp+vis', mean=mean, std=std)
    vis = OnlineVis(VisHead((384, 1280), 4, mean, std), FramePrep((384, 1280), img_mean, img_std), embed_net)
    trk = OnlineTracker(model, cur_win_size=5, spec=spec, vis=vis)
    for img, (cat, score, box) in camera:              # img [h, w, 3] uint8 as decoded
        trk.push(cat, score, box, frame=img)

(`push(cat, score, box, vis=host_array)` still takes ready-made visual features.)

The per-sequence buffers of `TrackGraph` (features, detection ids, tracks, finalisation scratch) are capacity-sized here and
grow by doubling with a device-side copy; raw detections become standardised feature rows in one launch
(`tmpnn_online_features`, csrc/online.hip) whose host definition is `online_features_host`.
"""
from __future__ import annotations

import re
from typing import Optional

import numpy as np
import torch

from . import _lib
from .loops import _fast_greedy, _pos_score
from .tracking import TrackGraph

VIS_COLS = 128              # width of the 'vis' feature group (models/track_mpnn.py:17-33)
MAX_FRAMES = 2 ** 24        # timesteps are exact in float32 below it (the temporal pair is computed on a float32 column)


class FeatureSpec:
    """How raw detections become the model's feature rows (reference dataset/kitti_mot.py:545-566).

    ncategories   one-hot width (categories are 1-based)
    feats         the model's groups in its order: '2d', '2d+temp', '2d+temp+vis', '2d+vis' ('-' separators are taken too)
    mean, std     [F] with F = ncategories + 5 (+ 2 with 'temp') (+ 128 with 'vis'): the reference's values for the detector
                  at hand (kitti_mot.py:155-177; the library carries no presets)
    fr_range      period of the temporal pair (kitti_mot.py:414-420)

    `pair` float32 [fr_range, 2] is (sin, cos) of (t mod fr_range) pi / fr_range, built with numpy exactly as
    `DetectionStore.table` is before it is standardised."""

    def __init__(self, ncategories: int, feats: str, mean, std, fr_range: int = 30):
        names = re.split(r'[+-]', feats) if isinstance(feats, str) else None
        if not names or names[0] != '2d' or names not in (['2d'], ['2d', 'temp'], ['2d', 'temp', 'vis'], ['2d', 'vis']):
            raise ValueError(f"FeatureSpec: feats={feats!r}; '2d', '2d+temp', '2d+temp+vis' or '2d+vis' expected")
        self.feats = '+'.join(names)
        self.temp, self.vis = 'temp' in names, 'vis' in names
        self.ncat, self.fr_range = int(ncategories), int(fr_range)
        if self.ncat < 1 or self.fr_range < 1:
            raise ValueError(f'FeatureSpec: ncategories={ncategories}, fr_range={fr_range}')
        self.Fs = self.ncat + 5
        self.F = self.Fs + (2 if self.temp else 0) + (VIS_COLS if self.vis else 0)
        self.mean = np.ascontiguousarray(np.asarray(mean, dtype=np.float32).ravel())
        self.std = np.ascontiguousarray(np.asarray(std, dtype=np.float32).ravel())
        if self.mean.size != self.F or self.std.size != self.F:
            raise ValueError(f'FeatureSpec: mean / std of length {self.mean.size} / {self.std.size} for {self.F} feature columns '
                             f'({self.ncat} categories + 5{" + 2" if self.temp else ""}{" + 128" if self.vis else ""})')
        if not (np.isfinite(self.mean).all() and np.isfinite(self.std).all() and (self.std != 0).all()):
            raise ValueError('FeatureSpec: mean / std must be finite and std non-zero')
        a = np.mod(np.arange(self.fr_range, dtype=np.float32)[:, None], self.fr_range) * np.pi / self.fr_range
        self.pair = np.ascontiguousarray(np.concatenate((np.sin(a), np.cos(a)), axis=1).astype(np.float32))


def _raw_arrays(spec: FeatureSpec, cat, score, box, vis, from_frame: bool = False):
    """The raw detections of one frame, validated, as (cat int64 [D], score float32 [D], box float32 [D, 4], vis float32
    [D, 128] or None).  from_frame: the 'vis' columns come from the frame on the device (OnlineVis), not from `vis`."""
    cat = np.asarray(cat)
    if cat.size and not np.issubdtype(cat.dtype, np.integer):
        raise ValueError(f'online features: cat must be integers, got {cat.dtype}')
    cat = cat.astype(np.int64).ravel()
    D = cat.size
    score = np.asarray(score, dtype=np.float32).ravel()
    box = np.asarray(box, dtype=np.float32).reshape(-1, 4)
    if score.size != D or box.shape[0] != D:
        raise ValueError(f'online features: cat, score, box differ in length ({D}, {score.size}, {box.shape[0]})')
    if D and (cat.min() < 1 or cat.max() > spec.ncat):
        raise ValueError(f'online features: a cat outside 1 .. {spec.ncat}')
    if not (np.isfinite(box).all() and np.isfinite(score).all()):
        raise ValueError('online features: a box or score is not finite')
    if from_frame:
        vis = None
    elif spec.vis:
        if vis is None:
            raise ValueError("online features: the spec has 'vis' columns: pass vis [D, 128]")
        if isinstance(vis, torch.Tensor):
            vis = vis.detach().cpu().numpy()
        vis = np.asarray(vis, dtype=np.float32)
        if vis.shape != (D, VIS_COLS):
            raise ValueError(f'online features: vis of shape {vis.shape}, expected {(D, VIS_COLS)}')
    elif vis is not None:
        raise ValueError("online features: vis given but the spec has no 'vis' columns")
    return cat, score, box, vis


def online_features_host(spec: FeatureSpec, cat, score, box, t: int, vis=None) -> np.ndarray:
    """The feature rows [D, F] float32 of one frame's raw detections at timestep t (numpy; the definition the device kernel
    `tmpnn_online_features` equals bit for bit).  cat [D] 1-based ints, score [D], box [D, 4] x1 y1 x2 y2 (taken to float32
    first, as the reference holds them), vis [D, 128] with a 'vis' spec."""
    t = int(t)
    if not 0 <= t < MAX_FRAMES:
        raise ValueError(f'online features: t={t} (0 .. 2^24 - 1)')
    cat, s32, b32, vis = _raw_arrays(spec, cat, score, box, vis)
    D = cat.size
    eye = np.eye(spec.ncat, dtype=np.float32)
    two_d = np.stack((s32, (b32[:, 0] + b32[:, 2]) / 2.0, (b32[:, 1] + b32[:, 3]) / 2.0, b32[:, 2] - b32[:, 0],
                      b32[:, 3] - b32[:, 1]), axis=1).astype(np.float32)
    cols = [eye[cat - 1].reshape(D, spec.ncat), two_d]
    if spec.temp:
        cols.append(np.broadcast_to(spec.pair[t % spec.fr_range][None, :], (D, 2)))
    if spec.vis:
        cols.append(vis)
    return ((np.concatenate(cols, axis=1) - spec.mean[None, :]) / spec.std[None, :]).astype(np.float32)


class OnlineVis:
    """What turns a live frame into the 'vis' columns of its detections on the device (`OnlineTracker(..., vis=OnlineVis(...))`,
    then `push(cat, score, box, frame=img)`):

    head        a VisHead: the box-centre gather and the standardised softmax rows
    prep        a FramePrep with the head's input size: resize, ToTensor, Normalize
    embed_net   the embedding CNN (any callable): [1, 3, H, W] float32 -> maps [1, 128, H / down_ratio, W / down_ratio]

    `columns(frame, box_d, out, col)` runs, without an autograd graph and without a host round trip, maps =
    embed_net(prep.prep(frame)) and head.rows(maps, box, 0, (h, w), out, col)."""

    def __init__(self, head, prep, embed_net):
        for obj, names, what in ((head, ('input_h', 'input_w', 'mean', 'std', 'rows'), 'head: a VisHead'),
                                 (prep, ('input_hw', 'prep'), 'prep: a FramePrep')):
            if not all(hasattr(obj, n) for n in names):
                raise ValueError(f'OnlineVis: {what} expected, got {type(obj).__name__}')
        if not callable(embed_net):
            raise ValueError('OnlineVis: embed_net must be callable')
        want = (float(head.input_h), float(head.input_w))
        if tuple(float(v) for v in prep.input_hw) != want:
            raise ValueError(f"OnlineVis: prep resizes to {tuple(prep.input_hw)}, the head's input size is "
                             f'{(head.input_h, head.input_w)}')
        self.head, self.prep, self.embed_net = head, prep, embed_net
        self._zeros = None                         # map_of of every row: the one map of the frame

    def columns(self, frame, box_d: torch.Tensor, out: torch.Tensor, col: int) -> None:
        """Write columns col .. col + 127 of out [D, F] (device rows) for the boxes box_d [D, 4] (device float32) of `frame`
        [h, w, 3] uint8."""
        D = int(box_d.shape[0])
        if self._zeros is None or self._zeros.shape[0] < D:
            self._zeros = torch.zeros(max(D, 256), dtype=torch.int32, device=box_d.device)
        with torch.no_grad():
            maps = self.embed_net(self.prep.prep(frame))
            self.head.rows(maps, box_d, self._zeros[:D], (int(frame.shape[0]), int(frame.shape[1])), out=out, col=col)


class OnlineTracker:
    """The inference loop of infer.py:35-87, one pushed frame at a time (module docstring).

    model          a TrackMPNN in eval mode on `device`; its parameters must not change while the tracker lives
    cur_win_size   >= 2, ret_win_size, use_hungarian, tp_classifier: as `infer_sequence`
    spec           a FeatureSpec, needed by `push` (raw detections); `push_features` takes ready-made rows
    max_dets       initial capacity of the per-detection buffers (they double when full)

    `frames`, `ndets`, `finalised_upto` are host integers.  `finalised_upto`: the decode horizon -- detections of timesteps
    below it that the loop has decoded carry their final id in `tracks()` (-1: none); while streaming it is
    max(0, frames - cur_win_size + 1), after the end of the stream `frames`.  (Detections held back while the tracker waits
    for a second non-empty frame are decoded only once it arrives.)"""

    def __init__(self, model, cur_win_size: int = 5, ret_win_size: int = 0, use_hungarian: bool = False,
                 tp_classifier: bool = True, spec: Optional[FeatureSpec] = None, device='cuda:0', max_dets: int = 16384,
                 vis: Optional[OnlineVis] = None):
        self.cur_win_size, self.ret_win_size = int(cur_win_size), int(ret_win_size)
        if self.cur_win_size < 2:
            raise ValueError(f'OnlineTracker: cur_win_size={cur_win_size}; >= 2 expected (with 1 the decode that follows a '
                             're-initialisation would finalise rows of the block it has just built)')
        if self.ret_win_size < 0:
            raise ValueError(f'OnlineTracker: ret_win_size={ret_win_size}')
        if int(max_dets) < 1:
            raise ValueError(f'OnlineTracker: max_dets={max_dets}')
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'OnlineTracker on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path): pass a '
                               'cuda device')
        if spec is not None and not isinstance(spec, FeatureSpec):
            raise ValueError('OnlineTracker: spec must be a FeatureSpec')
        ms = getattr(model, 'spec', None)
        self.F = int(ms.F_total) if ms is not None else (spec.F if spec is not None else None)
        if self.F is None:
            raise ValueError('OnlineTracker: the feature width is unknown (a model without .spec and no FeatureSpec)')
        if spec is not None and spec.F != self.F:
            raise ValueError(f'OnlineTracker: the spec builds {spec.F} feature columns, the model takes {self.F}')
        if getattr(model, 'training', False):
            raise ValueError('OnlineTracker: the model must be in eval mode')
        if vis is not None:
            if not isinstance(vis, OnlineVis):
                raise ValueError('OnlineTracker: vis must be an OnlineVis')
            if spec is None or not spec.vis:
                raise ValueError("OnlineTracker: vis=OnlineVis(...) needs a FeatureSpec with the 'vis' columns "
                                 f'(spec={None if spec is None else spec.feats!r})')
            hm, hs = (np.asarray(v, np.float32).ravel() for v in (vis.head.mean, vis.head.std))
            if not (np.array_equal(hm, spec.mean[-VIS_COLS:]) and np.array_equal(hs, spec.std[-VIS_COLS:])):
                raise ValueError("OnlineTracker: the head's 128 mean / std values differ from the last 128 of the spec's")
        self.model, self.spec, self.device, self.vis = model, spec, dev, vis
        self.use_hungarian, self.tp_classifier = bool(use_hungarian), bool(tp_classifier)
        self._cap0 = int(max_dets)
        self._cap = 0
        self._X = self._ids = self._track = self._y_track = self._pos = None
        self._spec_d = None                       # mean | std | pair on the device (one upload)
        self._frames = self._ndets = 0
        self._closed = False
        self._tg: Optional[TrackGraph] = None
        self._prev_tg = None                      # the graph a re-initialisation abandoned (its launches may still run)
        self._h = self._sc = None
        self._h_cap = 0
        self._collecting, self._pending, self._restart_t = True, [], None
        self._fast = self._finfo = self._step_info = None
        self._fast_known = False
        self.native_steps = 0                     # pushes that ran through the native driver (diagnostics)
        self.growths = 0                          # times the buffers doubled (diagnostics)

    # ---- host counters ---------------------------------------------------------------------------------------------
    @property
    def frames(self) -> int:
        return self._frames

    @property
    def ndets(self) -> int:
        return self._ndets

    @property
    def finalised_upto(self) -> int:
        return self._frames if self._closed else max(0, self._frames - self.cur_win_size + 1)

    def tracks(self) -> np.ndarray:
        """y_out[:, 1] of the detections so far, in arrival order: int64 [ndets], -1 = not finalised (one device -> host
        copy)."""
        if self._ndets == 0:
            return np.zeros(0, np.int64)
        return self._y_track[:self._ndets].cpu().numpy().astype(np.int64)

    # ---- buffers ---------------------------------------------------------------------------------------------------
    def _reserve(self, n: int) -> None:
        """Room for n detections: capacity-sized buffers, doubled with a device-side copy (nothing waits for the device)."""
        if n <= self._cap:
            return
        if self._cap == 0:                        # first use of the device
            prm = next(iter(self.model.parameters()), None) if hasattr(self.model, 'parameters') else None
            if prm is not None and prm.device.type != 'cuda':
                raise RuntimeError(f'OnlineTracker: the model is on {prm.device}: trackmpnn_amd runs on the MI355X HIP kernels '
                                   'only (no CPU path)')
        cap = max(self._cap, self._cap0)
        while cap < n:
            cap *= 2
        self.growths += 1 if self._cap else 0
        if cap >= 2 ** 31 - 1:
            raise ValueError('OnlineTracker: detections must fit in int32')
        dev, nd = self.device, self._ndets
        X = torch.empty((cap, self.F), dtype=torch.float32, device=dev)
        ids = torch.arange(cap, dtype=torch.int32, device=dev)          # detection ids are arrival order
        track = torch.full((cap,), -1, dtype=torch.int32, device=dev)   # no ground truth in a stream
        y_track = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        pos = torch.empty((cap,), dtype=torch.int32, device=dev)
        if nd:
            X[:nd].copy_(self._X[:nd])
            y_track[:nd].copy_(self._y_track[:nd])
        self._X, self._ids, self._track, self._y_track, self._pos, self._cap = X, ids, track, y_track, pos, cap

    def _upload(self, host: torch.Tensor, dst: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One host -> device copy through pinned staging memory of torch's caching host allocator (it keeps the block until
        the copy has run): the host does not wait for the device."""
        st = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
        st.copy_(host)
        if dst is None:
            return st.to(self.device, non_blocking=True)
        dst.copy_(st, non_blocking=True)
        return dst

    def _check_open(self, D: int) -> None:
        if self._closed:
            raise RuntimeError('OnlineTracker: the stream has ended (close() or a push with last=True); start a new tracker')
        if self._frames >= MAX_FRAMES:
            raise ValueError('OnlineTracker: 2^24 frames pushed')

    # ---- the two ways in -------------------------------------------------------------------------------------------
    def push(self, cat, score, box, vis=None, last: bool = False, frame=None) -> None:
        """The raw detections of the next frame: cat [D] 1-based ints, score [D], box [D, 4] x1 y1 x2 y2; D may be 0.  With a
        'vis' spec either vis [D, 128] (host values, uploaded with the detections) or, on a tracker built with
        vis=OnlineVis(...), frame [h, w, 3] uint8 as decoded: the frame is resized, normalised and run through the CNN on the
        device and the head writes the 'vis' columns in place (D = 0 runs no CNN and no launch).  One host -> device copy of
        the packed detections and one launch build the other columns."""
        if self.spec is None:
            raise ValueError('OnlineTracker.push: raw detections need a FeatureSpec (spec=...); push_features takes ready rows')
        sp = self.spec
        if frame is not None:
            if vis is not None:
                raise ValueError('OnlineTracker.push: frame= and vis= together; the frame gives the vis columns')
            if self.vis is None:
                raise ValueError('OnlineTracker.push: frame= needs a tracker built with vis=OnlineVis(...)')
            fshape = tuple(getattr(frame, 'shape', ()))
            fdtype = getattr(frame, 'dtype', None)
            if len(fshape) != 3 or fshape[2] != 3 or min(fshape) < 1 or fdtype not in (torch.uint8, np.dtype(np.uint8)):
                raise ValueError(f'OnlineTracker.push: frame [h, w, 3] uint8 expected, got {fshape} {fdtype}')
        cat, s32, b32, vis = _raw_arrays(sp, cat, score, box, vis, from_frame=frame is not None)
        D = int(cat.size)
        self._check_open(D)
        nd = self._ndets
        if D:
            self._reserve(nd + D)
            if self._spec_d is None:
                self._spec_d = self._upload(torch.from_numpy(np.concatenate([sp.mean, sp.std, sp.pair.ravel()])))
            V = VIS_COLS if sp.vis and frame is None else 0      # (V = 0 with the same ld_x leaves the last 128 columns alone)
            raw = np.empty((D, 6), np.int32)
            raw[:, 0] = cat
            rf = raw.view(np.float32)
            rf[:, 1], rf[:, 2:] = s32, b32
            words = raw.ravel() if not V else np.concatenate([raw.ravel(), np.ascontiguousarray(vis).view(np.int32).ravel()])
            pk = self._upload(torch.from_numpy(words))
            sd = self._spec_d.data_ptr()
            _lib.call('tmpnn_online_features', D, nd, self._cap, self._frames % sp.fr_range, sp.fr_range, sp.ncat, int(sp.temp), V,
                      pk.data_ptr(), pk.data_ptr() + 4 * 6 * D if V else None, V, sd, sd + 4 * sp.F, sd + 8 * sp.F,
                      self._X.data_ptr(), self.F, self._y_track.data_ptr(), self._ids.data_ptr(), _lib.raw_stream(self.device))
            if frame is not None:
                box_d = pk.view(torch.float32).view(D, 6)[:, 2:6]        # the float32 boxes, already on the device
                self.vis.columns(frame, box_d, self._X[nd:nd + D], self.F - VIS_COLS)
        self._advance(D, last)

    def push_features(self, x, last: bool = False) -> None:
        """The next frame's rows, already standardised: x [D, F_total] float32, host or device; D may be 0."""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != self.F or x.dtype != torch.float32:
            raise ValueError(f'OnlineTracker.push_features: x [D, {self.F}] float32 expected, got '
                             f'{tuple(x.shape) if hasattr(x, "shape") else type(x)} {getattr(x, "dtype", "")}')
        D = int(x.shape[0])
        self._check_open(D)
        nd = self._ndets
        if D:
            self._reserve(nd + D)
            dst = self._X[nd:nd + D]
            if x.is_cuda:
                dst.copy_(x.detach(), non_blocking=True)
            else:
                self._upload(x.detach(), dst)
        self._advance(D, last)

    def close(self) -> None:
        """End of the stream.  After a push flagged `last` it does nothing; otherwise one decode with t_upto = frames pushed
        finalises what the window still holds (an extension: the reference always knows its last frame, and this is not
        required to equal a flagged last push -- that one also builds the last frame's block with the look-ahead decode
        horizon).  Afterwards push / push_features raise."""
        if self._closed:
            return
        self._closed = True
        tg = self._tg
        if tg is not None and not self._collecting and tg.N > 0:
            with torch.no_grad():
                self._bind()
                self._h, self._sc = tg.decode(self._h, self._sc, None, self._frames, self.ret_win_size,
                                              use_hungarian=self.use_hungarian, next_t=None)

    # ---- the loop of infer.py:35-87, one timestep per call ------------------------------------------------------------
    def _bind(self) -> None:
        self._tg.bind_stream(self._X, self._ids, self._track, self._y_track, self._pos, self._ndets)

    def _advance(self, D: int, last: bool) -> None:
        t, lo = self._frames, self._ndets
        hi = lo + D
        self._frames, self._ndets = t + 1, hi
        with torch.no_grad():
            if self._collecting:
                if D:
                    self._pending.append((t, lo, hi))
                if len(self._pending) == 2:
                    self._start()
            else:
                self._bind()
                self._step(t, lo, hi, bool(last))
        if last:
            self._closed = True

    def _start(self) -> None:
        """initialize_graph over the two non-empty frames collected + the first model call (h = None).  At a re-initialisation
        the reference's loop stands at the timestep the graph emptied (`_restart_t`) and decodes from there (infer.py:62-87)."""
        (t0, lo0, hi0), (t1, lo1, hi1) = self._pending
        self._pending, self._collecting = [], False
        self._prev_tg = self._tg
        tg, feats = TrackGraph.start_stream(self.device, self._X, self._ids, self._track, self._y_track, self._pos, self._ndets,
                                            t0, (lo0, hi0), t1, (lo1, hi1))
        self._tg = tg
        scores, _, h, _ = self.model.forward_dgraph(feats, None, tg.graph)
        self._h, self._sc, self._h_cap = h, _pos_score(tg, scores, self.tp_classifier), 0
        if self._restart_t is not None:
            tc = self._restart_t
            self._h, self._sc = tg.decode(self._h, self._sc, None, tc - self.cur_win_size + 2, self.ret_win_size,
                                          use_hungarian=self.use_hungarian, next_t=tc + 1)
        self._restart_t = None

    def _step(self, t: int, lo: int, hi: int, last: bool) -> None:
        """A steady-state timestep: update(t) -> eval model call -> decode; through the native driver wherever
        `infer_sequence` would take it (loops._fast_greedy's rules, TrackGraph.greedy_run_fast's preconditions)."""
        tg = self._tg
        tg._t_range = {t: (lo, hi)}
        t_upto = t + 1 if last else t - self.cur_win_size + 2
        if not self._fast_known:
            self._fast, self._finfo, _ = _fast_greedy(self.model, self.use_hungarian, self.tp_classifier, None)
            self._fast_known = True
        if self._fast is not None:
            if self._step_info is None:
                self._step_info = self._finfo()
            r = tg.greedy_run_fast(self._fast, self._step_info, self._h, self._h_cap, [(t, t_upto, -1 if last else t + 1)],
                                   self.ret_win_size, self.use_hungarian, self.tp_classifier)
            if r is not None:
                self._h, self._sc, self._h_cap = r[:3]
                self.native_steps += 1
                return
        feats = tg._update_rows(self._sc, t, 'test', self.use_hungarian)
        n_added = int(feats.shape[0])
        scores, _, h, _ = self.model.forward_dgraph(feats, self._h, tg.graph)
        self._h_cap = 0
        sc = _pos_score(tg, scores, self.tp_classifier)
        self._h, self._sc = tg.decode(h, sc, None, t_upto, self.ret_win_size, use_hungarian=self.use_hungarian,
                                      next_t=None if last else t + 1)
        if n_added == 0 and self._h.shape[0] == 0:         # infer.py:62-68: the graph emptied -> collect two frames again
            self._collecting, self._pending, self._restart_t = True, [], t + 1
