"""The reference's two per-timestep loops, composed from the device-resident pieces.

    train_chunk     reference/train.py:54-135   one tracking chunk: initialize_graph -> model -> targets + CE + focal
                                                losses, then per timestep update_graph(mode='train') -> model -> losses
                                                (hidden state carried, BPTT), ONE backward for the chunk
    train_chunks    the same for B chunks at once: a prebuilt block-diagonal TrainBatch (train_batch.py), one forward per
                    call of the batch, the losses of every chunk kept apart (one windowed loss launch per call), ONE
                    backward for the B chunks
    train_epoch     train.py's epoch over a ChunkSampler (chunks.py): per slice of the epoch's order one device draw of augmented
                    chunks -> device batch build -> train_chunks -> optimizer step
    infer_sequence  reference/infer.py:35-87    one sequence: per timestep update_graph(mode='test', greedy or Hungarian)
                                                -> model -> decode_tracks (track finalisation + rolling-window deletion)
    validate        reference/train.py:177-282  the validation pass: infer_sequence over every sequence, then the CLEAR-MOT
                                                counts of all tracks in one launch (moteval.MotEvaluator) and one host read;
                                                with a monitor.ValMonitor the F1 of every forward call (train.py:278)
    validate_store, infer_store                 validate / infer_dataset over a seqfeat.SequenceFeatures: the sequences' features
                                                made on the device from the DetectionStore (the reference's val / test samples)

Same order of operations, same arguments' meaning and the same results as the reference's drivers (which cannot be imported:
they parse the command line at import) -- but the graph, the hidden state, the losses' inputs and the tracks stay
in HBM: `TrackGraph` (tracking.py), the batch-1 model path (`TrackMPNN.forward_dgraph`) and the HIP losses (loss.py).  The
drivers' prints are not part of the loop here or in the timings it is compared with; their training statistics (F1 per
forward, the epoch's loss means: train.py:86-88, :157-171) are kept on the device when `train_chunk` / `train_chunks` are
given a `TrainMonitor` (monitor.py) -- counts after every forward, one fold per chunk / per step, no host read in the loop.

`stages`, when given, is a dict that accumulates wall time per stage with a device synchronisation around each stage
(an instrumented pass: its total is larger than an un-instrumented one).
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Any, Dict, Optional

import numpy as np
import torch

from .loss import CELoss, FocalLoss, train_losses, train_losses_windows
from .tracking import TrackGraph
from .train_batch import AllChunksSkipped, _to_device


class _Stages:
    def __init__(self, acc: Optional[Dict[str, float]]):
        self.acc = acc
        self.t = 0.0

    def start(self):
        if self.acc is not None:
            torch.cuda.synchronize()
            self.t = time.perf_counter()

    def stop(self, name: str):
        if self.acc is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.acc[name] = self.acc.get(name, 0.0) + (now - self.t)
            self.t = now


def _loss_terms(tg: TrackGraph, scores, logits, ce, focal_node, focal_edge, tp_classifier: bool, return_targets: bool = False):
    """train.py:70-81 / :109-120 for one forward call."""
    # one autograd node for targets + CE + the focal terms (trackmpnn_amd.loss.train_losses: the same C entry points as the
    # CELoss / FocalLoss modules `ce`, `focal_node`, `focal_edge` -- train.py's gamma = 0, alpha = None -- would call one by one)
    # (the DeviceGraph itself: the one-launch losses take its arrays through the C struct, no tensor views)
    if return_targets:
        return train_losses(scores, logits, tg.labels_u8(), tg.graph, tp_classifier, return_targets=True)
    return train_losses(scores, logits, tg.labels_u8(), tg.graph, tp_classifier)


def train_chunk(model, X: torch.Tensor, y: torch.Tensor, device='cuda:0', tp_classifier: bool = True,
                stages: Optional[Dict[str, float]] = None, monitor=None):
    """One chunk of train.py:54-135 up to and including loss.backward().  X [1, ND, F], y [1, ND, 2] (host or device).
    Returns (loss, number of forward calls, sum of E over them) or None where the reference skips the chunk.
    monitor: a TrainMonitor (monitor.py) that takes the counts of every forward call and, after the backward, the chunk's
    loss_c / loss_f (train.py:86-88, :125-133); return values, loss and gradients are the ones without it."""
    st = _Stages(stages)
    ce, focal_node, focal_edge = CELoss(), FocalLoss(gamma=0, alpha=None), FocalLoss(gamma=0, alpha=None)
    st.start()
    init = TrackGraph.initialize(X, y, 0, 'train', device)
    if init is None:
        return None
    tg, feats, t_st, t_end = init
    st.stop('graph')
    scores, logits, h, _ = model.forward_dgraph(feats, None, tg.graph)
    st.stop('model_fwd')
    if monitor is None:
        loss_c, loss_f = _loss_terms(tg, scores, logits, ce, focal_node, focal_edge, tp_classifier)
    else:
        counts = monitor.new_counts(1 + t_end - t_st, 1, zero=True)      # (one forward per timestep at the most)
        loss_c, loss_f, targets = _loss_terms(tg, scores, logits, ce, focal_node, focal_edge, tp_classifier, True)
        monitor.count(counts, 0, scores, targets, tg.graph, tp_classifier)
    st.stop('targets_losses')
    ncalls, edge_iters = 1, tg.E
    t_skip = t_st
    for t_cur in range(t_st, t_end):
        if t_cur < t_skip:
            continue
        if feats.shape[0] == 0 and h.shape[0] == 0:            # train.py:95-100: nothing carried over -> start again
            init = TrackGraph.initialize(X, y, t_cur, 'train', device)
            if init is None:
                break
            tg, feats, t_skip, _ = init
            h = None
        else:
            feats = tg.update(None, X, y, t_cur, mode='train')
        st.stop('graph')
        scores, logits, h, _ = model.forward_dgraph(feats, h, tg.graph)
        st.stop('model_fwd')
        if monitor is None:
            lc, lf = _loss_terms(tg, scores, logits, ce, focal_node, focal_edge, tp_classifier)
        else:
            lc, lf, targets = _loss_terms(tg, scores, logits, ce, focal_node, focal_edge, tp_classifier, True)
            monitor.count(counts, ncalls, scores, targets, tg.graph, tp_classifier)
        loss_c, loss_f = loss_c + lc, loss_f + lf
        st.stop('targets_losses')
        ncalls += 1
        edge_iters += tg.E
    loss = loss_c + loss_f
    loss.backward()
    st.stop('backward')
    if monitor is not None:
        monitor.fold(counts, loss_c, loss_f)
    return loss, ncalls, edge_iters


def train_chunks(model, batch, Xs, tp_classifier: bool = True, stages: Optional[Dict[str, float]] = None, monitor=None):
    """B chunks of train.py:54-135 up to and including loss.backward(), on a TrainBatch (trackmpnn_amd.train_batch.
    build_train_batch: built once per set of chunks -- train-mode graphs depend on the labels only).  Xs: the chunks'
    features in the order of the `ys` the batch was built from (TrainBatch.stacked_features).  Every call of the batch runs
    through model.forward_graph with the state carried (reserve_rows set); after each call the windowed losses add every live
    chunk's terms; one backward.  The optimizer is not stepped (train_chunk's contract).

    Returns (loss, per_chunk [B, 2] (loss_c, loss_f of every chunk of the batch, detached), ncalls, edge_iters) where ncalls /
    edge_iters are the sums over the chunks of what train_chunk returns.  Semantics:
      * the gradient is the sum of the B chunks' gradients: one optimizer step per B chunks (at B = 1 exactly the reference's
        schedule: one chunk per step);
      * BatchNorm running statistics are updated once per (call, chunk with new rows) in call-major order, so after a batch
        they differ from running the B chunks one after another, except at B = 1.
    monitor: a TrainMonitor (monitor.py): one counting launch per call over the targets the windowed loss wrote, one fold per
    step (every (call, chunk) pair with rows is a forward; per_chunk's terms are the chunks' losses), `monitor.last_counts` =
    the step's counts [calls, 4, B].  No host read; loss, per_chunk and the gradients are the ones without it."""
    from .functional import weight_cache
    st = _Stages(stages)
    st.start()
    Xz = batch.stacked_features(Xs)
    st.stop('features')
    h = None
    acc_c = acc_f = None
    n = len(batch.plans)
    counts = None if monitor is None else monitor.new_counts(n, batch.B, zero=False)
    with weight_cache():        # the weights do not change between the forward calls of one step
        for c, plan in enumerate(batch.plans):
            x = Xz.index_select(0, batch.feat_src[c])
            nxt = batch.plans[c + 1].n_new if c + 1 < n else 0
            scores, logits, h, _ = model.forward_graph(x, h, plan, reserve_rows=nxt)
            st.stop('model_fwd')
            if monitor is None:
                lc, lf = train_losses_windows(scores, logits, batch.call_labels(c), plan, batch.windows[c], tp_classifier)
            else:
                lc, lf, targets = train_losses_windows(scores, logits, batch.call_labels(c), plan, batch.windows[c],
                                                       tp_classifier, return_targets=True)
                monitor.count_windows(counts, c, scores, targets, plan, batch.windows[c], tp_classifier)
            acc_c = lc if acc_c is None else acc_c + lc
            acc_f = lf if acc_f is None else acc_f + lf
            st.stop('targets_losses')
    loss = acc_c.sum() + acc_f.sum()
    loss.backward()
    st.stop('backward')
    if monitor is not None:
        monitor.fold(counts, acc_c, acc_f)
        monitor.last_counts = counts
    return loss, torch.stack([acc_c.detach(), acc_f.detach()], 1), batch.ncalls, batch.edge_iters


@dataclass
class VisTraining:
    """What train_epoch needs for a store with 'vis' features (the reference's default, train.py:132: loss_d + loss_c + loss_f)."""
    head: Any               # vishead.VisHead: the CNN's input size, down ratio and the 128 'vis' statistics
    frames: Any             # frames.FrameStore: the resized frames of the store's sequences, in the store's order
    embed_net: Any          # the embedding CNN: images [T, 3, H, W] -> maps [T, 128, Hm, Wm] with a grad_fn (any callable: a
                            # torch module, or espnet.EspTrainNet, whose forward and backward run on the library's kernels)
    embed_opt: Any          # its optimizer (zero_grad / step next to the tracker's): torch.optim.Adam or BucketAdam over its parameters
    embed_loss: Any = 'identity'    # loss_d: 'identity' (FairMOTLoss), 'embedding' or an embedloss.EmbeddingLoss (its deltas)


def train_epoch(model, sampler, opt, batch_size: int, epoch: int, tp_classifier: bool = True, monitor=None, scheduler=None,
                vis: Optional[VisTraining] = None) -> int:
    """One epoch of train.py:54-135 over a ChunkSampler (trackmpnn_amd.chunks): `sampler.epoch_order(epoch)` in slices of
    `batch_size`, per slice draw -> DrawnChunks.batch() -> opt.zero_grad() -> train_chunks -> opt.step().  Every draw of the
    epoch uses step = epoch: a chunk's draw is keyed by (seed, step, chunk index) and a chunk comes up once per epoch, so the
    augmented data of an epoch do not depend on batch_size.  A slice in which the reference would skip every chunk (the
    build's AllChunksSkipped) takes no step.  `scheduler`, if given, is stepped once at the end (train.py:330's StepLR
    over `opt`; BucketAdam has no epoch step of its own).  Returns the number of optimizer steps.  A composition only: the
    waits for the device are the build's two per step.

    A store with 'vis' features needs `vis` (a VisTraining).  Per slice: drawn.batch() first (a slice whose chunks are all
    skipped runs no CNN), images = vis.frames.gather(drawn.plan), maps = vis.embed_net(images), loss_d =
    drawn.attach_vis(vis.head, maps) (the rows into the last 128 columns of X, detached as the reference's features.detach()),
    both optimizers' zero_grad, train_chunks, loss_d[batch.kept].sum().backward() (the identity loss of the chunks the batch
    kept: the reference `continue`s past a skipped chunk before its backward, train.py:56-67), both optimizers' step.
    vis.embed_loss chooses loss_d: the identity loss (the default) or the reference's EmbeddingLoss over the gathered logits.
    With vis.embed_net an espnet.EspTrainNet the step holds no torch CNN: its decoder tail trains with frozen statistics.
    The monitor takes the kept chunks' loss_d in one launch (TrainMonitor.fold_embed: 'avg_loss_d' and 'avg_loss_total', the
    reference's "Average embedding loss for epoch" and its total, train.py:157-171)."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'train_epoch: batch_size={batch_size}')
    if sampler.store.vis and vis is None:
        raise ValueError("train_epoch: the sampler's store draws 'vis' features: pass vis=VisTraining(head, frames, embed_net, "
                         'embed_opt)')
    if vis is not None and not sampler.store.vis:
        raise ValueError("train_epoch: vis= was given, but the sampler's store was built without 'vis' features")
    order = sampler.epoch_order(epoch)
    steps = 0
    for s in range(0, len(order), batch_size):
        idx = order[s:s + batch_size]
        if len(idx) == 0:
            continue
        drawn = sampler.draw(idx, epoch)
        try:
            batch = drawn.batch()
        except AllChunksSkipped:
            continue
        if vis is not None:
            loss_d = drawn.attach_vis(vis.head, vis.embed_net(vis.frames.gather(drawn.plan)), embed_loss=vis.embed_loss)
            vis.embed_opt.zero_grad()
        opt.zero_grad()
        train_chunks(model, batch, drawn.features(batch), tp_classifier, monitor=monitor)
        if vis is not None:
            kept = _to_device(batch.kept, loss_d.device)
            if monitor is not None:
                monitor.fold_embed(loss_d, kept)
            loss_d.index_select(0, kept).sum().backward()
            vis.embed_opt.step()
        opt.step()
        steps += 1
    if scheduler is not None:
        scheduler.step()
    return steps


def infer_sequence(model, X: torch.Tensor, y: torch.Tensor, cur_win_size: int = 5, ret_win_size: int = 0,
                   use_hungarian: bool = False, device='cuda:0', tp_classifier: bool = True,
                   stages: Optional[Dict[str, float]] = None, monitor=None, att_monitor=None):
    """One sequence of infer.py:35-87 (model in eval mode).  Returns (y_out [ND, 2] int64 as the reference keeps it, number
    of forward calls, sum of E over them).
    monitor: a ValMonitor (monitor.py) that counts every forward call as the validation pass does (train.py:207-219, :241-253):
    one more launch behind each model call -- the first call, the calls after a re-initialisation and every update call, a
    timestep without new detections included -- before the decode, on the native driver's timesteps as on the composed ones;
    no host read, and tracks, call count and edge count are the ones without it.
    att_monitor: a monitor.AttentionMonitor that counts the attention weights of every model call INSIDE the timestep loop --
    the calls after a re-initialisation included, the first call of the sequence not: the set attention_weights.py:172-174
    stores -- before the decode.  One launch per call and group of 8 heads, no host read; models with heads run the composed
    timesteps, and a model without heads raises ValueError at the first counted call.  None: nothing changes."""
    st = _Stages(stages)
    yy = y[0].detach().cpu().numpy().astype('int64')
    y_out = yy.copy()
    y_out[:, 1] = -1
    fast, finfo, h_cap = _fast_greedy(model, use_hungarian, tp_classifier, stages)
    if att_monitor is not None:
        fast = None                                            # (every counted call hands its attention to the monitor)
    with torch.no_grad():
        st.start()
        init = TrackGraph.initialize(X, y, 0, 'test', device)
        if init is None:
            return y_out, 0, 0
        tg, feats, t_st, t_end = init
        st.stop('graph')
        scores, logits, h, _ = model.forward_dgraph(feats, None, tg.graph)
        if monitor is not None:
            monitor.count(tg, scores, tp_classifier)
        sc = _pos_score(tg, scores, tp_classifier)
        st.stop('model_fwd')
        ncalls, edge_iters = 1, tg.E
        step_info = None
        done = []                                              # TrackGraphs abandoned by a re-initialisation
        t_skip = t_st
        n_added = int(feats.shape[0])                          # rows the last update added (feats.shape[0] of infer.py:62)
        for t_cur in range(t_st, t_end):
            if t_cur < t_skip:
                continue
            if n_added == 0 and h.shape[0] == 0:               # infer.py:62-68: the graph emptied -> initialise again
                init = TrackGraph.initialize(X, y, t_cur, 'test', device)
                if init is None:
                    break
                done.append(tg)
                prev = tg
                tg, feats, t_skip, _ = init
                tg.y_track.copy_(prev.y_track)                 # (the tracks finalised so far belong to the sequence)
                h = None
                n_added = int(feats.shape[0])
            else:
                t_upto = t_end if t_cur == t_end - 1 else t_cur - cur_win_size + 2
                if fast is not None and h is not None:
                    # steady state: the whole timestep (append, model call, decode, the one host read) in the native driver.
                    # Its model descriptor is built once per sequence (eval mode under no_grad: the parameters cannot change
                    # inside this call; the per-step field, the row count, is overwritten by the driver) -- building it
                    # sits between the host read of one timestep and the first launch of the next, i.e. on the critical path
                    if step_info is None:
                        step_info = finfo()
                    # every remaining timestep is offered: the driver runs them back to back and stops in front of the first
                    # one it does not take (no detections, a graph beyond the one-launch kernels, ...)
                    steps = [(t, t_end if t == t_end - 1 else t - cur_win_size + 2, t + 1 if t + 1 < t_end else -1)
                             for t in range(t_cur, t_end)]
                    r = tg.greedy_run_fast(fast, step_info, h, h_cap, steps, ret_win_size, use_hungarian, tp_classifier,
                                           monitor=monitor)
                    if r is not None:
                        h, sc, h_cap, n_done, edges = r
                        n_added = 1                            # (a native step only runs with D_t > 0 new detections)
                        ncalls += n_done
                        edge_iters += edges
                        t_skip = t_cur + n_done                # (the loop variable moves past the timesteps that ran)
                        continue
                feats = tg.update(sc, X, y, t_cur, mode='test', use_hungarian=use_hungarian)
                n_added = int(feats.shape[0])
            st.stop('graph')
            scores, logits, h, att = model.forward_dgraph(feats, h, tg.graph)
            h_cap = 0
            if monitor is not None:
                monitor.count(tg, scores, tp_classifier)         # (before the decode deletes rows and flips the row sets)
            if att_monitor is not None:
                att_monitor.count(tg, att)
            sc = _pos_score(tg, scores, tp_classifier)
            st.stop('model_fwd')
            ncalls += 1
            edge_iters += tg.E
            t_upto = t_end if t_cur == t_end - 1 else t_cur - cur_win_size + 2
            h, sc = tg.decode(h, sc, None, t_upto, ret_win_size, use_hungarian=use_hungarian,
                              next_t=t_cur + 1 if t_cur + 1 < t_end else None)
            st.stop('decode')
        y_out[:, 1] = tg.tracks()[:y_out.shape[0]]
        st.stop('decode')
    return y_out, ncalls, edge_iters


def infer_dataset(model, sequences, results, cur_win_size: int = 5, ret_win_size: int = 0, use_hungarian: bool = False,
                  tp_classifier: bool = True) -> list:
    """infer.py's loop over the sequences (infer.py:35-97) up to the result tables: the model in eval mode for the pass (its
    mode is restored afterwards), infer_sequence over every sequence, then one `results.apply` and one `results.read()`.
    sequences: one dict per sequence with 'X' [1, ND, F] and 'y' [1, ND, 2] as infer_sequence takes them; results: a
    results.TrackResults built over the same sequences in the same order (its store holds their frames, categories and scores).
    A sequence without detections is skipped as infer.py:38-40 skips it: it runs no inference and has None in the list.
    Returns what results.read() returns: per sequence the dict of results_host; results.write_kitti(out_dir, per) /
    write_bdd(out_dir, per) write the files from it."""
    store = results.store
    if len(sequences) != store.S:
        raise ValueError(f'infer_dataset: {len(sequences)} sequences, the results hold {store.S}')
    was_training = model.training
    model.eval()
    try:
        tracks = []
        for s, q in enumerate(sequences):
            X, y = q['X'], q['y']
            if int(y.shape[1]) != int(store.seq[s, 3]):
                raise ValueError(f'infer_dataset: sequence {s} has {int(y.shape[1])} detections, the results hold {int(store.seq[s, 3])}')
            if int(X.shape[1]) == 0:
                tracks.append(None)
                continue
            y_out, _, _ = infer_sequence(model, X, y, cur_win_size, ret_win_size, use_hungarian, results.device, tp_classifier)
            tracks.append(y_out[:, 1])
        results.apply(tracks)
        return results.read()
    finally:
        model.train(was_training)


def validate(model, sequences, evaluator, cur_win_size: int = 5, ret_win_size: int = 0, use_hungarian: bool = False,
             tp_classifier: bool = True, map_evaluator=None, monitor=None, hota_evaluator=None, results=None, prep=None,
             att_monitor=None) -> Dict:
    """The validation pass of train.py:177-282 up to the MOTA that chooses the checkpoint (train.py:300): the model in eval
    mode for the pass (its mode is restored afterwards), infer_sequence over every sequence, all tracks handed to
    `evaluator.evaluate` and read once.  sequences: one dict per sequence with 'X' [1, ND, F] and 'y' [1, ND, 2] as
    infer_sequence takes them; `evaluator`: a MotEvaluator built over the same sequences in the same order (its store holds
    their frames, boxes and ground truth).  A sequence without detections or without ground truth is skipped as
    train.py:190-192 skips it, and so is one in which no graph could be initialised (train.py:201-202): it runs no
    inference and has None in `per_sequence`.

    Returns {'mota', 'motp', 'motas', 'per_sequence'} and the overall counts (objects, predictions, matches, switches,
    false_positives, misses, frames, dist_sum, recall, precision): the overall figures are the ratios of the summed counts
    (train.py:282), `motas` the MOTA of every sequence that took part (train.py:281), as fractions -- train.py prints 100 x.
    map_evaluator: a mapeval.MapEvaluator built over the same sequences in the same order (or None: nothing more is done
    and nothing more returned).  It is handed the same track list -- the sequences left out of the MOTA are left out of the
    mAP (train.py:272-273) -- and the result gains 'map' (train.py:286, as a fraction) and 'aps' (class -> AP).
    The result is whatever the evaluator produces: one built with identity=True adds the rest of the MOT-challenge summary
    (unique_objects, mostly_tracked, partially_tracked, mostly_lost, fragmentations, idtp, idfp, idfn, idp, idr, idf1) to the
    overall figures and to every dict of `per_sequence`; no argument here changes.
    monitor: a monitor.ValMonitor (or None: nothing more is done and nothing more returned).  It is reset, counts every forward
    call of every sequence that runs (one launch each, on either inference path; a skipped sequence contributes none) and is
    read once, after the evaluator: the result gains 'f1' (train.py:278, the mean over the forwards, as a fraction) and
    'f1_forwards'.
    hota_evaluator: a hota.HotaEvaluator built over the same sequences in the same order (or None: nothing more is done and
    nothing more returned).  It is handed the same track list and read after the other evaluators: the result gains 'hota',
    'deta', 'assa', 'loca', 'detre', 'detpr', 'assre', 'asspr' (hota_overall's means over the alphas, as fractions) and
    'hota_per_sequence' (the dicts of hota_host, None for a sequence left out).
    results: a results.TrackResults built over the same sequences in the same order (or None: nothing more is done and nothing
    more returned).  The tracks go through `results.apply` first and every evaluator scores `results.filtered_tracks()` -- the
    tracks a submission would contain (infer.py:91-96), handed over on the device; the result gains 'results', the counts
    (kept_rows, kept_tracks, removed_rows, removed_tracks) summed over the sequences that took part, read after the evaluators.
    prep: an evalprep.EvalPrep built over the same sequences in the same order (or None: nothing more is done and nothing more
    returned); the evaluators are then to be built over `prep.eval_sequences()`, the ground truth the benchmark scores.  After
    `results.apply`, if any, the tracks go through `prep.apply` and every evaluator scores `prep.filtered_tracks()` -- the rows
    the KITTI benchmark scores for the class of prep.rules, handed over on the device; the result gains 'prep', the counts of
    evalprep_host (rows_in, other_class, the four removal counts, kept) summed over the sequences that took part, read last.
    att_monitor: a monitor.AttentionMonitor (or None: nothing more is done and nothing more returned).  It is reset, counts the
    model calls inside the timestep loop of every sequence that runs (infer_sequence) and is read once, after the evaluators:
    the result gains 'att_hist', the dict of AttentionMonitor.read()."""
    store = evaluator.store
    if prep is not None and [int(n) for n in prep.store.seq[:, 3]] != [int(n) for n in store.seq[:, 3]]:
        raise ValueError('validate: prep was not built over the sequences of evaluator')
    if results is not None and [int(n) for n in results.store.seq[:, 3]] != [int(n) for n in store.seq[:, 3]]:
        raise ValueError('validate: results was not built over the sequences of evaluator')
    if len(sequences) != store.S:
        raise ValueError(f'validate: {len(sequences)} sequences, the evaluator holds {store.S}')
    if map_evaluator is not None and [int(n) for n in np.diff(map_evaluator.store.det_base)] != [int(n) for n in store.seq[:, 3]]:
        raise ValueError('validate: map_evaluator was not built over the sequences of evaluator')
    if hota_evaluator is not None and [int(n) for n in hota_evaluator.store.seq[:, 3]] != [int(n) for n in store.seq[:, 3]]:
        raise ValueError('validate: hota_evaluator was not built over the sequences of evaluator')
    was_training = model.training
    model.eval()
    if monitor is not None:
        monitor.reset()
    if att_monitor is not None:
        att_monitor.reset()
    try:
        tracks = []
        for s, q in enumerate(sequences):
            X, y = q['X'], q['y']
            if int(y.shape[1]) != int(store.seq[s, 3]):
                raise ValueError(f'validate: sequence {s} has {int(y.shape[1])} detections, the evaluator holds {int(store.seq[s, 3])}')
            if store.empty[s]:
                tracks.append(None)
                continue
            y_out, ncalls, _ = infer_sequence(model, X, y, cur_win_size, ret_win_size, use_hungarian, evaluator.device,
                                              tp_classifier, monitor=monitor, att_monitor=att_monitor)
            tracks.append(y_out[:, 1] if ncalls > 0 else None)
        if results is not None:
            results.apply(tracks)
            tracks = [None if t is None else f for t, f in zip(tracks, results.filtered_tracks())]
        if prep is not None:
            prep.apply(tracks)
            tracks = [None if t is None else f for t, f in zip(tracks, prep.filtered_tracks())]
        evaluator.evaluate(tracks)
        if map_evaluator is not None:
            map_evaluator.evaluate(tracks)
        if hota_evaluator is not None:
            hota_evaluator.evaluate(tracks)
        per, overall = evaluator.read()
        mres = map_evaluator.read() if map_evaluator is not None else None
        vres = monitor.read() if monitor is not None else None
        hres = hota_evaluator.read() if hota_evaluator is not None else None
        rres = results.read() if results is not None else None
        pres = prep.read() if prep is not None else None
        ares = att_monitor.read() if att_monitor is not None else None
    finally:
        model.train(was_training)
    out = dict(overall)
    out['motas'] = [p['mota'] for p in per if p is not None]
    out['per_sequence'] = per
    if mres is not None:
        out['map'] = mres['map']
        out['aps'] = dict(zip(mres['classes'], mres['ap']))
    if vres is not None:
        out['f1'] = vres['f1']
        out['f1_forwards'] = vres['forwards']
    if hres is not None:
        out.update({k: hres[1][k] for k in ('hota', 'deta', 'assa', 'loca', 'detre', 'detpr', 'assre', 'asspr')})
        out['hota_per_sequence'] = hres[0]
    if rres is not None:
        from .results import results_overall
        out['results'] = results_overall(rres)
    if pres is not None:
        out['prep'] = pres[1]
    if ares is not None:
        out['att_hist'] = ares
    return out


@dataclass
class VisInference:
    """What validate_store / infer_store need for a store with 'vis' features (the counterpart of VisTraining without an
    optimizer: the embedding net is only evaluated)."""
    head: Any               # vishead.VisHead: the CNN's input size, down ratio and the 128 'vis' statistics
    frames: Any             # frames.FrameStore: the resized frames of the store's sequences, in the store's order
    embed_net: Any          # the embedding CNN: images [T, 3, H, W] -> maps [T, 128, Hm, Wm]
    frames_per_batch: int = 8


def _store_sequences(what: str, sf, vis: Optional[VisInference]) -> list:
    """The dicts of every sequence of sf's store: sf.build, with 'vis' sf.attach_vis, then sf.check()."""
    if sf.store.vis and vis is None:
        raise ValueError(f"{what}: the store holds 'vis' features: pass vis=VisInference(head, frames, embed_net)")
    if vis is not None and not sf.store.vis:
        raise ValueError(f"{what}: vis= was given, but the store was built without 'vis' features")
    sequences = sf.build(frames_per_batch=8 if vis is None else vis.frames_per_batch)
    if vis is not None:
        sf.attach_vis(vis.head, vis.frames, vis.embed_net, vis.frames_per_batch)
    sf.check()                  # (no extra stall: the first thing infer_sequence does is read y on the host)
    return sequences


def validate_store(model, sf, evaluator, vis: Optional[VisInference] = None, **kw) -> Dict:
    """`validate` over every sequence of a seqfeat.SequenceFeatures: sf.build() (one launch), for a store with 'vis' features
    sf.attach_vis(vis.head, vis.frames, vis.embed_net, vis.frames_per_batch) -- after every epoch the embedding net has moved
    and the visual columns are made anew --, then validate(model, sequences, evaluator, **kw).  `evaluator` (and whatever else
    **kw hands to validate) is built over the store's sequences in the store's order.  A 'vis' store without vis= raises, and
    vis= without a 'vis' store raises, as train_epoch does."""
    return validate(model, _store_sequences('validate_store', sf, vis), evaluator, **kw)


def infer_store(model, sf, results, vis: Optional[VisInference] = None, **kw) -> list:
    """`infer_dataset` over every sequence of a seqfeat.SequenceFeatures: the features as validate_store makes them, then
    infer_dataset(model, sequences, results, **kw)."""
    return infer_dataset(model, _store_sequences('infer_store', sf, vis), results, **kw)


def _fast_greedy(model, use_hungarian: bool, tp_classifier: bool, stages):
    """(native module, call-descriptor factory, 0) where a steady-state greedy timestep can run in csrc_host/fast_iter.cpp's
    greedy_step: models on the fused batch-1 path without attention heads, eval mode, greedy or (where the device solver takes
    the sequence's problems: the driver checks per timestep) Hungarian association, with or without the TP
    classifier (without: the iteration writes 1 as every detection's score, infer.py:77-80), no per-stage instrumentation;
    (None, None, 0) otherwise."""
    from .small import fast_module, plan_small_route
    sp = getattr(model, '_small', None)
    if stages is not None or model.training or sp is None:
        return None, None, 0
    fast = fast_module()
    # the route of a one-row call with nothing to differentiate: the driver issues the calls forward_dgraph would
    r = plan_small_route(sp.eligible, sp.att, getattr(model, '_padded', False), 1, 1, False, False, False, False, False, False,
                         fast is not None)
    if (r.path, r.node, r.grads, r.padded) != ('fused', 'native', 'none', False) or not hasattr(fast, 'greedy_run'):
        return None, None, 0

    class _G:                     # fast_info() only reads .N of the graph it is given (overwritten per step by the driver)
        N = 0

    def finfo():
        params = model._param_list()
        return sp.fast_info(params, _G, sp.params(params), False, False, False, 0)

    return fast, finfo, 0


def _pos_score(tg: TrackGraph, scores: torch.Tensor, tp_classifier: bool) -> torch.Tensor:
    """P(positive) per row; without the TP classifier every detection counts as a true positive (infer.py:53-56)."""
    sc = scores[:, 0]
    if not tp_classifier:
        sc = sc.clone()
        sc[tg.graph.frame_graph().det_row.long()] = 1.0
    return sc
