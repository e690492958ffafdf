"""The training monitor on the MI355X (-m gpu): classification counts per forward (tmpnn_cls_counts, tmpnn_cls_counts_win) and
the running record (tmpnn_train_record_fold, TrainMonitor) against a numpy definition on the very scores the kernels read.

Host definition: pred = s > 0.5 (fp32, strict); tp / fp / fn over the det + edge rows of a window (edge rows alone without the
TP classifier), rows = det + edge rows; F1 = 2 tp / (2 tp + fp + fn) in fp64, 0 on a zero denominator.  Where sklearn
imports, F1 is also held to f1_score(..., zero_division=0)."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests.conftest import chunk_golden_names, loss_golden_names
from tests.golden_util import Golden
from tests.test_train_batch_gpu import _mixed_chunks, _perturbed_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

try:
    from sklearn.metrics import f1_score as _sk_f1
except Exception:                                   # (sklearn is optional: only the cross-check against it is left out)
    _sk_f1 = None


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


# ---- the host definition ---------------------------------------------------------------------------------------------------
def _f1(c):
    tp, fp, fn = int(c[0]), int(c[1]), int(c[2])
    den = 2 * tp + fp + fn
    return 2 * tp / den if den else 0.0


def _host_counts(scores, targets, drow, erow, tp):
    """int32 [4] of one graph / window; scores fp32 [N], targets [N] (numpy), drow / erow: its det / edge rows."""
    rows = np.concatenate([drow, erow]) if tp else erow
    pred = scores[rows] > np.float32(0.5)
    t = targets[rows] != 0
    c = np.array([(pred & t).sum(), (pred & ~t).sum(), (~pred & t).sum(), drow.size + erow.size], np.int32)
    if _sk_f1 is not None:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            assert _sk_f1(t.astype(np.int64), pred.astype(np.int64), zero_division=0) == _f1(c)
    return c


def _window_rows(plan, w):
    """[(det rows, edge rows)] per window of a call, from its LossWindows lists."""
    g = plan.graph
    dptr, eptr = w.det_ptr.cpu().numpy(), w.edge_ptr.cpu().numpy()
    didx, eidx = w.det_idx.cpu().numpy(), w.edge_idx.cpu().numpy()
    drow, erow = g.det_row.cpu().numpy(), g.edge_row.cpu().numpy()
    return [(drow[didx[dptr[b]:dptr[b + 1]]], erow[eidx[eptr[b]:eptr[b + 1]]]) for b in range(w.W)]


def _host_counts_windows(plan, w, scores, targets, tp):
    s = scores.detach().reshape(-1).cpu().numpy()
    t = targets.reshape(-1).cpu().numpy()
    return np.stack([_host_counts(s, t, dr, er, tp) for dr, er in _window_rows(plan, w)], 1)       # [4, W]


def _record(m):
    raw = m.record.cpu().numpy()
    f = raw.view(np.float64)
    return dict(sum_f1=float(f[0]), forwards=int(raw[1]), sum_loss_c=float(f[2]), sum_loss_f=float(f[3]),
                sum_loss=float(f[4]), chunks=int(raw[5]))


def _inputs(seed=51):
    ys = _mixed_chunks(64, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    Xs = [torch.randn(y.shape[0], 8, generator=gen) for y in ys]
    return ys, Xs


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


# ---- 2. windowed counts -----------------------------------------------------------------------------------------------------
def test_windowed_counts_are_exact():
    from trackmpnn_amd import (build_train_batch_device, classification_counts_windows, create_targets,
                               train_losses_windows)
    ys = _mixed_chunks(64, seed=21)
    # every detection its own track: all dets true positives, no positive edge anywhere
    ys.append(np.array([[t, 3 * t + k] for t in range(4) for k in range(3)], np.int64))
    batch = build_train_batch_device(ys, DEV)
    bx = int(np.nonzero(batch.kept == len(ys) - 1)[0][0])
    assert batch.B == 64
    gen = torch.Generator().manual_seed(22)
    live = 0
    tot = {True: np.zeros(3, np.int64), False: np.zeros(3, np.int64)}
    zero_den = 0
    for c, (plan, w) in enumerate(zip(batch.plans, batch.windows)):
        N = plan.graph.N
        rows = _window_rows(plan, w)
        scores = 0.02 + 0.96 * torch.rand(N, 1, generator=gen)
        crafted = torch.from_numpy(np.concatenate(rows[bx])).long()
        scores[crafted] *= 0.49                                             # the crafted chunk's rows: below 0.5
        scores = scores.to(DEV)
        logits = (3 * torch.randn(N, 1, generator=gen)).to(DEV)
        labels = batch.call_labels(c)
        listed = torch.from_numpy(np.concatenate([np.concatenate(r) for r in rows])).long().to(DEV)
        ref_t = create_targets(labels, plan.graph, as_bytes=True)
        for tp in (True, False):
            lc, lf, targets = train_losses_windows(scores, logits, labels, plan, w, tp, return_targets=True)
            lc2, lf2 = train_losses_windows(scores, logits, labels, plan, w, tp)
            assert torch.equal(lc, lc2) and torch.equal(lf, lf2)
            assert targets.dtype == torch.uint8 and targets.shape == labels.shape
            assert torch.equal(targets[listed], ref_t[listed]), (c, tp)
            dev = classification_counts_windows(scores, targets, plan, w, tp)
            assert dev.dtype == torch.int32 and dev.shape == (4, batch.B) and dev.is_cuda
            host = _host_counts_windows(plan, w, scores, targets, tp)
            assert torch.equal(dev.cpu(), torch.from_numpy(host)), (c, tp)
            tot[tp] += host[:3].sum(1)
            has_rows = host[3] > 0
            zero_den += int(((2 * host[0] + host[1] + host[2] == 0) & has_rows).sum())
            assert (host[:, ~has_rows] == 0).all()
            if tp:
                live += int(has_rows.sum())
                assert (has_rows == (c < batch.ncalls_b)).all()
            else:
                assert (host[:3, bx] == 0).all() and (host[3, bx] > 0) == (c < batch.ncalls_b[bx])
    assert live == batch.ncalls
    for tp in (True, False):                                               # the inputs are not degenerate
        assert (tot[tp] > 0).all(), (tp, tot[tp])
    assert zero_den >= 1


# ---- 3. one graph = one window, on the reference's own targets ----------------------------------------------------------------
@pytest.mark.parametrize('name', loss_golden_names())
def test_one_graph_counts_on_the_reference_targets(name):
    from trackmpnn_amd import LossWindows, classification_counts, classification_counts_windows, graph_from_adjacency
    from trackmpnn_amd.loss import train_losses
    gold = Golden(name)
    gen = torch.Generator().manual_seed(33)
    i32 = lambda a: torch.as_tensor(a, dtype=torch.int32, device=DEV)
    for c in range(gold.ncalls):
        na = gold.adjacency(c, 'node_adj').to(DEV)
        labels, logits, targets = gold.t(f'c{c}/labels'), gold.t(f'c{c}/logits'), gold.t(f'c{c}/targets')
        g = graph_from_adjacency(na)
        N = g.N
        scores = (0.02 + 0.96 * torch.rand(N, 1, generator=gen)).to(DEV)
        drow, erow = g.det_row.cpu().numpy(), g.edge_row.cpu().numpy()
        one = LossWindows(1, g.Dn, g.E, i32([0, g.Dn]), i32(np.arange(g.Dn)), i32([0, g.E]), i32(np.arange(g.E)),
                          i32(np.zeros(g.Dn)), i32(np.zeros(g.E)))
        for tp in (True, False):
            _, _, t8 = train_losses(scores, logits.to(DEV), labels.to(DEV), g, tp, return_targets=True)
            assert t8.dtype == torch.uint8 and torch.equal(t8.cpu().long(), targets.reshape(-1).long()), (c, tp)
            host = _host_counts(scores.reshape(-1).cpu().numpy(), targets.reshape(-1).numpy(), drow, erow, tp)
            dev = classification_counts(scores, targets.to(DEV), g, tp)                 # the reference's int64 targets
            assert dev.dtype == torch.int32 and dev.shape == (4,)
            assert torch.equal(dev.cpu(), torch.from_numpy(host)), (c, tp, dev, host)
            assert torch.equal(classification_counts(scores, t8, na, tp), dev)          # bytes; the adjacency itself
            win = classification_counts_windows(scores, t8, g, one, tp)
            assert torch.equal(win.reshape(-1), dev), (c, tp)


# ---- 4. a monitor changes nothing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tp', [True, False])
def test_a_monitor_changes_nothing(tp):
    from trackmpnn_amd import TrainMonitor, build_train_batch
    from trackmpnn_amd.loops import train_chunk, train_chunks
    ys, Xs = _inputs()
    model = _perturbed_model()
    batch = build_train_batch(ys, DEV)
    model.zero_grad(set_to_none=True)
    loss0, pc0, nc0, ne0 = train_chunks(model, batch, Xs, tp)
    g0 = _grads(model)
    model.zero_grad(set_to_none=True)
    m = TrainMonitor(DEV)
    loss1, pc1, nc1, ne1 = train_chunks(model, batch, Xs, tp, monitor=m)
    assert torch.equal(loss0.detach(), loss1.detach()) and torch.equal(pc0, pc1) and (nc0, ne0) == (nc1, ne1)
    for k, g in _grads(model).items():
        assert torch.equal(g, g0[k]), k
    # batch 1: three chunks, gradients summed over them
    picks = [0, 3, 7]
    outs = []
    for mon in (None, TrainMonitor(DEV)):
        model.zero_grad(set_to_none=True)
        res = [train_chunk(model, Xs[i][None], torch.from_numpy(ys[i])[None], DEV, tp, monitor=mon) for i in picks]
        outs.append((res, _grads(model)))
    for r0, r1 in zip(outs[0][0], outs[1][0]):
        assert torch.equal(r0[0].detach(), r1[0].detach()) and r0[1:] == r1[1:]
    for k, g in outs[1][1].items():
        assert torch.equal(g, outs[0][1][k]), k


# ---- 5. batched and one by one ------------------------------------------------------------------------------------------------
def _batched_by_hand(model, batch, Xs, tp):
    """The calls as train_chunks runs them; host counts [C, 4, B] from every call's own scores and targets."""
    from trackmpnn_amd import train_losses_windows
    from trackmpnn_amd.functional import weight_cache
    Xz = batch.stacked_features(Xs)
    h, out = None, []
    n = len(batch.plans)
    with weight_cache():
        for c, plan in enumerate(batch.plans):
            nxt = batch.plans[c + 1].n_new if c + 1 < n else 0
            scores, logits, h, _ = model.forward_graph(Xz.index_select(0, batch.feat_src[c]), h, plan, reserve_rows=nxt)
            _, _, targets = train_losses_windows(scores, logits, batch.call_labels(c), plan, batch.windows[c], tp,
                                                 return_targets=True)
            out.append(_host_counts_windows(plan, batch.windows[c], scores, targets, tp))
    return np.stack(out)


def _chunk_by_hand(model, X, y, tp):
    """One chunk as train_chunk runs it (no backward): [(device counts, host counts)] per forward."""
    from trackmpnn_amd import TrackGraph, classification_counts
    from trackmpnn_amd.loss import train_losses
    out = []

    def forward(tg, feats, h):
        scores, logits, h, _ = model.forward_dgraph(feats, h, tg.graph)
        _, _, targets = train_losses(scores, logits, tg.labels_u8(), tg.graph, tp, return_targets=True)
        dev = classification_counts(scores, targets, tg.graph, tp)
        fg = tg.graph.frame_graph()
        host = _host_counts(scores.detach().reshape(-1).cpu().numpy(), targets.cpu().numpy(), fg.det_row.cpu().numpy(),
                            fg.edge_row.cpu().numpy(), tp)
        out.append((dev.cpu().numpy(), host))
        return h

    tg, feats, t_st, t_end = TrackGraph.initialize(X, y, 0, 'train', DEV)
    h = forward(tg, feats, None)
    t_skip = t_st
    for t_cur in range(t_st, t_end):
        if t_cur < t_skip:
            continue
        if feats.shape[0] == 0 and h.shape[0] == 0:
            init = TrackGraph.initialize(X, y, t_cur, 'train', DEV)
            if init is None:
                break
            tg, feats, t_skip, _ = init
            h = None
        else:
            feats = tg.update(None, X, y, t_cur, mode='train')
        h = forward(tg, feats, h)
    return out


@pytest.mark.parametrize('tp', [True, False])
def test_batched_and_one_by_one_tell_the_same_story(tp):
    from trackmpnn_amd import TrainMonitor, build_train_batch
    from trackmpnn_amd.loops import train_chunk, train_chunks
    ys, Xs = _inputs()
    model = _perturbed_model()
    batch = build_train_batch(ys, DEV)
    m1, mB = TrainMonitor(DEV), TrainMonitor(DEV)
    model.zero_grad(set_to_none=True)
    for X, y in zip(Xs, ys):
        train_chunk(model, X[None], torch.from_numpy(y)[None], DEV, tp, monitor=m1)
    model.zero_grad(set_to_none=True)
    train_chunks(model, batch, Xs, tp, monitor=mB)
    r1, rB = m1.read(), mB.read()
    assert isinstance(r1['forwards'], int) and isinstance(rB['chunks'], int)
    assert r1['forwards'] == rB['forwards'] == batch.ncalls
    assert r1['chunks'] == rB['chunks'] == batch.B
    for k in ('avg_loss_c', 'avg_loss_f', 'avg_loss'):
        assert abs(r1[k] - rB[k]) <= 1e-4 * abs(r1[k]), (k, r1[k], rB[k])
    assert 0.0 < r1['avg_f1'] < 1.0 and 0.0 < rB['avg_f1'] < 1.0
    # the batched path against the host definition on its own scores
    host = _batched_by_hand(model, batch, Xs, tp)
    last = mB.last_counts
    assert last.dtype == torch.int32 and tuple(last.shape) == (len(batch.plans), 4, batch.B) and last.is_cuda
    assert torch.equal(last.cpu(), torch.from_numpy(host))
    for c in range(len(batch.plans)):
        is_fwd = c < batch.ncalls_b
        assert (host[c][:, ~is_fwd] == 0).all() and (host[c][3, is_fwd] > 0).all()
    f1s = [_f1(host[c, :, b]) for c in range(host.shape[0]) for b in range(batch.B) if host[c, 3, b] > 0]
    assert len(f1s) == batch.ncalls
    assert abs(rB['avg_f1'] - math.fsum(f1s) / len(f1s)) <= (len(f1s) ** 2 + len(f1s)) * 2.0 ** -53
    # batch 1 against the host definition on its own scores: three chunks by hand, then train_chunk with a monitor
    picks = [1, 7, 12]
    total_f1, forwards = 0.0, 0
    for i in picks:
        acc = 0.0                                            # (the fold's order: a chunk's forwards in sequence, then the record)
        for dev, hc in _chunk_by_hand(model, Xs[i][None], torch.from_numpy(ys[i])[None], tp):
            assert (dev == hc).all() and hc[3] > 0, (i, dev, hc)
            acc += _f1(hc)
            forwards += 1
        total_f1 += acc
    m = TrainMonitor(DEV)
    model.zero_grad(set_to_none=True)
    sum_loss = 0.0
    for i in picks:
        loss, ncalls, _ = train_chunk(model, Xs[i][None], torch.from_numpy(ys[i])[None], DEV, tp, monitor=m)
        sum_loss += float(loss.detach())
    rec = _record(m)
    assert rec['forwards'] == forwards and rec['chunks'] == len(picks)
    assert rec['sum_f1'] == total_f1
    assert rec['sum_loss'] == sum_loss
    assert m.last_counts is None                              # (the per-chunk tensor belongs to batched steps)


# ---- 6. the record ------------------------------------------------------------------------------------------------------------
def test_the_record_is_right():
    from trackmpnn_amd import TrainMonitor, build_train_batch
    from trackmpnn_amd.loops import train_chunks
    ys, Xs = _inputs()
    model = _perturbed_model()
    batch = build_train_batch(ys, DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    m = TrainMonitor(DEV)
    f1s, lcs, lfs, ls = [], [], [], []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        _, per_chunk, _, _ = train_chunks(model, batch, Xs, monitor=m)
        opt.step()
        cnt = m.last_counts.cpu().numpy()
        f1s += [_f1(cnt[c, :, b]) for c in range(cnt.shape[0]) for b in range(cnt.shape[2]) if cnt[c, 3, b] > 0]
        pc = per_chunk.cpu().numpy()
        assert pc.dtype == np.float32
        lcs += [float(v) for v in pc[:, 0]]
        lfs += [float(v) for v in pc[:, 1]]
        ls += [float(np.float32(c + f)) for c, f in pc]
    r = m.read()
    assert r['forwards'] == len(f1s) == 2 * batch.ncalls and r['chunks'] == len(ls) == 2 * batch.B
    bound = lambda x: (len(x) ** 2 + len(x)) * 2.0 ** -53 * max(abs(v) for v in x)
    for key, x in (('avg_f1', f1s), ('avg_loss_c', lcs), ('avg_loss_f', lfs), ('avg_loss', ls)):
        exact = math.fsum(x)
        assert abs(r[key] * len(x) - exact) <= bound(x), (key, r[key] * len(x), exact, bound(x))
        assert abs(r[key] - exact / len(x)) <= bound(x), (key, r[key], exact / len(x))
    rec = _record(m)
    assert abs(rec['sum_f1'] - math.fsum(f1s)) <= bound(f1s) and abs(rec['sum_loss'] - math.fsum(ls)) <= bound(ls)
    # reset: zero counts, and the means of nothing are NaN (no division by zero)
    m.reset()
    z = m.read()
    assert z['forwards'] == 0 and z['chunks'] == 0
    assert all(math.isnan(z[k]) for k in ('avg_f1', 'avg_loss_c', 'avg_loss_f', 'avg_loss'))
    assert not m.record.cpu().numpy().any()


# ---- 7. no new waits ------------------------------------------------------------------------------------------------------------
def _sync_warnings(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    return [str(w.message) for w in rec if 'called a synchronizing' in str(w.message)]


def test_a_monitored_step_waits_no_more_than_a_plain_one():
    from trackmpnn_amd import TrainMonitor, build_train_batch_device
    from trackmpnn_amd.loops import train_chunks
    ys, Xs = _inputs()
    model = _perturbed_model()
    batch = build_train_batch_device(ys, DEV)
    Xd = torch.cat(Xs).to(DEV)
    m = TrainMonitor(DEV)
    plain = lambda: train_chunks(model, batch, Xd)
    watched = lambda: train_chunks(model, batch, Xd, monitor=m)
    for _ in range(2):                                        # warm: plans, allocators, code objects
        plain()
        watched()
    torch.cuda.synchronize()
    n_plain = _sync_warnings(plain)
    n_watched = _sync_warnings(watched)
    assert len(n_watched) == len(n_plain), (n_plain, n_watched)
    assert len(_sync_warnings(m.read)) >= 1


# ---- 8. repeatable ------------------------------------------------------------------------------------------------------------
def test_two_monitored_runs_give_the_same_bits():
    from trackmpnn_amd import TrainMonitor, build_train_batch
    from trackmpnn_amd.loops import train_chunks
    ys, Xs = _inputs()
    model = _perturbed_model()
    batch = build_train_batch(ys, DEV)
    runs = []
    for _ in range(2):
        m = TrainMonitor(DEV)
        model.zero_grad(set_to_none=True)
        train_chunks(model, batch, Xs, monitor=m)
        runs.append((m.last_counts.clone(), m.record.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert int(runs[0][1][1]) == batch.ncalls


# ---- 9. the reference's chunks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', chunk_golden_names())
def test_reference_chunk_with_a_monitor(name, monkeypatch):
    """train_chunk with a TrainMonitor on a chunk the real reference ran, in the fixture's mode (with the TP classifier, or
    without: train.py:80-88 counts edge rows only).  Besides the losses and gradients: the targets of every forward equal the
    reference's create_targets on every row; the scores the counts are taken from lie closer to the reference's than the
    fixture's min_margin (the smallest |score - 0.5| over the counted rows), so no prediction can differ; the monitor's counts
    of every forward equal the reference's tp / fp / fn; its F1 equals the mean of sklearn's values as closely as this file
    holds the fold to its host definition ((n^2 + n) 2^-53 over n forwards)."""
    from tests.golden_util import LossTermsRecorder, assert_chunk_grads, chunk_tp
    from tests.test_parity_gpu import build_model
    from trackmpnn_amd import TrainMonitor
    from trackmpnn_amd.loops import train_chunk
    gold = Golden(name)
    meta, tp = gold.meta, chunk_tp(gold)
    model = build_model(dict(meta, mode='train'), gold.params())
    model.train()
    X, y = gold.t('X'), gold.t('y')
    model.zero_grad(set_to_none=True)
    m = TrainMonitor(DEV)
    held, orig_new = [], m.new_counts

    def new_counts(*a, **k):                                   # (the chunk's counts tensor: train_chunk folds it and lets it go)
        held.append(orig_new(*a, **k))
        return held[-1]

    monkeypatch.setattr(m, 'new_counts', new_counts)
    with LossTermsRecorder() as rec:
        loss, ncalls, _ = train_chunk(model, X, y, DEV, tp, monitor=m)
    calls = []
    for call in rec.calls:
        assert call['tp_classifier'] is tp
        calls.append((call['scores'], call['targets'], call['loss_c'], call['loss_f'], call['det_row'], call['edge_row']))
    assert ncalls == meta['ncalls'] == len(calls) and len(held) == 1
    ref_total = float(gold.d['loss_c']) + float(gold.d['loss_f'])
    assert abs(float(loss.detach()) - ref_total) <= 1e-4 * abs(ref_total), (float(loss.detach()), ref_total)
    assert_chunk_grads(model, gold)
    per_call, ref_counts, ref_f1 = gold.d['per_call'], gold.d['counts'], gold.d['f1']
    counts = held[0].cpu().numpy()
    assert counts.shape == (ncalls, 4, 1)
    worst = 0.0
    for c, (scores, targets, lc, lf, drow, erow) in enumerate(calls):
        for k, got in enumerate((float(lc), float(lf))):
            assert abs(got - per_call[c, k]) <= 1e-4 * abs(per_call[c, k]), (c, k, got, per_call[c, k])
        assert targets.dtype == torch.uint8 and torch.equal(targets.cpu(), gold.t(f'c{c}/targets')), c
        counted = torch.cat([drow, erow]) if tp else erow
        worst = max(worst, float((scores[counted].cpu() - gold.t(f'c{c}/scores')[counted.cpu()]).abs().max()))
        assert tuple(counts[c, :3, 0]) == tuple(ref_counts[c]), (c, counts[c, :, 0], ref_counts[c])
        assert counts[c, 3, 0] == int(per_call[c, 2]), c
        assert abs(_f1(counts[c, :, 0]) - ref_f1[c]) <= 1e-12, c
    print(f'{name}: max |score - reference score| over the counted rows {worst:.2e}, min_margin {meta["min_margin"]:.2e}')
    # (worst < min_margin is what rules out a differing prediction -- the margins of the fixtures committed first are below
    #  the 1e-4 the scores are held to elsewhere, so that bound alone would not)
    assert worst < meta['min_margin'] and worst <= 1e-4, (worst, meta['min_margin'])
    r = m.read()
    assert r['forwards'] == meta['ncalls'] and r['chunks'] == 1
    assert abs(r['avg_loss_c'] - float(gold.d['loss_c'])) <= 1e-4 * abs(float(gold.d['loss_c']))
    assert abs(r['avg_loss_f'] - float(gold.d['loss_f'])) <= 1e-4 * abs(float(gold.d['loss_f']))
    assert abs(r['avg_loss'] - ref_total) <= 1e-4 * abs(ref_total)
    n = len(ref_f1)
    assert abs(r['avg_f1'] - math.fsum(ref_f1) / n) <= (n ** 2 + n) * 2.0 ** -53, (r['avg_f1'], math.fsum(ref_f1) / n)
