"""Batched chunk training on the MI355X (-m gpu): the windowed loss kernel (tmpnn_train_losses_win_*) against the one-launch
loss on every window's own subgraph, train_chunks against train_chunk chunk by chunk, the reference's chunk fixtures inside a
batch, and the batch's graphs / labels against TrackGraph's at B = 1."""

import numpy as np
import pytest
import torch

from tests.conftest import chunk_golden_names
from tests.golden_util import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _chunks(n, seed):
    from trackmpnn_amd import synth_window
    return [synth_window(seed * 1000 + s, 7, 6.0, 20) for s in range(n)]


def _with_gaps(y, drop=(3,), shift_from=5, shift=2):
    y = y[~np.isin(y[:, 0], drop)].copy()
    y[y[:, 0] >= shift_from, 0] += shift
    return y


def _mixed_chunks(n, seed):
    """C2-shaped chunks with empty timesteps, different lengths and one chunk the reference skips."""
    from trackmpnn_amd import synth_window
    ys = _chunks(n, seed)
    for i in range(0, n, 7):
        ys[i] = _with_gaps(ys[i], drop=(2 + i % 3,), shift_from=4, shift=1 + i % 2)
    for i in range(3, n, 11):
        ys[i] = synth_window(seed * 1000 + 500 + i, 3 + i % 4, 6.0, 20)
    ys[n // 2] = np.array([[0, -1], [0, -1], [1, -1], [2, -1]])
    return ys


def _subgraph(plan, w, b):
    """(global rows ascending, FrameGraph on DEV) of window b of a call: its own graph, rows renumbered in order."""
    from trackmpnn_amd import graph_from_edges
    g = plan.graph
    dptr, eptr = w.det_ptr.cpu().numpy(), w.edge_ptr.cpu().numpy()
    didx = w.det_idx.cpu().numpy()[dptr[b]:dptr[b + 1]]
    eidx = w.edge_idx.cpu().numpy()[eptr[b]:eptr[b + 1]]
    drow = g.det_row.cpu().numpy()[didx]
    erow = g.edge_row.cpu().numpy()[eidx]
    rows = np.sort(np.concatenate([drow, erow]))
    loc = np.full(g.N, -1, np.int64)
    loc[rows] = np.arange(rows.size)
    is_edge = np.zeros(rows.size, bool)
    is_edge[loc[erow]] = True
    src = loc[g.src.cpu().numpy()[eidx]]
    dst = loc[g.dst.cpu().numpy()[eidx]]
    assert (src >= 0).all() and (dst >= 0).all()
    sub = graph_from_edges(rows.size, torch.from_numpy(is_edge), torch.from_numpy(src), torch.from_numpy(dst), device=DEV)
    return torch.from_numpy(rows).to(DEV), sub


def _win_out(plan, w, logits, scores, labels, tp):
    """out [4][W] of tmpnn_train_losses_win_fwd (the focal sums are not autograd outputs)."""
    from trackmpnn_amd import _lib
    g = plan.graph
    lib = _lib.load()
    n_ws = int(lib.tmpnn_train_losses_win_ws(w.cref()))
    out = torch.empty((4, w.W), device=DEV)
    stats = torch.empty((max(g.Dn, 1) * 8,), device=DEV)
    ws = torch.empty((n_ws,), device=DEV)
    targets = torch.empty_like(labels)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call('tmpnn_train_losses_win_fwd', g.cref(), w.cref(), logits.data_ptr(), scores.data_ptr(), labels.data_ptr(), int(tp),
              targets.data_ptr(), stats.data_ptr(), out.data_ptr(), ws.data_ptr(), n_ws, st)
    return out


def _one_launch_out(sub, logits, scores, labels, tp):
    from trackmpnn_amd import _lib
    lib = _lib.load()
    assert lib.tmpnn_train_losses_supported(sub.E, sub.Dn)
    n_ws = int(lib.tmpnn_train_losses_ws(sub.E, sub.Dn))
    out = torch.empty((4,), device=DEV)
    stats = torch.empty((max(sub.Dn, 1) * 8,), device=DEV)
    ws = torch.empty((n_ws,), device=DEV)
    targets = torch.empty_like(labels)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call('tmpnn_train_losses_fwd', sub.cref(), logits.data_ptr(), scores.data_ptr(), labels.data_ptr(), int(tp),
              targets.data_ptr(), stats.data_ptr(), out.data_ptr(), ws.data_ptr(), n_ws, st)
    return out


def _ulp_diff(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _windowed(batch, c, logits, scores, tp, gc, gf):
    from trackmpnn_amd import train_losses_windows
    lg = logits.clone().requires_grad_(True)
    sc = scores.clone().requires_grad_(True)
    lc, lf = train_losses_windows(sc, lg, batch.call_labels(c), batch.plans[c], batch.windows[c], tp)
    ((lc * gc).sum() + (lf * gf).sum()).backward()
    return lc.detach(), lf.detach(), lg.grad, sc.grad


@pytest.mark.parametrize('tp', [True, False])
def test_windowed_loss_equals_the_one_launch_loss_per_window(tp):
    from trackmpnn_amd import build_train_batch
    from trackmpnn_amd.loss import train_losses
    batch = build_train_batch(_mixed_chunks(70, seed=31), DEV)
    assert batch.B >= 64
    gen = torch.Generator().manual_seed(5)
    checked = 0
    for c, (plan, w) in enumerate(zip(batch.plans, batch.windows)):
        N = plan.graph.N
        logits = (3 * torch.randn(N, 1, generator=gen)).to(DEV)
        scores = (0.02 + 0.96 * torch.rand(N, 1, generator=gen)).to(DEV)
        gc = torch.randn(batch.B, generator=gen).to(DEV)
        gf = torch.randn(batch.B, generator=gen).to(DEV)
        labels = batch.call_labels(c)
        out = _win_out(plan, w, logits, scores, labels, tp).cpu()
        lc, lf, dl, ds = _windowed(batch, c, logits, scores, tp, gc, gf)
        lc2, lf2, dl2, ds2 = _windowed(batch, c, logits, scores, tp, gc, gf)        # a second run: bitwise the same
        assert torch.equal(lc, lc2) and torch.equal(lf, lf2) and torch.equal(dl, dl2) and torch.equal(ds, ds2)
        assert torch.equal(lc.cpu(), out[0]) and torch.equal(lf.cpu(), out[3])
        dl, ds = dl.reshape(-1), ds.reshape(-1)
        covered = torch.zeros(N, dtype=torch.bool, device=DEV)
        for b in range(batch.B):
            if c >= batch.ncalls_b[b]:
                assert (out[:, b] == 0).all()
                continue
            rows, sub = _subgraph(plan, w, b)
            covered[rows] = True
            sl, ss, sb = logits[rows].contiguous(), scores[rows].contiguous(), labels[rows].contiguous()
            ref = _one_launch_out(sub, sl.reshape(-1), ss.reshape(-1), sb, tp).cpu()
            assert torch.equal(out[:3, b], ref[:3]), (c, b, out[:, b], ref)
            assert _ulp_diff(out[3, b], ref[3]) <= 2, (c, b, out[3, b], ref[3])
            rl = sl.clone().requires_grad_(True)
            rs = ss.clone().requires_grad_(True)
            rc, rf = train_losses(rs, rl, sb, sub, tp)
            (rc * gc[b] + rf * gf[b]).backward()
            assert torch.equal(dl[rows], rl.grad.reshape(-1)), (c, b)
            assert torch.equal(ds[rows], rs.grad.reshape(-1)), (c, b)
            checked += 1
        assert not dl[~covered].any() and not ds[~covered].any()          # rows of finished chunks: zero gradient
    assert checked >= 64 * 5


@pytest.mark.parametrize('tp', [True, False])
def test_windowed_loss_on_a_window_beyond_the_one_launch_limit(tp):
    """A window of more than 8192 edge rows (the one-launch loss's limit): the separate entry points within 1e-6 relative."""
    from trackmpnn_amd import build_train_batch, synth_window
    from trackmpnn_amd.loss import train_losses
    big = synth_window(8080, 3, 100.0, 110, dropout=0.05)
    batch = build_train_batch([big] + _chunks(3, seed=41), DEV)
    plan, w = batch.plans[0], batch.windows[0]
    assert int(w.edge_ptr[1]) > 8192
    gen = torch.Generator().manual_seed(6)
    N = plan.graph.N
    logits = (3 * torch.randn(N, 1, generator=gen)).to(DEV)
    scores = (0.02 + 0.96 * torch.rand(N, 1, generator=gen)).to(DEV)
    gc, gf = torch.randn(batch.B, generator=gen).to(DEV), torch.randn(batch.B, generator=gen).to(DEV)
    lc, lf, dl, ds = _windowed(batch, 0, logits, scores, tp, gc, gf)
    out = _win_out(plan, w, logits, scores, batch.call_labels(0), tp).cpu()
    rows, sub = _subgraph(plan, w, 0)
    from trackmpnn_amd import _lib
    assert not _lib.load().tmpnn_train_losses_supported(sub.E, sub.Dn)
    rl = logits[rows].clone().requires_grad_(True)
    rs = scores[rows].clone().requires_grad_(True)
    rc, rf = train_losses(rs, rl, batch.call_labels(0)[rows].contiguous(), sub, tp)
    (rc * gc[0] + rf * gf[0]).backward()
    for a, r in ((lc[0], rc.detach()), (lf[0], rf.detach())):
        assert abs(float(a) - float(r)) <= 1e-6 * abs(float(r)), (float(a), float(r))
    torch.testing.assert_close(dl.reshape(-1)[rows], rl.grad.reshape(-1), rtol=1e-6, atol=0)
    torch.testing.assert_close(ds.reshape(-1)[rows], rs.grad.reshape(-1), rtol=1e-6, atol=0)
    assert torch.isfinite(out).all()


def _perturbed_model(nhidden=64, heads=0, seed=9):
    from trackmpnn_amd import TrackMPNN
    torch.manual_seed(seed)
    model = TrackMPNN('2d', 3, nhidden, heads, 'diff')
    gp = torch.Generator().manual_seed(17)
    with torch.no_grad():                                       # scores on both sides of 0.5 (as bench.py's loop block)
        for k, prm in model.named_parameters():
            prm.add_(0.1 * torch.randn(prm.shape, generator=gp))
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=gp))
    return model.to(DEV).train()


@pytest.mark.parametrize('tp', [True, False])
def test_train_chunks_equals_train_chunk_one_by_one(tp, monkeypatch):
    from trackmpnn_amd import build_train_batch, loops
    from trackmpnn_amd.loops import train_chunk, train_chunks
    ys = _mixed_chunks(64, seed=51)
    gen = torch.Generator().manual_seed(52)
    Xs = [torch.randn(y.shape[0], 8, generator=gen) for y in ys]
    model = _perturbed_model()
    # sequential: train_chunk per chunk, gradients summed over the chunks, the loss terms recorded per chunk
    terms = []
    orig = loops._loss_terms

    def rec(*a, **k):
        lc, lf = orig(*a, **k)
        terms[-1][0].append(lc.detach())
        terms[-1][1].append(lf.detach())
        return lc, lf

    monkeypatch.setattr(loops, '_loss_terms', rec)
    model.zero_grad(set_to_none=True)
    seq, ncalls, edges = {}, 0, 0
    for i, (X, y) in enumerate(zip(Xs, ys)):
        terms.append(([], []))
        r = train_chunk(model, X[None], torch.from_numpy(y)[None], DEV, tp)
        if r is None:
            continue
        ncalls += r[1]
        edges += r[2]
        seq[i] = (sum(float(v) for v in terms[-1][0]), sum(float(v) for v in terms[-1][1]))
    monkeypatch.setattr(loops, '_loss_terms', orig)
    g_seq = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    batch = build_train_batch(ys, DEV)
    assert sorted(seq) == list(batch.kept) and len(batch.skipped) == 1
    assert (batch.ncalls_b != batch.ncalls_b[0]).any() and any(wc.n_new == 0 for calls in batch.chunk_calls for wc in calls)
    model.zero_grad(set_to_none=True)
    loss, per_chunk, nc, ne = train_chunks(model, batch, Xs, tp)
    assert (nc, ne) == (ncalls, edges)
    pc = per_chunk.cpu().double().numpy()
    for b, i in enumerate(batch.kept):
        for k in range(2):
            assert abs(pc[b, k] - seq[i][k]) <= 1e-4 * abs(seq[i][k]), (i, k, pc[b, k], seq[i][k])
    total = sum(a + b for a, b in seq.values())
    assert abs(float(loss.detach()) - total) <= 1e-4 * abs(total)
    gmax = max(float(g.abs().max()) for g in g_seq.values())
    for k, p in model.named_parameters():
        err = float((p.grad - g_seq[k]).abs().max())
        assert err <= 2e-4 * gmax, (k, err, gmax)


@pytest.mark.parametrize('name', chunk_golden_names())
def test_reference_chunk_inside_a_batch(name):
    """A chunk the real reference ran (fixture chunk_*), in the fixture's mode (with the TP classifier or without), as one
    window of a 17-chunk batch: the windowed loss's terms of every call within 1e-4 relative of the reference's, the targets it
    wrote equal to the reference's create_targets on every row the window lists, the window's scores closer to the reference's
    than the fixture's min_margin and its counts equal to the reference's tp / fp / fn, the gradients of the window's loss alone.
    Then as a batch of one through train_chunks with a monitor: loss_c, loss_f and the total, gradients (a parameter the
    reference leaves at zero holds a zero tensor), BatchNorm buffers, and the windowed counts of every call against the
    reference's tp / fp / fn."""
    from tests.golden_util import assert_chunk_buffers, assert_chunk_grads, chunk_tp
    from tests.test_parity_gpu import build_model
    from trackmpnn_amd import TrainMonitor, build_train_batch, classification_counts_windows, train_losses_windows
    from trackmpnn_amd.functional import weight_cache
    from trackmpnn_amd.loops import train_chunks
    gold = Golden(name)
    m, tp = gold.meta, chunk_tp(gold)
    X, y = gold.t('X')[0], gold.t('y')[0].numpy()
    ys = _mixed_chunks(16, seed=61)
    ys[8] = _chunks(1, seed=62)[0]                               # (no skipped chunk here: 16 kept)
    gen = torch.Generator().manual_seed(63)
    Xs = [torch.randn(yy.shape[0], X.shape[1], generator=gen) for yy in ys]
    pos = 5
    ys.insert(pos, y)
    Xs.insert(pos, X)
    batch = build_train_batch(ys, DEV)
    b = int(np.nonzero(batch.kept == pos)[0][0])
    assert batch.B >= 16 and batch.ncalls_b[b] == m['ncalls']
    model = build_model(dict(m, mode='train'), gold.params())
    # the loop by hand, keeping every call's per-window terms; then the backward of the fixture window's loss alone
    Xz = batch.stacked_features([x.to(DEV) for x in Xs])
    h, acc_c, acc_f, per_call, worst = None, 0, 0, [], 0.0
    with weight_cache():
        for c, plan in enumerate(batch.plans):
            nxt = batch.plans[c + 1].n_new if c + 1 < len(batch.plans) else 0
            scores, logits, h, _ = model.forward_graph(Xz.index_select(0, batch.feat_src[c]), h, plan, reserve_rows=nxt)
            lc, lf, targets = train_losses_windows(scores, logits, batch.call_labels(c), plan, batch.windows[c], tp,
                                                   return_targets=True)
            per_call.append((float(lc[b].detach()), float(lf[b].detach())))
            acc_c, acc_f = acc_c + lc, acc_f + lf
            if c < m['ncalls']:
                rows, _ = _subgraph(plan, batch.windows[c], b)      # the window's rows ascending = the chunk's own row order
                assert torch.equal(targets[rows].cpu(), gold.t(f'c{c}/targets')), c
                # scores closer to the reference's than the smallest |score - 0.5| it counted: the same predictions, so the
                # same counts
                worst = max(worst, float((scores.detach()[rows, 0].cpu() - gold.t(f'c{c}/scores')).abs().max()))
                cnt = classification_counts_windows(scores, targets, plan, batch.windows[c], tp)[:, b].cpu().numpy()
                assert tuple(cnt[:3]) == tuple(gold.d['counts'][c]) and cnt[3] == rows.numel(), (c, cnt, gold.d['counts'][c])
    print(f'{name}: max |score - reference score| {worst:.2e}, min_margin {m["min_margin"]:.2e}')
    # (worst < min_margin carries the weight: the margins of the fixtures committed first are below 1e-4)
    assert worst < m['min_margin'] and worst <= 1e-4, (worst, m['min_margin'])
    model.zero_grad(set_to_none=True)
    (acc_c[b] + acc_f[b]).backward()
    ref = gold.d['per_call']
    for c in range(m['ncalls']):
        for k in range(2):
            assert abs(per_call[c][k] - ref[c, k]) <= 1e-4 * abs(ref[c, k]), (c, k, per_call[c][k], ref[c, k])
    assert_chunk_grads(model, gold)
    # B = 1: train_chunks is the reference's schedule -- loss, gradients and the BatchNorm buffers after the chunk
    model = build_model(dict(m, mode='train'), gold.params())
    one = build_train_batch([y], DEV)
    model.zero_grad(set_to_none=True)
    mon = TrainMonitor(DEV)
    loss, per_chunk, ncalls, _ = train_chunks(model, one, X.to(DEV), tp, monitor=mon)
    assert ncalls == m['ncalls']
    ref_c, ref_f = float(gold.d['loss_c']), float(gold.d['loss_f'])
    assert abs(float(loss.detach()) - (ref_c + ref_f)) <= 1e-4 * abs(ref_c + ref_f)
    assert tuple(per_chunk.shape) == (1, 2)
    for got, r in zip(per_chunk[0].tolist(), (ref_c, ref_f)):
        assert abs(got - r) <= 1e-4 * abs(r), (got, r)
    assert_chunk_grads(model, gold)
    assert_chunk_buffers(model, gold)
    counts = mon.last_counts.cpu().numpy()
    assert counts.shape == (m['ncalls'], 4, 1)
    assert np.array_equal(counts[:, :3, 0], gold.d['counts']) and np.array_equal(counts[:, 3, 0], ref[:, 2].astype(np.int64))


def _b1_cases():
    from trackmpnn_amd import synth_window
    out = [(n, None) for n in chunk_golden_names()]
    out += [('gaps', _with_gaps(synth_window(71, 9, 5.0, 12), drop=(2, 5), shift_from=7, shift=2)), ('c2', _chunks(1, 72)[0])]
    return out


@pytest.mark.parametrize('case', range(len(chunk_golden_names()) + 2))
def test_batch_of_one_equals_track_graph(case):
    """At B = 1 every call's graph and labels are the ones train_chunk's composition (TrackGraph, mode='train') produces."""
    from trackmpnn_amd import TrackGraph, build_train_batch
    name, y = _b1_cases()[case]
    if y is None:
        y = Golden(name).t('y')[0].numpy()
    X = torch.randn(1, y.shape[0], 8)
    yt = torch.from_numpy(y)[None]
    batch = build_train_batch([y], DEV)
    tg, feats, t_st, t_end = TrackGraph.initialize(X, yt, 0, 'train', DEV)
    assert len(batch.plans) == 1 + t_end - t_st
    for c, plan in enumerate(batch.plans):
        if c > 0:
            tg.update(None, X, yt, t_st + c - 1, mode='train')
        g, lab, q = tg.graph.frame_graph(), tg.labels_u8(), plan.graph
        assert (g.N, g.E, g.Dn) == (q.N, q.E, q.Dn), c
        for f in ('src', 'dst', 'edge_row', 'det_row', 'rowptr', 'inc', 'is_edge'):
            assert torch.equal(getattr(g, f).cpu(), getattr(q, f).cpu()), (c, f)
        assert torch.equal(lab.reshape(-1).cpu(), batch.call_labels(c).cpu()), c


def test_attention_head_model_runs_through_train_chunks():
    from trackmpnn_amd import build_train_batch
    from trackmpnn_amd.loops import train_chunks
    ys = _mixed_chunks(12, seed=81)
    Xs = torch.randn(sum(y.shape[0] for y in ys), 8, generator=torch.Generator().manual_seed(82))
    model = _perturbed_model(64, 2)
    batch = build_train_batch(ys, DEV)
    loss, per_chunk, ncalls, edges = train_chunks(model, batch, Xs.to(DEV), tp_classifier=False)
    assert torch.isfinite(loss) and torch.isfinite(per_chunk).all() and ncalls == batch.ncalls
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
