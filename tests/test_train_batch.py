"""Batched chunk training, host side (no GPU): trackmpnn_amd.train_batch.build_train_batch against WindowBuilder + batch_windows,
the reference chunks' call counts and row counts, empty timesteps, skipped chunks and the loss-window lists."""
import numpy as np
import pytest
import torch

from tests.conftest import chunk_golden_names
from tests.golden_util import Golden
from trackmpnn_amd import WindowBuilder, batch_windows, build_train_batch, synth_window


def _chunks(n, seed=0):
    return [synth_window(seed * 1000 + s, 7, 6.0, 20) for s in range(n)]


def _with_gaps(y, drop=(3,), shift_from=5, shift=2):
    y = y[~np.isin(y[:, 0], drop)].copy()
    y[y[:, 0] >= shift_from, 0] += shift
    return y


def test_plans_equal_window_builder_and_batch_windows():
    ys = _chunks(12, seed=3) + [synth_window(77, 4, 3.0, 6)]
    batch = build_train_batch(ys)
    calls = [WindowBuilder(y).calls() for y in ys]
    assert all(len(a) == len(b) for a, b in zip(calls, batch.chunk_calls))
    plans, _ = batch_windows(calls)
    assert len(plans) == len(batch.plans)
    for p, q in zip(plans, batch.plans):
        assert (p.n_new, p.min_seg_cnt, p.max_seg_nd) == (q.n_new, q.min_seg_cnt, q.max_seg_nd)
        for f in ('new_det_local', 'new_det_row', 'seg_ptr', 'seg_cnt', 'seg_of_new', 'seg_of_det'):
            assert torch.equal(getattr(p, f), getattr(q, f)), f
        for f in ('src', 'dst', 'edge_row', 'det_row', 'rowptr', 'inc', 'is_edge', 'pos', 'src_pos', 'dst_pos', 'det_order'):
            assert torch.equal(getattr(p.graph, f), getattr(q.graph, f)), f
    assert batch.skipped == [] and list(batch.kept) == list(range(len(ys)))


def test_default_calls_unchanged_by_the_new_keyword():
    for y in _chunks(6, seed=5) + [_with_gaps(synth_window(9, 9, 5.0, 12))]:
        a, b = WindowBuilder(y).calls(), WindowBuilder(y).calls(empty_calls=False)
        assert len(a) == len(b)
        for p, q in zip(a, b):
            assert p.n_new == q.n_new
            for f in ('new_is_edge', 'new_src', 'new_dst', 'det_ids'):
                assert np.array_equal(getattr(p, f), getattr(q, f)) and getattr(p, f).dtype == getattr(q, f).dtype


@pytest.mark.parametrize('name', chunk_golden_names())
def test_reference_chunks_call_and_row_counts(name):
    gold = Golden(name)
    batch = build_train_batch([gold.t('y')])
    assert batch.ncalls == gold.meta['ncalls'] == len(batch.plans)
    assert [p.graph.N for p in batch.plans] == [int(v) for v in gold.d['per_call'][:, 2]]
    assert batch.edge_iters == sum(p.graph.E for p in batch.plans)


def test_chunk_with_gaps_gets_a_call_per_timestep():
    y = _with_gaps(synth_window(21, 8, 5.0, 12), drop=(3,), shift_from=5, shift=2)     # timesteps 3, 5, 6 empty
    times = np.unique(y[:, 0])
    t1, tN = int(times[1]), int(times[-1])
    batch = build_train_batch([y])
    assert batch.ncalls == 1 + tN - t1 == len(batch.plans)
    for c, t in enumerate(range(t1 + 1, tN + 1), start=1):
        empty = not (y[:, 0] == t).any()
        assert (batch.plans[c].n_new == 0) == empty, t
        if empty:
            assert batch.plans[c].graph.N == batch.plans[c - 1].graph.N
    non_empty = WindowBuilder(y).calls()
    assert sum(1 for wc in batch.chunk_calls[0] if wc.n_new > 0) == len(non_empty)


def test_skipped_chunks_are_reported():
    good = synth_window(5, 5, 4.0, 8)
    one_step = np.array([[2, 0], [2, 1], [2, -1]])
    all_fp = np.array([[0, -1], [0, -1], [1, -1], [2, -1]])
    empty = np.zeros((0, 2), np.int64)
    batch = build_train_batch([one_step, good, all_fp, empty, good])
    assert batch.skipped == [0, 2, 3]
    assert list(batch.kept) == [1, 4] and batch.B == 2
    assert batch.det_offset[-1] == sum(len(y) for y in (one_step, good, all_fp, empty, good))
    with pytest.raises(ValueError):
        build_train_batch([one_step, all_fp])


def test_loss_windows_cover_every_live_row_once():
    ys = _chunks(9, seed=7)
    ys[2] = _with_gaps(ys[2])
    ys[4] = synth_window(404, 4, 5.0, 10)                 # shorter chunk: finished before the others
    ys.insert(6, np.array([[0, -1], [1, -1]]))           # skipped
    batch = build_train_batch(ys)
    row_win = np.full(batch.plans[-1].graph.N, -1)
    off = 0
    for c, plan in enumerate(batch.plans):               # window of every row from the chunks' own calls, call-major
        for b, calls in enumerate(batch.chunk_calls):
            if c < len(calls):
                row_win[off:off + calls[c].n_new] = b
                off += calls[c].n_new
    edges = 0
    for c, (plan, w) in enumerate(zip(batch.plans, batch.windows)):
        g = plan.graph
        live = np.nonzero(c < batch.ncalls_b)[0]
        dwin, ewin = row_win[g.det_row.numpy()], row_win[g.edge_row.numpy()]
        dptr, didx = w.det_ptr.numpy(), w.det_idx.numpy()
        eptr, eidx = w.edge_ptr.numpy(), w.edge_idx.numpy()
        assert w.W == batch.B and (w.n_det, w.n_edge) == (dptr[-1], eptr[-1])
        for b in range(batch.B):
            ds, es = didx[dptr[b]:dptr[b + 1]], eidx[eptr[b]:eptr[b + 1]]
            if b in live:
                assert np.array_equal(ds, np.nonzero(dwin == b)[0]) and np.array_equal(es, np.nonzero(ewin == b)[0])
                assert ds.size > 0 and es.size > 0
            else:
                assert ds.size == 0 and es.size == 0
        assert np.array_equal(w.det_win.numpy(), np.where(np.isin(dwin, live), dwin, -1))
        assert np.array_equal(w.edge_win.numpy(), np.where(np.isin(ewin, live), ewin, -1))
        # every listed row once
        assert np.unique(didx).size == didx.size and np.unique(eidx).size == eidx.size
        edges += eidx.size
    assert edges == batch.edge_iters


def test_labels_and_feature_sources():
    ys = _chunks(5, seed=11)
    ys[1] = _with_gaps(ys[1])
    batch = build_train_batch(ys)
    trk = np.concatenate([y[:, 1] for y in ys])
    g = batch.plans[-1].graph
    lab = batch.labels.numpy()
    track = np.full(g.N, -1)
    for c, plan in enumerate(batch.plans):
        fs = batch.feat_src[c].numpy()
        assert fs.size == plan.n_new
        is_det = plan.graph.is_edge.numpy()[plan.graph.N - plan.n_new:] == 0
        assert (fs[~is_det] == batch.n_feat).all() and (fs[is_det] < batch.n_feat).all()
        track[plan.new_det_row.numpy()] = trk[fs[is_det]]
    dr, er = g.det_row.numpy(), g.edge_row.numpy()
    assert np.array_equal(lab[dr], (track[dr] >= 0).astype(np.uint8))
    ts, td = track[g.src.numpy()], track[g.dst.numpy()]
    assert np.array_equal(lab[er], ((ts == td) & (ts >= 0)).astype(np.uint8))
    X = torch.randn(batch.n_feat, 4)
    Xz = batch.stacked_features([X[batch.det_offset[i]:batch.det_offset[i + 1]][None] for i in range(len(ys))])
    assert torch.equal(Xz[:-1], X) and not Xz[-1].any()
