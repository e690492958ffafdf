"""The device training-batch builder on the MI355X (-m gpu): build_train_batch_device against build_train_batch field by field
(every call's graph, plan, loss windows, labels and feature sources), its input forms, its limits, and train_chunks on both
batches.  Inputs: seeded synthetic chunks and the labels of the tests/golden chunk fixtures."""

import numpy as np
import pytest
import torch

from tests.conftest import chunk_golden_names
from tests.golden_util import Golden
from tests.test_train_batch_gpu import _chunks, _mixed_chunks, _perturbed_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _teq(a, b, what):
    if b is None:
        assert a is None, what
        return
    assert isinstance(a, torch.Tensor), what
    assert (a.dtype, tuple(a.shape), a.device) == (b.dtype, tuple(b.shape), b.device), (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), what


def assert_same_batch(dv, hb):
    assert len(dv.plans) == len(hb.plans) == len(dv.windows) == len(dv.feat_src)
    for c, (p, q) in enumerate(zip(dv.plans, hb.plans)):
        g, h = p.graph, q.graph
        assert (g.N, g.E, g.Dn) == (h.N, h.E, h.Dn), c
        for f in ('src', 'dst', 'edge_row', 'det_row', 'rowptr', 'inc', 'is_edge', 'pos', 'src_pos', 'dst_pos', 'det_order'):
            _teq(getattr(g, f), getattr(h, f), (c, f))
        _teq(g.__dict__.get('_det_group'), h.__dict__.get('_det_group'), (c, '_det_group'))
        assert (p.n_new, p.min_seg_cnt, p.max_seg_nd) == (q.n_new, q.min_seg_cnt, q.max_seg_nd), c
        for f in ('new_det_local', 'new_det_row', 'seg_ptr', 'seg_cnt', 'seg_of_new', 'seg_of_det'):
            _teq(getattr(p, f), getattr(q, f), (c, f))
        w, v = dv.windows[c], hb.windows[c]
        assert (w.W, w.n_det, w.n_edge) == (v.W, v.n_det, v.n_edge), c
        for f in ('det_ptr', 'det_idx', 'edge_ptr', 'edge_idx', 'det_win', 'edge_win'):
            _teq(getattr(w, f), getattr(v, f), (c, f))
        _teq(dv.feat_src[c], hb.feat_src[c], (c, 'feat_src'))
    _teq(dv.labels, hb.labels, 'labels')
    for f in ('kept', 'ncalls_b', 'edges_b', 'det_offset'):
        a, b = getattr(dv, f), getattr(hb, f)
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), f
    assert dv.skipped == hb.skipped
    assert dv.chunk_calls == []


def _check(ys, **kw):
    from trackmpnn_amd import build_train_batch, build_train_batch_device
    hb = build_train_batch(ys, DEV)
    dv = build_train_batch_device(ys, DEV, **kw)
    assert_same_batch(dv, hb)
    return dv, hb


def _transform(y, rng, reverse=0.5, drop=0.2):
    """The reference's two label transforms (dataset/kitti_mot.py:494-532): time reversal, then per-detection dropout."""
    y = y.copy()
    if rng.rand() < reverse:
        y[:, 0] = y[:, 0].max() - y[:, 0] + y[:, 0].min()
    return y[rng.rand(y.shape[0]) >= drop]


def test_mixed_chunks():
    dv, _ = _check(_mixed_chunks(70, seed=31))
    assert dv.B >= 64 and len(dv.skipped) == 1 and (dv.ncalls_b != dv.ncalls_b[0]).any()


def test_one_timestep_all_fp_and_empty_chunks_are_skipped_in_place():
    ys = _mixed_chunks(20, seed=32)
    ys[3] = np.zeros((0, 2), np.int64)
    ys[5] = np.array([[4, 1], [4, 2], [4, -1]])
    ys[9] = np.array([[0, -1], [2, -1]])
    dv, _ = _check(ys)
    assert {3, 5, 9} <= set(dv.skipped)


def test_time_reversed_and_shuffled_rows():
    rng = np.random.RandomState(33)
    ys = []
    for y in _mixed_chunks(48, seed=34):
        y = y.copy()
        if rng.rand() < 0.5:
            y[:, 0] = y[:, 0].max() - y[:, 0] + y[:, 0].min()
        ys.append(y[rng.permutation(y.shape[0])] if rng.rand() < 0.7 else y[::-1].copy())
    _check(ys)


def test_c2_set_with_dropout():
    from trackmpnn_amd import synth_window
    rng = np.random.RandomState(35)
    ys = [_transform(synth_window(1000 + s, 7, 6.0, 20), rng) for s in range(1024)]
    dv, _ = _check(ys)
    assert dv.B > 1000


@pytest.mark.parametrize('name', chunk_golden_names())
def test_reference_chunk_labels(name):
    y = Golden(name).t('y')[0].numpy()
    _check([y])
    ys = _mixed_chunks(16, seed=36)
    ys.insert(7, y)
    _check(ys)


def test_chunks_at_the_limits():
    from trackmpnn_amd.train_batch import TB_MAX_CALLS, TB_MAX_DETS
    rng = np.random.RandomState(37)
    # TB_MAX_DETS detections: 64 timesteps of 64 (tracks that skip frames, false positives)
    T = TB_MAX_DETS // 64
    y = np.stack([np.repeat(np.arange(T), 64), rng.randint(-1, 80, T * 64)], 1)
    dv, _ = _check([y[rng.permutation(y.shape[0])]])
    assert dv.det_offset[-1] == TB_MAX_DETS
    # TB_MAX_CALLS calls: a few dets every 16th timestep, t1 = 1
    ts = np.concatenate([[0, 0, 1], np.arange(16, TB_MAX_CALLS + 1, 16).repeat(2)])
    y = np.stack([ts, rng.randint(-1, 3, ts.size)], 1)
    y[0, 1] = 1
    dv, _ = _check([y, np.array([[0, 1], [1, 1]])])
    assert dv.ncalls_b[0] == TB_MAX_CALLS


def test_beyond_the_limits_and_all_skipped_raise():
    from trackmpnn_amd import build_train_batch_device
    from trackmpnn_amd.train_batch import TB_MAX_CALLS, TB_MAX_DETS
    ok = np.array([[0, 1], [1, 1]])
    many = np.stack([np.arange(TB_MAX_DETS + 1) % 2, np.arange(TB_MAX_DETS + 1)], 1)
    with pytest.raises(ValueError, match='build_train_batch'):
        build_train_batch_device([ok, many], DEV)
    long = np.array([[0, 1], [1, 1], [TB_MAX_CALLS + 1, 1]])
    with pytest.raises(ValueError, match='calls.*build_train_batch'):
        build_train_batch_device([long, ok], DEV)
    build_train_batch_device([np.array([[0, 1], [1, 1], [TB_MAX_CALLS, 1]])], DEV)       # (just at the limit)
    with pytest.raises(ValueError, match='every chunk is skipped'):
        build_train_batch_device([np.array([[0, 1]]), np.array([[0, -1], [1, -1]])], DEV)


@pytest.mark.parametrize('bad, match', [(np.array([[0, 1], [1.5, 1]]), 'not an integer'),
                                         (np.array([[0, 1], [1, np.nan]]), 'not an integer'),
                                         (np.array([[-1, 1], [1, 1]]), 'negative'),
                                         (np.array([[0, 1], [1, 2 ** 31]]), 'int32'),
                                         (np.array([[0, 1], [2 ** 31, 1]]), 'int32')])
def test_malformed_values_raise(bad, match):
    from trackmpnn_amd import build_train_batch_device
    with pytest.raises(ValueError, match=match):
        build_train_batch_device([np.array([[0, 1], [1, 1]]), bad], DEV)


def test_input_forms_agree():
    from trackmpnn_amd import build_train_batch, build_train_batch_device
    ys = _mixed_chunks(40, seed=38)
    hb = build_train_batch(ys, DEV)
    assert_same_batch(build_train_batch_device(ys, DEV), hb)
    assert_same_batch(build_train_batch_device([torch.from_numpy(y).float()[None].to(DEV) for y in ys], DEV), hb)
    off = np.concatenate([[0], np.cumsum([y.shape[0] for y in ys])])
    stacked = torch.from_numpy(np.concatenate(ys)).to(DEV)
    assert_same_batch(build_train_batch_device(stacked, DEV, offsets=torch.from_numpy(off).to(DEV)), hb)
    assert_same_batch(build_train_batch_device(stacked.double()[None], DEV, offsets=off), hb)


def _train(batch, Xs, tp, seed=9):
    from trackmpnn_amd.loops import train_chunks
    model = _perturbed_model(seed=seed)
    model.zero_grad(set_to_none=True)
    loss, per_chunk, nc, ne = train_chunks(model, batch, Xs, tp)
    return (loss.detach(), per_chunk, nc, ne, {k: p.grad.detach().clone() for k, p in model.named_parameters()},
            {k: b.detach().clone() for k, b in model.named_buffers()})


def _assert_same_training(r, s):
    _teq(r[0], s[0], 'loss')
    _teq(r[1], s[1], 'per_chunk')
    assert r[2:4] == s[2:4]
    for k in s[4]:
        _teq(r[4][k], s[4][k], k)
    for k in s[5]:
        _teq(r[5][k], s[5][k], k)


@pytest.mark.parametrize('tp', [True, False])
def test_train_chunks_on_both_batches(tp):
    from trackmpnn_amd import build_train_batch, build_train_batch_device
    ys = _mixed_chunks(64, seed=39)
    gen = torch.Generator().manual_seed(40)
    Xs = torch.randn(sum(y.shape[0] for y in ys), 8, generator=gen).to(DEV)
    _assert_same_training(_train(build_train_batch_device(ys, DEV), Xs, tp), _train(build_train_batch(ys, DEV), Xs, tp))


def test_fresh_batches_back_to_back():
    from trackmpnn_amd import build_train_batch, build_train_batch_device
    rng = np.random.RandomState(41)
    base = _chunks(48, seed=42)
    sets = [[_transform(y, rng) for y in base] for _ in range(2)]
    gen = torch.Generator().manual_seed(43)
    feats = [torch.randn(sum(y.shape[0] for y in ys), 8, generator=gen).to(DEV) for ys in sets]
    ref = [_train(build_train_batch(ys, DEV), X, True) for ys, X in zip(sets, feats)]
    for k in (0, 1, 0):
        dv = build_train_batch_device(sets[k], DEV)
        assert_same_batch(dv, build_train_batch(sets[k], DEV))
        _assert_same_training(_train(dv, feats[k], True), ref[k])


def test_a_build_waits_for_the_device_twice():
    """Two host reads (the per-chunk counts, the per-call totals) are the only synchronisations of a build, from host arrays
    and from a stacked device tensor with host offsets."""
    import warnings
    from trackmpnn_amd import build_train_batch_device
    ys = _mixed_chunks(40, seed=44)
    off = np.concatenate([[0], np.cumsum([y.shape[0] for y in ys])])
    stacked = torch.from_numpy(np.concatenate(ys)).to(DEV)
    forms = [lambda: build_train_batch_device(ys, DEV), lambda: build_train_batch_device(stacked, DEV, offsets=off)]
    for build in forms:
        build()                                               # (warm: caching allocators, code objects)
    torch.cuda.synchronize()
    for build in forms:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                build()
            finally:
                torch.cuda.set_sync_debug_mode('default')
        syncs = [str(w.message) for w in rec if 'called a synchronizing' in str(w.message)]
        assert len(syncs) == 2, syncs


def test_undersized_lds_sizes_are_reported_not_overrun():
    """The C ABI's per-chunk kernels check a chunk against the descriptor's LDS sizes on the device."""
    import ctypes
    from trackmpnn_amd import _lib
    y = torch.tensor([[0, 1], [0, 2], [1, 1], [1, 2], [2, 1]], dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 5], dtype=torch.int64, device=DEV)
    info = torch.zeros(4, dtype=torch.int64, device=DEV)
    d = _lib.CTrainBuild()
    d.n, d.n_feat, d.y, d.offsets, d.info = 1, 5, y.data_ptr(), off.data_ptr(), info.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    _lib.call('tmpnn_train_build_count', ctypes.byref(d), st)
    assert info.tolist() == [0, 2, 0, 1]                      # valid, 2 calls, t0 = 0, t1 = 1
    kc = torch.tensor([0, 0, 2], dtype=torch.int32, device=DEV)                   # kept = [0], cptr = [0, 2]
    counts = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
    d.B, d.C, d.kept, d.cptr, d.counts = 1, 2, kc.data_ptr(), kc[1:].data_ptr(), counts.data_ptr()
    for max_dets, max_slots in ((4, 4), (8, 3)):              # 5 dets need 8; 2 calls need 4 slots
        d.max_dets, d.max_slots = max_dets, max_slots
        _lib.call('tmpnn_train_build_calls', ctypes.byref(d), st)
        assert int(info[0]) == 64 and (counts == -7).all()   # TMPNN_TB_ST_LDS, nothing written
        info[0] = 0
    d.max_dets, d.max_slots = 8, 4
    _lib.call('tmpnn_train_build_calls', ctypes.byref(d), st)
    assert int(info[0]) == 0 and counts.tolist() == [[4, 4], [2, 1]]
