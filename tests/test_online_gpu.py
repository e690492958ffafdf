"""The online tracker on the device (-m gpu): the feature kernel against its host definition bit for bit, and
trackmpnn_amd.online.OnlineTracker -- fed one frame per push -- against the reference's recorded inference sequences and against
loops.infer_sequence on random sequences: the same tracks, exactly."""
import warnings

import numpy as np
import pytest
import torch

from tests.golden_util import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FR_RANGE = 30
# the time-sorted inference fixtures (the two *_unsorted ones number their detections out of arrival order: a stream cannot)
SORTED_FIXTURES = ['infer_greedy_w3_r0', 'infer_greedy_w3_r0_reinit', 'infer_greedy_w4_r2', 'infer_greedy_w5_r0_notp',
                   'infer_hungarian_w3_r1', 'infer_hungarian_w5_r0_notp', 'dense_infer_greedy_w3_r1']


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the feature kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _mantissa_f32(rng, n, scale):
    bits = (rng.integers(0, 1 << 23, size=n, dtype=np.int64) | (127 << 23)).astype(np.uint32)
    return (bits.view(np.float32) - np.float32(1.0)) * np.float32(scale)


def _raw(rng, D, ncat, vis):
    x1, y1 = _mantissa_f32(rng, D, 1100.7), _mantissa_f32(rng, D, 330.3)
    w, h = _mantissa_f32(rng, D, 141.9) + np.float32(1.0), _mantissa_f32(rng, D, 93.1) + np.float32(1.0)
    box = np.stack([x1, y1, (x1 + w).astype(np.float32), (y1 + h).astype(np.float32)], 1).astype(np.float32)
    return (rng.integers(1, ncat + 1, size=D), _mantissa_f32(rng, D, 0.999), box,
            _mantissa_f32(rng, D * 128, 0.01).reshape(D, 128) if vis else None)


def _spec(feats, ncat=8, seed=3):
    from trackmpnn_amd import FeatureSpec
    F = ncat + 5 + (2 if 'temp' in feats else 0) + (128 if 'vis' in feats else 0)
    rng = np.random.default_rng(seed)
    return FeatureSpec(ncat, feats, _mantissa_f32(rng, F, 3.3) - np.float32(1.1), _mantissa_f32(rng, F, 2.7) + np.float32(0.3),
                       fr_range=FR_RANGE)


@pytest.mark.parametrize('feats', ['2d', '2d+temp', '2d+temp+vis'])
@pytest.mark.parametrize('D', [0, 1, 63, 64, 65, 300])
def test_device_feature_rows_equal_the_host_definition_bit_for_bit(feats, D):
    """tmpnn_online_features appends D rows at a non-zero nd: they equal online_features_host's bit patterns at
    t in {0, fr_range - 1, fr_range, 1000}; y_track of the new rows is -1, their ids are nd + j; the rows in front of nd and
    behind nd + D keep their sentinel fill in all three buffers."""
    from trackmpnn_amd import _lib, online_features_host
    sp = _spec(feats)
    F, nd, cap = sp.F, 7, 7 + 300 + 5
    rng = np.random.default_rng(100 + D)
    cat, score, box, vis = _raw(rng, D, sp.ncat, sp.vis)
    raw = np.empty((D, 6), np.int32)
    raw[:, 0] = cat
    raw.view(np.float32)[:, 1], raw.view(np.float32)[:, 2:] = score, box
    words = raw.ravel() if vis is None else np.concatenate([raw.ravel(), vis.view(np.int32).ravel()])
    pk = torch.from_numpy(np.concatenate([words, np.zeros(1, np.int32)])).to(DEV)      # (never empty)
    sd = torch.from_numpy(np.concatenate([sp.mean, sp.std, sp.pair.ravel()])).to(DEV)
    V = 128 if sp.vis else 0
    for t in (0, FR_RANGE - 1, FR_RANGE, 1000):
        SENT = 0x7fc0beef                                      # (a NaN pattern: compared as integers)
        X = torch.full((cap, F), SENT, dtype=torch.int32, device=DEV)
        y_track = torch.full((cap,), 12345, dtype=torch.int32, device=DEV)
        ids = torch.full((cap,), -777, dtype=torch.int32, device=DEV)
        _lib.call('tmpnn_online_features', D, nd, cap, t % FR_RANGE, FR_RANGE, sp.ncat, int(sp.temp), V, pk.data_ptr(),
                  pk.data_ptr() + 24 * D if V else None, V, sd.data_ptr(), sd.data_ptr() + 4 * F, sd.data_ptr() + 8 * F,
                  X.data_ptr(), F, y_track.data_ptr(), ids.data_ptr(), torch.cuda.current_stream().cuda_stream)
        want = online_features_host(sp, cat, score, box, t, vis)
        Xh, yh, ih = X.cpu().numpy(), y_track.cpu().numpy(), ids.cpu().numpy()
        assert np.array_equal(Xh[nd:nd + D].view(np.uint32), want.view(np.uint32)), (feats, D, t)
        assert (Xh[:nd] == SENT).all() and (Xh[nd + D:] == SENT).all()
        assert (yh[nd:nd + D] == -1).all() and (yh[:nd] == 12345).all() and (yh[nd + D:] == 12345).all()
        assert np.array_equal(ih[nd:nd + D], np.arange(nd, nd + D)) and (ih[:nd] == -777).all() and (ih[nd + D:] == -777).all()


def test_feature_entry_point_checks_its_bounds_before_launching():
    """Rows beyond the buffer's capacity are refused on the host (nothing is launched)."""
    from trackmpnn_amd import _lib
    lib = _lib.load()
    assert lib.tmpnn_online_features(4, 7, 10, 0, 30, 3, 0, 0, None, None, 0, None, None, None, None, 8, None, None, None) == -1
    assert b'capacity' in lib.tmpnn_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------
# the tracker
# ---------------------------------------------------------------------------------------------------------------------------------
class _ReplayModel:
    """The `infer_light` fixture (dense scene) records the reference's scores per call but no parameters: a stand-in model that
    hands back call k's recorded scores for the graph it is given (the rows must number what the reference's graph held)."""
    training = False

    def __init__(self, gold, F):
        self.gold, self.k = gold, 0
        self.spec = type('S', (), {'F_total': F})

    def forward_dgraph(self, feats, h, graph):
        s = self.gold.t(f'c{self.k}/scores').float()
        assert graph.N == s.shape[0] == int(self.gold.d[f'c{self.k}/N']), (self.k, graph.N, s.shape)
        self.k += 1
        return s.to(DEV), None, torch.zeros((graph.N, 1), device=DEV), None


def _fixture(name):
    from tests.test_parity_gpu import build_model
    gold = Golden(name)
    m = gold.meta
    X, y = gold.t('X'), gold.t('y')
    model = build_model(m, gold.params()) if m['kind'] != 'infer_light' else _ReplayModel(gold, int(X.shape[2]))
    return gold, m, model, X, y


def _frames_of(y):
    """Per timestep 0 .. last non-empty one: (lo, hi) of its detections in a time-sorted y [1, ND, 2]."""
    ts = y[0, :, 0].numpy().astype(np.int64)
    assert (np.diff(ts) >= 0).all(), 'the sequence is not time-sorted'
    T = int(ts[-1]) + 1
    lo = np.searchsorted(ts, np.arange(T), side='left')
    hi = np.searchsorted(ts, np.arange(T), side='right')
    return [(int(a), int(b)) for a, b in zip(lo, hi)]


def _stream(trk, X, y, flag_last=True, every=None):
    """Push X's rows frame by frame (empty frames included), `last` on the last non-empty frame."""
    fr = _frames_of(y)
    for t, (a, b) in enumerate(fr):
        trk.push_features(X[0, a:b].contiguous(), last=flag_last and t == len(fr) - 1)
        if every is not None:
            every(t)
    return trk


def _tracker(model, m, **kw):
    from trackmpnn_amd import OnlineTracker
    return OnlineTracker(model, m['cur_win_size'], m['ret_win_size'], m['hungarian'], m.get('tp_classifier', True), device=DEV, **kw)


@pytest.mark.parametrize('name', SORTED_FIXTURES)
def test_streamed_fixture_lands_on_the_reference_tracks(name):
    """The reference's recorded sequences pushed frame by frame: tracks() == the fixture's final y_out[:, 1]."""
    gold, m, model, X, y = _fixture(name)
    trk = _stream(_tracker(model, m), X, y)
    assert np.array_equal(trk.tracks(), gold.d[f'd{gold.ncalls - 1}/y_out'][:, 1].astype(np.int64))
    assert trk.ndets == X.shape[1] and trk.frames == int(y[0, -1, 0]) + 1 == trk.finalised_upto


def test_growth_keeps_the_tracks():
    """max_dets = 8 on the 47-detection fixture: the buffers grow at least twice (device-side copies) under the native driver's
    cached addresses; same tracks."""
    gold, m, model, X, y = _fixture('infer_greedy_w4_r2')
    assert X.shape[1] == 47
    trk = _stream(_tracker(model, m, max_dets=8), X, y)
    assert trk.growths >= 2 and trk._cap >= 47
    assert np.array_equal(trk.tracks(), gold.d[f'd{gold.ncalls - 1}/y_out'][:, 1].astype(np.int64))


def _random_case(seed):
    """The recipe of test_native_driver_equals_the_composed_loop_on_random_sequences."""
    from trackmpnn_amd import TrackMPNN
    from trackmpnn_amd.graph import synth_window
    rng = np.random.default_rng(700 + seed)
    frames = int(rng.integers(12, 40))
    mean = float(rng.choice([2.0, 5.0, 9.0, 16.0]))
    yy = synth_window(900 + seed, frames, mean, int(3 * mean) + 2)
    if seed % 3 == 0:
        gap = int(rng.integers(4, frames - 4))
        width = 1 if seed % 2 else int(rng.integers(2, 8))
        yy = yy[(yy[:, 0] < gap) | (yy[:, 0] >= gap + width)]
    feats = '2d+temp+vis' if seed % 4 == 1 else '2d'
    torch.manual_seed(50 + seed)
    model = TrackMPNN(feats, 3, 64 if seed % 2 else 32, 0, 'diff' if seed % 5 else 'concat').to(DEV).eval()
    with torch.no_grad():
        for k, prm in model.named_parameters():
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(seed)).to(DEV))
    y = torch.from_numpy(yy)[None]
    X = torch.randn(1, yy.shape[0], model.spec.F_total, generator=torch.Generator().manual_seed(3000 + seed))
    win, ret = int(rng.integers(2, 7)), int(rng.integers(0, 3))
    return model, X, y, win, ret, bool(seed % 2), bool(seed % 3)


@pytest.mark.parametrize('seed', range(8))
def test_online_tracker_equals_infer_sequence_on_random_sequences(seed):
    """Frames without detections, re-initialisations, windows 2-6, retention 0-2, greedy / Hungarian, with and without the TP
    classifier, H 32 / 64, one and three feature groups: OnlineTracker's tracks == infer_sequence's, and the pushes ran through
    the native driver wherever the offline loop's timesteps did: exactly as many native timesteps as infer_sequence ran on the
    same sequence, and at least (pushes with detections) - 4 - 3 * re-initialisations.  The bound counts pushes WITH
    detections: the native step's precondition is D_t > 0 (TrackGraph.greedy_run_fast, unchanged), so a push without
    detections runs the Python composition in the offline loop and here alike -- with all pushes counted the bound cannot hold
    on the sequences whose gap is wider than one frame (seeds 0 and 6: gaps of 3 and 4 frames without a re-initialisation)."""
    from trackmpnn_amd import OnlineTracker, loops
    from trackmpnn_amd.loops import infer_sequence
    from trackmpnn_amd.tracking import TrackGraph
    model, X, y, win, ret, hung, tp = _random_case(seed)
    taken, starts = [], []
    orig_run, orig_start = TrackGraph.greedy_run_fast, TrackGraph.__dict__['start_stream']

    def counting(self, *a, **k):
        r = orig_run(self, *a, **k)
        taken.append(0 if r is None else r[3])
        return r

    TrackGraph.greedy_run_fast = counting
    try:
        y1, _, _ = infer_sequence(model, X, y, win, ret, hung, DEV, tp)
        offline_native = sum(taken)
        del taken[:]
        TrackGraph.start_stream = classmethod(lambda cls, *a, **k: (starts.append(1), orig_start.__func__(cls, *a, **k))[1])
        trk = _stream(OnlineTracker(model, win, ret, hung, tp, device=DEV, max_dets=64), X, y)
    finally:
        TrackGraph.greedy_run_fast, TrackGraph.start_stream = orig_run, orig_start
    info = (seed, win, ret, hung, tp)
    assert np.array_equal(trk.tracks(), y1[:, 1]), info
    native, pushes, reinit = sum(taken), trk.frames, len(starts) - 1
    nonempty = int(np.unique(y[0, :, 0].numpy()).size)
    print(f'seed {seed}: pushes {pushes} ({nonempty} with detections), native {native} (offline loop: {offline_native}), '
          f're-initialisations {reinit}')
    assert native == trk.native_steps
    if loops._fast_greedy(model, hung, tp, None)[0] is not None:
        assert native == offline_native, info                  # (wherever infer_sequence takes the native driver)
        assert native >= nonempty - 4 - 3 * reinit, (info, native, pushes, nonempty, reinit)
    else:
        assert native == 0


def test_raw_pushes_equal_feature_pushes():
    """push(cat, score, box) under a spec == push_features(online_features_host(...)) on the same detections: same rows on the
    device (bit for bit) and the same tracks."""
    from trackmpnn_amd import OnlineTracker, TrackMPNN, online_features_host
    from trackmpnn_amd.graph import synth_window
    ncat = 3
    sp = _spec('2d+temp', ncat=ncat, seed=9)
    yy = synth_window(77, 14, 5.0, 12)
    yy = yy[(yy[:, 0] < 6) | (yy[:, 0] >= 8)]                   # (two frames without detections)
    torch.manual_seed(21)
    model = TrackMPNN('2d+temp', ncat, 32, 0, 'diff').to(DEV).eval()
    with torch.no_grad():
        for k, prm in model.named_parameters():
            if k.startswith('output_transform') and k.endswith('bias'):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(2)).to(DEV))
    rng = np.random.default_rng(5)
    a = OnlineTracker(model, 3, 1, False, True, spec=sp, device=DEV, max_dets=16)
    b = OnlineTracker(model, 3, 1, False, True, device=DEV, max_dets=16)
    T = int(yy[-1, 0]) + 1
    for t in range(T):
        D = int((yy[:, 0] == t).sum())
        cat, score, box, _ = _raw(rng, D, ncat, False)
        a.push(cat, score, box.astype(np.float64), last=t == T - 1)
        b.push_features(online_features_host(sp, cat, score, box, t), last=t == T - 1)
    assert a.ndets == b.ndets == yy.shape[0]
    assert torch.equal(a._X[:a.ndets].view(torch.int32), b._X[:b.ndets].view(torch.int32))
    ta, tb = a.tracks(), b.tracks()
    assert np.array_equal(ta, tb) and (ta >= 0).any()


def test_steady_state_push_waits_for_the_device_once():
    """Under torch's sync debug mode a steady-state push_features of device rows shows at most one synchronisation warning (the
    Python composition's decode) -- with the native driver's polled counters that is the timestep's one read."""
    gold, m, model, X, y = _fixture('infer_greedy_w4_r2')
    trk = _tracker(model, m)
    Xd = X.to(DEV)
    fr = _frames_of(y)
    per_push, where = [], set()
    for t, (a, b) in enumerate(fr):
        rows = Xd[0, a:b]
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                trk.push_features(rows, last=t == len(fr) - 1)
            finally:
                torch.cuda.set_sync_debug_mode('default')
        sync = [x for x in w if 'synchroniz' in str(x.message).lower()]
        per_push.append(len(sync))
        where |= {f'{x.filename.rsplit("/", 1)[-1]}:{x.lineno}' for x in sync}
    print('synchronisation warnings per push:', per_push, sorted(where))
    # pushes 0 and 1 collect, push 2 is the first step (no decode in front of it: its update reads the active-set size itself)
    assert max(per_push[3:]) <= 1 and max(per_push[:2]) == 0, (per_push, sorted(where))
    assert np.array_equal(trk.tracks(), gold.d[f'd{gold.ncalls - 1}/y_out'][:, 1].astype(np.int64))


def test_prefix_property_and_close():
    """An id once >= 0 never changes; finalised_upto follows the decode horizon; close() after a flagged last push changes
    nothing; after an unflagged stream it finalises the rest, keeps the earlier ids, and further pushes raise."""
    gold, m, model, X, y = _fixture('infer_greedy_w3_r0_reinit')
    cws = m['cur_win_size']
    seen = {}

    def check(trk):
        def every(t):
            assert trk.frames == t + 1
            if not trk._closed:
                assert trk.finalised_upto == max(0, trk.frames - cws + 1)
            if t % 3 == 2:
                cur = trk.tracks()
                for i, v in seen.items():
                    assert cur[i] == v, (t, i, v, cur[i])
                seen.update({int(i): int(cur[i]) for i in np.flatnonzero(cur >= 0)})
        return every

    trk = _tracker(model, m)
    _stream(trk, X, y, every=check(trk))
    final = trk.tracks()
    assert all(final[i] == v for i, v in seen.items()) and seen
    assert np.array_equal(final, gold.d[f'd{gold.ncalls - 1}/y_out'][:, 1].astype(np.int64))
    trk.close()
    assert np.array_equal(trk.tracks(), final) and trk.finalised_upto == trk.frames
    with pytest.raises(RuntimeError, match='stream has ended'):
        trk.push_features(X[0, :1])

    seen.clear()
    trk2 = _tracker(model, m)
    _stream(trk2, X, y, flag_last=False, every=check(trk2))
    before = trk2.tracks()
    trk2.close()
    after = trk2.tracks()
    keep = before >= 0
    assert np.array_equal(after[keep], before[keep]) and (after >= 0).sum() >= keep.sum()
    assert trk2.finalised_upto == trk2.frames
    with pytest.raises(RuntimeError, match='stream has ended'):
        trk2.push_features(X[0, :1])
    trk2.close()                                                # (a second close is a no-op)
    assert np.array_equal(trk2.tracks(), after)
