"""The validation F1 on the MI355X (-m gpu): the one-launch kernel (tmpnn_val_f1_count, ValMonitor.count) against the host
definition val_counts_host on graphs at the sizes where a one-workgroup kernel with 64-wide ballots and an LDS bitmap can go
wrong, and both inference paths of infer_sequence / validate with a monitor against what the REAL reference recorded per forward
call (tests/golden/val_f1, tests/test_val_f1.py pins the host definition to the same files).  Counts are compared exactly; the
mean F1 within n^2 2^-52 for n forwards (a bound on any fp64 summation order of n terms in [0, 1])."""
import numpy as np
import pytest
import torch

from tests.test_val_f1 import load, mean_bound, val_fixture_names
from trackmpnn_amd.monitor import val_counts_host, val_f1_host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


# ---- the kernel against the host definition ----------------------------------------------------------------------------------
# (n0, n1): dets of two timesteps with all-pairs edges, N = n0 + n0 n1 + n1 rows.  N = 1, 2, 3; 63 / 64 / 65 (one ballot);
# 1023 / 1024 / 1025 (one row per thread); 4095 / 4096 / 4097 and E = 4096 / 4100 (one unrolled trip of the workgroup);
# 16640 (the bitmap's upper half) and 32767 (its last bit, the tracker's row limit)
BLOCKS = [(1, 0), (2, 0), (1, 1), (7, 7), (4, 12), (5, 10), (31, 31), (24, 40), (26, 37), (63, 63), (16, 240), (1, 2048), (64, 64),
          (5, 820), (128, 128), (127, 255)]


class _Blocks:
    """One TrackGraph whose rows are refilled per case (the row form tmpnn_graph_from_rows_ws converts, and the label rows the
    monitor reads), with the host copy of every case: built once, shared by the tests below, never modified."""

    def __init__(self):
        from trackmpnn_amd.tracking import TrackGraph
        self.tg = TrackGraph(DEV)
        self.host = {}
        for k, (n0, n1) in enumerate(BLOCKS):
            rng = np.random.default_rng(100 + k)
            N, (ts, did, is_edge, src, dst, _) = TrackGraph._first_block(0, np.arange(n0), 1, n0 + np.arange(n1), np.full(n0, -1),
                                                                         np.full(n1, -1))
            # labels at random, NOT track-consistent: most dets have many label-positive edges on either side
            lab = (rng.random(N) < 0.5).astype(np.uint8)
            s = rng.random(N).astype(np.float32)
            s[rng.random(N) < 0.1] = 0.5                               # the tie: predicts 0
            self.host[(n0, n1)] = dict(N=N, E=n0 * n1, Dn=n0 + n1, is_edge=is_edge.astype(np.uint8), src=src, dst=dst, labels=lab,
                                       scores=s)

    def load(self, key):
        """The case's rows into the TrackGraph (index form re-derived on the device); returns (tg, scores on the device)."""
        q, tg = self.host[key], self.tg
        r = tg.rows
        N = q['N']
        r['is_edge'][:N].copy_(torch.from_numpy(q['is_edge']))
        r['src'][:N].copy_(torch.from_numpy(q['src']))
        r['dst'][:N].copy_(torch.from_numpy(q['dst']))
        r['labels'][:N].copy_(torch.from_numpy(q['labels']))
        tg.N, tg.E, tg.Dn = N, q['E'], q['Dn']
        tg._graph = None
        return tg, torch.from_numpy(q['scores']).to(DEV)

    def counts(self, key, tp):
        q = self.host[key]
        return val_counts_host(q['is_edge'], q['src'], q['dst'], q['labels'], q['scores'], tp)


@pytest.fixture(scope='module')
def blocks():
    return _Blocks()


@pytest.mark.parametrize('tp', [True, False])
@pytest.mark.parametrize('key', BLOCKS)
def test_kernel_equals_the_host_definition(blocks, key, tp):
    from trackmpnn_amd import ValMonitor
    vm = ValMonitor(DEV, log_forwards=2)
    tg, s = blocks.load(key)
    assert tg.graph.arena[:3].tolist() == [tg.E, tg.Dn, 0]               # E, Dn, status where the kernel reads them
    vm.count(tg, s[:, None], tp)                                          # scores [N, 1] as the model returns them
    want = blocks.counts(key, tp)
    assert want[3] == key[0] + key[0] * key[1] + key[1]
    r, ref = vm.read(), val_f1_host([want])
    print(key, tp, 'device', r, 'host', want)
    assert (r['tp'], r['fp'], r['fn'], r['rows'], r['forwards']) == (*want, 1)
    assert vm.log().tolist() == [list(want)]
    assert r['f1'] == ref['f1']                                           # one forward: the fp64 quotient itself
    if key[0] * key[1] > 4 and tp:
        assert want[0] > 0 and want[1] > 0 and want[2] > 0               # (the case does exercise all three counts)


def test_record_accumulates_and_the_log_saturates(blocks):
    from trackmpnn_amd import ValMonitor
    vm = ValMonitor(DEV, log_forwards=2)
    keys = [(7, 7), (24, 40), (1, 0), (63, 63)]
    wants = []
    for i, key in enumerate(keys):
        tg, s = blocks.load(key)
        vm.count(tg, s, i % 2 == 0)
        wants.append(blocks.counts(key, i % 2 == 0))
    r, ref = vm.read(), val_f1_host(wants)
    assert r['forwards'] == 4 and (r['tp'], r['fp'], r['fn'], r['rows']) == (ref['tp'], ref['fp'], ref['fn'], ref['rows'])
    assert abs(r['f1'] - ref['f1']) <= mean_bound(4)
    # log index = min(forwards before, log_cap - 1): the first forward, then the last one over the others
    assert vm.log().tolist() == [list(wants[0]), list(wants[3])]
    vm.reset()
    r = vm.read()
    assert r['forwards'] == 0 and np.isnan(r['f1']) and vm.log().shape == (0, 4)
    # without a log
    vm2 = ValMonitor(DEV)
    tg, s = blocks.load((4, 12))
    vm2.count(tg, s, True)
    vm2.count(tg, s, True)
    r2 = vm2.read()
    one = blocks.counts((4, 12), True)
    assert r2['forwards'] == 2 and (r2['tp'], r2['rows']) == (2 * one[0], 2 * one[3])
    assert abs(r2['f1'] - val_f1_host([one])['f1']) <= mean_bound(2)
    with pytest.raises(RuntimeError):
        vm2.log()
    with pytest.raises(ValueError):
        vm2.count(tg, s[:-1], True)


def test_invalid_graph_and_no_rows_are_no_forward(blocks):
    from trackmpnn_amd import ValMonitor
    vm = ValMonitor(DEV, log_forwards=2)
    tg, s = blocks.load((5, 10))
    g = tg.graph
    g.arena[2] = 1                                                        # meta[2]: the status word, on the device
    vm.count(tg, s, True)
    assert vm.read()['forwards'] == 0 and vm.read()['rows'] == 0
    g.arena[2] = 0
    vm.count(tg, s, True)
    assert vm.read()['forwards'] == 1
    # sizes that are not those of a graph of N rows (E + Dn > N) are presented as empty too
    g.arena[0] = tg.N
    vm.count(tg, s, True)
    assert vm.read()['forwards'] == 1
    tg.N = 0
    vm.count(tg, s[:0], True)
    assert vm.read()['forwards'] == 1


# ---- both inference paths on the reference's fixtures ------------------------------------------------------------------------
def _fixture_model(d, m):
    from tests.test_parity_gpu import build_model
    params = {k[len('param/'):]: torch.from_numpy(d[k].copy()) for k in d.files if k.startswith('param/')}
    return build_model(m, params)


def _run(model, d, m, stages, vm):
    """infer_sequence with a monitor; returns (y_out, ncalls, timesteps the native driver ran)."""
    from trackmpnn_amd import loops
    from trackmpnn_amd.tracking import TrackGraph
    X, y = torch.from_numpy(d['X'].copy()), torch.from_numpy(d['y'].copy())
    taken = []
    orig = TrackGraph.greedy_run_fast

    def counting(self, *a, **k):
        r = orig(self, *a, **k)
        taken.append(0 if r is None else r[3])
        return r

    TrackGraph.greedy_run_fast = counting
    try:
        y_out, ncalls, _ = loops.infer_sequence(model, X, y, m['cur_win_size'], m['ret_win_size'], m['hungarian'], DEV,
                                                m['tp_classifier'], stages=stages, monitor=vm)
    finally:
        TrackGraph.greedy_run_fast = orig
    return y_out, ncalls, sum(taken)


@pytest.mark.parametrize('name', val_fixture_names())
def test_both_inference_paths_count_what_the_reference_counted(name):
    from trackmpnn_amd import ValMonitor
    d, m = load(name)
    model = _fixture_model(d, m)
    n = m['ncalls']
    want = [[int(v) for v in d[f'f{c}/counts']] for c in range(n)]
    results = []
    for stages in (None, {}):                                             # the native driver; the composed Python path
        vm = ValMonitor(DEV, log_forwards=n + 4)
        y_out, ncalls, native = _run(model, d, m, stages, vm)
        r, log = vm.read(), vm.log().tolist()
        print(name, 'native' if stages is None else 'python', 'native steps', native, r, log)
        assert np.array_equal(y_out, d['y_out']) and ncalls == n          # the reference's tracks, as without a monitor
        assert (native > 0) == (stages is None)                           # the first run did go through the native driver
        assert log == want                                                # every forward's counts, exactly
        assert r['forwards'] == n
        assert abs(r['f1'] - float(d['mean_f1'])) <= mean_bound(n)
        results.append((r, log, y_out))
    assert results[0][0]['forwards'] == results[1][0]['forwards'] and results[0][1] == results[1][1]
    assert abs(results[0][0]['f1'] - results[1][0]['f1']) <= mean_bound(n)
    # and without a monitor nothing changes
    y0, n0, _ = _run(model, d, m, None, None)
    assert np.array_equal(y0, results[0][2]) and n0 == n


def _mot_sequence(d):
    """The fixture's sequence as validate takes it: a box per detection (apart per track, drifting per frame), the ground
    truth = the detections that have a track."""
    y = d['y'][0].astype(np.int64)
    fr, tr = y[:, 0], y[:, 1]
    x0 = np.where(tr >= 0, 200.0 * tr, 2000.0 + 150.0 * np.arange(y.shape[0])) + 3.0 * fr
    box = np.stack([x0, 10.0 + fr, x0 + 100.0, 110.0 + fr], 1).astype(np.float32)
    has = tr >= 0
    return dict(det_frame=fr, det_box=box, tracks=tr, gt_frame=fr[has], gt_track=tr[has], gt_box=box[has],
                X=torch.from_numpy(d['X'].copy()), y=torch.from_numpy(d['y'].copy()))


@pytest.mark.parametrize('name,other', [('greedy_w3_r0', 'greedy_w5_r0_shuffled_hole'), ('hungarian_w3_r0_notp_reinit', 'hungarian_w5_r2')])
def test_validate_returns_the_mean_over_every_forward(name, other):
    from trackmpnn_amd import MotEvaluator, ValMonitor, validate
    d, m = load(name)
    d2, _ = load(other)
    model = _fixture_model(d, m)
    a, b = _mot_sequence(d), _mot_sequence(d2)
    # a sequence without ground truth is skipped (train.py:190-192): no inference, no forward
    no_gt = dict(b, gt_frame=np.zeros(0, np.int64), gt_track=np.zeros(0, np.int64), gt_box=np.zeros((0, 4), np.float32))
    seqs = [a, no_gt, b]
    kw = dict(cur_win_size=m['cur_win_size'], ret_win_size=m['ret_win_size'], use_hungarian=m['hungarian'],
              tp_classifier=m['tp_classifier'])
    ev = MotEvaluator(seqs, DEV)
    plain = validate(model, seqs, ev, **kw)
    assert 'f1' not in plain and 'f1_forwards' not in plain
    vm = ValMonitor(DEV, log_forwards=64)
    out = validate(model, seqs, ev, monitor=vm, **kw)
    assert repr({k: v for k, v in out.items() if k not in ('f1', 'f1_forwards')}) == repr(plain)
    # each sequence on its own (the composed path, a monitor of its own)
    per = []
    for q, dd in ((a, d), (b, d2)):
        v1 = ValMonitor(DEV, log_forwards=64)
        _run(model, dd, m, {}, v1)
        per.append((v1.read(), v1.log().tolist()))
    (ra, la), (rb, lb) = per
    na, nb = ra['forwards'], rb['forwards']
    assert na == m['ncalls'] and nb > 0
    assert out['f1_forwards'] == na + nb                                  # the skipped sequence contributes none
    assert vm.log().tolist() == la + lb
    assert abs(out['f1'] - (na * ra['f1'] + nb * rb['f1']) / (na + nb)) <= mean_bound(na + nb)
    assert abs(out['f1'] - val_f1_host(la + lb)['f1']) <= mean_bound(na + nb)
    # the first sequence ran in its own fixture's settings: its forwards are the reference's
    assert la == [[int(v) for v in d[f'f{c}/counts']] for c in range(na)]
    # a second pass resets the monitor first
    out2 = validate(model, seqs, ev, monitor=vm, **kw)
    assert (out2['f1'], out2['f1_forwards']) == (out['f1'], out['f1_forwards'])
