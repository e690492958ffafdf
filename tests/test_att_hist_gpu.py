"""The attention histograms on the MI355X (-m gpu): the one-launch kernel (tmpnn_att_hist_count, AttentionMonitor.count) against
the host definition att_hist_host, bit for bit, on synthetic graphs at the sizes where a one-workgroup kernel with an unrolled
strided loop and an LDS histogram can go wrong, and infer_sequence / validate with an AttentionMonitor against what the REAL
reference's head study selected (tests/golden/att_hist; tests/test_att_hist.py pins the host definition to the same files).

Every count is compared exactly.  On the synthetic graphs the device reads the very float32 values the host bins, and both bin
against the same float32 edge table.  On the fixtures the device's alphas differ from the reference's by rounding, and exactness
is legitimate because every informative alpha of the set lies at least MARGIN (ten times the tolerance the device's attention
values are held to) from every bin edge -- tests/test_att_hist.py checks that on the committed files."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_att_hist import att_fixture_names, load, two_frames
from trackmpnn_amd.monitor import ATT_HIST_KMAX, att_csr_host, att_hist_edges, att_hist_host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


# ---- the kernel against the host definition ----------------------------------------------------------------------------------
# (n0, n1, isolated dets): two timesteps with all-pairs edges, E = n0 n1.  A graph's 2E is even, so the sizes around a wave (64),
# the workgroup (1024) and one unrolled trip of it (4096 positions) are taken both as E and, where even, as 2E:
#   E = 1, 63, 65, 1023, 1025                    (2E = 2, 126, 130, 2046, 2050)
#   2E = 62, 64, 66, 1022, 1024, 1026, 4096      (E = 31, 32, 33, 511, 512, 513, 2048)
#   2E = 4100: the loop runs twice, the second trip with a ragged tail of 4 positions; 2E = 9000: three trips
# (1, 100): a det with more than 64 incident edges; (1, 31), (1, 2050): one det owns half of the positions.
SHAPES = [(1, 1, 0), (7, 9, 2), (5, 13, 0), (31, 33, 3), (25, 41, 0), (1, 31, 1), (4, 8, 0), (3, 11, 5), (7, 73, 0), (16, 32, 1),
          (19, 27, 0), (32, 64, 2), (41, 50, 0), (1, 2050, 3), (1, 100, 1), (45, 100, 7), (3, 0, 0)]


class _Shapes:
    """One TrackGraph whose rows are refilled per case (the row form tmpnn_graph_from_rows_ws converts, and the label rows the
    monitor reads), with the host copy of every case: built once, shared by the tests below, never modified."""
    KMAX = ATT_HIST_KMAX + 1

    def __init__(self):
        from trackmpnn_amd.tracking import TrackGraph
        self.tg = TrackGraph(DEV)
        self.host = {}
        for i, (n0, n1, iso) in enumerate(SHAPES):
            rng = np.random.default_rng(300 + i)
            is_edge, src, dst = two_frames(n0, n1, iso)
            N, E = is_edge.size, n0 * n1
            lab = rng.integers(0, 3, N).astype(np.uint8)                 # labels 0, 1, 2: only 1 is a correct association
            a = rng.random((self.KMAX, 2 * E)).astype(np.float32)
            edges = att_hist_edges(64)
            r = rng.random(a.shape)
            a[r < 0.05] = 0.0                                             # underflowed: skipped, counted in `zeros`
            on25 = rng.choice(att_hist_edges(25), a.shape)                # exactly on an edge of either table, 0.0 and 1.0 included
            on64 = rng.choice(edges, a.shape)
            a = np.where((r >= 0.05) & (r < 0.15), on25, a)
            a = np.where((r >= 0.15) & (r < 0.25), on64, a)
            a = np.where((r >= 0.25) & (r < 0.27), np.float32(1.5), a)    # above the range: dropped
            a = np.where((r >= 0.27) & (r < 0.30), np.nextafter(on25, np.float32(0)), a)      # one ulp below an edge
            self.host[(n0, n1, iso)] = dict(N=N, E=E, Dn=n0 + n1 + iso, is_edge=is_edge, src=src, dst=dst, labels=lab,
                                            alpha=np.ascontiguousarray(a.astype(np.float32)))

    def load(self, key):
        q, tg = self.host[key], self.tg
        r = tg.rows
        N = q['N']
        r['is_edge'][:N].copy_(torch.from_numpy(q['is_edge']))
        r['src'][:N].copy_(torch.from_numpy(q['src']))
        r['dst'][:N].copy_(torch.from_numpy(q['dst']))
        r['labels'][:N].copy_(torch.from_numpy(q['labels']))
        tg.N, tg.E, tg.Dn = N, q['E'], q['Dn']
        tg._graph = None
        return tg

    def attention(self, key, K, one_buffer=True):
        """forward's fourth output for the case: one feature group of K heads, slices of one [K, max(2E, 1)] buffer (as the
        attention stage returns them) or K tensors of their own."""
        a = self.host[key]['alpha'][:K]
        P = a.shape[1]
        if one_buffer:
            buf = torch.full((K, max(P, 1)), float('nan'), device=DEV)
            buf[:, :P] = torch.from_numpy(a)
            return ([SimpleNamespace(alpha=buf[k, :P]) for k in range(K)],)
        return ([SimpleNamespace(alpha=torch.from_numpy(a[k].copy()).to(DEV)) for k in range(K)],)

    def want(self, key, K, bins):
        q = self.host[key]
        return att_hist_host(q['is_edge'], q['labels'], q['alpha'][:K], q['N'], bins, src=q['src'], dst=q['dst'])


@pytest.fixture(scope='module')
def shapes():
    return _Shapes()


def _same(r, want, forwards=1):
    assert np.array_equal(r['counts'], want['counts']), np.argwhere(r['counts'] != want['counts'])[:8]
    assert (r['forwards'], r['dets'], r['isolated'], r['zeros']) == (forwards, forwards * want['dets'], forwards * want['isolated'],
                                                                     forwards * want['zeros'])
    assert np.array_equal(r['edges'], want['edges'])


@pytest.mark.parametrize('bins', [25, 64])
@pytest.mark.parametrize('key', SHAPES)
def test_kernel_equals_the_host_definition(shapes, key, bins):
    from trackmpnn_amd import AttentionMonitor
    K = 3
    am = AttentionMonitor(DEV, K, bins=bins)
    tg = shapes.load(key)
    assert tg.graph.arena[:3].tolist() == [tg.E, tg.Dn, 0]               # E, Dn, status where the kernel reads them
    # the CSR order the alphas are in is the device graph's
    dets, rowptr, inc = att_csr_host(shapes.host[key]['is_edge'], shapes.host[key]['src'], shapes.host[key]['dst'])
    fg = tg.graph.frame_graph()
    assert fg.rowptr.cpu().tolist() == rowptr.tolist()
    assert (fg.inc.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist() == inc.tolist()
    am.count(tg, shapes.attention(key, K))
    r, want = am.read(), shapes.want(key, K, bins)
    print(key, bins, 'values', int(want['counts'].sum()), 'isolated', want['isolated'], 'zeros', want['zeros'])
    _same(r, want)
    if key[0] * key[1] >= 63:
        assert want['zeros'] > 0 and (want['counts'].sum(-1) > 0).all()  # (the case does exercise both lists and the skip)
    if key[2] and key[0] * key[1]:
        assert want['isolated'] == key[2]


@pytest.mark.parametrize('K', [1, ATT_HIST_KMAX, ATT_HIST_KMAX + 1])
@pytest.mark.parametrize('one_buffer', [True, False])
def test_head_groups(shapes, K, one_buffer):
    """K = 1, one full launch of 8 heads, and 9 heads = two launches of which only the first counts the forward; the heads as
    slices of one buffer and as tensors of their own (stacked by the monitor)."""
    from trackmpnn_amd import AttentionMonitor
    key = (7, 9, 2)
    am = AttentionMonitor(DEV, K)
    tg = shapes.load(key)
    am.count(tg, shapes.attention(key, K, one_buffer))
    want = shapes.want(key, K, 25)
    _same(am.read(), want)
    assert len({want['counts'][k].tobytes() for k in range(K)}) == K     # the heads' histograms differ: none can stand in for another
    # a second forward accumulates, reset() clears
    am.count(tg, shapes.attention(key, K, one_buffer))
    r = am.read()
    assert np.array_equal(r['counts'], 2 * want['counts'])
    assert (r['forwards'], r['dets'], r['isolated'], r['zeros']) == (2, 2 * want['dets'], 2 * want['isolated'], 2 * want['zeros'])
    n = am.normalized(r)
    assert n.shape == (K, 2, 25) and np.allclose(n.sum(-1), 1.0) and np.array_equal(n, am.normalized())
    am.reset()
    r = am.read()
    assert r['forwards'] == 0 and int(r['counts'].sum()) == 0 and np.isnan(am.normalized(r)).all()


def test_invalid_and_empty_graphs_leave_the_record_untouched(shapes):
    from trackmpnn_amd import AttentionMonitor
    key = (5, 13, 0)
    am = AttentionMonitor(DEV, 3)
    tg = shapes.load(key)
    g = tg.graph
    att = shapes.attention(key, 3)
    g.arena[2] = 1                                                        # meta[2]: the status word, on the device
    am.count(tg, att)
    assert not am.record.any().item()
    g.arena[2] = 0
    g.arena[0] = tg.N                                                     # sizes that are not those of a graph of N rows
    am.count(tg, att)
    assert not am.record.any().item()
    g.arena[0] = tg.E
    am.count(tg, att)
    _same(am.read(), shapes.want(key, 3, 25))
    before = am.record.clone()
    tg.N = 0                                                              # no rows: nothing is launched
    am.count(tg, att)
    assert torch.equal(am.record, before)
    # a graph without edges is a forward without values
    tg = shapes.load((3, 0, 0))
    am.reset()
    am.count(tg, shapes.attention((3, 0, 0), 3))
    r = am.read()
    assert (r['forwards'], r['dets'], r['isolated']) == (1, 3, 3) and int(r['counts'].sum()) == 0


def test_hand_made_edge_exact_values(shapes):
    """The CPU test's edge cases on the device: 1.0 in the closed last bin, 0.2f on edge 5, 1 / 25 on edge 1, label 2 as fp,
    alpha 0 skipped."""
    from trackmpnn_amd import AttentionMonitor
    from trackmpnn_amd.tracking import TrackGraph
    tg = TrackGraph(DEV)

    def run(n0, n1, iso, lab, alpha):
        is_edge, src, dst = two_frames(n0, n1, iso)
        N = is_edge.size
        for k, v in (('is_edge', is_edge), ('src', src), ('dst', dst), ('labels', np.asarray(lab, np.uint8))):
            tg.rows[k][:N].copy_(torch.from_numpy(v))
        tg.N, tg.E, tg.Dn, tg._graph = N, n0 * n1, n0 + n1 + iso, None
        a = np.asarray(alpha, np.float32)
        am = AttentionMonitor(DEV, a.shape[0])
        am.count(tg, ([SimpleNamespace(alpha=torch.from_numpy(a[k].copy()).to(DEV)) for k in range(a.shape[0])],))
        r = am.read()
        _same(r, att_hist_host(is_edge, lab, a, N, 25, src=src, dst=dst))
        return r['counts']

    c = run(1, 1, 0, [1, 1, 1], np.ones((1, 2)))
    assert c[0, 0, 24] == 2 and c.sum() == 2
    fifth = np.float32(1) / np.float32(5)
    lab = np.zeros(11, np.uint8)
    lab[[1, 3]] = 1
    c = run(1, 5, 0, lab, np.concatenate([np.full(5, fifth, np.float32), np.ones(5, np.float32)])[None])
    assert c[0, 0, 5] == 2 and c[0, 1, 5] == 3 and c[0, :, 4].sum() == 0
    lab = np.zeros(25, np.uint8)
    lab[[3, 8, 13]] = 1
    c = run(3, 4, 6, lab, np.full((2, 24), 0.5))
    assert c[1, 0, 1] == 18 and c[1, 1, 1] == 54 and c[1, :, 0].sum() == 0
    a = np.full((1, 8), 0.5, np.float32)
    a[0, 0] = 0.0
    c = run(2, 2, 0, [1, 1, 1, 2, 0, 1, 1, 1], a)
    assert c[0, 0, 12] == 3 and c[0, 1, 12] == 4


# ---- infer_sequence / validate on the reference's fixtures -------------------------------------------------------------------
def _fixture_model(d, m):
    from tests.test_parity_gpu import build_model
    params = {k[len('param/'):]: torch.from_numpy(d[k].copy()) for k in d.files if k.startswith('param/')}
    return build_model(m, params)


def _infer(model, d, m, am):
    from trackmpnn_amd import loops
    X, y = torch.from_numpy(d['X'].copy()), torch.from_numpy(d['y'].copy())
    return loops.infer_sequence(model, X, y, m['cur_win_size'], m['ret_win_size'], m['hungarian'], DEV, m['tp_classifier'],
                                att_monitor=am)


@pytest.fixture(scope='module')
def runs():
    """Every fixture through infer_sequence once with a monitor and once without: shared by the tests below."""
    from trackmpnn_amd import AttentionMonitor
    out = {}
    for name in att_fixture_names():
        d, m = load(name)
        model = _fixture_model(d, m)
        am = AttentionMonitor(DEV, m['nattheads'], bins=m['bins'])
        out[name] = dict(d=d, m=m, model=model, am=am, with_=_infer(model, d, m, am), read=am.read(),
                         without=_infer(model, d, m, None))
    return out


@pytest.mark.parametrize('name', att_fixture_names())
def test_infer_sequence_counts_what_the_reference_selected(runs, name):
    q = runs[name]
    d, m, r = q['d'], q['m'], q['read']
    y_out, ncalls, _ = q['with_']
    print(name, 'forwards', r['forwards'], 'values', int(r['counts'].sum()), 'isolated', r['isolated'], 'zeros', r['zeros'])
    assert np.array_equal(y_out, d['y_out'])                              # the reference's tracks
    assert r['forwards'] == m['forwards'] == int(d['forwards'])
    assert ncalls == m['forwards'] + 1                                    # the first call of the sequence is not counted
    assert np.array_equal(r['counts'], d['hist']), np.argwhere(r['counts'] != d['hist'])[:8]
    assert r['zeros'] == 0


@pytest.mark.parametrize('name', att_fixture_names())
def test_the_monitor_changes_nothing_else(runs, name):
    (y1, n1, e1), (y0, n0, e0) = runs[name]['with_'], runs[name]['without']
    assert np.array_equal(y1, y0) and (n1, e1) == (n0, e0)


def test_two_sequences_accumulate_and_reset_clears(runs):
    from trackmpnn_amd import AttentionMonitor
    a, b = [n for n in att_fixture_names() if runs[n]['m']['nattheads'] == 2][:2]
    am = AttentionMonitor(DEV, 2)
    for n in (a, b):
        _infer(runs[n]['model'], runs[n]['d'], runs[n]['m'], am)
    r = am.read()
    assert np.array_equal(r['counts'], runs[a]['d']['hist'] + runs[b]['d']['hist'])
    assert r['forwards'] == runs[a]['m']['forwards'] + runs[b]['m']['forwards']
    assert r['dets'] == runs[a]['read']['dets'] + runs[b]['read']['dets']
    am.reset()
    assert not am.record.any().item()


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


def test_validate_returns_the_sequences_summed(runs):
    from trackmpnn_amd import AttentionMonitor, MotEvaluator, validate
    a, b = [n for n in att_fixture_names() if runs[n]['m']['nattheads'] == 2][:2]
    m = runs[a]['m']
    model = runs[a]['model']
    sa, sb = _mot_sequence(runs[a]['d']), _mot_sequence(runs[b]['d'])
    no_gt = dict(sb, gt_frame=np.zeros(0, np.int64), gt_track=np.zeros(0, np.int64), gt_box=np.zeros((0, 4), np.float32))
    seqs = [sa, no_gt, sb]                                                # (a sequence without ground truth runs no inference)
    kw = dict(cur_win_size=m['cur_win_size'], ret_win_size=m['ret_win_size'], use_hungarian=m['hungarian'],
              tp_classifier=m['tp_classifier'])
    ev = MotEvaluator(seqs, DEV)
    plain = validate(model, seqs, ev, **kw)
    assert 'att_hist' not in plain
    am = AttentionMonitor(DEV, 2)
    out = validate(model, seqs, ev, att_monitor=am, **kw)
    assert repr({k: v for k, v in out.items() if k != 'att_hist'}) == repr(plain)
    # each sequence on its own, in the same settings and with the same model
    per = []
    for n in (a, b):
        one = AttentionMonitor(DEV, 2)
        _infer(model, runs[n]['d'], m, one)
        per.append(one.read())
    got = out['att_hist']
    assert np.array_equal(got['counts'], per[0]['counts'] + per[1]['counts'])
    for k in ('forwards', 'dets', 'isolated', 'zeros'):
        assert got[k] == per[0][k] + per[1][k]
    assert np.array_equal(per[0]['counts'], runs[a]['d']['hist'])         # the first sequence ran in its own fixture's settings
    # a second pass resets the monitor first
    out2 = validate(model, seqs, ev, att_monitor=am, **kw)
    assert np.array_equal(out2['att_hist']['counts'], got['counts']) and out2['att_hist']['forwards'] == got['forwards']


def test_error_paths(runs):
    from trackmpnn_amd import AttentionMonitor, TrackMPNN
    with pytest.raises(ValueError, match='nattheads'):
        AttentionMonitor(DEV, 0)
    with pytest.raises(ValueError, match='bins=65'):
        AttentionMonitor(DEV, 2, bins=65)
    AttentionMonitor(DEV, 2, bins=64)
    name = att_fixture_names()[0]
    q = runs[name]
    wrong = AttentionMonitor(DEV, q['m']['nattheads'] + 1)
    with pytest.raises(ValueError, match='heads'):                        # K different from the attention handed in
        _infer(q['model'], q['d'], q['m'], wrong)
    assert not wrong.record.any().item()
    torch.manual_seed(0)
    plain = TrackMPNN('2d', 3, 32, 0, 'diff').to(DEV).eval()             # a model without heads: nothing to count
    with pytest.raises(ValueError, match='no attention'):
        _infer(plain, q['d'], q['m'], AttentionMonitor(DEV, 2))
