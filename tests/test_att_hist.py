"""The attention histograms' host definition (trackmpnn_amd.monitor.att_hist_host) against what the REAL reference's head study
selects (fixtures tests/golden/att_hist/*.npz from tools/gen_att_hist_golden.py: attention_weights.py's pass over its own model
and graph functions, its plot function's walk over the dense [N, N] matrices, np.histogram with the figure's arguments), the
conditions the fixture set has to meet, hand cases on the bin edges and the entry point's argument checks -- no GPU.
tests/test_att_hist_gpu.py holds the device kernel and infer_sequence / validate to this definition."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN_DIR
from trackmpnn_amd.monitor import att_csr_host, att_hist_edges, att_hist_host

ATT_DIR = os.path.join(GOLDEN_DIR, 'att_hist')
# ten times the tolerance of tests/test_small_path_gpu.py::test_fused_iteration_with_attention_heads_matches_the_reference, the
# device-versus-fixture comparison of the attention values: allclose(atol=1e-5, rtol=1e-4) on weights of at most 1
MARGIN = 10 * (1e-5 + 1e-4)
SCORE_MARGIN = 1e-3      # as tests/test_val_f1.py: the loop's decisions (score >= 0.5) must agree between reference and device


def att_fixture_names():
    return sorted(f[:-4] for f in os.listdir(ATT_DIR) if f.endswith('.npz'))


def load(name):
    d = np.load(os.path.join(ATT_DIR, name + '.npz'))
    return d, json.loads(str(d['meta']))


def two_frames(n0, n1, isolated=0):
    """Row form of `[n0 dets][n0 x n1 edges, src-major][n1 dets][isolated dets]`: (is_edge uint8, src, dst int32), N rows."""
    E = n0 * n1
    N = n0 + E + n1 + isolated
    is_edge = np.zeros(N, np.uint8)
    is_edge[n0:n0 + E] = 1
    src, dst = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    src[n0:n0 + E] = np.repeat(np.arange(n0), n1)
    dst[n0:n0 + E] = n0 + E + np.tile(np.arange(n1), n0)
    return is_edge, src, dst


def test_the_set_is_there():
    assert len(att_fixture_names()) >= 3


def test_edge_table_is_numpys():
    e = att_hist_edges(25)
    assert e.dtype == np.float32 and e.shape == (26,)
    assert np.array_equal(e, np.linspace(0, 1, 26).astype(np.float32))
    assert np.array_equal(e, np.histogram(np.zeros(1, np.float32), 25, (0.0, 1.0))[1])


@pytest.mark.parametrize('name', att_fixture_names())
def test_host_definition_equals_the_reference_on_every_forward(name):
    d, m = load(name)
    K = m['nattheads']
    total = np.zeros((K, 2, m['bins']), np.int64)
    for c in range(m['forwards']):
        is_edge, lab = d[f'f{c}/is_edge'], d[f'f{c}/labels']
        got = att_hist_host(is_edge, lab, d[f'f{c}/alpha'], is_edge.size, m['bins'], src=d[f'f{c}/src'], dst=d[f'f{c}/dst'])
        assert np.array_equal(got['counts'], d[f'f{c}/hist']), (c, got['counts'], d[f'f{c}/hist'])
        assert got['forwards'] == 1 and got['zeros'] == 0
        # the stored histogram is np.histogram of the walk's two lists, and the definition selects as many values as the walk
        for k in range(K):
            vals, tp = d[f'f{c}/values_k{k}'], d[f'f{c}/tp_k{k}']
            assert vals.dtype == np.float32
            assert np.array_equal(np.histogram(vals[tp == 1], m['bins'], (0.0, 1.0))[0], d[f'f{c}/hist'][k, 0])
            assert np.array_equal(np.histogram(vals[tp == 0], m['bins'], (0.0, 1.0))[0], d[f'f{c}/hist'][k, 1])
            assert int(got['counts'][k].sum()) == vals.size
            n_edges = int((is_edge != 0).sum())
            assert vals.size == d[f'f{c}/alpha'].shape[1] + got['isolated'] * n_edges
        total += got['counts']
    assert np.array_equal(total, d['hist']) and int(d['forwards']) == m['forwards']


def _conditions(d, m):
    res = dict(margin=np.inf, score_margin=float(np.abs(d['first_scores'].astype(np.float64) - 0.5).min()), isolated=False,
               mixed=False)
    edges = att_hist_edges(m['bins']).astype(np.float64)
    for c in range(m['forwards']):
        is_edge, lab = d[f'f{c}/is_edge'] != 0, d[f'f{c}/labels']
        dets, rowptr, inc = att_csr_host(is_edge, d[f'f{c}/src'], d[f'f{c}/dst'])
        deg = np.diff(rowptr)
        res['score_margin'] = min(res['score_margin'], float(np.abs(d[f'f{c}/scores'].astype(np.float64) - 0.5).min()))
        if not inc.size:
            continue
        al = d[f'f{c}/alpha']
        dist = np.abs(al.astype(np.float64)[..., None] - edges).min(-1)
        one = (np.repeat(deg, deg)[None, :] == 1) & (al == np.float32(1))       # exact on both sides: exp(0) / exp(0)
        assert bool((al[:, np.repeat(deg, deg) == 1] == np.float32(1)).all())
        res['margin'] = min(res['margin'], float(np.where(one, np.inf, dist).min()))
        res['isolated'] = res['isolated'] or bool((deg == 0).any())
        pos = (lab[inc & 0x7FFFFFFF] == 1).astype(np.int64)
        n_pos = np.add.reduceat(pos, rowptr[:-1][deg > 0])
        res['mixed'] = res['mixed'] or bool(((n_pos > 0) & (n_pos < deg[deg > 0])).any())
    return res


def test_fixture_set_meets_its_conditions():
    """Conditions, not measurements (tools/gen_att_hist_golden.py refuses a seed that breaks one): checked on the committed files."""
    seen = dict(k2=False, k3=False, greedy=False, hungarian=False, ret2=False, reinit=False, isolated=False, mixed=False)
    for name in att_fixture_names():
        d, m = load(name)
        assert (m['nhidden'], m['features'], m['ncategories'], m['mode'], m['bins']) == (32, '2d', 3, 'eval', 25)
        assert 8 <= m['T'] <= 10 and m['forwards'] >= 4
        assert os.path.getsize(os.path.join(ATT_DIR, name + '.npz')) < 1 << 20
        r = _conditions(d, m)
        print(name, m['forwards'], 'forwards', int(d['hist'].sum()), 'values', r)
        assert r['margin'] >= MARGIN, (name, r)
        assert r['score_margin'] >= SCORE_MARGIN, (name, r)
        assert bool((d['hist'].sum(-1) > 0).all()), f'{name}: a head has an empty tp or fp list'
        for k, v in (('k2', m['nattheads'] == 2), ('k3', m['nattheads'] == 3), ('greedy', not m['hungarian']),
                     ('hungarian', m['hungarian']), ('ret2', m['hungarian'] and m['ret_win_size'] == 2),
                     ('reinit', m['reinitialisations'] > 0), ('isolated', r['isolated']), ('mixed', r['mixed'])):
            seen[k] = seen[k] or bool(v)
    assert all(seen.values()), seen


# ---- hand-made cases ----------------------------------------------------------------------------------------------------------
def test_single_incident_edge_is_in_the_closed_last_bin():
    is_edge, src, dst = two_frames(1, 1)
    r = att_hist_host(is_edge, [1, 1, 1], np.ones((1, 2), np.float32), src=src, dst=dst)
    want = np.zeros((1, 2, 25), np.int64)
    want[0, 0, 24] = 2                                             # both dets give the edge 1.0: the last bin is closed
    assert np.array_equal(r['counts'], want) and (r['forwards'], r['dets'], r['isolated'], r['zeros']) == (1, 2, 0, 0)


def test_a_fifth_sits_on_edge_5_and_goes_to_bin_5():
    is_edge, src, dst = two_frames(1, 5)                           # det 0 has five edges: five equal scores give 0.2f each
    fifth = np.float32(1) / np.float32(5)
    assert fifth == att_hist_edges(25)[5]
    dets, rowptr, inc = att_csr_host(is_edge, src, dst)
    assert rowptr.tolist() == [0, 5, 6, 7, 8, 9, 10] and inc[:5].tolist() == [1, 2, 3, 4, 5]
    assert (inc[5:] == (np.arange(1, 6) | 0x80000000)).all()       # the later end of an edge: the sign bit
    alpha = np.concatenate([np.full(5, fifth, np.float32), np.ones(5, np.float32)])[None]
    lab = np.zeros(11, np.uint8)
    lab[[1, 3]] = 1
    r = att_hist_host(is_edge, lab, alpha, src=src, dst=dst)
    assert r['counts'][0, 0, 5] == 2 and r['counts'][0, 1, 5] == 3 and r['counts'][0, :, 4].sum() == 0
    assert r['counts'][0, 0, 24] == 2 and r['counts'][0, 1, 24] == 3 and int(r['counts'].sum()) == 10
    # the CSR form gives the same
    r2 = att_hist_host(is_edge, lab, alpha, rowptr=rowptr, inc=inc)
    assert np.array_equal(r2['counts'], r['counts'])


def test_isolated_det_of_25_rows_gives_a_twentyfifth_on_edge_1():
    is_edge, src, dst = two_frames(3, 4, isolated=6)               # 3 + 12 + 4 + 6 = 25 rows
    assert is_edge.size == 25
    u = np.float32(1) / np.float32(25)
    assert u == att_hist_edges(25)[1]
    lab = np.zeros(25, np.uint8)
    lab[[3, 8, 13]] = 1                                            # three label-1 edge rows of twelve
    alpha = np.full((2, 24), 0.5, np.float32)
    r = att_hist_host(is_edge, lab, alpha, src=src, dst=dst)
    assert (r['dets'], r['isolated']) == (13, 6)
    for k in range(2):
        assert r['counts'][k, 0, 1] == 6 * 3 and r['counts'][k, 1, 1] == 6 * 9 and r['counts'][k, :, 0].sum() == 0
        assert r['counts'][k, 0, 12] == 2 * 3 and r['counts'][k, 1, 12] == 2 * 9
    # N is the call's row count: with another N the uniform value moves
    r = att_hist_host(is_edge, lab, alpha, N=50, src=src, dst=dst)
    assert r['counts'][0, 0, 0] == 18 and r['counts'][0, :, 1].sum() == 0


def test_label_2_counts_as_fp_and_alpha_0_is_skipped():
    is_edge, src, dst = two_frames(2, 2)                           # rows 0 1 | 2 3 4 5 | 6 7
    lab = np.array([1, 1, 1, 2, 0, 1, 1, 1], np.uint8)
    alpha = np.full((1, 8), 0.5, np.float32)
    dets, rowptr, inc = att_csr_host(is_edge, src, dst)
    alpha[0, 0] = 0.0                                              # det 0's weight for edge row 2 underflowed
    r = att_hist_host(is_edge, lab, alpha, src=src, dst=dst)
    assert (inc & 0x7FFFFFFF).tolist() == [2, 3, 4, 5, 2, 4, 3, 5]
    assert r['zeros'] == 1 and r['counts'][0, 0, 12] == 3 and r['counts'][0, 1, 12] == 4 and int(r['counts'].sum()) == 7
    # values above the range are dropped, as np.histogram drops them
    alpha[0, 1] = 1.5
    r = att_hist_host(is_edge, lab, alpha, src=src, dst=dst)
    assert r['zeros'] == 1 and int(r['counts'].sum()) == 6


def test_graph_without_edges_is_a_forward_without_values():
    is_edge, src, dst = two_frames(3, 0)
    r = att_hist_host(is_edge, [1, 0, 1], np.zeros((2, 0), np.float32), src=src, dst=dst)
    assert (r['forwards'], r['dets'], r['isolated'], r['zeros']) == (1, 3, 3, 0) and int(r['counts'].sum()) == 0
    r = att_hist_host(np.zeros(0, np.uint8), [], np.zeros((2, 0), np.float32), src=[], dst=[])
    assert r['forwards'] == 0


def test_shape_mismatch_raises():
    is_edge, src, dst = two_frames(2, 2)
    with pytest.raises(ValueError):
        att_hist_host(is_edge, np.zeros(8), np.zeros((1, 7), np.float32), src=src, dst=dst)


# ---- the entry point and the monitor without a GPU ----------------------------------------------------------------------------
def test_entry_point_checks_its_arguments_without_a_gpu():
    from trackmpnn_amd import _lib
    lib = _lib.load()
    assert 'tmpnn_att_hist_count' in _lib.header_symbols() and 'tmpnn_att_hist_count' in _lib._SIGNATURES
    rec = (C.c_int64 * (4 + 2 * 2 * 25))()
    f = lib.tmpnn_att_hist_count
    assert f(None, None, None, 1, 1, 0, None, 25, rec, 1, None) == -1 and b'graph is null' in lib.tmpnn_last_error()
    g = _lib.CDGraph(4, 4, None, None, None, None, None, None, None, None, None, None, None)
    assert f(C.byref(g), None, None, 1, 1, 0, None, 25, None, 1, None) == -1 and b'record is null' in lib.tmpnn_last_error()
    big = _lib.CDGraph(32769, 32769, None, None, None, None, None, None, None, None, None, None, None)
    assert f(C.byref(big), None, None, 1, 1, 0, None, 25, rec, 1, None) == -1 and b'32768' in lib.tmpnn_last_error()
    assert f(C.byref(g), None, None, 1, 9, 0, None, 25, rec, 1, None) == -1 and b'heads=9' in lib.tmpnn_last_error()
    assert f(C.byref(g), None, None, 1, 0, 0, None, 25, rec, 1, None) == -1
    assert f(C.byref(g), None, None, 1, 1, -1, None, 25, rec, 1, None) == -1
    assert f(C.byref(g), None, None, 1, 1, 0, None, 65, rec, 1, None) == -1 and b'bins=65' in lib.tmpnn_last_error()
    assert f(C.byref(g), None, None, 0, 1, 0, None, 25, rec, 1, None) == -1 and b'stride' in lib.tmpnn_last_error()
    assert f(C.byref(g), None, None, 1, 1, 0, None, 25, rec, 1, None) == -1 and b'arrays are null' in lib.tmpnn_last_error()
    empty = _lib.CDGraph(0, 0, None, None, None, None, None, None, None, None, None, None, None)
    assert f(C.byref(empty), None, None, 1, 1, 0, None, 25, rec, 1, None) == 0          # no rows: nothing is launched
    assert list(rec) == [0] * len(rec)


def test_monitor_off_gpu_fails_loudly():
    from trackmpnn_amd import AttentionMonitor
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        AttentionMonitor('cpu', 2)


def test_loops_take_the_monitor_argument():
    import inspect
    from trackmpnn_amd import loops
    for fn in (loops.infer_sequence, loops.validate):
        assert inspect.signature(fn).parameters['att_monitor'].default is None
