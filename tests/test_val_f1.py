"""The validation F1's host definition (trackmpnn_amd.monitor.val_counts_host / val_f1_host) against what the REAL reference
computed per forward call (fixtures tests/golden/val_f1/*.npz from tools/gen_val_f1_golden.py: the reference's create_targets,
argmax and sklearn's f1_score(zero_division=0) after every model call of its validation loop), the conditions the fixture set
has to meet, hand cases and the entry point's argument checks -- no GPU.  tests/test_val_f1_gpu.py holds the device kernel and
both inference paths to this definition."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN_DIR
from trackmpnn_amd.monitor import val_counts_host, val_f1_host

VAL_DIR = os.path.join(GOLDEN_DIR, 'val_f1')
MARGIN = 1e-3            # ten times the 1e-4 of tests/test_tracking_gpu.py's device-versus-fixture score comparisons


def val_fixture_names():
    return sorted(f[:-4] for f in os.listdir(VAL_DIR) if f.endswith('.npz'))


def load(name):
    d = np.load(os.path.join(VAL_DIR, name + '.npz'))
    return d, json.loads(str(d['meta']))


def mean_bound(n):
    """Any fp64 summation order of n terms in [0, 1] (and the division by n) stays within n^2 2^-52 of any other."""
    return n * n * 2.0 ** -52


def test_the_set_is_there():
    assert len(val_fixture_names()) >= 5


@pytest.mark.parametrize('name', val_fixture_names())
def test_host_definition_equals_the_reference_on_every_forward(name):
    d, m = load(name)
    counts = []
    for c in range(m['ncalls']):
        got = val_counts_host(d[f'f{c}/is_edge'], d[f'f{c}/src'], d[f'f{c}/dst'], d[f'f{c}/labels'], d[f'f{c}/scores'],
                              m['tp_classifier'])
        assert got == tuple(int(v) for v in d[f'f{c}/counts']), (c, got, d[f'f{c}/counts'])
        counts.append(got)
    r = val_f1_host(counts)
    assert r['forwards'] == m['ncalls']
    for c, f1 in enumerate(r['per_forward']):
        tp, fp, fn, _ = counts[c]
        assert f1 == float(d[f'f{c}/f1']), (c, f1, float(d[f'f{c}/f1']))                 # sklearn's value, to the bit
        assert f1 == (2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)        # the fp64 quotient
    assert abs(r['f1'] - float(d['mean_f1'])) <= mean_bound(m['ncalls'])
    assert (r['tp'], r['fp'], r['fn'], r['rows']) == tuple(sum(c[k] for c in counts) for k in range(4))


@pytest.mark.parametrize('name', val_fixture_names())
def test_targets_are_the_references(name):
    """The label rule itself, row by row: the selection val_counts_host counts is create_targets' output."""
    d, m = load(name)
    for c in range(m['ncalls']):
        is_edge, t = d[f'f{c}/is_edge'] != 0, d[f'f{c}/targets'] != 0
        # a forward whose scores are all 1 has tp = the number of positive targets over the selection
        ones = np.ones(is_edge.size, np.float32)
        tp, fp, fn, rows = val_counts_host(is_edge, d[f'f{c}/src'], d[f'f{c}/dst'], d[f'f{c}/labels'], ones, True)
        assert (tp, fp, fn, rows) == (int(t.sum()), int((~t).sum()), 0, is_edge.size)
        tp, fp, fn, rows = val_counts_host(is_edge, d[f'f{c}/src'], d[f'f{c}/dst'], d[f'f{c}/labels'], ones, False)
        assert (tp, fp, fn) == (int((t & is_edge).sum()), int((~t & is_edge).sum()), 0)


def test_fixture_set_meets_its_conditions():
    """Conditions, not measurements (tools/gen_val_f1_golden.py refuses a seed that breaks one): checked on the committed files."""
    seen = dict(greedy=False, hungarian=False, tp=False, notp=False, w3=False, w5=False, r0=False, r2=False, reinit=False,
                hole=False, shuffled=False, multi_past=False, multi_future=False, twice=False, empty_selection=False,
                label_deleted=False)
    for name in val_fixture_names():
        d, m = load(name)
        seen['hungarian' if m['hungarian'] else 'greedy'] = True
        seen['tp' if m['tp_classifier'] else 'notp'] = True
        for k, v in (('w3', m['cur_win_size'] == 3), ('w5', m['cur_win_size'] == 5), ('r0', m['ret_win_size'] == 0),
                     ('r2', m['ret_win_size'] == 2), ('reinit', m['reinitialisations'] > 0), ('shuffled', m['shuffled'])):
            seen[k] = seen[k] or bool(v)
        if m['shuffled']:
            ts = d['y'][0, :, 0]
            assert (np.diff(ts) < 0).any()                                               # not listed in time order
        n_prev = None
        for c in range(m['ncalls']):
            is_edge, lab = d[f'f{c}/is_edge'] != 0, d[f'f{c}/labels'] != 0
            src, dst = d[f'f{c}/src'].astype(np.int64), d[f'f{c}/dst'].astype(np.int64)
            # the margin: pred cannot differ between the reference's CPU scores and the device's
            assert np.abs(d[f'f{c}/scores'].astype(np.float64) - 0.5).min() >= MARGIN, (name, c)
            pos = np.flatnonzero(is_edge & lab)
            if pos.size:
                seen['multi_past'] |= bool(np.bincount(dst[pos]).max() >= 2)
                seen['multi_future'] |= bool(np.bincount(src[pos]).max() >= 2)
            for r in pos:
                if r == pos[dst[pos] == dst[r]].max() and r == pos[src[pos] == src[r]].min():
                    seen['twice'] = True
            if not m['tp_classifier'] and not is_edge.any():
                assert lab.size > 0 and float(d[f'f{c}/f1']) == 0.0                      # the reference appended 0.0
                seen['empty_selection'] = True
            if n_prev == lab.size and m['reinitialisations'] == 0:
                seen['hole'] = True                                                      # a forward without new rows
            if c >= 1:
                keep = d[f'f{c}/keep']
                gone = np.setdiff1d(np.flatnonzero(lab), keep)
                if gone.size and keep.size and keep.max() > gone.min():
                    seen['label_deleted'] = True
                n_prev = keep.size
            else:
                n_prev = lab.size
    assert all(seen.values()), [k for k, v in seen.items() if not v]


# ---- hand cases -------------------------------------------------------------------------------------------------------
def _block(n0, n1):
    """Rows of [dets t0][edges t0 x t1, src-major][dets t1]."""
    N = n0 + n0 * n1 + n1
    is_edge = np.zeros(N, np.uint8)
    is_edge[n0:n0 + n0 * n1] = 1
    src, dst = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    src[n0:n0 + n0 * n1] = np.repeat(np.arange(n0), n1)
    dst[n0:n0 + n0 * n1] = n0 + n0 * n1 + np.tile(np.arange(n1), n0)
    return N, is_edge, src, dst


def test_edge_chosen_by_both_endpoints_counts_once():
    N, is_edge, src, dst = _block(1, 1)                         # det, edge, det
    labels = np.array([1, 1, 1], np.uint8)
    assert val_counts_host(is_edge, src, dst, labels, np.full(N, 0.9, np.float32), True) == (3, 0, 0, 3)
    assert val_counts_host(is_edge, src, dst, labels, np.full(N, 0.9, np.float32), False) == (1, 0, 0, 3)


def test_last_past_and_first_future_edge():
    # two earlier dets and one later det, both edges label-positive: the later det chooses the LAST edge, and each earlier det
    # its own (first) future edge -- so both edges are targets; with one earlier det and two later ones likewise
    N, is_edge, src, dst = _block(2, 1)
    labels = np.ones(N, np.uint8)
    assert val_counts_host(is_edge, src, dst, labels, np.ones(N, np.float32), False) == (2, 0, 0, N)
    # a det with two positive past edges whose sources each have an EARLIER positive future edge: only the last one is chosen
    # rows: d0 d1 | e(d0->d2) e(d1->d2) | d2 | e(d0->d3) e(d1->d3) | d3
    is_edge = np.array([0, 0, 1, 1, 0, 1, 1, 0], np.uint8)
    src = np.array([-1, -1, 0, 1, -1, 0, 1, -1], np.int32)
    dst = np.array([-1, -1, 4, 4, -1, 7, 7, -1], np.int32)
    labels = np.ones(8, np.uint8)
    # chosen: first future of d0 = row 2, of d1 = row 3; last past of d2 = row 3, of d3 = row 6  ->  rows 2, 3, 6; row 5 is not
    s = np.ones(8, np.float32)
    assert val_counts_host(is_edge, src, dst, labels, s, False) == (3, 1, 0, 8)


def test_score_of_exactly_one_half_predicts_zero():
    N, is_edge, src, dst = _block(1, 1)
    labels = np.array([1, 1, 1], np.uint8)
    s = np.array([0.5, 0.5, np.nextafter(np.float32(0.5), np.float32(1))], np.float32)
    assert val_counts_host(is_edge, src, dst, labels, s, True) == (1, 0, 2, 3)


def test_empty_selection_is_a_forward_of_f1_zero_and_no_rows_is_none():
    is_edge = np.zeros(2, np.uint8)
    none = np.full(2, -1, np.int32)
    c = val_counts_host(is_edge, none, none, np.ones(2, np.uint8), np.ones(2, np.float32), False)
    assert c == (0, 0, 0, 2)
    r = val_f1_host([c])
    assert (r['f1'], r['forwards']) == (0.0, 1)
    e = np.zeros(0, np.int32)
    c0 = val_counts_host(e, e, e, e, np.zeros(0, np.float32), True)
    assert c0 == (0, 0, 0, 0)
    r = val_f1_host([c0])
    assert r['forwards'] == 0 and np.isnan(r['f1'])
    r = val_f1_host([c0, (1, 0, 1, 3), c])
    assert r['forwards'] == 2 and r['per_forward'] == [2.0 / 3.0, 0.0] and r['f1'] == (2.0 / 3.0 + 0.0) / 2


# ---- the entry point: declared, exported, bound; bad arguments rejected on the host -----------------------------------------
def test_entry_point_validates_on_the_host():
    from trackmpnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert 'tmpnn_val_f1_count' in _lib.header_symbols() and 'tmpnn_val_f1_count' in _lib._SIGNATURES
    rec = (C.c_int64 * 6)()
    g = _lib.CDGraph()
    assert lib.tmpnn_val_f1_count(None, None, None, 1, rec, None, 0, None) == -1 and b'graph is null' in lib.tmpnn_last_error()
    assert lib.tmpnn_val_f1_count(C.byref(g), None, None, 1, None, None, 0, None) == -1
    assert b'record is null' in lib.tmpnn_last_error()
    g.N, g.cap = 32769, 32769
    assert lib.tmpnn_val_f1_count(C.byref(g), None, None, 1, rec, None, 0, None) == -1 and b'32768' in lib.tmpnn_last_error()
    g.N, g.cap = 4, 4
    assert lib.tmpnn_val_f1_count(C.byref(g), None, None, 1, rec, rec, 0, None) == -1 and b'log_cap' in lib.tmpnn_last_error()
    assert lib.tmpnn_val_f1_count(C.byref(g), None, None, 1, rec, None, 0, None) == -1 and b'arrays are null' in lib.tmpnn_last_error()
    g.N = 0                                                              # no rows: nothing is launched, nothing is counted
    assert lib.tmpnn_val_f1_count(C.byref(g), None, None, 1, rec, None, 0, None) == 0
    assert list(rec) == [0] * 6


def test_val_monitor_needs_the_device():
    from trackmpnn_amd import ValMonitor
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        ValMonitor('cpu')
