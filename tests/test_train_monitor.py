"""The training monitor's C entry points without a GPU: declared, exported, bound (tests/test_abi.py covers that for every
entry point) and rejecting null arguments on the host, before any launch."""
import ctypes

import pytest

from trackmpnn_amd import _lib


@pytest.fixture(scope='module')
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_monitor_entry_points_are_declared_and_bound(lib):
    names = _lib.header_symbols()
    for n in ('tmpnn_cls_counts', 'tmpnn_cls_counts_win', 'tmpnn_train_record_fold'):
        assert n in names and n in _lib._SIGNATURES and hasattr(lib, n), n
    assert _lib.ABI_VERSION >= 7 and lib.tmpnn_abi_version() == _lib.ABI_VERSION


def test_monitor_entry_points_reject_null_arguments_on_the_host(lib):
    g = _lib.CGraph(3, 1, 2, None, None, None, None, None, None)
    w = _lib.CLossWindows(2, 2, 1, None, None, None, None, None, None)
    fake = 1 << 20                                             # never dereferenced: every call below fails validation first
    # counts of one graph
    assert lib.tmpnn_cls_counts(None, fake, fake, 1, fake, None) == -1
    assert b'cls_counts: graph is null' in lib.tmpnn_last_error()
    assert lib.tmpnn_cls_counts(ctypes.byref(g), fake, fake, 1, None, None) == -1
    assert b'counts is null' in lib.tmpnn_last_error()
    assert lib.tmpnn_cls_counts(ctypes.byref(g), None, fake, 1, fake, None) == -1
    assert b'scores / targets' in lib.tmpnn_last_error()
    assert lib.tmpnn_cls_counts(ctypes.byref(g), fake, None, 1, fake, None) == -1
    assert lib.tmpnn_cls_counts(ctypes.byref(g), fake, fake, 1, fake, None) == -1          # the graph's own lists are null
    assert b'row lists' in lib.tmpnn_last_error()
    # counts per window
    assert lib.tmpnn_cls_counts_win(None, ctypes.byref(w), fake, fake, 1, fake, None) == -1
    assert b'cls_counts_win: graph is null' in lib.tmpnn_last_error()
    assert lib.tmpnn_cls_counts_win(ctypes.byref(g), None, fake, fake, 1, fake, None) == -1
    assert b'windows is null' in lib.tmpnn_last_error()
    assert lib.tmpnn_cls_counts_win(ctypes.byref(g), ctypes.byref(w), fake, fake, 1, None, None) == -1
    assert b'counts is null' in lib.tmpnn_last_error()
    assert lib.tmpnn_cls_counts_win(ctypes.byref(g), ctypes.byref(w), fake, fake, 1, fake, None) == -1
    assert b'window pointers' in lib.tmpnn_last_error()
    big = _lib.CLossWindows(2, 5, 1, fake, fake, fake, fake, None, None)                    # more listed dets than the graph has
    assert lib.tmpnn_cls_counts_win(ctypes.byref(g), ctypes.byref(big), fake, fake, 1, fake, None) == -1
    assert b'n_det=5' in lib.tmpnn_last_error()
    # the fold
    assert lib.tmpnn_train_record_fold(fake, 2, 2, fake, fake, 2, None, None) == -1
    assert b'record is null' in lib.tmpnn_last_error()
    assert lib.tmpnn_train_record_fold(None, 2, 2, fake, fake, 2, fake, None) == -1
    assert b'counts is null' in lib.tmpnn_last_error()
    assert lib.tmpnn_train_record_fold(fake, 2, 2, None, fake, 2, fake, None) == -1
    assert b'loss_c / loss_f' in lib.tmpnn_last_error()
    assert lib.tmpnn_train_record_fold(fake, -1, 2, fake, fake, 2, fake, None) == -1


def test_monitor_needs_a_device():
    from trackmpnn_amd import TrainMonitor
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        TrainMonitor('cpu')
