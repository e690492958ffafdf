"""The device training-batch builder without a GPU: its entry points reject bad arguments on the host, and the Python front
rejects a CPU target and malformed labels before anything reaches the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from trackmpnn_amd import _lib


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    assert lib.tmpnn_train_build_count(None, None) == -1 and b'descriptor is null' in lib.tmpnn_last_error()
    d = _lib.CTrainBuild()
    d.n = 3
    assert lib.tmpnn_train_build_count(ctypes.byref(d), None) == -1 and b'null pointer' in lib.tmpnn_last_error()
    d.n = -1
    assert lib.tmpnn_train_build_count(ctypes.byref(d), None) == -1
    d.n = 0
    assert lib.tmpnn_train_build_count(ctypes.byref(d), None) == 0            # nothing to do, nothing launched
    assert lib.tmpnn_train_build_calls(None, None) == -1
    assert lib.tmpnn_train_build_fill(None, 0, None) == -1
    # a batch with more kept chunks than inputs, no kept chunk, or LDS sizes beyond the limits
    d.n, d.B = 2, 3
    assert lib.tmpnn_train_build_calls(ctypes.byref(d), None) == -1 and b'B=3' in lib.tmpnn_last_error()
    d.B = 0
    assert lib.tmpnn_train_build_calls(ctypes.byref(d), None) == -1
    fake = 0x1000                                                             # (never dereferenced: the checks fail first)
    d.B, d.y, d.offsets, d.info, d.kept, d.cptr, d.counts = 1, fake, fake, fake, fake, fake, fake
    d.max_dets, d.max_slots = 48, 8
    assert lib.tmpnn_train_build_calls(ctypes.byref(d), None) == -1 and b'max_dets=48' in lib.tmpnn_last_error()
    d.max_dets, d.max_slots = 8192, 8
    assert lib.tmpnn_train_build_calls(ctypes.byref(d), None) == -1
    d.max_dets, d.max_slots = 64, 2
    assert lib.tmpnn_train_build_calls(ctypes.byref(d), None) == -1 and b'max_slots=2' in lib.tmpnn_last_error()
    d.max_slots = 8
    assert lib.tmpnn_train_build_fill(ctypes.byref(d), 2, None) == -1 and b'phase=2' in lib.tmpnn_last_error()
    d.C = 0
    assert lib.tmpnn_train_build_fill(ctypes.byref(d), 0, None) == -1 and b'C=0' in lib.tmpnn_last_error()
    d.C = 2
    assert lib.tmpnn_train_build_fill(ctypes.byref(d), 0, None) == -1 and b'null table' in lib.tmpnn_last_error()
    d.blk, d.call_tab, d.cb_tab, d.rowptr = fake, fake, fake, fake
    assert lib.tmpnn_train_build_fill(ctypes.byref(d), 0, None) == -1 and b'null output' in lib.tmpnn_last_error()
    assert lib.tmpnn_train_build_fill(ctypes.byref(d), 1, None) == -1 and b'inc is null' in lib.tmpnn_last_error()


def test_cpu_target_fails_loudly():
    from trackmpnn_amd import build_train_batch_device
    y = np.array([[0, 1], [1, 1]])
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        build_train_batch_device([y], device='cpu')
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        build_train_batch_device(torch.from_numpy(y), device='cpu', offsets=[0, 2])


@pytest.mark.parametrize('bad', [np.zeros((4, 3), np.int64), np.zeros((2, 4, 2), np.int64), np.zeros(6, np.int64),
                                 np.zeros((3, 2), np.complex64)])
def test_malformed_labels_are_rejected_before_the_device(bad):
    from trackmpnn_amd import build_train_batch_device
    good = np.array([[0, 1], [1, 1]])
    with pytest.raises(ValueError, match='labels'):
        build_train_batch_device([good, bad], device='cuda:0')
    with pytest.raises(ValueError, match='labels'):
        build_train_batch_device(torch.as_tensor(bad), device='cuda:0', offsets=[0, bad.shape[0]])


def test_malformed_offsets_are_rejected_before_the_device():
    from trackmpnn_amd import build_train_batch_device
    y = torch.zeros((4, 2), dtype=torch.int64)
    for off in ([[0, 2], [2, 4]], [0.0, 4.0], []):
        with pytest.raises(ValueError, match='offsets'):
            build_train_batch_device(y, device='cuda:0', offsets=off)


def test_exported():
    import trackmpnn_amd
    assert 'build_train_batch_device' in trackmpnn_amd.__all__
    from trackmpnn_amd.train_batch import TB_MAX_CALLS, TB_MAX_DETS
    assert TB_MAX_DETS >= 4096 and TB_MAX_CALLS >= 1024
