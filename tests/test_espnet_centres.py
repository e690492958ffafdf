"""The embedding CNN answered at single pixels, without a GPU: the size of the smaller workspace, the host definition
espnet_centres_host against the fixtures under tests/golden/espnet, and the constructor's refusal of a host device."""
import os

import numpy as np
import pytest
import torch

from tests.espnet_cases import CASES, load_case
from trackmpnn_amd import EspEmbedNet, _lib, espnet_centres_host


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize('shape', [(1, 16, 16, 8), (3, 16, 32, 8), (1, 384, 1280, 128)])
def test_the_workspace_is_smaller_by_the_four_tail_maps(lib, shape):
    T, H, W, C = shape
    P2, P4 = (H // 2) * (W // 2), (H // 4) * (W // 4)
    dense, sparse = lib.tmpnn_espnet_ws_bytes(T, H, W, C), lib.tmpnn_espnet_centres_ws_bytes(T, H, W, C)
    print(f'{shape}: dense {dense} bytes, centres {sparse} bytes')
    assert 0 < sparse <= dense - 4 * T * C * (2 * P4 + 2 * P2)


def test_the_workspace_size_is_zero_for_the_shapes_the_dense_call_refuses(lib):
    for T, H, W, C in ((0, 16, 16, 8), (1, 24, 40, 8), (1, 16, 8, 8), (1, 16, 16, 0), (1, 16, 16, 1025), (65536, 16, 16, 8),
                       (1, 4096, 4096, 128)):
        assert lib.tmpnn_espnet_ws_bytes(T, H, W, C) == 0 and lib.tmpnn_espnet_centres_ws_bytes(T, H, W, C) == 0, (T, H, W, C)


def test_the_new_entry_points_validate_on_the_host(lib):
    p = 1 << 20
    assert lib.tmpnn_espnet_trunk(None, 8, p, 1, 16, 16, p, 1 << 30, None) == -1 and b'null pointer' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_trunk(p, 8, p, 1, 24, 16, p, 1 << 30, None) == -1 and b'multiples of 16' in lib.tmpnn_last_error()
    need = lib.tmpnn_espnet_centres_ws_bytes(1, 16, 16, 8)
    assert lib.tmpnn_espnet_trunk(p, 8, p, 1, 16, 16, p, need - 16, None) == -3 and b'workspace' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_centres(p, 8, 1, 16, 16, p, need - 16, p, 4, p, p, None) == -3
    assert lib.tmpnn_espnet_centres(p, 8, 1, 16, 16, p, need, None, 4, p, p, None) == -1
    assert lib.tmpnn_espnet_centres(p, 8, 1, 16, 16, p, need, p, -1, p, p, None) == -1
    assert lib.tmpnn_espnet_centres(p, 257, 1, 16, 16, p, 1 << 30, p, 4, p, p, None) == -1 and b'dense call' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_centres(p, 8, 1, 16, 16, p, need, None, 0, None, None, None) == 0          # D = 0: nothing to launch


def test_host_definition_at_every_pixel_equals_the_reference_in_float64():
    fx, sd = load_case('c1_16x16')
    T, C, H, W, _ = CASES['c1_16x16']
    pix = np.arange(T * H * W)
    got = espnet_centres_host(sd, torch.from_numpy(fx['images']), pix, torch.float64)
    assert got.dtype == torch.float64 and tuple(got.shape) == (T * H * W, C)
    ref = fx['ref_out64']
    want = ref.transpose(0, 2, 3, 1).reshape(T * H * W, C)                  # [pix, c] = ref[t, c, cy, cx]
    err = np.abs(got.numpy() - want).max()
    print(f'c1_16x16: max|host centres - ref| = {err:.3g}, max|ref| = {np.abs(ref).max():.3g}')
    assert err <= 1e-10 * np.abs(ref).max()
    with pytest.raises(ValueError, match='outside'):
        espnet_centres_host(sd, torch.from_numpy(fx['images']), [T * H * W], torch.float64)


def test_a_host_device_fails_as_loudly_as_the_dense_constructor():
    _, sd = load_case('c1_16x16')
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        EspEmbedNet.from_state_dict(sd, 'cpu', centres=True)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        EspEmbedNet(sd, 'cpu', centres=True)
