"""The embedding CNN without a GPU: the host definition espnet_host against the fixtures the reference's EESPNet_Seg left under
tests/golden/espnet (tools/gen_espnet_golden.py), strict loading, the shape checks, the module surface, the argument checks of
the new entry points, and the BatchNorm folding of the device's weight arena."""
import numpy as np
import pytest
import torch

from tests.espnet_cases import CASES, TAPS, espnet_weights, load_case
from trackmpnn_amd import EspEmbedNet, espnet_host
from trackmpnn_amd import _lib
from trackmpnn_amd.espnet import check_state_dict, espnet_spec, fold_bn, pack_arena


@pytest.fixture(scope='module')
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize('name', list(CASES))
def test_host_definition_equals_the_reference_in_float64(name):
    """The same float64 torch ops in the same composition: anything above 1e-10 max|ref| is a restatement error."""
    fx, sd = load_case(name)
    T, C, H, W, _ = CASES[name]
    assert fx['images'].shape == (T, 3, H, W) and fx['ref_out64'].shape == (T, C, H, W) and fx['ref_out32'].dtype == np.float32
    out, taps = espnet_host(sd, torch.from_numpy(fx['images']), torch.float64, taps=True)
    assert out.dtype == torch.float64 and tuple(out.shape) == (T, C, H, W)
    ref = fx['ref_out64']
    err = np.abs(out.numpy() - ref).max()
    print(f'{name}: max|host - ref| = {err:.3g}, max|ref| = {np.abs(ref).max():.3g}')
    assert err <= 1e-10 * np.abs(ref).max()
    for k in TAPS:
        assert taps[k].shape == fx[k].shape
        assert np.abs(taps[k].numpy() - fx[k]).max() <= 1e-10 * np.abs(fx[k]).max(), k
    assert set(taps) == set(TAPS) | {'merge_l3', 'merge_l2', 'merge_l1'}
    assert tuple(taps['merge_l1'].shape) == (T, C, H // 2, W // 2) and tuple(taps['merge_l3'].shape) == (T, 128, H // 8, W // 8)


def test_the_state_dict_is_the_reference_modules():
    sd = espnet_weights(8, 3)
    assert len(sd) == 418 and next(iter(sd)) == 'net.level1.conv.weight' and list(sd)[-1] == 'project_l1.1.conv.weight'
    assert len(espnet_spec(8)) + sum(k.endswith('num_batches_tracked') for k in sd) == 418
    assert not any(k.startswith('net.level5') or 'classifier' in k for k in sd)
    for C in (1, 8, 20, 128):
        assert check_state_dict(espnet_weights(C, 4)) == C                 # C is read from project_l3.1.conv.weight


def test_loading_is_strict():
    sd = espnet_weights(8, 5)
    for key in ('net.level4.6.spp_dw.3.conv.weight', 'act_l3.bn.running_var', 'net.level2_0.eesp.module_act.weight'):
        bad = dict(sd)
        del bad[key]
        with pytest.raises(ValueError, match='missing key ' + key.replace('.', r'\.')):
            EspEmbedNet.from_state_dict(bad)
    bad = dict(sd)
    bad['net.level5_0.act.weight'] = torch.zeros(512)
    with pytest.raises(ValueError, match=r'unexpected key net\.level5_0\.act\.weight'):
        EspEmbedNet.from_state_dict(bad)
    bad = dict(sd)
    bad['classifier.num_batches_tracked'] = torch.tensor(0)                    # only a BatchNorm of the net may carry one
    with pytest.raises(ValueError, match='unexpected key classifier'):
        EspEmbedNet.from_state_dict(bad)
    bad = dict(sd)
    bad['project_l2.conv.weight'] = torch.zeros(8, 64 + 9, 1, 1)
    with pytest.raises(ValueError, match=r'project_l2\.conv\.weight of shape \(8, 73, 1, 1\)'):
        EspEmbedNet.from_state_dict(bad)
    bad = dict(sd)
    bad['net.level3.1.proj_1x1.conv.weight'] = torch.zeros(32, 128, 1, 1)      # the ungrouped shape
    with pytest.raises(ValueError, match=r'net\.level3\.1\.proj_1x1\.conv\.weight'):
        EspEmbedNet.from_state_dict(bad)
    with pytest.raises(ValueError, match=r"module\.': this is the state dict of a DataParallel wrapper"):
        EspEmbedNet.from_state_dict({'module.' + k: v for k, v in sd.items()})
    no_counts = {k: v for k, v in sd.items() if not k.endswith('num_batches_tracked')}
    assert check_state_dict(no_counts) == 8                                    # accepted and ignored, present or not
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        EspEmbedNet.from_state_dict(sd, device='cpu')


def test_sizes_that_are_no_multiple_of_16_raise():
    sd = espnet_weights(8, 6)
    for H, W in ((24, 40), (20, 36), (16, 40), (0, 16)):
        with pytest.raises(ValueError, match='multiples of 16'):
            espnet_host(sd, torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError, match=r'images \[T, 3, H, W\]'):
        espnet_host(sd, torch.zeros(1, 4, 16, 16))


def test_the_module_surface_is_an_eval_mode_net():
    net = EspEmbedNet.__new__(EspEmbedNet)                                     # (no device is touched)
    assert net.training is False and net.eval() is net and net.train(False) is net
    with pytest.raises(NotImplementedError, match='eval-mode network: train the CNN in torch'):
        net.train(True)
    with pytest.raises(NotImplementedError):
        net.train()


def test_host_tensors_fail_loudly():
    net = EspEmbedNet.__new__(EspEmbedNet)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        net(torch.zeros(1, 3, 16, 16))


def test_entry_points_check_their_arguments_before_any_launch(lib):
    p = 1 << 20                                                                # (never read: every call fails its checks first)
    assert lib.tmpnn_espnet_fwd(None, 8, p, 1, 16, 16, p, 1 << 30, p, None) == -1 and b'null pointer' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_fwd(p, 8, None, 1, 16, 16, p, 1 << 30, p, None) == -1
    assert lib.tmpnn_espnet_fwd(p, 8, p, 1, 16, 16, None, 1 << 30, p, None) == -1
    assert lib.tmpnn_espnet_fwd(p, 8, p, 1, 16, 16, p, 1 << 30, None, None) == -1
    for H, W in ((24, 40), (20, 36), (16, 40), (0, 16), (-16, 16)):
        assert lib.tmpnn_espnet_fwd(p, 8, p, 1, H, W, p, 1 << 30, p, None) == -1 and b'multiples of 16' in lib.tmpnn_last_error()
        assert lib.tmpnn_espnet_ws_bytes(1, H, W, 8) == 0
    assert lib.tmpnn_espnet_fwd(p, 8, p, 0, 16, 16, p, 1 << 30, p, None) == -1 and b'T=0' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_fwd(p, 0, p, 1, 16, 16, p, 1 << 30, p, None) == -1
    assert lib.tmpnn_espnet_fwd(p, 128, p, 1, 4096, 4096, p, 1 << 30, p, None) == -1          # 160 H W >= 2^31
    assert lib.tmpnn_espnet_fwd(p, 8, p + 4, 1, 16, 16, p, 1 << 30, p, None) == -1 and b'aligned' in lib.tmpnn_last_error()
    need = lib.tmpnn_espnet_ws_bytes(1, 16, 16, 8)
    assert need > 0 and need % 16 == 0
    assert lib.tmpnn_espnet_fwd(p, 8, p, 1, 16, 16, p, need - 16, p, None) == -3 and b'workspace' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_ws_bytes(3, 16, 32, 8) > 3 * lib.tmpnn_espnet_ws_bytes(1, 16, 16, 8)
    assert lib.tmpnn_espnet_ws_bytes(0, 16, 16, 8) == 0 and lib.tmpnn_espnet_ws_bytes(1, 16, 16, 0) == 0
    assert lib.tmpnn_espnet_arena_floats(0) == 0 and lib.tmpnn_espnet_arena_floats(1025) == 0


def test_the_arena_holds_every_weight_once(lib):
    """Its length is the library's, and it grows with C by exactly the C-dependent segments (each padded to 4 floats)."""
    pad = lambda n: (n + 3) // 4 * 4
    for C in (8, 5, 128):
        arena = pack_arena(espnet_weights(C, 7))
        assert arena.dtype == np.float32 and arena.size == lib.tmpnn_espnet_arena_floats(C) and arena.size % 4 == 0
        assert np.isfinite(arena).all()
    tail = lambda C: pad(128 * C) + pad((64 + C) * C) + pad((32 + C) * C) + 9 * pad(C)
    assert lib.tmpnn_espnet_arena_floats(128) - lib.tmpnn_espnet_arena_floats(8) == tail(128) - tail(8)
    sd = espnet_weights(8, 7)
    arena = pack_arena(sd)
    w = sd['net.level1.conv.weight'].numpy().ravel()
    assert np.array_equal(arena[:w.size], w)                                   # the first segment: level1's conv as it is
    last = sd['project_l1.1.conv.weight'].numpy()[:, :, 0, 0].T                # the last layer: Wt [40][8] | ones | zeros | ones
    assert np.array_equal(arena[-(320 + 24):-24], last.ravel())
    assert np.array_equal(arena[-24:], np.concatenate([np.ones(8), np.zeros(8), np.ones(8)]).astype(np.float32))


def test_bn_folding_against_an_explicit_batch_norm_in_float64():
    rng = np.random.default_rng(11)
    c = 37
    w, b = rng.uniform(0.5, 1.5, c), rng.uniform(-0.3, 0.3, c)
    m, v = rng.uniform(-0.3, 0.3, c), rng.uniform(0.5, 1.5, c)
    x = rng.standard_normal((2, c, 5, 7)) * 3
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ref = torch.nn.functional.batch_norm(t(x), t(m), t(v), t(w), t(b), False, 0.0, 1e-5).numpy()
    scale, shift = fold_bn(t(w).float(), t(b).float(), t(m).float(), t(v).float())
    assert scale.dtype == np.float32 and shift.dtype == np.float32
    # exact folding from the float32 parameters, then one rounding of scale and of shift: 2^-24 relative each
    w32, b32, m32, v32 = (np.asarray(a, np.float32).astype(np.float64) for a in (w, b, m, v))
    exact = torch.nn.functional.batch_norm(t(x), t(m32), t(v32), t(w32), t(b32), False, 0.0, 1e-5).numpy()
    got = x * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None]
    s64 = w32 / np.sqrt(v32 + 1e-5)
    bound = 2.0 ** -24 * (np.abs(x) * np.abs(s64)[None, :, None, None] + np.abs(b32 - m32 * s64)[None, :, None, None]) + 1e-15
    assert (np.abs(got - exact) <= bound).all()
    assert np.abs(exact - ref).max() < 1e-6                                    # (float32 parameters against float64 ones)
