"""Training the embedding CNN's decoder, the parts that need no GPU: the host definition against the gradients recorded from the
reference module, the parameter lists, the state dict round trip, the size and table functions and the argument checks."""
import numpy as np
import pytest
import torch

from tests.espnet_cases import CASES, case_images, espnet_weights
from tests.espnet_grad_cases import GRAD_CASES, TAPS, case_d_maps, load_grad_case
from trackmpnn_amd import _lib
from trackmpnn_amd import espnet as E


@pytest.fixture(scope='module')
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize('name,form', GRAD_CASES)
def test_host_definition_equals_the_reference_gradients(name, form):
    """espnet_decoder_grads_host in float64 against the .double() reference module: 1e-10 of each tensor's largest entry (the
    bound tests/test_espnet.py holds the forward to)."""
    g64, _, gmax, sd = load_grad_case(name, form)
    got = E.espnet_decoder_grads_host(sd, torch.from_numpy(case_images(name)), torch.from_numpy(case_d_maps(name, form)))
    assert sorted(got) == sorted(g64) and len(got) == 40
    for k, ref in g64.items():
        g = got[k].numpy()
        assert g.dtype == np.float64 and g.shape == ref.shape, k
        assert gmax[k] > 0.0, k
        err = float(np.abs(g - ref).max())
        assert err <= 1e-10 * gmax[k], f'{name} {form} {k}: {err:.3e} against {gmax[k]:.3e}'


def test_fixture_files_are_small():
    import glob
    import os
    from tests.espnet_grad_cases import GOLDEN
    files = glob.glob(os.path.join(GOLDEN, '*.npz'))
    assert len(files) >= 2 * len(GRAD_CASES)
    for f in files:
        assert os.path.getsize(f) < 2 ** 20, f


def test_sparse_d_maps_keep_five_pixels():
    for name, form in GRAD_CASES:
        d = case_d_maps(name, form)
        T, C, H, W, _ = CASES[name]
        assert d.shape == (T, C, H, W) and d.dtype == np.float32
        live = int(np.any(d != 0, axis=1).sum())
        assert live == (5 if form == 'sparse' else T * H * W)


@pytest.mark.parametrize('C', [8, 128])
def test_parameter_names(C):
    """The decoder's 36 tensors, none of the encoder's, no running statistic; the trained ones are the tail behind merge_l3, in
    the state dict's order, and the table of the library lists the same tensors with the same sizes."""
    spec = E.espnet_spec(C)
    dec = E.decoder_param_names(C)
    assert len(dec) == 36 and len(set(dec)) == 36
    assert not [k for k in dec if k.startswith('net.') or 'running_' in k]
    assert sum(int(np.prod(spec[k])) for k in dec) == {8: 130192, 128: 190432}[C]
    assert set(dec) == {k for k in spec if not k.startswith('net.') and 'running_' not in k}
    tr = E.trained_param_names(C)
    assert tr == ('project_l3.1.conv.weight', 'act_l3.bn.weight', 'act_l3.bn.bias', 'act_l3.act.weight', 'project_l2.conv.weight',
                  'project_l2.bn.weight', 'project_l2.bn.bias', 'project_l2.act.weight', 'project_l1.1.conv.weight')
    assert [k for k in dec if k in tr] == list(tr)


@pytest.mark.parametrize('C', [1, 8, 128, 1024])
def test_table_and_sizes_need_no_gpu(lib, C):
    table = E.train_table(C)
    names = E.trained_param_names(C)
    spec = E.espnet_spec(C)
    assert len(table) == len(names) == 9
    at = 0
    for (off, n, arena_off), k in zip(table, names):
        assert off == at and n == int(np.prod(spec[k])), k              # one flat buffer, no padding: GradBucket's layout
        assert 0 <= arena_off and arena_off + n <= lib.tmpnn_espnet_arena_floats(C) and arena_off % 4 == 0
        at += n
    assert lib.tmpnn_espnet_train_param_floats(C) == at
    assert lib.tmpnn_espnet_train_ws_bytes(2, 32, 64, C) >= lib.tmpnn_espnet_ws_bytes(2, 32, 64, C) + 4 * 2 * C * (8 * 16 + 4 * 8)
    assert lib.tmpnn_espnet_train_bwd_ws_bytes(2, 32, 64, C) >= 4 * 2 * C * (2 * 16 * 32 + 2 * 8 * 16 + 4 * 8)


def test_table_matches_the_packed_arena(lib):
    """The arena offsets of the table point at the segments pack_arena fills from those tensors."""
    C = 8
    sd = espnet_weights(C, 102)
    arena = E.pack_arena(sd, C)
    for (_, n, arena_off), k in zip(E.train_table(C), E.trained_param_names(C)):
        seg = arena[arena_off:arena_off + n]
        v = sd[k].numpy()
        if k.endswith('conv.weight'):
            assert np.array_equal(seg, v[:, :, 0, 0].T.ravel()), k
        elif k.endswith('act.weight'):
            assert np.array_equal(seg, v), k
        else:                                                           # bn.weight -> scale, bn.bias -> shift
            p = k[:-len('.weight')] if k.endswith('.weight') else k[:-len('.bias')]
            scale, shift = E.fold_bn(*(sd[f'{p}.{s}'] for s in ('weight', 'bias', 'running_mean', 'running_var')))
            assert np.array_equal(seg, scale if k.endswith('.weight') else shift), k


def test_refused_shapes_and_arguments(lib):
    assert lib.tmpnn_espnet_train_param_floats(0) == 0 and lib.tmpnn_espnet_train_param_floats(1025) == 0
    for f in (lib.tmpnn_espnet_train_ws_bytes, lib.tmpnn_espnet_train_bwd_ws_bytes):
        assert f(0, 32, 32, 8) == 0 and f(1, 30, 32, 8) == 0 and f(1, 32, 32, 0) == 0 and f(1, 32768, 32768, 8) == 0
        assert f(1, 16, 16, 8) > 0
    assert lib.tmpnn_espnet_train_table(0, None, 0) == -1 and b'espnet_train_table' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_train_table(8, None, 4) == -1
    assert lib.tmpnn_espnet_refold(None, 8, None, None, None) == -1 and b'espnet_refold: null' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_refold(16, 0, 16, 16, None) == -1
    assert lib.tmpnn_espnet_train_fwd(None, 8, None, 1, 16, 16, None, 0, None, None) == -1
    assert b'espnet_train_fwd: null' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_train_fwd(16, 8, 16, 1, 16, 24, 16, 0, 16, None) == -1 and b'multiples of 16' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_train_fwd(16, 8, 16, 1, 16, 16, 16, 0, 16, None) == -3          # a short workspace, before any launch
    assert lib.tmpnn_espnet_train_bwd(None, 8, None, None, 1, 16, 16, None, 0, None, None, 0, None, None, None, None) == -1
    assert lib.tmpnn_espnet_train_bwd(16, 8, 16, 16, 1, 16, 16, 16, 1 << 40, 16, 16, 1 << 40, 16, 16, None, None) == -1
    assert b'together' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_train_bwd(16, 8, 16, 16, 1, 16, 16, 16, 0, 16, 16, 0, 16, None, None, None) == -3


def test_state_dict_round_trip_of_the_parameter_views():
    """What EspTrainNet.state_dict() is built from, without a device: the trained tensors laid out by the table and read back
    as views give a state dict check_state_dict takes, equal to the one that went in."""
    C = 8
    sd = espnet_weights(C, 105)
    names, table, spec = E.trained_param_names(C), E.train_table(C), E.espnet_spec(C)
    flat = torch.zeros(sum(n for _, n, _ in table))
    for (off, n, _), k in zip(table, names):
        flat[off:off + n] = sd[k].reshape(-1)
    back = type(sd)((k, flat[table[names.index(k)][0]:][:sd[k].numel()].view(spec[k]) if k in names else v) for k, v in sd.items())
    assert E.check_state_dict(back) == C
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)


def test_train_net_needs_a_device():
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        E.EspTrainNet(espnet_weights(8, 102), 'cpu')
    assert E.EspTrainNet is __import__('trackmpnn_amd').EspTrainNet


def test_eval_net_still_refuses_training():
    with pytest.raises(NotImplementedError):
        E.EspEmbedNet.train(object.__new__(E.EspEmbedNet), True)
