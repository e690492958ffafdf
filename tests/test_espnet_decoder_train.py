"""Training the embedding CNN's whole decoder (EspTrainNet(scope='decoder')), the parts that need no GPU: the 36-row table against
decoder_param_names and espnet_spec, its arena offsets against pack_arena, the sizes and the argument checks."""
import numpy as np
import pytest

from tests.espnet_cases import espnet_weights
from trackmpnn_amd import _lib
from trackmpnn_amd import espnet as E


@pytest.fixture(scope='module')
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize('C', [1, 8, 128, 1024])
def test_table_lists_the_decoder_in_state_dict_order(lib, C):
    table = E.train_table(C, 'decoder')
    names = E.trained_param_names(C, 'decoder')
    spec = E.espnet_spec(C)
    assert names == E.decoder_param_names(C) and len(table) == len(names) == 36
    at = 0
    for (off, n, arena_off), k in zip(table, names):
        assert off == at and n == int(np.prod(spec[k])), k              # one flat buffer, no padding: GradBucket's layout
        assert 0 <= arena_off and arena_off + n <= lib.tmpnn_espnet_arena_floats(C) and arena_off % 4 == 0, k
        at += n
    assert lib.tmpnn_espnet_dec_param_floats(C) == at
    if C in (8, 128):
        assert at == {8: 130192, 128: 190432}[C]
    # a short `rows` is filled as far as it goes
    rows = np.full((4, 3), -7, np.int64)
    assert lib.tmpnn_espnet_dec_table(C, rows.ctypes.data, 3) == 36
    assert [tuple(r) for r in rows[:3]] == table[:3] and tuple(rows[3]) == (-7, -7, -7)


def test_the_tail_scope_is_the_default_and_the_decoders_last_rows(lib):
    C = 8
    assert E.trained_param_names(C) == E.trained_param_names(C, 'tail') and E.train_table(C) == E.train_table(C, 'tail')
    tail, dec = E.train_table(C, 'tail'), E.train_table(C, 'decoder')
    shift = dec[-9][0]
    assert E.trained_param_names(C, 'decoder')[-9:] == E.trained_param_names(C, 'tail')
    assert [(o - shift, n, a) for o, n, a in dec[-9:]] == tail
    assert E.trained_norm_names(C, 'tail') == ('act_l3.bn', 'project_l2.bn')
    assert E.trained_norm_names(C, 'decoder') == ('proj_L4_C.bn', 'pspMod.0.proj_1x1.bn', 'pspMod.0.conv_1x1_exp.bn',
                                                  'pspMod.0.br_after_cat.bn', 'pspMod.1.project.bn', 'act_l3.bn', 'project_l2.bn')


@pytest.mark.parametrize('C', [8, 128])
def test_table_matches_the_packed_arena(lib, C):
    """Every row's arena offset points at the segment pack_arena fills from that tensor: conv weights in the packed layout (grouped
    ones included), depthwise weights as they lie, bn.weight at the folded scale, bn.bias at the folded shift, slopes as they lie."""
    sd = espnet_weights(C, 102)
    arena = E.pack_arena(sd, C)
    seen = set()
    for (_, n, arena_off), k in zip(E.train_table(C, 'decoder'), E.decoder_param_names(C)):
        seg = arena[arena_off:arena_off + n]
        v = sd[k].numpy()
        assert not seen & set(range(arena_off, arena_off + n)), k       # no two tensors share a float of the arena
        seen |= set(range(arena_off, arena_off + n))
        if k.endswith('conv.weight') and v.shape[2:] == (1, 1):
            assert np.array_equal(seg, v[:, :, 0, 0].T.ravel()), k       # [cin / groups][cout]
        elif k.endswith('conv.weight'):
            assert v.shape[1:] == (1, 3, 3) and np.array_equal(seg, v.ravel()), k
        elif k.endswith('act.weight') or k.endswith('module_act.weight'):
            assert np.array_equal(seg, v), k
        else:                                                           # bn.weight -> scale, bn.bias -> shift
            assert k.endswith(('bn.weight', 'bn.bias')), k
            p = k[:-len('.weight')] if k.endswith('.weight') else k[:-len('.bias')]
            scale, shift = E.fold_bn(*(sd[f'{p}.{s}'] for s in ('weight', 'bias', 'running_mean', 'running_var')))
            assert np.array_equal(seg, scale if k.endswith('.weight') else shift), k
    # the four depthwise tensors of the EESP lie behind one another, as k_esp_dw reads them: [4][n][9]
    rows = dict(zip(E.decoder_param_names(C), E.train_table(C, 'decoder')))
    d = [rows[f'pspMod.0.spp_dw.{i}.conv.weight'] for i in range(4)]
    assert all(d[i + 1][0] == d[i][0] + 288 and d[i + 1][2] == d[i][2] + 288 for i in range(3))


@pytest.mark.parametrize('C', [8, 128])
def test_workspaces_hold_at_least_the_tail_scopes(lib, C):
    for T, H, W in ((1, 16, 16), (2, 32, 64), (3, 48, 80)):
        P8, P16 = (H // 8) * (W // 8), (H // 16) * (W // 16)
        pooled, h, w = 0, H // 8, W // 8
        for _ in range(4):
            h, w = (h + 1) // 2, (w + 1) // 2
            pooled += h * w
        kept = 4 * T * (128 * P16 + (32 + 128 + 128) * P8 + 128 * pooled)
        assert lib.tmpnn_espnet_dec_ws_bytes(T, H, W, C) >= lib.tmpnn_espnet_train_ws_bytes(T, H, W, C) + kept
        assert lib.tmpnn_espnet_dec_bwd_ws_bytes(T, H, W, C) >= lib.tmpnn_espnet_train_bwd_ws_bytes(T, H, W, C) + 4 * T * (
            (128 + 640 + 128 + 128 + 32 + 128) * P8 + 128 * P16)


def test_refused_shapes_and_arguments(lib):
    assert lib.tmpnn_espnet_dec_param_floats(0) == 0 and lib.tmpnn_espnet_dec_param_floats(1025) == 0
    for f in (lib.tmpnn_espnet_dec_ws_bytes, lib.tmpnn_espnet_dec_bwd_ws_bytes):
        assert f(0, 32, 32, 8) == 0 and f(1, 30, 32, 8) == 0 and f(1, 32, 32, 0) == 0 and f(1, 32768, 32768, 8) == 0
        assert f(1, 16, 16, 8) > 0
    assert lib.tmpnn_espnet_dec_table(0, None, 0) == -1 and b'espnet_dec_table' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_dec_table(8, None, 4) == -1
    assert lib.tmpnn_espnet_dec_refold(None, 8, None, None, None) == -1 and b'espnet_dec_refold: null' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_dec_refold(16, 0, 16, 16, None) == -1
    assert lib.tmpnn_espnet_dec_fwd(None, 8, None, 1, 16, 16, None, 0, None, None) == -1
    assert b'espnet_dec_fwd: null' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_dec_fwd(16, 8, 16, 1, 16, 24, 16, 0, 16, None) == -1 and b'multiples of 16' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_dec_fwd(16, 8, 16, 1, 16, 16, 16, 0, 16, None) == -3            # a short workspace, before any launch
    assert lib.tmpnn_espnet_dec_bwd(None, 8, None, None, 1, 16, 16, None, 0, None, None, 0, None, None, None, None, None, None) == -1
    big = 1 << 40
    for taps in ((16, None, None, None), (16, 16, None, None), (16, 16, 16, None), (None, None, None, 16)):
        assert lib.tmpnn_espnet_dec_bwd(16, 8, 16, 16, 1, 16, 16, 16, big, 16, 16, big, 16, *taps, None) == -1
        assert b'together' in lib.tmpnn_last_error()
    assert lib.tmpnn_espnet_dec_bwd(16, 8, 16, 16, 1, 16, 16, 16, 0, 16, 16, 0, 16, None, None, None, None, None) == -3
    assert lib.tmpnn_espnet_dec_bwd(16, 8, 16, 16, 1, 16, 16, 16, big, 16, 16, 0, 16, 16, 16, 16, 16, None) == -3


def test_scope_argument():
    sd = espnet_weights(8, 102)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        E.EspTrainNet(sd, 'cpu', scope='decoder')
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        E.EspTrainNet.from_state_dict(sd, 'cpu', scope='decoder')
    for call in (lambda: E.EspTrainNet(sd, 'cpu', scope='psp'), lambda: E.EspTrainNet.from_state_dict(sd, 'cuda:0', scope='all'),
                 lambda: E.trained_param_names(8, 'encoder'), lambda: E.train_table(8, None)):
        with pytest.raises(ValueError, match='scope'):
            call()
