"""plan_route: the kernels of a message-passing call, decided once from the plan's host-side fields, the module's switches
and what the library says it can run.  No launch, no GPU: CPU plans and a stub that answers as the gfx950 library does
(trackmpnn_amd/csrc: gru_fwd.hip, gru_bwd.hip, wide.hip, intf.hip)."""
import dataclasses
from types import SimpleNamespace

import pytest
import torch

import trackmpnn_amd.functional as F
from trackmpnn_amd import TrackMPNN, WindowBuilder, batch_windows, synth_window
from trackmpnn_amd.graph import plan_single


def _head_parts(H, IN, xmode):
    if H not in (32, 64):
        return 0
    shm = 4 * (((0 if xmode == 3 else IN) + H) * 3 * H + (12 if H == 64 else 8) * 32 * 36 + 4)
    return 0 if shm > 160 * 1024 else H // 32


def _caps(**over):
    c = dict(
        tmpnn_gru_fwd_tiles_zero_state_available=lambda H, xmode: int(H in (32, 64) and xmode == 3),
        tmpnn_gru_bwd_fused_available=lambda H, IN, xmode: int(H == 64 and ((IN == 64 and xmode in (0, 1))
                                                                            or (IN == 128 and xmode == 2))),
        tmpnn_gru_bwd_fused_zero_state_available=lambda H, IN, xmode: int(H == 64 and IN == 64 and xmode == 1),
        tmpnn_wide_supported=lambda H, IN: int(128 <= H <= 1024 and H % 128 == 0 and IN == H),
        tmpnn_gru_fwd_head_parts=_head_parts,
        tmpnn_input_tf_supported=lambda H, F_, m: int(H in (32, 64) and 0 < F_ <= 128 and 0 <= m <= 128))
    c.update(over)
    return SimpleNamespace(**c)


@pytest.fixture(scope='module')
def plans():
    """Two windows of synth_window(seed, 7, 6, 20) as one batch, + one more iteration over the last graph (no new rows)."""
    wins = [WindowBuilder(synth_window(3000 + s, 7, 6, 20)).calls() for s in range(2)]
    ps, _ = batch_windows(wins, device='cpu')
    return ps + [plan_single(ps[-1].graph, 0)]


def _routes(plans, H=64, K=0, msg='diff', save=True, caps=None, P=None):
    model = TrackMPNN('2d', 3, H, K, msg)
    if P is None:
        P = dict(zip(model.spec.param_names(), model._params_and_buffers()[0]))
    return model.spec, [F.plan_route(model.spec, p, P, save, caps or _caps()) for p in plans]


def test_default_model_takes_the_zero_state_pair(plans):
    spec, routes = _routes(plans)
    for i, (p, r) in enumerate(zip(plans, routes)):
        new_edges = p.n_new - int(p.new_det_row.numel())
        assert r.n == p.n_new and r.E_old == p.graph.E - new_edges
        assert r.bwd_fused and r.edge_bwd == 'fused' and r.gather_bwd
        assert r.cw == 2 and not r.recompute_gates and not r.dense_plan and not r.win_plan
        if p.graph.E > 0:
            assert r.edge_fwd == 'proj_tiled' and r.tile_rows == 32
        zs = new_edges > 0
        assert (r.zs_fwd, r.zs_bwd, r.zs_rc, r.zs_groups) == (zs, zs, zs, (zs,)), i
        assert r.new_rows_unread == zs
        assert r.tf == ((True,) if p.n_new > 0 else (False,)) and r.tf_all == (int(p.new_det_row.numel()) > 0)
    assert routes[0].E_old == 0                              # the first call: every row is new
    first = next(r for p, r in zip(plans, routes) if p.graph.E > 0)
    assert first.E_old == 0 and first.zs_fwd                 # the first call with edges: every edge row is new
    assert any(r.zs_fwd and r.E_old > 0 for r in routes)     # later calls: a full part and a zero-state part
    last = routes[-1]
    assert last.n == 0 and last.E_old == plans[-1].graph.E
    assert not (last.zs_fwd or last.zs_bwd or last.zs_rc or any(last.zs_groups))


def test_without_a_backward(plans):
    _, routes = _routes(plans, save=False)
    for p, r in zip(plans, routes):
        assert not r.bwd_fused and not r.zs_bwd and not r.zs_rc and r.edge_bwd == ''
        assert r.new_rows_unread == r.zs_fwd
    assert any(r.zs_fwd for r in routes)


def test_attention_heads(plans):
    spec, routes = _routes(plans, K=2)
    assert spec.K == 2
    for r in routes:
        assert r.agg == 'attention'
        assert not (r.zs_fwd or r.zs_bwd or r.zs_rc or any(r.zs_groups) or r.new_rows_unread)
        assert r.bwd_fused and r.edge_bwd == 'fused' and r.gather_bwd
    assert all(r.agg == 'segsum' for r in _routes(plans)[1])


def test_concat_message(plans):
    spec, routes = _routes(plans, msg='concat')
    assert spec.IN_e == 128
    for p, r in zip(plans, routes):
        if p.graph.E > 0:
            assert r.edge_fwd == 'concat_proj' and r.cw == 2
        assert not (r.zs_fwd or r.zs_bwd or r.zs_rc) and r.bwd_fused


@pytest.mark.parametrize('H', [128, 256])
def test_wide_cells(plans, H):
    for K in (0, 2):
        _, routes = _routes(plans, H=H, K=K)
        for p, r in zip(plans, routes):
            if p.graph.E == 0:
                continue
            assert r.edge_fwd == 'wide_tiled' and r.wide and r.cw == 0 and not r.bwd_fused
            assert r.edge_bwd == ('wide_det_fused' if K == 0 else 'wide_det') and not r.gather_bwd
            assert r.dense_plan == (H % 256 == 0 and K == 0)
            assert not (r.zs_fwd or r.zs_bwd or r.zs_rc) and r.tf == (False,)


def _diff(a, b):
    return {k for k in dataclasses.asdict(a) if getattr(a, k) != getattr(b, k)}


def test_each_switch_changes_its_own_fields(plans, monkeypatch):
    _, base = _routes(plans)
    i = next(i for i, r in enumerate(base) if r.zs_fwd and r.E_old > 0)
    p, b = [plans[i]], base[i]

    def route(**sw):
        with monkeypatch.context() as m:
            for k, v in sw.items():
                m.setattr(F, k, v)
            return _routes(p)[1][0]

    r = route(ZERO_STATE_FWD=False)         # the zero-state backward runs on the planes the full forward saved
    assert _diff(b, r) == {'zs_fwd', 'zs_rc'} and r.zs_bwd and r.zs_groups == (True,) and not r.new_rows_unread
    r = route(ZERO_STATE_BWD=False)
    assert _diff(b, r) == {'zs_bwd', 'zs_groups', 'zs_rc'} and r.zs_fwd and not r.new_rows_unread
    r = route(ZS_RECOMPUTE=False)
    assert _diff(b, r) == {'zs_rc'} and r.new_rows_unread
    r = route(FUSED_BWD=False)
    assert _diff(b, r) == {'bwd_fused', 'edge_bwd', 'zs_bwd', 'zs_groups', 'zs_rc'}
    assert r.edge_bwd == 'generic' and r.zs_fwd and not r.zs_bwd and not r.new_rows_unread
    r = route(ZERO_STATE_FWD=False, ZERO_STATE_BWD=False)
    assert _diff(b, r) == {'zs_fwd', 'zs_bwd', 'zs_groups', 'zs_rc'}
    assert _routes(p)[1][0] == b            # the switches are read at call time: back to the defaults


def test_library_without_the_zero_state_backward(plans):
    _, base = _routes(plans)
    _, routes = _routes(plans, caps=_caps(tmpnn_gru_bwd_fused_zero_state_available=lambda H, IN, xmode: 0))
    for b, r in zip(base, routes):
        assert r.zs_fwd == b.zs_fwd and not r.zs_bwd and not r.zs_rc and not any(r.zs_groups)
        assert not r.new_rows_unread        # the forward zero-fills the rows' state and writes their hn plane
        assert r.bwd_fused
    _, routes = _routes(plans, caps=_caps(tmpnn_gru_fwd_tiles_zero_state_available=lambda H, xmode: 0))
    assert not any(r.zs_fwd or r.zs_rc for r in routes) and any(r.zs_bwd for r in routes)


def test_misaligned_b_hn(plans):
    model = TrackMPNN('2d', 3, 64, 0, 'diff')
    P = dict(zip(model.spec.param_names(), model._params_and_buffers()[0]))
    name = 'factor_grus.0.edge_gru.bias_hh'
    P[name] = torch.zeros(3 * 64 + 1)[1:]
    assert (P[name].data_ptr() + 4 * 2 * 64) % 16 != 0
    _, routes = _routes(plans, P=P)
    assert not any(r.zs_fwd or r.zs_bwd or r.zs_rc or any(r.zs_groups) for r in routes)
