"""The zero-state edge rows of a call without saved gate planes: the zero-state forward writes none and the zero-state
backward (tmpnn_gru_bwd_fused_zero_state, gate_plane = 0 + struct tmpnn_zs_gate_src) forms r, z, n again from the
projected det rows.  Everything is compared bit for bit (torch.equal) with the path that writes and reads the planes:
the kernel against itself reading the forward's planes, and the C2-shaped step against TMPNN_ZS_RECOMPUTE=0.

(At kernel level the recompute call takes no gate pointer at all, so there is no buffer left to poison; at step level
the gate tensor is still allocated and is filled with NaN before the forward touches it.)"""
import ctypes
from types import SimpleNamespace

import pytest
import torch

DEV = 'cuda:0'
H = 64
pytestmark = pytest.mark.gpu
ZS_FWD = 'tmpnn_gru_fwd_tiles_zero_state'
ZS_BWD = 'tmpnn_gru_bwd_fused_zero_state'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _case(R, seed):
    """R zero-state edge rows over Dn = 300 det rows (the state's first rows), built as tests/test_fwd_zero_state.py::_case
    builds them: tiles alternate between few dets and more than 24 distinct dets."""
    from trackmpnn_amd.graph import build_edge_tiles
    gen = torch.Generator().manual_seed(seed)
    Dn = 300
    N = Dn + R + 5
    e = torch.arange(R)
    few = (e // 32) % 2 == 0
    base = torch.randint(0, Dn - 8, (R,), generator=gen)
    src = torch.where(few, (e // 32) % (Dn - 8) + torch.randint(0, 8, (R,), generator=gen), base)
    dst = torch.where(few, (e // 32 + 3) % (Dn - 8) + torch.randint(0, 8, (R,), generator=gen),
                      torch.randint(0, Dn, (R,), generator=gen))
    rows = (Dn + torch.randperm(N - Dn, generator=gen)[:R]).sort().values
    g = SimpleNamespace(src_pos=src.to(torch.int32).to(DEV), dst_pos=dst.to(torch.int32).to(DEV),
                        edge_row=rows.to(torch.int32).to(DEV), E=R, Dn=Dn, device=torch.device(DEV))
    tiles = build_edge_tiles(g, 32, 4, 8, stats=True, order='rows')
    r32 = lambda *s: torch.randn(*s, generator=gen)         # noqa: E731
    h = r32(N, H)
    h[rows] = 0.0
    c = dict(proj=r32(Dn, 3 * H), h=h, b_ih=r32(3 * H), b_hh=r32(3 * H), w_head=r32(H), wih=0.3 * r32(3 * H, H),
             dout=r32(N, H), dy=r32(N), dmsg0=r32(N, H))
    c = {k: v.to(DEV) for k, v in c.items()}
    c.update(rows=g.edge_row, src_pos=g.src_pos, dst_pos=g.dst_pos)
    return c, tiles, N


def _planes(c, tiles, N, R):
    """The r, z, n planes the zero-state forward writes for the rows (the fourth plane is not written)."""
    from trackmpnn_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    h_out = torch.empty((N, H), device=DEV)
    gp = torch.full((4, N, H), float('nan'), device=DEV)
    _lib.call(ZS_FWD, tiles.cref(), R, c['proj'].data_ptr(), 3 * H, H, c['b_ih'].data_ptr(), c['b_hh'].data_ptr(),
              h_out.data_ptr(), H, gp.data_ptr(), N * H, 0, None, None, 0, st)
    torch.cuda.synchronize()
    return gp


def _gate_src(c, **over):
    from trackmpnn_amd import _lib
    f = dict(proj=c['proj'].data_ptr(), ld_proj=3 * H, src_pos=c['src_pos'].data_ptr(), dst_pos=c['dst_pos'].data_ptr(),
             b_ih=c['b_ih'].data_ptr(), b_hh=c['b_hh'].data_ptr())
    f.update(over)
    return _lib.CZsGateSrc(f['proj'], f['ld_proj'], f['src_pos'], f['dst_pos'], f['b_ih'], f['b_hh'])


def _bwd(c, N, R, up, gates, gate_plane, expect_rc=0):
    """d_msg, [dW_ih, db_ih, db_hh] of the zero-state backward; gates / gate_plane as given (planes, or 0 + a gate source)."""
    from trackmpnn_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.tmpnn_gru_bwd_fused_ws(R, H, H) // 4 + 1, device=DEV)
    dmsg = c['dmsg0'].clone()
    gW = [torch.full((3 * H, H), 0.5, device=DEV), torch.full((3 * H,), 1.0, device=DEV), torch.full((3 * H,), 2.0, device=DEV)]
    dho = c['dout'].data_ptr() if up & 1 else None
    dyp, whp = (c['dy'].data_ptr(), c['w_head'].data_ptr()) if up & 2 else (None, None)
    # (the det rows are the state's first Dn rows: a row's endpoints' state rows are its det positions)
    rc = lib.tmpnn_gru_bwd_fused_zero_state(
        c['rows'].data_ptr(), R, c['src_pos'].data_ptr(), c['dst_pos'].data_ptr(), H, c['h'].data_ptr(), H, H,
        c['wih'].data_ptr(), c['b_hh'].data_ptr() + 4 * 2 * H, gates, gate_plane, dho, H, dyp, whp, dmsg.data_ptr(), H,
        gW[0].data_ptr(), gW[1].data_ptr(), gW[2].data_ptr(), ws.data_ptr(), ws.numel() * 4, st)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, _lib.last_error())
    return dmsg, gW


@pytest.mark.parametrize('R', [1, 31, 32, 33, 2048, 2049, 4097])      # (2048 / 2049: 64 / 65 slabs, reduced directly / folded first)
def test_recomputed_gates_match_the_saved_planes(R):
    from trackmpnn_amd import _lib
    if not _lib.load().tmpnn_gru_bwd_fused_zero_state_available(H, H, 1):
        pytest.fail('tmpnn_gru_bwd_fused_zero_state is not available for H = IN = 64, xmode 1')
    c, tiles, N = _case(R, seed=R)
    if R > 64:
        assert tiles.max_dets > 24
    gp = _planes(c, tiles, N, R)
    for up in (1, 2, 3):
        m0, g0 = _bwd(c, N, R, up, gp.data_ptr(), N * H)
        src = _gate_src(c)
        m1, g1 = _bwd(c, N, R, up, ctypes.addressof(src), 0)
        m2, g2 = _bwd(c, N, R, up, ctypes.addressof(src), 0)
        tag = (R, up)
        assert bool(torch.isfinite(m0).all()), tag
        assert torch.equal(m0, m1), tag
        for name, a, b in zip(('dW_ih', 'db_ih', 'db_hh'), g0, g1):
            assert torch.equal(a, b), (tag, name)
        assert torch.equal(m1, m2) and all(torch.equal(a, b) for a, b in zip(g1, g2)), tag


def test_missing_or_misaligned_gate_source_is_refused():
    """gate_plane == 0 without a usable gate source: TMPNN_EINVAL on the host, nothing launched (the outputs keep their values)."""
    R = 33
    c, tiles, N = _case(R, seed=2)
    keep = [_gate_src(c, proj=None), _gate_src(c, src_pos=None), _gate_src(c, proj=c['proj'].data_ptr() + 4),
            _gate_src(c, ld_proj=3 * H - 1), _gate_src(c, b_hh=c['b_ih'].data_ptr())]       # (b_hn is not that b_hh + 2H)
    bad = [None] + [ctypes.addressof(s) for s in keep]
    for gates in bad:
        m, gW = _bwd(c, N, R, 3, gates, 0, expect_rc=-1)
        assert torch.equal(m, c['dmsg0'])
        assert bool((gW[0] == 0.5).all()) and bool((gW[1] == 1.0).all()) and bool((gW[2] == 2.0).all())


def _c2_batch(B, seed, extra_call=False):
    from trackmpnn_amd import WindowBuilder, batch_windows, synth_window
    from trackmpnn_amd.graph import plan_single
    wins = [WindowBuilder(synth_window(seed * 1000 + s, 7, 6, 20)).calls() for s in range(B)]
    plans, refs = batch_windows(wins, device='cpu')
    gen = torch.Generator().manual_seed(seed)
    xs = []
    for plan, ref in zip(plans, refs):
        x = torch.zeros(plan.n_new, 8)
        x[plan.new_det_local] = torch.randn(len(ref), 8, generator=gen)
        xs.append(x.to(DEV))
    plans = [p.to(DEV) for p in plans]
    if extra_call:          # one more iteration over the last graph: a call without new rows
        plans.append(plan_single(plans[-1].graph, 0))
        xs.append(torch.zeros(0, 8, device=DEV))
    return plans, xs


def _step(monkeypatch, plans, xs, rc, K=0, bwd_zs=True, poison=False, reserve=False, grad=True, nan_gates=False):
    """forward_graph over every call (+ one backward): (loss, outputs, last h, grads, [(entry point, args)])."""
    import trackmpnn_amd.functional as F
    from trackmpnn_amd import TrackMPNN, _lib
    from trackmpnn_amd.loss import bce_with_logits_sum
    monkeypatch.setattr(F, 'ZS_RECOMPUTE', rc)
    monkeypatch.setattr(F, 'ZERO_STATE_BWD', bwd_zs)
    calls = []
    real_call, real_empty = _lib.call, torch.empty

    def spy(name, *args):
        if name in (ZS_FWD, ZS_BWD):
            calls.append((name, args))
        return real_call(name, *args)

    def empty(*a, **k):      # the gate tensor [G, 4, N, H] starts as NaN: slots no kernel writes must not be read either
        t = real_empty(*a, **k)
        if t.dim() == 4 and t.shape[1] == 4 and t.shape[3] == H and t.is_floating_point():
            t.fill_(float('nan'))
        return t

    monkeypatch.setattr(_lib, 'call', spy)
    if nan_gates:
        monkeypatch.setattr(torch, 'empty', empty)
    torch.manual_seed(5)
    model = TrackMPNN('2d', 3, 64, K, 'diff').to(DEV).train(grad)
    h, loss, outs = None, 0.0, []
    with torch.set_grad_enabled(grad):
        for i, (plan, x) in enumerate(zip(plans, xs)):
            nxt = plans[i + 1].n_new if (reserve and i + 1 < len(plans)) else 0
            s, l, h, _ = model.forward_graph(x, h, plan, reserve_rows=nxt)
            if poison and nxt > 0:
                with torch.no_grad():
                    N = h.shape[0]
                    full = real_empty(0, device=DEV).set_(h.untyped_storage(), h.storage_offset(), (N + nxt, h.shape[1]))
                    full[N:] = float('nan')
            t = (torch.arange(l.numel(), device=DEV) % 3 == 0).float().view_as(l)
            loss = loss + bce_with_logits_sum(l, t)
            outs += [s.detach().clone(), l.detach().clone()]
        if grad:
            loss.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, 'call', real_call)
    monkeypatch.setattr(torch, 'empty', real_empty)
    grads = [p.grad.clone() for p in model.parameters()] if grad else []
    return loss.detach().clone(), outs, h.detach().clone(), grads, calls


def _assert_equal(a, b):
    (l0, o0, h0, g0, _), (l1, o1, h1, g1, _) = a, b
    assert torch.equal(l0, l1)
    assert len(o0) == len(o1) and all(torch.equal(x, y) for x, y in zip(o0, o1))
    assert torch.equal(h0, h1)
    assert len(g0) == len(g1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert bool(torch.isfinite(l1)) and all(bool(torch.isfinite(g).all()) for g in g1)


def _fwd_gates(calls):
    return [a[9] for n, a in calls if n == ZS_FWD]


def _bwd_planes(calls):
    return [a[11] for n, a in calls if n == ZS_BWD]


@pytest.fixture(scope='module')
def c2():
    return _c2_batch(B=24, seed=3)


def test_c2_step_is_bitwise_equal(monkeypatch, c2):
    plans, xs = c2
    off = _step(monkeypatch, plans, xs, rc=False)
    on = _step(monkeypatch, plans, xs, rc=True, nan_gates=True)
    _assert_equal(off, on)
    # switch off: planes written and read; on: the forward got no gate pointer, the backward gate_plane == 0
    assert _fwd_gates(off[4]) and all(p is not None for p in _fwd_gates(off[4])) and all(p != 0 for p in _bwd_planes(off[4]))
    assert _fwd_gates(on[4]) and all(p is None for p in _fwd_gates(on[4]))
    assert _bwd_planes(on[4]) and all(p == 0 for p in _bwd_planes(on[4]))
    assert len(_bwd_planes(on[4])) == len(_fwd_gates(on[4])) == len(_bwd_planes(off[4]))


def test_c2_step_with_poisoned_spare_rows(monkeypatch, c2):
    plans, xs = c2
    off = _step(monkeypatch, plans, xs, rc=False, reserve=True)
    on = _step(monkeypatch, plans, xs, rc=True, reserve=True, poison=True, nan_gates=True)
    _assert_equal(off, on)
    assert _bwd_planes(on[4]) and all(p == 0 for p in _bwd_planes(on[4]))


def test_full_backward_keeps_the_planes(monkeypatch, c2):
    """ZERO_STATE_BWD off with recompute requested: the forward writes r, z, n and hn for the full backward."""
    plans, xs = c2
    off = _step(monkeypatch, plans, xs, rc=False, bwd_zs=False)
    on = _step(monkeypatch, plans, xs, rc=True, bwd_zs=False, nan_gates=True)
    _assert_equal(off, on)
    assert not _bwd_planes(on[4])
    fw = [a for n, a in on[4] if n == ZS_FWD]
    assert fw and all(a[9] is not None and a[11] == 1 for a in fw)          # gates given, write_hn set


def test_attention_falls_back(monkeypatch):
    plans, xs = _c2_batch(B=8, seed=4)
    off = _step(monkeypatch, plans, xs, rc=False, K=2)
    on = _step(monkeypatch, plans, xs, rc=True, K=2)
    _assert_equal(off, on)
    assert not on[4]


def test_eval_outputs_are_equal(monkeypatch):
    plans, xs = _c2_batch(B=12, seed=7)
    off = _step(monkeypatch, plans, xs, rc=False, grad=False)
    on = _step(monkeypatch, plans, xs, rc=True, grad=False)
    _assert_equal(off, on)
    assert _fwd_gates(on[4]) and all(p is None for p in _fwd_gates(on[4])) and not _bwd_planes(on[4])


def test_a_call_without_new_rows(monkeypatch):
    plans, xs = _c2_batch(B=12, seed=8, extra_call=True)
    off = _step(monkeypatch, plans, xs, rc=False)
    on = _step(monkeypatch, plans, xs, rc=True, nan_gates=True)
    _assert_equal(off, on)
    # the calls with new rows take the zero-state pair, the last one (every row on the full kernels) does not
    assert _bwd_planes(on[4]) and all(p == 0 for p in _bwd_planes(on[4]))
    assert len(_bwd_planes(on[4])) == len(_fwd_gates(on[4])) == len(_fwd_gates(off[4]))
    ref = _step(monkeypatch, plans[:-1], xs[:-1], rc=True)
    assert len(_fwd_gates(ref[4])) == len(_fwd_gates(on[4]))
