"""The tiled edge forward of a call's NEW edge rows (zero incoming state) on its state-free kernel
(tmpnn_gru_fwd_tiles_zero_state): bit for bit against the full tiled kernel over the same rows, and end to end against
TMPNN_FWD_ZERO_STATE=0 on a C2-shaped window batch."""
from types import SimpleNamespace

import pytest
import torch

DEV = 'cuda:0'
H = 64
SENTINEL = 7.0
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _case(R, seed):
    """R edge rows of zero state over Dn det rows; the tiles alternate between few dets (staged in LDS) and more than TCAP
    = 24 distinct dets (the gather path)."""
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
    h = torch.randn(N, H, generator=gen)
    h[rows] = 0.0
    c = dict(proj=torch.randn(Dn, 3 * H, generator=gen), h=h, whh_t=0.3 * torch.randn(H, 3 * H, generator=gen),
             b_ih=torch.randn(3 * H, generator=gen), b_hh=torch.randn(3 * H, generator=gen),
             w_head=torch.randn(H, generator=gen))
    return {k: v.to(DEV) for k, v in c.items()}, tiles, N, rows.to(DEV)


def _run(c, tiles, N, R, zs, gates, write_hn=0):
    from trackmpnn_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    h_out = torch.full((N, H), SENTINEL, device=DEV)
    gp = torch.full((4, N, H), SENTINEL, device=DEV) if gates else None
    parts = torch.full((2, N), SENTINEL, device=DEV)
    if zs:
        _lib.call('tmpnn_gru_fwd_tiles_zero_state', tiles.cref(), R, c['proj'].data_ptr(), 3 * H, H, c['b_ih'].data_ptr(),
                  c['b_hh'].data_ptr(), h_out.data_ptr(), H, _lib.ptr(gp), N * H, write_hn, c['w_head'].data_ptr(),
                  parts.data_ptr(), N, st)
    else:
        _lib.call('tmpnn_gru_fwd_tiles', tiles.cref(), R, c['proj'].data_ptr(), 3 * H, c['h'].data_ptr(), H, H,
                  c['whh_t'].data_ptr(), c['b_ih'].data_ptr(), c['b_hh'].data_ptr(), h_out.data_ptr(), H, _lib.ptr(gp),
                  N * H, c['w_head'].data_ptr(), parts.data_ptr(), N, st)
    torch.cuda.synchronize()
    return h_out, gp, parts


@pytest.mark.parametrize('R', [1, 31, 32, 33, 4097])
def test_zero_state_kernel_matches_the_full_kernel(R):
    from trackmpnn_amd import _lib
    if not _lib.load().tmpnn_gru_fwd_tiles_zero_state_available(H, 3):
        pytest.fail('tmpnn_gru_fwd_tiles_zero_state is not available for H = 64')
    c, tiles, N, rows = _case(R, seed=R)
    if R > 64:
        assert tiles.max_dets > 24                 # (the gather path of big tiles is exercised)
    o0, g0, p0 = _run(c, tiles, N, R, zs=False, gates=True)
    o1, g1, p1 = _run(c, tiles, N, R, zs=True, gates=True)
    assert torch.equal(o0, o1) and torch.equal(p0, p1)
    assert torch.equal(g0[:3], g1[:3])
    assert bool((g1[3] == SENTINEL).all())          # hn plane untouched without write_hn
    o2, g2, p2 = _run(c, tiles, N, R, zs=True, gates=True, write_hn=1)
    assert torch.equal(o0, o2) and torch.equal(p0, p2) and torch.equal(g0, g2)
    assert torch.equal(g2[3][rows], c['b_hh'][2 * H:].expand(R, H))
    o3, _, p3 = _run(c, tiles, N, R, zs=True, gates=False)
    assert torch.equal(o0, o3) and torch.equal(p0, p3)
    other = torch.ones(N, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert bool((o3[other] == SENTINEL).all()) and bool((p3[:, other] == SENTINEL).all())


def _c2_batch(B, seed):
    from trackmpnn_amd import WindowBuilder, batch_windows, synth_window
    wins = [WindowBuilder(synth_window(seed * 1000 + s, 7, 6, 20)).calls() for s in range(B)]
    plans, refs = batch_windows(wins, device='cpu')
    gen = torch.Generator().manual_seed(seed)
    xs = []
    for plan, ref in zip(plans, refs):
        x = torch.zeros(plan.n_new, 8)
        x[plan.new_det_local] = torch.randn(len(ref), 8, generator=gen)
        xs.append(x.to(DEV))
    return [p.to(DEV) for p in plans], xs


def _step(monkeypatch, plans, xs, fwd_zs, K=0, bwd_zs=True, poison=False, reserve=False, grad=True):
    """forward_graph over every call (+ one backward): (loss, scores, logits, last h, grads, entry points called)."""
    import trackmpnn_amd.functional as F
    from trackmpnn_amd import TrackMPNN, _lib
    from trackmpnn_amd.loss import bce_with_logits_sum
    monkeypatch.setattr(F, 'ZERO_STATE_FWD', fwd_zs)
    monkeypatch.setattr(F, 'ZERO_STATE_BWD', bwd_zs)
    calls = set()
    real_call = _lib.call

    def spy(name, *args):
        calls.add(name)
        return real_call(name, *args)

    monkeypatch.setattr(_lib, 'call', spy)
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
                    full = torch.empty(0, device=DEV).set_(h.untyped_storage(), h.storage_offset(), (N + nxt, h.shape[1]))
                    full[N:] = float('nan')
            t = (torch.arange(l.numel(), device=DEV) % 3 == 0).float().view_as(l)
            loss = loss + bce_with_logits_sum(l, t)
            outs += [s.detach().clone(), l.detach().clone()]
        if grad:
            loss.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, 'call', real_call)
    grads = [p.grad.clone() for p in model.parameters()] if grad else []
    return loss.detach().clone(), outs, h.detach().clone(), grads, calls


def _assert_equal(a, b):
    (l0, o0, h0, g0, _), (l1, o1, h1, g1, _) = a, b
    assert torch.equal(l0, l1)
    assert len(o0) == len(o1) and all(torch.equal(x, y) for x, y in zip(o0, o1))
    assert torch.equal(h0, h1)
    assert len(g0) == len(g1) and all(torch.equal(x, y) for x, y in zip(g0, g1))


ZS_FWD = 'tmpnn_gru_fwd_tiles_zero_state'
ZS_BWD = 'tmpnn_gru_bwd_fused_zero_state'


def test_c2_step_is_bitwise_equal(monkeypatch):
    plans, xs = _c2_batch(B=24, seed=3)
    off = _step(monkeypatch, plans, xs, fwd_zs=False)
    on = _step(monkeypatch, plans, xs, fwd_zs=True)
    assert ZS_FWD not in off[4] and ZS_FWD in on[4] and ZS_BWD in on[4]
    _assert_equal(off, on)
    # the zero-state backward off: the forward writes the hn plane (and zero-fills) for the full backward
    off = _step(monkeypatch, plans, xs, fwd_zs=False, bwd_zs=False)
    on = _step(monkeypatch, plans, xs, fwd_zs=True, bwd_zs=False)
    assert ZS_FWD in on[4] and ZS_BWD not in on[4]
    _assert_equal(off, on)


def test_c2_step_with_attention_falls_back(monkeypatch):
    plans, xs = _c2_batch(B=8, seed=4)
    off = _step(monkeypatch, plans, xs, fwd_zs=False, K=2)
    on = _step(monkeypatch, plans, xs, fwd_zs=True, K=2)
    assert ZS_FWD not in on[4]
    _assert_equal(off, on)


def test_poisoned_spare_rows_are_not_read(monkeypatch):
    """reserve_rows: a call's new rows are the previous h_out's spare storage; NaN there must not reach anything."""
    plans, xs = _c2_batch(B=24, seed=6)
    ref = _step(monkeypatch, plans, xs, fwd_zs=False, reserve=True)
    on = _step(monkeypatch, plans, xs, fwd_zs=True, reserve=True, poison=True)
    assert ZS_FWD in on[4]
    _assert_equal(ref, on)
    assert torch.isfinite(on[0]) and all(bool(torch.isfinite(g).all()) for g in on[3])


def test_eval_outputs_are_equal(monkeypatch):
    plans, xs = _c2_batch(B=12, seed=7)
    off = _step(monkeypatch, plans, xs, fwd_zs=False, grad=False)
    on = _step(monkeypatch, plans, xs, fwd_zs=True, grad=False)
    assert ZS_FWD in on[4]
    _assert_equal(off, on)
