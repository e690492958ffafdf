"""The edge cell's backward of a call's NEW edge rows (zero incoming state) on its own kernel
(tmpnn_gru_bwd_fused_zero_state): against the full one-pass kernel over the same rows, and end to end against
TMPNN_BWD_ZERO_STATE=0 on a C2-shaped window batch."""
import pytest
import torch

DEV = 'cuda:0'
H = 64
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _case(R, R_old, seed):
    """A cell over R scattered rows whose rows [R_old, R) have h = 0 (and so ghn = b_hn in the fourth gate plane)."""
    gen = torch.Generator().manual_seed(seed)
    N = 2 * R + 7
    perm = torch.randperm(N, generator=gen)
    rows = perm[:R].sort().values
    others = perm[R:]
    src = others[torch.randint(0, N - R, (R,), generator=gen)]
    dst = others[torch.randint(0, N - R, (R,), generator=gen)]
    r32 = lambda *s: torch.randn(*s, generator=gen)         # noqa: E731
    h = r32(N, H)
    h[rows[R_old:]] = 0.0
    b_hh = r32(3 * H)
    gates = torch.cat([torch.sigmoid(r32(2, N, H)), torch.tanh(r32(1, N, H)), r32(1, N, H)], 0)
    gates[3, rows[R_old:]] = b_hh[2 * H:]
    c = dict(rows=rows.to(torch.int32), src=src.to(torch.int32), dst=dst.to(torch.int32), h=h, gates=gates.contiguous(),
             dout=r32(N, H), dy=r32(N), w_head=r32(H), wih=0.3 * r32(3 * H, H), whh=0.3 * r32(3 * H, H), b_hh=b_hh,
             dmsg0=r32(N, H))
    return {k: v.to(DEV) for k, v in c.items()}, N


def _run(c, N, R, R_old, up, split):
    """dmsg, dh, [dW_ih, dW_hh, db_ih, db_hh] of the full kernel over all R rows (split=False) or of the full kernel over
    [0, R_old) plus the zero-state kernel over [R_old, R), as mp_backward dispatches them (row-F adjoint fused)."""
    from trackmpnn_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.tmpnn_gru_bwd_fused_ws(R, H, H) // 4 + 1, device=DEV)
    dmsg = c['dmsg0'].clone()
    dh = torch.full((N, H), 5.0, device=DEV)
    gW = [torch.full((3 * H, H), 0.5, device=DEV), torch.full((3 * H, H), 0.25, device=DEV),
          torch.full((3 * H,), 1.0, device=DEV), torch.full((3 * H,), 2.0, device=DEV)]
    dho = c['dout'].data_ptr() if up & 1 else None
    dyp, whp = (c['dy'].data_ptr(), c['w_head'].data_ptr()) if up & 2 else (None, None)
    rows, src, dst = c['rows'], c['src'], c['dst']
    R_full = R_old if split else R
    if R_full > 0:
        _lib.call('tmpnn_gru_bwd_fused', rows.data_ptr(), R_full, 1, src.data_ptr(), dst.data_ptr(), None, H, 1, H,
                  c['h'].data_ptr(), H, H, c['wih'].data_ptr(), c['whh'].data_ptr(), c['gates'].data_ptr(), N * H, dho, H,
                  dyp, whp, dmsg.data_ptr(), H, dh.data_ptr(), H, src.data_ptr(), dst.data_ptr(), dmsg.data_ptr(), H,
                  gW[0].data_ptr(), gW[1].data_ptr(), gW[2].data_ptr(), gW[3].data_ptr(), ws.data_ptr(), ws.numel() * 4, st)
    if split:
        _lib.call('tmpnn_gru_bwd_fused_zero_state', rows.data_ptr() + 4 * R_old, R - R_old, src.data_ptr() + 4 * R_old,
                  dst.data_ptr() + 4 * R_old, H, c['h'].data_ptr(), H, H, c['wih'].data_ptr(),
                  c['b_hh'].data_ptr() + 4 * 2 * H, c['gates'].data_ptr(), N * H, dho, H, dyp, whp, dmsg.data_ptr(), H,
                  gW[0].data_ptr(), gW[2].data_ptr(), gW[3].data_ptr(), ws.data_ptr(), ws.numel() * 4, st)
    torch.cuda.synchronize()
    return dmsg, dh, gW


@pytest.mark.parametrize('R,R_old', [(1, 0), (31, 0), (32, 0), (33, 17), (100, 37), (255, 224), (4097, 1000),
                                     (8191 + 32 * 300, 5003),
                                     (2048, 0), (2049, 0)])      # the zero-state kernel's 64 / 65 slabs: reduced directly / folded first
def test_zero_state_split_matches_the_full_kernel(R, R_old):
    from trackmpnn_amd import _lib
    if not _lib.load().tmpnn_gru_bwd_fused_zero_state_available(H, H, 1):
        pytest.fail('tmpnn_gru_bwd_fused_zero_state is not available for H = IN = 64, xmode 1')
    c, N = _case(R, R_old, seed=R + R_old)
    rows = c['rows'].long()
    old = rows[:R_old]
    for up in (1, 2, 3):
        m0, h0, g0 = _run(c, N, R, R_old, up, split=False)
        m1, h1, g1 = _run(c, N, R, R_old, up, split=True)
        m2, h2, g2 = _run(c, N, R, R_old, up, split=True)
        tag = (R, R_old, up)
        # two runs of the split path: bitwise identical
        assert torch.equal(m1, m2) and torch.equal(h1, h2) and all(torch.equal(a, b) for a, b in zip(g1, g2)), tag
        # d_msg over every row (untouched outside `rows`), d_h over the old rows; the new rows' d_h is not formed
        assert (m0 - m1).abs().max().item() <= 1e-6 * max(1.0, m0.abs().max().item()), tag
        assert torch.equal(h0[old], h1[old]), tag
        for name, a, b in zip(('dW_ih', 'dW_hh', 'db_ih', 'db_hh'), g0, g1):
            assert (a - b).abs().max().item() <= 1e-6 * max(1.0, a.abs().max().item()), (tag, name)


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


def test_c2_step_matches_the_full_kernel_backward(monkeypatch):
    """forward_graph over the calls of a C2-shaped window batch + one backward: the same loss, and gradients within
    1e-6 of the largest, with the zero-state kernel on the new edge rows as with every row on the full kernel."""
    import trackmpnn_amd.functional as F
    from trackmpnn_amd import TrackMPNN, _lib
    from trackmpnn_amd.loss import bce_with_logits_sum
    plans, xs = _c2_batch(B=24, seed=3)
    calls = []
    real_call = _lib.call

    def spy(name, *args):
        calls.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(_lib, 'call', spy)
    outs = []
    for zs in (False, True, True):
        monkeypatch.setattr(F, 'ZERO_STATE_BWD', zs)
        calls.clear()
        torch.manual_seed(5)
        model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).train()
        h, loss = None, 0.0
        for plan, x in zip(plans, xs):
            s, l, h, _ = model.forward_graph(x, h, plan)
            t = (torch.arange(l.numel(), device=DEV) % 3 == 0).float().view_as(l)
            loss = loss + bce_with_logits_sum(l, t)
        loss.backward()
        torch.cuda.synchronize()
        assert ('tmpnn_gru_bwd_fused_zero_state' in calls) == zs
        outs.append((loss.detach().clone(), [p.grad.clone() for p in model.parameters()]))
    (l0, g0), (l1, g1), (l2, g2) = outs
    assert torch.equal(l0, l1)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    gmax = max(g.abs().max().item() for g in g0)
    for a, b in zip(g0, g1):
        assert (a - b).abs().max().item() <= 1e-6 * gmax
