"""The backward of a call follows the route its forward took (functional.CallRoute inside SavedCall): switches that change
between a call's forward and its backward do not reach it.  A C2-shaped step (the shape and the NaN-filled gate tensor
of tests/test_zs_recompute_gpu.py) run twice, the second time with FUSED_BWD and ZERO_STATE_BWD switched off after the
last forward: the forward left the zero-state rows' hn plane, state rows and gate slots unwritten, so anything but the
routed zero-state backward would read NaN."""
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


def _step(monkeypatch, plans, xs, switch_off_before_backward):
    """forward_graph over every call + one backward: (loss, outputs, last h, grads, entry points in launch order)."""
    import trackmpnn_amd.functional as F
    from trackmpnn_amd import TrackMPNN, _lib
    from trackmpnn_amd.loss import bce_with_logits_sum
    names = []
    real_call, real_empty = _lib.call, torch.empty

    def spy(name, *args):
        names.append(name)
        return real_call(name, *args)

    def empty(*a, **k):      # the gate tensor [G, 4, N, H] starts as NaN: slots no kernel writes must not be read either
        t = real_empty(*a, **k)
        if t.dim() == 4 and t.shape[1] == 4 and t.shape[3] == H and t.is_floating_point():
            t.fill_(float('nan'))
        return t

    with monkeypatch.context() as m:
        m.setattr(_lib, 'call', spy)
        m.setattr(torch, 'empty', empty)
        torch.manual_seed(5)
        model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).train()
        h, loss, outs = None, 0.0, []
        for plan, x in zip(plans, xs):
            s, l, h, _ = model.forward_graph(x, h, plan)
            t = (torch.arange(l.numel(), device=DEV) % 3 == 0).float().view_as(l)
            loss = loss + bce_with_logits_sum(l, t)
            outs += [s.detach().clone(), l.detach().clone()]
        if switch_off_before_backward:
            m.setattr(F, 'FUSED_BWD', False)
            m.setattr(F, 'ZERO_STATE_BWD', False)
        loss.backward()
        torch.cuda.synchronize()
    grads = [p.grad.clone() for p in model.parameters()]
    return loss.detach().clone(), outs, h.detach().clone(), grads, names


def test_backward_follows_the_forwards_route(monkeypatch):
    plans, xs = _c2_batch(B=4, seed=3)
    l0, o0, h0, g0, n0 = _step(monkeypatch, plans, xs, False)
    l1, o1, h1, g1, n1 = _step(monkeypatch, plans, xs, True)
    assert torch.equal(l0, l1) and bool(torch.isfinite(l1))
    assert len(o0) == len(o1) and all(torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(o0, o1))
    assert torch.equal(h0, h1) and bool(torch.isfinite(h1).all())
    assert len(g0) == len(g1) and all(torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(g0, g1))
    assert n0 == n1
    assert 'tmpnn_gru_bwd_fused_zero_state' in n1 and 'tmpnn_gru_fwd_tiles_zero_state' in n1
    assert 'tmpnn_gru_bwd_data' not in n1 and 'tmpnn_gru_bwd_weights' not in n1
