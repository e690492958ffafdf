"""Batch-1 routes on the device (-m gpu): every mode of a call takes the route plan_small_route names for it (the model keeps
the route of its last call), and all routes of one width compute the same bits -- they launch the same kernels on the same
inputs (tests/test_small_path_gpu.py::test_fused_iteration_is_bitwise_reproducible_and_sync_free)."""
import pytest
import torch

from tests.golden_util import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTHS = {'h64': (64, 0), 'h48': (48, 0), 'h64k2': (64, 2)}
MODES = ('no_grad', 'default', 'bucket', 'frozen', 'masked', 'masked_no_grad')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope='module')
def window():
    """The two calls of the c1_static_diff_k0_train window (5 frames x 20 dets) as the reference hands them over."""
    gold = Golden('c1_static_diff_k0_train')
    calls = [(gold.t(f'c{c}/x').to(DEV), gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV))
             for c in range(gold.ncalls)]
    assert len(calls) == 2
    return gold.meta, calls


def _model(meta, key):
    from trackmpnn_amd import TrackMPNN
    H, K = WIDTHS[key]
    torch.manual_seed(5)
    model = TrackMPNN(meta['features'], meta['ncategories'], H, K, meta['msg_type']).to(DEV).train()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(DEV))
    return model


def _run(meta, calls, key, mode, monkeypatch):
    """(per call: scores, logits, h_out ; parameter gradients | None) of the window in one mode, the route of every call held
    against plan_small_route of the facts of that call."""
    import trackmpnn_amd.track_mpnn as tm
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.small import fast_module, plan_small_route
    model = _model(meta, key)
    if mode == 'bucket':
        GradBucket(model)
    if mode == 'frozen':
        for p in model.parameters():
            p.requires_grad_(False)
    native = fast_module() is not None
    assert native, 'the native node is part of the build'
    outs, routes, h, loss = [], [], None, 0.0
    with monkeypatch.context() as mp, torch.set_grad_enabled(not mode.endswith('no_grad')):
        if mode.startswith('masked'):
            mp.setattr(tm, 'fast_module', lambda: None)       # (the one place forward_dgraph asks for the native node)
            native = False
        for x, na, ea in calls:
            grad_on = torch.is_grad_enabled()
            h_grad = grad_on and h is not None and h.requires_grad
            trainable = [p.requires_grad for p in model.parameters()]
            s, l, h, _ = model(x, h, na, ea)
            graph = model._graph_cache[3]
            assert graph.N == int(na.shape[0])
            want = plan_small_route(True, WIDTHS[key][1] > 0, key == 'h48', graph.N, graph.cap, grad_on, False, h_grad,
                                    any(trainable), all(trainable), mode == 'bucket', native)
            assert model._route == want, (key, mode, model._route, want)
            routes.append((want.node, want.grads))
            assert want.path == 'fused' and want.padded == (key == 'h48')
            assert s.requires_grad == l.requires_grad == h.requires_grad == want.need_grad
            outs.append((s.detach().clone(), l.detach().clone(), h.detach().clone()))
            loss = loss + (l * l).sum() + s.sum()
        grads = None
        if mode in ('default', 'masked'):
            (loss + h.sum()).backward()
            grads = [p.grad.clone() for p in model.parameters()]
    model.check_graphs()
    return outs, grads, routes


@pytest.mark.parametrize('key', list(WIDTHS))
def test_every_mode_takes_its_route_and_computes_the_same_bits(window, key, monkeypatch):
    meta, calls = window
    res = {mode: _run(meta, calls, key, mode, monkeypatch) for mode in MODES}
    ref = res['no_grad'][0]
    took = {mode: set(res[mode][2]) for mode in MODES}
    if key == 'h64k2':          # attention heads: the Python node sequences the attention stage
        assert took == dict(no_grad={('python', 'none')}, default={('python', 'autograd')}, bucket={('python', 'inplace')},
                            frozen={('python', 'none')}, masked={('python', 'autograd')}, masked_no_grad={('python', 'none')})
    else:                       # (in-place accumulation is ignored on a padded width)
        assert took == dict(no_grad={('native', 'none')}, default={('native', 'sink')},
                            bucket={('native', 'inplace' if key == 'h64' else 'sink')}, frozen={('native', 'none')},
                            masked={('python', 'autograd')}, masked_no_grad={('python', 'none')})
    for mode in MODES[1:]:
        for c, (a, b) in enumerate(zip(ref, res[mode][0])):
            for name, u, v in zip(('scores', 'logits', 'h_out'), a, b):
                assert u.shape == v.shape and torch.equal(u, v), (key, mode, c, name)
    # native node + gradient sink against the Python node with the parameters as autograd inputs: the tolerance of
    # tests/test_small_path_gpu.py::test_gradient_sink_keeps_the_autograd_contract for the same pair
    g0, g1 = res['default'][1], res['masked'][1]
    gscale = max(float(g.abs().max()) for g in g0)
    for i, (a, b) in enumerate(zip(g0, g1)):
        assert float((a - b).abs().max()) <= 1e-5 * gscale, (key, i)
