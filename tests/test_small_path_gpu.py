"""Batch-1 path (-m gpu): the one-launch adjacency conversion (tmpnn_graph_from_coo) and the fused iteration
(tmpnn_mp_iter_fwd / _bwd) against the torch-ops converter, the staged kernels, the oracle and the reference fixtures."""
import numpy as np
import pytest
import torch

from oracle import trackmpnn_oracle as orc
from tests.conftest import golden_names, infer_golden_names
from tests.golden_util import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _all_calls():
    out = []
    for name in golden_names() + infer_golden_names():
        gold = Golden(name)
        for c in range(gold.ncalls):
            out.append((name, c))
    return out


@pytest.mark.parametrize('name', golden_names() + infer_golden_names())
def test_device_conversion_equals_torch_conversion(name):
    """tmpnn_graph_from_coo on the reference's own adjacency tensors (dense first call, uncoalesced COO with explicit
    zeros afterwards, ragged graphs after decode_tracks' row deletion) gives bit for bit the arrays of the torch-ops
    converter, which tests/test_graph.py pins to the oracle."""
    from trackmpnn_amd import device_graph_from_adjacency, graph_from_adjacency
    gold = Golden(name)
    for c in range(gold.ncalls):
        na, ea = gold.adjacency(c, 'node_adj'), gold.adjacency(c, 'edge_adj')
        if na.shape[0] > 4096:
            continue
        ref = graph_from_adjacency(na, ea)
        dg = device_graph_from_adjacency(na, ea, DEV)
        assert dg.status() == 0
        g = dg.frame_graph()
        assert (g.N, g.E, g.Dn) == (ref.N, ref.E, ref.Dn)
        for f in ('src', 'dst', 'edge_row', 'det_row', 'rowptr', 'inc', 'is_edge', 'pos', 'src_pos', 'dst_pos'):
            assert torch.equal(getattr(g, f).cpu(), getattr(ref, f)), (c, f)
        # node_adj alone (no cross-check) converts to the same graph
        dg2 = device_graph_from_adjacency(na, None, DEV)
        assert dg2.status() == 0 and torch.equal(dg2.frame_graph().inc.cpu(), ref.inc)


def test_device_conversion_rejects_invalid_graphs():
    from trackmpnn_amd import TrackMPNN, device_graph_from_adjacency
    a = torch.zeros(3, 3)
    a[0, 0] = a[2, 2] = 1
    a[1, 0] = 1                          # edge row with only a +1
    dg = device_graph_from_adjacency(a, None, DEV)
    assert dg.status() & 2
    with pytest.raises(ValueError):
        dg.check()
    b = torch.zeros(3, 3)
    b[0, 0] = b[2, 2] = 1
    b[1, 0], b[1, 2] = 1, -1
    e = b.t().clone()
    e[0, 0] = e[2, 2] = 0
    e[1, 1] = 1
    assert device_graph_from_adjacency(b, e, DEV).status() == 0
    e2 = e.clone()
    e2[0, 1] = -1                        # sign flipped
    assert device_graph_from_adjacency(b, e2, DEV).status() & 32
    e3 = e.clone()
    e3[1, 1] = 0                         # diagonal does not complement
    assert device_graph_from_adjacency(b, e3, DEV).status() & 16
    c = b.clone()
    c[1, 0], c[1, 2] = -1, 1             # src after dst
    assert device_graph_from_adjacency(c, None, DEV).status() & 8
    d = b.clone()
    d[1, 0] = 0.5
    assert device_graph_from_adjacency(d, None, DEV).status() & 1
    # empty / edgeless graphs
    assert device_graph_from_adjacency(torch.eye(4), None, DEV).meta() == (0, 4, 0)
    # the model reports an invalid adjacency late (before backward / on check_graphs), or at once when asked to
    model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).eval()
    with torch.no_grad():
        model(torch.zeros(3, 8, device=DEV), None, a.to(DEV), a.t().contiguous().to(DEV))
    with pytest.raises(ValueError):
        model.check_graphs()


@pytest.mark.parametrize('mode', ['sink', 'bucket'])
def test_invalid_adjacency_cannot_reach_the_optimizer(mode):
    """A training forward on an adjacency that fails validation (reported late on the batch-1 path) returns NaN -- never
    uninitialised memory -- and the backward raises BEFORE any native node runs: default gradient mode (gradient sink)
    and GradBucket (anchored node), both through csrc_host/fast_iter.cpp when it is built."""
    from trackmpnn_amd import TrackMPNN
    from trackmpnn_amd.dist import GradBucket
    a = torch.zeros(4, 4)
    a[0, 0] = a[3, 3] = 1
    a[1, 0] = 1                          # edge row with only a +1
    a[2, 0], a[2, 3] = 1, -1
    e = a.t().clone()
    e[0, 0] = e[3, 3] = 0
    e[1, 1] = e[2, 2] = 1
    model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).train()
    if mode == 'bucket':
        GradBucket(model)
    x = torch.zeros(4, 8, device=DEV)
    x[0] = 1.0
    x[3] = -1.0
    s, l, h, _ = model(x, None, a.to(DEV), e.to(DEV))
    assert bool(torch.isnan(s).all()) and bool(torch.isnan(l).all()) and bool(torch.isnan(h).all())
    with pytest.raises(ValueError, match='factor graph'):
        (l.sum() + h.sum()).backward()
    model._pending_graphs = []


def test_nonzero_edge_row_features_are_rejected_not_ignored():
    """The reference runs every new row of x through Lin1 and the batch statistics (track_mpnn.py:59); its graph code always
    passes zeros on edge rows (utils/graph.py:148-149, 291-292) and this implementation reads det rows only.  A non-zero
    edge row is therefore an invalid call on the batch-1 path: NaN outputs and a ValueError at the next check, not a silent
    divergence."""
    from trackmpnn_amd import TrackMPNN
    b = torch.zeros(3, 3)
    b[0, 0] = b[2, 2] = 1
    b[1, 0], b[1, 2] = 1, -1
    e = b.t().clone()
    e[0, 0] = e[2, 2] = 0
    e[1, 1] = 1
    model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).eval()
    x = torch.randn(3, 8, device=DEV)
    x[1] = 0
    with torch.no_grad():
        s, l, h, _ = model(x, None, b.to(DEV), e.to(DEV))
    model.check_graphs()
    assert bool(torch.isfinite(s).all())
    x[1, 3] = 0.25                       # the edge row
    with torch.no_grad():
        s, l, h, _ = model(x, None, b.clone().to(DEV), e.clone().to(DEV))
    assert bool(torch.isnan(s).all())
    with pytest.raises(ValueError, match='EDGE rows'):
        model.check_graphs()


def _run_model(model, calls, small, monkeypatch, weights=None):
    import trackmpnn_amd.track_mpnn as tm
    monkeypatch.setattr(tm, 'SMALL_PATH', small)
    model._graph_cache = None
    h, loss, outs, xs = None, 0.0, [], []
    for i, (x, na, ea) in enumerate(calls):
        x = x.clone().requires_grad_(True)
        xs.append(x)
        s, l, h, _ = model(x, h, na, ea)
        w = weights[i]
        loss = loss + (w[0] * l).sum() + (w[1] * s).sum()
        outs.append((s.detach().clone(), l.detach().clone(), h.detach().clone()))
    loss = loss + (weights[-1] * h).sum()
    model.zero_grad(set_to_none=True)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    return outs, grads, [x.grad.clone() for x in xs]


@pytest.mark.parametrize('name', [n for n in golden_names() if '_k0_' in n or n.startswith(('roll_c', 'c1_'))
                                  or ('_k2_eval' in n and n.startswith('roll_'))])
def test_fused_iteration_matches_staged_kernels(name, monkeypatch):
    """Same fixture, same model: the fused batch-1 iteration against the staged C-ABI stages (round 1's path), forward
    of every call + gradients of every parameter and of x.  Covers diff / concat, 1 and 3 feature groups, H 32 / 64,
    train / eval, the C1 static window, the C2 / C3 / C4-size rolling windows and -- round 4 -- the models with attention
    heads (eval fixtures: the drawn dropout masks of a training call cannot be shared between two runs through model())."""
    from tests.test_parity_gpu import build_model
    gold = Golden(name)
    if gold.meta['nhidden'] > 64 or (gold.meta['nhidden'] not in (32, 64) and gold.meta['nattheads'] > 0):
        pytest.skip('fused path: nhidden <= 64 (widths other than 32 / 64 zero-padded, without attention heads)')
    calls = [(gold.t(f'c{c}/x').to(DEV), gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV))
             for c in range(gold.ncalls)]
    weights = [(gold.t(f'c{c}/wl').to(DEV), gold.t(f'c{c}/ws').to(DEV)) for c in range(gold.ncalls)] + [gold.t('V').to(DEV)]
    res = []
    for small in (False, True):
        model = build_model(gold.meta, gold.params())
        res.append(_run_model(model, calls, small, monkeypatch, weights) + (dict(model.named_buffers()),))
    (o0, g0, x0, b0), (o1, g1, x1, b1) = res
    for c, (a, b) in enumerate(zip(o0, o1)):
        assert (a[0] - b[0]).abs().max().item() <= 1e-5, f'scores call {c}'
        # (the 11-call C3 chain amplifies rounding differences: same budget as against the reference fixtures)
        assert torch.allclose(a[1], b[1], atol=2e-4, rtol=2e-5), f'logits call {c}'
        assert torch.allclose(a[2], b[2], atol=2e-4, rtol=2e-5), f'h_out call {c}'
    gscale = max(1.0, max(v.abs().max().item() for v in g0.values()))
    for k in g0:
        # (2e-5 on the 4..7-call chains; the 11-call C3 chain reaches 5e-5: same budget as against the fixtures)
        tol = 1e-4 * gscale * (10 if (k.endswith('.0.bias') and k.startswith('input_')) else 1)
        assert (g0[k] - g1[k]).abs().max().item() <= tol, f'grad {k}: {(g0[k] - g1[k]).abs().max().item()} > {tol}'
    for c, (a, b) in enumerate(zip(x0, x1)):
        if a.numel():
            assert torch.allclose(a, b, atol=1e-4 * max(1.0, a.abs().max().item()), rtol=0), f'd_x call {c}'
    for k in b0:
        if b0[k].dtype.is_floating_point:
            assert torch.allclose(b0[k], b1[k], atol=1e-6, rtol=1e-5), k
        else:
            assert int(b0[k]) == int(b1[k]), k


def test_fused_iteration_is_bitwise_reproducible_and_sync_free(monkeypatch):
    """Two runs give identical bits (fixed-order reductions, no float atomics); GradBucket's in-place accumulation
    gives the same gradients as returned ones; the forward calls of a window never synchronise with the host."""
    from tests.test_parity_gpu import build_model
    from trackmpnn_amd.dist import GradBucket
    gold = Golden('roll_c2_kitti_car_w5')
    calls = []
    for c in range(gold.ncalls):
        na, ea = gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV)
        if not na.is_sparse:                     # as initialize_graph(cuda=True) hands it over (utils/graph.py:180-184)
            na, ea = na.to_sparse(), ea.to_sparse()
        calls.append((gold.t(f'c{c}/x').to(DEV), na, ea))
    weights = [(gold.t(f'c{c}/wl').to(DEV), gold.t(f'c{c}/ws').to(DEV)) for c in range(gold.ncalls)] + [gold.t('V').to(DEV)]
    runs = []
    for _ in range(2):
        model = build_model(gold.meta, gold.params())
        runs.append(_run_model(model, calls, True, monkeypatch, weights))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    # in-place accumulation into a GradBucket
    model = build_model(gold.meta, gold.params())
    bucket = GradBucket(model)
    h, loss = None, 0.0
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.current_stream()):
        pass
    import trackmpnn_amd.track_mpnn as tm
    monkeypatch.setattr(tm, 'SMALL_PATH', True)
    # sync-free forward: with sync debug mode on 'error', any host synchronisation in the loop raises
    torch.cuda.set_sync_debug_mode('error')
    try:
        for i, (x, na, ea) in enumerate(calls):
            s, l, h, _ = model(x, h, na, ea)
            loss = loss + (weights[i][0] * l).sum() + (weights[i][1] * s).sum()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    loss = loss + (weights[-1] * h).sum()
    loss.backward()
    assert bucket.check_alias()
    gscale = max(1.0, max(v.abs().max().item() for v in runs[0][1].values()))
    for k, p in model.named_parameters():
        assert (p.grad - runs[0][1][k]).abs().max().item() <= 1e-6 * gscale, k


def test_fused_iteration_continuation_from_the_same_state_twice():
    """The carried state is extended in place only once: continuing twice from the same h_out (e.g. trying two
    hypotheses for the next frame) must give the same result both times and must not disturb the first call's
    backward."""
    from tests.test_parity_gpu import build_model
    gold = Golden('roll_2d_diff_k0_train')
    model = build_model(gold.meta, gold.params())
    calls = [(gold.t(f'c{c}/x').to(DEV), gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV))
             for c in range(2)]
    s0, l0, h0, _ = model(calls[0][0], None, calls[0][1], calls[0][2])
    s1, l1, h1, _ = model(calls[1][0], h0, calls[1][1], calls[1][2])
    model._graph_cache = None
    s2, l2, h2, _ = model(calls[1][0], h0, calls[1][1], calls[1][2])
    assert torch.equal(l1, l2) and torch.equal(h1, h2)
    (l1.sum() + l2.sum()).backward()
    g = [p.grad.clone() for p in model.parameters()]
    model.zero_grad()
    model._graph_cache = None
    s0, l0, h0, _ = model(calls[0][0], None, calls[0][1], calls[0][2])
    s1, l1, h1, _ = model(calls[1][0], h0, calls[1][1], calls[1][2])
    (2 * l1.sum()).backward()
    for a, p in zip(g, model.parameters()):
        assert torch.allclose(a, p.grad, rtol=1e-5, atol=1e-6 * max(1.0, float(a.abs().max())))


def test_captured_window_replay_equals_eager_steps():
    """CapturedWindow (whole-window hipGraph: forward calls + loss + backward + Adam) replayed three times gives the
    parameters of three eager steps bit for bit, and replays pick up refreshed features."""
    from tests.test_parity_gpu import build_model
    from trackmpnn_amd import CapturedWindow
    from trackmpnn_amd.dist import GradBucket
    gold = Golden('roll_c2_kitti_car_w5')
    calls = []
    for c in range(gold.ncalls):
        na, ea = gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV)
        if not na.is_sparse:
            na, ea = na.to_sparse(), ea.to_sparse()
        calls.append((gold.t(f'c{c}/x').to(DEV), na, ea))
    loss_fn = lambda outs, h: torch.cat([l for _, l in outs]).square().mean() + h.square().mean()      # noqa: E731
    xs2 = [x * 0.5 for x, _, _ in calls]

    def eager():
        model = build_model(gold.meta, gold.params())
        bucket = GradBucket(model)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
        losses = []
        for it in range(3):
            h, outs = None, []
            for i, (x, na, ea) in enumerate(calls):
                s, l, h, _ = model(xs2[i] if it == 2 else x, h, na, ea)
                outs.append((s, l))
            loss = loss_fn(outs, h)
            bucket.zero()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        return model, losses

    m_ref, l_ref = eager()
    model = build_model(gold.meta, gold.params())
    bucket = GradBucket(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    st0 = None
    win = CapturedWindow(model, calls, loss_fn, optimizer=opt, bucket=bucket, warmup=2)
    # the warm-up and the capture itself stepped the optimizer: rewind model and optimizer, then replay 3 steps
    model.load_state_dict(sd0)
    for st in opt.state.values():
        for k, v in st.items():
            if torch.is_tensor(v):
                v.zero_()
    losses = [win.replay().item(), win.replay().item(), win.replay(xs2).item()]
    assert losses == l_ref
    for (k, a), (_, b) in zip(model.state_dict().items(), m_ref.state_dict().items()):
        assert torch.equal(a, b), k


def test_gradient_sink_keeps_the_autograd_contract():
    """Default gradient mode on the native node (no GradBucket): every call returns its parameter gradients as ONE flat
    buffer to the model's gradient sink, which hands the slices to the parameters once per backward pass.  Checked here:
    torch.autograd.grad leaves .grad alone and equals .backward(); a tensor hook fires once per pass with the TOTAL
    gradient; two windows accumulated without an optimizer step (the sink node runs backward twice) give twice the
    gradient; a parameter update makes a fresh sink; a frozen parameter falls back to the Python node with equal results."""
    from tests.test_parity_gpu import build_model
    gold = Golden('roll_2d_diff_k0_train')
    model = build_model(gold.meta, gold.params())
    assert model.inplace_param_grads is False
    calls = [(gold.t(f'c{c}/x').to(DEV), gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV))
             for c in range(gold.ncalls)]

    def window_loss(m=model):
        h, loss = None, 0.0
        for x, na, ea in calls:
            s, l, h, _ = m(x, h, na, ea)
            loss = loss + (l * l).sum() + s.sum()
        return loss + h.sum()

    params = list(model.parameters())
    for p in params:
        p.grad = torch.full_like(p, 3.0)
    grads = torch.autograd.grad(window_loss(), params)
    assert (model._route.node, model._route.grads) == ('native', 'sink') and model._sink is not None
    assert all(bool((p.grad == 3.0).all()) for p in params)
    gscale = max(float(g.abs().max()) for g in grads)
    fired = []
    hook = params[4].register_hook(lambda g: fired.append(g.clone()))
    for p in params:
        p.grad = None
    sink0 = model._sink
    window_loss().backward()
    assert len(fired) == 1 and float((fired[0] - grads[4]).abs().max()) <= 1e-6 * gscale
    for p, g in zip(params, grads):
        assert float((p.grad - g).abs().max()) <= 1e-6 * gscale
    window_loss().backward()                                         # accumulate a second window, no step in between
    assert model._sink is sink0 and len(fired) == 2
    for p, g in zip(params, grads):
        assert float((p.grad - 2 * g).abs().max()) <= 2e-6 * gscale
    hook.remove()
    with torch.no_grad():
        params[0].mul_(1.0)                                          # an in-place update moves the version counter
    for p in params:
        p.grad = None
    window_loss().backward()
    assert model._sink is not sink0
    for p, g in zip(params, grads):
        assert float((p.grad - g).abs().max()) <= 1e-6 * gscale
    # a frozen parameter: Python node (gradients per parameter), same numbers for the others
    frozen = build_model(gold.meta, gold.params())
    fp = list(frozen.parameters())
    fp[2].requires_grad_(False)
    window_loss(frozen).backward()
    assert (frozen._route.node, frozen._route.grads) == ('python', 'autograd') and frozen._sink is None and fp[2].grad is None
    for i, (p, g) in enumerate(zip(fp, grads)):
        if i != 2:
            assert float((p.grad - g).abs().max()) <= 1e-5 * gscale, i


def _dense_window_calls(seed, frames, mean_dets, max_dets, F, with_sequence=False):
    """A dense synthetic chunk (BDD-like density) as the reference would hand it over: per call (x, node_adj, edge_adj)
    with the adjacency pair as sparse COO tensors (+1 / -1 on an edge row's src / dst column, 1 on det diagonals;
    edge_adj = the transpose off the diagonal, 1 on edge diagonals)."""
    from trackmpnn_amd import WindowBuilder, synth_window
    y = synth_window(seed, frames, mean_dets, max_dets)
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(y.shape[0], F, generator=gen)
    is_edge = np.zeros(0, bool)
    src = np.zeros(0, np.int64)
    dst = np.zeros(0, np.int64)
    calls = []
    for call in WindowBuilder(y).calls():
        n_old = is_edge.size
        is_edge = np.concatenate([is_edge, call.new_is_edge])
        src = np.concatenate([src, call.new_src])
        dst = np.concatenate([dst, call.new_dst])
        N = is_edge.size
        er = torch.from_numpy(np.nonzero(is_edge)[0])
        dr = torch.from_numpy(np.nonzero(~is_edge)[0])
        s, d = torch.from_numpy(src), torch.from_numpy(dst)
        ni = torch.stack([torch.cat([er, er, dr]), torch.cat([s, d, dr])])
        nv = torch.cat([torch.ones(er.numel()), -torch.ones(er.numel()), torch.ones(dr.numel())])
        ei = torch.stack([torch.cat([s, d, er]), torch.cat([er, er, er])])
        ev = torch.cat([torch.ones(er.numel()), -torch.ones(er.numel()), torch.ones(er.numel())])
        na = torch.sparse_coo_tensor(ni, nv, (N, N)).to(DEV)
        ea = torch.sparse_coo_tensor(ei, ev, (N, N)).to(DEV)
        x = torch.zeros(call.n_new, F)
        x[~call.new_is_edge] = X[call.det_ids]
        calls.append((x.to(DEV), na, ea))
    if with_sequence:
        return calls, X, torch.from_numpy(y)
    return calls


def test_dense_scene_above_4096_rows(monkeypatch):
    """Windows of dense scenes (tens of dets per frame) exceed the 4096 rows whose conversion work arrays fit the LDS:
    tmpnn_graph_from_coo_arena_ws keeps them in a global scratch (up to 65535 rows) and the fused iteration takes the
    graph as it is.  Conversion against the torch-ops converter, then the fused path against the staged kernels."""
    from trackmpnn_amd import TrackMPNN, device_graph_from_adjacency, graph_from_adjacency
    calls = _dense_window_calls(seed=3, frames=8, mean_dets=32, max_dets=45, F=8)
    sizes = [int(na.shape[0]) for _, na, _ in calls]
    assert sizes[-1] > 4096 and sizes[-1] <= 65535, sizes
    for _, na, ea in calls:
        if na.shape[0] <= 4096:
            continue
        ref = graph_from_adjacency(na, ea)
        dg = device_graph_from_adjacency(na, ea, DEV)
        assert dg.status() == 0
        g = dg.frame_graph()
        assert (g.N, g.E, g.Dn) == (ref.N, ref.E, ref.Dn)
        for f in ('src', 'dst', 'edge_row', 'det_row', 'rowptr', 'inc', 'is_edge', 'pos', 'src_pos', 'dst_pos'):
            assert torch.equal(getattr(g, f).cpu(), getattr(ref, f).cpu()), f
    # an invalid big graph is still reported: flip one sign
    _, na, ea = calls[-1]
    vals = na._values().clone()
    vals[0] = -vals[0]
    bad = torch.sparse_coo_tensor(na._indices(), vals, na.shape)
    assert device_graph_from_adjacency(bad, None, DEV).status() != 0
    gen = torch.Generator().manual_seed(7)
    weights = [(torch.randn(n, 1, generator=gen).to(DEV), torch.randn(n, 1, generator=gen).to(DEV)) for n in sizes]
    weights.append(torch.randn(sizes[-1], 64, generator=gen).to(DEV))
    res = []
    for small in (False, True):
        torch.manual_seed(5)
        model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).train()
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(DEV))
        res.append(_run_model(model, calls, small, monkeypatch, weights))
    (o0, g0, x0), (o1, g1, x1) = res
    for c, (a, b) in enumerate(zip(o0, o1)):
        assert (a[0] - b[0]).abs().max().item() <= 1e-5, f'scores call {c}'
        assert torch.allclose(a[1], b[1], atol=2e-4, rtol=2e-5), f'logits call {c}'
        assert torch.allclose(a[2], b[2], atol=2e-4, rtol=2e-5), f'h_out call {c}'
    gscale = max(1.0, max(v.abs().max().item() for v in g0.values()))
    for k in g0:
        tol = 1e-4 * gscale * (10 if (k.endswith('.0.bias') and k.startswith('input_')) else 1)
        assert (g0[k] - g1[k]).abs().max().item() <= tol, f'grad {k}: {(g0[k] - g1[k]).abs().max().item()} > {tol}'


def _window(gold):
    return [(gold.t(f'c{c}/x').to(DEV), gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV))
            for c in range(gold.ncalls)]


def _run_window(model, calls):
    h, loss = None, 0.0
    for x, na, ea in calls:
        s, l, h, _ = model(x, h, na, ea)
        loss = loss + (l * l).sum() + s.sum()
    return loss + h.sum()


def test_model_can_be_copied_and_pickled_after_use():
    """copy.deepcopy / pickle / torch.save of a module that has run the batch-1 path (its caches hold ctypes pointer
    structs and a non-leaf sink tensor): the copy is a working, independent model with the same parameters."""
    import copy
    import io
    import pickle
    from tests.test_parity_gpu import build_model
    gold = Golden('roll_2d_diff_k0_train')
    model = build_model(gold.meta, gold.params())
    calls = _window(gold)
    ref = _run_window(model, calls)
    ref.backward()
    twin = copy.deepcopy(model)
    again = pickle.loads(pickle.dumps(model))
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    for m in (twin, again, loaded):
        assert m._small is not model._small and m._sink is None
        out = _run_window(m, calls)
        assert torch.equal(out.detach(), ref.detach())
        out.backward()
        for (n1, p1), (_, p2) in zip(model.named_parameters(), m.named_parameters()):
            assert p1.data_ptr() != p2.data_ptr()
            assert torch.allclose(p1.grad, p2.grad, rtol=1e-5, atol=1e-6), n1
    # the copy is independent: changing it leaves the original's results alone
    with torch.no_grad():
        for p in twin.parameters():
            p.mul_(0.5)
    assert torch.equal(_run_window(model, calls).detach(), ref.detach())


def test_refresh_weights_after_an_edit_through_data():
    """The GRU operand images of the fused iteration follow the weights' version counters; `p.data` edits do not move
    them.  TrackMPNN.refresh_weights() re-reads everything: results then equal a model built with the edited weights."""
    from tests.test_parity_gpu import build_model
    gold = Golden('roll_2d_diff_k0_train')
    model = build_model(gold.meta, gold.params())
    calls = _window(gold)
    before = _run_window(model, calls).detach()
    w = model.factor_grus[0].edge_gru.weight_hh
    w.data.mul_(0.5)                                   # (no version bump)
    model.refresh_weights()
    after = _run_window(model, calls).detach()
    params = {k: v.clone() for k, v in gold.params().items()}
    params['factor_grus.0.edge_gru.weight_hh'] = params['factor_grus.0.edge_gru.weight_hh'] * 0.5
    fresh = build_model(gold.meta, params)
    assert not torch.equal(before, after)
    assert torch.equal(after, _run_window(fresh, calls).detach())


def test_frozen_model_in_grad_mode_returns_plain_tensors():
    """infer.py runs the model without torch.no_grad(): with every parameter frozen nothing needs a gradient, and the
    native node must hand back plain tensors (usable with .numpy()) exactly like the Python node."""
    from tests.test_parity_gpu import build_model
    gold = Golden('roll_2d_diff_k0_train')
    model = build_model(gold.meta, gold.params()).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    assert torch.is_grad_enabled()
    h = None
    for x, na, ea in _window(gold):
        s, l, h, _ = model(x, h, na, ea)
        assert not s.requires_grad and not l.requires_grad and not h.requires_grad
        s.cpu().numpy()


def test_native_node_outlives_the_python_side_caches():
    """The native node's backward reads its parameter structs from copies it owns: dropping every Python-side cache
    (SmallPath.invalidate, what .to() / load_state_dict / a detected storage swap do) between forward and backward
    changes nothing."""
    from tests.test_parity_gpu import build_model
    gold = Golden('roll_2d_diff_k0_train')
    calls = _window(gold)
    grads = []
    for drop in (False, True):
        model = build_model(gold.meta, gold.params())
        loss = _run_window(model, calls)
        if drop:
            model._small.invalidate()
            model._small.cparams = None
            model._small._tmpl = None
            import gc
            gc.collect()
        loss.backward()
        grads.append([p.grad.clone() for p in model.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize('desc,nhidden,heads,train', [('wide cells', 128, 0, True), ('padded width', 48, 0, True),
                                                      ('attention heads, eval', 64, 2, False)])
def test_captured_window_records_models_outside_the_fused_path(desc, nhidden, heads, train):
    """CapturedWindow on models the plain fused batch-1 iteration does not cover: nhidden 128 goes through the staged kernels on
    plans built before the capture; attention heads (round 4) through the fused iteration with the attention stage between its
    two launches; a padded width (round 5) through the fused iteration on its zero-padded parameter copies.  A replay gives the gradients and the loss of the eager step through
    model(x, h, node_adj, edge_adj) bit for bit (deterministic kernels; the attention model in eval mode, where no dropout
    mask is drawn)."""
    from trackmpnn_amd import CapturedWindow, TrackMPNN
    gold = Golden('roll_c2_kitti_car_w5')
    calls = []
    for c in range(gold.ncalls):
        na, ea = gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV)
        if not na.is_sparse:
            na, ea = na.to_sparse(), ea.to_sparse()
        calls.append((gold.t(f'c{c}/x').to(DEV), na, ea))
    loss_fn = lambda outs, h: torch.cat([l for _, l in outs]).square().mean() + h.square().mean()      # noqa: E731

    def make():
        torch.manual_seed(11)
        m = TrackMPNN('2d', 3, nhidden, heads, 'diff').to(DEV)
        return m.train() if train else m.eval()

    from trackmpnn_amd.dist import GradBucket
    ref = make()
    if not getattr(ref, '_padded', False):
        GradBucket(ref)            # a captured step accumulates in place (kernels add into .grad): compare like with like
    h, outs = None, []
    for x, na, ea in calls:
        s, l, h, _ = ref(x, h, na, ea)
        outs.append((s, l))
    loss_ref = loss_fn(outs, h)
    loss_ref.backward()
    model = make()
    h, outs = None, []
    for x, na, ea in calls:                                  # a first backward creates the .grad buffers the graph bakes in
        s, l, h, _ = model(x, h, na, ea)
        outs.append((s, l))
    loss_fn(outs, h).backward()
    if getattr(model, '_padded', False):
        del s, l, h, outs                                    # (padded widths: no autograd graph of the model may be alive)
    if train:                                                # (BatchNorm running statistics moved: start both from the same)
        model.load_state_dict(make().state_dict())
    win = CapturedWindow(model, calls, loss_fn, optimizer=None, bucket=None, warmup=2)
    assert win.staged == (nhidden > 64)                      # (a padded width without heads rides the fused iteration since round 5)
    first = win.replay().item()                              # (the returned tensor is static: read it before the next replay)
    assert first == loss_ref.item()
    for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    xs2 = [x * 0.5 for x, _, _ in calls]
    assert win.replay(xs2).item() != first                   # refreshed features are picked up


def test_captured_window_draws_fresh_attention_dropout_per_replay():
    """Train mode with attention heads: the dropout masks are drawn inside the captured region, so every replay draws new
    ones (the generator's offset advances per replay) -- two replays of the same step differ, both finite."""
    from trackmpnn_amd import CapturedWindow, TrackMPNN
    gold = Golden('roll_c2_kitti_car_w5')
    calls = []
    for c in range(gold.ncalls):
        na, ea = gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV)
        if not na.is_sparse:
            na, ea = na.to_sparse(), ea.to_sparse()
        calls.append((gold.t(f'c{c}/x').to(DEV), na, ea))
    torch.manual_seed(3)
    model = TrackMPNN('2d', 3, 64, 2, 'diff').to(DEV).train()
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.2 * torch.randn_like(p))                # (the default init makes the heads' output nearly input-independent)
    loss_fn = lambda outs, h: torch.cat([l for _, l in outs]).square().mean() + h.square().mean()      # noqa: E731
    h, outs = None, []
    for x, na, ea in calls:
        s, l, h, _ = model(x, h, na, ea)
        outs.append((s, l))
    loss_fn(outs, h).backward()
    win = CapturedWindow(model, calls, loss_fn, optimizer=None, bucket=None, warmup=2)
    a, b = win.replay().item(), win.replay().item()
    assert np.isfinite(a) and np.isfinite(b) and a != b


@pytest.mark.parametrize('name', ['roll_2d_diff_k2_train', 'roll_2d_concat_k2_train', 'roll_2d-temp-vis_concat_k2_train',
                                  'roll_2d_diff_k2_eval', 'roll_2d-temp-vis_diff_k2_eval'])
def test_fused_iteration_with_attention_heads_matches_the_reference(name):
    """Models with attention heads through the batch-1 path (tmpnn_mp_iter_*_parts with the attention stage between the two
    launches): every call of the reference's fixture (its drawn dropout mask injected), scores / logits / state, the
    attention values, and every parameter / input gradient -- same tolerances as the staged path against the fixtures."""
    from tests.test_parity_gpu import build_model
    from trackmpnn_amd.graph import device_graph_from_adjacency
    gold = Golden(name)
    m = gold.meta
    model = build_model(m, gold.params())
    assert model._small.att and model._small.eligible
    G = len(model.spec.groups)
    h, loss, xs = None, 0.0, []
    for c in range(gold.ncalls):
        x = gold.t(f'c{c}/x').to(DEV).requires_grad_(True)
        xs.append(x)
        dg = device_graph_from_adjacency(gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV), DEV)
        fg = dg.frame_graph()
        keep = None
        if m['mode'] == 'train':
            e, ep = fg.inc_edge_endpoint()
            keep = [gold.t(f'c{c}/keep_g{g}').to(DEV)[:, e, ep].contiguous() for g in range(G)]
        s, l, h, att = model.forward_dgraph(x, h, dg, dropout_keep=keep)
        assert (s.detach().cpu() - gold.t(f'c{c}/scores')).abs().max().item() <= 1e-4, f'scores call {c}'
        assert torch.allclose(l.detach().cpu(), gold.t(f'c{c}/logits'), atol=2e-4, rtol=2e-5), f'logits call {c}'
        assert torch.allclose(h.detach().cpu(), gold.t(f'c{c}/h_out'), atol=2e-4, rtol=2e-5), f'h_out call {c}'
        for g in range(G):
            for k in range(m['nattheads']):
                got = att[g][k].per_edge().cpu()                         # [E, 2]: (src side, dst side)
                assert torch.allclose(got, gold.t(f'c{c}/att_g{g}_k{k}'), atol=1e-5, rtol=1e-4), (c, g, k)
        loss = loss + (gold.t(f'c{c}/wl').to(DEV) * l).sum() + (gold.t(f'c{c}/ws').to(DEV) * s).sum()
    loss = loss + (gold.t('V').to(DEV) * h).sum()
    loss.backward()
    grads = gold.grads()
    gscale = max(1.0, max(v.abs().max().item() for k, v in grads.items() if k != 'X'))
    for k, p in model.named_parameters():
        tol = 2e-4 * gscale
        if m['mode'] == 'train' and k.startswith('input_transforms.') and k.endswith('.0.bias'):
            tol = 2e-3 * gscale      # exactly-zero true gradient (BatchNorm removes the mean): cancellation noise
        err = (p.grad.cpu() - grads[k]).abs().max().item()
        assert err <= tol, f'grad {k}: {err} > {tol}'


@pytest.mark.parametrize('features', ['2d', '2d+temp'])
def test_padded_width_state_honours_in_place_edits_between_calls(features):
    """A zero-padded width on the fused path keeps the carried state in padded form behind the [N, G nhidden] tensor the caller
    sees (one feature group: a view of it; several: a copy).  An in-place edit of that tensor between two calls -- resetting
    rows, as a loop that masks tracks does -- must reach the next call either way (round-5 advisor finding: the copy's edit
    was dropped): the continuation equals the one from a fresh clone of the edited state."""
    from trackmpnn_amd import TrackMPNN, WindowBuilder, synth_window
    from trackmpnn_amd.graph import device_graph_from_adjacency
    from oracle import trackmpnn_oracle as orc
    torch.manual_seed(9)
    model = TrackMPNN(features, 3, 48, 0, 'diff').to(DEV).eval()
    F = 8 + (2 if 'temp' in features else 0)
    y = synth_window(3, 4, 4, 8)
    calls = WindowBuilder(y).calls()
    gen = torch.Generator().manual_seed(1)

    def adj(c_upto):
        N = sum(c.n_new for c in calls[:c_upto + 1])
        is_edge = np.concatenate([c.new_is_edge for c in calls[:c_upto + 1]])
        src = np.concatenate([c.new_src for c in calls[:c_upto + 1]])
        dst = np.concatenate([c.new_dst for c in calls[:c_upto + 1]])
        er = np.nonzero(is_edge)[0]
        na = torch.zeros(N, N); ea = torch.zeros(N, N)
        na[er, src] = 1.0; na[er, dst] = -1.0
        dr = np.nonzero(~is_edge)[0]
        na[dr, dr] = 1.0
        ea[src, er] = 1.0; ea[dst, er] = -1.0
        ea[er, er] = 1.0
        return na.to(DEV), ea.to(DEV)

    xs = []
    for c in calls:
        x = torch.zeros(c.n_new, F)
        x[~torch.from_numpy(c.new_is_edge)] = torch.randn(int((~c.new_is_edge).sum()), F, generator=gen)
        xs.append(x.to(DEV))
    with torch.no_grad():
        na, ea = adj(0)
        _, _, h, _ = model(xs[0], None, na, ea)
        assert getattr(h, '_tmpnn_padded_state', None) is not None, 'expected the padded fused path'
        h[1::2] = 0.0                                        # the caller's in-place edit
        na, ea = adj(1)
        s_a, _, h_a, _ = model(xs[1], h, na, ea)
        s_b, _, h_b, _ = model(xs[1], h.clone(), na, ea)     # (a clone carries no padded state: padded afresh from its values)
    assert torch.equal(s_a, s_b) and torch.equal(h_a, h_b)
