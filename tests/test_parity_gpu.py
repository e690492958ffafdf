"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
(1) the reference-generated golden fixtures, (2) the CPU oracle on seeded inputs, (3) size-independent
properties at the bench sizes."""
import os
import numpy as np
import pytest
import torch

from oracle import trackmpnn_oracle as orc
from tests.conftest import golden_names
from tests.golden_util import Golden

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SCORE_TOL = 1e-4     # BASELINE.json: edge/node scores within 1e-4 fp32 of the reference
LOGIT_ATOL, LOGIT_RTOL = 2e-4, 2e-5   # fixtures have |y|,|h| up to ~50 (weights perturbed by 0.3*N(0,1))
GRAD_RTOL = 2e-4     # relative to the largest gradient entry of the fixture


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def test_stage_checks():
    """Every C-ABI stage against its torch-CPU formula, H in {32, 64, 128, 256}."""
    from tests import gpu_stage_checks
    lines = []
    res = gpu_stage_checks.run_all(report=lines.append)
    bad = [ln for ln in lines if ln.startswith('FAIL')]
    assert not bad, '\n'.join(bad)
    assert len(res) > 200


def test_stage_checks_f32_mfma_path():
    """The same stage checks with TMPNN_SPLIT=0: the GRU GEMMs on the f32-input MFMA kernels instead of the bf16x6
    split products.  The switch is read once per process, hence the child process (one, sequential)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TMPNN_SPLIT='0', PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, os.path.join(root, 'tests', 'gpu_stage_checks.py')], env=env, cwd=root,
                       capture_output=True, text=True, timeout=600)
    tail = '\n'.join([ln for ln in r.stdout.splitlines() if ln.startswith('FAIL')] + r.stdout.splitlines()[-2:])
    assert r.returncode == 0, tail + r.stderr[-2000:]


@pytest.mark.skipif(__import__('os').environ.get('TMPNN_TEST_VARIANTS') != '1',
                    reason='comparison kernels are compiled only with -DTMPNN_KEEP_VARIANTS (tools/build_variant.sh); '
                           'set TMPNN_TEST_VARIANTS=1 with TMPNN_LIB_PATH pointing at such a build')
def test_stage_checks_four_wave_one_pass_backward():
    """The stage checks (they run tmpnn_gru_bwd_fused wherever it is offered) with TMPNN_BWD_TWO=0: the one-pass backward as
    four 512-register waves per block (k_gru_bwd_one) instead of the default eight 256-register waves (k_gru_bwd_two).  The
    switch is read once per process, hence the child process.  Round 3: k_gru_bwd_one and the round-1 aggregation kernels
    are no longer in the shipped library (build flag TMPNN_KEEP_VARIANTS)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TMPNN_BWD_TWO='0', PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, os.path.join(root, 'tests', 'gpu_stage_checks.py')], env=env, cwd=root,
                       capture_output=True, text=True, timeout=600)
    tail = '\n'.join([ln for ln in r.stdout.splitlines() if ln.startswith('FAIL')] + r.stdout.splitlines()[-2:])
    assert r.returncode == 0, tail + r.stderr[-2000:]


def build_model(meta, params):
    from trackmpnn_amd import TrackMPNN
    m = TrackMPNN(meta['features'], meta['ncategories'], meta['nhidden'], meta['nattheads'], meta['msg_type'])
    missing = m.load_state_dict(params, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m = m.to(DEV)
    return m.train() if meta['mode'] == 'train' else m.eval()


@pytest.mark.parametrize('name', golden_names())
def test_golden_reference_parity(name):
    """Drop-in forward(x, h_in, node_adj, edge_adj) on the reference's own adjacency tensors, fwd + bwd."""
    from trackmpnn_amd import graph_from_adjacency, plan_single
    gold = Golden(name)
    meta = gold.meta
    model = build_model(meta, gold.params())
    K, G = meta['nattheads'], len(model.feature_idx)
    train = meta['mode'] == 'train'
    h = None
    loss = 0.0
    xs = []
    for c in range(gold.ncalls):
        na = gold.adjacency(c, 'node_adj', DEV)
        ea = gold.adjacency(c, 'edge_adj', DEV)
        x = gold.t(f'c{c}/x').to(DEV).requires_grad_(True)
        xs.append(x)
        if train and K > 0:
            # the reference's dense dropout stream cannot be replayed: inject the mask it actually drew
            graph = graph_from_adjacency(na, ea)
            e, ep = graph.inc_edge_endpoint()
            keep = [gold.t(f'c{c}/keep_g{g}').to(DEV)[:, e, ep].contiguous() for g in range(G)]
            scores, logits, h, att = model.forward_graph(x, h, plan_single(graph, x.shape[0]), dropout_keep=keep)
        else:
            scores, logits, h, att = model(x, h, na, ea)
        assert (scores.detach().cpu() - gold.t(f'c{c}/scores')).abs().max().item() <= SCORE_TOL, f'scores call {c}'
        assert torch.allclose(logits.detach().cpu(), gold.t(f'c{c}/logits'), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), c
        if gold.has(f'c{c}/h_out'):
            assert torch.allclose(h.detach().cpu(), gold.t(f'c{c}/h_out'), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), c
        for g in range(G):
            for k in range(K):
                got = att[g][k].per_edge().cpu()
                assert torch.allclose(got, gold.t(f'c{c}/att_g{g}_k{k}'), atol=1e-5, rtol=1e-4), (c, g, k)
        if K > 0 and not train and c == 0:
            # dense reference layout incl. the uniform rows of all-masked softmaxes
            dense = att[0][0].to_reference_dense()
            assert dense.shape == (logits.shape[0], logits.shape[0])
            assert torch.allclose(dense.sum(1), torch.ones_like(dense[:, 0]), atol=1e-5)
        loss = loss + (gold.t(f'c{c}/wl').to(DEV) * logits).sum() + (gold.t(f'c{c}/ws').to(DEV) * scores).sum()
    loss = loss + (gold.t('V').to(DEV) * h).sum()
    ref_loss = float(gold.d['loss'])
    assert abs(loss.item() - ref_loss) <= 2e-4 * max(1.0, abs(ref_loss))
    loss.backward()
    grads = gold.grads()
    gscale = max(1.0, max(v.abs().max().item() for k, v in grads.items() if k != 'X'))
    for k, prm in model.named_parameters():
        tol = GRAD_RTOL * gscale
        if train and k.startswith('input_transforms.') and k.endswith('.0.bias'):
            tol = 2e-3 * gscale      # exactly-zero true gradient (BatchNorm removes the mean): cancellation noise
        err = (prm.grad.cpu() - grads[k]).abs().max().item()
        assert err <= tol, f'grad {k}: {err} > {tol}'
    if meta['static_iters'] == 0:
        gx = torch.cat([x.grad.cpu() if x.grad is not None else torch.zeros(x.shape) for x in xs], 0)
        is_det_new = []
        for c in range(gold.ncalls):
            g = graph_from_adjacency(gold.adjacency(c, 'node_adj'), gold.adjacency(c, 'edge_adj'))
            n = xs[c].shape[0]
            is_det_new.append(g.is_edge[g.N - n:] == 0)
        is_det_new = torch.cat(is_det_new)
        gX = grads['X'][0]
        assert torch.allclose(gx[is_det_new], gX, atol=GRAD_RTOL * max(1.0, gX.abs().max().item()), rtol=0)
    for k, ref in gold.final_buffers().items():
        got = dict(model.named_buffers())[k].cpu()
        if ref.dtype.is_floating_point:
            assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5), k
        else:
            assert int(got) == int(ref), k


def _oracle_graph(g):
    return orc.OracleGraph(g.N, g.is_edge.cpu().numpy().astype(bool), g.src.cpu().numpy().astype(np.int64),
                           g.dst.cpu().numpy().astype(np.int64), g.edge_row.cpu().numpy().astype(np.int64),
                           g.det_row.cpu().numpy().astype(np.int64))


def _batched_case(B, frames, mean, max_dets, F, seed0=0, static=False):
    from trackmpnn_amd import WindowBuilder, batch_windows, synth_window
    ys = [synth_window(seed0 + s, frames, mean, max_dets) for s in range(B)]
    wins = [WindowBuilder(y).calls() for y in ys]
    plans, refs = batch_windows(wins, static=static)
    gen = torch.Generator().manual_seed(seed0 + 999)
    Xs = [torch.randn(y.shape[0], F, generator=gen) for y in ys]
    xs = []
    for plan, ref in zip(plans, refs):
        x = torch.zeros(plan.n_new, F)
        if len(ref):
            x[plan.new_det_local] = torch.stack([Xs[b][i] for b, i in ref])
        xs.append(x)
    return plans, xs


@pytest.mark.parametrize('features,ncat,H,K,msg,train', [
    ('2d', 3, 64, 0, 'diff', True),           # C2 shape (KITTI 2d feats)
    ('2d', 8, 64, 0, 'diff', True),           # C4 shape (BDD, F=13)
    ('2d', 3, 64, 2, 'diff', False),
    ('2d', 3, 128, 0, 'concat', True),
    ('2d+temp+vis', 3, 64, 0, 'diff', True),
    ('2d', 3, 256, 0, 'diff', True),          # C5 width
    ('2d', 3, 128, 0, 'diff', True),          # wide cells at H = 128 (one 128-column operand tile per block)
    ('2d', 3, 64, 0, 'concat', True),         # concat at the headline width (generic forward, output-tiled dW kernel)
    ('2d', 3, 32, 0, 'diff', True),           # H = 32 instances of the LDS / bf16x6 kernels
    ('2d', 3, 32, 1, 'concat', False),
    # widths the kernels are not instantiated for run zero-padded to the next one (reference: any int,
    # utils/training_options.py:22)
    ('2d', 3, 48, 0, 'diff', True),
    ('2d', 3, 20, 0, 'concat', True),
    ('2d+temp+vis', 3, 48, 0, 'diff', True),
    ('2d', 3, 100, 2, 'diff', False),
    # more heads than one attention call takes (8): groups of heads, means combined (reference: any number of heads)
    ('2d', 3, 64, 11, 'diff', False),
    ('2d', 3, 32, 9, 'concat', False),
    # widths above 256 (multiples of 128 native, others zero-padded to the next one): diff messages, no attention heads
    ('2d', 3, 384, 0, 'diff', True),
    ('2d', 3, 300, 0, 'diff', True),
    ('2d+temp+vis', 3, 512, 0, 'diff', False),
    ('2d', 3, 640, 0, 'diff', True),
    ('2d', 3, 1024, 0, 'diff', False),
    ('2d', 3, 384, 0, 'concat', True),
])
def test_batched_windows_vs_oracle(features, ncat, H, K, msg, train):
    """Block-diagonal batches of KITTI-shaped rolling windows (per-window BatchNorm segments), fwd + bwd."""
    from trackmpnn_amd import TrackMPNN
    cfg = orc.OracleConfig(features, ncat, H, K, msg)
    F = sum(f for _, f in cfg.groups)
    plans, xs = _batched_case(B=16, frames=7, mean=6, max_dets=20, F=F, seed0=H + K)
    # keep the per-layer gain (scale * sqrt(H)) fixed so wider models stay as well conditioned as H = 64
    p = orc.random_params(cfg, seed=H, scale=1.2 / (H ** 0.5))
    model = TrackMPNN(features, ncat, H, K, msg)
    model.load_state_dict({k: v.clone() for k, v in p.items()}, strict=True)
    model = model.to(DEV)
    model.train() if train else model.eval()
    pr = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and 'running' not in k else v.clone())
          for k, v in p.items()}
    h = h_ref = None
    loss = loss_ref = 0.0
    gen = torch.Generator().manual_seed(1)
    for plan, x in zip(plans, xs):
        s_ref, l_ref, h_ref, _ = orc.forward(pr, cfg, x, h_ref, _oracle_graph(plan.graph), training=train,
                                             seg_ids=plan.seg_of_new)
        s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV))
        assert (s.detach().cpu() - s_ref.detach()).abs().max().item() <= SCORE_TOL
        assert torch.allclose(l.detach().cpu(), l_ref.detach(), atol=LOGIT_ATOL, rtol=LOGIT_RTOL)
        assert torch.allclose(h.detach().cpu(), h_ref.detach(), atol=LOGIT_ATOL, rtol=LOGIT_RTOL)
        w = torch.randn(l.shape, generator=gen)
        loss = loss + (w.to(DEV) * l).sum() + s.sum()
        loss_ref = loss_ref + (w * l_ref).sum() + s_ref.sum()
    loss.backward()
    loss_ref.backward()
    gscale = max(1.0, max(v.grad.abs().max().item() for v in pr.values() if v.grad is not None))
    for k, prm in model.named_parameters():
        tol = GRAD_RTOL * gscale * (10 if (train and k.endswith('.0.bias') and k.startswith('input_')) else 1)
        err = (prm.grad.cpu() - pr[k].grad).abs().max().item()
        assert err <= tol, f'grad {k}: {err} > {tol}'
    for k, b in model.named_buffers():
        if b.dtype.is_floating_point:
            assert torch.allclose(b.cpu(), pr[k], atol=1e-5, rtol=1e-4), k


def test_eval_no_grad_and_empty_calls():
    """Inference pattern (infer.py:48-51,60-87): eval mode, no autograd, an empty-x extra iteration."""
    from trackmpnn_amd import TrackMPNN
    cfg = orc.OracleConfig('2d', 3, 64, 0, 'diff')
    plans, xs = _batched_case(B=3, frames=4, mean=4, max_dets=8, F=8, seed0=7)
    p = orc.random_params(cfg, seed=2, scale=0.2)
    model = TrackMPNN('2d', 3, 64, 0, 'diff')
    model.load_state_dict({k: v.clone() for k, v in p.items()})
    model = model.to(DEV).eval()
    h = h_ref = None
    with torch.no_grad():
        for plan, x in zip(plans, xs):
            s_ref, l_ref, h_ref, _ = orc.forward(p, cfg, x, h_ref, _oracle_graph(plan.graph), training=False)
            s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV))
            assert (s.cpu() - s_ref).abs().max().item() <= SCORE_TOL
        # extra message-passing iteration with no new rows (track_mpnn.py:67-68)
        from trackmpnn_amd import plan_single
        plan0 = plan_single(plans[-1].graph.to(DEV), 0)
        s_ref, l_ref, h_ref, _ = orc.forward(p, cfg, xs[0][:0], h_ref, _oracle_graph(plans[-1].graph), training=False)
        s, l, h, _ = model.forward_graph(xs[0][:0].to(DEV), h, plan0)
        assert (s.cpu() - s_ref).abs().max().item() <= SCORE_TOL
        assert torch.allclose(h.cpu(), h_ref, atol=LOGIT_ATOL, rtol=LOGIT_RTOL)


def test_single_row_batchnorm_raises():
    from trackmpnn_amd import TrackMPNN, graph_from_edges, plan_single
    model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).train()
    g = graph_from_edges(1, torch.zeros(1, dtype=torch.bool), torch.zeros(0), torch.zeros(0), device=DEV)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        model.forward_graph(torch.randn(1, 8, device=DEV), None, plan_single(g, 1))


def test_aggregation_properties_at_scale():
    """Size-independent properties of rows E/F on a graph far larger than the oracle can chew:
    <gather(h), m> == <h, gather^T(m)>  (the two kernels are exact adjoints), linearity, and
    bitwise run-to-run reproducibility (no float atomics)."""
    from trackmpnn_amd import _lib
    from trackmpnn_amd import WindowBuilder, batch_windows, synth_window
    wins = [WindowBuilder(synth_window(s, 7, 6, 20)).calls() for s in range(64)]
    plans, _ = batch_windows(wins * 32, static=True)           # 2048 windows, ~0.5 M rows
    g = plans[-1].graph.to(DEV)
    H = 64
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=DEV).manual_seed(0)
    h = torch.randn(g.N, H, device=DEV, generator=gen)
    m = torch.randn(g.N, H, device=DEV, generator=gen)
    h[g.edge_row.long()] = 0            # gather reads det rows only
    m[g.det_row.long()] = 0             # its adjoint reads edge rows only
    out = torch.zeros(g.N, H, device=DEV)
    _lib.call('tmpnn_gather_diff_fwd', g.cref(), h.data_ptr(), H, out.data_ptr(), H, H, 0, st)
    adj = torch.zeros(g.N, H, device=DEV)
    _lib.call('tmpnn_gather_diff_bwd', g.cref(), m.data_ptr(), H, adj.data_ptr(), H, H, 0, st)
    lhs = (out.double() * m.double()).sum().item()
    rhs = (h.double() * adj.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * max(1.0, abs(lhs))
    # segsum (row F) is the adjoint of "gather on gradients" as well
    es = torch.zeros(g.N, H, device=DEV)
    h2 = torch.randn(g.N, H, device=DEV, generator=gen)
    _lib.call('tmpnn_segsum_fwd', g.cref(), h2.data_ptr(), H, es.data_ptr(), H, H, 0, 0, st)
    es2 = torch.zeros(g.N, H, device=DEV)
    _lib.call('tmpnn_segsum_fwd', g.cref(), h2.data_ptr(), H, es2.data_ptr(), H, H, 0, 0, st)
    assert torch.equal(es, es2)                                   # bitwise reproducible
    es3 = torch.zeros(g.N, H, device=DEV)
    h3 = (2.0 * h2).contiguous()
    _lib.call('tmpnn_segsum_fwd', g.cref(), h3.data_ptr(), H, es3.data_ptr(), H, H, 0, 0, st)
    assert torch.equal(es3, 2.0 * es)                             # exact linearity under power-of-two scaling
    # sum over dets of es == sum over edges of (h[e] - h[e]) == 0 column-wise: every edge enters once with + and once with -
    col = es.double().sum(0)
    assert col.abs().max().item() <= 1e-6 * h2.double().abs().sum(0).max().item()
    # the visiting order (tmpnn_graph.det_order, set by batch_windows) only changes the access pattern, never a bit
    assert g.det_order is not None and torch.equal(torch.sort(g.det_order.long()).values, torch.arange(g.Dn, device=DEV))
    saved = g.det_order
    g.det_order, g._c = None, None
    es4 = torch.zeros(g.N, H, device=DEV)
    _lib.call('tmpnn_segsum_fwd', g.cref(), h2.data_ptr(), H, es4.data_ptr(), H, H, 0, 0, st)
    g.det_order, g._c = torch.flip(saved, [0]).contiguous(), None
    es5 = torch.zeros(g.N, H, device=DEV)
    _lib.call('tmpnn_segsum_fwd', g.cref(), h2.data_ptr(), H, es5.data_ptr(), H, H, 0, 0, st)
    g.det_order, g._c = saved, None
    assert torch.equal(es, es4) and torch.equal(es, es5)


def test_full_bench_size_tiling_invariance():
    """BASELINE C2 at the full bench size (16 384 windows, 6.8 M rows, 18.7 M edge-iterations): the batch is 64
    distinct windows tiled 256 times with identical features, and windows are independent (block-diagonal graph,
    per-window BatchNorm), so every copy must reproduce its original bit for bit -- scores of all six rolling calls --
    and the parameter gradients must be 256 x those of the 64-window batch.  Size-independent, no oracle needed."""
    import torch.nn.functional as Fnn
    from trackmpnn_amd import TrackMPNN, WindowBuilder, batch_windows, synth_window
    distinct, reps, F, H = 64, 256, 8, 64
    wins = [WindowBuilder(synth_window(1000 + s, 7, 6.0, 20)).calls() for s in range(distinct)]
    table = torch.randn(distinct, 512, F, generator=torch.Generator().manual_seed(3))      # features by (seed, det id)

    def run(B):
        plans, refs = batch_windows((wins * (B // distinct))[:B], device='cpu')
        torch.manual_seed(11)
        model = TrackMPNN('2d', F - 5, H, 0, 'diff').to(DEV).train()
        h, loss, outs = None, 0.0, []
        row_window = torch.empty(plans[-1].graph.N, dtype=torch.long)
        for c, (plan, ref) in enumerate(zip(plans, refs)):
            ref = torch.from_numpy(ref)
            assert int(ref[:, 1].max()) < table.shape[1]
            x = torch.zeros(plan.n_new, F)
            x[plan.new_det_local] = table[ref[:, 0] % distinct, ref[:, 1]]
            row_window[plan.new_det_row.long()] = ref[:, 0]
            pd = plan.to(DEV)
            nxt = plans[c + 1].n_new if c + 1 < len(plans) else 0
            scores, logits, h, _ = model.forward_graph(x.to(DEV), h, pd, reserve_rows=nxt)
            loss = loss + (Fnn.softplus(logits) * 0.5).sum()        # a loss that does not depend on the row position
            outs.append(scores.detach())
        g = plans[-1].graph
        row_window[g.edge_row.long()] = row_window[g.src.long()]
        loss.backward()
        grads = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).double().cpu()
        return plans, outs, row_window, grads

    plans, outs, row_window, grads_full = run(distinct * reps)
    assert plans[-1].graph.N > 6_000_000
    rw = row_window.to(DEV)
    for c, sc in enumerate(outs):
        n = sc.numel()
        w = rw[:n]
        order = torch.argsort(w, stable=True)
        ws, vs = w[order], sc[order]
        cnt = torch.bincount(ws, minlength=distinct * reps)
        start = torch.cumsum(cnt, 0) - cnt
        posw = torch.arange(n, device=DEV) - start[ws]
        assert torch.equal(cnt, cnt[:distinct].repeat(reps)), f'call {c}: copies differ in size'
        ref_idx = start[ws % distinct] + posw
        assert torch.equal(vs, vs[ref_idx]), f'call {c}: a tiled copy differs from its original'
    _, _, _, grads_small = run(distinct)
    err = (grads_full - reps * grads_small).abs().max().item()
    assert err <= 2e-4 * (reps * grads_small).abs().max().item(), err


def test_inplace_append_is_bitwise_identical():
    """reserve_rows (carried state extended in place, no copy) must not change a single bit, fwd or bwd."""
    from trackmpnn_amd import TrackMPNN
    plans, xs = _batched_case(B=8, frames=6, mean=5, max_dets=12, F=8, seed0=3)
    outs = []
    for reserve in (False, True):
        torch.manual_seed(5)
        model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).train()
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(DEV))
        h = None
        loss = 0.0
        for c, (plan, x) in enumerate(zip(plans, xs)):
            nxt = plans[c + 1].n_new if (reserve and c + 1 < len(plans)) else 0
            s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV), reserve_rows=nxt)
            loss = loss + (l * l).sum() + s.sum()
        loss.backward()
        outs.append((h.detach().clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('heads', [0, 2])
def test_inplace_param_grad_accumulation_matches_returned_grads(heads):
    """With `inplace_param_grads` (opt-in; set by GradBucket) and p.grad buffers in place the kernels add each call's
    parameter gradients straight into them and autograd gets None; without, the per-call tensors are returned and autograd adds
    them.  Same kernels; only the association of the per-call sums changes (a parameter that receives two partial sums
    per call sees (prev + a) + b instead of prev + (a + b)), so the results agree to fp32 rounding, and a second
    backward accumulates on top (2 x)."""
    from trackmpnn_amd import TrackMPNN
    plans, xs = _batched_case(B=6, frames=5, mean=4, max_dets=10, F=8, seed0=11)
    results = []
    for preallocate in (False, True):
        torch.manual_seed(5)
        model = TrackMPNN('2d', 3, 64, heads, 'diff').to(DEV).train()
        if preallocate:
            model.inplace_param_grads = True          # opt-in (what GradBucket sets); off by default
            for p in model.parameters():
                p.grad = torch.zeros_like(p)
        reps = 2 if preallocate else 1
        for _ in range(reps):
            torch.manual_seed(77)                     # same attention dropout draw in every run
            h, loss = None, 0.0
            for plan, x in zip(plans, xs):
                s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV))
                loss = loss + (l * l).sum() + s.sum()
            loss.backward()
            if len(results) < 2:
                results.append([p.grad.clone() for p in model.parameters()])
        if preallocate:
            final = [p.grad.clone() for p in model.parameters()]
    scale = max(float(a.abs().max()) for a in results[0])
    for a, b in zip(results[0], results[1]):
        assert float((a - b).abs().max()) <= 2e-6 * max(float(a.abs().max()), 1e-3 * scale)
    for a, b in zip(results[1], final):
        # (the pre-BatchNorm bias has a zero true gradient: what it holds is cancellation noise, so compare at the
        #  scale of the largest gradient)
        assert float((2 * a - b).abs().max()) <= 4e-6 * max(float(a.abs().max()), 1e-3 * scale)


def test_fused_backward_matches_two_kernel_backward(monkeypatch):
    """tmpnn_gru_bwd_fused (opt-in) gives the gradients of the default two-kernel backward."""
    import trackmpnn_amd.functional as F
    from trackmpnn_amd import TrackMPNN
    plans, xs = _batched_case(B=8, frames=6, mean=5, max_dets=12, F=8, seed0=11)
    outs = []
    for fused in (False, True):
        monkeypatch.setattr(F, 'FUSED_BWD', fused)
        torch.manual_seed(5)
        model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).train()
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(DEV))
        h = None
        loss = 0.0
        for plan, x in zip(plans, xs):
            s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV))
            loss = loss + (l * l).sum() + s.sum()
        loss.backward()
        outs.append([p.grad.clone() for p in model.parameters()])
    gmax = max(g.abs().max().item() for g in outs[0])
    for a, b in zip(outs[0], outs[1]):
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, gmax)


def test_ragged_graph_after_row_deletion_vs_oracle():
    """Inference pattern (infer.py:82-87, utils/graph.py:492-520): decode_tracks deletes the oldest frames'
    rows from states / node_adj, leaving a ragged graph (dets that lost all their past edges, uneven runs).
    Emulated by deleting whole det rows + their incident edge rows from a batched graph; HIP vs oracle, eval."""
    from trackmpnn_amd import TrackMPNN, graph_from_edges, plan_single
    plans, xs = _batched_case(B=4, frames=6, mean=5, max_dets=10, F=8, seed0=21)
    g = plans[-1].graph
    N = g.N
    rng = np.random.RandomState(0)
    is_edge = g.is_edge.numpy().astype(bool)
    det_rows = g.det_row.numpy()
    drop_det = set(det_rows[rng.rand(det_rows.size) < 0.3].tolist())
    src, dst, er = g.src.numpy(), g.dst.numpy(), g.edge_row.numpy()
    drop = np.zeros(N, bool)
    drop[list(drop_det)] = True
    drop[er[np.isin(src, list(drop_det)) | np.isin(dst, list(drop_det))]] = True
    drop[er[rng.rand(er.size) < 0.2]] = True                      # plus some pruned low-probability edges
    lone = [d for d in det_rows.tolist() if d not in drop_det][3]   # and one det that keeps no edge at all
    drop[er[(src == lone) | (dst == lone)]] = True
    keep = np.nonzero(~drop)[0]
    remap = -np.ones(N, np.int64)
    remap[keep] = np.arange(keep.size)
    ek = ~drop[er]
    g2 = graph_from_edges(keep.size, torch.from_numpy(is_edge[keep]), torch.from_numpy(remap[src[ek]]),
                          torch.from_numpy(remap[dst[ek]]))
    assert (g2.rowptr[1:] - g2.rowptr[:-1]).min().item() == 0       # some dets are isolated now
    cfg = orc.OracleConfig('2d', 3, 64, 2, 'diff')                 # attention too: isolated dets have an empty softmax
    p = orc.random_params(cfg, seed=4, scale=0.15)
    model = TrackMPNN('2d', 3, 64, 2, 'diff')
    model.load_state_dict({k: v.clone() for k, v in p.items()})
    model = model.to(DEV).eval()
    h0 = torch.randn(keep.size, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        s_ref, l_ref, h_ref, a_ref = orc.forward(p, cfg, torch.zeros(0, 8), h0, _oracle_graph(g2), training=False)
        s, l, h, att = model.forward_graph(torch.zeros(0, 8, device=DEV), h0.to(DEV), plan_single(g2.to(DEV), 0))
    assert (s.cpu() - s_ref).abs().max().item() <= SCORE_TOL
    assert torch.allclose(h.cpu(), h_ref, atol=LOGIT_ATOL, rtol=LOGIT_RTOL)
    for k in range(2):
        assert torch.allclose(att[0][k].per_edge().cpu(), a_ref[0][k], atol=1e-5, rtol=1e-4)


# ------------------------------------------------------------------------------------------------------------------
# round 2: the remaining BASELINE.json configs as workloads (C3, C4, C5) and the reference's inference loop
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,frames,mean,max_dets,ncat,pscale', [
    ('C3 KITTI All / CenterTrack, cur-win 10', 12, 8.0, 25, 3, 0.05),
    ('C4 BDD100K All / libra, cur-win 5', 7, 12.0, 40, 8, 0.07),
])
def test_baseline_workloads_vs_oracle(tag, frames, mean, max_dets, ncat, pscale):
    """BASELINE.json configs[2] / configs[3] as workloads (12-frame windows, D_t ~ clip(Poisson(8),
    1, 25); C4: 7 frames, D_t ~ clip(Poisson(12), 1, 40), F = 13): B = 16 rolling windows batched block-diagonally,
    forward of every call and one backward, HIP vs the oracle.  (pscale: the random model is a recurrence over up to
    11 calls; at weight scale 0.1 the fp32 oracle itself drifts 1e-3 from its fp64 evaluation by call 10, so the
    longer chain uses a better conditioned model -- measured drift <= 4e-5 at these scales.)"""
    from trackmpnn_amd import TrackMPNN
    H = 64
    cfg = orc.OracleConfig('2d', ncat, H, 0, 'diff')
    F = ncat + 5
    plans, xs = _batched_case(B=16, frames=frames, mean=mean, max_dets=max_dets, F=F, seed0=300 + frames)
    assert len(plans) == frames - 1 and plans[-1].graph.E > 4000
    p = orc.random_params(cfg, seed=frames, scale=pscale)
    model = TrackMPNN('2d', ncat, H, 0, 'diff')
    model.load_state_dict({k: v.clone() for k, v in p.items()}, strict=True)
    model = model.to(DEV).train()
    pr = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and 'running' not in k else v.clone())
          for k, v in p.items()}
    h = h_ref = None
    loss = loss_ref = 0.0
    gen = torch.Generator().manual_seed(1)
    for c, (plan, x) in enumerate(zip(plans, xs)):
        s_ref, l_ref, h_ref, _ = orc.forward(pr, cfg, x, h_ref, _oracle_graph(plan.graph), training=True,
                                             seg_ids=plan.seg_of_new)
        nxt = plans[c + 1].n_new if c + 1 < len(plans) else 0
        s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV), reserve_rows=nxt)
        assert (s.detach().cpu() - s_ref.detach()).abs().max().item() <= SCORE_TOL, (tag, c)
        assert torch.allclose(l.detach().cpu(), l_ref.detach(), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), (tag, c)
        assert torch.allclose(h.detach().cpu(), h_ref.detach(), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), (tag, c)
        w = torch.randn(l.shape, generator=gen)
        loss = loss + (w.to(DEV) * l).sum() + s.sum()
        loss_ref = loss_ref + (w * l_ref).sum() + s_ref.sum()
    loss.backward()
    loss_ref.backward()
    gscale = max(1.0, max(v.grad.abs().max().item() for v in pr.values() if v.grad is not None))
    for k, prm in model.named_parameters():
        tol = GRAD_RTOL * gscale * (10 if (k.endswith('.0.bias') and k.startswith('input_')) else 1)
        err = (prm.grad.cpu() - pr[k].grad).abs().max().item()
        assert err <= tol, f'{tag}: grad {k}: {err} > {tol}'


def test_c5_dense_stress_full_size():
    """BASELINE.json configs[4] (C5) at FULL size: one static window of 50 frames x 300 dets (Dn = 15 000,
    E = 4 410 000, N = 4 425 000), H = 256, 4 message-passing iterations, forward + backward.  The reference cannot
    hold this graph (dense N x N), so the checks are size-independent: (1) two tiny dense windows ride in the same
    block-diagonal batch and must agree with the oracle run on them alone (scores of all 4 iterations, and their
    d loss / d x); (2) the whole step re-run gives bit-identical scores and gradients; (3) the aggregation kernels
    are exact adjoints at H = 256 on the 4.4 M-edge graph."""
    from trackmpnn_amd import TrackMPNN, _lib, concat_static_graphs, dense_static_graph, plan_single
    H, F, iters = 256, 8, 4
    small = [dense_static_graph(4, 5), dense_static_graph(3, 7)]
    big = dense_static_graph(50, 300)
    assert (big.Dn, big.E, big.N) == (15000, 4410000, 4425000)
    graph, plan0 = concat_static_graphs([big] + small)
    graph = graph.to(DEV)
    plan0 = plan0.to(DEV)
    planr = plan_single(graph, 0)
    cfg = orc.OracleConfig('2d', 3, H, 0, 'diff')
    p = orc.random_params(cfg, seed=9, scale=1.2 / (H ** 0.5))
    gen = torch.Generator().manual_seed(4)
    x = torch.zeros(graph.N, F)
    x[graph.det_row.cpu().long()] = torch.randn(graph.Dn, F, generator=gen)
    w_small = torch.randn(graph.N - big.N, 1, generator=gen)

    def run():
        model = TrackMPNN('2d', 3, H, 0, 'diff')
        model.load_state_dict({k: v.clone() for k, v in p.items()}, strict=True)
        model = model.to(DEV).train()
        xd = x.to(DEV).requires_grad_(True)
        h, loss, outs = None, 0.0, []
        for it in range(iters):
            s, l, h, _ = model.forward_graph(xd if it == 0 else xd[:0], h, plan0 if it == 0 else planr)
            # a loss that couples nothing across windows: mean over the big window, weighted sum over the small ones
            loss = loss + l[:big.N].mean() + (w_small.to(DEV) * l[big.N:]).sum()
            outs.append(s.detach())
        loss.backward()
        grads = torch.cat([q.grad.reshape(-1) for q in model.parameters()])
        return outs, xd.grad.detach(), grads

    outs, gx, grads = run()
    assert all(bool(torch.isfinite(o).all()) for o in outs) and bool(torch.isfinite(grads).all())
    # (1) the small windows against the oracle (their own BatchNorm segments => independent of the big window)
    off = big.N
    for i, g in enumerate(small):
        pr = {k: v.clone() for k, v in p.items()}
        xs = x[off:off + g.N].clone().requires_grad_(True)
        h_ref, loss_ref = None, 0.0
        for it in range(iters):
            s_ref, l_ref, h_ref, _ = orc.forward(pr, cfg, xs if it == 0 else xs[:0], h_ref, _oracle_graph(g),
                                                 training=True)
            got = outs[it][off:off + g.N].cpu()
            assert (got - s_ref.detach()).abs().max().item() <= SCORE_TOL, (i, it)
            loss_ref = loss_ref + (w_small[off - big.N:off - big.N + g.N] * l_ref).sum()
        loss_ref.backward()
        det = ~torch.from_numpy(g.is_edge.cpu().numpy().astype(bool))
        ref = xs.grad[det]
        assert torch.allclose(gx[off:off + g.N].cpu()[det], ref, atol=GRAD_RTOL * max(1.0, ref.abs().max().item()), rtol=0)
        off += g.N
    # (2) bitwise reproducible at full size
    outs2, gx2, grads2 = run()
    for a, b in zip(outs, outs2):
        assert torch.equal(a, b)
    assert torch.equal(grads, grads2) and torch.equal(gx, gx2)
    del outs, outs2, gx2, grads2
    torch.cuda.empty_cache()
    # (3) rows E / F are each other's adjoints at H = 256
    st = torch.cuda.current_stream().cuda_stream
    gd = torch.Generator(device=DEV).manual_seed(0)
    hh = torch.randn(graph.N, H, device=DEV, generator=gd)
    mm = torch.randn(graph.N, H, device=DEV, generator=gd)
    hh[graph.edge_row.long()] = 0
    mm[graph.det_row.long()] = 0
    out = torch.zeros(graph.N, H, device=DEV)
    adj = torch.zeros(graph.N, H, device=DEV)
    _lib.call('tmpnn_gather_diff_fwd', graph.cref(), hh.data_ptr(), H, out.data_ptr(), H, H, 0, st)
    _lib.call('tmpnn_gather_diff_bwd', graph.cref(), mm.data_ptr(), H, adj.data_ptr(), H, H, 0, st)
    lhs = (out.double() * mm.double()).sum().item()
    rhs = (hh.double() * adj.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * max(1.0, abs(lhs))


@pytest.mark.parametrize('name', __import__('tests.conftest', fromlist=['x']).infer_golden_names())
def test_golden_inference_loop_parity(name):
    """The reference's inference loop (infer.py:48-87) captured call by call from the real reference: eval mode,
    graphs from update_graph(mode='test'), carried state with the rows decode_tracks deleted (utils/graph.py:492-520).
    Each call goes through the drop-in forward(x, h_in, node_adj, edge_adj) with the reference's own tensors."""
    gold = Golden(name)
    model = build_model(gold.meta, gold.params())
    with torch.no_grad():
        for c in range(gold.ncalls):
            na = gold.adjacency(c, 'node_adj', DEV)
            ea = gold.adjacency(c, 'edge_adj', DEV)
            h_in = gold.t(f'c{c}/h_in').to(DEV) if int(gold.d[f'c{c}/has_h_in']) else None
            scores, logits, h, att = model(gold.t(f'c{c}/x').to(DEV), h_in, na, ea)
            assert (scores.cpu() - gold.t(f'c{c}/scores')).abs().max().item() <= SCORE_TOL, f'scores call {c}'
            assert torch.allclose(logits.cpu(), gold.t(f'c{c}/logits'), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), c
            assert torch.allclose(h.cpu(), gold.t(f'c{c}/h_out'), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), c


def test_default_backward_honours_the_autograd_contract():
    """Default mode (no GradBucket, TMPNN_INPLACE_GRADS unset): parameter gradients are RETURNED to autograd even when
    p.grad buffers exist, so torch.autograd.grad, tensor hooks and post-accumulate hooks behave as for any module."""
    from trackmpnn_amd import TrackMPNN
    plans, xs = _batched_case(B=3, frames=4, mean=4, max_dets=8, F=8, seed0=5)
    torch.manual_seed(5)
    model = TrackMPNN('2d', 3, 64, 0, 'diff').to(DEV).train()
    assert model.inplace_param_grads is False
    params = list(model.parameters())
    for p in params:
        p.grad = torch.full_like(p, 7.0)
    fired = []
    hook = params[0].register_hook(lambda g: fired.append(g.shape))

    def loss_of():
        h, loss = None, 0.0
        for plan, x in zip(plans, xs):
            s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV))
            loss = loss + (l * l).sum() + s.sum()
        return loss

    grads = torch.autograd.grad(loss_of(), params)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert all(bool((p.grad == 7.0).all()) for p in params)          # autograd.grad must not touch .grad
    assert fired                                                     # tensor hooks fire
    for p in params:
        p.grad.zero_()
    loss_of().backward()                                             # autograd adds the returned gradients into .grad
    gscale = max(float(g.abs().max()) for g in grads)
    for p, g in zip(params, grads):
        assert float((p.grad - g).abs().max()) <= 1e-5 * gscale
    hook.remove()


def test_gradients_bitwise_equal_across_processes():
    """The C ABI is pure enqueue (tmpnn.h: nothing is measured or decided inside a call), so two FRESH processes
    running the same step -- more than 2^20 edge rows, the size at which round 1's hidden autotune kicked in -- must
    produce bit-identical scores and parameter gradients."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = []
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.join(root, 'tests', 'gpu_grad_digest.py')], cwd=root,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('GRAD_DIGEST')]
        assert line, r.stdout[-1500:]
        digests.append(line[-1])
    assert digests[0] == digests[1]


@pytest.mark.parametrize('R', [1, 31, 32, 33, 255, 2048, 2049, 4097, 8191 + 32 * 300])
def test_one_pass_backward_ragged_sizes_match_the_two_kernels(R):
    """tmpnn_gru_bwd_fused (one read of the gates) against tmpnn_gru_bwd_data + tmpnn_gru_bwd_weights on row counts
    around its tile (32 rows), pipeline (prologue stages tile 0 and requests tile 1) and grid (256 persistent blocks)
    boundaries, and on both sides of the 64 -> 65 slabs at which the weight-gradient slabs are folded before the final reduce
    (R = 2048 / 2049): every xmode (the concat cell, xmode 2, with IN = 2H: d_msg and dW_ih 2H wide) / upstream / fused-adjoint
    variant, scattered row ids, outputs outside `rows` untouched."""
    from trackmpnn_amd import _lib
    lib = _lib.load()
    H = 64
    gen = torch.Generator().manual_seed(R)
    N = 2 * R + 7                                                   # rows of the state; `rows` is a scattered subset
    perm = torch.randperm(N, generator=gen)
    rows = perm[:R].sort().values.to(torch.int32).to(DEV)
    others = perm[R:]                                               # endpoints are never rows of the cell (dets vs edges)
    src = others[torch.randint(0, N - R, (R,), generator=gen)].to(torch.int32).to(DEV)
    dst = others[torch.randint(0, N - R, (R,), generator=gen)].to(torch.int32).to(DEV)
    r32 = lambda *s: torch.randn(*s, generator=gen).to(DEV)         # noqa: E731
    h, dout, dyv, w_head, msg = r32(N, H), r32(N, H), r32(N), r32(H), r32(R, H)
    gates = torch.cat([torch.sigmoid(r32(2, N, H)), torch.tanh(r32(1, N, H)), r32(1, N, H)], 0).contiguous()
    wih, whh = 0.3 * r32(3 * H, H), 0.3 * r32(3 * H, H)
    st = torch.cuda.current_stream().cuda_stream
    ws_b = max(f(R, IN, H) for f in (lib.tmpnn_gru_bwd_weights_ws, lib.tmpnn_gru_bwd_fused_ws) for IN in (H, 2 * H))
    ws = torch.empty(ws_b // 4 + 1, device=DEV)
    dmsg_init = r32(N, H)
    wih2, dmsg_init2 = 0.3 * r32(3 * H, 2 * H), r32(N, 2 * H)      # the concat cell: W_ih = [W1 | W2], d_msg [N][2H]
    for xmode in (0, 1, 2):
        if xmode == 2 and not lib.tmpnn_gru_bwd_fused_available(H, 2 * H, 2):
            assert os.environ.get('TMPNN_BWD_TWO') == '0' and os.environ.get('TMPNN_TEST_VARIANTS') == '1'
            continue                  # (a comparison build on its four-wave form: the concat halves exist in the eight-wave one only)
        IN, w_in, dm_init = (2 * H, wih2, dmsg_init2) if xmode == 2 else (H, wih, dmsg_init)
        for up in (1, 2, 3):
            for fuse in (False, True):
                if fuse and xmode == 0 and os.environ.get('TMPNN_TEST_VARIANTS', '0') != '1':
                    continue                                          # (compact messages + fused adjoint: variant builds only)
                dho = dout.data_ptr() if up & 1 else None
                dyp, whp = (dyv.data_ptr(), w_head.data_ptr()) if up & 2 else (None, None)
                sp, dp = (src.data_ptr(), dst.data_ptr()) if xmode else (None, None)
                mp = msg.data_ptr() if xmode == 0 else None
                outs = []
                inside = torch.isin(torch.arange(N, device=DEV), rows.long())
                base = torch.where(inside[:, None], torch.full((N, IN), 7.0, device=DEV), dm_init)
                for one_pass in (False, True):
                    dmsg = base.clone()
                    add = dmsg                                        # as the model calls it: the adjoint's table IS d_msg
                    dh = torch.full((N, H), 5.0, device=DEV)
                    gW = [torch.full((3 * H, IN), 0.5, device=DEV), torch.full((3 * H, H), 0.25, device=DEV),
                          torch.full((3 * H,), 1.0, device=DEV), torch.full((3 * H,), 2.0, device=DEV)]
                    fa = (src.data_ptr(), dst.data_ptr(), add.data_ptr()) if fuse else (None, None, None)
                    if one_pass:
                        _lib.call('tmpnn_gru_bwd_fused', rows.data_ptr(), R, xmode, sp, dp, mp, H, 1, IN, h.data_ptr(), H, H,
                                  w_in.data_ptr(), whh.data_ptr(), gates.data_ptr(), N * H, dho, H, dyp, whp,
                                  dmsg.data_ptr(), IN, dh.data_ptr(), H, fa[0], fa[1], fa[2], IN,
                                  gW[0].data_ptr(), gW[1].data_ptr(), gW[2].data_ptr(), gW[3].data_ptr(),
                                  ws.data_ptr(), ws.numel() * 4, st)
                    else:
                        _lib.call('tmpnn_gru_bwd_data', rows.data_ptr(), R, IN, h.data_ptr(), H, H, w_in.data_ptr(),
                                  whh.data_ptr(), gates.data_ptr(), N * H, dho, H, dyp, whp, dmsg.data_ptr(), IN,
                                  dh.data_ptr(), H, fa[0], fa[1], fa[2], IN, st)
                        _lib.call('tmpnn_gru_bwd_weights', rows.data_ptr(), R, xmode, sp, dp, mp, H, 1, IN, h.data_ptr(), H, H,
                                  gates.data_ptr(), N * H, dho, H, dyp, whp, gW[0].data_ptr(), gW[1].data_ptr(),
                                  gW[2].data_ptr(), gW[3].data_ptr(), ws.data_ptr(), ws.numel() * 4, st)
                    torch.cuda.synchronize()
                    outs.append((dmsg, dh, gW))
                (m0, h0, g0), (m1, h1, g1) = outs
                tag = (R, xmode, up, fuse)
                scale = max(1.0, float(h0.abs().max()), float(m0.abs().max()))
                assert float((m0 - m1).abs().max()) <= 2e-5 * scale, tag
                assert float((h0 - h1).abs().max()) <= 2e-5 * scale, tag
                for a, b in zip(g0, g1):
                    assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(a.abs().max())), tag
                assert bool((h1[~inside] == 5.0).all()) and bool((m1[~inside] == base[~inside]).all()), tag
                if R in (2048, 2049):
                    # both routes share the slab fold and the final reduce: at its switch, each against the weight gradients
                    # formed in fp64 from the same planes (the bound is the one above)
                    for got in (g0, g1):
                        for name, a, ref, b0 in zip(('dW_ih', 'dW_hh', 'db_ih', 'db_hh'), got,
                                                    _weight_grads_fp64(xmode, up, rows, src, dst, msg, h, gates, dout, dyv, w_head),
                                                    (0.5, 0.25, 1.0, 2.0)):
                            err, sc = float((a.double() - b0 - ref).abs().max()), max(1.0, float(ref.abs().max()))
                            assert err <= 2e-5 * sc, (tag, name, err, sc)


def _weight_grads_fp64(xmode, up, rows, src, dst, msg, h, gates, dout, dyv, w_head):
    """dW_ih, dW_hh, db_ih, db_hh of a GRU cell over `rows` in fp64, from the saved planes r, z, n, hn = W_hn h + b_hn:
    h' = (1 - z) n + z h with n = tanh(i_n + r hn); the message is msg (by list position), h[src] - h[dst] or [h[src] | h[dst]]."""
    d64 = lambda t: t.double()                                        # noqa: E731
    ro, s, d = rows.long(), src.long(), dst.long()
    r, z, n, hn = (d64(gates[k][ro]) for k in range(4))
    hp = d64(h[ro])
    dh = (d64(dout[ro]) if up & 1 else 0.0) + (d64(dyv[ro])[:, None] * d64(w_head)[None, :] if up & 2 else 0.0)
    x = d64(msg) if xmode == 0 else d64(h[s]) - d64(h[d]) if xmode == 1 else torch.cat([d64(h[s]), d64(h[d])], 1)
    dn = dh * (1 - z) * (1 - n * n)
    dz = dh * (hp - n) * z * (1 - z)
    dr = dn * hn * r * (1 - r)
    gi, gh = torch.cat([dr, dz, dn], 1), torch.cat([dr, dz, dn * r], 1)
    return gi.t() @ x, gh.t() @ hp, gi.sum(0), gh.sum(0)


@pytest.mark.parametrize('R', [4096, 4097])
def test_weight_gradient_alone_on_both_sides_of_the_slab_fold(R):
    """tmpnn_gru_bwd_weights on the generic kernel (H = 32, IN = 32: one slab per 64 rows) with 64 slabs, reduced directly, and
    65, folded 32:1 first: dW_ih, dW_hh, db_ih, db_hh added into non-zero buffers against an fp64 autograd of the cell,
    within the one-pass test's 2e-5 x scale."""
    from trackmpnn_amd import _lib
    lib = _lib.load()
    H = IN = 32
    gen = torch.Generator().manual_seed(R)
    r64 = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(DEV)      # noqa: E731
    x, h, dout = r64(R, IN), r64(R, H), r64(R, H)
    P = [(0.3 * r64(3 * H, IN)).requires_grad_(), (0.3 * r64(3 * H, H)).requires_grad_(),
         r64(3 * H).requires_grad_(), r64(3 * H).requires_grad_()]
    gi, gh = x @ P[0].t() + P[2], h @ P[1].t() + P[3]
    r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    ((1 - z) * n + z * h).mul(dout).sum().backward()
    f32 = lambda t: t.detach().float().contiguous()                                     # noqa: E731
    gates = torch.stack([f32(r), f32(z), f32(n), f32(gh[:, 2 * H:])]).contiguous()
    rows = torch.arange(R, dtype=torch.int32, device=DEV)
    xD, hD, doutD = f32(x), f32(h), f32(dout)
    got = [torch.full(tuple(p.shape), 0.5, device=DEV) for p in P]
    ws_b = lib.tmpnn_gru_bwd_weights_ws(R, IN, H)
    ws = torch.empty(ws_b // 4 + 1, device=DEV)
    _lib.call('tmpnn_gru_bwd_weights', rows.data_ptr(), R, 0, None, None, xD.data_ptr(), IN, 1, IN, hD.data_ptr(), H, H,
              gates.data_ptr(), R * H, doutD.data_ptr(), H, None, None, got[0].data_ptr(), got[1].data_ptr(),
              got[2].data_ptr(), got[3].data_ptr(), ws.data_ptr(), ws_b, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for name, a, p in zip(('dW_ih', 'dW_hh', 'db_ih', 'db_hh'), got, P):
        err, scale = float((a.double() - 0.5 - p.grad).abs().max()), max(1.0, float(p.grad.abs().max()))
        print(f'R={R} {name}: err {err:.3e} scale {scale:.3e}')
        assert err <= 2e-5 * scale, (R, name)


@pytest.mark.parametrize('H', [64, 256])
def test_split_products_are_fp32_accurate_on_wide_dynamic_range(H):
    """The "bf16x6" products (three bf16 pieces per fp32 operand, six bf16 MFMAs, fp32 accumulate) against an
    fp64 product on operands whose magnitudes span 2^-20 .. 2^20 within a row: error relative to sum |a||b| within
    4e-9 H + 3e-7 and no worse than 2 x torch's own fp32 matmul on the same data (+ 1e-7); Inf / NaN inputs give non-finite outputs
    in exactly the rows where an fp32 product does (an Inf comes out as NaN: its residual is Inf - Inf), and leave every
    other row's bits alone.  H = 64: tmpnn_rows_linear (k_rows_gemm_split); H = 256: the wide cells' projection
    (k_wide_gemm_store), read back from tmpnn_wide_gru_fwd's P."""
    from trackmpnn_amd import _lib
    torch.manual_seed(7 + H)
    R = 3000
    st = torch.cuda.current_stream().cuda_stream
    scale = lambda shape: torch.randn(shape, dtype=torch.float64) * torch.pow(2.0, torch.empty(shape, dtype=torch.float64).uniform_(-20, 20))
    a = scale((R, H)).float()
    w = scale((3 * H, H)).float()                    # weight [3H][H]; the product is a @ w^T
    rows = torch.arange(R, dtype=torch.int32, device=DEV)

    def product(a_host):
        aD, wD = a_host.to(DEV), w.to(DEV)
        out = torch.empty(R, 3 * H, device=DEV)
        if H == 64:
            wt = wD.t().contiguous()
            _lib.call('tmpnn_rows_linear', rows.data_ptr(), R, aD.data_ptr(), H, H, wt.data_ptr(), 3 * H, out.data_ptr(), 3 * H, st)
        else:
            lib = _lib.load()
            prep = torch.empty(int(lib.tmpnn_wide_prep_bytes(H, H)), dtype=torch.uint8, device=DEV)
            _lib.call('tmpnn_wide_prepare', wD.data_ptr(), wD.data_ptr(), H, H, prep.data_ptr(), st)
            # one edge row (row R) between dets 0 and 1: the call writes P = a @ w^T for the R det rows
            hh = torch.cat([aD, torch.zeros(1, H, device=DEV)])
            e_row = torch.tensor([R], dtype=torch.int32, device=DEV)
            z = torch.zeros(1, dtype=torch.int32, device=DEV)
            o = torch.ones(1, dtype=torch.int32, device=DEV)
            b = torch.zeros(3 * H, device=DEV)
            hout = torch.empty(R + 1, H, device=DEV)
            _lib.call('tmpnn_wide_gru_fwd', prep.data_ptr(), rows.data_ptr(), R, e_row.data_ptr(), 1, z.data_ptr(), o.data_ptr(),
                      hh.data_ptr(), H, H, b.data_ptr(), b.data_ptr(), out.data_ptr(), hout.data_ptr(), H, None, 0, st)
        torch.cuda.synchronize()
        return out.cpu()

    got = product(a)
    ref64 = a.double() @ w.double().t()
    denom = a.double().abs() @ w.double().abs().t()
    err = ((got.double() - ref64).abs() / denom).max().item()
    err_torch = (((a @ w.t()).double() - ref64).abs() / denom).max().item()
    # fp32 accumulation over K = H products: the bound grows with K (observed 3.4e-7 / 6.8e-7 for torch at 64 / 256)
    assert err <= 4e-9 * H + 3e-7 and err <= 2.0 * err_torch + 1e-7, (err, err_torch)
    # non-finite inputs
    a2 = a.clone()
    a2[5, 3] = float('inf')
    a2[17, 0] = float('nan')
    a2[40, H - 1] = -float('inf')
    got2 = product(a2)
    bad = ~torch.isfinite(a2 @ w.t()).all(1)
    assert bad.sum() == 3 and bool((~torch.isfinite(got2[bad])).all())
    assert torch.equal(got2[~bad], got[~bad])


# ------------------------------------------------------------------------------------------------------------------
# round 6: the two thin spots of the round-5 review
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', ['bench_init', 'perturbed'])
def test_bench_own_windows_vs_oracle(weights):
    """The headline batch itself against the oracle: bench.build_batch's 64 DISTINCT windows of rank 0 (seeds 1000..1063,
    its own feature stream and BCE targets), B = 64 block-diagonal with per-window BatchNorm segments, the six rolling
    calls + one backward exactly as bench.step issues them -- (a) with the model bench.py times (torch.manual_seed(5)
    initial weights), (b) with those weights perturbed by 0.1 N(0,1) so that scores leave the +-4.595 plateau and an error
    anywhere would show.  bench.py's 16 384 windows are these 64 tiled 256 x (test_full_bench_size_tiling_invariance pins
    the tiling)."""
    import torch.nn.functional as Fnn
    import bench
    from trackmpnn_amd import TrackMPNN
    from trackmpnn_amd.loss import bce_with_logits_sum
    frames, mean_dets, max_dets, F, H = 7, 6.0, 20, 8, 64            # bench.main's workload constants
    plans, xs, edge_iters = bench.build_batch(64, frames, mean_dets, max_dets, F, seed=1, device='cpu')
    assert len(plans) == 6 and edge_iters > 60000
    gen = torch.Generator().manual_seed(0)                           # bench.main: targets from Generator(rank)
    targets = [(torch.rand(p.graph.N, 1, generator=gen) < 0.3).float() for p in plans]
    torch.manual_seed(5)
    model = TrackMPNN('2d', 3, H, 0, 'diff')
    if weights == 'perturbed':
        gp = torch.Generator().manual_seed(77)
        with torch.no_grad():
            for prm in model.parameters():
                prm.add_(0.1 * torch.randn(prm.shape, generator=gp))
    p = {k: v.clone() for k, v in model.state_dict().items()}
    cfg = orc.OracleConfig('2d', 3, H, 0, 'diff')
    pr = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and 'running' not in k else v.clone())
          for k, v in p.items()}
    model = model.to(DEV).train()
    h = h_ref = None
    loss = loss_ref = 0.0
    for c, (plan, x, t) in enumerate(zip(plans, xs, targets)):
        s_ref, l_ref, h_ref, _ = orc.forward(pr, cfg, x, h_ref, _oracle_graph(plan.graph), training=True,
                                             seg_ids=plan.seg_of_new)
        nxt = plans[c + 1].n_new if c + 1 < len(plans) else 0
        s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV), reserve_rows=nxt)
        assert (s.detach().cpu() - s_ref.detach()).abs().max().item() <= SCORE_TOL, c
        assert torch.allclose(l.detach().cpu(), l_ref.detach(), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), c
        assert torch.allclose(h.detach().cpu(), h_ref.detach(), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), c
        loss = loss + bce_with_logits_sum(l, t.to(DEV))                  # (bench.step's loss; the oracle side: torch's)
        loss_ref = loss_ref + Fnn.binary_cross_entropy_with_logits(l_ref, t, reduction='sum')
    assert abs(loss.item() - loss_ref.item()) <= 2e-5 * abs(loss_ref.item())
    loss.backward()
    loss_ref.backward()
    gscale = max(1.0, max(v.grad.abs().max().item() for v in pr.values() if v.grad is not None))
    for k, prm in model.named_parameters():
        tol = GRAD_RTOL * gscale * (10 if (k.endswith('.0.bias') and k.startswith('input_')) else 1)
        err = (prm.grad.cpu() - pr[k].grad).abs().max().item()
        assert err <= tol, f'grad {k}: {err} > {tol}'
    for k, b in model.named_buffers():
        if b.dtype.is_floating_point:
            assert torch.allclose(b.cpu(), pr[k], atol=1e-5, rtol=1e-4), k


@pytest.mark.parametrize('name', ['roll_2d_diff_k2_train', 'roll_2d-temp-vis_concat_k2_train'])
def test_self_drawn_attention_dropout_through_the_drop_in_call(name):
    """Train mode with attention heads through model(x, h, node_adj, edge_adj) -- the mask drawn by the implementation
    itself (functional._keep_bits; the reference's dense bernoulli stream cannot be replayed, models/layers.py:37).  The
    drawn mask is recovered from the returned attention (a dropped position is exactly 0) and the call is pinned three ways:
    (1) the SAME call with that mask injected (forward_dgraph(dropout_keep=...)) gives h_out, scores and attention bit for
    bit, and the staged kernels (forward_graph) agree within the parity tolerance; (2) against the all-kept run every kept
    weight is bit-equal and every dropped one 0 -- so dropping only zeroes, and the all-kept weights are 2 x the softmax
    (1 / (1 - p), checked against the oracle); (3) the oracle with the recovered mask reproduces scores, state and, after
    one backward over the whole sequence, every parameter gradient."""
    from trackmpnn_amd import graph_from_adjacency, plan_single
    from trackmpnn_amd.graph import device_graph_from_adjacency
    gold = Golden(name)
    meta = gold.meta
    K = meta['nattheads']
    model = build_model(meta, gold.params())
    G = len(model.feature_idx)
    cfg = orc.OracleConfig(meta['features'], meta['ncategories'], meta['nhidden'], K, meta['msg_type'])
    pr = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and 'running' not in k else v.clone())
          for k, v in gold.params().items()}
    bufs0 = None
    h = h_ref = None
    loss = loss_ref = 0.0
    masks_all = [[] for _ in range(K)]
    for c in range(gold.ncalls):
        na, ea = gold.adjacency(c, 'node_adj', DEV), gold.adjacency(c, 'edge_adj', DEV)
        x = gold.t(f'c{c}/x')
        og = orc.graph_from_adjacency(gold.adjacency(c, 'node_adj'), gold.adjacency(c, 'edge_adj'))
        bufs0 = {k: b.clone() for k, b in model.named_buffers()}       # (train-mode calls move the running statistics)
        h_prev = None if h is None else h.detach().clone()
        scores, logits, h, att = model(x.to(DEV), h, na, ea)
        after = {k: b.clone() for k, b in model.named_buffers()}
        graph = graph_from_adjacency(na, ea)
        e_idx, ep_idx = graph.inc_edge_endpoint()
        E = graph.E
        keep_csr, keep_orc = [], []
        for g in range(G):
            a_tr = torch.stack([att[g][k].alpha for k in range(K)])          # [K, 2E] CSR order
            keep_csr.append((a_tr != 0).to(torch.uint8))
            pe = torch.stack([att[g][k].per_edge() for k in range(K)])       # [K, E, 2] oracle layout
            keep_orc.append((pe != 0).float().cpu())
            for k in range(K):
                masks_all[k].append(keep_csr[g][k].flatten().cpu())

        def rerun(fn, keep):
            with torch.no_grad():
                for k_, b in model.named_buffers():
                    b.copy_(bufs0[k_])
            with torch.no_grad():
                out = fn(keep)
            for k_, b in model.named_buffers():
                with torch.no_grad():
                    b.copy_(after[k_])
            return out
        # (1) the drawn mask injected: same path bit for bit, staged kernels within tolerance
        dg = device_graph_from_adjacency(na, ea, torch.device(DEV))
        s2, l2, h2, att2 = rerun(lambda kp: model.forward_dgraph(x.to(DEV), h_prev, dg, dropout_keep=kp), keep_csr)
        assert torch.equal(h2, h.detach()) and torch.equal(s2, scores.detach()) and torch.equal(l2, logits.detach()), c
        for g in range(G):
            for k in range(K):
                assert torch.equal(att2[g][k].alpha, att[g][k].alpha), (c, g, k)
        s3, l3, h3, _ = rerun(lambda kp: model.forward_graph(x.to(DEV), h_prev, plan_single(graph, x.shape[0]),
                                                             dropout_keep=kp), keep_csr)
        assert (s3 - scores.detach()).abs().max().item() <= SCORE_TOL
        assert torch.allclose(h3, h.detach(), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), c
        # (2) against the all-kept run: dropping only zeroes
        ones = [torch.ones_like(kc) for kc in keep_csr]
        _, _, _, att_full = rerun(lambda kp: model.forward_dgraph(x.to(DEV), h_prev, dg, dropout_keep=kp), ones)
        for g in range(G):
            for k in range(K):
                full = att_full[g][k].alpha
                assert bool((full > 0).all()), 'a softmax weight underflowed: the mask cannot be read off the attention'
                assert torch.equal(att[g][k].alpha, full * keep_csr[g][k].float()), (c, g, k)
        # (3) the oracle with the recovered mask (its attention = softmax * keep / (1 - p))
        s_ref, l_ref, h_ref, a_ref = orc.forward(pr, cfg, x, h_ref, og, training=True, dropout_keep=keep_orc)
        assert (scores.detach().cpu() - s_ref.detach()).abs().max().item() <= SCORE_TOL, c
        assert torch.allclose(h.detach().cpu(), h_ref.detach(), atol=LOGIT_ATOL, rtol=LOGIT_RTOL), c
        for g in range(G):
            for k in range(K):
                assert torch.allclose(att[g][k].per_edge().cpu(), a_ref[g][k].detach(), atol=1e-5, rtol=1e-4), (c, g, k)
        wl, ws = gold.t(f'c{c}/wl'), gold.t(f'c{c}/ws')
        loss = loss + (wl.to(DEV) * logits).sum() + (ws.to(DEV) * scores).sum()
        loss_ref = loss_ref + (wl * l_ref).sum() + (ws * s_ref).sum()
    loss.backward()
    loss_ref.backward()
    gscale = max(1.0, max(v.grad.abs().max().item() for v in pr.values() if v.grad is not None))
    for k, prm in model.named_parameters():
        tol = GRAD_RTOL * gscale * (10 if (k.endswith('.0.bias') and k.startswith('input_')) else 1)
        err = (prm.grad.cpu() - pr[k].grad).abs().max().item()
        assert err <= tol, f'grad {k}: {err} > {tol}'
    # the fixture's graphs are small: the mask statistics proper are test_self_drawn_mask_statistics


def test_self_drawn_mask_statistics():
    """Keep rate 0.5 +- 4 sigma per head, heads pairwise independent, fresh masks per call -- on a batch large enough to
    say so (B = 64 windows, K = 2 and K = 3; ~1e5 positions per call), the mask read off the returned attention."""
    from trackmpnn_amd import TrackMPNN
    for K in (2, 3):
        cfg = orc.OracleConfig('2d', 3, 64, K, 'diff')
        plans, xs = _batched_case(B=64, frames=5, mean=6, max_dets=20, F=8, seed0=40 + K)
        p = orc.random_params(cfg, seed=K, scale=0.15)
        model = TrackMPNN('2d', 3, 64, K, 'diff')
        model.load_state_dict({k: v.clone() for k, v in p.items()}, strict=True)
        model = model.to(DEV).train()
        h = None
        prev = None
        with torch.no_grad():
            for plan, x in zip(plans, xs):
                _, _, h, att = model.forward_graph(x.to(DEV), h, plan.to(DEV))
                m = torch.stack([att[0][k].alpha != 0 for k in range(K)]).double()      # [K, 2E]
                n = m.shape[1]
                if n < 2000:
                    continue
                sig = 0.5 / n ** 0.5
                rate = m.mean(1)
                assert bool(((rate - 0.5).abs() <= 4 * sig).all()), (K, rate.tolist(), n)
                for a in range(K):
                    for b in range(a + 1, K):
                        both = (m[a] * m[b]).mean().item()                      # independent fair coins: 1/4
                        assert abs(both - 0.25) <= 4 * (0.25 * 0.75 / n) ** 0.5, (K, a, b, both)
                # no stale mask: this call's mask on the positions the previous graph already had is not the previous mask
                if prev is not None:
                    k0 = min(prev.shape[1], n)
                    agree = (m[:, :k0] == prev[:, :k0]).double().mean().item()
                    assert agree < 0.75, agree
                prev = m


@pytest.mark.parametrize('H', [64, 32])
@pytest.mark.parametrize('R', [1, 31, 32, 33, 255, 2049, 8 * 32 * 9 + 5, 70001])
def test_node_cell_forward_ragged_sizes(R, H):
    """tmpnn_gru_fwd with compact messages (the node cell, models/layers.py:114; round 6: k_gru_fwd_split_node, one 32-column
    half of the outputs per workgroup, row groups dealt to block pairs b, b + 8) on row counts around its tile (32 rows), its
    group granularity (8 row tiles per group, groups in sets of 8) and a grid larger than the chip: h_out, the four gate
    planes and the fused head partials against the fp64 formula, scattered row ids, rows outside the list untouched."""
    from trackmpnn_amd import _lib
    gen = torch.Generator().manual_seed(R + H)
    N = 2 * R + 5
    rows = torch.randperm(N, generator=gen)[:R].sort().values
    r32 = lambda *s: torch.randn(*s, generator=gen)                 # noqa: E731
    h, msg = r32(N, H + 4), r32(R, H)
    sc = 1.0 / H ** 0.5
    wih, whh = sc * r32(3 * H, H), sc * r32(3 * H, H)
    bih, bhh, w_head = 0.3 * r32(3 * H), 0.3 * r32(3 * H), r32(H)
    d = lambda t: t.to(DEV).contiguous()                            # noqa: E731
    hD, msgD, rowsD = d(h), d(msg), d(rows.to(torch.int32))
    out = torch.full((N, H), 3.0, device=DEV)
    gates = torch.full((4, N, H), 5.0, device=DEV)
    cw = H // 32
    parts = torch.full((cw, N), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    wih_t, whh_t, bihD, bhhD, whD = d(wih.t()), d(whh.t()), d(bih), d(bhh), d(w_head)       # (kept alive over the launch)
    _lib.call('tmpnn_gru_fwd', rowsD.data_ptr(), R, 0, None, None, msgD.data_ptr(), H, 1, H, hD.data_ptr(), H + 4, H,
              wih_t.data_ptr(), whh_t.data_ptr(), bihD.data_ptr(), bhhD.data_ptr(), out.data_ptr(), H,
              gates.data_ptr(), N * H, whD.data_ptr(), parts.data_ptr(), N, st)
    torch.cuda.synchronize()
    x64, h64 = msg.double(), h[rows, :H].double()
    gi = x64 @ wih.double().t() + bih.double()
    gh = h64 @ whh.double().t() + bhh.double()
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    hn = gh[:, 2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * hn)
    ref = (1 - z) * n + z * h64
    got = out.cpu()[rows].double()
    assert (got - ref).abs().max().item() <= 5e-6 * max(1.0, ref.abs().max().item()), (R, H)
    for plane, want in enumerate((r, z, n, hn)):
        assert (gates[plane].cpu()[rows].double() - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item()), (R, H, plane)
    head = (ref * w_head.double()).view(R, cw, 32).sum(2)           # partial dot product per 32-column block
    gp = parts.cpu()[:, rows].t().double()
    assert (gp - head).abs().max().item() <= 2e-5 * max(1.0, head.abs().max().item()), (R, H)
    outside = torch.ones(N, dtype=torch.bool)
    outside[rows] = False
    assert bool((out.cpu()[outside] == 3.0).all()) and bool((gates.cpu()[:, outside] == 5.0).all())
    assert bool((parts.cpu()[:, outside] == 7.0).all())


def test_c3_chain_at_realistic_weight_scale_vs_fp64():
    """BASELINE C3 (12-frame windows: an 11-call recurrence) at the weight scale of the other workload tests (0.1), where the
    chain is ill-conditioned in fp32 -- the fp32 ORACLE itself drifts ~1e-3 from its own fp64 evaluation by the last calls, so a
    1e-4 comparison against it would pin rounding noise (test_baseline_workloads_vs_oracle therefore runs C3 at scale 0.05).
    Here the yardstick is the fp64 evaluation of the oracle: the HIP path must be as close to it as the fp32 oracle is
    (error <= 2 x the oracle's own fp32 error + 1e-4, per call, for scores and state; gradients likewise), i.e. any error
    beyond fp32 conditioning would show."""
    from trackmpnn_amd import TrackMPNN
    H, ncat, frames = 64, 3, 12
    cfg = orc.OracleConfig('2d', ncat, H, 0, 'diff')
    plans, xs = _batched_case(B=16, frames=frames, mean=8.0, max_dets=25, F=ncat + 5, seed0=300 + frames)
    p = orc.random_params(cfg, seed=frames, scale=0.1)
    model = TrackMPNN('2d', ncat, H, 0, 'diff')
    model.load_state_dict({k: v.clone() for k, v in p.items()}, strict=True)
    model = model.to(DEV).train()

    def leaf(v, dt):
        v = v.clone().to(dt) if v.dtype.is_floating_point else v.clone()
        return v.requires_grad_(True) if (v.dtype.is_floating_point and 'running' not in k) else v
    p32, p64 = {}, {}
    for k, v in p.items():
        p32[k], p64[k] = leaf(v, torch.float32), leaf(v, torch.float64)
    h = h32 = h64 = None
    loss = loss32 = loss64 = 0.0
    gen = torch.Generator().manual_seed(1)
    worst = 0.0
    for c, (plan, x) in enumerate(zip(plans, xs)):
        og = _oracle_graph(plan.graph)
        s32, l32, h32, _ = orc.forward(p32, cfg, x, h32, og, training=True, seg_ids=plan.seg_of_new)
        s64, l64, h64, _ = orc.forward(p64, cfg, x.double(), h64, og, training=True, seg_ids=plan.seg_of_new)
        nxt = plans[c + 1].n_new if c + 1 < len(plans) else 0
        s, l, h, _ = model.forward_graph(x.to(DEV), h, plan.to(DEV), reserve_rows=nxt)
        for ours, o32, o64, what in ((s, s32, s64, 'scores'), (h, h32, h64, 'state')):
            e_or = (o32.detach().double() - o64.detach()).abs().max().item()
            e_us = (ours.detach().cpu().double() - o64.detach()).abs().max().item()
            assert e_us <= 2.0 * e_or + 1e-4, (c, what, e_us, e_or)
            worst = max(worst, e_or)
        w = torch.randn(l.shape, generator=gen)
        loss = loss + (w.to(DEV) * l).sum() + s.sum()
        loss32 = loss32 + (w * l32).sum() + s32.sum()
        loss64 = loss64 + (w.double() * l64).sum() + s64.sum()
    assert worst > 2e-5, 'the chain is expected to be ill-conditioned at this scale; if it is not, compare with the oracle directly'
    loss.backward()
    loss32.backward()
    loss64.backward()
    gscale = max(1.0, max(v.grad.abs().max().item() for v in p64.values() if v.grad is not None))
    for k, prm in model.named_parameters():
        e_or = (p32[k].grad.double() - p64[k].grad).abs().max().item()
        e_us = (prm.grad.cpu().double() - p64[k].grad).abs().max().item()
        assert e_us <= 2.0 * e_or + 2e-4 * gscale, f'grad {k}: {e_us} vs the fp32 oracle\'s {e_or}'
