"""BucketAdam on the MI355X (-m gpu): the one-launch Adam step (tmpnn_adam_step) against torch.optim.Adam, its folds
(grad_scale, zero_grads), the version counters it moves, whole training steps, a captured window, checkpoint interchange and
the gradient-flow statistics (tmpnn_grad_flow).

The update rule is held to torch's own fp32 error: with p64 the fp64 run of torch.optim.Adam on the same gradient sequence,
err(x) = max_i |x_i - p64_i| / (|p64_i| + lr), and err(BucketAdam) <= 4 * err(torch.optim.Adam on the CPU in fp32) at every
checkpoint (the 4: another operation order of the same fp32 formula lands at 0.9 .. 1.54 x torch's error; fma contraction and
the device's division / square root get the rest; a wrong rule is hundreds of times off).  Every test prints what it measured.
"""
import warnings

import numpy as np
import pytest
import torch

from tests.conftest import chunk_golden_names
from tests.golden_util import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LR, WD = 1e-4, 5e-4                                  # the reference's defaults (training_options.py:26, 28)
SIZES = (70001, 3, 64, 29932, 1, 99999)             # 200 000 elements; segments that start off a 16-byte boundary


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


# ---- helpers ---------------------------------------------------------------------------------------------------------------
class _Flat(torch.nn.Module):
    """Parameters of the given sizes holding `init` (a flat fp32 vector) in order."""

    def __init__(self, init, sizes=SIZES):
        super().__init__()
        assert sum(sizes) == init.numel()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(c.clone()) for c in torch.split(init, list(sizes))])

    def flat(self):
        return torch.cat([p.detach().reshape(-1) for p in self.ps])


def _synthetic(steps=60, n=200000, seed=77):
    """(initial parameters, [gradient per step]) on the host: per-element gradient scales log-uniform in [1e-6, 1e2] with
    every 7th element exactly zero, initial parameters of scale log-uniform in [1e-3, 1]."""
    gen = torch.Generator().manual_seed(seed)
    scale = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(np.log(1e-6), np.log(1e2), generator=gen))
    scale[::7] = 0.0
    mag = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(np.log(1e-3), np.log(1.0), generator=gen))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    p0 = (mag * sign).float()
    grads = [(scale * torch.randn(n, dtype=torch.float64, generator=gen)).float() for _ in range(steps)]
    assert all(float(g[::7].abs().max()) == 0.0 for g in grads)
    return p0, grads


def _torch_cpu(p0, grads, dtype, cut, checkpoints, lr=LR, wd=WD):
    """torch.optim.Adam on the CPU in `dtype` under StepLR(step_size=cut, gamma=0.2); {step: parameters (fp64)}."""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adam([p], lr=lr, weight_decay=wd)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=cut, gamma=0.2)
    out = {}
    for i, g in enumerate(grads, 1):
        p.grad = g.to(dtype).clone()
        opt.step()
        sched.step()
        if i in checkpoints:
            out[i] = p.detach().double().clone()
    return out


def _bucket_adam(module, bucket, grads, cut, checkpoints, read, lr=LR, wd=WD):
    """BucketAdam on the GPU, the gradients fed through bucket.flat; {step: parameters (fp64, host)}."""
    from trackmpnn_amd import BucketAdam
    opt = BucketAdam(module, bucket, lr=lr, weight_decay=wd)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=cut, gamma=0.2)
    out = {}
    for i, g in enumerate(grads, 1):
        bucket.flat.copy_(g)
        opt.step()
        sched.step()
        if i in checkpoints:
            out[i] = read().double().cpu()
    return out


def _err(x, p64, lr=LR):
    return float(((x - p64).abs() / (p64.abs() + lr)).max())


def _hold_to_torch(tag, mine, t32, t64, checkpoints):
    for i in checkpoints:
        e_mine, e_torch = _err(mine[i], t64[i]), _err(t32[i], t64[i])
        ratio = e_mine / e_torch if e_torch > 0 else float('inf')
        print(f'[optim] {tag}: step {i}: err(BucketAdam) = {e_mine:.3e}, err(torch fp32) = {e_torch:.3e}, ratio {ratio:.3f}')
    for i in checkpoints:
        e_mine, e_torch = _err(mine[i], t64[i]), _err(t32[i], t64[i])
        assert e_torch > 0, (tag, i)
        assert e_mine <= 4 * e_torch, (tag, i, e_mine, e_torch)


def _sync_warnings(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    return [str(w.message) for w in rec if 'called a synchronizing' in str(w.message)]


def _chunk_model(gold):
    from tests.test_parity_gpu import build_model
    return build_model(dict(gold.meta, mode='train'), gold.params())


# ---- 4. the update rule ------------------------------------------------------------------------------------------------------
def test_update_rule_on_synthetic_gradients():
    from trackmpnn_amd.dist import GradBucket
    p0, grads = _synthetic()
    cps = (1, 10, 30, len(grads))
    cut = len(grads) // 2
    module = _Flat(p0).to(DEV)
    bucket = GradBucket(module)
    mine = _bucket_adam(module, bucket, grads, cut, cps, module.flat)
    t32 = _torch_cpu(p0, grads, torch.float32, cut, cps)
    t64 = _torch_cpu(p0, grads, torch.float64, cut, cps)
    _hold_to_torch('synthetic 60 x 200000', mine, t32, t64, cps)
    moved = float((mine[cps[-1]] - p0.double()).abs().max())
    assert moved > 10 * LR                                        # (the run is not a no-op)


def test_zero_gradient_without_decay_does_not_move():
    from trackmpnn_amd import BucketAdam
    from trackmpnn_amd.dist import GradBucket
    p0, grads = _synthetic(steps=5)
    module = _Flat(p0).to(DEV)
    bucket = GradBucket(module)
    opt = BucketAdam(module, bucket, lr=LR, weight_decay=0)
    for g in grads:
        bucket.flat.copy_(g)
        opt.step()
    p = module.flat().cpu()
    assert torch.equal(p[::7], p0[::7])                                          # exact: zero gradient, zero decay
    rest = torch.ones(p0.numel(), dtype=torch.bool)
    rest[::7] = False
    assert float((p[rest] != p0[rest]).float().mean()) > 0.5
    assert float(opt.exp_avg.cpu()[::7].abs().max()) == 0.0 and float(opt.exp_avg_sq.cpu()[::7].abs().max()) == 0.0
    assert float(opt.state[module.ps[0]]['step']) == len(grads)


@pytest.mark.parametrize('name', chunk_golden_names())
def test_update_rule_on_the_gradients_of_training_chunks(name):
    from trackmpnn_amd import BucketAdam
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.loops import train_chunk
    from tests.golden_util import chunk_tp
    gold = Golden(name)
    X, y = gold.t('X'), gold.t('y')
    tp = chunk_tp(gold)             # (a *_notp fixture: the node output head's gradient is zero in every step)
    # record: the gradients of 10 consecutive training steps, taken from the bucket before each step
    model = _chunk_model(gold)
    bucket = GradBucket(model)
    opt = BucketAdam(model, bucket, lr=LR, weight_decay=WD)
    p0 = torch.cat([p.detach().reshape(-1) for p in bucket.params]).cpu()
    grads = []
    for _ in range(10):
        opt.zero_grad()
        train_chunk(model, X, y, DEV, tp)
        grads.append(bucket.flat.detach().cpu().clone())
        opt.step()
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    # open loop: the same sequence through the three optimizers
    cps, cut = (1, 10), 5
    model = _chunk_model(gold)
    bucket = GradBucket(model)
    read = lambda: torch.cat([p.detach().reshape(-1) for p in bucket.params])
    assert torch.equal(read().cpu(), p0)
    mine = _bucket_adam(model, bucket, grads, cut, cps, read)
    t32 = _torch_cpu(p0, grads, torch.float32, cut, cps)
    t64 = _torch_cpu(p0, grads, torch.float64, cut, cps)
    _hold_to_torch(f'{name}, 10 steps x {p0.numel()}', mine, t32, t64, cps)


# ---- 5. the folds ------------------------------------------------------------------------------------------------------------
def _fresh(p0, **kw):
    from trackmpnn_amd import BucketAdam
    from trackmpnn_amd.dist import GradBucket
    module = _Flat(p0).to(DEV)
    bucket = GradBucket(module)
    return module, bucket, BucketAdam(module, bucket, lr=LR, weight_decay=WD, **kw)


def _same(a, b):
    return (torch.equal(a[0].flat(), b[0].flat()) and torch.equal(a[2].exp_avg, b[2].exp_avg)
            and torch.equal(a[2].exp_avg_sq, b[2].exp_avg_sq))


def test_folds_are_exact():
    p0, grads = _synthetic(steps=10)
    gd = [g.to(DEV) for g in grads]
    for s in (1 / 2, 1 / 3, 1 / 8):
        a, b = _fresh(p0), _fresh(p0)
        for g in gd:
            a[1].flat.copy_(g)
            a[2].step(grad_scale=s)
            b[1].flat.copy_(g)
            b[1].flat.mul_(s)                                     # what allreduce_grads does with 1 / world
            b[2].step()
        assert _same(a, b), s
        assert not torch.equal(a[0].flat().cpu(), p0)
    a, b = _fresh(p0), _fresh(p0)
    for g in gd:
        a[1].flat.copy_(g)
        a[2].step(zero_grads=True)
        assert float(a[1].flat.abs().max()) == 0.0 and not bool(torch.isnan(a[1].flat).any())
        b[1].flat.copy_(g)
        b[2].step()
        assert torch.equal(b[1].flat, g)                          # (a plain step leaves the gradients alone)
        b[1].zero()
    assert _same(a, b)
    c = _fresh(p0)
    for g in gd:
        c[1].flat.copy_(g)
        c[2].step(zero_grads=True)
    assert _same(a, c)                                            # two identical runs: identical bits
    assert float(c[2].state[c[0].ps[0]]['step']) == len(gd)


# ---- 6. no host in the step --------------------------------------------------------------------------------------------------
def test_a_step_never_waits_for_the_device():
    p0, grads = _synthetic(steps=2)
    module, bucket, opt = _fresh(p0)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=5, gamma=0.2)
    bucket.flat.copy_(grads[0])
    opt.step()                                                    # warm: tables, code objects
    torch.cuda.synchronize()

    def ten():
        for _ in range(10):
            opt.step()
            sched.step()                                          # (crosses a StepLR boundary: the new lr goes to the device)

    assert _sync_warnings(ten) == []
    assert opt.param_groups[0]['lr'] == pytest.approx(LR * 0.2 ** 2)
    assert float(opt.state[module.ps[0]]['step']) == 11
    assert len(_sync_warnings(lambda: float(opt.state[module.ps[0]]['step']))) >= 1     # (the detector works)


# ---- 7. the model sees the new weights ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, staged', [('roll_2d_diff_k0_train', False), ('roll_2d_diff_k0_train_h48', False),
                                          ('roll_2d_diff_k0_train_h128', True)])
def test_the_model_sees_the_new_weights(name, staged):
    from tests.test_parity_gpu import build_model
    from trackmpnn_amd import BucketAdam, device_graph_from_adjacency, plan_single
    from trackmpnn_amd.dist import GradBucket
    gold = Golden(name)
    model = build_model(gold.meta, gold.params())
    assert model.nhidden == gold.meta['nhidden']
    bucket = GradBucket(model)
    opt = BucketAdam(model, bucket, lr=1e-2)
    x = gold.t('c0/x').to(DEV)
    na, ea = gold.adjacency(0, 'node_adj', DEV), gold.adjacency(0, 'edge_adj', DEV)
    g = device_graph_from_adjacency(na, ea, DEV)
    plan = plan_single(g.frame_graph(), int(x.shape[0])) if staged else None

    def forward(m):
        return m.forward_graph(x, None, plan) if staged else m.forward_dgraph(x, None, g)

    for it in range(2):                                           # two steps: every cache is warm before the second
        opt.zero_grad()
        s0, l0, h0, _ = forward(model)
        (l0.square().sum() + h0.square().sum()).backward()
        opt.step()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        s1, l1, h1, _ = forward(model)
        fresh = build_model(gold.meta, sd)
        s2, l2, h2, _ = forward(fresh)
        assert torch.equal(l1, l2) and torch.equal(s1, s2) and torch.equal(h1, h2), (name, it)
        assert not torch.equal(l1, l0), (name, it)                # (the step changed the outputs)


# ---- 8. whole steps ----------------------------------------------------------------------------------------------------------
def _pre_bn_biases(model):
    """The biases in front of a BatchNorm: their true gradient is zero, the computed one is rounding noise that Adam turns into
    +- lr (tests/test_dist_gloo.py) -- excluded from parameter comparisons."""
    return {k for k, _ in model.named_parameters() if k.startswith('input_transforms.') and k.endswith('.0.bias')}


def _divergence(a, b):
    skip = _pre_bn_biases(a)
    assert skip
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    return max(float((pa[k] - pb[k]).abs().max()) for k in pa if k not in skip)


def test_closed_loop_chunk_steps_match_torch_adam():
    from trackmpnn_amd import BucketAdam
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.loops import train_chunk
    gold = Golden('chunk_c2_kitti_car_w5')
    X, y = gold.t('X'), gold.t('y')
    runs = []
    for kind in ('bucket', 'torch'):
        model = _chunk_model(gold)
        bucket = GradBucket(model)
        opt = (BucketAdam(model, bucket, lr=LR, weight_decay=WD) if kind == 'bucket'
               else torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD))
        losses = []
        for _ in range(5):
            if kind == 'bucket':
                opt.zero_grad()
            else:
                opt.zero_grad(set_to_none=False)
            loss, _, _ = train_chunk(model, X, y, DEV)
            opt.step()
            losses.append(float(loss.detach()))
        assert bucket.check_alias()
        runs.append((model, losses))
    (ma, la), (mb, lb) = runs
    for i, (a, b) in enumerate(zip(la, lb)):
        print(f'[optim] closed loop, chunk step {i}: loss {a!r} (BucketAdam) / {b!r} (torch Adam), relative {abs(a - b) / abs(b):.3e}')
    print(f'[optim] closed loop, chunk: max parameter divergence after 5 steps {_divergence(ma, mb):.3e} (lr {LR})')
    assert la[0] != la[-1]
    for a, b in zip(la, lb):
        assert abs(a - b) <= 1e-4 * abs(b), (la, lb)


def test_closed_loop_batched_steps_with_a_monitor_match_torch_adam():
    from tests.test_train_batch_gpu import _chunks, _perturbed_model
    from trackmpnn_amd import BucketAdam, TrainMonitor, build_train_batch_device
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.loops import train_chunks
    ys = _chunks(8, seed=71)
    gen = torch.Generator().manual_seed(72)
    Xd = torch.cat([torch.randn(yy.shape[0], 8, generator=gen) for yy in ys]).to(DEV)
    batch = build_train_batch_device(ys, DEV)
    assert batch.B == 8
    runs = []
    for kind in ('bucket', 'torch'):
        model = _perturbed_model()
        bucket = GradBucket(model)
        opt = (BucketAdam(model, bucket, lr=LR, weight_decay=WD) if kind == 'bucket'
               else torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD))
        m = TrainMonitor(DEV)
        losses = []
        for _ in range(5):
            if kind == 'bucket':
                opt.zero_grad()
            else:
                opt.zero_grad(set_to_none=False)
            loss, _, _, _ = train_chunks(model, batch, Xd, monitor=m)
            opt.step()
            losses.append(float(loss.detach()))
        runs.append((model, losses, m.read()))
    (ma, la, ra), (mb, lb, rb) = runs
    for i, (a, b) in enumerate(zip(la, lb)):
        print(f'[optim] closed loop, B = 8 step {i}: loss {a!r} / {b!r}, relative {abs(a - b) / abs(b):.3e}')
    print(f'[optim] closed loop, B = 8: max parameter divergence {_divergence(ma, mb):.3e}; records {ra} / {rb}')
    for a, b in zip(la, lb):
        assert abs(a - b) <= 1e-4 * abs(b), (la, lb)
    assert ra['forwards'] == rb['forwards'] == 5 * batch.ncalls and ra['chunks'] == rb['chunks'] == 5 * batch.B
    for k in ('avg_loss_c', 'avg_loss_f', 'avg_loss'):
        assert abs(ra[k] - rb[k]) <= 1e-4 * abs(rb[k]), (k, ra[k], rb[k])
    assert 0.0 <= ra['avg_f1'] <= 1.0 and 0.0 <= rb['avg_f1'] <= 1.0


# ---- 9. captured -------------------------------------------------------------------------------------------------------------
def test_captured_window_with_bucket_adam_equals_eager_steps():
    """The structure of tests/test_small_path_gpu.py::test_captured_window_replay_equals_eager_steps with BucketAdam (no
    capturable flag), then a StepLR boundary between two replays: the device-resident lr and step count at work."""
    from tests.test_parity_gpu import build_model
    from trackmpnn_amd import BucketAdam, CapturedWindow
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
        opt = BucketAdam(model, bucket, lr=1e-3, weight_decay=WD)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.2)
        losses, snaps = [], []
        for it in range(4):
            h, outs = None, []
            for i, (x, na, ea) in enumerate(calls):
                s, l, h, _ = model(xs2[i] if it == 2 else x, h, na, ea)
                outs.append((s, l))
            loss = loss_fn(outs, h)
            bucket.zero()
            loss.backward()
            opt.step()
            losses.append(loss.item())
            snaps.append({k: v.detach().clone() for k, v in model.state_dict().items()})
            if it == 2:
                sched.step()                                      # lr 1e-3 -> 2e-4 before the fourth step
        return snaps, losses

    s_ref, l_ref = eager()
    model = build_model(gold.meta, gold.params())
    bucket = GradBucket(model)
    opt = BucketAdam(model, bucket, lr=1e-3, weight_decay=WD)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.2)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    win = CapturedWindow(model, calls, loss_fn, optimizer=opt, bucket=bucket, warmup=2)
    # the warm-up and the capture itself stepped the optimizer: rewind model and optimizer, then replay
    model.load_state_dict(sd0)
    for st in opt.state.values():
        for k, v in st.items():
            if torch.is_tensor(v):
                v.zero_()
    losses = [win.replay().item(), win.replay().item(), win.replay(xs2).item()]
    assert losses == l_ref[:3]
    for k, a in model.state_dict().items():
        assert torch.equal(a, s_ref[2][k]), k
    assert float(opt.state[bucket.params[0]]['step']) == 3
    sched.step()
    assert opt.param_groups[0]['lr'] == pytest.approx(2e-4)
    losses.append(win.replay([x for x, _, _ in calls]).item())
    assert losses == l_ref
    for k, a in model.state_dict().items():
        assert torch.equal(a, s_ref[3][k]), k
    # the fourth update is the smaller one (the new learning rate reached the captured launch)
    k0 = 'output_transform_edge.weight'
    d3 = float((s_ref[2][k0] - s_ref[1][k0]).abs().max())
    d4 = float((s_ref[3][k0] - s_ref[2][k0]).abs().max())
    assert 0 < d4 < 0.5 * d3, (d3, d4)


# ---- 10. checkpoint interchange ----------------------------------------------------------------------------------------------
def test_checkpoints_go_both_ways():
    from trackmpnn_amd import BucketAdam
    from trackmpnn_amd.dist import GradBucket
    p0, grads = _synthetic(steps=6)
    gd = [g.to(DEV) for g in grads]
    cps = (6,)
    t32 = _torch_cpu(p0, grads, torch.float32, 100, cps)
    t64 = _torch_cpu(p0, grads, torch.float64, 100, cps)
    for first in ('torch', 'bucket'):
        module = _Flat(p0).to(DEV)
        bucket = GradBucket(module)
        mk = dict(torch=lambda: torch.optim.Adam(module.parameters(), lr=LR, weight_decay=WD),
                  bucket=lambda: BucketAdam(module, bucket, lr=LR, weight_decay=WD))
        a = mk[first]()
        for g in gd[:3]:
            bucket.flat.copy_(g)
            a.step()
        b = mk['bucket' if first == 'torch' else 'torch']()
        if first == 'torch':
            ptrs = (b.exp_avg.data_ptr(), b.exp_avg_sq.data_ptr(), b.state[module.ps[0]]['step'].data_ptr())
            b.load_state_dict(a.state_dict())
            assert ptrs == (b.exp_avg.data_ptr(), b.exp_avg_sq.data_ptr(), b.state[module.ps[0]]['step'].data_ptr())
            assert b.state[module.ps[3]]['exp_avg'].data_ptr() == b.exp_avg.data_ptr() + 4 * sum(SIZES[:3])
        else:
            b.load_state_dict(a.state_dict())
        assert float(b.state[module.ps[0]]['step']) == 3
        for g in gd[3:]:
            bucket.flat.copy_(g)
            b.step()
        assert bucket.check_alias()
        _hold_to_torch(f'3 steps of {first} Adam, then the other', {6: module.flat().double().cpu()}, t32, t64, cps)


# ---- 11. gradient flow -------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_gradient_flow_statistics():
    from tests.test_train_batch_gpu import _perturbed_model
    from trackmpnn_amd import BucketAdam
    from trackmpnn_amd.dist import GradBucket
    for nhidden in (64, 256):
        model = _perturbed_model(nhidden=nhidden)
        bucket = GradBucket(model)
        opt = BucketAdam(model, bucket, lr=LR)
        gen = torch.Generator().manual_seed(5)
        n = bucket.flat.numel()
        scale = torch.exp(torch.empty(n).uniform_(np.log(1e-6), np.log(1e2), generator=gen))
        bucket.flat.copy_(scale * torch.randn(n, generator=gen))
        names, stats = opt.grad_flow()
        assert names == [k for k, p in model.named_parameters() if p.requires_grad]
        assert stats.is_cuda and stats.dtype == torch.float64 and tuple(stats.shape) == (len(names), 3)
        st = stats.cpu().numpy()
        for i, p in enumerate(bucket.params):
            g = p.grad.detach().abs().double().cpu()
            assert p.numel() <= 2 ** 22
            mean32 = np.float32(float(g.sum()) / g.numel())
            assert _ulps(np.float32(st[i, 0]), mean32) <= 1, (names[i], st[i, 0], mean32)
            assert st[i, 1] == float(g.max()), names[i]
            assert st[i, 2] == 0.0
        # planted non-finite values: the count is exact, mean and max follow torch (inf / NaN)
        sizes = [p.numel() for p in bucket.params]
        starts = np.concatenate([[0], np.cumsum(sizes)])
        big = int(np.argmax(sizes))
        bucket.flat[starts[big] + 5] = float('inf')
        bucket.flat[starts[big] + sizes[big] - 1] = float('-inf')
        bucket.flat[starts[2]] = float('nan')
        bucket.flat[starts[len(sizes) - 1]] = float('nan')             # (the last parameter: one element)
        _, stats = opt.grad_flow()
        st = stats.cpu().numpy()
        want = np.zeros(len(sizes))
        want[big] += 2
        want[2] += 1
        want[len(sizes) - 1] += 1
        assert (st[:, 2] == want).all(), (st[:, 2], want)
        for i, p in enumerate(bucket.params):
            g = p.grad.detach().abs()
            mx, mean = float(g.max()), float(g.double().mean())
            assert (np.isnan(mx) and np.isnan(st[i, 1])) or st[i, 1] == mx, (names[i], st[i, 1], mx)
            if np.isfinite(mean):
                assert _ulps(np.float32(st[i, 0]), np.float32(mean)) <= 1
            else:
                assert (np.isnan(mean) and np.isnan(st[i, 0])) or st[i, 0] == mean, (names[i], st[i, 0], mean)
        again = opt.grad_flow()[1]
        assert torch.equal(again.view(torch.int64), stats.view(torch.int64))         # the same bits (NaNs included)


def test_gradient_flow_repeats_its_bits_and_step_refuses_a_broken_alias():
    from tests.test_train_batch_gpu import _perturbed_model
    from trackmpnn_amd import BucketAdam
    from trackmpnn_amd.dist import GradBucket
    model = _perturbed_model()
    bucket = GradBucket(model)
    opt = BucketAdam(model, bucket, lr=LR)
    bucket.flat.copy_(torch.randn(bucket.flat.numel(), generator=torch.Generator().manual_seed(6)))
    a = opt.grad_flow()[1].clone()
    b = opt.grad_flow()[1].clone()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    opt.step()
    model.zero_grad(set_to_none=True)                             # the MODULE's zero_grad drops the aliasing
    with pytest.raises(RuntimeError, match='alias'):
        opt.step()
