"""The fused batch-1 iteration (-m gpu; csrc/small.hip, small_bn_dev.h: tmpnn_mp_iter_*) against the fp64 evaluation of the oracle
at the sizes where its internal routes switch: more tiles than persistent backward blocks, more new det rows than the BatchNorm
backward keeps in LDS, det tiles of 4 and of 16 dets whose incidence stretch is staged or too long to stage, carried rows beyond
one sweep of the finish kernel, exactly full and nearly empty tiles.  tests/test_small_iter_sizes.py shows on the CPU that the
windows land there and that the comparison notices single faults.

(The grid-stride of the carried rows is reached by the H = 64 models of case C only: 5040 carried rows, 4096 per sweep at H = 64,
8192 at H = 32.)  `python -m tests.test_small_iter_sizes_gpu OUT.md` writes the worst error of every case next to the fp32
oracle's: profiles/small_iter_parity.md is that table from an MI355X.

Bound, per quantity: error(HIP vs fp64) <= 2 x error(fp32 oracle vs fp64) + the parity floors of tests/test_parity_gpu.py, with
the fp32 oracle's own term capped (asserted) so that an ill-conditioned draw cannot widen it."""
import functools

import pytest
import torch

from oracle import trackmpnn_oracle as orc
from tests import small_iter_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


# id -> (window, features, nhidden, attention heads, msg_type, mode); mode: 'train' | 'eval' (with backward) | 'eval_nograd'
_FOUR = [(64, 'diff'), (64, 'concat'), (32, 'diff'), (32, 'concat')]
MODELS = {}
for _case in ('A', 'C'):
    for _H, _msg in _FOUR:
        MODELS[f'{_case}-h{_H}-{_msg}'] = (_case, '2d', _H, 0, _msg, 'train')
MODELS['A-h48-diff-padded'] = ('A', '2d', 48, 0, 'diff', 'train')
MODELS['C-h32-concat-3groups'] = ('C', '2d+temp+vis', 32, 0, 'concat', 'train')
MODELS['C-h64-diff-k2-eval'] = ('C', '2d', 64, 2, 'diff', 'eval')
MODELS['C-h64-diff-eval-nograd'] = ('C', '2d', 64, 0, 'diff', 'eval_nograd')
for _case in ('B', 'D', 'E4', 'E3'):
    MODELS[f'{_case}-h64-diff'] = (_case, '2d', 64, 0, 'diff', 'train')
    MODELS[f'{_case}-h32-concat'] = (_case, '2d', 32, 0, 'concat', 'train')


@functools.lru_cache(maxsize=None)
def reference(key):
    """(cfg, params, calls, xs, weights, V, fp32 oracle, fp64 oracle) of one entry of MODELS: computed once, never modified"""
    case, features, H, K, msg, mode = MODELS[key]
    cfg = orc.OracleConfig(features, sc.NCAT, H, K, msg)
    seed = sc.SEEDS.get((case, features, H, msg), 0)
    params = orc.random_params(cfg, seed=seed, scale=sc.PARAM_SCALE)
    calls, xs, weights, V = sc.inputs(case, cfg, seed)
    kw = dict(training=mode == 'train', grad=mode != 'eval_nograd')
    r32 = sc.run_oracle(cfg, params, calls, xs, weights, V, torch.float32, **kw)
    r64 = sc.run_oracle(cfg, params, calls, xs, weights, V, torch.float64, **kw)
    return cfg, params, calls, xs, weights, V, r32, r64


def run_hip(key, monkeypatch):
    """The window through the drop-in call model(x, h, node_adj, edge_adj) and one backward; returns (Result on the CPU, the
    names of the C-ABI entry points that went through trackmpnn_amd._lib.call meanwhile)."""
    import trackmpnn_amd.track_mpnn as tm
    from trackmpnn_amd import TrackMPNN, _lib
    from trackmpnn_amd.small import small_eligible
    case, features, H, K, msg, mode = MODELS[key]
    cfg, params, calls, xs, weights, V, _r32, _r64 = reference(key)
    model = TrackMPNN(features, sc.NCAT, H, K, msg)
    res = model.load_state_dict({k: v.clone() for k, v in params.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model = model.to(DEV)
    model = model.train() if mode == 'train' else model.eval()
    grad = mode != 'eval_nograd'
    names = []
    real = _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, 'call', spy)
    assert tm.SMALL_PATH
    h, loss, outs, xl = None, 0.0, [], []
    with torch.set_grad_enabled(grad):
        for i, c in enumerate(calls):
            assert small_eligible(model, c.N), (key, c.N)
            na, ea = sc.adjacency(c, DEV)
            x = xs[i].to(DEV).requires_grad_(grad)
            xl.append(x)
            s, l, h, _ = model(x, h, na, ea)
            assert tuple(h.shape) == (c.N, len(cfg.groups) * H)
            if grad:
                loss = loss + (weights[i][0].to(DEV) * l).sum() + (weights[i][1].to(DEV) * s).sum()
            outs.append((s.detach().cpu(), l.detach().cpu(), h.detach().cpu()))
        if grad:
            (loss + (V.to(DEV) * h).sum()).backward()
    model.check_graphs()
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, 'call', real)
    grads = {k: p.grad.cpu() for k, p in model.named_parameters()} if grad else None
    xg = [x.grad.cpu() for x in xl] if grad else None
    return sc.Result(outs, grads, xg, {k: v.cpu() for k, v in model.named_buffers()}), names


def test_floors_are_the_parity_constants():
    from tests import test_parity_gpu as tp
    assert (sc.SCORE_TOL, sc.LOGIT_ATOL, sc.LOGIT_RTOL, sc.GRAD_RTOL) == (tp.SCORE_TOL, tp.LOGIT_ATOL, tp.LOGIT_RTOL, tp.GRAD_RTOL)


def measure(key, monkeypatch):
    cfg, params, calls, xs, weights, V, r32, r64 = reference(key)
    got, names = run_hip(key, monkeypatch)
    return sc.compare(got, r32, r64), names, sc.grad_scale(r64)


@pytest.mark.parametrize('key', list(MODELS))
def test_fused_iteration_vs_fp64_at_its_size_switches(key, monkeypatch):
    """Scores, logits and state of every call, every parameter gradient and x.grad of every call after one backward of
    sum_c (w_l . logits + w_s . scores) + V . h_last, and the BatchNorm buffers after the window; the eval / no_grad entry:
    scores, logits and state.  The case must have run on the fused iteration: no staged entry point may have been called."""
    cmp, names, gscale = measure(key, monkeypatch)
    K = MODELS[key][3]
    staged = [n for n in names if n.startswith(sc.STAGED_PREFIXES)]
    assert not staged, f'{key} fell back to the staged kernels: {sorted(set(staged))}'
    assert 'tmpnn_mp_iter_prepare' in names, 'the fused iteration prepares its weight operands through this entry point'
    assert any(n.startswith('tmpnn_att_') for n in names) == (K > 0)
    worst = sc.summary(cmp, gscale)
    print(f'\n{key}: ' + ', '.join(f'{k} {e:.3g} (fp32 oracle {o:.3g})' for k, (e, o) in worst.items()))
    bad = sc.failures(cmp)
    assert not bad, f'{key}:\n' + '\n'.join(bad)


def write_report(path):
    """The table of profiles/small_iter_parity.md: per case the worst error of the HIP path against fp64 and, behind the slash, the
    fp32 oracle's own, for each class of compared quantity."""
    rows = []
    for key in MODELS:
        mp = pytest.MonkeyPatch()
        try:
            cmp, _names, gscale = measure(key, mp)
        finally:
            mp.undo()
        rows.append((key, sc.summary(cmp, gscale), max(e / b for e, b, _o in cmp.values() if b > 0), len(sc.failures(cmp))))
    with open(path, 'w') as f:
        f.write('| case | scores | logits, state | gradients, x.grad / largest fp64 entry | BatchNorm buffers | worst error / bound | over bound |\n')
        f.write('|---|---|---|---|---|---|---|\n')
        for key, s, ratio, nbad in rows:
            cells = [('%.1e / %.1e' % s[k]) if k in s else '-' for k in ('scores', 'state', 'grad', 'buffers')]
            f.write(f'| {key} | ' + ' | '.join(cells) + f' | {ratio:.3f} | {nbad} |\n')
    return rows


if __name__ == '__main__':
    import sys
    import __graft_entry__
    __graft_entry__.build()
    sys.exit(1 if any(r[3] for r in write_report(sys.argv[1])) else 0)
