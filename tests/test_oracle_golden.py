"""Pin the CPU oracle (oracle/trackmpnn_oracle.py) against the reference-generated fixtures."""
import numpy as np
import pytest
import torch

from oracle import trackmpnn_oracle as orc
from tests.conftest import golden_names
from tests.golden_util import Golden

TOL = 1e-4   # logits / h_out: observed 5e-7 at |y|~5; 7e-5 on one det element of C1 (N=1700, |h| up to 43)
SCORE_TOL = 1e-5   # sigmoid scores: the quantity BASELINE.json bounds at 1e-4
RTOL = 1e-5  # fixtures use weights perturbed by 0.3*N(0,1): |h|,|y| reach 35-50, where summation-order noise is ~1e-5 relative


def run_oracle_on_fixture(gold: Golden):
    m = gold.meta
    cfg = orc.OracleConfig(m['features'], m['ncategories'], m['nhidden'], m['nattheads'], m['msg_type'])
    p = gold.params()
    for k, v in p.items():
        if v.dtype.is_floating_point and not k.endswith(orc.BUFFER_SUFFIXES):
            v.requires_grad_(True)
    training = m['mode'] == 'train'
    h = None
    loss = 0.0
    outs = []
    xs = []
    for c in range(gold.ncalls):
        na, ea = gold.adjacency(c, 'node_adj'), gold.adjacency(c, 'edge_adj')
        graph = orc.graph_from_adjacency(na, ea)
        x = gold.t(f'c{c}/x').requires_grad_(True)
        xs.append(x)
        keep = None
        if training and cfg.nattheads > 0:
            keep = [gold.t(f'c{c}/keep_g{g}') for g in range(len(cfg.groups))]
        scores, logits, h, att = orc.forward(p, cfg, x, h, graph, training=training, dropout_keep=keep)
        loss = loss + (gold.t(f'c{c}/wl') * logits).sum() + (gold.t(f'c{c}/ws') * scores).sum()
        outs.append((scores, logits, h, att, graph))
    loss = loss + (gold.t('V') * h).sum()
    return cfg, p, xs, outs, loss


@pytest.mark.parametrize('name', golden_names())
def test_oracle_matches_reference(name):
    gold = Golden(name)
    cfg, p, xs, outs, loss = run_oracle_on_fixture(gold)
    for c, (scores, logits, h, att, graph) in enumerate(outs):
        assert torch.allclose(logits, gold.t(f'c{c}/logits'), atol=TOL, rtol=RTOL), f'logits call {c}'
        assert torch.allclose(scores, gold.t(f'c{c}/scores'), atol=SCORE_TOL, rtol=0), f'scores call {c}'
        if gold.has(f'c{c}/h_out'):
            assert torch.allclose(h, gold.t(f'c{c}/h_out'), atol=TOL, rtol=RTOL), f'h_out call {c}'
        for g in range(len(cfg.groups)):
            for k in range(cfg.nattheads):
                assert torch.allclose(att[g][k], gold.t(f'c{c}/att_g{g}_k{k}'), atol=TOL, rtol=RTOL)
    assert abs(loss.item() - float(gold.d['loss'])) <= 1e-4 * max(1.0, abs(float(gold.d['loss'])))
    loss.backward()
    # gradients: 1e-4 relative to the largest gradient entry of the fixture; the
    # pre-BatchNorm bias has an exactly-zero true gradient, so what it holds is cancellation noise
    gscale = max(1.0, max(v.abs().max().item() for k, v in gold.grads().items() if k != 'X'))
    for k, gref in gold.grads().items():
        if k == 'X':
            continue
        got = p[k].grad
        assert got is not None, k
        tol = 1e-4 * gscale
        if gold.meta['mode'] == 'train' and k.startswith('input_transforms.') and k.endswith('.0.bias'):
            tol = 1e-3 * gscale      # true gradient is exactly 0 (train-mode BN removes the mean): pure noise
        assert (got - gref).abs().max().item() <= tol, f'grad {k}'
    # grad wrt input features: the fixture holds d loss / d X over the whole sequence; the oracle
    # sees per-call slices whose det rows are the rows of X in order of appearance
    if gold.meta['static_iters'] == 0:
        gx = torch.cat([x.grad if x.grad is not None else torch.zeros_like(x) for x in xs], 0)
        det_new = torch.cat([torch.from_numpy(~outs[c][4].is_edge[outs[c][4].N - xs[c].shape[0]:])
                             for c in range(gold.ncalls)])
        gX = gold.grads()['X'][0]
        assert gx[det_new].shape == gX.shape
        # rows of X are visited frame by frame in index order (utils/graph.py:135-136,279)
        assert torch.allclose(gx[det_new], gX, atol=1e-4 * max(1.0, gX.abs().max().item()), rtol=0)
        if gold.meta['mode'] != 'train':
            # (in train mode the all-zero edge rows still feed the BatchNorm statistics, so they
            #  carry a gradient; the reference discards it because those rows are constants)
            assert gx[~det_new].abs().max().item() == 0.0
    # BatchNorm buffers after the run
    for k, ref in gold.final_buffers().items():
        if ref.dtype.is_floating_point:
            assert torch.allclose(p[k].detach(), ref, atol=1e-5, rtol=1e-5), k
        else:
            assert int(p[k]) == int(ref), k


def test_bn_single_row_raises():
    cfg = orc.OracleConfig('2d', 3, 32, 0, 'diff')
    p = orc.random_params(cfg)
    graph = orc.OracleGraph(N=1, is_edge=np.array([False]), src=np.zeros(0, np.int64), dst=np.zeros(0, np.int64),
                            edge_row=np.zeros(0, np.int64), det_row=np.array([0]))
    with pytest.raises(ValueError):
        orc.forward(p, cfg, torch.randn(1, 8), None, graph, training=True)


def test_graph_invariants_rejected():
    a = torch.zeros(3, 3)
    a[0, 0] = 1
    a[2, 2] = 1
    a[1, 0] = 1      # edge row with only a +1
    with pytest.raises(ValueError):
        orc.graph_from_adjacency(a)


@pytest.mark.parametrize('name', __import__('tests.conftest', fromlist=['x']).infer_golden_names())
def test_oracle_matches_reference_inference_loop(name):
    """Every forward call of the reference's inference loop (infer.py:48-87: eval mode, update_graph(mode='test'),
    decode_tracks row deletion between calls) with the call's own inputs: ragged graphs, carried state with rows
    deleted, dets that lost all their edges."""
    gold = Golden(name)
    m = gold.meta
    assert m['kind'] == 'infer' and m['rows_deleted'] > 0
    cfg = orc.OracleConfig(m['features'], m['ncategories'], m['nhidden'], m['nattheads'], m['msg_type'])
    p = gold.params()
    with torch.no_grad():
        for c in range(gold.ncalls):
            na, ea = gold.adjacency(c, 'node_adj'), gold.adjacency(c, 'edge_adj')
            graph = orc.graph_from_adjacency(na, ea)
            h_in = gold.t(f'c{c}/h_in') if int(gold.d[f'c{c}/has_h_in']) else None
            scores, logits, h, _ = orc.forward(p, cfg, gold.t(f'c{c}/x'), h_in, graph, training=False)
            assert torch.allclose(scores, gold.t(f'c{c}/scores'), atol=SCORE_TOL, rtol=0), f'scores call {c}'
            assert torch.allclose(logits, gold.t(f'c{c}/logits'), atol=TOL, rtol=RTOL), f'logits call {c}'
            assert torch.allclose(h, gold.t(f'c{c}/h_out'), atol=TOL, rtol=RTOL), f'h_out call {c}'
            # y_pred marks the type of every row (ts == -1 on edge rows, utils/graph.py:141-145,285-287)
            assert np.array_equal(gold.d[f'c{c}/y_pred'][:, 0] == -1, graph.is_edge)


REFERENCE = '/root/reference'


@pytest.mark.skipif(not __import__('os').path.isdir(REFERENCE), reason='the reference only exists in the build container')
def test_committed_fixtures_regenerate_from_the_reference(tmp_path):
    """oracle/gen_golden.py, run against the real reference, reproduces EVERY committed fixture -- every array and the meta
    string (the .npz containers themselves carry zip timestamps and cannot be byte-compared).  This is what pins the
    fixtures (and through them the oracle) to outputs of the reference itself; it runs wherever /root/reference exists."""
    import glob
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    subprocess.run([sys.executable, os.path.join(root, 'oracle', 'gen_golden.py'), '--reference-path', REFERENCE,
                    '--out', str(tmp_path)], check=True, env=env, cwd=root, stdout=subprocess.DEVNULL)
    # (parts/: the arrays a fixture keeps in a file of their own, tests/golden_util.Golden)
    committed = sorted(glob.glob(os.path.join(root, 'tests', 'golden', '*.npz')) +
                       glob.glob(os.path.join(root, 'tests', 'golden', 'parts', '*.npz')))
    fresh = sorted(glob.glob(os.path.join(str(tmp_path), '*.npz')) + glob.glob(os.path.join(str(tmp_path), 'parts', '*.npz')))
    rel = lambda fs, base: [os.path.relpath(f, base) for f in fs]
    assert rel(fresh, str(tmp_path)) == rel(committed, os.path.join(root, 'tests', 'golden'))
    for f in committed:                                     # what the parts are for: each file of a split fixture under 1 MiB
        if os.path.basename(os.path.dirname(f)) == 'parts':
            base = os.path.join(root, 'tests', 'golden', os.path.basename(f).split('.')[0] + '.npz')
            assert os.path.getsize(f) < 2 ** 20 and os.path.getsize(base) < 2 ** 20, f
    for fc, ff in zip(committed, fresh):
        a, b = np.load(fc, allow_pickle=False), np.load(ff, allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), os.path.basename(fc)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), \
                f'{os.path.basename(fc)}: {k} differs from what the reference produces now'
