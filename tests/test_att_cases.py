"""CPU checks of tests/att_cases.py: every graph lands on the branches of csrc/att.hip that tests/test_att_shapes_gpu.py relies
on it for, the CSR position map agrees with src / dst, the inputs keep ha and the scores exact in fp32 (and the hot scaling
really is hot), and the float64 definition equals a dense N x N evaluation written from the formula."""
import numpy as np
import pytest
import torch

from oracle import trackmpnn_oracle as orc
from tests import agg_cases as ac
from tests import att_cases as tc

ALL = list(tc.SMALL) + sorted(tc.LARGE)
FAMILY_CASES, HEAD_CASES, HOT_CASES, GRID_CASES = tc.FAMILY_CASES, tc.HEAD_CASES, tc.HOT_CASES, tc.GRID_CASES


@pytest.mark.parametrize('name', ALL)
def test_graphs_land_where_the_table_says(name):
    g = tc.graph(name)
    if name in tc.SIZES:
        assert (g.E, g.Dn) == tc.SIZES[name]
    else:
        assert (g.E, g.Dn) == ac.FAMILY[name][1:3]
    s, d = ac.degrees(g)
    deg = torch.unique(s + d).tolist()
    for H in tc.HS:
        assert (tc.run_classes(deg, H), tc.mixed_waves(g, H)) == tc.TABLE[name][H], H
    assert (g.det_order is not None) == (name == 'ragged')


def _gpu_cases():
    return {(n, H, K) for n, H, K, _ in FAMILY_CASES + HEAD_CASES + HOT_CASES + GRID_CASES}


def test_grid_caps():
    """The three grid legs exceed exactly the caps they are there for; no other case of the GPU file exceeds any."""
    for n, H, K in sorted(_gpu_cases()):
        g = tc.graph(n)
        assert tc.caps_exceeded(g.E, g.Dn, H, K) == tc.CAPS.get((n, H, K), set()), (n, H, K)
    assert tc.CAPS[('path16400', 256, 1)] == {'dotk'}
    assert tc.CAPS[('dense2x257', 256, 5)] == {'score'}
    assert tc.CAPS[('path524328', 32, 1)] >= {'fwd'}
    # the thresholds themselves (csrc/att.hip)
    assert tc.caps_exceeded(65536, 10, 256, 5) == set() and tc.caps_exceeded(65537, 10, 256, 5) == {'score'}
    assert tc.caps_exceeded(4 * 65536, 10, 256, 2) == set() and tc.caps_exceeded(4 * 65536 + 1, 10, 256, 1) == {'score'}
    assert tc.caps_exceeded(0, 16384, 256, 1) == set() and tc.caps_exceeded(0, 16385, 256, 1) == {'dotk'}
    assert tc.caps_exceeded(0, 524288, 256, 1) == {'dotk'} and tc.caps_exceeded(0, 524289, 256, 1) == {'dotk', 'fwd'}


def test_ladders_hold_every_run_length():
    """ladder131 holds 0, 1, lpr - 1, lpr, lpr + 1, 2 lpr - 1, 2 lpr, 2 lpr + 1 for all four widths (lpr = 8, 16, 32, 64) and a
    run of three chunks or more for the first three; ladder70_sparse (top degree 69) for lpr = 8, 16, 32 -- at lpr = 64 its
    runs stop at lpr + 5."""
    for name, widths in (('ladder131', tc.HS), ('ladder70_sparse', (32, 64, 128))):
        for H in widths:
            assert tc.ALL_TO_2L1 <= tc.TABLE[name][H][0], (name, H)
    assert tc.TABLE['ladder70_sparse'][256][0] == {'0', '1', 'l-1', 'l', 'l+1'}
    for H in (32, 64, 128):
        assert '3l+' in tc.TABLE['ladder131'][H][0]


def test_star_out_hub_has_short_neighbours():
    """The hub (degree 1000) shares its wave with isolated dets at H = 32, 64 and 128, and with dets of degree 1 at H = 32:
    the wave's loops run to 1000 while its neighbours have nothing, or one position, to do."""
    g = tc.graph('star_out')
    want = {32: {0, 1, 1000}, 64: {0, 1000}, 128: {0, 1000}, 256: {1000}}
    for H in tc.HS:
        w = tc.wave_runs(g, H)
        hub = w[(w == 1000).any(1)]
        assert hub.shape[0] == 1 and set(hub[0].tolist()) == want[H], H


@pytest.mark.parametrize('name', ALL)
def test_position_map_agrees_with_src_and_dst(name):
    """Position p of det d's run (rowptr[d] <= p < rowptr[d + 1]) maps to (e, side) with d = the src (side 0) / dst (side 1) of
    edge e, and every (e, side) has exactly one position."""
    g = tc.graph(name)
    e, side = tc.position_map(g)
    assert e.numel() == 2 * g.E
    owner = torch.repeat_interleave(torch.arange(g.Dn), torch.diff(g.rowptr.long()))
    sp, dp = tc.det_index(g)
    assert torch.equal(owner, torch.where(side == 0, sp[e], dp[e]))
    assert torch.equal(torch.sort(2 * e + side).values, torch.arange(2 * g.E))
    assert torch.equal(g.det_row.long()[sp], g.src.long()) and torch.equal(g.det_row.long()[dp], g.dst.long())
    # keep_bytes / to_positions / from_positions are that map
    x = torch.arange(2 * g.E, dtype=torch.float32).reshape(1, g.E, 2)
    assert torch.equal(tc.from_positions(g, tc.to_positions(g, x)), x)


@pytest.mark.parametrize('name,H,K,hot', FAMILY_CASES + HEAD_CASES + HOT_CASES + GRID_CASES[:2],
                         ids=lambda v: str(v))
def test_inputs_are_exact(name, H, K, hot):
    """ha and t evaluated in fp32 equal their float64 values bit for bit, and the sums of absolute addends leave room in 24
    bits: every summation order (the bf16x6 products included) gives the same fp32 value."""
    g = tc.graph(name)
    x = tc.inputs(g, H, K, hot)
    assert float(x.h.abs().max()) <= 1 and torch.equal(x.h * 8, (x.h * 8).round())
    assert float(x.W.abs().max()) <= 0.5 and torch.equal(x.W * 8, (x.W * 8).round())
    amax, astep = (2.0, 4) if hot else (0.25, 32)
    assert float(x.a.abs().max()) <= amax and torch.equal(x.a * astep, (x.a * astep).round())
    ex = tc.exactness(g, x)
    assert ex.ha_equal and ex.t_equal
    assert ex.ha_room < 2.0 ** 18 and ex.t_room < ex.t_limit
    if hot:
        assert ex.score_max > 89 and ex.score_min < -17, (ex.score_max, ex.score_min)


def test_inputs_are_exact_on_the_large_path():
    g = tc.graph('path524328')
    ex = tc.exactness(g, tc.inputs(g, 32, 1))
    assert ex.ha_equal and ex.t_equal and ex.t_room < ex.t_limit


def test_ties_occur():
    """Exact zeros of ha_s - ha_d (sgn(0) = 0) occur by the thousand, and of t (the kink: slope 0.2 at 0) a few times."""
    g = tc.graph('ladder131')
    ex = tc.exactness(g, tc.inputs(g, 256, 8))
    assert ex.diff_zeros > 1000 and ex.t_zeros >= 1
    ex = tc.exactness(g, tc.inputs(g, 32, 8))
    assert ex.diff_zeros > 1000 and ex.t_zeros >= 1


def _dense_evaluation(g, x, keep, d_es):
    """The formula with N x N matrices (models/layers.py:26-43 as include/tmpnn.h states it), float64, one head at a time:
    S[d, e] = score of edge e where det d is an endpoint of it, -inf elsewhere; a masked softmax over the rows; dropout; times
    the signed incidence; times h of the edge rows."""
    K, H = x.a.shape
    N = g.N
    h = x.h.double().requires_grad_(True)
    W = x.W.double().requires_grad_(True)
    a = x.a.double().requires_grad_(True)
    src, dst, er, dr = g.src.long(), g.dst.long(), g.edge_row.long(), g.det_row.long()
    inc = torch.zeros(N, N, dtype=torch.float64)                  # det row x edge row: +1 src, -1 dst
    inc[src, er] = 1.0
    inc[dst, er] = -1.0
    esk, alphas = [], []
    for k in range(K):
        ha = h @ W[k]
        s = torch.nn.functional.leaky_relu((ha[src] - ha[dst]).abs() @ a[k], 0.2)
        S = torch.full((N, N), -float('inf'), dtype=torch.float64)
        S = S.index_put((src, er), s).index_put((dst, er), s)
        live = (inc != 0).any(1)
        A = torch.zeros(N, N, dtype=torch.float64)
        A = A.index_put((torch.nonzero(live).flatten(),), torch.softmax(S[live], 1))
        if keep is not None:
            M = torch.zeros(N, N, dtype=torch.float64)
            M[src, er] = keep[k, :, 0].double() * 2.0
            M[dst, er] = keep[k, :, 1].double() * 2.0
            A = A * M
        alphas.append(torch.stack([A[src, er], A[dst, er]], 1).detach())
        esk.append(((A * inc) @ h)[dr] / K)
    es = sum(esk)
    (es * d_es.double()).sum().backward()
    return torch.stack(esk).detach(), torch.stack(alphas), h.grad, W.grad, a.grad


@pytest.mark.parametrize('name,training', [('pair', False), ('pair', True), ('k24x24', False), ('k24x24', True),
                                           ('ladder12', False), ('ladder12', True)])
def test_definition_equals_the_dense_evaluation(name, training):
    g = ac.ladder(12, iso_a=2, iso_b=1) if name == 'ladder12' else ac.graph(name)
    H, K = 8, 3
    x = tc.inputs(g, H, K)
    x.h = x.h + torch.randn(g.N, H, generator=torch.Generator().manual_seed(3)) * 0.1        # (off the grid: generic values)
    keep = tc.draw_keep(g, K) if training else None
    d_es = tc.draw_d_es(g, H)
    r = tc.evaluate(g, x, keep, d_es)
    esk, alpha, d_h, dW, da = _dense_evaluation(g, x, keep, d_es)
    tol = dict(rtol=0, atol=1e-12)
    assert torch.allclose(r.esk, esk, **tol) and torch.allclose(r.es, esk.sum(0), **tol)
    assert torch.allclose(r.alpha, alpha, **tol)
    assert torch.allclose(r.d_h, d_h, **tol) and torch.allclose(r.dW, dW, **tol) and torch.allclose(r.da, da, **tol)
    # isolated dets aggregate to 0 and report (max, sum exp) = (0, 1); a softmax row sums to 1 before dropout
    s, d = ac.degrees(g)
    iso = (s + d) == 0
    if name == 'ladder12':
        assert int(iso.sum()) == 4
    assert bool((r.es[iso] == 0).all()) and bool((r.mx[:, iso] == 0).all()) and bool((r.den[:, iso] == 1).all())
    if not training and g.E:
        sp, dp = tc.det_index(g)
        tot = torch.zeros(K, g.Dn, dtype=torch.float64).index_add(1, torch.cat([sp, dp]), torch.cat([r.alpha[..., 0], r.alpha[..., 1]], 1))
        assert torch.allclose(tot[:, ~iso], torch.ones(K, int((~iso).sum()), dtype=torch.float64), **tol)


def test_definition_equals_the_oracle_head():
    """oracle._attention in float64, head by head: the same es and alpha."""
    g = ac.graph('mid3x33')
    H, K = 32, 2
    x = tc.inputs(g, H, K)
    keep = tc.draw_keep(g, K)
    r = tc.evaluate(g, x, keep)
    og = orc.OracleGraph(g.N, g.is_edge.numpy().astype(bool), g.src.numpy().astype(np.int64), g.dst.numpy().astype(np.int64),
                         g.edge_row.numpy().astype(np.int64), g.det_row.numpy().astype(np.int64))
    p = {f'gat.{k}.W_att': x.W[k].double() for k in range(K)}
    p.update({f'gat.{k}.a': x.a[k].double().reshape(H, 1) for k in range(K)})
    for k in range(K):
        es, al = orc._attention(p, '', k, x.h.double(), og, keep[k].to(torch.uint8))
        assert torch.allclose(es[g.det_row.long()] / K, r.esk[k], rtol=0, atol=1e-12)
        assert torch.allclose(al, r.alpha[k], rtol=0, atol=1e-12)


def test_definition_does_not_use_the_csr():
    g = ac.fresh_graph('mid3x33')
    x = tc.inputs(g, 32, 2)
    d_es = tc.draw_d_es(g, 32)
    want = tc.evaluate(g, x, None, d_es)
    g.rowptr = torch.zeros_like(g.rowptr)
    g.inc = torch.zeros_like(g.inc)
    got = tc.evaluate(g, x, None, d_es)
    for f in ('ha', 'score', 'mx', 'den', 'alpha', 'esk', 'es', 'd_h', 'dW', 'da'):
        assert torch.equal(getattr(got, f), getattr(want, f)), f


def test_bound():
    ref = torch.tensor([0.5, -3.0], dtype=torch.float64)
    b, e32, scale = tc.bound(ref, ref.float())
    assert (e32, scale) == (0.0, 3.0) and b == 96 * 2.0 ** -24
    b, e32, _ = tc.bound(ref, torch.tensor([0.5, -3.0 + 2.0 ** -10]))
    assert e32 == 2.0 ** -10 and b == 2.0 ** -8
    assert 32 * 2.0 ** -24 < 2e-4                          # never looser than the stage checks' absolute 2e-4 * scale
