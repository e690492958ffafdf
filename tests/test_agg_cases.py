"""CPU checks of tests/agg_cases.py: every graph of the family lands on the branch of csrc/agg.hip that
tests/test_agg_shapes_gpu.py relies on it for, and the float64 reference equals the dense matrix definition."""
import pytest
import torch

from tests import agg_cases as ac
from trackmpnn_amd.graph import build_seg_plan, dense_static_graph


@pytest.mark.parametrize('name', sorted(ac.FAMILY))
def test_family_sizes_and_launch_shape(name):
    _, E, Dn, deep = ac.FAMILY[name]
    g = ac.graph(name)
    assert (g.E, g.Dn, g.N) == (E, Dn, E + Dn)
    assert ac.is_deep(g) == deep
    # src row < edge row < dst row, rows of either type ascending (graph_from_edges checked the first already)
    assert bool((g.src < g.edge_row).all()) and bool((g.edge_row < g.dst).all())


def test_family_edges_of_the_deep_rule():
    g24, g25 = ac.graph('k24x24'), ac.graph('k24x25')
    assert 2 * g24.E == 24 * g24.Dn                    # the last shallow graph ...
    assert 2 * g25.E == 24 * g25.Dn + 24               # ... and the first deep one
    assert ac.degree_set(g24) == {24}
    assert ac.degree_set(g25) == {24, 25}


def test_family_degrees():
    assert ac.degree_set(ac.graph('pair')) == {1}
    assert ac.degree_set(ac.graph('no_edges')) == {0}
    assert ac.degree_set(ac.graph('star_out')) == {0, 1, 1000}
    assert ac.degree_set(ac.graph('star_in')) == {1, 1000}
    assert ac.degree_set(ac.graph('mid3x33')) == {33, 66}
    rg = ac.graph('ragged')
    ds = ac.degree_set(rg)
    assert (min(ds), max(ds)) == (3, 53)
    assert rg.det_order is not None and sorted(rg.det_order.tolist()) == list(range(rg.Dn))
    for name in ('ladder131', 'ladder70_sparse'):
        assert ac.graph(name).det_order is None
    s, d = ac.degrees(ac.graph('ladder131'))
    assert set(s[:131].tolist()) == set(range(131)) and set(d[131:].tolist()) == set(range(1, 131))
    s, d = ac.degrees(ac.graph('ladder70_sparse'))
    both = set(s.tolist()) | set(d.tolist())
    assert both == set(range(70))
    # the hub of star_in meets every edge as its dst: every incidence of its run carries the sign bit
    g = ac.graph('star_in')
    s, d = ac.degrees(g)
    assert int(d[-1]) == 1000 and int(s[-1]) == 0
    # middle dets of mid3x33 carry both signs
    s, d = ac.degrees(ac.graph('mid3x33'))
    assert int(((s > 0) & (d > 0)).sum()) == 33


@pytest.mark.parametrize('name,deep', [('ladder131', True), ('ladder70_sparse', False)])
def test_ladders_cover_the_pass_edges(name, deep):
    """Run lengths 0, 1, P - 1, P, P + 1, 2P - 1, 2P, 2P + 1 exist for the pass width of every H on the graph's launch shape."""
    g = ac.graph(name)
    assert ac.is_deep(g) == deep
    widths = [ac.pass_width(H, deep) for H in ac.HS]
    assert widths == ([64, 32, 16, 8] if deep else [32, 16, 8, 4])
    ds = ac.degree_set(g)
    for P in widths:
        assert ac.pass_edges(P) <= ds, (P, sorted(ac.pass_edges(P) - ds))
    # and, with either sign alone (a run of only +1 / only -1 incidences of that length)
    s, d = ac.degrees(g)
    for P in widths:
        assert ac.pass_edges(P) <= set(s.tolist())
        assert (ac.pass_edges(P) - {0}) <= set(d.tolist())


def test_passes_of_the_top_degree():
    assert ac.passes(0, 32, False) == 1
    assert [ac.passes(130, H, True) for H in ac.HS] == [3, 5, 9, 17]
    assert [ac.passes(69, H, False) for H in ac.HS] == [3, 5, 9, 18]
    assert [ac.passes(1000, H, False) for H in ac.HS] == [32, 63, 125, 250]
    assert [ac.passes(53, H, False) for H in ac.HS] == [2, 4, 7, 14]


def test_path_graph():
    g = ac.path_graph(45)
    assert (g.Dn, g.E, g.N) == (45, 44, 89)
    assert not ac.is_deep(g) and ac.degree_set(g) == {1, 2}
    assert g.edge_row.tolist() == list(range(1, 89, 2))


def _dense_matrices(g):
    pos = g.pos.long()
    Ap = torch.zeros(g.Dn, g.E, dtype=torch.float64)
    Am = torch.zeros(g.Dn, g.E, dtype=torch.float64)
    e = torch.arange(g.E)
    Ap[pos[g.src.long()], e] = 1.0
    Am[pos[g.dst.long()], e] = 1.0
    return Ap, Am


@pytest.mark.parametrize('name', ['pair', 'k24x25', 'mid3x33'])
def test_reference_equals_the_dense_definition(name):
    g = ac.graph(name)
    H = 8
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(g.N, 2 * H, generator=gen, dtype=torch.float64)
    Ap, Am = _dense_matrices(g)
    xe = x[g.edge_row.long()]
    tol = dict(rtol=0, atol=1e-12)
    assert torch.allclose(ac.ref_segsum(g, x[:, :H]), (Ap - Am) @ xe[:, :H], **tol)
    assert torch.allclose(ac.ref_concat_bwd(g, x), Ap @ xe[:, :H] + Am @ xe[:, H:], **tol)
    xd = x[g.det_row.long()]
    assert torch.equal(ac.ref_gather_diff(g, x[:, :H]), (Ap - Am).t() @ xd[:, :H])      # (one +1 and one -1 per row: exact)
    assert torch.equal(ac.ref_gather_concat(g, x[:, :H]), torch.cat([Ap.t() @ xd[:, :H], Am.t() @ xd[:, :H]], 1))
    assert torch.allclose(ac.segsum_abs(g, x[:, :H]), (Ap + Am) @ xe[:, :H].abs(), **tol)
    assert torch.allclose(ac.segsum_abs(g, x, concat=True), Ap @ xe[:, :H].abs() + Am @ xe[:, H:].abs(), **tol)
    # row_limit: rows >= limit count as zero; >= N: every row counts
    lim = int(g.edge_row[g.E // 2])
    xz = x.clone()
    xz[lim:] = 0
    assert torch.equal(ac.ref_segsum(g, x[:, :H], lim), ac.ref_segsum(g, xz[:, :H]))
    assert torch.equal(ac.ref_concat_bwd(g, x, lim), ac.ref_concat_bwd(g, xz))
    assert torch.equal(ac.ref_segsum(g, x[:, :H], g.N + 5), ac.ref_segsum(g, x[:, :H]))
    assert torch.equal(ac.ref_segsum(g, x[:, :H], 0), torch.zeros(g.Dn, H, dtype=torch.float64))


def test_reference_does_not_use_the_csr():
    """A graph whose rowptr / inc are scrambled gives the same reference: the kernel's CSR is not its own witness."""
    g = ac.fresh_graph('k24x25')
    x = torch.randn(g.N, 8, generator=torch.Generator().manual_seed(2))
    want = ac.ref_segsum(g, x)
    g.rowptr = torch.zeros_like(g.rowptr)
    g.inc = torch.zeros_like(g.inc)
    assert torch.equal(ac.ref_segsum(g, x), want)


def test_bounds():
    n = torch.tensor([0, 1, 1000])
    gm = ac.gamma(n)
    assert gm[0] == 0 and abs(float(gm[1]) - 2.0 ** -24) < 1e-14 and 1000 * 2.0 ** -24 < float(gm[2]) < 1001 * 2.0 ** -24
    g = ac.graph('star_out')
    b = ac.segsum_bound(g, torch.ones(g.Dn, 1, dtype=torch.float64), accumulate=False)
    assert float(b[0]) == 0.0                           # an isolated det: exact zeros, no allowance
    assert float(ac.gather_bound(torch.tensor([1.0]), torch.tensor([-2.0]), torch.tensor([4.0]))) == 14 * 2.0 ** -24


def _item_sizes(plan):
    return sorted(set(plan.items[:, 1].tolist()))


def _partial_rows(plan):
    return torch.diff(plan.rowptr2.long())


@pytest.mark.parametrize('T,D', sorted(ac.DENSE))
def test_dense_graphs_get_a_plan(T, D):
    g = dense_static_graph(T, D)
    assert g.E == ac.DENSE[(T, D)]
    assert g.E >= 8192 and g.E >= 32 * g.Dn            # what dense_seg_plan asks before it builds one
    plan = build_seg_plan(g)
    assert plan is not None
    fill = g.E / (128.0 * plan.T)
    assert 0.73 <= fill <= 0.85, fill                   # border tiles with -1 slots (0.799, 0.736, 0.846, 0.839)
    assert int((plan.t_row < 0).sum()) == 128 * plan.T - g.E
    parts = _partial_rows(plan)
    s, d = ac.degrees(g)
    if (T, D) == (2, 107):
        assert plan.T == 112 and _item_sizes(plan) == [1, 13]
        # dst indices 107..213 span eight groups of 16: a src det has eight partial rows, exactly ONE pass of the second kernel
        assert sorted(set(parts.tolist())) == [2, 8] and ac.passes(8, 256, True) == 1
    elif (T, D) == (3, 70):
        assert plan.T == 104 and _item_sizes(plan) == [5, 9, 10, 13]
        assert int(((s > 0) & (d > 0)).sum()) == 70     # dets with both signs
        assert sorted(set(parts.tolist())) == [1, 2, 5, 7]
    elif (T, D) == (3, 99):
        # a middle det: seven partial rows as a src (dst indices 198..296 span seven groups), then one as a dst -- the only
        # graph of the set whose second pass has a NEGATIVE entry in the last slot (u = 7) of a pass
        assert sorted(set(parts.tolist())) == [1, 2, 7, 8]
        mid = torch.arange(D, 2 * D)
        assert bool((parts[mid] == 8).all())
        assert bool((plan.inc2[plan.rowptr2.long()[mid] + 7] < 0).all()) and bool((plan.inc2[plan.rowptr2.long()[mid] + 6] >= 0).all())
    else:
        # dst indices 139..277 span ten groups of 16: a src det has ten partial rows, so the DUAL second pass (8 rows a pass at
        # H = 256) takes TWO passes
        assert plan.T == 180 and _item_sizes(plan) == [5, 13]
        assert sorted(set(parts.tolist())) == [2, 10] and ac.passes(10, 256, True) == 2


def test_ladder131_gets_a_plan_too():
    """Recorded: build_seg_plan(ladder131) at the default min_fill returns a plan (89 tiles, 0.75 full), and the graph passes
    dense_seg_plan's size test (E >= 8192, E >= 32 Dn).  tests/test_agg_shapes_gpu.py therefore runs it both ways at H = 256:
    without a plan attached (k_segsum_pipe) and with one (the dense form on a triangular edge set: items and partial-row
    counts of every size, dets with no partial row at all)."""
    g = ac.graph('ladder131')
    assert g.E >= 8192 and g.E >= 32 * g.Dn
    plan = build_seg_plan(g)
    assert plan is not None and plan.T == 89 and plan.I == 12
    parts = _partial_rows(plan)
    assert int(parts.min()) == 0 and int(parts.max()) >= 9
    assert '_seg_plan' not in g.__dict__                # (the shared graph itself stays without one)
