"""The host half of the input-transform shape tests: route() of tests/intf_cases.py switches where the kernels do and TABLE holds
a case on each side of every switch, the inputs are exact where the GPU file compares with torch.equal, few rows sit on the
ReLU's kink, the analytic backward is torch autograd of the float64 forward, and the ceiling of the bound is never the active
one."""
import pytest
import torch

from tests import intf_cases as ic

CASES = pytest.mark.parametrize('case', ic.TABLE, ids=lambda c: c.id)
SHAPES = sorted({(c.H, c.F, c.training) for c in ic.TABLE})


def test_ids_are_unique():
    ids = [c.id for c in ic.TABLE]
    assert len(ids) == len(set(ids))
    assert len(ic.TWICE) == 10 and len({c.id for c in ic.TWICE}) == 10


# ---- route() switches where the kernels do ----------------------------------------------------------------------------------------
def _rt(entry, H, F, segs, msr=None, training=True, dx=False, cus=256):
    return ic.route(entry, H, F, sum(segs), segs, max(segs) if msr is None else msr, training, dx, cus)


def test_route_form_switches():
    assert _rt('tf_fwd', 64, 16, (32,))['form'] == 'wave' and _rt('tf_fwd', 64, 17, (32,))['form'] == 'workgroup'
    assert _rt('tf_fwd', 64, 16, (33,))['form'] == 'workgroup' and _rt('tf_fwd', 64, 16, (5,), msr=33)['form'] == 'workgroup'
    assert _rt('tf_fwd', 32, 16, (5,))['form'] == 'workgroup' and _rt('tf_fwd', 64, 16, (5,), training=False)['form'] == 'workgroup'
    # the backward takes the workgroup form whenever a gradient with respect to x is asked for
    assert _rt('tf_bwd', 64, 16, (5,))['form'] == 'wave' and _rt('tf_bwd', 64, 16, (5,), dx=True)['form'] == 'workgroup'
    assert _rt('bn_bwd', 64, 16, (5,))['form'] == 'staged'
    with pytest.raises(AssertionError):
        _rt('tf_fwd', 64, 16, (129,))
    with pytest.raises(AssertionError):
        _rt('tf_fwd', 128, 16, (5,))


def test_route_tiles_chunks_and_groups():
    t = lambda segs: _rt('tf_fwd', 64, 8, segs)['tiles']
    assert t((31, 1)) == [[(32, 2)]] and t((31, 2)) == [[(31, 1), (2, 1)]] and t((32,)) == [[(32, 1)]]
    assert t((1,) * 8) == [[(8, 8)]] and t((1,) * 9) == [[(8, 8), (1, 1)]]
    assert t((0,) * 8 + (3,)) == [[(0, 8), (3, 1)]]
    nine = _rt('tf_fwd', 64, 8, ic.NINE_TILES)
    assert len(ic.NINE_TILES) == 64 and nine['groups'] == 1 and len(nine['tiles'][0]) == 9 and nine['tiles_per_wave'] == 2
    assert nine['tiles'][0][0] == (30, 1) and all(s == 8 for _, s in nine['tiles'][0][1:8]) and nine['tiles'][0][8][1] == 7
    assert any(r % 2 for r, _ in nine['tiles'][0])
    r65 = _rt('tf_fwd', 64, 8, ic.NINE_TILES + (5,))
    assert r65['groups'] == 2 and r65['grid'] == 2 and r65['tiles'][1] == [(5, 1)]
    c = lambda segs, H=64: _rt('tf_fwd', H, 17, segs)['tiles']
    assert c((127, 1)) == [[(128, 2)]] and c((127, 2)) == [[(127, 1), (2, 1)]] and c((128,)) == [[(128, 1)]]
    assert c((0,) * 32 + (5,)) == [[(0, 32)], [(5, 1)]]
    assert c((3, 4, 0, 0), 32) == [[(7, 4)]]
    assert _rt('tf_fwd', 64, 17, (2,) * 32)['groups'] == 1 and _rt('tf_fwd', 64, 17, (2,) * 33)['groups'] == 2
    e = lambda nd: _rt('tf_fwd', 64, 16, (nd,), msr=0, training=False)
    assert [e(nd)['groups'] for nd in (1, 127, 128, 129)] == [1, 1, 1, 2] and e(129)['tiles'] == [[(128, 1)], [(1, 1)]]


@pytest.mark.parametrize('cus', [256, 304])
def test_route_second_trip(cus):
    """The persistent loops take a second trip one segment (eval: one row) past grid * group size."""
    for entry in ('tf_fwd', 'tf_bwd'):
        w = lambda S: _rt(entry, 64, 8, (1,) * S, cus=cus)
        assert w(64 * cus)['groups_per_block'] == 1 and w(64 * cus + 1)['groups_per_block'] == 2 and w(64 * cus + 1)['grid'] == cus
        g = lambda S: _rt(entry, 64, 17, (1,) * S, cus=cus)
        assert g(32 * cus)['groups_per_block'] == 1 and g(32 * cus + 1)['groups_per_block'] == 2 and g(32 * cus + 1)['grid'] == cus
        e = lambda nd: _rt(entry, 64, 2, (nd,), msr=0, training=False, cus=cus)
        assert e(128 * cus)['groups_per_block'] == 1 and e(128 * cus + 1)['groups_per_block'] == 2


def test_route_staged():
    g = lambda H, segs, training=True: _rt('bn_fwd', H, 8, segs, training=training)['G']
    assert g(256, (255,)) == 1 and g(256, (256,)) == 4 and g(128, (256,)) == 8 and g(64, (256,)) == 16 and g(32, (256,)) == 32
    assert g(64, (1, 511)) == 16 and g(64, (1, 510)) == 1 and g(64, (300,), training=False) == 1
    s = lambda nd: _rt('bn_bwd', 64, 8, (nd,))
    assert [s(nd)['slabs'] for nd in (1, 128, 129, 8192, 8193)] == [1, 1, 2, 64, 65]
    assert [s(nd)['fold'] for nd in (128, 129, 8192, 8193)] == [False, False, False, True]


def test_table_holds_both_sides_of_every_switch():
    rts = [(c, ic.routes(c)) for c in ic.TABLE]
    for c, (f, b) in rts:
        assert f['form'] == c.form and b['form'] == (c.bwd_form or c.form), c.id
    by = lambda form, k=0: [(c, r[k]) for c, r in rts if r[k]['form'] == form]
    # wave form: every width of the issue, both x layouts, one and two tiles, the 8-segment limit, nine tiles, two groups
    wf = by('wave')
    assert {c.F for c, _ in wf} == {1, 8, 15, 16} and {c.xlist for c, _ in wf} == {True, False}
    tl = [r['tiles'] for _, r in wf]
    assert [[(1, 1)]] in tl and [[(32, 1)]] in tl and [[(32, 2)]] in tl and [[(31, 1), (2, 1)]] in tl
    assert [[(8, 8)]] in tl and [[(8, 8), (1, 1)]] in tl and [[(0, 8), (3, 1)]] in tl
    assert {r['tiles_per_wave'] for _, r in wf} >= {1, 2}
    assert any(r['groups'] == 2 and len(r['tiles'][1]) == 1 for _, r in wf)
    for k in (0, 1):
        assert {r['groups_per_block'] for _, r in by('wave', k)} == {1, 2}
        assert {r['groups_per_block'] for c, r in by('workgroup', k) if c.training} == {1, 2}
        assert {r['groups_per_block'] for c, r in by('workgroup', k) if not c.training} == {1, 2}
    S = {len(ic.seg_rows(c)) for c, _ in wf}
    assert {ic.RUNNING_CUT, ic.RUNNING_CUT + 1} <= S
    # the route switches: F = 16 / 17 and max_seg_rows = 32 / 33 at H = 64 in training mode
    t64 = [c for c in ic.TABLE if c.H == 64 and c.training and c.form != 'staged']
    assert any(c.F == 16 and c.form == 'wave' for c in t64) and any(c.F == 17 and c.form == 'workgroup' for c in t64)
    assert any(c.segs == (32,) and c.form == 'wave' for c in t64) and any(c.segs == (33,) and c.form == 'workgroup' for c in t64)
    # workgroup form: widths, modes, gradients with respect to x given and not, chunk sizes around NSUB and 4 NSUB
    wg = by('workgroup')
    assert {c.H for c, _ in wg} == {32, 64} and {c.F for c, _ in wg} >= {2, 16, 17, 128}
    assert {(c.training, c.dx) for c, _ in wg} == {(a, b) for a in (True, False) for b in (True, False)}
    for H, sizes in ((64, (1, 15, 16, 17, 63, 64, 65, 128)), (32, (1, 31, 32, 33, 127, 128))):
        have = {r['tiles'][0][0][0] for c, r in wg if c.H == H and c.training and len(ic.seg_rows(c)) == 1}
        assert set(sizes) <= have, (H, have)
    tl = [r['tiles'] for c, r in wg if c.training]
    assert [[(128, 2)]] in tl and [[(127, 1), (2, 1)]] in tl and [[(7, 4)]] in tl and [[(0, 32)], [(5, 1)]] in tl
    assert {r['groups'] for c, r in wg if c.training and c.segs[:1] == ('rand',)} >= {1, 2}
    ev = sorted(sum(ic.seg_rows(c)) for c, _ in wg if not c.training)
    assert ev == [1, 127, 128, 129, 128 * 256 + 1]
    # cross-form pairs on the nine-tile list
    assert {(c.form, c.bwd_form) for c in ic.CROSS} == {('wave', 'workgroup'), ('workgroup', 'wave')}
    assert all(c.segs == ic.NINE_TILES for c in ic.CROSS)
    # staged form
    st = by('staged', 1)
    assert {c.H for c, _ in st} == {32, 64, 128, 256}
    assert {(c.H, r['G']) for c, r in st} >= {(256, 1), (256, 4), (128, 8), (64, 16), (32, 32)}
    assert {r['slabs'] for c, r in st if c.H == 64} >= {1, 2, 64, 65} and {r['fold'] for _, r in st} == {False, True}
    assert any(0 in ic.seg_rows(c) for c, _ in st) and any(not c.training for c, _ in st)
    assert any(c.segs == (1, 511) for c, _ in st)
    assert max(sum(ic.seg_rows(c)) for c in ic.TABLE) <= 35000


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
@CASES
def test_inputs(case):
    """Lin1 in fp32 equals float64 bit for bit, by torch's product and by a term-by-term sum in another order; at most 1 % of
    the det rows are kink rows and their upstream gradient is zero; seg_cnt >= 2 and counts every det row."""
    x = ic.inputs(case)
    r64, r32 = ic.evaluate(x), ic.evaluate(x, dtype=torch.float32)
    assert torch.equal(r32.y_save.double(), r64.y_save) and torch.equal(r64.y_save.float().double(), r64.y_save)
    for t in (x.x, x.W1, x.b1, x.gamma, x.beta, x.W2, x.b2, x.d_out, x.rm0, x.rv0):
        assert torch.equal(t.float().double(), t)
    assert float(x.x.abs().max()) <= 1 and float(x.W1.abs().max()) <= ic.weight_q(case.F) / 64 and float(x.b1.abs().max()) <= 0.5
    assert float((x.x.abs() @ x.W1.abs().t()).max()) + 0.5 < 2 ** 15
    sub = slice(0, 40)
    k = torch.cat([torch.arange(case.F - 1, -1, -2), torch.arange(case.F - 2, -1, -2)])     # the odd f downwards, then the even
    acc = torch.zeros(x.x[sub].shape[0], case.H, dtype=torch.float32)
    for f in k.tolist():
        acc = acc + x.x[sub, f:f + 1].float() * x.W1[:, f].float()[None, :]
    assert torch.equal((acc + x.b1.float()).double(), r64.y_save[sub])
    assert int(x.kink.sum()) <= 0.01 * x.nd
    assert not bool(x.d_out[x.kink].any()) and torch.equal(x.kink, (r64.z.abs() < ic.KINK).any(1))
    assert int(x.seg_cnt.min()) >= 2 and bool((x.seg_cnt >= x.seg_nd).all())
    assert int(x.seg_ptr[-1]) == x.nd and x.out_row.unique().numel() == x.nd and int(x.out_row.max()) < x.N
    assert float((r64.z.abs() > 6).double().mean()) <= 0.05


@pytest.mark.parametrize('H,F,training', SHAPES)
def test_relu_inputs_take_both_signs(H, F, training):
    """Conditions on the inputs, on 60 segments of the shape's own recipe: a column whose ReLU never switches would hide a
    wrong mask, a saturated one a wrong operand."""
    case = ic.Case('workgroup', H, F, ('rand', 60, 0, 9), 'host check', training=training)
    z = ic.evaluate(ic.inputs(case)).z
    assert bool((z > 0).any(0).all()) and bool((z < 0).any(0).all())
    assert float((z.abs() > 6).double().mean()) <= 0.05


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def _autograd(x):
    """The transform on the full row set (each segment's zero rows next to its det rows) in float64, differentiated by torch."""
    g = lambda v: v.clone().requires_grad_(True)
    X, W1, b1, gamma, beta, W2, b2 = (g(v) for v in (x.x, x.W1, x.b1, x.gamma, x.beta, x.W2, x.b2))
    nz = x.seg_cnt - x.seg_nd
    segz = torch.repeat_interleave(torch.arange(x.S), nz)
    Z = torch.zeros(int(nz.sum()), x.F, dtype=torch.float64, requires_grad=True)
    yd, yz = X @ W1.t() + b1, Z @ W1.t() + b1
    if x.training:
        cnt = x.seg_cnt.double()[:, None]
        zero = torch.zeros(x.S, x.H, dtype=torch.float64)
        mean = (zero.index_add(0, x.seg_of_det, yd) + zero.index_add(0, segz, yz)) / cnt
        dd, dz = yd - mean[x.seg_of_det], yz - mean[segz]
        var = (zero.index_add(0, x.seg_of_det, dd * dd) + zero.index_add(0, segz, dz * dz)) / cnt
        yhat = dd / torch.sqrt(var[x.seg_of_det] + ic.EPS)
    else:
        yhat = (yd - x.rm0) / torch.sqrt(x.rv0 + ic.EPS)
    out = torch.relu(yhat * gamma + beta) @ W2.t() + b2
    (out * x.d_out).sum().backward()
    return dict(out=out.detach(), dW1=W1.grad, db1=b1.grad, dgamma=gamma.grad, dbeta=beta.grad, dW2=W2.grad, db2=b2.grad,
                d_xdet=X.grad, d_xzero_rows=Z.grad, segz=segz)


@CASES
def test_backward_is_autograd_and_the_ceiling_is_idle(case):
    """With the unrounded statistics the analytic backward equals autograd to 1e-10 * scale; and for every rounded quantity
    4 * err32 < ceiling * scale: the bound of the GPU file is sized by the host fp32 evaluation or the floor, never the ceiling."""
    x = ic.inputs(case)
    ex = ic.evaluate(x, exact_stats=True)
    ag = _autograd(x)
    amax = lambda t: float(t.abs().max()) if t.numel() else 0.0
    sc = lambda t: max(1.0, amax(t))
    assert amax(ex.out - ag['out']) <= 1e-10 * sc(ag['out'])
    for q in ic.GRADS + ('d_xdet',):
        assert amax(getattr(ex, q) - ag[q]) <= 1e-10 * sc(ag[q]), q
    zr = ag['d_xzero_rows'] if ag['d_xzero_rows'] is not None else torch.zeros(len(ag['segz']), case.F, dtype=torch.float64)
    assert amax(ex.d_xzero[ag['segz']] - zr) <= 1e-10 * sc(zr)
    if case.training:
        assert not bool(ex.d_xzero[x.seg_nd == 0].any())       # an empty segment's zero rows receive exactly nothing
        assert amax(ex.db1) <= 1e-10 * sc(ex.dW2)              # BatchNorm removes the bias in front of it: db1 is zero
    r64, r32 = ic.evaluate(x), ic.evaluate(x, dtype=torch.float32)
    for q in ic.ROUNDED:
        b, e32, scale = ic.bound(q, r64, r32, case.training)
        assert 4 * e32 < ic.CEILING * scale, (q, e32, scale)
        assert b < ic.CEILING * scale
