"""The gather and segment-sum kernels of csrc/agg.hip (k_gather_pipe, every instantiation of k_segsum_pipe, k_segsum_tiles)
through the C ABI, against the float64 definitions of tests/agg_cases.py, on graphs at the kernels' branch points: both launch
shapes, run lengths at and around one and two passes for every H, empty runs, det_order on and off, chunk tails, the
grid-stride leg, 256-column slices of wide rows, the dense form with one and with two second passes.

Integer rows ([-8, 8], degree <= 1000: every partial sum is an exactly representable integer) are compared with torch.equal;
random rows with the derived bound gamma_n * sum |addends| (segment sums, any order) and 2u (|a| + |b| + |p|) (gathers).
Every buffer is poisoned: NaN in every row and column of the input the operation must not read (row 0 is a det row: the dead
pipeline slots of k_segsum_pipe load it), NaN in the output cells a plain launch must overwrite, and every other byte of the
output is compared with its value before the call."""
from types import SimpleNamespace

import pytest
import torch

from tests import agg_cases as ac
from trackmpnn_amd import _lib
from trackmpnn_amd.graph import dense_seg_plan, dense_static_graph, set_det_groups

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
HS = ac.HS
TO_DETS = {'segsum_fwd': 'tmpnn_segsum_fwd', 'live': 'tmpnn_segsum_fwd_live', 'gdiff_bwd': 'tmpnn_gather_diff_bwd',
           'gconcat_bwd': 'tmpnn_gather_concat_bwd'}
TO_EDGES = {'gdiff_fwd': 'tmpnn_gather_diff_fwd', 'gconcat_fwd': 'tmpnn_gather_concat_fwd', 'segsum_bwd': 'tmpnn_segsum_bwd'}


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


_ON_DEVICE = {}


def graphs(name):
    """(the family's host graph, its device copy): both shared, neither modified."""
    g = ac.graph(name)
    if name not in _ON_DEVICE:
        _ON_DEVICE[name] = g.to(DEV)
    return g, _ON_DEVICE[name]


def _values(kind, shape, gen):
    if kind == 'int':
        return torch.randint(-8, 9, shape, generator=gen).float()
    return torch.randn(shape, generator=gen)


def check_op(op, g, gd, H, kind, acc=False, compact=False, pad=0, limit=None, seed=0):
    """One call of `op` on poisoned buffers, asserted against the float64 definition.  pad = 4: the operand starts 4 floats into a
    wider row (a pointer 16 bytes past the buffer's).  Returns the whole output buffer, the values of its target cells and the
    operand's valued rows."""
    to_dets = op in TO_DETS
    concat = op in ('gconcat_bwd', 'gconcat_fwd')
    in_w = 2 * H if op == 'gconcat_bwd' else H
    out_w = 2 * H if op == 'gconcat_fwd' else H
    in_ld, out_ld = pad + in_w + 4, pad + out_w + 8
    er, dr = g.edge_row.long(), g.det_row.long()
    gen = torch.Generator().manual_seed(1000 * seed + H)
    valued = er if to_dets else dr
    vals = _values(kind, (valued.numel(), in_w), gen)
    xin = torch.full((g.N, in_ld), NAN)                       # the other row type and the columns beyond the operand: NaN
    xin[valued, pad:pad + in_w] = vals
    xop = torch.zeros(g.N, in_w)
    xop[valued] = vals
    if limit is not None:
        xin[max(limit, 0):] = NAN                             # rows >= row_limit are promised to be zero and must stay unread
    out_rows = g.Dn if (to_dets and compact) else g.N
    target = torch.arange(g.Dn) if (to_dets and compact) else (dr if to_dets else er)
    out0 = torch.randint(-99, 100, (out_rows, out_ld), generator=gen).float() + 0.25      # no value any case computes
    prev = torch.randint(-8, 9, (target.numel(), out_w), generator=gen).float() if acc else None
    out0[target, pad:pad + out_w] = prev if acc else NAN
    # float64 definition and the bound for random rows
    if to_dets:
        ref = ac.ref_concat_bwd(g, xop, limit) if concat else ac.ref_segsum(g, xop, limit)
        mag = ac.segsum_abs(g, xop, concat, limit)
        if acc:
            ref, mag = ref + prev.double(), mag + prev.double().abs()
        bound = ac.segsum_bound(g, mag, acc)
    else:
        a, b = xop[g.src.long()], xop[g.dst.long()]
        if concat:
            ref = ac.ref_gather_concat(g, xop)
            bound = ac.gather_bound(torch.cat([a, b], 1), torch.zeros(g.E, 2 * H), prev)
        else:
            ref = ac.ref_gather_diff(g, xop)
            bound = ac.gather_bound(a, b, prev)
        if acc:
            ref = ref + prev.double()
    xd, od = xin.to(DEV), out0.to(DEV)
    st = _lib.raw_stream()
    head = (gd.cref(), xd.data_ptr() + 4 * pad, in_ld, od.data_ptr() + 4 * pad, out_ld, H)
    if op == 'segsum_fwd':
        _lib.call(TO_DETS[op], *head, int(acc), int(compact), st)
    elif op == 'live':
        assert not acc
        _lib.call(TO_DETS[op], *head, int(compact), int(limit), st)
    else:
        assert not compact
        _lib.call((TO_DETS if to_dets else TO_EDGES)[op], *head, int(acc), st)
    torch.cuda.synchronize()
    got = od.cpu()
    what = f'{op} H={H} {kind} acc={int(acc)} compact={int(compact)} pad={pad} limit={limit}'
    cells = torch.zeros(out_rows, out_ld, dtype=torch.bool)
    cells[target, pad:pad + out_w] = True
    assert torch.equal(got.view(torch.int32)[~cells], out0.view(torch.int32)[~cells]), f'{what}: bytes outside the target cells changed'
    val = got[target, pad:pad + out_w]
    if kind == 'int':
        if not torch.equal(val, ref.float()):
            bad = torch.nonzero((val != ref.float()).any(1)).flatten()
            raise AssertionError(f'{what}: {bad.numel()} of {target.numel()} rows differ, first at target index {bad[:8].tolist()}')
    else:
        err = (val.double() - ref).abs()
        ok = err <= bound                                     # (NaN compares false)
        if not bool(ok.all()):
            bad = torch.nonzero(~ok.all(1)).flatten()
            raise AssertionError(f'{what}: {bad.numel()} rows beyond the bound, first {bad[:8].tolist()}, '
                                 f'max err {err[bad].max().item():.3e} vs bound {bound[bad].max().item():.3e}')
    return SimpleNamespace(buf=got, val=val, operand=vals)


MODES4 = [(False, False), (False, True), (True, False), (True, True)]      # (accumulate, compact)


# ---- 1. tmpnn_segsum_fwd: every graph, every mode ------------------------------------------------------------------------------
@pytest.mark.parametrize('H', HS)
@pytest.mark.parametrize('name', sorted(ac.FAMILY))
def test_segsum_fwd(name, H):
    g, gd = graphs(name)
    for kind in ('int', 'rand'):
        for acc, compact in MODES4:
            check_op('segsum_fwd', g, gd, H, kind, acc, compact)
    check_op('segsum_fwd', g, gd, H, 'int', False, False, pad=4)
    check_op('segsum_fwd', g, gd, H, 'rand', True, True, pad=4)


# ---- 2. the gathers' backward: segment sums with signs +1/-1 and with column offsets 0/H --------------------------------------
@pytest.mark.parametrize('H', HS)
@pytest.mark.parametrize('name', ['ladder131', 'ladder70_sparse', 'star_in', 'mid3x33', 'no_edges'])
def test_gather_bwd(name, H):
    g, gd = graphs(name)
    for op in ('gdiff_bwd', 'gconcat_bwd'):
        for kind in ('int', 'rand'):
            for acc in (False, True):
                check_op(op, g, gd, H, kind, acc)
        check_op(op, g, gd, H, 'int', True, pad=4)


# ---- 3. tmpnn_segsum_fwd_live: rows >= row_limit stay unread ------------------------------------------------------------------
def live_limits(g):
    """0; the first edge row; edge rows inside the edge block (some dets get whole dead passes, others a live and a dead half
    inside one pass); N - 1; N; N + 5 (the last two read every row: the plain launch)."""
    er = g.edge_row.tolist()
    return [0, er[0], er[g.E // 3], er[g.E // 2], er[g.E // 2 + 37], g.N - 1, g.N, g.N + 5]


@pytest.mark.parametrize('H', HS)
@pytest.mark.parametrize('name', ['ladder131', 'ladder70_sparse', 'star_out'])
def test_segsum_live(name, H):
    g, gd = graphs(name)
    for i, limit in enumerate(live_limits(g)):
        check_op('live', g, gd, H, 'int', compact=bool(i & 1), limit=limit)
        check_op('live', g, gd, H, 'rand', compact=not (i & 1), limit=limit)
    check_op('live', g, gd, H, 'int', limit=g.edge_row.tolist()[g.E // 2], pad=4)


# ---- 4. the gathers and tmpnn_segsum_bwd ---------------------------------------------------------------------------------------
GATHER_GRAPHS = ['pair', 'no_edges', 'star_out', 'k24x25', 'ragged']      # E below one block, off a chunk, several chunks


@pytest.mark.parametrize('H', HS)
@pytest.mark.parametrize('name', GATHER_GRAPHS)
def test_gathers_fwd(name, H):
    g, gd = graphs(name)
    for op in ('gdiff_fwd', 'gconcat_fwd', 'segsum_bwd'):
        for kind in ('int', 'rand'):
            for acc in (False, True):
                check_op(op, g, gd, H, kind, acc)
        check_op(op, g, gd, H, 'int', True, pad=4)


@pytest.mark.parametrize('H', HS)
@pytest.mark.parametrize('name', GATHER_GRAPHS)
def test_segsum_bwd_is_gather_diff_fwd_and_the_adjoint_of_segsum_fwd(name, H):
    g, gd = graphs(name)
    for kind in ('int', 'rand'):
        for acc in (False, True):
            a = check_op('segsum_bwd', g, gd, H, kind, acc, seed=3)
            b = check_op('gdiff_fwd', g, gd, H, kind, acc, seed=3)
            assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), (kind, acc)
    # <segsum_fwd(x), y> = <x, segsum_bwd(y)>, both sides in float64 from the device results: exact on integer rows
    for seed in (5, 6):
        f = check_op('segsum_fwd', g, gd, H, 'int', seed=seed)          # operand x on the edge rows, val on the dets
        bw = check_op('segsum_bwd', g, gd, H, 'int', seed=seed + 10)    # operand y on the dets, val on the edge rows
        lhs = (f.val.double() * bw.operand.double()).sum().item()
        rhs = (f.operand.double() * bw.val.double()).sum().item()
        assert lhs == rhs, (lhs, rhs)


# ---- 5. det_order changes the order of visiting dets, never a bit of a result -------------------------------------------------
def _order_variants(name):
    plain = ac.fresh_graph(name)
    plain.det_order, plain._c = None, None
    gen = torch.Generator().manual_seed(7)
    grouped = set_det_groups(ac.fresh_graph(name), torch.randint(0, 7, (plain.Dn,), generator=gen))
    assert sorted(grouped.det_order.tolist()) == list(range(plain.Dn)) and grouped.det_order.tolist() != list(range(plain.Dn))
    out = [plain, grouped]
    own = ac.graph(name)
    if own.det_order is not None:
        out.append(own)
    return [(v, v.to(DEV)) for v in out]


@pytest.mark.parametrize('name', ['ladder131', 'ladder70_sparse', 'ragged'])
def test_det_order_changes_no_bit(name):
    variants = _order_variants(name)
    assert variants[0][1].det_order is None and variants[1][1].det_order is not None
    for H in HS:
        for op, kind, acc, compact in (('segsum_fwd', 'int', False, False), ('segsum_fwd', 'rand', False, True),
                                       ('segsum_fwd', 'rand', True, False), ('gconcat_bwd', 'rand', False, False),
                                       ('gdiff_bwd', 'int', True, False)):
            outs = [check_op(op, v, vd, H, kind, acc, compact, seed=9).buf for v, vd in variants]
            for o in outs[1:]:
                assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32)), (op, H, kind, acc, compact)
        g, _ = variants[0]
        lim = g.edge_row.tolist()[g.E // 2]
        outs = [check_op('live', v, vd, H, 'rand', limit=lim, seed=9).buf for v, vd in variants]
        for o in outs[1:]:
            assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32)), ('live', H)


# ---- 7. the dense form (k_segsum_tiles + k_segsum_pipe<DUAL>) against the formula ----------------------------------------------
_DENSE_ON_DEVICE = {}


def dense_graphs(key):
    """(host graph, device graph with its seg plan attached).  key: (T, D) of dense_static_graph or a name of the family."""
    if key not in _DENSE_ON_DEVICE:
        g = dense_static_graph(*key) if isinstance(key, tuple) else ac.fresh_graph(key)
        gd = g.to(DEV)
        plan = dense_seg_plan(gd)
        assert plan is not None and plan.T > 0 and 128 * plan.T > g.E        # (border tiles have empty slots)
        assert gd.cstruct().seg_plan
        _DENSE_ON_DEVICE[key] = (g, gd)
    return _DENSE_ON_DEVICE[key]


# (2, 107): items of 13 tiles and of one, a second pass that is exactly full (8 partial rows); (3, 70): dets with both signs;
# (3, 99): a NEGATIVE partial row in the last slot of the second pass; (2, 139): ten partial rows, two second passes;
# ladder131: a triangular edge set -- items and partial-row counts of every size, a det with no partial row at all
DENSE_KEYS = sorted(ac.DENSE) + ['ladder131']


@pytest.mark.parametrize('key', DENSE_KEYS, ids=lambda k: k if isinstance(k, str) else 'dense%dx%d' % k)
def test_dense_form(key):
    g, gd = dense_graphs(key)
    for kind in ('int', 'rand'):
        for acc, compact in MODES4:
            check_op('segsum_fwd', g, gd, 256, kind, acc, compact)
    check_op('segsum_fwd', g, gd, 256, 'int', False, True, pad=4)
    check_op('segsum_fwd', g, gd, 256, 'rand', True, False, pad=4)


def test_dense_form_and_csr_kernel_in_one_call():
    """H = 384 on a graph with a plan: columns 0..255 take the dense form, the last 128 k_segsum_pipe."""
    g, gd = dense_graphs((2, 107))
    for kind, acc, compact in (('int', False, False), ('int', True, True), ('rand', False, True), ('rand', True, False)):
        check_op('segsum_fwd', g, gd, 384, kind, acc, compact)
    check_op('segsum_fwd', g, gd, 384, 'int', False, False, pad=4)


# ---- 6. repeatability: one graph per launch shape ------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['shallow', 'deep', 'live_shallow', 'live_deep', 'dense', 'gather'])
def test_two_launches_give_equal_bytes(shape):
    name = 'ladder131' if shape in ('deep', 'live_deep') else 'ladder70_sparse'
    g, gd = dense_graphs((2, 139)) if shape == 'dense' else graphs('ragged' if shape == 'gather' else name)
    for H in ((256,) if shape == 'dense' else HS):
        for acc in (False, True):
            if shape.startswith('live'):
                if acc:
                    continue
                kw = dict(op='live', limit=g.edge_row.tolist()[g.E // 2])
            else:
                kw = dict(op='gdiff_fwd' if shape == 'gather' else 'segsum_fwd', acc=acc)
            a = check_op(g=g, gd=gd, H=H, kind='rand', seed=4, **kw)
            b = check_op(g=g, gd=gd, H=H, kind='rand', seed=4, **kw)
            assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), (shape, H, acc)


# ---- 8. wide rows: 256-column slices -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [384, 640])
@pytest.mark.parametrize('name', ['ladder131', 'ragged'])
def test_wide_rows_in_slices(name, H):
    g, gd = graphs(name)
    for op in ('segsum_fwd', 'gdiff_bwd', 'gdiff_fwd', 'segsum_bwd'):
        check_op(op, g, gd, H, 'int', False)
        check_op(op, g, gd, H, 'rand', True, pad=4)
    check_op('segsum_fwd', g, gd, H, 'int', True, True)
    check_op('live', g, gd, H, 'int', limit=g.edge_row.tolist()[g.E // 2])


def test_concat_forms_at_wide_rows():
    """tmpnn_gather_concat_fwd keeps the four widths: at H = 384 it returns an error that names the width and writes nothing.
    tmpnn_gather_concat_bwd is sliced like the others (include/tmpnn.h: the second half stays H columns further on), so it is
    held to the formula instead."""
    g, gd = graphs('ladder131')
    H = 384
    x = torch.ones(g.N, H + 4, device=DEV)
    out = torch.full((g.N, 2 * H + 8), 3.25, device=DEV)
    with pytest.raises(RuntimeError, match='384'):
        _lib.call('tmpnn_gather_concat_fwd', gd.cref(), x.data_ptr(), H + 4, out.data_ptr(), 2 * H + 8, H, 0, _lib.raw_stream())
    torch.cuda.synchronize()
    assert bool((out == 3.25).all())
    for kind, acc in (('int', False), ('rand', True)):
        check_op('gconcat_bwd', g, gd, H, kind, acc)
    check_op('gconcat_bwd', g, gd, H, 'int', True, pad=4)


# ---- 9. the grid-stride leg: more chunks than grid_for's 16 384 blocks ----------------------------------------------------------
def test_grid_stride_leg():
    """A path det, edge, det, ... with Dn = 16384 * 32 + 40: tmpnn_segsum_fwd at H = 32 (32 dets a block) leaves the last 40 dets
    to the second stride of k_segsum_pipe<., 4, 32>, tmpnn_gather_diff_fwd at H = 256 (4 rows x 8 in flight = 32 edges a block)
    the last 39 edges to the second stride of k_gather_pipe.  Integer rows, reference by torch index ops on the device (exact
    sums: their order does not matter).  The only large case (about 3 GB of device memory)."""
    Dn = 16384 * 32 + 40
    g = ac.path_graph(Dn, device=DEV)
    assert (g.Dn, g.E) == (Dn, Dn - 1) and not ac.is_deep(g)
    er, dr, src, dst = g.edge_row.long(), g.det_row.long(), g.src.long(), g.dst.long()
    st = _lib.raw_stream()
    gen = torch.Generator(device=DEV).manual_seed(1)

    def buffers(H, valued, target):
        x = torch.full((g.N, H + 4), NAN, device=DEV)
        x[valued, :H] = torch.randint(-8, 9, (valued.numel(), H), generator=gen, device=DEV).float()
        out = torch.full((g.N, H + 8), 77.25, device=DEV)
        out[target, :H] = NAN
        return x, out

    H = 32
    x, out = buffers(H, er, dr)
    full = torch.zeros(g.N, H, device=DEV)
    full.index_add_(0, src, x[er, :H])
    full.index_add_(0, dst, -x[er, :H])
    exp = torch.full_like(out, 77.25)
    exp[dr, :H] = full[dr]
    _lib.call('tmpnn_segsum_fwd', g.cref(), x.data_ptr(), H + 4, out.data_ptr(), H + 8, H, 0, 0, st)
    torch.cuda.synchronize()
    assert torch.equal(out[dr[-64:]], exp[dr[-64:]]), 'the dets of the second stride'
    assert torch.equal(out, exp)
    del x, out, exp, full

    H = 256
    x, out = buffers(H, dr, er)
    exp = torch.full_like(out, 77.25)
    exp[er, :H] = x[src, :H] - x[dst, :H]
    _lib.call('tmpnn_gather_diff_fwd', g.cref(), x.data_ptr(), H + 4, out.data_ptr(), H + 8, H, 0, st)
    torch.cuda.synchronize()
    assert torch.equal(out[er[-64:]], exp[er[-64:]]), 'the edges of the second stride'
    assert torch.equal(out, exp)


# ---- 10. argument checks that need no launch -----------------------------------------------------------------------------------
def test_argument_checks():
    g, gd = graphs('k24x25')
    H = 64
    x = torch.ones(g.N, 2 * H + 16, device=DEV)
    out = torch.full((g.N, 2 * H + 16), 3.25, device=DEV)
    st = _lib.raw_stream()
    xp, op, ld = x.data_ptr(), out.data_ptr(), 2 * H + 16
    bad = [
        ('tmpnn_segsum_fwd', (xp, ld - 2, op, ld, H, 0, 0, st)),               # ld no multiple of 4 floats
        ('tmpnn_segsum_fwd', (xp, ld, op, ld - 2, H, 0, 0, st)),
        ('tmpnn_gather_diff_fwd', (xp, ld - 2, op, ld, H, 0, st)),
        ('tmpnn_segsum_fwd', (xp + 4, ld, op, ld, H, 0, 0, st)),               # a pointer 4 bytes off 16-byte alignment
        ('tmpnn_segsum_fwd', (xp, ld, op + 4, ld, H, 0, 0, st)),
        ('tmpnn_gather_concat_fwd', (xp + 4, ld, op, ld, H, 0, st)),
        ('tmpnn_segsum_bwd', (xp, ld, op + 4, ld, H, 0, st)),
        ('tmpnn_gather_concat_bwd', (xp, 2 * H - 4, op, ld, H, 0, st)),        # ld_in < H + cneg
        ('tmpnn_gather_concat_fwd', (xp, ld, op, 2 * H - 4, H, 0, st)),        # ld_out < 2H
        ('tmpnn_segsum_fwd', (xp, H - 4, op, ld, H, 0, 0, st)),                # ld_in < H
        ('tmpnn_segsum_fwd_live', (xp, ld, op, ld, H, 0, -1, st)),             # row_limit < 0
        ('tmpnn_segsum_fwd', (xp, ld, op, ld, 48, 0, 0, st)),                  # a width no kernel serves
        ('tmpnn_segsum_fwd', (None, ld, op, ld, H, 0, 0, st)),
    ]
    for name, args in bad:
        with pytest.raises(RuntimeError):
            _lib.call(name, gd.cref(), *args)
    # wide rows: the WHOLE row must fit the leading dimension, not just each 256-column slice of it
    W = 384
    xw = torch.ones(g.N, 2 * W, device=DEV)
    ow = torch.full((g.N, 2 * W), 3.25, device=DEV)
    for name, args in [('tmpnn_segsum_fwd', (xw.data_ptr(), 260, ow.data_ptr(), W, W, 0, 0, st)),
                       ('tmpnn_segsum_fwd', (xw.data_ptr(), W, ow.data_ptr(), 260, W, 0, 0, st)),
                       ('tmpnn_gather_diff_fwd', (xw.data_ptr(), W, ow.data_ptr(), 260, W, 0, st)),
                       ('tmpnn_segsum_bwd', (xw.data_ptr(), 260, ow.data_ptr(), W, W, 0, st)),
                       ('tmpnn_gather_diff_bwd', (xw.data_ptr(), W, ow.data_ptr(), 260, W, 0, st)),
                       ('tmpnn_gather_concat_bwd', (xw.data_ptr(), 2 * W - 128, ow.data_ptr(), W, W, 0, st)),
                       ('tmpnn_segsum_fwd_live', (xw.data_ptr(), 260, ow.data_ptr(), W, W, 0, 5, st))]:
        with pytest.raises(RuntimeError, match='leading dimension'):
            _lib.call(name, gd.cref(), *args)
    torch.cuda.synchronize()
    assert bool((out == 3.25).all()) and bool((ow == 3.25).all())
