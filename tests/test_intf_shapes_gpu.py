"""The input transform of a call's new det rows in its three implementations -- the staged launches of tmpnn_input_bn_fwd / _bwd
(csrc/dense.hip), the workgroup form k_it_fwd / k_it_bwd and the wave-owned form k_itw_fwd / k_itw_bwd behind
tmpnn_input_tf_fwd / _bwd (csrc/intf.hip) -- through the C ABI against the float64 definition of tests/intf_cases.py, at the
segment lists where a tile, a chunk, a group or the grid ends, where a persistent workgroup takes a second group, where segments
hold no det row, where the route switches forms, and where the staged form switches its row groups and its split-K slabs.
tests/test_intf_cases.py asserts on the host that the table reaches each of these; every case here asserts its own route with
the device's CU count.

Lin1 is exact in fp32 on the inputs' grid: y_save is compared with torch.equal.  What is rounded (mean, rstd, the output rows,
the running statistics, the six parameter gradients, d_xdet, d_xzero) is held to intf_cases.bound(): max(FACTOR err32,
32 * 2^-24 * scale) and never past 2e-4 * scale, err32 being the error of the HOST fp32 evaluation of the same definition --
never another kernel.  Every buffer is poisoned: NaN in x outside the group's columns and the listed rows, in every output cell
a call must write, in d_h outside the listed rows' H columns, in the rows of y_save / mean / rstd beyond nd and S, and in the
workspace; every byte outside the written cells is compared with its value before the call; the parameter gradients accumulate
onto non-zero contents.  The backward reads y_save, mean and rstd of the float64 definition rounded to fp32, not a forward
kernel's."""
import functools
import os
from types import SimpleNamespace

import pytest
import torch

from tests import intf_cases as ic
from trackmpnn_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
_LOG = os.environ.get('TMPNN_INTF_SHAPES_LOG')          # a file that collects err / err32 / scale / bound / ratio per quantity


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


@functools.lru_cache(maxsize=1)
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=2)
def reference(case):
    """(inputs, the float64 definition, its host fp32 evaluation): computed once per case, shared, left unchanged."""
    x = ic.inputs(case, cus())
    return x, ic.evaluate(x), ic.evaluate(x, dtype=torch.float32)


def _pattern(shape, gen):
    """Non-zero contents on a grid of 1/16 in (-1, 1): no value that any case computes by accident, and small enough that the
    one rounding of adding onto them stays inside the floor of the bound."""
    return (torch.randint(-8, 8, shape, generator=gen).float() + 0.5) / 8


def bits(t):
    return t.contiguous().view(torch.int32)


def i32(t):
    return t.to(torch.int32).contiguous().to(DEV)


def f32(t):
    return t.float().contiguous().to(DEV)


def _sync(what):
    """A fault ends the session: nothing more is launched on a device whose context is gone."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'{what}: {e}', returncode=3)


FIELDS = ('h', 'y', 'mean', 'rstd', 'rm', 'rv', 'd_xdet', 'd_xzero') + ic.GRADS


def run(case, x, r64):
    """One forward and one backward on poisoned buffers.  Returns the buffers as they came back, on the host, with their
    contents before the calls (name + '0')."""
    H, F, nd, S, N, training = case.H, case.F, x.nd, x.S, x.N, int(case.training)
    staged = case.form == 'staged'
    lib, st = _lib.load(), _lib.raw_stream()
    gen = torch.Generator().manual_seed(91 + H + F)
    ld, Ft, SS = 2 * H + 8, F + 5, (S if training else 1)
    assert int(x.out_row.max()) < N and x.out_row.numel() == nd and int(x.seg_ptr[-1]) == nd
    longest = int(x.seg_nd.max()) if training else 0
    mf = longest if case.msr_fwd is None else case.msr_fwd
    mb = longest if case.msr_bwd is None else case.msr_bwd
    if not staged:
        assert lib.tmpnn_input_tf_supported(H, F, mf) and lib.tmpnn_input_tf_supported(H, F, mb)
    # ---- what both directions read
    w1, b1, gamma, beta, w2, b2 = (f32(v) for v in (x.W1, x.b1, x.gamma, x.beta, x.W2, x.b2))
    seg_ptr, seg_cnt, out_row = i32(x.seg_ptr), i32(x.seg_cnt), i32(x.out_row)
    seg_of_det = None if (staged and H == 32) else i32(x.seg_of_det)        # (NULL: the staged form searches seg_ptr)
    if case.xlist:
        assert not staged and int(x.x_rows.max()) < x.NX
        xb = torch.full((x.NX, Ft), NAN)
        xb[x.x_rows, 1:1 + F] = x.x.float()
        x_rows = x.x_rows.contiguous().to(DEV)
    else:
        xb = torch.full((nd, Ft), NAN)
        xb[:, 1:1 + F] = x.x.float()
        x_rows = None
    xD = xb.to(DEV)
    r = SimpleNamespace()
    # ---- forward
    r.cells = torch.zeros(N, ld, dtype=torch.bool)
    r.cells[x.out_row, H:2 * H] = True
    r.h0 = _pattern((N, ld), gen)
    r.h0[r.cells] = NAN
    r.y0, r.mean0, r.rstd0 = _pattern((nd + 3, H), gen), _pattern((SS + 2, H), gen), _pattern((SS + 2, H), gen)
    r.y0[:nd], r.mean0[:SS], r.rstd0[:SS] = NAN, NAN, NAN
    r.rm0, r.rv0 = x.rm0.float(), x.rv0.float()
    h, y, mean, rstd, rm, rv = (v.to(DEV) for v in (r.h0, r.y0, r.mean0, r.rstd0, r.rm0, r.rv0))
    params = (w1.data_ptr(), b1.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), w2.data_ptr(),
              b2.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    segs = (seg_ptr.data_ptr(), seg_cnt.data_ptr(), _lib.ptr(seg_of_det), S)
    if staged:
        ws_a = torch.full((nd, H), NAN, device=DEV)
        _lib.call('tmpnn_input_bn_fwd', xD.data_ptr() + 4, Ft, F, nd, *segs, H, training, *params, ws_a.data_ptr(),
                  out_row.data_ptr(), h.data_ptr() + 4 * H, ld, st)
    else:
        _lib.call('tmpnn_input_tf_fwd', xD.data_ptr() + 4, _lib.ptr(x_rows), Ft, F, nd, *segs, mf, H, training, *params,
                  out_row.data_ptr(), h.data_ptr() + 4 * H, ld, st)
    _sync(f'{case.id} forward')
    r.h, r.y, r.mean, r.rstd, r.rm, r.rv = (v.cpu() for v in (h, y, mean, rstd, rm, rv))
    # ---- backward, from the float64 forward's saved tensors rounded to fp32 (NaN in the rows beyond nd and S)
    ys, mg, rg = torch.full((nd + 3, H), NAN), torch.full((SS + 2, H), NAN), torch.full((SS + 2, H), NAN)
    ys[:nd], mg[:SS], rg[:SS] = r64.y_save.float(), r64.mean.float(), r64.rstd.float()
    d_h = torch.full((N, ld), NAN)
    d_h[x.out_row, H:2 * H] = x.d_out.float()
    ysD, mgD, rgD, d_hD = ys.to(DEV), mg.to(DEV), rg.to(DEV), d_h.to(DEV)
    shapes = dict(dW1=(H, F), db1=(H,), dgamma=(H,), dbeta=(H,), dW2=(H, H), db2=(H,))
    g = {}
    for q in ic.GRADS:
        setattr(r, q + '0', _pattern(shapes[q], gen))
        g[q] = getattr(r, q + '0').to(DEV)
    r.dcells = torch.zeros(nd + 3, Ft, dtype=torch.bool)
    r.dcells[:nd, 1:1 + F] = True
    r.d_xdet0, r.d_xzero0 = _pattern((nd + 3, Ft), gen), _pattern((S + 2, F), gen)
    r.d_xdet0[r.dcells] = NAN
    r.d_xzero0[:S] = NAN
    d_xdet, d_xzero = r.d_xdet0.to(DEV), r.d_xzero0.to(DEV)
    dx = ((d_xdet.data_ptr() + 4) if case.dx else None, Ft, d_xzero.data_ptr() if case.dx else None)
    gp = tuple(g[q].data_ptr() for q in ic.GRADS)
    bparams = (w1.data_ptr(), b1.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w2.data_ptr(), ysD.data_ptr(), mgD.data_ptr(),
               rgD.data_ptr(), out_row.data_ptr(), d_hD.data_ptr() + 4 * H, ld, *dx, *gp)
    if staged:
        wsn = int(lib.tmpnn_input_bn_bwd_ws(nd, S, H, F))
        ws = torch.full((wsn + 4,), NAN, device=DEV)
        _lib.call('tmpnn_input_bn_bwd', xD.data_ptr() + 4, Ft, F, nd, *segs, H, training, *bparams, ws.data_ptr(), wsn, st)
    else:
        wsb = int(lib.tmpnn_input_tf_bwd_ws(nd, S, H, F, training))
        ws = torch.full((wsb // 4 + 4,), NAN, device=DEV)
        _lib.call('tmpnn_input_tf_bwd', xD.data_ptr() + 4, _lib.ptr(x_rows), Ft, F, nd, *segs, mb, H, training, *bparams,
                  ws.data_ptr(), wsb, st)
    _sync(f'{case.id} backward')
    r.d_xdet, r.d_xzero = d_xdet.cpu(), d_xzero.cpu()
    for q in ic.GRADS:
        setattr(r, q, g[q].cpu())
    return r


def check(what, case, x, r64, r32, r):
    """Every quantity of one run is measured and printed, then everything is asserted."""
    H, F, nd, S = case.H, case.F, x.nd, x.S
    SS = S if case.training else 1
    ratios, missed = {}, []

    def held(qty, got, prev=None):
        b, e32, scale = ic.bound(qty, r64, r32, case.training)
        ref = getattr(r64, qty)
        want = ref if prev is None else ref + prev.double()
        err = float((got.double() - want).abs().max()) if ref.numel() else 0.0
        ratios[qty] = (err, e32, scale, b)
        if not err <= b:                                         # (NaN compares false)
            missed.append(f'{qty} is {err:.3e} from float64, bound {b:.3e} (host fp32 {e32:.3e}, scale {scale:.3g})')

    def same(ok, text):
        if not ok:
            missed.append(text)

    # -- rounded
    held('mean', r.mean[:SS])
    held('rstd', r.rstd[:SS])
    held('out', r.h[x.out_row, H:2 * H])
    held('run_mean', r.rm)
    held('run_var', r.rv)
    for q in ic.GRADS:
        held(q, getattr(r, q), prev=getattr(r, q + '0'))
    if case.dx:
        held('d_xdet', r.d_xdet[:nd, 1:1 + F])
        held('d_xzero', r.d_xzero[:S])
    for q, (e, e32, scale, b) in ratios.items():
        line = (f'{what} {q} err={e:.3e} err32={e32:.3e} scale={scale:.3g} bound={b:.3e} '
                f'ratio={e / e32 if e32 else float("nan"):.2f}')
        print(line)
        if _LOG:
            with open(_LOG, 'a') as f:
                f.write(line + '\n')
    # -- exact: Lin1, and every byte outside the written cells
    assert torch.equal(r64.y_save.float().double(), r64.y_save)
    same(torch.equal(r.y[:nd], r64.y_save.float()), 'y_save differs from the float64 Lin1')
    same(torch.equal(bits(r.y[nd:]), bits(r.y0[nd:])), 'y_save changed beyond nd rows')
    same(torch.equal(bits(r.h)[~r.cells], bits(r.h0)[~r.cells]), 'h_new changed outside out_row x [0, H)')
    same(torch.equal(bits(r.mean[SS:]), bits(r.mean0[SS:])), 'mean changed beyond its rows')
    same(torch.equal(bits(r.rstd[SS:]), bits(r.rstd0[SS:])), 'rstd changed beyond its rows')
    if not case.training:
        same(torch.equal(bits(r.rm), bits(r.rm0)) and torch.equal(bits(r.rv), bits(r.rv0)), 'eval mode changed the running statistics')
    if case.dx:
        same(torch.equal(bits(r.d_xdet)[~r.dcells], bits(r.d_xdet0)[~r.dcells]), 'd_xdet changed outside its rows x [0, F)')
        same(torch.equal(bits(r.d_xzero[S:]), bits(r.d_xzero0[S:])), 'd_xzero changed beyond S rows')
        empty = (x.seg_nd == 0) if case.training else torch.ones(S, dtype=torch.bool)
        same(torch.equal(r.d_xzero[:S][empty], torch.zeros(int(empty.sum()), F)), 'd_xzero of a segment without det rows is not 0')
    else:
        same(torch.equal(bits(r.d_xdet), bits(r.d_xdet0)) and torch.equal(bits(r.d_xzero), bits(r.d_xzero0)),
             'd_xdet / d_xzero written although not asked for')
    assert not missed, f'{what}: ' + '; '.join(missed)


def _routes(case):
    """The case's routes with the device's CU count; asserts that it still reaches the branch it is there for."""
    fwd, bwd = ic.routes(case, cus())
    assert fwd['form'] == case.form and bwd['form'] == (case.bwd_form or case.form), (case.id, fwd['form'], bwd['form'])
    if case.segs[0] in ('cus', 'rows_cus'):
        assert fwd['groups_per_block'] == 2 and bwd['groups_per_block'] == 2 and fwd['grid'] == cus()
    return fwd, bwd


@pytest.mark.parametrize('case', ic.TABLE, ids=lambda c: c.id)
def test_case(case):
    fwd, bwd = _routes(case)
    x, r64, r32 = reference(case)
    check(f'{case.id} [{fwd["form"]} / {bwd["form"]}]', case, x, r64, r32, run(case, x, r64))


@pytest.mark.parametrize('case', ic.TWICE, ids=lambda c: c.id)
def test_two_runs_give_equal_bytes(case):
    """Every output of both directions, byte for byte: the wave combine, the slab order and the fold are deterministic."""
    _routes(case)
    x, r64, _ = reference(case)
    a, b = run(case, x, r64), run(case, x, r64)
    for f in FIELDS:
        assert torch.equal(bits(getattr(a, f)), bits(getattr(b, f))), f
