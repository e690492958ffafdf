"""The GRU cell kernels of csrc/gru_fwd.hip and csrc/gru_bwd.hip through the C ABI (tmpnn_gru_fwd, tmpnn_gru_bwd_data,
tmpnn_gru_bwd_weights, tmpnn_rows_linear, tmpnn_gru_fwd_tiles, tmpnn_gru_fwd_tiles_zero_state) against the float64 definition
of tests/gru_cases.py, at the row counts where the dispatch switches kernels or instantiations (CT = 1 -> 2, NT = 1 -> 4),
where a persistent grid passes its cap and leaves blocks without an item, where whole items lie beyond R, and where the
weight slabs fold.  tests/test_gru_cases.py asserts on the host that the table reaches each of these.

The inputs sit on a grid (gru_cases.inputs) on which every pre-activation is exact in fp32 in any summation order and under any
bf16 split: the hn plane and the projection P are compared with torch.equal.  What is rounded (h_out, r, z, n, the head
partials, d_msg, d_h, dW_ih, dW_hh, db_ih, db_hh) is held to gru_cases.bound(): max(FACTOR err32, 32 * 2^-24 * scale) and never
past the node cell's tolerances, err32 being the error of the HOST fp32 evaluation of the same definition -- never another
kernel.  Every buffer is poisoned: NaN in the other feature group's columns of the state and in every spare column, in every
output cell a call must write, in the rows of every input table outside the list, and in the workspace; every byte outside the
written cells is compared with its value before the call; the weight gradients accumulate onto non-zero contents.  The
backward entries read gate planes taken from the float64 definition rounded to fp32, not a forward kernel's."""
import functools
import os
from types import SimpleNamespace

import pytest
import torch

from tests import gru_cases as gc
from trackmpnn_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
_LOG = os.environ.get('TMPNN_GRU_SHAPES_LOG')           # a file that collects err_kernel / err32 per quantity and case


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


@functools.lru_cache(maxsize=2)
def reference(case, up=None, fuse=False, zero_state=False):
    """(inputs, the float64 definition, its host fp32 evaluation): computed once per case, shared, left unchanged."""
    x = gc.inputs(case)
    return (x, gc.evaluate(case, x, up=up, fuse=fuse, zero_state=zero_state),
            gc.evaluate(case, x, dtype=torch.float32, up=up, fuse=fuse, zero_state=zero_state))


def _pattern(shape, gen):
    """Non-zero contents on a grid of 1/16 in (-1, 1): no value that any case computes by accident, and small enough that the
    one rounding of adding onto them stays inside the floor of the bound."""
    return (torch.randint(-8, 8, shape, generator=gen).float() + 0.5) / 8


def bits(t):
    return t.contiguous().view(torch.int32)


def i32(t):
    return t.to(torch.int32).contiguous().to(DEV)


def _state(case, x, zero_state=False):
    """[N, 2H + 8]: the cell's group second, NaN in every other column."""
    H = case.H
    hfull = torch.full((x.N, 2 * H + 8), NAN)
    hfull[:, H:2 * H] = x.h.float()
    if zero_state:
        hfull[x.rows, H:2 * H] = 0.0
    return hfull.to(DEV)


def _compact_msg(case, x):
    m = torch.full((case.R, case.IN + 4), NAN)
    m[:, :case.IN] = x.msg.float()
    return m.to(DEV)


def _edge_tiles(x, R):
    from trackmpnn_amd.graph import build_edge_tiles
    g = SimpleNamespace(src_pos=i32(x.src), dst_pos=i32(x.dst), edge_row=i32(x.rows), E=R, Dn=gc.DN, device=torch.device(DEV))
    return build_edge_tiles(g, 32, 4, 8, stats=True, order='rows')


# ---- forward --------------------------------------------------------------------------------------------------------------------
def run_fwd(case, x, via='entry', zero_state=False):
    """One forward on poisoned buffers (xmode 3: tmpnn_rows_linear first).  `via`: tmpnn_gru_fwd, or one of the tiled entries
    over the same rows.  Returns the buffers as they came back, on the host, with their contents before the call."""
    H, IN, xmode, R, N = case.H, case.IN, case.xmode, case.R, x.N
    lib, st = _lib.load(), _lib.raw_stream()
    ld = 2 * H + 8
    gen = torch.Generator().manual_seed(77 + H + xmode)
    hD = _state(case, x, zero_state)
    h_ptr = hD.data_ptr() + 4 * H
    off = 1 if case.misalign else 0
    r = SimpleNamespace(off=off)
    r.cells = torch.zeros(N, ld, dtype=torch.bool)
    r.cells[x.rows, H + off:2 * H + off] = True
    r.out0 = _pattern((N, ld), gen)
    r.out0[r.cells] = NAN
    r.gates0 = _pattern((4, N, H), gen)
    r.gates0[:, x.rows] = NAN
    nparts = 0 if case.misalign else lib.tmpnn_gru_fwd_head_parts(H, IN, xmode)
    assert nparts == (0 if case.misalign else gc.fwd_head_parts(H, IN, xmode))
    r.parts0 = _pattern((max(nparts, 1), N), gen)
    if nparts:
        r.parts0[:, x.rows] = NAN
    out, gates, parts = r.out0.to(DEV), r.gates0.to(DEV), r.parts0.to(DEV)
    f = lambda t: t.float().contiguous().to(DEV)
    wih_t, whh_t, b_ih, b_hh, w_head = f(x.W_ih.t()), f(x.W_hh.t()), f(x.b_ih), f(x.b_hh), f(x.w_head)
    rows = i32(x.rows)
    src, dst = (i32(x.src), i32(x.dst)) if xmode else (None, None)
    msg, ld_msg = None, IN
    if xmode == 0:
        msg, ld_msg = _compact_msg(case, x), IN + 4
    elif xmode == 3:
        r.proj0 = torch.full((gc.DN, 3 * H + 4), NAN)
        msg, ld_msg = r.proj0.to(DEV), 3 * H + 4
        _lib.call('tmpnn_rows_linear', i32(x.dets).data_ptr(), gc.DN, h_ptr, ld, H, wih_t.data_ptr(), 3 * H, msg.data_ptr(), ld_msg, st)
        torch.cuda.synchronize()
        r.proj = msg.cpu()
    head = (w_head.data_ptr(), parts.data_ptr(), N) if nparts else (None, None, 0)
    if via == 'entry':
        _lib.call('tmpnn_gru_fwd', rows.data_ptr(), R, xmode, _lib.ptr(src), _lib.ptr(dst), _lib.ptr(msg), ld_msg, 1, IN, h_ptr, ld, H,
                  wih_t.data_ptr(), whh_t.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), out.data_ptr() + 4 * (H + off), ld,
                  gates.data_ptr(), N * H, *head, st)
    else:
        tiles = _edge_tiles(x, R)
        assert tiles.max_dets > 24                          # (the gather path of big tiles is exercised)
        if via == 'tiles':
            _lib.call('tmpnn_gru_fwd_tiles', tiles.cref(), R, msg.data_ptr(), ld_msg, h_ptr, ld, H, whh_t.data_ptr(), b_ih.data_ptr(),
                      b_hh.data_ptr(), out.data_ptr() + 4 * H, ld, gates.data_ptr(), N * H, *head, st)
        else:
            assert zero_state and lib.tmpnn_gru_fwd_tiles_zero_state_available(H, 3)
            _lib.call('tmpnn_gru_fwd_tiles_zero_state', tiles.cref(), R, msg.data_ptr(), ld_msg, H, b_ih.data_ptr(), b_hh.data_ptr(),
                      out.data_ptr() + 4 * H, ld, gates.data_ptr(), N * H, 1, *head, st)
    torch.cuda.synchronize()
    r.out, r.gates, r.parts, r.nparts = out.cpu(), gates.cpu(), parts.cpu(), nparts
    return r


def _held(qty, got, ref64, ref32, ratios, prev=None):
    """got against float64 (+ what the buffer held before, for an accumulated gradient: the bound is the gradient's own)."""
    b, e32, scale = gc.bound(qty, ref64, ref32)
    want = ref64 if prev is None else ref64 + prev.double()
    err = float((got.double() - want).abs().max()) if ref64.numel() else 0.0
    ratios[qty] = (err, e32, scale, b)
    if not err <= b:                                         # (NaN compares false; every quantity is measured before any fails)
        return [f'{qty} is {err:.3e} from float64, bound {b:.3e} (host fp32 {e32:.3e}, scale {scale:.3g})']
    return []


def _finish(what, ratios, missed):
    for q, (e, e32, scale, b) in ratios.items():
        line = (f'{what} {q} err={e:.3e} err32={e32:.3e} scale={scale:.3g} bound={b:.3e} '
                f'ratio={e / e32 if e32 else float("nan"):.2f}')
        print(line)
        if _LOG:
            with open(_LOG, 'a') as f:
                f.write(line + '\n')
    assert not missed, f'{what}: ' + '; '.join(missed)


def check_fwd(what, case, x, r64, r32, r):
    """Every assertion on one forward run's buffers."""
    H, rows = case.H, x.rows
    # -- exact: the projection, the hn plane
    if case.xmode == 3:
        assert torch.equal(r64.P.float().double(), r64.P)
        assert torch.equal(r.proj[:, :3 * H], r64.P.float()), f'{what}: P differs from the float64 product'
        assert torch.equal(bits(r.proj[:, 3 * H:]), bits(r.proj0[:, 3 * H:])), f'{what}: P changed beyond its 3H columns'
    assert torch.equal(r64.hn.float().double(), r64.hn)
    assert torch.equal(r.gates[3][rows], r64.hn.float()), f'{what}: the hn plane differs from W_hn h + b_hn'
    # -- every byte outside the written cells
    assert torch.equal(bits(r.out)[~r.cells], bits(r.out0)[~r.cells]), f'{what}: h_out changed outside the list rows\' H columns'
    listed = torch.zeros(x.N, dtype=torch.bool)
    listed[rows] = True
    assert torch.equal(bits(r.gates)[:, ~listed], bits(r.gates0)[:, ~listed]), f'{what}: a gate plane changed outside the list rows'
    assert torch.equal(bits(r.parts)[:, ~listed], bits(r.parts0)[:, ~listed]), f'{what}: head partials changed outside the list rows'
    if not r.nparts:
        assert torch.equal(bits(r.parts), bits(r.parts0))
    # -- rounded
    ratios = {}
    missed = _held('h_out', r.out[rows, H + r.off:2 * H + r.off], r64.h_out, r32.h_out, ratios)
    for k, q in enumerate(('r', 'z', 'n')):
        missed += _held(q, r.gates[k][rows], getattr(r64, q), getattr(r32, q), ratios)
    if r.nparts:
        missed += _held('parts', r.parts[:, rows].t(), r64.parts, r32.parts, ratios)
    _finish(what, ratios, missed)


@pytest.mark.parametrize('case', gc.FWD, ids=lambda c: c.id)
def test_forward(case):
    x, r64, r32 = reference(case)
    rt = gc.route('fwd', case.H, case.IN, case.xmode, case.R, aligned=not case.misalign)
    check_fwd(f'{case.id} [{rt["family"]}]', case, x, r64, r32, run_fwd(case, x))


# ---- backward, data -----------------------------------------------------------------------------------------------------------------
def _bwd_inputs(case, x, r64, up):
    """What both backward entries read: state, gate planes of the float64 definition rounded to fp32 (NaN outside the list
    rows), and the upstream gradient in the form `up` (d_hout NaN outside the list rows' H columns, dy NaN outside the list)."""
    H, N, rows = case.H, x.N, x.rows
    b = SimpleNamespace(hD=_state(case, x))
    g = torch.full((4, N, H), NAN)
    for k, q in enumerate(('r', 'z', 'n', 'hn')):
        g[k, rows] = getattr(r64, q).float()
    b.gates = g.to(DEV)
    b.d_hout = b.dy = None
    if up & 1:
        d = torch.full((N, H + 4), NAN)
        d[rows, :H] = x.d_hout.float()
        b.d_hout = d.to(DEV)
    if up & 2:
        d = torch.full((N,), NAN)
        d[rows] = x.dy[rows].float()
        b.dy = d.to(DEV)
    b.w_head = x.w_head.float().to(DEV)
    b.rows = i32(rows)
    return b


def run_bwd_data(case, x, r64, up, fuse):
    H, IN, R, N = case.H, case.IN, case.R, x.N
    ld = 2 * H + 8
    gen = torch.Generator().manual_seed(79 + H + IN)
    b = _bwd_inputs(case, x, r64, up)
    r = SimpleNamespace()
    r.d_msg0, r.d_h0 = _pattern((N, IN + 4), gen), _pattern((N, ld), gen)
    r.d_msg0[x.rows, :IN] = NAN
    r.d_h0[x.rows, H:2 * H] = NAN
    d_msg, d_h = r.d_msg0.to(DEV), r.d_h0.to(DEV)
    w_ih, w_hh = x.W_ih.float().contiguous().to(DEV), x.W_hh.float().contiguous().to(DEV)
    add = src = dst = None
    if fuse:
        a = torch.full((N, H + 8), NAN)                      # read at the endpoints, which are never list rows
        a[:, :H] = x.add.float()
        a[x.rows] = NAN
        add, src, dst = a.to(DEV), i32(x.src), i32(x.dst)
    _lib.call('tmpnn_gru_bwd_data', b.rows.data_ptr(), R, IN, b.hD.data_ptr() + 4 * H, ld, H, w_ih.data_ptr(), w_hh.data_ptr(),
              b.gates.data_ptr(), N * H, _lib.ptr(b.d_hout), H + 4, _lib.ptr(b.dy), b.w_head.data_ptr() if up & 2 else None,
              d_msg.data_ptr(), IN + 4, d_h.data_ptr() + 4 * H, ld, _lib.ptr(src), _lib.ptr(dst), _lib.ptr(add), H + 8,
              _lib.raw_stream())
    torch.cuda.synchronize()
    r.d_msg, r.d_h = d_msg.cpu(), d_h.cpu()
    return r


def check_bwd_data(what, case, x, r64, r32, r):
    H, IN, rows = case.H, case.IN, x.rows
    cells = torch.zeros(x.N, IN + 4, dtype=torch.bool)
    cells[rows, :IN] = True
    assert torch.equal(bits(r.d_msg)[~cells], bits(r.d_msg0)[~cells]), f'{what}: d_msg changed outside the list rows\' IN columns'
    cells = torch.zeros(x.N, 2 * H + 8, dtype=torch.bool)
    cells[rows, H:2 * H] = True
    assert torch.equal(bits(r.d_h)[~cells], bits(r.d_h0)[~cells]), f'{what}: d_h changed outside the list rows\' H columns'
    ratios = {}
    missed = _held('d_msg', r.d_msg[rows, :IN], r64.d_msg, r32.d_msg, ratios)
    missed += _held('d_h', r.d_h[rows, H:2 * H], r64.d_h, r32.d_h, ratios)
    _finish(what, ratios, missed)


@pytest.mark.parametrize('case', gc.BWD_DATA, ids=lambda c: c.id)
def test_backward_data(case):
    rt = gc.route('bwd_data', case.H, case.IN, case.xmode, case.R)
    for up, fuse in gc.up_fuse_of(case):
        x, r64, r32 = reference(case, up, fuse)
        what = f'{case.id} UP={up} fuse={int(fuse)} [{rt["family"]}]'
        check_bwd_data(what, case, x, r64, r32, run_bwd_data(case, x, r64, up, fuse))


# ---- backward, weights --------------------------------------------------------------------------------------------------------------
def run_bwd_weights(case, x, r64, up):
    H, IN, xmode, R, N = case.H, case.IN, case.xmode, case.R, x.N
    ld = 2 * H + 8
    gen = torch.Generator().manual_seed(83 + H + IN)
    b = _bwd_inputs(case, x, r64, up)
    r = SimpleNamespace(dW_ih0=_pattern((3 * H, IN), gen), dW_hh0=_pattern((3 * H, H), gen), db_ih0=_pattern((3 * H,), gen),
                        db_hh0=_pattern((3 * H,), gen))
    dW_ih, dW_hh, db_ih, db_hh = r.dW_ih0.to(DEV), r.dW_hh0.to(DEV), r.db_ih0.to(DEV), r.db_hh0.to(DEV)
    wsb = _lib.load().tmpnn_gru_bwd_weights_ws(R, IN, H)
    ws = torch.full((wsb // 4 + 4,), NAN, device=DEV)
    src, dst = (i32(x.src), i32(x.dst)) if xmode else (None, None)
    msg = _compact_msg(case, x) if xmode == 0 else None
    _lib.call('tmpnn_gru_bwd_weights', b.rows.data_ptr(), R, xmode, _lib.ptr(src), _lib.ptr(dst), _lib.ptr(msg), IN + 4, 1, IN,
              b.hD.data_ptr() + 4 * H, ld, H, b.gates.data_ptr(), N * H, _lib.ptr(b.d_hout), H + 4, _lib.ptr(b.dy),
              b.w_head.data_ptr() if up & 2 else None, dW_ih.data_ptr(), dW_hh.data_ptr(), db_ih.data_ptr(), db_hh.data_ptr(),
              ws.data_ptr(), wsb, _lib.raw_stream())
    torch.cuda.synchronize()
    r.dW_ih, r.dW_hh, r.db_ih, r.db_hh = dW_ih.cpu(), dW_hh.cpu(), db_ih.cpu(), db_hh.cpu()
    return r


@pytest.mark.parametrize('case', gc.BWD_WEIGHTS, ids=lambda c: c.id)
def test_backward_weights(case):
    rt = gc.route('bwd_weights', case.H, case.IN, case.xmode, case.R)
    for up in ((1, 2, 3) if case.R <= 65 else (3,)):
        x, r64, r32 = reference(case, up)
        r = run_bwd_weights(case, x, r64, up)
        ratios, missed = {}, []
        for q in ('dW_ih', 'dW_hh', 'db_ih', 'db_hh'):
            missed += _held(q, getattr(r, q), getattr(r64, q), getattr(r32, q), ratios, prev=getattr(r, q + '0'))
        _finish(f'{case.id} UP={up} [{rt["family"]}, {rt["slabs"]} slabs]', ratios, missed)


# ---- the tiled forward entries beyond their grid caps ---------------------------------------------------------------------------------
FWD_FIELDS = ('out', 'gates', 'parts')


def test_tiles_beyond_the_grid_cap():
    """tmpnn_gru_fwd_tiles, H = 64, R = 49160: 257 passes of 192 rows asked, 256 blocks: against float64, and bit-equal to
    tmpnn_gru_fwd's xmode 3 on the same buffers."""
    case = gc.TILES[0]
    assert gc.route('tiles', case.H, case.IN, 3, case.R)['capped']
    x, r64, r32 = reference(case)
    r = run_fwd(case, x, via='tiles')
    check_fwd(case.id, case, x, r64, r32, r)
    e = run_fwd(case, x)
    for f in FWD_FIELDS:
        assert torch.equal(bits(getattr(r, f)), bits(getattr(e, f))), f


def test_zero_state_tiles_beyond_the_grid_cap():
    """tmpnn_gru_fwd_tiles_zero_state, H = 64, R = 73736: 769 passes of 96 rows asked, 768 blocks; the list rows' state is
    zero.  Against float64, and bit-equal to tmpnn_gru_fwd's xmode 3 on the same (zero) state rows."""
    case = gc.TILES[1]
    rt = gc.route('tiles_zs', case.H, case.IN, 3, case.R)
    assert rt['capped'] and rt['grid'] == (768,)
    x, r64, r32 = reference(case, zero_state=True)
    assert torch.equal(r64.hn, x.b_hh[2 * case.H:].expand(case.R, case.H))
    r = run_fwd(case, x, via='tiles_zs', zero_state=True)
    check_fwd(case.id, case, x, r64, r32, r)
    e = run_fwd(case, x, zero_state=True)
    for f in FWD_FIELDS:
        assert torch.equal(bits(getattr(r, f)), bits(getattr(e, f))), f


# ---- two runs give identical bytes ------------------------------------------------------------------------------------------------------
def _pick(table, H, IN, xmode, R):
    return next(c for c in table if (c.H, c.IN, c.xmode, c.R) == (H, IN, xmode, R) and not c.shuffled and not c.misalign)


@pytest.mark.parametrize('case', [_pick(gc.FWD, 64, 64, 3, 193), _pick(gc.FWD, 32, 32, 1, 257), _pick(gc.FWD, 64, 128, 2, 129),
                                  _pick(gc.FWD, 128, 128, 1, 8065), _pick(gc.BWD_DATA, 64, 64, 1, 257),
                                  _pick(gc.BWD_DATA, 32, 64, 2, 257), _pick(gc.BWD_DATA, 128, 256, 2, 5377),
                                  _pick(gc.BWD_WEIGHTS, 64, 128, 2, 2049), _pick(gc.BWD_WEIGHTS, 32, 32, 1, 4097),
                                  _pick(gc.BWD_WEIGHTS, 128, 128, 0, 8193)], ids=lambda c: c.id)
def test_two_runs_give_equal_bytes(case):
    if case.entry == 'fwd':
        x = gc.inputs(case)
        a, b, fields = run_fwd(case, x), run_fwd(case, x), FWD_FIELDS
    elif case.entry == 'bwd_data':
        x, r64, _ = reference(case, 3, True)
        a, b, fields = run_bwd_data(case, x, r64, 3, True), run_bwd_data(case, x, r64, 3, True), ('d_msg', 'd_h')
    else:
        x, r64, _ = reference(case, 3)
        a, b, fields = run_bwd_weights(case, x, r64, 3), run_bwd_weights(case, x, r64, 3), ('dW_ih', 'dW_hh', 'db_ih', 'db_hh')
    for f in fields:
        assert torch.equal(bits(getattr(a, f)), bits(getattr(b, f))), f
