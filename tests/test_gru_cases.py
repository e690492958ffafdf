"""The host half of the GRU shape tests: the inputs of tests/gru_cases.py are exact where the GPU file compares with
torch.equal, they do not saturate the gates, route() puts a case of TABLE on each side of every dispatch switch and grid cap,
and the float64 definition is torch.nn.GRUCell."""
import pytest
import torch

from tests import gru_cases as gc

SHAPES = sorted({(c.H, c.IN, c.xmode) for c in gc.TABLE})


def _small(H, IN, xmode, R=257):
    return gc.Case('fwd', H, IN, xmode, R, 'host check')


# ---- exactness ------------------------------------------------------------------------------------------------------------------
def _bf16_exact(t):
    return torch.equal(t.float().bfloat16().double(), t)


@pytest.mark.parametrize('H,IN,xmode', SHAPES)
def test_inputs_are_exact(H, IN, xmode):
    """fp32 equals float64 bit for bit in two summation orders, every operand is bf16-exact, and the sums of absolute addends
    (multiples of 2^-9) stay below 2^24 * 2^-9: no order and no split of an operand into bf16 pieces can round."""
    case = _small(H, IN, xmode)
    x = gc.inputs(case)
    for t in (x.h, x.W_ih, x.W_hh, x.b_ih, x.b_hh) + (() if x.msg is None else (x.msg,)):
        assert _bf16_exact(t)
    r64 = gc.evaluate(case, x)
    r32 = gc.evaluate(case, x, dtype=torch.float32)
    assert torch.equal(r32.pre.double(), r64.pre) and torch.equal(r32.hn.double(), r64.hn)
    hrow = x.h[x.rows]
    # the operand of the W_ih product: the det rows of the projected form (P enters a gate twice), else the cell's x
    xin = x.h[x.dets] if xmode == 3 else gc.message(x, xmode, x.h, torch.float64)
    assert _bf16_exact(xin)
    if xmode == 3:
        assert torch.equal(r32.P.double(), r64.P)
    tot = (2 if xmode == 3 else 1) * float((xin.abs() @ x.W_ih.abs().t()).max())
    tot += float((hrow.abs() @ x.W_hh.abs().t()).max()) + 1.0                      # |b_ih| + |b_hh| <= 1
    assert tot * 2 ** 9 < 2 ** 24

    def chained(a, W):
        """a W^T in fp32, term by term, k in another order: the odd k downwards, then the even k downwards."""
        k = torch.cat([torch.arange(a.shape[1] - 1, -1, -2), torch.arange(a.shape[1] - 2, -1, -2)])
        acc = torch.zeros(a.shape[0], W.shape[0], dtype=torch.float32)
        for j in k.tolist():
            acc = acc + a[:, j:j + 1].float() * W[:, j].float()[None, :]
        return acc

    sub = slice(0, 40)
    gh = chained(hrow[sub], x.W_hh)
    assert torch.equal((gh[:, 2 * H:] + x.b_hh[2 * H:].float()).double(), r64.hn[sub])
    gi = chained(xin[sub], x.W_ih)
    if xmode == 3:
        assert torch.equal(gi.double(), r64.P[sub])
    else:
        pre = (gi[:, :2 * H] + gh[:, :2 * H]) + (x.b_ih[:2 * H] + x.b_hh[:2 * H]).float()
        assert torch.equal(pre.double(), r64.pre[sub, :2 * H])
        assert torch.equal((gi[:, 2 * H:] + x.b_ih[2 * H:].float()).double(), r64.pre[sub, 2 * H:3 * H])


@pytest.mark.parametrize('H,IN,xmode', SHAPES)
def test_gates_do_not_saturate(H, IN, xmode):
    """Conditions on the inputs: a saturated gate would hide a wrong operand behind sigmoid'(x) ~ 0."""
    case = _small(H, IN, xmode, R=1025)
    pre = gc.evaluate(case, gc.inputs(case)).pre
    assert float((pre.abs() > 6).double().mean()) <= 0.01
    assert 0.5 <= float(pre.std()) <= 2.0


# ---- the definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('xmode', [0, 1, 2, 3])
def test_definition_is_torch_grucell(xmode):
    H = 32
    IN = 2 * H if xmode == 2 else H
    case = gc.Case('fwd', H, IN, xmode, 37, 'host check')
    x = gc.inputs(case)
    cell = torch.nn.GRUCell(IN, H).double()
    with torch.no_grad():
        cell.weight_ih.copy_(x.W_ih), cell.weight_hh.copy_(x.W_hh), cell.bias_ih.copy_(x.b_ih), cell.bias_hh.copy_(x.b_hh)
    if xmode == 3:
        hd = x.h[x.dets]
        xin = hd[x.src] - hd[x.dst]
    else:
        xin = gc.message(x, xmode, x.h, torch.float64)
    xin = xin.clone().requires_grad_(True)
    hrow = x.h[x.rows].clone().requires_grad_(True)
    want = cell(xin, hrow)
    got = gc.evaluate(case, x, up=None if xmode == 3 else 3, fuse=False)
    assert float((got.h_out - want.detach()).abs().max()) <= 1e-12
    assert float((got.parts.sum(1) - want.detach() @ x.w_head).abs().max()) <= 1e-12
    if xmode == 3:
        return
    (want * (x.d_hout + x.dy[x.rows, None] * x.w_head[None, :])).sum().backward()
    for name, ref in (('d_msg', xin.grad), ('d_h', hrow.grad), ('dW_ih', cell.weight_ih.grad), ('dW_hh', cell.weight_hh.grad),
                      ('db_ih', cell.bias_ih.grad), ('db_hh', cell.bias_hh.grad)):
        assert float((getattr(got, name) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), name
    # the upstream forms add up, and the fused adjoint is add[src] - add[dst] on d_h alone
    u1, u2 = gc.evaluate(case, x, up=1), gc.evaluate(case, x, up=2)
    assert float((u1.d_h + u2.d_h - got.d_h).abs().max()) <= 1e-12
    if xmode:
        f = gc.evaluate(case, x, up=3, fuse=True)
        assert torch.equal(f.d_msg, got.d_msg)
        assert float(((f.d_h - got.d_h) - (x.add[x.src] - x.add[x.dst])).abs().max()) <= 1e-12


# ---- the row lists ------------------------------------------------------------------------------------------------------------------
def test_row_lists():
    for case in (c for c in gc.TABLE if c.R <= 257):
        x = gc.inputs(case)
        assert x.N == 2 * case.R + 7 + (gc.DN if case.xmode == 3 else 0)
        assert x.rows.unique().numel() == case.R and int(x.rows.max()) < x.N
        assert case.shuffled or bool((x.rows[1:] > x.rows[:-1]).all())
        listed = torch.zeros(x.N, dtype=torch.bool)
        listed[x.rows] = True
        if case.xmode in (1, 2):
            assert not bool(listed[x.src].any()) and not bool(listed[x.dst].any())
        if case.xmode == 3:
            assert x.dets.numel() == gc.DN and not bool(listed[x.dets].any())
            assert int(x.src.max()) < gc.DN and int(x.dst.max()) < gc.DN and int(x.src.min()) >= 0
    sh = [c for c in gc.TABLE if c.shuffled]
    assert len(sh) == 1 and not bool((gc.inputs(sh[0]).rows[1:] > gc.inputs(sh[0]).rows[:-1]).all())


# ---- switch coverage ----------------------------------------------------------------------------------------------------------------
def _routes(entry, H=None, IN=None, xmode=None):
    return [(c, gc.route(c.entry, c.H, c.IN, c.xmode, c.R, aligned=not c.misalign)) for c in gc.TABLE
            if c.entry == entry and H in (None, c.H) and IN in (None, c.IN) and xmode in (None, c.xmode)]


@pytest.mark.parametrize('entry,H,IN,xmode,key,below,above,R', gc.SWITCHES)
def test_switches_have_a_case_on_each_side(entry, H, IN, xmode, key, below, above, R):
    """R is the FIRST count of the wider instantiation, and TABLE holds it (and, where the issue names one, R - 1)."""
    assert gc.route(entry, H, IN, xmode, R - 1)[key] == below and gc.route(entry, H, IN, xmode, R)[key] == above
    got = {r[key] for _, r in _routes(entry, H, IN, None if entry == 'bwd_data' else xmode) if key in r}
    assert above in got
    assert any(c.R == R for c, _ in _routes(entry, H, IN, None if entry == 'bwd_data' else xmode))
    if not (entry == 'fwd' and H == 256 and xmode == 2):
        assert below in got


def test_every_family_is_reached():
    fam = lambda entry: {r['family'] for _, r in _routes(entry)}
    assert fam('fwd') == {'k_gru_fwd_split', 'k_gru_fwd_lds', 'k_gru_fwd'}
    assert fam('bwd_data') == {'k_gru_bwd_data_split', 'k_gru_bwd_data_lds', 'k_gru_bwd_data'}
    assert fam('bwd_weights') == {'k_gru_bwd_weights_chunk', 'k_gru_bwd_weights'}
    mis = [r for c, r in _routes('fwd') if c.misalign]
    assert len(mis) == 1 and mis[0]['family'] == 'k_gru_fwd'
    for x in (0, 1, 2):
        assert {r['ct'] for _, r in _routes('fwd', xmode=x) if 'ct' in r} == {1, 2}


def test_grid_caps_and_empty_items():
    # the figures the issue derives
    r = gc.route('fwd', 64, 64, 3, 49160)
    assert (r['items'], r['per_block'], r['idle_blocks'], r['capped']) == (3074, 13, 19, True) and 49160 % 32
    r = gc.route('fwd', 32, 32, 3, 65544)
    assert (r['items'], r['per_block'], r['idle_blocks'], r['capped']) == (2049, 9, 28, True)
    assert gc.route('bwd_data', 64, 64, 1, 1)['empty_items'] == 7
    for fam in ('k_gru_fwd_split', 'k_gru_fwd_lds'):
        rs = [r for _, r in _routes('fwd') if r['family'] == fam]
        assert any(r['capped'] and r['idle_blocks'] > 0 for r in rs) and any(not r['capped'] for r in rs), fam
    for H in (32, 64):
        rs = [r for _, r in _routes('bwd_data', H=H) if r['family'] == 'k_gru_bwd_data_split']
        assert any(r['capped'] and r['idle_blocks'] > 0 for r in rs) and any(r['empty_items'] == 7 for r in rs)
        assert any(r['empty_items'] == 0 for r in rs)
        rs = [r for _, r in _routes('bwd_data', H=H) if r['family'] == 'k_gru_bwd_data_lds']
        assert any(r['empty_items'] == 7 for r in rs) and any(r['grid'] == (2,) for r in rs)
    # the passes: one row short of a second block, and the first row of it
    by_R = {c.R: r for c, r in _routes('fwd', H=64, xmode=3)}
    assert by_R[192]['grid'] == (1,) and by_R[193]['grid'] == (2,)
    by_R = {c.R: r for c, r in _routes('fwd', H=32, xmode=3)}
    assert by_R[256]['grid'] == (1,) and by_R[257]['grid'] == (2,)
    by_R = {c.R: r for c, r in _routes('fwd', H=64, xmode=2)}
    assert by_R[128]['grid'] == (1, 2) and by_R[129]['grid'] == (2, 2) and by_R[16257]['grid'] == (128, 1)
    for c, r in _routes('tiles') + _routes('tiles_zs'):
        assert r['capped'] and c.R % 32
    assert _routes('tiles_zs')[0][1]['grid'] == (768,)


def test_weight_slabs():
    rw = lambda H, IN, x, R: gc.route('bwd_weights', H, IN, x, R)
    assert [rw(128, 128, 0, R)['slabs'] for R in (33, 8192, 8193)] == [2, 256, 256]
    assert [rw(128, 128, 0, R)['tiles_per_slab'] for R in (8192, 8193)] == [1, 2]
    # at H = IN = 256 the slab count is capped at 64: the 65th tile shares a slab, the fold is not taken at this width
    assert [rw(256, 256, 0, R)['slabs'] for R in (2048, 2049)] == [64, 64] and not rw(256, 256, 0, 2049)['fold']
    assert [rw(256, 256, 0, R)['tiles_per_slab'] for R in (2048, 2049)] == [1, 2]
    assert rw(64, 128, 2, 2049)['slabs'] == 65 and rw(64, 128, 2, 2049)['fold'] and not rw(64, 128, 2, 2048)['fold']
    assert [rw(32, 32, 0, R)['slabs'] for R in (1, 63, 64, 65)] == [1, 1, 1, 2]
    assert rw(32, 32, 1, 4097)['slabs'] == 65 and rw(32, 32, 1, 4096)['slabs'] == 64
    listed = {(c.H, c.IN, c.xmode, c.R) for c in gc.TABLE if c.entry == 'bwd_weights'}
    for key in ((128, 128, 0, 33), (128, 128, 0, 8192), (128, 128, 0, 8193), (256, 256, 0, 2048), (256, 256, 0, 2049),
                (64, 128, 2, 2049), (32, 32, 0, 1), (32, 32, 0, 63), (32, 32, 0, 64), (32, 32, 0, 65), (32, 32, 1, 4097)):
        assert key in listed
    folds = {(r['family'], r['fold']) for _, r in _routes('bwd_weights')}
    assert folds == {(f, b) for f in ('k_gru_bwd_weights_chunk', 'k_gru_bwd_weights') for b in (False, True)}


def test_head_parts():
    assert gc.fwd_head_parts(64, 64, 3) == 2 and gc.fwd_head_parts(32, 32, 1) == 1 and gc.fwd_head_parts(32, 64, 2) == 1
    assert gc.fwd_head_parts(64, 128, 2) == 0 and gc.fwd_head_parts(128, 128, 0) == 0


def test_ids_are_unique():
    ids = [c.id for c in gc.TABLE]
    assert len(ids) == len(set(ids))
