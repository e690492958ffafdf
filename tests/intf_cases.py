"""The input transform of a call's new det rows (Lin1 -> per-window BatchNorm -> ReLU -> Lin2) as a definition, its inputs, the
dispatch arithmetic of its three implementations restated on the host, and the table of cases of
tests/test_intf_shapes_gpu.py.  Host code only (torch on the CPU).

evaluate() is the transform in torch, float64 (the definition) or float32 (the host twin whose distance from float64 sizes the
bounds): the forward with the analytic zero-row terms and the sequential running-statistics recurrence, and the backward as the
analytic formulas the staged form (csrc/dense.hip), the workgroup form and the wave-owned form (csrc/intf.hip) share, evaluated
from the float64 forward's y_save / mean / rstd rounded to fp32 -- what a kernel reads -- never from a kernel's output.
inputs() draws everything from a seed; x, W1 and b1 sit on a grid on which Lin1 is exact in fp32 in any summation order (every
product a multiple of 2^-9, the sums far below 2^15), so y_save is compared with torch.equal.

route() follows tmpnn_input_tf_fwd / _bwd (intf.hip: itw_serves, itw_blocks, it_blocks, it_chunk_end, itw_chunk_end) and
tmpnn_input_bn_fwd / _bwd (dense.hip: bn_row_groups, splitk_plan)."""
import functools
import zlib
from types import SimpleNamespace
from typing import NamedTuple, Optional, Tuple

import torch

U32 = 2.0 ** -24
EPS = 1e-5
MOMENTUM = 0.1
KINK = 2.0 ** -16
CEILING = 2e-4                # what tests/gpu_stage_checks.py::check_input_bn holds this stage to, times scale
FACTOR = 4.0                  # bound = max(FACTOR * err32, 32 * 2^-24 * scale), see bound()
FACTORS = {}                  # a named quantity's own factor, with its reason in profiles/input_tf_shape_tests.md

IT_CH, IT_SPB, IT_FMAX, IT_NT = 128, 32, 128, 1024          # intf.hip: rows of a chunk, segments of a group, widest F, threads
ITW_R, ITW_MS, ITW_NW, ITW_SPB = 32, 8, 8, 64               # intf.hip: rows and segments of a tile, waves, segments of a group
RUNNING_CUT = 320                                           # k_it_running / k_bn_running: S beyond which the old value is dropped

ROUNDED_FWD = ('mean', 'rstd', 'out', 'run_mean', 'run_var')
GRADS = ('dW1', 'db1', 'dgamma', 'dbeta', 'dW2', 'db2')
ROUNDED = ROUNDED_FWD + GRADS + ('d_xdet', 'd_xzero')


class Case(NamedTuple):
    form: str                 # 'wave' | 'workgroup' | 'staged': the forward's implementation
    H: int
    F: int
    segs: tuple               # det rows per segment; or ('rand', S, lo, hi); or ('cus', k, lo, hi): S = k * cus + 1;
    #                           or ('rows_cus', k): one run of k * cus + 1 rows (eval)
    tag: str                  # the boundary the case is there for
    training: bool = True
    dx: bool = False          # d_xdet / d_xzero asked for
    xlist: bool = True        # x through a shuffled row list into a larger NaN-filled x (else x_rows NULL)
    msr_fwd: Optional[int] = None     # max_seg_rows handed to the forward (None: the longest segment): a routing argument only
    msr_bwd: Optional[int] = None
    bwd_form: Optional[str] = None    # the backward's implementation where it differs from `form`

    @property
    def id(self):
        s = self.segs
        if s and isinstance(s[0], str):
            sg = '_'.join(str(v) for v in s)
        elif len(s) <= 4:
            sg = 'x'.join(str(v) for v in s)
        else:
            sg = f'{len(s)}segs{sum(s)}rows{zlib.crc32(repr(s).encode()) % 1000:03d}'
        return (f'{self.form}-H{self.H}-F{self.F}-{sg}' + ('' if self.training else '-eval') + ('-dx' if self.dx else '')
                + ('' if self.xlist else '-nolist') + (f'-mf{self.msr_fwd}' if self.msr_fwd is not None else '')
                + (f'-mb{self.msr_bwd}' if self.msr_bwd is not None else ''))


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def seg_rows(case: Case, cus: int = 256) -> Tuple[int, ...]:
    """The det rows of each segment."""
    s = case.segs
    if not (s and isinstance(s[0], str)):
        return tuple(s)
    if s[0] == 'rows_cus':
        return (s[1] * cus + 1,)
    S, lo, hi = (s[1] * cus + 1 if s[0] == 'cus' else s[1]), s[2], s[3]
    gen = torch.Generator().manual_seed(zlib.crc32(repr((s, S)).encode()))
    return tuple(torch.randint(lo, hi + 1, (S,), generator=gen).tolist())


# ---- the dispatch arithmetic ----------------------------------------------------------------------------------------------------
def itw_serves(H, F, max_seg_rows, training):
    return bool(training) and H == 64 and F <= 16 and max_seg_rows <= ITW_R


def tf_supported(H, F, max_seg_rows):
    return H in (32, 64) and 0 < F <= IT_FMAX and 0 <= max_seg_rows <= IT_CH


def _chunks(ptr, s0, s1, rows_max, segs_max):
    """it_chunk_end / itw_chunk_end walked over the group [s0, s1): [(rows, segments)] of whole segments, at least one each."""
    out, sa = [], s0
    while sa < s1:
        sb = sa + 1
        while sb < s1 and sb - sa < segs_max and ptr[sb + 1] - ptr[sa] <= rows_max:
            sb += 1
        out.append((ptr[sb] - ptr[sa], sb - sa))
        sa = sb
    return out


def bn_row_groups(nd, S, H):
    return 1024 // H if (S > 0 and nd // S >= 256 and H <= 256) else 1


def splitk_plan(K):
    """(slabs, rows per slab) of the staged form's weight-gradient products over K = nd rows."""
    ns = max(1, min(1024, ceil_div(K, 128)))
    kp = max(16, (ceil_div(K, ns) + 15) & ~15)
    return max(1, ceil_div(K, kp)), kp


def route(entry, H, F, nd, seg_nd, max_seg_rows, training, want_dx, cus=256):
    """Which implementation a call takes and how its work is cut.  entry: 'tf_fwd' | 'tf_bwd' | 'bn_fwd' | 'bn_bwd'.
    form, grid, groups, groups_per_block (of the busiest workgroup), tiles (one list of (rows, segments) per group),
    tiles_per_wave (of the busiest wave of any group); the staged form: G (row groups of the per-segment reductions), slabs
    and fold (more than 64 slabs: the two-level reduction) of the split-K weight gradients."""
    S = len(seg_nd)
    if entry in ('bn_fwd', 'bn_bwd'):
        slabs, kper = splitk_plan(nd)
        return dict(form='staged', G=bn_row_groups(nd, S, H) if training else 1, slabs=slabs, rows_per_slab=kper, fold=slabs > 64)
    assert tf_supported(H, F, max_seg_rows), 'callers use the staged form'
    ptr = [0]
    for n in seg_nd:
        ptr.append(ptr[-1] + n)
    wave = itw_serves(H, F, max_seg_rows, training) and not (entry == 'tf_bwd' and want_dx)
    if wave:
        groups = ceil_div(S, ITW_SPB)
        tiles = [_chunks(ptr, g * ITW_SPB, min(S, (g + 1) * ITW_SPB), ITW_R, ITW_MS) for g in range(groups)]
        r = dict(form='wave', tiles_per_wave=max(ceil_div(len(t), ITW_NW) for t in tiles))
    elif training:
        groups = ceil_div(S, IT_SPB)
        tiles = [_chunks(ptr, g * IT_SPB, min(S, (g + 1) * IT_SPB), IT_CH, IT_SPB) for g in range(groups)]
        r = dict(form='workgroup')
    else:
        groups = ceil_div(nd, IT_CH)
        tiles = [[(min(nd, (g + 1) * IT_CH) - g * IT_CH, 1)] for g in range(groups)]
        r = dict(form='workgroup')
    grid = min(groups, cus)
    r.update(grid=grid, groups=groups, groups_per_block=ceil_div(groups, grid) if grid else 0, tiles=tiles)
    return r


def routes(case: Case, cus: int = 256):
    """(forward route, backward route) of a case."""
    sn = seg_rows(case, cus)
    nd = sum(sn)
    if case.form == 'staged':
        return (route('bn_fwd', case.H, case.F, nd, sn, 0, case.training, case.dx, cus),
                route('bn_bwd', case.H, case.F, nd, sn, 0, case.training, case.dx, cus))
    longest = max(sn) if case.training else 0          # (eval mode cuts rows, not segments: the cases hand it 0)
    mf = longest if case.msr_fwd is None else case.msr_fwd
    mb = longest if case.msr_bwd is None else case.msr_bwd
    assert mf >= longest and mb >= longest, 'max_seg_rows is an upper bound'
    return (route('tf_fwd', case.H, case.F, nd, sn, mf, case.training, case.dx, cus),
            route('tf_bwd', case.H, case.F, nd, sn, mb, case.training, case.dx, cus))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def weight_q(F: int) -> int:
    return max(1, round(64 / F ** 0.5))


def _grid(shape, lo, hi, step, gen):
    """Multiples of `step` in [lo * step, hi * step]."""
    return torch.randint(lo, hi + 1, shape, generator=gen).double() * step


def _forward(x, dtype, training):
    """y, mean, rstd, var, z (the ReLU's input), out."""
    t = lambda v: v.to(dtype)
    H, S, seg = x.H, x.S, x.seg_of_det
    b1 = t(x.b1)
    y = t(x.x) @ t(x.W1).t() + b1
    if training:
        cnt = t(x.seg_cnt)[:, None]
        nz = cnt - t(x.seg_nd)[:, None]
        mean = (torch.zeros(S, H, dtype=dtype).index_add(0, seg, y) + nz * b1) / cnt
        d = y - mean[seg]
        var = (torch.zeros(S, H, dtype=dtype).index_add(0, seg, d * d) + nz * (b1 - mean) ** 2) / cnt
        rstd = 1.0 / torch.sqrt(var + EPS)
        sg = seg
    else:
        mean, var = t(x.rm0)[None, :], t(x.rv0)[None, :]
        rstd = 1.0 / torch.sqrt(var + EPS)
        sg = torch.zeros_like(seg)
    z = (y - mean[sg]) * rstd[sg] * t(x.gamma) + t(x.beta)
    out = torch.relu(z) @ t(x.W2).t() + t(x.b2)
    return SimpleNamespace(y=y, mean=mean, rstd=rstd, var=var, z=z, out=out)


@functools.lru_cache(maxsize=4)
def inputs(case: Case, cus: int = 256) -> SimpleNamespace:
    """Everything a case reads, in float64 (fp32-exact values), from a seed that depends on the case alone.  Shared, never
    modified."""
    H, F = case.H, case.F
    sn = seg_rows(case, cus)
    S, nd = len(sn), sum(sn)
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + 17 * cus)
    x = SimpleNamespace(H=H, F=F, S=S, nd=nd, training=case.training)
    x.seg_nd = torch.tensor(sn, dtype=torch.int64)
    x.seg_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), x.seg_nd.cumsum(0)])
    x.seg_cnt = torch.clamp(x.seg_nd + torch.randint(0, 7, (S,), generator=gen), min=2)      # dets + zero rows, at least 2
    x.seg_of_det = torch.repeat_interleave(torch.arange(S), x.seg_nd)
    q = weight_q(F)
    x.x = _grid((nd, F), -8, 8, 1 / 8, gen)
    # (magnitudes in the upper half of the range: at F <= 2 a column of small weights would keep y next to b1 and its ReLU
    # from ever switching)
    x.W1 = _grid((H, F), (q + 1) // 2, q, 1 / 64, gen) * (2.0 * torch.randint(0, 2, (H, F), generator=gen).double() - 1.0)
    x.b1 = _grid((H,), -8, 8, 1 / 16, gen)
    # rounded quantities anyway: seeded fp32 values, so that both evaluations and the kernels read the same numbers
    nrm = lambda *s: torch.randn(*s, generator=gen).double()
    x.gamma = (0.5 + torch.rand(H, generator=gen)).double()
    # (beta a quarter of a normal: yhat has unit variance, so every column's ReLU switches within a few dozen rows)
    x.beta, x.W2, x.b2, x.d_out = nrm(H) / 4, nrm(H, H) / 8, nrm(H), nrm(nd, H)
    # non-zero initial running statistics, of the size of Lin1's own output (mean b1, variance about 1/8): eval mode
    # normalises with them, and its ReLU inputs must take both signs as well
    x.rm0 = x.b1 + _grid((H,), -2, 2, 1 / 64, gen)
    x.rv0 = (0.05 + 0.15 * torch.rand(H, generator=gen)).double()
    # where the rows sit: out_row a drawn permutation into a taller buffer, x_rows a drawn list into a taller x
    x.N = nd + 5
    x.out_row = torch.randperm(x.N, generator=gen)[:nd]
    x.NX = nd + 7
    x.x_rows = torch.randperm(x.NX, generator=gen)[:nd] if case.xlist else None
    # kink rows: a ReLU input within 2^-16 of zero -- their upstream gradient is zero, so that row's mask cannot matter
    z = _forward(x, torch.float64, case.training).z
    x.kink = (z.abs() < KINK).any(1)
    x.d_out[x.kink] = 0.0
    return x


# ---- the definition -------------------------------------------------------------------------------------------------------------
def evaluate(x: SimpleNamespace, dtype=torch.float64, exact_stats: bool = False) -> SimpleNamespace:
    """Forward: y_save, mean, rstd ([S, H]; eval mode: one row, the running statistics), out ([nd, H], det row i's output),
    run_mean / run_var after the sequential momentum recurrence over all S segments (eval mode: unchanged).  Backward for the
    upstream gradient x.d_out by the analytic formulas, from the float64 forward's y_save / mean / rstd rounded to fp32
    (exact_stats: from this evaluation's own, unrounded): dW1, db1, dgamma, dbeta, dW2, db2, d_xdet [nd, F], d_xzero [S, F]."""
    t = lambda v: v.to(dtype)
    training, seg, S = x.training, x.seg_of_det, x.S
    f = _forward(x, dtype, training)
    o = SimpleNamespace(y_save=f.y, mean=f.mean, rstd=f.rstd, out=f.out, z=f.z)
    rm, rv = t(x.rm0).clone(), t(x.rv0).clone()
    cnt = t(x.seg_cnt)
    if training:
        unb = f.var * (cnt / (cnt - 1.0))[:, None]
        for s in range(S):                                  # windows are seen one after another in the reference
            rm = (1 - MOMENTUM) * rm + MOMENTUM * f.mean[s]
            rv = (1 - MOMENTUM) * rv + MOMENTUM * unb[s]
    o.run_mean, o.run_var = rm, rv
    # ---- backward
    if exact_stats:
        ys, mean, rstd = f.y, f.mean, f.rstd
    else:
        g = f if dtype == torch.float64 else _forward(x, torch.float64, training)
        ys, mean, rstd = (t(v.float()) for v in (g.y, g.mean, g.rstd))
    sg = seg if training else torch.zeros_like(seg)
    gamma, beta, b1, W1, W2, d = t(x.gamma), t(x.beta), t(x.b1), t(x.W1), t(x.W2), t(x.d_out)
    yhat = (ys - mean[sg]) * rstd[sg]
    zz = yhat * gamma + beta
    a = torch.relu(zz)
    o.dW2, o.db2 = d.t() @ a, d.sum(0)
    dz = (d @ W2) * (zz > 0).to(dtype)
    o.dgamma, o.dbeta = (dz * yhat).sum(0), dz.sum(0)
    dyh = dz * gamma
    if training:
        H = x.H
        q1 = torch.zeros(S, H, dtype=dtype).index_add(0, seg, dyh)
        q2 = torch.zeros(S, H, dtype=dtype).index_add(0, seg, dyh * yhat)
        inv = (1.0 / cnt)[:, None]
        dy = rstd[seg] * (dyh - (q1 * inv)[seg] - yhat * (q2 * inv)[seg])
        yh0 = (b1 - mean) * rstd
        dy0 = rstd * (-q1 * inv - yh0 * q2 * inv)
        nz = (cnt - t(x.seg_nd))[:, None]
        o.db1 = dy.sum(0) + (nz * dy0).sum(0)
        o.d_xzero = dy0 @ W1
    else:
        dy = rstd[sg] * dyh
        o.db1 = dy.sum(0)
        o.d_xzero = torch.zeros(S, x.F, dtype=dtype)
    o.dW1 = dy.t() @ t(x.x)
    o.d_xdet = dy @ W1
    return o


def scale_of(qty: str, r64: SimpleNamespace, training: bool) -> float:
    """scale = max(1, max |ref64|) of the quantity itself.  The one exception is db1 in training mode: BatchNorm removes a
    bias added in front of it, so db1 is identically zero in exact arithmetic -- sum over a segment's rows, zero rows included,
    of dy is 0 -- and what a kernel returns is the rounding residue of sums whose addends are the size of the other
    gradients.  Its own magnitude (1e-13 in float64) says nothing about them; its scale is that of the six parameter gradients
    together, the normalisation tests/gpu_stage_checks.py::check_input_bn applies to every gradient of this stage."""
    names = GRADS if (qty == 'db1' and training) else (qty,)
    return max([1.0] + [float(getattr(r64, n).abs().max()) for n in names if getattr(r64, n).numel()])


def bound(qty: str, r64: SimpleNamespace, r32: SimpleNamespace, training: bool) -> Tuple[float, float, float]:
    """(bound, err32, scale) of a rounded quantity: max(factor * err32, 32 * 2^-24 * scale) and never past CEILING * scale;
    scale as scale_of(), err32 the distance of the HOST fp32 evaluation of the same definition from float64."""
    ref64, ref32 = getattr(r64, qty), getattr(r32, qty)
    scale = scale_of(qty, r64, training)
    err32 = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return min(max(FACTORS.get(qty, FACTOR) * err32, 32.0 * U32 * scale), CEILING * scale), err32, scale


# ---- the cases --------------------------------------------------------------------------------------------------------------------
NINE_TILES = (30,) + (3, 0, 1, 2, 1, 0, 1, 1) * 7 + (3, 0, 1, 2, 1, 0, 1)       # 64 segments: [30], seven tiles of 8, one of 7


def _w(F, segs, tag, **kw):
    return Case('wave', 64, F, tuple(segs), tag, **kw)


WAVE = [
    _w(1, (1,), 'one segment of one row'),
    _w(16, (32,), 'one segment of 32 rows: a full tile'),
    _w(8, (31, 1), '31 + 1 rows: one tile of exactly 32 rows', xlist=False),
    _w(15, (31, 2), '31 + 2 rows: two tiles'),
    _w(8, (1,) * 8, 'eight 1-row segments: one tile at the 8-segment limit'),
    _w(16, (1,) * 9, 'nine 1-row segments: the ninth opens a second tile', xlist=False),
    _w(16, (0,) * 8 + (3,), 'eight empty segments (a tile of no row), then one of 3 rows'),
    _w(15, (5,), 'odd nr: the two-rows-per-pass tails'),
    _w(1, (7, 0, 9), 'odd nr, an empty segment in the middle'),
    _w(8, (0, 4, 0, 3, 0), 'empty segments first, in the middle and last in one tile', xlist=False),
    _w(8, NINE_TILES, 'a group of 64 segments in 9 tiles: the second lap of wave 0'),
    _w(16, NINE_TILES + (5,), '65 segments: a second group of one tile, seven waves idle'),
    _w(16, ('rand', 320, 0, 3), 'S = 320: the last S whose old running value is kept'),
    _w(1, ('rand', 321, 0, 3), 'S = 321: the old running value and segment 0 are dropped'),
    _w(8, ('cus', 64, 0, 3), 'S = 64 cus + 1: a second group for workgroup 0, its accumulators span two groups'),
]


def _g(H, F, segs, tag, **kw):
    return Case('workgroup', H, F, tuple(segs), tag, **kw)


def _chunk_sizes():
    out = []
    for H, sizes in ((64, (1, 15, 16, 17, 63, 64, 65, 128)), (32, (1, 31, 32, 33, 127, 128))):
        for k, nr in enumerate(sizes):
            F = (2, 16, 17, 128)[k % 4]
            out.append(_g(H, F, (nr,), f'one chunk of nr = {nr} rows against NSUB = {1024 // H} and 4 NSUB', dx=k % 2 == 0,
                          msr_fwd=128, msr_bwd=128, xlist=k % 3 != 0))
    return out


WORKGROUP = _chunk_sizes() + [
    _g(64, 16, (127, 1), '127 + 1 rows: one chunk of exactly 128 rows', dx=True),
    _g(64, 2, (127, 2), '127 + 2 rows: two chunks', dx=True),
    _g(32, 17, (127, 2), '127 + 2 rows: two chunks, wide input', dx=True, xlist=False),
    _g(64, 16, ('rand', 32, 0, 5), '32 segments: one full group', msr_fwd=128, msr_bwd=128),
    _g(64, 16, ('rand', 33, 0, 5), '33 segments: a second group of one segment', msr_fwd=128, dx=True),
    _g(32, 2, (3, 4, 0, 0), 'a group whose trailing segments are empty', dx=True),
    _g(64, 16, (0,) * 32 + (5,), '32 leading empty segments, then one of 5 rows: a chunk of no row at ra = 0', dx=True,
       msr_fwd=128),
    _g(32, 128, (0,) * 32 + (5,), '32 leading empty segments, then one of 5 rows, wide input', dx=True),
    _g(64, 17, (20,), 'F = 17 at a wave-eligible shape: the workgroup form by width'),
    _g(64, 16, (33,), 'a segment of 33 rows at a wave-eligible width: the workgroup form by length'),
    _g(64, 128, ('rand', 40, 0, 9), 'the widest input (FPT = 8), two groups', dx=True),
    _g(32, 128, ('rand', 40, 0, 9), 'the widest input (FPT = 4), two groups'),
    _g(64, 17, ('cus', 32, 0, 6), 'S = 32 cus + 1: a second group for workgroup 0, its accumulators span two groups', dx=True),
    _g(64, 16, (1,), 'eval, nd = 1', training=False, dx=True),
    _g(32, 2, (127,), 'eval, nd = 127: one group short of a row', training=False),
    _g(64, 17, (128,), 'eval, nd = 128: one full group', training=False, dx=True, xlist=False),
    _g(32, 128, (129,), 'eval, nd = 129: a second group of one row', training=False, dx=True),
    _g(64, 2, ('rows_cus', 128), 'eval, nd = 128 cus + 1: a second group for workgroup 0', training=False, dx=True),
]

CROSS = [
    _w(8, NINE_TILES, 'forward by the wave form, backward by the workgroup form', msr_bwd=128, bwd_form='workgroup'),
    _g(64, 8, NINE_TILES, 'forward by the workgroup form, backward by the wave form', msr_fwd=128, bwd_form='wave'),
]


def _s(H, F, segs, tag, **kw):
    return Case('staged', H, F, tuple(segs), tag, xlist=False, dx=kw.pop('dx', True), **kw)


STAGED = [
    _s(256, 8, (255,), 'S = 1, nd = 255: G = 1'),
    _s(256, 8, (256,), 'S = 1, nd = 256: G = 1024 / H = 4'),
    _s(128, 3, (256,), 'S = 1, nd = 256: G = 8'),
    _s(32, 17, (256,), 'S = 1, nd = 256: G = 32'),
    _s(64, 40, (1, 511), 'segments of 1 and 511 rows: G = 16, row groups with no row'),
    _s(128, 8, (1, 511), 'segments of 1 and 511 rows: G = 8, row groups with no row'),
    _s(64, 8, (128,), 'nd = 128: the direct product'),
    _s(64, 8, (129,), 'nd = 129: two slabs'),
    _s(64, 17, (8192,), 'nd = 8192: 64 slabs'),
    _s(64, 17, (8193,), 'nd = 8193: 65 slabs, the two-level fold'),
    _s(32, 3, (0, 5, 0, 0, 7, 0), 'empty segments first, in the middle and last (segments found by search)'),
    _s(64, 8, (0, 5, 0, 0, 7, 0), 'empty segments first, in the middle and last'),
    _s(128, 17, (300,), 'eval', training=False),
]

TABLE = WAVE + WORKGROUP + CROSS + STAGED

# two runs of these give equal bytes: the wave combine, the slab order of every form, the fold
TWICE = [WAVE[10], WAVE[14], WORKGROUP[15], WORKGROUP[31], WORKGROUP[26], CROSS[0], CROSS[1], STAGED[4], STAGED[9], STAGED[10]]
