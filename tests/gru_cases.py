"""The GRU cell of csrc/gru_fwd.hip and csrc/gru_bwd.hip as a definition, its inputs, the dispatch arithmetic of the three entry
points restated on the host, and the table of cases of tests/test_gru_shapes_gpu.py.  Host code only (torch on the CPU).

evaluate() is the cell in torch, forward and autograd backward, in float64 (the definition) or float32 (the host twin whose
distance from float64 sizes the bounds).  inputs() draws everything from a seed; h, the messages, the weights and the biases
sit on a grid on which every pre-activation -- W_ih x + b_ih, W_hh h + b_hh, their sums, and P = h W_ih^T of the projected
form -- is exact in fp32 in any summation order and under any split of an operand into bf16 pieces: all operands are
bf16-exact (at most 8 significant bits), every product is a multiple of 2^-9, and the sums of absolute addends stay far
below 2^15 = 2^24 * 2^-9.  tests/test_gru_cases.py asserts that for every shape of the GPU file.

route() follows tmpnn_gru_fwd (gru_fwd.hip:1517-1579), tmpnn_gru_bwd_data (gru_bwd.hip:1138-1163) and
tmpnn_gru_bwd_weights (gru_bwd.hip:1166-1180, 1226-1270) of the default build (bf16x6 operand split on)."""
import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional, Tuple

import torch

U32 = 2.0 ** -24
DN = 300                      # det rows behind the projected form (xmode 3)
STG_LD = 36                   # csrc/gru_common.h: floats per row of a wave's staging tile
# what the suite already holds the node cell to (test_node_cell_forward_ragged_sizes, test_bwd_slab_switch), times scale:
# no bound of the GPU file goes past these
CEILING = dict(h_out=5e-6, r=1e-5, z=1e-5, n=1e-5, parts=2e-5, d_msg=2e-5, d_h=2e-5, dW_ih=2e-5, dW_hh=2e-5, db_ih=2e-5,
               db_hh=2e-5)
FACTOR = 4.0                  # bound = max(FACTOR * err32, 32 * 2^-24 * scale), see bound()


class Case(NamedTuple):
    entry: str                # 'fwd' | 'bwd_data' | 'bwd_weights' | 'tiles' | 'tiles_zs'
    H: int
    IN: int
    xmode: int
    R: int
    tag: str                  # what the case is there for
    shuffled: bool = False    # the row list in a drawn order instead of ascending
    misalign: bool = False    # h_out 4 bytes off a 16-byte boundary: the H <= 64 cell falls back to k_gru_fwd<CT, X>

    @property
    def id(self):
        return (f'{self.entry}-H{self.H}-IN{self.IN}-x{self.xmode}-R{self.R}' + ('-shuffled' if self.shuffled else '')
                + ('-misaligned' if self.misalign else ''))


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ---- the dispatch arithmetic ----------------------------------------------------------------------------------------------------
def _persistent(items: int, grid: int) -> dict:
    """A persistent grid: block b owns items [b * per_block, min(items, (b + 1) * per_block))."""
    per_block = ceil_div(items, grid)
    idle = sum(1 for b in range(grid) if b * per_block >= items)
    return dict(grid=(grid,), items=items, per_block=per_block, idle_blocks=idle, capped=False)


def fwd_head_parts(H: int, IN: int, xmode: int) -> int:
    """tmpnn_gru_fwd_head_parts (gru_fwd.hip:1486-1492)."""
    if H not in (32, 64):
        return 0
    wpb = 12 if H == 64 else 8
    shm = 4 * (((0 if xmode == 3 else IN) + H) * 3 * H + wpb * 32 * STG_LD + 4)
    return 0 if shm > 160 * 1024 else H // 32


def route(entry: str, H: int, IN: int, xmode: int, R: int, aligned: bool = True) -> dict:
    """Which kernel a call takes and how its work is cut: family, ct / nt, grid, items, per_block, idle_blocks (blocks of a
    persistent grid that get no item), empty_items (items that lie wholly beyond R), capped (the grid is at its cap and a
    block owns more than one pass), slabs and fold (more than 64 slabs: the two-level reduction) for the weights."""
    if entry in ('tiles', 'tiles_zs'):
        zs = entry == 'tiles_zs'
        per_pass, cap = ((96 if H == 64 else 128), 768) if zs else ((192 if H == 64 else 256), 256)
        want = ceil_div(R, per_pass)
        r = _persistent(ceil_div(R, 32) * (H // 32), min(want, cap))
        r.update(family='k_gru_fwd_split_tiled' + ('<zs>' if zs else ''), capped=want > cap, empty_items=0)
        return r
    if entry == 'fwd':
        if H <= 64 and aligned:
            per_pass = 192 if H == 64 else 256
            want = ceil_div(R, per_pass)
            grid = min(want, 256)
            items = ceil_div(R, 32) * (H // 32)
            if xmode == 3:
                r = _persistent(items, grid)
                r.update(family='k_gru_fwd_split', capped=want > 256, empty_items=0)
                return r
            if xmode == 0 and IN == H:
                cwn = H // 32
                groups = min(ceil_div(ceil_div(R, 32), 8), 256 // cwn)
                groups = (groups + 7) & ~7
                return dict(family='k_gru_fwd_split_node', grid=(groups * cwn,), capped=False)
            if fwd_head_parts(H, IN, xmode) > 0:
                r = _persistent(items, grid)
                r.update(family='k_gru_fwd_lds', capped=want > 256, empty_items=0)
                return r
        assert xmode != 3, 'xmode 3 exists on the LDS path only'
        ct = 2 if H % 64 == 0 else 1
        if ct == 2 and ceil_div(R, 128) * (H // 64) < 128:
            ct = 1
        return dict(family='k_gru_fwd', ct=ct, grid=(ceil_div(R, 128), H // (32 * ct)), capped=False)
    if entry == 'bwd_data':
        if H <= 64 and IN in (H, 2 * H):
            ntiles = ceil_div(R, 256)
            r = _persistent(8 * ntiles, min(ntiles, 256))
            r.update(family='k_gru_bwd_data_split' if IN == H else 'k_gru_bwd_data_lds', capped=ntiles > 256,
                     empty_items=8 * ntiles - ceil_div(R, 32))
            return r
        nt = 4 if (H % 128 == 0 and IN % 128 == 0) else 2 if H % 64 == 0 else 1
        if nt > 1 and ceil_div(R, 128) * ((IN + H) // (32 * nt)) < 128:
            nt = 1
        return dict(family='k_gru_bwd_data', nt=nt, grid=(ceil_div(R, 128), (IN + H) // (32 * nt)), capped=False)
    if entry == 'bwd_weights':
        ntiles = ceil_div(R, 32)
        if H == 64 and IN == H and xmode != 2:
            slabs = min(ntiles, 512)
            return dict(family='k_gru_bwd_weights_split', slabs=slabs, grid=(slabs,), fold=slabs > 64,
                        tiles_per_slab=ceil_div(ntiles, slabs))
        if H % 64 == 0 and IN % 64 == 0:
            n_cc = ceil_div(IN + H, 128)
            per = (H // 64) * n_cc
            slabs = min(ntiles, max(1, 1024 // per))
            return dict(family='k_gru_bwd_weights_chunk', slabs=slabs, grid=(slabs, per), fold=slabs > 64,
                        tiles_per_slab=ceil_div(ntiles, slabs))
        nq, nch = 3 * H // 32, ceil_div(IN + H, 128)                 # plan_weights (gru_bwd.hip:1094-1110)
        n = max(1, min(ceil_div(R, 64), max(1, 4096 // (nq * nch))))
        rs = max(2, (ceil_div(R, n) + 1) & ~1)
        n = max(1, ceil_div(R, rs))
        return dict(family='k_gru_bwd_weights', slabs=n, rows_per_slab=rs, grid=(ceil_div(n * nq * nch, 4),), fold=n > 64)
    raise ValueError(entry)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def weight_q(H: int, IN: int) -> int:
    return max(1, round(128 / (IN + H) ** 0.5))


def _grid(shape, lo, hi, step, gen):
    """Multiples of `step` in [lo * step, hi * step]."""
    return torch.randint(lo, hi + 1, shape, generator=gen).double() * step


@functools.lru_cache(maxsize=4)
def inputs(case: Case) -> SimpleNamespace:
    """Everything a case reads, in float64, from a seed that depends on the shape alone.  Shared, never modified."""
    H, IN, xmode, R = case.H, case.IN, case.xmode, case.R
    assert IN == (2 * H if xmode == 2 else H if xmode in (1, 3) else IN)
    gen = torch.Generator().manual_seed(1000003 * H + 7919 * IN + 101 * xmode + R)
    extra = DN if xmode == 3 else 0                     # (room for the det rows next to the R list rows)
    N = 2 * R + 7 + extra
    perm = torch.randperm(N, generator=gen)
    rows = perm[:R].sort().values
    if case.shuffled:
        rows = rows[torch.randperm(R, generator=gen)]
    others = perm[R:].sort().values                     # R + 7 (+ DN) rows outside the list: the endpoints come from these
    x = SimpleNamespace(N=N, rows=rows, others=others, src=None, dst=None, dets=None, msg=None)
    if xmode in (1, 2):
        x.src = others[torch.randint(0, others.numel(), (R,), generator=gen)]
        x.dst = others[torch.randint(0, others.numel(), (R,), generator=gen)]
    elif xmode == 3:
        # positions into the det list; 32-row tiles alternate between few distinct dets (staged in LDS by the tiled kernels)
        # and more than 24 of them (their gather path), as tests/test_fwd_zero_state.py builds its lists
        x.dets = others[torch.randperm(others.numel(), generator=gen)[:DN]].sort().values
        e = torch.arange(R)
        few = (e // 32) % 2 == 0
        ri = lambda hi: torch.randint(0, hi, (R,), generator=gen)
        x.src = torch.where(few, (e // 32) % (DN - 8) + ri(8), ri(DN - 8))
        x.dst = torch.where(few, (e // 32 + 3) % (DN - 8) + ri(8), ri(DN))
    else:
        x.msg = _grid((R, IN), -8, 8, 1 / 8, gen)       # compact messages
    q = weight_q(H, IN)
    x.h = _grid((N, H), -8, 8, 1 / 8, gen)
    x.W_ih = _grid((3 * H, IN), -q, q, 1 / 64, gen)
    x.W_hh = _grid((3 * H, H), -q, q, 1 / 64, gen)
    x.b_ih = _grid((3 * H,), -8, 8, 1 / 16, gen)
    x.b_hh = _grid((3 * H,), -8, 8, 1 / 16, gen)
    # rounded quantities anyway: seeded normals (fp32 values, so that both evaluations and the kernels read the same numbers)
    nrm = lambda *s: torch.randn(*s, generator=gen).double()
    x.w_head, x.d_hout, x.dy, x.add = nrm(H), nrm(R, H), nrm(N), nrm(N, H)
    return x


def message(x: SimpleNamespace, xmode: int, h: torch.Tensor, dtype) -> torch.Tensor:
    """x of the cell for xmode 0, 1, 2 ([R, IN])."""
    if xmode == 0:
        return x.msg.to(dtype)
    if xmode == 1:
        return h[x.src] - h[x.dst]
    if xmode == 2:
        return torch.cat([h[x.src], h[x.dst]], 1)
    raise ValueError(xmode)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def evaluate(case: Case, x: SimpleNamespace, dtype=torch.float64, up: Optional[int] = None, fuse: bool = False,
             zero_state: bool = False) -> SimpleNamespace:
    """The cell over the R list rows.  Forward: h_out, the planes r, z, n, hn = W_hn h + b_hn, parts [R, H / 32] (the dot product
    of h_out with w_head over each 32-column slice), and P [DN, 3H] for xmode 3.  With `up` in {1, 2, 3} also the backward
    by autograd for the upstream gradient d_hout (1), dy * w_head (2) or their sum (3): d_msg (the gradient of the cell's x,
    [R, IN]), d_h ([R, H], with `fuse` plus add[src] - add[dst]), dW_ih, dW_hh, db_ih, db_hh."""
    H, xmode = case.H, case.xmode
    t = lambda v: v.detach().clone().to(dtype)            # (never a view of the shared inputs)
    h = t(x.h)
    if zero_state:
        h = h.clone()
        h[x.rows] = 0
    grad = up is not None
    W_ih, W_hh, b_ih, b_hh = (t(v).requires_grad_(grad) for v in (x.W_ih, x.W_hh, x.b_ih, x.b_hh))
    hrow = h[x.rows].clone().requires_grad_(grad)
    o = SimpleNamespace()
    if xmode == 3:
        assert not grad, 'the projected form has no backward entry of its own'
        o.P = h[x.dets] @ W_ih.t()
        gi = (o.P[x.src] - o.P[x.dst]) + b_ih
        xin = None
    else:
        xin = message(x, xmode, h, dtype).clone().requires_grad_(grad)
        gi = xin @ W_ih.t() + b_ih
    gh = hrow @ W_hh.t() + b_hh
    o.r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    o.z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    o.hn = gh[:, 2 * H:]
    o.n = torch.tanh(gi[:, 2 * H:] + o.r * o.hn)
    o.h_out = (1 - o.z) * o.n + o.z * hrow
    o.pre = torch.cat([gi[:, :2 * H] + gh[:, :2 * H], gi[:, 2 * H:], o.hn], 1)      # the four pre-activations
    o.parts = (o.h_out.view(-1, H // 32, 32) * t(x.w_head).view(H // 32, 32)).sum(-1)
    if grad:
        dh_up = torch.zeros(case.R, H, dtype=dtype)
        if up & 1:
            dh_up = dh_up + t(x.d_hout)
        if up & 2:
            dh_up = dh_up + t(x.dy)[x.rows, None] * t(x.w_head)[None, :]
        (o.h_out * dh_up).sum().backward()
        o.d_msg, o.d_h = xin.grad, hrow.grad
        if fuse:
            o.d_h = o.d_h + (t(x.add)[x.src] - t(x.add)[x.dst])
        o.dW_ih, o.dW_hh, o.db_ih, o.db_hh = W_ih.grad, W_hh.grad, b_ih.grad, b_hh.grad
    for k, v in list(vars(o).items()):
        setattr(o, k, v.detach())
    return o


def bound(qty: str, ref64: torch.Tensor, ref32: torch.Tensor, factor: float = FACTOR) -> Tuple[float, float, float]:
    """(bound, err32, scale) of a rounded quantity: max(factor * err32, 32 * 2^-24 * scale) and never past CEILING[qty] * scale;
    scale = max(1, max |ref64|), err32 the distance of the HOST fp32 evaluation of the same definition from float64."""
    scale = max(1.0, float(ref64.abs().max())) if ref64.numel() else 1.0
    err32 = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return min(max(factor * err32, 32.0 * U32 * scale), CEILING[qty] * scale), err32, scale


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def _fwd(H, xmode, Rs, tag, IN=None):
    IN = IN if IN is not None else (2 * H if xmode == 2 else H)
    return [Case('fwd', H, IN, xmode, R, tag) for R in Rs]


FWD = (
    _fwd(64, 3, (1, 31, 32, 33, 192, 193), 'k_gru_fwd_split<64>: one row, around one 32-row tile, around one 192-row pass')
    + _fwd(64, 3, (49160,), 'k_gru_fwd_split<64> beyond its grid cap: 3074 items, 13 a block, 19 idle blocks, partial last tile')
    + _fwd(32, 3, (1, 33, 256, 257), 'k_gru_fwd_split<32>: one row, a partial second tile, around one 256-row pass')
    + _fwd(32, 3, (65544,), 'k_gru_fwd_split<32> beyond its grid cap: 2049 items, 9 a block, 28 idle blocks')
    + _fwd(64, 1, (1, 33, 192, 193), 'k_gru_fwd_lds<64, diff>')
    + _fwd(64, 1, (49160,), 'k_gru_fwd_lds<64, diff> beyond its grid cap')
    + _fwd(32, 1, (1, 257), 'k_gru_fwd_lds<32, diff>')
    + _fwd(32, 2, (1, 257), 'k_gru_fwd_lds<32, concat>')
    + _fwd(64, 2, (1, 33, 127, 128, 129, 16256), 'k_gru_fwd<1, concat> at H = 64 (the weights do not fit LDS)')
    + _fwd(64, 2, (16257,), 'k_gru_fwd<2, concat> at H = 64: first R of CT = 2')
    + [c for x in (0, 1, 2) for c in _fwd(128, x, (129, 8064), f'k_gru_fwd<1, {x}> at H = 128', IN=None if x else 128)]
    + [c for x in (0, 1, 2) for c in _fwd(128, x, (8065,), f'k_gru_fwd<2, {x}> at H = 128: first R of CT = 2', IN=None if x else 128)]
    + _fwd(256, 0, (3968,), 'k_gru_fwd<1, 0> at H = 256', IN=256)
    + _fwd(256, 0, (3969,), 'k_gru_fwd<2, 0> at H = 256', IN=256)
    + _fwd(256, 2, (3969,), 'k_gru_fwd<2, concat> at H = 256')
    + _fwd(384, 0, (2688,), 'k_gru_fwd<1, 0> at a width above 256', IN=384)
    + _fwd(384, 0, (2689,), 'k_gru_fwd<2, 0> at a width above 256', IN=384)
    + [Case('fwd', 64, 64, 1, 193, 'h_out 4 bytes off: the generic fallback of the H = 64 diff cell', misalign=True),
       Case('fwd', 64, 64, 3, 193, 'a shuffled row list', shuffled=True)]
)

# (UP, fuse) in full at the small R of each family, one combination at the large ones
ALL_UP = tuple((u, f) for u in (1, 2, 3) for f in (False, True))


def _bwd_data(H, IN, Rs, tag):
    return [Case('bwd_data', H, IN, 1 if IN == H else 2, R, tag) for R in Rs]


BWD_DATA = (
    [c for H in (32, 64) for c in _bwd_data(H, H, (1,), f'k_gru_bwd_data_split<{H}>: seven of the eight items lie beyond R')]
    + [c for H in (32, 64) for c in _bwd_data(H, H, (33, 256, 257), f'k_gru_bwd_data_split<{H}>')]
    + [c for H in (32, 64) for c in _bwd_data(H, H, (65544,), f'k_gru_bwd_data_split<{H}> beyond its grid cap: idle blocks')]
    + [c for H in (32, 64) for c in _bwd_data(H, 2 * H, (1, 257), f'k_gru_bwd_data_lds<{H}, concat>')]
    + _bwd_data(128, 128, (8064,), 'k_gru_bwd_data<1>') + _bwd_data(128, 128, (8065,), 'k_gru_bwd_data<4>: first R of NT = 4')
    + _bwd_data(128, 256, (5376,), 'k_gru_bwd_data<1>') + _bwd_data(128, 256, (5377,), 'k_gru_bwd_data<4>: first R of NT = 4')
    + _bwd_data(256, 256, (3968,), 'k_gru_bwd_data<1>') + _bwd_data(256, 256, (3969,), 'k_gru_bwd_data<4>: first R of NT = 4')
    + _bwd_data(256, 512, (2688,), 'k_gru_bwd_data<1>') + _bwd_data(256, 512, (2689,), 'k_gru_bwd_data<4>: first R of NT = 4')
)


def up_fuse_of(case: Case):
    """The (UP, fuse) combinations a backward-data case runs."""
    if case.R <= 257:
        return ALL_UP
    return ((3, True),)


def _bwd_w(H, IN, xmode, Rs, tag):
    return [Case('bwd_weights', H, IN, xmode, R, tag) for R in Rs]


BWD_WEIGHTS = (
    _bwd_w(128, 128, 0, (33, 8192), 'k_gru_bwd_weights_chunk: 2 and 256 slabs of one tile')
    + _bwd_w(128, 128, 0, (8193,), 'k_gru_bwd_weights_chunk: 256 slabs, more than one tile a slab')
    + _bwd_w(256, 256, 0, (2048,), 'k_gru_bwd_weights_chunk: 64 slabs of one tile')
    + _bwd_w(256, 256, 0, (2049,), 'k_gru_bwd_weights_chunk: 64 slabs (its cap at this width), the first with two tiles')
    + _bwd_w(64, 128, 2, (2049,), 'k_gru_bwd_weights_chunk: 65 slabs, the two-level fold')
    + _bwd_w(32, 32, 0, (1, 63, 64), 'k_gru_bwd_weights<0>: one slab')
    + _bwd_w(32, 32, 0, (65,), 'k_gru_bwd_weights<0>: two slabs')
    + _bwd_w(32, 32, 1, (4097,), 'k_gru_bwd_weights<1>: 65 slabs, the two-level fold')
)

TILES = [Case('tiles', 64, 64, 3, 49160, 'k_gru_fwd_split_tiled<64> beyond its grid cap'),
         Case('tiles_zs', 64, 64, 3, 73736, 'the zero-state tiled kernel beyond its cap of 768 blocks of 96 rows')]

TABLE = FWD + BWD_DATA + BWD_WEIGHTS + TILES

# every switch and cap: (entry, H, IN, xmode, the key of route() that switches, its value below, the value from R on, R)
SWITCHES = (
    [('fwd', 64, 128, 2, 'ct', 1, 2, 16257)]
    + [('fwd', 128, 2 * 128 if x == 2 else 128, x, 'ct', 1, 2, 8065) for x in (0, 1, 2)]
    + [('fwd', 256, 256, 0, 'ct', 1, 2, 3969), ('fwd', 384, 384, 0, 'ct', 1, 2, 2689)]
    + [('bwd_data', 128, 128, 1, 'nt', 1, 4, 8065), ('bwd_data', 128, 256, 2, 'nt', 1, 4, 5377),
       ('bwd_data', 256, 256, 1, 'nt', 1, 4, 3969), ('bwd_data', 256, 512, 2, 'nt', 1, 4, 2689)]
)
