"""Graphs at the branch points of the attention kernels (csrc/att.hip: k_att_score, k_att_fwd, k_att_dotk, k_att_bwd_edge,
k_att_bwd_dha), inputs on a grid that keeps everything up to the softmax exact in fp32, and the float64 definition of the
operation (include/tmpnn.h, row G) with its gradients.  Host code only, shared by tests/test_att_cases.py (CPU: every graph
lands where the table says, the inputs are exact, the definition equals a dense N x N evaluation of the formula) and
tests/test_att_shapes_gpu.py.

What the kernels branch on, and what therefore varies over the family:
  run chunks     k_att_fwd / k_att_bwd_dha walk a det's CSR run in chunks of lpr = H / 4 positions; chunks 0 and 1 come from a
                 prefetch, nch > 2 takes an early advance() and un-prefetched loads
  wave sharing   64 / lpr dets sit side by side in a wave and the loops run to the longest of them
  rows in flight U rows at a time (U depends on K in k_att_score, k_att_bwd_edge, k_att_bwd_dha)
  det chunks     ATT_CHUNK = 32 positions of the visiting order (det_order or 0, 1, 2, ...) per block visit
  grid caps      k_att_fwd / k_att_bwd_dha 16 384 blocks, k_att_score 16 384 blocks, k_att_dotk 4096 blocks
The definition never touches rowptr / inc for a value: the kernel's own CSR must not be its own witness.  Only the map from
CSR position to (edge, side), which is needed to read the kernel's alpha, comes from the graph (inc_edge_endpoint());
tests/test_att_cases.py holds it to src / dst."""
from __future__ import annotations

import functools
from types import SimpleNamespace
from typing import Dict, FrozenSet, Optional, Set, Tuple

import torch
import torch.nn.functional as F

from tests import agg_cases as ac
from trackmpnn_amd.graph import FrameGraph, dense_static_graph

HS = ac.HS
U32 = ac.U32
LEAKY = 0.2
P_DROP = 0.5                         # 1 / (1 - p) = 2: a kept alpha is doubled exactly
ATT_CHUNK = 32

SMALL = ('pair', 'no_edges', 'star_out', 'star_in', 'ladder131', 'ladder70_sparse', 'mid3x33', 'ragged')
LARGE = {
    'path16400': lambda: ac.path_graph(16400),
    'path524328': lambda: ac.path_graph(524328),
    'dense2x257': lambda: dense_static_graph(2, 257),
}
SIZES = {'path16400': (16399, 16400), 'path524328': (524327, 524328), 'dense2x257': (66049, 514)}      # name -> (E, Dn)


@functools.lru_cache(maxsize=None)
def graph(name: str) -> FrameGraph:
    """The graph on the host, built once, shared and never modified."""
    return LARGE[name]() if name in LARGE else ac.graph(name)


def fresh_graph(name: str) -> FrameGraph:
    return LARGE[name]() if name in LARGE else ac.fresh_graph(name)


# ---- where a graph lands ----------------------------------------------------------------------------------------------------------
def lpr(H: int) -> int:
    """Lanes per row = positions per chunk of a run."""
    return H // 4


def run_classes(deg, H: int) -> FrozenSet[str]:
    """Which of the run lengths 0, 1, lpr-1, lpr, lpr+1, 2lpr-1, 2lpr, 2lpr+1 and '3lpr+' (nch > 2 with a full third chunk or
    more) occur among the degrees `deg`."""
    L = lpr(H)
    names = {0: '0', 1: '1', L - 1: 'l-1', L: 'l', L + 1: 'l+1', 2 * L - 1: '2l-1', 2 * L: '2l', 2 * L + 1: '2l+1'}
    ds = set(int(x) for x in deg)
    out = {names[d] for d in ds if d in names}
    if any(d >= 3 * L for d in ds):
        out.add('3l+')
    return frozenset(out)


ALL_TO_2L1 = frozenset({'0', '1', 'l-1', 'l', 'l+1', '2l-1', '2l', '2l+1'})


def visiting_order(g: FrameGraph) -> torch.Tensor:
    return torch.arange(g.Dn) if g.det_order is None else g.det_order.long().cpu()


def wave_runs(g: FrameGraph, H: int) -> torch.Tensor:
    """[waves, 64 / lpr] run lengths of the dets that share a wave of k_att_fwd / k_att_bwd_dha: consecutive positions of the
    visiting order (ATT_DET_ROUNDS: position = chunk * 32 + round * dpr + wave * ngrp + group; 32 is a multiple of ngrp).
    Slots behind the last det count as empty runs (-1 here, so that they can be told from a det of degree 0)."""
    ngrp = 64 // lpr(H)
    s, d = ac.degrees(g)
    deg = (s + d)[visiting_order(g)]
    pad = (-g.Dn) % ngrp
    deg = torch.cat([deg, torch.full((pad,), -1, dtype=deg.dtype)])
    return deg.reshape(-1, ngrp)


def mixed_waves(g: FrameGraph, H: int) -> bool:
    """Do dets of different run length share a wave?"""
    w = wave_runs(g, H).clamp(min=0)
    return bool((w.min(1).values != w.max(1).values).any())


def score_unroll(K: int) -> int:
    return 4 if K <= 2 else (2 if K <= 4 else 1)


def caps_exceeded(E: int, Dn: int, H: int, K: int) -> Set[str]:
    """The launch grids that are capped (the kernel then loops): csrc/att.hip, tmpnn_att_fwd, att_bwd_impl, att_grid."""
    rpb = 256 // lpr(H)
    out = set()
    per = rpb * score_unroll(K)
    if -(-E // per) > 16384:
        out.add('score')
    if -(-Dn // rpb) > 4096:
        out.add('dotk')
    if -(-Dn // ATT_CHUNK) > 16384:
        out.add('fwd')
    return out


# name -> H -> (run classes, dets of different run length share a wave); asserted by tests/test_att_cases.py.
_C = lambda *names: frozenset(names)
_NARROW = (32, 64, 128)              # 8, 4 and 2 dets a wave; at H = 256 a wave holds one det
_LADDER = ALL_TO_2L1 | {'3l+'}
_RAGGED = _C('l-1', 'l', 'l+1', '2l-1', '2l', '2l+1', '3l+')                  # degrees 3..53
TABLE: Dict[str, Dict[int, Tuple[FrozenSet[str], bool]]] = {
    # (a wave's slots behind the last det are empty runs: two dets of degree 1 beside six of those)
    'pair': {32: (_C('1'), True), 64: (_C('1'), True), 128: (_C('1'), False), 256: (_C('1'), False)},
    'no_edges': {H: (_C('0'), False) for H in HS},
    'star_out': {H: (_C('0', '1', '3l+'), H != 256) for H in HS},
    'star_in': {H: (_C('1', '3l+'), H != 256) for H in HS},
    'ladder131': {**{H: (_LADDER, True) for H in _NARROW}, 256: (ALL_TO_2L1, False)},      # top degree 130 < 3 * 64
    # top degree 69: at H = 256 (lpr = 64) the runs end at lpr + 5, the second chunk is never full
    'ladder70_sparse': {32: (_LADDER, True), 64: (_LADDER, True), 128: (ALL_TO_2L1, True),
                        256: (_C('0', '1', 'l-1', 'l', 'l+1'), False)},
    'mid3x33': {32: (_C('3l+'), True), 64: (_C('2l+1', '3l+'), True), 128: (_C('l+1'), True), 256: (_C(), False)},
    'ragged': {32: (_RAGGED, True), 64: (_RAGGED, True), 128: (_C('l-1', 'l', 'l+1'), True), 256: (_C(), False)},
    'path16400': {H: (_C('1'), H != 256) for H in HS},                         # degrees 1 (the two ends) and 2
    'path524328': {H: (_C('1'), H != 256) for H in HS},
    'dense2x257': {H: (_C('3l+'), H in (32, 64)) for H in HS},                 # every degree 257; 514 dets: a wave's tail is empty
}
# (graph, H, K) -> the capped grids, for the cases of the GPU file that are there for it; everything else exceeds none
CAPS = {('path16400', 256, 1): {'dotk'}, ('dense2x257', 256, 5): {'score'}, ('path524328', 32, 1): {'fwd', 'dotk'}}


# every (graph, H, K, hot) that tests/test_att_shapes_gpu.py runs; tests/test_att_cases.py asserts the inputs' exactness on each
FAMILY_CASES = [(n, H, 2, False) for n in SMALL for H in HS]
HEAD_CASES = [(n, H, K, False) for n in ('ladder131', 'star_out') for H in HS for K in (1, 3, 5, 8)]
HOT_CASES = [('ladder131', 256, 2, True), ('star_in', 256, 2, True)]
GRID_CASES = [('path16400', 256, 1, False), ('dense2x257', 256, 5, False), ('path524328', 32, 1, False)]


# ---- inputs on a grid -------------------------------------------------------------------------------------------------------------
def inputs(g: FrameGraph, H: int, K: int, hot: bool = False, seed: int = 0) -> SimpleNamespace:
    """h [N, H] multiples of 1/8 in [-1, 1], W [K, H, H] (head k's W_att, in x out) multiples of 1/8 in [-1/2, 1/2], a [K, H]
    multiples of 1/32 in [-1/4, 1/4] (hot: times 8).  fp32 tensors.  Every product h W is a multiple of 1/64 below 1/2, a row
    of ha a multiple of 1/64 below H / 2: exact in fp32 in any order, and so are the three bf16 parts of an operand (h and W
    have four significant bits: the first part is the value, the others are 0).  |ha_s - ha_d| a is a multiple of 2^-11
    (hot 2^-8); its sum is exact in any order while sum |diff| |a| stays below 2^13 (hot 2^16): exactness() measures that."""
    gen = torch.Generator().manual_seed(7919 * seed + 31 * H + K + (500 if hot else 0))
    h = torch.randint(-8, 9, (g.N, H), generator=gen).float() / 8
    W = torch.randint(-4, 5, (K, H, H), generator=gen).float() / 8
    a = torch.randint(-8, 9, (K, H), generator=gen).float() / 32
    if hot:
        a = a * 8
    return SimpleNamespace(h=h, W=W, a=a, hot=hot)


def draw_keep(g: FrameGraph, K: int, seed: int = 0) -> torch.Tensor:
    """bool [K, E, 2]: head k keeps the src side / dst side of edge e."""
    gen = torch.Generator().manual_seed(104729 * seed + K + 13 * g.E)
    return torch.rand(K, g.E, 2, generator=gen) > 0.5


def draw_d_es(g: FrameGraph, H: int, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(15485863 * seed + H + g.Dn)
    return torch.randn(g.Dn, H, generator=gen)


def det_index(g: FrameGraph) -> Tuple[torch.Tensor, torch.Tensor]:
    """(det index of src[e], det index of dst[e]) from src / dst / det_row alone."""
    det_of = torch.full((g.N,), -1, dtype=torch.long, device=g.src.device)
    det_of[g.det_row.long()] = torch.arange(g.Dn, device=g.src.device)
    sp, dp = det_of[g.src.long()], det_of[g.dst.long()]
    assert g.E == 0 or (int(sp.min()) >= 0 and int(dp.min()) >= 0)
    return sp, dp


def position_map(g: FrameGraph) -> Tuple[torch.Tensor, torch.Tensor]:
    """For every CSR position: (edge index, 0 = src side / 1 = dst side).  From the graph's inc; asserted against src / dst."""
    e, side = g.inc_edge_endpoint()
    return e.cpu(), side.cpu()


def keep_bytes(g: FrameGraph, keep: torch.Tensor) -> torch.Tensor:
    """uint8 [2E] in CSR order, bit k = head k keeps the position."""
    e, side = position_map(g)
    kk = keep[:, e, side].to(torch.int32)                       # [K, 2E]
    b = torch.zeros(2 * g.E, dtype=torch.int32)
    for k in range(keep.shape[0]):
        b |= kk[k] << k
    return b.to(torch.uint8)


def to_positions(g: FrameGraph, x: torch.Tensor) -> torch.Tensor:
    """[K, E, 2] -> [K, 2E] in CSR order."""
    e, side = position_map(g)
    return x[:, e, side]


def from_positions(g: FrameGraph, x: torch.Tensor) -> torch.Tensor:
    """[K, 2E] in CSR order -> [K, E, 2]."""
    e, side = position_map(g)
    out = torch.full((x.shape[0], g.E, 2), float('nan'), dtype=x.dtype)
    out[:, e, side] = x
    return out


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def evaluate(g: FrameGraph, x: SimpleNamespace, keep: Optional[torch.Tensor] = None, d_es: Optional[torch.Tensor] = None,
             dtype=torch.float64) -> SimpleNamespace:
    """include/tmpnn.h, row G, in `dtype` with torch ops, head by head, from src / dst / edge_row / det_row alone:
      ha [Dn, K, H]   h[det rows] W_k
      t, score [K, E] |ha_k[src] - ha_k[dst]| . a_k and its LeakyReLU_0.2
      mx, den [K, Dn] the softmax's maximum and sum of exp over a det's incident edges ((0, 1) for a det without any)
      alpha [K, E, 2] what the src det / the dst det gives the edge, after dropout (keep bool [K, E, 2], scale 1 / (1 - p))
      esk [K, Dn, H]  1/K (sum_{e: src = d} alpha h[row e] - sum_{e: dst = d} alpha h[row e]);  es [Dn, H] = sum_k esk
    and, with d_es [Dn, H] given, the gradients of sum(es * d_es): d_h [N, H], dW [K, H, H], da [K, H] (autograd: abs'(0) = 0,
    LeakyReLU'(0) = 0.2, the conventions of the kernels' sgn() and `s > 0 ? 1 : 0.2`)."""
    K, H = x.a.shape
    E, Dn, N = g.E, g.Dn, g.N
    grad = d_es is not None
    er, dr = g.edge_row.long(), g.det_row.long()
    sp, dp = det_index(g)
    det = torch.cat([sp, dp])
    er2 = torch.cat([er, er])
    sign = torch.cat([torch.ones(E, dtype=dtype), -torch.ones(E, dtype=dtype)])
    h = x.h.detach().to(dtype, copy=True).requires_grad_(grad)             # (leaves of their own: x stays as it is)
    W = x.W.detach().to(dtype, copy=True).requires_grad_(grad)
    a = x.a.detach().to(dtype, copy=True).requires_grad_(grad)
    r = SimpleNamespace(ha=[], t=[], score=[], mx=[], den=[], alpha=[], esk=[])
    loss = 0
    with torch.set_grad_enabled(grad):
        for k in range(K):
            ha = h[dr] @ W[k]
            t = (torch.abs(ha[sp] - ha[dp]) * a[k]).sum(1)
            s = F.leaky_relu(t, LEAKY)
            sc = torch.cat([s, s])
            mx = torch.full((Dn,), -float('inf'), dtype=dtype).scatter_reduce(0, det, sc.detach(), 'amax')
            ex = torch.exp(sc - mx[det])
            den = torch.zeros(Dn, dtype=dtype).index_add(0, det, ex)
            al = ex / den[det]
            if keep is not None:
                al = al * torch.cat([keep[k, :, 0], keep[k, :, 1]]).to(dtype) / (1.0 - P_DROP)
            esk = torch.zeros(Dn, H, dtype=dtype).index_add(0, det, h[er2] * (al * sign / K)[:, None])
            if grad:
                loss = loss + (esk * d_es.to(dtype)).sum()
            iso = torch.isinf(mx)
            r.ha.append(ha.detach()); r.t.append(t.detach()); r.score.append(s.detach())
            r.mx.append(torch.where(iso, torch.zeros_like(mx), mx)); r.den.append(torch.where(iso, torch.ones_like(den), den).detach())
            r.alpha.append(torch.stack([al[:E], al[E:]], 1).detach()); r.esk.append(esk.detach())
    out = SimpleNamespace(ha=torch.stack(r.ha, 1), t=torch.stack(r.t), score=torch.stack(r.score), mx=torch.stack(r.mx),
                          den=torch.stack(r.den), alpha=torch.stack(r.alpha), esk=torch.stack(r.esk))
    out.es = out.esk.sum(0)
    if grad:
        loss.backward()
        z = torch.zeros_like
        out.d_h = h.grad if h.grad is not None else z(h)
        out.dW = W.grad if W.grad is not None else z(W)
        out.da = a.grad if a.grad is not None else z(a)
    return out


def exactness(g: FrameGraph, x: SimpleNamespace) -> SimpleNamespace:
    """The conditions under which every summation order gives the same fp32 ha and t: bits of the fp32 evaluation against the
    float64 one, and the head room of the sums of absolute addends."""
    r64, r32 = evaluate(g, x), evaluate(g, x, dtype=torch.float32)
    sp, dp = det_index(g)
    K, H = x.a.shape
    abs_t = torch.stack([((r64.ha[sp, k] - r64.ha[dp, k]).abs() * x.a[k].double().abs()).sum(1) for k in range(K)]) \
        if g.E else torch.zeros(K, 0, dtype=torch.float64)
    abs_ha = x.h.double().abs()[g.det_row.long()] @ x.W.double().abs().sum(0)      # >= every head's sum |h||W|
    return SimpleNamespace(
        ha_equal=torch.equal(r32.ha.double(), r64.ha), t_equal=torch.equal(r32.t.double(), r64.t),
        # multiples of 2^-6 below 2^18 and multiples of 2^-11 (hot: 2^-8) below 2^13 (2^16): 24 bits hold every partial sum
        ha_room=float(abs_ha.max()) if abs_ha.numel() else 0.0, t_room=float(abs_t.max()) if abs_t.numel() else 0.0,
        t_limit=2.0 ** 16 if x.hot else 2.0 ** 13,
        score_max=float(r64.score.max()) if g.E else 0.0, score_min=float(r64.score.min()) if g.E else 0.0,
        diff_zeros=int(sum(((r64.ha[sp, k] - r64.ha[dp, k]) == 0).sum() for k in range(K))) if g.E else 0,
        t_zeros=int((r64.t == 0).sum()))


def bound(ref64: torch.Tensor, ref32: torch.Tensor) -> Tuple[float, float, float]:
    """(bound, err32, scale) for a rounded quantity: max(4 err32, 32 * 2^-24 * scale), scale = max(1, max |ref64|), err32 the
    distance of the HOST fp32 evaluation of the same definition from the float64 one.  4: the kernel sums in another (fixed)
    order and uses the device expf; with the inputs on the grid there is no kink to forgive."""
    scale = max(1.0, float(ref64.abs().max())) if ref64.numel() else 1.0
    err32 = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return max(4.0 * err32, 32.0 * U32 * scale), err32, scale
