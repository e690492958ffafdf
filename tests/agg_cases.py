"""Graphs at the branch points of the aggregation kernels (csrc/agg.hip: k_gather_pipe, k_segsum_pipe, k_segsum_tiles), the
float64 definitions of the operations (include/tmpnn.h, rows E and F) and the rounding bounds the HIP path is held to.  Host
code only, shared by tests/test_agg_cases.py (CPU: every graph really lands on the branch the table says, the reference equals
the dense matrix definition) and tests/test_agg_shapes_gpu.py.

What the kernels branch on, and what therefore varies over the family:
  launch shape   deep = 2E > 24 Dn: k_segsum_pipe<., 8, 16> (and <.., LIM> with U = 8), else <., 4, 32>
  pass width     a det's CSR run is summed in passes of P = (256 / H) * U incidences, U = 8 (deep) or 4 (shallow)
  empty runs     dets without an edge; E = 0
  det_order      NULL or a permutation
  chunk tails    Dn below one wave's share of a chunk, Dn no multiple of the chunk
The reference never touches rowptr / inc: the kernel's own CSR must not be its own witness."""
from __future__ import annotations

import functools
from typing import Callable, Dict, Optional, Sequence, Set, Tuple

import torch

from trackmpnn_amd.graph import FrameGraph, dense_static_graph, graph_from_edges

HS = (32, 64, 128, 256)
U32 = 2.0 ** -24                     # unit roundoff of fp32


def bipartite_graph(A: int, B: int, pairs: Sequence[Tuple[int, int]], iso_a: int = 0, iso_mid: int = 0,
                    iso_b: int = 0) -> FrameGraph:
    """Rows: iso_a isolated dets, A src dets, the first half of the edge rows, iso_mid isolated dets, the second half of the edge
    rows, B dst dets, iso_b isolated dets.  `pairs` = (src a, dst b); the edges are listed src-major."""
    pairs = sorted(pairs)
    E = len(pairs)
    h1 = E // 2
    src0 = iso_a
    e0 = src0 + A
    mid0 = e0 + h1
    e1 = mid0 + iso_mid
    dst0 = e1 + (E - h1)
    N = dst0 + B + iso_b
    is_edge = torch.zeros(N, dtype=torch.bool)
    is_edge[e0:mid0] = True
    is_edge[e1:dst0] = True
    pr = torch.tensor(pairs, dtype=torch.long).reshape(E, 2)
    return graph_from_edges(N, is_edge, src0 + pr[:, 0], dst0 + pr[:, 1])


def ladder(n: int, **iso) -> FrameGraph:
    """src a in 0..n-1 -> dsts 0..a-1: src degrees 0..n-1, dst degrees 1..n-1 (dst b is met by srcs b+1..n-1)."""
    return bipartite_graph(n, n - 1, [(a, b) for a in range(n) for b in range(a)], **iso)


def path_graph(Dn: int, device='cpu') -> FrameGraph:
    """det, edge, det, edge, ..., det: Dn dets, Dn - 1 edges, every degree 1 or 2 (the grid-stride case)."""
    N = 2 * Dn - 1
    rows = torch.arange(N, device=device)
    er = rows[1::2]
    return graph_from_edges(N, (rows & 1) == 1, er - 1, er + 1, device=device)


def _ragged() -> FrameGraph:
    from tests.gpu_stage_checks import make_graph
    return make_graph(B=40, frames=7, mean=7, seed=3)


# name -> (constructor, E, Dn, deep): the figures are asserted by tests/test_agg_cases.py, so that a graph edited later cannot
# drift off its branch unnoticed
FAMILY: Dict[str, Tuple[Callable[[], FrameGraph], int, int, bool]] = {
    'pair': (lambda: bipartite_graph(1, 1, [(0, 0)]), 1, 2, False),
    'no_edges': (lambda: bipartite_graph(3, 2, []), 0, 5, False),
    'star_out': (lambda: bipartite_graph(1, 1000, [(0, b) for b in range(1000)], iso_a=3, iso_mid=1, iso_b=2), 1000, 1007, False),
    'star_in': (lambda: bipartite_graph(1000, 1, [(a, 0) for a in range(1000)]), 1000, 1001, False),
    'ladder131': (lambda: ladder(131), 8515, 261, True),
    'ladder70_sparse': (lambda: ladder(70, iso_a=30, iso_b=40), 2415, 209, False),
    'k24x24': (lambda: dense_static_graph(2, 24), 576, 48, False),
    'k24x25': (lambda: bipartite_graph(24, 25, [(a, b) for a in range(24) for b in range(25)]), 600, 49, True),
    'mid3x33': (lambda: dense_static_graph(3, 33), 2178, 99, True),
    'ragged': (_ragged, 17816, 1994, False),
}
# (T, D) of dense_static_graph -> E: graphs that trackmpnn_amd.graph.dense_seg_plan serves (E >= 8192 and E >= 32 Dn)
DENSE = {(2, 107): 11449, (3, 70): 9800, (3, 99): 19602, (2, 139): 19321}


@functools.lru_cache(maxsize=None)
def graph(name: str) -> FrameGraph:
    """The family's graph on the host, built once.  Shared and never modified: whoever needs another det_order or a plan takes
    fresh_graph()."""
    return FAMILY[name][0]()


def fresh_graph(name: str) -> FrameGraph:
    return FAMILY[name][0]()


def is_deep(g: FrameGraph) -> bool:
    """csrc/agg.hip, segsum(): the launch shape of the CSR kernel."""
    return 2 * g.E > 24 * g.Dn


def pass_width(H: int, deep: bool) -> int:
    """Incidences of one det that one pass of k_segsum_pipe covers: 256 / H lane groups of a wave, U rows in flight each."""
    return (256 // H) * (8 if deep else 4)


def passes(degree: int, H: int, deep: bool) -> int:
    """Passes over a CSR run (an empty run still takes one: it writes the zeros)."""
    P = pass_width(H, deep)
    return max(1, -(-degree // P))


def degrees(g: FrameGraph) -> Tuple[torch.Tensor, torch.Tensor]:
    """(edges a det is the src of, edges it is the dst of), per det index, from src / dst alone."""
    det_of = torch.full((g.N,), -1, dtype=torch.long)
    det_of[g.det_row.long()] = torch.arange(g.Dn)
    s = torch.bincount(det_of[g.src.long()], minlength=g.Dn) if g.E else torch.zeros(g.Dn, dtype=torch.long)
    d = torch.bincount(det_of[g.dst.long()], minlength=g.Dn) if g.E else torch.zeros(g.Dn, dtype=torch.long)
    return s, d


def degree_set(g: FrameGraph) -> Set[int]:
    s, d = degrees(g)
    return set((s + d).tolist())


def pass_edges(P: int) -> Set[int]:
    """The run lengths at which the pass bookkeeping of k_segsum_pipe (`last`, pbC, the hand-over to the next det) can go wrong."""
    return {0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1}


# ---- float64 definitions (include/tmpnn.h, rows E and F) ---------------------------------------------------------------------
def _limited(x: torch.Tensor, row_limit: Optional[int]) -> torch.Tensor:
    x = x.double()
    if row_limit is not None and row_limit < x.shape[0]:
        x = x.clone()
        x[max(row_limit, 0):] = 0
    return x


def ref_segsum(g: FrameGraph, x: torch.Tensor, row_limit: Optional[int] = None) -> torch.Tensor:
    """[Dn, H]: out[d] = sum_{e: src = d} x[row e] - sum_{e: dst = d} x[row e]; input rows >= row_limit count as zero."""
    x = _limited(x, row_limit)
    xe = x[g.edge_row.long()]
    full = torch.zeros(g.N, x.shape[1], dtype=torch.float64)
    full.index_add_(0, g.src.long(), xe)
    full.index_add_(0, g.dst.long(), -xe)
    return full[g.det_row.long()]


def ref_concat_bwd(g: FrameGraph, x: torch.Tensor, row_limit: Optional[int] = None) -> torch.Tensor:
    """[Dn, H] from x [N, 2H]: out[d] = sum_{e: src = d} x[row e, 0:H] + sum_{e: dst = d} x[row e, H:2H]."""
    x = _limited(x, row_limit)
    H = x.shape[1] // 2
    xe = x[g.edge_row.long()]
    full = torch.zeros(g.N, H, dtype=torch.float64)
    full.index_add_(0, g.src.long(), xe[:, :H])
    full.index_add_(0, g.dst.long(), xe[:, H:])
    return full[g.det_row.long()]


def ref_gather_diff(g: FrameGraph, x: torch.Tensor) -> torch.Tensor:
    """[E, H]: out[e] = x[src[e]] - x[dst[e]]."""
    x = x.double()
    return x[g.src.long()] - x[g.dst.long()]


def ref_gather_concat(g: FrameGraph, x: torch.Tensor) -> torch.Tensor:
    """[E, 2H]: out[e] = [x[src[e]] | x[dst[e]]]."""
    x = x.double()
    return torch.cat([x[g.src.long()], x[g.dst.long()]], 1)


def segsum_abs(g: FrameGraph, x: torch.Tensor, concat: bool = False, row_limit: Optional[int] = None) -> torch.Tensor:
    """[Dn, H]: the sum of the ABSOLUTE addends of a det (what the rounding bound scales with)."""
    x = _limited(x, row_limit).abs()
    H = x.shape[1] // 2 if concat else x.shape[1]
    xe = x[g.edge_row.long()]
    full = torch.zeros(g.N, H, dtype=torch.float64)
    full.index_add_(0, g.src.long(), xe[:, :H])
    full.index_add_(0, g.dst.long(), xe[:, H:] if concat else xe)
    return full[g.det_row.long()]


def gamma(n: torch.Tensor) -> torch.Tensor:
    """gamma_n = n u / (1 - n u), u = 2^-24: an fp32 sum of n addends, in ANY order, is within gamma_n * sum |addends| of the exact
    one (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; gamma_{n-1} would do, n is what the tests use)."""
    nu = n.double() * U32
    return nu / (1.0 - nu)


def segsum_bound(g: FrameGraph, abs_sum: torch.Tensor, accumulate: bool) -> torch.Tensor:
    """[Dn, H]: gamma_n * sum |addends| with n = degree (+ 1 when accumulating; abs_sum then includes |previous value|)."""
    s, d = degrees(g)
    n = s + d + (1 if accumulate else 0)
    return gamma(n)[:, None] * abs_sum


def gather_bound(a: torch.Tensor, b: torch.Tensor, prev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """2 u (|a| + |b| + |p|): a - b rounded once, + p rounded once."""
    t = a.double().abs() + b.double().abs()
    if prev is not None:
        t = t + prev.double().abs()
    return 2.0 * U32 * t
