"""One TrackMPNN message-passing call (reference/models/track_mpnn.py:54-75) on the HIP kernels.

`mp_forward` / `mp_backward` sequence the C-ABI stages of include/tmpnn.h on the current HIP
stream; `MPIteration` wraps them in a torch.autograd.Function so that the carried hidden state
`h_in` (BPTT over a chunk, reference/train.py:104-107,132-135), the new-row features `x` and every
parameter receive gradients exactly as in the reference.  torch is used for memory, streams and
index plumbing only -- every flop of the path runs in libtmpnn.so, and there is no fallback.

Which kernels a call runs is decided once, by `plan_route` (a `CallRoute`), before its first launch; the forward hands
the route to the backward inside `SavedCall`.  Each stage is one function that issues its launches and takes the route:
forward -- state append, input transform, edge cell, aggregation (segment sum or attention), node cell, heads;
backward -- heads, node cell, edge cell (one-pass: full rows + zero-state rows; else the wide forms or the two generic
kernels), attention, message adjoint, input transform.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .graph import CallPlan, dense_seg_plan, edge_tiles, win_plan

ATT_DROPOUT_P = 0.5
# OPT-IN fast path: accumulate parameter gradients straight into existing p.grad buffers (the kernels add into their
# outputs) instead of returning per-call tensors for autograd to add: saves a zero-fill and ~20 small add kernels per
# call.  It bypasses autograd's bookkeeping for the parameters (autograd receives None), so it is only valid for a
# plain `loss.backward()` with no parameter hooks, no DistributedDataParallel wrapper and no torch.autograd.grad();
# `GradBucket(model)` (trackmpnn_amd.dist) turns it on for its module (`module.inplace_param_grads = True`), the
# environment variable TMPNN_INPLACE_GRADS=1 for every module.  Default: off -- real gradients are returned.
INPLACE_GRADS = os.environ.get('TMPNN_INPLACE_GRADS', '0') == '1'
FUSED_BWD = os.environ.get('TMPNN_FUSED_BWD', '1') == '1'     # one-pass cell backward (see mp_backward); its A/B is a test
# the one-pass edge backward of a call's NEW edge rows (zero incoming state) on its own kernel (see mp_backward);
# TMPNN_BWD_ZERO_STATE=0 runs every edge row through the full kernel
ZERO_STATE_BWD = os.environ.get('TMPNN_BWD_ZERO_STATE', '1') != '0'
# the tiled edge forward of a call's NEW edge rows on its state-free kernel (see mp_forward); TMPNN_FWD_ZERO_STATE=0 runs
# every edge row through the full kernel (and zero-fills the new rows of the state for it)
ZERO_STATE_FWD = os.environ.get('TMPNN_FWD_ZERO_STATE', '1') != '0'
# wide cells: the det-side branch of the backward on a second stream next to the E-row matrix kernels (tmpnn_wide_gru_bwd_diff_aux)
# (det-side branches of the wide cells on a second stream: worth 1.5-6 ms of a 195-ms C5 step until round 4's single-read segment sum
#  took most of what it hid -- since then the two forms are within the run-to-run spread (4 alternating pairs: 186.8 vs 188.5 ms, a
#  later pair 184.7 vs 183.4); off by default: the simpler form)
WIDE_OVERLAP = os.environ.get('TMPNN_WIDE_OVERLAP', '0') == '1' and os.environ.get('TMPNN_KEEP_VARIANTS', '0') == '1'   # (tmpnn_wide_gru_bwd_diff_aux: comparison builds)
ATT_KMAX = 8                 # heads per tmpnn_att_fwd / _bwd call (include/tmpnn.h)
_SPLIT = os.environ.get('TMPNN_SPLIT', '1')[:1] != '0'        # TMPNN_SPLIT=0: every GEMM on the f32-input MFMA (tested)

# Switches whose A/B has been run and lost (DESIGN sections 4, 11): they are constants of a normal process and only read from the
# environment when TMPNN_KEEP_VARIANTS=1 (the Python side of the -DTMPNN_KEEP_VARIANTS build flag; tools/ set it for comparisons).
_VARIANTS = os.environ.get('TMPNN_KEEP_VARIANTS', '0') == '1'


def _variant(name: str, default: str) -> str:
    return os.environ.get(name, default) if _VARIANTS else default


WIDE_DW = _variant('TMPNN_WIDE_DW', '1') == '1'              # wide cells: dW from the materialised gate gradients
# wide cells: both W_ih products of the backward on the DET side (linearity of the diff message, tmpnn_wide_gru_bwd_diff);
# TMPNN_WIDE_DET=0 keeps the per-edge products (tmpnn_wide_gru_bwd_data + _weights + the message adjoint's segment sum)
WIDE_DET = _variant('TMPNN_WIDE_DET', '1') == '1'
# H = 128 / 256 edge cells as LDS-tiled bf16x6 GEMMs (csrc/wide.hip); TMPNN_WIDE=0 keeps round 1's f32-MFMA kernels
WIDE = _variant('TMPNN_WIDE', '1') != '0' and _SPLIT
# wide cells: forward over edge tiles (projected det rows staged in LDS); TMPNN_WIDE_TILED=0 keeps the per-row gathers
WIDE_TILED = _variant('TMPNN_WIDE_TILED', '1') != '0'
# H <= 64 edge cells: forward over 32-row edge tiles (projected det rows staged in LDS an item ahead); TMPNN_FWD_TILED=0
# keeps the per-row gathers of tmpnn_gru_fwd (xmode 3)
FWD_TILED = _variant('TMPNN_FWD_TILED', '1') != '0' and _SPLIT
# rows per edge tile of the H <= 64 forward: 32 (k_gru_fwd_split_tiled, the default) or 16 (k_gru_fwd_split_t16, sixteen waves
# per CU, stores straight from the accumulators: measured 7 % slower with the gate planes, 5 % faster without)
FWD_TILE_ROWS = 16 if _variant('TMPNN_FWD_TILE_ROWS', '32') == '16' else 32
# input transform in one launch per direction where every window adds few det rows (csrc/intf.hip); TMPNN_INPUT_TF=0 keeps
# the staged launches of tmpnn_input_bn_*
INPUT_TF = _variant('TMPNN_INPUT_TF', '1') != '0'
# Experiment ("save h only"): the H <= 64 edge cell's forward does not write its four gate planes; the
# backward runs the forward kernel again into the gate planes (and a scratch state) right before the one-pass backward
# reads them.  Same gradients bit for bit; measured SLOWER (numbers in DESIGN), so off by default.
RECOMPUTE_GATES = _variant('TMPNN_RECOMPUTE_GATES', '0') == '1'
CONCAT_PROJ = _variant('TMPNN_CONCAT_PROJ', '1') != '0'
# a call's new (zero-state) edge rows: the forward saves NO gate planes for them and the zero-state backward forms r, z, n again
# from the call's projected det rows (no matrix product: see k_gru_bwd_zs<., true>); TMPNN_ZS_RECOMPUTE=0 keeps the planes
ZS_RECOMPUTE = _variant('TMPNN_ZS_RECOMPUTE', '1') != '0'
# the window-owned segment sum (csrc/agg.hip k_segsum_win) on graphs with window labels: bit-equal to the CSR kernel, 0.9 ms
# against its 0.43 ms per 6 M edges on MI355X -- kept opt-in
WIN_SEGSUM = _variant('TMPNN_SEGSUM_WIN', '0') == '1'
WIDE_FUSED_ADJOINT = _variant('TMPNN_WIDE_FUSED_ADJOINT', '1') != '0'
_aux_streams: Dict[torch.device, 'torch.cuda.Stream'] = {}


def _aux_stream(dev) -> Optional[int]:
    """Raw handle of this device's auxiliary stream, or None while the current stream is being captured (a forked stream
    inside a capture does not survive hipStreamEndCapture on this stack) or when the current stream is the auxiliary one."""
    if not WIDE_OVERLAP or torch.cuda.is_current_stream_capturing():
        return None
    key = torch.device(dev)
    s = _aux_streams.get(key)
    if s is None:
        s = torch.cuda.Stream(key)
        _aux_streams[key] = s
    if s.cuda_stream == torch.cuda.current_stream(key).cuda_stream:
        return None
    return s.cuda_stream


def _seg_plan_guard(g, dev, on_aux: bool) -> None:
    """The dense segment sum's partial-row buffer belongs to the graph's cached plan (struct tmpnn_seg_plan.ws): one segment sum
    at a time per plan.  Uses on ONE stream are ordered by the stream; when the stream changes (main <-> auxiliary, or a
    caller that moves the graph to another stream) the new stream first waits for everything the previous user's stream
    has been given so far."""
    plan = g.__dict__.get('_seg_plan')
    if plan is None or torch.cuda.is_current_stream_capturing():
        return
    cur = _aux_streams[torch.device(dev)] if on_aux else torch.cuda.current_stream(dev)
    last = plan.__dict__.get('_last_stream')
    if last is not None and last.cuda_stream != cur.cuda_stream:
        ev = torch.cuda.Event()
        ev.record(last)
        cur.wait_event(ev)
    plan._last_stream = cur


_aux_events: Dict[torch.device, tuple] = {}


def _aux_event_pair(dev):
    """The device's fork / join events for the two-stream forms (created once, under the device, and recorded once so that
    their native handles exist): the C entry points only record and wait on what the caller hands them."""
    key = torch.device(dev)
    ev = _aux_events.get(key)
    if ev is None:
        with torch.cuda.device(key):
            ev = (torch.cuda.Event(enable_timing=False), torch.cuda.Event(enable_timing=False))
            for e in ev:
                e.record(torch.cuda.current_stream(key))
        _aux_events[key] = ev
    return ev


_wide_ws: Dict[torch.device, torch.Tensor] = {}


def _wide_workspace(nbytes: int, dev, slot: int = 0) -> torch.Tensor:
    """The materialised gate gradients of a wide cell's backward (24 H bytes per row: 27 GB at C5) live in ONE
    grow-only buffer per device, reused by every call (all users are ordered on the stream): handing tens of GB back
    and forth through the caching allocator cost up to 200 ms per C5 step in allocator stalls."""
    key = (torch.device(dev), slot)           # slot 0: gate gradients; slot 1: the weight-gradient slabs that read them
    ws = _wide_ws.get(key)
    if ws is None or ws.numel() * 4 < nbytes + 16:
        _wide_ws.pop(key, None)
        ws = torch.empty((nbytes // 4 + 4,), dtype=torch.float32, device=dev)
        _wide_ws[key] = ws
    return ws


_weight_images = None      # inside weight_cache(): {key: (source tensors kept alive, derived tensor)}


@contextlib.contextmanager
def weight_cache():
    """Within the context a weight's derived images (the transposes, the wide cells' MFMA operand images) are built once
    per source tensor instead of once per forward call -- for callers that KNOW the weights do not change inside: the
    forward calls of one training step (CapturedWindow: 4-6 launches less per call of a window).  Nothing outlives the
    context, so nothing can go stale; outside it every forward call rebuilds them."""
    global _weight_images
    prev = _weight_images
    _weight_images = {}
    try:
        yield
    finally:
        _weight_images = prev


def _cached(key, sources, build):
    if _weight_images is None:
        return build()
    hit = _weight_images.get(key)
    if hit is None:                                  # (the sources stay referenced: their addresses cannot be reused)
        hit = _weight_images[key] = (sources, build())
    return hit[1]


def _wide_prep(w_ih: torch.Tensor, w_hh: torch.Tensor, H: int) -> torch.Tensor:
    """MFMA operand images of one wide cell's weights (tmpnn_wide_prepare: four small launches).  Rebuilt on every
    forward call -- microseconds next to a wide cell's work, and never stale (weight_cache() narrows that to once per
    context); the backward reuses the call's images."""
    def build():
        nb = int(_lib.load().tmpnn_wide_prep_bytes(H, H))
        prep = torch.empty((nb // 4 + 4,), dtype=torch.float32, device=w_ih.device)
        _lib.call('tmpnn_wide_prepare', w_ih.data_ptr(), w_hh.data_ptr(), H, H, prep.data_ptr(), _stream())
        return prep
    return _cached(('wide', w_ih.data_ptr(), w_hh.data_ptr(), H), (w_ih, w_hh), build)


@dataclass(frozen=True)
class ModelSpec:
    groups: Tuple[Tuple[str, int], ...]   # (name, F_g)
    H: int
    K: int
    msg_type: str

    @property
    def G(self) -> int:
        return len(self.groups)

    @property
    def IN_e(self) -> int:
        return 2 * self.H if self.msg_type == 'concat' else self.H

    @property
    def F_total(self) -> int:
        return sum(f for _, f in self.groups)

    def param_names(self) -> List[str]:
        """state_dict names of every nn.Parameter, in the order MPIteration takes them."""
        names = []
        for g in range(self.G):
            t = f'input_transforms.{g}.'
            names += [t + '0.weight', t + '0.bias', t + '1.weight', t + '1.bias', t + '3.weight', t + '3.bias']
        for g in range(self.G):
            f = f'factor_grus.{g}.'
            names += [f + 'edge_gru.weight_ih', f + 'edge_gru.weight_hh', f + 'edge_gru.bias_ih', f + 'edge_gru.bias_hh']
            for k in range(self.K):
                names += [f + f'gat.{k}.W_att', f + f'gat.{k}.a']
            names += [f + 'node_gru.weight_ih', f + 'node_gru.weight_hh', f + 'node_gru.bias_ih', f + 'node_gru.bias_hh']
        names += ['output_transform_node.weight', 'output_transform_node.bias',
                  'output_transform_edge.weight', 'output_transform_edge.bias']
        return names


def _stream() -> int:
    return _lib.raw_stream()


def _keep_bits(keep, K: int, n: int, dev) -> torch.Tensor:
    """The attention dropout mask as the kernels take it: uint8 [n], bit k set = head k keeps the position.  `keep` None:
    drawn here (p = 0.5: every bit of a uniform byte is an independent fair coin -- one launch for all heads); else a
    [K, n] mask (the reference's drawn mask in the parity tests) packed."""
    n = max(n, 1)
    if keep is None:
        if ATT_DROPOUT_P == 0.5:
            return torch.empty((n,), dtype=torch.uint8, device=dev).random_(0, 1 << K)
        keep = torch.empty((K, n), dtype=torch.uint8, device=dev).bernoulli_(1.0 - ATT_DROPOUT_P)
    keep = (keep != 0).to(torch.uint8)
    bits = keep[0].clone()
    for k in range(1, K):
        bits |= keep[k] << k
    return bits.contiguous()


def _require_device(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f'{what} is on {t.device}: trackmpnn_amd runs on the MI355X HIP kernels only '
                           '(no CPU or torch fallback exists)')


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _transpose(w: torch.Tensor) -> torch.Tensor:
    def build():
        out = torch.empty((w.shape[1], w.shape[0]), dtype=torch.float32, device=w.device)
        _lib.call('tmpnn_transpose', w.data_ptr(), w.shape[0], w.shape[1], out.data_ptr(), _stream())
        return out
    return _cached(('t', w.data_ptr(), w.shape[0], w.shape[1]), (w,), build)


@dataclass(frozen=True)
class CallRoute:
    """Which kernels one message-passing call runs, forward and backward: filled once by plan_route() before the call's
    first launch.  The forward leaves unwritten what the routed backward does not read (of the call's new edge rows: the
    state rows, the hn plane and, with zs_rc, the gate slots), so mp_backward follows the route of its forward and never
    decides again -- a switch that changes between the two has no effect on that call."""
    n: int                           # the call's new rows
    E_old: int                       # the edge rows [E_old, E) are new: they enter the edge cell with h = 0
    save: bool                       # a backward follows
    # edge cell, forward: 'wide_tiled' | 'wide_rows' (H >= 128), 'concat_proj' (stacked projection), 'proj_tiled' |
    # 'proj_rows' (diff message through the projected det rows; rows: tmpnn_gru_fwd xmode 3), 'generic'
    edge_fwd: str
    tile_rows: int                   # rows per edge tile of the H <= 64 tiled forward
    agg: str                         # edge -> node aggregation: 'segsum' | 'attention' (K > 0 heads)
    zs_fwd: bool                     # the new edge rows on the state-free forward kernel
    zs_bwd: bool                     # ... and on the zero-state backward kernel (in the groups of zs_groups)
    zs_groups: Tuple[bool, ...]      # per feature group: zs_bwd and the group's b_hn is 16-byte aligned
    zs_rc: bool                      # no gate planes for those rows: the backward forms r, z, n from the projected det rows
    recompute_gates: bool            # no gate planes for any edge row: the backward runs the forward kernel again
    cw: int                          # partial head sums per group from the cells' epilogues (0: tmpnn_heads_fwd)
    tf: Tuple[bool, ...]             # per feature group: the one-launch input transform
    tf_all: bool                     # ... for every group: x is read through the row list, no gather
    dense_plan: bool                 # build the dense segment-sum plan of the graph
    win_plan: bool                   # build the window segment-sum plan of the graph
    bwd_fused: bool                  # one-pass cell backward (else the data and the weight kernel)
    # edge cell, backward: 'fused', 'wide_det_fused' | 'wide_det' (det-side products; 'wide_det' goes to the auxiliary
    # stream when _aux_stream() gives one at launch), 'wide_data_dw' | 'wide_data' (per-edge products, dW from the gate
    # gradients | the generic weight kernel), 'generic'; '' without a backward
    edge_bwd: str
    gather_bwd: bool                 # the message adjoint runs as its own launch (the det-side wide forms contain it)

    @property
    def wide(self) -> bool:
        return self.edge_fwd in ('wide_tiled', 'wide_rows')

    @property
    def new_rows_unread(self) -> bool:
        """No kernel reads the state rows or the hn plane of the call's new edge rows: the forward neither zero-fills
        nor writes them."""
        return self.zs_fwd and (self.zs_bwd or not self.save)


def _input_tf(plan: CallPlan, H: int, F: int, caps) -> bool:
    """The one-launch input transform serves plans whose windows each add at most 128 det rows (H in {32, 64})."""
    return (INPUT_TF and plan.max_seg_nd >= 0 and plan.seg_of_det is not None
            and bool(caps.tmpnn_input_tf_supported(H, F, plan.max_seg_nd)))


def plan_route(spec: ModelSpec, plan: CallPlan, P: Dict[str, torch.Tensor], save: bool, caps=None) -> CallRoute:
    """The route of one call.  Pure: reads the module's switches as they stand now, the plan's host-side fields and the
    parameters' addresses, and asks `caps` what the library can run (default: the loaded library; anything with the six
    tmpnn_*_available / _supported / _head_parts functions serves, so plans on the CPU can be routed)."""
    if caps is None:
        caps = _lib.load()
    g = plan.graph
    H, G, K, IN_e = spec.H, spec.G, spec.K, spec.IN_e
    E, Dn, n = g.E, g.Dn, plan.n_new
    diff = spec.msg_type == 'diff'
    xmode = 1 if diff else 2
    has_pos = g.src_pos is not None and Dn > 0
    nd = int(plan.new_det_row.numel()) if n > 0 else 0
    # A call's new edge rows enter the edge cell with h = 0 and form the suffix [E_old, E) of the ascending edge list (E_old
    # from the plan: the call's new rows less its new det rows, never from the device).
    E_old = E - (n - nd) if n > 0 else E
    if WIDE and diff and H >= 128 and bool(caps.tmpnn_wide_supported(H, H)) and has_pos and E > 0:
        edge_fwd = 'wide_tiled' if WIDE_TILED else 'wide_rows'
    elif CONCAT_PROJ and not diff and H <= 64 and FWD_TILED and has_pos and E > 0:
        edge_fwd = 'concat_proj'
    elif diff and H <= 64 and has_pos:
        edge_fwd = 'proj_tiled' if FWD_TILED and E > 0 else 'proj_rows'
    else:
        edge_fwd = 'generic'
    recompute = edge_fwd == 'proj_tiled' and RECOMPUTE_GATES and save
    # The forward runs the new edge rows on the state-free kernel, and the backward takes its zero-state kernel on exactly
    # those rows when zs_bwd (with both, the forward does not write their hn plane, nor zero-fill their state rows: no
    # kernel reads them).  zs_bwd does not need zs_fwd: the zero-state backward also runs on planes the full forward saved.
    zs_rows = n > 0 and K == 0 and diff and 0 <= E_old < E
    aligned = (tuple((P[f'factor_grus.{gi}.edge_gru.bias_hh'].data_ptr() + 4 * 2 * H) % 16 == 0 for gi in range(G))
               if zs_rows else (False,) * G)
    zs_fwd = (ZERO_STATE_FWD and zs_rows and edge_fwd == 'proj_tiled' and H == 64 and FWD_TILE_ROWS == 32
              and not RECOMPUTE_GATES and all(aligned) and bool(caps.tmpnn_gru_fwd_tiles_zero_state_available(H, 3)))
    # The one-pass backward (tmpnn_gru_bwd_fused: H = 64, K-independent) reads dh, the gates and h ONCE for the data
    # and the weight gradient: 2.39 vs 2.85 ms per 3 M edge rows for the two stand-alone kernels, 35.3 vs 37.9 ms per
    # C2 step (round 2).  TMPNN_FUSED_BWD=0 keeps the two kernels.
    bwd_fused = bool(save and FUSED_BWD and caps.tmpnn_gru_bwd_fused_available(H, H, 0)
                     and caps.tmpnn_gru_bwd_fused_available(H, IN_e, xmode))
    zs_bwd = bool(bwd_fused and ZERO_STATE_BWD and zs_rows and not recompute and any(aligned)
                  and caps.tmpnn_gru_bwd_fused_zero_state_available(H, IN_e, xmode))
    # ... and whether that backward forms the rows' r, z, n itself (then their gate slots are allocated but never touched, and the
    # call's projected det rows are kept for it: 768 B per det row and feature group)
    zs_rc = zs_fwd and zs_bwd and ZS_RECOMPUTE
    proj_table = edge_fwd in ('concat_proj', 'proj_tiled', 'proj_rows')
    # output head fused into the cells' epilogues where the LDS-resident kernel runs (else tmpnn_heads_fwd)
    cw = min(caps.tmpnn_gru_fwd_head_parts(H, H if edge_fwd == 'concat_proj' else IN_e, 3 if proj_table else xmode),
             caps.tmpnn_gru_fwd_head_parts(H, H, 0))
    tf = tuple(_input_tf(plan, H, F, caps) for _, F in spec.groups) if n > 0 else (False,) * G
    wide = edge_fwd in ('wide_tiled', 'wide_rows')
    if not save:
        edge_bwd = ''
    elif bwd_fused:
        edge_bwd = 'fused'
    elif wide and WIDE_DET:
        edge_bwd = 'wide_det_fused' if K == 0 and WIDE_FUSED_ADJOINT else 'wide_det'
    elif wide:
        edge_bwd = 'wide_data_dw' if WIDE_DW else 'wide_data'
    else:
        edge_bwd = 'generic'
    return CallRoute(n=n, E_old=E_old, save=save, edge_fwd=edge_fwd, tile_rows=FWD_TILE_ROWS,
                     agg='attention' if K > 0 else 'segsum', zs_fwd=zs_fwd, zs_bwd=zs_bwd,
                     zs_groups=tuple(zs_bwd and a for a in aligned), zs_rc=zs_rc, recompute_gates=recompute, cw=cw,
                     tf=tf, tf_all=nd > 0 and all(tf), dense_plan=wide and H % 256 == 0 and K == 0,
                     win_plan=WIN_SEGSUM and H == 64 and E > 0, bwd_fused=bwd_fused, edge_bwd=edge_bwd,
                     gather_bwd=edge_bwd not in ('wide_det_fused', 'wide_det'))


@dataclass
class SavedCall:
    """What a forward call hands its backward: the route it took and the tensors that route's backward reads."""
    route: CallRoute
    h_cat: Optional[torch.Tensor] = None
    gates: Optional[torch.Tensor] = None
    es: Optional[torch.Tensor] = None
    h_out: Optional[torch.Tensor] = None
    scores: Optional[torch.Tensor] = None
    att: Optional[list] = None       # per feature group: the attention head groups' saves
    wide: Optional[list] = None      # per feature group: the wide cell's operand images
    proj: Optional[dict] = None      # group -> (projected det rows, W_hh^T) where zs_rc or recompute_gates needs them
    # input transform: the rows of x it read (+ the row list of the one-launch form) and, per group, its saves
    xdet: Optional[torch.Tensor] = None
    xrows: Optional[torch.Tensor] = None
    y_save: Optional[list] = None
    mean: Optional[list] = None
    rstd: Optional[list] = None


def _call_dims(spec: ModelSpec, plan: CallPlan, dev) -> SimpleNamespace:
    """The sizes and handles every stage of one call takes."""
    g = plan.graph
    return SimpleNamespace(spec=spec, plan=plan, g=g, H=spec.H, G=spec.G, K=spec.K, GH=spec.G * spec.H, IN_e=spec.IN_e,
                           N=g.N, E=g.E, Dn=g.Dn, n=plan.n_new, N_old=g.N - plan.n_new, plane=g.N * spec.H,
                           xmode=2 if spec.msg_type == 'concat' else 1, dev=dev, st=_stream(),
                           opts=dict(dtype=torch.float32, device=dev))


_CELL = ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')


def _cell_ptrs(T: Dict[str, torch.Tensor], prefix: str) -> Tuple[int, int, int, int]:
    """(weight_ih, weight_hh, bias_ih, bias_hh) addresses of one GRU cell in T (the parameters, or their gradients)."""
    return tuple(T[prefix + s].data_ptr() for s in _CELL)


def _tf_head(tf: bool, plan: CallPlan, xg: int, xrows, Ft: int, F: int, nd: int, H: int) -> tuple:
    """The leading arguments of a feature group's input transform, either direction: tmpnn_input_tf_* (tf) reads x through
    a row list and takes the plan's largest segment, tmpnn_input_bn_* the gathered det rows."""
    segs = (plan.seg_ptr.data_ptr(), plan.seg_cnt.data_ptr(), _lib.ptr(plan.seg_of_det), plan.S)
    if tf:
        return (xg, _lib.ptr(xrows), Ft, F, nd, *segs, plan.max_seg_nd, H)
    return (xg, Ft, F, nd, *segs, H)


# ---- forward stages -------------------------------------------------------------------------------------------------

def _fwd_state(c, route: CallRoute, h_in: Optional[torch.Tensor], h_spare: int) -> torch.Tensor:
    """State append: the carried state with the call's n new rows behind it, in place where the previous call reserved room."""
    N, GH, n, N_old = c.N, c.GH, c.n, c.N_old
    h_cat = None
    if h_in is not None and N_old > 0 and n > 0 and h_in.is_contiguous():
        st_ = h_in.untyped_storage()
        if h_spare >= n and st_.nbytes() >= 4 * (h_in.storage_offset() + N * GH):
            h_cat = torch.empty(0, **c.opts).set_(st_, h_in.storage_offset(), (N, GH), (GH, 1))   # append in place
    if h_cat is None:
        if h_in is not None and n == 0:
            h_cat = h_in                               # pure extra iteration: nothing to append
        else:
            h_cat = torch.empty((N, GH), **c.opts)
            if N_old > 0:
                h_cat[:N_old].copy_(h_in)
    if n > 0 and not route.new_rows_unread:
        h_cat[N_old:].zero_()                   # new edge rows start at 0 (track_mpnn.py:61)
    return h_cat


def _fwd_input_transform(c, route: CallRoute, x, h_cat, P, buffers, training: bool, saved: SavedCall) -> None:
    """Input transform of the call's new det rows into their rows of h_cat (Linear, BatchNorm per window, ReLU, Linear)."""
    spec, plan, H, GH = c.spec, c.plan, c.H, c.GH
    nd = int(plan.new_det_row.numel())
    S = plan.S
    if training and plan.min_seg_cnt <= 1:
        # torch.nn.functional.batch_norm refuses a single row in training mode; so does the reference
        raise ValueError('Expected more than 1 value per channel when training, got input size '
                         f'[1, {H}]')
    # the det rows of x: gathered here for the staged transform; the one-launch transform reads x through the row list
    # (tmpnn_input_tf_*'s x_rows) -- no gather launch, no compact copy
    if route.tf_all:
        xsrc, xrows = _f32c(x.detach()), plan.new_det_local
        if xrows.dtype != torch.int64 or not xrows.is_contiguous():
            xrows = xrows.long().contiguous()
    else:
        xsrc = _f32c(x.detach().index_select(0, plan.new_det_local)) if nd > 0 else torch.empty((0, spec.F_total), **c.opts)
        xrows = None
    ws_a = torch.empty((max(nd, 1), H), **c.opts)
    y_saves, means, rstds = [], [], []
    f0 = 0
    for gi, (_, F) in enumerate(spec.groups):
        t = f'input_transforms.{gi}.'
        y_save = torch.empty((max(nd, 1), H), **c.opts)
        SS = S if training else 1
        mean = torch.empty((SS, H), **c.opts)
        rstd = torch.empty((SS, H), **c.opts)
        tf = route.tf[gi]
        args = (*_tf_head(tf, plan, xsrc.data_ptr() + 4 * f0, xrows, spec.F_total, F, nd, H), int(training),
                P[t + '0.weight'].data_ptr(), P[t + '0.bias'].data_ptr(), P[t + '1.weight'].data_ptr(), P[t + '1.bias'].data_ptr(),
                buffers[t + '1.running_mean'].data_ptr(), buffers[t + '1.running_var'].data_ptr(),
                P[t + '3.weight'].data_ptr(), P[t + '3.bias'].data_ptr(), y_save.data_ptr(), mean.data_ptr(), rstd.data_ptr())
        if not tf:
            args += (ws_a.data_ptr(),)
        _lib.call('tmpnn_input_tf_fwd' if tf else 'tmpnn_input_bn_fwd', *args,
                  plan.new_det_row.data_ptr(), h_cat.data_ptr() + 4 * gi * H, GH, c.st)
        if training:
            buffers[t + '1.num_batches_tracked'] += S
        y_saves.append(y_save)
        means.append(mean)
        rstds.append(rstd)
        f0 += F
    if route.save:
        saved.xdet, saved.xrows, saved.y_save, saved.mean, saved.rstd = xsrc, xrows, y_saves, means, rstds


def _fwd_group(c, route: CallRoute, gi: int, P, h_cat, h_out, gates, parts) -> SimpleNamespace:
    """A feature group's pointers for the forward stages (and its transposed weights: four launches, unless cached)."""
    f = f'factor_grus.{gi}.'
    H, cw = c.H, route.cw
    e_wih, e_whh = P[f + 'edge_gru.weight_ih'], P[f + 'edge_gru.weight_hh']
    q = SimpleNamespace(gi=gi, f=f, e_wih=e_wih, e_whh=e_whh,
                        hg=h_cat.data_ptr() + 4 * gi * H, og=h_out.data_ptr() + 4 * gi * H,
                        gp=gates[gi].data_ptr() if gates is not None else None,
                        part=(parts.data_ptr() + 4 * gi * cw * c.N) if cw > 0 else None,
                        we=(P['output_transform_edge.weight'].data_ptr() + 4 * gi * H) if cw > 0 else None,
                        wn=(P['output_transform_node.weight'].data_ptr() + 4 * gi * H) if cw > 0 else None,
                        e_bih=P[f + 'edge_gru.bias_ih'].data_ptr(), e_bhh=P[f + 'edge_gru.bias_hh'].data_ptr(),
                        n_bih=P[f + 'node_gru.bias_ih'].data_ptr(), n_bhh=P[f + 'node_gru.bias_hh'].data_ptr())
    # (temporaries stay referenced until their consumer is enqueued: the caching allocator may
    #  hand a freed block to the very next allocation)
    q.e_wih_t, q.e_whh_t = _transpose(e_wih), _transpose(e_whh)
    q.n_wih_t, q.n_whh_t = _transpose(P[f + 'node_gru.weight_ih']), _transpose(P[f + 'node_gru.weight_hh'])
    return q


def _fwd_edge_wide(c, route: CallRoute, q, saved: SavedCall):
    """H = 128 / 256: LDS-tiled bf16x6 GEMMs, the diff message through the projected det rows (csrc/wide.hip)."""
    g, H, GH, E, Dn = c.g, c.H, c.GH, c.E, c.Dn
    prep = _wide_prep(q.e_wih, q.e_whh, H)
    if route.save:
        saved.wide.append(prep)
    proj = torch.empty((Dn, 3 * H), **c.opts)
    if route.edge_fwd == 'wide_tiled':
        _lib.call('tmpnn_wide_gru_fwd_tiled', prep.data_ptr(), g.det_row.data_ptr(), Dn, edge_tiles(g, 128).cref(), E,
                  q.hg, GH, H, q.e_bih, q.e_bhh, proj.data_ptr(), q.og, GH, q.gp, c.plane, c.st)
    else:
        _lib.call('tmpnn_wide_gru_fwd', prep.data_ptr(), g.det_row.data_ptr(), Dn, g.edge_row.data_ptr(), E,
                  g.src_pos.data_ptr(), g.dst_pos.data_ptr(), q.hg, GH, H, q.e_bih, q.e_bhh,
                  proj.data_ptr(), q.og, GH, q.gp, c.plane, c.st)
    return prep, proj


def _fwd_edge_tiles(c, route: CallRoute, q, proj, saved: SavedCall) -> None:
    """The tiled H <= 64 forward over the projected det rows: the rows with a state on the full kernel, the call's new rows
    on the state-free one (zs_fwd)."""
    g, H, GH, E, E_old = c.g, c.H, c.GH, c.E, route.E_old
    E_full = E_old if route.zs_fwd else E
    if E_full > 0:
        tiles = edge_tiles(g, route.tile_rows, e1=E_full)
        _lib.call('tmpnn_gru_fwd_tiles', tiles.cref(), E_full, proj.data_ptr(), 3 * H, q.hg, GH, H,
                  q.e_whh_t.data_ptr(), q.e_bih, q.e_bhh,
                  q.og, GH, None if route.recompute_gates else q.gp, c.plane, q.we, q.part, c.N, c.st)
    if route.zs_fwd:
        _lib.call('tmpnn_gru_fwd_tiles_zero_state', edge_tiles(g, route.tile_rows, e0=E_old).cref(), E - E_old,
                  proj.data_ptr(), 3 * H, H, q.e_bih,
                  q.e_bhh, q.og, GH, None if route.zs_rc else q.gp, c.plane,
                  int(route.save and not route.zs_bwd), q.we, q.part, c.N, c.st)
    if route.zs_rc or route.recompute_gates:
        saved.proj[q.gi] = (proj, q.e_whh_t if route.recompute_gates else None)


def _fwd_edge_cell(c, route: CallRoute, q, saved: SavedCall):
    """Edge cell: GRU(h[src]-h[dst] | concat, h[e])      (layers.py:90-97).  Returns the temporaries its launches read."""
    g, H, GH, E, Dn, st = c.g, c.H, c.GH, c.E, c.Dn, c.st
    arm = route.edge_fwd
    if route.wide:
        return _fwd_edge_wide(c, route, q, saved)
    if arm == 'generic':
        _lib.call('tmpnn_gru_fwd', g.edge_row.data_ptr(), E, c.xmode, g.src.data_ptr(), g.dst.data_ptr(),
                  None, 0, 0, c.IN_e, q.hg, GH, H,
                  q.e_wih_t.data_ptr(), q.e_whh_t.data_ptr(), q.e_bih, q.e_bhh,
                  q.og, GH, q.gp, c.plane, q.we, q.part, c.N, st)
        return None
    # (h[src]-h[dst]) W_ih^T = P[src] - P[dst] with P = h[dets] W_ih^T: the x-half of the edge cell's
    # forward GEMM runs over the Dn det rows instead of the E edge rows
    # concat: [h_src | h_dst] W_ih^T = P1[src] + P2[dst] -- the same tiled kernel on a stacked table [P1; -P2] and tile lists
    # whose dst entries are offset by Dn (TMPNN_CONCAT_PROJ=0 keeps the per-edge GEMM over IN = 2H)
    proj = torch.empty(((2 if arm == 'concat_proj' else 1) * Dn, 3 * H), **c.opts)
    _lib.call('tmpnn_rows_linear', g.det_row.data_ptr(), Dn, q.hg, GH, H, q.e_wih_t.data_ptr(), 3 * H,
              proj.data_ptr(), 3 * H, st)
    if arm == 'concat_proj':
        # (the kernel forms P[src] - P[dst]: the dst half of the table is projected with -W2^T -- negating H x 3H weights
        #  instead of Dn x 3H projected rows)
        e_wih_t = q.e_wih_t
        w2n = _cached(('negt', e_wih_t.data_ptr(), H), (e_wih_t,), lambda: e_wih_t[H:].neg().contiguous())
        _lib.call('tmpnn_rows_linear', g.det_row.data_ptr(), Dn, q.hg, GH, H, w2n.data_ptr(), 3 * H,
                  proj.data_ptr() + 4 * Dn * 3 * H, 3 * H, st)
        _lib.call('tmpnn_gru_fwd_tiles', edge_tiles(g, route.tile_rows, dst_offset=Dn).cref(), E, proj.data_ptr(), 3 * H, q.hg, GH,
                  H, q.e_whh_t.data_ptr(), q.e_bih, q.e_bhh,
                  q.og, GH, q.gp, c.plane, q.we, q.part, c.N, st)
        return proj, w2n
    if arm == 'proj_tiled':
        _fwd_edge_tiles(c, route, q, proj, saved)
    else:
        _lib.call('tmpnn_gru_fwd', g.edge_row.data_ptr(), E, 3, g.src_pos.data_ptr(), g.dst_pos.data_ptr(),
                  proj.data_ptr(), 3 * H, 0, H, q.hg, GH, H, None, q.e_whh_t.data_ptr(), q.e_bih, q.e_bhh,
                  q.og, GH, q.gp, c.plane, q.we, q.part, c.N, st)
    return proj


def _fwd_attention(c, q, es, P, training: bool, keep):
    """Attention aggregation of one feature group into es.  Returns (the heads' alphas, the head groups' saves)."""
    g, H, GH, E, Dn, K, opts = c.g, c.H, c.GH, c.E, c.Dn, c.K, c.opts
    # the kernels take up to ATT_KMAX heads per call (all of them from one read of h[e]); more heads run in groups whose
    # means are combined with their share K_g / K (reference: any number of heads, utils/training_options.py:23)
    erec, inc_other = g.att_index() if E > 0 else (None, None)
    groups, al = [], []
    for k0 in range(0, K, ATT_KMAX):
        Kg = min(ATT_KMAX, K - k0)
        Ws = [P[q.f + f'gat.{k}.W_att'] for k in range(k0, k0 + Kg)]
        As = [P[q.f + f'gat.{k}.a'] for k in range(k0, k0 + Kg)]
        # (the heads' weights side by side for the kernels: one copy per call, or per weight_cache() context)
        W = _cached(('attW', tuple(t.data_ptr() for t in Ws)), tuple(Ws), lambda: torch.cat(Ws, 1).contiguous())
        a = _cached(('atta', tuple(t.data_ptr() for t in As)), tuple(As),
                    lambda: torch.stack([t.reshape(-1) for t in As]).contiguous())
        ws_ha = torch.empty((max(Dn, 1), Kg * H), **opts)
        score = torch.empty((max(2 * E, 1), Kg), **opts)  # (k_att_score writes both CSR positions of every edge)
        stats = torch.empty((max(Dn, 1), Kg, 2), **opts)
        esk = torch.empty((Kg, max(Dn, 1), H), **opts)
        alpha = torch.empty((Kg, max(2 * E, 1)), **opts)
        kp = None
        if training:
            kp = _keep_bits(None if keep is None else keep[q.gi][k0:k0 + Kg], Kg, 2 * E, c.dev)
        out_g = es if Kg == K else torch.empty_like(es)
        _lib.call('tmpnn_att_fwd', g.cref(), _lib.ptr(erec), q.hg, GH, H, Kg, W.data_ptr(),
                  a.data_ptr(), _lib.ptr(kp), ATT_DROPOUT_P, ws_ha.data_ptr(), score.data_ptr(), stats.data_ptr(),
                  esk.data_ptr(), alpha.data_ptr(), out_g.data_ptr(), H, c.st)
        if Kg != K:
            if k0 == 0:
                torch.mul(out_g, Kg / K, out=es)
            else:
                es.add_(out_g, alpha=Kg / K)
        al += [alpha[k, :2 * E] for k in range(Kg)]
        groups.append((k0, Kg, W, a, kp, ws_ha, score, stats, esk))
    return al, groups


def _fwd_aggregate(c, route: CallRoute, q, es, P, training: bool, keep, zero_from: int, st_det, on_aux: bool, saved):
    """Edge -> node aggregation into es (layers.py:99-112): segment sum, or attention heads.  Returns the heads' alphas | None."""
    if route.agg == 'segsum':
        _seg_plan_guard(c.g, c.dev, on_aux)
        # (the call's new edge rows are 0 and are not read: rows >= N_old -- h_cat[N_old:] was just zero-filled and only
        #  its det rows written; without new rows every row is read)
        _lib.call('tmpnn_segsum_fwd_live', c.g.cref(), q.hg, c.GH, es.data_ptr(), c.H, c.H, 1, zero_from, st_det)
        return None
    al, groups = _fwd_attention(c, q, es, P, training, keep)
    if route.save:
        saved.att.append(groups)
    return al


def _fwd_node_cell(c, q, es, st_det) -> None:
    """Node cell: GRU(es, h[d])                            (layers.py:114)."""
    _lib.call('tmpnn_gru_fwd', c.g.det_row.data_ptr(), c.Dn, 0, None, None,
              es.data_ptr(), c.H, 1, c.H, q.hg, c.GH, c.H,
              q.n_wih_t.data_ptr(), q.n_whh_t.data_ptr(), q.n_bih, q.n_bhh,
              q.og, c.GH, q.gp, c.plane, q.wn, q.part, c.N, st_det)


def _fwd_heads(c, route: CallRoute, P, parts, h_out):
    """Output heads (track_mpnn.py:72-75): finished from the cells' partial sums, or over h_out.  Returns (scores, logits)."""
    g, N, GH = c.g, c.N, c.GH
    logits = torch.empty((N, 1), **c.opts)
    scores = torch.empty((N, 1), **c.opts)
    if route.cw > 0:
        _lib.call('tmpnn_heads_finish', parts.data_ptr(), N, c.G * route.cw, N, g.is_edge.data_ptr(),
                  P['output_transform_node.bias'].data_ptr(), P['output_transform_edge.bias'].data_ptr(),
                  logits.data_ptr(), scores.data_ptr(), c.st)
    else:
        _lib.call('tmpnn_heads_fwd', h_out.data_ptr(), GH, GH, N, g.is_edge.data_ptr(),
                  P['output_transform_node.weight'].data_ptr(), P['output_transform_node.bias'].data_ptr(),
                  P['output_transform_edge.weight'].data_ptr(), P['output_transform_edge.bias'].data_ptr(),
                  logits.data_ptr(), scores.data_ptr(), c.st)
    return scores, logits


def _aux_fork(c):
    """Wide cells without attention: the det-side chain (row F, then the node cell: row movers + a Dn-row cell) goes to the
    auxiliary stream next to the edge cell's persistent matrix kernel -- both only read h_cat and write disjoint rows of
    h_out / the gate planes; nothing is allocated under the auxiliary stream.  Returns (stream of the det-side chain, the
    auxiliary stream to join | None): asked at launch time, the answer depends on capture state."""
    aux = _aux_stream(c.dev)
    if aux is None:
        return c.st, None
    aux_obj = _aux_streams[torch.device(c.dev)]
    fork, _ = _aux_event_pair(c.dev)
    fork.record(torch.cuda.current_stream(c.dev))
    aux_obj.wait_event(fork)
    return aux, aux_obj


def mp_forward(spec: ModelSpec, plan: CallPlan, x: torch.Tensor, h_in: Optional[torch.Tensor],
               P: Dict[str, torch.Tensor], buffers: Dict[str, torch.Tensor], training: bool, save: bool,
               keep: Optional[Sequence[torch.Tensor]] = None, reserve_rows: int = 0, h_spare: int = 0):
    """Returns (scores [N,1], logits [N,1], h_out [N,G*H], alphas, saved).

    reserve_rows > 0 allocates h_out with that many spare rows behind it; the NEXT call, when handed
    that h_out as h_in with n <= spare new rows, appends its new rows in place instead of copying
    the carried state (the caller promises to continue from a given h_out at most once).
    """
    c = _call_dims(spec, plan, x.device)
    g, H, G, K, GH, N, Dn, n, dev, st, opts = c.g, c.H, c.G, c.K, c.GH, c.N, c.Dn, c.n, c.dev, c.st, c.opts
    if h_in is None:
        if c.N_old != 0:
            raise ValueError(f'h_in is None but the graph has {c.N_old} rows that are not new')
    else:
        if h_in.shape[0] != c.N_old or h_in.shape[1] != GH:
            raise ValueError(f'h_in must be [{c.N_old}, {GH}] (N - n, G*H), got {tuple(h_in.shape)}')
    if x.shape[0] != n or (n > 0 and x.shape[1] != spec.F_total):
        raise ValueError(f'x must be [{n}, {spec.F_total}], got {tuple(x.shape)}')

    route = plan_route(spec, plan, P, save)
    saved = SavedCall(route, att=[], wide=[] if route.wide else None, proj={})
    h_cat = _fwd_state(c, route, h_in, h_spare)
    if n > 0:
        _fwd_input_transform(c, route, x, h_cat, P, buffers, training, saved)

    spare = max(int(reserve_rows), 0)
    if spare > 0:      # plain (non-view) tensor over a larger storage: the next call may extend it in place
        buf = torch.empty(((N + spare) * GH,), **opts)
        h_out = torch.empty(0, **opts).set_(buf.untyped_storage(), 0, (N, GH), (GH, 1))
    else:
        h_out = torch.empty((N, GH), **opts)
    gates = torch.empty((G, 4, N, H), **opts) if save else None
    es_all = torch.empty((G, max(Dn, 1), H), **opts)
    alphas: List[Optional[List[torch.Tensor]]] = []
    if route.dense_plan:
        # dense scenes: the plan of the single-read segment sum rides on the graph's C struct (tmpnn_segsum_fwd here and inside
        # the wide backward take it on 256-column blocks); None for ragged graphs
        dense_seg_plan(g)
    if route.win_plan:
        # batches of small windows (batch_windows): the plan of the window-owned segment sum rides on the graph's C struct
        # (None for graphs without window labels).  Opt-in: measured slower than the CSR kernel
        win_plan(g)
    # the call's new EDGE rows enter the state as zeros (h_cat[N_old:] zero-filled above unless no kernel reads those rows, only
    # det rows written since): the segment sum does not read them.  (Measured and dropped in round 6: the tiled edge forward skipping the 72 MFMAs of tiles
    # made of such rows -- bit-equal, 8.10 -> 8.09 ms per step: the matrix pipe is not what an item waits for.)
    zero_from = c.N_old if n > 0 else N
    parts = torch.empty((G * route.cw, N), **opts) if route.cw > 0 else None
    for gi in range(G):
        q = _fwd_group(c, route, gi, P, h_cat, h_out, gates, parts)
        st_det, aux_obj = _aux_fork(c) if route.wide and K == 0 else (st, None)
        held = _fwd_edge_cell(c, route, q, saved)      # (referenced until the group's launches are enqueued and joined)
        es = es_all[gi]
        alphas.append(_fwd_aggregate(c, route, q, es, P, training, keep, zero_from, st_det, aux_obj is not None, saved))
        _fwd_node_cell(c, q, es, st_det)
        if aux_obj is not None:
            _, join = _aux_event_pair(dev)
            join.record(aux_obj)
            torch.cuda.current_stream(dev).wait_event(join)
        del held
    scores, logits = _fwd_heads(c, route, P, parts, h_out)
    if save:
        saved.h_cat, saved.gates, saved.es, saved.h_out, saved.scores = h_cat, gates, es_all, h_out, scores
    return scores, logits, h_out, alphas, saved


# ---- backward stages ------------------------------------------------------------------------------------------------

def _bwd_grads(spec: ModelSpec, P, opts, grad_out) -> Dict[str, torch.Tensor]:
    """One zero-filled buffer for every parameter gradient of this call (the kernels accumulate with +=), or the caller's."""
    if grad_out is not None:
        return dict(grad_out)                  # caller-owned accumulators (p.grad): every kernel below adds into them
    names = spec.param_names()
    sizes = [P[nm].numel() for nm in names]
    offs = [0]
    for sz in sizes:
        offs.append(offs[-1] + ((sz + 63) // 64) * 64)          # 256-byte aligned slices
    flat = torch.zeros((offs[-1],), **opts)
    return {nm: flat[o:o + sz].view(P[nm].shape) for nm, o, sz in zip(names, offs, sizes)}


def _bwd_heads(c, saved: SavedCall, P, grads, d_scores, d_logits, d_hout):
    """Heads (track_mpnn.py:72-75): dy = d_logits + d_scores * s(1-s); its contribution dy * w_type to the
    gradient of h_out is folded into the GRU backward kernels (never materialised).  Returns (dy | None, dh_up | None)."""
    g, N, GH, opts = c.g, c.N, c.GH, c.opts
    lib = _lib.load()
    dh_up = _f32c(d_hout) if d_hout is not None else None
    dy = None
    if d_scores is not None or d_logits is not None:
        dy = torch.empty((N,), **opts)
        dl = _f32c(d_logits) if d_logits is not None else None
        ds = _f32c(d_scores) if d_scores is not None else None
        # (the kernel takes up to 1024 columns of h_out per call: wider states -- three feature groups above nhidden 256 --
        #  go in column slices; dy is the same in every slice, the two bias gradients are taken from the first)
        for c0 in range(0, GH, 1024):
            cw_ = min(1024, GH - c0)
            ws_b = lib.tmpnn_heads_bwd_ws(N, cw_)
            ws = torch.empty((max(ws_b // 4, 1),), **opts)
            db_n = grads['output_transform_node.bias'] if c0 == 0 else torch.zeros((1,), **opts)
            db_e = grads['output_transform_edge.bias'] if c0 == 0 else torch.zeros((1,), **opts)
            _lib.call('tmpnn_heads_bwd', saved.h_out.data_ptr() + 4 * c0, GH, cw_, N, g.is_edge.data_ptr(),
                      P['output_transform_node.weight'].data_ptr() + 4 * c0, P['output_transform_edge.weight'].data_ptr() + 4 * c0,
                      saved.scores.data_ptr(), _lib.ptr(dl), _lib.ptr(ds), dy.data_ptr(), None, 0, 0,
                      grads['output_transform_node.weight'].data_ptr() + 4 * c0, db_n.data_ptr(),
                      grads['output_transform_edge.weight'].data_ptr() + 4 * c0, db_e.data_ptr(),
                      ws.data_ptr(), ws_b, c.st)
    elif dh_up is None:
        dh_up = torch.zeros((N, GH), **opts)
    return dy, dh_up


def _bwd_group(c, gi: int, saved: SavedCall, P, grads, dy, dh_up, d_hcat, dmsg, ws_w) -> SimpleNamespace:
    """A feature group's pointers for the backward stages; e / n: the edge / node cell's (weight_ih, weight_hh, bias_ih,
    bias_hh), ge / gn: their gradients."""
    f = f'factor_grus.{gi}.'
    H = c.H
    return SimpleNamespace(gi=gi, f=f, hg=saved.h_cat.data_ptr() + 4 * gi * H,
                           dog=(dh_up.data_ptr() + 4 * gi * H) if dh_up is not None else None,
                           dhg=d_hcat.data_ptr() + 4 * gi * H, gp=saved.gates[gi].data_ptr(), es=saved.es[gi],
                           dyp=_lib.ptr(dy), dmsg=dmsg.data_ptr(), ws=ws_w.data_ptr(), ws_bytes=ws_w.numel() * 4,
                           wn=(P['output_transform_node.weight'].data_ptr() + 4 * gi * H) if dy is not None else None,
                           we=(P['output_transform_edge.weight'].data_ptr() + 4 * gi * H) if dy is not None else None,
                           e=_cell_ptrs(P, f + 'edge_gru.'), n=_cell_ptrs(P, f + 'node_gru.'),
                           ge=_cell_ptrs(grads, f + 'edge_gru.'), gn=_cell_ptrs(grads, f + 'node_gru.'))


def _bwd_node_cell(c, route: CallRoute, q) -> None:
    """Node cell backward: d_es -> dmsg[det rows, 0:H], d_hcat[det rows], the cell's parameter gradients."""
    g, H, GH, Dn, IN_e, st = c.g, c.H, c.GH, c.Dn, c.IN_e, c.st
    if route.bwd_fused:
        # one pass over the gates per cell: data and weight gradients together
        _lib.call('tmpnn_gru_bwd_fused', g.det_row.data_ptr(), Dn, 0, None, None, q.es.data_ptr(), H, 1, H,
                  q.hg, GH, H, q.n[0], q.n[1],
                  q.gp, c.plane, q.dog, GH, q.dyp, q.wn, q.dmsg, IN_e, q.dhg, GH, None, None, None, 0,
                  *q.gn, q.ws, q.ws_bytes, st)
        return
    _lib.call('tmpnn_gru_bwd_data', g.det_row.data_ptr(), Dn, H, q.hg, GH, H, q.n[0], q.n[1],
              q.gp, c.plane, q.dog, GH, q.dyp, q.wn, q.dmsg, IN_e, q.dhg, GH, None, None, None, 0, st)
    _lib.call('tmpnn_gru_bwd_weights', g.det_row.data_ptr(), Dn, 0, None, None, q.es.data_ptr(), H, 1, H,
              q.hg, GH, H, q.gp, c.plane, q.dog, GH, q.dyp, q.wn, *q.gn, q.ws, q.ws_bytes, st)


def _bwd_edge_fused(c, route: CallRoute, q, saved: SavedCall) -> None:
    """Edge cell backward on the one-pass kernel: the rows with a state on the full kernel, the call's new rows on the
    zero-state one where the route says so."""
    g, H, GH, N, E, IN_e, st, E_old = c.g, c.H, c.GH, c.N, c.E, c.IN_e, c.st, route.E_old
    fuse = c.K == 0
    if route.recompute_gates:
        # (RECOMPUTE_GATES) the edge rows of the gate planes, formed again from the saved state
        proj_s, whh_t_s = saved.proj[q.gi]
        h_scr = _wide_workspace(4 * N * GH, c.dev, slot=2)
        _lib.call('tmpnn_gru_fwd_tiles', edge_tiles(g, route.tile_rows).cref(), E, proj_s.data_ptr(), 3 * H, q.hg, GH, H,
                  whh_t_s.data_ptr(), q.e[2], q.e[3],
                  h_scr.data_ptr() + 4 * q.gi * H, GH, q.gp, c.plane, None, None, 0, st)
    # a call's new edge rows enter with h = 0 (mp_forward zero-fills h_cat[N_old:]) and form the suffix [E_old, E) of
    # the ascending edge list: their backward has no W_hh side and no d_h (those d_hcat rows lie behind d_h_in), so it
    # runs on its own kernel.  The forward's decision: with it set (and zs_fwd), those rows' hn plane and state rows
    # were never written
    zs = route.zs_groups[q.gi]
    E_full = E_old if zs else E
    if E_full > 0:
        _lib.call('tmpnn_gru_bwd_fused', g.edge_row.data_ptr(), E_full, c.xmode, g.src.data_ptr(), g.dst.data_ptr(),
                  None, 0, 0, IN_e, q.hg, GH, H, q.e[0], q.e[1],
                  q.gp, c.plane, q.dog, GH, q.dyp, q.we, q.dmsg, IN_e, q.dhg, GH,
                  g.src.data_ptr() if fuse else None, g.dst.data_ptr() if fuse else None,
                  q.dmsg if fuse else None, IN_e, *q.ge, q.ws, q.ws_bytes, st)
    if zs:
        zg, zplane = q.gp, c.plane
        if route.zs_rc:
            # no planes were saved for these rows: the kernel forms the gates from the forward's projected det rows
            # (struct tmpnn_zs_gate_src, read at launch; gate_plane = 0 says so)
            src_ = _lib.CZsGateSrc(saved.proj[q.gi][0].data_ptr(), 3 * H, g.src_pos.data_ptr() + 4 * E_old,
                                   g.dst_pos.data_ptr() + 4 * E_old, q.e[2], q.e[3])
            zg, zplane = ctypes.addressof(src_), 0
        _lib.call('tmpnn_gru_bwd_fused_zero_state', g.edge_row.data_ptr() + 4 * E_old, E - E_old,
                  g.src.data_ptr() + 4 * E_old, g.dst.data_ptr() + 4 * E_old, IN_e, q.hg, GH, H,
                  q.e[0], q.e[3] + 4 * 2 * H, zg, zplane, q.dog, GH, q.dyp, q.we,
                  q.dmsg, IN_e, q.ge[0], q.ge[2], q.ge[3], q.ws, q.ws_bytes, st)


def _bwd_edge_weights(c, q) -> None:
    """The stand-alone weight-gradient kernel over the edge rows."""
    g = c.g
    _lib.call('tmpnn_gru_bwd_weights', g.edge_row.data_ptr(), c.E, c.xmode, g.src.data_ptr(), g.dst.data_ptr(),
              None, 0, 0, c.IN_e, q.hg, c.GH, c.H, q.gp, c.plane, q.dog, c.GH, q.dyp, q.we, *q.ge, q.ws, q.ws_bytes, c.st)


def _bwd_edge_generic(c, q) -> None:
    """Edge cell backward on the two stand-alone kernels: d_ns -> dmsg[edge rows, 0:IN_e], d_hcat[edge rows]; without
    attention the adjoint of the edge -> node sum (d_es[src] - d_es[dst], read from dmsg's det rows) rides along."""
    g, IN_e = c.g, c.IN_e
    fuse = c.K == 0
    _lib.call('tmpnn_gru_bwd_data', g.edge_row.data_ptr(), c.E, IN_e, q.hg, c.GH, c.H, q.e[0], q.e[1],
              q.gp, c.plane, q.dog, c.GH, q.dyp, q.we, q.dmsg, IN_e, q.dhg, c.GH,
              g.src.data_ptr() if fuse else None, g.dst.data_ptr() if fuse else None,
              q.dmsg if fuse else None, IN_e, c.st)
    _bwd_edge_weights(c, q)


def _bwd_edge_wide_det(c, route: CallRoute, q, prep: int) -> None:
    """Wide cell, det-side: the whole edge-cell backward in one call; the message adjoint lands on d_hcat's det rows directly."""
    g, H, GH, IN_e, dev, st = c.g, c.H, c.GH, c.IN_e, c.dev, c.st
    fuse = c.K == 0
    wsb = int(_lib.load().tmpnn_wide_gru_bwd_diff_ws(c.N, c.E, c.Dn, H))
    ws_wide = _wide_workspace(wsb, dev)
    aux = _aux_stream(dev)
    args = (prep, g.cref(), q.hg, GH, H, q.gp, c.plane, q.dog, GH, q.dyp, q.we, q.dhg, GH, *q.ge,
            ws_wide.data_ptr(), wsb, st)
    # (every buffer the auxiliary stream touches was allocated on, and is next used on, the current stream,
    #  which the call leaves waiting for the auxiliary work: no record_stream needed)
    evf = evj = None
    if aux is not None:
        ef, ej = _aux_event_pair(dev)
        evf, evj = ef.cuda_event, ej.cuda_event
        if not evf or not evj:                     # (no native handle: one stream)
            aux = evf = evj = None
    _seg_plan_guard(g, dev, aux is not None)       # (the three d_gi segment sums run on `aux` when it is given)
    if route.edge_bwd == 'wide_det_fused':
        # the adjoint of the edge -> node sum rides in the epilogue of the E-row product (no separate pass over d_h)
        _lib.call('tmpnn_wide_gru_bwd_diff_fused', *args[:-1], q.dmsg, IN_e, st, aux, evf, evj)
        return
    if aux is not None:
        _lib.call('tmpnn_wide_gru_bwd_diff_aux', *args, aux, evf, evj)
    else:
        _lib.call('tmpnn_wide_gru_bwd_diff', *args)
    if fuse:
        _lib.call('tmpnn_gather_diff_fwd', g.cref(), q.dmsg, IN_e, q.dhg, GH, H, 1, st)


def _bwd_edge_wide(c, route: CallRoute, q, saved: SavedCall) -> None:
    """Wide cell (H >= 128) backward, in the form the route names."""
    g, H, GH, E, IN_e, dev, st = c.g, c.H, c.GH, c.E, c.IN_e, c.dev, c.st
    prep = saved.wide[q.gi].data_ptr()
    if route.edge_bwd in ('wide_det_fused', 'wide_det'):
        _bwd_edge_wide_det(c, route, q, prep)
        return
    lib = _lib.load()
    wsb = int(lib.tmpnn_wide_gru_bwd_data_ws(E, H))
    ws_wide = _wide_workspace(wsb, dev)
    _lib.call('tmpnn_wide_gru_bwd_data', prep, g.edge_row.data_ptr(), E, q.hg, GH, H,
              q.gp, c.plane, q.dog, GH, q.dyp, q.we, q.dmsg, IN_e, q.dhg, GH, ws_wide.data_ptr(), wsb, st)
    if c.K == 0:
        _lib.call('tmpnn_gather_diff_fwd', g.cref(), q.dmsg, IN_e, q.dhg, GH, H, 1, st)
    if route.edge_bwd == 'wide_data_dw':
        # ... and the weight gradient from the gate gradients that call left in its workspace
        ws2b = int(lib.tmpnn_wide_gru_bwd_weights_ws(E, H))
        ws2 = _wide_workspace(ws2b, dev, slot=1)
        _lib.call('tmpnn_wide_gru_bwd_weights', ws_wide.data_ptr(), g.edge_row.data_ptr(), E, g.src.data_ptr(),
                  g.dst.data_ptr(), q.hg, GH, H, *q.ge, ws2.data_ptr(), ws2b, st)
    else:
        _bwd_edge_weights(c, q)


def _bwd_attention(c, q, att_groups, grads, grad_out, dmsg: torch.Tensor) -> None:
    """Attention backward of one feature group: into d_hcat, and the heads' parameter gradients."""
    g, H, GH, N, E, Dn, K, IN_e, opts = c.g, c.H, c.GH, c.N, c.E, c.Dn, c.K, c.IN_e, c.opts
    f = q.f
    lib = _lib.load()
    erec, inc_other = g.att_index() if E > 0 else (None, None)
    for k0, Kg, W, a, kp, ws_ha, score, stats, esk in att_groups:
        ws_n_att = lib.tmpnn_att_bwd_ws(E, Dn, H, Kg)
        ws_att = torch.empty((max(ws_n_att, 1),), **opts)
        if Kg == K:
            d_out, ld_dout = dmsg.data_ptr(), IN_e
        else:           # this group's share of the head mean: d es / d es_group = K_g / K
            d_es_g = torch.zeros((N, H), **opts)
            d_es_g[g.det_row.long()] = dmsg[g.det_row.long(), :H] * (Kg / K)
            d_out, ld_dout = d_es_g.data_ptr(), H
        gW = [grads.get(f + f'gat.{k}.W_att') for k in range(k0, k0 + Kg)] if grad_out is not None else []
        ga = [grads.get(f + f'gat.{k}.a') for k in range(k0, k0 + Kg)] if grad_out is not None else []
        args = (g.cref(), _lib.ptr(erec), _lib.ptr(inc_other), q.hg, GH, H, Kg, W.data_ptr(),
                a.data_ptr(), _lib.ptr(kp), ATT_DROPOUT_P, ws_ha.data_ptr(), score.data_ptr(), stats.data_ptr(),
                esk.data_ptr(), d_out, ld_dout, ws_att.data_ptr(), ws_att.numel(), q.dhg, GH)
        if grad_out is not None and all(t is not None and t.is_contiguous() for t in gW + ga):
            # in-place mode: the heads' gradient buffers are accumulated directly (no stacked temporary, no adds)
            pW = (ctypes.c_void_p * Kg)(*[t.data_ptr() for t in gW])
            pa = (ctypes.c_void_p * Kg)(*[t.data_ptr() for t in ga])
            _lib.call('tmpnn_att_bwd_heads', *args, ctypes.cast(pW, ctypes.c_void_p), ctypes.cast(pa, ctypes.c_void_p), c.st)
        else:
            dW = torch.zeros((Kg, H, H), **opts)
            da = torch.zeros_like(a)
            _lib.call('tmpnn_att_bwd', *args, dW.data_ptr(), da.data_ptr(), c.st)
            for k in range(Kg):
                if grad_out is not None:
                    grads[f + f'gat.{k0 + k}.W_att'].add_(dW[k])
                    grads[f + f'gat.{k0 + k}.a'].add_(da[k].reshape(-1, 1))
                else:
                    grads[f + f'gat.{k0 + k}.W_att'] = dW[k]
                    grads[f + f'gat.{k0 + k}.a'] = da[k].reshape(-1, 1)


def _bwd_input_transform(c, route: CallRoute, saved: SavedCall, P, grads, d_hcat, training: bool, need_x: bool):
    """Input transform backward from d_hcat's new det rows: the transforms' parameter gradients and (need_x) d_x."""
    spec, plan, H, GH, n, opts = c.spec, c.plan, c.H, c.GH, c.n, c.opts
    lib = _lib.load()
    nd = int(plan.new_det_row.numel())
    S = plan.S
    Ft = spec.F_total
    d_xdet = torch.empty((max(nd, 1), Ft), **opts) if need_x else None
    d_xzero = torch.empty((max(S, 1), Ft), **opts) if need_x else None
    f0 = 0
    for gi, (_, F) in enumerate(spec.groups):
        t = f'input_transforms.{gi}.'
        # d_xzero is [S][F] per group: write into a per-group buffer, then place it
        dz_g = torch.empty((max(S, 1), F), **opts) if need_x else None
        tf = route.tf[gi]
        if tf:
            wsb = int(lib.tmpnn_input_tf_bwd_ws(nd, S, H, F, int(training)))
            ws = torch.empty((wsb // 4 + 1,), **opts)
        else:
            ws = torch.empty((max(lib.tmpnn_input_bn_bwd_ws(nd, S, H, F), 1),), **opts)
            wsb = ws.numel()
        _lib.call('tmpnn_input_tf_bwd' if tf else 'tmpnn_input_bn_bwd',
                  *_tf_head(tf, plan, saved.xdet.data_ptr() + 4 * f0, saved.xrows, Ft, F, nd, H), int(training),
                  P[t + '0.weight'].data_ptr(), P[t + '0.bias'].data_ptr(),
                  P[t + '1.weight'].data_ptr(), P[t + '1.bias'].data_ptr(), P[t + '3.weight'].data_ptr(),
                  saved.y_save[gi].data_ptr(), saved.mean[gi].data_ptr(), saved.rstd[gi].data_ptr(),
                  plan.new_det_row.data_ptr(), d_hcat.data_ptr() + 4 * gi * H, GH,
                  (d_xdet.data_ptr() + 4 * f0) if need_x else None, Ft, _lib.ptr(dz_g),
                  grads[t + '0.weight'].data_ptr(), grads[t + '0.bias'].data_ptr(),
                  grads[t + '1.weight'].data_ptr(), grads[t + '1.bias'].data_ptr(),
                  grads[t + '3.weight'].data_ptr(), grads[t + '3.bias'].data_ptr(),
                  ws.data_ptr(), wsb, c.st)
        if need_x:
            d_xzero[:, f0:f0 + F] = dz_g
        f0 += F
    if not need_x:
        return None
    # all-zero (edge) rows get the gradient that flows through their segment's batch statistics
    d_x = d_xzero[:S].index_select(0, plan.seg_of_new) if S > 0 else torch.zeros((n, Ft), **opts)
    if nd > 0:
        d_x.index_copy_(0, plan.new_det_local, d_xdet[:nd])
    return d_x


def mp_backward(spec: ModelSpec, plan: CallPlan, saved: SavedCall, P: Dict[str, torch.Tensor], training: bool,
                d_scores: Optional[torch.Tensor], d_logits: Optional[torch.Tensor], d_hout: Optional[torch.Tensor],
                need_x: bool, need_h: bool, grad_out=None):
    """Returns (d_x | None, d_h_in | None, {param name: grad}).  Runs the backward of saved.route: whatever the forward
    prepared for, whatever the switches say by now."""
    route = saved.route
    c = _call_dims(spec, plan, saved.h_cat.device)
    g, H, GH, N, E, Dn, IN_e, opts = c.g, c.H, c.GH, c.N, c.E, c.Dn, c.IN_e, c.opts
    lib = _lib.load()
    grads = _bwd_grads(spec, P, opts, grad_out)
    dy, dh_up = _bwd_heads(c, saved, P, grads, d_scores, d_logits, d_hout)

    d_hcat = torch.empty((N, GH), **opts)
    dmsg = torch.empty((N, IN_e), **opts)
    ws_e = lib.tmpnn_gru_bwd_weights_ws(E, IN_e, H)
    ws_n = lib.tmpnn_gru_bwd_weights_ws(Dn, H, H)
    ws_f = max(lib.tmpnn_gru_bwd_fused_ws(E, IN_e, H), lib.tmpnn_gru_bwd_fused_ws(Dn, H, H)) if route.bwd_fused else 0
    ws_w = torch.empty((max(ws_e, ws_n, ws_f) // 4 + 1,), **opts)
    # adjoint of the node -> edge message: into d_hcat[det rows] (the det-side wide backward has already put it there)
    gather = 'tmpnn_gather_concat_bwd' if spec.msg_type == 'concat' else 'tmpnn_gather_diff_bwd'
    for gi in range(c.G):
        q = _bwd_group(c, gi, saved, P, grads, dy, dh_up, d_hcat, dmsg, ws_w)
        _bwd_node_cell(c, route, q)
        if route.edge_bwd == 'fused':
            _bwd_edge_fused(c, route, q, saved)
        elif route.edge_bwd == 'generic':
            _bwd_edge_generic(c, q)
        else:
            _bwd_edge_wide(c, route, q, saved)
        if c.K > 0:
            _bwd_attention(c, q, saved.att[gi], grads, grad_out, dmsg)
        if route.gather_bwd:
            _lib.call(gather, g.cref(), q.dmsg, IN_e, q.dhg, GH, H, 1, c.st)

    d_x = None
    if c.n > 0:
        d_x = _bwd_input_transform(c, route, saved, P, grads, d_hcat, training, need_x)
    elif need_x:
        d_x = torch.zeros((0, spec.F_total), **opts)
    d_h_in = d_hcat[:c.N_old] if (need_h and c.N_old > 0) else None
    return d_x, d_h_in, grads


class MPIteration(torch.autograd.Function):
    """autograd node of one forward call.  Inputs: (ctx_obj, x, h_in_or_None, *params)."""

    @staticmethod
    def forward(ctx, call, x, h_in, *params):
        spec: ModelSpec = call['spec']
        names = spec.param_names()
        P = {nm: _f32c(p.detach()) for nm, p in zip(names, params)}
        for nm, p in P.items():
            _require_device(p, nm)
        need_grad = call['need_grad']
        scores, logits, h_out, alphas, saved = mp_forward(
            spec, call['plan'], x.detach(), None if h_in is None else _f32c(h_in.detach()), P, call['buffers'],
            call['training'], need_grad, call.get('keep'), call.get('reserve', 0), call.get('h_spare', 0))
        call['alphas'] = alphas
        ctx.call = call
        ctx.saved = saved
        ctx.P = P
        ctx.has_h = h_in is not None
        ctx.set_materialize_grads(False)
        return scores, logits, h_out

    @staticmethod
    def backward(ctx, d_scores, d_logits, d_hout):
        call = ctx.call
        spec: ModelSpec = call['spec']
        need = ctx.needs_input_grad
        names = spec.param_names()
        objs = call.get('param_objs')
        grad_out = None
        if (INPLACE_GRADS or call.get('inplace')) and objs is not None and all(need[3:]):
            gs = [p.grad for p in objs]
            if all(g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.device == ctx.P[nm].device
                   and g.shape == ctx.P[nm].shape for g, nm in zip(gs, names)):
                grad_out = dict(zip(names, gs))
        d_x, d_h_in, grads = mp_backward(spec, call['plan'], ctx.saved, ctx.P, call['training'],
                                         d_scores, d_logits, d_hout, need_x=need[1],
                                         need_h=ctx.has_h and need[2], grad_out=grad_out)
        ctx.saved = None
        if grad_out is not None:
            return (None, d_x, d_h_in) + (None,) * len(names)      # already added into p.grad
        return (None, d_x, d_h_in) + tuple(grads[nm] for nm in names)
