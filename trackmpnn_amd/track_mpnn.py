"""Drop-in `TrackMPNN` (reference/models/track_mpnn.py:8-75) running on the MI355X HIP kernels.

Same constructor, same `state_dict` keys, same
`forward(x, h_in, node_adj, edge_adj) -> (scores, logits, h_out, attention)` signature, so the
reference's train.py / infer.py call pattern works unchanged (train.py:320-325, 68, 107;
infer.py:106-110, 51, 75).  Added on top: `forward_graph(x, h_in, plan)` takes a prebuilt
`CallPlan` (graph already in index form and resident on the device; many windows may be batched
block-diagonally), which is what the benchmark and any loop that owns its graphs should call.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn

import os
import weakref

from . import functional as _functional
from .functional import MPIteration, ModelSpec
from .graph import (DG_BIG_ROWS, CallPlan, DeviceGraph, FrameGraph, device_graph_from_adjacency, graph_from_adjacency,
                    plan_single)
from .layers import FactorGraphGRU
from .small import SmallPath, _ParamSink, _SmallIter, fast_module, plan_small_route, small_eligible

# hidden widths the kernels run natively; above 256 (multiples of 128, csrc/common.h supported_H_big) models without
# attention heads are served: the wide edge cell and the H-generic f32 kernels, row movers in 256-column slices
KERNEL_WIDTHS = (32, 64, 128, 256, 384, 512, 640, 768, 896, 1024)

STRICT_GRAPH = os.environ.get('TMPNN_STRICT_GRAPH', '0') == '1'     # validate every adjacency at once (host sync)
SMALL_PATH = os.environ.get('TMPNN_SMALL_PATH', '1') != '0'         # fused batch-1 iteration for eligible calls
DEBUG_INPUTS = os.environ.get('TMPNN_DEBUG', '0') == '1'            # check the all-zero contract of x's edge rows (host sync)


class SparseAttention:
    """Attention weights of one head in CSR (per det, per incident edge) form.

    The reference returns a dense [N, N] matrix per head (models/layers.py:35-37) whose only
    informative entries are (det row, incident edge row); `to_reference_dense()` rebuilds that
    matrix, including the uniform 1/N rows an all-masked softmax produces for edge rows and
    isolated dets (eval mode; in train mode the reference additionally applies a dense dropout to
    those uninformative rows, which is not reproduced).
    """

    def __init__(self, graph: FrameGraph, alpha: torch.Tensor):
        self.graph = graph
        self.alpha = alpha          # [2E] CSR order

    def to_reference_dense(self) -> torch.Tensor:
        g = self.graph
        N = g.N
        out = torch.full((N, N), 1.0 / max(N, 1), dtype=self.alpha.dtype, device=self.alpha.device)
        counts = (g.rowptr[1:] - g.rowptr[:-1]).long()
        det_of_pos = torch.repeat_interleave(g.det_row.long(), counts)
        has = g.det_row.long()[counts > 0]
        out[has] = 0.0
        out[det_of_pos, (g.inc & 0x7FFFFFFF).long()] = self.alpha
        return out

    # ---- the reference's consumers of forward()'s 4th output treat a head's attention as a dense [N, N] tensor
    #      (attention_weights.py:62: `att.cpu().detach().numpy()`, :84-93: `.shape`, `a[row][col]`): those uses work on this
    #      object unchanged -- the dense matrix is built on first use and kept
    def _dense(self) -> torch.Tensor:
        d = self.__dict__.get('_dense_cache')
        if d is None:
            d = self.__dict__['_dense_cache'] = self.to_reference_dense()
        return d

    @property
    def shape(self):
        return torch.Size((self.graph.N, self.graph.N))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def cpu(self) -> torch.Tensor:
        return self._dense().cpu()

    def detach(self) -> torch.Tensor:
        return self._dense().detach()

    def numpy(self):
        return self._dense().detach().cpu().numpy()

    def __array__(self, dtype=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)

    def __getitem__(self, idx):
        return self._dense()[idx]

    def per_edge(self) -> torch.Tensor:
        """[E, 2]: weight the src det / the dst det gives each edge (oracle layout)."""
        g = self.graph
        e, ep = g.inc_edge_endpoint()
        out = torch.zeros((g.E, 2), dtype=self.alpha.dtype, device=self.alpha.device)
        out[e, ep] = self.alpha
        return out


class TrackMPNN(nn.Module):
    def __init__(self, features, ncategories, nhidden, nattheads, msg_type):
        super().__init__()
        nhidden = int(nhidden)
        if not 1 <= nhidden <= KERNEL_WIDTHS[-1]:
            raise ValueError(f'nhidden={nhidden}: the gfx950 kernels cover 1 .. {KERNEL_WIDTHS[-1]} hidden units')
        if nhidden > 256 and int(nattheads) > 0:
            raise ValueError(f'nhidden={nhidden} > 256 is served without attention heads only (got nattheads={nattheads})')
        # the kernels are instantiated for KERNEL_WIDTHS; any other width runs zero-padded to the next one (exact:
        # a padded unit has zero weights and biases everywhere, so it stays 0 through BatchNorm, both GRU cells,
        # the attention scores and the heads -- see _pad_params)
        self.hpad = next(w for w in KERNEL_WIDTHS if nhidden <= w)
        self._padded = self.hpad != nhidden
        self.input_transforms = nn.ModuleList([])
        self.factor_grus = nn.ModuleList([])
        self.feature_idx = []
        self.nhidden = nhidden
        groups = []
        nfeatures = 0
        for key, width in (('2d', ncategories + 5), ('temp', 2), ('vis', 128)):     # track_mpnn.py:17-33
            if key in features:
                self.input_transforms.append(self.get_input_transform(width, nhidden))
                self.factor_grus.append(FactorGraphGRU(nhidden, nattheads, msg_type, True))
                self.feature_idx.append(list(range(nfeatures, nfeatures + width)))
                groups.append((key, width))
                nfeatures += width
        if not groups:
            raise ValueError("features must contain at least one of '2d', 'temp', 'vis'")
        self.output_transform_node = nn.Linear(len(groups) * nhidden, 1, bias=True)
        self.output_transform_node.weight.data.normal_(mean=0.0, std=0.01)
        self.output_transform_node.bias.data.uniform_(+4.595, +4.595)
        self.output_transform_edge = nn.Linear(len(groups) * nhidden, 1, bias=True)
        self.output_transform_edge.weight.data.normal_(mean=0.0, std=0.01)
        self.output_transform_edge.bias.data.uniform_(-4.595, -4.595)
        self.output_activation = nn.Sigmoid()
        self.spec = ModelSpec(tuple(groups), self.hpad, max(int(nattheads), 0), msg_type)
        # set by trackmpnn_amd.dist.GradBucket: parameter gradients are added straight into p.grad (functional.py)
        self.inplace_param_grads = False
        self._small = SmallPath(self)          # batch-1 path state (pointer structs, operand images)
        self._drop(TrackMPNN._CACHED)

    # cached state and per-call bookkeeping of the batch-1 path, each field named once with what it holds; every field drops
    # to None (the call counter to 0, the pending list to []).  Plain Python values, reassigned on every forward call: kept
    # out of nn.Module.__setattr__'s parameter / buffer / sub-module checks (~2.5 us per assignment, twice per call)
    _CACHED = ('_pad_cache',            # (key, padded parameter copies, token) of the zero-padded widths
               '_small_pad',            # SmallPath of a zero-padded width (its parameters are the padded copies)
               '_plist', '_bufs',       # parameters in spec.param_names() order / buffers by name (_param_list)
               '_anchor',               # the dummy autograd input of the in-place gradient mode
               '_anch_key', '_anch_calls', '_gst',      # usable .grad buffers: sentinel pointers, call count, pointer struct
               '_sink', '_sink_key',    # gradient sink of the native node (default gradient mode) and what it was built over
               '_graph_cache',          # the last adjacency pair forward() converted
               '_pending_graphs',       # DeviceGraphs whose validation status has not been read back yet
               '_route')                # SmallRoute of the last forward_dgraph call (a record, not a cache)
    _PLAIN = frozenset(_CACHED)
    _ON_LOAD = ('_pad_cache', '_plist', '_bufs', '_sink', '_sink_key')          # what load_state_dict drops (new values)
    _ON_MOVE = _ON_LOAD + ('_anchor', '_anch_key', '_graph_cache')              # what _apply drops (new storage)

    def __setattr__(self, name, value):
        if name in TrackMPNN._PLAIN:
            object.__setattr__(self, name, value)
        else:
            super().__setattr__(name, value)

    def _drop(self, fields, state=None):
        """Drop the named cached fields: on the module (the pointer structs of `_small` are then re-read as well), or on
        `state`, a copy of its __dict__."""
        d = self.__dict__ if state is None else state
        for k in fields:
            d[k] = [] if k == '_pending_graphs' else (0 if k == '_anch_calls' else None)
        if state is None:
            self._small.invalidate()

    def _drop_caches(self):
        # adjacencies converted by earlier eager calls and not yet checked are validated NOW (one host round trip) instead of
        # being forgotten: the caller is promised a ValueError for an invalid graph, not just NaN outputs
        if self._pending_graphs and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            self.check_graphs()
        self._drop(TrackMPNN._CACHED)

    def __getstate__(self):
        # copy.deepcopy(model), pickle, torch.save(model): the batch-1 path's caches hold ctypes pointer structs, function
        # pointers and a non-leaf sink tensor -- none of them copyable, all of them rebuilt on the next forward call
        state = self.__dict__.copy()
        self._drop(TrackMPNN._CACHED, state)
        state['_small'] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        object.__setattr__(self, '_small', SmallPath(self))

    def refresh_weights(self):
        """Re-read every parameter for the batch-1 path.  Its GRU operand images are rebuilt when a weight's version
        counter moves (optimizer steps, in-place ops, load_state_dict); an edit through `.data` (`p.data.copy_`, an EMA
        swap, `p.data.normal_()`) does not move it -- call this after such an edit.  TMPNN_DEBUG=1 rebuilds on every call."""
        self._drop_caches()

    def _apply(self, fn, *args, **kwargs):
        # .cuda() / .to() / .float(): parameter storage moves -> drop every cached device pointer
        out = super()._apply(fn, *args, **kwargs)
        self._drop(TrackMPNN._ON_MOVE)
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._drop(TrackMPNN._ON_LOAD)
        return out

    def get_input_transform(self, n_in, n_out):
        lin1 = nn.Linear(n_in, n_out, bias=True)
        lin1.weight.data.normal_(mean=0.0, std=0.01)
        lin1.bias.data.uniform_(0, 0)
        lin2 = nn.Linear(n_out, n_out, bias=True)
        lin2.weight.data.normal_(mean=0.0, std=0.01)
        lin2.bias.data.uniform_(0, 0)
        return nn.Sequential(lin1, nn.BatchNorm1d(n_out), nn.ReLU(), lin2)

    # ------------------------------------------------------------------------------------------
    def _params_and_buffers(self):
        named = dict(self.named_parameters())
        params = [named[nm] for nm in self.spec.param_names()]
        buffers = dict(self.named_buffers())
        return params, buffers

    # ------------------------------------------------------------------------------------------
    # nhidden outside KERNEL_WIDTHS: the call runs on zero-padded copies of the parameters (differentiable torch ops, so
    # autograd hands the true parameters their gradients); the carried state keeps the reference's [N, G * nhidden] shape
    # ------------------------------------------------------------------------------------------
    def _pad_params(self, params):
        H, Hp, G, K = self.nhidden, self.hpad, self.spec.G, self.spec.K
        d = Hp - H
        nb_e = 2 if self.spec.msg_type == 'concat' else 1
        pad = torch.nn.functional.pad

        def gru_w(w, nb):                      # [3H, nb*H] -> [3Hp, nb*Hp], gate by gate and input block by block
            return pad(w.reshape(3, H, nb, H), (0, d, 0, 0, 0, d)).reshape(3 * Hp, nb * Hp)

        def gru_b(b):
            return pad(b.reshape(3, H), (0, d)).reshape(3 * Hp)

        it = iter(params)
        out = []
        for _ in range(G):
            w1, b1, gam, bet, w2, b2 = (next(it) for _ in range(6))
            out += [pad(w1, (0, 0, 0, d)), pad(b1, (0, d)), pad(gam, (0, d)), pad(bet, (0, d)),
                    pad(w2, (0, d, 0, d)), pad(b2, (0, d))]
        for _ in range(G):
            w_ih, w_hh, b_ih, b_hh = (next(it) for _ in range(4))
            out += [gru_w(w_ih, nb_e), gru_w(w_hh, 1), gru_b(b_ih), gru_b(b_hh)]
            for _k in range(K):
                W_att, a = next(it), next(it)
                out += [pad(W_att, (0, d, 0, d)), pad(a, (0, 0, 0, d))]
            w_ih, w_hh, b_ih, b_hh = (next(it) for _ in range(4))
            out += [gru_w(w_ih, 1), gru_w(w_hh, 1), gru_b(b_ih), gru_b(b_hh)]
        for _ in range(2):
            w, b = next(it), next(it)
            out += [pad(w.reshape(1, G, H), (0, d)).reshape(1, G * Hp), b]
        return [t.contiguous() for t in out]

    def _padded_params(self, params):
        """The zero-padded parameter copies of a non-native width, built ONCE per set of parameter values (every parameter's
        version counter) instead of once per forward call: the calls of a window share one set of copies, so the ~30 pad
        kernels (and their backward) run once per step; autograd still hands the true parameters their gradients through
        the copies.  Dropped when a backward pass reaches the copies (their graph is spent), when a version moves, and by
        refresh_weights() / .to() / load_state_dict().  Edits through `p.data` (copy_, mul_) do NOT move the version counter:
        call refresh_weights() after them, as for the operand images of the fused path."""
        key = (torch.is_grad_enabled(), tuple((id(p), p._version, p.requires_grad) for p in params))
        c = self._pad_cache
        if c is not None and c[0] == key:
            return c[1]
        out = self._pad_params(params)
        token = object()
        self._pad_cache = (key, out, token)
        if self._small_pad is not None:
            self._small_pad.invalidate()       # (fresh copies: new pointers AND new values behind version counters that start at 0)
        if torch.is_grad_enabled():
            live = [t for t in out if t.requires_grad]
            if live:
                me = weakref.ref(self)                 # (no reference cycle tensor -> hook -> copies -> tensor)

                def spent(_g, me=me, token=token):
                    m = me()
                    if m is not None and m._pad_cache is not None and m._pad_cache[2] is token:
                        m._pad_cache = None
                for t_ in live:                          # (any copy a backward pass reaches spends the shared graph: a pass that
                    t_.register_hook(spent)              #  stops short of the first parameter must invalidate the cache too)
        return out

    def _pad_state(self, h):
        N, G = h.shape[0], self.spec.G
        return torch.nn.functional.pad(h.reshape(N, G, self.nhidden), (0, self.hpad - self.nhidden)).reshape(N, G * self.hpad)

    def _unpad_state(self, h):
        N, G = h.shape[0], self.spec.G
        return h.reshape(N, G, self.hpad)[:, :, :self.nhidden].reshape(N, G * self.nhidden)

    def forward_graph(self, x: torch.Tensor, h_in: Optional[torch.Tensor], plan: CallPlan,
                      dropout_keep: Optional[Sequence[torch.Tensor]] = None, reserve_rows: int = 0):
        """One message-passing call on a prebuilt CallPlan (see trackmpnn_amd.graph).

        dropout_keep: optional per-group uint8 [K, 2E] keep masks (CSR order) replacing the
        internally drawn attention dropout (train mode, nattheads > 0).
        reserve_rows: rows the NEXT call will append; h_out is then allocated with that much spare room
        and the next call extends it in place instead of copying the carried state (only valid when
        each h_out is continued from at most once, as in the reference's train / infer loops).
        """
        if not x.is_cuda:
            raise RuntimeError(f'x is on {x.device}: trackmpnn_amd runs on the MI355X HIP kernels only '
                               '(no CPU or torch fallback exists)')
        params, buffers = self._params_and_buffers()
        need_grad = torch.is_grad_enabled() and (
            x.requires_grad or (h_in is not None and h_in.requires_grad) or any(p.requires_grad for p in params))
        true_buffers = None
        if self._padded:
            params = self._padded_params(params)
            h_in = self._pad_state(h_in) if h_in is not None else None
            d = self.hpad - self.nhidden
            true_buffers, buffers = buffers, dict(buffers)
            for k, b in true_buffers.items():            # BatchNorm running statistics of the padded units: (0, 1)
                if k.endswith('running_mean') or k.endswith('running_var'):
                    buffers[k] = torch.nn.functional.pad(b, (0, d), value=1.0 if k.endswith('var') else 0.0)
            reserve_rows = 0
        call = dict(spec=self.spec, plan=plan, buffers=buffers, training=self.training, need_grad=need_grad,
                    keep=dropout_keep, reserve=reserve_rows,
                    h_spare=getattr(h_in, '_tmpnn_spare_rows', 0) if h_in is not None else 0,
                    param_objs=params, inplace=self.inplace_param_grads and not self._padded)
        scores, logits, h_out = MPIteration.apply(call, x, h_in, *params)
        if self._padded:
            with torch.no_grad():
                for k, b in true_buffers.items():
                    if buffers[k] is not b:
                        b.copy_(buffers[k][:self.nhidden])
            h_out = self._unpad_state(h_out)
        h_out._tmpnn_spare_rows = max(int(reserve_rows), 0)
        attention = tuple(None if a is None else [SparseAttention(plan.graph, ak) for ak in a]
                          for a in call['alphas'])
        return scores, logits, h_out, attention

    # ------------------------------------------------------------------------------------------
    # batch-1 path (csrc/small.hip): one ctypes call per forward / backward, no host synchronisation
    # ------------------------------------------------------------------------------------------
    def check_graphs(self) -> None:
        """Read back the validation status of every adjacency converted since the last check (ONE host round trip)
        and raise ValueError for the first invalid one.  Called automatically before a backward (a gradient hook on the
        outputs of every call whose adjacency is still unchecked) and every 64 calls; until then an invalid graph's outputs
        are NaN (k_small_iter_fwd fills them), never stale memory."""
        if not self._pending_graphs or torch.cuda.is_current_stream_capturing():
            return                                   # (a capture cannot synchronise: the check happens after it)
        pending, self._pending_graphs = self._pending_graphs, []
        metas = torch.stack([g.arena[:8] for g in pending]).tolist()
        for g, m in zip(pending, metas):
            g._meta = (m[4], m[5], m[2])
        for g in pending:
            g.check()

    def _param_list(self):
        """The parameters in spec.param_names() order (the buffers by name land in `_bufs`), read once per set of storages."""
        if self._plist is None:
            named = dict(self.named_parameters())
            self._plist = [named[nm] for nm in self.spec.param_names()]
            self._bufs = dict(self.named_buffers())
        return self._plist

    def _padded_set(self, dev):
        """(padded parameter copies, their SmallPath) of a width the kernels are not instantiated for: the copies are built
        once per set of parameter values, the padded BatchNorm buffers are kept next to the true ones."""
        H, Hp = self.nhidden, self.hpad
        params = self._padded_params(self._param_list())
        sp = self._small_pad
        if sp is None or sp.pad_buffers is None or next(iter(sp.pad_buffers.values())).device != dev:
            sp = SmallPath(self, padded=True)
            sp.set_grad_layout(params)
            pb = {}
            for k, b in self._bufs.items():
                if k.endswith('running_mean') or k.endswith('running_var'):
                    pb[k] = torch.nn.functional.pad(b.detach().to(dev), (0, Hp - H), value=1.0 if k.endswith('var') else 0.0).contiguous()
                else:
                    pb[k] = b.detach().to(dev).clone()
            sp.pad_buffers = pb
            sp._buf_ver = {k: b._version for k, b in self._bufs.items()}
            self._small_pad = sp
        else:
            # the true buffers are the source of truth between calls (load_state_dict, manual edits): a padded copy is
            # refreshed when its original's version counter has moved since this path last wrote it
            for k, b in self._bufs.items():
                if sp._buf_ver.get(k) != b._version or torch.cuda.is_current_stream_capturing():
                    with torch.no_grad():
                        if k.endswith('running_mean') or k.endswith('running_var'):
                            sp.pad_buffers[k][:H].copy_(b)
                        else:
                            sp.pad_buffers[k].copy_(b)
                    sp._buf_ver[k] = b._version
        return params, sp

    def _grad_buffers_usable(self, params, dev) -> bool:
        """In-place accumulation (GradBucket): every parameter must own a usable .grad buffer; checked in full when the
        first / last buffer moves and every 64th call, by two sentinel pointers otherwise."""
        g0, g1 = params[0].grad, params[-1].grad
        key = (g0.data_ptr(), g1.data_ptr()) if (g0 is not None and g1 is not None) else None
        self._anch_calls += 1
        if key is not None and key == self._anch_key and (self._anch_calls & 63):
            return True
        ok = all(p.requires_grad and p.grad is not None and p.grad.dtype == torch.float32
                 and p.grad.is_contiguous() and p.grad.device == dev for p in params)
        self._anch_key = key if ok else None
        self._gst = self._small.grad_struct([p.grad for p in params]) if ok else None
        return ok

    def forward_dgraph(self, x: torch.Tensor, h_in: Optional[torch.Tensor], graph: DeviceGraph,
                       dropout_keep: Optional[Sequence[torch.Tensor]] = None):
        """One message-passing call on a DeviceGraph: the fused iteration (H in {32, 64}, other widths up to 64 zero-padded
        when they have no attention heads; with heads the attention stage runs between its two launches), the staged kernels
        for every other model.  What runs is decided once (small.plan_small_route) and kept in `_route`.  A padded width runs
        the same two launches per direction on the ZERO-PADDED parameter copies (autograd hands the true parameters their
        gradients through the pads, summed over the calls of a window first), with the carried state kept in its padded form
        behind the [N, G * nhidden] tensor the caller sees (a view of it where there is one feature group).
        dropout_keep: as forward_graph."""
        if not x.is_cuda:
            raise RuntimeError(f'x is on {x.device}: trackmpnn_amd runs on the MI355X HIP kernels only '
                               '(no CPU or torch fallback exists)')
        # ---- the route
        sp, padded, dev = self._small, self._padded, x.device
        fused = small_eligible(self, graph.N)
        params = self._param_list()
        if fused and padded:
            params, sp = self._padded_set(dev)           # (the node is handed the copies: the route reads THEIR flags)
        fast = fast_module()
        grad_on = torch.is_grad_enabled()
        pgrad = grad_on and any(p.requires_grad for p in params)
        inplace = (fused and pgrad and not padded and (self.inplace_param_grads or _functional.INPLACE_GRADS)
                   and self._grad_buffers_usable(params, dev))
        route = self._route = plan_small_route(
            fused, sp.att, padded, graph.N, graph.cap, grad_on, grad_on and x.requires_grad,
            grad_on and h_in is not None and h_in.requires_grad, pgrad,
            inplace or (pgrad and all(p.requires_grad for p in params)), inplace, fast is not None)
        if route.path == 'staged':
            # the staged kernels on the same device-resident graph (frame_graph() reads E and Dn back: their launch sizes
            # are host values)
            return self.forward_graph(x, h_in, plan_single(graph.frame_graph(), int(x.shape[0])), dropout_keep=dropout_keep)
        need_grad = route.need_grad
        # ---- carried state: extended IN PLACE when it came out of this path (it has spare rows behind it) and has not been
        # continued from before; a second continuation from the same tensor copies instead
        h_c = h_in
        if padded and h_in is not None:
            h_c = getattr(h_in, '_tmpnn_padded_state', None)
            # the padded tensor behind h_in is reused only while h_in is what this path returned: for several feature groups
            # h_in is a COPY of it, so an in-place edit by the caller (masking / resetting rows) moves h_in's version counter
            # and the state is padded afresh from h_in (one group: h_in is a view of the padded tensor, edits reach it)
            if (h_c is None or h_c.shape[0] != h_in.shape[0]
                    or (self.spec.G > 1 and getattr(h_in, '_tmpnn_padded_ver', None) != (h_in.data_ptr(), h_in._version))):
                h_c = self._pad_state(h_in)
        spare = max(256, graph.N)
        n = int(x.shape[0])
        append = (h_c is not None and n > 0 and getattr(h_c, '_tmpnn_spare_rows', 0) >= n
                  and not getattr(h_c, '_tmpnn_consumed', False))
        if append:
            h_c._tmpnn_consumed = True
        # ---- node call
        if (inplace or (route.node, route.grads) == ('native', 'none')) and (self._anchor is None or self._anchor.device != dev):
            self._anchor = torch.zeros(1, device=dev, requires_grad=True)     # one dummy tensor stands in for the parameters
        if route.node == 'native':
            # C++ autograd node (csrc_host/fast_iter.cpp): same kernels, no interpreter between the allocations
            if route.grads == 'sink':
                # one gradient SINK per set of parameter values (a fresh one whenever a parameter's version counter moved, i.e.
                # after every optimizer step; a padded width: whenever the copies were rebuilt).  Each call returns one flat
                # gradient buffer, autograd sums those per window and hands the slices to the parameters (the copies) once
                gst, total, offs, shapes = sp.grad_template(params)
                key = (self._pad_cache or (None,) * 3)[2] if padded else tuple(p._version for p in params)
                if self._sink is None or self._sink_key != key or self._sink.device != dev:
                    self._sink = _ParamSink.apply(total, offs, shapes, *params)
                    self._sink_key = key
                carrier = self._sink
            else:
                gst, total, carrier = (self._gst if inplace else sp.params(params)), 0, self._anchor
            info = sp.fast_info(params, graph, gst, self.training, need_grad, append, spare, sink_total=total)
            args = (x, h_c, carrier, graph.arena, info, sp.keep(gst if inplace else None))
            if route.grads == 'none':
                with torch.no_grad():
                    scores, logits, h_out = fast.small_iter(*args)
            else:
                scores, logits, h_out = fast.small_iter(*args)
        else:
            call = dict(small=sp, graph=graph, training=self.training, need_grad=need_grad, spare=spare, append=append,
                        param_objs=params, anchored=inplace, check_pending=self.check_graphs, keep=dropout_keep)
            scores, logits, h_out = _SmallIter.apply(call, x, h_c, *([self._anchor] if inplace else params))
        # ---- epilogue
        h_out._tmpnn_spare_rows = spare
        if need_grad and self._pending_graphs:
            # deferred validation must have happened before ANY backward node of this call runs (the native node does
            # not check): the first gradient that reaches one of the outputs triggers the one host round trip
            for t in (scores, logits, h_out):
                if t.requires_grad:
                    t.register_hook(self._check_graphs_hook)
        if padded:
            H = self.nhidden
            if self.training and n > 0:
                with torch.no_grad():                                  # running statistics of the true units (one fused copy + the counters)
                    fl = [k for k in self._bufs if k.endswith('running_mean') or k.endswith('running_var')]
                    torch._foreach_copy_([self._bufs[k] for k in fl], [sp.pad_buffers[k][:H] for k in fl])
                    for k, b in self._bufs.items():
                        if k not in fl:
                            b.copy_(sp.pad_buffers[k])
                        sp._buf_ver[k] = b._version
            h_pad = h_out
            h_out = h_pad[:, :H] if self.spec.G == 1 else self._unpad_state(h_pad)
            h_out._tmpnn_padded_state = h_pad
            h_out._tmpnn_padded_ver = (h_out.data_ptr(), h_out._version)
        if sp.att:
            fg = graph.frame_graph()
            return scores, logits, h_out, tuple([SparseAttention(fg, ak) for ak in a] for a in call['alphas'])
        return scores, logits, h_out, (None,) * self.spec.G

    def _check_graphs_hook(self, grad):
        self.check_graphs()
        return None

    def forward(self, x, h_in, node_adj, edge_adj):
        """reference/models/track_mpnn.py:54-75.  node_adj / edge_adj: dense or sparse-COO [N, N].

        Contract on x (as produced by utils/graph.py:148-149,291-292): rows of new EDGE nodes are all-zero; only the
        new det rows are read.  A non-zero edge row would enter the reference's BatchNorm statistics: on the batch-1 path
        such a call is marked invalid on the device (NaN outputs, ValueError at the next check_graphs()); the staged
        path checks it under TMPNN_DEBUG=1.  Graphs of up to 65535 rows without attention heads take the fused batch-1 path: the adjacency is
        converted on the device in one launch and validated LATE (check_graphs(); TMPNN_STRICT_GRAPH=1 validates
        at once), everything else is converted with torch index ops and validated immediately."""
        if not x.is_cuda:
            raise RuntimeError(f'x is on {x.device}: trackmpnn_amd runs on the MI355X HIP kernels only '
                               '(no CPU or torch fallback exists)')
        N = int(node_adj.shape[0])
        small = SMALL_PATH and small_eligible(self, N)
        # the last call's graph is reused when the SAME adjacency objects come again unmodified (the static-window pattern:
        # several MP iterations on one graph).  Weak references: the cache pins neither a dense N x N adjacency nor its
        # device copy, and a recycled id() cannot alias (a dead reference never matches).
        key = (N, node_adj._version, edge_adj._version, x.device, small)
        c = self._graph_cache
        if c is not None and c[0]() is node_adj and c[1]() is edge_adj and c[2] == key:
            graph = c[3]
        else:
            if small:
                graph = device_graph_from_adjacency(node_adj, edge_adj, x.device)
                if STRICT_GRAPH:
                    graph.check()
                else:
                    self._pending_graphs.append(graph)
                    if len(self._pending_graphs) >= 64:
                        self.check_graphs()
            elif N <= DG_BIG_ROWS:
                # staged path (attention heads, wide or padded cells): the same one-launch conversion, validated at
                # once (one host round trip for E / Dn, which the staged kernels' launch sizes need) -- the torch-ops
                # converter it replaces took 2 of the 2.4 ms of such a call on a KITTI-sized window
                graph = device_graph_from_adjacency(node_adj, edge_adj, x.device).frame_graph()
            else:
                graph = graph_from_adjacency(node_adj.to(x.device), edge_adj.to(x.device))
            self._graph_cache = (weakref.ref(node_adj), weakref.ref(edge_adj), key, graph)
        if DEBUG_INPUTS and x.shape[0] > 0:
            fg = graph.frame_graph() if isinstance(graph, DeviceGraph) else graph
            new_edges = fg.is_edge[N - int(x.shape[0]):] != 0
            if bool(new_edges.any()) and float(x[new_edges].abs().max()) != 0.0:
                raise ValueError('x has non-zero features on new EDGE rows: the reference would feed them to the BatchNorm '
                                 'statistics (utils/graph.py:148,291 always passes zeros); this implementation reads det '
                                 'rows only')
        if small:
            return self.forward_dgraph(x, h_in, graph)
        plan = plan_single(graph, int(x.shape[0]))
        return self.forward_graph(x, h_in, plan)
