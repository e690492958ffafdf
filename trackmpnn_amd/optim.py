"""The optimizer step on the device: `BucketAdam`, the reference's `optim.Adam(model.parameters(), lr, weight_decay)`
(train.py:329, stepped at train.py:135, driven by the `StepLR(step_size=15, gamma=0.2)` of train.py:330) over the flat
gradient bucket.

    bucket = GradBucket(model)
    opt = BucketAdam(model, bucket, lr=args.learning_rate, weight_decay=args.weight_decay)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=15, gamma=0.2)
    for epoch in ...:
        for X, y in chunks:
            opt.zero_grad()                    # bucket.zero(): p.grad keeps aliasing the bucket, whatever set_to_none says
            loss, _, _ = train_chunk(model, X, y, device)
            opt.step()                         # ONE launch (tmpnn_adam_step); nothing is read back
        sched.step()

The gradients already live in one flat buffer (`GradBucket.flat`); `exp_avg` and `exp_avg_sq` are two more flat buffers of the
same layout, and the parameters keep their own storage (a segment table tells the kernel where each one lives).  The learning
rate and the step count are device memory, so the same launch works inside a captured step (`CapturedWindow`) and a scheduler
step between replays takes effect.  `step(grad_scale=1 / world)` folds `allreduce_grads`' division, `step(zero_grads=True)`
folds `bucket.zero()`; `grad_flow()` is the per-parameter mean |g| of --plot-gradients (utils/gradients.py:23) in one launch.
"""
from __future__ import annotations

import inspect
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .dist import GradBucket

_FULL_CHECK_EVERY = 64          # steps between two full walks over the aliasing of p.grad / the parameter addresses
_CHUNK: Optional[int] = None


def chunk_elems() -> int:
    """Elements of one work item of the step kernel (tmpnn_optim_chunk)."""
    global _CHUNK
    if _CHUNK is None:
        _CHUNK = int(_lib.load().tmpnn_optim_chunk())
    return _CHUNK


def segment_table(bucket: GradBucket) -> np.ndarray:
    """int64 [P, 3] = struct tmpnn_optim_seg per parameter of the bucket, in bucket order: (address of the parameter's own
    storage, first element of its slice of the flat buffers, element count)."""
    rows, o = [], 0
    for p in bucket.params:
        rows.append((p.data_ptr(), o, p.numel()))
        o += p.numel()
    if o != bucket.flat.numel():
        raise ValueError(f'the bucket holds {bucket.flat.numel()} elements, its parameters {o}')
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def work_list(counts, chunk: Optional[int] = None) -> np.ndarray:
    """int32 [n, 2]: one (segment, offset inside the segment) pair per chunk of `chunk` elements; every element of every
    segment belongs to exactly one chunk, segments in order."""
    chunk = chunk_elems() if chunk is None else int(chunk)
    if chunk <= 0:
        raise ValueError(f'work_list: chunk={chunk}')
    segs, offs = [], []
    for s, n in enumerate(counts):
        n = int(n)
        if n < 0:
            raise ValueError(f'work_list: segment {s} has {n} elements')
        o = np.arange(0, n, chunk, dtype=np.int64)
        segs.append(np.full(o.shape, s, dtype=np.int64))
        offs.append(o)
    out = np.stack([np.concatenate(segs), np.concatenate(offs)], 1) if segs else np.zeros((0, 2), np.int64)
    if out.size and out.max() >= 2 ** 31:
        raise ValueError('work_list: a segment of 2^31 elements or more')
    return np.ascontiguousarray(out.astype(np.int32))


def _adam_defaults(lr, betas, eps, weight_decay) -> Dict:
    """The keys of torch.optim.Adam's parameter group in this torch (so that a state_dict goes either way)."""
    d = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    for k, prm in inspect.signature(torch.optim.Adam.__init__).parameters.items():
        if k not in ('self', 'params') and k not in d and prm.default is not inspect.Parameter.empty:
            d[k] = prm.default
    return d


_REFUSED = ('amsgrad', 'maximize', 'differentiable', 'decoupled_weight_decay')      # group flags that change the rule


class BucketAdam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight decay, no amsgrad) over a `GradBucket`; one HIP launch per step (module docstring).

    model_or_params  the module the bucket was made for, or its trainable parameters (a list, or ONE parameter group);
                     they must be exactly `bucket.params`.
    `opt.state[p]`   holds views: `exp_avg` / `exp_avg_sq` of the flat moment buffers, `step` of the device step count (one
                     fp32 scalar shared by every parameter), so in-place edits through it reach what the kernel reads.
    betas, eps and weight_decay are launch arguments: a captured step keeps the values it was recorded with."""

    def __init__(self, model_or_params, bucket: GradBucket, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0, **flags):
        for k, v in flags.items():
            if k in _REFUSED or k in ('foreach', 'capturable', 'fused'):
                if k in _REFUSED and v:
                    raise ValueError(f'BucketAdam: {k}={v!r} is not supported (plain Adam with L2 weight decay only)')
            else:
                raise TypeError(f'BucketAdam: unexpected argument {k!r}')
        self.model = model_or_params if isinstance(model_or_params, torch.nn.Module) else None
        if self.model is not None:
            params = [p for p in self.model.parameters() if p.requires_grad]
            group: Dict = {}
        else:
            params = list(model_or_params)
            group = {}
            if params and isinstance(params[0], dict):
                if len(params) != 1:
                    raise ValueError(f'BucketAdam: one parameter group only ({len(params)} given)')
                group = dict(params[0])
                params = list(group.pop('params'))
        lr = group.pop('lr', lr)
        betas = group.pop('betas', betas)
        eps = group.pop('eps', eps)
        weight_decay = group.pop('weight_decay', weight_decay)
        for k, v in group.items():
            if k in _REFUSED and v:
                raise ValueError(f'BucketAdam: {k}={v!r} is not supported (plain Adam with L2 weight decay only)')
        if isinstance(lr, torch.Tensor):
            raise ValueError('BucketAdam: lr must be a Python number (the device copy is the optimizer\'s own)')
        _check_hyper(lr, betas, eps, weight_decay)
        if len(params) != len(bucket.params) or any(a is not b for a, b in zip(params, bucket.params)):
            raise ValueError('BucketAdam: the parameters must be exactly bucket.params (same tensors, same order)')
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != bucket.flat.device:
                raise ValueError('BucketAdam: contiguous fp32 parameters on the bucket\'s device only')
        self.bucket = bucket
        self._params: List[torch.nn.Parameter] = params
        super().__init__(params, _adam_defaults(float(lr), (float(betas[0]), float(betas[1])), float(eps),
                                                float(weight_decay)))
        dev = bucket.flat.device
        n = bucket.flat.numel()
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        # struct tmpnn_adam_state: fp64 lr, fp32 step count, int32 ticket
        self._dev_state = torch.zeros(2, dtype=torch.float64, device=dev)
        self._lr_dev = self._dev_state[0]
        self._step_dev = self._dev_state.view(torch.float32)[2]
        self._lr_pushed: Optional[float] = None
        o = 0
        for p in params:
            k = p.numel()
            self.state[p] = dict(step=self._step_dev, exp_avg=self.exp_avg[o:o + k].view_as(p),
                                 exp_avg_sq=self.exp_avg_sq[o:o + k].view_as(p))
            o += k
        self._segs_host = self._work_host = None
        self._segs = self._work = self._stats = None
        self._calls = 0
        self._f_step = None

    # ---- torch.optim.Optimizer's surface ------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError('BucketAdam: one parameter group only')
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none: bool = True) -> None:
        """`bucket.zero()` whatever the argument: p.grad must keep aliasing the bucket (reference train.py:62 as written)."""
        self.bucket.zero()

    def state_dict(self):
        """torch.optim.Adam's format: per parameter `step` (an fp32 scalar on the host, as torch's default keeps it),
        `exp_avg`, `exp_avg_sq` (copies shaped like the parameter); the group's hyper-parameters."""
        sd = super().state_dict()
        step = self._step_dev.detach().cpu()
        sd['state'] = {i: dict(step=step.clone(), exp_avg=st['exp_avg'].detach().clone(),
                               exp_avg_sq=st['exp_avg_sq'].detach().clone()) for i, st in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        """A state_dict of a BucketAdam or of a torch.optim.Adam over the same parameters.  The values are copied INTO the flat
        buffers and the device record (their addresses may be baked into a captured graph)."""
        groups = state_dict['param_groups']
        if len(groups) != 1:
            raise ValueError(f'BucketAdam.load_state_dict: one parameter group only ({len(groups)} given)')
        g = dict(groups[0])
        ids = list(g.pop('params'))
        if len(ids) != len(self._params):
            raise ValueError(f'BucketAdam.load_state_dict: {len(ids)} parameters in the state, {len(self._params)} here')
        for k in _REFUSED:
            if g.get(k):
                raise ValueError(f'BucketAdam.load_state_dict: {k}={g[k]!r} is not supported')
        lr = g.get('lr', self.param_groups[0]['lr'])
        if isinstance(lr, torch.Tensor):
            g['lr'] = lr = float(lr)
        betas = g.get('betas', self.param_groups[0]['betas'])
        _check_hyper(lr, betas, g.get('eps', self.param_groups[0]['eps']),
                     g.get('weight_decay', self.param_groups[0]['weight_decay']))
        state = state_dict['state']
        steps = set()
        entries = []
        for pid, p in zip(ids, self._params):
            st = state.get(pid)
            if st is None:
                entries.append(None)
                steps.add(0.0)
                continue
            for k in ('exp_avg', 'exp_avg_sq'):
                if tuple(st[k].shape) != tuple(p.shape):
                    raise ValueError(f'BucketAdam.load_state_dict: {k} of parameter {pid} is {tuple(st[k].shape)}, '
                                     f'the parameter {tuple(p.shape)}')
            entries.append(st)
            steps.add(float(st['step']))
        if len(steps) != 1:
            raise ValueError(f'BucketAdam.load_state_dict: the parameters are at different steps {sorted(steps)}; '
                             'one step count serves the whole bucket')
        with torch.no_grad():
            for st, p in zip(entries, self._params):
                mine = self.state[p]
                if st is None:
                    mine['exp_avg'].zero_()
                    mine['exp_avg_sq'].zero_()
                else:
                    mine['exp_avg'].copy_(st['exp_avg'])
                    mine['exp_avg_sq'].copy_(st['exp_avg_sq'])
            self._step_dev.fill_(steps.pop())
        self.param_groups[0].update(g)
        self._lr_pushed = None
        if bucket_on_gpu(self.bucket):
            self.push_hyper()

    # ---- the device side ----------------------------------------------------------------------------------------------------
    def push_hyper(self) -> None:
        """Write the group's learning rate to the device record if it changed (a scheduler stepped).  One fill, no read."""
        lr = self.param_groups[0]['lr']
        if lr != self._lr_pushed:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('BucketAdam: the learning rate changed inside a capture; call push_hyper() before it')
            self._lr_dev.fill_(float(lr))
            self._lr_pushed = lr

    def _need_gpu(self, what: str) -> None:
        if not bucket_on_gpu(self.bucket):
            raise RuntimeError(f'BucketAdam.{what} on {self.bucket.flat.device}: trackmpnn_amd runs on the MI355X HIP kernels '
                               'only (no CPU or torch fallback exists)')

    def _tables(self) -> None:
        """(Re)build the segment table and the work list and copy them to the device."""
        self._segs_host = segment_table(self.bucket)
        self._work_host = work_list(self._segs_host[:, 2])
        dev = self.bucket.flat.device
        self._segs = torch.from_numpy(self._segs_host).to(dev)
        self._work = torch.from_numpy(self._work_host).to(dev)
        self._ptr_key = (int(self._segs_host[0, 0]), int(self._segs_host[-1, 0]), self.bucket.flat.data_ptr())
        if self._f_step is None:
            self._f_step, self._f_flow = _lib.fn('tmpnn_adam_step'), _lib.fn('tmpnn_grad_flow')

    def _check(self, full: bool) -> None:
        """p.grad must alias the bucket and the parameters must live where the segment table says: first and last parameter
        on every step, all of them every _FULL_CHECK_EVERY steps."""
        ps, flat = self._params, self.bucket.flat
        g0, g1 = ps[0].grad, ps[-1].grad
        fp = flat.data_ptr()
        ok = (g0 is not None and g1 is not None and g0.data_ptr() == fp
              and g1.data_ptr() == fp + 4 * (flat.numel() - ps[-1].numel()))
        if ok and full:
            ok = self.bucket.check_alias()
        if not ok:
            raise RuntimeError('BucketAdam.step: parameter gradients no longer alias the bucket (use opt.zero_grad() or '
                               'bucket.zero(); zero_grad(set_to_none=True) of the MODULE replaces them)')
        moved = self._segs is None or self._ptr_key != (ps[0].data_ptr(), ps[-1].data_ptr(), fp)
        if not moved and full:
            moved = any(p.data_ptr() != int(a) for p, a in zip(ps, self._segs_host[:, 0]))
        if moved:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('BucketAdam.step: parameter storage moved; take one step outside the capture first')
            self._tables()

    def step(self, grad_scale: float = 1.0, zero_grads: bool = False, closure=None):
        """One Adam step in one launch.  grad_scale multiplies the gradient first (1 / world after
        `allreduce_grads(..., average=False)`, 1 / B for the mean over B chunks), zero_grads clears the bucket behind the
        read.  No host synchronisation, no allocation."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._need_gpu('step')
        g = self.param_groups[0]
        if g['lr'] != self._lr_pushed:
            self.push_hyper()
        self._check(full=self._calls % _FULL_CHECK_EVERY == 0)
        self._calls += 1
        flat = self.bucket.flat
        b1, b2 = g['betas']
        rc = self._f_step(self._segs.data_ptr(), self._segs.shape[0], self._work.data_ptr(), self._work.shape[0],
                          flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), flat.numel(),
                          self._dev_state.data_ptr(), b1, b2, g['eps'], g['weight_decay'], grad_scale, 1 if zero_grads else 0,
                          _lib.raw_stream(flat.device))
        if rc != 0:
            raise RuntimeError(f'tmpnn_adam_step failed (code {rc}): {_lib.last_error()}')
        # the kernel wrote through raw pointers: move the version counters, so that every cache keyed by them (the fused path's
        # operand images, the zero-padded copies, the gradient sink) sees new weights
        torch.autograd.graph.increment_version(self._params)
        return loss

    def grad_flow(self):
        """(names, stats): per parameter of the bucket mean |g|, max |g| and the number of non-finite elements, as an fp64
        [P, 3] DEVICE tensor from one launch (read it when you plot; call this before a step that zeroes the bucket).
        names: `model.named_parameters()` in bucket order when the optimizer was given the module."""
        self._need_gpu('grad_flow')
        self._check(full=True)
        if self._stats is None:
            self._stats = torch.empty((len(self._params), 3), dtype=torch.float64, device=self.bucket.flat.device)
        flat = self.bucket.flat
        _lib.call('tmpnn_grad_flow', self._segs.data_ptr(), self._segs.shape[0], flat.data_ptr(), flat.numel(),
                  self._stats.data_ptr(), _lib.raw_stream(flat.device))
        return self.names(), self._stats

    def names(self) -> List[str]:
        if self.model is not None:
            by_id = {id(p): n for n, p in self.model.named_parameters()}
            return [by_id[id(p)] for p in self._params]
        return [f'param{i}' for i in range(len(self._params))]


def bucket_on_gpu(bucket: GradBucket) -> bool:
    return bucket.flat.device.type == 'cuda'


def _check_hyper(lr, betas, eps, weight_decay) -> None:
    if not 0.0 <= float(lr):
        raise ValueError(f'Invalid learning rate: {lr}')
    if not 0.0 <= float(eps):
        raise ValueError(f'Invalid epsilon value: {eps}')
    if len(betas) != 2 or not 0.0 <= float(betas[0]) < 1.0 or not 0.0 <= float(betas[1]) < 1.0:
        raise ValueError(f'Invalid betas: {betas}')
    if not 0.0 <= float(weight_decay):
        raise ValueError(f'Invalid weight_decay value: {weight_decay}')
