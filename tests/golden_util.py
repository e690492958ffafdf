"""Helpers to read the golden fixtures written by oracle/gen_golden.py."""
import glob
import json
import os

import numpy as np
import torch

from tests.conftest import GOLDEN_DIR


class _Parts:
    """The arrays of several .npz files of one fixture behind NpzFile's `files` / [] interface."""

    def __init__(self, npzs):
        self._of = {k: z for z in npzs for k in z.files}
        self.files = list(self._of)

    def __getitem__(self, key):
        return self._of[key][key]


class Golden:
    def __init__(self, name):
        self.d = np.load(os.path.join(GOLDEN_DIR, name + '.npz'))
        # a fixture too large for one committed file (< 1 MiB each) keeps some arrays in parts/<name>.<part>.npz
        parts = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'parts', name + '.*.npz')))
        if parts:
            self.d = _Parts([self.d] + [np.load(f) for f in parts])
        self.meta = json.loads(str(self.d['meta']))
        self.ncalls = self.meta['ncalls']

    def params(self, prefix='param/'):
        return {k[len(prefix):]: torch.from_numpy(self.d[k].copy()) for k in self.d.files if k.startswith(prefix)}

    def grads(self):
        return self.params('grad/')

    def final_buffers(self):
        return self.params('final/')

    def t(self, key):
        return torch.from_numpy(np.asarray(self.d[key]).copy())

    def has(self, key):
        return key in self.d.files

    def adjacency(self, c, which, device='cpu'):
        """Rebuild the adjacency exactly as the reference produced it (dense on the first
        CPU call, otherwise a sparse COO tensor with its original, possibly uncoalesced, entries)."""
        pre = f'c{c}/{which}'
        N = int(self.d[f'c{c}/N'])
        idx = torch.from_numpy(self.d[pre + '_idx'].copy())
        val = torch.from_numpy(self.d[pre + '_val'].copy())
        if int(self.d[pre + '_dense']):
            a = torch.zeros(N, N)
            a[idx[0], idx[1]] = val
            return a.to(device)
        return torch.sparse_coo_tensor(idx, val, (N, N)).to(device)


def chunk_tp(gold: Golden) -> bool:
    """The mode of a chunk_* fixture: True = the default --tp-classifier, False = --no-tp-classifier (train.py:80-85)."""
    return bool(gold.meta.get('tp_classifier', True))


def assert_chunk_grads(model, gold: Golden):
    """Every parameter gradient of a chunk_* fixture within 2e-4 of the fixture's largest gradient entry; a parameter whose
    reference gradient is all zero (the node output head without the TP classifier) holds a zero tensor, not None."""
    import numpy as np
    gmax = max(float(np.abs(gold.d['grad/' + k]).max()) for k, _ in model.named_parameters())
    zero = []
    for k, p in model.named_parameters():
        ref = gold.t('grad/' + k)
        assert p.grad is not None, f'{k}: no gradient'
        err = float((p.grad.cpu() - ref).abs().max())
        assert err <= 2e-4 * gmax, (k, err, gmax)
        if not ref.any():
            zero.append(k)
            assert p.grad.shape == ref.shape and not p.grad.any(), f'{k}: the reference gradient is zero'
    heads = {'output_transform_node.weight', 'output_transform_node.bias'}
    assert (heads <= set(zero)) == (not chunk_tp(gold)), zero


def assert_chunk_buffers(model, gold: Golden):
    """BatchNorm buffers after the chunk against the fixture's buf_after/ (1e-5 of the largest entry; counters exact)."""
    for k, b in model.named_buffers():
        ref = gold.t('buf_after/' + k)
        if b.dtype.is_floating_point:
            assert float((b.cpu() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), k
        else:
            assert int(b) == int(ref), k


class LossTermsRecorder:
    """Context manager: records every call of trackmpnn_amd.loops._loss_terms inside train_chunk -- its arguments by NAME
    (bound to the function's own signature, so a change in their order does not pass unnoticed) and what it returned.
    `calls`: one dict per forward with det_row, edge_row, scores, tp_classifier, loss_c, loss_f (detached) and targets (None unless asked for)."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        import inspect
        from trackmpnn_amd import loops
        self._loops, self._orig = loops, loops._loss_terms
        sig = inspect.signature(self._orig)

        def rec(*a, **k):
            out = self._orig(*a, **k)
            arg = sig.bind(*a, **k).arguments
            fg = arg['tg'].graph.frame_graph()                  # (the row sets of THIS call: the graph grows afterwards)
            self.calls.append(dict(det_row=fg.det_row.long().clone(), edge_row=fg.edge_row.long().clone(), scores=arg['scores'].detach().reshape(-1).clone(),
                                   tp_classifier=arg['tp_classifier'], loss_c=out[0].detach(), loss_f=out[1].detach(),
                                   targets=out[2].clone() if len(out) > 2 else None))
            return out

        loops._loss_terms = rec
        return self

    def __exit__(self, *exc):
        self._loops._loss_terms = self._orig
        return False
