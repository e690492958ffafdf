"""The recorded gradients of the embedding CNN's decoder (tests/test_espnet_train.py, tests/test_espnet_train_gpu.py,
tools/gen_espnet_grad_golden.py).

Weights and images are the seeded ones of tests/espnet_cases.py.  d_maps, the gradient handed to the net's output, comes from
numpy.random.default_rng(seed + 2000): standard_normal(out.shape) rounded to float32 (what a device test can hand over exactly),
    dense       as it is
    sparse      what VisHead's backward hands over: 5 pixels, drawn next from the same generator by choice(T H W, 5,
                replace=False), keep all their channels; everything else is zero
The fixtures under tests/golden/espnet_grad hold, per case and form, the gradients of the reference module in .double() for the 36
decoder tensors and the four encoder taps (float64, split over files below the size limit of a committed file), and per tensor
e_ref = max |g32 - g64| of the float32 module and gmax = max |g64|.  No weights are stored: `wsum` guards the seed.
"""
import glob
import os

import numpy as np

from tests.espnet_cases import CASES, espnet_weights, weight_sum

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'espnet_grad')
TAPS = ('out_l1', 'out_l2', 'out_l3', 'out_l4')
N_CENTRES = 5

# (case, form): the smallest shapes at which each kernel can go wrong (tests/espnet_cases.py says why)
GRAD_CASES = (('c1_16x16', 'dense'), ('c1_16x16', 'sparse'), ('c3_48x80', 'dense'), ('c3_48x80', 'sparse'),
              ('c4_batch3', 'dense'), ('c4_batch3', 'sparse'), ('c5_c128', 'dense'))


def case_d_maps(name, form):
    """d_maps [T, C, H, W] float32 of a case (module docstring)."""
    T, C, H, W, seed = CASES[name]
    rng = np.random.default_rng(seed + 2000)
    d = rng.standard_normal((T, C, H, W)).astype(np.float32)
    if form == 'dense':
        return d
    assert form == 'sparse', form
    pix = rng.choice(T * H * W, N_CENTRES, replace=False)
    keep = np.zeros(T * H * W, dtype=bool)
    keep[pix] = True
    keep = keep.reshape(T, 1, H, W)
    return np.where(keep, d, np.float32(0.0))


_cache = {}


def load_grad_case(name, form):
    """({tensor name: g64}, {tensor name: e_ref}, {tensor name: gmax}, seeded state dict) of a case and form, read once per process."""
    key = (name, form)
    if key not in _cache:
        meta = dict(np.load(os.path.join(GOLDEN, f'{name}_{form}_meta.npz')))
        sd = espnet_weights(int(meta['C']), int(meta['seed']))
        assert abs(weight_sum(sd) - float(meta['wsum'])) <= 1e-9 * float(meta['wsum']), 'the seeded weights are not the fixture\'s'
        names = [str(n) for n in meta['names']]
        g64 = {}
        for path in sorted(glob.glob(os.path.join(GOLDEN, f'{name}_{form}_part*.npz'))):
            with np.load(path) as part:
                for k in part.files:
                    g64[k] = part[k]
        assert sorted(g64) == sorted(names), 'the parts do not hold the tensors the meta file names'
        e_ref = dict(zip(names, (float(v) for v in meta['e_ref'])))
        gmax = dict(zip(names, (float(v) for v in meta['gmax'])))
        _cache[key] = (g64, e_ref, gmax, sd)
    return _cache[key]
