"""Seeded weights and the recorded fixtures of the embedding CNN (tests/test_espnet.py, tests/test_espnet_gpu.py,
tools/gen_espnet_golden.py).

The default initialisation would hide a wrong channel index: every BatchNorm is the identity and every PReLU slope 0.25.  So every
tensor is drawn from numpy.random.default_rng(seed), in the order of trackmpnn_amd.espnet.espnet_spec(C):
    conv weights    uniform in +-sqrt(3 / fan_in): unit gain, activations stay O(1) through the ~40 layers
    BN weight, running_var      uniform in [0.5, 1.5]
    BN bias, running_mean       uniform in +-0.3
    PReLU slopes    uniform in [0.05, 0.5], distinct per channel
The fixtures under tests/golden/espnet hold no weights: a test regenerates them from the seed and checks `wsum`.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'espnet')

# name -> (T, C, H, W, seed): the smallest shapes at which each kernel can go wrong.  A seed is kept only if the generating tool's
# assertions hold for it (with seeds 101, 104 and 106 the 2 x 2 or 2 x 4 reinforcement map of a 16-row case reaches one PReLU with one sign only).
CASES = OrderedDict([
    ('c1_16x16', (1, 8, 16, 16, 102)),      # level 4 is 1 x 1: every dilation exceeds the map, bilinear from one pixel
    ('c2_32x64', (1, 8, 32, 64, 101)),      # non-square: the reinforcement pyramid is keyed on height
    ('c3_48x80', (1, 8, 48, 80, 103)),      # level 4 is 3 x 5: odd sizes at the stride-2 and pool borders, PSP 6x10 -> .. -> 1x1
    ('c4_batch3', (3, 8, 16, 32, 105)),     # batch indexing
    ('c5_c128', (1, 128, 16, 32, 107)),     # the real channel count
])
TAPS = ('out_l1', 'out_l2', 'out_l3', 'out_l4')


def espnet_weights(C, seed):
    """The seeded state dict of EESPNet_Seg(classes=C, s=1): float32 tensors, num_batches_tracked (0) included, so that the
    reference module loads it with strict=True."""
    from trackmpnn_amd.espnet import espnet_spec
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k, shp in espnet_spec(C).items():
        if k.endswith('conv.weight'):
            fan_in = shp[1] * shp[2] * shp[3]
            v = rng.uniform(-1.0, 1.0, shp) * np.sqrt(3.0 / fan_in)
        elif k.endswith('bn.weight') or k.endswith('running_var'):
            v = rng.uniform(0.5, 1.5, shp)
        elif k.endswith('bn.bias') or k.endswith('running_mean'):
            v = rng.uniform(-0.3, 0.3, shp)
        else:
            assert k.endswith('act.weight'), k
            v = rng.uniform(0.05, 0.5, shp)
        sd[k] = torch.from_numpy(v.astype(np.float32))
        if k.endswith('running_var'):
            sd[k[:-len('running_var')] + 'num_batches_tracked'] = torch.tensor(0, dtype=torch.int64)
    return sd


def weight_sum(sd):
    """The guard a fixture records: the float64 sum of squares over every float tensor of the state dict."""
    return float(sum((v.double() ** 2).sum().item() for v in sd.values() if v.dtype.is_floating_point))


def case_images(name):
    T, _, H, W, seed = CASES[name]
    return np.random.default_rng(seed + 1000).standard_normal((T, 3, H, W)).astype(np.float32)


_cache = {}


def load_case(name):
    """(fixture arrays, seeded state dict) of a case, read once per process."""
    if name not in _cache:
        fx = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
        sd = espnet_weights(int(fx['C']), int(fx['seed']))
        assert abs(weight_sum(sd) - float(fx['wsum'])) <= 1e-9 * float(fx['wsum']), 'the seeded weights are not the fixture\'s'
        _cache[name] = (fx, sd)
    return _cache[name]
