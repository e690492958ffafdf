#!/usr/bin/env python
"""Record the gradients of the embedding CNN's decoder from the reference implementation (run by hand; no test uses this tool).

    python tools/gen_espnet_grad_golden.py --reference-path /path/to/TrackMPNN --out tests/golden/espnet_grad

Imports the reference's models.espv2.SegmentationModel.EESPNet_Seg as it is (pretrained=None, on the CPU, .eval()), loads the
seeded weights of tests/espnet_cases.py with strict=True, sets requires_grad on the 36 decoder tensors alone, cuts the graph at
the four encoder outputs (a wrapper around the encoder's forward, at run time) and back-propagates sum(out * d_maps) with the
d_maps of tests/espnet_grad_cases.py.  Stored per case and form: the gradients of the .double() module (float64, split over files
below the size limit), per tensor e_ref = max |g32 - g64| of the float32 module and gmax = max |g64|.  No weights and none of the
reference's text are stored.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.espnet_cases import CASES, case_images, espnet_weights, weight_sum   # noqa: E402
from tests.espnet_grad_cases import GRAD_CASES, TAPS, case_d_maps               # noqa: E402
from trackmpnn_amd.espnet import decoder_param_names                            # noqa: E402

MAX_BYTES = 1_000_000
PART_BYTES = 700_000           # raw float64 bytes of one part (random mantissas do not compress)


def reference_grads(EESPNet_Seg, sd, C, images, d_maps, dtype, check_signs):
    net = EESPNet_Seg(classes=C, s=1, pretrained=None).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(dtype)
    names = decoder_param_names(C)
    params = dict(net.named_parameters())
    assert sorted(k for k in params if not k.startswith('net.')) == sorted(names)
    for k, p in params.items():
        p.requires_grad_(k in names)
    cut = []
    encoder = net.net.forward

    def encoder_cut(*a, **kw):
        cut[:] = [t.detach().requires_grad_(True) for t in encoder(*a, **kw)]
        return tuple(cut)

    net.net.forward = encoder_cut
    signs, hooks = {}, []
    for mod_name, mod in net.named_modules():
        if isinstance(mod, torch.nn.PReLU) and not mod_name.startswith('net.'):
            def hook(m, inp, out, key=mod_name):
                signs[key] = (bool((inp[0] > 0).any()), bool((inp[0] < 0).any()))
            hooks.append(mod.register_forward_hook(hook))
    out = net(torch.from_numpy(images).to(dtype))
    for h in hooks:
        h.remove()
    if check_signs:
        decoder_acts = sorted(k for k, m in net.named_modules() if isinstance(m, torch.nn.PReLU) and not k.startswith('net.'))
        assert sorted(signs) == decoder_acts, (sorted(signs), decoder_acts)
        one_sided = [k for k, (p, n) in signs.items() if not (p and n)]
        assert not one_sided, f'decoder PReLUs that saw one sign only: {one_sided}'
    (out * torch.from_numpy(d_maps).to(dtype)).sum().backward()
    g = {k: params[k].grad.detach().numpy() for k in names}
    g.update({k: t.grad.detach().numpy() for k, t in zip(TAPS, cut)})
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'espnet_grad'))
    args = ap.parse_args()
    sys.path.insert(0, args.reference_path)
    from models.espv2.SegmentationModel import EESPNet_Seg

    os.makedirs(args.out, exist_ok=True)
    torch.manual_seed(0)
    for name, form in GRAD_CASES:
        T, C, H, W, seed = CASES[name]
        sd = espnet_weights(C, seed)
        images, d_maps = case_images(name), case_d_maps(name, form)
        g32 = reference_grads(EESPNet_Seg, sd, C, images, d_maps, torch.float32, True)
        g64 = reference_grads(EESPNet_Seg, sd, C, images, d_maps, torch.float64, False)
        names = list(g64)
        assert len(names) == 40
        zero = [k for k in names if not np.any(g64[k])]
        assert not zero, f'{name} {form}: gradients that are identically zero: {zero}'
        e_ref = np.array([np.abs(g32[k].astype(np.float64) - g64[k]).max() for k in names])
        gmax = np.array([np.abs(g64[k]).max() for k in names])
        np.savez_compressed(os.path.join(args.out, f'{name}_{form}_meta.npz'), seed=np.int64(seed), C=np.int64(C),
                            wsum=np.float64(weight_sum(sd)), names=np.array(names), e_ref=e_ref, gmax=gmax)
        parts, cur, size = [], {}, 0
        for k in names:
            if cur and size + g64[k].nbytes > PART_BYTES:
                parts.append(cur)
                cur, size = {}, 0
            cur[k] = g64[k]
            size += g64[k].nbytes
        parts.append(cur)
        for i, part in enumerate(parts):
            path = os.path.join(args.out, f'{name}_{form}_part{i:02d}.npz')
            np.savez_compressed(path, **part)
            nbytes = os.path.getsize(path)
            assert nbytes < MAX_BYTES, f'{path}: {nbytes} bytes'
        units = e_ref / (2.0 ** -23 * gmax)
        print(f'{name} {form}: T={T} C={C} {H}x{W}  {len(parts)} parts  e_ref / (2^-23 gmax): {units.min():.2f} .. {units.max():.2f}')


if __name__ == '__main__':
    main()
