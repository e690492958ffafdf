#!/usr/bin/env python
"""Record the fixtures of the embedding CNN from the reference implementation (run by hand; no test uses this tool).

    python tools/gen_espnet_golden.py --reference-path /path/to/TrackMPNN --out tests/golden/espnet

Imports the reference's models.espv2.SegmentationModel.EESPNet_Seg as it is (pretrained=None, on the CPU), loads the seeded
weights of tests/espnet_cases.py with strict=True, and stores per case: seed, C, wsum (the weights' sum of squares), images,
ref_out32 (the float32 forward), ref_out64 (the .double() forward) and the encoder taps out_l1 .. out_l4 in float64.  No weights
and none of the reference's text are stored.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.espnet_cases import CASES, TAPS, case_images, espnet_weights, weight_sum   # noqa: E402

MAX_BYTES = 1_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'espnet'))
    args = ap.parse_args()
    sys.path.insert(0, args.reference_path)
    from models.espv2.SegmentationModel import EESPNet_Seg

    os.makedirs(args.out, exist_ok=True)
    torch.manual_seed(0)
    for name, (T, C, H, W, seed) in CASES.items():
        sd = espnet_weights(C, seed)
        net = EESPNet_Seg(classes=C, s=1, pretrained=None).eval()
        net.load_state_dict(sd, strict=True)
        assert len(net.state_dict()) == len(sd)
        images = torch.from_numpy(case_images(name))
        signs, hooks = {}, []
        for mod_name, mod in net.named_modules():
            if isinstance(mod, torch.nn.PReLU):
                def hook(m, inp, out, key=mod_name):
                    signs[key] = (bool((inp[0] > 0).any()), bool((inp[0] < 0).any()))
                hooks.append(mod.register_forward_hook(hook))
        with torch.no_grad():
            out32 = net(images)
            for h in hooks:
                h.remove()
            never = sorted(k for k, m in net.named_modules() if isinstance(m, torch.nn.PReLU) and k not in signs)
            # (the stride-2 EESP of a DownSampler returns before its own PReLU)
            assert never == ['net.level2_0.eesp.module_act', 'net.level3_0.eesp.module_act', 'net.level4_0.eesp.module_act'], never
            one_sided = [k for k, (p, n) in signs.items() if not (p and n)]
            assert not one_sided, f'{name}: PReLUs that saw one sign only: {one_sided}'
            net64 = net.double()
            out64 = net64(images.double())
            taps = net64.net(images.double(), seg=True)
        std = float(out64.std())
        assert 1e-2 <= std <= 1e2, f'{name}: output std {std}'
        fx = {'seed': np.int64(seed), 'C': np.int64(C), 'wsum': np.float64(weight_sum(sd)), 'images': images.numpy(),
              'ref_out32': out32.numpy(), 'ref_out64': out64.numpy()}
        for k, t in zip(TAPS, taps):
            fx[k] = t.numpy()
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, f'{path}: {size} bytes'
        e_ref = float(np.abs(out32.numpy().astype(np.float64) - out64.numpy()).max())
        print(f'{name}: T={T} C={C} {H}x{W}  std={std:.3f}  max|out|={float(out64.abs().max()):.3f}  e_ref={e_ref:.3e}  {size} bytes')


if __name__ == '__main__':
    main()
