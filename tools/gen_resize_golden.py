#!/usr/bin/env python
"""Write tests/golden/resize/*.npz: random source frames and Pillow's bilinear resize of them, at the small sizes of
tests/test_frame_resize_gpu.py.  Needs Pillow (run where it is installed; the tests only read the files).

    python tools/gen_resize_golden.py

Every file holds `src` uint8 [n, h, w, 3], `out` uint8 [n, H, W, 3] = Image.resize((W, H), Image.BILINEAR) of every frame
(what transforms.Resize((H, W)) calls on a PIL image), and `pillow`: the version that wrote it.  The frames of a case are: random
bytes, all 255 (the accumulator's top), and columns alternating 0 / 255."""
import os

import numpy as np

# (h, w) -> (H, W)
CASES = [((37, 61), (48, 80)), ((50, 70), (20, 33)), ((23, 45), (33, 7)), ((9, 9), (9, 17)), ((9, 17), (5, 17)),
         ((64, 64), (64, 64)), ((3, 2), (11, 5)), ((5, 300), (1, 7))]
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'resize')


def case_name(hw, HW) -> str:
    return f'{hw[0]}x{hw[1]}_to_{HW[0]}x{HW[1]}'


def source_frames(hw, seed: int) -> np.ndarray:
    h, w = hw
    rng = np.random.default_rng(seed)
    stripes = np.zeros((h, w, 3), np.uint8)
    stripes[:, 1::2] = 255
    return np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.full((h, w, 3), 255, np.uint8), stripes])


def main() -> None:
    import PIL
    from PIL import Image
    os.makedirs(OUT, exist_ok=True)
    for k, (hw, HW) in enumerate(CASES):
        src = source_frames(hw, 1000 + k)
        out = np.stack([np.asarray(Image.fromarray(f).resize((HW[1], HW[0]), Image.BILINEAR)) for f in src])
        path = os.path.join(OUT, case_name(hw, HW) + '.npz')
        np.savez_compressed(path, src=src, out=out, pillow=np.array(PIL.__version__))
        print(f'{path}: src {src.shape} -> out {out.shape}, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
