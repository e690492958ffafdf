"""Record what the reference's get_vis_feats (dataset/kitti_mot.py:391-412, dataset/bdd100k_mot.py:376-397), F.softmax with the
standardisation (kitti_mot.py:558-566) and FairMOTLoss (models/loss.py:162-181) give on seeded synthetic inputs.

    python tools/gen_vis_golden.py --reference-path DIR --out tests/golden/vis

DIR is a checkout of the reference.  Its dataset modules are imported as they are, under the stub modules tools/gen_label_golden.py
uses (cv2, PIL, torchvision(.transforms), models.espv2(.SegmentationModel), models.dla(.pose_dla_dcn)); get_vis_feats is called
unbound on a namespace that carries input_w, input_h, down_ratio and num_vis_feats.  Each case is written as vis_<name>.npz with
two parts:

    the index part   in-image float32 boxes on the real image and input sizes (KITTI 375 x 1242 and 370 x 1224 resized to
                     384 x 1280 at down_ratio 1 and 4; BDD 720 x 1280 at 4) and the (c_y, c_x) the reference indexes its map with,
                     recorded by an object that stands in for the map and notes the index (a real map at down_ratio 1 is 250 MB).
                     Boxes whose centre truncates differently when the same formula is evaluated in float64 are searched for
                     among seeded random boxes and appended (`fp64_differs`); the tool asserts that at least one case has one.
    the head part    two small maps [2, 128, 6, 10], boxes on them, track ids (some -1, some >= 128) and chunk boundaries; the
                     reference's gathered rows (through real torch maps), F.softmax of them, the standardised rows
                     (softmax - 0.5) / 0.5 and FairMOTLoss per chunk.  Every chunk holds a labelled row (the reference gives NaN
                     otherwise; that case is pinned in the tests as the library's stated choice).

The fixtures live in a directory of their own: tests/conftest.py takes every .npz directly under tests/golden for a model
fixture.  They are data; nothing of the reference's text is copied here."""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (data set, image (h, w), input (h, w), down_ratio, seed)
CASES = {'kitti_375_d4': ('kitti', (375, 1242), (384, 1280), 4, 11), 'kitti_375_d1': ('kitti', (375, 1242), (384, 1280), 1, 12),
         'kitti_370_d4': ('kitti', (370, 1224), (384, 1280), 4, 13), 'kitti_370_d1': ('kitti', (370, 1224), (384, 1280), 1, 14),
         'bdd_d4': ('bdd', (720, 1280), (720, 1280), 4, 15)}
N_BOXES = 1500            # random boxes of the index part
N_SEARCH = 400000         # boxes searched for a float64 disagreement
HEAD_MAP = (6, 10)        # the head part's maps: input (24, 40) at down_ratio 4
HEAD_INPUT, HEAD_DOWN = (24, 40), 4


def reference_classes(path):
    """{'kitti': KittiMOTDataset, 'bdd': BDD100kMOTDataset}, FairMOTLoss of the reference."""
    def stub(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    stub('cv2')
    stub('PIL')
    stub('torchvision', transforms=stub('torchvision.transforms'))
    sys.path.insert(0, path)
    import models                                                   # noqa: F401  the reference's package; the networks are stubbed
    stub('models.espv2', SegmentationModel=stub('models.espv2.SegmentationModel', EESPNet_Seg=None))
    stub('models.dla', pose_dla_dcn=stub('models.dla.pose_dla_dcn', get_pose_net=None))
    from dataset.bdd100k_mot import BDD100kMOTDataset
    from dataset.kitti_mot import KittiMOTDataset
    from models.loss import FairMOTLoss
    return {'kitti': KittiMOTDataset, 'bdd': BDD100kMOTDataset}, FairMOTLoss


class IndexRecorder:
    """Stands in for feat_maps[:, :, c_y, c_x]: notes the index."""

    def __init__(self):
        self.idx = []

    def __getitem__(self, key):
        self.idx.append((int(key[2]), int(key[3])))
        return torch.zeros(1, 128)


def random_boxes(rng, n, h, w):
    x = np.sort(rng.uniform(0, w - 1, (n, 2)), axis=1)
    y = np.sort(rng.uniform(0, h - 1, (n, 2)), axis=1)
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)


def centres64(box, im_hw, input_hw, down):
    b = box.astype(np.float64)
    cx = np.trunc(((b[:, 0] + b[:, 2]) / 2.0) * input_hw[1] / im_hw[1] / down).astype(np.int64)
    cy = np.trunc(((b[:, 1] + b[:, 3]) / 2.0) * input_hw[0] / im_hw[0] / down).astype(np.int64)
    return cy, cx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join('tests', 'golden', 'vis'))
    a = ap.parse_args()
    from trackmpnn_amd.vishead import vis_centres_host, vis_head_host
    classes, FairMOTLoss = reference_classes(a.reference_path)
    loss_fn = FairMOTLoss(128)
    os.makedirs(a.out, exist_ok=True)
    found_any = 0
    for name, (ds, im_hw, input_hw, down, seed) in CASES.items():
        rng = np.random.default_rng([seed, 77])
        cls = classes[ds]
        ns = types.SimpleNamespace(input_h=input_hw[0], input_w=input_hw[1], down_ratio=down, num_vis_feats=128)
        # ---- the index part
        box = random_boxes(rng, N_BOXES, *im_hw)
        cand = random_boxes(rng, N_SEARCH, *im_hw)
        cy32, cx32 = vis_centres_host(cand, im_hw, input_hw, down)
        cy64, cx64 = centres64(cand, im_hw, input_hw, down)
        odd = np.where((cy32 != cy64) | (cx32 != cx64))[0][:4]
        found_any += odd.size
        box = np.concatenate([box, cand[odd]])
        differs = np.concatenate([np.zeros(N_BOXES, bool), np.ones(odd.size, bool)])
        rec = IndexRecorder()
        cls.get_vis_feats(ns, rec, box, im_hw)
        ref_cy, ref_cx = (np.asarray(v, np.int64) for v in zip(*rec.idx))
        hm, wm = input_hw[0] // down, input_hw[1] // down
        assert ref_cy.min() >= 0 and ref_cx.min() >= 0 and ref_cy.max() < hm and ref_cx.max() < wm      # in-image boxes stay on the map
        ours = vis_centres_host(box, im_hw, input_hw, down)
        same_idx = np.array_equal(ours[0], ref_cy) and np.array_equal(ours[1], ref_cx)
        # ---- the head part: frames 0 and 1, three chunks
        hns = types.SimpleNamespace(input_h=HEAD_INPUT[0], input_w=HEAD_INPUT[1], down_ratio=HEAD_DOWN, num_vis_feats=128)
        maps = (2.0 * rng.standard_normal((2, 128) + HEAD_MAP)).astype(np.float32)
        counts = [(0, 9), (1, 8), (0, 7), (1, 11), (1, 6)]          # (map, detections) of consecutive frames
        offsets = np.asarray([0, 17, 35, 41], np.int64)             # chunks of two, two and one frame
        map_of = np.concatenate([np.full(n, m) for m, n in counts]).astype(np.int64)
        hbox = random_boxes(rng, map_of.shape[0], *im_hw)
        track = rng.integers(0, 300, map_of.shape[0])
        track[rng.random(map_of.shape[0]) < 0.3] = -1
        track[[0, 20, 36]] = [130, 257, 5]                           # every chunk has a labelled row, ids >= 128 occur
        feats, lo = [], 0
        for m, n in counts:
            feats.append(cls.get_vis_feats(hns, torch.from_numpy(maps[m:m + 1]), hbox[lo:lo + n], im_hw))
            lo += n
        vis = torch.cat(feats, 0)
        soft = torch.nn.functional.softmax(vis, dim=1)
        rows = (soft - 0.5) / 0.5
        labels = np.stack([map_of, track], axis=1).astype('int64')
        loss = np.asarray([float(loss_fn(vis[offsets[c]:offsets[c + 1]], labels[offsets[c]:offsets[c + 1]])) for c in range(3)])
        assert np.isfinite(loss).all()
        mean, std = np.full(128, 0.5, np.float32), np.full(128, 0.5, np.float32)
        h = vis_head_host(maps, hbox, map_of, im_hw, track, offsets, mean, std, HEAD_INPUT, HEAD_DOWN)
        h0 = vis_head_host(maps, hbox, map_of, im_hw, track, offsets, np.zeros(128, np.float32), np.ones(128, np.float32), HEAD_INPUT, HEAD_DOWN)
        # the softmax and the loss to rtol 1e-5; the standardised rows cancel against the mean, so their bound is absolute
        same_head = (np.array_equal(h[0], vis.numpy()) and np.allclose(h0[1], soft.numpy(), rtol=1e-5, atol=0)
                     and np.allclose(h[2], loss, rtol=1e-5, atol=0)
                     and (np.abs(h[1] - rows.numpy()) <= 1e-5 * (1 + np.abs(rows.numpy())) / 0.5).all())
        path = os.path.join(a.out, f'vis_{name}.npz')
        np.savez_compressed(path, im_hw=np.asarray(im_hw, np.int64), input_hw=np.asarray(input_hw, np.int64), down_ratio=np.int64(down),
                            box=box, fp64_differs=differs, ref_cy=ref_cy, ref_cx=ref_cx,
                            head_input_hw=np.asarray(HEAD_INPUT, np.int64), head_down_ratio=np.int64(HEAD_DOWN), head_maps=maps,
                            head_box=hbox, head_map_of=map_of, head_track=track.astype(np.int64), head_offsets=offsets,
                            ref_logits=vis.numpy(), ref_softmax=soft.numpy(), ref_rows=rows.numpy(), ref_loss=loss.astype(np.float32))
        print(f'{path}: {os.path.getsize(path)} bytes, {box.shape[0]} boxes ({odd.size} whose float64 centre differs), '
              f'vis_centres_host equal: {same_idx}; head part {map_of.shape[0]} rows, vis_head_host within 1e-5: {same_head}')
    assert found_any > 0, 'no box whose float64 centre truncates differently was found: raise N_SEARCH'


if __name__ == '__main__':
    main()
