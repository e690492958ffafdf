"""Record what the reference's dataset classes hand out as `val` samples (dataset/kitti_mot.py:488-568, dataset/bdd100k_mot.py:473-553)
on a tiny data set this tool writes itself.

    python tools/gen_seqfeat_golden.py --reference-path DIR --out tests/golden/seqfeat

DIR is a checkout of the reference, read at generation time only.  Its dataset.kitti_mot and dataset.bdd100k_mot are imported as
they are, under stub modules for what their imports need and a `val` sample without 'vis' does not use: cv2,
torchvision(.transforms), models.espv2(.SegmentationModel) with an EESPNet_Seg attribute, models.dla(.pose_dla_dcn) with
get_pose_net.  Pillow is the real one: the sample opens every frame.

The data set, in a temporary directory: few-pixel images written with Pillow (.png for KITTI, .jpg for BDD), one detection text
file per frame, one label text file per sequence, and for KITTI the 21 sequence folders get_tracking_chunks('val') indexes (its
val sequences are folders 16, 18 and 20 of the sorted list; the others stay empty).  Then the reference's own
KittiMOTDataset(root, split='val', feats='2d' and '2d+temp', cuda=False)[i] and BDD100kMOTDataset(..., feats='2d+temp')[i] run.

Per case one seqfeat_<name>.npz holds only data: per sequence the parsed inputs (frame, cat, box, score as the text files give
them, in an order that is NOT sorted by frame -- even frames first -- but keeps the file order within a frame; the image's width
and height; num_frames; the label rows), the track ids the reference's get_track_ids assigned inside __getitem__ (the store is
fed the same ids; trackmpnn_amd.labeling.DetectionLabeler is pinned elsewhere), and the reference's outputs: `features` and
`bbox_pred[:, :2]`; and the data set's mean / std.  Nothing of the reference's text is copied here.

What the sequences cover: frames without detections at the start, in the middle and at the end; a sequence longer than
fr_range = 30 frames, so the temporal pair wraps; a sparse sequence of more than 256 frames (beyond one training chunk's list);
a sequence with one detection; for BDD a frame whose detection file is missing and detections at or below its 0.8 score cut
(dropped by the reference's loader: they are not among the parsed inputs).  Every label row overlaps one detection by far more
than the 0.5 IoU threshold and nothing else, and there are no ignore regions, so get_track_ids removes no detection and its
order is defined.

With 'vis' the reference's __getitem__ needs torchvision.transforms (Resize, ToTensor, Normalize), which is not installed where
this runs: the visual columns are pinned through trackmpnn_amd.seqfeat.sequence_vis_host, a composition of parts that
tests/golden/vis (the box-centre index, softmax and standardisation) and tests/golden/resize (the resize) pin.

The files are written with fixed zip timestamps, so a second run gives the same bytes.  They live in a directory of their own:
tests/conftest.py takes every .npz directly under tests/golden for a model fixture."""
import argparse
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KITTI_CATS = ('Pedestrian', 'Car', 'Cyclist')
BDD_CATS = ('pedestrian', 'rider', 'car', 'bus', 'truck', 'train', 'motorcycle', 'bicycle')
# data set -> [(folder, frames, (image w, h), frames with detections)]
KITTI_SEQS = [('0016', 40, (16, 6), [f for f in range(2, 38) if f not in (10, 11, 12)]),
              ('0018', 300, (14, 5), [f for f in range(3, 290) if f % 7 == 3 or f in (255, 256, 257)]),
              ('0020', 6, (16, 6), [2])]
BDD_SEQS = [('b1c66a42-6f7d68ca', 35, (16, 9), [f for f in range(1, 33) if f % 5 != 0]),
            ('b1c81faa-3df17267', 8, (12, 7), [0, 1, 2, 5])]
# name -> (data set, feats)
CASES = {'kitti_2d': ('kitti', '2d'), 'kitti_2d_temp': ('kitti', '2d+temp'), 'bdd_2d_temp': ('bdd', '2d+temp')}


def reference_classes(path):
    """{'kitti': KittiMOTDataset, 'bdd': BDD100kMOTDataset} of the reference."""
    import PIL.Image                                                # noqa: F401  the real Pillow, before anything could stub it

    def stub(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    stub('cv2')
    stub('torchvision', transforms=stub('torchvision.transforms'))
    sys.path.insert(0, path)
    import models                                                   # noqa: F401  the reference's package; the networks are stubbed
    stub('models.espv2', SegmentationModel=stub('models.espv2.SegmentationModel', EESPNet_Seg=None))
    stub('models.dla', pose_dla_dcn=stub('models.dla.pose_dla_dcn', get_pose_net=None))
    from dataset.bdd100k_mot import BDD100kMOTDataset
    from dataset.kitti_mot import KittiMOTDataset
    return {'kitti': KittiMOTDataset, 'bdd': BDD100kMOTDataset}


def synth_sequence(rng, frames, det_frames, ncat, min_score):
    """Detections (frame-sorted, file order within a frame) and label rows of one sequence; every value has two decimals, as
    the text files hold it.  The up to four detections of a frame lie in slots 300 px apart, so no two boxes overlap."""
    det, gt = [], []
    tracks = {}
    for f in det_frames:
        n = int(rng.integers(1, 5)) if len(det_frames) > 1 else 1
        for slot in rng.permutation(4)[:n]:
            x1 = round(float(slot * 300 + rng.uniform(5, 120)), 2)
            y1 = round(float(rng.uniform(100, 250)), 2)
            x2, y2 = round(x1 + float(rng.uniform(45, 160)), 2), round(y1 + float(rng.uniform(45, 110)), 2)
            cat = int(rng.integers(1, ncat + 1))
            score = round(float(rng.uniform(min_score, 1.0)), 2)
            det.append((f, cat, x1, y1, x2, y2, score))
            if rng.random() < 0.65:                                 # a label row on top of it (a jitter of at most a pixel)
                tid = tracks.setdefault((int(slot), cat), len(tracks) + 3)
                j = [round(float(v), 2) for v in rng.uniform(-1, 1, 4)]
                gt.append((f, tid, cat, round(x1 + j[0], 2), round(y1 + j[1], 2), round(x2 + j[2], 2), round(y2 + j[3], 2)))
    return det, gt


def write_dataset(root, ds, rng):
    """Writes the tiny data set under root; returns per sequence the dict of parsed inputs (what the text files hold)."""
    from PIL import Image
    kitti = ds == 'kitti'
    split_dir = 'training' if kitti else 'validation'
    names = KITTI_CATS if kitti else BDD_CATS
    specs = KITTI_SEQS if kitti else BDD_SEQS
    im_root = os.path.join(root, split_dir, 'image_02')
    det_root = os.path.join(root, split_dir, ('centertrack' if kitti else 'hin') + '_detections')
    lab_root = os.path.join(root, split_dir, 'label_02')
    os.makedirs(lab_root)
    if kitti:
        for i in range(21):
            os.makedirs(os.path.join(im_root, '%.4d' % i))
    out = []
    for folder, frames, (w, h), det_frames in specs:
        os.makedirs(os.path.join(im_root, folder), exist_ok=True)
        os.makedirs(os.path.join(det_root, folder))
        det, gt = synth_sequence(rng, frames, det_frames, len(names), 0.5 if kitti else 0.7)
        for f in range(frames):
            px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            Image.fromarray(px).save(os.path.join(im_root, folder, ('%.6d.png' if kitti else '%.4d.jpg') % f))
            rows = [d for d in det if d[0] == f]
            if not kitti and not rows and f % 2:                    # (the BDD loader takes a missing file for an empty frame)
                continue
            with open(os.path.join(det_root, folder, '%.4d.txt' % f), 'w') as fh:
                for _, cat, x1, y1, x2, y2, sc in rows:
                    fh.write('%s,%.2f,%.2f,%.2f,%.2f,%.2f\n' % (names[cat - 1], x1, y1, x2, y2, sc))
        with open(os.path.join(lab_root, folder + '.txt'), 'w') as fh:
            for f, tid, cat, x1, y1, x2, y2 in gt:
                fh.write('%d %d %s 0 0 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10\n' % (f, tid, names[cat - 1], x1, y1, x2, y2))
        # the parsed inputs: what a reader of the text files gets (BDD: its loader keeps score > 0.8 only)
        kept = [d for d in det if kitti or float('%.2f' % d[6]) > 0.8]
        a = np.asarray(kept, np.float64).reshape(-1, 7)
        g = np.asarray(gt, np.float64).reshape(-1, 7)
        out.append(dict(frame=a[:, 0].astype(np.int64), cat=a[:, 1].astype(np.int64), box=a[:, 2:6].copy(), score=a[:, 6].copy(),
                        width=np.int64(w), height=np.int64(h), num_frames=np.int64(frames), gt_frame=g[:, 0].astype(np.int64),
                        gt_track=g[:, 1].astype(np.int64), gt_cat=g[:, 2].astype(np.int64), gt_box=g[:, 3:7].copy()))
    return out


def save_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join('tests', 'golden', 'seqfeat'))
    a = ap.parse_args()
    from trackmpnn_amd.chunks import DetectionStore
    from trackmpnn_amd.seqfeat import sequence_features_host
    classes = reference_classes(a.reference_path)
    os.makedirs(a.out, exist_ok=True)
    for name, (ds, feats) in CASES.items():
        with tempfile.TemporaryDirectory() as root:
            seqs = write_dataset(root, ds, np.random.default_rng([41, 0 if ds == 'kitti' else 1]))
            data = classes[ds](root, split='val', feats=feats, cuda=False)
            assert len(data) == len(seqs)
            mean, std = data.mean.numpy().ravel(), data.std.numpy().ravel()
            out = dict(mean=mean, std=std, ncat=np.int64(len(data.class_dict)), fr_range=np.int64(data.fr_range), feats=np.asarray(feats),
                       nseq=np.int64(len(seqs)))
            store_in = []
            for i, q in enumerate(seqs):
                features, bbox_pred, _, _ = data[i]
                n = q['frame'].shape[0]
                # nothing was removed and nothing reordered: the reference's rows are the parsed rows, one for one
                assert bbox_pred.shape[0] == n and np.array_equal(bbox_pred[:, 0], q['frame']) and np.array_equal(bbox_pred[:, 2], q['cat'])
                assert np.array_equal(bbox_pred[:, 4:8], q['box'].astype(np.float32)) and np.array_equal(bbox_pred[:, 15], q['score'].astype(np.float32))
                q['track'] = bbox_pred[:, 1].astype(np.int64)
                # the stored order: even frames first, file order within a frame (the store sorts stably by frame)
                order = np.argsort(q['frame'] % 2, kind='stable')
                for k in ('frame', 'cat', 'box', 'score', 'track'):
                    q[k] = q[k][order]
                q['ref_features'] = features.numpy().astype(np.float32).reshape(n, mean.size)
                q['ref_y'] = bbox_pred[:, :2].copy()
                store_in.append(q)
                out.update({f's{i}_{k}': v for k, v in q.items()})
            store = DetectionStore(store_in, len(data.class_dict), feats, mean, std, fr_range=int(data.fr_range), device=None)
            same = all(np.array_equal(sequence_features_host(store, i).X.view(np.int32), q['ref_features'].view(np.int32))
                       and np.array_equal(sequence_features_host(store, i).y, q['ref_y'].astype(np.int64)) for i, q in enumerate(store_in))
            path = os.path.join(a.out, f'seqfeat_{name}.npz')
            save_npz(path, out)
            print(f'{path}: {os.path.getsize(path)} bytes; sequences of {[int(q["num_frames"]) for q in seqs]} frames, '
                  f'{[int(q["frame"].shape[0]) for q in seqs]} detections, {[int((q["track"] >= 0).sum()) for q in seqs]} with a track id; '
                  f'sequence_features_host equal: {same}')


if __name__ == '__main__':
    main()
