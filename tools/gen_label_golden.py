"""Record what the reference's get_track_ids (dataset/kitti_mot.py:422-486, dataset/bdd100k_mot.py:407-470) gives on seeded
synthetic frames, and time it.

    python tools/gen_label_golden.py --reference-path DIR --out tests/golden/label [--time]

DIR is a checkout of the reference.  Its dataset.kitti_mot and dataset.bdd100k_mot are imported as they are, under stub modules
for what their imports need and get_track_ids does not use: cv2, PIL, torchvision(.transforms), models.espv2(.SegmentationModel)
with an EESPNet_Seg attribute, models.dla(.pose_dla_dcn) with get_pose_net.  KittiMOTDataset.get_track_ids(None, pred, gt) (and
the BDD one) is called frame by frame on the frames of trackmpnn_amd.labeling.synth_label_sequence, as float32 16-column rows in
the reference's layout (frame, track, category, alpha, x1, y1, x2, y2, ..., score) with the row's own index written into the
unused alpha column, so that the rows that survive can be identified.  Each case is written as label_<name>.npz: the inputs
(the DetectionLabeler fields), which rule set, and the reference's keep / track per detection and gt_keep per GT row.

The tool asserts, for every frame without exception, that the IoU values >= iou_thresh of the detections against the GT rows
that are not ignore rows are pairwise distinct: that is the condition under which the reference's own order is defined (its
argsort is unstable).  Change the seed, not the condition, if one turns up.  It also asserts that assigned, unassigned-but-kept
and removed detections each make up between 10 % and 90 %.

--time: the reference's function alone, on this machine's CPU cores, over the frames of the two sets profiles/label_dets.md
quotes (tools/label_dets_bench.py builds the same sets from the same seeds).

The fixtures live in a directory of their own: tests/conftest.py takes every .npz directly under tests/golden for a model
fixture.  They are data; nothing of the reference's text is copied here."""
import argparse
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYS = ('det_frame', 'det_cat', 'det_box', 'det_score', 'gt_frame', 'gt_track', 'gt_cat', 'gt_box')
# name -> (rule set, seed, frames)
CASES = {'kitti_a': ('kitti', 101, 40), 'kitti_b': ('kitti', 202, 44), 'bdd': ('bdd', 303, 40)}


def reference_functions(path):
    """{'kitti': get_track_ids, 'bdd': get_track_ids} of the reference's two dataset classes (unbound: self is not used)."""
    def stub(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    stub('cv2')
    stub('PIL')
    stub('torchvision', transforms=stub('torchvision.transforms'))
    sys.path.insert(0, path)
    import models                                                   # the reference's package; the two networks are stubbed
    stub('models.espv2', SegmentationModel=stub('models.espv2.SegmentationModel', EESPNet_Seg=None))
    stub('models.dla', pose_dla_dcn=stub('models.dla.pose_dla_dcn', get_pose_net=None))
    from dataset.bdd100k_mot import BDD100kMOTDataset
    from dataset.kitti_mot import KittiMOTDataset
    return {'kitti': KittiMOTDataset.get_track_ids, 'bdd': BDD100kMOTDataset.get_track_ids}


def rows16(frame, track, cat, box, score):
    r = np.zeros((frame.shape[0], 16), np.float32)
    r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4:8], r[:, 15] = frame, track, cat, np.arange(frame.shape[0]), box, score
    return r


def frame_rows(q, t):
    d, g = np.where(q['det_frame'] == t)[0], np.where(q['gt_frame'] == t)[0]
    pred = rows16(q['det_frame'][d], np.full(d.shape[0], -1), q['det_cat'][d], q['det_box'][d], q['det_score'][d])
    gt = rows16(q['gt_frame'][g], q['gt_track'][g], q['gt_cat'][g], q['gt_box'][g], np.zeros(g.shape[0]))
    return d, g, pred, gt


def reference_labels(fn, q, rules, check_ties=True):
    """(keep, track, gt_keep) of the reference over the frames of q."""
    from trackmpnn_amd.labeling import label_overlaps_host
    keep, track = np.zeros(q['det_frame'].shape[0], bool), np.full(q['det_frame'].shape[0], -1, np.int64)
    gt_keep = np.zeros(q['gt_frame'].shape[0], bool)
    for t in range(q['num_frames']):
        d, g, pred, gt = frame_rows(q, t)
        if check_ties and d.size and g.size:
            real = (q['gt_cat'][g] != rules.iom_ignore_cat) & (q['gt_cat'][g] != rules.iou_ignore_cat)
            v = label_overlaps_host(q['det_box'][d], q['gt_box'][g][real])[0].ravel()
            v = v[v >= np.float32(rules.iou_thresh)]
            assert np.unique(v).shape[0] == v.shape[0], f'frame {t}: two equal IoU values >= {rules.iou_thresh}: change the seed'
        out_pred, out_gt = fn(None, pred.copy(), gt.copy())
        i, j = out_pred[:, 3].astype(np.int64), out_gt[:, 3].astype(np.int64)
        keep[d[i]], track[d[i]], gt_keep[g[j]] = True, out_pred[:, 1].astype(np.int64), True
    return keep, track, gt_keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join('tests', 'golden', 'label'))
    ap.add_argument('--time', action='store_true')
    a = ap.parse_args()
    from trackmpnn_amd.labeling import BDD_RULES, KITTI_RULES, label_detections_host, synth_label_sequence
    rule_sets = {'kitti': KITTI_RULES, 'bdd': BDD_RULES}
    fns = reference_functions(a.reference_path)
    os.makedirs(a.out, exist_ok=True)
    for name, (rs, seed, frames) in CASES.items():
        rules = rule_sets[rs]
        q = synth_label_sequence(seed, frames, rules)
        keep, track, gt_keep = reference_labels(fns[rs], q, rules)
        n = keep.shape[0]
        shares = {'assigned': (track >= 0).sum() / n, 'unassigned, kept': (keep & (track < 0)).sum() / n, 'removed': (~keep).sum() / n}
        assert all(0.1 < v < 0.9 for v in shares.values()), shares
        ours = label_detections_host([q], rules)[0]
        same = (np.array_equal(ours['keep'], keep) and np.array_equal(np.where(keep, ours['track'], -1), track)
                and np.array_equal(ours['gt_keep'], gt_keep))
        out = {k: q[k] for k in KEYS}
        out.update(num_frames=np.int64(q['num_frames']), width=np.int64(q['width']), rules=np.asarray(rs),
                   ref_keep=keep, ref_track=track, ref_gt_keep=gt_keep)
        path = os.path.join(a.out, f'label_{name}.npz')
        np.savez_compressed(path, **out)
        print(f'{path}: {os.path.getsize(path)} bytes, {frames} frames, {n} detections, {gt_keep.shape[0]} GT rows, '
              + ', '.join(f'{k} {v:.3f}' for k, v in shares.items()) + f'; label_detections_host equal: {same}')
    if a.time:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from label_dets_bench import SETS, build_set
        for name in SETS:
            rs, seqs = build_set(name)
            rules, fn = rule_sets[rs], fns[rs]
            frames = [frame_rows(q, t)[2:] for q in seqs for t in range(q['num_frames'])]
            t0 = time.perf_counter()
            for pred, gt in frames:
                fn(None, pred, gt)
            dt = time.perf_counter() - t0
            print(f'{name}: the reference\'s get_track_ids over {len(frames)} frames ({sum(p.shape[0] for p, _ in frames)} detections): '
                  f'{dt:.2f} s on this machine\'s CPU ({1e6 * dt / len(frames):.0f} us a frame)')


if __name__ == '__main__':
    main()
