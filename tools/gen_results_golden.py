"""Record what the reference's store_kitti_results (dataset/kitti_mot.py:21-73) and store_bdd100k_results
(dataset/bdd100k_mot.py:22-67) do to seeded synthetic sequences.

    python tools/gen_results_golden.py --reference-path DIR --out tests/golden/results

DIR is a checkout of the reference.  Its two functions are imported as they are, under the stub modules tools/gen_label_golden.py
uses for what the dataset modules import and these functions do not need.  Each case is a trackmpnn_amd.results.
synth_result_sequence; the reference gets bbox_pred [n, 14] float32 (results.bbox_pred_of: the columns infer.py:92 cuts out) and
y_out [n, 2] int64 (frame, track) and writes into a temporary directory.  Recorded per case, as results_<name>.npz, data only:
the sequence's arrays, bbox_pred, y_out before and after the call (the reference filters y_out in place), and
    kitti   the bytes of the file it wrote, as uint8
    bdd     the `data` list it hands to json.dump, as JSON text made with a converter for numpy scalars -- captured from the
            call, because json.dump itself raises TypeError on the numpy scalars of any frame that is not empty, so no file
            holds it
The tool asserts that the host functions of trackmpnn_amd.results reproduce every recorded case, and that the cases hold what
they are for (removed and kept tracks, the boundary scores, gaps).  The fixtures live in a directory of their own:
tests/conftest.py takes every .npz directly under tests/golden for a model fixture.  Nothing of the reference's text is copied."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KEYS = ('det_frame', 'det_cat', 'det_score', 'det_box', 'det_alpha', 'det_dim', 'det_loc', 'det_rot')
# name -> (rule set, arguments of synth_result_sequence)
CASES = {
    'kitti_mixed': ('kitti', dict(seed=11, frames=10, n_tracks=20, p_gap=0.0, t0=0, with_3d=True)),
    'kitti_boundary': ('kitti', dict(seed=12, frames=6, n_tracks=40, p_gap=0.0, t0=0, stray_rate=0.3, max_len=4)),
    'kitti_gaps': ('kitti', dict(seed=13, frames=14, n_tracks=16, p_gap=0.4, t0=7)),
    'kitti_sparse': ('kitti', dict(seed=14, frames=10, n_tracks=24, sparse_ids=True, max_len=6)),
    'bdd': ('bdd', dict(seed=15, frames=8, n_tracks=18, p_gap=0.3, t0=2)),
}


def reference_functions(path):
    """{'kitti': store_kitti_results, 'bdd': store_bdd100k_results} and the reference's bdd100k_mot module."""
    from gen_label_golden import reference_functions as stub_and_import
    stub_and_import(path)                                           # (stubs what the dataset modules import, then imports them)
    import dataset.bdd100k_mot as bdd
    import dataset.kitti_mot as kitti
    return {'kitti': kitti.store_kitti_results, 'bdd': bdd.store_bdd100k_results}, bdd


def plain(o):
    """json's `default`: numpy scalars as int / float."""
    if isinstance(o, np.integer):
        return int(o)
    if isinstance(o, np.floating):
        return float(o)
    raise TypeError(type(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join('tests', 'golden', 'results'))
    a = ap.parse_args()
    from trackmpnn_amd.results import (BDD_RESULT_RULES, KITTI_RESULT_RULES, bbox_pred_of, bdd_document_host, kitti_lines_host,
                                       results_host, synth_result_sequence)
    rule_sets = {'kitti': KITTI_RESULT_RULES, 'bdd': BDD_RESULT_RULES}
    fns, bdd_module = reference_functions(a.reference_path)
    os.makedirs(a.out, exist_ok=True)
    for name, (rs, kw) in CASES.items():
        rules = rule_sets[rs]
        q = synth_result_sequence(rules=rules, **kw)
        n = q['det_frame'].shape[0]
        assert 0 < n <= 200, (name, n)
        bbox_pred = bbox_pred_of(q, rules)
        y_in = np.stack([q['det_frame'], q['tracks']], 1).astype(np.int64)
        y_out = y_in.copy()
        class_dict = {v: k for k, v in rules.names.items()}
        out = {k: q[k] for k in KEYS if k in q}
        out.update(rules=np.asarray(rs), bbox_pred=bbox_pred, y_in=y_in)
        res = results_host(q, q['tracks'], rules)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'out', '0007.txt' if rs == 'kitti' else '0007.json')
            if rs == 'kitti':
                fns[rs](bbox_pred.copy(), y_out, class_dict, path)
                with open(path, 'rb') as f:
                    data = f.read()
                out['kitti_bytes'] = np.frombuffer(data, np.uint8)
                same = data == kitti_lines_host(q, res, rules)
            else:
                captured = []
                real_dump = bdd_module.json.dump
                bdd_module.json.dump = lambda data, f, **k: captured.append(data)
                try:
                    fns[rs](bbox_pred.copy(), y_out, class_dict, path)
                finally:
                    bdd_module.json.dump = real_dump
                text = json.dumps(captured[0], default=plain)
                out['bdd_json'] = np.asarray(text)
                out['bdd_name'] = np.asarray(os.path.basename(path))
                same = json.loads(text) == bdd_document_host(q, res, rules, os.path.basename(path))
        out['y_out'] = y_out
        same = same and np.array_equal(res['tracks'], y_out[:, 1]) and np.array_equal(y_out[:, 0], y_in[:, 0])
        removed = np.unique(y_in[(y_in[:, 1] >= 0) & (y_out[:, 1] == -1), 1]).shape[0]
        kept = np.unique(y_out[y_out[:, 1] >= 0, 1]).shape[0]
        assert same, f'{name}: the host functions differ from the reference'
        assert kept > 0 and (removed > 0) == bool(rules.min_track_score), (name, kept, removed)
        fpath = os.path.join(a.out, f'results_{name}.npz')
        np.savez_compressed(fpath, **out)
        print(f'{fpath}: {os.path.getsize(fpath)} bytes, {n} rows, frames {res["t_range"]}, {kept} tracks kept, {removed} removed; '
              f'host functions equal: {same}')


if __name__ == '__main__':
    main()
