"""Record what the reference's validation pass computes per forward call (train.py:200-260) on a few small sequences.

    python tools/gen_val_f1_golden.py --reference-path DIR --out tests/golden/val_f1

DIR is a checkout of the reference.  Its TrackMPNN, initialize_graph, update_graph, decode_tracks and create_targets are imported
as they are and driven by the loop below -- the order of calls of train.py's validation pass: after EVERY model call the
targets of the current graph, pred = argmax((1 - score, score)) and sklearn's f1_score(targets[idx], pred[idx], zero_division=0)
over the det and edge rows (the edge rows alone without the TP classifier), then decode_tracks.  train.py itself cannot be
imported (it parses the command line at import).  Written per case as <name>.npz:

    param/*          the model's parameters and buffers (H = 32, no attention heads, eval mode)
    X, y             the sequence; meta (JSON): the loop's settings and what the case is there for
    f<c>/...         per forward call c: scores [N] (P(positive) as the model returned it), labels, is_edge, src, dst (the graph
                     in row form: rows of an edge's earlier / later det, -1 on det rows), targets (create_targets), counts
                     (tp, fp, fn, rows over the selected rows), f1 (sklearn's value) and, for c >= 1, keep (the rows its decode kept)
    mean_f1, y_out   the mean over the forwards (train.py:278) and the finalised tracks

The set has to exercise the label rule and the loop's corners, so the conditions below are CHECKED here -- a seed that breaks
one is refused -- and again on the committed files by tests/test_val_f1.py:
    margin           every score of every forward is at least MARGIN away from 0.5 (ten times the score tolerance of the
                     device-versus-fixture inference tests): pred cannot differ between the reference's scores and the device's
    multi_past / multi_future   some det has two or more label-positive past / future edges (the last / first rule decides)
    twice            some edge is chosen by both of its endpoints
    empty_selection  some forward without the TP classifier has no edge row (an empty selection: F1 = 0, still a forward)
    label_deleted    some decode deletes a label-positive row and keeps a later row

The fixtures live in a directory of their own: tests/conftest.py takes every .npz directly under tests/golden for a model
fixture.  They are data; nothing of the reference's text is copied here."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MARGIN = 1e-3          # 10 x the 1e-4 of tests/test_tracking_gpu.py's score comparisons
H = 32

# name -> settings.  drop: timesteps whose detections are removed; a run of them longer than the window empties the graph
# (re-initialisation), a shorter one gives forwards without new rows.
CASES = {
    'greedy_w3_r0': dict(seed=25, T=9, win=3, ret=0, hung=False, tp=True),
    'hungarian_w5_r2': dict(seed=17, T=10, win=5, ret=2, hung=True, tp=True),
    'hungarian_w3_r0_notp_reinit': dict(seed=12, T=9, win=3, ret=0, hung=True, tp=False, drop=(3, 4)),
    'greedy_w3_r2_notp_empty': dict(seed=31, T=10, win=3, ret=2, hung=False, tp=False, drop=(4, 5, 6)),
    'greedy_w5_r0_shuffled_hole': dict(seed=10, T=10, win=5, ret=0, hung=False, tp=True, drop=(4,), shuffle=True),
}


class Reference:
    def __init__(self, path):
        sys.path.insert(0, path)
        from models.loss import create_targets
        from models.track_mpnn import TrackMPNN
        from utils.graph import decode_tracks, initialize_graph, update_graph
        self.TrackMPNN, self.create_targets = TrackMPNN, create_targets
        self.initialize_graph, self.update_graph, self.decode_tracks = initialize_graph, update_graph, decode_tracks


def make_model(ref, seed):
    """The reference's model with seeded, spread-out weights: scores on both sides of 0.5, BatchNorm statistics off their defaults."""
    torch.manual_seed(seed)
    model = ref.TrackMPNN('2d', 3, H, 0, 'diff')
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith('output_transform') and name.endswith('bias'):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            else:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
        for name, b in model.named_buffers():
            if name.endswith('running_mean'):
                b.copy_(0.2 * torch.randn(b.shape, generator=g))
            elif name.endswith('running_var'):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return model.eval()


def make_sequence(cfg):
    from oracle.gen_golden import synth_sequence
    X, y = synth_sequence(cfg['seed'], cfg['T'], cfg.get('dmean', 3), 3, '2d', fp_rate=0.2)
    if cfg.get('drop'):
        keep = ~torch.isin(y[0, :, 0], torch.tensor(cfg['drop']))
        X, y = X[:, keep], y[:, keep]
    if cfg.get('shuffle'):
        perm = torch.randperm(y.shape[1], generator=torch.Generator().manual_seed(cfg['seed'] + 99))
        X, y = X[:, perm], y[:, perm]
    return X.contiguous(), y.contiguous()


def row_form(node_adj, y_pred):
    """(is_edge, src, dst) of the reference's node_adj: an edge row holds +1 at its earlier det and -1 at its later det."""
    a = (node_adj.to_dense() if node_adj.is_sparse else node_adj).numpy().copy()
    np.fill_diagonal(a, 0)
    is_edge = (y_pred[:, 0] == -1).numpy()
    N = a.shape[0]
    src, dst = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    for r in np.flatnonzero(is_edge):
        (s,), (d,) = np.flatnonzero(a[r] == 1), np.flatnonzero(a[r] == -1)
        src[r], dst[r] = s, d
    return is_edge.astype(np.uint8), src, dst


def run_case(ref, name, cfg, out_dir):
    from sklearn.metrics import f1_score
    model = make_model(ref, cfg['seed'])
    X, y = make_sequence(cfg)
    out = {'param/' + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    out['X'], out['y'] = X.numpy().copy(), y.numpy().copy()
    y_out = y[0].numpy().astype('int64').copy()
    y_out[:, 1] = -1
    f1s = []

    def forward(feats, states, node_adj, edge_adj, y_pred, labels):
        """One model call and what the validation pass computes after it; returns the [N, 2] scores the graph functions take."""
        s, _, states, _ = model(feats, states, node_adj, edge_adj)
        two = torch.cat((1 - s, s), 1)
        idx_edge = torch.nonzero(y_pred[:, 0] == -1)[:, 0]
        idx_node = torch.nonzero(y_pred[:, 0] != -1)[:, 0]
        targets = ref.create_targets(labels, node_adj, idx_node)
        if cfg['tp']:
            idx = torch.cat((idx_node, idx_edge))
        else:
            two[idx_node, 0], two[idx_node, 1] = 0, 1
            idx = idx_edge
        pred = two.max(1)[1]
        t, p = targets[idx].numpy(), pred[idx].numpy()
        f1 = float(f1_score(t, p, zero_division=0))
        c = len(f1s)
        is_edge, src, dst = row_form(node_adj, y_pred)
        out[f'f{c}/scores'] = s[:, 0].numpy().astype(np.float32).copy()
        out[f'f{c}/labels'] = labels.numpy().astype(np.uint8)
        out[f'f{c}/is_edge'], out[f'f{c}/src'], out[f'f{c}/dst'] = is_edge, src, dst
        out[f'f{c}/targets'] = targets.numpy().astype(np.uint8)
        out[f'f{c}/counts'] = np.array([int(((p == 1) & (t == 1)).sum()), int(((p == 1) & (t == 0)).sum()),
                                        int(((p == 0) & (t == 1)).sum()), int(labels.shape[0])], np.int64)
        out[f'f{c}/f1'] = np.float64(f1)
        f1s.append(f1)
        return two, states

    reinit = 0
    with torch.no_grad():
        y_pred, feats, node_adj, edge_adj, labels, t_st, t_end = ref.initialize_graph(X, y, t_st=0, mode='test', cuda=False)
        assert y_pred is not None, name
        scores, states = forward(feats, None, node_adj, edge_adj, y_pred, labels)
        t_skip = t_st
        for t_cur in range(t_st, t_end):
            if t_cur < t_skip:
                continue
            if feats.size()[0] == 0 and states.size()[0] == 0:
                y_pred, feats, node_adj, edge_adj, labels, t_skip, _ = ref.initialize_graph(X, y, t_st=t_cur, mode='test', cuda=False)
                if y_pred is None:
                    break
                states = None
                reinit += 1
            else:
                y_pred, feats, node_adj, edge_adj, labels = ref.update_graph(node_adj, labels, scores, y_pred, X, y, t_cur,
                                                                             use_hungraian=cfg['hung'], mode='test', cuda=False)
            scores, states = forward(feats, states, node_adj, edge_adj, y_pred, labels)
            t_upto = t_end if t_cur == t_end - 1 else t_cur - cfg['win'] + 2
            # decode_tracks deletes the same rows of whatever it is given as labels: row number and label travel together
            tagged = 2 * torch.arange(labels.shape[0], dtype=torch.int64) + labels
            y_pred, y_out, states, node_adj, tagged, scores = ref.decode_tracks(states, node_adj, tagged, scores, y_pred, y_out, t_upto,
                                                                                cfg['ret'], use_hungraian=cfg['hung'], cuda=False)
            labels = tagged % 2
            out[f'f{len(f1s) - 1}/keep'] = (tagged // 2).numpy().astype(np.int32)
    out['mean_f1'] = np.float64(np.mean(f1s))
    out['y_out'] = y_out.copy()
    meta = dict(name=name, kind='val_f1', features='2d', ncategories=3, nhidden=H, nattheads=0, msg_type='diff', mode='eval',
                ncalls=len(f1s), seed=cfg['seed'], T=cfg['T'], cur_win_size=cfg['win'], ret_win_size=cfg['ret'],
                hungarian=bool(cfg['hung']), tp_classifier=bool(cfg['tp']), dropped_timesteps=list(cfg.get('drop', ())),
                shuffled=bool(cfg.get('shuffle', False)), reinitialisations=reinit, margin=MARGIN, torch=torch.__version__,
                reference='arangesh/TrackMPNN train.py:200-260 (the validation pass, per forward call)')
    out['meta'] = np.array(json.dumps(meta))
    return out, meta


def conditions(d):
    """What a case contributes to the set's conditions (module docstring), from the arrays it stores."""
    n = json.loads(str(d['meta']))['ncalls']
    tp = json.loads(str(d['meta']))['tp_classifier']
    res = dict(margin=np.inf, multi_past=False, multi_future=False, twice=False, empty_selection=False, label_deleted=False,
               no_new_rows=False)
    prev_n = None
    for c in range(n):
        is_edge, lab = d[f'f{c}/is_edge'] != 0, d[f'f{c}/labels'] != 0
        src, dst = d[f'f{c}/src'], d[f'f{c}/dst']
        res['margin'] = min(res['margin'], float(np.abs(d[f'f{c}/scores'].astype(np.float64) - 0.5).min()))
        pos = np.flatnonzero(is_edge & lab)
        for ends, key in ((dst, 'multi_past'), (src, 'multi_future')):
            if pos.size and np.bincount(ends[pos]).max() >= 2:
                res[key] = True
        for r in pos:
            if r == pos[dst[pos] == dst[r]].max() and r == pos[src[pos] == src[r]].min():
                res['twice'] = True
        if not tp and not is_edge.any():
            res['empty_selection'] = True
        if prev_n is not None and prev_n == lab.size:
            res['no_new_rows'] = True
        if c >= 1:
            keep = d[f'f{c}/keep']
            gone = np.setdiff1d(np.flatnonzero(lab), keep)
            if gone.size and keep.size and keep.max() > gone.min():
                res['label_deleted'] = True
            prev_n = keep.size
        else:
            prev_n = lab.size
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join('tests', 'golden', 'val_f1'))
    a = ap.parse_args()
    ref = Reference(a.reference_path)
    os.makedirs(a.out, exist_ok=True)
    total = {}
    for name, cfg in CASES.items():
        out, meta = run_case(ref, name, cfg, a.out)
        res = conditions(out)
        if res['margin'] < MARGIN:
            raise SystemExit(f'{name}: a score lies {res["margin"]:.2e} from 0.5 (< {MARGIN}): choose another seed')
        if bool(cfg.get('drop')) and len(cfg['drop']) >= cfg['win'] - 1 and cfg['ret'] == 0 and meta['reinitialisations'] == 0:
            raise SystemExit(f'{name}: the gap did not force a re-initialisation')
        if cfg.get('drop') and meta['reinitialisations'] == 0 and not res['no_new_rows']:
            raise SystemExit(f'{name}: no forward without new rows')
        path = os.path.join(a.out, name + '.npz')
        np.savez_compressed(path, **out)
        for k, v in res.items():
            total[k] = min(total.get(k, np.inf), v) if k == 'margin' else (total.get(k, False) or v)
        print(f'{path}: {os.path.getsize(path)} bytes, {meta["ncalls"]} forwards, mean F1 {float(out["mean_f1"]):.4f}, '
              f'{meta["reinitialisations"]} re-initialisations, {res}')
    missing = [k for k, v in total.items() if k != 'margin' and not v]
    if missing:
        raise SystemExit(f'the set does not cover: {missing}')
    if sum(json.loads(str(np.load(os.path.join(a.out, n + ".npz"))["meta"]))['reinitialisations'] for n in CASES) == 0:
        raise SystemExit('no case re-initialises')
    print('set:', total)


if __name__ == '__main__':
    main()
