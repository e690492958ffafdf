"""Record what the reference's head study (attention_weights.py) computes on a few small sequences.

    python tools/gen_att_hist_golden.py --reference-path DIR --out tests/golden/att_hist

DIR is a checkout of the reference.  Its TrackMPNN, initialize_graph, update_graph and decode_tracks are imported as they are
and driven by the loop below -- the order of calls of attention_weights.py's pass: the first model call of a sequence is NOT
stored, every model call inside the timestep loop (the calls after a re-initialisation included) is, with its labels, y_pred
and the dense [N, N] attention matrices of feature group 0.  The selection rule of its plot function is then applied to those
dense matrices as they are (for every det row and every column: an entry > 0 in an edge column is `tp` where the column's label
== 1, `fp` otherwise) and each list is binned with np.histogram(values, 25, (0.0, 1.0)), the figure's arguments.
attention_weights.py itself cannot be imported (it parses the command line and opens a dataset at import).  Written per case as
<name>.npz:

    param/*          the model's parameters and buffers (H = 32, '2d', 3 categories, K heads, eval mode)
    X, y             the sequence; meta (JSON): the loop's settings and what the case is there for
    f<c>/...         per STORED forward c: is_edge, src, dst (the graph in row form: rows of an edge's earlier / later det, -1
                     on det rows), labels, scores (P(positive), for the margin below), alpha [K, 2E] (the informative entries of
                     the dense matrices in CSR order: per det row ascending, its incident edge rows ascending), values_k<k> /
                     tp_k<k> (the walk's values of head k in row-major order and their tp flag), hist [K, 2, 25]
    hist, forwards   the histograms summed over the stored forwards, and their number
    y_out            the finalised tracks

The conditions below are CHECKED here -- a seed that breaks one is refused -- and again on the committed files by
tests/test_att_hist.py:
    margin      every informative alpha (a det row's entry at an incident edge) is at least MARGIN from every bin edge, so that
                the device's alpha -- held to atol + rtol of the reference's by the existing test -- falls into the same bin.  The
                one exception is exact: a det with ONE incident edge has alpha == 1.0f on both sides (exp(0) / exp(0)), which sits
                on the closed last edge.  Every score is at least SCORE_MARGIN from 0.5, so that the loop's decisions agree too.
    uniform     every dense row of a det without incident edges equals np.float32(1) / np.float32(N) in every column, bit for bit;
                every other det row is exactly 0 off its incident edges
    both        tp and fp are non-empty for every head of every case
    isolated    some det of the set has no incident edge while its graph has edges
    mixed       some det of some forward has a label-1 and a label-0 incident edge

The fixtures live in a directory of their own: tests/conftest.py takes every .npz directly under tests/golden for a model
fixture.  They are data; nothing of the reference's text is copied here."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# ten times the tolerance of tests/test_small_path_gpu.py::test_fused_iteration_with_attention_heads_matches_the_reference, the
# device-versus-fixture comparison of the attention values: allclose(atol=1e-5, rtol=1e-4) on weights of at most 1
MARGIN = 10 * (1e-5 + 1e-4)
SCORE_MARGIN = 1e-3    # as tools/gen_val_f1_golden.py: 10 x the 1e-4 of tests/test_tracking_gpu.py's score comparisons
H = 32
BINS = 25
ATT_SCALE = 0.005       # (see CASES: `att`)

# name -> settings.  drop: timesteps whose detections are removed; a run of them longer than the window empties the graph
# (re-initialisation), a shorter one gives forwards without new rows (with ret > 0: retained dets without an edge).
# att: the scale of the heads' `a` vectors -- small enough that the softmax rows stay clear of the bin edges (a row over d edges
# sits near 1 / d), which is what lets a whole case meet the margin.
CASES = {
    'greedy_k2_w3_r0': dict(seed=8, T=9, K=2, win=3, ret=0, hung=False),
    'hungarian_k3_w3_r2': dict(seed=5, T=9, K=3, win=3, ret=2, hung=True),
    'greedy_k2_w3_r0_reinit': dict(seed=10, T=10, K=2, win=3, ret=0, hung=False, drop=(4, 5)),
    'greedy_k2_w3_r2_isolated': dict(seed=47, T=10, K=2, win=3, ret=2, hung=False, drop=(5,)),
}


class Reference:
    def __init__(self, path):
        sys.path.insert(0, path)
        from models.track_mpnn import TrackMPNN
        from utils.graph import decode_tracks, initialize_graph, update_graph
        self.TrackMPNN = TrackMPNN
        self.initialize_graph, self.update_graph, self.decode_tracks = initialize_graph, update_graph, decode_tracks


def make_model(ref, cfg):
    """The reference's model with seeded, spread-out weights (scores on both sides of 0.5, BatchNorm statistics off their
    defaults) and the heads' `a` vectors scaled by cfg['att']."""
    seed = cfg['seed']
    torch.manual_seed(seed)
    model = ref.TrackMPNN('2d', 3, H, cfg['K'], 'diff')
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith('output_transform') and name.endswith('bias'):
                # (most detections score above 0.5 and stay active: graphs with edges, not rows of isolated dets)
                p.copy_(0.5 * torch.randn(p.shape, generator=g) + (cfg.get('node_bias', 1.0) if '_node' in name else 0.0))
            elif name.endswith('.a'):
                p.mul_(cfg.get('att', ATT_SCALE))
            elif '.gat.' not in name:
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


def walk(att, is_edge, labels):
    """The plot function's selection on one head's dense matrix: (values in row-major order, their tp flag)."""
    sel = (~is_edge)[:, None] & (att > 0) & is_edge[None, :]
    r, c = np.nonzero(sel)
    return att[r, c].astype(np.float32), (labels[c] == 1).astype(np.uint8)


def run_case(ref, name, cfg):
    from trackmpnn_amd.monitor import att_csr_host
    model = make_model(ref, cfg)
    X, y = make_sequence(cfg)
    K = cfg['K']
    out = {'param/' + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    out['X'], out['y'] = X.numpy().copy(), y.numpy().copy()
    y_out = y[0].numpy().astype('int64').copy()
    y_out[:, 1] = -1
    stored = 0
    total = np.zeros((K, 2, BINS), np.int64)
    reinit = 0
    with torch.no_grad():
        y_pred, feats, node_adj, edge_adj, labels, t_st, t_end = ref.initialize_graph(X, y, t_st=0, mode='test', cuda=False)
        assert y_pred is not None, name
        s, _, states, _ = model(feats, None, node_adj, edge_adj)                   # the first call: not stored
        out['first_scores'] = s[:, 0].numpy().astype(np.float32).copy()
        scores = torch.cat((1 - s, s), 1)
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
            s, _, states, attention = model(feats, states, node_adj, edge_adj)
            # ---- what attention_weights.py stores, and its plot function's walk
            c = stored
            is_edge, src, dst = row_form(node_adj, y_pred)
            lab = labels.numpy().astype(np.int64)
            dense = [a.detach().numpy().astype(np.float32) for a in attention[0]]
            assert len(dense) == K
            dets, rowptr, inc = att_csr_host(is_edge, src, dst)
            det_of_pos = np.repeat(dets, np.diff(rowptr))
            out[f'f{c}/is_edge'], out[f'f{c}/src'], out[f'f{c}/dst'] = is_edge, src, dst
            out[f'f{c}/labels'] = lab.astype(np.uint8)
            out[f'f{c}/scores'] = s[:, 0].numpy().astype(np.float32).copy()
            out[f'f{c}/alpha'] = np.stack([a[det_of_pos, inc & 0x7FFFFFFF] for a in dense]).astype(np.float32).reshape(K, -1)
            hist = np.zeros((K, 2, BINS), np.int64)
            for k, a in enumerate(dense):
                vals, tp = walk(a, is_edge != 0, lab)
                out[f'f{c}/values_k{k}'], out[f'f{c}/tp_k{k}'] = vals, tp
                hist[k, 0] = np.histogram(vals[tp == 1], BINS, (0.0, 1.0))[0]
                hist[k, 1] = np.histogram(vals[tp == 0], BINS, (0.0, 1.0))[0]
                # the uniform / zero structure of the dense rows (condition `uniform`)
                iso = dets[np.diff(rowptr) == 0]
                u = np.float32(1) / np.float32(a.shape[0])
                if not (a[iso] == u).all():
                    raise SystemExit(f'{name}: forward {c}: a uniform row is not float32(1) / float32(N)')
                informative = np.zeros_like(a, dtype=bool)
                informative[det_of_pos, inc & 0x7FFFFFFF] = True
                busy = dets[np.diff(rowptr) > 0]
                if (a[busy][~informative[busy]] != 0).any():
                    raise SystemExit(f'{name}: forward {c}: a det row is not 0 off its incident edges')
            out[f'f{c}/hist'] = hist
            total += hist
            stored += 1
            scores = torch.cat((1 - s, s), 1)
            t_upto = t_end if t_cur == t_end - 1 else t_cur - cfg['win'] + 2
            y_pred, y_out, states, node_adj, labels, scores = ref.decode_tracks(states, node_adj, labels, scores, y_pred, y_out,
                                                                                t_upto, cfg['ret'], use_hungraian=cfg['hung'],
                                                                                cuda=False)
    out['hist'], out['forwards'], out['y_out'] = total, np.int64(stored), y_out.copy()
    meta = dict(name=name, kind='att_hist', features='2d', ncategories=3, nhidden=H, nattheads=K, msg_type='diff', mode='eval',
                forwards=stored, seed=cfg['seed'], T=cfg['T'], cur_win_size=cfg['win'], ret_win_size=cfg['ret'],
                hungarian=bool(cfg['hung']), tp_classifier=True, dropped_timesteps=list(cfg.get('drop', ())),
                reinitialisations=reinit, bins=BINS, margin=MARGIN, score_margin=SCORE_MARGIN, att_scale=cfg.get('att', ATT_SCALE),
                torch=torch.__version__, reference='arangesh/TrackMPNN attention_weights.py:84-105, :157-196')
    out['meta'] = np.array(json.dumps(meta))
    return out, meta


def edge_distance(alpha, degree, bins=BINS):
    """Per informative alpha: its distance to the nearest bin edge (float64); inf for the exact 1.0f of a degree-1 det."""
    edges = np.histogram_bin_edges(np.zeros(0, np.float32), bins, (0.0, 1.0)).astype(np.float64)
    a = np.asarray(alpha, np.float64)
    d = np.abs(a[..., None] - edges).min(-1)
    return np.where((np.asarray(degree) == 1) & (np.asarray(alpha) == np.float32(1)), np.inf, d)


def conditions(d):
    """What a case contributes to the set's conditions (module docstring), from the arrays it stores."""
    from trackmpnn_amd.monitor import att_csr_host
    m = json.loads(str(d['meta']))
    res = dict(margin=np.inf, score_margin=float(np.abs(d['first_scores'].astype(np.float64) - 0.5).min()), both=True,
               isolated=False, mixed=False)
    for c in range(m['forwards']):
        is_edge, lab = d[f'f{c}/is_edge'] != 0, d[f'f{c}/labels']
        dets, rowptr, inc = att_csr_host(is_edge, d[f'f{c}/src'], d[f'f{c}/dst'])
        deg = np.diff(rowptr)
        res['score_margin'] = min(res['score_margin'], float(np.abs(d[f'f{c}/scores'].astype(np.float64) - 0.5).min()))
        if inc.size:
            res['margin'] = min(res['margin'], float(edge_distance(d[f'f{c}/alpha'], np.repeat(deg, deg)[None, :]).min()))
            if (deg == 0).any():
                res['isolated'] = True
            pos = lab[inc & 0x7FFFFFFF] == 1
            n_pos = np.add.reduceat(pos.astype(np.int64), rowptr[:-1][deg > 0]) if (deg > 0).any() else np.zeros(0)
            if ((n_pos > 0) & (n_pos < deg[deg > 0])).any():
                res['mixed'] = True
    res['both'] = bool((d['hist'].sum(-1) > 0).all())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join('tests', 'golden', 'att_hist'))
    a = ap.parse_args()
    ref = Reference(a.reference_path)
    os.makedirs(a.out, exist_ok=True)
    total = {}
    reinits = 0
    for name, cfg in CASES.items():
        out, meta = run_case(ref, name, cfg)
        res = conditions(out)
        if res['margin'] < MARGIN:
            raise SystemExit(f'{name}: an attention weight lies {res["margin"]:.2e} from a bin edge (< {MARGIN}): choose another seed')
        if res['score_margin'] < SCORE_MARGIN:
            raise SystemExit(f'{name}: a score lies {res["score_margin"]:.2e} from 0.5 (< {SCORE_MARGIN}): choose another seed')
        if not res['both']:
            raise SystemExit(f'{name}: a head has an empty tp or fp list')
        if 'reinit' in name and meta['reinitialisations'] == 0:
            raise SystemExit(f'{name}: the gap did not force a re-initialisation')
        if 'isolated' in name and not res['isolated']:
            raise SystemExit(f'{name}: no det without an incident edge in a graph with edges')
        reinits += meta['reinitialisations']
        path = os.path.join(a.out, name + '.npz')
        np.savez_compressed(path, **out)
        for k, v in res.items():
            total[k] = min(total.get(k, np.inf), v) if k.endswith('margin') else (total.get(k, False) or v)
        print(f'{path}: {os.path.getsize(path)} bytes, {meta["forwards"]} stored forwards, '
              f'{meta["reinitialisations"]} re-initialisations, {int(out["hist"].sum())} values, {res}')
    missing = [k for k, v in total.items() if not k.endswith('margin') and not v]
    if missing:
        raise SystemExit(f'the set does not cover: {missing}')
    if reinits == 0:
        raise SystemExit('no case re-initialises')
    print('set:', total)


if __name__ == '__main__':
    main()
