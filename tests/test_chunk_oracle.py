"""The reference's whole training chunks (fixtures chunk_*: train.py:54-135 in the TP-classifier mode and with
--no-tp-classifier) on the host, no GPU: the CPU oracle run over the host plan builder's call graphs in the fixture's mode
against the reference's per-call losses, targets and parameter gradients; the host definition of the monitor's counts
(trackmpnn_amd.monitor) on the reference's own scores against its tp / fp / fn; F1 from the counts against sklearn's values."""
import numpy as np
import pytest
import torch

from oracle import trackmpnn_oracle as orc
from tests.conftest import chunk_golden_names
from tests.golden_util import Golden, chunk_tp
from trackmpnn_amd import build_train_batch
from trackmpnn_amd.monitor import val_counts_host, val_f1_host


def _oracle_graph(g):
    return orc.OracleGraph(g.N, g.is_edge.numpy().astype(bool), g.src.numpy().astype(np.int64), g.dst.numpy().astype(np.int64),
                           g.edge_row.numpy().astype(np.int64), g.det_row.numpy().astype(np.int64))


def _host_calls(gold):
    """[(oracle graph, features of the new rows, uint8 row labels)] per call, from the host plan builder at B = 1."""
    batch = build_train_batch([gold.t('y')[0].numpy()])
    assert batch.ncalls == gold.ncalls == len(batch.plans)
    Xz = batch.stacked_features(gold.t('X')[0])
    return [(_oracle_graph(plan.graph), Xz.index_select(0, batch.feat_src[c]), batch.call_labels(c))
            for c, plan in enumerate(batch.plans)]


@pytest.mark.parametrize('name', chunk_golden_names())
def test_oracle_chunk_matches_the_reference_chunk(name):
    """oracle.forward with the state carried + orc.create_targets / ce_loss / focal_loss in the fixture's mode: per-call
    loss_c and loss_f within 1e-5 relative (test_oracle_losses_match_reference's tolerance), every call's targets equal,
    parameter gradients of the one backward within atol 1e-5, rtol 1e-4, BatchNorm buffers after the chunk."""
    gold = Golden(name)
    m, tp = gold.meta, chunk_tp(gold)
    cfg = orc.OracleConfig(m['features'], m['ncategories'], m['nhidden'], m['nattheads'], m['msg_type'])
    p = gold.params()
    for k, v in p.items():
        if v.dtype.is_floating_point and not k.endswith(orc.BUFFER_SUFFIXES):
            v.requires_grad_(True)
    ref = gold.d['per_call']
    h, total = None, 0.0
    for c, (og, x, labels) in enumerate(_host_calls(gold)):
        assert og.N == int(ref[c, 2])
        scores, logits, h, _ = orc.forward(p, cfg, x, h, og, training=True)
        t = orc.create_targets(labels.long(), og)
        assert torch.equal(t.to(torch.uint8), gold.t(f'c{c}/targets')), c
        assert torch.allclose(scores.detach().reshape(-1), gold.t(f'c{c}/scores'), atol=1e-5, rtol=0), c
        dr, er = torch.from_numpy(og.det_row), torch.from_numpy(og.edge_row)
        loss_c = orc.ce_loss(logits, t, og)
        loss_f = orc.focal_loss(scores[er, 0], t[er])
        if tp:                                                   # train.py:77 / :81
            loss_f = orc.focal_loss(scores[dr, 0], t[dr]) + loss_f
        for k, got in enumerate((loss_c, loss_f)):
            assert abs(got.item() - ref[c, k]) <= 1e-5 * max(1.0, abs(ref[c, k])), (c, k, got.item(), ref[c, k])
        total = total + loss_c + loss_f
    total.backward()
    zero_ref = []
    for k, gref in gold.grads().items():
        got = p[k].grad
        assert got is not None, k
        assert torch.allclose(got, gref, atol=1e-5, rtol=1e-4), (k, float((got - gref).abs().max()), float(gref.abs().max()))
        if not gref.any():
            zero_ref.append(k)
            assert not got.any(), k
    # without the TP classifier nothing reaches the node output head (train.py:81): the reference leaves its gradient at zero
    heads = {'output_transform_node.weight', 'output_transform_node.bias'}
    assert heads <= set(zero_ref) if not tp else not (heads & set(zero_ref))
    for k, r in gold.params('buf_after/').items():
        if r.dtype.is_floating_point:
            assert torch.allclose(p[k].detach(), r, atol=1e-5, rtol=1e-5), k
        else:
            assert int(p[k]) == int(r), k


@pytest.mark.parametrize('name', chunk_golden_names())
def test_host_counts_on_the_reference_scores(name):
    """train.py:86-88 / :125-127 per forward: val_counts_host (the monitor's host definition: its own targets from the row
    labels, pred = s > 0.5, edge rows alone without the TP classifier) on the reference's scores gives the reference's
    tp / fp / fn exactly, and so does the plain count over the reference's own targets; F1 from the counts equals sklearn's
    f1_score within 1e-12."""
    gold = Golden(name)
    tp = chunk_tp(gold)
    counts, f1 = gold.d['counts'], gold.d['f1']
    assert counts.shape == (gold.ncalls, 3) and counts.dtype == np.int64 and f1.shape == (gold.ncalls,)
    got = []
    for c, (og, _, labels) in enumerate(_host_calls(gold)):
        s = gold.d[f'c{c}/scores']
        t = gold.d[f'c{c}/targets'] != 0
        assert s.dtype == np.float32 and s.shape == (og.N,) and t.shape == (og.N,)
        src, dst = np.zeros(og.N, np.int64), np.zeros(og.N, np.int64)
        src[og.edge_row], dst[og.edge_row] = og.src, og.dst
        got.append(val_counts_host(og.is_edge, src, dst, labels.numpy(), s, tp))
        assert got[-1][:3] == tuple(int(v) for v in counts[c]) and got[-1][3] == og.N, (c, got[-1], counts[c])
        sel = og.is_edge if not tp else np.ones(og.N, bool)
        pred = s > np.float32(0.5)
        plain = (int((pred & t & sel).sum()), int((pred & ~t & sel).sum()), int((~pred & t & sel).sum()))
        assert plain == got[-1][:3], c
        # the recorded margin covers every counted row
        assert float(np.abs(s[sel].astype(np.float64) - 0.5).min()) >= gold.meta['min_margin']
    assert gold.meta['min_margin'] > 0.0
    r = val_f1_host(got)
    assert r['forwards'] == gold.ncalls
    assert np.abs(np.asarray(r['per_forward']) - f1).max() <= 1e-12
    assert abs(r['f1'] - f1.mean()) <= 1e-12
    assert (counts[:, 0] > 0).any() and (counts[:, 1:] > 0).any()          # the inputs are not degenerate


def test_the_two_modes_share_sequence_and_forward():
    """A *_notp fixture is its TP-mode partner's chunk in the other mode: same sequence and parameters, hence the same forward
    (scores, targets, loss_c per call); loss_f is the edge term alone and the counts leave the det rows out."""
    names = chunk_golden_names()
    pairs = [(n[:-5], n) for n in names if n.endswith('_notp')]
    assert len(pairs) >= 2 and all(a in names for a, _ in pairs)
    for a, b in pairs:
        ga, gb = Golden(a), Golden(b)
        assert chunk_tp(ga) and not chunk_tp(gb)
        for k in ['X', 'y'] + [k for k in ga.d.files if k.startswith('param/') or k.endswith(('/scores', '/targets'))]:
            assert np.array_equal(ga.d[k], gb.d[k]), (a, k)
        assert np.array_equal(ga.d['per_call'][:, [0, 2]], gb.d['per_call'][:, [0, 2]])
        assert (gb.d['per_call'][:, 1] < ga.d['per_call'][:, 1]).all()
        assert (gb.d['counts'] <= ga.d['counts']).all() and (gb.d['counts'] < ga.d['counts']).any()
        for k in ('output_transform_node.weight', 'output_transform_node.bias'):
            assert ga.d['grad/' + k].any() and not gb.d['grad/' + k].any()
