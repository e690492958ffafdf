"""The embedding loss's host definition (trackmpnn_amd.embedloss.embedding_loss_host) against the reference's EmbeddingLoss
(models/loss.py:118-159) as recorded in tests/golden/embed (tools/gen_embed_golden.py), hand-computed chunks, the permutation
property and the host twin of attach_vis(embed_loss='embedding').  No GPU.

Bounds against the fixtures.
  Loss: the reference accumulates it in a float32 scalar whatever the feature dtype (float64 features give a float32 loss).
  Every `+=` costs at most two float32 roundings of a non-negative running sum, so the relative error is at most
  (2 max(C, C (C - 1)) + 3) 2^-24.
  Gradient: 1e-12 (1 + |value|), about 100 times the error of a 128-term float64 sum with margin for the division by a norm;
  every norm divided by is asserted to be exactly 0 or >= 1e-2 (a condition on the inputs).  What the reference's backward
  multiplies by, however, is not 1 / C and 1 / (C (C - 1)) in float64: `var_loss /= C` and `dist_loss /= C * (C - 1)` divide
  float32 tensors, so autograd hands float32(1 / C) and float32(1 / (C (C - 1))) down to the float64 terms (measured: the
  recorded gradient differs from the float64 one by up to 2.8e-9 relative where C is not a power of two, by 2.5e-16 at C = 2).
  The host's gradient splits exactly into the variance part (delta_dist = 0 switches the distance hinge off) and the distance
  part (delta_var = 1e30 switches the variance hinge off); the test scales the two by C float32(1 / C) and
  C (C - 1) float32(1 / (C (C - 1))) and holds the sum to the 1e-12 bound, and holds the two parts to the whole at the
  same bound."""
import glob
import os

import numpy as np
import pytest

from trackmpnn_amd.embedloss import embedding_loss_host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'embed')
FIXTURES = sorted(os.path.basename(p)[len('embed_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'embed_*.npz')))


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f'embed_{name}.npz')) as z:
        return {k: z[k] for k in z.files}


def n_clusters(track):
    track = np.asarray(track)
    return int(np.unique(track[track >= 0]).size)


def test_the_fixture_set_is_complete():
    assert set(FIXTURES) == {'c0_rows', 'n0', 'c1', 'c2', 'singletons', 'mod128', 'twins', 'mixed'}
    for name in FIXTURES:
        z = load_fixture(name)
        n = z['features'].shape[0]
        assert n <= 130 and z['features'].shape == (n, 128) and z['features'].dtype == np.float64 and z['labels'].shape == (n, 2)
        assert np.array_equal(z['features'], z['features'].astype(np.float32).astype(np.float64))     # float32 values
        assert z['ref_loss'].dtype == np.float32 and z['ref_grad'].shape == (n, 128) and z['ref_grad'].dtype == np.float64
    assert load_fixture('n0')['features'].shape[0] == 0 and n_clusters(load_fixture('c0_rows')['labels'][:, 1]) == 0
    assert n_clusters(load_fixture('c1')['labels'][:, 1]) == 1 and n_clusters(load_fixture('c2')['labels'][:, 1]) == 2
    ids = load_fixture('mod128')['labels'][:, 1]
    assert n_clusters(ids) == 3 and np.unique(ids[ids >= 0] % 128).size == 1
    assert float(load_fixture('twins')['ref_loss']) == 100.0 and not load_fixture('twins')['ref_grad'].any()   # m = 0: direction 0


@pytest.mark.parametrize('name', FIXTURES)
def test_host_equals_the_reference(name):
    z = load_fixture(name)
    x, track = z['features'], z['labels'][:, 1]
    dv, dd = float(z['delta_var']), float(z['delta_dist'])
    norms = []
    loss, terms, grad = embedding_loss_host(x, track, None, dv, dd, norms=norms)
    assert loss.dtype == np.float64 and loss.shape == (1,) and terms.shape == (1, 2) and grad.shape == x.shape
    assert loss[0] == terms[0, 0] + terms[0, 1]
    norms = np.asarray(norms)
    assert ((norms == 0) | (norms >= 1e-2)).all()
    C = n_clusters(track)
    bound = (2 * max(C, C * (C - 1)) + 3) * 2.0 ** -24
    ref = float(z['ref_loss'])
    err = abs(loss[0] - ref) / ref if ref else abs(loss[0])
    # the gradient in its two parts (module docstring)
    g_var = embedding_loss_host(x, track, None, dv, 0.0)[2]
    g_dist = embedding_loss_host(x, track, None, 1e30, dd)[2]
    sv = C * float(np.float32(1.0) / np.float32(C)) if C > 0 else 1.0
    sd = C * (C - 1) * float(np.float32(1.0) / np.float32(C * (C - 1))) if C > 1 else 1.0
    e_split = np.abs(g_var + g_dist - grad) / (1 + np.abs(grad))
    e_grad = np.abs(sv * g_var + sd * g_dist - z['ref_grad']) / (1 + np.abs(z['ref_grad']))
    print(f'{name}: C = {C}, loss rel err {err:.3g} (bound {bound:.3g}), gradient err / (1 + |value|) {e_grad.max(initial=0):.3g}, '
          f'parts against the whole {e_split.max(initial=0):.3g} (bound 1e-12)')
    assert err <= bound
    assert e_split.max(initial=0) <= 1e-12 and e_grad.max(initial=0) <= 1e-12
    assert not grad[track < 0].any()                                                                # exactly 0
    if C == 0:
        assert loss[0] == 0 and not grad.any()


def test_hand_computed_chunks():
    # two rows, one track: mu = (1.5, 2), d = 2.5 each, hinge 2: var = (1 / 1) (1 / 2) (4 + 4) = 4; u_i = 0.8 (x_i - mu), sum 0
    loss, terms, grad = embedding_loss_host(np.asarray([[0.0, 0.0], [3.0, 4.0]]), [7, 7], None)
    assert loss.tolist() == [4.0] and terms.tolist() == [[4.0, 0.0]]
    np.testing.assert_allclose(grad, [[-1.2, -1.6], [1.2, 1.6]], rtol=1e-15)
    # two tracks, one row each, 6 apart: d = 0, m = 6, hinge 4: dist = (1 / 2) (16 + 16) = 16; d loss / d x_0 = 2 * 4 * (+1, 0)
    loss, terms, grad = embedding_loss_host(np.asarray([[0.0, 0.0], [6.0, 0.0]]), [5, 133], None)
    assert loss.tolist() == [16.0] and terms.tolist() == [[0.0, 16.0]] and grad.tolist() == [[8.0, 0.0], [-8.0, 0.0]]
    # the same rows as two chunks of one cluster each, a false positive between them, and g: nothing left to pull or push
    loss, _, grad = embedding_loss_host(np.asarray([[0.0, 0.0], [9.0, 9.0], [6.0, 0.0]]), [5, -1, 5], [0, 1, 3], g=[2.0, 3.0])
    assert loss.tolist() == [0.0, 0.0] and not grad.any()
    # one chunk again: rows 0 and 2 are one cluster 6 apart (d = 3, hinge 2.5), g scales the gradient
    loss, _, grad = embedding_loss_host(np.asarray([[0.0, 0.0], [9.0, 9.0], [6.0, 0.0]]), [5, -1, 5], [0, 3], g=[2.0])
    assert loss.tolist() == [6.25] and grad[1].tolist() == [0.0, 0.0]
    np.testing.assert_allclose(grad[[0, 2]], [[-5.0, 0.0], [5.0, 0.0]], rtol=1e-15)                  # 2 * 2 * 2.5 * (-+3) / (3 * 1 * 2)
    # float32 in, float32 out
    out = embedding_loss_host(np.asarray([[0.0, 0.0], [3.0, 4.0]], np.float32), [7, 7], None)
    assert all(o.dtype == np.float32 for o in out)
    with pytest.raises(ValueError, match='offsets'):
        embedding_loss_host(np.zeros((3, 2)), [0, 0, 0], [0, 2, 1])
    with pytest.raises(ValueError, match='integers'):
        embedding_loss_host(np.zeros((3, 2)), [0.5, 0, 0], None)


def test_permuting_the_rows_of_a_chunk_permutes_the_gradient():
    """Every sum runs over at most n = 130 non-negative terms (the loss) or over the rows of a cluster: permuting the rows
    reorders them, which changes a float64 sum by at most n 2^-53 relative to the sum of the magnitudes; 1e-12 (1 + |value|)
    covers it as it covers the fixture bound."""
    z = load_fixture('mixed')
    x, track = z['features'], z['labels'][:, 1]
    n = x.shape[0]
    off = np.asarray([0, 50, n])
    loss, terms, grad = embedding_loss_host(x, track, off, g=[0.5, -2.0])
    rng = np.random.default_rng(3)
    perm = np.concatenate([rng.permutation(50), 50 + rng.permutation(n - 50)])
    loss_p, terms_p, grad_p = embedding_loss_host(x[perm], track[perm], off, g=[0.5, -2.0])
    assert (loss > 0).all() and not np.array_equal(perm, np.arange(n))
    np.testing.assert_allclose(loss_p, loss, rtol=1e-12)
    np.testing.assert_allclose(terms_p, terms, rtol=1e-12)
    assert (np.abs(grad_p - grad[perm]) <= 1e-12 * (1 + np.abs(grad[perm]))).all()
    assert not grad_p[track[perm] < 0].any()


def test_a_host_attach_with_the_embedding_loss():
    from tests.test_chunk_vis import VIS_MEAN, VIS_STD, vis_rule_cases, vis_stats, vis_store
    from trackmpnn_amd import ChunkSampler, EmbeddingLoss
    from trackmpnn_amd.vishead import VIS_COLS, vis_head_host
    seqs, chunks = vis_rule_cases()
    store = vis_store(seqs, '2d+temp+vis')
    sampler = ChunkSampler(store, chunks, seed=11)
    idx = np.arange(len(chunks))[::2]
    Hm, Wm, input_hw, down = 12, 40, (48, 160), 4
    mean, std = vis_stats('2d+temp+vis')
    hd = sampler.draw_host(idx, 4)
    maps = 3.0 * np.random.default_rng(5).standard_normal((hd.plan.frames.shape[0], VIS_COLS, Hm, Wm))
    logits, rows, ident, _ = vis_head_host(maps, hd.box, hd.map_of, hd.im_hw, hd.track, hd.offsets, VIS_MEAN, VIS_STD, input_hw, down)
    want = embedding_loss_host(logits, hd.track, hd.offsets)[0]
    got = hd.attach_vis(maps, mean, std, input_hw, down, embed_loss='embedding')
    assert np.array_equal(got, want) and got.shape == (idx.size,) and (got > 0).any() and not np.array_equal(got, ident)
    assert np.array_equal(hd.X[:, store.F - VIS_COLS:], rows.astype(np.float32))
    hd2 = sampler.draw_host(idx, 4)
    assert np.array_equal(hd2.attach_vis(maps, mean, std, input_hw, down), ident)                    # the default stays the identity loss
    hd3 = sampler.draw_host(idx, 4)
    tight = hd3.attach_vis(maps, mean, std, input_hw, down, embed_loss=EmbeddingLoss(0.25, 40.0))
    assert np.array_equal(tight, embedding_loss_host(logits, hd.track, hd.offsets, 0.25, 40.0)[0]) and (tight > want).any()
    with pytest.raises(ValueError, match='embed_loss'):
        sampler.draw_host(idx, 4).attach_vis(maps, mean, std, input_hw, down, embed_loss='triplet')


def test_the_device_class_refuses_the_host():
    import torch
    from trackmpnn_amd import EmbeddingLoss
    with pytest.raises(RuntimeError, match='no CPU path'):
        EmbeddingLoss()(torch.zeros(3, 128), [0, 0, 1])
    with pytest.raises(ValueError, match='delta_var'):
        EmbeddingLoss(delta_var=-1.0)
