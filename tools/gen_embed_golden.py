"""Record what the reference's EmbeddingLoss (models/loss.py:118-159) gives on seeded synthetic chunks.

    python tools/gen_embed_golden.py --reference-path DIR --out tests/golden/embed

DIR is a checkout of the reference; its models.loss is imported as it is.  Each case is one chunk, written as embed_<name>.npz:

    features   [n, 128] float32 values held in float64
    labels     [n, 2] int64 = [frame, track id] (-1: a false positive), the reference's second argument
    ref_loss   what EmbeddingLoss()(features, labels) returns for the float64 features (a float32 scalar: the reference
               accumulates in torch.tensor(0.0) whatever the feature dtype)
    ref_grad   features.grad after loss.backward(), float64 (zeros where the loss does not depend on the features)

The cases: no labelled row with rows present, no rows, one cluster, two clusters, singleton clusters (d_i = 0), ids equal mod
128 but different, two singleton clusters with identical rows (m = 0 with the hinge active: torch's subgradient of norm at 0),
and `mixed`: within-cluster noise of sigma 0.045 around centres of sigma 0.6, which puts d_i around delta_var = 0.5 and m around
delta_dist = 10 -- the tool asserts that each hinge is active on some terms and inactive on others.

The fixtures live in a directory of their own: tests/conftest.py takes every .npz directly under tests/golden for a model
fixture.  They are data; nothing of the reference's text is copied here."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W = 128
DELTA_VAR, DELTA_DIST = 0.5, 10.0


def rows(rng, n, sigma=0.6):
    return (sigma * rng.standard_normal((n, W))).astype(np.float32)


def clustered(rng, ids, noise, centre_sigma=0.6):
    """One row per entry of ids: the id's centre (sigma centre_sigma) plus noise of sigma `noise`; -1 rows are plain rows."""
    centres = {int(t): centre_sigma * rng.standard_normal(W) for t in np.unique(ids) if t >= 0}
    x = np.stack([centres[int(t)] + noise * rng.standard_normal(W) if t >= 0 else centre_sigma * rng.standard_normal(W) for t in ids])
    return x.astype(np.float32)


def cases():
    rng = np.random.default_rng([2024, 118])
    out = {}
    out['c0_rows'] = (rows(rng, 12), np.full(12, -1))
    out['n0'] = (np.zeros((0, W), np.float32), np.zeros(0, np.int64))
    ids = np.asarray([7, -1, 7, 7, -1, 7, 7, 7, -1])
    out['c1'] = (clustered(rng, ids, 0.06), ids)
    ids = np.asarray([3, 9, 3, -1, 9, 9, 3, 9, 3, 3, -1])
    out['c2'] = (clustered(rng, ids, 0.05), ids)
    out['singletons'] = (rows(rng, 7), np.asarray([4, 90, 2, 300, 17, 5, 1000]))
    ids = np.asarray([5, 133, 5, 261, 133, -1, 5, 261, 133, 261])
    out['mod128'] = (clustered(rng, ids, 0.05), ids)
    x = rows(rng, 3)
    x[2] = x[0]
    out['twins'] = (x, np.asarray([11, -1, 12]))
    ids = rng.integers(0, 14, 130) * 37                                   # 14 ids, some above 128
    ids[rng.random(130) < 0.12] = -1
    ids[[63, 64, 65]] = 37
    out['mixed'] = (clustered(rng, ids, 0.045), ids)
    return out


def hinge_states(x, ids):
    """(d_i active, d_i inactive, m active, m inactive) counts of a chunk, in float64."""
    x = x.astype(np.float64)
    cl = [np.flatnonzero(ids == t) for t in np.unique(ids) if t >= 0]
    mus = [x[c].mean(0) for c in cl]
    d = np.concatenate([np.linalg.norm(x[c] - m, axis=1) for c, m in zip(cl, mus)]) if cl else np.zeros(0)
    m = np.asarray([np.linalg.norm(a - b) for i, a in enumerate(mus) for j, b in enumerate(mus) if i != j])
    return int((d > DELTA_VAR).sum()), int((d <= DELTA_VAR).sum()), int((m < DELTA_DIST).sum()), int((m >= DELTA_DIST).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference-path', required=True)
    ap.add_argument('--out', default=os.path.join('tests', 'golden', 'embed'))
    a = ap.parse_args()
    from trackmpnn_amd.embedloss import embedding_loss_host
    sys.path.insert(0, a.reference_path)
    from models.loss import EmbeddingLoss
    crit = EmbeddingLoss(DELTA_VAR, DELTA_DIST)
    os.makedirs(a.out, exist_ok=True)
    for name, (x32, ids) in cases().items():
        n = x32.shape[0]
        assert n <= 130 and x32.dtype == np.float32
        labels = np.stack([np.arange(n) // 8, ids], axis=1).astype(np.int64).reshape(n, 2)
        feats = torch.from_numpy(x32.astype(np.float64)).requires_grad_()
        loss = crit(feats, labels)
        if loss.requires_grad:
            loss.backward()
        grad = np.zeros((n, W)) if feats.grad is None else feats.grad.numpy().astype(np.float64)
        assert loss.dtype == torch.float32 and np.isfinite(grad).all() and np.isfinite(float(loss))
        st = hinge_states(x32, ids)
        if name == 'mixed':
            assert min(st) > 0, f'mixed: a hinge has one state only {st}'
        if name == 'twins':
            assert st[2] == 2 and float(loss) == DELTA_DIST ** 2, 'twins: two ordered pairs at m = 0'
        ours = embedding_loss_host(x32.astype(np.float64), ids, None, DELTA_VAR, DELTA_DIST)
        same = (abs(ours[0][0] - float(loss)) <= 1e-5 * abs(float(loss)) and (np.abs(ours[2] - grad) <= 1e-12 * (1 + np.abs(grad))).all())
        path = os.path.join(a.out, f'embed_{name}.npz')
        np.savez_compressed(path, features=x32.astype(np.float64), labels=labels, ref_loss=np.float32(float(loss)), ref_grad=grad,
                            delta_var=np.float64(DELTA_VAR), delta_dist=np.float64(DELTA_DIST))
        print(f'{path}: {os.path.getsize(path)} bytes, {n} rows, loss {float(loss):.6g}, hinge states (d on, d off, m on, m off) {st}, '
              f'embedding_loss_host agrees: {same}')


if __name__ == '__main__':
    main()
