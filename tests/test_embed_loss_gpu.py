"""The embedding loss on the device (-m gpu; csrc/embedloss.hip: tmpnn_embed_loss_fwd, tmpnn_embed_loss_bwd;
trackmpnn_amd.embedloss.EmbeddingLoss) against the host definition embedding_loss_host in float64.

Bounds.  Counts: integers, exact.  Gradient of a row without a label or a chunk: exactly 0.  Loss, terms, gradient: the device
works in float32 (eps = 2^-24) through four kinds of sums -- the n_c-term mean of a cluster, the W-term norms (a butterfly), the
C-term walk over the other leaders and the n-term reduction of a chunk -- and two hinges that subtract a constant from a norm, so
the absolute error of the norm, not its relative error, is what reaches the result.  `error_bounds` evaluates the first-order
worst case from the float64 intermediates, cluster by cluster and row by row (a sum of k terms in ANY order errs by at most
k eps times the sum of the magnitudes; C clusters, n labelled rows, n_c rows in cluster c):

    e2_c  = n_c eps |max_i |x_i||_2,  e1_c = n_c eps max |x|     the mean of cluster c (n_c - 1 additions and a division): the
                                                           2-norm of its error and the error of one channel
    e_d_i = e2_c + (W / 2 + 2) eps d_i                     d_i: the mean's error moves it by at most |d mu|_2; the W-term sum of
                                                           squares and the root add (W + 1) / 2 + 1 roundings, relative
    e_m   = e2_c + e2_c' + (W / 2 + 2) eps m               m of a pair, likewise, with two means
    E_loss = (1 / C) sum_i (2 h_i e_d_i + e_d_i^2) / n_c + (1 / (C (C - 1))) sum_pairs (2 hd e_m + e_m^2)
             + (n + 2 C + 10) eps |loss|
             (h = relu(d - delta_var), hd = relu(delta_dist - m): (h + e)^2 - h^2 = 2 h e + e^2, weighted as the terms weigh
             them; then the reductions' own roundings)
    e_u_i = (2 / (C n_c)) [e_d_i + (h_i / d_i) (e1_c + 2 eps d_i) + 6 eps h_i]      (the first term only where d_i + e_d_i >
             delta_var) a channel of u_i = (2 / (C n_c)) (h / d) (x - mu): h / d = 1 - delta_var / d has slope delta_var / d^2
             where h > 0, |x - mu| <= d channel by channel, and delta_var / d <= 1 there
    e_v_c = (4 / (C (C - 1))) sum_c' [delta_dist e_m / (m - e_m) + (hd / m) (e1_c + e1_c' + 2 eps m) + (C + 6) eps hd]
             (the first term only where m - e_m < delta_dist) a channel of v_c, term by term: (hd / m) (mu_c - mu_c') with
             |mu_c - mu_c'| <= m channel by channel and slope delta_dist / m^2 of hd / m
    E_grad_k = |g| [e_u_k + (e_v_c + sum_{i in c} e_u_i + n_c eps sum_i |u_i|) / n_c + 6 eps (|u_k| + |t_c|)]
             g (u_k + (v_c - sum u_i) / n_c), with |u_i| <= (2 / (C n_c)) h_i and |v_c| <= (4 / (C (C - 1))) sum hd a channel

Both are fixed here, before the first run on the device.  Every comparing test prints the measured maxima in units of its bound
and, for orientation, in units of (1 + |value|); profiles/embed_loss.md records them."""
import functools

import numpy as np
import pytest
import torch

from trackmpnn_amd.embedloss import EmbeddingLoss, embedding_loss_host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -24


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def error_bounds(x, track, offsets, g, delta_var=0.5, delta_dist=10.0, x_err=0.0):
    """(E_loss [B], E_grad [D], counts [B, 2] = labelled rows, clusters) of the module docstring from the float64 intermediates.
    x_err: what a channel of the device's rows may differ by from x (rows a float32 network computed): a mean and a difference
    x - mu then move by at most 2 x_err a channel, 2 sqrt(W) x_err in the 2-norm."""
    x, track, off = np.asarray(x, np.float64), np.asarray(track), np.asarray(offsets)
    (D, W), B = x.shape, off.size - 1
    loss = embedding_loss_host(x, track, off, delta_var, delta_dist)[0]
    e_loss, e_grad, counts = np.zeros(B), np.zeros(D), np.zeros((B, 2), np.int64)
    kw = (W / 2 + 2) * EPS
    for b in range(B):
        rows = np.arange(off[b], off[b + 1])
        rows = rows[track[rows] >= 0]
        ids = np.unique(track[rows])
        n, C = rows.size, ids.size
        counts[b] = (n, C)
        if C == 0:
            continue
        members = [rows[track[rows] == t] for t in ids]
        mus = [x[c].mean(0) for c in members]
        e2 = [c.size * EPS * np.linalg.norm(np.abs(x[c]).max(0)) + 2 * np.sqrt(W) * x_err for c in members]
        e1 = [c.size * EPS * np.abs(x[c]).max() + 2 * x_err for c in members]
        pairs = C * (C - 1)
        acc = (n + 2 * C + 10) * EPS * abs(loss[b])
        e_v, vmax = np.zeros(C), np.zeros(C)
        for k in range(C):
            for k2 in range(C):
                m = np.linalg.norm(mus[k] - mus[k2])
                if k2 == k or m == 0:
                    continue
                hd, e_m = max(delta_dist - m, 0.0), e2[k] + e2[k2] + kw * m
                acc += (2 * hd * e_m + e_m ** 2) / pairs
                assert m > 2 * e_m                                                                  # (a condition on the inputs)
                slope = delta_dist * e_m / (m - e_m) if m - e_m < delta_dist else 0.0
                e_v[k] += (4.0 / pairs) * (slope + (hd / m) * (e1[k] + e1[k2] + 2 * EPS * m) + (C + 6) * EPS * hd)
                vmax[k] += (4.0 / pairs) * hd
        for k, c in enumerate(members):
            nc = c.size
            d = np.linalg.norm(x[c] - mus[k], axis=1)
            h = np.maximum(d - delta_var, 0)
            e_d = e2[k] + kw * d
            acc += ((2 * h * e_d + e_d ** 2) / nc).sum() / C
            q = 2.0 / (C * nc)
            ratio = np.divide(h, d, out=np.zeros_like(d), where=d > 0)
            e_u = q * (e_d * (d + e_d > delta_var) + ratio * (e1[k] + 2 * EPS * d) + 6 * EPS * h)
            umax = q * h
            e_t = (e_v[k] + e_u.sum() + nc * EPS * umax.sum()) / nc
            tmax = (vmax[k] + umax.sum()) / nc
            e_grad[c] = abs(g[b]) * (e_u + e_t + 6 * EPS * (umax + tmax))
        e_loss[b] = acc
    return e_loss, e_grad, counts


def clustered(rng, ids, W):
    """Rows around one centre per id: noise of sigma 0.6 / sqrt(W) (d_i around delta_var = 0.5) and centres of sigma
    7.07 / sqrt(W) (m around delta_dist = 10), so both hinges take both states where a chunk is large enough."""
    centres = {int(t): (7.07 / np.sqrt(W)) * rng.standard_normal(W) for t in np.unique(ids)}
    return np.stack([centres[int(t)] + (0.6 / np.sqrt(W)) * rng.standard_normal(W) for t in ids]).astype(np.float32).reshape(len(ids), W)


@functools.lru_cache(maxsize=None)
def case(n, W):
    """Three chunks of n, 0 and 65 rows, and the float64 reference (computed once).  The first chunk: every id on about 8 rows;
    at n >= 63 one cluster on the chunk's rows 3, 62, 63 and (n >= 65) 64, 65, 129: its rows straddle the multiples of 64 of both
    scans; at n = 2 false positives only.  The last chunk: a cluster on its rows 0, 63 and 64; the id 37 of the first chunk again
    (another cluster there); ids equal mod 128."""
    rng = np.random.default_rng([n, W, 5])
    a = rng.integers(0, max(2, n // 8), n) * 37 + 37
    a[rng.random(n) < 0.15] = -1
    a[[i for i in (3, 62, 63, 64, 65, 129) if i < n]] = 5
    if n == 2:
        a[:] = -1
    if n == 1:
        a[:] = 9
    c = rng.integers(0, 8, 65) * 128 + 37                                    # 37, 165, 293, ...: equal mod 128
    c[rng.random(65) < 0.15] = -1
    c[[0, 63, 64]] = 6
    c[1] = 37
    track = np.concatenate([a, c]).astype(np.int64)
    x = clustered(rng, np.where(track >= 0, track, 10 ** 6 + np.arange(track.size)) + 10 ** 7 * (np.arange(track.size) >= n), W)
    offsets = np.asarray([0, n, n, n + 65], np.int64)
    g = np.asarray([0.75, -1.25, 2.0])
    loss, terms, grad = embedding_loss_host(x.astype(np.float64), track, offsets, g=g)
    e_loss, e_grad, counts = error_bounds(x, track, offsets, g)
    return dict(x=x, track=track, offsets=offsets, g=g, loss=loss, terms=terms, grad=grad, e_loss=e_loss, e_grad=e_grad, counts=counts)


def run_device(c, pad=0, crit=None, offsets=None):
    """(loss, terms, grad as numpy; the criterion) of one forward + backward; pad > 0: the rows lie in a wider tensor."""
    crit = crit or EmbeddingLoss()
    D, W = c['x'].shape
    big = torch.full((D, W + pad), -7.5, device=DEV)
    big[:, :W] = torch.from_numpy(c['x']).to(DEV)
    f = (big[:, :W] if pad else big).detach().requires_grad_()
    loss = crit(f, c['track'], c['offsets'] if offsets is None else offsets)
    assert loss.requires_grad and tuple(loss.shape) == (c['offsets'].size - 1,)
    (loss * torch.from_numpy(c['g'].astype(np.float32)).to(DEV)).sum().backward()
    return loss.detach().cpu().numpy(), crit.last_terms().cpu().numpy(), f.grad.cpu().numpy(), crit


def check(c, out, what):
    loss, terms, grad, crit = out
    rec = crit.record()
    B = c['offsets'].size - 1
    assert np.array_equal(rec['labelled'], c['counts'][:, 0]) and np.array_equal(rec['clusters'], c['counts'][:, 1])
    assert np.array_equal(rec['rows'], np.diff(c['offsets']))
    assert loss.dtype == np.float32 and grad.dtype == np.float32 and grad.shape == c['x'].shape
    assert not grad[c['track'] < 0].any()                                                            # exactly 0
    err_l = np.abs(loss - c['loss'])
    err_t = np.abs(terms - c['terms']).max(axis=1)
    err_g = np.abs(grad - c['grad']).max(axis=1) if grad.size else np.zeros(0)
    unit = lambda e, b: (e / np.where(b > 0, b, 1.0)).max(initial=0)
    rel_g = (np.abs(grad - c['grad']) / (1 + np.abs(c['grad']))).max(initial=0)
    print(f'{what}: loss err / bound {unit(err_l, c["e_loss"]):.3g}, terms {unit(err_t, c["e_loss"]):.3g}, gradient '
          f'{unit(err_g, c["e_grad"]):.3g} (each must be <= 1); in units of (1 + |value|): loss '
          f'{(err_l / (1 + np.abs(c["loss"]))).max():.3g}, gradient {rel_g:.3g}; largest bounds: loss {c["e_loss"].max():.3g}, '
          f'gradient {c["e_grad"].max():.3g}')
    assert (err_l <= c['e_loss']).all() and (err_t <= c['e_loss']).all() and (err_g <= c['e_grad']).all()
    assert (loss[c['counts'][:, 1] == 0] == 0).all()                                                 # exactly


@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, 130])
def test_device_equals_the_host(n):
    c = case(n, 128)
    assert c['counts'][1].tolist() == [0, 0] and c['loss'][1] == 0 and c['counts'][2, 1] >= 5
    if n >= 63:
        assert (c['terms'][[0, 2]] > 0).all()                                                        # both terms live in both chunks
        assert 37 in c['track'][:n] and 37 in c['track'][n:]
    if n == 2:
        assert c['counts'][0].tolist() == [0, 0]
    check(c, run_device(c), f'n={n} W=128')


@pytest.mark.parametrize('W', [1, 3, 64, 130])
def test_other_widths_and_a_row_stride(W):
    c = case(65, W)
    assert (c['loss'][[0, 2]] > 0).all()
    check(c, run_device(c, pad=5), f'n=65 W={W} ld={W + 5}')


def test_two_runs_give_the_same_bits():
    for n, W, pad in ((130, 128, 0), (65, 130, 5)):
        a, b = run_device(case(n, W), pad), run_device(case(n, W), pad)
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u.view(np.int32), v.view(np.int32))
        assert a[2].any()


def test_bad_offsets_are_counted_not_followed():
    """Every array is exactly as long as its valid part.  Offsets beyond D and descending offsets are clamped and counted
    (record() raises); a row belongs to the first chunk whose clamped bounds hold it, so the chunks untouched by the bad
    boundary give what the host gives for them."""
    c = case(65, 128)
    D = c['x'].shape[0]
    for bad, good in (([0, 20, D + 10], [0, 20, 20]), ([0, 20, 10, D], [0, 20, 20, D]), ([-5, 20, D], [20, 20, D])):
        k = dict(c, offsets=np.asarray(good, np.int64), g=c['g'][:len(good) - 1])
        want_loss, _, want_grad = embedding_loss_host(c['x'].astype(np.float64), c['track'], k['offsets'], g=k['g'])
        e_loss, e_grad, _ = error_bounds(c['x'], c['track'], k['offsets'], k['g'])
        loss, _, grad, crit = run_device(k, offsets=torch.tensor(bad, dtype=torch.int32, device=DEV))
        with pytest.raises(RuntimeError, match='offsets'):
            crit.record()
        for b in range(len(good) - 1):
            lo, hi = good[b], good[b + 1]
            if bad[b] != lo or bad[b + 1] != hi or hi == lo:                                         # (a chunk the bad boundary touches)
                continue
            assert abs(loss[b] - want_loss[b]) <= e_loss[b] and want_loss[b] > 0
            assert (np.abs(grad[lo:hi] - want_grad[lo:hi]).max(axis=1) <= e_grad[lo:hi]).all()
        assert np.isfinite(loss).all() and np.isfinite(grad).all()
    crit = EmbeddingLoss()
    f = torch.from_numpy(c['x']).to(DEV)
    with pytest.raises(ValueError, match='offsets'):
        crit(f, c['track'], [0, 40, 30, D])
    wide = c['track'].copy()
    wide[5] = 2 ** 31
    with pytest.raises(ValueError, match='track outside int32'):
        crit(f, wide, c['offsets'])
    with pytest.raises(RuntimeError, match='no CPU path'):
        crit(f.cpu(), c['track'], c['offsets'])
    with pytest.raises(ValueError, match='W <= 1024'):
        crit(torch.zeros((2, 1025), device=DEV), [0, 0])


def test_one_chunk_without_offsets_and_other_deltas():
    """The reference's call shape: features and ids of one chunk; the deltas are constructor arguments."""
    c = case(65, 128)
    x, track = c['x'][:65], c['track'][:65]
    crit = EmbeddingLoss(0.25, 12.0)
    f = torch.from_numpy(x).to(DEV).requires_grad_()
    loss = crit(f, torch.from_numpy(track).to(DEV))
    loss.sum().backward()
    want_loss, _, want_grad = embedding_loss_host(x.astype(np.float64), track, None, 0.25, 12.0)
    e_loss, e_grad, counts = error_bounds(x, track, [0, 65], [1.0], 0.25, 12.0)
    assert tuple(loss.shape) == (1,) and abs(float(loss.detach()) - want_loss[0]) <= e_loss[0]
    assert (np.abs(f.grad.cpu().numpy() - want_grad).max(axis=1) <= e_grad).all()
    assert crit.record()['clusters'].tolist() == [counts[0, 1]]
    w = torch.ones_like(loss).requires_grad_()
    (d,) = torch.autograd.grad((crit(f, track) * w).sum(), f, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        d.sum().backward()
