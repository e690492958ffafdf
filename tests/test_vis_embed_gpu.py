"""The embedding loss behind the visual head and in the training loop on the device (-m gpu): VisHead.forward(loss='embedding')
(the head's forward launches, tmpnn_embed_loss_fwd over the saved logits; backward tmpnn_embed_loss_bwd, tmpnn_vis_head_scatter),
the untouched identity default, and train_epoch(vis=VisTraining(..., embed_loss='embedding'), monitor=m).

Bounds.  The logits are a gather, bit for bit, so the loss and the gradient wrt the logits carry the bounds E_loss, E_grad of
tests/test_embed_loss_gpu.py (error_bounds, fixed there before the first run on the device).  A pixel of dmaps is the sum of
the gradient rows of its s sharers in ascending row order: the sum of their E_grad, plus s 2^-24 times the sum of their largest
magnitudes for the additions.  Pixels no labelled row of a chunk reads: exactly 0."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.test_embed_loss_gpu import EPS, error_bounds
from tests.test_vis_head import small_case
from tests.test_vis_head_gpu import MEAN, STD, special_case
from trackmpnn_amd import _lib
from trackmpnn_amd.embedloss import EmbeddingLoss, embedding_loss_host
from trackmpnn_amd.vishead import VIS_COLS, VisHead, vis_centres_host, vis_head_host, vis_pixels_host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def reference(c, g, crit=(0.5, 10.0)):
    """The float64 host results of a case: vis_head_host's gather, embedding_loss_host over the logits, a scatter in ascending
    row order; with them the bounds and the number of labelled rows of a chunk on every pixel."""
    T, _, Hm, Wm = c['maps'].shape
    logits = vis_head_host(c['maps'].astype(np.float64), c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'], MEAN, STD,
                           c['input_hw'], c['down_ratio'])[0]
    loss, terms, dlog = embedding_loss_host(logits, c['track'], c['offsets'], *crit, g=g)
    e_loss, e_grad, counts = error_bounds(logits, c['track'], c['offsets'], g, *crit)
    cy, cx, _, _ = vis_pixels_host(*vis_centres_host(c['box'], c['im_hw'], c['input_hw'], c['down_ratio']), c['map_of'], Hm, Wm)
    dmaps, bound, mag = np.zeros(c['maps'].shape), np.zeros((T, Hm, Wm)), np.zeros((T, Hm, Wm))
    sharers = np.zeros((T, Hm, Wm), np.int64)
    off = c['offsets']
    for i in range(int(off[0]), int(off[-1])):                                                      # ascending rows
        if c['track'][i] < 0:
            continue
        at = (c['map_of'][i], cy[i], cx[i])
        dmaps[at[0], :, at[1], at[2]] += dlog[i]
        bound[at] += e_grad[i]
        mag[at] += np.abs(dlog[i]).max()
        sharers[at] += 1
    return dict(loss=loss, dlog=dlog, dmaps=dmaps, e_loss=e_loss, bound=bound + sharers * EPS * mag, sharers=sharers, counts=counts)


@functools.lru_cache(maxsize=None)
def case(D):
    """small_case(D) with every seventh box pushed off the image (clamped centres), 11 track ids so that clusters have several
    rows, and maps of sigma 0.5 so that cluster means lie around delta_dist apart; its reference (computed once)."""
    c = small_case(D, seed=2)
    c['box'][::7] += np.float32(100)
    c['maps'] = (0.25 * c['maps']).astype(np.float32)
    c['track'] = np.where(c['track'] >= 0, (c['track'] % 11) * 37, -1).astype(np.int64)
    c['g'] = np.asarray([0.75, -1.25, 2.0])
    return c, reference(c, c['g'])


def run_device(c, g, loss='embedding'):
    head = VisHead(c['input_hw'], c['down_ratio'], MEAN, STD, DEV)
    maps = torch.from_numpy(c['maps']).to(DEV).requires_grad_()
    rows, ls = head.forward(maps, c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'], loss=loss)
    assert not rows.requires_grad and ls.requires_grad
    (ls * torch.from_numpy(np.asarray(g, np.float32)).to(DEV)).sum().backward()
    return rows.cpu().numpy(), ls.detach().cpu().numpy(), maps.grad.cpu().numpy(), head


def check(ref, out, what):
    _, loss, dmaps, head = out
    rec = head.embed_record()
    assert np.array_equal(rec['labelled'], ref['counts'][:, 0]) and np.array_equal(rec['clusters'], ref['counts'][:, 1])
    err_l = np.abs(loss - ref['loss'])
    err_d = np.abs(dmaps - ref['dmaps']).max(axis=1)
    touched = ref['sharers'] > 0
    print(f'{what}: loss err / bound {(err_l / np.where(ref["e_loss"] > 0, ref["e_loss"], 1)).max(initial=0):.3g}, dmaps err / bound '
          f'{(err_d[touched] / ref["bound"][touched]).max(initial=0):.3g} (each must be <= 1); dmaps err / (1 + |value|) '
          f'{(np.abs(dmaps - ref["dmaps"]) / (1 + np.abs(ref["dmaps"]))).max(initial=0):.3g}, max |dmaps| {np.abs(ref["dmaps"]).max(initial=0):.3g}')
    assert (err_l <= ref['e_loss']).all() and (err_d <= ref['bound']).all()
    assert (dmaps[np.broadcast_to(~touched[:, None], dmaps.shape)] == 0).all()                      # untouched pixels: exactly 0


@pytest.mark.parametrize('D', [1, 65, 130])
def test_head_with_the_embedding_loss_equals_the_host(D):
    c, ref = case(D)
    if D >= 65:
        assert (ref['sharers'] > 1).any() and (ref['counts'][:, 1] > 1).any() and np.abs(ref['dmaps']).max() > 1e-3
    out = run_device(c, c['g'])
    check(ref, out, f'D={D}')
    plain = VisHead(c['input_hw'], c['down_ratio'], MEAN, STD, DEV).rows(torch.from_numpy(c['maps']).to(DEV), c['box'], c['map_of'], c['im_hw'])
    assert np.array_equal(out[0].view(np.int32), plain.cpu().numpy().view(np.int32))                # the rows are the head's own
    if D == 65:
        again = run_device(c, c['g'])
        assert np.array_equal(again[2].view(np.int32), out[2].view(np.int32)) and np.array_equal(again[1].view(np.int32), out[1].view(np.int32))
        tight = EmbeddingLoss(0.25, 12.0)                                                           # an instance: other deltas
        ref2 = reference(c, c['g'], (0.25, 12.0))
        check(ref2, run_device(c, c['g'], loss=tight), 'D=65, deltas (0.25, 12)')
        assert not np.array_equal(ref2['loss'], ref['loss'])
        with pytest.raises(ValueError, match='loss='):
            run_device(c, c['g'], loss='triplet')


def test_sharers_of_two_clusters_on_one_pixel():
    """Rows 0-4 read one pixel and belong to the clusters 7 (rows 0, 2), 135, 300 and 2: their logits are equal, so inside the
    pixel d_i = 0 and m = 0 (direction terms 0, the hinge at its full delta_dist), and the pixel's gradient is the sum over
    five rows of four clusters of what the clusters elsewhere push with.  Chunk 2 holds no labelled row."""
    c = special_case()
    c['maps'] = (0.25 * c['maps']).astype(np.float32)                                               # pixels about 8 apart: the hinge is active
    ref = reference(c, np.ones(3))
    assert ref['sharers'][0, 2, 3] == 5 and ref['counts'].tolist() == [[6, 5], [3, 2], [0, 0]] and ref['loss'][2] == 0
    assert np.abs(ref['dmaps'][0, :, 2, 3]).max() > 1e-3
    out = run_device(c, np.ones(3))
    check(ref, out, 'special')
    assert out[1][2] == 0.0                                                                         # exactly


def test_the_identity_default_is_what_it_was():
    """forward() without `loss`, and with loss='identity', through the changed signature: the loss and dmaps of
    tmpnn_vis_head_fwd / tmpnn_vis_head_bwd called directly, bit for bit."""
    c, _ = case(65)
    for kw in ({}, {'loss': 'identity'}):
        head = VisHead(c['input_hw'], c['down_ratio'], MEAN, STD, DEV)
        maps = torch.from_numpy(c['maps']).to(DEV).requires_grad_()
        _, loss = head.forward(maps, c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'], **kw)
        g = torch.from_numpy(c['g'].astype(np.float32)).to(DEV)
        (loss * g).sum().backward()
        call = head._last
        direct = torch.full(tuple(maps.shape), 7.0, device=DEV)
        _lib.call('tmpnn_vis_head_bwd', C.byref(call.c), g.data_ptr(), direct.data_ptr(), _lib.raw_stream(torch.device(DEV)))
        assert torch.equal(maps.grad.view(torch.int32), direct.view(torch.int32)) and direct.abs().max() > 0
        assert torch.equal(loss.detach().view(torch.int32), call.loss.view(torch.int32))
        want = vis_head_host(c['maps'].astype(np.float64), c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'], MEAN, STD,
                             c['input_hw'], c['down_ratio'])[2]
        np.testing.assert_allclose(loss.detach().cpu().numpy(), want, rtol=1e-5)                    # (the identity loss, not the embedding loss)


def torch_embedding_loss(f, track, delta_var=0.5, delta_dist=10.0):
    """The rule of the module docstring of trackmpnn_amd.embedloss for one chunk in torch operations (float64, autograd)."""
    lab = track >= 0
    f, ids = f[lab], track[lab]
    uniq, inv = torch.unique(ids, return_inverse=True)
    Cn = int(uniq.numel())
    if Cn == 0:
        return f.sum() * 0
    onehot = torch.nn.functional.one_hot(inv, Cn).to(f.dtype)
    cnt = onehot.sum(0)
    mu = (onehot.t() @ f) / cnt[:, None]
    d = (f - mu[inv]).norm(dim=1)
    loss = (torch.relu(d - delta_var) ** 2 / cnt[inv]).sum() / Cn
    if Cn > 1:
        i, j = torch.nonzero(~torch.eye(Cn, dtype=torch.bool), as_tuple=True)
        loss = loss + (torch.relu(delta_dist - (mu[i] - mu[j]).norm(dim=1)) ** 2).sum() / (Cn * (Cn - 1))
    return loss


def test_autograd_through_a_convolution():
    """A one-layer convolution as the CNN: loss.sum().backward() through VisHead(loss='embedding') against the same graph from
    torch indexing and torch operations in float64 on the CPU.  The float32 convolution in front of the head rounds its 27-term
    sums (plus the bias): a logit differs from the float64 one by at most 29 * 2^-24 times the sum of the magnitudes of its
    terms, which error_bounds takes as x_err.  The weight gradient is the convolution's backward over dmaps: its bound is that
    backward over the bound of dmaps, plus the float32 rounding of the backward's own sum over at most D touched pixels."""
    T, Hm, Wm = 2, 12, 20
    c = small_case(24, seed=6, T=T, Hm=Hm, Wm=Wm)
    c['input_hw'], c['down_ratio'] = (Hm, Wm), 1
    c['offsets'] = np.asarray([0, 9, 24], np.int64)
    c['track'] = np.where(c['track'] >= 0, (c['track'] % 4) * 130, -1).astype(np.int64)
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(3, VIS_COLS, 3, padding=1)
    with torch.no_grad():
        conv.weight.mul_(6.0)                                                                       # logits of sigma about 1: d_i above delta_var
    img = torch.randn(T, 3, Hm, Wm)
    c64 = torch.nn.Conv2d(3, VIS_COLS, 3, padding=1).double()
    c64.load_state_dict({k: v.double() for k, v in conv.state_dict().items()})
    m64 = c64(img.double())
    m64.retain_grad()
    cy, cx, _, _ = vis_pixels_host(*vis_centres_host(c['box'], c['im_hw'], c['input_hw'], 1), c['map_of'], Hm, Wm)
    lg = m64[torch.from_numpy(c['map_of']), :, torch.from_numpy(cy), torch.from_numpy(cx)]
    off, tr = c['offsets'], torch.from_numpy(c['track'])
    ref_loss = torch.stack([torch_embedding_loss(lg[off[b]:off[b + 1]], tr[off[b]:off[b + 1]]) for b in range(2)])
    ref_loss.sum().backward()
    # the bounds, from the float64 logits
    mag = torch.nn.functional.conv2d(img.double().abs(), c64.weight.detach().abs(), c64.bias.detach().abs(), padding=1)
    x_err = float(29 * EPS * mag.max())
    e_loss, e_grad, counts = error_bounds(lg.detach().numpy(), c['track'], off, np.ones(2), x_err=x_err)
    assert (counts[:, 1] > 1).all() and (ref_loss > 0).all()
    dm = m64.grad
    E = torch.zeros(T, Hm, Wm, dtype=torch.float64)
    for i in range(24):
        if c['track'][i] >= 0:
            E[c['map_of'][i], cy[i], cx[i]] += e_grad[i]
    E = E[:, None] + 24 * EPS * dm.abs()
    bound_w = torch.nn.grad.conv2d_weight(img.double().abs(), tuple(c64.weight.shape), E.expand_as(dm).contiguous(), padding=1)
    bound_b = E.expand_as(dm).sum((0, 2, 3))
    # the device
    conv = conv.to(DEV)
    head = VisHead(c['input_hw'], 1, MEAN, STD, DEV)
    _, loss = head.forward(conv(img.to(DEV)), c['box'], c['map_of'], c['im_hw'], c['track'], c['offsets'], loss='embedding')
    loss.sum().backward()
    el = np.abs(loss.detach().cpu().numpy() - ref_loss.detach().numpy())
    ew = (conv.weight.grad.cpu().double() - c64.weight.grad).abs()
    eb = (conv.bias.grad.cpu().double() - c64.bias.grad).abs()
    print(f'autograd: loss err / bound {(el / e_loss).max():.3g}, weight-gradient err / bound {(ew / bound_w).max():.3g}, bias '
          f'{(eb / bound_b).max():.3g} (<= 1); max |dW| {c64.weight.grad.abs().max():.3g}, max err {ew.max():.3g}, max bound {bound_w.max():.3g}')
    assert c64.weight.grad.abs().max() > 1e-2
    assert (el <= e_loss).all() and (ew <= bound_w).all() and (eb <= bound_b).all()


def test_fold_embed_is_an_fp64_sum_over_the_kept_chunks():
    """float32 values are exact in float64 and 700 of them below 2^7 add without rounding beyond 2^-53 relative per addition:
    the mean equals numpy's float64 mean within 700 * 2^-53 relative.  An index outside loss_d is counted and read() raises."""
    from trackmpnn_amd import TrainMonitor
    rng = np.random.default_rng(8)
    ld = (100 * rng.random(700)).astype(np.float32)
    kept = np.sort(rng.choice(700, 300, replace=False)).astype(np.int64)
    m = TrainMonitor(DEV)
    m.fold_embed(torch.from_numpy(ld).to(DEV), torch.from_numpy(kept).to(DEV))
    m.fold_embed(torch.from_numpy(ld[:5]).to(DEV))                                                  # kept = None: every chunk
    got = m.read()
    want = (ld[kept].astype(np.float64).sum() + ld[:5].astype(np.float64).sum()) / 305
    assert abs(got['avg_loss_d'] - want) <= 700 * 2.0 ** -53 * want
    assert np.isnan(got['avg_loss']) and np.isnan(got['avg_loss_total']) and got['chunks'] == 0     # (no chunk was folded)
    record = m.embed_record.cpu().numpy()
    assert record[1] == 305 and record[2] == 0
    m.fold_embed(torch.from_numpy(ld).to(DEV), torch.tensor([3, 700, -1], device=DEV))
    with pytest.raises(RuntimeError, match='2 chunk indices outside'):
        m.read()
    m.reset()
    assert 'avg_loss_d' not in m.read()
    with pytest.raises(ValueError, match='int64'):
        m.fold_embed(torch.from_numpy(ld).to(DEV), torch.tensor([3], dtype=torch.int32, device=DEV))


def test_train_epoch_with_the_embedding_loss_and_the_monitor():
    """One step of train_epoch(vis=VisTraining(..., embed_loss='embedding'), monitor=m) on the tiny store of
    tests/test_chunk_vis_gpu.py: the embedding CNN's parameters change, and avg_loss_d is the mean of the kept chunks' loss_d
    computed on the host from the same draw and the same maps (the CNN's float32 output), within the mean of their E_loss."""
    from tests.test_chunk_vis_gpu import _fresh, _state, _vis_training_set
    from trackmpnn_amd import TrainMonitor, VisTraining
    from trackmpnn_amd.loops import train_epoch
    today = {'avg_f1', 'avg_loss_c', 'avg_loss_f', 'avg_loss', 'forwards', 'chunks'}
    sampler, fs, hw = _vis_training_set()
    epoch = 2
    order = sampler.epoch_order(epoch)
    # the host, from the same draw
    _, net0, _, _, head0 = _fresh(hw)
    drawn = sampler.draw(order, epoch)
    kept = np.asarray(drawn.batch().kept)
    with torch.no_grad():
        maps = net0(fs.gather(drawn.plan)).cpu().numpy()
    off = drawn.offsets.cpu().numpy()
    nd = int(off[-1])
    track = drawn.track[:nd].cpu().numpy().astype(np.int64)
    logits = vis_head_host(maps.astype(np.float64), drawn.box[:nd].cpu().numpy(), drawn.map_of[:nd].cpu().numpy().astype(np.int64),
                           drawn.im_hw[:nd].cpu().numpy(), track, off, head0.mean, head0.std, hw, 1)[0]
    want = embedding_loss_host(logits, track, off)[0]
    e_loss = error_bounds(logits, track, off, np.ones(off.size - 1))[0]
    assert 0 < kept.size < len(order) and (want[kept] > 0).all()
    # the device
    model, net, opt, net_opt, head = _fresh(hw)
    before = _state(model, net)
    m = TrainMonitor(DEV)
    assert set(m.read()) == today                                                                   # no fold_embed: today's keys
    steps = train_epoch(model, sampler, opt, len(order), epoch, monitor=m, vis=VisTraining(head, fs, net, net_opt, embed_loss='embedding'))
    assert steps == 1 and net.calls == 1
    after = _state(model, net)
    assert not any(torch.equal(a, b) for a, b in zip(before[1], after[1]))                          # the CNN's weight and bias moved
    stats = m.read()
    assert set(stats) == today | {'avg_loss_d', 'avg_loss_total'} and stats['chunks'] == kept.size
    err, bound = abs(stats['avg_loss_d'] - want[kept].mean()), e_loss[kept].mean() + EPS * want[kept].mean()
    print(f'train_epoch: avg_loss_d {stats["avg_loss_d"]:.6g}, host {want[kept].mean():.6g}, err / bound {err / bound:.3g} (<= 1)')
    assert err <= bound
    assert stats['avg_loss_total'] == stats['avg_loss_d'] + stats['avg_loss']
    assert head.embed_record()['clusters'].sum() > 0
    m.reset()
    assert set(m.read()) == today
    # the identity loss is folded as well
    model, net, opt, net_opt, head = _fresh(hw)
    train_epoch(model, sampler, opt, len(order), epoch, monitor=m, vis=VisTraining(head, fs, net, net_opt))
    ident = m.read()
    assert set(ident) == today | {'avg_loss_d', 'avg_loss_total'} and 3.0 < ident['avg_loss_d'] < 7.0   # about log(128)
