"""The training-loss kernels (csrc/loss.hip) against float64 at their structural edges (-m gpu).

`train_losses` (the one-launch kernel k_train_losses_fwd / _bwd up to 8192 rows per side, the separate entry points beyond) and
`train_losses_windows` (k_train_losses_win_fwd / _bwd) on graphs built row by row with `graph_from_edges`, in both modes (with
the TP classifier and without), at the sizes where the code changes: the ordered sum's 128-row chunks, the one-launch limit, a
thread of the one-launch kernel that takes a second det (Dn > 1024), the windowed kernel's fold after 16 chunks.

Reference: the CPU oracle's create_targets / ce_loss / focal_loss (the restatement of models/loss.py that
tests/test_loss.py pins to the reference) evaluated in float64 on the float32 inputs, autograd for the gradients.  One thing is
kept as the reference's float32 forms it: the argument of the focal logarithm, q = fl32(fl32(t ? s : 1 - s) + fl32(1e-10)) --
at s = 0 or s = 1 that rounding IS the value (log(1e-10) or log(1)), so a float64 q would be another function.  The logarithm,
the means and every sum are float64.  Upstream factors 0.7 on loss_c and 1.3 on loss_f.

Tolerances (tests/test_loss.py::test_hip_losses_at_scale_vs_torch's): values 1e-5 max(1, |ref|); d_logits atol 1e-6, rtol 1e-4;
d_scores rtol 1e-4 plus 1e-6 max|ref| (saturated rows reach 1e10 / E); targets exact."""
import numpy as np
import pytest
import torch

from oracle import trackmpnn_oracle as orc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GC, GF = 0.7, 1.3


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


# ---- graphs: (N, is_edge [N], src [E], dst [E]) with src row < edge row < dst row ------------------------------------------------
def _bipartite(n0, n1, pairs=None, seed=0):
    """Two frames: n0 dets, the edge rows, n1 dets.  pairs: [E, 2] (i, j) or None = all n0 x n1, in a shuffled row order."""
    rng = np.random.RandomState(seed)
    if pairs is None:
        pairs = np.stack(np.meshgrid(np.arange(n0), np.arange(n1), indexing='ij'), -1).reshape(-1, 2)
    pairs = pairs[rng.permutation(pairs.shape[0])]
    E = pairs.shape[0]
    is_edge = np.zeros(n0 + E + n1, bool)
    is_edge[n0:n0 + E] = True
    return n0 + E + n1, is_edge, pairs[:, 0].astype(np.int64), (n0 + E + pairs[:, 1]).astype(np.int64)


def _sparse_two_frames(seed=3):
    """700 + 700 dets, 1500 distinct random edges: Dn = 1400 > 1024 threads, dets without any edge on both sides.  (In a
    two-frame graph a det has future edges only or past edges only by construction; dets with edges on both sides, and sets
    with several positives, are the three-frame case's.)"""
    rng = np.random.RandomState(seed)
    flat = rng.choice(700 * 700, 1500, replace=False)
    g = _bipartite(700, 700, np.stack([flat // 700, flat % 700], 1), seed)
    deg0, deg1 = np.bincount(g[2], minlength=700), np.bincount(g[3] - 700 - 1500, minlength=700)
    assert (deg0 == 0).any() and (deg1 == 0).any() and (deg0 > 1).any() and (deg1 > 1).any()
    return g


def _three_frames():
    """6 + 6 + 6 dets; rows: frame 0, edges 0->1, frame 1, edges into frame 2, frame 2.  Labels follow tracks (a det: 1 unless
    a false positive; an edge: 1 where both ends carry the same track).  Tracks 0, 1 and 2 are present in all three frames: their
    frame-0 det has two positive future edges (the FIRST, its 0->1 edge, is the target) and their frame-2 det two positive past
    edges (the LAST is the target).  The edges into a frame-2 det are listed 0->2 first for an even det, 1->2 first for an odd
    one, so the 0->2 edge of tracks 0 and 2 is positive and NOT a target (neither end chooses it), and the 0->2 edge of
    track 1 is a target although its own src det chose another -- it is set from its other endpoint.
    Returns ((N, is_edge, src, dst), labels uint8 [N], rows of the 0->2 edges, their track or -1)."""
    tracks = [np.array([0, 1, 2, 3, -1, 4]), np.array([1, 0, 2, -1, 5, 3]), np.array([2, 5, 0, 1, -1, -1])]
    r0, r01, r1, r2x, r2 = 0, 6, 42, 48, 120
    N = 126
    src = [r0 + i for i in range(6) for j in range(6)]
    dst = [r1 + j for i in range(6) for j in range(6)]
    from_f0 = [False] * 36
    for j in range(6):
        for f0 in ((True, False) if j % 2 == 0 else (False, True)):
            src += [(r0 if f0 else r1) + i for i in range(6)]
            dst += [r2 + j] * 6
            from_f0 += [f0] * 6
    src, dst, from_f0 = np.array(src, np.int64), np.array(dst, np.int64), np.array(from_f0)
    is_edge = np.zeros(N, bool)
    is_edge[r01:r1] = True
    is_edge[r2x:r2] = True
    trk = np.full(N, -2)
    trk[r0:r0 + 6], trk[r1:r1 + 6], trk[r2:r2 + 6] = tracks
    labels = np.zeros(N, np.uint8)
    labels[~is_edge] = trk[~is_edge] >= 0
    same = (trk[src] == trk[dst]) & (trk[src] >= 0)
    labels[is_edge] = same
    rows = np.flatnonzero(is_edge)
    return (N, is_edge, src, dst), labels, rows[from_f0], np.where(same, trk[src], -1)[from_f0]


# name -> (graph builder, labels: None = Bernoulli(0.3) | 'zeros' | 'ones' | array, one-launch kernel expected)
_CASES = {
    '1x1': (lambda: _bipartite(1, 1), None, True),                                  # smallest graph
    '127x1': (lambda: _bipartite(127, 1), None, True),                              # below one chunk
    '8x16': (lambda: _bipartite(8, 16), None, True),                                # exactly one chunk
    '3x43': (lambda: _bipartite(3, 43), None, True),                                # one row into the second chunk
    '64x128': (lambda: _bipartite(64, 128), None, True),                            # the one-launch limit: E = 8192
    '64x129': (lambda: _bipartite(64, 129), None, False),                           # over it: the separate entry points
    'sparse_700_700': (_sparse_two_frames, None, True),                             # Dn = 1400: a thread's second det
    'three_frames': (lambda: _three_frames()[0], 'tracks', True),                   # several positives per set
    '3x43_labels_zero': (lambda: _bipartite(3, 43), 'zeros', True),
    '8x16_labels_one': (lambda: _bipartite(8, 16), 'ones', True),
}


def _oracle_graph(N, is_edge, src, dst):
    return orc.OracleGraph(N, is_edge.copy(), src.copy(), dst.copy(), np.flatnonzero(is_edge), np.flatnonzero(~is_edge))


def _inputs(og, labels, seed):
    """logits ~ N(0, 8) clamped to +-40; scores = sigmoid of independent logits of the same law, then up to eight rows forced to
    exactly 0.0 and exactly 1.0: an edge row and a det row of either target value for each, where the graph has one."""
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.randn(og.N, 1, generator=gen) * 8.0).clamp(-40, 40)
    scores = torch.sigmoid((torch.randn(og.N, 1, generator=gen) * 8.0).clamp(-40, 40))
    t = orc.create_targets(torch.from_numpy(labels).long(), og).numpy()
    for rows in (og.edge_row, og.det_row):
        for tv in (0, 1):
            cand = rows[t[rows] == tv]
            if cand.size > 0:
                scores[int(cand[0]), 0] = 0.0
            if cand.size > 1:
                scores[int(cand[-1]), 0] = 1.0
    return logits, scores


def _focal_arg(s64, s32, t):
    """float64, differentiable in s64: the reference's float32 q = fl32(fl32(t ? s : 1 - s) + fl32(1e-10)) minus 1e-10, so that
    orc.focal_loss(arg, ones) takes log(q) and d arg / d s = +-1."""
    q32 = torch.where(t, s32, 1.0 - s32) + 1e-10
    assert q32.dtype == torch.float32
    sign = torch.where(t, 1.0, -1.0).double()
    return sign * (s64 - s64.detach()) + (q32.double() - 1e-10)


def _fp64_reference(og, logits, scores, labels):
    """dict: targets uint8 [N]; loss_c, focal_e, focal_d (float); d_logits (of GC loss_c), d_scores_e / d_scores_d (of GF x the
    edge / det mean), float64 [N].  focal_* are NaN over an empty selection (models/loss.py:71-74)."""
    t = orc.create_targets(torch.from_numpy(np.asarray(labels)).long(), og)
    lo = logits.reshape(-1).double().requires_grad_(True)
    loss_c = orc.ce_loss(lo, t, og)
    d_logits = torch.zeros_like(lo)
    if loss_c.requires_grad:
        (GC * loss_c).backward()
        d_logits = lo.grad
    out = dict(targets=t.to(torch.uint8), loss_c=float(loss_c.detach()), d_logits=d_logits.detach())
    s32 = scores.reshape(-1)
    for key, rows in (('e', og.edge_row), ('d', og.det_row)):
        s64 = s32.double().requires_grad_(True)
        r = torch.from_numpy(rows)
        loss = orc.focal_loss(_focal_arg(s64, s32, t != 0)[r], torch.ones(r.numel(), dtype=torch.int64))
        if r.numel():
            (GF * loss).backward()
        out['focal_' + key] = float(loss.detach())
        out['d_scores_' + key] = s64.grad.detach() if s64.grad is not None else torch.zeros_like(s64)
    return out


def _close(got, ref):
    return abs(got - ref) <= 1e-5 * max(1.0, abs(ref))


def _check_against(ref, tp, loss_c, loss_f, d_logits, d_scores, targets, what):
    """Hold one (loss_c, loss_f, gradients, targets) of the HIP path to the float64 reference `ref` in mode tp."""
    assert torch.equal(targets.cpu().reshape(-1), ref['targets']), what
    ref_f = ref['focal_d'] + ref['focal_e'] if tp else ref['focal_e']
    assert _close(float(loss_c), ref['loss_c']), (what, float(loss_c), ref['loss_c'])
    assert _close(float(loss_f), ref_f), (what, float(loss_f), ref_f)
    dl, ds = d_logits.cpu().reshape(-1).double(), d_scores.cpu().reshape(-1).double()
    assert torch.allclose(dl, ref['d_logits'], atol=1e-6, rtol=1e-4), (what, float((dl - ref['d_logits']).abs().max()))
    rs = ref['d_scores_e'] + ref['d_scores_d'] if tp else ref['d_scores_e']
    bound = 1e-4 * rs.abs() + 1e-6 * float(rs.abs().max())
    assert bool(((ds - rs).abs() <= bound).all()), (what, float(((ds - rs).abs() - bound).max()))
    if not tp:
        det = ~ref['is_edge']
        assert not ds[det].any(), what                          # (train.py:81: no det term -- exactly zero, not small)


_ref_cache = {}


def _case(name):
    """(graph arrays, labels, logits, scores, float64 reference) of a case, computed once for both modes."""
    if name not in _ref_cache:
        build, lab, fused = _CASES[name]
        arrays = build()
        og = _oracle_graph(*arrays)
        seed = sorted(_CASES).index(name)
        if lab is None:
            labels = (np.random.RandomState(100 + seed).rand(og.N) < 0.3).astype(np.uint8)
        elif lab == 'tracks':
            labels = _three_frames()[1]
        else:
            labels = np.full(og.N, 1 if lab == 'ones' else 0, np.uint8)
        logits, scores = _inputs(og, labels, 200 + seed)
        ref = _fp64_reference(og, logits, scores, labels)
        ref['is_edge'] = torch.from_numpy(og.is_edge.copy())
        _ref_cache[name] = (arrays, labels, logits, scores, ref)
    return _ref_cache[name]


@pytest.mark.parametrize('tp', [True, False])
@pytest.mark.parametrize('name', list(_CASES))
def test_train_losses_against_float64(name, tp):
    from trackmpnn_amd import _lib, graph_from_edges
    from trackmpnn_amd.loss import train_losses
    (N, is_edge, src, dst), labels, logits, scores, ref = _case(name)
    g = graph_from_edges(N, torch.from_numpy(is_edge), torch.from_numpy(src), torch.from_numpy(dst), device=DEV)
    assert bool(_lib.load().tmpnn_train_losses_supported(g.E, g.Dn)) == _CASES[name][2], (g.E, g.Dn)
    lg = logits.to(DEV).requires_grad_(True)
    sc = scores.to(DEV).requires_grad_(True)
    loss_c, loss_f, targets = train_losses(sc, lg, torch.from_numpy(labels).to(DEV), g, tp, return_targets=True)
    (GC * loss_c + GF * loss_f).backward()
    _check_against(ref, tp, loss_c.detach(), loss_f.detach(), lg.grad, sc.grad, targets, (name, tp))
    # without the targets handed back (the call the loops make): the same bits
    lg2, sc2 = logits.to(DEV).requires_grad_(True), scores.to(DEV).requires_grad_(True)
    c2, f2 = train_losses(sc2, lg2, torch.from_numpy(labels).to(DEV), g, tp)
    (GC * c2 + GF * f2).backward()
    assert torch.equal(c2.detach(), loss_c.detach()) and torch.equal(f2.detach(), loss_f.detach())
    assert torch.equal(lg2.grad, lg.grad) and torch.equal(sc2.grad, sc.grad)
    # the cases' own promises
    if name == 'three_frames':
        t = ref['targets'].numpy()
        _, _, e02, e02_track = _three_frames()
        assert sorted(e02_track[e02_track >= 0]) == [0, 1, 2] and labels[e02[e02_track >= 0]].all()
        assert not t[e02[(e02_track == 0) | (e02_track == 2)]].any()            # positive, and neither end chooses it
        assert t[e02[e02_track == 1]].all()                                    # chosen by its dst det alone
        assert t[is_edge].sum() == labels[is_edge].sum() - 2
    if name.endswith('labels_zero'):
        assert float(loss_c.detach()) == 0.0 and not lg.grad.any() and not ref['targets'].any()
    if name.endswith('labels_one'):
        assert ref['targets'][~ref['is_edge']].all() and float(loss_c.detach()) > 0.0
    if name == 'sparse_700_700':
        assert g.Dn > 1024 and g.E == 1500


@pytest.mark.parametrize('tp', [True, False])
def test_train_losses_without_edges(tp):
    """E = 0, Dn = 5, forward only: loss_c is 0 and loss_f NaN -- the mean over an empty edge selection (models/loss.py:71-74),
    with or without the det term."""
    from trackmpnn_amd import _lib, graph_from_edges
    from trackmpnn_amd.loss import train_losses
    g = graph_from_edges(5, torch.zeros(5, dtype=torch.bool), torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long),
                         device=DEV)
    assert (g.E, g.Dn) == (0, 5) and _lib.load().tmpnn_train_losses_supported(0, 5)
    gen = torch.Generator().manual_seed(9)
    logits, scores = torch.randn(5, 1, generator=gen).to(DEV), torch.rand(5, 1, generator=gen).to(DEV)
    labels = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=DEV)
    loss_c, loss_f, targets = train_losses(scores, logits, labels, g, tp, return_targets=True)
    assert float(loss_c) == 0.0 and torch.isnan(loss_f)
    assert torch.equal(targets, labels)


# ---- the windowed form --------------------------------------------------------------------------------------------------------
def _window_chunks():
    """Hand-written chunks (y = [timestep, track id], -1 = false positive).  Call 0 (timesteps 0 and 1): A has 33 x 65 = 2145 edge
    rows = 17 chunks of 128, one past the 16 chunks a pass of the windowed sum folds; B has 8 x 16 = 128, exactly one chunk; C is
    small.  Call 1 (timestep 2): A and B grow (a partial 18th and a partial second chunk), C is finished: a window with no rows."""
    A = np.array([[0, i if i % 5 else -1] for i in range(33)] + [[1, j if j % 7 else -1] for j in range(65)] + [[2, 3]], np.int64)
    B = np.array([[0, i if i % 3 else -1] for i in range(8)] + [[1, j] for j in range(16)] + [[2, 1], [2, -1]], np.int64)
    C = np.array([[0, 0], [0, 1], [1, 1], [1, -1]], np.int64)
    return [A, B, C]


_win_cache = {}


def _window_case(batch, c):
    """Inputs of call c and the float64 reference of every live window on its own subgraph (computed once for both modes)."""
    from tests.test_train_batch_gpu import _subgraph
    if c not in _win_cache:
        plan, w = batch.plans[c], batch.windows[c]
        gen = torch.Generator().manual_seed(40 + c)
        N = plan.graph.N
        logits = (torch.randn(N, 1, generator=gen) * 8.0).clamp(-40, 40)
        scores = torch.sigmoid((torch.randn(N, 1, generator=gen) * 8.0).clamp(-40, 40))
        scores[::97] = 0.0
        scores[5::89] = 1.0
        labels = batch.call_labels(c).cpu()
        refs = {}
        for b in range(batch.B):
            if c >= batch.ncalls_b[b]:
                continue
            rows, sub = _subgraph(plan, w, b)
            rows = rows.cpu()
            og = orc.OracleGraph(sub.N, sub.is_edge.cpu().numpy().astype(bool), sub.src.cpu().numpy().astype(np.int64),
                                 sub.dst.cpu().numpy().astype(np.int64), sub.edge_row.cpu().numpy().astype(np.int64),
                                 sub.det_row.cpu().numpy().astype(np.int64))
            ref = _fp64_reference(og, logits[rows], scores[rows], labels[rows].numpy())
            ref['is_edge'] = torch.from_numpy(og.is_edge.copy())
            refs[b] = (rows, og.E, ref)
        _win_cache[c] = (logits, scores, refs)
    return _win_cache[c]


@pytest.mark.parametrize('tp', [True, False])
def test_windowed_losses_against_float64(tp):
    from tests.test_train_batch_gpu import _windowed
    from trackmpnn_amd import build_train_batch, train_losses_windows
    batch = build_train_batch(_window_chunks(), DEV)
    assert batch.B == 3 and list(batch.ncalls_b) == [2, 2, 1]
    gc, gf = torch.full((3,), GC, device=DEV), torch.full((3,), GF, device=DEV)
    sizes = []
    for c in range(2):
        logits, scores, refs = _window_case(batch, c)
        lg, sc = logits.to(DEV), scores.to(DEV)
        lc, lf, dl, ds = _windowed(batch, c, lg, sc, tp, gc, gf)
        _, _, targets = train_losses_windows(sc, lg, batch.call_labels(c), batch.plans[c], batch.windows[c], tp,
                                             return_targets=True)
        covered = torch.zeros(batch.plans[c].graph.N, dtype=torch.bool)
        for b in range(batch.B):
            if b not in refs:
                assert float(lc[b]) == 0.0 and float(lf[b]) == 0.0, (c, b)         # no rows at this call: 0 and 0
                continue
            rows, E, ref = refs[b]
            covered[rows] = True
            sizes.append((c, b, E))
            r = rows.to(DEV)
            _check_against(ref, tp, lc[b], lf[b], dl.reshape(-1)[r], ds.reshape(-1)[r], targets[r], (c, b, tp))
        assert not dl.reshape(-1).cpu()[~covered].any() and not ds.reshape(-1).cpu()[~covered].any()
    assert sizes[:3] == [(0, 0, 33 * 65), (0, 1, 128), (0, 2, 4)] and [s[:2] for s in sizes[3:]] == [(1, 0), (1, 1)]
    assert sizes[3][2] > 17 * 128 and sizes[4][2] > 128
