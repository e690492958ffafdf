"""tmpnn_heads_bwd at the row counts where its partition and the reduction of its per-block partials change: one block, 64 / 65
rows (one block / two), 4097 rows (65 partials: the two-level order of the reduction), 2048 * 64 + 1 rows (the first count at
which a block takes more than 64 rows).  dy and the four gradients against a float64 host sum within the bound the stage checks
use for this entry point (tests/gpu_stage_checks.py: 2e-4, gradients relative to max(1, largest weight gradient)); two runs
agree bit for bit."""
import pytest
import torch

DEV = 'cuda:0'
C = 64
TOL = 2e-4
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _run(N, c, with_scores):
    from trackmpnn_amd import _lib
    lib = _lib.load()
    wsb = lib.tmpnn_heads_bwd_ws(N, C)
    ws = torch.empty(wsb // 4 + 1, device=DEV)
    g = [torch.full((C,), 0.5, device=DEV), torch.full((1,), 0.25, device=DEV), torch.full((C,), -1.0, device=DEV),
         torch.full((1,), 2.0, device=DEV)]                                      # dw_node, db_node, dw_edge, db_edge
    dyo = torch.zeros(N, device=DEV)
    dh = c['pre'].clone()
    _lib.call('tmpnn_heads_bwd', c['h'].data_ptr(), C + 4, C, N, c['is_edge'].data_ptr(), c['wn'].data_ptr(), c['we'].data_ptr(),
              c['scores'].data_ptr() if with_scores else None, c['dl'].data_ptr(), c['ds'].data_ptr() if with_scores else None,
              dyo.data_ptr(), dh.data_ptr(), C, 1, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(),
              ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [t.cpu() for t in g], dyo.cpu(), dh.cpu()


@pytest.mark.parametrize('with_scores', [True, False])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 4097, 2048 * 64 + 1])
def test_heads_bwd_matches_a_float64_sum(N, with_scores):
    gen = torch.Generator().manual_seed(N)
    h = torch.randn(N, C + 4, generator=gen)
    ie = torch.rand(N, generator=gen) < 0.6          # both row types (N = 1 has one row: a det row)
    if N > 1:
        ie[0], ie[-1] = True, False
    else:
        ie[0] = False
    wn, we = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    scores = torch.sigmoid(torch.randn(N, generator=gen))
    dl, ds = torch.randn(N, generator=gen), torch.randn(N, generator=gen)
    pre = torch.randn(N, C, generator=gen)
    c = {k: v.to(DEV).contiguous() for k, v in dict(h=h, is_edge=ie.to(torch.uint8), wn=wn, we=we, scores=scores, dl=dl, ds=ds,
                                                    pre=pre).items()}
    # float64 on the host
    dy = dl.double() + (ds.double() * scores.double() * (1 - scores.double()) if with_scores else 0.0)
    x = h[:, :C].double()
    want = [(dy[~ie, None] * x[~ie]).sum(0), dy[~ie].sum().view(1), (dy[ie, None] * x[ie]).sum(0), dy[ie].sum().view(1)]
    want_dh = pre.double() + dy[:, None] * torch.where(ie[:, None], we.double(), wn.double())
    g1, dy1, dh1 = _run(N, c, with_scores)
    g2, dy2, dh2 = _run(N, c, with_scores)
    tag = (N, with_scores)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)) and torch.equal(dy1, dy2) and torch.equal(dh1, dh2), tag
    assert (dy1.double() - dy).abs().max().item() <= TOL, tag
    assert (dh1.double() - want_dh).abs().max().item() <= TOL, tag
    sc = max(1.0, want[0].abs().max().item(), want[2].abs().max().item())
    for name, got, w, init in zip(('dw_node', 'db_node', 'dw_edge', 'db_edge'), g1, want, (0.5, 0.25, -1.0, 2.0)):
        assert (got.double() - init - w).abs().max().item() <= TOL * sc, (tag, name)
