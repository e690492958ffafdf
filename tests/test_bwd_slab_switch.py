"""The weight gradients of the one-pass edge backward (tmpnn_gru_bwd_fused) and of the zero-state backward
(tmpnn_gru_bwd_fused_zero_state) on both sides of the slab reduction's switch at 64 slabs: each is the host's ordered sum
(tests/test_reduce_slabs_gpu.py) of the very per-block partials the kernel left in its workspace, bit for bit, and two runs
agree bit for bit.  Both kernels write one slab per block of min(256, ceil(R / 32)) blocks: 2048 rows give 64 slabs (added one
after the other), 2049 give 65 (32 at a time, then the groups); 32 * 257 rows reach the 256-block cap."""
import pytest
import torch

from tests.test_reduce_slabs_gpu import host_ordered_sum

DEV = 'cuda:0'
H = 64
pytestmark = pytest.mark.gpu

INIT = (0.5, 0.25, 1.0, 2.0)                # what dW_ih, dW_hh, db_ih, db_hh hold before the call: the sums are added to them


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _case(R, seed, zero_state):
    """A cell over R scattered rows (the layout of tests/test_bwd_zero_state.py); for the zero-state kernel every row has h = 0
    and ghn = b_hn in the fourth gate plane."""
    gen = torch.Generator().manual_seed(seed)
    N = 2 * R + 7
    perm = torch.randperm(N, generator=gen)
    rows = perm[:R].sort().values
    others = perm[R:]
    src = others[torch.randint(0, N - R, (R,), generator=gen)]
    dst = others[torch.randint(0, N - R, (R,), generator=gen)]
    r32 = lambda *s: torch.randn(*s, generator=gen)         # noqa: E731
    h = r32(N, H)
    if zero_state:
        h[rows] = 0.0
    b_hh = r32(3 * H)
    gates = torch.cat([torch.sigmoid(r32(2, N, H)), torch.tanh(r32(1, N, H)), r32(1, N, H)], 0)
    if zero_state:
        gates[3, rows] = b_hh[2 * H:]
    c = dict(rows=rows.to(torch.int32), src=src.to(torch.int32), dst=dst.to(torch.int32), h=h, gates=gates.contiguous(),
             dout=r32(N, H), dy=r32(N), w_head=r32(H), wih=0.3 * r32(3 * H, H), whh=0.3 * r32(3 * H, H), b_hh=b_hh,
             dmsg0=r32(N, H))
    return {k: v.to(DEV) for k, v in c.items()}, N


def _run(c, N, R, zero_state):
    """[dW_ih, dW_hh, db_ih, db_hh] and the workspace (the slabs) after one call, upstream gradient from d_hout and dy"""
    from trackmpnn_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.zeros(lib.tmpnn_gru_bwd_fused_ws(R, H, H) // 4 + 1, device=DEV)
    dmsg = c['dmsg0'].clone()
    dh = torch.full((N, H), 5.0, device=DEV)
    gW = [torch.full(s, v, device=DEV) for s, v in zip(((3 * H, H), (3 * H, H), (3 * H,), (3 * H,)), INIT)]
    rows, src, dst = c['rows'], c['src'], c['dst']
    if zero_state:
        _lib.call('tmpnn_gru_bwd_fused_zero_state', rows.data_ptr(), R, src.data_ptr(), dst.data_ptr(), H, c['h'].data_ptr(), H,
                  H, c['wih'].data_ptr(), c['b_hh'].data_ptr() + 4 * 2 * H, c['gates'].data_ptr(), N * H, c['dout'].data_ptr(),
                  H, c['dy'].data_ptr(), c['w_head'].data_ptr(), dmsg.data_ptr(), H, gW[0].data_ptr(), gW[2].data_ptr(),
                  gW[3].data_ptr(), ws.data_ptr(), ws.numel() * 4, st)
    else:
        _lib.call('tmpnn_gru_bwd_fused', rows.data_ptr(), R, 1, src.data_ptr(), dst.data_ptr(), None, H, 1, H,
                  c['h'].data_ptr(), H, H, c['wih'].data_ptr(), c['whh'].data_ptr(), c['gates'].data_ptr(), N * H,
                  c['dout'].data_ptr(), H, c['dy'].data_ptr(), c['w_head'].data_ptr(), dmsg.data_ptr(), H, dh.data_ptr(), H,
                  src.data_ptr(), dst.data_ptr(), dmsg.data_ptr(), H, gW[0].data_ptr(), gW[1].data_ptr(), gW[2].data_ptr(),
                  gW[3].data_ptr(), ws.data_ptr(), ws.numel() * 4, st)
    torch.cuda.synchronize()
    return [g.cpu() for g in gW], ws.cpu()


def _host_sums(ws, n_rs, zero_state):
    """the four gradients' sums from the slabs at the front of the workspace: n_rs x [3H][2H], then n_rs x [2][3H]"""
    nW, nB = 3 * H * 2 * H, 6 * H
    w = ws[:n_rs * nW].view(n_rs, 3 * H, 2 * H)
    b = host_ordered_sum(ws[n_rs * nW:n_rs * (nW + nB)].view(n_rs, nB))
    if not zero_state:
        s = host_ordered_sum(w)
        return [s[:, :H], s[:, H:], b[:3 * H], b[3 * H:]]
    # the zero-state slabs hold the two K-steps' partials of dW_ih in their column halves: the halves of a slab (up to 64
    # slabs) or of a group's sum (more) are added first, then summed in order
    if n_rs <= 64:
        s = host_ordered_sum(w[:, :, :H] + w[:, :, H:])
    else:
        groups = torch.stack([host_ordered_sum(w[k:k + 32]) for k in range(0, n_rs, 32)])
        s = torch.zeros(3 * H, H)
        for g in groups:
            s = s + (g[:, :H] + g[:, H:])
    return [s, None, b[:3 * H], b[3 * H:]]


@pytest.mark.parametrize('zero_state', [False, True])
@pytest.mark.parametrize('R', [2048, 2049, 32 * 257])
def test_weight_gradients_are_the_ordered_sum_of_the_slabs(R, zero_state):
    from trackmpnn_amd import _lib
    lib = _lib.load()
    if not (lib.tmpnn_gru_bwd_fused_available(H, H, 1) and lib.tmpnn_gru_bwd_fused_zero_state_available(H, H, 1)):
        pytest.fail('the one-pass backward kernels are not available for H = IN = 64, xmode 1')
    n_rs = min(256, (R + 31) // 32)
    assert (R, n_rs) in ((2048, 64), (2049, 65), (32 * 257, 256))
    c, N = _case(R, R, zero_state)
    g1, ws1 = _run(c, N, R, zero_state)
    g2, ws2 = _run(c, N, R, zero_state)
    assert torch.equal(ws1, ws2) and all(torch.equal(a, b) for a, b in zip(g1, g2))      # two runs: the same bits
    want = _host_sums(ws1, n_rs, zero_state)
    for name, got, s, init in zip(('dW_ih', 'dW_hh', 'db_ih', 'db_hh'), g1, want, INIT):
        if s is None:                                     # the zero-state kernel has no dW_hh: left as it was
            assert torch.equal(got, torch.full_like(got, init)), (R, zero_state, name)
            continue
        assert s.abs().max().item() > 0, (R, zero_state, name)
        assert torch.equal(got, torch.full_like(got, init) + s), (R, zero_state, name)
