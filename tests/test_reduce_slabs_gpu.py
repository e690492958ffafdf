"""tmpnn_reduce_slabs, the one-launch ordered sum behind every per-block partial of the library, against a host restatement
of its order: up to 64 slabs one after the other; more than 64 in groups of 32 consecutive slabs, then the group sums in
ascending order.  Whole slabs are added on the CPU in fp32, one at a time; elementwise fp32 adds are exact, so the comparison
is torch.equal."""
import pytest
import torch

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

NSLABS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 256, 257, 2048)
NS = (1, 130, 255, 256, 257, 24960)
PAD = 5                                     # stride = n + PAD: rows off 16-byte alignment, NaN between them


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def host_ordered_sum(slabs):
    """slabs [nslab, ...] fp32 on the CPU -> their sum in the library's order"""
    nslab = slabs.shape[0]
    s = torch.zeros_like(slabs[0])
    if nslab <= 64:
        for k in range(nslab):
            s = s + slabs[k]
        return s
    for k0 in range(0, nslab, 32):
        a = torch.zeros_like(slabs[0])
        for k in range(k0, min(nslab, k0 + 32)):
            a = a + slabs[k]
        s = s + a
    return s


def _reduce(buf, stride, nslab, dst, n, accumulate):
    from trackmpnn_amd import _lib
    _lib.call('tmpnn_reduce_slabs', buf.data_ptr(), stride, nslab, dst.data_ptr(), n, accumulate,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize('nslab', NSLABS)
def test_reduce_slabs_equals_the_host_order(nslab):
    gen = torch.Generator().manual_seed(nslab)
    for n in NS:
        stride = n + PAD
        buf = torch.full((nslab, stride), float('nan'))
        # magnitudes spread over a few binades, so that a different order of the adds gives different bits
        buf[:, :n] = torch.randn(nslab, n, generator=gen) * torch.exp2(torch.randint(-3, 4, (nslab, 1), generator=gen).float())
        want = host_ordered_sum(buf[:, :n])
        assert torch.isfinite(want).all()
        d_buf = buf.to(DEV)
        init = torch.randn(n + 2, generator=gen)
        for accumulate in (0, 1):
            outs = []
            for _ in range(2):
                dst = init.to(DEV)
                _reduce(d_buf, stride, nslab, dst, n, accumulate)
                outs.append(dst.cpu())
            tag = (nslab, n, accumulate)
            assert torch.equal(outs[0], outs[1]), tag                    # two runs: the same bits
            assert torch.equal(outs[0][n:], init[n:]), tag               # nothing written behind n
            assert torch.equal(outs[0][:n], init[:n] + want if accumulate else want), tag


def test_reduce_slabs_rejects_bad_arguments():
    from trackmpnn_amd import _lib
    lib = _lib.load()
    x = torch.zeros(8, device=DEV)
    assert lib.tmpnn_reduce_slabs(x.data_ptr(), 2, 2, x.data_ptr(), 4, 0, None) == -1       # stride < n
    assert lib.tmpnn_reduce_slabs(x.data_ptr(), 4, 0, x.data_ptr(), 4, 0, None) == -1       # no slabs
    assert lib.tmpnn_reduce_slabs(None, 4, 2, x.data_ptr(), 4, 0, None) == -1
