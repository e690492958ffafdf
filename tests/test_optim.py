"""BucketAdam without a GPU: the segment table and the work list of the one-launch Adam step, torch.optim.Adam's state_dict
format, the constructor's refusals, argument validation of tmpnn_adam_step / tmpnn_grad_flow (no launch), and
allreduce_grads(average=False) under gloo."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from trackmpnn_amd import _lib


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _models():
    from trackmpnn_amd import TrackMPNN
    torch.manual_seed(3)
    return [TrackMPNN('2d-temp-vis', 3, 64, 2, 'concat'), TrackMPNN('2d', 3, 48, 0, 'diff')]


# ---- 1. segment table and work list ----------------------------------------------------------------------------------------
def test_segment_table_and_work_list_cover_the_bucket(lib):
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.optim import chunk_elems, segment_table, work_list
    chunk = chunk_elems()
    assert chunk == lib.tmpnn_optim_chunk() and chunk > 0 and chunk % 4 == 0
    for model in _models():
        bucket = GradBucket(model)
        segs = segment_table(bucket)
        assert segs.dtype == np.int64 and segs.shape == (len(bucket.params), 3)
        o = 0
        for row, p in zip(segs, bucket.params):
            assert (int(row[0]), int(row[1]), int(row[2])) == (p.data_ptr(), o, p.numel())
            assert p.grad.data_ptr() == bucket.flat.data_ptr() + 4 * o
            o += p.numel()
        assert o == bucket.flat.numel()
        assert any(int(r[1]) % 4 for r in segs), 'no segment starts off a 16-byte boundary: the scalar path is not exercised'
        work = work_list(segs[:, 2])
        assert work.dtype == np.int32 and work.shape[1] == 2 and work.flags['C_CONTIGUOUS']
        hits = np.zeros(bucket.flat.numel(), np.int64)
        last = (-1, -1)
        for s, off in work:
            assert 0 <= s < len(segs) and off % chunk == 0 and 0 <= off < segs[s, 2]
            assert (s, off) > last                                  # segments in order, offsets ascending
            last = (s, off)
            n = min(chunk, segs[s, 2] - off)
            hits[segs[s, 1] + off:segs[s, 1] + off + n] += 1
        assert (hits == 1).all()
    # odd sizes, an empty segment, another chunk size
    w = work_list([5, 0, 9, 4], chunk=4)
    assert w.tolist() == [[0, 0], [0, 4], [2, 0], [2, 4], [2, 8], [3, 0]]
    with pytest.raises(ValueError):
        work_list([3, -1])


# ---- 2. state_dict format, refusals, argument checks -------------------------------------------------------------------------
def test_state_dict_speaks_torch_adam(lib):
    from trackmpnn_amd import BucketAdam
    from trackmpnn_amd.dist import GradBucket
    model = _models()[0]
    bucket = GradBucket(model)
    opt = BucketAdam(model, bucket, lr=1e-4, weight_decay=5e-4)
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1
    assert [id(p) for p in opt.param_groups[0]['params']] == [id(p) for p in bucket.params]
    ref = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-4)
    gen = torch.Generator().manual_seed(4)
    bucket.flat.copy_(torch.randn(bucket.flat.numel(), generator=gen))
    ref.step()
    ref.step()
    a, b = opt.state_dict(), ref.state_dict()
    assert sorted(a) == sorted(b) and len(a['param_groups']) == 1
    assert sorted(a['param_groups'][0]) == sorted(b['param_groups'][0])
    for k, v in b['param_groups'][0].items():
        assert a['param_groups'][0][k] == v, k
    assert sorted(a['state']) == sorted(b['state']) == list(range(len(bucket.params)))
    for i, p in enumerate(bucket.params):
        assert sorted(a['state'][i]) == sorted(b['state'][i]) == ['exp_avg', 'exp_avg_sq', 'step']
        for k in ('exp_avg', 'exp_avg_sq', 'step'):
            assert a['state'][i][k].shape == b['state'][i][k].shape and a['state'][i][k].dtype == b['state'][i][k].dtype, (i, k)
        assert a['state'][i]['exp_avg'].shape == p.shape
    # torch's state into the bucket optimizer: copied INTO the flat buffers, views of them in opt.state
    ptrs = (opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(), opt.state[bucket.params[0]]['step'].data_ptr())
    b['param_groups'][0]['lr'] = 2e-5
    opt.load_state_dict(b)
    assert ptrs == (opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(), opt.state[bucket.params[0]]['step'].data_ptr())
    assert opt.param_groups[0]['lr'] == 2e-5
    o = 0
    for p in bucket.params:
        st = opt.state[p]
        assert float(st['step']) == 2.0
        assert torch.equal(st['exp_avg'], ref.state[p]['exp_avg']) and torch.equal(st['exp_avg_sq'], ref.state[p]['exp_avg_sq'])
        assert st['exp_avg'].data_ptr() == opt.exp_avg.data_ptr() + 4 * o          # a view: edits reach the kernel's buffer
        o += p.numel()
    opt.state[bucket.params[1]]['exp_avg'].zero_()
    n0 = bucket.params[0].numel()
    assert float(opt.exp_avg[n0:n0 + bucket.params[1].numel()].abs().sum()) == 0.0
    # and back: torch continues from the bucket optimizer's state
    ref2 = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-4)
    ref2.load_state_dict(opt.state_dict())
    assert float(ref2.state[bucket.params[0]]['step']) == 2.0
    assert torch.equal(ref2.state[bucket.params[2]]['exp_avg_sq'], ref.state[bucket.params[2]]['exp_avg_sq'])
    assert ref2.state[bucket.params[2]]['exp_avg'].data_ptr() != opt.state[bucket.params[2]]['exp_avg'].data_ptr()
    ref2.step()
    # a scheduler drives it like torch's
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=15, gamma=0.2)
    assert opt.param_groups[0]['initial_lr'] == 2e-5 and sched.get_last_lr() == [2e-5]
    # zero_grad keeps the aliasing, whatever the argument
    bucket.flat.fill_(1.0)
    opt.zero_grad()
    assert bucket.check_alias() and float(bucket.flat.abs().sum()) == 0.0
    bucket.flat.fill_(1.0)
    opt.zero_grad(set_to_none=True)
    assert bucket.check_alias() and float(bucket.flat.abs().sum()) == 0.0


def test_constructor_refusals(lib):
    from trackmpnn_amd import BucketAdam, TrackMPNN
    from trackmpnn_amd.dist import GradBucket
    model = _models()[0]
    bucket = GradBucket(model)
    params = list(model.parameters())
    with pytest.raises(ValueError, match='amsgrad'):
        BucketAdam(model, bucket, amsgrad=True)
    with pytest.raises(ValueError, match='maximize'):
        BucketAdam(model, bucket, maximize=True)
    with pytest.raises(ValueError, match='one parameter group'):
        BucketAdam([{'params': params[:3]}, {'params': params[3:]}], bucket)
    with pytest.raises(ValueError, match='bucket.params'):
        BucketAdam(params[:-1], bucket)
    with pytest.raises(ValueError, match='bucket.params'):
        BucketAdam(list(reversed(params)), bucket)
    with pytest.raises(ValueError, match='bucket.params'):
        BucketAdam(TrackMPNN('2d-temp-vis', 3, 64, 2, 'concat'), bucket)         # another model's parameters
    with pytest.raises(ValueError):
        BucketAdam(model, bucket, betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        BucketAdam(model, bucket, lr=-1.0)
    opt = BucketAdam([{'params': params, 'lr': 3e-4}], bucket)                   # one group, as a list of dicts
    assert opt.param_groups[0]['lr'] == 3e-4
    with pytest.raises(ValueError, match='one parameter group'):
        opt.add_param_group({'params': [torch.nn.Parameter(torch.zeros(2))]})
    other = torch.optim.Adam(params, amsgrad=True)
    with pytest.raises(ValueError, match='amsgrad'):
        opt.load_state_dict(other.state_dict())
    # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        opt.step()
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        opt.grad_flow()


def test_entry_points_check_their_arguments(lib):
    import ctypes as C
    fake = C.c_void_p(1 << 20)              # never dereferenced: every call below fails on the host
    err = lambda: lib.tmpnn_last_error()

    def adam(segs=fake, P=3, work=fake, nwork=5, grad=fake, m=fake, v=fake, n=100, st=fake, b1=0.9, b2=0.999, eps=1e-8, wd=0.0,
             scale=1.0, zero=0):
        return lib.tmpnn_adam_step(segs, P, work, nwork, grad, m, v, n, st, b1, b2, eps, wd, scale, zero, None)

    assert adam(segs=None) == -1 and b'adam_step' in err() and b'null' in err()
    assert adam(work=None) == -1 and b'null' in err()
    assert adam(P=0) == -1 and b'empty table' in err()
    assert adam(nwork=0) == -1 and b'empty table' in err()
    assert adam(P=-2) == -1
    assert adam(n=-5) == -1 and b'n_flat' in err()
    assert adam(grad=None) == -1 and adam(m=None) == -1 and adam(v=None) == -1 and b'null' in err()
    assert adam(st=None) == -1 and b'state is null' in err()
    assert adam(grad=C.c_void_p((1 << 20) + 4)) == -1 and b'aligned' in err()
    assert adam(b1=1.0) == -1 and b'betas' in err()
    assert adam(b2=-0.1) == -1 and b'betas' in err()
    assert adam(b2=1.5) == -1
    assert adam(eps=-1e-8) == -1 and adam(wd=-1.0) == -1
    assert adam(scale=float('nan')) == -1 and b'grad_scale' in err()
    flow = lib.tmpnn_grad_flow
    assert flow(None, 3, fake, 100, fake, None) == -1 and b'grad_flow' in err()
    assert flow(fake, 0, fake, 100, fake, None) == -1 and b'empty table' in err()
    assert flow(fake, 3, None, 100, fake, None) == -1 and b'null' in err()
    assert flow(fake, 3, fake, 100, None, None) == -1
    assert flow(fake, 3, fake, -1, fake, None) == -1 and b'n_flat' in err()
    assert _lib.ABI_VERSION >= 8 and lib.tmpnn_abi_version() == _lib.ABI_VERSION
    for n in ('tmpnn_optim_chunk', 'tmpnn_adam_step', 'tmpnn_grad_flow'):
        assert n in _lib._SIGNATURES and n in _lib.header_symbols()


# ---- 3. allreduce_grads(average=False) ---------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from trackmpnn_amd import TrackMPNN
    from trackmpnn_amd.dist import GradBucket, allreduce_grads
    torch.manual_seed(5)
    model = TrackMPNN('2d', 3, 32, 2, 'concat')
    bucket = GradBucket(model)
    n = bucket.flat.numel()
    local = [torch.randn(n, generator=torch.Generator().manual_seed(100 + r)) for r in range(world)]
    total = local[0].clone()
    for g in local[1:]:
        total += g                                               # gloo's sum over two ranks: one fp32 add per element
    bucket.flat.copy_(local[rank])
    allreduce_grads(model, bucket, world, average=False)
    ok = torch.equal(bucket.flat, total) and bucket.check_alias()
    # the default is the parent's behaviour: the sum, then flat.mul_(1 / world)
    bucket.flat.copy_(local[rank])
    allreduce_grads(model, bucket, world)
    ok = ok and torch.equal(bucket.flat, total.mul(1.0 / world))
    bucket.flat.copy_(local[rank])
    allreduce_grads(model, bucket, world, average=True)
    ok = ok and torch.equal(bucket.flat, total.mul(1.0 / world))
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_allreduce_can_leave_the_sum_world2():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res), res
