"""Training the embedding CNN's whole decoder on the MI355X (-m gpu): EspTrainNet(scope='decoder') against EspEmbedNet bit for bit,
its 36 parameter gradients and four tap gradients against the reference module's (tests/golden/espnet_grad) and against
espnet_decoder_grads_host, accumulation, determinism, the tail's bits inside the decoder, the optimizer step with the refold on the
device, and a step of train_epoch(vis=...).

The rule is the one of tests/test_espnet_train_gpu.py, unchanged: per tensor, max |device - g64| <= 8 max(e_ref, 2^-23 max |g64|).
A device run of a (case, form) is made once per process and shared by the tests that read it."""
import functools

import numpy as np
import pytest
import torch

from tests.espnet_cases import CASES, case_images, load_case
from tests.espnet_grad_cases import GRAD_CASES, TAPS, case_d_maps, load_grad_case
from tests.test_espnet_train_gpu import _bits, _tracker_and_head, _vis_set, hold_to_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _all40(C):
    from trackmpnn_amd.espnet import decoder_param_names
    return decoder_param_names(C) + TAPS


def run_grads(sd, images, d_maps, scope='decoder', tap_grads=True, passes=1):
    """{name: gradient (host, float32)} of a fresh EspTrainNet after `passes` backward passes without zero_grad."""
    from trackmpnn_amd import EspTrainNet
    net = EspTrainNet.from_state_dict(sd, DEV, scope=scope)
    x, d = torch.from_numpy(images).to(DEV), torch.from_numpy(d_maps).to(DEV)
    net.tap_grads = None
    for _ in range(passes):
        net(x, tap_grads=tap_grads).backward(d)
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    if tap_grads:
        got.update({k: v.detach().cpu() for k, v in net.tap_grads.items() if v is not None})
    else:
        assert net.tap_grads is None
    return got


@functools.lru_cache(maxsize=None)
def case_grads(name, form, scope='decoder', tap_grads=True, passes=1):
    _, sd = load_case(name)
    return run_grads(sd, case_images(name), case_d_maps(name, form), scope, tap_grads, passes)


# ---- 1. the forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['c1_16x16', 'c3_48x80', 'c4_batch3'])
def test_forward_has_the_bits_of_the_eval_net(name):
    from trackmpnn_amd import EspEmbedNet, EspTrainNet
    fx, sd = load_case(name)
    x = torch.from_numpy(fx['images']).to(DEV)
    want = EspEmbedNet.from_state_dict(sd, DEV)(x)
    net = EspTrainNet.from_state_dict(sd, DEV, scope='decoder')
    assert net.scope == 'decoder' and EspTrainNet.from_state_dict(sd, DEV).scope == 'tail'
    maps = net(x)
    assert maps.requires_grad and maps.grad_fn is not None
    assert torch.equal(_bits(maps.detach()), _bits(want))
    with torch.no_grad():
        quiet = net(x)
    assert not quiet.requires_grad and torch.equal(_bits(quiet), _bits(want))
    assert torch.equal(_bits(net(x).detach()), _bits(want))


# ---- 2. gradients against the reference module ------------------------------------------------------------------------------
@pytest.mark.parametrize('name,form', GRAD_CASES)
def test_all_forty_gradients_within_eight_times_the_references_own_float32_error(name, form):
    g64, e_ref, _, _ = load_grad_case(name, form)
    C = CASES[name][1]
    got = case_grads(name, form)
    assert sorted(got) == sorted(_all40(C)) and len(got) == 40
    T, _, H, W, _ = CASES[name]
    assert tuple(got['out_l3'].shape) == (T, 128, H // 8, W // 8) and tuple(got['out_l4'].shape) == (T, 256, H // 16, W // 16)
    hold_to_rule(f'decoder {name} {form}', got, g64, e_ref, _all40(C))


# ---- 3. zero and negative slopes --------------------------------------------------------------------------------------------
def test_zero_and_negative_slopes():
    """Every one of the 7 decoder PReLUs gets a zero and a negative slope: the backward must take the sign from the value in front of
    the activation (stored, or for br_after_cat recomputed), which no output tells."""
    from trackmpnn_amd.espnet import espnet_decoder_grads_host
    name = 'c4_batch3'
    _, sd0 = load_case(name)
    sd = type(sd0)((k, v.clone()) for k, v in sd0.items())
    acts = [k for k in sd if not k.startswith('net.') and k.endswith('act.weight')]
    assert len(acts) == 7
    for k in acts:
        sd[k][0], sd[k][1] = 0.0, -0.25
    images, d = case_images(name), case_d_maps(name, 'dense')
    x, dd = torch.from_numpy(images), torch.from_numpy(d)
    h64 = {k: v.numpy() for k, v in espnet_decoder_grads_host(sd, x, dd, torch.float64).items()}
    h32 = espnet_decoder_grads_host(sd, x, dd, torch.float32)
    e_ref = {k: float(np.abs(h32[k].numpy().astype(np.float64) - h64[k]).max()) for k in h64}
    hold_to_rule('decoder slopes', run_grads(sd, images, d), h64, e_ref, _all40(CASES[name][1]))


# ---- 4. accumulation and determinism ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,form', [('c3_48x80', 'dense'), ('c4_batch3', 'sparse')])
def test_accumulation_and_determinism(name, form):
    _, sd = load_case(name)
    images, d = case_images(name), case_d_maps(name, form)
    once, again = case_grads(name, form), run_grads(sd, images, d)
    assert sorted(once) == sorted(_all40(CASES[name][1]))
    for k in once:
        assert torch.equal(_bits(once[k]), _bits(again[k])), k             # two fresh runs: equal bits
        assert float(once[k].abs().max()) > 0.0, k
    twice = run_grads(sd, images, d, passes=2)
    bare = case_grads(name, form, 'decoder', False)
    assert len(bare) == 36
    for k in bare:
        assert torch.equal(_bits(twice[k]), _bits(2.0 * once[k])), k       # no zero_grad in between: exactly twice
        assert torch.equal(_bits(bare[k]), _bits(once[k])), k              # the tap-only work changes no parameter gradient
    for k in TAPS:
        assert k not in bare and torch.equal(_bits(twice[k]), _bits(once[k])), k   # tap gradients are overwritten, not added


# ---- 5. the tail inside the decoder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['dense', 'sparse'])
def test_the_tail_keeps_its_bits_inside_the_decoder(form):
    from trackmpnn_amd.espnet import trained_param_names
    name = 'c3_48x80'
    dec, tail = case_grads(name, form), case_grads(name, form, 'tail')
    names = trained_param_names(CASES[name][1]) + ('out_l1', 'out_l2')
    assert sorted(tail) == sorted(names)
    for k in names:
        assert torch.equal(_bits(dec[k]), _bits(tail[k])), k
    for taps in (True, False):                                              # and the tail scope still answers as it did
        t = case_grads(name, form, 'tail', taps)
        assert len(t) == (11 if taps else 9)


# ---- 6. the optimizer step and the refold -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['c3_48x80', 'c5_c128'])
def test_adam_step_and_refold(name):
    from trackmpnn_amd import BucketAdam, EspEmbedNet, EspTrainNet
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.espnet import check_state_dict, decoder_param_names
    from tests.test_optim_gpu import _err
    _, sd = load_case(name)
    C = CASES[name][1]
    names = decoder_param_names(C)
    x, d = torch.from_numpy(case_images(name)).to(DEV), torch.from_numpy(case_d_maps(name, 'dense')).to(DEV)
    lr, wd = 5e-4, 5e-4                                                     # the reference's embedding optimizer
    net = EspTrainNet.from_state_dict(sd, DEV, scope='decoder')
    assert [k for k, _ in net.named_parameters()] == list(names)
    params = list(net.parameters())
    assert len(params) == 36 and all(isinstance(p, torch.nn.Parameter) for p in params)
    at = params[0].data_ptr()
    for p in params:                                                        # views of ONE flat float32 buffer, no padding
        assert p.dtype == torch.float32 and p.is_contiguous() and p.data_ptr() == at
        at += 4 * p.numel()
    opt = torch.optim.Adam(net.parameters(), lr, weight_decay=wd)
    opt.zero_grad()
    net(x).backward(d)
    grads = [p.grad.detach().clone() for p in net.parameters()]
    opt.step()
    after = net.state_dict()
    assert check_state_dict(after) == C and list(after) == list(sd)
    for k in sd:
        same = torch.equal(after[k].cpu(), sd[k])
        assert same != (k in names), k                                      # all 36 moved, nothing else did
    # the next forward runs on the refolded arena: the bits of an eval net packed on the host from the same tensors
    want = EspEmbedNet.from_state_dict(after, DEV)(x)
    assert torch.equal(_bits(net(x).detach()), _bits(want))
    assert torch.equal(_bits(net.snapshot()(x)), _bits(want))
    assert torch.equal(net._arena.cpu(), EspEmbedNet.from_state_dict(after, DEV)._arena.cpu())     # every segment, not just the output
    # BucketAdam over GradBucket(net) from the same gradients, held to torch's own float32 error as tests/test_optim_gpu.py does
    net2 = EspTrainNet.from_state_dict(sd, DEV, scope='decoder')
    bucket = GradBucket(net2)
    opt2 = BucketAdam(net2, bucket, lr=lr, weight_decay=wd)
    opt2.zero_grad()
    net2(x).backward(d)
    assert bucket.check_alias()
    for p, g in zip(net2.parameters(), grads):
        assert torch.equal(_bits(p.grad), _bits(g))                        # in place into the bucket: the same bits
    opt2.step()
    p0 = torch.cat([sd[k].reshape(-1) for k in names])
    p64 = torch.nn.Parameter(p0.double())
    p64.grad = torch.cat([g.reshape(-1) for g in grads]).double().cpu()
    torch.optim.Adam([p64], lr, weight_decay=wd).step()
    flat = lambda n: torch.cat([p.detach().reshape(-1) for p in n.parameters()]).double().cpu()
    e_torch, e_mine = _err(flat(net), p64.detach(), lr), _err(flat(net2), p64.detach(), lr)
    print(f'[espnet_decoder_train] {name}: err(BucketAdam) = {e_mine:.3e}, err(torch.optim.Adam fp32) = {e_torch:.3e}')
    assert e_torch > 0 and e_mine <= 4 * e_torch
    want2 = EspEmbedNet.from_state_dict(net2.state_dict(), DEV)(x)
    assert torch.equal(_bits(net2(x).detach()), _bits(want2))              # BucketAdam moved the version counter: refolded


# ---- 7. through the library -------------------------------------------------------------------------------------------------
def test_a_training_step_of_the_default_mode_moves_the_whole_decoder():
    from trackmpnn_amd import EspTrainNet, VisTraining
    from trackmpnn_amd.loops import train_epoch
    from trackmpnn_amd.vishead import VIS_COLS
    sampler, fs, hw, chunks = _vis_set()
    _, sd = load_case('c5_c128')
    assert CASES['c5_c128'][1] == VIS_COLS
    net = EspTrainNet.from_state_dict(sd, DEV, scope='decoder')
    before = [p.detach().clone() for p in net.parameters()]
    assert len(before) == 36
    net_opt = torch.optim.Adam(net.parameters(), 5e-4, weight_decay=5e-4)
    model, opt, head = _tracker_and_head(hw)
    few = type(sampler)(sampler.store, chunks[:6], seed=23)
    steps = train_epoch(model, few, opt, 2, 0, vis=VisTraining(head, fs, net, net_opt))
    assert steps >= 1
    for (k, p), a in zip(net.named_parameters(), before):
        assert bool(torch.isfinite(p).all()) and not torch.equal(a, p.detach()), k
