"""Training the embedding CNN's decoder on the MI355X (-m gpu): EspTrainNet against EspEmbedNet bit for bit, its gradients against
the reference module's (tests/golden/espnet_grad) and against espnet_decoder_grads_host, accumulation, determinism, the optimizer
step with the refold on the device, and a step of train_epoch(vis=...) with no torch CNN in it.

The rule for a gradient (fixed before the first device run): per tensor, max |device - g64| <= 8 max(e_ref, 2^-23 max |g64|), g64
the float64 gradient, e_ref the error of the same computation in float32 by torch (the reference's own float32 error; 8 is the
factor the project holds the forward to, profiles/espnet.md), the floor one float32 unit of the tensor's largest entry.  This
version trains the decoder behind merge_l3, so the rule is applied to its 9 tensors and to the taps out_l1 and out_l2; the fixtures
hold the other 27 + 2 gradients for the version that completes the decoder (the host definition is held to all 40 without a GPU)."""
import random

import numpy as np
import pytest
import torch

from tests.espnet_cases import CASES, case_images, load_case
from tests.espnet_grad_cases import GRAD_CASES, case_d_maps, load_grad_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 8.0
U = 2.0 ** -23


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _checked(C):
    from trackmpnn_amd.espnet import trained_param_names
    return trained_param_names(C) + ('out_l1', 'out_l2')


def device_grads(sd, images, d_maps, tap_grads=True, passes=1):
    """{name: gradient (host, float32)} of a fresh EspTrainNet after `passes` backward passes without zero_grad."""
    from trackmpnn_amd import EspTrainNet
    net = EspTrainNet.from_state_dict(sd, DEV)
    x, d = torch.from_numpy(images).to(DEV), torch.from_numpy(d_maps).to(DEV)
    for _ in range(passes):
        net(x, tap_grads=tap_grads).backward(d)
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    if tap_grads:
        got.update({k: v.detach().cpu() for k, v in net.tap_grads.items() if v is not None})
        assert net.tap_grads['out_l3'] is None and net.tap_grads['out_l4'] is None
    return got


def hold_to_rule(tag, got, g64, e_ref, names):
    lines, bad = [], []
    for k in names:
        ref = np.asarray(g64[k], np.float64)
        g = got[k].numpy().astype(np.float64)
        assert g.shape == ref.shape, (tag, k, g.shape, ref.shape)
        gmax = float(np.abs(ref).max())
        bound = FACTOR * max(float(e_ref[k]), U * gmax)
        err = float(np.abs(g - ref).max())
        lines.append(f'[espnet_train] {tag} {k}: err {err:.3e}  e_ref {float(e_ref[k]):.3e}  unit {U * gmax:.3e}  err / yardstick '
                     f'{err / (bound / FACTOR):.2f}')
        if not err <= bound:
            bad.append((k, err, bound))
    print('\n'.join(lines))
    assert not bad, (tag, bad)


# ---- 1. the forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['c1_16x16', 'c3_48x80', 'c4_batch3'])
def test_forward_has_the_bits_of_the_eval_net(name):
    from trackmpnn_amd import EspEmbedNet, EspTrainNet
    fx, sd = load_case(name)
    x = torch.from_numpy(fx['images']).to(DEV)
    want = EspEmbedNet.from_state_dict(sd, DEV)(x)
    net = EspTrainNet.from_state_dict(sd, DEV)
    maps = net(x)
    assert maps.requires_grad and maps.grad_fn is not None
    assert torch.equal(_bits(maps.detach()), _bits(want))
    with torch.no_grad():
        quiet = net(x)
    assert not quiet.requires_grad and torch.equal(_bits(quiet), _bits(want))
    assert net.train() is net and net.eval() is net
    assert torch.equal(_bits(net(x).detach()), _bits(want))                 # both modes compute the same function
    # captured and replayed
    out = torch.zeros_like(want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        net(x, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        net(x, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))


# ---- 2. gradients against the reference module ------------------------------------------------------------------------------
@pytest.mark.parametrize('name,form', GRAD_CASES)
def test_gradients_within_eight_times_the_references_own_float32_error(name, form):
    g64, e_ref, _, sd = load_grad_case(name, form)
    got = device_grads(sd, case_images(name), case_d_maps(name, form))
    hold_to_rule(f'{name} {form}', got, g64, e_ref, _checked(CASES[name][1]))


# ---- 3. zero and negative slopes --------------------------------------------------------------------------------------------
def test_zero_and_negative_slopes():
    """Every decoder PReLU gets a zero and a negative slope: the backward must take the sign from the stored pre-activation."""
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
    hold_to_rule('slopes', device_grads(sd, images, d), h64, e_ref, _checked(CASES[name][1]))


# ---- 4. accumulation and determinism ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,form', [('c3_48x80', 'dense'), ('c4_batch3', 'sparse')])
def test_accumulation_and_determinism(name, form):
    _, sd = load_case(name)
    images, d = case_images(name), case_d_maps(name, form)
    once, again = device_grads(sd, images, d), device_grads(sd, images, d)
    assert sorted(once) == sorted(_checked(CASES[name][1]))
    for k in once:
        assert torch.equal(_bits(once[k]), _bits(again[k])), k             # two fresh runs: equal bits
        assert float(once[k].abs().max()) > 0.0, k
    twice = device_grads(sd, images, d, passes=2)
    bare = device_grads(sd, images, d, tap_grads=False)
    for k in bare:
        assert torch.equal(_bits(twice[k]), _bits(2.0 * once[k])), k       # no zero_grad in between: exactly twice
        assert torch.equal(_bits(bare[k]), _bits(once[k])), k              # the tap launches change no parameter gradient
    for k in ('out_l1', 'out_l2'):
        assert k not in bare and torch.equal(_bits(twice[k]), _bits(once[k]))      # tap gradients are overwritten, not added


def test_a_second_forward_invalidates_the_first_backward():
    from trackmpnn_amd import EspTrainNet
    _, sd = load_case('c1_16x16')
    net = EspTrainNet.from_state_dict(sd, DEV)
    x = torch.from_numpy(case_images('c1_16x16')).to(DEV)
    first = net(x)
    net(x)
    with pytest.raises(RuntimeError, match='before the backward'):
        first.sum().backward()


# ---- 5. the optimizer step and the refold -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['c3_48x80', 'c5_c128'])
def test_adam_step_and_refold(name):
    from trackmpnn_amd import BucketAdam, EspEmbedNet, EspTrainNet
    from trackmpnn_amd.dist import GradBucket
    from trackmpnn_amd.espnet import check_state_dict, trained_param_names
    from tests.test_optim_gpu import _err
    _, sd = load_case(name)
    C = CASES[name][1]
    x, d = torch.from_numpy(case_images(name)).to(DEV), torch.from_numpy(case_d_maps(name, 'dense')).to(DEV)
    lr, wd = 5e-4, 5e-4                                                     # the reference's embedding optimizer
    net = EspTrainNet.from_state_dict(sd, DEV)
    assert [k for k, _ in net.named_parameters()] == list(trained_param_names(C))
    assert len(list(net.parameters())) == 9 and all(isinstance(p, torch.nn.Parameter) for p in net.parameters())
    opt = torch.optim.Adam(net.parameters(), lr, weight_decay=wd)
    opt.zero_grad()
    net(x).backward(d)
    grads = [p.grad.detach().clone() for p in net.parameters()]
    opt.step()
    after = net.state_dict()
    assert check_state_dict(after) == C and list(after) == list(sd)
    for k in sd:
        same = torch.equal(after[k].cpu(), sd[k])
        assert same != (k in trained_param_names(C)), k                    # every trained tensor moved, nothing else did
    # the next forward runs on the refolded arena: the bits of an eval net packed on the host from the same tensors
    want = EspEmbedNet.from_state_dict(after, DEV)(x)
    assert torch.equal(_bits(net(x).detach()), _bits(want))
    assert torch.equal(_bits(net.snapshot()(x)), _bits(want))
    # BucketAdam over GradBucket(net) from the same gradients, held to torch's own float32 error as tests/test_optim_gpu.py does
    net2 = EspTrainNet.from_state_dict(sd, DEV)
    bucket = GradBucket(net2)
    opt2 = BucketAdam(net2, bucket, lr=lr, weight_decay=wd)
    opt2.zero_grad()
    net2(x).backward(d)
    assert bucket.check_alias()
    for p, g in zip(net2.parameters(), grads):
        assert torch.equal(_bits(p.grad), _bits(g))                        # in place into the bucket: the same bits
    opt2.step()
    p0 = torch.cat([sd[k].reshape(-1) for k in trained_param_names(C)])
    p64 = torch.nn.Parameter(p0.double())
    p64.grad = torch.cat([g.reshape(-1) for g in grads]).double().cpu()
    torch.optim.Adam([p64], lr, weight_decay=wd).step()
    flat = lambda n: torch.cat([p.detach().reshape(-1) for p in n.parameters()]).double().cpu()
    e_torch, e_mine = _err(flat(net), p64.detach(), lr), _err(flat(net2), p64.detach(), lr)
    print(f'[espnet_train] {name}: err(BucketAdam) = {e_mine:.3e}, err(torch.optim.Adam fp32) = {e_torch:.3e}')
    assert e_torch > 0 and e_mine <= 4 * e_torch
    want2 = EspEmbedNet.from_state_dict(net2.state_dict(), DEV)(x)
    assert torch.equal(_bits(net2(x).detach()), _bits(want2))              # BucketAdam moved the version counter: refolded


# ---- 6. through the library -------------------------------------------------------------------------------------------------
def _vis_set():
    from tests.test_chunk_draw import synth_sequences
    from tests.test_chunk_vis import IMG_MEAN, IMG_STD, vis_store, with_height
    from trackmpnn_amd import ChunkSampler, FrameStore, make_chunks
    seqs = with_height(synth_sequences(seed=21, lengths=(12, 9, 1, 14)))
    chunks = make_chunks([s['num_frames'] for s in seqs], 5, 3, rng=random.Random(22))
    sampler = ChunkSampler(vis_store(seqs, '2d+vis', DEV), chunks, seed=23)
    rng = np.random.default_rng(4)
    H, W = 32, 80
    fs = FrameStore([rng.integers(0, 256, (q['num_frames'], H, W, 3), dtype=np.uint8) for q in seqs], IMG_MEAN, IMG_STD, DEV)
    return sampler, fs, (H, W), chunks


def _tracker_and_head(hw):
    from tests.test_chunk_draw import NCAT
    from tests.test_chunk_vis import vis_stats
    from trackmpnn_amd import BucketAdam, TrackMPNN, VisHead
    from trackmpnn_amd.dist import GradBucket
    torch.manual_seed(9)
    model = TrackMPNN('2d+vis', NCAT, 32, 0, 'diff').to(DEV).train()
    opt = BucketAdam(model, GradBucket(model), lr=1e-3, weight_decay=0)
    mean, std = vis_stats('2d+vis')
    return model, opt, VisHead(hw, 1, mean, std, DEV)


@pytest.mark.parametrize('embed_loss', ['identity', 'embedding'])
def test_a_training_step_of_the_default_mode_without_a_torch_cnn(embed_loss):
    from trackmpnn_amd import EspTrainNet, VisTraining
    from trackmpnn_amd.loops import train_epoch
    from trackmpnn_amd.vishead import VIS_COLS
    sampler, fs, hw, chunks = _vis_set()
    _, sd = load_case('c5_c128')
    assert CASES['c5_c128'][1] == VIS_COLS
    net = EspTrainNet.from_state_dict(sd, DEV)
    before = [p.detach().clone() for p in net.parameters()]
    net_opt = torch.optim.Adam(net.parameters(), 5e-4, weight_decay=5e-4)
    model, opt, head = _tracker_and_head(hw)
    few = type(sampler)(sampler.store, chunks[:6], seed=23)
    steps = train_epoch(model, few, opt, 2, 0, vis=VisTraining(head, fs, net, net_opt, embed_loss))
    assert steps >= 1
    for a, p in zip(before, net.parameters()):
        assert bool(torch.isfinite(p).all()) and not torch.equal(a, p.detach())


def test_gradients_behind_the_head_equal_the_host_definition():
    """The parameter gradients of one slice's identity loss, through VisHead.forward's backward, against
    espnet_decoder_grads_host on the d_maps the head's backward handed over (the rule of this file's docstring)."""
    from trackmpnn_amd import AllChunksSkipped, EspTrainNet
    from trackmpnn_amd.espnet import espnet_decoder_grads_host
    sampler, fs, hw, _ = _vis_set()
    _, sd = load_case('c5_c128')
    net = EspTrainNet.from_state_dict(sd, DEV)
    _, _, head = _tracker_and_head(hw)
    for ci in sampler.epoch_order(0):
        drawn = sampler.draw([ci], 0)
        try:
            drawn.batch()
            break
        except AllChunksSkipped:
            continue
    images = fs.gather(drawn.plan)
    maps = net(images, tap_grads=True)
    seen = []
    maps.register_hook(lambda g: seen.append(g.detach().clone()))
    drawn.attach_vis(head, maps).sum().backward()
    assert len(seen) == 1 and float(seen[0].abs().max()) > 0.0
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    got.update({k: v.cpu() for k, v in net.tap_grads.items() if v is not None})
    x, d = images.cpu(), seen[0].cpu()
    h64 = {k: v.numpy() for k, v in espnet_decoder_grads_host(sd, x, d, torch.float64).items()}
    h32 = espnet_decoder_grads_host(sd, x, d, torch.float32)
    e_ref = {k: float(np.abs(h32[k].numpy().astype(np.float64) - h64[k]).max()) for k in h64}
    hold_to_rule('behind the head', got, h64, e_ref, _checked(128))
