"""The embedding CNN: the reference's default `--embed-arch espv2`, EESPNet_Seg(classes=C, s=1) (models/espv2), in eval mode.

    espnet_spec(C)          every tensor name of the net's state_dict() with its shape: the DEFINITION of what loads
    espnet_host(sd, images) the eval forward over a state dict with torch ops, written from the architecture (float64: the
                            yardstick of the device tests; on a device tensor torch runs it through MIOpen: the timing baseline)
    fold_bn                 a BatchNorm's running statistics as a per-channel scale and shift, float64 then rounded once
    pack_arena(sd, C)       the float32 weight arena of the device (layout: include/tmpnn.h, struct-free: one array)
    EspEmbedNet             the same forward on the device (tmpnn_espnet_fwd; csrc/espnet.hip): `net(images) -> maps`, drops in
                            wherever an `embed_net` is taken (OnlineVis, VisInference, SequenceFeatures.attach_vis)
    espnet_centres_host(sd, images, pix)    espnet_host(...)[t, :, cy, cx] for pix = (t H + cy) W + cx: the DEFINITION of
                            what the net answers at single pixels
    EspCentres              `net.centres(images)`: the net run up to its C-channel map at 1/8 size (tmpnn_espnet_trunk), and
                            `.logits_at(pix)` the rest of the decoder at the pixels asked for (tmpnn_espnet_centres), equal bit
                            for bit to the dense map there
    espnet_decoder_grads_host(sd, images, d_maps)   the gradients of the 36 decoder tensors and at the four encoder taps by
                            torch autograd over espnet_host's ops: the DEFINITION of the decoder's backward
    EspTrainNet             the same forward with a backward on the device (tmpnn_espnet_train_fwd / _bwd / tmpnn_espnet_refold and
                            their tmpnn_espnet_dec_* siblings; csrc/espnet_train.hip): fine-tuning with frozen statistics;
                            scope='tail' (the default) trains the decoder behind merge_l3 (9 of the 36 tensors of
                            decoder_param_names), scope='decoder' all 36; the encoder is frozen in both

The sparse path.  VisHead reads one pixel per detection, and everything behind the 1/8-size map is pointwise convs and x2 bilinear
steps: one output pixel depends on 2 x 2 pixels of merge_l1, 3 x 3 of merge_l2 and their taps at 1/8 size.  So for inference
`EspEmbedNet.from_state_dict(sd, device, centres=True)` makes `net(images)` return an EspCentres in the map's place, which
VisHead.rows takes as it takes the map; the dense tail's five launches, their four workspace maps (2 C (P4 + P2) floats an image)
and the [T, C, H, W] result are not made.  Training through VisHead.forward keeps the dense map (its backward hands d(maps) to
EspTrainNet's backward, or to a torch CNN).

The net.  Encoder (widths 32 / 64 / 128 / 256 at 1/2, 1/4, 1/8, 1/16 of the input):
    level1      3x3 stride-2 conv 3 -> 32, BN, PReLU
    level2_0    DownSampler 32 -> 64;  level3_0  DownSampler 64 -> 128, then 3 EESP(128);  level4_0  DownSampler 128 -> 256, then
                7 EESP(256)
    DownSampler(nin, nout)(x, image) = PReLU(cat[avg_pool3x3 s2 p1 (x), EESP_s2(x)] + inp_reinf(image pooled to that size));
                the pool counts its padding (every window / 9); inp_reinf = 3x3 conv 3 -> 3, BN, PReLU, 1x1 conv 3 -> nout, BN; its
                stride-2 EESP returns before the residual and the PReLU
    EESP(nin, nout, stride, r_lim): grouped 1x1 conv (groups 4) nin -> n = nout / 4, BN, PReLU; four depthwise 3x3 convs of dilation
                d_k (padding d_k, the block's stride) fused as out_k = conv_k + out_{k-1} for every k >= 1; concat, BN, PReLU;
                grouped 1x1 conv nout -> nout (groups 4), BN; + input where the shapes agree; PReLU.  The dilations are
                ((s - 1) / 2 for s in sorted(3 + 2 i if 3 + 2 i <= r_lim else 3 for i in 0..3)): 1 2 3 4 for r_lim >= 9 (level2_0,
                level3_0, level3, level4_0), 1 1 2 3 for r_lim = 7 (level4, pspMod)
Decoder: proj_L4_C (1x1 256 -> 128, BN, PReLU), bilinear x2, pspMod = EESP(256 -> 128) over cat[out_l3, up] then the PSP module (four
times: pool the previous level 3x3 s2 p1, depthwise 3x3, bilinear back to the level-3 size; concat 5 x 128; 1x1 640 -> 128, BN,
PReLU), project_l3 (1x1 128 -> C), act_l3 (BN, PReLU), x2, project_l2 (1x1 64 + C -> C, BN, PReLU over cat[out_l2, up]), x2,
project_l1 (1x1 32 + C -> C, nothing else, over cat[out_l1, up]), x2.  Every bilinear is align_corners=True.  Every BatchNorm uses
its running statistics and both Dropout2d are the identity.

Training (EspTrainNet).  The reference draws the line itself: EESPNet_Seg.net is the ImageNet-pretrained encoder, everything else
is initialised for this task.  EspTrainNet differentiates exactly the eval forward above -- running statistics, not updated, and
Dropout2d the identity: fine-tuning with frozen statistics -- with respect to the decoder: with scope='tail' the part behind
merge_l3 (project_l3, act_l3, project_l2, project_l1; proj_L4_C and pspMod frozen with the encoder), with scope='decoder' all of it,
which is what the reference's optimizer moves outside the encoder; the gradients then reach all four encoder taps.

Out of scope: batch statistics, Dropout2d in training mode, the encoder's backward, the reference's other backbone (dla34 / DCNv2), s != 1, ImageNet classification checkpoints (they hold level5 and a classifier).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

BN_EPS = 1e-5
_BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')
_PSP = 128
MAX_CENTRES_C = 256            # channels the per-centre tail serves (csrc/espnet.hip ESPC_MAX_C)


def _dilations(r_lim: int) -> Tuple[int, ...]:
    sizes = sorted(3 + 2 * i if 3 + 2 * i <= r_lim else 3 for i in range(4))
    return tuple((s - 1) // 2 for s in sizes)


# ---- the state dict ----------------------------------------------------------------------------------------------------------
def _spec_bn(spec, p, c):
    for k in _BN_KEYS:
        spec[f'{p}.{k}'] = (c,)


def _spec_cbr(spec, p, cin, cout, k, groups=1, bn=True, act=True):
    spec[f'{p}.conv.weight'] = (cout, cin // groups, k, k)
    if bn:
        _spec_bn(spec, f'{p}.bn', cout)
    if act:
        spec[f'{p}.act.weight'] = (cout,)


def _spec_eesp(spec, p, nin, nout):
    n = nout // 4
    _spec_cbr(spec, f'{p}.proj_1x1', nin, n, 1, groups=4)
    for i in range(4):
        spec[f'{p}.spp_dw.{i}.conv.weight'] = (n, 1, 3, 3)
    _spec_cbr(spec, f'{p}.conv_1x1_exp', nout, nout, 1, groups=4, act=False)
    _spec_bn(spec, f'{p}.br_after_cat.bn', nout)
    spec[f'{p}.br_after_cat.act.weight'] = (nout,)
    spec[f'{p}.module_act.weight'] = (nout,)


def _spec_down(spec, p, nin, nout):
    _spec_eesp(spec, f'{p}.eesp', nin, nout - nin)
    _spec_cbr(spec, f'{p}.inp_reinf.0', 3, 3, 3)
    _spec_cbr(spec, f'{p}.inp_reinf.1', 3, nout, 1, act=False)
    spec[f'{p}.act.weight'] = (nout,)


def espnet_spec(C: int) -> 'OrderedDict[str, Tuple[int, ...]]':
    """name -> shape of every tensor EESPNet_Seg(classes=C, s=1).state_dict() holds, the BatchNorms' num_batches_tracked
    (shape (), accepted and ignored) left out."""
    C = int(C)
    if C < 1 or C > 1024:
        raise ValueError(f'espnet: C={C} (1 .. 1024 expected)')
    s: 'OrderedDict[str, Tuple[int, ...]]' = OrderedDict()
    _spec_cbr(s, 'net.level1', 3, 32, 3)
    _spec_down(s, 'net.level2_0', 32, 64)
    _spec_down(s, 'net.level3_0', 64, 128)
    for i in range(3):
        _spec_eesp(s, f'net.level3.{i}', 128, 128)
    _spec_down(s, 'net.level4_0', 128, 256)
    for i in range(7):
        _spec_eesp(s, f'net.level4.{i}', 256, 256)
    _spec_cbr(s, 'proj_L4_C', 256, _PSP, 1)
    _spec_eesp(s, 'pspMod.0', 2 * _PSP, _PSP)
    for i in range(4):
        s[f'pspMod.1.stages.{i}.conv.weight'] = (_PSP, 1, 3, 3)
    _spec_cbr(s, 'pspMod.1.project', 5 * _PSP, _PSP, 1)
    s['project_l3.1.conv.weight'] = (C, _PSP, 1, 1)
    _spec_bn(s, 'act_l3.bn', C)
    s['act_l3.act.weight'] = (C,)
    _spec_cbr(s, 'project_l2', 64 + C, C, 1)
    s['project_l1.1.conv.weight'] = (C, 32 + C, 1, 1)
    return s


def check_state_dict(sd) -> int:
    """C of a state dict that is exactly EESPNet_Seg(classes=C, s=1).state_dict(); ValueError naming the first key that is
    missing, unexpected or of the wrong shape."""
    if not hasattr(sd, 'keys'):
        raise ValueError('espnet: a state dict (name -> tensor) expected')
    keys = list(sd.keys())
    if keys and all(str(k).startswith('module.') for k in keys):
        raise ValueError("espnet: every key starts with 'module.': this is the state dict of a DataParallel wrapper; save "
                         "model.module.state_dict(), or strip the prefix, and load that")
    k3 = 'project_l3.1.conv.weight'
    if k3 not in sd:
        raise ValueError(f'espnet: missing key {k3}')
    w3 = sd[k3]
    if w3.dim() != 4 or tuple(w3.shape[1:]) != (_PSP, 1, 1):
        raise ValueError(f'espnet: {k3} of shape {tuple(w3.shape)}; (C, {_PSP}, 1, 1) expected')
    spec = espnet_spec(int(w3.shape[0]))
    for k, shp in spec.items():
        if k not in sd:
            raise ValueError(f'espnet: missing key {k}')
        if tuple(sd[k].shape) != shp:
            raise ValueError(f'espnet: {k} of shape {tuple(sd[k].shape)}; {shp} expected')
    for k in keys:
        if k in spec:
            continue
        if str(k).endswith('.num_batches_tracked') and str(k)[:-len('num_batches_tracked')] + 'weight' in spec:
            continue
        raise ValueError(f'espnet: unexpected key {k}')
    return int(w3.shape[0])


# ---- the host definition -----------------------------------------------------------------------------------------------------
def espnet_host(sd, images, dtype=torch.float64, taps: bool = False):
    """maps [T, C, H, W] in `dtype` on the device of `images`: the eval forward (module docstring) over the state dict `sd` with
    torch ops.  images [T, 3, H, W], H and W positive multiples of 16.  taps=True: (maps, {'out_l1' .. 'out_l4': the encoder
    outputs, 'merge_l3', 'merge_l2', 'merge_l1': the decoder merges before each upsampling})."""
    check_state_dict(sd)
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[1] != 3:
        raise ValueError('espnet_host: images [T, 3, H, W] expected')
    _check_hw(int(images.shape[2]), int(images.shape[3]))
    dev = images.device
    x = images.detach().to(dtype)
    out, tp = _host_forward(lambda k: sd[k].detach().to(device=dev, dtype=dtype), x)
    return (out, tp) if taps else out


def _host_forward(g, x, tap=None):
    """(maps, taps and merges) of the eval forward on x [T, 3, H, W]; g(name) gives a tensor of the state dict in x's dtype on
    x's device (espnet_host hands detached ones over, espnet_decoder_grads_host leaves that require a gradient).  tap(t): what the
    decoder reads in the place of each encoder output t (espnet_decoder_grads_host cuts the graph there)."""

    def bn(v, p):
        return F.batch_norm(v, g(p + '.running_mean'), g(p + '.running_var'), g(p + '.weight'), g(p + '.bias'), False, 0.0, BN_EPS)

    def conv(v, p, stride=1, pad=0, dil=1, groups=1):
        return F.conv2d(v, g(p + '.conv.weight'), None, stride, pad, dil, groups)

    def pool(v):
        return F.avg_pool2d(v, kernel_size=3, stride=2, padding=1)

    def up(v, size=None):
        if size is None:
            size = (2 * v.shape[2], 2 * v.shape[3])
        return F.interpolate(v, size=size, mode='bilinear', align_corners=True)

    def cbr(v, p, **kw):
        return F.prelu(bn(conv(v, p, **kw), p + '.bn'), g(p + '.act.weight'))

    def eesp(v, p, stride, r_lim, down):
        r = cbr(v, p + '.proj_1x1', groups=4)
        outs = []
        for k, d in enumerate(_dilations(r_lim)):
            o = F.conv2d(r, g(f'{p}.spp_dw.{k}.conv.weight'), None, stride, d, d, r.shape[1])
            outs.append(o if k == 0 else o + outs[k - 1])
        cat = torch.cat(outs, 1)
        cat = F.prelu(bn(cat, p + '.br_after_cat.bn'), g(p + '.br_after_cat.act.weight'))
        e = bn(conv(cat, p + '.conv_1x1_exp', groups=4), p + '.conv_1x1_exp.bn')
        if down:
            return e
        if e.shape == v.shape:
            e = e + v
        return F.prelu(e, g(p + '.module_act.weight'))

    def down(v, p, r_lim, image):
        o = torch.cat([pool(v), eesp(v, p + '.eesp', 2, r_lim, True)], 1)
        r = cbr(image, p + '.inp_reinf.0', pad=1)
        r = bn(conv(r, p + '.inp_reinf.1'), p + '.inp_reinf.1.bn')
        return F.prelu(o + r, g(p + '.act.weight'))

    img2 = pool(x)
    img4 = pool(img2)
    img8 = pool(img4)
    img16 = pool(img8)
    out_l1 = cbr(x, 'net.level1', stride=2, pad=1)
    out_l2 = down(out_l1, 'net.level2_0', 13, img4)
    out_l3 = down(out_l2, 'net.level3_0', 11, img8)
    for i in range(3):
        out_l3 = eesp(out_l3, f'net.level3.{i}', 1, 9, False)
    out_l4 = down(out_l3, 'net.level4_0', 9, img16)
    for i in range(7):
        out_l4 = eesp(out_l4, f'net.level4.{i}', 1, 7, False)
    if tap is not None:
        out_l1, out_l2, out_l3, out_l4 = tap(out_l1), tap(out_l2), tap(out_l3), tap(out_l4)

    p4 = cbr(out_l4, 'proj_L4_C')
    feats = eesp(torch.cat([out_l3, up(p4)], 1), 'pspMod.0', 1, 7, False)
    hw = (feats.shape[2], feats.shape[3])
    stages, lvl = [feats], feats
    for k in range(4):
        lvl = pool(lvl)
        stages.append(up(F.conv2d(lvl, g(f'pspMod.1.stages.{k}.conv.weight'), None, 1, 1, 1, _PSP), hw))
    merge_l3 = cbr(torch.cat(stages, 1), 'pspMod.1.project')
    m3 = F.prelu(bn(conv(merge_l3, 'project_l3.1'), 'act_l3.bn'), g('act_l3.act.weight'))
    merge_l2 = cbr(torch.cat([out_l2, up(m3)], 1), 'project_l2')
    merge_l1 = conv(torch.cat([out_l1, up(merge_l2)], 1), 'project_l1.1')
    out = up(merge_l1)
    return out, {'out_l1': out_l1, 'out_l2': out_l2, 'out_l3': out_l3, 'out_l4': out_l4, 'merge_l3': merge_l3,
                 'merge_l2': merge_l2, 'merge_l1': merge_l1}


def espnet_centres_host(sd, images, pix, dtype=torch.float64):
    """logits [D, C] in `dtype`: espnet_host(sd, images, dtype)[t, :, cy, cx] for every pix = (t H + cy) W + cx in [0, T H W).
    The definition of EspCentres.logits_at."""
    out = espnet_host(sd, images, dtype)
    T, _, H, W = (int(v) for v in out.shape)
    px = torch.as_tensor(np.asarray(pix.detach().cpu().numpy() if isinstance(pix, torch.Tensor) else pix, dtype=np.int64).ravel())
    if px.numel() and (int(px.min()) < 0 or int(px.max()) >= T * H * W):
        raise ValueError(f'espnet_centres_host: a pix outside [0, {T * H * W})')
    px = px.to(out.device)
    t, rem = px // (H * W), px % (H * W)
    return out[t, :, rem // W, rem % W]


# ---- training the decoder: names and the host definition ---------------------------------------------------------------------
def decoder_param_names(C: int) -> Tuple[str, ...]:
    """The 36 tensors of the reference's decoder that an optimizer sees (proj_L4_C, pspMod, project_l3, act_l3, project_l2,
    project_l1; no running statistic), in the order of espnet_spec(C)."""
    return tuple(k for k in espnet_spec(C) if not k.startswith('net.') and not k.endswith(('running_mean', 'running_var')))


SCOPES = ('tail', 'decoder')


def _check_scope(scope) -> str:
    if scope not in SCOPES:
        raise ValueError(f'espnet: scope={scope!r}; one of {SCOPES} expected')
    return scope


def trained_param_names(C: int, scope: str = 'tail') -> Tuple[str, ...]:
    """The tensors EspTrainNet trains.  scope='tail': the decoder behind merge_l3 (project_l3, act_l3, project_l2, project_l1: 9
    tensors), the other 27 of decoder_param_names (proj_L4_C, pspMod) frozen with the encoder.  scope='decoder': all 36."""
    if _check_scope(scope) == 'decoder':
        return decoder_param_names(C)
    return tuple(k for k in decoder_param_names(C) if k.startswith(('project_l3.', 'act_l3.', 'project_l2.', 'project_l1.')))


def trained_norm_names(C: int, scope: str = 'tail') -> Tuple[str, ...]:
    """The BatchNorms among the trained tensors, in the state dict's order: their running statistics are what the library takes
    as `stats` (running_mean | running_var of each)."""
    return tuple(k[:-len('.weight')] for k in trained_param_names(C, scope) if k.endswith('bn.weight'))


def espnet_decoder_grads_host(sd, images, d_maps, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """{name: gradient} of sum(maps * d_maps) for the 36 tensors of decoder_param_names and for the four encoder taps 'out_l1' ..
    'out_l4' (the gradient that reaches each tap through the decoder: where an encoder backward would start), in `dtype` on the
    device of `images`.  maps = espnet_host(sd, images, dtype): torch autograd over the same ops, running statistics and all.  The
    definition EspTrainNet's backward is tested against."""
    C = check_state_dict(sd)
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[1] != 3:
        raise ValueError('espnet_decoder_grads_host: images [T, 3, H, W] expected')
    _check_hw(int(images.shape[2]), int(images.shape[3]))
    dev = images.device
    names = decoder_param_names(C)
    leaves = {k: sd[k].detach().to(device=dev, dtype=dtype).clone().requires_grad_(True) for k in names}
    cut = []

    def g(k):
        return leaves[k] if k in leaves else sd[k].detach().to(device=dev, dtype=dtype)

    def tap(t):
        cut.append(t.detach().requires_grad_(True))
        return cut[-1]

    with torch.enable_grad():
        out, _ = _host_forward(g, images.detach().to(dtype), tap)
        d = torch.as_tensor(d_maps).detach().to(device=dev, dtype=dtype)
        if tuple(d.shape) != tuple(out.shape):
            raise ValueError(f'espnet_decoder_grads_host: d_maps of shape {tuple(d.shape)}; {tuple(out.shape)} expected')
        grads = torch.autograd.grad((out * d).sum(), [leaves[k] for k in names] + cut)
    res = dict(zip(names, grads[:len(names)]))
    res.update(zip(('out_l1', 'out_l2', 'out_l3', 'out_l4'), grads[len(names):]))
    return res


def _check_hw(H: int, W: int) -> None:
    if H <= 0 or W <= 0 or H % 16 or W % 16:
        raise ValueError(f'espnet: images of {H} x {W}; H and W must be positive multiples of 16 (the decoder concatenates maps '
                         'of 1/2, 1/4 and 1/8 of the input with upsampled ones)')


# ---- the device's weights ----------------------------------------------------------------------------------------------------
def fold_bn(weight, bias, running_mean, running_var, eps: float = BN_EPS) -> Tuple[np.ndarray, np.ndarray]:
    """(scale, shift) float32 with BN(x) = x scale + shift for the running statistics: computed in float64, rounded once."""
    w, b, m, v = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64)
                  for t in (weight, bias, running_mean, running_var))
    scale = w / np.sqrt(v + eps)
    return scale.astype(np.float32), (b - m * scale).astype(np.float32)


def pack_arena(sd, C: Optional[int] = None) -> np.ndarray:
    """The float32 weight arena tmpnn_espnet_fwd reads (the segment order is documented in include/tmpnn.h)."""
    c = check_state_dict(sd)
    if C is not None and int(C) != c:
        raise ValueError(f'espnet: the state dict has C={c}, not {C}')
    C = c
    segs = []

    def a(k):
        return sd[k].detach().cpu().numpy().astype(np.float32)

    def seg(x):
        x = np.ascontiguousarray(x, np.float32).ravel()
        pad = (-x.size) % 4
        segs.append(np.concatenate([x, np.zeros(pad, np.float32)]) if pad else x)

    def norm(p, c):
        if p is None:
            seg(np.ones(c, np.float32)), seg(np.zeros(c, np.float32))
        else:
            s, t = fold_bn(*(sd[f'{p}.{k}'] for k in _BN_KEYS))
            seg(s), seg(t)

    def pw(conv, bn, slope):
        w = a(conv + '.weight')[:, :, 0, 0]                      # [cout][cin / groups]
        seg(w.T)
        norm(bn, w.shape[0])
        seg(np.ones(w.shape[0], np.float32) if slope is None else slope)

    def eesp(p, exp_slope):
        pw(p + '.proj_1x1.conv', p + '.proj_1x1.bn', a(p + '.proj_1x1.act.weight'))
        seg(np.stack([a(f'{p}.spp_dw.{k}.conv.weight').reshape(-1, 9) for k in range(4)]))
        norm(p + '.br_after_cat.bn', 0)
        seg(a(p + '.br_after_cat.act.weight'))
        pw(p + '.conv_1x1_exp.conv', p + '.conv_1x1_exp.bn', exp_slope)

    def down(p, nin):
        seg(a(p + '.inp_reinf.0.conv.weight'))
        norm(p + '.inp_reinf.0.bn', 3)
        seg(a(p + '.inp_reinf.0.act.weight'))
        seg(a(p + '.inp_reinf.1.conv.weight')[:, :, 0, 0].T)
        norm(p + '.inp_reinf.1.bn', 0)
        act = a(p + '.act.weight')
        seg(act[:nin])
        eesp(p + '.eesp', act[nin:])

    seg(a('net.level1.conv.weight'))
    norm('net.level1.bn', 32)
    seg(a('net.level1.act.weight'))
    down('net.level2_0', 32)
    down('net.level3_0', 64)
    for i in range(3):
        eesp(f'net.level3.{i}', a(f'net.level3.{i}.module_act.weight'))
    down('net.level4_0', 128)
    for i in range(7):
        eesp(f'net.level4.{i}', a(f'net.level4.{i}.module_act.weight'))
    pw('proj_L4_C.conv', 'proj_L4_C.bn', a('proj_L4_C.act.weight'))
    eesp('pspMod.0', a('pspMod.0.module_act.weight'))
    for i in range(4):
        seg(a(f'pspMod.1.stages.{i}.conv.weight'))
    pw('pspMod.1.project.conv', 'pspMod.1.project.bn', a('pspMod.1.project.act.weight'))
    pw('project_l3.1.conv', 'act_l3.bn', a('act_l3.act.weight'))
    pw('project_l2.conv', 'project_l2.bn', a('project_l2.act.weight'))
    pw('project_l1.1.conv', None, None)
    arena = np.concatenate(segs)
    want = int(_lib.fn('tmpnn_espnet_arena_floats')(C))
    if arena.size != want:
        raise RuntimeError(f'espnet: packed {arena.size} floats, the library expects {want} for C={C}')
    return arena


class EspEmbedNet:
    """EESPNet_Seg(classes=C, s=1) in eval mode on the device (module docstring).

        net = EspEmbedNet.from_state_dict(sd)           sd: the torch module's state_dict() (a vis-net_*.pth snapshot)
        maps = net(images, out=None)                    images [T, 3, H, W] float32 contiguous on the device, H and W multiples
                                                        of 16 -> maps [T, C, H, W] float32 contiguous NCHW (what VisHead reads)

    No autograd graph is built.  The workspace of a (T, H, W) is allocated at its first call and reused; a call then allocates
    nothing but its result (nothing at all with `out`), waits for nothing and reads nothing back; every launch goes on the
    current stream and their number (70) does not depend on T.  Results are bitwise reproducible, and image i of a batch gives
    the same bits for every T.

        h = net.centres(images)                         the trunk alone (65 launches); h.logits_at(pix) -> ([D, C], flags [D])
        net = EspEmbedNet.from_state_dict(sd, dev, centres=True)       net(images) returns that handle (inference behind VisHead)
  The net is an eval-mode network: `training` is False, eval() and train(False) return it,
    train(True) raises."""

    training = False
    _sparse = False              # centres=True: __call__ returns centres(images)

    def __init__(self, sd, device='cuda:0', centres: bool = False):
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'EspEmbedNet on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path): pass a cuda '
                               'device')
        self.C = check_state_dict(sd)
        self._sd = OrderedDict(sd.items())
        arena = pack_arena(sd, self.C)
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        self._arena = torch.from_numpy(arena).to(dev)
        self._ws: Dict[Tuple[int, int, int], torch.Tensor] = {}
        self._fwd = _lib.fn('tmpnn_espnet_fwd')
        self._sparse = bool(centres)
        self._cws: Dict[Tuple[int, int, int], torch.Tensor] = {}             # the smaller workspaces of centres()
        self._cgen: Dict[Tuple[int, int, int], int] = {}                      # calls of centres() per shape: a handle's validity

    @classmethod
    def from_state_dict(cls, sd, device='cuda:0', centres: bool = False) -> 'EspEmbedNet':
        """centres=True: `net(images)` returns `net.centres(images)`, the handle VisHead.rows reads per detection, in the dense
        map's place (inference: OnlineVis, VisInference, SequenceFeatures.attach_vis run sparse with nothing else changed)."""
        return cls(sd, device, centres)

    def state_dict(self):
        """The tensors `from_state_dict` was given, under their names."""
        return OrderedDict(self._sd.items())

    def eval(self) -> 'EspEmbedNet':
        return self

    def train(self, mode: bool = True) -> 'EspEmbedNet':
        if mode:
            raise NotImplementedError('eval-mode network: train the CNN in torch')
        return self

    def _check_images(self, images) -> Tuple[int, int, int]:
        if not isinstance(images, torch.Tensor) or images.device.type != 'cuda':
            raise RuntimeError('EspEmbedNet: images on the host: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path)')
        if images.device != self.device or images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
            raise ValueError(f'EspEmbedNet: images [T, 3, H, W] float32 on {self.device} expected, got {tuple(images.shape)} '
                             f'{images.dtype} on {images.device}')
        T, _, H, W = (int(v) for v in images.shape)
        _check_hw(H, W)
        if not images.is_contiguous():
            raise ValueError('EspEmbedNet: images must be contiguous')
        if T < 1:
            raise ValueError('EspEmbedNet: an empty batch')
        return T, H, W

    def centres(self, images) -> 'EspCentres':
        """The trunk of the net on `images` (as __call__ takes and checks them): 65 launches that leave the encoder outputs at
        1/2 and 1/4 size and the C-channel map at 1/8 size in a workspace of this (T, H, W), allocated at the first call of the
        shape and smaller than the dense call's by its four tail maps.  The handle answers `logits_at(pix)`.  It reads that
        workspace, so it is valid until the net's next centres() call of the same shape (using it later raises).  C <= 256."""
        T, H, W = self._check_images(images)
        if self.C > MAX_CENTRES_C:
            raise ValueError(f'EspEmbedNet.centres: C={self.C}; the per-centre tail serves C <= {MAX_CENTRES_C}: take the dense '
                             'call, net(images), of a net built with centres=False')
        ws = self._cws.get((T, H, W))
        if ws is None:
            nbytes = int(_lib.fn('tmpnn_espnet_centres_ws_bytes')(T, H, W, self.C))
            if nbytes == 0 or T * H * W >= 2 ** 31:
                raise ValueError(f'EspEmbedNet: a batch of {T} x {H} x {W} with C={self.C} is too large for one call (T <= 65535, '
                                 'max(C, 160) H W < 2^31, T H W < 2^31)')
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._cws[(T, H, W)] = ws
        _lib.call('tmpnn_espnet_trunk', self._arena.data_ptr(), self.C, images.data_ptr(), T, H, W, ws.data_ptr(), ws.numel(),
                  _lib.raw_stream(self.device))
        gen = self._cgen.get((T, H, W), 0) + 1
        self._cgen[(T, H, W)] = gen
        return EspCentres(self, ws, T, H, W, gen)

    def __call__(self, images, out: Optional[torch.Tensor] = None):
        if self._sparse:
            if out is not None:
                raise ValueError('EspEmbedNet: out given to a net built with centres=True (it returns a handle, not a map)')
            return self.centres(images)
        T, H, W = self._check_images(images)
        ws = self._ws.get((T, H, W))
        if ws is None:
            nbytes = int(_lib.fn('tmpnn_espnet_ws_bytes')(T, H, W, self.C))
            if nbytes == 0:
                raise ValueError(f'EspEmbedNet: a batch of {T} x {H} x {W} with C={self.C} is too large for one call (T <= 65535, '
                                 'max(C, 160) H W < 2^31)')
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws[(T, H, W)] = ws
        if out is None:
            out = torch.empty((T, self.C, H, W), dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
              or tuple(out.shape) != (T, self.C, H, W) or not out.is_contiguous()):
            raise ValueError(f'EspEmbedNet: out [{T}, {self.C}, {H}, {W}] float32 contiguous on {self.device} expected')
        rc = self._fwd(self._arena.data_ptr(), self.C, images.data_ptr(), T, H, W, ws.data_ptr(), ws.numel(), out.data_ptr(),
                       _lib.raw_stream(self.device))
        if rc != 0:
            raise RuntimeError(f'tmpnn_espnet_fwd failed (code {rc}): {_lib.last_error()}')
        return out


class EspCentres:
    """What `EspEmbedNet.centres(images)` returns: the net's answer to `images`, read per pixel.

        h.T, h.C, h.H, h.W, h.shape == (T, C, H, W)     the map it stands for
        logits, flags = h.logits_at(pix)                pix [D] int32 on the device, pix = (t H + cy) W + cx
                                                        -> logits [D, C] float32 = net(images)[t, :, cy, cx] bit for bit (one
                                                        launch on the current stream, no host wait), flags [D] int32: 1 where
                                                        a pix lay outside [0, T H W) and was clamped into it

    VisHead.rows takes the handle in the map's place.  It holds no map: it reads the workspace the trunk filled, which the net's
    next centres() call of the same (T, H, W) overwrites -- the handle is valid until then, and logits_at raises afterwards."""

    def __init__(self, net: EspEmbedNet, ws: torch.Tensor, T: int, H: int, W: int, gen: int):
        self._net, self._ws, self._gen = net, ws, gen
        self.T, self.C, self.H, self.W = T, net.C, H, W
        self.shape = (T, net.C, H, W)
        self.device = net.device

    def logits_at(self, pix, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        net = self._net
        if net._cgen.get((self.T, self.H, self.W)) != self._gen:
            raise RuntimeError("EspCentres: the net's centres() has run again on this shape and overwritten what this handle reads")
        if (not isinstance(pix, torch.Tensor) or pix.device != self.device or pix.dtype != torch.int32 or pix.dim() != 1
                or not pix.is_contiguous()):
            raise ValueError(f'EspCentres.logits_at: pix [D] int32 contiguous on {self.device} expected')
        D = int(pix.shape[0])
        if out is None:
            out = torch.empty((D, self.C), dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
              or tuple(out.shape) != (D, self.C) or not out.is_contiguous()):
            raise ValueError(f'EspCentres.logits_at: out [{D}, {self.C}] float32 contiguous on {self.device} expected')
        flags = torch.empty(D, dtype=torch.int32, device=self.device)
        if D:
            _lib.call('tmpnn_espnet_centres', net._arena.data_ptr(), self.C, self.T, self.H, self.W, self._ws.data_ptr(),
                      self._ws.numel(), pix.data_ptr(), D, out.data_ptr(), flags.data_ptr(), _lib.raw_stream(self.device))
        return out, flags


# ---- training the decoder on the device --------------------------------------------------------------------------------------
class _EspTrainFn(torch.autograd.Function):
    """maps = net(images) with a backward on the device.  The parameters are inputs, so plain autograd works (the gradients come
    back as views of one fresh flat buffer); where every p.grad already aliases one flat buffer in the net's layout (GradBucket(net))
    the kernels add into it directly and autograd receives None: the in-place convention of functional.INPLACE_GRADS / GradBucket,
    valid for a plain loss.backward()."""

    @staticmethod
    def forward(ctx, net, images, taps, out, *params):
        ctx.net, ctx.taps = net, bool(taps)
        ctx.key, ctx.gen = net._forward(images, out)
        return net._out

    @staticmethod
    def backward(ctx, d_maps):
        net = ctx.net
        grads = net._backward(ctx.key, ctx.gen, d_maps, ctx.taps)
        return (None, None, None, None) + tuple(grads)


class EspTrainNet(torch.nn.Module):
    """EESPNet_Seg(classes=C, s=1) on the device with a trainable decoder: FINE-TUNING WITH FROZEN STATISTICS.

        net = EspTrainNet.from_state_dict(sd)           sd: the torch module's state_dict(); trains the decoder's tail
        net = EspTrainNet.from_state_dict(sd, dev, scope='decoder')            trains the whole decoder (below)
        maps = net(images)                              [T, C, H, W] float32, the bits of EspEmbedNet for the same weights; under
                                                        torch.no_grad() just the forward, else maps carry a grad_fn
        opt = torch.optim.Adam(net.parameters(), 5e-4, weight_decay=5e-4)      or BucketAdam(net, GradBucket(net), ...)
        loss.backward(); opt.step()                     the backward runs on the device (tmpnn_espnet_train_bwd, 13 launches)
        train_epoch(..., vis=VisTraining(head, frames, net, opt))              a training step with no torch CNN in it

    The function differentiated is exactly the eval forward (espnet_host): every BatchNorm uses its running statistics and does not
    update them, both Dropout2d are the identity; train() and eval() return the net and compute the same function.
    Trained: the decoder behind merge_l3 -- project_l3.1.conv, act_l3.{bn, act}, project_l2.{conv, bn, act}, project_l1.1.conv: the
    9 tensors of trained_param_names(C), as torch.nn.Parameter views of ONE flat float32 buffer in espnet_spec order under the
    reference's names.  Frozen: every net.* tensor (the pretrained encoder), every running statistic, and -- the cut of this version
    -- proj_L4_C and pspMod (the other 27 tensors of decoder_param_names(C)); they are no parameters, so no optimizer moves them.
    Out of scope: batch statistics, Dropout2d in training mode, the encoder's backward.

    scope='decoder': all 36 tensors of decoder_param_names(C) are parameters (proj_L4_C and pspMod as well: what the reference's
    optimizer moves outside the encoder), views of one flat buffer in that order; the backward is tmpnn_espnet_dec_bwd (48
    launches, the first 13 the tail's with the tail's bits), tap_grads holds all four taps ('out_l3' [T, 128, H/8, W/8], 'out_l4'
    [T, 256, H/16, W/16]), and everything else said here holds unchanged.  An unknown scope raises ValueError.

        net(images, tap_grads=True)                     after the backward, net.tap_grads = {'out_l1': [T, 32, H/2, W/2],
                                                        'out_l2': [T, 64, H/4, W/4], 'out_l3': None, 'out_l4': None}: the gradients at
                                                        the encoder taps the scope reaches (buffers of the shape, overwritten by the
                                                        next such backward; scope='decoder' fills all four).  tap_grads=False skips those channels' launches' work.
        net.state_dict()                                the current tensors under the reference's names, frozen ones included:
                                                        loads with strict=True into the reference module and into EspEmbedNet
        net.snapshot(centres=False)                     an EspEmbedNet of the current weights (centres=True for validation)

    The weight arena follows the parameters: when their version counter has moved (an optimizer step, any in-place write), the next
    forward rewrites the trained layers' segments in one launch on the device (tmpnn_espnet_refold: float64, rounded once, the bits
    of pack_arena); a write that autograd cannot see (`p.data`) needs net.refold().  Workspaces are allocated at the first call of a
    (T, H, W); then a step allocates only its result (and, outside the in-place convention, the flat gradient).  The backward reads
    what the forward left in the workspace of its shape: one backward per forward, before the next forward of that shape (it raises
    otherwise).  Sums run in a fixed order without atomics: equal inputs give equal bits."""

    inplace_param_grads = False          # GradBucket(net) sets it; the backward recognises the bucket by its addresses anyway

    def __init__(self, sd, device='cuda:0', scope: str = 'tail'):
        super().__init__()
        self.scope = _check_scope(scope)
        self._ep = {'tail': ('tmpnn_espnet_train_ws_bytes', 'tmpnn_espnet_train_bwd_ws_bytes', 'tmpnn_espnet_refold',
                             'tmpnn_espnet_train_fwd', 'tmpnn_espnet_train_bwd', 'tmpnn_espnet_train_param_floats'),
                    'decoder': ('tmpnn_espnet_dec_ws_bytes', 'tmpnn_espnet_dec_bwd_ws_bytes', 'tmpnn_espnet_dec_refold',
                                'tmpnn_espnet_dec_fwd', 'tmpnn_espnet_dec_bwd', 'tmpnn_espnet_dec_param_floats')}[scope]
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError(f'EspTrainNet on {dev}: trackmpnn_amd runs on the MI355X HIP kernels only (no CPU path): pass a cuda '
                               'device')
        self.C = C = check_state_dict(sd)
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        self._names = trained_param_names(C, scope)
        table = train_table(C, scope)
        spec = espnet_spec(C)
        if len(table) != len(self._names) or any(int(n) != int(np.prod(spec[k])) for (_, n, _), k in zip(table, self._names)):
            raise RuntimeError('espnet: the library trains other tensors than trained_param_names lists')
        self._frozen = OrderedDict((k, v.detach().clone()) for k, v in sd.items() if k not in self._names)
        self._keys = list(sd.keys())
        n = int(_lib.fn(self._ep[5])(C))
        host = np.zeros(n, np.float32)
        for (o, cnt, _), k in zip(table, self._names):
            host[o:o + cnt] = sd[k].detach().cpu().numpy().astype(np.float32).ravel()
        self._flat = torch.from_numpy(host).to(dev)
        self._params: 'OrderedDict[str, torch.nn.Parameter]' = OrderedDict()
        for (o, cnt, _), k in zip(table, self._names):
            self._params[k] = torch.nn.Parameter(self._flat[o:o + cnt].view(spec[k]))
        stats = [sd[f'{p}.{k}'].detach().cpu().numpy().astype(np.float32) for p in trained_norm_names(C, scope)
                 for k in ('running_mean', 'running_var')]
        self._stats = torch.from_numpy(np.concatenate(stats)).to(dev)
        self._arena = torch.from_numpy(pack_arena(sd, C)).to(dev)
        self._folded = self._version()
        self._ws: Dict[Tuple[int, int, int], torch.Tensor] = {}
        self._bws: Dict[Tuple[int, int, int], torch.Tensor] = {}
        self._taps: Dict[Tuple[int, int, int], Tuple[torch.Tensor, ...]] = {}
        self._gen: Dict[Tuple[int, int, int], int] = {}
        self._out = None
        self.tap_grads: Optional[Dict[str, Optional[torch.Tensor]]] = None

    @classmethod
    def from_state_dict(cls, sd, device='cuda:0', scope: str = 'tail') -> 'EspTrainNet':
        return cls(sd, device, scope)

    # ---- torch.nn.Module's surface --------------------------------------------------------------------------------------------
    def named_parameters(self, prefix: str = '', recurse: bool = True, remove_duplicate: bool = True):
        for k, p in self._params.items():
            yield (prefix + '.' if prefix else '') + k, p

    def state_dict(self, *args, **kwargs):
        """The current tensors under the reference's names (copies), the frozen ones and num_batches_tracked as they were given."""
        if args or kwargs:
            raise TypeError('EspTrainNet.state_dict takes no arguments')
        return OrderedDict((k, self._params[k].detach().clone() if k in self._params else self._frozen[k]) for k in self._keys)

    def load_state_dict(self, *args, **kwargs):
        raise NotImplementedError('EspTrainNet: build a new net with EspTrainNet.from_state_dict(sd)')

    def _apply(self, fn, recurse=True):
        raise NotImplementedError('EspTrainNet lives on the device it was built for (no .to / .cuda / .float)')

    def snapshot(self, centres: bool = False) -> EspEmbedNet:
        """An eval-mode EspEmbedNet of the current weights (it packs its own arena: a copy, not a view)."""
        return EspEmbedNet.from_state_dict(self.state_dict(), self.device, centres)

    # ---- the device side ------------------------------------------------------------------------------------------------------
    def _version(self) -> int:
        return self._flat._version                  # the parameters are views of the flat buffer: one counter for all

    def refold(self) -> None:
        """Rewrite the trained layers' arena segments from the parameters (one launch, no host copy)."""
        _lib.call(self._ep[2], self._arena.data_ptr(), self.C, self._flat.data_ptr(), self._stats.data_ptr(),
                  _lib.raw_stream(self.device))
        self._folded = self._version()

    def _sized(self, cache, fn_name, key):
        buf = cache.get(key)
        if buf is None:
            nbytes = int(_lib.fn(fn_name)(*key, self.C))
            if nbytes == 0:
                raise ValueError(f'EspTrainNet: a batch of {key[0]} x {key[1]} x {key[2]} with C={self.C} is too large for one call '
                                 '(T <= 65535, max(C, 160) H W < 2^31)')
            buf = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return buf

    def _forward(self, images, out):
        key = EspEmbedNet._check_images(self, images)
        T, H, W = key
        ws = self._sized(self._ws, self._ep[0], key)
        if self._version() != self._folded:
            self.refold()
        if out is None:
            out = torch.empty((T, self.C, H, W), dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
              or tuple(out.shape) != (T, self.C, H, W) or not out.is_contiguous()):
            raise ValueError(f'EspTrainNet: out [{T}, {self.C}, {H}, {W}] float32 contiguous on {self.device} expected')
        _lib.call(self._ep[3], self._arena.data_ptr(), self.C, images.data_ptr(), T, H, W, ws.data_ptr(), ws.numel(),
                  out.data_ptr(), _lib.raw_stream(self.device))
        gen = self._gen.get(key, 0) + 1
        self._gen[key] = gen
        self._out = out
        return key, gen

    def forward(self, images, tap_grads: bool = False, out: Optional[torch.Tensor] = None):
        if not torch.is_grad_enabled():
            self._forward(images, out)
            maps, self._out = self._out, None
            return maps
        if out is not None:
            raise ValueError('EspTrainNet: out is taken under torch.no_grad() only (a map with a grad_fn is the call\'s own)')
        maps = _EspTrainFn.apply(self, images, tap_grads, out, *self._params.values())
        self._out = None
        return maps

    def _backward(self, key, gen, d_maps, taps: bool):
        if self._gen.get(key) != gen:
            raise RuntimeError('EspTrainNet: the net ran forward again on this shape before the backward of the earlier call; its '
                               'saved state is overwritten (one backward per forward, before the next forward of the shape)')
        if self._version() != self._folded:
            raise RuntimeError('EspTrainNet: the parameters changed between the forward and its backward')
        T, H, W = key
        d = d_maps.detach()
        if d.dtype != torch.float32 or not d.is_contiguous():
            d = d.to(torch.float32).contiguous()
        ws = self._ws[key]
        bws = self._sized(self._bws, self._ep[1], key)
        params = list(self._params.values())
        g0 = params[0].grad
        inplace = g0 is not None
        if inplace:
            at = g0.data_ptr()
            for p in params:
                g = p.grad
                if (g is None or g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous()
                        or g.shape != p.shape or g.data_ptr() != at):
                    inplace = False
                    break
                at += 4 * p.numel()
        flat = None
        if not inplace:
            flat = torch.zeros_like(self._flat)
        shapes = ((32, 2), (64, 4), (_PSP, 8), (2 * _PSP, 16))[:4 if self.scope == 'decoder' else 2]
        tg = (None,) * len(shapes)
        if taps:
            tg = self._taps.get(key)
            if tg is None:
                tg = self._taps[key] = tuple(torch.empty((T, c, H // f, W // f), dtype=torch.float32, device=self.device)
                                             for c, f in shapes)
        _lib.call(self._ep[4], self._arena.data_ptr(), self.C, self._flat.data_ptr(), self._stats.data_ptr(), T, H, W,
                  ws.data_ptr(), ws.numel(), d.data_ptr(), bws.data_ptr(), bws.numel(),
                  g0.data_ptr() if inplace else flat.data_ptr(), *(g.data_ptr() if taps else None for g in tg),
                  _lib.raw_stream(self.device))
        self._gen[key] = gen + 1                      # the backward turned d(act) into d(pre-activation) in place: once only
        if taps:
            self.tap_grads = dict(zip(('out_l1', 'out_l2', 'out_l3', 'out_l4'), tg + (None,) * (4 - len(tg))))
        if inplace:
            return [None] * len(params)
        out, o = [], 0
        for p in params:
            out.append(flat[o:o + p.numel()].view_as(p))
            o += p.numel()
        return out


def train_table(C: int, scope: str = 'tail'):
    """[(offset in the flat parameter buffer, element count, offset of the arena segment the tensor is folded into)] of the
    tensors EspTrainNet trains, in the order of trained_param_names(C, scope) (tmpnn_espnet_train_table / tmpnn_espnet_dec_table;
    needs no GPU)."""
    f = _lib.fn('tmpnn_espnet_train_table' if _check_scope(scope) == 'tail' else 'tmpnn_espnet_dec_table')
    n = int(f(int(C), None, 0))
    if n < 0:
        raise ValueError(f'espnet: {_lib.last_error()}')
    rows = np.zeros((n, 3), np.int64)
    if int(f(int(C), rows.ctypes.data, n)) != n:
        raise RuntimeError(f'espnet train_table: {_lib.last_error()}')
    return [tuple(int(v) for v in r) for r in rows]
