"""Torch restatement of the reference's ESPNetV2 on EESPNet (segmentron/models/espnetv2.py,
segmentron/models/backbones/eespnet.py, EESP in segmentron/modules/module.py) for the tests and
tools/espnetv2_bench.py: OracleNet's `bn` and `conv` plus PReLU, the EESP unit, the DownSampler and
the decoder in torch.nn.functional — no kernel of this repository.  Runs in float32 / float64 on
the CPU and, for the bench tool, on the device through torch's own kernels.  Pinned against the
reference itself by tests/golden/espnetv2_*.npz (tools/gen_golden_espnetv2.py,
tests/test_espnetv2.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

B, H, W = 2, 64, 96            # evaluation and small-train fixtures
H2, W2 = 48, 80                # second evaluation shape (one image); odd sizes are not valid
TB, TH, TW = 4, 128, 192       # training fixture: the 1/8 BatchNorms see 1536 rows, the 1/16 384
# Image / target seed of the training fixture.  PReLU has a kink at zero as ReLU has: a float32 run
# cannot tell the sign of an input that lies within a few float32 roundings of zero, and its mask
# decides a (1 - alpha) share of that element's gradient.  tools/gen_golden_espnetv2.py takes the
# FIRST seed whose float64 reference run keeps every PReLU input at least 16 * 2^-24 away from
# zero, relative to the magnitudes added to form it (|xhat * gamma| + |beta| of each BatchNorm
# operand, |x| of a plain one) — a property of the reference alone — and asserts it is this one.
TRAIN_SEED = 2
PRELU_MARGIN = 16 * 2.0 ** -24
K = 4
# r_lim of the EESP units the segmentation forward reaches (eespnet.py:52-93, espnetv2.py:23)
R_LIM = {"encoder.level2_0.eesp": 13, "encoder.level3_0.eesp": 11, "encoder.level3": 9,
         "encoder.level4_0.eesp": 9, "encoder.level4": 7, "pspMod.0": 7}
PRELU_KEYS = ("prelu.weight", "module_act.weight", ".act.weight")
# modules of the state_dict the segmentation forward never runs — level5*, fc, and the module_act
# of a DownSampler's EESP unit, which returns before it (module.py:201-202): no gradient
UNUSED = ("encoder.level5_0.", "encoder.level5.", "encoder.fc.")


def unused(key):
    return key.startswith(UNUSED) or key.endswith("_0.eesp.module_act.weight")


def state(keys_and_shapes):
    """The fixtures' weights: oracle.synth, seed 0, conditioned; the PReLU slopes (which synth
    would draw like BatchNorm gammas) uniform in [0.05, 0.45] instead, keyed by name."""
    keys_and_shapes = list(keys_and_shapes)
    sd = synth.synth_state_dict(keys_and_shapes, seed=0, conditioned=True)
    for k, s in keys_and_shapes:
        if k.endswith(PRELU_KEYS):
            sd[k] = 0.05 + 0.4 * torch.rand(tuple(s), generator=synth._gen(0, k))
    return sd


def dilations(r_lim, k=K):
    """EESP.__init__ (module.py:176-186): kernel sizes 3, 5, .. capped by r_lim, sorted."""
    sizes = sorted((3 + 2 * i) if (3 + 2 * i) <= r_lim else 3 for i in range(k))
    return [(s - 1) // 2 for s in sizes]


def _r_lim(p):
    for key, r in R_LIM.items():
        if p == key or p.startswith(key + "."):
            return r
    raise KeyError(p)


def _bn(net, t, p):
    """-> (BatchNorm output, the magnitudes added to form it)"""
    z = net.bn(t, p)
    b = net.sd[p + ".bias"].view(1, -1, 1, 1)
    return z, (z - b).abs() + b.abs()


def _prelu(z, mag, alpha, margins):
    if margins is not None:
        margins.append((z.detach().abs() / mag.detach().clamp_min(1e-300)).min().item())
    return TF.prelu(z, alpha)


def _cbp(net, x, p, stride=1, padding=0, groups=1, margins=None):
    z, mag = _bn(net, net.conv(x, p + ".conv", stride, padding, 1, groups), p + ".bn")
    return _prelu(z, mag, net.sd[p + ".prelu.weight"], margins)


def eesp(net, x, p, stride=1, down_avg=False, margins=None):
    """EESP.forward (module.py:192-207); down_avg: returns (bn(expanded), its magnitudes)."""
    sd = net.sd
    o1 = _cbp(net, x, p + ".proj_1x1", groups=K, margins=margins)
    n = o1.shape[1]
    outs = []
    for k, d in enumerate(dilations(_r_lim(p))):
        o = net.conv(o1, p + ".spp_dw.%d" % k, stride, d, d, n)
        outs.append(o if not outs else o + outs[-1])
    z, mag = _bn(net, torch.cat(outs, 1), p + ".br_after_cat.bn")
    cat = _prelu(z, mag, sd[p + ".br_after_cat.prelu.weight"], margins)
    e, emag = _bn(net, net.conv(cat, p + ".conv_1x1_exp.conv", 1, 0, 1, K), p + ".conv_1x1_exp.bn")
    if stride == 2 and down_avg:
        return e, emag
    if e.shape == x.shape:
        e, emag = e + x, emag + x.abs()
    return _prelu(e, emag, sd[p + ".module_act.weight"], margins)


def down_sampler(net, x, x2, p, margins=None):
    """DownSampler.forward (eespnet.py:30-43) with input reinforcement."""
    avg = TF.avg_pool2d(x, 3, 2, 1)
    e, emag = eesp(net, x, p + ".eesp", 2, True, margins)
    out, mag = torch.cat([avg, e], 1), torch.cat([avg.abs(), emag], 1)
    w1 = avg.shape[2]
    while True:
        x2 = TF.avg_pool2d(x2, 3, 2, 1)
        if x2.shape[2] == w1:
            break
    r = _cbp(net, x2, p + ".inp_reinf.0", 1, 1, margins=margins)
    r, rmag = _bn(net, net.conv(r, p + ".inp_reinf.1.conv"), p + ".inp_reinf.1.bn")
    return _prelu(out + r, mag + rmag, net.sd[p + ".act.weight"], margins)


def n_units(sd, level):
    return len({k.split(".")[2] for k in sd if k.startswith("encoder.%s." % level)})


def encoder(net, x, margins=None):
    """EESPNet.forward with seg=True (eespnet.py:116-133)."""
    p = "encoder"
    out_l1 = _cbp(net, x, p + ".level1", 2, 1, margins=margins)
    out_l2 = down_sampler(net, out_l1, x, p + ".level2_0", margins)
    out_l3 = down_sampler(net, out_l2, x, p + ".level3_0", margins)
    for i in range(n_units(net.sd, "level3")):
        out_l3 = eesp(net, out_l3, "%s.level3.%d" % (p, i), margins=margins)
    out_l4 = down_sampler(net, out_l3, x, p + ".level4_0", margins)
    for i in range(n_units(net.sd, "level4")):
        out_l4 = eesp(net, out_l4, "%s.level4.%d" % (p, i), margins=margins)
    return out_l1, out_l2, out_l3, out_l4


def psp(net, x, p, margins=None):
    """_PSPModule.forward (espnetv2.py:70-75)."""
    size = x.shape[2:]
    feats = [x]
    c = x.shape[1]
    for i in range(4):
        x = TF.avg_pool2d(x, 3, 2, 1)
        s = net.conv(x, "%s.stages.%d" % (p, i), 1, 1, 1, c)
        feats.append(TF.interpolate(s, size, mode="bilinear", align_corners=True))
    return _cbp(net, torch.cat(feats, 1), p + ".project", margins=margins)


def forward(net, x, aux=False, margins=None):
    """ESPNetV2.forward (espnetv2.py:36-59) -> tuple of full-resolution logits (dropout 0)."""
    sd = net.sd
    size = x.shape[2:]
    up2 = lambda t: TF.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)
    out_l1, out_l2, out_l3, out_l4 = encoder(net, x, margins)
    out_l4_proj = _cbp(net, out_l4, "proj_L4_C", margins=margins)
    merged = eesp(net, torch.cat([out_l3, up2(out_l4_proj)], 1), "pspMod.0", margins=margins)
    merged = psp(net, merged, "pspMod.1", margins)
    bef_act = net.conv(merged, "project_l3.1")
    z, mag = _bn(net, bef_act, "act_l3.bn")
    proj_merge_l3 = _prelu(z, mag, sd["act_l3.prelu.weight"], margins)
    merge_l2 = _cbp(net, torch.cat([out_l2, up2(proj_merge_l3)], 1), "project_l2", margins=margins)
    merge_l1 = net.conv(torch.cat([out_l1, up2(merge_l2)], 1), "project_l1.1")
    outs = [up2(merge_l1)]
    if aux:
        outs.append(TF.interpolate(bef_act, size, mode="bilinear", align_corners=True))
    return tuple(outs)


def min_prelu_margin(sd, x):
    """Smallest |z| / (magnitudes added to form z) over every PReLU input z of one float64
    training-mode forward pass."""
    margins = []
    s = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        forward(torch_ref.OracleNet(s, training=True, drop_p=0.0), x.double(), margins=margins)
    return min(margins)


def evaluate(sd, x):
    net = torch_ref.OracleNet({k: v.clone() for k, v in sd.items()}, training=False)
    with torch.no_grad():
        return forward(net, x)


def train(sd, x, y, dtype=torch.float32, device=None, autocast=False, aux=False, aux_weight=0.4):
    """One training forward + cross-entropy (ignore_index -1; MixSoftmaxCrossEntropyLoss: with
    `aux` the second output's loss times aux_weight is added) + backward, dropout 0 -> (loss,
    outputs, gradients by key, state after the step: running statistics and counters).  autocast:
    float32 parameters under torch.autocast(bfloat16) — what mixed precision costs the reference
    itself on this fixture."""
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    if device is not None:
        s = {k: v.to(device) for k, v in s.items()}
        x, y = x.to(device), y.to(device)
    s = torch_ref.clone_state(s, requires_grad=True)
    net = torch_ref.OracleNet(s, training=True, drop_p=0.0)
    with torch.autocast(x.device.type, dtype=torch.bfloat16, enabled=autocast):
        outs = forward(net, x.to(dtype), aux=aux)
        loss = TF.cross_entropy(outs[0], y, ignore_index=-1)
        if aux:
            loss = loss + aux_weight * TF.cross_entropy(outs[1], y, ignore_index=-1)
    loss.backward()
    grads = {k: v.grad for k, v in s.items() if v.grad is not None}
    return loss.item(), tuple(o.detach() for o in outs), grads, s
