"""Torch restatement of the reference's FPENet (segmentron/models/fpenet.py) for the tests and
tools/fpenet_bench.py: OracleNet's `bn` and `conv` plus the FPE block and the MEU module in
torch.nn.functional — no kernel of this repository.  Runs in float32 / float64 on the CPU and, for
the bench tool, on the device through torch's own kernels.  Pinned against the reference itself by
tests/golden/fpenet_*.npz (tools/gen_golden_fpenet.py, tests/test_fpenet.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

B, H, W = 2, 64, 96            # evaluation and small-train fixtures: 8 x 12 maps at 1/8 (192 rows),
#                                at dilation 8 every side tap along H lies outside
H_ODD, W_ODD = 65, 97          # second evaluation size: the output is 66 x 98
TB, TH, TW = 4, 128, 192       # training fixture: 6144 rows per BatchNorm at 1/4 (the plain path),
#                                1536 at 1/8 (the few-sample path)
# Image / target seed of the training fixture: the FIRST seed whose float64 run keeps every ReLU
# input at least RELU_MARGIN (relative to the magnitudes of the terms that form it) away from the
# kink, so that the ReLU masks are decidable in float32 (see tests/_lednet_oracle.py);
# tools/gen_golden_fpenet.py repeats the scan and asserts that it is this one.
TRAIN_SEED = 1
RELU_MARGIN = 16 * 2.0 ** -24
DILATION = (1, 2, 4, 8)
# (prefix, stride, has a down-sampling shortcut) of the 13 FPE blocks (fpenet.py:35-40, 62-79)
BLOCKS = ([("layer1.0", 1, False)]
          + [("layer2.%d" % i, 2 if i == 0 else 1, i == 0) for i in range(3)]
          + [("layer3.%d" % i, 2 if i == 0 else 1, i == 0) for i in range(9)])


def state(keys_and_shapes):
    """The fixtures' weights: oracle.synth, seed 0, conditioned."""
    return synth.synth_state_dict(list(keys_and_shapes), seed=0, conditioned=True)


def _relu(z, scale):
    return TF.relu(z)


def _bn_relu(net, t, prefix, relu):
    z = net.bn(t, prefix)
    b = net.sd[prefix + ".bias"].view(1, -1, 1, 1)
    return relu(z, (z - b).abs() + b.abs())


def fpe_block(net, x, p, stride, down, relu=_relu):
    """FPEBlock.forward (fpenet.py:173-201)."""
    out = _bn_relu(net, net.conv(x, p + ".conv1", stride), p + ".bn1", relu)
    n = out.shape[1] // 4
    xs = torch.chunk(out, 4, 1)
    ys = []
    for s, d in enumerate(DILATION):
        t = xs[s] if s == 0 else xs[s] + ys[-1]
        t = net.conv(t, "%s.conv2.%d" % (p, s), 1, d, d, groups=n)
        ys.append(_bn_relu(net, t, "%s.bn2.%d" % (p, s), relu))
    out = net.bn(net.conv(torch.cat(ys, 1), p + ".conv3"), p + ".bn3")
    if down:
        x = net.bn(net.conv(x, p + ".downsample.0", stride), p + ".downsample.1")
    return relu(out + x, out.abs() + x.abs())


def meu(net, high, low, p, relu=_relu):
    """MEUModule.forward (fpenet.py:222-247)."""
    low = net.bn(net.conv(low, p + ".conv1x1_low"), p + ".bn_low")
    sa = torch.sigmoid(net.conv(low.mean(1, keepdim=True), p + ".sa_conv"))
    high = net.bn(net.conv(high, p + ".conv1x1_high"), p + ".bn_high")
    pooled = high.mean((2, 3), keepdim=True)
    z = net.conv(pooled, p + ".ca_conv")
    ca = torch.sigmoid(relu(z, TF.conv2d(pooled.abs(), net.sd[p + ".ca_conv.weight"].abs())))
    up = TF.interpolate(high, size=low.shape[2:], mode="bilinear", align_corners=True)
    return ca * low + sa * up


def forward(net, x, relu=_relu):
    """FPENet.forward (fpenet.py:81-118) -> list of one map of 2*ceil(H/2) x 2*ceil(W/2)."""
    x = _bn_relu(net, net.conv(x, "conv1", 2, 1), "bn1", relu)
    outs = {}
    for p, stride, down in BLOCKS:
        x = fpe_block(net, x, p, stride, down, relu)
        outs[p] = x
        if p == "layer2.2":
            x = outs["layer2.2"] = outs["layer2.0"] + x
        elif p == "layer3.8":
            x = outs["layer3.8"] = outs["layer3.0"] + x
    x2 = meu(net, outs["layer3.8"], outs["layer2.2"], "meu1", relu)
    x1 = meu(net, x2, outs["layer1.0"], "meu2", relu)
    x = net.conv(x1, "project_layer")
    return [TF.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)]


def min_relu_margin(sd, x):
    """Smallest |z| / scale over every ReLU input z of one float64 training-mode forward pass:
    the BatchNorm + ReLU inputs (scale |z - beta| + |beta|), the block tails relu(bn3 + identity)
    (scale |bn3| + |identity|) and the ReLU in the MEU's channel-attention path (scale
    |W| * |pooled|)."""
    margins = []

    def relu(z, scale):
        margins.append((z.abs() / scale).min().item())
        return TF.relu(z)
    s = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        forward(torch_ref.OracleNet(s, training=True, drop_p=0.0), x.double(), relu)
    return min(margins)


def evaluate(sd, x):
    net = torch_ref.OracleNet({k: v.clone() for k, v in sd.items()}, training=False)
    with torch.no_grad():
        return forward(net, x)


def train(sd, x, y, dtype=torch.float32, device=None, autocast=False):
    """One training forward + cross-entropy (ignore_index -1; MixSoftmaxCrossEntropyLoss with one
    output) + backward -> (loss, outputs, gradients by key, state after the step: running
    statistics and counters).  autocast: float32 parameters under torch.autocast(bfloat16) — what
    mixed precision costs the reference itself on this fixture."""
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    if device is not None:
        s = {k: v.to(device) for k, v in s.items()}
        x, y = x.to(device), y.to(device)
    s = torch_ref.clone_state(s, requires_grad=True)
    net = torch_ref.OracleNet(s, training=True, drop_p=0.0)
    with torch.autocast(x.device.type, dtype=torch.bfloat16, enabled=autocast):
        outs = forward(net, x.to(dtype))
        loss = TF.cross_entropy(outs[0], y, ignore_index=-1)
    loss.backward()
    grads = {k: v.grad for k, v in s.items() if v.grad is not None}
    return loss.item(), tuple(o.detach() for o in outs), grads, s
