"""Torch restatement of the reference's ContextNet (segmentron/models/contextnet.py) for the tests
and tools/contextnet_bench.py: OracleNet's `bn` and `conv` plus the depthwise-separable blocks, the
t = 6 linear bottlenecks and the feature fusion in torch.nn.functional — no kernel of this
repository.  Runs in float32 / float64 on the CPU and, for the bench tool, on the device through
torch's own kernels.  Pinned against the reference itself by tests/golden/contextnet_*.npz
(tools/gen_golden_contextnet.py, tests/test_contextnet.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

B, H, W = 2, 64, 96            # evaluation, small-train and loop fixtures: hi 8 x 12, lo 2 x 3
H_ODD, W_ODD = 70, 97          # second evaluation size: hi 9 x 12, x_low 17 x 24, lo 2 x 3
H_ONE, W_ONE = 32, 32          # the low map is 1 x 1: the fusion's resize has scale 0
TB, TH, TW = 4, 112, 160       # training fixture: hi 14 x 20 (1120 rows per BatchNorm: the plain
#                                path), x_low 28 x 40, bottleneck3 onwards 7 x 10 and 4 x 5 (280 /
#                                80 rows: the few-sample path); the fusion resizes 4 x 5 to 14 x 20,
#                                ratios 3/13 and 4/19
FB, FH, FW = 2, 576, 584       # the fused-loss tier test: logits at head stride 8 (72 x 73)
# Image / target seed of the training fixture: the FIRST seed whose float64 run keeps every ReLU
# input at least RELU_MARGIN, relative to the magnitudes of the terms that form it, away from the
# kink (see tests/_lednet_oracle.py).  tools/gen_golden_contextnet.py repeats the scan and asserts
# that it is this one.
TRAIN_SEED = 1
RELU_MARGIN = 16 * 2.0 ** -24
# Deep_net (contextnet.py:130-162): (name, in, out, t, blocks, stride of the first block)
BOTTLENECKS = (("bottleneck1", 32, 32, 1, 1, 1), ("bottleneck2", 32, 32, 6, 1, 1),
               ("bottleneck3", 32, 48, 6, 3, 2), ("bottleneck4", 48, 64, 6, 3, 2),
               ("bottleneck5", 64, 96, 6, 2, 1), ("bottleneck6", 96, 128, 6, 2, 1))


def state(keys_and_shapes):
    """The fixtures' weights: oracle.synth, seed 0, conditioned."""
    return synth.synth_state_dict(list(keys_and_shapes), seed=0, conditioned=True)


def _relu(z, scale):
    return TF.relu(z)


def _bn(net, t, prefix):
    """-> (bn(t), the magnitude a ReLU behind it is decided against)."""
    z = net.bn(t, prefix)
    b = net.sd[prefix + ".bias"].view(1, -1, 1, 1)
    return z, (z - b).abs() + b.abs()


def _bn_relu(net, t, prefix, relu):
    return relu(*_bn(net, t, prefix))


def custom_conv(net, x, p, relu, stride=1):
    """Custom_Conv (contextnet.py:54-64): conv (padding 0), BN, ReLU."""
    return _bn_relu(net, net.conv(x, p + ".conv.0", stride, 0), p + ".conv.1", relu)


def depth_conv(net, x, p, relu, stride=1):
    """DepthConv (contextnet.py:83-93): depthwise 3x3, BN, ReLU."""
    return _bn_relu(net, net.conv(x, p + ".conv.0", stride, 1, 1, x.shape[1]), p + ".conv.1", relu)


def depth_sep_conv(net, x, p, relu, stride=1):
    """DepthSepConv (contextnet.py:67-80)."""
    x = depth_conv(net, x, p, relu, stride)
    return _bn_relu(net, net.conv(x, p + ".conv.3"), p + ".conv.4", relu)


def linear_bottleneck(net, x, p, relu, stride, shortcut):
    """LinearBottleneck (contextnet.py:96-111): no ReLU behind the last BatchNorm."""
    out = custom_conv(net, x, p + ".block.0", relu)
    out = depth_conv(net, out, p + ".block.1", relu, stride)
    out = net.bn(net.conv(out, p + ".block.2"), p + ".block.3")
    return x + out if shortcut else out


def deep_net(net, x, relu, p="context_feature_extractor"):
    x = custom_conv(net, x, p + ".conv_", relu, 2)
    for name, cin, cout, t, blocks, stride in BOTTLENECKS:
        for i in range(blocks):
            s, ci = (stride, cin) if i == 0 else (1, cout)
            x = linear_bottleneck(net, x, "%s.%s.%d" % (p, name, i), relu, s, s == 1 and ci == cout)
    return x


def fusion(net, hi, lo, relu, p="feature_fusion"):
    """FeatureFusionModule.forward (contextnet.py:180-188)."""
    lo = TF.interpolate(lo, size=tuple(hi.shape[2:]), mode="bilinear", align_corners=True)
    lo = depth_conv(net, lo, p + ".dwconv", relu)
    zl, sl = _bn(net, net.conv(lo, p + ".conv_lower_res.0"), p + ".conv_lower_res.1")
    zh, sh = _bn(net, net.conv(hi, p + ".conv_higher_res.0"), p + ".conv_higher_res.1")
    return relu(zh + zl, sh + sl)


def forward(net, x, relu=_relu):
    """ContextNet.forward (contextnet.py:29-51) -> list of full-resolution logits (+ aux)."""
    size = tuple(x.shape[2:])
    p = "spatial_detail"
    hi = custom_conv(net, x, p + ".conv", relu, 2)
    hi = depth_sep_conv(net, hi, p + ".dsconv1", relu, 2)
    hi = depth_sep_conv(net, hi, p + ".dsconv2", relu, 2)
    hi = depth_sep_conv(net, hi, p + ".dsconv3", relu, 1)
    x_low = TF.interpolate(x, scale_factor=0.25, mode="bilinear", align_corners=True)
    y = fusion(net, hi, deep_net(net, x_low, relu), relu)
    y = depth_sep_conv(net, y, "classifier.dsconv1", relu)
    y = depth_sep_conv(net, y, "classifier.dsconv2", relu)
    y = net.conv(y, "classifier.conv.1")  # (nn.Dropout(0.1) in front: p = 0 in every fixture)
    outs = [TF.interpolate(y, size, mode="bilinear", align_corners=True)]
    if "auxlayer.0.weight" in net.sd:
        a = _bn_relu(net, net.conv(hi, "auxlayer.0", 1, 1), "auxlayer.1", relu)
        outs.append(TF.interpolate(net.conv(a, "auxlayer.4"), size, mode="bilinear",
                                   align_corners=True))
    return outs


def min_relu_margin(sd, x):
    """Smallest |z| / scale over every ReLU input z of one float64 training-mode forward pass:
    scale = |z - beta| + |beta| behind a BatchNorm, the sum of the two branches' scales at the
    fusion's ReLU."""
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


def train(sd, x, y, dtype=torch.float32, device=None, autocast=False, aux_weight=0.4):
    """One training forward + cross-entropy (ignore_index -1; MixSoftmaxCrossEntropyLoss, the aux
    output weighted by aux_weight where the state has the aux head) + backward -> (loss, outputs,
    gradients by key, state after the step: running statistics and counters).  autocast: float32
    parameters under torch.autocast(bfloat16) — what mixed precision costs the reference itself on
    this fixture."""
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    if device is not None:
        s = {k: v.to(device) for k, v in s.items()}
        x, y = x.to(device), y.to(device)
    s = torch_ref.clone_state(s, requires_grad=True)
    net = torch_ref.OracleNet(s, training=True, drop_p=0.0)
    with torch.autocast(x.device.type, dtype=torch.bfloat16, enabled=autocast):
        outs = forward(net, x.to(dtype))
        loss = TF.cross_entropy(outs[0], y, ignore_index=-1)
        for o in outs[1:]:
            loss = loss + aux_weight * TF.cross_entropy(o, y, ignore_index=-1)
    loss.backward()
    grads = {k: v.grad for k, v in s.items() if v.grad is not None}
    return loss.item(), tuple(o.detach() for o in outs), grads, s
