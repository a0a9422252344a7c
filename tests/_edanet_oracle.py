"""Torch restatement of the reference's EDANet (segmentron/models/edanet.py) for the tests and
tools/edanet_bench.py: OracleNet's `bn` and `conv` plus the down-sampler block and the dense
EDABlock in torch.nn.functional — no kernel of this repository.  Runs in float32 / float64 on the
CPU and, for the bench tool, on the device through torch's own kernels.  Pinned against the
reference itself by tests/golden/edanet_*.npz (tools/gen_golden_edanet.py, tests/test_edanet.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

B, H, W = 2, 64, 96            # evaluation and small-train fixtures
H2, W2 = 72, 104               # second evaluation size: divisible by 8, not by 16
TB, TH, TW = 4, 128, 192       # training fixture: 16 x 24 maps at 1/8 (1536 rows per BatchNorm);
#                                at dilation 16 every side tap along H lies outside
# Image / target seed of the training fixture: the FIRST seed whose float64 run keeps every
# BatchNorm + ReLU input at least RELU_MARGIN (relative to |xhat * gamma| + |beta|) away from the
# kink, so that the ReLU masks are decidable in float32 (see tests/_lednet_oracle.py);
# tools/gen_golden_edanet.py repeats the scan and asserts that it is this one.
TRAIN_SEED = 22
RELU_MARGIN = 16 * 2.0 ** -24
K_GROWTH = 40
# layers.0 .. layers.15 (edanet.py:22-37): ("down", cin, cout) or ("eda", cin, dilation)
LAYERS = ([("down", 3, 15), ("down", 15, 60)]
          + [("eda", 60 + K_GROWTH * i, d) for i, d in enumerate([1, 1, 1, 2, 2])]
          + [("down", 260, 130)]
          + [("eda", 130 + K_GROWTH * j, d) for j, d in enumerate([2, 2, 4, 4, 8, 8, 16, 16])])


def state(keys_and_shapes):
    """The fixtures' weights: oracle.synth, seed 0, conditioned."""
    return synth.synth_state_dict(list(keys_and_shapes), seed=0, conditioned=True)


def downsampler(net, x, p, cin, cout):
    """DownsamplerBlock.forward (edanet.py:90-97)."""
    y = net.conv(x, p + ".conv", 2, 1)
    if cin < cout:
        y = torch.cat([y, TF.max_pool2d(x, 2, 2)], 1)
    return TF.relu(net.bn(y, p + ".bn"))


def eda_block(net, x, p, d, drop=None):
    """EDABlock.forward (edanet.py:120-142).  drop: the Dropout2d multiplier [N, 40, 1, 1] of
    the 40 new channels (None: p = 0)."""
    y = TF.relu(net.bn(net.conv(x, p + ".conv1x1"), p + ".bn0"))
    y = net.conv(y, p + ".conv3x1_1", 1, (1, 0))
    y = TF.relu(net.bn(net.conv(y, p + ".conv1x3_1", 1, (0, 1)), p + ".bn1"))
    y = net.conv(y, p + ".conv3x1_2", 1, (d, 0), (d, 1))
    y = TF.relu(net.bn(net.conv(y, p + ".conv1x3_2", 1, (0, d), (1, d)), p + ".bn2"))
    if drop is not None:
        y = y * drop
    return torch.cat([y, x], 1)


def forward(net, x):
    """EDANet.forward (edanet.py:53-70) -> tuple of full-resolution logits."""
    size = x.shape[2:]
    for i, layer in enumerate(LAYERS):
        p = "layers.%d" % i
        if layer[0] == "down":
            x = downsampler(net, x, p, layer[1], layer[2])
        else:
            x = eda_block(net, x, p, layer[2])
    x = net.conv(x, "project_layer")
    return (TF.interpolate(x, size, mode="bilinear", align_corners=True),)


def min_relu_margin(sd, x):
    """Smallest |z| / (|z - beta| + |beta|) over every BatchNorm + ReLU input z of one float64
    training-mode forward pass (every BatchNorm of the model is followed by a ReLU)."""
    margins = []

    class Net(torch_ref.OracleNet):
        def bn(self, t, prefix):
            z = super().bn(t, prefix)
            b = self.sd[prefix + ".bias"].view(1, -1, 1, 1)
            margins.append((z.abs() / ((z - b).abs() + b.abs())).min().item())
            return z
    s = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        forward(Net(s, training=True, drop_p=0.0), x.double())
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
