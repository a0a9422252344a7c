"""Torch restatement of the reference's DUNet (segmentron/models/dunet.py) for the tests and
tools/dunet_bench.py: OracleNet's ResNet (`_resnet`), `bn`, `conv` and `fcn_head` plus the DUNet
head and DUpsampling in torch.nn.functional — no kernel of this repository.  Runs in float32 /
float64 on the CPU and, for the bench tool, on the device through torch's own kernels.  Pinned
against the reference itself by tests/golden/dunet_*.npz (tools/gen_golden_dunet.py,
tests/test_dunet.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

B, H, W = 2, 64, 96
H_ODD, W_ODD = 65, 97  # the output-shape fixture
AUX_WEIGHT = 0.4
SCALE = 8


def state(keys_and_shapes):
    """The fixtures' weights: oracle.synth, seed 0, conditioned (few ReLUs at ties)."""
    return synth.synth_state_dict(keys_and_shapes, seed=0, conditioned=True)


def _up(x, hw):
    if tuple(x.shape[2:]) == tuple(hw):
        return x
    return TF.interpolate(x, size=tuple(hw), mode="bilinear", align_corners=True)


def _cbr(net, x, p, padding=0):
    """nn.Sequential(conv, norm, ReLU) with keys p.0 / p.1."""
    return TF.relu(net.bn(net.conv(x, p + ".0", 1, padding), p + ".1"))


def dupsample(lo, s=SCALE):
    """DUpsampling.forward behind conv_w (dunet.py:100-117) as one permute:
    out[n, k, h*s + a, w*s + b] = lo[n, (a*s + b)*C + k, h, w]."""
    n, c, h, w = lo.shape
    k = c // (s * s)
    return lo.view(n, s, s, k, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, k, h * s, w * s)


def forward(net, x):
    """DUNet.forward (dunet.py:33-44) -> tuple of full-resolution logits."""
    _, c2, c3, c4 = torch_ref._resnet(net, x)
    size = c4.shape[2:]
    f2 = _cbr(net, _up(c2, size), "head.fuse.conv2")
    f3 = _cbr(net, _up(c3, size), "head.fuse.conv3")
    y = torch.cat([c4, f3, f2], 1)
    y = TF.relu(net.bn(net.conv(y, "head.block.0", 1, 1), "head.block.1"))
    y = TF.relu(net.bn(net.conv(y, "head.block.3", 1, 1), "head.block.4"))
    outs = [dupsample(net.conv(y, "dupsample.conv_w"))]
    if net.aux:
        a = net.fcn_head(c3, "auxlayer")
        outs.append(dupsample(net.conv(a, "aux_dupsample.conv_w")))
    return tuple(outs)


def evaluate(sd, x, aux=True, output_stride=8):
    net = torch_ref.OracleNet({k: v.clone() for k, v in sd.items()}, training=False,
                              output_stride=output_stride, aux=aux)
    with torch.no_grad():
        return forward(net, x)


def train(sd, x, y, dtype=torch.float32, aux=True, device=None, autocast=False):
    """One training forward + MixSoftmaxCrossEntropyLoss (aux weight 0.4) + backward, dropout 0 ->
    (loss, outputs, gradients by key, state after the step: running statistics and counters).
    autocast: float32 parameters under torch.autocast(bfloat16) — what mixed precision costs the
    reference itself on this fixture (the yardstick of the bf16 bars)."""
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    if device is not None:
        s = {k: v.to(device) for k, v in s.items()}
        x, y = x.to(device), y.to(device)
    s = torch_ref.clone_state(s, requires_grad=True)
    net = torch_ref.OracleNet(s, training=True, drop_p=0.0, output_stride=8, aux=aux)
    with torch.autocast(x.device.type, dtype=torch.bfloat16, enabled=autocast):
        outs = forward(net, x.to(dtype))
        loss = torch_ref.mix_softmax_ce(outs, y, AUX_WEIGHT, -1) if aux else \
            TF.cross_entropy(outs[0], y, ignore_index=-1)
    loss.backward()
    grads = {k: v.grad for k, v in s.items() if v.grad is not None}
    return loss.item(), tuple(o.detach() for o in outs), grads, s
