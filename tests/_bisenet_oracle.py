"""Torch restatement of the reference's BiSeNet (segmentron/models/bisenet.py) for the tests and
tools/bisenet_bench.py: OracleNet's ResNet (`_resnet`), `conv_bn_relu`, `bn` and `conv` plus the
BiSeNet paths in torch.nn.functional — no kernel of this repository.  Runs in float32 / float64 on
the CPU and, for the bench tool, on the device through torch's own kernels.  Pinned against the
reference itself by tests/golden/bisenet_*.npz (tools/gen_golden_bisenet.py, tests/test_bisenet.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

B_EVAL, B_TRAIN, H, W = 2, 4, 65, 97
H32, W32 = 64, 96  # the OUTPUT_STRIDE 32 fixture
AUX_WEIGHT = 0.4


def state(keys_and_shapes):
    """The fixtures' weights: oracle.synth, seed 0, conditioned (few ReLUs at ties)."""
    return synth.synth_state_dict(keys_and_shapes, seed=0, conditioned=True)


def _up(x, hw):
    return TF.interpolate(x, size=tuple(hw), mode="bilinear", align_corners=True)


def _head(net, x, p):
    """_BiSeHead (bisenet.py:55-66)."""
    x = net.conv_bn_relu(x, p + ".block.0", 1, 1)
    x = TF.dropout(x, net.drop_p, net.training)
    return net.conv(x, p + ".block.2")


def _attention(net, x, p, layers):
    a = TF.adaptive_avg_pool2d(x, 1)
    for i in layers:
        a = net.conv_bn_relu(a, "%s.channel_attention.%d" % (p, i))
    return torch.sigmoid(a)


def forward(net, x):
    """BiSeNet.forward (bisenet.py:34-52) -> tuple of full-resolution logits."""
    size = x.shape[2:]
    sp = net.conv_bn_relu(x, "spatial_path.conv7x7", 2, 3)
    sp = net.conv_bn_relu(sp, "spatial_path.conv3x3_1", 2, 1)
    sp = net.conv_bn_relu(sp, "spatial_path.conv3x3_2", 2, 1)
    sp = net.conv_bn_relu(sp, "spatial_path.conv1x1")
    c1, c2, c3, c4 = torch_ref._resnet(net, x)
    # ContextPath.forward (bisenet.py:139-167)
    p = "context_path."
    g = TF.adaptive_avg_pool2d(c4, 1)
    g = TF.relu(net.bn(net.conv(g, p + "global_context.gap.1"), p + "global_context.gap.2"))
    last = _up(g, c4.shape[2:])
    blocks, ctx = [c4, c3, c2, c1], []
    for i in range(2):
        f = net.conv_bn_relu(blocks[i], p + "arms.%d.conv3x3" % i, 1, 1)
        f = f * _attention(net, f, p + "arms.%d" % i, (1,))
        f = f + last
        last = _up(f, blocks[i + 1].shape[2:])
        last = net.conv_bn_relu(last, p + "refines.%d" % i, 1, 1)
        ctx.append(last)
    # FeatureFusion (bisenet.py:170-186)
    out = net.conv_bn_relu(torch.cat([sp, ctx[-1]], 1), "ffm.conv1x1")
    out = out + out * _attention(net, out, "ffm", (1, 2))
    outs = [_up(_head(net, out, "head"), size)]
    if net.aux:
        outs.append(_up(_head(net, ctx[0], "auxlayer1"), size))
        outs.append(_up(_head(net, ctx[1], "auxlayer2"), size))
    return tuple(outs)


def evaluate(sd, x, output_stride=16, aux=True):
    net = torch_ref.OracleNet({k: v.clone() for k, v in sd.items()}, training=False,
                              output_stride=output_stride, aux=aux)
    with torch.no_grad():
        return forward(net, x)


def train(sd, x, y, dtype=torch.float32, output_stride=16, aux=True, device=None, autocast=False):
    """One training forward + MixSoftmaxCrossEntropyLoss (aux weight 0.4) + backward, dropout 0 ->
    (loss, outputs, gradients by key, state after the step: running statistics and counters).
    autocast: float32 parameters under torch.autocast(bfloat16) — what mixed precision costs the
    reference itself on this fixture (the yardstick of the bf16 bars)."""
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    if device is not None:
        s = {k: v.to(device) for k, v in s.items()}
        x, y = x.to(device), y.to(device)
    s = torch_ref.clone_state(s, requires_grad=True)
    net = torch_ref.OracleNet(s, training=True, drop_p=0.0, output_stride=output_stride, aux=aux)
    with torch.autocast(x.device.type, dtype=torch.bfloat16, enabled=autocast):
        outs = forward(net, x.to(dtype))
        loss = torch_ref.mix_softmax_ce(outs, y, AUX_WEIGHT, -1) if aux else \
            TF.cross_entropy(outs[0], y, ignore_index=-1)
    loss.backward()
    grads = {k: v.grad for k, v in s.items() if v.grad is not None}
    return loss.item(), tuple(o.detach() for o in outs), grads, s
