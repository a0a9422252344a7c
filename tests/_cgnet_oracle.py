"""Torch restatement of the reference's CGNet (segmentron/models/cgnet.py) for the tests and
tools/cgnet_bench.py: OracleNet's `bn` and `conv` plus PReLU, the context guided block and the
input injection in torch.nn.functional — no kernel of this repository.  Runs in float32 / float64
on the CPU and, for the bench tool, on the device through torch's own kernels.  Pinned against
the reference itself by tests/golden/cgnet_*.npz (tools/gen_golden_cgnet.py, tests/test_cgnet.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

B, H, W = 2, 64, 96            # evaluation and small-train fixtures
H_ODD, W_ODD = 65, 97          # the output-shape fixture
TB, TH, TW = 4, 128, 192       # training fixture: stage-2 / stage-3 BatchNorms see 6144 / 1536 rows
SMALL_BLOCKS = (2, 2)          # MODEL.CGNET.STAGE2_BLOCK_NUM / STAGE3_BLOCK_NUM of the small fixture
SMALL_OVERRIDES = ["MODEL.CGNET.STAGE2_BLOCK_NUM", "2", "MODEL.CGNET.STAGE3_BLOCK_NUM", "2"]


def state(keys_and_shapes):
    """The fixtures' weights: oracle.synth, seed 0, conditioned; the PReLU slopes (which synth
    would draw like BatchNorm gammas) uniform in [0.05, 0.45] instead, keyed by name."""
    keys_and_shapes = list(keys_and_shapes)
    sd = synth.synth_state_dict(keys_and_shapes, seed=0, conditioned=True)
    for k, s in keys_and_shapes:
        if k.endswith("prelu.weight"):
            sd[k] = 0.05 + 0.4 * torch.rand(tuple(s), generator=synth._gen(0, k))
    return sd


def _bn_prelu(net, x, p):
    return TF.prelu(net.bn(x, p + ".bn"), net.sd[p + ".prelu.weight"])


def _prelu(z, alpha, margins):
    if margins is not None:  # how far the nearest PReLU input is from the kink at 0
        margins.append(z.detach().abs().min().item())
    return TF.prelu(z, alpha)


def _cbp(net, x, p, stride=1, padding=0, margins=None):
    return _prelu(net.bn(net.conv(x, p + ".conv", stride, padding), p + ".bn"),
                  net.sd[p + ".prelu.weight"], margins)


def block(net, x, p, dilation, down, residual, margins=None):
    """ContextGuidedBlock.forward (cgnet.py:167-181).  margins: a list that receives min |z| of
    the block's two PReLU inputs."""
    sd = net.sd
    out = _cbp(net, x, p + ".conv", 2, 1, margins) if down else _cbp(net, x, p + ".conv",
                                                                     margins=margins)
    c = out.shape[1]
    loc = net.conv(out, p + ".f_loc.conv", 1, 1, 1, c)
    sur = net.conv(out, p + ".f_sur.conv", 1, dilation, dilation, c)
    joi = _prelu(net.bn(torch.cat([loc, sur], 1), p + ".bn"), sd[p + ".prelu.weight"], margins)
    if down:
        joi = net.conv(joi, p + ".reduce")
    g = joi.mean((2, 3))
    g = TF.relu(TF.linear(g, sd[p + ".f_glo.fc.0.weight"], sd[p + ".f_glo.fc.0.bias"]))
    g = torch.sigmoid(TF.linear(g, sd[p + ".f_glo.fc.2.weight"], sd[p + ".f_glo.fc.2.bias"]))
    out = joi * g[:, :, None, None]
    return out + x if residual else out


def n_blocks(sd, stage):
    """Blocks in the ModuleList `stage2` / `stage3`, from the state_dict's keys."""
    return len({k.split(".")[1] for k in sd if k.startswith(stage + ".")})


def forward(net, x):
    """CGNet.forward (cgnet.py:60-93) -> tuple of full-resolution logits."""
    size = x.shape[2:]
    out0 = _cbp(net, x, "stage1_0", 2, 1)
    out0 = _cbp(net, out0, "stage1_1", 1, 1)
    out0 = _cbp(net, out0, "stage1_2", 1, 1)
    inp1 = TF.avg_pool2d(x, 3, 2, 1)
    inp2 = TF.avg_pool2d(inp1, 3, 2, 1)
    out0_cat = _bn_prelu(net, torch.cat([out0, inp1], 1), "bn_prelu1")
    out1_0 = block(net, out0_cat, "stage2_0", 2, True, False)
    out1 = out1_0
    for i in range(n_blocks(net.sd, "stage2")):
        out1 = block(net, out1, "stage2.%d" % i, 2, False, True)
    out1_cat = _bn_prelu(net, torch.cat([out1, out1_0, inp2], 1), "bn_prelu2")
    out2_0 = block(net, out1_cat, "stage3_0", 4, True, False)
    out2 = out2_0
    for i in range(n_blocks(net.sd, "stage3")):
        out2 = block(net, out2, "stage3.%d" % i, 4, False, True)
    out2_cat = _bn_prelu(net, torch.cat([out2_0, out2], 1), "bn_prelu3")
    out = net.conv(out2_cat, "head.1")
    return (TF.interpolate(out, size, mode="bilinear", align_corners=True),)


def evaluate(sd, x):
    net = torch_ref.OracleNet({k: v.clone() for k, v in sd.items()}, training=False)
    with torch.no_grad():
        return forward(net, x)


def train(sd, x, y, dtype=torch.float32, device=None, autocast=False):
    """One training forward + cross-entropy (ignore_index -1; MixSoftmaxCrossEntropyLoss with one
    output) + backward, dropout 0 -> (loss, outputs, gradients by key, state after the step:
    running statistics and counters).  autocast: float32 parameters under
    torch.autocast(bfloat16) — what mixed precision costs the reference itself on this fixture."""
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
