"""Torch restatement of the reference's UNet (segmentron/models/unet.py) for the tests and
tools/unet_bench.py: OracleNet's `bn` and `conv` plus the double convolution, the max-pool and the
padded upsampling in torch.nn.functional — no kernel of this repository.  Runs in float32 / float64
on the CPU and, for the bench tool, on the device through torch's own kernels.  Pinned against the
reference itself by tests/golden/unet_*.npz (tools/gen_golden_unet.py, tests/test_unet.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

B, H, W = 2, 64, 96            # evaluation, small-train and loop fixtures: maps down to 4 x 6
H_ODD, W_ODD = 70, 97          # second evaluation size: 70x97, 35x48, 17x24, 8x12, 4x6 — the decoder
#                                pads one row at the 35- and 17-row levels and one column at the top
TB, TH, TW = 4, 64, 96         # training fixture: 24576 / 6144 / 1536 rows per BatchNorm at levels
#                                0-2 (the plain path), 384 / 96 at levels 3-4 (the few-sample path)
FB, FH, FW = 2, 48, 80         # the fused-loss tier test: logits at head stride 1
# Image / target seed of the training fixture: the FIRST seed whose float64 run keeps decidable in
# float32 (a) every ReLU input — at least RELU_MARGIN, relative to the magnitudes of the terms that
# form it, away from the kink — and (b) every 2x2 max-pool window with a positive winner — its top-2
# gap at least RELU_MARGIN of the winner's scale — and whose float32 run then takes every one of
# those decisions as the float64 run does, so that neither a ReLU mask nor a pool's winner depends on
# float32 rounding (see tests/_lednet_oracle.py).  The second condition is not implied by the first
# here: the sums behind a BatchNorm input have up to 9216 terms, and ONE moved winner at level 1
# (seed 493, the first with the margin) is 3.4e-4 of the gradient's global norm — a weight gradient
# is a sum with cancellation over the map, one routed element is 1 / sqrt(elements) of it.
# tools/gen_golden_unet.py repeats the scan and asserts that it is this one.  (About 13 M ReLU
# inputs and 0.7 M windows per run: the margin alone is met by one seed in several hundred — 493,
# 765, 1318 — and the scan takes minutes.)
TRAIN_SEED = 765
RELU_MARGIN = 16 * 2.0 ** -24
LEVELS = ("inc", "down1.maxpool_conv.1", "down2.maxpool_conv.1", "down3.maxpool_conv.1",
          "down4.maxpool_conv.1")


def state(keys_and_shapes):
    """The fixtures' weights: oracle.synth, seed 0, conditioned."""
    return synth.synth_state_dict(list(keys_and_shapes), seed=0, conditioned=True)


def _relu(z, scale):
    return TF.relu(z)


def _pool(a, scale):
    return TF.max_pool2d(a, 2)


def _bn_relu(net, t, prefix, relu):
    """-> (relu(bn(t)), the magnitude its input is decided against)."""
    z = net.bn(t, prefix)
    b = net.sd[prefix + ".bias"].view(1, -1, 1, 1)
    scale = (z - b).abs() + b.abs()
    return relu(z, scale), scale


def double_conv(net, x, p, relu=_relu):
    """DoubleConv.forward (unet.py:63-78)."""
    x, _ = _bn_relu(net, net.conv(x, p + ".double_conv.0", 1, 1), p + ".double_conv.1", relu)
    return _bn_relu(net, net.conv(x, p + ".double_conv.3", 1, 1), p + ".double_conv.4", relu)


def forward(net, x, relu=_relu, pool=_pool):
    """UNet.forward (unet.py:27-40, 53-60, 109-121) -> list of one map of the input's size."""
    size = x.shape[2:]
    a, s = double_conv(net, x, LEVELS[0], relu)
    feats = [a]
    for p in LEVELS[1:]:
        a, s = double_conv(net, pool(a, s), p, relu)
        feats.append(a)
    x = feats[4]
    for i, skip in enumerate(reversed(feats[:4])):
        x = TF.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        dy, dx = skip.shape[2] - x.shape[2], skip.shape[3] - x.shape[3]
        x = TF.pad(x, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
        x, _ = double_conv(net, torch.cat([skip, x], 1), "head.up%d.conv" % (i + 1), relu)
    x = net.conv(x, "head.outc.conv")
    return [TF.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)]


def _decisions(sd, x, dtype, margins=None):
    """One training-mode forward pass in `dtype` -> every ReLU mask and every positive window's
    winner; margins (a list): the relative margins of those decisions are appended."""
    taken = []

    def relu(z, scale):
        if margins is not None:
            margins.append((z.abs() / scale).min().item())
        taken.append(z > 0)
        return TF.relu(z)

    def pool(a, scale):
        n, c, h, w = a.shape
        h2, w2 = h // 2, w // 2

        def windows(t):
            t = t[..., :2 * h2, :2 * w2].reshape(n, c, h2, 2, w2, 2)
            return t.permute(0, 1, 2, 4, 3, 5).reshape(n, c, h2, w2, 4)
        top, idx = windows(a).topk(2, dim=-1)
        won = top[..., 0] > 0
        if margins is not None and won.any():
            sc = windows(scale).gather(-1, idx[..., :1])[..., 0]
            margins.append((((top[..., 0] - top[..., 1]) / sc)[won]).min().item())
        p, where = TF.max_pool2d(a, 2, return_indices=True)
        taken.append(torch.where(p > 0, where, torch.full_like(where, -1)))
        return p
    # (copies: the training-mode pass moves the running statistics it is given)
    s = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        forward(torch_ref.OracleNet(s, training=True, drop_p=0.0), x.to(dtype), relu, pool)
    return taken


def min_relu_margin(sd, x):
    """Smallest margin of one float64 training-mode forward pass over (a) |z| / scale of every
    BatchNorm + ReLU input z (scale |z - beta| + |beta|) and (b) (top1 - top2) / scale(top1) of
    every 2x2 max-pool window whose winner is positive — or 0 where that margin reaches RELU_MARGIN
    and the float32 run still takes one of these decisions differently."""
    margins = []
    d64 = _decisions(sd, x, torch.float64, margins)
    m = min(margins)
    if m >= RELU_MARGIN:
        d32 = _decisions(sd, x, torch.float32)
        if any(not torch.equal(a, b) for a, b in zip(d64, d32)):
            return 0.0
    return m


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
