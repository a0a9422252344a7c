"""CPU restatement of the reference's PointRend (segmentron/models/pointrend.py) and PointRendLoss
(segmentron/solver/loss.py:364-387) for the tests: OracleNet's xception65, ASPP and separable
convs composed into the decoder-less DeepLabV3+ head, plus the point head with F.grid_sample,
conv1d and a stable sort (ties to the lower index).  Pinned against the reference itself by
tests/golden/pointrend_ref_run.npz (tools/gen_golden_pointrend.py, tests/test_pointrend.py)."""
import torch
import torch.nn.functional as TF

from oracle import synth, torch_ref

H, W, B = 97, 129, 2  # 97 * 129 > 8096: the last evaluation step really selects


def grid(x, p, mode="bilinear"):
    """The reference's point_sample (pointrend.py:119-141)."""
    return TF.grid_sample(x, 2.0 * p.unsqueeze(2) - 1.0, mode=mode, padding_mode="zeros",
                          align_corners=False).squeeze(3)


def state(keys_and_shapes):
    """Synthesised weights of the fixture: oracle.synth (seed 1, conditioned) with He-scaled
    Conv1d weights (synth treats 3-d tensors as BatchNorm gammas)."""
    sd = synth.synth_state_dict(keys_and_shapes, seed=1, conditioned=True)
    g = torch.Generator().manual_seed(1)
    for i in (0, 2, 4, 6):
        w = sd["head.mlp.%d.weight" % i]
        sd["head.mlp.%d.weight" % i] = torch.randn(w.shape, generator=g) * (2.0 / w.shape[1]) ** 0.5
    return sd


def draws():
    """The recorded torch.rand draws: over-generation [B, 3P, 2], coverage [B, P - 0.75P, 2]."""
    P = (W // 16) ** 2
    g = torch.Generator().manual_seed(0)
    over = torch.rand(B, 3 * P, 2, generator=g)
    cover = torch.rand(B, P - int(0.75 * P), 2, generator=g)
    return over, cover


def head(net, x):
    """DeepLabV3Plus.encoder + _DeepLabHead with ENABLE_DECODER False -> (c1, coarse logits)."""
    c1, _, _, c4 = net.xception65(x, prefix="backbone.encoder")
    h = net.aspp(c4, "backbone.head.aspp")
    h = net.separable_conv(h, "backbone.head.block.0", relu_first=False)
    h = net.separable_conv(h, "backbone.head.block.1", relu_first=False)
    return c1, net.conv(h, "backbone.head.block.2")


def mlp(s, feat):
    h = feat
    for i in (0, 2, 4):
        h = TF.relu(TF.conv1d(h, s["head.mlp.%d.weight" % i], s["head.mlp.%d.bias" % i]))
    return TF.conv1d(h, s["head.mlp.6.weight"], s["head.mlp.6.bias"])


def uncertainty_at(coarse, over):
    srt = coarse.sort(1, descending=True)[0]
    og = grid(srt[:, :2], over.to(coarse.dtype))
    return -(og[:, 0] - og[:, 1])


def select_train(coarse, over, cover, beta=0.75):
    """sampling_points, training (pointrend.py:183-195): importance points in descending
    uncertainty order, then the coverage draws."""
    with torch.no_grad():
        unc = uncertainty_at(coarse, over)
        n_imp = int(beta * (over.shape[1] // 3))
        idx = torch.sort(-unc, dim=1, stable=True)[1][:, :n_imp]
        imp = torch.gather(over, 1, idx.unsqueeze(-1).expand(-1, -1, 2))
        return torch.cat([imp, cover], 1)


def train(sd, x, y, dtype, over=None, cover=None, pts=None):
    """PointRend training forward + PointRendLoss at the given points (or at the points the
    draws select) -> (loss, seg loss, point loss, gradients, coarse logits, points)."""
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    s = torch_ref.clone_state(s, requires_grad=True)
    net = torch_ref.OracleNet(s, training=True, drop_p=0.0)
    c1, coarse = head(net, x.to(dtype))
    if pts is None:
        pts = select_train(coarse.detach().float(), over, cover)
    p = pts.to(dtype)
    rend = mlp(s, torch.cat([grid(coarse, p), grid(c1, p)], 1))
    pred = TF.interpolate(coarse, y.shape[-2:], mode="bilinear", align_corners=True)
    gtp = grid(y.to(dtype).unsqueeze(1), p, mode="nearest").squeeze(1).long()
    seg = TF.cross_entropy(pred, y, ignore_index=-1)
    pl = TF.cross_entropy(rend, gtp, ignore_index=-1)
    loss = seg + pl
    loss.backward()
    grads = {k: v.grad for k, v in s.items() if v.grad is not None}
    return loss.item(), seg.item(), pl.item(), grads, coarse.detach(), pts


def eval_head(sd, c1, coarse, out_hw, steps=None):
    """PointHead.inference (pointrend.py:72-116) from the backbone's c1 / coarse logits."""
    with torch.no_grad():
        out = coarse
        while True:
            last = not out.shape[-1] * 2 < out_hw[1]
            if last:
                out = TF.interpolate(out, size=out_hw, mode="bilinear", align_corners=False)
            else:
                out = TF.interpolate(out, scale_factor=2, mode="bilinear", align_corners=False)
            n, C, h, w = out.shape
            srt = out.sort(1, descending=True)[0]
            unc = -(srt[:, 0] - srt[:, 1]).view(n, -1)
            k = min(h * w, 8096)
            idx = torch.sort(-unc, dim=1, stable=True)[1][:, :k]
            pts = torch.zeros(n, k, 2)
            pts[:, :, 0] = 1 / w / 2.0 + (idx % w).to(torch.float) * (1 / w)
            pts[:, :, 1] = 1 / h / 2.0 + (idx // w).to(torch.float) * (1 / h)
            rend = mlp(sd, torch.cat([grid(out, pts), grid(c1, pts)], 1))
            out = out.reshape(n, C, -1).scatter_(2, idx.unsqueeze(1).expand(-1, C, -1),
                                                 rend).view(n, C, h, w)
            if steps is not None:
                steps.append((h, w))
            if last:
                return out


def evaluate(sd, x, steps=None):
    """PointRend evaluation forward (eval BatchNorm, float32) -> fine [B, C, H, W]."""
    net = torch_ref.OracleNet({k: v.clone() for k, v in sd.items()}, training=False)
    with torch.no_grad():
        c1, coarse = head(net, x)
    return eval_head(sd, c1, coarse, tuple(x.shape[-2:]), steps)
