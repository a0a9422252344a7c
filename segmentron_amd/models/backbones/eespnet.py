"""EESPNet, the backbone of ESPNetv2 — module tree / state_dict of
segmentron/models/backbones/eespnet.py:14-166, the segmentation forward (`seg=True`) on the HIP
kernels.

Four levels: a 3x3 / stride-2 stem, then three DownSamplers (a 3x3 / stride-2 average pool next
to a stride-2 EESP unit, concatenated, plus a reinforcement branch that reads the image pooled
down to the same size) with 3 and 7 stride-1 EESP units behind the second and third.  A
DownSampler writes the pool and the EESP expansion into the two channel slices of one buffer; the
tail `act(cat[avg, bn(eesp)] + bn(inp_reinf(x2)))` is one pass (functional.bn_add_prelu with the
BatchNorm of the concat operand on its EESP channels only).

`level5_0`, `level5` and `fc` exist for state_dict parity: the segmentation forward never runs
them, so their parameters have no gradient (not a zero one: weight decay must not move them).  The
classification path (`seg=False`) is not on the HIP path."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as TF

from ... import functional as F
from ...modules import EESP, _ConvBN, _ConvBNPReLU
from .build import BACKBONE_REGISTRY

__all__ = ["EESPNet", "eespnet"]


class DownSampler(nn.Module):
    """eespnet.py:14-43.  x: plain NHWC; x2: the float32 NCHW image already pooled to this
    DownSampler's output size (EESPNet.forward cascades the pools: the same arithmetic as the
    reference's loop from the full image, once); returns the plain NHWC output."""

    def __init__(self, in_channels, out_channels, k=4, r_lim=9, reinf=True, inp_reinf=3,
                 norm_layer=None):
        super().__init__()
        channels_diff = out_channels - in_channels
        self.eesp = EESP(in_channels, channels_diff, stride=2, k=k, r_lim=r_lim, down_method="avg",
                         norm_layer=norm_layer)
        self.avg = nn.AvgPool2d(kernel_size=3, padding=1, stride=2)
        if reinf:
            self.inp_reinf = nn.Sequential(
                _ConvBNPReLU(inp_reinf, inp_reinf, 3, 1, 1),
                _ConvBN(inp_reinf, out_channels, 1, 1))
        self.act = nn.PReLU(out_channels)

    def _reinforce(self, x2, dtype):
        """inp_reinf on the pooled image -> Act [N,H,W,out_channels], BatchNorm pending.  The
        3-channel maps live in zero-padded 8-channel buffers (as CGNet's injected image does)."""
        m0, m1 = self.inp_reinf[0], self.inp_reinf[1]
        img = F.Act(F.image_to_nhwc(x2, dtype))
        N, H, W, _ = img.shape
        c = m0.conv.out_channels
        buf = torch.zeros((N, H, W, F.K.round_up8(c)), dtype=dtype, device=img.t.device)
        a = F.conv_bn(img, m0.conv, m0.bn, out=buf[..., :c])
        r = F.bn_prelu(F.Act(F.concat_alias(buf, [a.t]), a.bn), m0.prelu)
        return m1(F.Act(r))

    def forward(self, x, x2=None, out=None):
        N, H, W, cin = x.shape
        cout = self.act.weight.numel()
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        buf = torch.empty((N, Ho, Wo, cout), dtype=x.dtype, device=x.device)
        xa, xb = F.fork(x, 2)
        avg = F.avg_pool3x3s2(xa, out=buf[..., :cin])
        e = self.eesp(xb, out=buf[..., cin:])
        cat = F.Act(F.concat_alias(buf, [avg, e.t]), e.bn)
        if x2 is None:
            raise NotImplementedError("DownSampler without input reinforcement (level5_0, the "
                                      "classification path) is not on the HIP path")
        if tuple(x2.shape[2:]) != (Ho, Wo):
            raise ValueError("DownSampler: the pooled image %s does not match the output %s"
                             % (tuple(x2.shape[2:]), (Ho, Wo)))
        return F.bn_add_prelu(cat, self._reinforce(x2, x.dtype), self.act, lead=cin, out=out)


class EESPNet(nn.Module):
    def __init__(self, num_classes=1000, scale=1, reinf=True, norm_layer=nn.BatchNorm2d):
        super().__init__()
        if scale != 1:
            raise NotImplementedError("EESPNet: scale != 1 is not served")
        inp_reinf = 3 if reinf else None
        reps = [0, 3, 7, 3]
        r_lim = [13, 11, 9, 7, 5]
        K = [4] * len(r_lim)

        base, levels, base_s = 32, 5, 0
        out_channels = [base] * levels
        for i in range(levels):
            if i == 0:
                base_s = int(base * scale)
                base_s = math.ceil(base_s / K[0]) * K[0]
                out_channels[i] = base if base_s > base else base_s
            else:
                out_channels[i] = base_s * pow(2, i)
        out_channels.append(1024)

        self.level1 = _ConvBNPReLU(3, out_channels[0], 3, 2, 1, norm_layer=norm_layer)

        self.level2_0 = DownSampler(out_channels[0], out_channels[1], k=K[0], r_lim=r_lim[0],
                                    reinf=reinf, inp_reinf=inp_reinf, norm_layer=norm_layer)

        self.level3_0 = DownSampler(out_channels[1], out_channels[2], k=K[1], r_lim=r_lim[1],
                                    reinf=reinf, inp_reinf=inp_reinf, norm_layer=norm_layer)
        self.level3 = nn.ModuleList()
        for i in range(reps[1]):
            self.level3.append(EESP(out_channels[2], out_channels[2], k=K[2], r_lim=r_lim[2],
                                    norm_layer=norm_layer))

        self.level4_0 = DownSampler(out_channels[2], out_channels[3], k=K[2], r_lim=r_lim[2],
                                    reinf=reinf, inp_reinf=inp_reinf, norm_layer=norm_layer)
        self.level4 = nn.ModuleList()
        for i in range(reps[2]):
            self.level4.append(EESP(out_channels[3], out_channels[3], k=K[3], r_lim=r_lim[3],
                                    norm_layer=norm_layer))

        self.level5_0 = DownSampler(out_channels[3], out_channels[4], k=K[3], r_lim=r_lim[3],
                                    reinf=reinf, inp_reinf=inp_reinf, norm_layer=norm_layer)
        self.level5 = nn.ModuleList()
        for i in range(reps[2]):
            self.level5.append(EESP(out_channels[4], out_channels[4], k=K[4], r_lim=r_lim[4],
                                    norm_layer=norm_layer))
        self.level5.append(_ConvBNPReLU(out_channels[4], out_channels[4], 3, 1, 1,
                                        groups=out_channels[4], norm_layer=norm_layer))
        self.level5.append(_ConvBNPReLU(out_channels[4], out_channels[5], 1, 1, 0,
                                        groups=K[4], norm_layer=norm_layer))

        self.fc = nn.Linear(out_channels[5], num_classes)

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=0.001)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward(self, x, seg=True, outs=None):
        """x: the NCHW image.  -> (out_l1, out_l2, out_l3, out_l4), plain NHWC.  `outs`: optional
        NHWC views (channel slices of the decoder's concat buffers) for out_l1 .. out_l3."""
        from ... import compute_dtype
        if not seg:
            raise NotImplementedError("EESPNet: the classification path (seg=False) is not on "
                                      "the HIP path")
        if x.shape[2] % 16 != 0 or x.shape[3] % 16 != 0:
            # (the reference itself raises at its first concat for any other size)
            raise ValueError("ESPNetv2 takes input sizes that are multiples of 16, got %s"
                             % (tuple(x.shape[2:]),))
        o1, o2, o3 = outs if outs is not None else (None, None, None)
        dt = compute_dtype()
        # the image pooled to 1/4, 1/8 and 1/16: no gradient, torch's own pooling on NCHW float32
        p = TF.avg_pool2d(x.float(), 3, 2, 1)
        p2 = TF.avg_pool2d(p, 3, 2, 1)
        p3 = TF.avg_pool2d(p2, 3, 2, 1)
        p4 = TF.avg_pool2d(p3, 3, 2, 1)

        out_l1 = self.level1(F.Act(F.image_to_nhwc(x, dt)), out=o1)
        a, out_l1 = F.fork(out_l1, 2)
        out_l2 = self.level2_0(a, p2, out=o2)
        a, out_l2 = F.fork(out_l2, 2)
        t = self.level3_0(a, p3)
        for i, layer in enumerate(self.level3):
            t = layer(t, out=o3 if i == len(self.level3) - 1 else None)
        a, out_l3 = F.fork(t, 2)
        t = self.level4_0(a, p4)
        for layer in self.level4:
            t = layer(t)
        return out_l1, out_l2, out_l3, t


@BACKBONE_REGISTRY.register()
def eespnet(norm_layer=nn.BatchNorm2d):
    return EESPNet(norm_layer=norm_layer)
