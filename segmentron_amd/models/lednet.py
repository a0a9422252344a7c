"""LEDNet ("A Lightweight Encoder-Decoder Network for Real-Time Semantic Segmentation") — module
tree / state_dict of segmentron/models/lednet.py:13-159, forward on the HIP kernels.

No backbone.  Three two-branch stride-2 downsamplings and 15 split-shuffle blocks (SSnbt): each
block splits its input into two channel halves, runs four factorised 3-tap convolutions per half
((3,1) / (1,3), the second pair dilated), concatenates, adds the input, applies ReLU and shuffles
the channels.  Here the 120 line convolutions of a forward pass run on csrc/conv_line.hip
(functional.line_conv_bn: MFMA without LDS staging, BatchNorm statistics from the epilogue, the
pending BatchNorm / ReLU of the producer in the prologue), and the tail of a block — two BatchNorm
+ ReLU, cat, + x, ReLU, channel_shuffle — is one pass (functional.ssnbt_tail).  In backward the
three gradients of a block input (two halves, residual) meet in the epilogues of the two first
convolutions' data-gradient launches (functional.BlockGrad).

The attention pyramid head (APNModule) runs on the existing operators: dense 3x3 / 5x5 / 7x7
stride-2 convolutions, bilinear resizes, the few-sample BatchNorm path for the pooled branch.  Its
nclass-channel maps (19 on Cityscapes) live in zero-padded buffers of round_up8(nclass) channels
with a zero-padded BatchNorm, as CGNet's 35- and 131-channel concats do.  The last three
statements, `level4(x) * out + level5(x)`, act on those maps at 1/8 resolution and use torch's
element-wise operators on the NHWC tensors."""
import torch
import torch.nn as nn

from .. import functional as F
from ..hip_ops import conv_out_size, round_up8
from ..modules import _ConvBNReLU
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["LEDNet"]


@MODEL_REGISTRY.register()
class LEDNet(SegBaseModel):
    def __init__(self):
        super().__init__(need_backbone=False)
        nl = self.norm_layer
        self.encoder = nn.Sequential(
            Downsampling(3, 32),
            SSnbt(32, norm_layer=nl), SSnbt(32, norm_layer=nl), SSnbt(32, norm_layer=nl),
            Downsampling(32, 64),
            SSnbt(64, norm_layer=nl), SSnbt(64, norm_layer=nl),
            Downsampling(64, 128),
            SSnbt(128, norm_layer=nl),
            SSnbt(128, 2, norm_layer=nl), SSnbt(128, 5, norm_layer=nl), SSnbt(128, 9, norm_layer=nl),
            SSnbt(128, 2, norm_layer=nl), SSnbt(128, 5, norm_layer=nl), SSnbt(128, 9, norm_layer=nl),
            SSnbt(128, 17, norm_layer=nl),
        )
        self.head = APNModule(128, self.nclass, norm_layer=nl)
        self.__setattr__("decoder", ["head"])

    def forward(self, x):
        from .. import compute_dtype
        size = x.shape[2:]
        t = F.image_to_nhwc(x, compute_dtype())
        for layer in self.encoder:
            t = layer(t)
        lo = self.head(t)
        return (F.logits_to_nchw(lo, size, align_corners=True,
                                 lazy=F.want_lazy_logits(self.training)),)


class Downsampling(nn.Module):
    """Two 3x3 / stride 2 / pad 2 convolutions over the same input, each followed by
    MaxPool2d(2, stride 1), concatenated (lednet.py:55-69).  The convolutions write the two halves
    of one buffer and ONE pooling pass follows: the pool is per channel.  x: plain NHWC."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, out_channels // 2, 3, 2, 2, bias=False)
        self.conv2 = nn.Conv2d(in_channels, out_channels // 2, 3, 2, 2, bias=False)
        self.pool = nn.MaxPool2d(kernel_size=2, stride=1)

    def forward(self, x):
        N, H, W, _ = x.shape
        h = self.conv1.out_channels
        Ho, Wo = conv_out_size(H, 3, 2, 2, 1), conv_out_size(W, 3, 2, 2, 1)
        buf = torch.empty((N, Ho, Wo, 2 * h), dtype=x.dtype, device=x.device)
        a, b = F.fork(x, 2)
        y1 = F.conv_bn(F.Act(a), self.conv1, None, out=buf[..., :h]).t
        y2 = F.conv_bn(F.Act(b), self.conv2, None, out=buf[..., h:]).t
        return F.max_pool(F.Act(F.concat_alias(buf, [y1, y2])), 2, 1, 0)


class SSnbt(nn.Module):
    """Split-shuffle non-bottleneck block (lednet.py:72-128).  x: plain NHWC; returns plain."""

    def __init__(self, in_channels, dilation=1, norm_layer=nn.BatchNorm2d):
        super().__init__()
        c = in_channels // 2
        d = dilation
        self.branch1 = nn.Sequential(
            nn.Conv2d(c, c, (3, 1), padding=(1, 0), bias=False),
            nn.ReLU(True),
            nn.Conv2d(c, c, (1, 3), padding=(0, 1), bias=False),
            norm_layer(c),
            nn.ReLU(True),
            nn.Conv2d(c, c, (3, 1), padding=(d, 0), dilation=(d, 1), bias=False),
            nn.ReLU(True),
            nn.Conv2d(c, c, (1, 3), padding=(0, d), dilation=(1, d), bias=False),
            norm_layer(c),
            nn.ReLU(True))
        self.branch2 = nn.Sequential(
            nn.Conv2d(c, c, (1, 3), padding=(0, 1), bias=False),
            nn.ReLU(True),
            nn.Conv2d(c, c, (3, 1), padding=(1, 0), bias=False),
            norm_layer(c),
            nn.ReLU(True),
            nn.Conv2d(c, c, (1, 3), padding=(0, d), dilation=(1, d), bias=False),
            nn.ReLU(True),
            nn.Conv2d(c, c, (3, 1), padding=(d, 0), dilation=(d, 1), bias=False),
            norm_layer(c),
            nn.ReLU(True))
        self.relu = nn.ReLU(True)

    @staticmethod
    def _branch(seq, x, bg, half, out):
        """conv, ReLU, conv, BN, ReLU, conv, ReLU, conv, BN, ReLU: the ReLUs and BatchNorms ride
        in the next convolution's prologue (the last pair in the tail)."""
        a = F.line_conv_bn(F.Act(x), seq[0], None, first=bg, half=half)
        a.relu = True
        a = F.line_conv_bn(a, seq[2], seq[3])
        a.relu = True
        a = F.line_conv_bn(a, seq[5], None)
        a.relu = True
        a = F.line_conv_bn(a, seq[7], seq[8], out=out)
        a.relu = True
        return a

    def forward(self, x):
        N, H, W, C = x.shape
        h = C // 2
        bg = None
        if torch.is_grad_enabled() and x.requires_grad:
            bg = F.BlockGrad()
            x1, x2 = F.split_halves(x, bg)
        else:
            x1, x2 = x[..., :h], x[..., h:]
        # the branches' last convolutions write the two halves of one buffer
        ybuf = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
        a1 = self._branch(self.branch1, x1, bg, 0, ybuf[..., :h])
        a2 = self._branch(self.branch2, x2, bg, 1, ybuf[..., h:])
        return F.ssnbt_tail(a1, a2, x, bg)


class APNModule(nn.Module):
    """Attention pyramid network (lednet.py:131-159).  x: plain NHWC [N,H,W,128]; returns the
    nclass-channel logits at x's resolution as a view of a channel-padded buffer."""

    def __init__(self, in_channels, nclass, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.conv1 = _ConvBNReLU(in_channels, in_channels, 3, 2, 1, norm_layer=norm_layer)
        self.conv2 = _ConvBNReLU(in_channels, in_channels, 5, 2, 2, norm_layer=norm_layer)
        self.conv3 = _ConvBNReLU(in_channels, in_channels, 7, 2, 3, norm_layer=norm_layer)
        self.level1 = _ConvBNReLU(in_channels, nclass, 1, norm_layer=norm_layer)
        self.level2 = _ConvBNReLU(in_channels, nclass, 1, norm_layer=norm_layer)
        self.level3 = _ConvBNReLU(in_channels, nclass, 1, norm_layer=norm_layer)
        self.level4 = _ConvBNReLU(in_channels, nclass, 1, norm_layer=norm_layer)
        self.level5 = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            _ConvBNReLU(in_channels, nclass, 1))
        self.nclass = nclass

    def _level(self, mod, act):
        """1x1 conv to nclass channels + BN + ReLU -> a deferred activation of round_up8(nclass)
        channels: the convolution writes its nclass channels into a zeroed buffer, the BatchNorm
        is padded with zeros (scale = shift = gamma = 0 there: the pad channels stay zero in
        every consumer and their gradients are exact zeros)."""
        N, H, W, _ = act.shape
        nc, cp = self.nclass, round_up8(self.nclass)
        buf = torch.zeros((N, H, W, cp), dtype=act.t.dtype, device=act.t.device)
        a = F.conv_bn(act, mod.conv, mod.bn, out=buf[..., :nc])
        return F.Act(F.concat_alias(buf, [a.t]), F._pad_bn(a.bn, cp), F.RELU)

    def forward(self, x):
        N, H, W, _ = x.shape
        xa, xb, xc = F.fork(x, 3)
        b3 = self.conv1(F.Act(xa))
        b2 = self.conv2(b3)
        b1 = self.conv3(b2)
        out = F.bilinear(self._level(self.level1, b1), ((H + 3) // 4, (W + 3) // 4))
        out = F.materialize(self._level(self.level2, b2), residual=F.Act(out))
        out = F.bilinear(F.Act(out), ((H + 1) // 2, (W + 1) // 2))
        out = F.materialize(self._level(self.level3, b3), residual=F.Act(out))
        out = F.bilinear(F.Act(out), (H, W))
        l4 = F.materialize(self._level(self.level4, F.Act(xb)))
        # nn.AdaptiveAvgPool2d(1) -> 1x1 conv + nn.BatchNorm2d over N rows (float32, two-pass
        # statistics) + ReLU
        pooled = F.global_avg_pool(xc, keep_fp32=True)
        l5 = F.materialize(self._level(self.level5[1], F.Act(pooled)))
        # at most round_up8(nclass) channels at 1/8 resolution: torch's element-wise operators
        out = l4 * out + l5.to(out.dtype)
        return out[..., :self.nclass]
