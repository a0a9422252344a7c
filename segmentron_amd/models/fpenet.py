"""FPENet ("Feature Pyramid Encoding Network for Real-time Semantic Segmentation") — module tree /
state_dict of segmentron/models/fpenet.py:14-247, forward on the HIP kernels.

No backbone.  A 3x3 / stride-2 stem and three stages of FPE blocks (1, 3 and 9 blocks of 16, 32 and
64 channels at 1/2, 1/4 and 1/8 resolution), then two MEU modules that fuse 1/8 into 1/4 and 1/4
into 1/2, a biased 1x1 projection to the classes and a bilinear resize by 2.

An FPE block is a 1x1 convolution to the bottleneck (4n channels), the feature pyramid — four
depthwise 3x3 of dilation 1, 2, 4, 8 over the four quarters, stage s reading its quarter plus the
activated output of stage s - 1, each with its own BatchNorm + ReLU — a 1x1 convolution back, and
the residual sum with ReLU.  The pyramid is ONE autograd node (functional.fpe_pyramid on
csrc/fpenet.hip): per stage one launch, nothing but the raw stage outputs and the activated concat
is ever stored.  The quarters are 4 (layer1.0), 16, 8, 8 (layer2) and 32, 16 x 8 (layer3) channels
wide.  The tail of an MEU module — the channel gate, the spatial gate, the resize and the sum — is
one launch forward and two backward (functional.meu_fuse)."""
import torch
import torch.nn as nn

from .. import functional as F
from ..config import cfg
from ..hip_ops import vec_of
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["FPENet"]


@MODEL_REGISTRY.register()
class FPENet(SegBaseModel):
    def __init__(self):
        super().__init__(need_backbone=False)
        if cfg.MODEL.BN_TYPE != "BN":
            raise NotImplementedError("FPENet: BN_TYPE %r is not served (the pyramid stages hand "
                                      "their statistics to a BatchNorm)" % cfg.MODEL.BN_TYPE)
        norm_layer = self.norm_layer if self.norm_layer is not None else nn.BatchNorm2d
        width, scales = 16, 4
        planes = [width * 2 ** i for i in range(3)]
        self.block_num = [1, 3, 9]
        self.dilation = [1, 2, 4, 8]
        self.inplanes = planes[0]
        self.conv1 = nn.Conv2d(3, planes[0], kernel_size=3, stride=2, padding=1, bias=False)
        self.bn1 = norm_layer(planes[0])
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = self._make_layer(planes[0], self.block_num[0], 1, 1, scales, norm_layer)
        self.layer2 = self._make_layer(planes[1], self.block_num[1], 2, 4, scales, norm_layer)
        self.layer3 = self._make_layer(planes[2], self.block_num[2], 2, 4, scales, norm_layer)
        self.meu1 = MEUModule(64, 32, 64)
        self.meu2 = MEUModule(64, 16, 32)
        self.project_layer = nn.Conv2d(32, self.nclass, kernel_size=1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride, t, scales, norm_layer):
        """The first block changes the width and the resolution (expansion t, a 1x1 shortcut); the
        others keep both and, as in the reference, fall back to t = 1."""
        downsample = None
        if stride != 1 or self.inplanes != planes:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes, kernel_size=1, stride=stride, bias=False),
                norm_layer(planes))
        layers = [FPEBlock(self.inplanes, planes, self.dilation, downsample, stride, t, scales,
                           norm_layer=norm_layer)]
        self.inplanes = planes
        for _ in range(1, blocks):
            layers.append(FPEBlock(planes, planes, self.dilation, scales=scales,
                                   norm_layer=norm_layer))
        return nn.Sequential(*layers)

    def forward(self, x):
        from .. import compute_dtype
        H, W = x.shape[2:]
        t = F.image_to_nhwc(x, compute_dtype())
        a = F.conv_bn(F.Act(t), self.conv1, self.bn1)
        a.relu = True
        x_1 = self.layer1[0](F.materialize(a))
        x_1, low1 = F.fork(x_1, 2)

        x_2_0 = self.layer2[0](x_1)
        x_2_0, skip = F.fork(x_2_0, 2)
        x_2_2 = self.layer2[2](self.layer2[1](x_2_0))
        x_2 = F.materialize(F.Act(skip), residual=F.Act(x_2_2))
        x_2, low2 = F.fork(x_2, 2)

        x_3_0 = self.layer3[0](x_2)
        x_3_0, skip = F.fork(x_3_0, 2)
        t = x_3_0
        for blk in list(self.layer3)[1:]:
            t = blk(t)
        x_3 = F.materialize(F.Act(skip), residual=F.Act(t))

        x2 = self.meu1(x_3, low2)
        x1 = self.meu2(x2, low1)
        lo = self._project(x1)
        # F.interpolate(scale_factor=2, align_corners=True) of the map at ceil(H/2) x ceil(W/2)
        size = (2 * lo.shape[1], 2 * lo.shape[2])
        assert size == (2 * ((H + 1) // 2), 2 * ((W + 1) // 2))
        return [F.logits_to_nchw(lo, size, align_corners=True,
                                 lazy=F.want_lazy_logits(self.training))]

    def _project(self, t):
        """The biased 32 -> nclass projection, in float32 in every compute dtype as CGNet's
        classifier; returns the nclass leading channels of a vector-padded NHWC buffer."""
        if t.dtype != torch.float32:
            t = t.float()
        N, H, W, _ = t.shape
        vec = vec_of(t.dtype)
        pitch = (self.nclass + 2 * vec - 1) // vec * vec
        out = torch.empty((N, H, W, pitch), dtype=t.dtype, device=t.device)
        return F.conv_bn(F.Act(t), self.project_layer, None, out=out[..., :self.nclass]).t


class SEModule(nn.Module):
    """fpenet.py:132-147.  FPENet builds its blocks with se=False: never instantiated there, kept
    for the module tree."""

    def __init__(self, channels, reduction=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, channels // reduction, kernel_size=1, padding=0)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(channels // reduction, channels, kernel_size=1, padding=0)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        raise NotImplementedError("SEModule: se=True is not served (the reference never sets it)")


class FPEBlock(nn.Module):
    """fpenet.py:150-201.  x: plain NHWC; returns the plain activated output."""

    def __init__(self, inplanes, outplanes, dilat, downsample=None, stride=1, t=1, scales=4,
                 se=False, norm_layer=None):
        super().__init__()
        if inplanes % scales != 0:
            raise ValueError("Planes must be divisible by scales")
        if scales != 4:
            raise NotImplementedError("FPEBlock: scales = %d (the pyramid node has 4 stages)"
                                      % scales)
        if se:
            raise NotImplementedError("FPEBlock: se=True is not served")
        norm_layer = norm_layer if norm_layer is not None else nn.BatchNorm2d
        bottleneck = inplanes * t
        n = bottleneck // scales
        self.conv1 = nn.Conv2d(inplanes, bottleneck, kernel_size=1, stride=stride, bias=False)
        self.bn1 = norm_layer(bottleneck)
        self.conv2 = nn.ModuleList([nn.Conv2d(n, n, kernel_size=3, padding=dilat[i],
                                              dilation=dilat[i], groups=n, bias=False)
                                    for i in range(scales)])
        self.bn2 = nn.ModuleList([norm_layer(n) for _ in range(scales)])
        self.conv3 = nn.Conv2d(bottleneck, outplanes, kernel_size=1, bias=False)
        self.bn3 = norm_layer(outplanes)
        self.relu = nn.ReLU(inplace=True)
        self.se = None
        self.downsample = downsample
        self.stride = stride
        self.scales = scales

    def forward(self, x):
        x, identity = F.fork(x, 2)
        a = F.conv_bn(F.Act(x), self.conv1, self.bn1)
        cat = F.fpe_pyramid(a, list(self.conv2), list(self.bn2))
        out = F.conv_bn(F.Act(cat), self.conv3, self.bn3)
        if self.downsample is not None:
            res = F.conv_bn(F.Act(identity), self.downsample[0], self.downsample[1])
        else:
            res = F.Act(identity)
        return F.materialize(out, residual=res, post_relu=True)


class MEUModule(nn.Module):
    """fpenet.py:205-247.  fms_high / fms_low: plain NHWC; returns the plain fused map at the
    low-level resolution."""

    def __init__(self, channels_high, channels_low, channel_out):
        super().__init__()
        self.conv1x1_low = nn.Conv2d(channels_low, channel_out, kernel_size=1, bias=False)
        self.bn_low = nn.BatchNorm2d(channel_out)
        self.sa_conv = nn.Conv2d(1, 1, kernel_size=1, bias=False)
        self.conv1x1_high = nn.Conv2d(channels_high, channel_out, kernel_size=1, bias=False)
        self.bn_high = nn.BatchNorm2d(channel_out)
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.ca_conv = nn.Conv2d(channel_out, channel_out, kernel_size=1, bias=False)
        self.sa_sigmoid = nn.Sigmoid()
        self.ca_sigmoid = nn.Sigmoid()
        self.relu = nn.ReLU(inplace=True)

    def forward(self, fms_high, fms_low):
        low = F.conv_bn(F.Act(fms_low), self.conv1x1_low, self.bn_low)
        high = F.conv_bn(F.Act(fms_high), self.conv1x1_high, self.bn_high)
        return F.meu_fuse(low, high, self.ca_conv, self.sa_conv)
