"""DUNet ("Decoders Matter for Semantic Segmentation") — module tree / state_dict of
segmentron/models/dunet.py:13-117, forward on the HIP kernels.  Up to the last layer the model is
composition: ResNet encoder, 1x1 and 3x3 conv + BN + ReLU, a channel concat that its producers
write in place, _FCNHead.  The last layer, DUpsampling, is a 1x1 convolution to s*s*nclass
channels followed by a depth-to-space rearrangement; in NHWC that rearrangement is an address
computation, so the training forward returns functional.DUpLogitsView and the loss runs on the
convolution's own output (csrc/dupsample.hip).

OUTPUT_STRIDE 8 is the supported configuration (configs/cityscapes_dunet.yaml): there c2, c3 and c4
share one resolution and FeatureFused's two resizes are identities.  At OUTPUT_STRIDE 16 the resize
of c2 is real (it shrinks c2 to c4's size, functional.bilinear) and the forward is checked against
a fixture of the reference; its output is half the size of the target there, so neither this loss
nor the reference's can be computed: F.cross_entropy raises as torch does."""
import torch
import torch.nn as nn

from .. import functional as F
from ..modules import _FCNHead
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["DUNet"]


@MODEL_REGISTRY.register()
class DUNet(SegBaseModel):
    def __init__(self):
        super().__init__()
        self.head = _DUHead(2144, norm_layer=self.norm_layer)
        self.dupsample = DUpsampling(256, self.nclass, scale_factor=8)
        if self.aux:
            self.auxlayer = _FCNHead(1024, 256, norm_layer=self.norm_layer)
            self.aux_dupsample = DUpsampling(256, self.nclass, scale_factor=8)
        self.__setattr__("decoder", ["dupsample", "head", "auxlayer", "aux_dupsample"]
                         if self.aux else ["dupsample", "head"])

    def forward(self, x):
        lazy = F.want_lazy_logits(self.training)  # see functional.DUpLogitsView
        _, c2, c3, c4 = self.encoder(x)
        outputs = [self.dupsample(self.head(c2, c3, c4), lazy)]
        if self.aux:
            outputs.append(self.aux_dupsample(F.Act(self.auxlayer(c3)), lazy))
        return tuple(outputs)


def _cbr(act, conv, bn, out=None):
    a = F.conv_bn(act, conv, bn, out=out)
    a.relu = True
    return a


class FeatureFused(nn.Module):
    """1x1 conv + BN + ReLU of c2 (512 -> 48) and c3 (1024 -> 48), brought to c4's size first,
    then cat([c4, c3, c2]) (dunet.py:47-68).  Every part is written straight into its channel
    slice of one [N, h, w, 2144] buffer."""

    def __init__(self, inter_channels=48, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.conv2 = nn.Sequential(nn.Conv2d(512, inter_channels, 1, bias=False),
                                   norm_layer(inter_channels), nn.ReLU(True))
        self.conv3 = nn.Sequential(nn.Conv2d(1024, inter_channels, 1, bias=False),
                                   norm_layer(inter_channels), nn.ReLU(True))

    @staticmethod
    def _to(act, hw):
        """F.interpolate(.., hw, 'bilinear', align_corners=True); the same-size resize is an
        exact identity, skipped."""
        if tuple(act.shape[1:3]) == tuple(hw):
            return act
        return F.Act(F.bilinear(act, tuple(hw)))

    def forward(self, c2, c3, c4):
        x4 = F.materialize(c4)
        N, H, W, C4 = x4.shape
        ic = self.conv2[0].out_channels
        buf = torch.empty((N, H, W, C4 + 2 * ic), dtype=x4.dtype, device=x4.device)
        parts = [F.materialize(F.Act(x4), out=buf[..., :C4], force=True)]
        a3 = _cbr(self._to(c3, (H, W)), self.conv3[0], self.conv3[1])
        parts.append(F.materialize(a3, out=buf[..., C4:C4 + ic]))
        a2 = _cbr(self._to(c2, (H, W)), self.conv2[0], self.conv2[1])
        parts.append(F.materialize(a2, out=buf[..., C4 + ic:]))
        return F.Act(F.concat_alias(buf, parts))


class _DUHead(nn.Module):
    """FeatureFused -> two 3x3 conv + BN + ReLU to 256 channels (dunet.py:71-87); returns the
    deferred activation."""

    def __init__(self, in_channels, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.fuse = FeatureFused(norm_layer=norm_layer)
        self.block = nn.Sequential(
            nn.Conv2d(in_channels, 256, 3, padding=1, bias=False), norm_layer(256), nn.ReLU(True),
            nn.Conv2d(256, 256, 3, padding=1, bias=False), norm_layer(256), nn.ReLU(True))

    def forward(self, c2, c3, c4):
        b = self.block
        return _cbr(_cbr(self.fuse(c2, c3, c4), b[0], b[1]), b[3], b[4])


class DUpsampling(nn.Module):
    """conv_w: 1x1 to nclass * scale^2 channels, no bias; the three permute / view rounds of
    dunet.py:98-117 are  out[n, k, h*s + a, w*s + b] = conv_w(x)[n, (a*s + b)*nclass + k, h, w],
    which stays pending in a DUpLogitsView (`lazy`) or is written out as NCHW float32."""

    def __init__(self, in_channels, out_channels, scale_factor=2):
        super().__init__()
        self.scale_factor = scale_factor
        self.out_channels = out_channels
        self.conv_w = nn.Conv2d(in_channels, out_channels * scale_factor * scale_factor, 1,
                                bias=False)

    def forward(self, act, lazy=False):
        lo = F.conv_bn(act, self.conv_w).t
        return F.dup_logits(lo, self.scale_factor, self.out_channels, lazy=lazy)
