"""ContextNet ("ContextNet: Exploring Context and Detail for Semantic Segmentation in Real-time") —
module tree / state_dict of segmentron/models/contextnet.py:11-205, forward on the HIP kernels.

No backbone.  A shallow full-resolution branch (3x3 stride-2 conv WITHOUT padding + three
depthwise-separable convs, 1/8) and a deep branch on the image resized to 1/4 (3x3 stride-2 conv
without padding, twelve linear bottlenecks with t = 6, 1/32) meet in the feature fusion: the deep
map is resized to the shallow map's size, runs through a REAL depthwise 3x3 + BN + ReLU (Fast-SCNN's
`dwconv` is a 1x1), then two 1x1 + BN paths and the ReLU of their sum; the classifier is two
separable convs, nn.Dropout and a 1x1.  The resize and the depthwise 3x3 are ONE node
(functional.up_dwconv_bn on csrc/contextnet.hip): the upsampled map, 16 times the deep map's
pixels, is never stored.

Quirks kept: the stem and `Deep_net.conv_` have padding 0, the model sets no `decoder` attribute
(the optimizer takes model.parameters()), every norm is nn.BatchNorm2d whatever BN_TYPE says, the
class is spelt `Classifer`, the classifier's and the aux head's dropout is the per-element
nn.Dropout, `conv_lower_res` / `conv_higher_res` carry biases in front of a BatchNorm."""
import torch
import torch.nn as nn

from .. import functional as F
from ..config import cfg
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["ContextNet"]


def _logits(act, conv, nclass):
    """1x1 classifier (+bias) -> NHWC logits as a view of a channel-padded buffer."""
    N, H, W, _ = act.shape
    vec = 8 if act.t.dtype == torch.bfloat16 else 4
    pitch = (nclass + 2 * vec - 1) // vec * vec
    out = torch.empty((N, H, W, pitch), dtype=act.t.dtype, device=act.t.device)[..., :nclass]
    return F.conv_bn(act, conv, None, out=out).t


def _dropout(act, drop, training):
    """nn.Dropout on a deferred activation: a per-element multiplier applied while the activation
    is materialised (seg_bn_apply elem_mul)."""
    p = drop.p
    if not training or p <= 0.0:
        return act
    mask = F.dropout_mask(act.t.shape, p, act.t.dtype, act.t.device)
    return F.Act(F.materialize(act, elem_mul=mask))


@MODEL_REGISTRY.register()
class ContextNet(SegBaseModel):
    def __init__(self):
        super().__init__(need_backbone=False)
        if cfg.MODEL.BN_TYPE != "BN":
            raise NotImplementedError("ContextNet: BN_TYPE %r is not served (the reference's "
                                      "ContextNet builds nn.BatchNorm2d whatever BN_TYPE says; the "
                                      "fusion's resize + depthwise node hands its rows to a "
                                      "BatchNorm)" % cfg.MODEL.BN_TYPE)
        self.spatial_detail = Shallow_net(32, 64, 128)
        self.context_feature_extractor = Deep_net(32, [32, 32, 48, 64, 96, 128],
                                                  [1, 6, 6, 6, 6, 6], [1, 1, 3, 3, 2, 2])
        self.feature_fusion = FeatureFusionModule(128, 128, 128)
        self.classifier = Classifer(128, self.nclass)
        if self.aux:
            self.auxlayer = nn.Sequential(nn.Conv2d(128, 32, 3, padding=1, bias=False),
                                          nn.BatchNorm2d(32), nn.ReLU(True), nn.Dropout(0.1),
                                          nn.Conv2d(32, self.nclass, 1))

    def forward(self, x):
        from .. import compute_dtype
        size = x.shape[2:]
        H, W = int(size[0]), int(size[1])
        lazy = F.want_lazy_logits(self.training)
        img = F.image_to_nhwc(x, compute_dtype())
        hi = self.spatial_detail(F.Act(img))
        # F.interpolate(x, scale_factor=0.25, align_corners=True) (contextnet.py:34): floor(in / 4)
        hl, wl = H // 4, W // 4
        if hl < 1 or wl < 1:
            raise RuntimeError("Input and output sizes should be greater than 0, but got input "
                               "(H: %d, W: %d) output (H: %d, W: %d)" % (H, W, hl, wl))
        x_low = F.bilinear(F.Act(img), (hl, wl), align_corners=True)
        lo = self.context_feature_extractor(F.Act(x_low))
        y = self.classifier(self.feature_fusion(hi, lo))
        outputs = [F.logits_to_nchw(y, size, align_corners=True, lazy=lazy)]
        if self.aux:
            head = self.auxlayer
            a = F.conv_bn(hi, head[0], head[1])
            a.relu = True
            a = _dropout(a, head[3], self.training)
            outputs.append(F.logits_to_nchw(_logits(a, head[4], self.nclass), size,
                                            align_corners=True, lazy=lazy))
        return tuple(outputs)


class Custom_Conv(nn.Module):
    """conv (bias-free, padding 0 by default) -> BN -> ReLU (contextnet.py:54-64); returns a
    deferred activation."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, **kwargs):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=False),
            nn.BatchNorm2d(out_channels), nn.ReLU(True))

    def forward(self, act):
        a = F.conv_bn(act, self.conv[0], self.conv[1])
        a.relu = True
        return a


class DepthSepConv(nn.Module):
    """depthwise 3x3 -> BN -> ReLU -> 1x1 -> BN -> ReLU (contextnet.py:67-80)."""

    def __init__(self, dw_channels, out_channels, stride=1, **kwargs):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(dw_channels, dw_channels, 3, stride, 1, groups=dw_channels, bias=False),
            nn.BatchNorm2d(dw_channels), nn.ReLU(True),
            nn.Conv2d(dw_channels, out_channels, 1, bias=False),
            nn.BatchNorm2d(out_channels), nn.ReLU(True))

    def forward(self, act):
        d = F.dwconv_bn(act, self.conv[0], self.conv[1])
        d.relu = True
        p = F.conv_bn(d, self.conv[3], self.conv[4])
        p.relu = True
        return p


class DepthConv(nn.Module):
    """depthwise 3x3 -> BN -> ReLU (contextnet.py:83-93)."""

    def __init__(self, dw_channels, out_channels, stride=1, **kwargs):
        super().__init__()
        if out_channels != dw_channels:
            raise NotImplementedError("DepthConv: a channel multiplier (%d -> %d) is not on the HIP "
                                      "path" % (dw_channels, out_channels))
        self.conv = nn.Sequential(
            nn.Conv2d(dw_channels, out_channels, 3, stride, 1, groups=dw_channels, bias=False),
            nn.BatchNorm2d(out_channels), nn.ReLU(True))

    def forward(self, act):
        d = F.dwconv_bn(act, self.conv[0], self.conv[1])
        d.relu = True
        return d


class LinearBottleneck(nn.Module):
    """1x1 expand + BN + ReLU -> depthwise 3x3 + BN + ReLU -> 1x1 linear + BN (+ x)
    (contextnet.py:96-111).  The last BatchNorm stays deferred, so the NEXT block's expansion conv
    folds it into its weights (csrc/fold.hip), as modules.InvertedResidual does."""

    def __init__(self, in_channels, out_channels, t=6, stride=2, **kwargs):
        super().__init__()
        self.use_shortcut = stride == 1 and in_channels == out_channels
        self.block = nn.Sequential(
            Custom_Conv(in_channels, in_channels * t, 1),
            DepthConv(in_channels * t, in_channels * t, stride),
            nn.Conv2d(in_channels * t, out_channels, 1, bias=False),
            nn.BatchNorm2d(out_channels))

    def forward(self, x):
        b = self.block
        a = F.conv_bn(b[1](b[0](x)), b[2], b[3])
        if self.use_shortcut:
            return F.Act(F.materialize(a, residual=x))
        return a


class Shallow_net(nn.Module):
    def __init__(self, dw_channels1=32, dw_channels2=64, out_channels=128, **kwargs):
        super().__init__()
        self.conv = Custom_Conv(3, dw_channels1, 3, 2)
        self.dsconv1 = DepthSepConv(dw_channels1, dw_channels2, 2)
        self.dsconv2 = DepthSepConv(dw_channels2, out_channels, 2)
        self.dsconv3 = DepthSepConv(out_channels, out_channels, 1)

    def forward(self, act):
        return self.dsconv3(self.dsconv2(self.dsconv1(self.conv(act))))


class Deep_net(nn.Module):
    def __init__(self, in_channels, block_channels, t, num_blocks, **kwargs):
        super().__init__()
        self.block_channels = block_channels
        self.t = t
        self.num_blocks = num_blocks
        self.conv_ = Custom_Conv(3, in_channels, 3, 2)
        chans = [in_channels] + list(block_channels)
        strides = [1, 1, 2, 2, 1, 1]
        for i in range(6):
            setattr(self, "bottleneck%d" % (i + 1),
                    self._layer(LinearBottleneck, chans[i], chans[i + 1], num_blocks[i], t[i],
                                strides[i]))

    def _layer(self, block, in_channels, out_channels, blocks, t, stride):
        layers = [block(in_channels, out_channels, t, stride)]
        for _ in range(1, blocks):
            layers.append(block(out_channels, out_channels, t, 1))
        return nn.Sequential(*layers)

    def forward(self, a):
        a = self.conv_(a)
        for i in range(6):
            for m in getattr(self, "bottleneck%d" % (i + 1)):
                a = m(a)
        return a


class FeatureFusionModule(nn.Module):
    def __init__(self, highter_in_channels, lower_in_channels, out_channels, scale_factor=4,
                 **kwargs):
        super().__init__()
        self.scale_factor = scale_factor
        self.dwconv = DepthConv(lower_in_channels, out_channels, 1)
        self.conv_lower_res = nn.Sequential(nn.Conv2d(out_channels, out_channels, 1),
                                            nn.BatchNorm2d(out_channels))
        self.conv_higher_res = nn.Sequential(nn.Conv2d(highter_in_channels, out_channels, 1),
                                             nn.BatchNorm2d(out_channels))
        self.relu = nn.ReLU(True)

    def forward(self, hi, lo):
        """hi: the 1/8 activation, lo: the 1/32 one (its last BatchNorm pending).  The resize to
        hi's size and the depthwise 3x3 behind it are one node; the biases of the two 1x1
        convolutions go into their BatchNorms' mean offsets (functional.conv_bn)."""
        dw = self.dwconv.conv
        up = F.up_dwconv_bn(lo, tuple(hi.shape[1:3]), dw[0], dw[1])
        up.relu = True
        up = F.conv_bn(up, self.conv_lower_res[0], self.conv_lower_res[1])
        hr = F.conv_bn(hi, self.conv_higher_res[0], self.conv_higher_res[1])
        return F.Act(F.materialize(hr, residual=up, post_relu=True))


class Classifer(nn.Module):
    def __init__(self, dw_channels, num_classes, stride=1, **kwargs):
        super().__init__()
        self.dsconv1 = DepthSepConv(dw_channels, dw_channels, stride)
        self.dsconv2 = DepthSepConv(dw_channels, dw_channels, stride)
        self.conv = nn.Sequential(nn.Dropout(0.1), nn.Conv2d(dw_channels, num_classes, 1))
        self.num_classes = num_classes

    def forward(self, act):
        a = self.dsconv2(self.dsconv1(act))
        a = _dropout(a, self.conv[0], self.training)
        return _logits(a, self.conv[1], self.num_classes)
