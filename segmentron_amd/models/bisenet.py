"""BiSeNet — module tree / state_dict of segmentron/models/bisenet.py:13-186, forward on the HIP
kernels.  The two attention-refinement modules and the feature fusion are one operator here,
functional.channel_gate (csrc/chan_gate.hip): the activation is pooled while its BatchNorm + ReLU
is written out, the one- or two-layer attention branch runs in float32 on the N pooled rows, and
gate, `feature += last_feature` and `feature += global_context` are one pass."""
import torch
import torch.nn as nn

from .. import functional as F
from ..modules import _ConvBNReLU
from ..modules.module import head_tail
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["BiSeNet"]


@MODEL_REGISTRY.register()
class BiSeNet(SegBaseModel):
    def __init__(self):
        super().__init__()
        self.spatial_path = SpatialPath(3, 128, norm_layer=self.norm_layer)
        self.context_path = ContextPath(norm_layer=self.norm_layer)
        # (the reference builds the fusion and the heads WITHOUT norm_layer: plain BatchNorm2d)
        self.ffm = FeatureFusion(256, 256, 4)
        self.head = _BiSeHead(256, 64, self.nclass)
        if self.aux:
            self.auxlayer1 = _BiSeHead(128, 256, self.nclass)
            self.auxlayer2 = _BiSeHead(128, 256, self.nclass)
        self.__setattr__("decoder",
                         ["spatial_path", "context_path", "ffm", "head", "auxlayer1", "auxlayer2"]
                         if self.aux else ["spatial_path", "context_path", "ffm", "head"])

    def forward(self, x):
        from .. import compute_dtype
        size = x.shape[2:]
        lazy = F.want_lazy_logits(self.training)  # see functional.LogitsView
        img = F.Act(F.image_to_nhwc(x, compute_dtype()))  # once, for both paths
        spatial = self.spatial_path(img)
        c1, c2, c3, c4 = self.encoder(img)
        N, H8, W8, _ = spatial.shape
        # torch.cat([spatial_out, context_out[-1]], 1): both producers write their channel slice
        buf = torch.empty((N, H8, W8, 256), dtype=spatial.t.dtype, device=spatial.t.device)
        sp = F.materialize(spatial, out=buf[..., :128])
        ctx1, ctx2 = self.context_path(c2, c3, c4, buf[..., 128:], fork=self.aux)
        fusion = self.ffm(F.Act(F.concat_alias(buf, [sp, ctx2[0]])))
        outputs = [F.logits_to_nchw(self.head(F.Act(fusion)), size, align_corners=True, lazy=lazy)]
        if self.aux:
            # (context_out[0] sits at the stride of c3, 16: the fused loss's 16.1x tier)
            outputs.append(F.logits_to_nchw(self.auxlayer1(F.Act(ctx1[1])), size,
                                            align_corners=True, lazy=lazy, max_scale=16.1))
            outputs.append(F.logits_to_nchw(self.auxlayer2(F.Act(ctx2[1])), size,
                                            align_corners=True, lazy=lazy))
        return tuple(outputs)


class _BiSeHead(nn.Module):
    """3x3 conv + BN + ReLU -> nn.Dropout(0.1), per element -> 1x1 classifier (bisenet.py:55-66).
    Returns NHWC logits."""

    def __init__(self, in_channels, inter_channels, nclass, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.block = nn.Sequential(
            _ConvBNReLU(in_channels, inter_channels, 3, 1, 1, norm_layer=norm_layer),
            nn.Dropout(0.1),
            nn.Conv2d(inter_channels, nclass, 1))
        self.nclass = nclass

    def forward(self, act):
        b = self.block
        return head_tail(act, b[0].conv, b[0].bn, b[1], b[2], self.training, self.nclass)


class SpatialPath(nn.Module):
    """7x7/2 -> 3x3/2 -> 3x3/2 -> 1x1, each + BN + ReLU (bisenet.py:69-86): 1/8 resolution."""

    def __init__(self, in_channels, out_channels, norm_layer=nn.BatchNorm2d):
        super().__init__()
        inter_channels = 64
        self.conv7x7 = _ConvBNReLU(in_channels, inter_channels, 7, 2, 3, norm_layer=norm_layer)
        self.conv3x3_1 = _ConvBNReLU(inter_channels, inter_channels, 3, 2, 1, norm_layer=norm_layer)
        self.conv3x3_2 = _ConvBNReLU(inter_channels, inter_channels, 3, 2, 1, norm_layer=norm_layer)
        self.conv1x1 = _ConvBNReLU(inter_channels, out_channels, 1, 1, 0, norm_layer=norm_layer)

    def forward(self, act):
        return self.conv1x1(self.conv3x3_2(self.conv3x3_1(self.conv7x7(act))))


class _GlobalAvgPooling(nn.Module):
    """gap -> 1x1 -> BN -> ReLU (bisenet.py:89-103).  The reference resizes the 1x1 map back with
    align_corners=True, which repeats it: the Act returned here stays [N,1,1,C] (float32) and is
    added as a per-image, per-channel constant (functional.channel_gate bcast_residual)."""

    def __init__(self, in_channels, out_channels, norm_layer):
        super().__init__()
        self.gap = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            nn.Conv2d(in_channels, out_channels, 1, bias=False),
            norm_layer(out_channels),
            nn.ReLU(True))

    def forward(self, act):
        a = F.conv_bn(F.Act(F.global_avg_pool_all(act, keep_fp32=True)), self.gap[1], self.gap[2])
        a.relu = True
        return a


class AttentionRefinmentModule(nn.Module):
    """3x3 conv + BN + ReLU, then x * sigmoid(conv-bn-relu(gap(x))) (bisenet.py:106-120)."""

    def __init__(self, in_channels, out_channels, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.conv3x3 = _ConvBNReLU(in_channels, out_channels, 3, 1, 1, norm_layer=norm_layer)
        self.channel_attention = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            _ConvBNReLU(out_channels, out_channels, 1, 1, 0, norm_layer=norm_layer),
            nn.Sigmoid())

    def forward(self, act, residual=None, bcast_residual=None):
        """-> plain NHWC tensor: the refined feature with ContextPath's `feature += last_feature`
        already added (residual: a plain tensor, or bcast_residual: the global context)."""
        return F.channel_gate(self.conv3x3(act), self.channel_attention[1], identity=False,
                              residual=residual, bcast_residual=bcast_residual)


class ContextPath(nn.Module):
    def __init__(self, norm_layer=nn.BatchNorm2d):
        super().__init__()
        inter_channels = 128
        self.global_context = _GlobalAvgPooling(512, inter_channels, norm_layer)
        self.arms = nn.ModuleList(
            [AttentionRefinmentModule(512, inter_channels, norm_layer),
             AttentionRefinmentModule(256, inter_channels, norm_layer)])
        self.refines = nn.ModuleList(
            [_ConvBNReLU(inter_channels, inter_channels, 3, 1, 1, norm_layer=norm_layer),
             _ConvBNReLU(inter_channels, inter_channels, 3, 1, 1, norm_layer=norm_layer)])

    def forward(self, c2, c3, c4, out, fork=False):
        """bisenet.py:139-167.  -> the two refine outputs, each materialised ONCE (the second into
        `out`, its channel slice of the fusion's concat buffer) and handed out as the pair
        (tensor for the next stage, tensor for the aux head) — aliases whose gradients meet in one
        sum when `fork`."""
        feature = self.arms[0](c4, bcast_residual=self.global_context(c4))
        last = self._up(feature, c3.shape[1:3], self.refines[0])
        ctx1 = F.fork(F.materialize(last), 2) if fork else (F.materialize(last),) * 2
        feature = self.arms[1](c3, residual=ctx1[0])
        last = self._up(feature, c2.shape[1:3], self.refines[1])
        p = F.materialize(last, out=out)
        ctx2 = F.fork(p, 2) if fork else (p, p)
        return ctx1, ctx2

    @staticmethod
    def _up(feature, hw, refine):
        """refine(F.interpolate(feature, hw, 'bilinear', align_corners=True)); the same-size
        resize (OUTPUT_STRIDE 16: c4 and c3 share a resolution) is an exact identity, skipped."""
        if tuple(feature.shape[1:3]) != tuple(hw):
            feature = F.bilinear(F.Act(feature), tuple(hw))
        return refine(F.Act(feature))


class FeatureFusion(nn.Module):
    """1x1 conv + BN + ReLU over the concat, then out + out * sigmoid(two 1x1 conv-bn-relu of
    gap(out)) (bisenet.py:170-186)."""

    def __init__(self, in_channels, out_channels, reduction=1, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.conv1x1 = _ConvBNReLU(in_channels, out_channels, 1, 1, 0, norm_layer=norm_layer)
        self.channel_attention = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            _ConvBNReLU(out_channels, out_channels // reduction, 1, 1, 0, norm_layer=norm_layer),
            _ConvBNReLU(out_channels // reduction, out_channels, 1, 1, 0, norm_layer=norm_layer),
            nn.Sigmoid())

    def forward(self, act):
        ca = self.channel_attention
        return F.channel_gate(self.conv1x1(act), lambda p: ca[2](ca[1](p)), identity=True)
