"""ESPNetv2 ("A Light-weight, Power Efficient, and General Purpose Convolutional Neural Network") —
module tree / state_dict of segmentron/models/espnetv2.py:12-75, forward on the HIP kernels.

The EESPNet backbone (models/backbones/eespnet.py) hands over its four levels; the decoder
projects level 4, resizes it next to level 3, runs one more EESP unit and a pyramid-pooling module
(four cascaded 3x3 / stride-2 average pools, each followed by a depthwise 3x3 and a resize back),
and climbs to 1/2 resolution through two concat-and-project steps.

Every concat is one buffer whose producers write their channel slices (the backbone's last kernels
included); nothing is copied.  The nclass-channel maps (19 on Cityscapes) live in zero-padded
buffers of round_up8(nclass) channels, so `64 + 19` and `32 + 19` are 88- and 56-channel buffers
and the convolutions that read them take the padded width (their packed weights are zero there),
as CGNet's 35- and 131-channel concats do."""
import torch
import torch.nn as nn

from .. import functional as F
from ..hip_ops import round_up8, vec_of
from ..modules import EESP, _BNPReLU, _ConvBNPReLU
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["ESPNetV2"]


@MODEL_REGISTRY.register()
class ESPNetV2(SegBaseModel):
    def __init__(self, **kwargs):
        super().__init__()
        self.proj_L4_C = _ConvBNPReLU(256, 128, 1, **kwargs)
        self.pspMod = nn.Sequential(
            EESP(256, 128, stride=1, k=4, r_lim=7, **kwargs),
            _PSPModule(128, 128, **kwargs))
        self.project_l3 = nn.Sequential(
            nn.Dropout2d(0.1),
            nn.Conv2d(128, self.nclass, 1, bias=False))
        self.act_l3 = _BNPReLU(self.nclass, **kwargs)
        self.project_l2 = _ConvBNPReLU(64 + self.nclass, self.nclass, 1, **kwargs)
        self.project_l1 = nn.Sequential(
            nn.Dropout2d(0.1),
            nn.Conv2d(32 + self.nclass, self.nclass, 1, bias=False))

        self.__setattr__("exclusive", ["proj_L4_C", "pspMod", "project_l3", "act_l3", "project_l2",
                                       "project_l1"])

    @staticmethod
    def _dropped(drop, t, training):
        """nn.Dropout2d: a per-(image, channel) multiplier (seg_bn_apply chan_mul)."""
        if not (training and drop.p > 0.0):
            return t
        N, C = t.shape[0], t.shape[-1]
        mul = (torch.rand((N, C), device=t.device) >= drop.p).float() / (1.0 - drop.p)
        return F.materialize(F.Act(t), chan_mul=mul)

    def _narrow(self, t, conv, pitch=None):
        """Bias-free 1x1 convolution to nclass channels -> the raw NHWC map as the nclass leading
        channels of a zeroed buffer of `pitch` (default round_up8(nclass)) channels."""
        N, H, W, _ = t.shape
        buf = torch.zeros((N, H, W, pitch or round_up8(self.nclass)), dtype=t.dtype,
                          device=t.device)
        a = F.conv_bn(F.Act(t), conv, None, out=buf[..., :self.nclass])
        return F.concat_alias(buf, [a.t])

    def forward(self, x):
        size = x.shape[2:]
        nc, cp = self.nclass, round_up8(self.nclass)
        if size[0] % 16 != 0 or size[1] % 16 != 0:
            raise ValueError("ESPNetv2 takes input sizes that are multiples of 16, got %s"
                             % (tuple(size),))
        from .. import compute_dtype
        dt = compute_dtype()
        N = x.shape[0]
        (H2, W2), (H4, W4), (H8, W8) = [(size[0] >> s, size[1] >> s) for s in (1, 2, 3)]

        def buffer(H, W, C):
            return torch.empty((N, H, W, C), dtype=dt, device=x.device)
        buf1 = buffer(H2, W2, 32 + cp)    # cat([out_l1, out_up_l2])
        buf2 = buffer(H4, W4, 64 + cp)    # cat([out_l2, out_up_l3])
        buf3 = buffer(H8, W8, 256)        # cat([out_l3, up_l4_to_l3])
        out_l1, out_l2, out_l3, out_l4 = self.encoder(
            x, seg=True, outs=(buf1[..., :32], buf2[..., :64], buf3[..., :128]))

        out_l4_proj = self.proj_L4_C(F.Act(out_l4))
        up_l4_to_l3 = F.bilinear(F.Act(out_l4_proj), (H8, W8), out=buf3[..., 128:])
        psp = self.pspMod[1]
        pbuf = psp.buffer(buf3)
        e = self.pspMod[0](F.concat_alias(buf3, [out_l3, up_l4_to_l3]), out=pbuf[..., :128])
        merged_l3_upl4 = psp(e, pbuf)

        bef_act = self._narrow(self._dropped(self.project_l3[0], merged_l3_upl4, self.training),
                               self.project_l3[1])
        aux_in = None
        if self.aux:
            bef_act, aux_in = F.fork(bef_act, 2)
        proj_merge_l3 = self.act_l3(bef_act)
        out_up_l3 = F.bilinear(F.Act(proj_merge_l3), (H4, W4), out=buf2[..., 64:])
        # project_l2: conv to nclass + BN + PReLU on the 88-channel concat
        m = self.project_l2
        mbuf = torch.zeros((N, H4, W4, cp), dtype=dt, device=x.device)
        a = F.conv_bn(F.Act(F.concat_alias(buf2, [out_l2, out_up_l3])), m.conv, m.bn,
                      out=mbuf[..., :nc])
        merge_l2 = F.bn_prelu(F.Act(F.concat_alias(mbuf, [a.t]), a.bn), m.prelu)
        out_up_l2 = F.bilinear(F.Act(merge_l2), (H2, W2), out=buf1[..., 32:])
        cat1 = self._dropped(self.project_l1[0], F.concat_alias(buf1, [out_l1, out_up_l2]),
                             self.training)
        vec = vec_of(dt)
        merge_l1 = self._narrow(cat1, self.project_l1[1], (nc + 2 * vec - 1) // vec * vec)

        lazy = F.want_lazy_logits(self.training)
        outputs = [F.logits_to_nchw(merge_l1[..., :nc], size, align_corners=True, lazy=lazy)]
        if self.aux:
            # (different from the paper, as the reference notes: the level-3 map before its BN)
            outputs.append(F.logits_to_nchw(aux_in[..., :nc], size, align_corners=True, lazy=lazy))
        return tuple(outputs)


class _PSPModule(nn.Module):
    """espnetv2.py:63-75 (different from PSPNet's): x next to four maps, each the depthwise 3x3 of
    x pooled once more (3x3 / stride 2, cascaded) resized back, then a 1x1 projection + BN + PReLU.
    The stages have no BatchNorm; every resize writes its slice of the concat buffer."""

    def __init__(self, in_channels, out_channels=1024, sizes=(1, 2, 4, 8), **kwargs):
        super().__init__()
        self.stages = nn.ModuleList(
            [nn.Conv2d(in_channels, in_channels, 3, 1, 1, groups=in_channels, bias=False)
             for _ in sizes])
        self.project = _ConvBNPReLU(in_channels * (len(sizes) + 1), out_channels, 1, 1, **kwargs)

    def buffer(self, like):
        """The concat buffer; the producer of x writes its first in_channels channels."""
        C = self.stages[0].in_channels
        N, H, W, _ = like.shape
        return torch.empty((N, H, W, C * (len(self.stages) + 1)), dtype=like.dtype,
                           device=like.device)

    def forward(self, x, buf):
        N, H, W, C = x.shape
        x0, t = F.fork(x, 2)
        feats = [x0]
        for i, stage in enumerate(self.stages):
            t = F.avg_pool3x3s2(t)  # (cascaded: each pool feeds its stage and the next pool)
            a, t = F.fork(t, 2) if i < len(self.stages) - 1 else (t, None)
            s = F.dwconv_plain(F.Act(a), stage)
            feats.append(F.bilinear(F.Act(s), (H, W), out=buf[..., (i + 1) * C:(i + 2) * C]))
        return self.project(F.Act(F.concat_alias(buf, feats)))
