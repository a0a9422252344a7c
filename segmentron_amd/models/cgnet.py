"""CGNet ("A Light-weight Context Guided Network for Semantic Segmentation") — module tree /
state_dict of segmentron/models/cgnet.py:13-181, forward on the HIP kernels.

No backbone.  Three 3x3 conv + BN + PReLU at 1/2 resolution, then 3 + 21 ContextGuidedBlocks at
1/4 and 1/8: 1x1 (or 3x3 stride-2) conv + BN + PReLU, a local and a surrounding (dilated)
depthwise 3x3 over the same tensor, BN + PReLU over their concat, and a squeeze-and-gate with two
Linear layers (`_FGlo`) plus the block's residual.  Here the two depthwise convolutions are one
launch (functional.cg_joint_bn, csrc/cgnet.hip), BN + PReLU is written out once and pooled for the
gate in the same pass (functional.bn_prelu), and gate + residual are one pass (csrc/chan_gate.hip).

The stage concats have 35 and 131 channels (32 resp. 128 features + the 3-channel image pooled
down): they live in buffers of 40 and 136 channels whose pad channels hold zeros; the convolution
that reads them takes the padded width (its packed weights are zero there).  Every producer writes
its channel slice of the buffer; nothing is copied."""
import torch
import torch.nn as nn
import torch.nn.functional as TF

from .. import functional as F
from ..config import cfg
from ..hip_ops import round_up8, vec_of
from ..modules import _BNPReLU, _ConvBNPReLU
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["CGNet"]


@MODEL_REGISTRY.register()
class CGNet(SegBaseModel):
    def __init__(self):
        super().__init__(need_backbone=False)
        stage2_block_num = cfg.MODEL.CGNET.STAGE2_BLOCK_NUM
        stage3_block_num = cfg.MODEL.CGNET.STAGE3_BLOCK_NUM
        if stage2_block_num < 2 or stage3_block_num < 2:
            # (the reference's forward reads the last block's output: it needs one)
            raise ValueError("CGNet needs STAGE2_BLOCK_NUM and STAGE3_BLOCK_NUM >= 2")
        self.stage1_0 = _ConvBNPReLU(3, 32, 3, 2, 1, norm_layer=self.norm_layer)
        self.stage1_1 = _ConvBNPReLU(32, 32, 3, 1, 1, norm_layer=self.norm_layer)
        self.stage1_2 = _ConvBNPReLU(32, 32, 3, 1, 1, norm_layer=self.norm_layer)

        self.sample1 = _InputInjection(1)
        self.sample2 = _InputInjection(2)
        self.bn_prelu1 = _BNPReLU(32 + 3, norm_layer=self.norm_layer)

        self.stage2_0 = ContextGuidedBlock(32 + 3, 64, dilation=2, reduction=8, down=True,
                                           residual=False, norm_layer=self.norm_layer)
        self.stage2 = nn.ModuleList()
        for _ in range(0, stage2_block_num - 1):
            self.stage2.append(ContextGuidedBlock(64, 64, dilation=2, reduction=8,
                                                  norm_layer=self.norm_layer))
        self.bn_prelu2 = _BNPReLU(128 + 3, norm_layer=self.norm_layer)

        self.stage3_0 = ContextGuidedBlock(128 + 3, 128, dilation=4, reduction=16, down=True,
                                           residual=False, norm_layer=self.norm_layer)
        self.stage3 = nn.ModuleList()
        for _ in range(0, stage3_block_num - 1):
            self.stage3.append(ContextGuidedBlock(128, 128, dilation=4, reduction=16,
                                                  norm_layer=self.norm_layer))
        self.bn_prelu3 = _BNPReLU(256, norm_layer=self.norm_layer)

        self.head = nn.Sequential(
            nn.Dropout2d(0.1, False),
            nn.Conv2d(256, self.nclass, 1))

        self.__setattr__("decoder", ["stage1_0", "stage1_1", "stage1_2", "sample1", "sample2",
                                     "bn_prelu1", "stage2_0", "stage2", "bn_prelu2", "stage3_0",
                                     "stage3", "bn_prelu3", "head"])

    @staticmethod
    def _buffer(like, H, W, C):
        return torch.empty((like.shape[0], H, W, round_up8(C)), dtype=like.dtype,
                           device=like.device)

    def forward(self, x):
        from .. import compute_dtype
        size = x.shape[2:]
        dt = compute_dtype()
        img = F.Act(F.image_to_nhwc(x, dt))
        # the pooled image goes into the concat buffers first (torch's in-place copies, before
        # any autograd node holds a view of them); the producers then write their channel slices
        inp1 = self.sample1(x)
        inp2 = self.sample2(inp1, first=1)
        (H2, W2), (H4, W4) = inp1.shape[2:], inp2.shape[2:]
        buf1 = self._buffer(img.t, H2, W2, 32 + 3)
        buf2 = self._buffer(img.t, H4, W4, 128 + 3)
        _inject(buf1, 32, inp1)
        _inject(buf2, 128, inp2)

        # stage 1; its last layer writes channels 0..31 of cat([out0, inp1])
        t = self.stage1_1(F.Act(self.stage1_0(img)))
        o = self.stage1_2(F.Act(t), out=buf1[..., :32])
        out0_cat = self.bn_prelu1(F.concat_alias(buf1, [o]))

        # stage 2: cat([out1, out1_0, inp2])
        out1_0 = self.stage2_0(out0_cat, out=buf2[..., 64:128])
        a, b = F.fork(out1_0, 2)
        out1 = self._blocks(self.stage2, a, buf2[..., :64])
        out1_cat = self.bn_prelu2(F.concat_alias(buf2, [out1, b]))

        # stage 3: cat([out2_0, out2])
        H8, W8 = (H4 + 1) // 2, (W4 + 1) // 2
        buf3 = self._buffer(t, H8, W8, 256)
        out2_0 = self.stage3_0(out1_cat, out=buf3[..., :128])
        a, b = F.fork(out2_0, 2)
        out2 = self._blocks(self.stage3, a, buf3[..., 128:])
        out2_cat = self.bn_prelu3(F.concat_alias(buf3, [b, out2]))

        lo = self._head(F.Act(out2_cat))
        return (F.logits_to_nchw(lo, size, align_corners=True,
                                 lazy=F.want_lazy_logits(self.training)),)

    @staticmethod
    def _blocks(blocks, x, out):
        for i, layer in enumerate(blocks):
            x = layer(x, out=out if i == len(blocks) - 1 else None)
        return x

    def _head(self, act):
        """nn.Dropout2d (a per-(image, channel) multiplier, seg_bn_apply chan_mul) -> the biased
        1x1 classifier; returns channel-padded NHWC logits.

        The classifier runs in float32 in every compute dtype (256 -> 19 channels at 1/8
        resolution: a float32 GEMM of 0.4 GFLOP).  Measured on the training fixture with the
        float64 oracle (tests/_cgnet_oracle.py): rounding THIS ONE weight tensor to bf16 moves the
        loss by 6.8e-4 relative, the image, every other convolution weight and (on the device) every
        stored activation together by about 1e-4 — the bf16 step would be as far from float64 as
        its classifier weights' rounding and no nearer."""
        drop, conv = self.head[0], self.head[1]
        if self.training and drop.p > 0.0:
            N, C = act.shape[0], act.shape[-1]
            mul = (torch.rand((N, C), device=act.t.device) >= drop.p).float() / (1.0 - drop.p)
            act = F.Act(F.materialize(act, chan_mul=mul))
        if act.t.dtype != torch.float32:
            act = F.Act(act.t.float())
        N, H, W, _ = act.shape
        vec = vec_of(act.t.dtype)
        pitch = (self.nclass + 2 * vec - 1) // vec * vec
        out = torch.empty((N, H, W, pitch), dtype=act.t.dtype, device=act.t.device)
        return F.conv_bn(act, conv, None, out=out[..., :self.nclass]).t


def _inject(buf, c0, inp):
    """The pooled float32 NCHW image `inp` -> channels c0 .. c0+2 of the NHWC concat buffer, zeros
    up to the buffer's width (the BatchNorm and the convolution behind it read the pad channels).
    Three channels that need no gradient: data movement, not a hot path."""
    nhwc = F.image_to_nhwc(inp, buf.dtype)  # [N, H, W, vec], zeros beyond channel 2
    v = nhwc.shape[-1]
    buf[..., c0:c0 + v].copy_(nhwc)
    if c0 + v < buf.shape[-1]:
        buf[..., c0 + v:].zero_()


class _ChannelWiseConv(nn.Module):
    """Parameter container (cgnet.py:96-103): the depthwise 3x3 runs inside
    functional.cg_joint_bn together with its sibling."""

    def __init__(self, in_channels, out_channels, dilation=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, 3, 1, dilation, dilation,
                              groups=in_channels, bias=False)

    def forward(self, act):
        return F.dwconv_bn(act, self.conv, None)


class _FGlo(nn.Module):
    """x * sigmoid(Linear(ReLU(Linear(gap(x))))) (cgnet.py:106-120).  The two Linear layers act on
    the N pooled float32 rows with hidden width C / reduction (8): element-wise products and row
    sums in float32 under autograd — no BLAS call, safe inside a HIP-graph capture; the gate itself
    (and the block's residual) is functional.gate."""

    def __init__(self, in_channels, reduction=16):
        super().__init__()
        self.gap = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(
            nn.Linear(in_channels, in_channels // reduction),
            nn.ReLU(True),
            nn.Linear(in_channels // reduction, in_channels),
            nn.Sigmoid())

    def logits(self, pooled):
        """pooled float32 [N,1,1,C] -> the pre-sigmoid gate [N,1,1,C]."""
        N, C = pooled.shape[0], pooled.shape[-1]
        l1, l2 = self.fc[0], self.fc[2]
        p = pooled.reshape(N, 1, C).float()
        h = torch.relu((p * l1.weight.unsqueeze(0)).sum(-1) + l1.bias)
        a = (h.unsqueeze(1) * l2.weight.unsqueeze(0)).sum(-1) + l2.bias
        return a.view(N, 1, 1, C)

    def forward(self, x, pooled=None, residual=None, out=None):
        if pooled is None:
            pooled = F.global_avg_pool_all(F.Act(x), keep_fp32=True)
        return F.gate(x, self.logits(pooled), residual=residual, out=out)


class _InputInjection(nn.Module):
    """`ratio` times nn.AvgPool2d(3, 2, 1) of the float32 NCHW image (cgnet.py:123-133): three
    channels without gradient, on torch's own pooling.  `first`: the pools before it were already
    applied (sample2 continues from sample1's output: the same arithmetic, once)."""

    def __init__(self, ratio):
        super().__init__()
        self.pool = nn.ModuleList()
        for _ in range(0, ratio):
            self.pool.append(nn.AvgPool2d(3, 2, 1))

    def forward(self, x, first=0):
        x = x.float()
        for pool in list(self.pool)[first:]:
            x = TF.avg_pool2d(x, pool.kernel_size, pool.stride, pool.padding)
        return x


class _ConcatInjection(nn.Module):
    """BN + PReLU over cat([x1, x2]) (cgnet.py:136-146; the reference defines and never uses it).
    x: the concat, already in one buffer."""

    def __init__(self, in_channels, norm_layer=nn.BatchNorm2d, **kwargs):
        super().__init__()
        self.bn = norm_layer(in_channels)
        self.prelu = nn.PReLU(in_channels)

    def forward(self, x):
        return F.bn_prelu(F.bn_of_concat(x, self.bn, self.prelu.weight.numel()), self.prelu)


class ContextGuidedBlock(nn.Module):
    """cgnet.py:149-181.  x: plain NHWC tensor (for the two down blocks: the stage concat at its
    padded width); returns the plain NHWC output, written into `out` where given."""

    def __init__(self, in_channels, out_channels, dilation=2, reduction=16, down=False,
                 residual=True, norm_layer=nn.BatchNorm2d):
        super().__init__()
        inter_channels = out_channels // 2 if not down else out_channels
        if down:
            self.conv = _ConvBNPReLU(in_channels, inter_channels, 3, 2, 1, norm_layer=norm_layer)
            self.reduce = nn.Conv2d(inter_channels * 2, out_channels, 1, bias=False)
        else:
            self.conv = _ConvBNPReLU(in_channels, inter_channels, 1, 1, 0, norm_layer=norm_layer)
        self.f_loc = _ChannelWiseConv(inter_channels, inter_channels)
        self.f_sur = _ChannelWiseConv(inter_channels, inter_channels, dilation)
        self.bn = norm_layer(inter_channels * 2)
        self.prelu = nn.PReLU(inter_channels * 2)
        self.f_glo = _FGlo(out_channels, reduction)
        self.down = down
        self.residual = residual

    def forward(self, x, out=None):
        res = None
        if self.residual:
            x, res = F.fork(x, 2)
        t = self.conv(F.Act(x))
        joi = F.cg_joint_bn(t, self.f_loc.conv, self.f_sur.conv, self.bn)
        if self.down:
            y = F.conv_bn(F.Act(F.bn_prelu(joi, self.prelu)), self.reduce).t
            return self.f_glo(y, residual=res, out=out)
        y, pooled = F.bn_prelu(joi, self.prelu, pool=True)
        return self.f_glo(y, pooled=pooled, residual=res, out=out)
