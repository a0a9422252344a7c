"""EDANet ("Efficient Dense Modules of Asymmetric Convolution for Real-Time Semantic Segmentation")
— module tree / state_dict of segmentron/models/edanet.py:13-142, forward on the HIP kernels.

No backbone.  Three stride-2 down-samplings and two stages of dense blocks (5 blocks from 60 to 260
channels at 1/4 resolution, 8 blocks from 130 to 450 at 1/8).  An EDABlock is a biased 1x1
convolution to k = 40 channels and two pairs of biased factorised 3-tap convolutions
((3,1) -> (1,3), the second pair dilated up to 16), each group followed by BatchNorm + ReLU; its
output is `cat([new 40 channels, input], 1)`.

Here a stage lives in ONE NHWC buffer of round_up8(final width) channels (264 / 456, pad channels
zero) with the stage's input at the back: block j reads the channel suffix buf[..., off_j:] and
writes its 40 channels directly in front of it, so every block output is again a suffix and
torch.cat never runs.  Segments are stored activated (the block's last BatchNorm + ReLU and the
Dropout2d multiplier are one apply pass into the slice), the inner BatchNorms + ReLU ride in the
next line convolution's prologue.  The 52 line convolutions run on csrc/conv_line.hip at C = 40
(functional.line_pair_bn: two line_conv_bn launches per pair — the first bias is added by the
kernel, every bias in front of a BatchNorm is dropped as conv_bn does — or one launch of
csrc/conv_line_pair.hip for the classes where that measured faster).  In backward a stage has one gradient buffer of the same
layout: block j reads its own 40 channels of it and its 1x1 convolution's data-gradient GEMM adds
into the suffix behind them in place (functional.DenseGrad).

The reference fails for inputs whose height or width is not divisible by 8 (the stride-2
convolution rounds up, the 2x2 pool down, and their torch.cat raises); forward says so first."""
import torch
import torch.nn as nn

from .. import functional as F
from ..config import cfg
from ..hip_ops import round_up8, vec_of
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["EDANet"]

K_GROWTH = 40


@MODEL_REGISTRY.register()
class EDANet(SegBaseModel):
    def __init__(self):
        super().__init__(need_backbone=False)
        if cfg.MODEL.BN_TYPE != "BN":
            raise NotImplementedError("EDANet: BN_TYPE %r is not served (the line convolutions "
                                      "hand their statistics to a BatchNorm)" % cfg.MODEL.BN_TYPE)
        self.layers = nn.ModuleList()
        self.dilation1 = [1, 1, 1, 2, 2]
        self.dilation2 = [2, 2, 4, 4, 8, 8, 16, 16]
        self.layers.append(DownsamplerBlock(3, 15))
        self.layers.append(DownsamplerBlock(15, 60))
        for i in range(5):
            self.layers.append(EDABlock(60 + K_GROWTH * i, self.dilation1[i]))
        self.layers.append(DownsamplerBlock(260, 130))
        for j in range(8):
            self.layers.append(EDABlock(130 + K_GROWTH * j, self.dilation2[j]))
        self.project_layer = nn.Conv2d(450, self.nclass, kernel_size=1)
        self.weights_init()

    def weights_init(self):
        for m in self.modules():
            classname = m.__class__.__name__
            if classname.find("Conv") != -1:
                m.weight.data.normal_(0.0, 0.02)
            elif classname.find("BatchNorm") != -1:
                m.weight.data.normal_(1.0, 0.02)
                m.bias.data.fill_(0)

    @staticmethod
    def _stage(blocks, down, x):
        """One dense stage: `down` writes its activated output at the back of the stage buffer,
        the blocks grow it towards channel 0.  -> the whole buffer (plain, pad channels zero)."""
        N, H, W, _ = x.shape
        cin = down.noutput
        width = cin + K_GROWTH * len(blocks)
        buf = torch.empty((N, H // 2, W // 2, round_up8(width)), dtype=x.dtype, device=x.device)
        off = width - cin
        # (the pad behind the input segment is written with it, as zeros, once)
        t = down(x, out=buf[..., off:])
        for blk in blocks:
            t = blk(t, buf, off)
            off -= K_GROWTH
        return t

    def forward(self, x):
        from .. import compute_dtype
        size = x.shape[2:]
        if size[0] % 8 or size[1] % 8:
            raise ValueError("EDANet: the input size %s is not divisible by 8 (each "
                             "DownsamplerBlock concatenates a stride-2 convolution, which rounds "
                             "up, with a 2x2 max-pool, which rounds down)" % (tuple(size),))
        t = F.image_to_nhwc(x, compute_dtype())
        t = self.layers[0](t)
        t = self._stage(self.layers[2:7], self.layers[1], t)
        t = self._stage(self.layers[8:16], self.layers[7], t)
        lo = self._project(t)
        return (F.logits_to_nchw(lo, size, align_corners=True,
                                 lazy=F.want_lazy_logits(self.training)),)

    def _project(self, t):
        """The biased 450 -> nclass projection on the stage buffer (456 channels: the packed
        weight carries zero columns for the pad), in float32 in every compute dtype as CGNet's
        classifier; returns channel-padded NHWC logits."""
        if t.dtype != torch.float32:
            t = t.float()
        N, H, W, _ = t.shape
        vec = vec_of(t.dtype)
        pitch = (self.nclass + 2 * vec - 1) // vec * vec
        out = torch.empty((N, H, W, pitch), dtype=t.dtype, device=t.device)
        return F.conv_bn(F.Act(t), self.project_layer, None, out=out[..., :self.nclass]).t


class DownsamplerBlock(nn.Module):
    """edanet.py:73-97: 3x3 / stride 2 convolution [next to MaxPool2d(2, 2) of the same input,
    concatenated], BatchNorm, ReLU.  x: plain NHWC whose channels beyond `ninput` are zero;
    returns the plain activated output, round_up8(noutput) channels wide with zeros in the pad,
    written into `out` where given."""

    def __init__(self, ninput, noutput):
        super().__init__()
        self.ninput = ninput
        self.noutput = noutput
        if self.ninput < self.noutput:
            self.conv = nn.Conv2d(ninput, noutput - ninput, kernel_size=3, stride=2, padding=1)
            self.pool = nn.MaxPool2d(2, stride=2)
        else:
            self.conv = nn.Conv2d(ninput, noutput, kernel_size=3, stride=2, padding=1)
        self.bn = nn.BatchNorm2d(noutput)

    def forward(self, x, out=None):
        N, H, W, _ = x.shape
        cout, cp = self.noutput, round_up8(self.noutput)
        buf = torch.empty((N, H // 2, W // 2, cp), dtype=x.dtype, device=x.device)
        if cp > cout:
            buf[..., cout:].zero_()
        if self.ninput < self.noutput:
            # the convolution (its bias kept: no BatchNorm of its own) and the pooled input fill
            # one buffer; the BatchNorm takes its statistics from that buffer in one pass
            nc = cout - self.ninput
            a, b = F.fork(x, 2)
            y1 = F.conv_bn(F.Act(a), self.conv, None, out=buf[..., :nc]).t
            y2 = F.place(F.max_pool(F.Act(b), 2, 2, 0), self.ninput, buf[..., nc:cout])
            act = F.bn_of_concat(F.concat_alias(buf, [y1, y2]), self.bn, cout)
        else:
            a = F.conv_bn(F.Act(x), self.conv, self.bn, out=buf[..., :cout])
            act = F.Act(F.concat_alias(buf, [a.t]), a.bn)
        # zero-padded BatchNorm: scale = shift = 0 in the pad, which stays zero through the ReLU
        return F.materialize(F.Act(act.t, F._pad_bn(act.bn, cp), F.RELU), out=out)


class EDABlock(nn.Module):
    """edanet.py:100-142.  x: the plain suffix buf[..., off:] of the stage buffer; writes the 40
    new activated channels to buf[..., off-40:off] and returns the suffix buf[..., off-40:]."""

    def __init__(self, ninput, dilated, k=K_GROWTH, dropprob=0.02):
        super().__init__()
        self.conv1x1 = nn.Conv2d(ninput, k, kernel_size=1)
        self.bn0 = nn.BatchNorm2d(k)
        self.conv3x1_1 = nn.Conv2d(k, k, kernel_size=(3, 1), padding=(1, 0))
        self.conv1x3_1 = nn.Conv2d(k, k, kernel_size=(1, 3), padding=(0, 1))
        self.bn1 = nn.BatchNorm2d(k)
        self.conv3x1_2 = nn.Conv2d(k, k, (3, 1), stride=1, padding=(dilated, 0), dilation=dilated)
        self.conv1x3_2 = nn.Conv2d(k, k, (1, 3), stride=1, padding=(0, dilated), dilation=dilated)
        self.bn2 = nn.BatchNorm2d(k)
        self.dropout = nn.Dropout2d(dropprob)

    @staticmethod
    def _pair(act, conv_a, conv_b, bn):
        """(3,1) -> (1,3) with nothing but the first bias in between: one launch or two
        (functional.line_pair_bn)."""
        a = F.line_pair_bn(act, conv_a, conv_b, bn)
        a.relu = True
        return a

    def forward(self, x, buf, off):
        k = self.conv1x1.out_channels
        dg = F.DenseGrad() if torch.is_grad_enabled() and x.requires_grad else None
        a = F.conv_bn(F.Act(x), self.conv1x1, self.bn0, fork=dg)
        a.relu = True
        a = self._pair(a, self.conv3x1_1, self.conv1x3_1, self.bn1)
        a = self._pair(a, self.conv3x1_2, self.conv1x3_2, self.bn2)
        mul = None
        if self.training and self.dropout.p != 0:
            # nn.Dropout2d: one multiplier per (image, channel), applied by the write-out pass
            p = self.dropout.p
            mul = (torch.rand((x.shape[0], k), device=x.device) >= p).float() / (1.0 - p)
        new = F.materialize(a, chan_mul=mul, out=buf[..., off - k:off])
        return F.dense_cat(new, x, buf, off - k, dg)
