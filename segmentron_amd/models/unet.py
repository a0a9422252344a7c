"""UNet ("U-Net: Convolutional Networks for Biomedical Image Segmentation") — module tree /
state_dict of segmentron/models/unet.py:13-130, forward on the HIP kernels.

No backbone.  Five levels of (3x3 convolution, BatchNorm, ReLU) x 2 at 64, 128, 256, 512 and 512
channels, a 2x2 max-pool between them; four decoder steps that resize the deeper map by 2
(align_corners=True), pad it to the skip's size, concatenate [skip, up] and run another double
convolution; a biased 1x1 projection to the classes.  Every convolution is a dense 3x3 (or the
final 1x1) on the MFMA implicit GEMM; a convolution's bias in front of a training BatchNorm is
dropped and handed to the statistics as the mean offset (functional.conv_bn).

Each encoder level's raw output is consumed twice.  ONE node (functional.skip_pool on
csrc/unet.hip) reads it once: the activated skip is written straight into channels [0, C) of the
level's concat buffer [N, H_l, W_l, 2C], the pooled map is handed on.  The decoder's resize writes
channels [C, 2C) of the same buffer — with a destination window where the level's size is odd
(functional.bilinear_placed) — and the two slices are joined without a copy
(functional.concat_alias)."""
import torch
import torch.nn as nn

from .. import functional as F
from ..config import cfg
from ..hip_ops import vec_of
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["UNet"]

MIN_SIZE = 16  # four 2x2 pools: the deepest one must still see a 2 x 2 map


@MODEL_REGISTRY.register()
class UNet(SegBaseModel):
    def __init__(self):
        super().__init__(need_backbone=False)
        if cfg.MODEL.BN_TYPE != "BN":
            raise NotImplementedError("UNet: BN_TYPE %r is not served (the reference's UNet builds "
                                      "nn.BatchNorm2d whatever BN_TYPE says; the skip + max-pool "
                                      "node hands its rows to a BatchNorm)" % cfg.MODEL.BN_TYPE)
        self.inc = DoubleConv(3, 64)
        self.down1 = Down(64, 128)
        self.down2 = Down(128, 256)
        self.down3 = Down(256, 512)
        self.down4 = Down(512, 512)
        self.head = _UNetHead(self.nclass)
        self.__setattr__("decoder", ["head", "auxlayer"] if self.aux else ["head"])

    def forward(self, x):
        from .. import compute_dtype
        H, W = x.shape[2:]
        if H < MIN_SIZE or W < MIN_SIZE:
            raise NotImplementedError("UNet: a %d x %d input is smaller than %d in an axis (the "
                                      "deepest 2x2 max-pool would see less than a 2 x 2 map)"
                                      % (H, W, MIN_SIZE))
        t = F.image_to_nhwc(x, compute_dtype())
        a = self.inc(F.Act(t))
        skips = []
        for down in (self.down1, self.down2, self.down3, self.down4):
            # the level's concat buffer: the skip now, the decoder's resized map later
            N, Hl, Wl, C = a.shape
            buf = torch.empty((N, Hl, Wl, 2 * C), dtype=a.t.dtype, device=a.t.device)
            skip, pooled = F.skip_pool(a, buf[..., :C])
            skips.append((buf, skip))
            a = down(pooled)
        lo = self.head(a, skips, self.nclass)
        # F.interpolate(x, size) of the full-resolution logits: an identity resize
        return tuple([F.logits_to_nchw(lo, (H, W), align_corners=True,
                                       lazy=F.want_lazy_logits(self.training))])


class _UNetHead(nn.Module):
    def __init__(self, nclass, norm_layer=nn.BatchNorm2d):
        super().__init__()
        bilinear = True
        self.up1 = Up(1024, 256, bilinear)
        self.up2 = Up(512, 128, bilinear)
        self.up3 = Up(256, 64, bilinear)
        self.up4 = Up(128, 64, bilinear)
        self.outc = OutConv(64, nclass)

    def forward(self, a, skips, nclass):
        """a: the deepest level's pending activation; skips: (concat buffer, skip view) per level,
        shallowest first.  -> the nclass leading channels of vector-padded float32 NHWC logits."""
        for up, (buf, skip) in zip((self.up1, self.up2, self.up3, self.up4), reversed(skips)):
            a = up(a, buf, skip)
        return self.outc(a, nclass)


class DoubleConv(nn.Module):
    """(convolution => [BN] => ReLU) * 2 (unet.py:63-78).  Act -> the pending activation."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.double_conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1),
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels, out_channels, kernel_size=3, padding=1),
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True))

    def forward(self, act):
        dc = self.double_conv
        a = F.conv_bn(act, dc[0], dc[1])
        a.relu = True
        a = F.conv_bn(a, dc[3], dc[4])
        a.relu = True
        return a


class Down(nn.Module):
    """Downscaling with maxpool then double conv (unet.py:81-92).  The pool itself ran with the
    skip's write-out (functional.skip_pool): x is the pooled plain tensor."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), DoubleConv(in_channels, out_channels))

    def forward(self, x):
        return self.maxpool_conv[1](F.Act(x))


class Up(nn.Module):
    """Upscaling then double conv (unet.py:95-121), the reference's bilinear = True."""

    def __init__(self, in_channels, out_channels, bilinear=True):
        super().__init__()
        if not bilinear:
            raise NotImplementedError("Up: the ConvTranspose2d variant is not served (the "
                                      "reference hard-codes bilinear = True)")
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self.conv = DoubleConv(in_channels, out_channels)

    def forward(self, a, buf, skip):
        """a: the deeper level's pending activation [N,h,w,C]; buf [N,Hs,Ws,2C] with the skip in
        channels [0, C).  The resized map (2h x 2w) goes to channels [C, 2C), padded to the skip's
        size as F.pad(x1, [dX // 2, dX - dX // 2, dY // 2, dY - dY // 2]) does."""
        N, h, w, C = a.shape
        Hs, Ws = buf.shape[1:3]
        if skip.shape[-1] != C or buf.shape[-1] != 2 * C:
            raise ValueError("Up: %d channels from below, a %d-channel skip" % (C, skip.shape[-1]))
        dy, dx = Hs - 2 * h, Ws - 2 * w
        if dy < 0 or dx < 0:
            raise ValueError("Up: the resized map %d x %d exceeds the skip %d x %d"
                             % (2 * h, 2 * w, Hs, Ws))
        up = F.bilinear_placed(a, (2 * h, 2 * w), buf[..., C:], place=(dy // 2, dx // 2))
        return self.conv(F.Act(F.concat_alias(buf, [skip, up])))


class OutConv(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=1)

    def forward(self, a, nclass):
        """The biased 64 -> nclass projection, in float32 in every compute dtype as CGNet's and
        FPENet's classifiers; returns the nclass leading channels of a vector-padded buffer."""
        t = F.materialize(a)
        if t.dtype != torch.float32:
            t = t.float()
        N, H, W, _ = t.shape
        vec = vec_of(t.dtype)
        pitch = (nclass + 2 * vec - 1) // vec * vec
        out = torch.empty((N, H, W, pitch), dtype=t.dtype, device=t.device)
        return F.conv_bn(F.Act(t), self.conv, None, out=out[..., :nclass]).t
