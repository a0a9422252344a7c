"""PointRend — module tree / state_dict of segmentron/models/pointrend.py:11-195, with the point
head on the HIP kernels of csrc/pointrend.hip.

`backbone` is the model named by cfg.MODEL.POINTREND.BASEMODEL (DeepLabV3_Plus: its `encoder`,
`head` and, with SOLVER.AUX, an unused `auxlayer`); `head.mlp` is the four Conv1d(k=1) layers
275 -> 256 -> 256 -> 256 -> nclass, run as 1x1 GEMMs with the points as pixels.  `encoder` is
None, so solver/optimizer.py takes its single-group branch (no BN_EPS_FOR_ENCODER).

A training forward returns the reference's dict:
  coarse  CoarseLogits: the head's NHWC logits behaving as [N, nclass, h, w] float32; the
          F.interpolate of PointRendLoss (solver/loss.py:374) stays pending into its fused loss
  rend    PointLogits: the MLP's point rows behaving as [N, nclass, P] float32; F.cross_entropy
          on them runs seg_point_ce_*
  points  float32 [N, P, 2]
  res2    c1 as an NCHW view (nothing in the training loop reads it)
An evaluation forward runs the subdivision loop (PointHead.inference) on float32 NCHW maps and
returns (fine,) at the input size.
"""
import contextlib
import dataclasses

import torch
import torch.nn as nn

from .. import functional as F
from .. import hip_ops as K
from ..config import cfg
from .model_zoo import MODEL_REGISTRY
from .segbase import SegBaseModel

__all__ = ["PointRend", "PointHead", "point_sample", "sampling_points"]


@MODEL_REGISTRY.register(name="PointRend")
class PointRend(SegBaseModel):
    # data-dependent point selection: never captured into a HIP graph (model_zoo)
    graph_capturable = False

    def __init__(self):
        super().__init__(need_backbone=False)
        self.backbone = MODEL_REGISTRY.get(cfg.MODEL.POINTREND.BASEMODEL)()
        self.head = PointHead(num_classes=self.nclass)

    def forward(self, x):
        c1, _, _, c4 = self.backbone.encoder(x)
        coarse = self.backbone.head(c4, c1)  # NHWC logits (pitched), output stride 16
        fine = F.materialize(c1)  # c1's pending BatchNorm + ReLU, applied once
        if not self.training:
            return (self.head.inference(x, fine, coarse),)
        rend, points = self.head(x, fine, coarse)
        return {"res2": fine.permute(0, 3, 1, 2),
                "coarse": CoarseLogits(coarse, tuple(coarse.shape[1:3])),
                "rend": rend, "points": points}


class PointHead(nn.Module):
    """pointrend.py:32-116."""

    def __init__(self, in_c=275, num_classes=19, k=3, beta=0.75):
        super().__init__()
        self.mlp = nn.Sequential(
            nn.Conv1d(in_c, 256, kernel_size=1, stride=1, padding=0, bias=True),
            nn.ReLU(True),
            nn.Conv1d(256, 256, kernel_size=1, stride=1, padding=0, bias=True),
            nn.ReLU(True),
            nn.Conv1d(256, 256, kernel_size=1, stride=1, padding=0, bias=True),
            nn.ReLU(True),
            nn.Conv1d(256, num_classes, 1))
        self.k = k
        self.beta = beta
        self._draws = None

    @contextlib.contextmanager
    def recorded_draws(self, over_generation=None, coverage=None):
        """Inside: training forwards take these device tensors ([N, k*P, 2] / [N, P - beta*P, 2],
        either may be None) instead of the two torch.rand calls of sampling_points — to replay
        a recorded run.  Outside nothing is kept."""
        prev, self._draws = self._draws, (over_generation, coverage)
        try:
            yield self
        finally:
            self._draws = prev

    def forward(self, x, fine, coarse):
        """Training: N = W // 16, P = N * N points (pointrend.py:60-70)."""
        n = x.shape[-1] // 16
        points = _sampling_points(K.map_nhwc(coarse.detach()), n * n, self.k, self.beta, True,
                                  self._draws)
        rows = _PointFeaturesFn.apply(coarse, fine, points, False)
        return PointLogits(self.run_mlp(rows), x.shape[0]), points

    def run_mlp(self, rows):
        """rows [1, 1, R, ld] (zero beyond the 275 features) -> logits [1, 1, R, nclass] (a slice
        of a vector-pitched buffer).  The Conv1d parameters keep K = 275; the first layer runs
        on a zero-padded [256, ld, 1, 1] copy of its weight made per call (autograd slices the
        gradient back), which the GEMM path then packs."""
        convs = [self.mlp[i] for i in (0, 2, 4, 6)]
        R, ld = rows.shape[2], rows.shape[3]
        h = F.Act(rows)
        for i, conv in enumerate(convs):
            w = conv.weight.unsqueeze(-1)
            if w.shape[1] != h.t.shape[-1]:
                w = nn.functional.pad(w, (0, 0, 0, 0, 0, h.t.shape[-1] - w.shape[1]))
            out = None
            if i == len(convs) - 1:
                O = conv.out_channels
                out = torch.empty((1, 1, R, F._round_up(O, K.vec_of(rows.dtype))),
                                  dtype=rows.dtype, device=rows.device)[..., :O]
            spec = F.ConvSpec(h, out=out, want_stats=False)
            y = F._ConvFn.apply(h.t, None, None, w, conv.bias, spec)
            h = F.Act(y, relu=i < len(convs) - 1)  # nn.ReLU: the next GEMM's prologue
        return h.t

    @torch.no_grad()
    def inference(self, x, fine, coarse):
        """pointrend.py:72-116 with float32 NCHW maps (also in bfloat16 mode): x2 upsamples while
        out.shape[-1] * 2 < x.shape[-1], then the input size (align_corners=False); at every step
        the min(H*W, 8096) most uncertain pixels are re-predicted by the MLP."""
        num_points = 8096
        m = K.map_nhwc(coarse)
        H, W = m[5], m[6]
        while W * 2 < x.shape[-1]:
            H, W = 2 * H, 2 * W
            m = K.map_nchw(K.point_resize(m, (H, W), align_corners=False))
            self._refine(m, fine, num_points)
        m = K.map_nchw(K.point_resize(m, tuple(x.shape[-2:]), align_corners=False))
        self._refine(m, fine, num_points)
        return m[0]

    def _refine(self, m, fine, num_points):
        idx, points = _sampling_points(m, num_points, training=False)
        rend = self.run_mlp(_PointFeaturesFn.apply(m[0], fine, points, True))
        K.point_scatter(rend.view(rend.shape[2], rend.shape[3]), idx, m)


class _PointFeaturesFn(torch.autograd.Function):
    """torch.cat([point_sample(coarse), point_sample(fine)], 1) of pointrend.py:63-66 written as
    point rows [1, 1, N*P, ld] in fine's dtype: coarse at columns [0, C0), fine at [C0, C0 + C1),
    zeros up to the GEMM's vector pitch.  The concatenation is never materialised."""

    @staticmethod
    def forward(ctx, coarse, fine, points, coarse_nchw):
        mc = K.map_nchw(coarse) if coarse_nchw else K.map_nhwc(coarse)
        mf = K.map_nhwc(fine)
        C0, C1 = mc[7], mf[7]
        N, P = points.shape[0], points.shape[1]
        ld = F._round_up(C0 + C1, K.vec_of(fine.dtype))
        rows = torch.zeros((N * P, ld), dtype=fine.dtype, device=fine.device)
        K.point_sample(mc, points, rows, 0)
        K.point_sample(mf, points, rows, C0)
        ctx.save_for_backward(points)
        ctx.meta = (C0, C1, (mc[5], mc[6]), coarse.dtype,
                    None if coarse_nchw else K.nhwc(coarse)[4], (mf[5], mf[6]), fine.dtype)
        return rows.view(1, 1, N * P, ld)

    @staticmethod
    def backward(ctx, g):
        (points,) = ctx.saved_tensors
        C0, C1, chw, cdt, cpitch, fhw, fdt = ctx.meta
        g = g.reshape(g.shape[2], g.shape[3])
        if g.stride(1) != 1:
            g = g.contiguous()
        dc = df = None
        if ctx.needs_input_grad[0]:
            dc = K.point_sample_bwd(g, 0, C0, points, chw, cdt, cpitch)
        if ctx.needs_input_grad[1]:
            df = K.point_sample_bwd(g, C0, C1, points, fhw, fdt)
        return dc, df, None, None


class _PointCEFn(torch.autograd.Function):
    """F.cross_entropy(rend, labels, ignore_index) with reduction 'mean' on the point rows."""

    @staticmethod
    def forward(ctx, rows, target, ignore_index):
        target = target.reshape(-1).contiguous()
        out = K.point_ce_fwd(rows, target, ignore_index)
        ctx.save_for_backward(rows, target, out)
        ctx.ignore_index = ignore_index
        return out[0]

    @staticmethod
    def backward(ctx, g):
        rows, target, out = ctx.saved_tensors
        return K.point_ce_bwd(rows, target, ctx.ignore_index, out, g), None, None


def _bind_ce(input, target, weight=None, size_average=None, ignore_index=-100, reduce=None,
             reduction="mean", label_smoothing=0.0):
    return target, weight, size_average, ignore_index, reduce, reduction, label_smoothing


@dataclasses.dataclass(eq=False, repr=False)
class PointLogits:
    """What the training forward returns as `rend`: the MLP's logits rows [1, 1, N*P, nclass]
    (compute dtype, vector-pitched) behaving as the reference's [N, nclass, P] float32 tensor.
    `F.cross_entropy(rend, labels [N, P], ignore_index=..)` (PointRendLoss, solver/loss.py:383)
    runs seg_point_ce_*; any other use reads the materialised tensor (cast + transposed view).
    A dataclass, so DistributedDataParallel's `_find_tensors` finds `lo`."""
    lo: torch.Tensor
    n: int
    _full: object = dataclasses.field(default=None, init=False, repr=False)

    dtype = torch.float32

    @property
    def shape(self):
        return torch.Size((self.n, self.lo.shape[-1], self.lo.shape[2] // self.n))

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return 3

    @property
    def device(self):
        return self.lo.device

    @property
    def requires_grad(self):
        return self.lo.requires_grad

    def rows(self):
        return self.lo.view(self.lo.shape[2], self.lo.shape[3])

    def materialize(self):
        if self._full is None:
            self._full = self.lo.view(self.n, -1, self.lo.shape[-1]).float().permute(0, 2, 1)
        return self._full

    def __getattr__(self, name):  # only called when normal lookup fails
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    def __getitem__(self, idx):
        return self.materialize()[idx]

    def __len__(self):
        return self.n

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is torch.nn.functional.cross_entropy and args and isinstance(args[0], cls):
            view = args[0]
            target, weight, size_average, ignore_index, reduce, reduction, smoothing = \
                _bind_ce(*args, **kwargs)
            if (weight is None and size_average is None and reduce is None
                    and reduction == "mean" and smoothing == 0.0
                    and isinstance(target, torch.Tensor) and target.dtype == torch.int64
                    and tuple(target.shape) == (view.n, view.shape[2])):
                return _PointCEFn.apply(view.rows(), target, int(ignore_index))

        def real(o):
            if isinstance(o, cls):
                return o.materialize()
            if isinstance(o, (list, tuple)):
                return type(o)(real(v) for v in o)
            return o
        return func(*real(args), **{k: real(v) for k, v in kwargs.items()})


@dataclasses.dataclass(eq=False, repr=False)
class CoarseLogits(F.LogitsView):
    """What the training forward returns as `coarse`: the head's NHWC logits behaving as the
    reference's [N, nclass, h, w] float32 tensor.  `F.interpolate(coarse, size, mode='bilinear',
    align_corners=a)` (PointRendLoss, solver/loss.py:374) returns a LogitsView of the same
    low-resolution tensor, so the resize stays pending into the following F.cross_entropy; any
    other use materialises [N, nclass, h, w]."""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is torch.nn.functional.interpolate and args and isinstance(args[0], cls):
            def bind(input, size=None, scale_factor=None, mode="nearest", align_corners=None,
                     recompute_scale_factor=None, antialias=False):
                return size, scale_factor, mode, align_corners, antialias
            size, scale, mode, align, antialias = bind(*args, **kwargs)
            if mode == "bilinear" and size is not None and scale is None and not antialias:
                if isinstance(size, int):
                    size = (size, size)
                return CoarseUpsampled(args[0].lo, tuple(size), bool(align))
        return super().__torch_function__(func, types, args, kwargs)


@dataclasses.dataclass(eq=False, repr=False)
class CoarseUpsampled(F.LogitsView):
    """F.interpolate of CoarseLogits: a LogitsView whose fused cross-entropy also takes the
    output-stride-16 resize of PointRendLoss (x16 at a 769 crop: 49 -> 769), up to 16.1x
    (seg_upsample_ce_bwd's third tier).  LogitsView's own 8.1x limit, which decides the path of
    every other model, is unchanged."""

    def _fusable(self, target, weight, size_average, ignore_index, reduce, reduction,
                 label_smoothing):
        n, hi, wi, c = self.lo.shape
        return (weight is None and size_average is None and reduce is None
                and reduction == "mean" and label_smoothing == 0.0 and c <= 32
                and isinstance(target, torch.Tensor) and target.dtype == torch.int64
                and target.dim() == 3 and tuple(target.shape) == (n,) + self.out_hw
                and self.align_corners and self.out_hw[0] >= hi and self.out_hw[1] >= wi
                and hi > 1 and wi > 1
                and self.out_hw[0] - 1 <= 16.1 * (hi - 1) and self.out_hw[1] - 1 <= 16.1 * (wi - 1))


class _PointSampleFn(torch.autograd.Function):
    """Public point_sample on NCHW tensors: [N, C, H, W] at [N, P, 2] -> [N, C, P] float32."""

    @staticmethod
    def forward(ctx, input, points, nearest):
        m = K.map_nchw(input)
        N, P = points.shape[0], points.shape[1]
        rows = K.point_sample(m, points, nearest=nearest)
        ctx.save_for_backward(points)
        ctx.meta = (m[5], m[6], m[7], input.dtype, nearest)
        return rows.view(N, P, m[7]).permute(0, 2, 1)

    @staticmethod
    def backward(ctx, g):
        (points,) = ctx.saved_tensors
        H, W, C, dtype, nearest = ctx.meta
        if nearest:
            raise RuntimeError("point_sample: no gradient for mode='nearest'")
        rows = g.permute(0, 2, 1).contiguous().view(-1, C)
        dx = K.point_sample_bwd(rows, 0, C, points, (H, W), dtype)
        return dx.permute(0, 3, 1, 2), None, None


def point_sample(input, point_coords, **kwargs):
    """pointrend.py:119-141 (F.grid_sample(input, 2 * point_coords - 1, **kwargs)) on the HIP
    kernels.  input: NCHW float32 / bfloat16 device tensor; point_coords: float32 [N, P, 2] in
    [0, 1] -> [N, C, P] float32.  mode 'bilinear' (differentiable) or 'nearest'
    (std::nearbyint taps); align_corners False and padding_mode 'zeros', as every caller passes."""
    mode = kwargs.pop("mode", "bilinear")
    align = kwargs.pop("align_corners", None)
    padding = kwargs.pop("padding_mode", "zeros")
    if kwargs or align or padding != "zeros" or mode not in ("bilinear", "nearest") \
            or point_coords.dim() != 3:
        raise NotImplementedError(
            "point_sample: only [N, P, 2] points, mode bilinear / nearest, align_corners=False, "
            "padding_mode='zeros' run on the HIP path (got mode=%r align_corners=%r "
            "padding_mode=%r, %d-d points, extra %s)"
            % (mode, align, padding, point_coords.dim(), sorted(kwargs)))
    return _PointSampleFn.apply(input, point_coords, mode == "nearest")


@torch.no_grad()
def sampling_points(mask, N, k=3, beta=0.75, training=True, draws=None):
    """pointrend.py:144-195 on the HIP kernels; mask: NCHW [B, C, H, W] device tensor.
    Training: [B, N, 2] = int(beta*N) most uncertain of k*N random points, then N - int(beta*N)
    random ones.  Evaluation: (idx [B, min(H*W, N)], pixel-centre points).  Indices come out in
    ascending order (the reference's topk order is by value; ties here go to the lower index).
    draws: optional (over_generation [B, k*N, 2], coverage [B, N - int(beta*N), 2]) in place of
    the two torch.rand calls."""
    assert mask.dim() == 4, "Dim must be N(Batch)CHW"
    return _sampling_points(K.map_nchw(mask), N, k, beta, training, draws)


def _sampling_points(m, N, k=3, beta=0.75, training=True, draws=None):
    t, B, H, W = m[0], m[4], m[5], m[6]
    if not training:
        N = min(H * W, N)
        idx = K.point_topk(K.point_uncertainty(m), N)
        return idx, K.point_coords_grid(idx, (H, W))
    over, cover = draws if draws is not None else (None, None)
    if over is None:
        over = torch.rand(B, k * N, 2, device=t.device)
    n_imp = int(beta * N)
    idx = K.point_topk(K.point_uncertainty(m, over), n_imp) if n_imp > 0 else None
    if cover is None:
        cover = torch.rand(B, N - n_imp, 2, device=t.device)
    return K.point_coords_train(over, idx, cover)
