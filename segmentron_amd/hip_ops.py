"""Thin tensor-level wrappers over the C-ABI (include/segmentron_hip.h).

Everything here takes raw ``torch`` CUDA(HIP) tensors purely as device-memory handles — NHWC views
``[N, H, W, C]`` whose channel dimension may be a slice of a wider buffer — and launches on the
current HIP stream.  No autograd, no fallbacks: a CPU tensor raises.
"""
import torch

from ._lib import LIB

PRO_NONE, PRO_RELU, PRO_AFFINE, PRO_AFFINE_RELU = 0, 1, 2, 3
_DT = {torch.float32: 0, torch.bfloat16: 1}


def vec_of(dtype):
    return 8 if dtype == torch.bfloat16 else 4


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream.  The raw getter is ~10x cheaper than building a
    torch.cuda.Stream object — with ~1200 launches per step that was 4 ms of host time in the
    launch-bound eager path (N > 1 DDP runs)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _count(count):
    """BatchNorm element count: a host number, or (SyncBN) a device float64 scalar tensor that
    came out of the statistics all-reduce -> (host double, device pointer)."""
    if isinstance(count, torch.Tensor):
        return 0.0, count.data_ptr()
    return float(count), 0


def nhwc(t):
    """-> (N, H, W, C, ld) of an NHWC view; checks it is addressable as rows with pitch ld."""
    if not t.is_cuda:
        raise RuntimeError("segmentron_amd ops need HIP device tensors (no CPU fallback)")
    if t.dim() != 4:
        raise RuntimeError("expected NHWC 4-d tensor, got %s" % (tuple(t.shape),))
    N, H, W, C = t.shape
    # torch leaves arbitrary strides on size-1 dims: derive the row pitch from the innermost
    # dimension that actually has extent
    if W > 1:
        ld = t.stride(2)
    elif H > 1:
        ld = t.stride(1)
    elif N > 1:
        ld = t.stride(0)
    else:
        ld = C
    ok = (t.stride(3) == 1 or C == 1) and ld >= C
    if W > 1 and H > 1:
        ok = ok and t.stride(1) == W * ld
    if N > 1 and (H > 1 or W > 1):
        ok = ok and t.stride(0) == H * W * ld
    if not ok:
        raise RuntimeError("tensor is not a dense-row NHWC view: shape %s strides %s"
                           % (tuple(t.shape), t.stride()))
    return N, H, W, C, ld


def _pro(pro):
    if pro is None:
        return PRO_NONE, None, None
    return pro


def new_act(N, H, W, C, dtype, device, pitch=None):
    """Allocate an NHWC activation [N,H,W,C] (optionally as the leading slice of pitch channels)."""
    if pitch is None or pitch == C:
        return torch.empty((N, H, W, C), dtype=dtype, device=device)
    return torch.empty((N, H, W, pitch), dtype=dtype, device=device)[..., :C]


# ----------------------------------------------------------------------------- conv (GEMM)
def conv_out_size(Hi, k, stride, pad, dil):
    return (Hi + 2 * pad - dil * (k - 1) - 1) // stride + 1


def conv_gemm(x, w_packed, O, KH, KW, stride, pad, dil, pro=None, bias=None, out=None,
              want_stats=False, scatter=None, ep=None, tconv_out_hw=None):
    """x NHWC; w_packed [O, KH*KW*C] in x.dtype.  Returns (y, stat_partial|None).
    scatter=(out_H, out_W, s): write output pixel (ho,wo) at (ho*s, wo*s) of a zero-filled
    [N,out_H,out_W,O] tensor (data gradient of a strided 1x1 conv)."""
    N, Hi, Wi, C, ldx = nhwc(x)
    if tconv_out_hw is not None:  # transposed-stride gather: x is dy, the output is dx
        Ho, Wo = tconv_out_hw
    else:
        Ho, Wo = conv_out_size(Hi, KH, stride, pad, dil), conv_out_size(Wi, KW, stride, pad, dil)
    mode, ps, pt = _pro(pro)
    if scatter is None:
        oH, oW, os_ = Ho, Wo, 1
        if out is None:
            out = torch.empty((N, Ho, Wo, O), dtype=x.dtype, device=x.device)
    else:
        oH, oW, os_ = scatter
        if out is None:
            out = torch.zeros((N, oH, oW, O), dtype=x.dtype, device=x.device)
    ldy = nhwc(out)[4]
    partial = None
    if want_stats:
        tm = LIB.query("seg_conv_gemm_stat_rows", _DT[x.dtype], N, Ho, Wo, C, O, KH, KW, stride,
                       pad, dil, 1 if tconv_out_hw is not None else 0, int(bias is not None), mode)
        partial = torch.empty((tm, 2, O), dtype=torch.float32, device=x.device)
    assert w_packed.dtype == x.dtype and w_packed.is_contiguous()
    ep_x, ldep, ep_c0, ep_c1 = None, 0, None, None
    if ep is not None:  # (x_like_output, c0, c1): y = acc - c0 - c1 * x  (folded-BN backward)
        ep_x, ep_c0, ep_c1 = ep
        assert tuple(ep_x.shape) == tuple(out.shape)
        ldep = nhwc(ep_x)[4]
    LIB.call("seg_conv_gemm_fwd", _DT[x.dtype], _p(x), ldx, N, Hi, Wi, C, _p(w_packed), O, KH, KW,
             stride, pad, dil, mode, _p(ps), _p(pt), _p(bias), _p(out), ldy, Ho, Wo, oH, oW, os_,
             _p(partial), _p(ep_x), ldep, _p(ep_c0), _p(ep_c1),
             1 if tconv_out_hw is not None else 0, _stream())
    return out, partial


def colsum(partial2d, f64=True):
    """partial2d: fp32 [R, L] -> [L] (float64 or float32)."""
    R, L = partial2d.shape
    dev = partial2d.device
    out = torch.empty(L, dtype=torch.float64 if f64 else torch.float32, device=dev)
    ws = torch.empty(64 * L, dtype=torch.float64, device=dev) if R > 128 else None
    LIB.call("seg_colsum", _p(partial2d), R, L, _p(out) if f64 else 0, 0 if f64 else _p(out),
             _p(ws), _stream())
    return out


# ---- nn.GroupNorm (csrc/groupnorm.hip) ----------------------------------------------------------
def gn_moments(u, v=None):
    """NHWC u (, v) -> fp32 [N, chunks, 2, C]: (sum u, sum u*v) per sample, pixel chunk and channel
    (v None: sum u, sum u^2)."""
    N, H, W, C, ldu = nhwc(u)
    ldv = 0
    if v is not None:
        assert tuple(v.shape) == tuple(u.shape) and v.dtype == u.dtype
        ldv = nhwc(v)[4]
    chunks = LIB.query("seg_gn_chunks", H * W)
    partial = torch.empty((N, chunks, 2, C), dtype=torch.float32, device=u.device)
    LIB.call("seg_gn_moments", _DT[u.dtype], _p(u), ldu, _p(v), ldv, N, H * W, C, _p(partial),
             _stream())
    return partial


def gn_fwd_finalize(partial, HW, G, gamma, beta, eps):
    """-> (mean_rstd fp32 [N, G, 2], coef fp32 [N, 3, C]) with z = coef[n,0,c]*x + coef[n,2,c]."""
    N, _, _, C = partial.shape
    mean_rstd = torch.empty((N, G, 2), dtype=torch.float32, device=partial.device)
    coef = torch.empty((N, 3, C), dtype=torch.float32, device=partial.device)
    LIB.call("seg_gn_fwd_finalize", _p(partial), N, HW, C, G, _p(gamma), _p(beta), float(eps),
             _p(mean_rstd), _p(coef), _stream())
    return mean_rstd, coef


def gn_bwd_finalize(partial, HW, G, mean_rstd, gamma):
    """moments of (dz, x) -> (coef [N, 3, C] of dx = k1*dz + k2*x + k3, contrib [N, 2, C]: the
    per-sample terms of dgamma | dbeta)."""
    N, _, _, C = partial.shape
    coef = torch.empty((N, 3, C), dtype=torch.float32, device=partial.device)
    contrib = torch.empty((N, 2, C), dtype=torch.float32, device=partial.device)
    LIB.call("seg_gn_bwd_finalize", _p(partial), N, HW, C, G, _p(mean_rstd), _p(gamma), _p(coef),
             _p(contrib), _stream())
    return coef, contrib


def gn_affine(u, v, coef, out=None):
    """out = coef[n,0,c]*u + coef[n,1,c]*v + coef[n,2,c]  (v may be None)."""
    N, H, W, C, ldu = nhwc(u)
    ldv = 0 if v is None else nhwc(v)[4]
    if out is None:
        out = torch.empty((N, H, W, C), dtype=u.dtype, device=u.device)
    LIB.call("seg_gn_affine", _DT[u.dtype], _p(u), ldu, _p(v), ldv, _p(coef), _p(out),
             nhwc(out)[4], N, H * W, C, _stream())
    return out


def colsum_count(partial2d, count):
    """partial2d fp32 [R, L] -> float64 [L + 1] = (column sums | count): the SyncBatchNorm
    forward message of one BatchNorm in one launch."""
    R, L = partial2d.shape
    dev = partial2d.device
    out = torch.empty(L + 1, dtype=torch.float64, device=dev)
    ws = torch.empty(64 * L, dtype=torch.float64, device=dev) if R > 128 else None
    LIB.call("seg_colsum_count", _p(partial2d), R, L, _p(out), float(count), _p(ws), _stream())
    return out


def conv_wgrad(x, dy, O, KH, KW, stride, pad, dil, pro=None, raw_partial=False):
    """-> dW fp32 [O, KH*KW*C]."""
    N, Hi, Wi, C, ldx = nhwc(x)
    Nd, Ho, Wo, Od, lddy = nhwc(dy)
    assert Nd == N and Od == O
    mode, ps, pt = _pro(pro)
    K = KH * KW * C
    splits = LIB.query("seg_conv_gemm_wgrad_splits", _DT[x.dtype], N, Ho, Wo, C, O, KH, KW,
                       stride, pad, dil, mode)
    partial = torch.empty((splits, O * K), dtype=torch.float32, device=x.device)
    LIB.call("seg_conv_gemm_wgrad", _DT[x.dtype], _p(x), ldx, N, Hi, Wi, C, _p(dy), lddy, Ho, Wo,
             O, KH, KW, stride, pad, dil, mode, _p(ps), _p(pt), _p(partial), splits, _stream())
    if raw_partial:  # [splits, O*K]: the consumer sums the splits itself (fold_bwd_reduce)
        return partial
    if splits == 1:
        return partial.view(O, K)
    return colsum(partial, f64=False).view(O, K)


# ----------------------------------------------------------------------------- depthwise
def dw_tiled(stride, dil):
    """True where the depthwise kernels take torch's tap layout — stride 1 at dilation 1 (the
    register-sliding kernels; the separate weight gradient is LDS-tiled) and at dilation 2 (the
    LDS-tiled ones): they read the taps as the [C,1,3,3] parameter holds them (no repacking) and,
    for the data gradient, reversed in place."""
    return stride == 1 and dil in (1, 2)


def _dw_weight_arg(w, C, stride, dil, reverse=False, is_reversed=False):
    """-> (tensor, w_layout) for a launch that wants the taps in forward order, or (`reverse`: the
    stride-1 data gradient) reversed.  w: the [C,1,3,3] / [C,9] parameter itself (bit 0; only
    where dw_tiled), or a tap-major [9, C] packing, `is_reversed` already or not.  Where dw_tiled
    the kernels reverse while they stage the taps (bit 1); the others get a reversed copy."""
    tiled = dw_tiled(stride, dil)
    if w.dim() == 4 or (w.dim() == 2 and w.shape == (C, 9) and C != 9):
        if not tiled:
            raise ValueError("depthwise row-chain / strip kernels need tap-major [9, C] weights")
        return w, 1 | (2 if reverse else 0)
    reverse = reverse and not is_reversed
    if reverse and not tiled:
        return w.flip(0).contiguous(), 0
    return w, 2 if reverse else 0


def _dw_grid_y(query, *args):
    """Partial rows of a depthwise launch; raises before anything is allocated where the library
    has no such launch (-1: an empty tensor, C not made of the kernels' channel vectors)."""
    gy = LIB.query(query, *args)
    if gy < 1:
        raise ValueError("%s%s: no such depthwise launch (empty tensor, or C is not a multiple "
                         "of the kernels' channel vector)" % (query, args))
    return gy


def dw_torch_layout(dW9c):
    """weight gradient [9, C] (tap-major) -> the parameter's [C,1,3,3]."""
    return dW9c.t().reshape(-1, 1, 3, 3).contiguous()


def dwconv(x, w9c, stride, dil, pro=None, out=None, want_stats=False):
    """w9c: tap-major [9, C] fp32, or (stride 1, dil <= 2) the [C,1,3,3] parameter itself."""
    N, Hi, Wi, C, ldx = nhwc(x)
    Ho, Wo = conv_out_size(Hi, 3, stride, dil, dil), conv_out_size(Wi, 3, stride, dil, dil)
    mode, ps, pt = _pro(pro)
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    ldy = nhwc(out)[4]
    w, layout = _dw_weight_arg(w9c, C, stride, dil)
    gy = _dw_grid_y("seg_dwconv_grid_y", _DT[x.dtype], C, N, Ho, Wo, stride, dil, 0)
    partial = torch.empty((gy, 2, C), dtype=torch.float32, device=x.device) if want_stats else None
    LIB.call("seg_dwconv3x3", _DT[x.dtype], 0, _p(x), ldx, N, Hi, Wi, C, _p(w), layout, stride,
             dil, mode, _p(ps), _p(pt), _p(out), ldy, Ho, Wo, _p(partial), gy, _stream())
    return out, partial


def _dw_grad_out(out, N, H, W, C, like):
    """-> (g, ldg): a fresh [N,H,W,C] gradient tensor, or the caller's `out` (an NHWC view of that
    shape and dtype, possibly a channel slice of a wider buffer)."""
    if out is None:
        return torch.empty((N, H, W, C), dtype=like.dtype, device=like.device), C
    if tuple(out.shape) != (N, H, W, C) or out.dtype != like.dtype:
        raise RuntimeError("out: expected %s %s, got %s %s"
                           % ((N, H, W, C), like.dtype, tuple(out.shape), out.dtype))
    return out, nhwc(out)[4]


def dwconv_dgrad(dy, w9c, stride, dil, in_hw, flipped=True, out=None):
    """stride 1: the forward correlation with the taps reversed.  `w9c` is either the
    [C,1,3,3] parameter (reversed inside the kernel), or a tap-major [9, C] packing that is
    ALREADY reversed (`flipped=True`, pack_dw_weight(..., flipped=True)) / not yet.
    out: write dx there (an NHWC view, e.g. a channel slice) instead of a fresh tensor."""
    N, Ho, Wo, C, lddy = nhwc(dy)
    Hi, Wi = in_hw
    dx, lddx = _dw_grad_out(out, N, Hi, Wi, C, dy)
    gy = _dw_grid_y("seg_dwconv_grid_y", _DT[dy.dtype], C, N, Hi, Wi, stride, dil, 0)
    # stride 1: the forward launch (mode 0) on reversed taps; strided: the data-gradient one
    w, layout = _dw_weight_arg(w9c, C, stride, dil, stride == 1, flipped)
    LIB.call("seg_dwconv3x3", _DT[dy.dtype], int(stride != 1), _p(dy), lddy, N, Ho, Wo, C, _p(w),
             layout, stride, dil, PRO_NONE, 0, 0, _p(dx), lddx, Hi, Wi, 0, gy, _stream())
    return dx


def dw_wgrad_finalize(pw, C):
    """weight-gradient partials [R, 9C] -> dW [C,1,3,3]."""
    dW = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=pw.device)
    LIB.call("seg_dwconv3x3_wgrad_finalize", _p(pw), pw.shape[0], C, _p(dW), _stream())
    return dW


def dw_bwd_finalize(pb, pw, count, mean, invstd, gamma):
    """Both reductions behind a fused depthwise backward in one launch: BatchNorm-backward
    partials pb [Rb, 2C] -> (dgamma, dbeta, c0, c1) and weight-gradient partials pw [Rw, 9C] ->
    dW [C,1,3,3]."""
    C = mean.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=mean.device)
    dW = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=mean.device)
    LIB.call("seg_dw_bwd_finalize", _p(pb), pb.shape[0], float(count), _p(mean), _p(invstd),
             _p(gamma), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(pw), pw.shape[0],
             _p(dW), C, _stream())
    return out[0], out[1], out[2], out[3], dW


def dw_bwd_finalize_sync(box, pb, pw, count_dev, mean, invstd, gamma, grad_scale):
    """dw_bwd_finalize for SyncBatchNorm: the BatchNorm sums are exchanged between the ranks
    inside the kernel (box: xgmi.PeerMailbox); the weight gradient stays local."""
    C = mean.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=mean.device)
    dW = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=mean.device)
    LIB.call("seg_dw_bwd_finalize_sync", box.handle, _p(pb), pb.shape[0], _p(count_dev), _p(mean),
             _p(invstd), _p(gamma), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(pw),
             pw.shape[0], _p(dW), C, float(grad_scale), _stream())
    return out[0], out[1], out[2], out[3], dW


def dwconv_bwd_fused_add_ok(dil):
    """Can the fused depthwise backward add a second gradient in its store path?"""
    return bool(LIB.query("seg_dwconv3x3_bwd_fused_add_ok", int(dil)))


def dwconv_bwd_fused_sum_ok(dtype, C, dil):
    """Does the fused depthwise backward with a second gradient run on the sliding kernels, which
    can add it exactly like the separate 2-ary sum (dwconv_bwd_fused(res_sum=True))?"""
    return bool(LIB.query("seg_dwconv3x3_bwd_fused_sum_ok", _DT[dtype], int(C), int(dil)))


def dwconv_bwd_fused(x, dy, w, dil, pro=None, want_bn=False, torch_layout=False, raw_dw=False,
                     res=None, out=None, res_sum=False):
    """stride-1 depthwise backward in one pass: returns (g masked by the prologue's ReLU,
    dW fp32 [9, C] (or [C,1,3,3] with torch_layout), bn_partial fp32 [gy, 2C] | None).
    w: tap-major [9, C] or (dil <= 2) the [C,1,3,3] parameter itself.
    out: write g there (an NHWC view, e.g. a channel slice) instead of a fresh tensor.
    res: a second gradient added in the store path, g = mask * dgrad + res — with res_sum the masked
    gradient is rounded to the storage type first: bit for bit sum_n([g without res, res])."""
    N, H, W, C, ldx = nhwc(x)
    lddy = nhwc(dy)[4]
    mode, ps, pt = _pro(pro)
    g, ldg = _dw_grad_out(out, N, H, W, C, x)
    w, layout = _dw_weight_arg(w, C, 1, dil)
    gy = _dw_grid_y("seg_dwconv_grid_y", _DT[x.dtype], C, N, H, W, 1, dil, 1)
    pw = torch.empty((gy, 9 * C), dtype=torch.float32, device=x.device)
    pb = torch.empty((gy, 2 * C), dtype=torch.float32, device=x.device) if want_bn else None
    if res is not None:  # g = masked dgrad + res (the other gradient of a forked activation)
        assert dil == 1 and tuple(res.shape) == (N, H, W, C) and res.dtype == x.dtype
        LIB.call("seg_dwconv3x3_bwd_fused_sum" if res_sum else "seg_dwconv3x3_bwd_fused_add",
                 _DT[x.dtype], _p(dy), lddy, _p(x), ldx, N, H, W, C, _p(w), layout, mode, _p(ps),
                 _p(pt), _p(res), nhwc(res)[4], _p(g), ldg, _p(pw), _p(pb), gy, _stream())
    else:
        LIB.call("seg_dwconv3x3_bwd_fused", _DT[x.dtype], _p(dy), lddy, _p(x), ldx, N, H, W, C,
                 _p(w), layout, dil, mode, _p(ps), _p(pt), _p(g), ldg, _p(pw), _p(pb), gy, _stream())
    if raw_dw:  # the caller reduces pw together with pb (dw_bwd_finalize)
        return g, pw, pb
    if torch_layout:
        return g, dw_wgrad_finalize(pw, C), pb
    return g, colsum(pw, f64=False).view(9, C), pb


def dwconv_bwd_fused_s2(x, dy, w, pro=None, want_bn=False, raw_dw=False, out=None):
    """stride-2 (pad 1, dil 1) depthwise backward in one pass over dy and x: returns (g masked by
    the prologue's ReLU, dW fp32 [C,1,3,3], bn_partial fp32 [gy, 2C] | None).  w: the [C,1,3,3]
    parameter.  out: write g there (an NHWC view) instead of a fresh tensor."""
    N, H, W, C, ldx = nhwc(x)
    Nd, Ho, Wo, Cd, lddy = nhwc(dy)
    assert (Nd, Ho, Wo, Cd) == (N, (H + 1) // 2, (W + 1) // 2, C) and tuple(w.shape) == (C, 1, 3, 3)
    mode, ps, pt = _pro(pro)
    g, ldg = _dw_grad_out(out, N, H, W, C, x)
    gy = _dw_grid_y("seg_dwconv3x3_s2_grid_y", C, N, H, W)
    pw = torch.empty((gy, 9 * C), dtype=torch.float32, device=x.device)
    pb = torch.empty((gy, 2 * C), dtype=torch.float32, device=x.device) if want_bn else None
    LIB.call("seg_dwconv3x3_s2_bwd_fused", _DT[x.dtype], _p(dy), lddy, _p(x), ldx, N, H, W, C,
             _p(w), mode, _p(ps), _p(pt), _p(g), ldg, _p(pw), _p(pb), gy, _stream())
    return g, (pw if raw_dw else dw_wgrad_finalize(pw, C)), pb


def dwconv_wgrad(x, dy, stride, dil, pro=None, torch_layout=False):
    """-> fp32 [9, C], or with torch_layout the parameter's own [C, 1, 3, 3]."""
    N, Hi, Wi, C, ldx = nhwc(x)
    _, Ho, Wo, _, lddy = nhwc(dy)
    mode, ps, pt = _pro(pro)
    gy = _dw_grid_y("seg_dwconv_grid_y", _DT[x.dtype], C, N, Ho, Wo, stride, dil, 2)
    partial = torch.empty((gy, 9 * C), dtype=torch.float32, device=x.device)
    LIB.call("seg_dwconv3x3_wgrad", _DT[x.dtype], _p(x), ldx, N, Hi, Wi, C, _p(dy), lddy, Ho, Wo,
             stride, dil, mode, _p(ps), _p(pt), _p(partial), gy, _stream())
    if torch_layout:
        return dw_wgrad_finalize(partial, C)
    return colsum(partial, f64=False).view(9, C)


def bn_finalize(sums, count, gamma, beta, eps, momentum, running_mean, running_var,
                mean_offset=None):
    C = sums.numel() // 2
    dev = sums.device
    out = torch.empty((4, C), dtype=torch.float32, device=dev)
    LIB.call("seg_bn_finalize", _p(sums), *_count(count), _p(gamma), _p(beta), float(eps),
             float(momentum), _p(running_mean), _p(running_var), _p(out[0]), _p(out[1]),
             _p(out[2]), _p(out[3]), C, _p(mean_offset), _stream())
    return out[0], out[1], out[2], out[3]  # mean, invstd, scale, shift


def bn_eval_affine(gamma, beta, rm, rv, eps):
    C = rm.numel()
    out = torch.empty((2, C), dtype=torch.float32, device=rm.device)
    LIB.call("seg_bn_eval_affine", _p(gamma), _p(beta), _p(rm), _p(rv), float(eps), _p(out[0]),
             _p(out[1]), C, _stream())
    return out[0], out[1]


def bn_eval_affine_multi(jobs):
    """jobs: [(gamma|None, beta|None, running_mean, running_var, eps)] -> [(scale, shift)] by one
    launch per 48 BatchNorms."""
    import ctypes
    n = len(jobs)
    outs = [torch.empty((2, j[2].numel()), dtype=torch.float32, device=j[2].device) for j in jobs]
    vp, fp, ip = ctypes.c_void_p * n, ctypes.c_float * n, ctypes.c_int * n
    LIB.call("seg_bn_eval_affine_multi", n, vp(*[_p(j[0]) for j in jobs]),
             vp(*[_p(j[1]) for j in jobs]), vp(*[_p(j[2]) for j in jobs]),
             vp(*[_p(j[3]) for j in jobs]), fp(*[float(j[4]) for j in jobs]),
             vp(*[o.data_ptr() for o in outs]), ip(*[j[2].numel() for j in jobs]), _stream())
    return [(o[0], o[1]) for o in outs]


def bn_apply(x, pro_x=None, r=None, pro_r=None, chan_mul=None, post_relu=False, out=None,
             elem_mul=None):
    N, H, W, C, ldx = nhwc(x)
    mx, sx, tx = _pro(pro_x)
    mr, sr, tr = _pro(pro_r)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    ldy = nhwc(out)[4]
    ldr = nhwc(r)[4] if r is not None else 0
    ldm = nhwc(elem_mul)[4] if elem_mul is not None else 0
    LIB.call("seg_bn_apply", _DT[x.dtype], _p(x), ldx, mx, _p(sx), _p(tx), _p(r), ldr, mr, _p(sr),
             _p(tr), _p(chan_mul), H * W, _p(elem_mul), ldm, int(post_relu), _p(out), ldy,
             N * H * W, C, _stream())
    return out


def sum_n(tensors, out=None):
    """NHWC tensors of one shape / dtype -> their sum (fp32 accumulation in list order, one
    rounding): ONE launch for up to 8 operands (more: in groups).  out: an NHWC view (a channel
    slice of a wider buffer, none of the operands) the last launch writes."""
    import ctypes
    ts = list(tensors)
    while len(ts) > 1:
        group, ts = ts[:8], ts[8:]
        N, H, W, C, _ = nhwc(group[0])
        lds = [nhwc(t)[4] for t in group]
        assert all(t.shape == group[0].shape and t.dtype == group[0].dtype for t in group)
        if out is not None and not ts:
            assert out.shape == group[0].shape and out.dtype == group[0].dtype
            dst = out
        else:
            dst = torch.empty((N, H, W, C), dtype=group[0].dtype, device=group[0].device)
        n = len(group)
        LIB.call("seg_sum_n", _DT[dst.dtype], n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in group]),
                 (ctypes.c_long * n)(*lds), _p(dst), nhwc(dst)[4], N * H * W, C, _stream())
        ts.insert(0, dst)
    return ts[0]


def nearest_add(x, pro_x, r, pro_r, shift, post_relu=False, out=None):
    """y = post_relu?(act_x(x) + act_r(nearest_upsample_{2^shift}(r)))  (hrnet.py:186,215-229)"""
    N, H, W, C, ldx = nhwc(x)
    Nr, Hr, Wr, Cr, ldr = nhwc(r)
    if (Nr, Hr << shift, Wr << shift, Cr) != (N, H, W, C):
        raise ValueError("nearest_add: %s is not %s upsampled by 2^%d"
                         % (tuple(x.shape), tuple(r.shape), shift))
    mx, sx, tx = _pro(pro_x)
    mr, sr, tr = _pro(pro_r)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    LIB.call("seg_nearest_add", _DT[x.dtype], _p(x), ldx, mx, _p(sx), _p(tx), _p(r), ldr, mr,
             _p(sr), _p(tr), shift, int(post_relu), _p(out), nhwc(out)[4], N, H, W, C, _stream())
    return out


def nearest_sum_bwd(g, shift):
    """gradient of nearest_upsample_{2^shift}: 2^shift x 2^shift block sums."""
    N, H, W, C, ldg = nhwc(g)
    out = torch.empty((N, H >> shift, W >> shift, C), dtype=g.dtype, device=g.device)
    LIB.call("seg_nearest_sum_bwd", _DT[g.dtype], _p(g), ldg, N, H, W, C, shift, _p(out), C,
             _stream())
    return out


def bn_bwd_reduce_partial(g, x, pro, chan_mul=None, elem_mul=None):
    """-> fp32 [grid_y, 2C] per-block (sum g', sum g'*x)."""
    N, H, W, C, ldg = nhwc(g)
    ldx = nhwc(x)[4]
    mode, s, t = _pro(pro)
    M = N * H * W
    gy = LIB.query("seg_bn_bwd_grid_y", _DT[g.dtype], C, M)
    partial = torch.empty((gy, 2 * C), dtype=torch.float32, device=g.device)
    ldm = nhwc(elem_mul)[4] if elem_mul is not None else 0
    LIB.call("seg_bn_bwd_reduce", _DT[g.dtype], _p(g), ldg, _p(x), ldx, mode, _p(s), _p(t),
             _p(chan_mul), H * W, _p(elem_mul), ldm, M, C, _p(partial), gy, _stream())
    return partial


def ew_geom(dtype, C, M):
    """Launch geometry of the row-tile kernels (bn_apply, bn_bwd_reduce_partial, bn_bwd_apply,
    sum_n) for C channels of `dtype` over M rows (host only) -> dict: lanes per row and rows of a
    block, threads, gx, gy (gridDim.y of the apply kernels / sum_n), gy_reduce (partial rows)."""
    vals = [LIB.query("seg_ew_geom_query", _DT[dtype], C, M, k) for k in range(5)]
    if min(vals) < 1:
        raise ValueError("ew_geom: bad dtype / C / M: %s %d %d" % (dtype, C, M))
    geo = dict(zip(("lanes", "rows", "threads", "gx", "gy"), vals))
    geo["gy_reduce"] = LIB.query("seg_bn_bwd_grid_y", _DT[dtype], C, M)
    return geo


def bn_bwd_small(g, x, pro, count, mean, invstd, gamma, chan_mul=None, elem_mul=None,
                 training=True, out=None):
    """BatchNorm backward of a small tensor (<= SMALL_BN_ROWS samples per channel) in one
    float64 launch -> (dx, dgamma, dbeta)."""
    N, H, W, C, ldg = nhwc(g)
    ldx = nhwc(x)[4]
    mode, s, t = _pro(pro)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=g.dtype, device=g.device)
    lddx = nhwc(out)[4]
    dgb = torch.empty((2, C), dtype=torch.float32, device=g.device)
    ldm = nhwc(elem_mul)[4] if elem_mul is not None else 0
    LIB.call("seg_bn_bwd_small", _DT[g.dtype], _p(g), ldg, _p(x), ldx, _p(out), lddx, N * H * W, C,
             mode, _p(s), _p(t), _p(mean), _p(invstd), _p(gamma), _p(chan_mul), H * W,
             _p(elem_mul), ldm, float(count), 1 if training else 0, _p(dgb[0]), _p(dgb[1]),
             _stream())
    return out, dgb[0], dgb[1]


def bn_bwd_reduce(g, x, pro, chan_mul=None):
    """-> float64 [2C]: (sum g', sum g'*x)."""
    return colsum(bn_bwd_reduce_partial(g, x, pro, chan_mul), f64=True)


def _ws(R, C, dev):
    return torch.empty(128 * C, dtype=torch.float64, device=dev) if R > 1024 else None


def bn_finalize_p(partial, count, gamma, beta, eps, momentum, running_mean, running_var,
                  mean_offset=None):
    """partial fp32 [R, 2, C] (or [R, 2C]) -> mean, invstd, scale, shift (one fused launch)."""
    R = partial.shape[0]
    C = partial.numel() // (2 * R)
    out = torch.empty((4, C), dtype=torch.float32, device=partial.device)
    ws = _ws(R, C, partial.device)
    LIB.call("seg_bn_finalize_p", _p(partial), R, float(count), _p(gamma), _p(beta), float(eps),
             float(momentum), _p(running_mean), _p(running_var), _p(out[0]), _p(out[1]),
             _p(out[2]), _p(out[3]), C, _p(mean_offset), _p(ws), _stream())
    return out[0], out[1], out[2], out[3]


SMALL_BN_ROWS = 1024


def bn_finalize_small(y, gamma, beta, eps, momentum, running_mean, running_var, mean_offset=None):
    """BatchNorm statistics of a SMALL stored tensor y [N,H,W,C] (N*H*W <= 4096 rows), two-pass
    (mean, then sum (x - mean)^2) -> mean, invstd, scale, shift (+ running-stat update)."""
    N, H, W, C, ldy = nhwc(y)
    out = torch.empty((4, C), dtype=torch.float32, device=y.device)
    LIB.call("seg_bn_finalize_small", _DT[y.dtype], _p(y), ldy, N * H * W, C, _p(gamma), _p(beta),
             float(eps), float(momentum), _p(running_mean), _p(running_var), _p(out[0]),
             _p(out[1]), _p(out[2]), _p(out[3]), _p(mean_offset), _stream())
    return out[0], out[1], out[2], out[3]


def bn_moments_small(y):
    """This rank's two-pass moments of a small stored tensor as float64 sums [2C + 1] =
    (n*mean | M2 + n*mean^2 | n): the SyncBatchNorm forward message of a small BatchNorm."""
    N, H, W, C, ldy = nhwc(y)
    out = torch.empty(2 * C + 1, dtype=torch.float64, device=y.device)
    LIB.call("seg_bn_moments_small", _DT[y.dtype], _p(y), ldy, N * H * W, C, _p(out), _stream())
    return out


def bn_finalize_small_sync(box, y, gamma, beta, eps, momentum, running_mean, running_var,
                           mean_offset=None):
    """bn_finalize_small for SyncBatchNorm through the peer mailbox (one launch) -> mean, invstd,
    scale, shift, global count (float64 [1])."""
    N, H, W, C, ldy = nhwc(y)
    out = torch.empty((4, C), dtype=torch.float32, device=y.device)
    cnt = torch.empty(1, dtype=torch.float64, device=y.device)
    LIB.call("seg_bn_finalize_small_sync", box.handle, _DT[y.dtype], _p(y), ldy, N * H * W, C,
             _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean), _p(running_var),
             _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(mean_offset), _p(cnt), _stream())
    return out[0], out[1], out[2], out[3], cnt


def bn_finalize_p_sync(box, partial, local_count, gamma, beta, eps, momentum, running_mean,
                       running_var, mean_offset=None):
    """bn_finalize_p for SyncBatchNorm in ONE launch: this rank's partial rows are summed, the
    sums and the local element count exchanged through the peer mailbox inside the kernel, and
    the global statistics finalized -> mean, invstd, scale, shift, global count (float64 [1])."""
    R = partial.shape[0]
    C = partial.numel() // (2 * R)
    out = torch.empty((4, C), dtype=torch.float32, device=partial.device)
    cnt = torch.empty(1, dtype=torch.float64, device=partial.device)
    ws = _ws(R, C, partial.device)
    LIB.call("seg_bn_finalize_p_sync", box.handle, _p(partial), R, float(local_count), _p(gamma),
             _p(beta), float(eps), float(momentum), _p(running_mean), _p(running_var), _p(out[0]),
             _p(out[1]), _p(out[2]), _p(out[3]), C, _p(mean_offset), _p(cnt), _p(ws), _stream())
    return out[0], out[1], out[2], out[3], cnt


def bn_bwd_finalize_p_sync(box, partial, count_dev, mean, invstd, gamma, grad_scale):
    C = mean.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=mean.device)
    ws = _ws(partial.shape[0], C, mean.device)
    LIB.call("seg_bn_bwd_finalize_p_sync", box.handle, _p(partial), partial.shape[0], _p(count_dev),
             _p(mean), _p(invstd), _p(gamma), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), C,
             float(grad_scale), _p(ws), _stream())
    return out[0], out[1], out[2], out[3]


def bn_bwd_finalize_p(partial, count, mean, invstd, gamma):
    R = partial.shape[0]
    C = mean.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=mean.device)
    ws = _ws(R, C, mean.device)
    LIB.call("seg_bn_bwd_finalize_p", _p(partial), R, float(count), _p(mean), _p(invstd),
             _p(gamma), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), C, _p(ws), _stream())
    return out[0], out[1], out[2], out[3]


def bn_bwd_finalize(sums, count, mean, invstd, gamma, grad_scale=1.0):
    """grad_scale multiplies dgamma / dbeta only (SyncBatchNorm: 1 / world size)."""
    C = mean.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=mean.device)
    LIB.call("seg_bn_bwd_finalize_s", _p(sums), *_count(count), _p(mean), _p(invstd), _p(gamma),
             _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), C, float(grad_scale), _stream())
    return out[0], out[1], out[2], out[3]  # dgamma, dbeta, c0, c1


def bn_bwd_apply(g, x, pro, c0=None, c1=None, chan_mul=None, out=None, elem_mul=None, add=None,
                 add_pro=None):
    """add: the gradient another consumer of the same raw tensor parked (the output's shape and
    dtype), joined in the same pass.  add_pro None: it is w.r.t. the raw tensor and is added as it
    is; (mode, c0', c1'): it is w.r.t. that consumer's activated input (prologue bits `mode` on
    the same scale / shift) and takes its own BatchNorm backward with ITS coefficients first.
    Either way the result is bit for bit sum_n([this apply, that consumer's own dx])."""
    N, H, W, C, ldg = nhwc(g)
    ldx = nhwc(x)[4]
    mode, s, t = _pro(pro)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=g.dtype, device=g.device)
    lddx = nhwc(out)[4]
    if add is not None:
        assert chan_mul is None and elem_mul is None
        assert tuple(add.shape) == (N, H, W, C) and add.dtype == out.dtype
        am, ac0, ac1 = add_pro if add_pro is not None else (0, None, None)
        LIB.call("seg_bn_bwd_apply_add", _DT[g.dtype], _p(g), ldg, _p(x), ldx, mode, _p(s), _p(t),
                 _p(c0), _p(c1), _p(add), nhwc(add)[4], int(am), _p(ac0), _p(ac1), _p(out), lddx,
                 N * H * W, C, _stream())
        return out
    ldm = nhwc(elem_mul)[4] if elem_mul is not None else 0
    LIB.call("seg_bn_bwd_apply", _DT[g.dtype], _p(g), ldg, _p(x), ldx, mode, _p(s), _p(t), _p(c0),
             _p(c1), _p(chan_mul), H * W, _p(elem_mul), ldm, _p(out), lddx, N * H * W, C,
             _stream())
    return out


# ----------------------------------------------------------------------------- BN fold
def fold_weights(w2d, scale, shift, dtype, want_transpose=False, want_bias=True):
    """fp32 W [O,C] -> (W*scale in dtype, its transpose [C,O] or None, W@shift fp32 or None)."""
    O, C = w2d.shape
    dev = w2d.device
    wp = torch.empty((O, C), dtype=dtype, device=dev)
    wpt = torch.empty((C, O), dtype=dtype, device=dev) if want_transpose else None
    bp = torch.empty(O, dtype=torch.float32, device=dev) if want_bias else None
    LIB.call("seg_fold_weights", _DT[dtype], _p(w2d), _p(scale), _p(shift), _p(wp), _p(wpt),
             _p(bp), O, C, _stream())
    return wp, wpt, bp


def fold_bwd_reduce(w2d, dwp, scale, shift, db=None):
    """dwp: dW' [O, C] or the weight-gradient split partials [S, O*C].
    -> (dW fp32 [O,C], dsdt fp32 [R, 2C] partial rows for fold_bwd_finalize)."""
    O, C = w2d.shape
    S = 1 if tuple(dwp.shape) == (O, C) else dwp.shape[0]
    assert dwp.numel() == S * O * C and dwp.is_contiguous()
    R = LIB.query("seg_fold_bwd_rows", O)
    if S > 8 and R == 1:
        # a narrow conv on a huge map (decoder c1_block: 256 -> 48 on 263 k pixels, 256 pixel
        # splits): the fold reduction would walk all S partials with ONE row group of blocks
        # (184 us for 12.6 MB) — sum the splits with the wide column-sum kernel first
        dwp = colsum(dwp.view(S, O * C), f64=False).view(O, C)
        S = 1
    dW = torch.empty((O, C), dtype=torch.float32, device=w2d.device)
    dsdt = torch.empty((R, 2 * C), dtype=torch.float32, device=w2d.device)
    LIB.call("seg_fold_bwd_reduce", _p(w2d), _p(dwp), S, _p(scale), _p(shift), _p(db), _p(dW),
             _p(dsdt), O, C, _stream())
    return dW, dsdt


def fold_bwd_finalize(dsdt, count, mean, invstd, gamma, scale, grad_scale=1.0):
    C = mean.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=mean.device)
    dsdt = dsdt.view(-1, 2 * C)
    LIB.call("seg_fold_bwd_finalize_s", _p(dsdt), dsdt.shape[0], *_count(count), _p(mean),
             _p(invstd), _p(gamma), _p(scale), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), C,
             float(grad_scale), _stream())
    return out[0], out[1], out[2], out[3]  # dgamma, dbeta, c0, c1


def fold_bwd_finalize_sync(box, dsdt, count_dev, mean, invstd, gamma, scale, grad_scale):
    """fold_bwd_finalize for SyncBatchNorm: dsdt = this rank's LOCAL (ds, dt) partial rows; the
    exchange happens inside the kernel."""
    C = mean.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=mean.device)
    dsdt = dsdt.view(-1, 2 * C)
    LIB.call("seg_fold_bwd_finalize_sync", box.handle, _p(dsdt), dsdt.shape[0], _p(count_dev),
             _p(mean), _p(invstd), _p(gamma), _p(scale), _p(out[0]), _p(out[1]), _p(out[2]),
             _p(out[3]), C, float(grad_scale), _stream())
    return out[0], out[1], out[2], out[3]


# ----------------------------------------------------------------------------- pooling
def maxpool(x, k, stride, pad, pro=None):
    """-> (y, idx uint8): y = maxpool(act(x)), -inf padding."""
    N, Hi, Wi, C, ldx = nhwc(x)
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    mode, ps, pt = _pro(pro)
    y = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    idx = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    LIB.call("seg_maxpool_fwd", _DT[x.dtype], _p(x), ldx, N, Hi, Wi, C, k, stride, pad, mode,
             _p(ps), _p(pt), _p(y), C, Ho, Wo, _p(idx), _stream())
    return y, idx


def maxpool_bwd(gy, idx, in_hw, k, stride, pad):
    N, Ho, Wo, C, ldgy = nhwc(gy)
    Hi, Wi = in_hw
    gx = torch.empty((N, Hi, Wi, C), dtype=gy.dtype, device=gy.device)
    LIB.call("seg_maxpool_bwd", _DT[gy.dtype], _p(gx), C, N, Hi, Wi, C, k, stride, pad, _p(gy),
             ldgy, Ho, Wo, _p(idx), _stream())
    return gx


def adaptive_avgpool_sums(x, o):
    """-> fp32 [N, o, o, C] bin SUMS (caller divides by the bin areas)."""
    N, H, W, C, ldx = nhwc(x)
    chunks = LIB.query("seg_adaptive_avgpool_chunks", H, W, o)
    partial = torch.empty((chunks, N * o * o * C), dtype=torch.float32, device=x.device)
    LIB.call("seg_adaptive_avgpool_partial", _DT[x.dtype], _p(x), ldx, N, H, W, C, o, _p(partial),
             chunks, _stream())
    sums = partial[0] if chunks == 1 else colsum(partial, f64=False)
    return sums.view(N, o, o, C)


def adaptive_avgpool_bwd(gy, in_hw):
    N, o, _, C, ldgy = nhwc(gy)
    H, W = in_hw
    gx = torch.empty((N, H, W, C), dtype=gy.dtype, device=gy.device)
    LIB.call("seg_adaptive_avgpool_bwd", _DT[gy.dtype], _p(gx), C, N, H, W, C, o, _p(gy), ldgy,
             _stream())
    return gx


# ---- channel attention: squeeze + sigmoid gate (csrc/chan_gate.hip) ----------------------------
def _gate_chunks(N, HW, C):
    chunks = LIB.query("seg_apply_pool_chunks", N, HW, C)
    if chunks < 1:
        raise ValueError("seg_apply_pool_chunks(%d, %d, %d): empty tensor" % (N, HW, C))
    return chunks


def _nc(t, N, C, what):
    if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N * C):
        raise RuntimeError("%s: expected a contiguous float32 [%d, %d] tensor" % (what, N, C))
    return t


def apply_pool(x, pro=None, want_y=True, out=None):
    """-> (y = act(x) in x.dtype | None, sums fp32 [N, C] of the fp32 activated values per image):
    one pass, all images in one launch."""
    N, H, W, C, ldx = nhwc(x)
    mode, s, t = _pro(pro)
    y, ldy = None, 0
    if want_y:
        y = out if out is not None else torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
        assert tuple(y.shape) == (N, H, W, C) and y.dtype == x.dtype
        ldy = nhwc(y)[4]
    chunks = _gate_chunks(N, H * W, C)
    partial = torch.empty((chunks, N * C), dtype=torch.float32, device=x.device)
    LIB.call("seg_apply_pool_fwd", _DT[x.dtype], _p(x), ldx, mode, _p(s), _p(t), _p(y), ldy, N,
             H * W, C, _p(partial), chunks, _stream())
    sums = partial[0] if chunks == 1 else colsum(partial, f64=False)
    return y, sums.view(N, C)


def chan_gate(x, a, identity=False, r=None, radd=None, out=None):
    """y = x * (identity + sigmoid(a[n][c])) + r + radd[n][c]; a / radd fp32 [N, C]."""
    N, H, W, C, ldx = nhwc(x)
    _nc(a, N, C, "chan_gate a")
    _nc(radd, N, C, "chan_gate radd")
    ldr = 0
    if r is not None:
        assert tuple(r.shape) == (N, H, W, C) and r.dtype == x.dtype
        ldr = nhwc(r)[4]
    if out is None:
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    assert tuple(out.shape) == (N, H, W, C) and out.dtype == x.dtype
    LIB.call("seg_chan_gate_fwd", _DT[x.dtype], _p(x), ldx, _p(a), int(bool(identity)), _p(r), ldr,
             _p(radd), _p(out), nhwc(out)[4], N, H * W, C, _gate_chunks(N, H * W, C), _stream())
    return out


def chan_gate_bwd(dy, x, a, identity=False, want_dx=True, want_da=True, want_dradd=True):
    """-> (dx = dy * (identity + sigmoid(a)), da = s(1-s) * sum_hw dy*x, dradd = sum_hw dy)."""
    N, H, W, C, lddy = nhwc(dy)
    assert tuple(x.shape) == (N, H, W, C) and x.dtype == dy.dtype
    _nc(a, N, C, "chan_gate_bwd a")
    ldx = nhwc(x)[4]
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device) if want_dx else None
    chunks = _gate_chunks(N, H * W, C)
    partial = torch.empty((chunks, N, 2, C), dtype=torch.float32, device=dy.device)
    LIB.call("seg_chan_gate_bwd", _DT[dy.dtype], _p(dy), lddy, _p(x), ldx, _p(a),
             int(bool(identity)), _p(dx), C, N, H * W, C, _p(partial), chunks, _stream())
    da = torch.empty((N, C), dtype=torch.float32, device=dy.device) if want_da else None
    dradd = torch.empty((N, C), dtype=torch.float32, device=dy.device) if want_dradd else None
    if want_da or want_dradd:
        LIB.call("seg_chan_gate_bwd_finalize", _p(partial), chunks, N, C, _p(a), _p(da), _p(dradd),
                 _stream())
    return dx, da, dradd


def bcast_add(g, v, scale, like=None, inplace=True):
    """g[n,h,w,c] += v[n][c] * scale (v fp32 [N, C]), in place or (`inplace` False) into a fresh
    tensor; g None: a fresh tensor shaped and typed `like` that holds the broadcast alone."""
    ref = g if g is not None else like
    N, H, W, C, ldr = nhwc(ref)
    _nc(v, N, C, "bcast_add v")
    ldg = 0 if g is None else ldr
    if g is None or not inplace:
        out = torch.empty((N, H, W, C), dtype=ref.dtype, device=ref.device)
    else:
        out = g
    LIB.call("seg_bcast_add", _DT[out.dtype], _p(g), ldg, _p(v), float(scale), _p(out),
             nhwc(out)[4], N, H * W, C, _gate_chunks(N, H * W, C), _stream())
    return out


# ---- CGNet's ContextGuidedBlock (csrc/cgnet.hip) -------------------------------------------------
def round_up8(C):
    """Channel width of a buffer that holds C channels for the kernels of csrc/cgnet.hip."""
    return (C + 7) // 8 * 8


def _padded_view(t, N, H, W, C, what, dtype=None):
    """-> the row pitch of `t`, an NHWC view of C (or C rounded up to 8) channels whose rows hold C
    rounded up to 8 elements — the element-wise kernels of csrc/cgnet.hip read and write whole
    channel vectors up to there."""
    n, h, w, c, ld = nhwc(t)
    Cp = round_up8(C)
    if (n, h, w) != (N, H, W) or c not in (C, Cp) or (dtype is not None and t.dtype != dtype):
        raise RuntimeError("%s: expected %s %s (or %d channels), got %s %s"
                           % (what, (N, H, W, C), dtype, Cp, tuple(t.shape), t.dtype))
    if n * h * w == 1 and c < Cp:
        # (a single row has no pitch that could show the room behind its C channels)
        raise RuntimeError("%s: a single-row tensor of a ragged channel count is passed as the "
                           "view of all %d channels of its buffer, got %d" % (what, Cp, c))
    if ld < Cp or ld % vec_of(t.dtype) != 0:
        raise RuntimeError("%s: row pitch %d does not hold %d channels in whole %d-element vectors"
                           % (what, ld, Cp, vec_of(t.dtype)))
    return ld


def _chan_param(t, C, what):
    if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                              and t.numel() == C):
        raise RuntimeError("%s: expected a contiguous float32 device tensor of %d elements"
                           % (what, C))
    return t


def bn_prelu(x, alpha, scale=None, shift=None, want_y=True, pool=False, out=None):
    """-> (y | None, sums fp32 [N, C] | None): y = prelu(x * scale + shift, alpha) (scale / shift
    None: plain PReLU) and, with `pool`, the per-image sums of the fp32 activated values, in one
    pass.  C = alpha.numel() may be ragged (35, 131): x and y are views of C or round_up8(C)
    channels whose row pitch holds round_up8(C); y is allocated at round_up8(C) channels and its
    channels beyond C are written as zeros; the parameter arrays have exactly C elements."""
    C = alpha.numel()
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    ldx = _padded_view(x, N, H, W, C, "bn_prelu x")
    _chan_param(alpha, C, "bn_prelu alpha")
    _chan_param(scale, C, "bn_prelu scale")
    _chan_param(shift, C, "bn_prelu shift")
    if (scale is None) != (shift is None):
        raise RuntimeError("bn_prelu: scale and shift go together")
    if not (want_y or pool):
        raise RuntimeError("bn_prelu: neither y nor the pooled sums wanted")
    y, ldy = None, 0
    if want_y:
        y = out if out is not None else \
            torch.empty((N, H, W, round_up8(C)), dtype=x.dtype, device=x.device)
        ldy = _padded_view(y, N, H, W, C, "bn_prelu out", x.dtype)
    chunks = _gate_chunks(N, H * W, C)
    partial = torch.empty((chunks, N * C), dtype=torch.float32, device=x.device) if pool else None
    LIB.call("seg_bn_prelu_fwd", _DT[x.dtype], _p(x), ldx, _p(scale), _p(shift), _p(alpha), _p(y),
             ldy, N, H * W, C, _p(partial), chunks, _stream())
    sums = None
    if pool:
        sums = (partial[0] if chunks == 1 else colsum(partial, f64=False)).view(N, C)
    return y, sums


def prelu_bwd(g_y, g_pool, x, alpha, scale=None, shift=None, out=None):
    """PReLU backward behind bn_prelu -> (g_z, dalpha fp32 [C]): g = g_y + g_pool[n][c] / HW
    (either may be None), z = x * scale + shift recomputed, g_z = z > 0 ? g : alpha * g (the slope
    at z == 0 is alpha, as torch), dalpha = sum over z <= 0 of g * z.  g_z has round_up8(C)
    channels, zeros beyond C: it goes to bn_bwd_* / the producer at that width."""
    C = alpha.numel()
    N, H, W = x.shape[0], x.shape[1], x.shape[2]
    ldx = _padded_view(x, N, H, W, C, "prelu_bwd x")
    _chan_param(alpha, C, "prelu_bwd alpha")
    _chan_param(scale, C, "prelu_bwd scale")
    _chan_param(shift, C, "prelu_bwd shift")
    if (scale is None) != (shift is None):
        raise RuntimeError("prelu_bwd: scale and shift go together")
    if g_y is None and g_pool is None:
        raise RuntimeError("prelu_bwd: no gradient at all")
    ldgy = 0 if g_y is None else _padded_view(g_y, N, H, W, C, "prelu_bwd g_y", x.dtype)
    _nc(g_pool, N, C, "prelu_bwd g_pool")
    g_z = out if out is not None else \
        torch.empty((N, H, W, round_up8(C)), dtype=x.dtype, device=x.device)
    ldgz = _padded_view(g_z, N, H, W, C, "prelu_bwd out", x.dtype)
    chunks = _gate_chunks(N, H * W, C)
    partial = torch.empty((chunks * N, C), dtype=torch.float32, device=x.device)
    LIB.call("seg_prelu_bwd", _DT[x.dtype], _p(g_y), ldgy, _p(g_pool), _p(x), ldx, _p(scale),
             _p(shift), _p(alpha), _p(g_z), ldgz, N, H * W, C, _p(partial), chunks, _stream())
    return g_z, colsum(partial, f64=False)


def _cg_weights(w_loc, w_sur, C):
    for w in (w_loc, w_sur):
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
                and tuple(w.shape) == (C, 1, 3, 3)):
            raise RuntimeError("cg_joint: the weights are contiguous float32 [%d,1,3,3] device "
                               "tensors, got %s %s" % (C, tuple(w.shape), w.dtype))


def _cg_chunks(N, H, W, C):
    chunks = LIB.query("seg_cg_joint_chunks", N, H, W, C)
    if chunks < 1:
        raise ValueError("seg_cg_joint_chunks(%d, %d, %d, %d): empty tensor, or C is not a "
                         "multiple of 4" % (N, H, W, C))
    return chunks


def cg_joint(x, w_loc, w_sur, dil, out=None, want_stats=True):
    """-> (joi [N,H,W,2C], partial fp32 [rows, 2, 2C] | None): joi[..., :C] = depthwise 3x3 of x
    with w_loc (pad 1), joi[..., C:] = depthwise 3x3 with w_sur (pad = dilation = dil), one pass
    over x; partial: sum | sum of squares of the fp32 accumulators for finish_bn."""
    N, H, W, C, ldx = nhwc(x)
    _cg_weights(w_loc, w_sur, C)
    if out is None:
        out = torch.empty((N, H, W, 2 * C), dtype=x.dtype, device=x.device)
    if tuple(out.shape) != (N, H, W, 2 * C) or out.dtype != x.dtype:
        raise RuntimeError("cg_joint out: expected %s %s, got %s %s"
                           % ((N, H, W, 2 * C), x.dtype, tuple(out.shape), out.dtype))
    chunks = _cg_chunks(N, H, W, C)
    partial = torch.empty((chunks * N, 2, 2 * C), dtype=torch.float32, device=x.device) \
        if want_stats else None
    LIB.call("seg_cg_joint_fwd", _DT[x.dtype], _p(x), ldx, N, H, W, C, _p(w_loc), _p(w_sur),
             int(dil), _p(out), nhwc(out)[4], _p(partial), chunks, _stream())
    return out, partial


# ---- ESPNetv2's EESP unit and DownSampler (csrc/espnetv2.hip) ------------------------------------
def _eesp_weights(ws, n):
    if len(ws) != 4:
        raise RuntimeError("eesp_pyramid: four branch weights, got %d" % len(ws))
    for w in ws:
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
                and tuple(w.shape) == (n, 1, 3, 3)):
            raise RuntimeError("eesp_pyramid: the weights are contiguous float32 [%d,1,3,3] device "
                               "tensors, got %s %s" % (n, tuple(w.shape), w.dtype))


def eesp_pyramid(x, ws, dils, stride, out=None, want_stats=True):
    """-> (y [N,Ho,Wo,4n], partial fp32 [rows, 2, 4n] | None): y[..., j*n:(j+1)*n] = the sum over
    i <= j of the depthwise 3x3 of x with ws[i] (pad = dilation = dils[i], `stride`), one pass over
    x; partial: sum | sum of squares of the fp32 values for finish_bn.  The launcher refuses n that
    is no multiple of 8, dilations outside 1..4 or decreasing, and strides other than 1 and 2."""
    N, H, W, n, ldx = nhwc(x)
    _eesp_weights(ws, n)
    dils = [int(d) for d in dils]
    if len(dils) != 4:
        raise RuntimeError("eesp_pyramid: four dilations, got %s" % (dils,))
    stride = int(stride)
    Ho = (H - 1) // stride + 1 if stride > 0 else 0
    Wo = (W - 1) // stride + 1 if stride > 0 else 0
    if out is None:
        out = torch.empty((N, Ho, Wo, 4 * n), dtype=x.dtype, device=x.device)
    if tuple(out.shape) != (N, Ho, Wo, 4 * n) or out.dtype != x.dtype:
        raise RuntimeError("eesp_pyramid out: expected %s %s, got %s %s"
                           % ((N, Ho, Wo, 4 * n), x.dtype, tuple(out.shape), out.dtype))
    chunks = LIB.query("seg_eesp_pyr_chunks", N, H, W, n, stride)
    if chunks < 1:
        chunks = 1  # (out of contract: the launcher below says what is wrong)
    partial = torch.empty((chunks * N, 2, 4 * n), dtype=torch.float32, device=x.device) \
        if want_stats else None
    LIB.call("seg_eesp_pyr_fwd", _DT[x.dtype], _p(x), ldx, N, H, W, n, _p(ws[0]), _p(ws[1]),
             _p(ws[2]), _p(ws[3]), dils[0], dils[1], dils[2], dils[3], stride, _p(out),
             nhwc(out)[4], _p(partial), chunks, _stream())
    return out, partial


def eesp_suffix_sum(g, out=None):
    """g [N,H,W,4n] -> S with S[..., j*n:(j+1)*n] = sum over i >= j of g's slice i (fp32 sums, one
    rounding): the gradients the four branches of the pyramid see.  out may be g."""
    N, H, W, C4, ldg = nhwc(g)
    if C4 % 4 != 0:
        raise RuntimeError("eesp_suffix_sum: %d channels are not four slices" % C4)
    if out is None:
        out = torch.empty((N, H, W, C4), dtype=g.dtype, device=g.device)
    if tuple(out.shape) != (N, H, W, C4) or out.dtype != g.dtype:
        raise RuntimeError("eesp_suffix_sum out: expected %s %s" % ((N, H, W, C4), g.dtype))
    LIB.call("seg_eesp_suffix_sum", _DT[g.dtype], _p(g), ldg, _p(out), nhwc(out)[4], N * H * W,
             C4 // 4, _stream())
    return out


def avgpool3x3s2(x, out=None):
    """nn.AvgPool2d(3, 2, 1) (count_include_pad: divisor 9 everywhere) -> [N, (H-1)//2+1,
    (W-1)//2+1, C]."""
    N, H, W, C, ldx = nhwc(x)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    if tuple(out.shape) != (N, Ho, Wo, C) or out.dtype != x.dtype:
        raise RuntimeError("avgpool3x3s2 out: expected %s %s" % ((N, Ho, Wo, C), x.dtype))
    LIB.call("seg_avgpool3x3s2_fwd", _DT[x.dtype], _p(x), ldx, N, H, W, C, _p(out), nhwc(out)[4],
             _stream())
    return out


def avgpool3x3s2_bwd(gy, in_hw, out=None):
    """Gradient of avgpool3x3s2 w.r.t. its [N, H, W, C] input (in_hw = (H, W)): a gather that
    writes every element once."""
    N, Ho, Wo, C, ldgy = nhwc(gy)
    H, W = in_hw
    if (Ho, Wo) != ((H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise RuntimeError("avgpool3x3s2_bwd: gy %s is not the pool of %s" % (tuple(gy.shape), in_hw))
    if out is None:
        out = torch.empty((N, H, W, C), dtype=gy.dtype, device=gy.device)
    if tuple(out.shape) != (N, H, W, C) or out.dtype != gy.dtype:
        raise RuntimeError("avgpool3x3s2_bwd out: expected %s %s" % ((N, H, W, C), gy.dtype))
    LIB.call("seg_avgpool3x3s2_bwd", _DT[gy.dtype], _p(gy), ldgy, N, H, W, C, _p(out),
             nhwc(out)[4], _stream())
    return out


def _same_nhwc(t, like, what):
    if tuple(t.shape) != tuple(like.shape) or t.dtype != like.dtype:
        raise RuntimeError("%s: expected %s %s, got %s %s"
                           % (what, tuple(like.shape), like.dtype, tuple(t.shape), t.dtype))
    return nhwc(t)[4]


def bn_add_prelu(a, b, alpha, aff_a=None, aff_b=None, out=None):
    """y = prelu(a * sa + ta + b * sb + tb, alpha); aff_a = (sa, ta) / aff_b = (sb, tb) fp32 [C],
    None: that operand is plain."""
    N, H, W, C, lda = nhwc(a)
    ldb = _same_nhwc(b, a, "bn_add_prelu b")
    _chan_param(alpha, C, "bn_add_prelu alpha")
    sa, ta = aff_a if aff_a is not None else (None, None)
    sb, tb = aff_b if aff_b is not None else (None, None)
    for t in (sa, ta, sb, tb):
        _chan_param(t, C, "bn_add_prelu scale / shift")
    if out is None:
        out = torch.empty((N, H, W, C), dtype=a.dtype, device=a.device)
    ldy = _same_nhwc(out, a, "bn_add_prelu out")
    LIB.call("seg_bn_add_prelu_fwd", _DT[a.dtype], _p(a), lda, _p(sa), _p(ta), _p(b), ldb, _p(sb),
             _p(tb), _p(alpha), _p(out), ldy, N, H * W, C, _gate_chunks(N, H * W, C), _stream())
    return out


def bn_add_prelu_bwd(g, a, b, alpha, aff_a=None, aff_b=None, out=None):
    """-> (g_z, dalpha fp32 [C]): z recomputed, g_z = z > 0 ? g : alpha * g (the slope at z == 0 is
    alpha, as torch), dalpha = sum over z <= 0 of g * z."""
    N, H, W, C, lda = nhwc(a)
    ldb = _same_nhwc(b, a, "bn_add_prelu_bwd b")
    ldg = _same_nhwc(g, a, "bn_add_prelu_bwd g")
    _chan_param(alpha, C, "bn_add_prelu_bwd alpha")
    sa, ta = aff_a if aff_a is not None else (None, None)
    sb, tb = aff_b if aff_b is not None else (None, None)
    for t in (sa, ta, sb, tb):
        _chan_param(t, C, "bn_add_prelu_bwd scale / shift")
    if out is None:
        out = torch.empty((N, H, W, C), dtype=a.dtype, device=a.device)
    ldgz = _same_nhwc(out, a, "bn_add_prelu_bwd out")
    chunks = _gate_chunks(N, H * W, C)
    partial = torch.empty((chunks * N, C), dtype=torch.float32, device=a.device)
    LIB.call("seg_bn_add_prelu_bwd", _DT[a.dtype], _p(g), ldg, _p(a), lda, _p(sa), _p(ta), _p(b),
             ldb, _p(sb), _p(tb), _p(alpha), _p(out), ldgz, N, H * W, C, _p(partial), chunks,
             _stream())
    return out, colsum(partial, f64=False)


def chan_moments(x):
    """Per-channel (sum, sum of squares) partial rows fp32 [R, 2, C] of a plain pitched NHWC tensor
    for finish_bn — the existing seg_bn_bwd_reduce with g = x and no prologue (column sums of
    (x, x*x), as functional._GapFn uses it)."""
    C = x.shape[-1]
    return bn_bwd_reduce_partial(x, x, None).view(-1, 2, C)


_BIN_AREAS = {}


def adaptive_bin_areas(H, W, o, device):
    """[o, o] fp32 areas of ATen's adaptive-pool bins (cached per geometry: a host-to-device
    copy must not happen inside a HIP-graph capture)."""
    key = (H, W, o, str(device))
    if key not in _BIN_AREAS:
        _BIN_AREAS[key] = _adaptive_bin_areas(H, W, o, device)
    return _BIN_AREAS[key]


def _adaptive_bin_areas(H, W, o, device):
    import math
    hs = [math.ceil((i + 1) * H / o) - (i * H) // o for i in range(o)]
    ws = [math.ceil((j + 1) * W / o) - (j * W) // o for j in range(o)]
    return torch.tensor([[float(a * b) for b in ws] for a in hs], device=device)


# ----------------------------------------------------------------------------- resize
def bilinear(x, out_hw, pro=None, chan_mul=None, align_corners=True, out=None):
    N, Hi, Wi, C, ldx = nhwc(x)
    Ho, Wo = out_hw
    mode, s, t = _pro(pro)
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    ldy = nhwc(out)[4]
    LIB.call("seg_bilinear_fwd", _DT[x.dtype], _p(x), ldx, N, Hi, Wi, C, mode, _p(s), _p(t),
             _p(chan_mul), _p(out), ldy, Ho, Wo, int(align_corners), _stream())
    return out


def bilinear_bwd(gy, in_hw, align_corners=True):
    N, Ho, Wo, C, ldgy = nhwc(gy)
    Hi, Wi = in_hw
    gx = torch.empty((N, Hi, Wi, C), dtype=gy.dtype, device=gy.device)
    LIB.call("seg_bilinear_bwd", _DT[gy.dtype], _p(gx), C, N, Hi, Wi, C, _p(gy), ldgy, Ho, Wo,
             int(align_corners), _stream())
    return gx


def upsample_to_nchw(x, C, out_hw, align_corners=True):
    """x: NHWC view whose first C channels are valid -> float32 NCHW [N,C,Ho,Wo]."""
    N, Hi, Wi, _, ldx = nhwc(x)
    Ho, Wo = out_hw
    out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    LIB.call("seg_upsample_to_nchw", _DT[x.dtype], _p(x), ldx, N, Hi, Wi, C, _p(out), Ho, Wo,
             int(align_corners), _stream())
    return out


def upsample_to_nchw_bwd(gy, in_hw, dtype, pitch, align_corners=True):
    """gy float32 NCHW -> NHWC [N,Hi,Wi,pitch] of `dtype` (channels >= C are zero)."""
    if not gy.is_cuda or gy.dtype != torch.float32:
        raise RuntimeError("upsample_to_nchw_bwd needs a float32 HIP device tensor")
    N, C, Ho, Wo = gy.shape
    Hi, Wi = in_hw
    gy = gy.contiguous()
    gx = torch.empty((N, Hi, Wi, pitch), dtype=dtype, device=gy.device)
    LIB.call("seg_upsample_to_nchw_bwd", _DT[dtype], _p(gx), pitch, N, Hi, Wi, C, _p(gy), Ho, Wo,
             int(align_corners), _stream())
    return gx


def nchw_to_nhwc_pad(x, dtype):
    """float32 NCHW image (C <= 16B/elem) -> NHWC [N,H,W,VEC] zero-padded."""
    if not x.is_cuda:
        raise RuntimeError("segmentron_amd ops need HIP device tensors (no CPU fallback)")
    N, Cin, H, W = x.shape
    x = x.contiguous().float()
    y = torch.empty((N, H, W, vec_of(dtype)), dtype=dtype, device=x.device)
    LIB.call("seg_nchw_to_nhwc_pad", _DT[dtype], _p(x), N, Cin, H, W, _p(y), _stream())
    return y


# ----------------------------------------------------------------------------- fused loss tail
def upsample_ce_fwd(lo, target, out_hw, ignore_index, align_corners=True):
    """lo: NHWC logits view [N,Hi,Wi,C] of a channel-padded buffer; target int64 [N,H,W].
    -> float32[2] device tensor (mean cross-entropy over valid pixels, 1 / valid count)."""
    N, Hi, Wi, C, ld = nhwc(lo)
    H, W = out_hw
    if not target.is_cuda or target.dtype != torch.int64 or tuple(target.shape) != (N, H, W):
        raise RuntimeError("upsample_ce: target must be an int64 HIP tensor [N, H, W] = %s, got %s"
                           % ((N, H, W), tuple(target.shape)))
    target = target.contiguous()
    blocks = LIB.query("seg_upsample_ce_blocks", N, H, W)
    ws = torch.empty(2 * blocks, dtype=torch.float64, device=lo.device)
    out = torch.empty(2, dtype=torch.float32, device=lo.device)
    LIB.call("seg_upsample_ce_fwd", _DT[lo.dtype], _p(lo), ld, N, Hi, Wi, C, _p(target), H, W,
             int(ignore_index), int(align_corners), _p(ws), _p(out), _stream())
    return out


def upsample_ce_bwd(lo, target, out_hw, ignore_index, loss_out, grad_out, pitch,
                    align_corners=True):
    """-> d(loss)/d(lo) * grad_out as NHWC [N,Hi,Wi,pitch] in lo.dtype (channels >= C zero)."""
    N, Hi, Wi, C, ld = nhwc(lo)
    H, W = out_hw
    grad_out = grad_out.reshape(1).to(torch.float32).contiguous()
    dlo = torch.empty((N, Hi, Wi, pitch), dtype=lo.dtype, device=lo.device)
    # fp32 [N, H, Wi, C] between the row pass and the column pass (under graph capture it comes from
    # the graph's pool like every other temporary)
    ws_bytes = LIB.query("seg_upsample_ce_bwd_ws_bytes", N, H, Wi, C)
    if ws_bytes < 0:
        raise RuntimeError("upsample_ce_bwd: workspace for N=%d H=%d Wi=%d C=%d exceeds 2 GiB"
                           % (N, H, Wi, C))
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=lo.device)
    LIB.call("seg_upsample_ce_bwd", _DT[lo.dtype], _p(lo), ld, N, Hi, Wi, C,
             _p(target.contiguous()), H, W, int(ignore_index), int(align_corners), _p(loss_out),
             _p(grad_out), _p(dlo), pitch, _p(ws), ws_bytes, _stream())
    return dlo


# ----------------------------------------------------------------------------- DUpsampling
def _dup_geometry(lo, s, C, what):
    """-> (N, h, w, ld) of the NHWC output of DUpsampling's 1x1 convolution (s*s*C channels)."""
    N, h, w, K, ld = nhwc(lo)
    if lo.dtype not in _DT:
        raise RuntimeError("%s: float32 or bfloat16 logits, got %s" % (what, lo.dtype))
    if K != s * s * C:
        raise RuntimeError("%s: %d channels are not s*s*C = %d*%d*%d" % (what, K, s, s, C))
    return N, h, w, ld


def dup_ce_fwd(lo, target, s, C, ignore_index):
    """F.cross_entropy(DUpsampling(lo), target, ignore_index) on the low-resolution NHWC tensor
    lo [N, h, w, s*s*C]; target int64 [N, h*s, w*s].  -> float32[2] device tensor (mean loss over
    the valid pixels, 1 / valid count)."""
    N, h, w, ld = _dup_geometry(lo, s, C, "dup_ce")
    if not target.is_cuda or target.dtype != torch.int64 \
            or tuple(target.shape) != (N, h * s, w * s):
        raise RuntimeError("dup_ce: target must be an int64 HIP tensor [N, H, W] = %s, got %s"
                           % ((N, h * s, w * s), tuple(target.shape)))
    blocks = LIB.query("seg_dup_ce_blocks", _DT[lo.dtype], ld, N, h, w, s, C)
    ws = torch.empty(2 * max(blocks, 1), dtype=torch.float64, device=lo.device)
    out = torch.empty(2, dtype=torch.float32, device=lo.device)
    LIB.call("seg_dup_ce_fwd", _DT[lo.dtype], _p(lo), ld, N, h, w, s, C, _p(target.contiguous()),
             int(ignore_index), _p(ws), _p(out), _stream())
    return out


def dup_ce_bwd(lo, target, s, C, ignore_index, loss_out, grad_out, pitch=None):
    """-> d(loss)/d(lo) * grad_out as NHWC [N, h, w, pitch] in lo.dtype (channels >= s*s*C and
    the rows of invalid pixels are zero); pitch defaults to s*s*C rounded up to a vector."""
    N, h, w, ld = _dup_geometry(lo, s, C, "dup_ce_bwd")
    vec = vec_of(lo.dtype)
    pitch = pitch or (s * s * C + vec - 1) // vec * vec
    grad_out = grad_out.reshape(1).to(torch.float32).contiguous()
    dlo = torch.empty((N, h, w, pitch), dtype=lo.dtype, device=lo.device)
    LIB.call("seg_dup_ce_bwd", _DT[lo.dtype], _p(lo), ld, N, h, w, s, C, _p(target.contiguous()),
             int(ignore_index), _p(loss_out), _p(grad_out), _p(dlo), pitch, _stream())
    return dlo


def dup_to_nchw(lo, s, C):
    """lo NHWC [N, h, w, s*s*C] -> DUpsampling's float32 NCHW [N, C, h*s, w*s]."""
    N, h, w, ld = _dup_geometry(lo, s, C, "dup_to_nchw")
    out = torch.empty((N, C, h * s, w * s), dtype=torch.float32, device=lo.device)
    LIB.call("seg_dup_to_nchw", _DT[lo.dtype], _p(lo), ld, N, h, w, s, C, _p(out), _stream())
    return out


def dup_to_nchw_bwd(gy, s, dtype, pitch=None):
    """gy float32 NCHW [N, C, h*s, w*s] -> NHWC [N, h, w, pitch] of `dtype` (pad channels zero)."""
    if not gy.is_cuda or gy.dtype != torch.float32 or gy.dim() != 4:
        raise RuntimeError("dup_to_nchw_bwd needs a float32 HIP device tensor [N, C, H, W]")
    N, C, H, W = gy.shape
    if H % s or W % s:
        raise RuntimeError("dup_to_nchw_bwd: %d x %d is not a multiple of s = %d" % (H, W, s))
    vec = vec_of(dtype)
    pitch = pitch or (s * s * C + vec - 1) // vec * vec
    gx = torch.empty((N, H // s, W // s, pitch), dtype=dtype, device=gy.device)
    LIB.call("seg_dup_to_nchw_bwd", _DT[dtype], _p(gx), pitch, N, H // s, W // s, s, C,
             _p(gy.contiguous()), _stream())
    return gx


# ----------------------------------------------------------------------------- optimizer
def sgd_check(p, g, b):
    if not (p.is_cuda and g.is_cuda and b.is_cuda):
        raise RuntimeError("segmentron_amd SGD needs HIP device tensors (no CPU fallback)")
    if not (p.dtype == g.dtype == b.dtype == torch.float32):
        raise RuntimeError("segmentron_amd SGD: parameters / gradients / buffers are fp32")
    if not (p.is_contiguous() and g.is_contiguous() and b.is_contiguous()):
        raise RuntimeError("segmentron_amd SGD: non-contiguous tensor")
    if g.numel() != p.numel() or b.numel() != p.numel():
        raise RuntimeError("segmentron_amd SGD: size mismatch")


def pack_multi(jobs, dtype):
    """jobs: [(src fp32 [O, C] contiguous, transpose)] -> list of packed tensors in `dtype`
    ([O, C] or [C, O]) written by as few seg_pack_multi launches as possible."""
    import ctypes
    n = len(jobs)
    outs = []
    for src, tr in jobs:
        assert src.dtype == torch.float32 and src.is_cuda and src.is_contiguous() and src.dim() == 2
        O, C = src.shape
        outs.append(torch.empty((C, O) if tr else (O, C), dtype=dtype, device=src.device))
    vp = ctypes.c_void_p * n
    ci = ctypes.c_int * n
    LIB.call("seg_pack_multi", _DT[dtype], n, vp(*[j[0].data_ptr() for j in jobs]),
             vp(*[o.data_ptr() for o in outs]), ci(*[j[0].shape[0] for j in jobs]),
             ci(*[j[0].shape[1] for j in jobs]), ci(*[1 if j[1] else 0 for j in jobs]), _stream())
    return outs


def sgd_plan(params, bufs, groups):
    """The per-step-invariant half of a multi-tensor SGD launch: ctypes arrays of the parameter /
    buffer pointers, sizes and group indices (440 tensors: rebuilt only when they change)."""
    import ctypes
    n = len(params)
    vp = ctypes.c_void_p * n
    return (n, vp, vp(*[p.data_ptr() for p in params]), vp(*[b.data_ptr() for b in bufs]),
            (ctypes.c_long * n)(*[p.numel() for p in params]), (ctypes.c_int * n)(*groups))


def sgd_multi_tensor(plan, grads, lr_dev, wd_dev, momentum, first):
    """One fused SGD(momentum, weight decay) step over the tensors of `plan` (sgd_plan) with
    this step's gradient tensors (csrc/optim.hip); the plan's group indices address the DEVICE
    float arrays lr_dev / wd_dev."""
    n, vp, pp, pb, pn, pg = plan
    LIB.call("seg_sgd_multi_tensor", n, pp, vp(*[g.data_ptr() for g in grads]), pb, pn, pg,
             _p(lr_dev), _p(wd_dev), float(momentum), int(bool(first)), _stream())


# ----------------------------------------------------------------------------- metrics
def metric_counters(nclass, device):
    """Zeroed int64 [2 + 3*nclass]: correct, labelled, inter[], pred[], lab[] (csrc/metric.hip)."""
    return torch.zeros(2 + 3 * nclass, dtype=torch.int64, device=device)


def metric_update_nchw(logits, target, nclass, counters):
    """logits fp32 NCHW, target int64 [N,H,W]: accumulates score.py:83-113's counts."""
    if not (logits.is_cuda and target.is_cuda and counters.is_cuda):
        raise RuntimeError("segmentron_amd metrics need HIP device tensors (no CPU fallback)")
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        logits = logits.float().contiguous()
    if target.dtype != torch.int64 or not target.is_contiguous():
        target = target.long().contiguous()
    N, C, H, W = logits.shape
    assert tuple(target.shape) == (N, H, W) and counters.numel() == 2 + 3 * nclass
    LIB.call("seg_metric_update_nchw", _p(logits), N, C, H, W, _p(target), nclass, _p(counters),
             _stream())
    return counters


def metric_update_upsample(lo, target, align_corners, nclass, counters):
    """lo: NHWC logits [N,Hi,Wi,C]; the counts are taken on their bilinear upsample to the
    target's [H, W] without materialising it."""
    if not (lo.is_cuda and target.is_cuda and counters.is_cuda):
        raise RuntimeError("segmentron_amd metrics need HIP device tensors (no CPU fallback)")
    N, Hi, Wi, C, ld = nhwc(lo)
    if target.dtype != torch.int64 or not target.is_contiguous():
        target = target.long().contiguous()
    assert target.shape[0] == N and counters.numel() == 2 + 3 * nclass
    H, W = target.shape[1:]
    LIB.call("seg_metric_update_upsample", _DT[lo.dtype], _p(lo), ld, N, Hi, Wi, C, _p(target), H,
             W, int(bool(align_corners)), nclass, _p(counters), _stream())
    return counters


# ----------------------------------------------------------------------------- DANet attention
def row_softmax(e, L, out_dtype, sign=1.0):
    """e [R, Lp] (fp32 or bf16, row-major) -> a [R, Lp] in out_dtype: softmax over the first L
    columns of sign * e, zeros in the padding columns."""
    R, Lp = e.shape
    assert e.is_cuda and e.stride(1) == 1
    a = torch.empty((R, Lp), dtype=out_dtype, device=e.device)
    LIB.call("seg_row_softmax", _p(e), _DT[e.dtype], e.stride(0), _p(a), _DT[out_dtype], Lp, R, L,
             Lp, float(sign), _stream())
    return a


def row_softmax_bwd(a, g, L, out_dtype, sign=1.0):
    """de = sign * a * (g - sum_j a g) over the first L columns (zeros behind)."""
    R, Lp = a.shape
    assert a.stride(1) == 1 and g.stride(1) == 1 and tuple(g.shape) == (R, Lp)
    de = torch.empty((R, Lp), dtype=out_dtype, device=a.device)
    LIB.call("seg_row_softmax_bwd", _p(a), _DT[a.dtype], a.stride(0), _p(g), _DT[g.dtype],
             g.stride(0), _p(de), _DT[out_dtype], Lp, R, L, Lp, float(sign), _stream())
    return de


def gemm_nt(a, b):
    """a [P, K], b [O, K] (both compute dtype, row-major, K and O multiples of the channel
    vector) -> a @ b.T [P, O] in the compute dtype: a 1x1 convolution of the P "pixels" of a
    (seg_conv_gemm_fwd — fp32 MFMA accumulation)."""
    P, Kd = a.shape
    y, _ = conv_gemm(a.view(1, 1, P, Kd), b, b.shape[0], 1, 1, 1, 0, 1)
    return y.view(P, b.shape[0])


def gemm_tn(a, b):
    """a [P, M], b [P, K] -> a.T @ b [M, K] float32: the weight-gradient GEMM of a 1x1
    convolution (seg_conv_gemm_wgrad: sum over the P pixels, fixed-order fp32 partials)."""
    P, M = a.shape
    return conv_wgrad(b.view(1, 1, P, b.shape[1]), a.view(1, 1, P, M), M, 1, 1, 1, 0, 1)


# ----------------------------------------------------------------------------- criss-cross attention
def cca_attention(q, k):
    """q, k NHWC [N,H,W,C'] -> fp32 attention [N,H,W,W+H-1] = softmax over the criss-cross set."""
    N, H, W, C, ldq = nhwc(q)
    ldk = nhwc(k)[4]
    att = torch.empty((N, H, W, H + W - 1), dtype=torch.float32, device=q.device)
    LIB.call("seg_cca_attention", _DT[q.dtype], _p(q), ldq, _p(k), ldk, N, H, W, C, _p(att),
             _stream())
    return att


def cca_attention_bwd(dout, v, att, scale=None):
    """dE (fp32, like att): softmax backward of dA = scale * dout . v[partner]."""
    N, H, W, C, lddo = nhwc(dout)
    ldv = nhwc(v)[4]
    de = torch.empty_like(att)
    LIB.call("seg_cca_attention_bwd", _DT[v.dtype], _p(dout), lddo, _p(v), ldv, N, H, W, C,
             _p(att), _p(scale), _p(de), _stream())
    return de


def cca_map(wt, b, transposed=False, gamma=None, res=None, want_raw=False):
    """out[p] = gamma * sum_z wt(p, z) * b[partner(p, z)] (+ res[p]); transposed: summed over the
    pixels attending TO p.  -> out, or (out, raw sum) with want_raw."""
    N, H, W, C, ldb = nhwc(b)
    out = torch.empty((N, H, W, C), dtype=b.dtype, device=b.device)
    raw = torch.empty_like(out) if want_raw else None
    ldres = nhwc(res)[4] if res is not None else 0
    LIB.call("seg_cca_map", _DT[b.dtype], _p(wt), _p(b), ldb, N, H, W, C, int(bool(transposed)),
             _p(gamma), _p(res), ldres, _p(out), C, _p(raw), C, _stream())
    return (out, raw) if want_raw else out


# ----------------------------------------------------------------------------- PointRend
# A "map" is (tensor, sn, sp, sc, N, H, W, C): element (n, pixel, c) at n*sn + pixel*sp + c*sc.
def map_nhwc(t):
    """NHWC view (channel slice of a pitched buffer allowed) as a point-head map."""
    N, H, W, C, ld = nhwc(t)
    return (t, H * W * ld, ld, 1, N, H, W, C)


def map_nchw(t):
    """NCHW tensor (made contiguous) as a point-head map."""
    if not t.is_cuda:
        raise RuntimeError("segmentron_amd ops need HIP device tensors (no CPU fallback)")
    if t.dim() != 4 or t.dtype not in _DT:
        raise RuntimeError("expected a float32 / bfloat16 NCHW tensor, got %s %s"
                           % (tuple(t.shape), t.dtype))
    t = t.contiguous()
    N, C, H, W = t.shape
    return (t, C * H * W, 1, H * W, N, H, W, C)


def _points(pts, N):
    if not pts.is_cuda or pts.dtype != torch.float32 or pts.dim() != 3 or pts.shape[0] != N \
            or pts.shape[2] != 2:
        raise RuntimeError("points must be a float32 HIP tensor [%d, P, 2], got %s %s"
                           % (N, tuple(pts.shape), pts.dtype))
    return pts.contiguous()


def _rows(t):
    """-> (R, C, ld) of a 2-d row view [R, C] with row pitch ld."""
    if not t.is_cuda or t.dim() != 2 or (t.stride(1) != 1 and t.shape[1] > 1):
        raise RuntimeError("expected a 2-d HIP row view, got %s strides %s"
                           % (tuple(t.shape), t.stride()))
    return t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else t.shape[1]


def point_sample(m, pts, out=None, col=0, nearest=False):
    """grid_sample of map m at pts [N, P, 2] into rows out[N*P, ld][:, col:col+C] (allocated
    float32 [N*P, C] when None)."""
    t, sn, sp, sc, N, H, W, C = m
    pts = _points(pts, N)
    P = pts.shape[1]
    if out is None:
        out = torch.empty((N * P, C), dtype=torch.float32, device=t.device)
    R, _, ld = _rows(out)
    assert R == N * P and out.shape[1] >= col + C
    LIB.call("seg_point_sample", _DT[t.dtype], _p(t), sn, sp, sc, N, H, W, C, _p(pts), P,
             int(bool(nearest)), _DT[out.dtype], _p(out), ld, col, _stream())
    return out


def point_sample_bwd(g, col, C, pts, in_hw, dtype, pitch=None):
    """Bilinear backward of point_sample: rows g[N*P, ld][:, col:col+C] -> NHWC dx
    [N, H, W, pitch][..., :C] in `dtype` (every pixel written)."""
    N, P = pts.shape[0], pts.shape[1]
    pts = _points(pts, N)
    H, W = in_hw
    R, _, ldg = _rows(g)
    assert R == N * P and g.shape[1] >= col + C
    nws = LIB.query("seg_point_sample_bwd_ws", N, H, W, P)
    if nws < 0:
        raise RuntimeError("point_sample_bwd: geometry too large")
    ws = torch.empty(nws, dtype=torch.int32, device=g.device)
    pitch = pitch or C
    # the kernel writes channels [0, C): the pad of a pitched result is zeroed
    dx = (torch.zeros if pitch > C else torch.empty)((N, H, W, pitch), dtype=dtype,
                                                     device=g.device)
    LIB.call("seg_point_sample_bwd", _DT[g.dtype], _p(g), ldg, col, _p(pts), N, P, H, W, C,
             _DT[dtype], _p(dx), pitch, _p(ws), _stream())
    return dx if pitch == C else dx[..., :C]


def point_uncertainty(m, pts=None):
    """-(top1 - top2) over the channels: per pixel ([N, H*W]) or at pts ([N, P], rank planes
    interpolated)."""
    t, sn, sp, sc, N, H, W, C = m
    if pts is None:
        P, u = 0, torch.empty((N, H * W), dtype=torch.float32, device=t.device)
    else:
        pts = _points(pts, N)
        P = pts.shape[1]
        u = torch.empty((N, P), dtype=torch.float32, device=t.device)
    LIB.call("seg_point_uncertainty", _DT[t.dtype], _p(t), sn, sp, sc, N, H, W, C, _p(pts), P,
             _p(u), _stream())
    return u


def point_topk(keys, K):
    """int64 [N, K]: indices of the K largest of float32 keys [N, L] (ties: lower index), in
    ascending order."""
    if not keys.is_cuda or keys.dtype != torch.float32 or keys.dim() != 2:
        raise RuntimeError("point_topk: keys must be a float32 HIP tensor [N, L]")
    keys = keys.contiguous()
    N, L = keys.shape
    ws = torch.empty(LIB.query("seg_point_topk_ws", N, L), dtype=torch.int32, device=keys.device)
    idx = torch.empty((N, K), dtype=torch.int64, device=keys.device)
    LIB.call("seg_point_topk", _p(keys), N, L, K, _p(idx), _p(ws), _stream())
    return idx


def point_coords_train(over, idx, cover):
    """[N, P, 2]: over[n, idx[n]] (importance points), then cover[n] (idx None: cover alone)."""
    if idx is None:
        return cover.contiguous()
    N, L, _ = over.shape
    over, cover = _points(over, N), _points(cover, N)
    K = idx.shape[1]
    P = K + cover.shape[1]
    pts = torch.empty((N, P, 2), dtype=torch.float32, device=over.device)
    LIB.call("seg_point_coords", _p(over), _p(idx.contiguous()), N, L, K, _p(cover), P, 0, 0,
             _p(pts), _stream())
    return pts


def point_coords_grid(idx, hw):
    """[N, K, 2]: centres of the pixels idx [N, K] of an H x W grid (pointrend.py:170-172)."""
    N, K = idx.shape
    H, W = hw
    pts = torch.empty((N, K, 2), dtype=torch.float32, device=idx.device)
    LIB.call("seg_point_coords", None, _p(idx.contiguous()), N, 0, K, None, K, H, W, _p(pts),
             _stream())
    return pts


def point_scatter(rows, idx, m):
    """m[n, idx[n, p], c] = rows[n*P + p, c] (m: float32 map, written in place)."""
    t, sn, sp, sc, N, H, W, C = m
    assert t.dtype == torch.float32
    R, Cr, ldr = _rows(rows)
    P = idx.shape[1]
    assert R == N * P and Cr == C
    LIB.call("seg_point_scatter", _DT[rows.dtype], _p(rows), ldr, _p(idx.contiguous()), N, P, C,
             _p(t), sn, sp, sc, _stream())


def point_resize(m, out_hw, align_corners=False):
    """F.interpolate(map, out_hw, 'bilinear', align_corners) -> float32 NCHW [N, C, Ho, Wo]."""
    t, sn, sp, sc, N, H, W, C = m
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    y = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=t.device)
    LIB.call("seg_point_resize", _DT[t.dtype], _p(t), sn, sp, sc, N, H, W, C, _p(y), Ho, Wo,
             int(bool(align_corners)), _stream())
    return y


def point_ce_fwd(rows, target, ignore_index):
    """Mean cross-entropy of the rows [R, C] against int64 target [R] -> float32[2] = (loss,
    1 / valid rows)."""
    R, C, ld = _rows(rows)
    if not target.is_cuda or target.dtype != torch.int64 or target.numel() != R:
        raise RuntimeError("point_ce: target must be an int64 HIP tensor of %d elements" % R)
    ws = torch.empty(2 * LIB.query("seg_point_ce_blocks", R), dtype=torch.float64,
                     device=rows.device)
    out = torch.empty(2, dtype=torch.float32, device=rows.device)
    LIB.call("seg_point_ce_fwd", _DT[rows.dtype], _p(rows), ld, R, C, _p(target.contiguous()),
             int(ignore_index), _p(ws), _p(out), _stream())
    return out


def point_ce_bwd(rows, target, ignore_index, loss_out, grad_out):
    """-> d(loss)/d(rows) * grad_out, [R, C] in rows.dtype."""
    R, C, ld = _rows(rows)
    grad_out = grad_out.reshape(1).to(torch.float32).contiguous()
    dx = torch.empty((R, C), dtype=rows.dtype, device=rows.device)
    LIB.call("seg_point_ce_bwd", _DT[rows.dtype], _p(rows), ld, R, C, _p(target.contiguous()),
             int(ignore_index), _p(loss_out), _p(grad_out), _p(dx), C, _stream())
    return dx


# ---- LEDNet: 3-tap line convolutions and the split-shuffle tail (csrc/conv_line.hip) ------------
AXIS_H, AXIS_W = 0, 1


def conv_line_ok(dtype, C, axis, dil):
    return dtype in _DT and LIB.query("seg_conv_line_ok", _DT[dtype], C, axis, dil) == 1


def conv_line_bias_ok(dtype, C, axis, dil):
    """conv_line_ok for the classes of conv_line_bias: C = 40 as well."""
    return dtype in _DT and LIB.query("seg_conv_line_bias_ok", _DT[dtype], C, axis, dil) == 1


def conv_line_geom(dtype, N, H, W, C):
    """Launch geometry of conv_line / conv_line_bias on [N,H,W,C]: pixels per tile, grid (=
    statistic rows), tiles per block, pixels per weight-gradient trip, weight-gradient splits."""
    vals = [LIB.query("seg_conv_line_bias_geom", _DT[dtype], N, H, W, C, k) for k in range(4)]
    vals.append(LIB.query("seg_conv_line_wgrad_splits", _DT[dtype], N, H, W, C))
    if min(vals) < 1:
        raise ValueError("conv_line_geom: bad dtype / shape: %s %s" % (dtype, (N, H, W, C)))
    return dict(zip(("tile", "grid", "tiles_per_block", "wgrad_trip", "wgrad_splits"), vals))


def _conv_line(entry, ok, x, wp, bias, axis, dil, pro, out, add, want_stats):
    N, H, W, C, ldx = nhwc(x)
    if not ok(x.dtype, C, axis, dil):
        raise RuntimeError("conv_line: no kernel for %s C=%d axis=%d dil=%d" % (x.dtype, C, axis, dil))
    assert wp.dtype == x.dtype and wp.is_contiguous() and tuple(wp.shape) == (C, 3 * C)
    mode, ps, pt = _pro(pro)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    assert tuple(out.shape) == (N, H, W, C) and out.dtype == x.dtype
    ldy = nhwc(out)[4]
    ldadd = 0
    if add is not None:
        assert tuple(add.shape) == (N, H, W, C) and add.dtype == x.dtype
        ldadd = nhwc(add)[4]
    partial = None
    if want_stats:
        rows = LIB.query("seg_conv_line_bias_geom", _DT[x.dtype], N, H, W, C, 1)
        partial = torch.empty((rows, 2, C), dtype=torch.float32, device=x.device)
    head = (_DT[x.dtype], _p(x), ldx, N, H, W, C, _p(wp))
    tail = (axis, dil, mode, _p(ps), _p(pt), _p(out), ldy, _p(add), ldadd, _p(partial), _stream())
    if entry == "seg_conv_line_fwd":
        LIB.call(entry, *head, *tail)
    else:
        assert bias is None or (bias.dtype == torch.float32 and bias.numel() == C
                                and bias.is_contiguous())
        LIB.call(entry, *head, _p(bias), *tail)
    return out, partial


def conv_line(x, wp, axis, dil, pro=None, out=None, add=None, want_stats=False):
    """x NHWC [N,H,W,C] (a channel slice is fine), C in {16, 32, 64}; wp [C, 3*C] in x.dtype,
    taps along `axis` (AXIS_H: a (3,1) kernel, AXIS_W: (1,3)).  Returns (y, stat_partial|None);
    y = conv (+ add)."""
    return _conv_line("seg_conv_line_fwd", conv_line_ok, x, wp, None, axis, dil, pro, out, add,
                      want_stats)


def conv_line_bias(x, wp, bias, axis, dil, pro=None, out=None, add=None, want_stats=False):
    """conv_line for C in {16, 32, 40, 64} with a float32 bias [C] (None: no bias), added before
    `add`, the rounding and the statistics: y = conv + bias (+ add)."""
    return _conv_line("seg_conv_line_bias_fwd", conv_line_bias_ok, x, wp, bias, axis, dil, pro,
                      out, add, want_stats)


def conv_line_wgrad(x, dy, axis, dil, pro=None):
    """-> dW fp32 [C, C, 3] = [o][c][tap]: the memory layout of the [O,C,3,1] / [O,C,1,3]
    parameter."""
    N, H, W, C, ldx = nhwc(x)
    Nd, Hd, Wd, Cd, lddy = nhwc(dy)
    assert (Nd, Hd, Wd, Cd) == (N, H, W, C) and dy.dtype == x.dtype
    mode, ps, pt = _pro(pro)
    splits = LIB.query("seg_conv_line_wgrad_splits", _DT[x.dtype], N, H, W, C)
    if splits < 1:
        raise RuntimeError("conv_line_wgrad: no kernel for %s C=%d" % (x.dtype, C))
    partial = torch.empty((splits, 3 * C * C), dtype=torch.float32, device=x.device)
    LIB.call("seg_conv_line_wgrad", _DT[x.dtype], _p(x), ldx, _p(dy), lddy, N, H, W, C, axis, dil,
             mode, _p(ps), _p(pt), _p(partial), splits, _stream())
    if splits == 1:
        return partial.view(C, C, 3)
    return colsum(partial, f64=False).view(C, C, 3)


def ssnbt_tail_geom(dtype, P, C):
    vals = [LIB.query("seg_ssnbt_tail_geom", _DT[dtype], P, C, k) for k in range(3)]
    if min(vals) < 1:
        raise ValueError("ssnbt_tail_geom: bad dtype / P / C: %s %d %d" % (dtype, P, C))
    return dict(zip(("threads", "grid", "trips"), vals))


def ssnbt_tail_fwd(y0, s0, t0, y1, s1, t1, x, out=None):
    """out[..., 2i+g] = relu(relu(y_g[..., i]*s_g[i] + t_g[i]) + x[..., g*C/2 + i])."""
    N, H, W, C, ldx = nhwc(x)
    h = C // 2
    assert tuple(y0.shape) == (N, H, W, h) and tuple(y1.shape) == (N, H, W, h)
    assert y0.dtype == x.dtype and y1.dtype == x.dtype
    for v in (s0, t0, s1, t1):
        assert v.dtype == torch.float32 and v.numel() == h and v.is_contiguous()
    if out is None:
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    LIB.call("seg_ssnbt_tail_fwd", _DT[x.dtype], _p(y0), nhwc(y0)[4], _p(s0), _p(t0), _p(y1),
             nhwc(y1)[4], _p(s1), _p(t1), _p(x), ldx, _p(out), nhwc(out)[4], N * H * W, C,
             _stream())
    return out


def ssnbt_tail_bwd(gout, out, gm=None):
    """gm[..., g*C/2 + i] = gout[..., 2i+g] * (out[..., 2i+g] > 0)."""
    N, H, W, C, ldo = nhwc(out)
    assert tuple(gout.shape) == (N, H, W, C) and gout.dtype == out.dtype
    if gm is None:
        gm = torch.empty((N, H, W, C), dtype=out.dtype, device=out.device)
    LIB.call("seg_ssnbt_tail_bwd", _DT[out.dtype], _p(gout), nhwc(gout)[4], _p(out), ldo, _p(gm),
             nhwc(gm)[4], N * H * W, C, _stream())
    return gm


# ---- EDANet: channel placement for the down-sampler's concat (csrc/edanet.hip) ------------------
def chan_copy(src, dst, C=None):
    """dst[..., c] = src[..., c] for c < C (default: src's width), 0 for C <= c < dst's width.
    src, dst: NHWC views over the same pixels, any channel offset (element-wise)."""
    N, H, W, Cs, lds = nhwc(src)
    Nd, Hd, Wd, Cz, ldd = nhwc(dst)
    C = Cs if C is None else C
    assert (Nd, Hd, Wd) == (N, H, W) and dst.dtype == src.dtype and 1 <= C <= min(Cs, Cz)
    LIB.call("seg_chan_copy", _DT[src.dtype], _p(src), lds, _p(dst), ldd, N * H * W, C, Cz,
             _stream())
    return dst


# ---- EDANet: a pair of line convolutions in one launch (csrc/conv_line_pair.hip) ----------------
def conv_line_pair_ok(dtype, C, L, dil):
    """Does the pair kernel serve lines of L pixels (along the SECOND axis) of C channels?"""
    return dtype in _DT and LIB.query("seg_conv_line_pair_ok", _DT[dtype], C, L, dil) == 1


def conv_line_pair(x, wa, bias_a, wb, bias_b, order, dil, pro=None, out=None, add=None,
                   want_mid=True, want_stats=False, want_mid_sums=False):
    """mid = lineA(act(x)) + bias_a, y = lineB(mid) + bias_b (+ add) in one launch; order 0: A = H,
    B = W; 1: A = W, B = H.  wa / wb [C, 3*C] in x.dtype, biases float32 [C] or None.
    Returns (y, mid|None, stat_partial|None, mid_sums|None)."""
    N, H, W, C, ldx = nhwc(x)
    L = W if order == 0 else H
    if not conv_line_pair_ok(x.dtype, C, L, dil):
        raise RuntimeError("conv_line_pair: no kernel for %s C=%d line=%d dil=%d"
                           % (x.dtype, C, L, dil))
    for w in (wa, wb):
        assert w.dtype == x.dtype and w.is_contiguous() and tuple(w.shape) == (C, 3 * C)
    for b in (bias_a, bias_b):
        assert b is None or (b.dtype == torch.float32 and b.numel() == C and b.is_contiguous())
    mode, ps, pt = _pro(pro)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    assert tuple(out.shape) == (N, H, W, C) and out.dtype == x.dtype
    ldadd = 0
    if add is not None:
        assert tuple(add.shape) == (N, H, W, C) and add.dtype == x.dtype
        ldadd = nhwc(add)[4]
    mid = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device) if want_mid else None
    rows = LIB.query("seg_conv_line_pair_rows", N, H, W, order)
    stat = torch.empty((rows, 2, C), dtype=torch.float32, device=x.device) if want_stats else None
    msum = torch.empty((rows, C), dtype=torch.float32, device=x.device) if want_mid_sums else None
    LIB.call("seg_conv_line_pair_fwd", _DT[x.dtype], _p(x), ldx, N, H, W, C, _p(wa), _p(bias_a),
             _p(wb), _p(bias_b), order, dil, mode, _p(ps), _p(pt), _p(mid), C, _p(out),
             nhwc(out)[4], _p(add), ldadd, _p(stat), _p(msum), _stream())
    return out, mid, stat, msum


# ---- FPENet's FPE pyramid stages and MEU fusion (csrc/fpenet.hip) ---------------------------------
FPE_MAX_N, FPE_MAX_DIL, MEU_MAX_C = 64, 8, 128


def fpe_stage_check(n, dil):
    """The contract of seg_fpe_stage_fwd / _bwd, on the host and before any tensor is read."""
    if not (isinstance(n, int) and n >= 4 and n % 4 == 0 and n <= FPE_MAX_N):
        raise ValueError("fpe_stage: n=%r is not a positive multiple of 4 up to %d"
                         % (n, FPE_MAX_N))
    if not (isinstance(dil, int) and 1 <= dil <= FPE_MAX_DIL):
        raise ValueError("fpe_stage: dilation %r is not in 1..%d" % (dil, FPE_MAX_DIL))


def meu_check(C, low_hw, high_hw):
    """The contract of seg_meu_fwd / _bwd_low / _bwd_high."""
    if not (C >= 8 and C % 8 == 0 and C <= MEU_MAX_C):
        raise ValueError("meu: C=%r is not a positive multiple of 8 up to %d" % (C, MEU_MAX_C))
    (h, w), (h2, w2) = low_hw, high_hw
    if not (1 <= h2 <= h and 1 <= w2 <= w):
        raise ValueError("meu: the high-level map %dx%d is not within the low-level map %dx%d"
                         % (h2, w2, h, w))


def _fpe_slice(t, like, what):
    if t.dtype != like.dtype or tuple(t.shape) != tuple(like.shape):
        raise ValueError("%s: expected %s %s, got %s %s"
                         % (what, tuple(like.shape), like.dtype, tuple(t.shape), t.dtype))
    ld = nhwc(t)[4]
    if ld % 4 != 0 or t.storage_offset() % 4 != 0:
        raise ValueError("%s: pitch %d / offset %d are not multiples of 4"
                         % (what, ld, t.storage_offset()))
    return ld


def _fpe_vecs(n, what, *vs):
    for v in vs:
        if not (v.is_cuda and v.dtype == torch.float32 and v.numel() == n and v.is_contiguous()):
            raise ValueError("%s: per-channel parameters are contiguous float32 [%d] device tensors"
                             % (what, n))


def fpe_stage_rows(dtype, N, H, W, n):
    rows = LIB.query("seg_fpe_stage_rows", _DT[dtype], N, H, W, n)
    if rows < 1:
        raise ValueError("seg_fpe_stage_rows(%s, %d, %d, %d, %d): out of contract"
                         % (dtype, N, H, W, n))
    return rows


def fpe_stage_fwd(a, sa, ta, w, dil, b=None, sb=None, tb=None, b_act=None, out=None,
                  want_stats=True):
    """-> (y, partial fp32 [rows, 2, n] | None): y = depthwise 3x3 (w [n,1,3,3], pad = dilation =
    dil) of relu(sa*a + ta) + relu(sb*b + tb) on n-channel NHWC slices (n, pitches and offsets
    multiples of 4); b None: stage 0.  b_act: an NHWC slice that receives relu(sb*b + tb)."""
    n = int(a.shape[-1])
    fpe_stage_check(n, dil)
    if (b is None) != (sb is None) or (b is None) != (tb is None) or (b is None and b_act is not None):
        raise ValueError("fpe_stage_fwd: b, sb and tb go together, and b_act needs b")
    N, H, W, _, lda = nhwc(a)
    _fpe_slice(a, a, "fpe_stage_fwd a")
    _fpe_vecs(n, "fpe_stage_fwd", sa, ta, *([] if b is None else [sb, tb]))
    if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
            and tuple(w.shape) == (n, 1, 3, 3)):
        raise ValueError("fpe_stage_fwd: w is a contiguous float32 [%d,1,3,3] device tensor" % n)
    if out is None:
        out = torch.empty((N, H, W, n), dtype=a.dtype, device=a.device)
    ldy = _fpe_slice(out, a, "fpe_stage_fwd out")
    ldb = _fpe_slice(b, a, "fpe_stage_fwd b") if b is not None else 0
    ldo = _fpe_slice(b_act, a, "fpe_stage_fwd b_act") if b_act is not None else 0
    rows = fpe_stage_rows(a.dtype, N, H, W, n)
    partial = torch.empty((rows, 2, n), dtype=torch.float32, device=a.device) if want_stats \
        else None
    LIB.call("seg_fpe_stage_fwd", _DT[a.dtype], _p(a), lda, _p(sa), _p(ta), _p(b), ldb, _p(sb),
             _p(tb), _p(w), dil, _p(out), ldy, _p(b_act), ldo, N, H, W, n, _p(partial), rows,
             _stream())
    return out, partial


def fpe_act_fwd(b, sb, tb, out=None):
    """relu(sb*b + tb) on an n-channel NHWC slice (n a multiple of 4) -> out."""
    n = int(b.shape[-1])
    if n < 4 or n % 4 != 0:
        raise ValueError("fpe_act_fwd: n=%d is not a positive multiple of 4" % n)
    N, H, W, _, ldb = nhwc(b)
    _fpe_slice(b, b, "fpe_act_fwd b")
    _fpe_vecs(n, "fpe_act_fwd", sb, tb)
    if out is None:
        out = torch.empty((N, H, W, n), dtype=b.dtype, device=b.device)
    ldy = _fpe_slice(out, b, "fpe_act_fwd out")
    LIB.call("seg_fpe_act_fwd", _DT[b.dtype], _p(b), ldb, _p(sb), _p(tb), _p(out), ldy, N * H * W,
             n, _stream())
    return out


def fpe_bn_bwd_apply(g, x, scale, c0=None, c1=None, out=None):
    """dx = scale*g - c0 - c1*x on an n-channel NHWC slice (c0 / c1 None: scale*g); out may be g."""
    n = int(g.shape[-1])
    if n < 4 or n % 4 != 0:
        raise ValueError("fpe_bn_bwd_apply: n=%d is not a positive multiple of 4" % n)
    N, H, W, _, ldg = nhwc(g)
    _fpe_slice(g, g, "fpe_bn_bwd_apply g")
    ldx = _fpe_slice(x, g, "fpe_bn_bwd_apply x")
    if out is None:
        out = torch.empty((N, H, W, n), dtype=g.dtype, device=g.device)
    lddx = _fpe_slice(out, g, "fpe_bn_bwd_apply out")
    LIB.call("seg_fpe_bn_bwd_apply", _DT[g.dtype], _p(g), ldg, _p(x), ldx, _p(scale), _p(c0),
             _p(c1), _p(out), lddx, N * H * W, n, _stream())
    return out


def fpe_stage_bwd(dy, a, sa, ta, w, dil, b=None, sb=None, tb=None, res=None, ga=None, gb=None,
                  pa=None, pa_col=0):
    """One pass over (dy, a, b, res) -> (ga, gb, pw [rows, 9, n], pa, pb [rows, 2, n]).
    ga = mask(a) * dgrad, gb = mask(b) * (dgrad + res); pa: [rows, 2, P] fp32 whose columns
    pa_col .. pa_col + n receive (sum ga | sum ga*a_raw) (a fresh [rows, 2, n] if None).
    dy None (with a, sa, ta, w None): gb = mask(b) * res and pb only — the last stage's slice."""
    ref = b if dy is None else dy
    n = int(ref.shape[-1])
    fpe_stage_check(n, dil)
    if (b is None) != (res is None) or (b is None) != (sb is None) or (b is None) != (tb is None) \
            or (b is None and dy is None):
        raise ValueError("fpe_stage_bwd: b, sb, tb and res go together (and dy or b is given)")
    N, H, W, _, _ = nhwc(ref)
    rows = fpe_stage_rows(ref.dtype, N, H, W, n)
    dev = ref.device
    lddy = lda = ldga = ldb = ldres = ldgb = 0
    pw = pb = None
    pitch = 0
    if dy is not None:
        lddy = _fpe_slice(dy, ref, "fpe_stage_bwd dy")
        lda = _fpe_slice(a, ref, "fpe_stage_bwd a")
        _fpe_vecs(n, "fpe_stage_bwd", sa, ta)
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
                and tuple(w.shape) == (n, 1, 3, 3)):
            raise ValueError("fpe_stage_bwd: w is a contiguous float32 [%d,1,3,3] device tensor" % n)
        if ga is None:
            ga = torch.empty((N, H, W, n), dtype=ref.dtype, device=dev)
        ldga = _fpe_slice(ga, ref, "fpe_stage_bwd ga")
        pw = torch.empty((rows, 9, n), dtype=torch.float32, device=dev)
        if pa is None:
            pa = torch.empty((rows, 2, n), dtype=torch.float32, device=dev)
        pitch = pa.shape[2]
        if not (pa.dtype == torch.float32 and pa.is_contiguous() and pa.dim() == 3
                and tuple(pa.shape[:2]) == (rows, 2) and pa_col % 4 == 0
                and 0 <= pa_col and pa_col + n <= pitch):
            raise ValueError("fpe_stage_bwd: partial_a is a contiguous float32 [%d, 2, P] array "
                             "with %d + %d <= P" % (rows, pa_col, n))
    else:
        a = sa = ta = w = ga = pa = None
    if b is not None:
        ldb = _fpe_slice(b, ref, "fpe_stage_bwd b")
        ldres = _fpe_slice(res, ref, "fpe_stage_bwd res")
        _fpe_vecs(n, "fpe_stage_bwd", sb, tb)
        if gb is None:
            gb = torch.empty((N, H, W, n), dtype=ref.dtype, device=dev)
        ldgb = _fpe_slice(gb, ref, "fpe_stage_bwd gb")
        pb = torch.empty((rows, 2, n), dtype=torch.float32, device=dev)
    else:
        gb = None
    LIB.call("seg_fpe_stage_bwd", _DT[ref.dtype], _p(dy), lddy, _p(a), lda, _p(sa), _p(ta), _p(b),
             ldb, _p(sb), _p(tb), _p(res), ldres, _p(w), dil, _p(ga), ldga, _p(gb), ldgb, N, H, W, n,
             _p(pw), _p(pa), pitch, pa_col, _p(pb), rows, _stream())
    return ga, gb, pw, pa, pb


def _meu_rows(N, h, w, C, high):
    rows = LIB.query("seg_meu_rows", N, h, w, C, 1 if high else 0)
    if rows < 1:
        raise ValueError("seg_meu_rows(%d, %d, %d, %d): out of contract" % (N, h, w, C))
    return rows


def _meu_operands(L, Hr, what):
    C = int(L.shape[-1])
    meu_check(C, (int(L.shape[1]), int(L.shape[2])), (int(Hr.shape[1]), int(Hr.shape[2])))
    N, h, w, _, ldl = nhwc(L)
    N2, h2, w2, C2, ldh = nhwc(Hr)
    if N2 != N or C2 != C or Hr.dtype != L.dtype:
        raise ValueError("%s: the maps disagree: %s %s / %s %s"
                         % (what, tuple(L.shape), L.dtype, tuple(Hr.shape), Hr.dtype))
    _fpe_slice(L, L, what + " L")
    _fpe_slice(Hr, Hr, what + " H")
    return N, h, w, h2, w2, C, ldl, ldh


def _meu_aff(aff):
    return (None, None) if aff is None else aff


def meu_fwd(L, aff_l, Hr, aff_h, a, w_sa, out=None):
    """-> (out [N,h,w,C], sa fp32 [N,h,w]): out = a[n][c]*(sl*L + tl) + sa*(sh*bilinear(Hr) + th),
    sa = sigmoid(w_sa * mean_c(sl*L + tl)); aff_* = (scale, shift) | None; a fp32 [N, C]; w_sa a
    float32 device tensor of one element."""
    N, h, w, h2, w2, C, ldl, ldh = _meu_operands(L, Hr, "meu_fwd")
    _nc(a, N, C, "meu_fwd a")
    if not (w_sa.is_cuda and w_sa.dtype == torch.float32 and w_sa.numel() == 1):
        raise ValueError("meu_fwd: w_sa is a float32 device tensor of one element")
    (sl, tl), (sh, th) = _meu_aff(aff_l), _meu_aff(aff_h)
    if out is None:
        out = torch.empty((N, h, w, C), dtype=L.dtype, device=L.device)
    ldo = _fpe_slice(out, L, "meu_fwd out")
    sa = torch.empty((N, h, w), dtype=torch.float32, device=L.device)
    LIB.call("seg_meu_fwd", _DT[L.dtype], _p(L), ldl, _p(sl), _p(tl), _p(Hr), ldh, _p(sh), _p(th),
             _p(a), _p(w_sa), _p(out), ldo, _p(sa), N, h, w, h2, w2, C, _stream())
    return out, sa


def meu_bwd_low(g, L, aff_l, Hr, aff_h, a, w_sa, sa, out=None):
    """-> (dL at bn_low's output, da fp32 [N, C], d w_sa fp32 [1], p_bn [rows, 2, C] =
    (sum dL | sum dL*L))."""
    N, h, w, h2, w2, C, ldl, ldh = _meu_operands(L, Hr, "meu_bwd_low")
    _nc(a, N, C, "meu_bwd_low a")
    ldg = _fpe_slice(g, L, "meu_bwd_low g")
    (sl, tl), (sh, th) = _meu_aff(aff_l), _meu_aff(aff_h)
    if out is None:
        out = torch.empty((N, h, w, C), dtype=L.dtype, device=L.device)
    ldo = _fpe_slice(out, L, "meu_bwd_low out")
    rows = _meu_rows(N, h, w, C, False)
    p_a = torch.empty((rows, 2, C), dtype=torch.float32, device=L.device)
    p_bn = torch.empty((rows, 2, C), dtype=torch.float32, device=L.device)
    LIB.call("seg_meu_bwd_low", _DT[L.dtype], _p(g), ldg, _p(L), ldl, _p(sl), _p(tl), _p(Hr), ldh,
             _p(sh), _p(th), _p(a), _p(w_sa), _p(sa), _p(out), ldo, N, h, w, h2, w2, C, _p(p_a),
             _p(p_bn), rows, _stream())
    chunks = rows // N
    s = p_a.view(chunks, N * 2 * C)
    s = (s[0] if chunks == 1 else colsum(s, f64=False)).view(N, 2, C)
    return out, s[:, 0, :].contiguous(), s[:, 1, 0].sum().view(1), p_bn


def meu_bwd_high(g, sa, Hr, dpool=None, out=None):
    """-> (dH at bn_high's output [N,h2,w2,C], p_bn [rows, 2, C] = (sum dH | sum dH*Hr)):
    dH[q] = sum_p wgt(p, q) * sa[p] * g[p] + dpool[n] / (h2*w2)."""
    N, h, w, h2, w2, C, ldg, ldh = _meu_operands(g, Hr, "meu_bwd_high")
    _nc(dpool, N, C, "meu_bwd_high dpool")
    if out is None:
        out = torch.empty((N, h2, w2, C), dtype=g.dtype, device=g.device)
    ldo = _fpe_slice(out, Hr, "meu_bwd_high out")
    rows = _meu_rows(N, h2, w2, C, True)
    p_bn = torch.empty((rows, 2, C), dtype=torch.float32, device=g.device)
    LIB.call("seg_meu_bwd_high", _DT[g.dtype], _p(g), ldg, _p(sa), _p(Hr), ldh, _p(dpool), _p(out),
             ldo, N, h, w, h2, w2, C, _p(p_bn), rows, _stream())
    return out, p_bn


# ---- UNet: encoder skips written in place, padded upsampling (csrc/unet.hip) ----------------------
def _same_shape(t, shape, like, what):
    if tuple(t.shape) != tuple(shape) or t.dtype != like.dtype:
        raise ValueError("%s: expected %s of %s, got %s of %s"
                         % (what, tuple(shape), like.dtype, tuple(t.shape), t.dtype))
    return nhwc(t)[4]


def skip_pool_rows(dtype, N, H, W, C):
    """Partial rows of skip_pool_bwd for an [N,H,W,C] level (host only)."""
    rows = LIB.query("seg_skip_pool_bwd_rows", _DT[dtype], N, H, W, C)
    if rows < 1:
        raise ValueError("skip_pool_rows: bad dtype / shape: %s %s" % (dtype, (N, H, W, C)))
    return rows


def skip_pool_fwd(y, pro=None, out=None):
    """One pass over the raw y: -> (skip = act(y), written into `out` — a channel slice of a concat
    buffer — where given, pooled [N, H//2, W//2, C] = the 2x2 max of the stored skip)."""
    N, H, W, C, ldy = nhwc(y)
    mode, s, t = _pro(pro)
    if out is None:
        out = torch.empty((N, H, W, C), dtype=y.dtype, device=y.device)
    lds = _same_shape(out, (N, H, W, C), y, "skip_pool_fwd out")
    pooled = torch.empty((N, H // 2, W // 2, C), dtype=y.dtype, device=y.device)
    LIB.call("seg_skip_pool_fwd", _DT[y.dtype], _p(y), ldy, N, H, W, C, int(mode), _p(s), _p(t),
             _p(out), lds, _p(pooled), C, _stream())
    return out, pooled


def skip_pool_bwd(g_skip, g_pool, y, pro=None, out=None):
    """-> (g' = relu_mask * (g_skip + scatter(g_pool)) dense [N,H,W,C], partial fp32 [R, 2, C] =
    (sum g' | sum g'*y)).  Either gradient may be None; the activation and the windows' winners are
    recomputed from the raw y."""
    N, H, W, C, ldy = nhwc(y)
    mode, s, t = _pro(pro)
    ldgs = 0 if g_skip is None else _same_shape(g_skip, (N, H, W, C), y, "skip_pool_bwd g_skip")
    ldgp = 0 if g_pool is None else _same_shape(g_pool, (N, H // 2, W // 2, C), y,
                                                "skip_pool_bwd g_pool")
    if out is None:
        out = torch.empty((N, H, W, C), dtype=y.dtype, device=y.device)
    ldgx = _same_shape(out, (N, H, W, C), y, "skip_pool_bwd out")
    rows = LIB.query("seg_skip_pool_bwd_rows", _DT[y.dtype], N, H, W, C)
    partial = torch.empty((max(rows, 1), 2, C), dtype=torch.float32, device=y.device)
    LIB.call("seg_skip_pool_bwd", _DT[y.dtype], _p(g_skip), ldgs, _p(g_pool), ldgp, _p(y), ldy, N, H,
             W, C, int(mode), _p(s), _p(t), _p(out), ldgx, _p(partial), rows, _stream())
    return out, partial


def bilinear_pad(x, out_hw, out, place=(0, 0), pro=None, align_corners=True):
    """F.pad(F.interpolate(act(x), out_hw, 'bilinear')) to out's size: the resized map lands at
    place = (top, left) of `out` [N, Hd, Wd, C] (a channel slice), the rest of `out` is zero."""
    N, Hi, Wi, C, ldx = nhwc(x)
    Ho, Wo = out_hw
    mode, s, t = _pro(pro)
    Hd, Wd = out.shape[1:3]
    ldy = _same_shape(out, (N, Hd, Wd, C), x, "bilinear_pad out")
    LIB.call("seg_bilinear_pad_fwd", _DT[x.dtype], _p(x), ldx, N, Hi, Wi, C, int(mode), _p(s), _p(t),
             _p(out), ldy, Ho, Wo, Hd, Wd, int(place[0]), int(place[1]), int(align_corners),
             _stream())
    return out


def bilinear_pad_bwd(gy, in_hw, out_hw, place=(0, 0), align_corners=True):
    """gy [N, Hd, Wd, C] -> gx [N, Hi, Wi, C], read from the out_hw window at `place` alone."""
    N, Hd, Wd, C, ldgy = nhwc(gy)
    Hi, Wi = in_hw
    gx = torch.empty((N, Hi, Wi, C), dtype=gy.dtype, device=gy.device)
    LIB.call("seg_bilinear_pad_bwd", _DT[gy.dtype], _p(gx), C, N, Hi, Wi, C, _p(gy), ldgy,
             out_hw[0], out_hw[1], Hd, Wd, int(place[0]), int(place[1]), int(align_corners),
             _stream())
    return gx


# ---- ContextNet: bilinear resize + depthwise 3x3 without the upsampled map (csrc/contextnet.hip) ----
def up_dw_rows(dtype, N, H, W, C, kind=0):
    """Partial rows of up_dw's statistics (kind 0) / up_dw_bwd's weight gradient (kind 1) for an
    [N,H,W,C] output (host only)."""
    if dtype not in _DT:
        raise ValueError("up_dw_rows: dtype %s (float32 or bfloat16)" % (dtype,))
    rows = LIB.query("seg_up_dw_rows", _DT[dtype], int(N), int(H), int(W), int(C), int(kind))
    if rows < 1:
        raise ValueError("up_dw_rows: bad shape / kind: %s %s kind %s (C a positive multiple of %d)"
                         % (dtype, (N, H, W, C), kind, vec_of(dtype)))
    return rows


def _up_dw_operand(t, shape, dtype, what):
    """-> the row pitch of an NHWC operand of up_dw / up_dw_bwd; raises instead of over-reading."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise ValueError("%s: expected an NHWC 4-d tensor" % what)
    if t.dtype not in _DT or (dtype is not None and t.dtype != dtype):
        raise ValueError("%s: dtype %s (float32 or bfloat16, one for every operand)" % (what, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected %s, got %s" % (what, tuple(shape), tuple(t.shape)))
    vec = vec_of(t.dtype)
    if min(t.shape) < 1 or t.shape[-1] % vec != 0:
        raise ValueError("%s: %s: C is a positive multiple of %d, no dimension empty"
                         % (what, tuple(t.shape), vec))
    if t.stride(3) != 1:
        raise ValueError("%s: the channel dimension is not contiguous (strides %s)"
                         % (what, t.stride()))
    ld = nhwc(t)[4]
    if ld % vec != 0 or t.storage_offset() % vec != 0:
        raise ValueError("%s: row pitch %d / offset %d are no multiples of the %d-element vector"
                         % (what, ld, t.storage_offset(), vec))
    return ld


def _up_dw_taps(w9c, C, like, what):
    if not isinstance(w9c, torch.Tensor) or w9c.dtype != torch.float32 \
            or tuple(w9c.shape) != (9, C) or not w9c.is_contiguous():
        raise ValueError("%s: the taps are a contiguous float32 [9, %d] (tap-major)" % (what, C))
    if w9c.device != like.device:
        raise ValueError("%s: the taps live on %s, the activation on %s"
                         % (what, w9c.device, like.device))


def _up_dw_pro(pro, C, like, what):
    mode, s, t = _pro(pro)
    mode = int(mode)
    if mode & PRO_AFFINE:
        for p in (s, t):
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or p.numel() != C \
                    or not p.is_contiguous() or p.device != like.device:
                raise ValueError("%s: the prologue's scale / shift are contiguous float32 [%d] on "
                                 "the activation's device" % (what, C))
    else:
        s = t = None
    return mode, s, t


def up_dw(lo, out_hw, w9c, pro=None, align_corners=True, out=None, want_stats=False):
    """y = depthwise 3x3 (zero padding 1) of bilinear(act(lo), out_hw), the upsampled map never
    stored -> (y [N,H,W,C], partial [rows,2,C] fp32 (sum | sum of squares) or None)."""
    N, h, w, C = lo.shape if isinstance(lo, torch.Tensor) and lo.dim() == 4 else (0, 0, 0, 0)
    ldlo = _up_dw_operand(lo, None, None, "up_dw lo")
    H, W = int(out_hw[0]), int(out_hw[1])
    if H < 1 or W < 1:
        raise ValueError("up_dw: output size %s" % ((H, W),))
    _up_dw_taps(w9c, C, lo, "up_dw")
    mode, s, t = _up_dw_pro(pro, C, lo, "up_dw")
    if out is None:
        out = torch.empty((N, H, W, C), dtype=lo.dtype, device=lo.device)
    ldy = _up_dw_operand(out, (N, H, W, C), lo.dtype, "up_dw out")
    rows = up_dw_rows(lo.dtype, N, H, W, C, 0)
    partial = torch.empty((rows, 2, C), dtype=torch.float32, device=lo.device) if want_stats \
        else None
    LIB.call("seg_up_dw_fwd", _DT[lo.dtype], _p(lo), ldlo, N, h, w, C, mode, _p(s), _p(t),
             _p(w9c), _p(out), ldy, H, W, int(bool(align_corners)), _p(partial), rows, _stream())
    return out, partial


def up_dw_bwd(dy, lo, w9c, pro=None, align_corners=True, out=None):
    """One pass over dy [N,H,W,C] and lo -> (d_up [N,H,W,C] in the activation dtype = dy correlated
    with the flipped taps, pw [rows,9,C] fp32 = weight-gradient rows with the upsampled map
    recomputed from lo; dw_wgrad_finalize reduces them)."""
    if not isinstance(dy, torch.Tensor) or dy.dim() != 4:
        raise ValueError("up_dw_bwd dy: expected an NHWC 4-d tensor")
    N, h, w, C = lo.shape if isinstance(lo, torch.Tensor) and lo.dim() == 4 else (0, 0, 0, 0)
    ldlo = _up_dw_operand(lo, None, None, "up_dw_bwd lo")
    H, W = int(dy.shape[1]), int(dy.shape[2])
    lddy = _up_dw_operand(dy, (N, H, W, C), lo.dtype, "up_dw_bwd dy")
    _up_dw_taps(w9c, C, lo, "up_dw_bwd")
    mode, s, t = _up_dw_pro(pro, C, lo, "up_dw_bwd")
    if out is None:
        out = torch.empty((N, H, W, C), dtype=lo.dtype, device=lo.device)
    ldd = _up_dw_operand(out, (N, H, W, C), lo.dtype, "up_dw_bwd out")
    rows = up_dw_rows(lo.dtype, N, H, W, C, 1)
    pw = torch.empty((rows, 9, C), dtype=torch.float32, device=lo.device)
    LIB.call("seg_up_dw_bwd", _DT[lo.dtype], _p(dy), lddy, _p(lo), ldlo, N, h, w, C, mode, _p(s),
             _p(t), _p(w9c), _p(out), ldd, H, W, int(bool(align_corners)), _p(pw), rows, _stream())
    return out, pw
