"""functional.dw_backward — the one place that composes a depthwise 3x3 backward — at every class
of launches it can choose, (stride, dilation, C, activation dtype):

  (1,1,16,bf16) (1,1,12,fp32)  register-sliding (12: a multiple of 4, not of 8)
  (1,2,16,bf16)                LDS-tiled
  (1,3,16,bf16)                row-chain: the first class whose kernels read the tap-major [9,C]
                               packing and whose weight gradient has to be transposed back
  (1,65,8,fp32)                strip, one pass
  (2,1,8,fp32) (2,1,16,bf16)   stride 2, one pass
  (2,2,8,fp32)                 the two-launch half: strided data gradient, strip weight gradient
  (2,1,8,fp32), bf16 weight    the two-launch half again: stride 2 is one pass for fp32 taps only

on 2 x 9 x 20 maps (20: not a multiple of the sliding kernels' 16-column block, more than one
strip; dilation 65 on 1 x 70 x 72, where every tap contributes), with the prologue none / ReLU /
affine + ReLU (the last with the BatchNorm-backward rows), the weight-gradient rows raw or
reduced, `out=` a channel slice of a wider NaN-filled buffer, and at (1,1,*) a second gradient
`res` added in the store, plainly and as the 2-ary sum.

Each case asserts (1) bit equality with the composition written out here from the hip_ops
wrappers, operands in the layout each kernel family reads — so a caller of the entry cannot
receive a weight gradient that is still tap-major — and (2) g and dW against torch float64 (conv2d
under autograd, mask applied) at the bars tests/test_dwconv_families_gpu.py sets for the same
quantities."""
import functools

import pytest
import torch

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc
from test_dwconv_families_gpu import BF16, F32, FUSED_DW_FAC, NAN, WGRAD_FAC, _ref_autograd
from test_dwconv_slide_gpu import _act_ref, _pro

pytestmark = pytest.mark.gpu

# stride, dilation, C, activation dtype, weight dtype, takes the one-pass half
CLASSES = [(1, 1, 16, BF16, F32, True), (1, 1, 12, F32, F32, True), (1, 2, 16, BF16, F32, True),
           (1, 3, 16, BF16, F32, True), (1, 65, 8, F32, F32, True), (2, 1, 8, F32, F32, True),
           (2, 1, 16, BF16, F32, True), (2, 2, 8, F32, F32, False), (2, 1, 8, F32, BF16, False)]
MODES = [0, 1, 3]  # prologue: none, ReLU, affine + ReLU


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def Fn():
    from segmentron_amd import functional
    return functional


def _shape(dil):
    return (1, 70, 72) if dil == 65 else (2, 9, 20)


@functools.lru_cache(maxsize=None)
def _case(stride, dil, C, dtype, wdtype, mode):
    """Inputs and the float64 reference of one (class, prologue), computed once."""
    N, H, W = _shape(dil)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    x = quant(rnd((N, C, H, W), 1), dtype)
    w = quant(rnd((C, 1, 3, 3), 2, 0.4), wdtype)
    pro, s, t = _pro(mode, C, 3)
    dy = quant(rnd((N, C, Ho, Wo), 4), dtype)
    res = quant(rnd((N, C, H, W), 5), dtype)
    act = _act_ref(x, mode, s, t).double()
    _, dx, dwref = _ref_autograd(act, w.double(), dy.double(), stride, dil)
    mask = (act > 0).double() if mode & 1 else torch.ones_like(act)
    return dict(x=to_dev_nhwc(x, dtype), dy=to_dev_nhwc(dy, dtype), res=to_dev_nhwc(res, dtype),
                w=torch.nn.Parameter(w.to(wdtype).to(DEV)), pro=pro, dx=dx, gref=dx * mask,
                dwref=dwref, resref=res.double())


def _nan_slice(like, vec):
    C = like.shape[-1]
    full = torch.full((*like.shape[:-1], C + 2 * vec), NAN, dtype=like.dtype, device=DEV)
    return full, full[..., vec:vec + C]


def _same(a, b):
    return (a is None and b is None) or (a.shape == b.shape and torch.equal(a, b))


def _id(c):
    return "s%d_d%d_c%d_%s_w%s" % (c[0], c[1], c[2], *(str(d).split(".")[1] for d in c[3:5]))


@pytest.mark.parametrize("cls", [c for c in CLASSES if c[5]], ids=_id)
def test_one_pass_half(cls):
    stride, dil, C, dtype, wdtype, _ = cls
    k, F = K(), Fn()
    vec = 8 if dtype == BF16 else 4
    tiled = stride == 1 and dil <= 2  # these kernels take torch's [C,1,3,3] and return dW in it
    assert F._dw_bwd_is_fused(stride, dil, C, wdtype)
    assert F.dw_backward_raw_ok(stride, dil, C, wdtype) == (tiled or stride == 2)
    res_modes = [None]
    if stride == 1 and dil == 1:
        assert k.dwconv_bwd_fused_add_ok(dil) and k.dwconv_bwd_fused_sum_ok(dtype, C, dil)
        res_modes += [False, True]  # res_sum off / on
    n = 0
    for mode in MODES:
        c = _case(stride, dil, C, dtype, wdtype, mode)
        x, dy, w, pro = c["x"], c["dy"], c["w"], c["pro"]
        want_bn = mode == 3
        for raw in ([False, True] if tiled or stride == 2 else [False]):
            for sl in (False, True):
                for res_sum in res_modes:
                    res = None if res_sum is None else c["res"]
                    full, out = _nan_slice(x, vec) if sl else (None, None)
                    full_e, out_e = _nan_slice(x, vec) if sl else (None, None)
                    g, dW, pb, fused = F.dw_backward(x, dy, w, stride, dil, pro, want_bn=want_bn,
                                                     raw_dw=raw, res=res, res_sum=bool(res_sum),
                                                     out=out)
                    assert fused
                    # ---- (1) the K-level composition
                    if stride == 2:
                        ge, dWe, pbe = k.dwconv_bwd_fused_s2(x, dy, w.detach().contiguous(), pro,
                                                             want_bn=want_bn, raw_dw=raw, out=out_e)
                    else:
                        taps = w.detach() if tiled else w.detach().view(C, 9).t().contiguous()
                        ge, dWe, pbe = k.dwconv_bwd_fused(x, dy, taps, dil, pro, want_bn=want_bn,
                                                          torch_layout=tiled, raw_dw=raw, res=res,
                                                          res_sum=bool(res_sum), out=out_e)
                        if not tiled:
                            dWe = dWe.t().reshape(C, 1, 3, 3).contiguous()
                    assert _same(g, ge) and _same(dW, dWe) and _same(pb, pbe)
                    assert (pb is not None) == want_bn
                    if sl:
                        assert g.data_ptr() == out.data_ptr()
                        assert torch.isnan(full[..., :vec].float()).all()
                        assert torch.isnan(full[..., vec + C:].float()).all()
                    # ---- (2) float64
                    gref = c["gref"] if res is None else c["gref"] + c["resref"]
                    assert_close(to_cpu_nchw(g), gref, dtype, "g")
                    if raw:
                        assert dW.dim() == 2 and dW.shape[1] == 9 * C  # the unreduced rows
                        dW = k.dw_wgrad_finalize(dW, C)
                    assert tuple(dW.shape) == (C, 1, 3, 3) and dW.dtype == F32
                    assert_close(dW.cpu(), c["dwref"], F32, "dW", fac=FUSED_DW_FAC)
                    n += 1
    assert n == 3 * (2 if tiled or stride == 2 else 1) * 2 * len(res_modes)


@pytest.mark.parametrize("cls", CLASSES, ids=_id)
def test_two_launch_half(cls):
    """The classes the policy sends there with a data gradient wanted, and every class without
    one (a layer whose input needs no gradient gets the weight gradient alone)."""
    stride, dil, C, dtype, wdtype, one_pass = cls
    k, F = K(), Fn()
    tiled = stride == 1 and dil <= 2
    N, H, W = _shape(dil)
    for mode in MODES:
        if dtype == BF16 and mode & 2:
            continue  # (the bar of the bf16 separate weight gradient under an affine prologue is
            # per case in test_dwconv_families_gpu._check; no class of the two-launch half is bf16)
        c = _case(stride, dil, C, dtype, wdtype, mode)
        x, dy, w, pro = c["x"], c["dy"], c["w"], c["pro"]
        dWe = k.dwconv_wgrad(x, dy, stride, dil, pro, torch_layout=tiled)
        if not tiled:
            dWe = dWe.t().reshape(C, 1, 3, 3).contiguous()
        for want_dx in ([False] if one_pass else [False, True]):
            g, dW, pb, fused = F.dw_backward(x, dy, w, stride, dil, pro, want_dx=want_dx)
            assert not fused and pb is None and _same(dW, dWe)
            assert tuple(dW.shape) == (C, 1, 3, 3) and dW.dtype == F32
            assert_close(dW.cpu(), c["dwref"], F32, "dW", fac=WGRAD_FAC[dtype])
            if not want_dx:
                assert g is None
                continue
            w9c = w.detach().float().view(C, 9).t().contiguous()
            ge = k.dwconv_dgrad(dy, w9c.flip(0).contiguous() if stride == 1 else w9c, stride, dil,
                                (H, W))
            assert _same(g, ge)
            assert_close(to_cpu_nchw(g), c["dx"], dtype, "g (no mask yet)")
