"""GPU: the kernels of csrc/contextnet.hip against torch float64 on the CPU — F.interpolate
(bilinear) + F.conv2d(groups=C, padding=1) and their autograd: the forward with and without the
BatchNorm statistics rows, the backward's d_up and finalized weight gradient, and
functional.up_dwconv_bn behind a training BatchNorm (the plain and the few-sample path).  Bars:
_util.assert_close / tol(dtype) for what is stored in the activation dtype; float32 sums (the
statistics rows, the weight gradient) against float64 at tol(float32) of the sum of the magnitudes
that were added.

Every pitched operand is a slice at element offset `vec` (one 16-byte vector: the least aligned
offset the contract allows) of a NaN-filled buffer whose pitch is two vectors more than the operand
is wide: a NaN that reaches a result or leaves the padding shows an out-of-slice access.

Shapes (N, h, w -> H, W, C), each a place the kernel can go wrong: scale 0 on both axes (a 1 x 1 low
map), ratio 1, non-integer ratios, a one-row output whose every row touches the zero padding, more
than one channel block (136 channels: three blocks of 64), column block (67 columns: five blocks of
14) and row strip, the model's 24 x 24 -> 96 x 96.  One shape is added to the issue's list: 5 x 130
with 8 channels, because a block of the narrow-channel class holds 126 columns and no listed shape
crosses its column-block boundary."""
import functools

import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
NONE, AFFINE, AFFINE_RELU = 0, 2, 3
MODES = [NONE, AFFINE, AFFINE_RELU]
MODE_IDS = ["plain", "affine", "affine_relu"]
SHAPES = [(2, 1, 1, 4, 4, 8), (2, 1, 1, 5, 5, 8), (1, 2, 2, 2, 2, 8), (2, 2, 3, 8, 12, 24),
          (2, 2, 3, 9, 12, 24), (1, 4, 5, 14, 20, 128), (1, 3, 2, 1, 7, 8),
          (2, 9, 17, 37, 67, 136), (1, 24, 24, 96, 96, 16), (1, 3, 40, 5, 130, 8)]
SHAPE_ID = lambda s: "%dx%dx%d_to_%dx%d_c%d" % s  # noqa: E731


def _K():
    from segmentron_amd import hip_ops
    return hip_ops


def _F():
    from segmentron_amd import functional
    return functional


def _vec_of(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def _sum_close(got, ref, mag, what, rel=None):
    """float32 sums against float64: within `rel` (default tol(float32)) of the summed magnitudes."""
    rel = tol(torch.float32) if rel is None else rel
    got, ref, mag = got.double().cpu(), ref.double(), mag.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = ((got - ref).abs() / mag.clamp_min(1e-30)).max().item()
    print("%s: %.3e of the summed magnitudes (bar %.3e)" % (what, err, rel))
    assert err <= rel, "%s: %.3e of the summed magnitudes (bar %.3e)" % (what, err, rel)


def _sliced(x_nchw, dtype):
    v = _vec_of(dtype)
    return to_dev_nhwc(x_nchw, dtype, pitch=x_nchw.shape[1] + 2 * v, off=v)


def _out_slice(N, H, W, C, dtype):
    v = _vec_of(dtype)
    buf = torch.full((N, H, W, C + 2 * v), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[..., v:v + C]


def _pad_is_nan(buf, C):
    v = _vec_of(buf.dtype)
    return bool(torch.isnan(buf[..., :v]).all() and torch.isnan(buf[..., v + C:]).all())


def _c(v):
    return v.view(1, -1, 1, 1).double()


def _bits(t):
    return t.reshape(-1).clone().view(torch.uint8)


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5


def _pro(mode, s, t):
    if mode == NONE:
        return (NONE, None, None)
    return (mode, s.to(DEV), t.to(DEV))


def _act(lo, mode, s, t):
    a = lo.double()
    if mode & 2:
        a = a * _c(s) + _c(t)
    if mode & 1:
        a = torch.relu(a)
    return a


@functools.lru_cache(maxsize=None)
def _case(shape, mode, dtype, align=True):
    """The operands (rounded to the dtype) and the float64 reference of one case, computed once and
    shared by the tests: y, the statistics sums, d_up, dW and the magnitudes behind the sums."""
    N, h, w, H, W, C = shape
    lo = quant(rnd((N, C, h, w), 31) * 1.5 + 0.25, dtype)
    wt = rnd((C, 1, 3, 3), 32) * 0.5
    dy = quant(rnd((N, C, H, W), 33), dtype)
    s, t = _affine(C, 34)
    U = TF.interpolate(_act(lo, mode, s, t), size=(H, W), mode="bilinear",
                       align_corners=align).requires_grad_()
    w64 = wt.double().requires_grad_()
    y = TF.conv2d(U, w64, None, 1, 1, 1, C)
    y.backward(dy.double())
    # the magnitudes the weight gradient's sums add up: the same correlation of |dy| and |U|
    Ua, wa = U.detach().abs(), wt.double().requires_grad_()
    TF.conv2d(Ua, wa, None, 1, 1, 1, C).backward(dy.double().abs())
    yd = y.detach()
    ref = dict(y=yd, d_up=U.grad, dW=w64.grad, dW_mag=wa.grad,
               stat=torch.stack([yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))]),
               stat_mag=torch.stack([yd.abs().sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))]))
    return lo, wt, dy, s, t, ref


def _taps(wt):
    return _F().pack_dw_weight(wt.to(DEV))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
def test_up_dw_forward(shape, mode, dtype):
    """y and the statistics rows; a launch without the rows and a second one with them give the
    same bits."""
    K = _K()
    N, h, w, H, W, C = shape
    lo, wt, _, s, t, ref = _case(shape, mode, dtype)
    lod, w9c = _sliced(lo, dtype), _taps(wt)
    obuf, o = _out_slice(N, H, W, C, dtype)
    y, partial = K.up_dw(lod, (H, W), w9c, _pro(mode, s, t), out=o, want_stats=True)
    assert y.data_ptr() == o.data_ptr()
    rows = K.up_dw_rows(dtype, N, H, W, C, 0)
    assert tuple(partial.shape) == (rows, 2, C) and partial.dtype == torch.float32
    assert_close(to_cpu_nchw(y), ref["y"], dtype, "y")
    tot = partial.double().sum(0).cpu()
    _sum_close(tot[0], ref["stat"][0], ref["stat_mag"][0], "sum y")
    _sum_close(tot[1], ref["stat"][1], ref["stat_mag"][1], "sum y^2")
    assert _pad_is_nan(obuf, C) and _pad_is_nan(lod._base, C)
    y2, none = K.up_dw(lod, (H, W), w9c, _pro(mode, s, t), want_stats=False)
    assert none is None and y2.is_contiguous()
    assert torch.equal(_bits(y2), _bits(y.contiguous()))
    y3, partial3 = K.up_dw(lod, (H, W), w9c, _pro(mode, s, t), want_stats=True)
    assert torch.equal(_bits(y3), _bits(y2)) and torch.equal(_bits(partial3), _bits(partial))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
def test_up_dw_backward(shape, mode, dtype):
    """d_up and the finalized weight gradient in the parameter's [C,1,3,3] layout; two launches
    give the same bits."""
    K = _K()
    N, h, w, H, W, C = shape
    lo, wt, dy, s, t, ref = _case(shape, mode, dtype)
    lod, dyd, w9c = _sliced(lo, dtype), _sliced(dy, dtype), _taps(wt)
    gbuf, g = _out_slice(N, H, W, C, dtype)
    d_up, pw = K.up_dw_bwd(dyd, lod, w9c, _pro(mode, s, t), out=g)
    assert d_up.data_ptr() == g.data_ptr() and d_up.dtype == dtype
    rows = K.up_dw_rows(dtype, N, H, W, C, 1)
    assert tuple(pw.shape) == (rows, 9, C) and pw.dtype == torch.float32
    assert_close(to_cpu_nchw(d_up), ref["d_up"], dtype, "d_up")
    dW = K.dw_wgrad_finalize(pw.view(rows, 9 * C), C)
    assert tuple(dW.shape) == (C, 1, 3, 3)
    _sum_close(dW, ref["dW"], ref["dW_mag"], "dW")
    assert _pad_is_nan(gbuf, C) and _pad_is_nan(lod._base, C) and _pad_is_nan(dyd._base, C)
    d2, pw2 = K.up_dw_bwd(dyd, lod, w9c, _pro(mode, s, t))
    assert torch.equal(_bits(d2), _bits(d_up.contiguous())) and torch.equal(_bits(pw2), _bits(pw))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 2, 3, 8, 12, 24), (2, 1, 1, 5, 5, 8)], ids=SHAPE_ID)
def test_up_dw_without_aligned_corners(shape, dtype):
    K = _K()
    N, h, w, H, W, C = shape
    lo, wt, dy, s, t, ref = _case(shape, AFFINE_RELU, dtype, False)
    lod, dyd, w9c = _sliced(lo, dtype), _sliced(dy, dtype), _taps(wt)
    y, _ = K.up_dw(lod, (H, W), w9c, _pro(AFFINE_RELU, s, t), align_corners=False)
    assert_close(to_cpu_nchw(y), ref["y"], dtype, "y")
    d_up, pw = K.up_dw_bwd(dyd, lod, w9c, _pro(AFFINE_RELU, s, t), align_corners=False)
    assert_close(to_cpu_nchw(d_up), ref["d_up"], dtype, "d_up")
    _sum_close(K.dw_wgrad_finalize(pw.view(pw.shape[0], 9 * C), C), ref["dW"], ref["dW_mag"], "dW")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", [(1, 2, 2, 2, 2, 8), (2, 9, 17, 9, 17, 136)], ids=SHAPE_ID)
def test_ratio_one_equals_the_plain_depthwise_conv(shape, mode, dtype):
    """A resize to the same size is the identity: act followed by seg_dwconv3x3."""
    K = _K()
    N, h, w, H, W, C = shape
    lo, wt, _, s, t, ref = _case(shape, mode, dtype)
    lod, w9c = _sliced(lo, dtype), _taps(wt)
    y, _ = K.up_dw(lod, (H, W), w9c, _pro(mode, s, t))
    plain, _ = K.dwconv(lod, wt.to(DEV), 1, 1, _pro(mode, s, t))
    assert_close(to_cpu_nchw(y), to_cpu_nchw(plain).double(), dtype, "against seg_dwconv3x3")
    assert_close(to_cpu_nchw(y), ref["y"], dtype, "against float64")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bf16_low_map_gradient_through_the_rounded_d_up(dtype):
    """d_up (rounded to the activation dtype) through the existing seg_bilinear_bwd: the gradient
    of the activated low map."""
    K = _K()
    shape = (2, 9, 17, 37, 67, 136)
    N, h, w, H, W, C = shape
    lo, wt, dy, s, t, ref = _case(shape, NONE, dtype)
    lo64 = lo.double().requires_grad_()
    U = TF.interpolate(lo64, size=(H, W), mode="bilinear", align_corners=True)
    TF.conv2d(U, wt.double(), None, 1, 1, 1, C).backward(dy.double())
    d_up, _ = K.up_dw_bwd(_sliced(dy, dtype), _sliced(lo, dtype), _taps(wt))
    ga = K.bilinear_bwd(d_up, (h, w), True)
    assert_close(to_cpu_nchw(ga), lo64.grad, dtype, "d_lo")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_operands_are_checked_before_the_launch(dtype):
    K = _K()
    v = _vec_of(dtype)
    C = 2 * v
    lo = torch.zeros((1, 2, 3, C), dtype=dtype, device=DEV)
    w9c = torch.zeros((9, C), device=DEV)
    with pytest.raises(ValueError, match="expected"):
        K.up_dw(lo, (4, 6), w9c, out=torch.zeros((1, 4, 6, C + v), dtype=dtype, device=DEV))
    with pytest.raises(ValueError, match="tap-major"):
        K.up_dw(lo, (4, 6), torch.zeros((C, 9), device=DEV))
    with pytest.raises(ValueError, match="tap-major"):
        K.up_dw(lo, (4, 6), w9c.to(dtype) if dtype != torch.float32 else w9c.double())
    with pytest.raises(ValueError, match="offset"):
        K.up_dw(torch.zeros((1, 2, 3, C + v), dtype=dtype, device=DEV)[..., 1:C + 1], (4, 6), w9c)
    with pytest.raises(ValueError, match="scale / shift"):
        K.up_dw(lo, (4, 6), w9c, (AFFINE, torch.zeros(C - 1, device=DEV), torch.zeros(C, device=DEV)))
    with pytest.raises(ValueError, match="one for every operand"):
        other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
        K.up_dw_bwd(torch.zeros((1, 4, 6, C), dtype=other, device=DEV), lo, w9c)
    with pytest.raises(ValueError, match="expected"):
        K.up_dw_bwd(torch.zeros((2, 4, 6, C), dtype=dtype, device=DEV), lo, w9c)
    torch.cuda.synchronize()


# ------------------------------------------------- functional.up_dwconv_bn behind a BatchNorm
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", [(2, 24, 24, 53, 47), (2, 9, 17, 37, 67)],
                         ids=["plain", "few_sample"])
def test_functional_up_dwconv_bn_behind_a_training_batchnorm(geom, dtype, monkeypatch):
    """The low map carries a pending training-mode BatchNorm (N*h*w = 1152 rows: reduce + finalize +
    apply; 306 rows: the float64 few-sample launch); the node saves the low map and the weight
    alone, its backward is one seg_up_dw_bwd, the existing seg_bilinear_bwd and the BatchNorm's
    own backward."""
    F, K = _F(), _K()
    N, h, w, H, W = geom
    C = 16
    plain = N * h * w > K.SMALL_BN_ROWS
    assert plain == (geom[1] == 24)
    calls = []
    for name in ("up_dw", "up_dw_bwd", "bilinear", "bilinear_bwd", "dwconv", "bn_bwd_small",
                 "bn_bwd_reduce_partial"):
        def spy(*a, _f=getattr(K, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(K, name, spy)
    monkeypatch.setattr(F, "_CTX_UP_DW", "1")
    eps = 1e-5
    lo = quant(rnd((N, C, h, w), 41) * 1.5 + 0.25, dtype)
    gam, bet = _affine(C, 42)
    gam2, bet2 = _affine(C, 43)
    wt = rnd((C, 1, 3, 3), 44) * 0.5
    gout = quant(rnd((N, C, H, W), 45), dtype)
    bn_in = torch.nn.BatchNorm2d(C, eps=eps).to(DEV).train()
    bn_out = torch.nn.BatchNorm2d(C, eps=eps).to(DEV).train()
    conv = torch.nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False).to(DEV)
    with torch.no_grad():
        bn_in.weight.copy_(gam)
        bn_in.bias.copy_(bet)
        bn_out.weight.copy_(gam2)
        bn_out.bias.copy_(bet2)
        conv.weight.copy_(wt)
    lod = to_dev_nhwc(lo, dtype).requires_grad_()
    with torch.no_grad():  # the producer's statistics partials, as a conv epilogue leaves them
        lf = lod.double()
        part = torch.stack([lf.sum((0, 1, 2)), (lf * lf).sum((0, 1, 2))]).float().view(1, 2, C)
    act = F.Act(lod, F.finish_bn(bn_in, part, N * h * w, y=lod))
    assert F._bn_backward_is_plain(act.bn) == plain
    # (no ReLU behind the output BatchNorm here: its mask would be taken of the y STORED in the
    # activation dtype, and in bf16 the few elements whose sign the rounding decides would each
    # move the gradient of the low-map pixel below them by a whole term — a property of the
    # consumer's mask, not of the node; the model tests run the ReLU)
    a = F.up_dwconv_bn(act, (H, W), conv, bn_out)
    saved = a.t.grad_fn.saved_tensors
    assert len(saved) == 2 and {tuple(v.shape) for v in saved} == {(N, h, w, C), (C, 1, 3, 3)}
    out = F.materialize(a)

    lor = lo.double().requires_grad_()
    ps = [p.double().requires_grad_() for p in (gam, bet, wt, gam2, bet2)]
    al = TF.batch_norm(lor, None, None, ps[0], ps[1], True, 0.1, eps)
    al.retain_grad()
    U = TF.interpolate(al, size=(H, W), mode="bilinear", align_corners=True)
    yr = TF.conv2d(U, ps[2], None, 1, 1, 1, C)
    yr.retain_grad()
    outr = TF.batch_norm(yr, None, None, ps[3], ps[4], True, 0.1, eps)
    assert_close(to_cpu_nchw(a.t), yr.detach(), dtype, "y")
    # (the output BatchNorm normalises the STORED y: its rounding is amplified by gamma / std)
    assert_close(to_cpu_nchw(out), outr.detach(), dtype, "bn(y)",
                 scale=max(outr.abs().max().item(), gam2.max().item()
                           * yr.abs().max().item() / yr.std().item()))
    out.backward(to_dev_nhwc(gout, dtype))
    outr.backward(gout.double())
    assert calls.count("up_dw") == 1 and calls.count("up_dw_bwd") == 1
    assert calls.count("bilinear_bwd") == 1
    assert "bilinear" not in calls and "dwconv" not in calls
    if plain:  # (the output BatchNorm has more than 1024 rows in both cases)
        assert "bn_bwd_small" not in calls and calls.count("bn_bwd_reduce_partial") >= 1
    else:
        assert calls.count("bn_bwd_small") == 1
    # the weight gradient: a float32 sum of products of dy, which is stored in the activation dtype
    dy, Ud = yr.grad, U.detach()
    wa = wt.double().requires_grad_()
    TF.conv2d(Ud.abs(), wa, None, 1, 1, 1, C).backward(dy.abs())
    _sum_close(conv.weight.grad, ps[2].grad, wa.grad, "dW", rel=tol(dtype))
    # dgamma / dbeta of the low map's BatchNorm: sums of the gradient of the activated low map,
    # which is stored in the activation dtype
    ga = al.grad
    xhat = (al.detach() - _c(bet)) / _c(gam)
    _sum_close(bn_in.weight.grad, ps[0].grad, (ga * xhat).abs().sum((0, 2, 3)), "dgamma",
               rel=tol(dtype))
    _sum_close(bn_in.bias.grad, ps[1].grad, ga.abs().sum((0, 2, 3)), "dbeta", rel=tol(dtype))
    # (dx is the remainder of cancelling terms of the size of that gradient times gamma / std)
    scale = max(ga.abs().max().item() * gam.max().item() / (lo.std().item() + eps),
                lor.grad.abs().max().item())
    assert_close(to_cpu_nchw(lod.grad), lor.grad, dtype, "d_lo", scale=scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_functional_routes_agree(dtype, monkeypatch):
    """SEG_CTX_UP_DW = 0 (bilinear + dwconv_bn) and = 1 (the node) on the same operands: both within
    the bar of the float64 reference, in evaluation mode (no statistics) too."""
    F = _F()
    shape = (2, 4, 5, 14, 20, 128)
    N, h, w, H, W, C = shape
    lo, wt, dy, s, t, ref = _case(shape, NONE, dtype)
    conv = torch.nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(wt)
    for training in (True, False):
        bn = torch.nn.BatchNorm2d(C).to(DEV).train(training)
        for side in ("0", "1"):
            monkeypatch.setattr(F, "_CTX_UP_DW", side)
            lod = to_dev_nhwc(lo, dtype).requires_grad_()
            conv.weight.grad = None
            a = F.up_dwconv_bn(F.Act(lod), (H, W), conv, bn)
            assert a.bn.training == training
            # (the two-launch route rounds the upsampled map to the activation dtype first)
            assert_close(to_cpu_nchw(a.t), ref["y"], dtype, "y, side " + side, fac=2 - int(side))
            a.t.backward(to_dev_nhwc(dy, dtype))
            _sum_close(conv.weight.grad, ref["dW"], ref["dW_mag"], "dW, side " + side,
                       rel=tol(dtype))
            assert lod.grad is not None and torch.isfinite(lod.grad).all()
