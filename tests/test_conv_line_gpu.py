"""GPU: the 3-tap line convolution of csrc/conv_line.hip (forward, data gradient through the same
entry point, weight gradient, BatchNorm statistics, the epilogue addend) against a float64
conv2d on the CPU.

The oracle's operands are the operands as the kernel is documented to see them: the prologue in
float32 (a fused multiply-add, as every prologue of the library, then max), rounded to bf16 where
the dtype is bf16, zero padding AFTER it.  Bounds are derived, not tuned.  With n the number of
summed products of an output element and S the same sum over the absolute values:
    float32   |y - y64| <= n * 2^-23 * S
    bf16      that + 2^-8 * |y64|            (the one rounding on store)
and the same form for the weight gradient (n = pixels) and the statistics (n = pixels, of the
values as stored).  Every launch is repeated and must give the same bits."""
import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
H_, W_ = 0, 1  # axis
SENTINEL = 12345.0

# (N, H, W, C, axis, d)
SHAPE_1 = (2, 5, 37, 16, W_, 1)    # W crosses a 32-pixel fragment with a tail; row wrap shows
SHAPE_2 = (2, 37, 5, 16, H_, 2)    # a tap that reaches the neighbouring image shows
SHAPE_3H = (2, 12, 9, 16, H_, 17)  # every side tap outside: the centre tap alone
SHAPE_3W = (2, 7, 40, 16, W_, 17)  # some inside
SHAPES_4 = [(2, 19, 23, C, ax, d) for C in (32, 64) for d in (5, 9) for ax in (H_, W_)]
BASE_SHAPES = [SHAPE_1, SHAPE_2, SHAPE_3H, SHAPE_3W] + SHAPES_4
PRO_SHAPES = [SHAPE_1, SHAPE_2, (2, 19, 23, 32, W_, 5), (2, 19, 23, 64, H_, 9)]


def _sid(s):
    return "%dx%dx%dx%d-%s-d%d" % (s[0], s[1], s[2], s[3], "HW"[s[4]], s[5])


def _K():
    from segmentron_amd import hip_ops
    return hip_ops


def _F():
    from segmentron_amd import functional
    return functional


def _fma32(x, s, t):
    """float32 fused multiply-add: the product of two float32 is exact in float64."""
    return (x.double() * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)).float()


def _activated(x, pro_kind, s, t, dtype):
    """The operand the MFMA sees, as float64 (x: CPU NCHW float, already rounded to dtype)."""
    v = x
    if pro_kind == "affine_relu":
        v = _fma32(v, s, t)
    if pro_kind in ("relu", "affine_relu"):
        v = v.clamp_min(0.0)
    return quant(v, dtype).double()


def _pro_arg(K, pro_kind, s, t):
    if pro_kind == "none":
        return None
    if pro_kind == "relu":
        return (K.PRO_RELU, None, None)
    return (K.PRO_AFFINE_RELU, s.to(DEV), t.to(DEV))


def _conv64(x, w, axis, d):
    pad, dil = ((d, 0), (d, 1)) if axis == H_ else ((0, d), (1, d))
    return TF.conv2d(x, w, None, 1, pad, dil)


def _weight(C, axis, dtype, seed):
    shape = (C, C, 3, 1) if axis == H_ else (C, C, 1, 3)
    return quant(rnd(shape, seed, (3.0 * C) ** -0.5), dtype)


def _bound(err_ok_n, S, y64, dtype):
    b = err_ok_n * 2.0 ** -23 * S
    if dtype == torch.bfloat16:
        b = b + 2.0 ** -8 * y64.abs()
    return b


def _check(got, y64, S, n, dtype, what):
    got = got.double()
    assert torch.isfinite(got).all(), what
    over = (got - y64).abs() - _bound(n, S, y64, dtype)
    assert over.max().item() <= 0.0, "%s: %.3e beyond the bound" % (what, over.max().item())


def _inputs(shape, dtype, seed, pro_kind):
    N, H, W, C, axis, d = shape
    x = quant(rnd((N, C, H, W), seed), dtype)
    w = _weight(C, axis, dtype, seed + 1)
    s = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 2))
    t = 0.25 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 3))  # act(0) != 0
    return x, w, s, t


def _forward_case(shape, dtype, pro_kind="none", slices=False, add=False, stats=False, seed=1):
    K, F = _K(), _F()
    N, H, W, C, axis, d = shape
    x, w, s, t = _inputs(shape, dtype, seed, pro_kind)
    xa = _activated(x, pro_kind, s, t, dtype)
    y64 = _conv64(xa, w.double(), axis, d)
    S = _conv64(xa.abs(), w.double().abs(), axis, d)
    n = 3 * C
    tdt = dtype
    wp = F.pack_conv_weight(w.to(DEV), C, tdt)
    out = obuf = None
    if slices:  # x: the upper half of a 2C-wide buffer; y: the lower half of another one
        xd = to_dev_nhwc(x, dtype, pitch=2 * C, off=C)
        obuf = torch.full((N, H, W, 2 * C), SENTINEL, dtype=dtype, device=DEV)
        out = obuf[..., :C]
    else:
        xd = to_dev_nhwc(x, dtype)
    addd = None
    if add:
        a = quant(rnd((N, C, H, W), seed + 5), dtype)
        addd = to_dev_nhwc(a, dtype, pitch=C + 8, off=8)
        y64 = y64 + a.double()
        S = S + a.double().abs()
        n += 1
    pro = _pro_arg(K, pro_kind, s, t)
    y, partial = K.conv_line(xd, wp, axis, d, pro, out=out, add=addd, want_stats=stats)
    _check(to_cpu_nchw(y), y64, S, n, dtype, "y")
    if slices:
        assert torch.equal(obuf[..., C:], torch.full_like(obuf[..., C:], SENTINEL))
    if stats:
        geo = K.conv_line_geom(dtype, N, H, W, C)
        assert tuple(partial.shape) == (geo["grid"], 2, C) and partial.dtype == torch.float32
        ys = to_cpu_nchw(y).double()  # the values as stored
        P = N * H * W
        sums = K.colsum(partial.view(partial.shape[0], 2 * C), f64=False).double().cpu().view(2, C)
        a1, a2 = ys.abs().sum((0, 2, 3)), (ys * ys).sum((0, 2, 3))
        assert ((sums[0] - ys.sum((0, 2, 3))).abs() <= P * 2.0 ** -23 * a1).all()
        assert ((sums[1] - a2).abs() <= P * 2.0 ** -23 * a2).all()
    # bit-identical on a second launch
    if slices:
        obuf2 = torch.full((N, H, W, 2 * C), SENTINEL, dtype=dtype, device=DEV)
        out = obuf2[..., :C]
    y2, partial2 = K.conv_line(xd, wp, axis, d, pro, out=out, add=addd, want_stats=stats)
    assert torch.equal(y2, y)
    if stats:
        assert torch.equal(partial2, partial)
    return y, y64


def _dgrad_case(shape, dtype, seed=11):
    """The data gradient: the same entry point on dy with the weights repacked [C][2-t][O];
    the oracle is float64 autograd through conv2d."""
    K, F = _K(), _F()
    N, H, W, C, axis, d = shape
    dy = quant(rnd((N, C, H, W), seed), dtype)
    w = _weight(C, axis, dtype, seed + 1)
    x0 = torch.zeros((N, C, H, W), dtype=torch.float64, requires_grad=True)
    (dx64,) = torch.autograd.grad(_conv64(x0, w.double(), axis, d), x0, dy.double())
    wt_abs = w.double().abs().permute(1, 0, 2, 3).flip(2, 3)
    S = _conv64(dy.double().abs(), wt_abs, axis, d)
    wt = F.pack_conv_weight_dgrad(w.to(DEV), C, dtype)
    dyd = to_dev_nhwc(dy, dtype)
    dx, _ = K.conv_line(dyd, wt, axis, d)
    _check(to_cpu_nchw(dx), dx64, S, 3 * C, dtype, "dx")
    dx2, _ = K.conv_line(dyd, wt, axis, d)
    assert torch.equal(dx2, dx)


def _wgrad_case(shape, dtype, pro_kind="none", slices=False, seed=21):
    K = _K()
    N, H, W, C, axis, d = shape
    x, w, s, t = _inputs(shape, dtype, seed, pro_kind)
    dy = quant(rnd((N, C, H, W), seed + 7), dtype)
    xa = _activated(x, pro_kind, s, t, dtype)
    w0 = torch.zeros_like(w, dtype=torch.float64, requires_grad=True)
    (dw64,) = torch.autograd.grad(_conv64(xa, w0, axis, d), w0, dy.double())
    (S,) = torch.autograd.grad(_conv64(xa.abs(), w0, axis, d), w0, dy.double().abs())
    if slices:
        xd = to_dev_nhwc(x, dtype, pitch=2 * C, off=C)
        dyd = to_dev_nhwc(dy, dtype, pitch=2 * C, off=0)
    else:
        xd, dyd = to_dev_nhwc(x, dtype), to_dev_nhwc(dy, dtype)
    pro = _pro_arg(K, pro_kind, s, t)
    dW = K.conv_line_wgrad(xd, dyd, axis, d, pro)  # [o][c][tap], after seg_colsum
    assert dW.dtype == torch.float32 and tuple(dW.shape) == (C, C, 3)
    got = dW.view(w.shape).cpu()  # the parameter's own memory layout for both kernel shapes
    _check(got, dw64, S, N * H * W, torch.float32, "dW")
    assert torch.equal(K.conv_line_wgrad(xd, dyd, axis, d, pro), dW)


# ------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", BASE_SHAPES, ids=_sid)
def test_forward(shape, dtype):
    _forward_case(shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_forward_dilation_beyond_the_image_is_the_centre_tap(dtype):
    N, H, W, C, axis, d = SHAPE_3H
    _, y64 = _forward_case(SHAPE_3H, dtype, seed=1)
    x, w, _, _ = _inputs(SHAPE_3H, dtype, 1, "none")
    centre = TF.conv2d(x.double(), w.double()[:, :, 1:2, :])
    assert (y64 - centre).abs().max().item() <= 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", BASE_SHAPES, ids=_sid)
def test_data_gradient(shape, dtype):
    _dgrad_case(shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [SHAPE_1, SHAPE_2, (2, 19, 23, 64, W_, 9)], ids=_sid)
def test_forward_channel_slices_leave_the_other_half_alone(shape, dtype):
    _forward_case(shape, dtype, slices=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pro_kind", ["none", "relu", "affine_relu"])
@pytest.mark.parametrize("shape", PRO_SHAPES, ids=_sid)
def test_forward_prologue_padding_stays_zero(shape, pro_kind, dtype):
    _forward_case(shape, dtype, pro_kind=pro_kind, seed=3)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [SHAPE_1] + SHAPES_4[:2] + SHAPES_4[-2:], ids=_sid)
def test_statistics(shape, dtype):
    N, H, W, C, _, _ = shape
    assert _K().conv_line_geom(dtype, N, H, W, C)["grid"] >= 2
    _forward_case(shape, dtype, pro_kind="affine_relu", stats=True, seed=5)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_tiles_per_block(dtype):
    shape = (2, 260, 256, 16, W_, 2)
    N, H, W, C, _, _ = shape
    assert N * H * W <= 2 ** 18
    assert _K().conv_line_geom(dtype, N, H, W, C)["tiles_per_block"] >= 2
    _forward_case(shape, dtype, pro_kind="relu", stats=True, seed=7)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [SHAPE_1, SHAPE_2, (2, 19, 23, 64, H_, 5)], ids=_sid)
def test_epilogue_addend(shape, dtype):
    _forward_case(shape, dtype, add=True, seed=9)


# ------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", BASE_SHAPES, ids=_sid)
def test_weight_gradient(shape, dtype):
    _wgrad_case(shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [SHAPE_1, SHAPE_2, (2, 19, 23, 64, W_, 9)], ids=_sid)
def test_weight_gradient_channel_slices(shape, dtype):
    _wgrad_case(shape, dtype, slices=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pro_kind", ["relu", "affine_relu"])
@pytest.mark.parametrize("shape", PRO_SHAPES, ids=_sid)
def test_weight_gradient_prologue(shape, pro_kind, dtype):
    _wgrad_case(shape, dtype, pro_kind=pro_kind, seed=23)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [16, 64])
def test_weight_gradient_splits_and_trips(C, dtype):
    """splits >= 2 and a split that covers more than one staging trip."""
    N, H, W = (2, 192, 192) if C == 16 else (2, 72, 64)
    geo = _K().conv_line_geom(dtype, N, H, W, C)
    trips = -(-N * H * W // geo["wgrad_trip"])
    assert geo["wgrad_splits"] >= 2 and trips > geo["wgrad_splits"]
    _wgrad_case((N, H, W, C, H_ if C == 16 else W_, 2), dtype, pro_kind="relu", seed=25)


def test_host_queries_refuse_what_the_kernels_do_not_serve():
    K = _K()
    assert K.conv_line_ok(torch.bfloat16, 16, 0, 17) and K.conv_line_ok(torch.float32, 64, 1, 1)
    assert not K.conv_line_ok(torch.bfloat16, 40, 0, 1)
    assert not K.conv_line_ok(torch.bfloat16, 32, 2, 1)
    assert not K.conv_line_ok(torch.bfloat16, 32, 0, 0)
    assert K.LIB.query("seg_conv_line_geom", 1, 2, 5, 37, 40, 1) == -1
    x = torch.zeros((1, 4, 4, 40), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        K.conv_line(x, torch.zeros((40, 120), dtype=torch.bfloat16, device=DEV), 0, 1)
