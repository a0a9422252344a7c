"""GPU: the 40-channel class and the bias of the 3-tap line convolution (csrc/conv_line.hip,
EDANet's EDABlock) against a float64 conv2d on the CPU: forward, data gradient through the same
entry point, weight gradient, statistics, and the bias gradient taken from the statistics rows of
a data-gradient launch.

Oracle and bounds are those of tests/test_conv_line_gpu.py (its helpers are used as they are): the
operands as the kernel sees them (prologue in float32, rounded to bf16 where the dtype is bf16,
zero padding AFTER it), and with n the number of summed terms of an output element and S the same
sum over the absolute values
    float32   |y - y64| <= n * 2^-23 * S
    bf16      that + 2^-8 * |y64|
The bias is one more term (n + 1, S + |b|).  Every launch is repeated and must give the same bits.
In bf16 a k-step is 16 channels: channels 40..47 of the third step and output rows 40..63 of the
second 32-row group are void, which the pitched cases guard with NaN on the input side (a read
beyond channel 39 would poison the product) and a sentinel on the output side."""
import pytest
import torch
import torch.nn as nn

import test_conv_line_gpu as L
from _util import DEV, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu

DTYPES, IDS, H_, W_, SENTINEL = L.DTYPES, L.IDS, L.H_, L.W_, L.SENTINEL
C = 40
# (N, H, W, C, axis, d)
SHAPES = [(2, 5, 37, C, W_, 1),    # fragment tail, row wrap
          (2, 37, 5, C, H_, 2),    # a tap that reaches the neighbouring image
          (2, 12, 9, C, H_, 16),   # every side tap outside: the centre tap alone
          (2, 7, 40, C, W_, 16)]   # some taps inside
BUF, LO = 264, 80                  # the pitched cases: channels [80, 120) of a stage-1 buffer


def _bias(seed):
    return rnd((C,), seed + 40, 0.5)  # float32 in every dtype


def _forward_case(shape, dtype, pro_kind="none", bias=False, pitched=False, add=False, seed=1):
    K, F = L._K(), L._F()
    N, H, W, _, axis, d = shape
    x, w, s, t = L._inputs(shape, dtype, seed, pro_kind)
    xa = L._activated(x, pro_kind, s, t, dtype)
    y64 = L._conv64(xa, w.double(), axis, d)
    S = L._conv64(xa.abs(), w.double().abs(), axis, d)
    n = 3 * C
    b = None
    if bias:
        b = _bias(seed)
        y64 = y64 + b.double().view(1, -1, 1, 1)
        S = S + b.double().abs().view(1, -1, 1, 1)
        n += 1
    addd = None
    if add:
        a = quant(rnd((N, C, H, W), seed + 5), dtype)
        addd = to_dev_nhwc(a, dtype, pitch=C + 8, off=8)
        y64, S, n = y64 + a.double(), S + a.double().abs(), n + 1
    wp = F.pack_conv_weight(w.to(DEV), C, dtype)
    assert tuple(wp.shape) == (C, 3 * C)

    def target():
        if not pitched:
            return None, None
        obuf = torch.full((N, H, W, BUF), SENTINEL, dtype=dtype, device=DEV)
        return obuf, obuf[..., LO:LO + C]
    xd = to_dev_nhwc(x, dtype, pitch=BUF, off=LO + C) if pitched else to_dev_nhwc(x, dtype)
    pro = L._pro_arg(K, pro_kind, s, t)
    bd = None if b is None else b.to(DEV)
    obuf, out = target()
    y, partial = K.conv_line_bias(xd, wp, bd, axis, d, pro, out=out, add=addd, want_stats=True)
    L._check(to_cpu_nchw(y), y64, S, n, dtype, "y")
    if pitched:
        keep = torch.ones(BUF, dtype=torch.bool, device=DEV)
        keep[LO:LO + C] = False
        assert (obuf[..., keep] == SENTINEL).all()
    # the statistics: of the values as stored, the bias among them
    geo = K.conv_line_geom(dtype, N, H, W, C)
    assert tuple(partial.shape) == (geo["grid"], 2, C) and partial.dtype == torch.float32
    ys = to_cpu_nchw(y).double()
    P = N * H * W
    sums = K.colsum(partial.view(partial.shape[0], 2 * C), f64=False).double().cpu().view(2, C)
    a1, a2 = ys.abs().sum((0, 2, 3)), (ys * ys).sum((0, 2, 3))
    assert ((sums[0] - ys.sum((0, 2, 3))).abs() <= P * 2.0 ** -23 * a1).all()
    assert ((sums[1] - a2).abs() <= P * 2.0 ** -23 * a2).all()
    obuf2, out2 = target()
    y2, partial2 = K.conv_line_bias(xd, wp, bd, axis, d, pro, out=out2, add=addd,
                                    want_stats=True)
    assert torch.equal(y2, y) and torch.equal(partial2, partial)
    return y, y64


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("pro_kind", ["none", "affine_relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=L._sid)
def test_forward(shape, pro_kind, bias, dtype):
    _forward_case(shape, dtype, pro_kind=pro_kind, bias=bias, seed=3)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=L._sid)
def test_forward_into_a_pitched_slice(shape, bias, dtype):
    """x: channels [120, 160) of a 264-channel buffer of NaN; y: channels [80, 120) of a buffer of
    a sentinel, whose other 224 channels must keep it."""
    _forward_case(shape, dtype, pro_kind="affine_relu", bias=bias, pitched=True, seed=5)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES[:2], ids=L._sid)
def test_bias_comes_before_the_addend(shape, dtype):
    _forward_case(shape, dtype, bias=True, add=True, seed=9)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_tiles_per_block(dtype):
    shape = (2, 260, 256, C, W_, 2)
    assert L._K().conv_line_geom(dtype, 2, 260, 256, C)["tiles_per_block"] >= 2
    _forward_case(shape, dtype, pro_kind="affine_relu", bias=True, seed=7)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 12, 9, C, H_, 16), (2, 9, 7, C, H_, 1)], ids=L._sid)
def test_bias_is_visible_at_the_border_of_the_next_convolution(shape, dtype):
    """mid = lineH(x) + bias, y = lineW(mid): the second convolution pads `mid` with zeros, not
    with the bias.  The oracle's `mid` is the one the device stored; folding the bias through the
    second convolution (sum of its taps x bias everywhere) is what the result must NOT be."""
    K, F = L._K(), L._F()
    N, H, W, _, _, d = shape
    x, wa, _, _ = L._inputs(shape, dtype, 13, "none")
    wb = L._weight(C, W_, dtype, 17)
    b = _bias(13)
    mid, _ = K.conv_line_bias(to_dev_nhwc(x, dtype), F.pack_conv_weight(wa.to(DEV), C, dtype),
                              b.to(DEV), H_, d)
    y, _ = K.conv_line_bias(mid, F.pack_conv_weight(wb.to(DEV), C, dtype), None, W_, 1)
    m = to_cpu_nchw(mid).double()
    L._check(to_cpu_nchw(mid), L._conv64(x.double(), wa.double(), H_, d) + b.double().view(1, -1, 1, 1),
             L._conv64(x.double().abs(), wa.double().abs(), H_, d) + b.double().abs().view(1, -1, 1, 1),
             3 * C + 1, dtype, "mid")
    y64 = L._conv64(m, wb.double(), W_, 1)
    L._check(to_cpu_nchw(y), y64, L._conv64(m.abs(), wb.double().abs(), W_, 1), 3 * C, dtype, "y")
    folded = L._conv64(m - b.double().view(1, -1, 1, 1), wb.double(), W_, 1) \
        + (wb.double().sum((2, 3)) @ b.double()).view(1, -1, 1, 1)
    edge = (folded - y64)[..., 0].abs().max().item()
    inner = (folded - y64)[..., 1:-1].abs().max().item()
    assert edge > 1e-2 and inner < 1e-9


# ------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=L._sid)
def test_data_gradient_and_the_bias_gradient_from_its_statistics(shape, dtype):
    """dx through the forward entry point with the weights repacked [C][2-t][O]; row 0 of its
    statistics is the per-channel sum of dx as stored — the bias gradient of a biased producer of
    x — in a fixed order."""
    K, F = L._K(), L._F()
    N, H, W, _, axis, d = shape
    dy = quant(rnd((N, C, H, W), 11), dtype)
    w = L._weight(C, axis, dtype, 12)
    x0 = torch.zeros((N, C, H, W), dtype=torch.float64, requires_grad=True)
    (dx64,) = torch.autograd.grad(L._conv64(x0, w.double(), axis, d), x0, dy.double())
    wt_abs = w.double().abs().permute(1, 0, 2, 3).flip(2, 3)
    S = L._conv64(dy.double().abs(), wt_abs, axis, d)
    wt = F.pack_conv_weight_dgrad(w.to(DEV), C, dtype)
    dyd = to_dev_nhwc(dy, dtype, pitch=BUF, off=LO)
    dx, rows = K.conv_line_bias(dyd, wt, None, axis, d, want_stats=True)
    L._check(to_cpu_nchw(dx), dx64, S, 3 * C, dtype, "dx")
    stored = to_cpu_nchw(dx).double()
    db = K.colsum(rows.view(rows.shape[0], 2 * C), f64=False)[:C].double().cpu()
    bound = N * H * W * 2.0 ** -23 * stored.abs().sum((0, 2, 3))
    assert ((db - stored.sum((0, 2, 3))).abs() <= bound).all()
    dx2, rows2 = K.conv_line_bias(dyd, wt, None, axis, d, want_stats=True)
    assert torch.equal(dx2, dx) and torch.equal(rows2, rows)


# ------------------------------------------------------------------------------ weight gradient
def _wgrad_case(shape, dtype, pro_kind="none", pitched=False, seed=21):
    K = L._K()
    N, H, W, _, axis, d = shape
    x, w, s, t = L._inputs(shape, dtype, seed, pro_kind)
    dy = quant(rnd((N, C, H, W), seed + 7), dtype)
    xa = L._activated(x, pro_kind, s, t, dtype)
    w0 = torch.zeros_like(w, dtype=torch.float64, requires_grad=True)
    (dw64,) = torch.autograd.grad(L._conv64(xa, w0, axis, d), w0, dy.double())
    (S,) = torch.autograd.grad(L._conv64(xa.abs(), w0, axis, d), w0, dy.double().abs())
    if pitched:
        xd = to_dev_nhwc(x, dtype, pitch=BUF, off=LO + C)
        dyd = to_dev_nhwc(dy, dtype, pitch=BUF, off=LO)
    else:
        xd, dyd = to_dev_nhwc(x, dtype), to_dev_nhwc(dy, dtype)
    pro = L._pro_arg(K, pro_kind, s, t)
    dW = K.conv_line_wgrad(xd, dyd, axis, d, pro)
    assert dW.dtype == torch.float32 and tuple(dW.shape) == (C, C, 3)
    L._check(dW.view(w.shape).cpu(), dw64, S, N * H * W, torch.float32, "dW")
    assert torch.equal(K.conv_line_wgrad(xd, dyd, axis, d, pro), dW)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
@pytest.mark.parametrize("pro_kind", ["none", "affine_relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=L._sid)
def test_weight_gradient(shape, pro_kind, pitched, dtype):
    _wgrad_case(shape, dtype, pro_kind=pro_kind, pitched=pitched)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_weight_gradient_splits_and_trips(dtype):
    """splits >= 2 and a split that covers more than one staging trip."""
    N, H, W = 2, 72, 64
    geo = L._K().conv_line_geom(dtype, N, H, W, C)
    trips = -(-N * H * W // geo["wgrad_trip"])
    assert geo["wgrad_splits"] >= 2 and trips > geo["wgrad_splits"]
    _wgrad_case((N, H, W, C, W_, 2), dtype, pro_kind="relu", seed=25)


# ------------------------------------------------------------------------- functional.line_conv_bn
def _pair_modules(d, seed):
    torch.manual_seed(seed)
    ca = nn.Conv2d(C, C, (3, 1), padding=(d, 0), dilation=d)
    cb = nn.Conv2d(C, C, (1, 3), padding=(0, d), dilation=d)
    return ca.to(DEV), cb.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_first_bias_gradient_comes_from_the_second_convolutions_launch(dtype):
    """A pair as the EDABlock runs it (no BatchNorm behind it here, so both biases are added by
    the kernel).  The first convolution's bias gradient is the column sum of the gradient with
    respect to `mid` AS STORED, folded from the statistics rows of the launch that produced it."""
    F = L._F()
    N, H, W, d = 2, 9, 11, 2
    ca, cb = _pair_modules(d, 3)
    x = to_dev_nhwc(quant(rnd((N, C, H, W), 31), dtype), dtype).requires_grad_(True)
    lb = F.LineBias()
    mid = F.line_conv_bn(F.Act(x), ca, None, bias_grad=lb).t
    seen = {}
    mid.register_hook(lambda g: seen.setdefault("dmid", g.detach().clone()))
    y = F.line_conv_bn(F.Act(mid), cb, None, mid_of=lb).t
    dy = to_dev_nhwc(quant(rnd((N, C, H, W), 32), dtype), dtype)
    y.backward(dy)
    assert lb.partial is None  # taken
    dmid = seen["dmid"].double()
    want, mag = dmid.sum((0, 1, 2)), dmid.abs().sum((0, 1, 2))
    assert ((ca.bias.grad.double() - want).abs() <= N * H * W * 2.0 ** -23 * mag).all()
    dyd = dy.double()
    assert ((cb.bias.grad.double() - dyd.sum((0, 1, 2))).abs()
            <= N * H * W * 2.0 ** -23 * dyd.abs().sum((0, 1, 2))).all()
    assert x.grad is not None and ca.weight.grad is not None and cb.weight.grad is not None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bias_in_front_of_a_training_batchnorm_is_dropped(dtype):
    """As conv_bn's drop_bias: the stored tensor is the bias-free convolution, the bias enters the
    running mean, and its gradient is an exact zero tensor, not None."""
    F, K = L._F(), L._K()
    N, H, W, d = 2, 9, 11, 1
    _, cb = _pair_modules(d, 5)
    bn = nn.BatchNorm2d(C).to(DEV).train()
    x = to_dev_nhwc(quant(rnd((N, C, H, W), 41), dtype), dtype).requires_grad_(True)
    a = F.line_conv_bn(F.Act(x), cb, bn)
    bare, _ = K.conv_line_bias(x.detach(), F.pack_conv_weight(cb.weight.detach(), C, dtype), None,
                               W_, d)
    assert torch.equal(a.t.detach(), bare)
    mean = bare.double().mean((0, 1, 2)) + cb.bias.detach().double()
    assert ((bn.running_mean.double() - 0.1 * mean).abs() <= 1e-5 * (1 + mean.abs())).all()
    out = F.materialize(F.Act(a.t, a.bn, True))
    out.backward(to_dev_nhwc(quant(rnd((N, C, H, W), 42), dtype), dtype))
    assert cb.bias.grad is not None and cb.bias.grad.dtype == torch.float32
    assert tuple(cb.bias.grad.shape) == (C,) and not cb.bias.grad.any()
    assert torch.isfinite(cb.weight.grad).all() and torch.isfinite(x.grad).all()


def test_host_queries_serve_40_and_still_refuse_the_rest():
    """C = 40 belongs to the bias entries and the weight gradient; the entries that existed before
    (seg_conv_line_ok / _geom / _fwd) keep their classes."""
    K = L._K()
    for dt in DTYPES:
        assert K.conv_line_bias_ok(dt, 40, 0, 16) and K.conv_line_bias_ok(dt, 40, 1, 1)
        assert K.conv_line_bias_ok(dt, 16, 0, 17) and K.conv_line_bias_ok(dt, 64, 1, 1)
        assert not K.conv_line_bias_ok(dt, 24, 0, 1) and not K.conv_line_bias_ok(dt, 48, 0, 1)
        assert not K.conv_line_bias_ok(dt, 40, 2, 1) and not K.conv_line_bias_ok(dt, 40, 0, 0)
        assert not K.conv_line_ok(dt, 40, 0, 1) and K.conv_line_ok(dt, 32, 0, 1)
        geo = K.conv_line_geom(dt, 2, 7, 40, 40)
        assert geo["tile"] == 128 and geo["grid"] == 5
        assert K.conv_line_geom(dt, 2, 7, 40, 32)["grid"] == K.LIB.query(
            "seg_conv_line_geom", K._DT[dt], 2, 7, 40, 32, 1) == 5
    x = torch.zeros((1, 4, 4, 40), dtype=torch.float32, device=DEV)
    wp = torch.zeros((40, 120), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):  # the entry without a bias does not take the class
        K.conv_line(x, wp, 0, 1)
    with pytest.raises(AssertionError):  # the bias is float32 [C]
        K.conv_line_bias(x, wp, torch.zeros(40, dtype=torch.bfloat16, device=DEV), 0, 1)
