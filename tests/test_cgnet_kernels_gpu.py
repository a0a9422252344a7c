"""GPU: the kernels of csrc/cgnet.hip against torch float64 on the CPU — the joint local /
surround depthwise forward (and functional.cg_joint_bn on both of its routes with the backward
they share), BatchNorm + PReLU with its pooled sums, the PReLU backward, and the moments pass of
the stage concats.  Bars: _util.assert_close / tol(dtype) for
what is stored in the activation dtype; float32 sums (statistics, pooled sums, weight gradients,
dalpha) against float64 at tol(float32) of the sum of the magnitudes that were added."""
import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _K():
    from segmentron_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------- joint depthwise
JOINT_HW = [(1, 1), (3, 5), (9, 7), (33, 65), (24, 40)]


def _joint_inputs(N, H, W, C, dtype, seed):
    """-> x (device NHWC view: C == 72 sits at channel 8 of a NaN-filled buffer), its CPU NCHW
    float copy (rounded to dtype), both weights."""
    x = quant(rnd((N, C, H, W), seed), dtype)
    wl, ws = rnd((C, 1, 3, 3), seed + 1, 0.4), rnd((C, 1, 3, 3), seed + 2, 0.4)
    xd = to_dev_nhwc(x, dtype, pitch=C + 16, off=8) if C == 72 else to_dev_nhwc(x, dtype)
    return xd, x, wl, ws


def _joint_ref(x, wl, ws, d):
    C = x.shape[1]
    x, wl, ws = x.double(), wl.double(), ws.double()
    return torch.cat([TF.conv2d(x, wl, None, 1, 1, 1, C), TF.conv2d(x, ws, None, 1, d, d, C)], 1)


def _sum_close(got, ref, mag, what):
    """float32 sums against float64: within tol(float32) of the summed magnitudes."""
    got, ref, mag = got.double().cpu(), ref.double(), mag.double()
    assert torch.isfinite(got).all(), what
    err = ((got - ref).abs() / mag.clamp_min(1e-30)).max().item()
    assert err <= tol(torch.float32), "%s: %.3e of the summed magnitudes" % (what, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 32, 64, 72])
@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("hw", JOINT_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 3])
def test_joint_forward(N, hw, d, C, dtype):
    K = _K()
    H, W = hw
    xd, x, wl, ws = _joint_inputs(N, H, W, C, dtype, 1)
    out = None
    if C == 72:  # the 2C-wide output too is a slice at channel 8 of a NaN-filled buffer
        obuf = torch.full((N, H, W, 2 * C + 16), float("nan"), dtype=dtype, device=DEV)
        out = obuf[..., 8:8 + 2 * C]
    y, partial = K.cg_joint(xd, wl.to(DEV), ws.to(DEV), d, out=out)
    ref = _joint_ref(x, wl, ws, d)
    assert_close(to_cpu_nchw(y), ref, dtype, "joi")
    if C == 72:
        assert torch.isnan(obuf[..., :8]).all() and torch.isnan(obuf[..., 8 + 2 * C:]).all()
        assert torch.isnan(xd._base[..., :8]).all() and torch.isnan(xd._base[..., 8 + C:]).all()
    # statistics partials [rows, 2, 2C]: sum | sum of squares of the fp32 accumulators
    assert partial.dtype == torch.float32 and tuple(partial.shape[1:]) == (2, 2 * C)
    sums = partial.double().sum(0).cpu()
    _sum_close(sums[0], ref.sum((0, 2, 3)), ref.abs().sum((0, 2, 3)), "sum")
    _sum_close(sums[1], (ref * ref).sum((0, 2, 3)), (ref * ref).sum((0, 2, 3)), "sum of squares")
    # a second run gives the same bits
    y2, partial2 = K.cg_joint(xd, wl.to(DEV), ws.to(DEV), d)
    assert torch.equal(y2, y) and torch.equal(partial2, partial)
    if N == 3:  # one image at 1e30 leaves the other images' outputs and partial rows bit-equal
        xb = xd.clone()
        xb[1] = 1e30
        y3, partial3 = K.cg_joint(xb, wl.to(DEV), ws.to(DEV), d)
        rows = partial.view(-1, N, 2, 2 * C)
        rows3 = partial3.view(-1, N, 2, 2 * C)
        for n in (0, 2):
            assert torch.equal(y3[n], y[n]) and torch.equal(rows3[:, n], rows[:, n])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [2, 4])
def test_cg_joint_bn_forward_and_backward(d, dtype):
    """functional.cg_joint_bn on both routes (dilation 2: the two depthwise launches; dilation 4:
    the joint kernel) with the backward both share — raw output, BatchNorm statistics, input
    gradient and both weight gradients against float64."""
    import torch.nn as nn
    from segmentron_amd import functional as F
    N, H, W, C = 2, 24, 40, 32
    assert F.cg_joint_routed(dtype, C, d) == (d == 4)
    xd, x, wl, ws = _joint_inputs(N, H, W, C, dtype, 71)
    f_loc = nn.Conv2d(C, C, 3, 1, 1, 1, groups=C, bias=False).to(DEV)
    f_sur = nn.Conv2d(C, C, 3, 1, d, d, groups=C, bias=False).to(DEV)
    bn = nn.BatchNorm2d(2 * C, momentum=1.0).to(DEV).train()
    with torch.no_grad():
        f_loc.weight.copy_(wl)
        f_sur.weight.copy_(ws)
    xd = xd.clone().requires_grad_()
    act = F.cg_joint_bn(xd, f_loc, f_sur, bn)
    ref = _joint_ref(x, wl, ws, d)
    assert_close(to_cpu_nchw(act.t), ref, dtype, "joi")
    assert act.bn is not None and not act.relu
    _sum_close(bn.running_mean, ref.mean((0, 2, 3)), ref.abs().mean((0, 2, 3)), "batch mean")
    # (the variance is a difference of float32 sums: within tol(float32) of E[x^2])
    _sum_close(bn.running_var, ref.var((0, 2, 3)), (ref * ref).mean((0, 2, 3)), "batch variance")
    g = quant(rnd((N, 2 * C, H, W), 73), dtype)
    act.t.backward(to_dev_nhwc(g, dtype))
    xo = x.double().requires_grad_()
    wlo, wso = wl.double().requires_grad_(), ws.double().requires_grad_()
    yo = torch.cat([TF.conv2d(xo, wlo, None, 1, 1, 1, C), TF.conv2d(xo, wso, None, 1, d, d, C)], 1)
    yo.backward(g.double())
    # (two roundings in bf16: the surround gradient is stored before it joins the local one)
    assert_close(to_cpu_nchw(xd.grad), xo.grad, dtype, "dx", fac=1.0 if dtype == torch.float32 else 2.0)
    xa, ga = x.double().abs(), g.double().abs()
    ones = torch.ones(C, 1, 3, 3, dtype=torch.float64)
    for conv, refg, gpart, dil in ((f_loc, wlo.grad, ga[:, :C], 1), (f_sur, wso.grad, ga[:, C:], d)):
        mag = torch.autograd.grad(TF.conv2d(xa, ones.requires_grad_(), None, 1, dil, dil, C),
                                  ones, gpart)[0]
        assert tuple(conv.weight.grad.shape) == (C, 1, 3, 3)
        _sum_close(conv.weight.grad, refg, mag, "dW (dilation %d)" % dil)


# ------------------------------------------------------------------------------- BN + PReLU
PRELU_HW = [(1, 1), (7, 9), (33, 65), (48, 48)]
PITCH = {35: 48, 131: 144}  # the ragged counts sit in NaN-filled buffers of this pitch


def _up8(C):
    return (C + 7) // 8 * 8


def _nan_buffer(t_nchw, dtype, C):
    """CPU NCHW float -> device NHWC view of C channels: ragged C at the head of a NaN-filled
    buffer of pitch 48 / 144 (-> the view, the buffer), else a dense tensor (-> it, None)."""
    if C not in PITCH:
        return to_dev_nhwc(t_nchw, dtype), None
    v = to_dev_nhwc(t_nchw, dtype, pitch=PITCH[C], off=0)
    return _ragged_view(v._base, C), v._base


def _ragged_view(buf, C):
    """The C channels of a ragged tensor at the head of its buffer; a single row (which has no
    pitch to show the room behind it) is passed as the rounded width, NaN pads included."""
    rows = buf.shape[0] * buf.shape[1] * buf.shape[2]
    return buf[..., :C] if rows > 1 else buf[..., :_up8(C)]


def _prelu_case(N, H, W, C, dtype, affine, seed):
    x = quant(rnd((N, C, H, W), seed), dtype)
    alpha = rnd((C,), seed + 1, 0.5)
    alpha[0], alpha[1], alpha[2] = 0.0, -0.3, 1.7  # zero, negative, above one
    scale = shift = None
    if affine:
        scale = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 2))
        scale[::3] *= -1.0
        shift = rnd((C,), seed + 3, 0.5)
        # exact zeros of z: a power-of-two scale makes scale * x exact, shift = -scale * x
        scale[3], scale[4] = 0.5, -2.0
        shift[3], shift[4] = -0.5 * x[0, 3, 0, 0], 2.0 * x[N - 1, 4, H - 1, W - 1]
    else:
        x[0, 3, 0, 0] = 0.0
        x[N - 1, 4, H - 1, W - 1] = 0.0
    z = x.double()
    if affine:
        z = z * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)
    assert z[0, 3, 0, 0] == 0 and z[N - 1, 4, H - 1, W - 1] == 0
    return x, alpha, scale, shift, z


def _dev(t):
    return None if t is None else t.to(DEV)


def _check_pads(buf, C, what):
    """finite zeros in channels [C, round_up(C, 8)), the NaNs beyond untouched"""
    if buf is None:
        return
    pad = buf[..., C:_up8(C)]
    assert torch.isfinite(pad).all() and (pad == 0).all(), what + ": pad channels"
    assert torch.isnan(buf[..., _up8(C):]).all(), what + ": wrote beyond the rounded width"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("C", [8, 35, 128, 131])
@pytest.mark.parametrize("hw", PRELU_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 3])
def test_bn_prelu_forward(N, hw, C, affine, dtype):
    K = _K()
    H, W = hw
    x, alpha, scale, shift, z = _prelu_case(N, H, W, C, dtype, affine, 21)
    xd, _ = _nan_buffer(x, dtype, C)
    ref = torch.where(z > 0, z, alpha.double().view(1, C, 1, 1) * z)

    def run(want_y, pool):
        out = obuf = None
        if want_y and C in PITCH:
            obuf = torch.full((N, H, W, PITCH[C]), float("nan"), dtype=dtype, device=DEV)
            out = _ragged_view(obuf, C)
        y, sums = K.bn_prelu(xd, _dev(alpha), _dev(scale), _dev(shift), want_y=want_y, pool=pool,
                             out=out)
        return y, sums, obuf

    y, sums, obuf = run(True, True)
    assert_close(to_cpu_nchw(y[..., :C]), ref, dtype, "y")
    _check_pads(obuf, C, "y")
    if C not in PITCH:
        assert y.shape[-1] == C
    # per-image channel sums of the fp32 activated values
    assert tuple(sums.shape) == (N, C) and sums.dtype == torch.float32
    _sum_close(sums, ref.sum((2, 3)), ref.abs().sum((2, 3)), "pooled sums")
    # without the pool: the same y; the pool alone: the same sums, bit for bit
    y1, s1, obuf1 = run(True, False)
    assert s1 is None and torch.equal(y1[..., :C], y[..., :C])
    _check_pads(obuf1, C, "y (no pool)")
    y2, s2, _ = run(False, True)
    assert y2 is None and torch.equal(s2, sums)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("C", [8, 35, 128, 131])
@pytest.mark.parametrize("hw", PRELU_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 3])
def test_prelu_backward(N, hw, C, affine, dtype):
    K = _K()
    H, W = hw
    x, alpha, scale, shift, z = _prelu_case(N, H, W, C, dtype, affine, 33)
    xd, _ = _nan_buffer(x, dtype, C)
    gy = quant(rnd((N, C, H, W), 41), dtype)
    gyd, _ = _nan_buffer(gy, dtype, C)  # (ragged: NaNs behind the C channels of the gradient too)
    gp = rnd((N, C), 43)
    a4 = alpha.double().view(1, C, 1, 1)
    for pooled in (True, False):
        g = gy.double() + (gp.double().view(N, C, 1, 1) / (H * W) if pooled else 0.0)
        ref = torch.where(z > 0, g, a4 * g)          # at z == 0 the slope is alpha, as in torch
        neg = (z <= 0).double()
        dalpha_ref = (g * z * neg).sum((0, 2, 3))
        out = obuf = None
        if C in PITCH:
            obuf = torch.full((N, H, W, PITCH[C]), float("nan"), dtype=dtype, device=DEV)
            out = _ragged_view(obuf, C)
        gz, dalpha = K.prelu_bwd(gyd, _dev(gp) if pooled else None, xd, _dev(alpha), _dev(scale),
                                 _dev(shift), out=out)
        assert_close(to_cpu_nchw(gz[..., :C]), ref, dtype, "g_z (pool %s)" % pooled)
        _check_pads(obuf, C, "g_z")
        assert tuple(dalpha.shape) == (C,) and dalpha.dtype == torch.float32
        mag = (g * z * neg).abs().sum((0, 2, 3))
        _sum_close(dalpha, dalpha_ref, mag, "dalpha (pool %s)" % pooled)
        gz2, dalpha2 = K.prelu_bwd(gyd, _dev(gp) if pooled else None, xd, _dev(alpha), _dev(scale),
                                   _dev(shift))
        assert torch.equal(gz2[..., :C], gz[..., :C]) and torch.equal(dalpha2, dalpha)
    # the pooled gradient alone (nothing reached y)
    gz, _ = K.prelu_bwd(None, _dev(gp), xd, _dev(alpha), _dev(scale), _dev(shift))
    g = (gp.double().view(N, C, 1, 1) / (H * W)).expand(N, C, H, W)
    assert_close(to_cpu_nchw(gz[..., :C]), torch.where(z > 0, g, a4 * g), dtype, "g_z (pool only)")


def test_prelu_backward_matches_torch_autograd_at_zero():
    """The z == 0 rule is torch's: autograd of TF.prelu on the same inputs, float64."""
    K = _K()
    N, H, W, C = 1, 7, 9, 8
    x, alpha, _, _, z = _prelu_case(N, H, W, C, torch.float32, False, 51)
    gy = rnd((N, C, H, W), 53)
    xo, ao = x.double().requires_grad_(), alpha.double().requires_grad_()
    TF.prelu(xo, ao).backward(gy.double())
    gz, dalpha = K.prelu_bwd(to_dev_nhwc(gy, torch.float32), None, to_dev_nhwc(x, torch.float32),
                             alpha.to(DEV))
    assert_close(to_cpu_nchw(gz), xo.grad, torch.float32, "g_z")
    assert_close(dalpha.cpu(), ao.grad, torch.float32, "dalpha")
    assert gz[0, 0, 0, 3].item() == (alpha[3] * gy[0, 3, 0, 0]).item()  # (float32 product)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 35, 128, 131])
@pytest.mark.parametrize("hw", PRELU_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 3])
def test_moments_of_a_plain_tensor(N, hw, C, dtype):
    """hip_ops.chan_moments at the buffer's width (ragged C: zeros in the pad channels, cut back
    to C afterwards, as functional.bn_of_concat does)."""
    K = _K()
    H, W = hw
    x = quant(rnd((N, C, H, W), 61) + 0.5, dtype)
    buf = torch.zeros((N, H, W, _up8(C)), dtype=dtype, device=DEV)
    buf[..., :C] = x.permute(0, 2, 3, 1).to(dtype).to(DEV)
    partial = K.chan_moments(buf)
    assert partial.dtype == torch.float32 and tuple(partial.shape[1:]) == (2, _up8(C))
    sums = partial.double().sum(0).cpu()
    xd = x.double()
    _sum_close(sums[0, :C], xd.sum((0, 2, 3)), xd.abs().sum((0, 2, 3)), "sum")
    _sum_close(sums[1, :C], (xd * xd).sum((0, 2, 3)), (xd * xd).sum((0, 2, 3)), "sum of squares")
    assert (sums[:, C:] == 0).all()
