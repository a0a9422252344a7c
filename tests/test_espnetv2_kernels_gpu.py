"""GPU: the kernels of csrc/espnetv2.hip and the grouped 1x1 route against torch float64 on the
CPU — the EESP depthwise pyramid (the joint kernel, and functional.eesp_pyramid on both of its
routes with the suffix-sum backward they share), the 3x3 / stride-2 average pool, BatchNorm + add +
PReLU, and conv_bn with groups=4 through the block-diagonal packing.  Bars: _util.assert_close /
tol(dtype) for what is stored in the activation dtype; float32 sums (statistics, weight gradients,
dalpha, dgamma, dbeta) against float64 at tol(float32) of the sum of the magnitudes that were
added.  Where a route stores bf16 intermediates before a sum or a store, `fac` is the number of
roundings on that route and the error is taken relative to the magnitudes that were added."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _K():
    from segmentron_amd import hip_ops
    return hip_ops


def _F():
    from segmentron_amd import functional
    return functional


def _sum_close(got, ref, mag, what, rel=None):
    """float32 sums against float64: within `rel` (default tol(float32)) of the summed magnitudes."""
    rel = tol(torch.float32) if rel is None else rel
    got, ref, mag = got.double().cpu(), ref.double(), mag.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = ((got - ref).abs() / mag.clamp_min(1e-30)).max().item()
    print("%s: %.3e of the summed magnitudes (bar %.3e)" % (what, err, rel))
    assert err <= rel, "%s: %.3e of the summed magnitudes" % (what, err)


# ------------------------------------------------------------------------------- pyramid forward
PYR_HW = [(1, 1), (2, 2), (3, 5), (9, 7), (8, 12), (33, 65)]
PYR_DILS = [(1, 2, 3, 4), (1, 1, 2, 3), (1, 1, 1, 2)]
SLICED_N = 16  # this width runs as slices at channel 8 of NaN-filled wider buffers


def _pyr_inputs(N, H, W, n, dtype, seed):
    x = quant(rnd((N, n, H, W), seed), dtype)
    ws = [rnd((n, 1, 3, 3), seed + 1 + j, 0.4) for j in range(4)]
    xd = to_dev_nhwc(x, dtype, pitch=n + 16, off=8) if n == SLICED_N else to_dev_nhwc(x, dtype)
    return xd, x, ws


def _pyr_branches(x, ws, dils, s):
    n = x.shape[1]
    return [TF.conv2d(x.double(), w.double(), None, s, d, d, n) for w, d in zip(ws, dils)]


def _pyr_ref(x, ws, dils, s):
    """-> (the fused concat, the magnitudes that were added to form each element)"""
    outs, mags = [], []
    for b in _pyr_branches(x, ws, dils, s):
        outs.append(b if not outs else b + outs[-1])
        mags.append(b.abs() if not mags else b.abs() + mags[-1])
    return torch.cat(outs, 1), torch.cat(mags, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [8, 16, 32, 64])
@pytest.mark.parametrize("dils", PYR_DILS, ids=lambda v: "d" + "".join(map(str, v)))
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", PYR_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 3])
def test_pyramid_forward(N, hw, stride, dils, n, dtype):
    K = _K()
    H, W = hw
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xd, x, ws = _pyr_inputs(N, H, W, n, dtype, 1)
    wd = [w.to(DEV) for w in ws]
    out = obuf = None
    if n == SLICED_N:
        obuf = torch.full((N, Ho, Wo, 4 * n + 16), float("nan"), dtype=dtype, device=DEV)
        out = obuf[..., 8:8 + 4 * n]
    y, partial = K.eesp_pyramid(xd, wd, dils, stride, out=out)
    ref, mag = _pyr_ref(x, ws, dils, stride)
    assert tuple(y.shape) == (N, Ho, Wo, 4 * n)
    assert_close(to_cpu_nchw(y), ref, dtype, "pyramid")  # fp32 sums, one rounding
    if n == SLICED_N:
        assert torch.isnan(obuf[..., :8]).all() and torch.isnan(obuf[..., 8 + 4 * n:]).all()
        assert torch.isnan(xd._base[..., :8]).all() and torch.isnan(xd._base[..., 8 + n:]).all()
    # statistics partials [rows, 2, 4n]: sum | sum of squares of the fp32 values
    assert partial.dtype == torch.float32 and tuple(partial.shape[1:]) == (2, 4 * n)
    sums = partial.double().sum(0).cpu()
    # (the magnitudes that were added: a fused slice is itself a sum of up to four branches)
    _sum_close(sums[0], ref.sum((0, 2, 3)), mag.sum((0, 2, 3)), "sum")
    _sum_close(sums[1], (ref * ref).sum((0, 2, 3)), (mag * mag).sum((0, 2, 3)), "sum of squares")
    # without the statistics: the same y; a second run gives the same bits
    y1, p1 = K.eesp_pyramid(xd, wd, dils, stride, want_stats=False)
    assert p1 is None and torch.equal(y1, y)
    y2, partial2 = K.eesp_pyramid(xd, wd, dils, stride)
    assert torch.equal(y2, y) and torch.equal(partial2, partial)
    if N == 3:  # one image at 1e30 leaves the other images' outputs and partial rows bit-equal
        xb = xd.clone()
        xb[1] = 1e30
        y3, partial3 = K.eesp_pyramid(xb, wd, dils, stride)
        rows = partial.view(-1, N, 2, 4 * n)
        rows3 = partial3.view(-1, N, 2, 4 * n)
        for i in (0, 2):
            assert torch.equal(y3[i], y[i]) and torch.equal(rows3[:, i], rows[:, i])


@pytest.mark.parametrize("n,dils,stride", [(12, (1, 2, 3, 4), 1), (8, (1, 2, 3, 5), 1),
                                           (8, (1, 3, 2, 4), 1), (8, (0, 1, 2, 3), 2),
                                           (8, (1, 2, 3, 4), 3)],
                         ids=["n12", "dil5", "decreasing", "dil0", "stride3"])
def test_pyramid_rejects_what_is_outside_its_contract(n, dils, stride):
    K = _K()
    N, H, W = 1, 6, 6
    xd = to_dev_nhwc(rnd((N, n, H, W), 3), torch.float32)
    wd = [rnd((n, 1, 3, 3), 4 + j).to(DEV) for j in range(4)]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.full((N, Ho, Wo, 4 * n), float("nan"), device=DEV)
    with pytest.raises(RuntimeError, match="eesp_pyr_fwd"):
        K.eesp_pyramid(xd, wd, dils, stride, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert not _F().eesp_pyramid_in_contract(n, dils, stride)


# ---------------------------------------------------------- functional.eesp_pyramid, both routes
EESP_CASES = [((2, 24, 40, 32), 1), ((2, 25, 41, 16), 2)]


def _spp(n, ws, dils, stride):
    convs = nn.ModuleList([nn.Conv2d(n, n, 3, stride, d, d, groups=n, bias=False) for d in dils])
    with torch.no_grad():
        for c, w in zip(convs, ws):
            c.weight.copy_(w)
    return convs.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("joint", [True, False], ids=["joint", "per_branch"])
@pytest.mark.parametrize("case", EESP_CASES, ids=["s1", "s2"])
def test_eesp_pyramid_forward_and_backward(case, joint, dtype, monkeypatch):
    """functional.eesp_pyramid on both routes (forced through the routing function) with the
    suffix-sum backward both share: raw output, BatchNorm statistics, input gradient and the four
    weight gradients against float64."""
    F = _F()
    (N, H, W, n), stride = case
    dils = (1, 2, 3, 4)
    bf16 = dtype == torch.bfloat16
    monkeypatch.setattr(F, "eesp_pyramid_routed", lambda *a: joint)
    x = quant(rnd((N, n, H, W), 71), dtype)
    ws = [rnd((n, 1, 3, 3), 72 + j, 0.4) for j in range(4)]
    convs = _spp(n, ws, dils, stride)
    bn = nn.BatchNorm2d(4 * n, momentum=1.0).to(DEV).train()
    xd = to_dev_nhwc(x, dtype).requires_grad_()
    calls = []
    real = F.K.eesp_pyramid
    monkeypatch.setattr(F.K, "eesp_pyramid", lambda *a, **k: calls.append(1) or real(*a, **k))
    act = F.eesp_pyramid(xd, list(convs), bn)
    assert len(calls) == (1 if joint else 0)
    ref, mag = _pyr_ref(x, ws, dils, stride)
    # joint: one rounding.  per branch, bf16: slice j adds a rounded branch to the rounded slice
    # before it and rounds again, 2 j + 1 <= 7 roundings of magnitudes within `mag`
    fac = 7.0 if bf16 and not joint else 1.0
    assert_close(to_cpu_nchw(act.t), ref, dtype, "pyramid", scale=mag.max().item(), fac=fac)
    assert act.bn is not None and not act.relu
    # joint: statistics of the fp32 values — unless the BatchNorm sees at most SMALL_BN_ROWS rows
    # (the stride-2 case: 546), where finish_bn takes them two-pass from the stored tensor: one
    # rounding; per branch: of the stored values, `fac` roundings
    small = ref.shape[0] * ref.shape[2] * ref.shape[3] <= F.K.SMALL_BN_ROWS
    assert small == (stride == 2)
    rel = tol(torch.float32)
    if bf16 and (small or not joint):
        rel = tol(dtype) * fac
    _sum_close(bn.running_mean, ref.mean((0, 2, 3)), mag.mean((0, 2, 3)), "batch mean", rel)
    # (a square carries twice the relative error of its root)
    _sum_close(bn.running_var, ref.var((0, 2, 3)), (mag * mag).mean((0, 2, 3)), "batch variance",
               2 * rel)
    g = quant(rnd(tuple(ref.shape), 79), dtype)
    act.t.backward(to_dev_nhwc(g, dtype))
    # float64: the branches see the suffix sums of the gradient's slices
    gd = g.double()
    S = [sum(gd[:, i * n:(i + 1) * n] for i in range(j, 4)) for j in range(4)]
    xo = x.double().requires_grad_()
    wo = [w.double().requires_grad_() for w in ws]
    _pyr_ref(xo, wo, dils, stride)[0].backward(gd)
    xa = x.double().abs()
    dx_mag = torch.zeros_like(xa)
    for j, d in enumerate(dils):
        xr = xa.clone().requires_grad_()
        TF.conv2d(xr, wo[j].detach().abs(), None, stride, d, d, n).backward(S[j].abs())
        dx_mag += xr.grad
    # bf16: S_j is stored, each branch's data gradient is stored, their sum is stored: 3 roundings
    assert_close(to_cpu_nchw(xd.grad), xo.grad, dtype, "dx", scale=dx_mag.max().item(),
                 fac=3.0 if bf16 else 1.0)
    ones = torch.ones(n, 1, 3, 3, dtype=torch.float64)
    for j, d in enumerate(dils):
        o = ones.clone().requires_grad_()
        TF.conv2d(xa, o, None, stride, d, d, n).backward(S[j].abs())
        assert tuple(convs[j].weight.grad.shape) == (n, 1, 3, 3)
        # bf16: S_j is rounded once before it enters the float32 sums
        _sum_close(convs[j].weight.grad, wo[j].grad, o.grad, "dW %d" % j,
                   tol(dtype) if bf16 else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 24, 40, 32), (2, 13, 21, 16)], ids=["s1", "s2"])
def test_suffix_sum(shape, dtype):
    K = _K()
    N, H, W, n = shape
    g = quant(rnd((N, 4 * n, H, W), 81), dtype)
    gd = to_dev_nhwc(g, dtype, pitch=4 * n + 16, off=8)
    S = K.eesp_suffix_sum(gd)
    d = g.double()
    ref = torch.cat([sum(d[:, i * n:(i + 1) * n] for i in range(j, 4)) for j in range(4)], 1)
    assert_close(to_cpu_nchw(S), ref, dtype, "suffix sums")
    assert torch.isnan(gd._base[..., :8]).all() and torch.isnan(gd._base[..., 8 + 4 * n:]).all()
    assert torch.equal(K.eesp_suffix_sum(gd), S)
    g2 = gd.clone()
    assert torch.equal(K.eesp_suffix_sum(g2, out=g2), S)  # in place


# ------------------------------------------------------------------------------- average pool
POOL_HW = [(1, 1), (2, 3), (8, 12), (33, 65)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [8, 128])
@pytest.mark.parametrize("hw", POOL_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 2])
def test_avgpool3x3s2(N, hw, C, dtype):
    K = _K()
    H, W = hw
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = quant(rnd((N, C, H, W), 91) + 1.0, dtype)  # (a mean of 1: a border divided by 9 shows)
    sliced = C == 8
    xd = to_dev_nhwc(x, dtype, pitch=C + 16, off=8) if sliced else to_dev_nhwc(x, dtype)
    out = obuf = None
    if sliced:
        obuf = torch.full((N, Ho, Wo, C + 16), float("nan"), dtype=dtype, device=DEV)
        out = obuf[..., 8:8 + C]
    y = K.avgpool3x3s2(xd, out=out)
    xo = x.double().requires_grad_()
    ref = TF.avg_pool2d(xo, 3, 2, 1)  # count_include_pad: the divisor is 9 at the borders too
    assert tuple(y.shape) == (N, Ho, Wo, C)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "avg pool")
    if sliced:
        assert torch.isnan(obuf[..., :8]).all() and torch.isnan(obuf[..., 8 + C:]).all()
    g = quant(rnd((N, C, Ho, Wo), 93), dtype)
    ref.backward(g.double())
    gd = to_dev_nhwc(g, dtype, pitch=C + 16, off=8) if sliced else to_dev_nhwc(g, dtype)
    gx = K.avgpool3x3s2_bwd(gd, (H, W))
    assert_close(to_cpu_nchw(gx), xo.grad, dtype, "avg pool backward")
    assert torch.equal(K.avgpool3x3s2_bwd(gd, (H, W)), gx)
    # through autograd
    xg = xd.detach().clone().requires_grad_()
    _F().avg_pool3x3s2(xg).backward(gd)
    assert torch.equal(xg.grad, gx)


# ------------------------------------------------------------------------------- BN + add + PReLU
ADD_CASES = ["both_bn", "b_plain", "padded_concat", "a_plain"]


def _away_from_kink(make_z, a, dtype, what):
    """Move the entries of `a` whose PReLU input lies within 1e-4 of zero (the mask of such an
    element is not decided by float32 arithmetic) until none is left."""
    for _ in range(8):
        bad = make_z(a).abs() < 1e-4
        if not bad.any():
            return a
        a = quant(torch.where(bad, a + 0.0625, a), dtype)
    raise AssertionError(what + ": PReLU inputs stay at the kink")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ADD_CASES)
@pytest.mark.parametrize("shape", [(2, 24, 40, 32), (2, 24, 40, 64), (2, 12, 20, 32)],
                         ids=["c32", "c64", "few_rows"])
def test_bn_add_prelu(shape, case, dtype):
    """functional.bn_add_prelu: y, both input gradients, dalpha, dgamma and dbeta of each
    BatchNorm against float64 autograd.  (2, 12, 20, 32) has 480 <= SMALL_BN_ROWS rows: the
    few-sample BatchNorm paths."""
    F = _F()
    N, H, W, C = shape
    bf16 = dtype == torch.bfloat16
    lead = C // 4 if case == "padded_concat" else 0
    bn_on_a, bn_on_b = case != "a_plain", case != "b_plain"
    b = quant(rnd((N, C, H, W), 102, 0.7) - 0.2, dtype)
    alpha = rnd((C,), 103, 0.5)
    alpha[0], alpha[1], alpha[2] = 0.0, -0.3, 1.7  # zero, negative, above one
    wa, ba_ = 0.5 + torch.rand(C - lead, generator=torch.Generator().manual_seed(104)), \
        rnd((C - lead,), 105, 0.3)
    wb, bb_ = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(106)), rnd((C,), 107, 0.3)
    wa[::3] *= -1.0

    def ref_z(a, a_par=(wa.double(), ba_.double()), b_par=(wb.double(), bb_.double()), bt=None):
        a, bt = a.double(), (b.double() if bt is None else bt)
        za = a
        if bn_on_a:
            tail = TF.batch_norm(a[:, lead:], None, None, a_par[0], a_par[1], True, 0.0, 1e-5)
            za = torch.cat([a[:, :lead], tail], 1)
        zb = TF.batch_norm(bt, None, None, b_par[0], b_par[1], True, 0.0, 1e-5) if bn_on_b else bt
        return za + zb

    a = _away_from_kink(ref_z, quant(rnd((N, C, H, W), 101) + 0.3, dtype), dtype, case)
    # device
    ad, bd = to_dev_nhwc(a, dtype).requires_grad_(), to_dev_nhwc(b, dtype).requires_grad_()
    bn_a = nn.BatchNorm2d(C - lead).to(DEV).train()
    bn_b = nn.BatchNorm2d(C).to(DEV).train()
    prelu = nn.PReLU(C).to(DEV)
    with torch.no_grad():
        bn_a.weight.copy_(wa); bn_a.bias.copy_(ba_)
        bn_b.weight.copy_(wb); bn_b.bias.copy_(bb_)
        prelu.weight.copy_(alpha)
    act_a = F.Act(ad, F.bn_of_concat(ad[..., lead:], bn_a).bn) if bn_on_a else F.Act(ad)
    act_b = F.bn_of_concat(bd, bn_b) if bn_on_b else F.Act(bd)
    y = F.bn_add_prelu(act_a, act_b, prelu, lead=lead)
    g = quant(rnd((N, C, H, W), 108), dtype)
    y.backward(to_dev_nhwc(g, dtype))
    # float64
    ao, bo, al = a.double().requires_grad_(), b.double().requires_grad_(), \
        alpha.double().requires_grad_()
    pa = (wa.double().requires_grad_(), ba_.double().requires_grad_())
    pb = (wb.double().requires_grad_(), bb_.double().requires_grad_())
    z = ref_z(ao, pa, pb, bo)
    assert z.detach().abs().min() >= 1e-4
    yo = TF.prelu(z, al)
    yo.backward(g.double())
    assert_close(to_cpu_nchw(y), yo.detach(), dtype, "y")
    # bf16: g_z is stored, then the BatchNorm backward stores dx: 2 roundings (a plain operand: 1)
    assert_close(to_cpu_nchw(ad.grad), ao.grad, dtype, "da", fac=2.0 if bf16 else 1.0)
    assert_close(to_cpu_nchw(bd.grad), bo.grad, dtype, "db", fac=2.0 if bf16 else 1.0)
    zd, gd = z.detach(), g.double()
    neg = (zd <= 0).double()
    _sum_close(prelu.weight.grad, al.grad, (gd * zd * neg).abs().sum((0, 2, 3)), "dalpha")
    # dgamma = sum g_z * xhat, dbeta = sum g_z; bf16: g_z is rounded once before the float32 sums
    gz = torch.where(zd > 0, gd, alpha.double().view(1, C, 1, 1) * gd)
    rel = tol(dtype) if bf16 else None
    for on, bn, par, t, lo in ((bn_on_a, bn_a, pa, a, lead), (bn_on_b, bn_b, pb, b, 0)):
        if not on:
            continue
        xt = t.double()[:, lo:]
        xhat = (xt - xt.mean((0, 2, 3), keepdim=True)) / \
            (xt.var((0, 2, 3), unbiased=False, keepdim=True) + 1e-5).sqrt()
        gzt = gz[:, lo:].abs()
        _sum_close(bn.weight.grad, par[0].grad, (gzt * xhat.abs()).sum((0, 2, 3)), "dgamma", rel)
        _sum_close(bn.bias.grad, par[1].grad, gzt.sum((0, 2, 3)), "dbeta", rel)


# ------------------------------------------------------------------------------- grouped 1x1
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("co", [(32, 8), (256, 32), (128, 128), (256, 256)],
                         ids=lambda v: "%dto%d" % v)
def test_grouped_pointwise_conv_bn(co, dtype):
    """conv_bn with groups=4 (1x1, stride 1) through the block-diagonal packing: forward, dx, dW in
    the parameter's [O, C/4, 1, 1] layout and the BatchNorm statistics."""
    F = _F()
    C, O = co
    N, H, W, G = 2, 12, 20, 4
    x = quant(rnd((N, C, H, W), 111), dtype)
    w = quant(rnd((O, C // G, 1, 1), 112, 0.3), dtype)  # (the GEMM reads the weight in dtype)
    conv = nn.Conv2d(C, O, 1, groups=G, bias=False).to(DEV)
    bn = nn.BatchNorm2d(O, momentum=1.0).to(DEV).train()
    with torch.no_grad():
        conv.weight.copy_(w)
    xd = to_dev_nhwc(x, dtype).requires_grad_()
    act = F.conv_bn(F.Act(xd), conv, bn)
    xo, wo = x.double().requires_grad_(), w.double().requires_grad_()
    ref = TF.conv2d(xo, wo, None, 1, 0, 1, G)
    r = ref.detach()
    assert_close(to_cpu_nchw(act.t), r, dtype, "y")
    mag = TF.conv2d(x.double().abs(), w.double().abs(), None, 1, 0, 1, G)
    # 480 rows <= SMALL_BN_ROWS: finish_bn takes the statistics two-pass from the stored tensor,
    # in bf16 one rounding of each value (a square carries twice the relative error of its root)
    assert N * H * W <= F.K.SMALL_BN_ROWS
    rel = tol(dtype) if dtype == torch.bfloat16 else tol(torch.float32)
    _sum_close(bn.running_mean, r.mean((0, 2, 3)), mag.mean((0, 2, 3)), "batch mean", rel)
    _sum_close(bn.running_var, r.var((0, 2, 3)), (mag * mag).mean((0, 2, 3)), "batch variance",
               2 * rel)
    g = quant(rnd((N, O, H, W), 113), dtype)
    act.t.backward(to_dev_nhwc(g, dtype))
    ref.backward(g.double())
    assert_close(to_cpu_nchw(xd.grad), xo.grad, dtype, "dx")
    assert tuple(conv.weight.grad.shape) == (O, C // G, 1, 1)
    ones = torch.ones_like(wo).requires_grad_()
    TF.conv2d(x.double().abs(), ones, None, 1, 0, 1, G).backward(g.double().abs())
    _sum_close(conv.weight.grad, wo.grad, ones.grad, "dW")


def test_conv_bn_refuses_other_grouped_geometry():
    F = _F()
    x = F.Act(torch.zeros((1, 8, 8, 32), device=DEV))
    for conv in (nn.Conv2d(32, 32, 3, 1, 1, groups=4, bias=False),
                 nn.Conv2d(32, 32, 1, 2, 0, groups=4, bias=False)):
        with pytest.raises(NotImplementedError):
            F.conv_bn(x, conv.to(DEV))
