"""GPU: the kernels of csrc/fpenet.hip against torch float64 on the CPU — one stage of the FPE
pyramid forward and backward, functional.fpe_pyramid (four stages with training BatchNorm, the
few-sample and the plain path), the MEU forward and its two backward kernels, and
functional.meu_fuse.  Bars: _util.assert_close / tol(dtype) for what is stored in the activation
dtype; float32 sums (statistics, weight-gradient and BatchNorm-backward rows) against float64 at
tol(float32) of the sum of the magnitudes that were added.  Where a route stores intermediates in
the activation dtype before the value under test, `fac` is the number of roundings on that route.

Every stage / MEU operand is a slice at element offset 4 of a NaN-filled buffer whose pitch is 8
more than the operand is wide: offset 4 is 8-byte aligned only in bf16 and 16-byte aligned in
float32, the least the kernels ask for, and a NaN that reaches a result or leaves the padding
shows an out-of-slice access."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
OFF = 4


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
    assert err <= rel, "%s: %.3e of the summed magnitudes (bar %.3e)" % (what, err, rel)


def _sliced(x_nchw, dtype):
    """CPU NCHW -> the device NHWC slice at offset OFF of a NaN-filled buffer of pitch C + 8."""
    return to_dev_nhwc(x_nchw, dtype, pitch=x_nchw.shape[1] + 8, off=OFF)


def _out_slice(N, H, W, C, dtype):
    buf = torch.full((N, H, W, C + 8), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[..., OFF:OFF + C]


def _pad_is_nan(buf, C):
    return bool(torch.isnan(buf[..., :OFF]).all() and torch.isnan(buf[..., OFF + C:]).all())


def _vec(n, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) * (hi - lo) + lo


def _c(v):
    return v.view(1, -1, 1, 1).double()


# ------------------------------------------------------------------------------- one stage
STAGE_HW = [(1, 1), (2, 3), (7, 9), (9, 17), (33, 65)]


def _stage_inputs(N, H, W, n, dtype, seed):
    t = dict(a=quant(rnd((N, n, H, W), seed), dtype), b=quant(rnd((N, n, H, W), seed + 1), dtype),
             dy=quant(rnd((N, n, H, W), seed + 2), dtype),
             res=quant(rnd((N, n, H, W), seed + 3), dtype),
             w=rnd((n, 1, 3, 3), seed + 4, 0.4),
             sa=_vec(n, seed + 5, 0.5, 1.5), ta=_vec(n, seed + 6, -0.5, 0.5),
             sb=_vec(n, seed + 7, 0.5, 1.5), tb=_vec(n, seed + 8, -0.5, 0.5))
    return t


def _stage_ref(t, dil, has_b):
    """float64 autograd -> forward values, both masked gradients, dW and every summed row with the
    magnitudes that were added."""
    n = t["a"].shape[1]
    a, b, w = t["a"].double(), t["b"].double(), t["w"].double().requires_grad_()
    za = (a * _c(t["sa"]) + _c(t["ta"])).requires_grad_()
    zb = (b * _c(t["sb"]) + _c(t["tb"])).requires_grad_()
    rb = TF.relu(zb)
    inp = TF.relu(za) + rb if has_b else TF.relu(za)
    y = TF.conv2d(inp, w, None, 1, dil, dil, groups=n)
    ymag = TF.conv2d(inp.abs(), w.abs(), None, 1, dil, dil, groups=n)
    dy, res = t["dy"].double(), t["res"].double()
    loss = (y * dy).sum() + ((rb * res).sum() if has_b else 0.0)
    loss.backward()
    # the magnitudes behind the gradients: |dy| through |w|
    gmag = TF.conv_transpose2d(dy.abs(), w.detach().abs(), None, 1, dil, 0, n, dil)
    r = dict(y=y.detach(), ymag=ymag.detach(), rb=rb.detach(), ga=za.grad, dW=w.grad,
             gmag=gmag.detach(), inp=inp.detach())
    if has_b:
        r["gb"] = zb.grad
        r["gbmag"] = (gmag + res.abs()).detach()
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("has_b", [True, False], ids=["b", "nob"])
@pytest.mark.parametrize("n", [4, 8, 16, 32])
@pytest.mark.parametrize("dil", [1, 2, 4, 8])
@pytest.mark.parametrize("hw", STAGE_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 3])
def test_stage_forward_and_backward(N, hw, dil, n, has_b, dtype):
    K = _K()
    H, W = hw
    t = _stage_inputs(N, H, W, n, dtype, 11)
    ref = _stage_ref(t, dil, has_b)
    d = {k: _sliced(t[k], dtype) for k in ("a", "b", "dy", "res")}
    p = {k: t[k].to(DEV) for k in ("w", "sa", "ta", "sb", "tb")}

    # ---- forward
    def fwd(dd):
        ybuf, y = _out_slice(N, H, W, n, dtype)
        obuf, o = _out_slice(N, H, W, n, dtype)
        kw = dict(b=dd["b"], sb=p["sb"], tb=p["tb"], b_act=o) if has_b else {}
        _, partial = K.fpe_stage_fwd(dd["a"], p["sa"], p["ta"], p["w"], dil, out=y, **kw)
        return ybuf, y, obuf, o, partial
    ybuf, y, obuf, o, partial = fwd(d)
    rows = K.fpe_stage_rows(dtype, N, H, W, n)
    assert tuple(partial.shape) == (rows, 2, n) and rows % N == 0
    assert_close(to_cpu_nchw(y), ref["y"], dtype, "y", scale=ref["ymag"].max().item())
    assert _pad_is_nan(ybuf, n) and _pad_is_nan(d["a"]._base, n)
    if has_b:
        # act(b) at the centre pixel, one rounding
        assert_close(to_cpu_nchw(o), ref["rb"], dtype, "b_act")
        assert _pad_is_nan(obuf, n)
    else:
        assert torch.isnan(obuf).all()
    sums = partial.double().sum(0).cpu()
    _sum_close(sums[0], ref["y"].sum((0, 2, 3)), ref["ymag"].sum((0, 2, 3)), "sum")
    _sum_close(sums[1], (ref["y"] ** 2).sum((0, 2, 3)), (ref["ymag"] ** 2).sum((0, 2, 3)),
               "sum of squares")
    _, y2, _, o2, partial2 = fwd(d)
    assert torch.equal(y2, y) and torch.equal(partial2, partial)
    assert not has_b or torch.equal(o2, o)

    # ---- backward
    def bwd(dd):
        gabuf, ga = _out_slice(N, H, W, n, dtype)
        gbbuf, gb = _out_slice(N, H, W, n, dtype)
        pa = torch.full((rows, 2, 4 * n), float("nan"), device=DEV)
        kw = dict(b=dd["b"], sb=p["sb"], tb=p["tb"], res=dd["res"], gb=gb) if has_b else {}
        _, _, pw, _, pb = K.fpe_stage_bwd(dd["dy"], dd["a"], p["sa"], p["ta"], p["w"], dil, ga=ga,
                                          pa=pa, pa_col=n, **kw)
        return gabuf, ga, gbbuf, gb, pw, pa, pb
    gabuf, ga, gbbuf, gb, pw, pa, pb = bwd(d)
    gscale = ref["gmag"].max().item()
    assert_close(to_cpu_nchw(ga), ref["ga"], dtype, "ga", scale=gscale)
    assert _pad_is_nan(gabuf, n)
    # partial_a lands in its column slice and nowhere else
    assert torch.isnan(pa[..., :n]).all() and torch.isnan(pa[..., 2 * n:]).all()
    sa_ = pa[..., n:2 * n].double().sum(0).cpu()
    a64 = t["a"].double()
    gam = ref["gmag"]
    _sum_close(sa_[0], ref["ga"].sum((0, 2, 3)), gam.sum((0, 2, 3)), "sum ga")
    _sum_close(sa_[1], (ref["ga"] * a64).sum((0, 2, 3)), (gam * a64.abs()).sum((0, 2, 3)),
               "sum ga*a")
    # weight-gradient rows [rows, 9, n]: sum_p dy[p - d_k] * in[p]
    assert tuple(pw.shape) == (rows, 9, n)
    dW = pw.double().sum(0).cpu().t().reshape(n, 1, 3, 3)
    _sum_close(dW, ref["dW"], _wgrad_mag(ref["inp"], t["dy"].double(), dil), "dW")
    if has_b:
        assert_close(to_cpu_nchw(gb), ref["gb"], dtype, "gb", scale=ref["gbmag"].max().item())
        assert _pad_is_nan(gbbuf, n)
        sb_ = pb.double().sum(0).cpu()
        b64 = t["b"].double()
        _sum_close(sb_[0], ref["gb"].sum((0, 2, 3)), ref["gbmag"].sum((0, 2, 3)), "sum gb")
        _sum_close(sb_[1], (ref["gb"] * b64).sum((0, 2, 3)),
                   (ref["gbmag"] * b64.abs()).sum((0, 2, 3)), "sum gb*b")
    else:
        assert pb is None and torch.isnan(gbbuf).all()
    _, ga2, _, gb2, pw2, pa2, pb2 = bwd(d)
    assert torch.equal(ga2, ga) and torch.equal(pw2, pw)
    assert torch.equal(pa2[..., n:2 * n], pa[..., n:2 * n])
    assert not has_b or (torch.equal(gb2, gb) and torch.equal(pb2, pb))

    if N == 3:  # image 1 at 1e30 leaves images 0 and 2 and their partial rows bit-equal
        big = {}
        for k, v in d.items():
            big[k] = _sliced(t[k], dtype)
            big[k][1] = 1e30
        _, y3, _, o3, partial3 = fwd(big)
        _, ga3, _, gb3, pw3, pa3, pb3 = bwd(big)
        for i in (0, 2):
            assert torch.equal(y3[i], y[i])
            assert torch.equal(partial3.view(-1, N, 2, n)[:, i], partial.view(-1, N, 2, n)[:, i])
            assert torch.equal(ga3[i], ga[i])
            assert torch.equal(pw3.view(-1, N, 9, n)[:, i], pw.view(-1, N, 9, n)[:, i])
            assert torch.equal(pa3.view(-1, N, 2, 4 * n)[:, i, :, n:2 * n],
                               pa.view(-1, N, 2, 4 * n)[:, i, :, n:2 * n])
            if has_b:
                assert torch.equal(o3[i], o[i]) and torch.equal(gb3[i], gb[i])
                assert torch.equal(pb3.view(-1, N, 2, n)[:, i], pb.view(-1, N, 2, n)[:, i])


def _wgrad_mag(inp, dy, dil):
    """[n,1,3,3]: sum_p |dy[p - d_k]| * |in[p]|, the magnitudes behind each weight gradient."""
    N, n, H, W = inp.shape
    pad = TF.pad(inp.abs(), (dil,) * 4)
    out = torch.empty((n, 1, 3, 3), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            win = pad[:, :, kh * dil:kh * dil + H, kw * dil:kw * dil + W]
            out[:, 0, kh, kw] = (win * dy.abs()).sum((0, 2, 3))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [4, 16])
def test_last_slice_forward_and_backward(n, dtype):
    """Slice 3 of the concat: relu(sb*b + tb) forward; gb = mask(b) * res and its rows backward."""
    K = _K()
    N, H, W = 3, 9, 17
    t = _stage_inputs(N, H, W, n, dtype, 23)
    b, res = _sliced(t["b"], dtype), _sliced(t["res"], dtype)
    sb, tb = t["sb"].to(DEV), t["tb"].to(DEV)
    obuf, o = _out_slice(N, H, W, n, dtype)
    K.fpe_act_fwd(b, sb, tb, out=o)
    zb = t["b"].double() * _c(t["sb"]) + _c(t["tb"])
    assert_close(to_cpu_nchw(o), TF.relu(zb), dtype, "act")
    assert _pad_is_nan(obuf, n)
    gbbuf, gb = _out_slice(N, H, W, n, dtype)
    ga, _, pw, pa, pb = K.fpe_stage_bwd(None, None, None, None, None, 8, b=b, sb=sb, tb=tb,
                                        res=res, gb=gb)
    assert ga is None and pw is None and pa is None
    ref = (zb > 0).double() * t["res"].double()
    assert torch.equal(to_cpu_nchw(gb).double(), ref)  # (a select: exact)
    assert _pad_is_nan(gbbuf, n)
    s = pb.double().sum(0).cpu()
    b64 = t["b"].double()
    _sum_close(s[0], ref.sum((0, 2, 3)), ref.abs().sum((0, 2, 3)), "sum gb")
    _sum_close(s[1], (ref * b64).sum((0, 2, 3)), (ref * b64).abs().sum((0, 2, 3)), "sum gb*b")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_slice_bn_backward_apply(train, dtype):
    K = _K()
    N, H, W, n = 2, 5, 7, 4
    g, x = quant(rnd((N, n, H, W), 31), dtype), quant(rnd((N, n, H, W), 32), dtype)
    s, c0, c1 = _vec(n, 33, 0.5, 1.5), _vec(n, 34, -0.1, 0.1), _vec(n, 35, -0.1, 0.1)
    obuf, o = _out_slice(N, H, W, n, dtype)
    K.fpe_bn_bwd_apply(_sliced(g, dtype), _sliced(x, dtype), s.to(DEV),
                       c0.to(DEV) if train else None, c1.to(DEV) if train else None, out=o)
    ref = _c(s) * g.double()
    mag = ref.abs()
    if train:
        ref = ref - _c(c0) - _c(c1) * x.double()
        mag = mag + _c(c0).abs() + (_c(c1) * x.double()).abs()
    assert_close(to_cpu_nchw(o), ref, dtype, "dx", scale=mag.max().item())
    assert _pad_is_nan(obuf, n)


@pytest.mark.parametrize("n,dil", [(6, 1), (0, 1), (68, 1), (8, 0), (8, 9)],
                         ids=["n6", "n0", "n68", "dil0", "dil9"])
def test_stage_rejects_what_is_outside_its_contract(n, dil):
    """The host raises before any launch: the output buffer keeps its NaNs."""
    K = _K()
    N, H, W = 1, 5, 5
    a = torch.zeros((N, H, W, n), device=DEV)
    out = torch.full((N, H, W, max(n, 1)), float("nan"), device=DEV)
    one = torch.ones(max(n, 1), device=DEV)
    with pytest.raises(ValueError, match="fpe_stage"):
        K.fpe_stage_fwd(a, one, one, torch.zeros((max(n, 1), 1, 3, 3), device=DEV), dil, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------- the pyramid node
def _pyramid_modules(n, seed):
    torch.manual_seed(seed)
    bn1 = nn.BatchNorm2d(4 * n)
    convs = nn.ModuleList([nn.Conv2d(n, n, 3, 1, d, d, groups=n, bias=False) for d in (1, 2, 4, 8)])
    bns = nn.ModuleList([nn.BatchNorm2d(n) for _ in range(4)])
    with torch.no_grad():
        for m in [bn1] + list(bns):
            m.weight.copy_(_vec(m.num_features, seed + m.num_features, 0.5, 1.5))
            m.bias.copy_(_vec(m.num_features, seed + 1 + m.num_features, -0.3, 0.3))
    return bn1, convs, bns


def _pyramid_ref(u, bn1, convs, bns, dtype=torch.float32):
    """The four stages in float64.  bf16: each raw stage output is stored once and read back by its
    BatchNorm and by the next stage, so the restatement rounds it at that one point too (straight
    through in backward) — a ReLU mask taken from an unrounded value would differ from the one
    the stored tensor decides wherever the rounding crosses zero."""
    n = u.shape[1] // 4
    xs = torch.chunk(TF.relu(bn1(u)), 4, 1)
    ys = []
    for s in range(4):
        t = convs[s](xs[s] if s == 0 else xs[s] + ys[-1])
        if dtype != torch.float32:
            t = t + (t.detach().to(dtype).double() - t.detach())
        ys.append(TF.relu(bns[s](t)))
    assert ys[0].shape[1] == n
    return torch.cat(ys, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("stage0", [True, False], ids=["stage0_new", "stage0_dw"])
@pytest.mark.parametrize("shape", [(3, 9, 17, 16), (3, 9, 17, 64), (2, 48, 48, 16)],
                         ids=["few_n4", "few_n16", "plain_n4"])
def test_fpe_pyramid_forward_and_backward(shape, stage0, dtype, monkeypatch):
    """functional.fpe_pyramid against a float64 restatement of the four stages with training
    BatchNorm: 459 rows take the few-sample BatchNorm path, 4608 the plain one.  bf16: every stage
    stores its raw output once and the next reads it, so slice s carries up to s + 2 roundings
    forward (fac 8 covers the BatchNorm's division by the batch deviation); backward each stage
    stores three gradients in turn, 3 x 4 + the incoming and the outgoing one (fac 16)."""
    F, K = _F(), _K()
    N, H, W, C4 = shape
    n = C4 // 4
    assert (N * H * W <= K.SMALL_BN_ROWS) == (H == 9)
    # stage 0's forward on either of its routes (forced through the routing function; 4 channels
    # of bf16 are outside the depthwise launch's contract and stay on the new kernel)
    monkeypatch.setattr(F, "fpe_stage0_routed", lambda *a: stage0)
    calls = []
    real = F.K.dwconv
    monkeypatch.setattr(F.K, "dwconv", lambda *a, **k: calls.append(1) or real(*a, **k))
    u = quant(rnd((N, C4, H, W), 41), dtype)
    g = quant(rnd((N, C4, H, W), 42), dtype)
    bn1, convs, bns = _pyramid_modules(n, 43)
    ref_m = [copy.deepcopy(m).double().train() for m in (bn1, convs, bns)]
    dev_m = [m.to(DEV).train() for m in (bn1, convs, bns)]
    # float64
    u64 = u.double().requires_grad_()
    ref = _pyramid_ref(u64, *ref_m, dtype=dtype)
    ref.backward(g.double())
    # HIP
    ud = to_dev_nhwc(u, dtype).requires_grad_()
    act = F.bn_of_concat(ud, dev_m[0])
    cat = F.fpe_pyramid(act, list(dev_m[1]), list(dev_m[2]))
    assert tuple(cat.shape) == (N, H, W, C4) and cat.dtype == dtype
    assert len(calls) == (0 if stage0 or n % K.vec_of(dtype) else 1)
    cat.backward(to_dev_nhwc(g, dtype))
    assert_close(to_cpu_nchw(cat), ref.detach(), dtype, "concat", fac=8.0)
    assert_close(to_cpu_nchw(ud.grad), u64.grad, dtype, "du", fac=16.0)
    for s in range(4):
        assert_close(dev_m[1][s].weight.grad.cpu(), ref_m[1][s].weight.grad, dtype, "dW%d" % s,
                     fac=16.0)
    for name, md, mr in [("bn1", dev_m[0], ref_m[0])] + [("bn2.%d" % s, dev_m[2][s], ref_m[2][s])
                                                         for s in range(4)]:
        assert_close(md.weight.grad.cpu(), mr.weight.grad, dtype, name + " dgamma", fac=16.0)
        assert_close(md.bias.grad.cpu(), mr.bias.grad, dtype, name + " dbeta", fac=16.0)
        assert_close(md.running_mean.cpu(), mr.running_mean, dtype, name + " running_mean",
                     fac=8.0)
        assert_close(md.running_var.cpu(), mr.running_var, dtype, name + " running_var", fac=8.0)
        assert int(md.num_batches_tracked) == int(mr.num_batches_tracked) == 1


def test_stage0_routing_follows_the_measured_classes():
    F = _F()
    bf, rows = torch.bfloat16, 4 * 192 * 192
    assert not F.fpe_stage0_routed(bf, 16, rows) and not F.fpe_stage0_routed(bf, 32, rows // 4)
    assert F.fpe_stage0_routed(bf, 8, rows) and F.fpe_stage0_routed(bf, 16, rows // 4)
    assert F.fpe_stage0_routed(bf, 4, 4 * rows) and F.fpe_stage0_routed(torch.float32, 32, rows)


def test_fpe_pyramid_evaluation_mode_runs_the_same_code():
    F = _F()
    N, H, W, n = 2, 9, 17, 8
    dtype = torch.float32
    u, g = rnd((N, 4 * n, H, W), 51), rnd((N, 4 * n, H, W), 52)
    bn1, convs, bns = _pyramid_modules(n, 53)
    with torch.no_grad():
        for m in [bn1] + list(bns):
            m.running_mean.copy_(_vec(m.num_features, 54, -0.2, 0.2))
            m.running_var.copy_(_vec(m.num_features, 55, 0.5, 1.5))
    ref_m = [copy.deepcopy(m).double().eval() for m in (bn1, convs, bns)]
    dev_m = [m.to(DEV).eval() for m in (bn1, convs, bns)]
    u64 = u.double().requires_grad_()
    ref = _pyramid_ref(u64, *ref_m)
    ref.backward(g.double())
    ud = to_dev_nhwc(u, dtype).requires_grad_()
    cat = F.fpe_pyramid(F.bn_of_concat(ud, dev_m[0]), list(dev_m[1]), list(dev_m[2]))
    cat.backward(to_dev_nhwc(g, dtype))
    assert_close(to_cpu_nchw(cat), ref.detach(), dtype, "concat", fac=8.0)
    assert_close(to_cpu_nchw(ud.grad), u64.grad, dtype, "du", fac=16.0)
    for s in range(4):
        assert_close(dev_m[1][s].weight.grad.cpu(), ref_m[1][s].weight.grad, dtype, "dW", fac=16.0)
        assert_close(dev_m[2][s].weight.grad.cpu(), ref_m[2][s].weight.grad, dtype, "dgamma",
                     fac=16.0)
        assert int(dev_m[2][s].num_batches_tracked) == 0


# ------------------------------------------------------------------------------- MEU
MEU_GEOM = [((1, 1), (1, 1)), ((1, 1), (2, 2)), ((2, 3), (3, 5)), ((4, 6), (8, 12)),
            ((5, 7), (9, 13)), ((8, 12), (8, 12)), ((17, 33), (33, 65))]


def _meu_inputs(N, C, hw2, hw, dtype, seed):
    (h2, w2), (h, w) = hw2, hw
    return dict(L=quant(rnd((N, C, h, w), seed), dtype), H=quant(rnd((N, C, h2, w2), seed + 1), dtype),
                g=quant(rnd((N, C, h, w), seed + 2), dtype),
                a=torch.sigmoid(rnd((N, C), seed + 3)), dpool=rnd((N, C), seed + 4),
                wsa=torch.tensor([1.7]),
                sl=_vec(C, seed + 5, 0.5, 1.5), tl=_vec(C, seed + 6, -0.5, 0.5),
                sh=_vec(C, seed + 7, 0.5, 1.5), th=_vec(C, seed + 8, -0.5, 0.5))


def _meu_ref(t):
    L, Hr = t["L"].double(), t["H"].double()
    a = t["a"].double().requires_grad_()
    wsa = t["wsa"].double().requires_grad_()
    lbn = (L * _c(t["sl"]) + _c(t["tl"])).requires_grad_()
    hbn = (Hr * _c(t["sh"]) + _c(t["th"])).requires_grad_()
    sa = torch.sigmoid(wsa * lbn.mean(1, keepdim=True))
    up = TF.interpolate(hbn, size=L.shape[2:], mode="bilinear", align_corners=True)
    out = a[:, :, None, None] * lbn + sa * up
    mag = (a[:, :, None, None] * lbn).abs() + (sa * up).abs()
    g = t["g"].double()
    ((out * g).sum() + (hbn.mean((2, 3)) * t["dpool"].double()).sum()).backward()
    # the magnitudes behind dH: |g| * sa through the transposed interpolation, plus the pool's share
    gs = (g.abs() * sa.detach()).requires_grad_()
    hb = torch.zeros_like(hbn).requires_grad_()
    TF.interpolate(hb, size=L.shape[2:], mode="bilinear", align_corners=True).backward(gs.detach())
    dhmag = hb.grad + (t["dpool"].double().abs() / (Hr.shape[2] * Hr.shape[3]))[:, :, None, None]
    S = (g * up.detach()).sum(1, keepdim=True)
    Smag = (g * up.detach()).abs().sum(1, keepdim=True)
    ds = (sa * (1 - sa)).detach()
    dlmag = (a.detach()[:, :, None, None] * g).abs() + wsa.detach().abs() * ds * Smag / L.shape[1]
    return dict(out=out.detach(), mag=mag.detach(), sa=sa.detach()[:, 0], dL=lbn.grad, dH=hbn.grad,
                da=a.grad, dwsa=wsa.grad, dhmag=dhmag.detach(), dlmag=dlmag.detach(),
                damag=(g * lbn.detach()).abs().sum((2, 3)),
                dwmag=(ds * lbn.detach().mean(1, keepdim=True).abs() * Smag).sum(),
                S=S)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [8, 32, 64])
@pytest.mark.parametrize("geom", MEU_GEOM, ids=lambda v: "%dx%d_%dx%d" % (v[0] + v[1]))
@pytest.mark.parametrize("N", [1, 3])
def test_meu_forward_and_backward(N, geom, C, dtype):
    K = _K()
    hw2, hw = geom
    (h2, w2), (h, w) = hw2, hw
    t = _meu_inputs(N, C, hw2, hw, dtype, 61)
    ref = _meu_ref(t)
    p = {k: t[k].to(DEV) for k in ("a", "dpool", "wsa", "sl", "tl", "sh", "th")}
    aff_l, aff_h = (p["sl"], p["tl"]), (p["sh"], p["th"])

    def run(big=False):
        d = {k: _sliced(t[k], dtype) for k in ("L", "H", "g")}
        if big:
            for v in d.values():
                v[1] = 1e30
        obuf, o = _out_slice(N, h, w, C, dtype)
        _, sa = K.meu_fwd(d["L"], aff_l, d["H"], aff_h, p["a"], p["wsa"], out=o)
        lbuf, dl = _out_slice(N, h, w, C, dtype)
        _, da, dwsa, pbl = K.meu_bwd_low(d["g"], d["L"], aff_l, d["H"], aff_h, p["a"], p["wsa"], sa,
                                         out=dl)
        hbuf, dh = _out_slice(N, h2, w2, C, dtype)
        _, pbh = K.meu_bwd_high(d["g"], sa, d["H"], p["dpool"], out=dh)
        return dict(obuf=obuf, o=o, sa=sa, lbuf=lbuf, dl=dl, da=da, dwsa=dwsa, pbl=pbl, hbuf=hbuf,
                    dh=dh, pbh=pbh, d=d)
    r = run()
    assert_close(to_cpu_nchw(r["o"]), ref["out"], dtype, "out", scale=ref["mag"].max().item())
    assert r["sa"].dtype == torch.float32 and tuple(r["sa"].shape) == (N, h, w)
    assert_close(r["sa"].cpu(), ref["sa"], torch.float32, "sa")
    assert _pad_is_nan(r["obuf"], C) and _pad_is_nan(r["d"]["L"]._base, C)
    assert _pad_is_nan(r["d"]["H"]._base, C)
    # the low-resolution pass
    assert_close(to_cpu_nchw(r["dl"]), ref["dL"], dtype, "dL", scale=ref["dlmag"].max().item())
    assert _pad_is_nan(r["lbuf"], C)
    _sum_close(r["da"], ref["da"], ref["damag"], "da")
    _sum_close(r["dwsa"], ref["dwsa"], ref["dwmag"].view(1), "d w_sa")
    L64, H64 = t["L"].double(), t["H"].double()
    s = r["pbl"].double().sum(0).cpu()
    _sum_close(s[0], ref["dL"].sum((0, 2, 3)), ref["dlmag"].sum((0, 2, 3)), "sum dL")
    _sum_close(s[1], (ref["dL"] * L64).sum((0, 2, 3)), (ref["dlmag"] * L64.abs()).sum((0, 2, 3)),
               "sum dL*L")
    # the gather at high-level resolution
    assert_close(to_cpu_nchw(r["dh"]), ref["dH"], dtype, "dH", scale=ref["dhmag"].max().item())
    assert _pad_is_nan(r["hbuf"], C)
    s = r["pbh"].double().sum(0).cpu()
    _sum_close(s[0], ref["dH"].sum((0, 2, 3)), ref["dhmag"].sum((0, 2, 3)), "sum dH")
    _sum_close(s[1], (ref["dH"] * H64).sum((0, 2, 3)), (ref["dhmag"] * H64.abs()).sum((0, 2, 3)),
               "sum dH*H")
    # a second run gives the same bits
    r2 = run()
    for k in ("o", "sa", "dl", "da", "dwsa", "pbl", "dh", "pbh"):
        assert torch.equal(r2[k], r[k]), k
    if N == 3:  # image 1 at 1e30 leaves images 0 and 2 and their partial rows bit-equal
        r3 = run(big=True)
        for i in (0, 2):
            for k in ("o", "sa", "dl", "da", "dh"):
                assert torch.equal(r3[k][i], r[k][i]), k
            for k in ("pbl", "pbh"):
                assert torch.equal(r3[k].view(-1, N, 2, C)[:, i], r[k].view(-1, N, 2, C)[:, i]), k


@pytest.mark.parametrize("C,hw2,hw", [(12, (2, 2), (4, 4)), (4, (2, 2), (4, 4)),
                                      (136, (2, 2), (4, 4)), (8, (5, 2), (4, 4)),
                                      (8, (2, 5), (4, 4))],
                         ids=["C12", "C4", "C136", "high_taller", "high_wider"])
def test_meu_rejects_what_is_outside_its_contract(C, hw2, hw):
    K = _K()
    L = torch.zeros((1,) + hw + (C,), device=DEV)
    Hr = torch.zeros((1,) + hw2 + (C,), device=DEV)
    out = torch.full((1,) + hw + (C,), float("nan"), device=DEV)
    with pytest.raises(ValueError, match="meu"):
        K.meu_fwd(L, None, Hr, None, torch.zeros((1, C), device=DEV), torch.ones(1, device=DEV),
                  out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


class _MEURef(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.bn_low, self.bn_high = nn.BatchNorm2d(C), nn.BatchNorm2d(C)
        self.sa_conv = nn.Conv2d(1, 1, 1, bias=False)
        self.ca_conv = nn.Conv2d(C, C, 1, bias=False)

    def forward(self, L, Hr):
        low, high = self.bn_low(L), self.bn_high(Hr)
        sa = torch.sigmoid(self.sa_conv(low.mean(1, keepdim=True)))
        ca = torch.sigmoid(TF.relu(self.ca_conv(high.mean((2, 3), keepdim=True))))
        up = TF.interpolate(high, size=L.shape[2:], mode="bilinear", align_corners=True)
        return ca * low + sa * up


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", [((5, 7), (9, 13)), ((24, 24), (40, 40))], ids=["few", "plain"])
def test_meu_fuse_forward_and_backward(geom, dtype):
    """functional.meu_fuse with training BatchNorms against float64 autograd: both raw maps, both
    BatchNorms, ca_conv (through da and the pool's gradient) and sa_conv.  2 x 9 x 13 and 2 x 5 x 7
    rows take the few-sample path, 3200 and 1152 the plain one.  bf16: the stored gradient at each
    BatchNorm's output and the stored result, 2 roundings before the value under test (fac 4 with
    the division by the batch deviation)."""
    F, K = _F(), _K()
    (h2, w2), (h, w) = geom
    N, C = 2, 32
    assert (N * h * w <= K.SMALL_BN_ROWS) == (h == 9)
    torch.manual_seed(71)
    m = _MEURef(C)
    with torch.no_grad():
        for bn in (m.bn_low, m.bn_high):
            bn.weight.copy_(_vec(C, 72, 0.5, 1.5))
            bn.bias.copy_(_vec(C, 73, -0.3, 0.3))
        m.sa_conv.weight.fill_(1.3)
    L, Hr, g = (quant(rnd((N, C, h, w), 74), dtype), quant(rnd((N, C, h2, w2), 75), dtype),
                quant(rnd((N, C, h, w), 76), dtype))
    mr = copy.deepcopy(m).double().train()
    md = m.to(DEV).train()
    L64, H64 = L.double().requires_grad_(), Hr.double().requires_grad_()
    ref = mr(L64, H64)
    ref.backward(g.double())
    Ld, Hd = to_dev_nhwc(L, dtype).requires_grad_(), to_dev_nhwc(Hr, dtype).requires_grad_()
    out = F.meu_fuse(F.bn_of_concat(Ld, md.bn_low), F.bn_of_concat(Hd, md.bn_high), md.ca_conv,
                     md.sa_conv)
    out.backward(to_dev_nhwc(g, dtype))
    fac = 4.0
    assert_close(to_cpu_nchw(out), ref.detach(), dtype, "out", fac=fac)
    assert_close(to_cpu_nchw(Ld.grad), L64.grad, dtype, "dL", fac=fac)
    assert_close(to_cpu_nchw(Hd.grad), H64.grad, dtype, "dH", fac=fac)
    assert_close(md.sa_conv.weight.grad.cpu(), mr.sa_conv.weight.grad, dtype, "d w_sa", fac=fac)
    assert_close(md.ca_conv.weight.grad.cpu(), mr.ca_conv.weight.grad, dtype, "d ca_conv", fac=fac)
    for name in ("bn_low", "bn_high"):
        bd, br = getattr(md, name), getattr(mr, name)
        assert_close(bd.weight.grad.cpu(), br.weight.grad, dtype, name + " dgamma", fac=fac)
        assert_close(bd.bias.grad.cpu(), br.bias.grad, dtype, name + " dbeta", fac=fac)
        assert_close(bd.running_mean.cpu(), br.running_mean, dtype, name + " running_mean", fac=fac)
        assert_close(bd.running_var.cpu(), br.running_var, dtype, name + " running_var", fac=fac)
        assert int(bd.num_batches_tracked) == 1
