"""GPU: the kernels of csrc/unet.hip against torch float64 on the CPU — the fused skip + max-pool
pass forward and backward, functional.skip_pool behind a training BatchNorm (the plain and the
few-sample path), the bilinear resize with a destination window forward and backward — and the fused
cross-entropy at resize factor 1, which UNet is the first model to reach.  Bars:
_util.assert_close / tol(dtype) for what is stored in the activation dtype; float32 sums (the
BatchNorm-backward rows) against float64 at tol(float32) of the sum of the magnitudes that were
added.

Every pitched operand is a slice at element offset `vec` (one 16-byte vector: the least aligned
offset the contract allows) of a NaN-filled buffer whose pitch is two vectors more than the operand
is wide: a NaN that reaches a result or leaves the padding shows an out-of-slice access."""
import functools

import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
AFFINE_RELU, NONE = 3, 0


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


# ------------------------------------------------------------------------- skip + max-pool
SP_HW = [(2, 2), (3, 3), (2, 5), (7, 9), (9, 17), (33, 65)]
SP_C = [8, 24, 64, 136]


def _general_affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5


def _dyadic_affine(C, seed):
    """scale a power of two, shift a multiple of 1/8: s*y + t of a value of at most 24 significant
    bits is exact in float64 and rounds once in float32, so the reference's rounded activation IS
    the kernel's, and with it the windows' winners (a general scale would leave the winner of a
    window whose top two lie within one rounding of each other to the last bit of an fmaf)."""
    g = torch.Generator().manual_seed(seed)
    s = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
    t = torch.randint(-4, 5, (C,), generator=g).float() / 8.0
    return s, t


def _pro(mode, s, t):
    if mode == NONE:
        return (NONE, None, None)
    return (mode, s.to(DEV), t.to(DEV))


def _act_ref(y, mode, s, t, dtype):
    """float64 activation, and the same rounded to the activation dtype (what is stored)."""
    a = y.double()
    if mode & 2:
        a = a * _c(s) + _c(t)
    if mode & 1:
        a = torch.relu(a)
    return a, a.to(dtype).double()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [AFFINE_RELU, NONE], ids=["affine_relu", "plain"])
@pytest.mark.parametrize("C", SP_C)
@pytest.mark.parametrize("hw", SP_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 3])
def test_skip_pool_forward(N, hw, C, mode, dtype):
    K = _K()
    H, W = hw
    y = quant(rnd((N, C, H, W), 3), dtype)
    s, t = _general_affine(C, 5)
    a, _ = _act_ref(y, mode, s, t, dtype)
    yd = _sliced(y, dtype)
    sbuf, sk = _out_slice(N, H, W, C, dtype)
    skip, pooled = K.skip_pool_fwd(yd, _pro(mode, s, t), out=sk)
    assert skip.data_ptr() == sk.data_ptr()
    assert tuple(pooled.shape) == (N, H // 2, W // 2, C) and pooled.dtype == dtype
    assert_close(to_cpu_nchw(skip), a, dtype, "skip")
    # the pooled map is the 2x2 max of the STORED values, bit for bit (floor: a trailing odd row or
    # column has no window)
    own = TF.max_pool2d(to_cpu_nchw(skip), 2)
    assert torch.equal(_bits(to_cpu_nchw(pooled)), _bits(own))
    assert _pad_is_nan(sbuf, C) and _pad_is_nan(yd._base, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [(1, 4), (4, 1), (1, 1)], ids=lambda v: "%dx%d" % v)
def test_skip_pool_without_a_window_raises(hw, dtype):
    K = _K()
    H, W = hw
    C = 8
    yd = _sliced(rnd((1, C, H, W), 3), dtype)
    with pytest.raises(RuntimeError, match="2x2 window"):
        K.skip_pool_fwd(yd, None)
    with pytest.raises(RuntimeError, match="2x2 window"):
        K.skip_pool_bwd(yd, None, yd, None)
    torch.cuda.synchronize()


def _sp_bwd_ref(y, gs, gp, mode, s, t, dtype):
    """The issue's reference: the activation rounded to the dtype, F.max_pool2d(return_indices) on
    it, g_pool scattered, g_skip added, the ReLU mask.  -> g', the two column sums and the summed
    magnitudes."""
    N, C, H, W = y.shape
    _, ar = _act_ref(y, mode, s, t, dtype)
    g = torch.zeros_like(ar) if gs is None else gs.double().clone()
    if gp is not None:
        _, idx = TF.max_pool2d(ar, 2, return_indices=True)
        g = g + torch.zeros(N, C, H * W, dtype=torch.float64).scatter_(
            2, idx.view(N, C, -1), gp.double().view(N, C, -1)).view(N, C, H, W)
    if mode & 1:
        g = g * (ar > 0)
    gy = g * y.double()
    return g, (g.sum((0, 2, 3)), g.abs().sum((0, 2, 3))), (gy.sum((0, 2, 3)), gy.abs().sum((0, 2, 3)))


def _sp_bwd_check(N, H, W, C, mode, dtype, which=("skip", "pool"), y=None, seed=7):
    K = _K()
    if y is None:
        y = quant(rnd((N, C, H, W), seed), dtype)
    s, t = _dyadic_affine(C, seed + 1)
    gs = quant(rnd((N, C, H, W), seed + 2), dtype) if "skip" in which else None
    gp = quant(rnd((N, C, H // 2, W // 2), seed + 3), dtype) if "pool" in which else None
    g, (sg, mg), (sgy, mgy) = _sp_bwd_ref(y, gs, gp, mode, s, t, dtype)
    yd = _sliced(y, dtype)
    gsd = None if gs is None else _sliced(gs, dtype)
    gpd = None if gp is None else _sliced(gp, dtype)
    obuf, o = _out_slice(N, H, W, C, dtype)
    out, partial = K.skip_pool_bwd(gsd, gpd, yd, _pro(mode, s, t), out=o)
    rows = K.skip_pool_rows(dtype, N, H, W, C)
    assert tuple(partial.shape) == (rows, 2, C) and partial.dtype == torch.float32
    got = to_cpu_nchw(out)
    assert_close(got, g, dtype, "g'", scale=max(g.abs().max().item(), 1e-3))
    tot = partial.double().sum(0).cpu()
    _sum_close(tot[0], sg, mg, "sum g'")
    _sum_close(tot[1], sgy, mgy, "sum g'*y")
    assert _pad_is_nan(obuf, C) and _pad_is_nan(yd._base, C)
    return got, g, gs, gp, rows


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [AFFINE_RELU, NONE], ids=["affine_relu", "plain"])
@pytest.mark.parametrize("C", SP_C)
@pytest.mark.parametrize("hw", SP_HW, ids=lambda v: "%dx%d" % v)
@pytest.mark.parametrize("N", [1, 3])
def test_skip_pool_backward(N, hw, C, mode, dtype):
    H, W = hw
    got, g, gs, gp, _ = _sp_bwd_check(N, H, W, C, mode, dtype)
    if mode == NONE:
        # a trailing odd row or column receives g_skip alone (no mask without a ReLU): bit for bit
        if H % 2:
            assert torch.equal(got[:, :, H - 1, :], gs[:, :, H - 1, :])
        if W % 2:
            assert torch.equal(got[:, :, :, W - 1], gs[:, :, :, W - 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", [("skip",), ("pool",)], ids=["skip_only", "pool_only"])
def test_skip_pool_backward_takes_a_missing_gradient(which, dtype):
    _sp_bwd_check(2, 7, 9, 24, AFFINE_RELU, dtype, which=which)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [AFFINE_RELU, NONE], ids=["affine_relu", "plain"])
def test_skip_pool_backward_ties_go_to_the_top_left(mode, dtype):
    """A constant positive y: every window is a four-way tie, the first maximum in row-major order
    wins (ATen's max_pool2d rule)."""
    N, H, W, C = 2, 7, 9, 24
    y = torch.full((N, C, H, W), 3.0)
    got, g, gs, gp, _ = _sp_bwd_check(N, H, W, C, mode, dtype, which=("pool",), y=y)
    want = torch.zeros(N, C, H, W)
    want[:, :, 0:2 * (H // 2):2, 0:2 * (W // 2):2] = gp
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_skip_pool_backward_of_an_all_negative_map_is_zero(dtype):
    K = _K()
    N, H, W, C = 2, 7, 9, 24
    y = -(rnd((N, C, H, W), 9).abs() + 0.5)
    s, t = torch.full((C,), 2.0), torch.full((C,), -0.25)
    gs, gp = rnd((N, C, H, W), 10), rnd((N, C, H // 2, W // 2), 11)
    out, partial = K.skip_pool_bwd(_sliced(gs, dtype), _sliced(gp, dtype), _sliced(y, dtype),
                                   _pro(AFFINE_RELU, s, t))
    assert float(out.float().abs().max()) == 0.0 and float(partial.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_skip_pool_backward_past_one_loop_trip(dtype):
    """The smallest class whose blocks stride: 32 channel-vector lanes leave 8 window lanes per
    block, the query caps the rows at 1024, so 91 x 91 = 8281 windows (of a 181 x 181 map: a
    trailing row and column) are 1024 rows and a second trip for the first 89 blocks."""
    C = 32 * _vec_of(dtype)
    got, g, gs, gp, rows = _sp_bwd_check(1, 181, 181, C, AFFINE_RELU, dtype)
    assert rows == 1024 and 91 * 91 > rows * 8
    assert _K().skip_pool_rows(dtype, 1, 2, 34, C) == 3   # (two rows need no second trip: 17 windows)


# ---------------------------------------------------------- functional.skip_pool behind a BatchNorm
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("missing", ["pool", "skip"], ids=["no_g_pool", "no_g_skip"])
@pytest.mark.parametrize("rows", [2048, 512], ids=["plain", "few_sample"])
def test_functional_skip_pool_behind_a_training_batchnorm(rows, missing, dtype, monkeypatch):
    F, K = _F(), _K()
    N, W, C = 2, 32, 16
    H = rows // (N * W)
    assert (rows > K.SMALL_BN_ROWS) == (rows == 2048)
    calls = []
    for name in ("skip_pool_bwd", "bn_bwd_finalize_p", "bn_bwd_small", "maxpool_bwd"):
        def spy(*a, _f=getattr(K, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(K, name, spy)
    monkeypatch.setattr(F, "_UNET_SKIP_POOL", "1")
    eps = 1e-5
    y = quant(rnd((N, C, H, W), 21) * 1.5 + 0.25, dtype)
    gam, bet = _general_affine(C, 22)
    gs, gp = quant(rnd((N, C, H, W), 23), dtype), quant(rnd((N, C, H // 2, W // 2), 24), dtype)
    bn = torch.nn.BatchNorm2d(C, eps=eps).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gam)
        bn.bias.copy_(bet)
    yd = to_dev_nhwc(y, dtype).requires_grad_()
    with torch.no_grad():  # the producer's statistics partials, as a conv epilogue leaves them
        yf = yd.double()
        part = torch.stack([yf.sum((0, 1, 2)), (yf * yf).sum((0, 1, 2))]).float().view(1, 2, C)
    act = F.Act(yd, F.finish_bn(bn, part, N * H * W, y=yd), relu=True)
    assert F._bn_backward_is_plain(act.bn) == (rows == 2048)
    buf = torch.full((N, H, W, 2 * C), float("nan"), dtype=dtype, device=DEV)
    skip, pooled = F.skip_pool(act, buf[..., :C])
    assert skip.data_ptr() == buf.data_ptr() and bool(torch.isnan(buf[..., C:]).all())

    yr = y.double().requires_grad_()
    ps = [p.double().requires_grad_() for p in (gam, bet)]
    a = torch.relu(TF.batch_norm(yr, None, None, ps[0], ps[1], True, 0.1, eps))
    assert_close(to_cpu_nchw(skip), a.detach(), dtype, "skip")
    # max_pool2d by ATen's rule on the STORED values: in bf16 about one window in a hundred holds
    # its maximum twice after the rounding, and the first one takes the gradient
    stored = to_cpu_nchw(skip)
    own, idx = TF.max_pool2d(stored, 2, return_indices=True)
    assert torch.equal(_bits(to_cpu_nchw(pooled)), _bits(own))
    p = a.flatten(2).gather(2, idx.flatten(2)).view(own.shape)
    assert_close(own, p.detach(), dtype, "pooled")
    if missing == "pool":
        skip.backward(to_dev_nhwc(gs, dtype))
        a.backward(gs.double())
    else:
        pooled.backward(to_dev_nhwc(gp, dtype))
        p.backward(gp.double())
    assert calls.count("skip_pool_bwd") == 1 and "maxpool_bwd" not in calls
    assert calls.count("bn_bwd_finalize_p") == (1 if rows == 2048 else 0)
    assert calls.count("bn_bwd_small") == (0 if rows == 2048 else 1)
    # (dx is the remainder of cancelling terms of the size of the incoming gradient)
    scale = max((gs if missing == "pool" else gp).abs().max().item() * gam.max().item()
                / (y.std().item() + eps), yr.grad.abs().max().item())
    assert_close(to_cpu_nchw(yd.grad), yr.grad, dtype, "dx", scale=scale, fac=5)
    assert_close(bn.weight.grad.cpu(), ps[0].grad, dtype, "dgamma", fac=20)
    assert_close(bn.bias.grad.cpu(), ps[1].grad, dtype, "dbeta", fac=20)


# ------------------------------------------------------------------------------ placed resize
PLACED = [((h, w), (dy, dx), (0, 0)) for (h, w) in [(1, 1), (2, 3), (6, 9), (17, 33)]
          for dy in (0, 1) for dx in (0, 1)] + [((6, 9), (3, 3), (1, 1))]


@functools.lru_cache(maxsize=None)
def _placed_case(hw, pad, place, C, mode, dtype):
    (h, w), (dy, dx), (top, left) = hw, pad, place
    N = 2
    x = quant(rnd((N, C, h, w), 31), dtype)
    s, t = _general_affine(C, 32)
    g = quant(rnd((N, C, 2 * h + dy, 2 * w + dx), 33), dtype)
    xr = x.double().requires_grad_()
    a = xr
    if mode:
        a = torch.relu(a * _c(s) + _c(t))
    up = TF.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True)
    out = TF.pad(up, [left, dx - left, top, dy - top])
    out.backward(g.double())
    return x, s, t, g, out.detach(), xr.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [NONE, AFFINE_RELU], ids=["plain", "affine_relu"])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("case", PLACED,
                         ids=lambda c: "%dx%d+%d+%d@%d,%d" % (c[0] + c[1] + c[2]))
def test_placed_resize_forward_and_backward(case, C, mode, dtype):
    K = _K()
    (h, w), (dy, dx), (top, left) = case
    x, s, t, g, ref, ref_dx = _placed_case(case[0], case[1], case[2], C, mode, dtype)
    N, Hd, Wd = x.shape[0], 2 * h + dy, 2 * w + dx
    xd = _sliced(x, dtype)
    obuf, o = _out_slice(N, Hd, Wd, C, dtype)
    out = K.bilinear_pad(xd, (2 * h, 2 * w), o, (top, left), _pro(mode, s, t))
    got = to_cpu_nchw(out)
    assert_close(got, ref, dtype, "placed resize")
    # the border is exactly zero inside the slice, and nothing outside the slice is touched
    border = torch.ones(Hd, Wd, dtype=torch.bool)
    border[top:top + 2 * h, left:left + 2 * w] = False
    assert float(got[:, :, border].abs().max()) == 0.0 if border.any() else True
    assert _pad_is_nan(obuf, C) and _pad_is_nan(xd._base, C)
    # backward: the gather reads the window alone — NaN outside it must not reach dx
    gw = g.clone()
    gw[:, :, border] = float("nan")
    gd = _sliced(gw, dtype)
    ga = K.bilinear_pad_bwd(gd, (h, w), (2 * h, 2 * w), (top, left))
    assert tuple(ga.shape) == (N, h, w, C) and bool(torch.isfinite(ga).all())
    if mode == NONE:
        assert_close(to_cpu_nchw(ga), ref_dx, dtype, "placed resize dx",
                     scale=max(ref_dx.abs().max().item(), 1e-3))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [NONE, AFFINE_RELU], ids=["plain", "affine_relu"])
@pytest.mark.parametrize("case", [((6, 9), (1, 1), (0, 0)), ((6, 9), (3, 3), (1, 1)),
                                  ((6, 9), (0, 0), (0, 0))],
                         ids=["pad_bottom_right", "pad_around", "no_pad"])
def test_functional_bilinear_placed(case, mode, dtype, monkeypatch):
    """Through autograd, the pending affine + ReLU included; a zero pad keeps the existing launch."""
    F, K = _F(), _K()
    (h, w), (dy, dx), (top, left) = case
    C = 8
    calls = []
    for name in ("bilinear_pad", "bilinear"):
        def spy(*a, _f=getattr(K, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(K, name, spy)
    x, s, t, g, ref, ref_dx = _placed_case(case[0], case[1], case[2], C, mode, dtype)
    N, Hd, Wd = x.shape[0], 2 * h + dy, 2 * w + dx
    xd = to_dev_nhwc(x, dtype).requires_grad_()
    bn = None
    if mode:  # an evaluation-mode BatchNorm (mean 0, invstd 1): dx = mask * scale * g
        sd, td = s.to(DEV), t.to(DEV)
        bn = F.BNState(sd.clone().requires_grad_(), td.clone().requires_grad_(),
                       torch.zeros(C, device=DEV), torch.ones(C, device=DEV), sd, td,
                       N * h * w, False)
    buf = torch.full((N, Hd, Wd, 2 * C), float("nan"), dtype=dtype, device=DEV)
    out = F.bilinear_placed(F.Act(xd, bn, relu=bool(mode)), (2 * h, 2 * w), buf[..., C:],
                            place=(top, left))
    assert calls == (["bilinear_pad"] if (dy or dx) else ["bilinear"])
    assert out.data_ptr() == buf[..., C:].data_ptr() and bool(torch.isnan(buf[..., :C]).all())
    assert_close(to_cpu_nchw(out), ref, dtype, "placed resize")
    out.backward(to_dev_nhwc(g, dtype))
    assert_close(to_cpu_nchw(xd.grad), ref_dx, dtype, "dx",
                 scale=max(ref_dx.abs().max().item(), 1e-3), fac=3 if mode else 1)


# ----------------------------------------------------------------- fused cross-entropy at factor 1
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_cross_entropy_at_factor_one(dtype):
    """UNet's logits are at full resolution: out_hw == lo.shape[1:3].  Loss and d lo against
    F.cross_entropy in float64, the bars of tests/test_loss_resize_gpu.py (loss 1e-5 relative in
    float32 storage, the gradient at assert_close's fac = 1)."""
    F = _F()
    N, Hi, Wi, C = 2, 9, 13, 19
    lo = quant(rnd((N, C, Hi, Wi), 41) * 2.0, dtype)
    g = torch.Generator().manual_seed(42)
    target = torch.randint(0, C, (N, Hi, Wi), generator=g)
    target[torch.rand(N, Hi, Wi, generator=g) < 0.15] = -1
    assert bool((target == -1).any())
    ref_in = lo.double().requires_grad_()
    ref = TF.cross_entropy(ref_in, target, ignore_index=-1)
    ref.backward(torch.tensor(1.7, dtype=torch.float64))
    vec = _vec_of(dtype)
    pitch = (C + 2 * vec - 1) // vec * vec
    lod = to_dev_nhwc(lo, dtype, pitch=pitch, off=0).requires_grad_()   # NaN behind the classes
    view = F.LogitsView(lod, (Hi, Wi), True)
    assert view._fusable(target.to(DEV), None, None, -1, None, "mean", 0.0)
    loss = TF.cross_entropy(view, target.to(DEV), ignore_index=-1)
    assert view._full is None   # the fused path, nothing materialised
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    (loss * 1.7).backward()
    assert tuple(lod.grad.shape) == (N, Hi, Wi, C)
    assert_close(to_cpu_nchw(lod.grad), ref_in.grad, dtype, "CE dlo at factor 1", fac=1.0)
