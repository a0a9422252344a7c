"""GPU parity of the register-sliding depthwise kernels (csrc/dwconv_slide.hip: every stride-1,
dilation-1 depthwise conv, forward and fused backward) at the edges their tricks depend on, each
against torch float64 (conv2d groups=C on the activated operand, autograd for dgrad / wgrad):

  * prologue modes 0 1 2 3 5 7 (compile-time instances) on both neighbour variants: three loads per
    row, or lane exchange + half-active buffer loads for maps of >= 30 MiB (`slide_exchange`);
  * the strip / column-block / channel-block geometry of `slide_geom` / `sl_thread`: heights where
    H / 8 is 0 or 1, ragged last strips, widths of 1-4 live columns per wave, partly mirrored
    column and channel blocks, one strip spanning a tall map;
  * more than 1024 partial rows (N * ceil(W / 16) > 1024) and the host path that finishes them;
  * channel slices in and out (NaN around them), pitches the vector accesses cannot take;
  * activated values exactly at the ReLU / ReLU6 mask boundaries (0, -0, 6);
  * the finalize kernels behind the fused backward, on their own.

Every output the sliding path produces is checked: y (into a NaN-prefilled `out=`) and its
statistics partials; the fused backward's masked g, dW (tap-major and torch layout) and
BatchNorm-backward partials; the fused-add (res) instance.  Bars as tests/test_ops_gpu.py:
2e-5 (fp32) / 6e-3 (bf16) of the max, the same `fac` for sums."""
import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
NAN = float("nan")


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def F():
    from segmentron_amd import functional
    return functional


def _esize(dtype):
    return 2 if dtype == torch.bfloat16 else 4


def _xchg(N, H, W, C, dtype):
    """slide_exchange: neighbour columns by lane exchange on maps of at least 30 MiB."""
    return N * H * W * C * _esize(dtype) >= (30 << 20)


def _slide_geom(N, H, W, C):
    """slide_geom -> (rows per strip, strips, column blocks)."""
    ncblk, nwblk = (C // 4 + 15) // 16, (W + 15) // 16
    ns = (H + 21) // 43
    per_strip = N * nwblk * ncblk
    ns = max(ns, (400 + per_strip - 1) // per_strip)
    ns = min(ns, H // 8, 1024 // (N * nwblk))
    ns = max(ns, 1)
    rs = (H + ns - 1) // ns
    return rs, (H + rs - 1) // rs, nwblk


def _rows(N, H, W, C):
    _, ns, nwblk = _slide_geom(N, H, W, C)
    return N * ns * nwblk


def _grid_y(dtype, N, H, W, C, kind):
    return K().LIB.query("seg_dwconv_grid_y", K()._DT[dtype], C, N, H, W, 1, 1, kind)


def _act_ref(x, mode, scale, shift):
    if mode & 2:
        x = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if mode & 1:
        x = torch.relu(x)
    if mode & 4:  # ReLU6
        x = x.clamp(max=6.0)
    return x


def _pro(mode, c, seed, ties=False):
    if not (mode & 2):
        return (mode, None, None), None, None
    g = torch.Generator().manual_seed(seed)
    if ties:
        # exact in fp32 fma: grid points (multiples of 0.5) land exactly on 0 and 6, e.g.
        # scale 2 / shift -1 maps 0.5 -> 0 and 3.5 -> 6, scale 0.5 / shift 2 maps -4 -> 0, 8 -> 6
        s = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g)]
        t = torch.tensor([-1.0, 0.0, 1.0, 2.0])[torch.randint(0, 4, (c,), generator=g)]
    else:
        s = torch.rand(c, generator=g) + 0.5
        t = rnd((c,), seed + 1, 0.3)
    return (mode, s.to(DEV), t.to(DEV)), s, t


def _ties_input(shape, seed):
    """multiples of 0.5 in [-8, 8] (bf16-exact), half of the zeros negative"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-16, 17, shape, generator=g).float() * 0.5
    neg = torch.rand(shape, generator=g) < 0.5
    return torch.where((x == 0) & neg, torch.full_like(x, -0.0), x)


def _check(N, H, W, C, mode, dtype, sl=False, ties=False, seed=1):
    """Forward (+ statistics), stride-1 data gradient, fused backward (both weight layouts) and
    the fused-add backward of one geometry against float64; returns the number of checks run."""
    vec = 8 if dtype == torch.bfloat16 else 4
    shape = (N, C, H, W)
    x = _ties_input(shape, seed) if ties else quant(rnd(shape, seed), dtype)
    w = rnd((C, 1, 3, 3), seed + 1, 0.4)
    pro, s, t = _pro(mode, C, seed + 2, ties)
    xa = _act_ref(x, mode, s, t).double().requires_grad_()
    wd = w.double().requires_grad_()
    ref = TF.conv2d(xa, wd, None, 1, 1, 1, groups=C)
    dy = quant(rnd(shape, seed + 3), dtype)
    ref.backward(dy.double())
    r = ref.detach()
    act = xa.detach()
    # hardtanh's mask: the gradient passes strictly inside (0, 6)
    mask = ((act > 0) & ((act < 6) if (mode & 4) else torch.ones_like(act, dtype=torch.bool))).double() \
        if (mode & 1) else torch.ones_like(act)
    gref = xa.grad * mask
    if ties and (mode & 1):  # the point of the inputs: many activated values exactly on the boundary
        assert (act == 0).sum() > 0.05 * act.numel()
        if mode & 4:
            assert (act == 6).sum() > 0.01 * act.numel()
    pad = dict(pitch=C + 16, off=8) if sl else {}
    xd = to_dev_nhwc(x, dtype, **pad)
    dyd = to_dev_nhwc(dy, dtype, **pad)
    w9c = w.view(C, 9).t().contiguous().to(DEV)
    w4 = w.to(DEV)
    rows = _rows(N, H, W, C)
    assert _grid_y(dtype, N, H, W, C, 0) == rows and _grid_y(dtype, N, H, W, C, 1) == rows
    sfac = 5 if dtype == torch.float32 else 60
    bfac = 5 if dtype == torch.float32 else 300
    n = 0
    if C % vec == 0:  # the forward entry takes whole vectors of the storage dtype
        P, off = (C + 2 * vec, vec) if sl else (C, 0)
        full = torch.full((N, H, W, P), NAN, dtype=dtype, device=DEV)
        out = full[..., off:off + C]
        y, partial = K().dwconv(xd, w9c, 1, 1, pro, out=out, want_stats=True)
        assert y.data_ptr() == out.data_ptr() and partial.shape[0] == rows
        assert_close(to_cpu_nchw(y), r, dtype, "slide y")  # (a skipped element stays NaN)
        if sl:  # nothing outside the slice was touched
            assert torch.isnan(full[..., :off].float()).all()
            assert torch.isnan(full[..., off + C:].float()).all()
        sums = K().colsum(partial.view(rows, -1)).cpu()
        assert_close(sums[:C], r.sum((0, 2, 3)), torch.float32, "slide sum",
                     scale=r.abs().sum((0, 2, 3)).max().item(), fac=sfac)
        assert_close(sums[C:], (r * r).sum((0, 2, 3)), torch.float32, "slide sumsq", fac=sfac)
        # torch's [C,1,3,3] parameter as is: the same taps in the same order
        y4, _ = K().dwconv(xd, w4, 1, 1, pro)
        assert torch.equal(y4, y)
        # stride-1 data gradient = the forward kernel with the taps reversed in the kernel
        g = K().dwconv_dgrad(dyd, w4, 1, 1, (H, W))
        assert_close(to_cpu_nchw(g), xa.grad, dtype, "slide dgrad")
        n += 2
    gf, dWf, pb = K().dwconv_bwd_fused(xd, dyd, w9c, 1, pro, want_bn=True)
    assert pb.shape[0] == rows
    assert_close(to_cpu_nchw(gf), gref, dtype, "fused g")
    assert_close(dWf.t().reshape(C, 1, 3, 3).cpu(), wd.grad, torch.float32, "fused dW", fac=20)
    sums = K().colsum(pb).cpu()
    gx = gref * x.double()
    assert_close(sums[:C], gref.sum((0, 2, 3)), torch.float32, "fused sum g",
                 scale=gref.abs().sum((0, 2, 3)).max().item(), fac=bfac)
    assert_close(sums[C:], gx.sum((0, 2, 3)), torch.float32, "fused sum gx",
                 scale=gx.abs().sum((0, 2, 3)).max().item(), fac=bfac)
    g4, dW4, pb4 = K().dwconv_bwd_fused(xd, dyd, w4, 1, pro, want_bn=True, torch_layout=True)
    assert torch.equal(g4, gf) and torch.equal(pb4, pb)
    assert_close(dW4.cpu(), wd.grad, torch.float32, "fused dW torch layout", fac=20)
    n += 1
    if C % vec == 0:  # fused-add instance (RES): the entry takes whole vectors
        res = quant(rnd(shape, seed + 4), dtype)
        resd = to_dev_nhwc(res, dtype, **pad)
        gr, dWr, pbr = K().dwconv_bwd_fused(xd, dyd, w4, 1, pro, want_bn=True, torch_layout=True,
                                            res=resd)
        # one rounding of (masked dgrad + res); weight / BatchNorm sums of the masked part only
        assert_close(to_cpu_nchw(gr), gref + res.double(), dtype, "fused+res g")
        assert torch.equal(dWr, dW4) and torch.equal(pbr, pb)
        n += 1
    return n


# ------------------------------------------------------------------------ prologue x variant
# One map per dtype below the exchange threshold, one above it.  (2, 100, 601, 72) is 8.65 M
# elements: 34.6 MB in fp32 (exchange), 17.3 MB in bf16 (three loads); (2, 151, 771, 72) is
# 16.8 M elements, 33.5 MB in bf16: the bf16 exchange kernels.  72 channels = 18 quads: the
# second channel block holds 2 live quads; odd widths: a partly mirrored last column block;
# three / four strips with a ragged last one.
MODES = [0, 1, 2, 3, 5, 7]
BELOW = (2, 45, 37, 72)
ABOVE = {torch.float32: (2, 100, 601, 72), torch.bfloat16: (2, 151, 771, 72)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("xchg", [False, True], ids=["loads", "exchange"])
@pytest.mark.parametrize("mode", MODES)
def test_slide_prologue_modes_on_both_neighbour_variants(mode, xchg, dtype):
    geom = ABOVE[dtype] if xchg else BELOW
    assert _xchg(*geom, dtype) == xchg
    assert _check(*geom, mode, dtype, sl=True, seed=10 + mode) == 4


# --------------------------------------------------------------------------- geometry edges
GEOM_CASES = [
    # N, H, W, C, mode
    # heights: H / 8 = 0 or 1 (one strip), and a ragged last strip (6 strips of 9 rows + 5)
    (1, 1, 20, 64, 3),
    (2, 2, 17, 64, 1),
    (1, 7, 65, 64, 7),
    (2, 8, 16, 64, 0),
    (1, 9, 63, 64, 5),
    (1, 50, 20, 64, 2),
    # widths: 1 / 2 live columns (the rest of the wave mirrors them), 15 / 16 / 17 (one column of
    # a second block), 20, 63, 65
    (2, 13, 1, 64, 3),
    (1, 11, 2, 64, 1),
    (1, 12, 15, 64, 0),
    (1, 10, 16, 64, 7),
    (2, 9, 65, 64, 2),
    # channels: one live quad of 16, 15 quads, a ragged second block (fp32 forward; bf16 takes
    # only the fused backward: C % 8 != 0)
    (1, 19, 33, 4, 3),
    (2, 10, 20, 60, 7),
    (1, 24, 65, 68, 1),
    # bf16 backward with C = 4 (mod 8)
    (2, 9, 17, 12, 3),
    (1, 16, 21, 20, 5),
    # one strip of 120 rows (N * ceil(W / 16) = 513: strip cap 1); 31.49 MB in fp32 (exchange),
    # 15.7 MB in bf16 (three loads)
    (1, 120, 8200, 8, 3),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", GEOM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_slide_geometry_edges(case, dtype):
    N, H, W, C, mode = case
    rs, ns, _ = _slide_geom(N, H, W, C)
    if (N, H, W, C) == (1, 50, 20, 64):
        assert ns > 1 and H % rs != 0
    if W == 8200:
        assert ns == 1 and rs == H and _xchg(N, H, W, C, torch.float32)
    _check(N, H, W, C, mode, dtype, sl=(H % 2 == 1), seed=20 + H)


# ------------------------------------------------------------------ more than 1024 partial rows
# (2, 9, 8192, 8): N * 512 column blocks = 1024 rows, the last geometry on the one-launch finalize;
# (2, 9, 8200, 8): 1026 rows; (33, 10, 513, 64): 33 * 33 = 1089 rows, 10.8 M elements: exchange in
# fp32 (43 MB), three loads in bf16 (21.7 MB).  All of them one strip per image.
ROW_CASES = [(2, 9, 8192, 8, 3), (2, 9, 8200, 8, 7), (33, 10, 513, 64, 1)]


def _rows_written(dtype, N, H, W, C, mode):
    """Launch the sliding forward and fused backward on partial buffers two rows longer than
    seg_dwconv_grid_y says, NaN-filled: -> (grid_y, rows the forward wrote, rows the backward
    wrote to each of its two partials).  A launch writes every one of its rows."""
    L = K().LIB
    x = torch.randn(N, H, W, C, device=DEV).to(dtype)
    dy = torch.randn(N, H, W, C, device=DEV).to(dtype)
    w = torch.randn(9, C, device=DEV)
    (m, sc, sh), _, _ = _pro(mode, C, 5)
    gy0, gy1 = _grid_y(dtype, N, H, W, C, 0), _grid_y(dtype, N, H, W, C, 1)
    pf = torch.full((gy0 + 2, 2, C), NAN, device=DEV)
    y = torch.empty_like(x)
    L.call("seg_dwconv3x3", K()._DT[dtype], 0, K()._p(x), C, N, H, W, C, K()._p(w), 0, 1, 1, m,
           K()._p(sc), K()._p(sh), K()._p(y), C, H, W, K()._p(pf), gy0, K()._stream())
    pw = torch.full((gy1 + 2, 9 * C), NAN, device=DEV)
    pb = torch.full((gy1 + 2, 2 * C), NAN, device=DEV)
    g = torch.empty_like(x)
    L.call("seg_dwconv3x3_bwd_fused", K()._DT[dtype], K()._p(dy), C, K()._p(x), C, N, H, W, C,
           K()._p(w), 0, 1, m, K()._p(sc), K()._p(sh), K()._p(g), C, K()._p(pw), K()._p(pb), gy1,
           K()._stream())

    def written(p):
        fin = torch.isfinite(p.view(p.shape[0], -1)).all(1).cpu()
        nan = torch.isnan(p.view(p.shape[0], -1)).all(1).cpu()
        k = int(fin.sum())
        assert fin[:k].all() and nan[k:].all(), "partial rows written out of order"
        return k
    return gy0, gy1, written(pf), written(pw), written(pb)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_slide_more_than_1024_partial_rows(case, dtype):
    N, H, W, C, mode = case
    rows = _rows(N, H, W, C)
    assert rows == (1024 if W == 8192 else N * ((W + 15) // 16)) and _slide_geom(N, H, W, C)[1] == 1
    gy0, gy1, rf, rw, rb = _rows_written(dtype, N, H, W, C, mode)
    assert gy0 == gy1 == rows and rf == rw == rb == rows
    _check(N, H, W, C, mode, dtype, seed=30 + C)


@pytest.mark.parametrize("W", [8192, 8200], ids=["1024rows", "1026rows"])
def test_dwconv_bn_module_with_pending_batchnorm_finishes_any_row_count(W, monkeypatch):
    """functional.dwconv_bn on an input with a training BatchNorm + ReLU pending, followed by a
    training BatchNorm: forward and backward against float64 autograd of
    BN(train) -> ReLU -> depthwise -> BN(train).  At <= 1024 partial rows _DwFn.backward
    finishes the weight gradient and the BatchNorm backward in one launch (dw_bwd_finalize); above
    it (one strip per image, N * ceil(W / 16) rows) in two (dw_wgrad_finalize +
    bn_bwd_finalize_p): both routes are asserted."""
    N, H, C, dtype = 2, 9, 8, torch.float32
    eps = 1e-5
    rows = _grid_y(dtype, N, H, W, C, 1)
    assert rows == _rows(N, H, W, C) and (rows > 1024) == (W == 8200)
    calls = []
    for name in ("dw_bwd_finalize", "dw_wgrad_finalize", "bn_bwd_finalize_p"):
        def spy(*a, _f=getattr(K(), name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(K(), name, spy)
    x = rnd((N, C, H, W), 41) * 1.5 + 0.5
    w = rnd((C, 1, 3, 3), 42, 0.4)
    gen = torch.Generator().manual_seed(43)
    g0, b0 = torch.rand(C, generator=gen) + 0.5, rnd((C,), 44, 0.3)
    g1, b1 = torch.rand(C, generator=gen) + 0.5, rnd((C,), 45, 0.3)
    dy = rnd((N, C, H, W), 46)

    bn0 = torch.nn.BatchNorm2d(C, eps=eps).to(DEV).train()
    bn1 = torch.nn.BatchNorm2d(C, eps=eps).to(DEV).train()
    conv = torch.nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False).to(DEV)
    with torch.no_grad():
        for p, v in ((bn0.weight, g0), (bn0.bias, b0), (bn1.weight, g1), (bn1.bias, b1),
                     (conv.weight, w)):
            p.copy_(v)
    xd = to_dev_nhwc(x, dtype).requires_grad_()
    with torch.no_grad():  # the producer's statistics partials, as a conv epilogue leaves them
        xf = xd.double()
        part = torch.stack([xf.sum((0, 1, 2)), (xf * xf).sum((0, 1, 2))]).float().view(1, 2, C)
    act = F().Act(xd, F().finish_bn(bn0, part, N * H * W, y=xd), relu=True)
    out = F().materialize(F().dwconv_bn(act, conv, bn1))
    out.backward(to_dev_nhwc(dy, dtype))
    # (the trailing BatchNorm's own backward, _ApplyFn, takes bn_bwd_finalize_p in both cases)
    if rows > 1024:
        assert "dw_bwd_finalize" not in calls and calls.count("dw_wgrad_finalize") == 1 \
            and calls.count("bn_bwd_finalize_p") == 2, calls
    else:
        assert calls.count("dw_bwd_finalize") == 1 and "dw_wgrad_finalize" not in calls \
            and calls.count("bn_bwd_finalize_p") == 1, calls

    xr = x.double().requires_grad_()
    ps = [p.double().requires_grad_() for p in (g0, b0, w, g1, b1)]
    a = torch.relu(TF.batch_norm(xr, None, None, ps[0], ps[1], True, 0.1, eps))
    z = TF.conv2d(a, ps[2], None, 1, 1, 1, groups=C)
    o = TF.batch_norm(z, None, None, ps[3], ps[4], True, 0.1, eps)
    o.backward(dy.double())
    assert_close(to_cpu_nchw(out), o.detach(), dtype, "dwconv_bn y")
    assert_close(to_cpu_nchw(xd.grad), xr.grad, dtype, "dwconv_bn dx", fac=5)
    for got, p, what in ((bn0.weight, ps[0], "dgamma0"), (bn0.bias, ps[1], "dbeta0"),
                         (conv.weight, ps[2], "dW"), (bn1.weight, ps[3], "dgamma1"),
                         (bn1.bias, ps[4], "dbeta1")):
        assert_close(got.grad.cpu(), p.grad, dtype, "dwconv_bn " + what, fac=20)


# ------------------------------------------------------------------------- pitches and slices
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_slide_pitch_off_the_vector_width_is_reported_not_launched(dtype):
    N, H, W, C = 1, 9, 20, 16
    x = rnd((N, C, H, W), 50)
    xd = to_dev_nhwc(x, dtype, pitch=C + 2)  # rows of C + 2 elements: not a 4-channel vector
    dy = to_dev_nhwc(rnd((N, C, H, W), 51), dtype)
    w = rnd((C, 1, 3, 3), 52).to(DEV)
    out = torch.full((N, H, W, C), NAN, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError, match="multiples"):
        K().dwconv(xd, w, 1, 1, (1, None, None), out=out)
    with pytest.raises(RuntimeError, match="multiples"):
        K().dwconv_bwd_fused(xd, dy, w, 1, (1, None, None), want_bn=True)
    with pytest.raises(RuntimeError, match="multiples"):
        K().dwconv_bwd_fused(dy, xd, w, 1, (1, None, None), want_bn=True)
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()  # nothing was launched
    # ... and the device is fine: the same op on a valid pitch
    _check(N, H, W, C, 1, dtype, sl=True, seed=53)


# -------------------------------------------------------------------------------- mask ties
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [1, 3, 5, 7])
def test_slide_mask_at_exact_relu_and_relu6_boundaries(mode, dtype):
    """Activated values exactly 0 (also from -0 inputs: bf16 ReLU on the raw storage words) and
    exactly 6: the gradient passes strictly inside (0, 6), as hardtanh's."""
    for geom in [(2, 20, 37, 72), (1, 9, 17, 8)]:
        _check(*geom, mode, dtype, ties=True, seed=60 + mode)


# ------------------------------------------------------------------------- finalize kernels
@pytest.mark.parametrize("R", [1, 7, 1024, 1025, 5000])
def test_dw_wgrad_finalize_sums_partials_in_torch_layout(R):
    C = 44  # 9 C = 396 columns: a partial last block of 8
    pw = rnd((R, 9 * C), 70 + R)
    dW = K().dw_wgrad_finalize(pw.to(DEV), C).cpu()
    ref = pw.double().view(R, 9, C).sum(0).t().reshape(C, 1, 3, 3)
    assert_close(dW, ref, torch.float32, "dw_wgrad_finalize")


@pytest.mark.parametrize("Rb", [1, 1024, 1025])
def test_dw_bwd_finalize_against_float64(Rb):
    C, Rw = 44, 300
    count = float(Rb * 37)
    pb = rnd((Rb, 2 * C), 80)
    pw = rnd((Rw, 9 * C), 81)
    mean = rnd((C,), 82)
    gen = torch.Generator().manual_seed(83)
    invstd = torch.rand(C, generator=gen) + 0.5
    gamma = torch.rand(C, generator=gen) + 0.5
    args = (pb.to(DEV), pw.to(DEV), count, mean.to(DEV), invstd.to(DEV), gamma.to(DEV))
    if Rb > 1024:  # the one-launch kernel reduces at most 1024 rows: a reported error
        with pytest.raises(RuntimeError, match="dw_bwd_finalize"):
            K().dw_bwd_finalize(*args)
        return
    dgamma, dbeta, c0, c1, dW = K().dw_bwd_finalize(*args)
    # bn_bwd_finalize_p's definitions
    sg, sgx = pb[:, :C].double().sum(0), pb[:, C:].double().sum(0)
    mu, ist, gm = mean.double(), invstd.double(), gamma.double()
    dg = (sgx - mu * sg) * ist
    s = gm * ist
    c1r = s * (dg / count) * ist
    c0r = s * (sg / count) - c1r * mu
    assert_close(dgamma.cpu(), dg, torch.float32, "dgamma")
    assert_close(dbeta.cpu(), sg, torch.float32, "dbeta")
    assert_close(c0.cpu(), c0r, torch.float32, "c0")
    assert_close(c1.cpu(), c1r, torch.float32, "c1")
    assert_close(dW.cpu(), pw.double().view(Rw, 9, C).sum(0).t().reshape(C, 1, 3, 3),
                 torch.float32, "dw_bwd_finalize dW")
