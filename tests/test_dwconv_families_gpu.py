"""GPU parity of the three depthwise 3x3 kernel families behind the register-sliding kernels, at the
edges their launch code depends on, each against torch float64 (conv2d groups=C on the activated
operand, autograd for the data / weight gradients; nine shifted multiply-adds above 4 M elements):

  * LDS-tiled, dilation 2 (csrc/dwconv_tiled.hip): forward, stride-1 data gradient (flipped
    taps), separate weight gradient, fused backward — the remainder tiling of `tiled_geom`
    (2 x 64 bottom strips, 32 x 4 right strips, the corner they share), forward and backward on
    different tilings, persistent blocks with remainder tiles behind the 8 x 16 ones;
  * row-chain, dilation 3..64 (csrc/dwconv_row.hip): forward and fused backward — several
    segments per row, a ragged last segment, a block walking a second chain, a dilation at or
    beyond the map, both ends of the family (dilation 3, 64) and the strip fallback behind it
    (dilation 65, csrc/dwconv.hip);
  * stride 2 (dwconv_tiled_s2_kernel forward, csrc/dwconv_s2.hip fused backward; data and weight
    gradient on the strip fallback): the smallest maps, exact and ragged tiles, persistent blocks.

For every geometry `_check` compares every output the family produces: y (into a NaN-prefilled
`out=` slice) and its statistics partials; the data gradient; the separate weight gradient; the
fused backward's masked g, dW and BatchNorm-backward partials, in both weight layouts where the
kernel takes torch's [C,1,3,3]; optionally with every tensor a channel slice of a NaN-filled wider
buffer.  Every launch that writes partial rows is repeated on buffers two rows longer than the
grid query says, NaN-filled: exactly the first grid_y rows are written.  Python mirrors of the
host geometry (`tiled_geom`, `row_geom`, the grid caps) are asserted against the grid queries, and
each case asserts the geometric property it exists for: a retuned tile size or cap fails here
instead of silently testing nothing.

Bars as tests/test_ops_gpu.py: 2e-5 (fp32) / 6e-3 (bf16) of the max for y and g; `fac` 5 / 60
for the forward sums, 5 / 300 for the BatchNorm-backward sums, 20 for the fused dW, 20 / 100 for
the separate weight gradient.  Two of them widen, by a rule written down in `_check`, on the cases
where a CPU emulation of the kernels' one bf16 rounding of the staged operand is itself over the
bar: the forward sums of three maps of a few pixels, and the bf16 LDS-tiled weight gradient of
two shapes (figures in `_check`)."""
import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc
from test_dwconv_slide_gpu import _act_ref, _pro, _ties_input

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
NAN = float("nan")
MODES = [0, 1, 2, 3, 5, 7]
F32, BF16 = torch.float32, torch.bfloat16
# assert_close `fac` of the two weight gradients (shared with tests/test_dw_backward_gpu.py)
FUSED_DW_FAC = 20
WGRAD_FAC = {F32: 20, BF16: 100}


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def _cdiv(a, b):
    return (a + b - 1) // b


def _vec(dtype):
    return 8 if dtype == BF16 else 4


# ----------------------------------------------------------------------------- host mirrors
def _tiled_geom(N, H, W, rem, rem_pct=0):
    """tiled_geom (csrc/dwconv_tiled.hip): 8 x 16 tiles, with `rem` a ragged last tile row of at
    most 2 image rows / tile column of at most 4 image columns replaced by 2 x 64 bottom strips /
    32 x 4 right strips where that saves at least rem_pct percent of the classic tile count."""
    full_h, full_w, rb, rr = H // 8, W // 16, H % 8, W % 16
    th, tw = _cdiv(H, 8), _cdiv(W, 16)
    use_b = rem and 0 < rb <= 2 and full_h > 0
    use_c = rem and 0 < rr <= 4 and full_w > 0
    if use_b or use_c:
        hc = full_h * 8 if use_b else H
        now = (full_h if use_b else th) * (full_w if use_c else tw) \
            + (_cdiv(W, 64) if use_b else 0) + (_cdiv(hc, 32) if use_c else 0)
        if (th * tw - now) * 100 < rem_pct * th * tw:
            use_b = use_c = False
    g = dict(tiles_h=full_h if use_b else th, tiles_w=full_w if use_c else tw,
             hb0=full_h * 8, wc0=full_w * 16, hc=full_h * 8 if use_b else H)
    g["nb"] = _cdiv(W, 64) if use_b else 0
    g["nc"] = _cdiv(g["hc"], 32) if use_c else 0
    g["ntiles_a"] = N * g["tiles_h"] * g["tiles_w"]
    g["ntiles"] = g["ntiles_a"] + N * (g["nb"] + g["nc"])
    return g


def _tiled_grid(dtype, C, N, H, W, kind):
    """dw_tiled_grid_y -> (geometry, grid_y); kind 0 forward / data gradient, 1 fused backward
    (4-channel vectors, remainder tiles only for a 6 % saving), 2 weight gradient (classic)."""
    g = _tiled_geom(N, H, W, kind != 2, 6 if kind == 1 else 0)
    gx = _cdiv(C // 4 if kind == 1 else C // _vec(dtype), 8)
    cap = max((2048, 512, 768)[kind] // gx, 1)
    return g, min(g["ntiles"], cap)


def _row_geom(dtype, W, dil):
    """row_geom (csrc/dwconv_row.hip) -> (TW, ntw): equal segments of at most 160 pixels whose
    three-row ring (TW + 2 dil pixels x 32 channels) fits 120 KiB of LDS."""
    px = 3 * 32 * (2 if dtype == BF16 else 4)
    ntw = _cdiv(W, 160)
    while True:
        TW = _cdiv(W, ntw)
        if (TW + 2 * dil) * px <= 120 * 1024 or TW == 1:
            return TW, ntw
        ntw += 1


def _row_grid(dtype, C, N, H, W, dil):
    """dw_row_grid_y -> (chains, grid_y): one chain per (image, phase < min(dil, H), segment)."""
    chains = N * min(dil, H) * _row_geom(dtype, W, dil)[1]
    return chains, min(chains, max(768 // _cdiv(C, 32), 1))


def _strip_grid_y(dtype, C, N, Ho, Wo):
    """the strip kernels of csrc/dwconv.hip (seg_dwconv_grid_y's last branch)"""
    CV = C // _vec(dtype)
    lg = max((5, 4, 3), key=lambda b: (CV / (_cdiv(CV, 1 << b) << b), b))  # ties -> wider
    spb = 256 >> lg
    return min(_cdiv(N * Ho * _cdiv(Wo, 4), spb), max(1536 // _cdiv(CV, 1 << lg), 1))


def _s2_fwd_grid(dtype, C, N, Ho, Wo):
    """dw_tiled_s2_grid_y -> (tiles, grid_y): 4 x 16 OUTPUT pixels per tile"""
    tiles = N * _cdiv(Ho, 4) * _cdiv(Wo, 16)
    return tiles, min(tiles, max(2048 // _cdiv(C // _vec(dtype), 8), 1))


def _s2_bwd_grid(C, N, H, W):
    """s2_grid_y (csrc/dwconv_s2.hip) -> (tiles, grid_y): 8 x 16 INPUT pixels per tile"""
    tiles = N * _cdiv(H, 8) * _cdiv(W, 16)
    return tiles, min(tiles, max(768 // _cdiv(C // 4, 8), 1))


def _grid_y_mirror(dtype, C, N, H, W, stride, dil, kind):
    """seg_dwconv_grid_y for the families of this file; H x W: the input size"""
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    if stride == 1 and dil <= 2:
        assert dil == 2 or kind == 2  # (dilation 1: only the weight gradient is still tiled)
        return _tiled_grid(dtype, C, N, H, W, kind)[1]
    if stride == 2 and kind == 0:
        return _s2_fwd_grid(dtype, C, N, Ho, Wo)[1]
    if stride == 1 and 3 <= dil <= 64 and kind in (0, 1):
        return _row_grid(dtype, C, N, H, W, dil)[1]
    return _strip_grid_y(dtype, C, N, Ho, Wo)


def _grid_y(dtype, C, N, H, W, stride, dil, kind):
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    return K().LIB.query("seg_dwconv_grid_y", K()._DT[dtype], C, N, Ho, Wo, stride, dil, kind)


# ------------------------------------------------------------------------------- references
def _ref_autograd(xa, w, dy, stride, dil):
    xa = xa.clone().requires_grad_()
    w = w.clone().requires_grad_()
    y = TF.conv2d(xa, w, None, stride, dil, dil, groups=xa.shape[1])
    y.backward(dy)
    return y.detach(), xa.grad, w.grad


def _ref_shifted(xa, w, dy, stride, dil):
    """the same three float64 results by nine shifted multiply-adds (no im2col, no autograd)"""
    N, C, H, W = xa.shape
    Ho, Wo = dy.shape[2:]
    xp = TF.pad(xa, (dil, dil, dil, dil))
    y = torch.zeros_like(dy)
    gp = torch.zeros_like(xp)
    dw = torch.zeros_like(w)
    for kh in range(3):
        for kw in range(3):
            sl = (slice(None), slice(None),
                  slice(kh * dil, kh * dil + stride * (Ho - 1) + 1, stride),
                  slice(kw * dil, kw * dil + stride * (Wo - 1) + 1, stride))
            wk = w[:, 0, kh, kw].view(1, C, 1, 1)
            y += xp[sl] * wk
            gp[sl] += dy * wk
            dw[:, 0, kh, kw] = (xp[sl] * dy).sum((0, 2, 3))
    return y, gp[:, :, dil:dil + H, dil:dil + W].contiguous(), dw


def test_shifted_reference_is_the_autograd_reference():
    for (N, H, W, C, stride, dil) in [(2, 9, 11, 5, 1, 2), (1, 5, 7, 3, 1, 12), (2, 9, 12, 4, 2, 1),
                                      (1, 1, 1, 2, 2, 1)]:
        xa, w = rnd((N, C, H, W), 1).double(), rnd((C, 1, 3, 3), 2).double()
        dy = rnd((N, C, (H + stride - 1) // stride, (W + stride - 1) // stride), 3).double()
        for a, b in zip(_ref_autograd(xa, w, dy, stride, dil), _ref_shifted(xa, w, dy, stride, dil)):
            assert a.shape == b.shape and (a - b).abs().max() <= 1e-13 * max(a.abs().max(), 1.0)


def _nerr(got, ref, scale=None):
    """max-normalised error in units of 2e-5 (assert_close's `fac`)"""
    s = max(ref.abs().max().item() if scale is None else scale, 1e-12)
    return (got.double() - ref).abs().max().item() / s / 2e-5


def _emu_fac(fac, emu, ref, scale=None):
    """`fac`, unless the bf16 emulation of the kernel's operand rounding (`emu`) alone is further
    than that from the float64 reference: then twice the emulated error (see _check)."""
    if emu is None:
        return fac
    e = _nerr(emu, ref, scale)
    return fac if e <= fac else 2 * e


def _written(p):
    """rows of a NaN-prefilled partial buffer a launch wrote: whole rows, from the first on"""
    p = p.view(p.shape[0], -1)
    fin, nan = torch.isfinite(p).all(1).cpu(), torch.isnan(p).all(1).cpu()
    k = int(fin.sum())
    assert fin[:k].all() and nan[k:].all(), "partial rows written in part or out of order"
    return k


# ------------------------------------------------------------------------------------ check
def _check(N, H, W, C, stride, dil, mode, dtype, sl=False, ties=False, seed=1):
    """Every output of one geometry against float64: forward (+ statistics), data gradient,
    separate weight gradient, fused backward (g, dW, BatchNorm-backward partials), the partial
    rows each launch owns, the grid queries against the host mirrors.

    One bar is not a constant.  bf16 with an affine prologue: the kernels that park the activated
    operand in LDS (every forward here but the strip fallback; the LDS-tiled weight gradient)
    round it to bf16 once, 2^-9 relative per term (oracle/bf16_emulation.py), which the float64
    reference does not.  A CPU emulation of that one rounding (float64 otherwise) predicts the
    kernels' error to the digit; measured on an MI355X, in units of 2e-5 (kernel = emulation):
      * forward sums, `fac` 60: the error of a sum over n output pixels averages out as
        1 / sqrt(n), so the bar holds from a few dozen pixels per channel on and misses below:
        stride 2, 1 x 1 x 1: sum 144.9, sum of squares 289.3; 2 x 2 x 3: 48.7 / 94.3; dilation 2,
        2 x 5 x 3: 32.8 / 80.6.  Every larger map is inside (at most 56.4, 1 x 9 x 33 in mode 7).
      * LDS-tiled weight gradient, `fac` 100: its error does NOT shrink with n relative to its
        max (both grow as sqrt(n): dy has random sign) and sits at 75 - 123 at every size:
        2 x 65 x 129 x 72 in mode 2: 123.2, 1 x 65 x 129 x 1024 in mode 3: 100.7; inside: 93.1
        (2 x 41 x 50 x 512), 83.7, 80.8, 79.3, 79.0, 76.0, 75.8, 75.3.
    Where the emulated error alone is over the usual bar, the bar is twice the emulated error;
    everywhere else it is the usual one.  It is computed from the inputs on the CPU, never from
    the kernel's output."""
    vec = _vec(dtype)
    assert C % vec == 0
    tiled = stride == 1 and dil <= 2  # takes torch's [C,1,3,3] as is
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    shape, oshape = (N, C, H, W), (N, C, Ho, Wo)
    x = _ties_input(shape, seed) if ties else quant(rnd(shape, seed), dtype)
    w = rnd((C, 1, 3, 3), seed + 1, 0.4)
    pro, s, t = _pro(mode, C, seed + 2, ties)
    dy = quant(rnd(oshape, seed + 3), dtype)
    act = _act_ref(x, mode, s, t).double()
    ref = _ref_shifted if x.numel() > (4 << 20) else _ref_autograd
    r, dx, dwref = ref(act, w.double(), dy.double(), stride, dil)
    # hardtanh's mask: the gradient passes strictly inside (0, 6)
    mask = ((act > 0) & ((act < 6) if (mode & 4) else torch.ones_like(act, dtype=torch.bool))).double() \
        if (mode & 1) else torch.ones_like(act)
    gref = dx * mask
    ye = dwe = None
    if dtype == BF16 and (mode & 2) and not ties:  # (the tie inputs stay exact in bf16)
        ye, _, dwe = ref(quant(_act_ref(x, mode, s, t), BF16).double(), w.double(), dy.double(),
                         stride, dil)
        if stride == 1 and dil > 64:  # the strip kernels keep the activation in fp32
            ye = None
        if not tiled:
            dwe = None
    if ties and (mode & 1):  # the point of the inputs: many activated values exactly on the boundary
        assert (act == 0).sum() > 0.05 * act.numel()
        if mode & 4:
            assert (act == 6).sum() > 0.01 * act.numel()
    pad = dict(pitch=C + 16, off=8) if sl else {}
    xd = to_dev_nhwc(x, dtype, **pad)
    dyd = to_dev_nhwc(dy, dtype, **pad)
    w9c = w.view(C, 9).t().contiguous().to(DEV)
    w4 = w.to(DEV)
    gy = [_grid_y(dtype, C, N, H, W, stride, dil, k) for k in range(3)]
    assert gy == [_grid_y_mirror(dtype, C, N, H, W, stride, dil, k) for k in range(3)]
    sfac = 5 if dtype == F32 else 60
    bfac = 5 if dtype == F32 else 300
    wfac = WGRAD_FAC[dtype]

    def out_slice(h, ww):
        P, off = (C + 2 * vec, vec) if sl else (C, 0)
        full = torch.full((N, h, ww, P), NAN, dtype=dtype, device=DEV)
        return full, full[..., off:off + C], off

    def border_is_nan(full, off):  # nothing outside the slice was touched
        assert torch.isnan(full[..., :off].float()).all()
        assert torch.isnan(full[..., off + C:].float()).all()

    # ---- forward + statistics
    full, out, off = out_slice(Ho, Wo)
    y, partial = K().dwconv(xd, w9c, stride, dil, pro, out=out, want_stats=True)
    assert y.data_ptr() == out.data_ptr() and partial.shape[0] == gy[0]
    assert_close(to_cpu_nchw(y), r, dtype, "y")  # (a skipped element stays NaN)
    border_is_nan(full, off)
    sums = K().colsum(partial.view(gy[0], -1)).cpu()
    sabs = r.abs().sum((0, 2, 3)).max().item()
    assert_close(sums[:C], r.sum((0, 2, 3)), F32, "sum y", scale=sabs,
                 fac=_emu_fac(sfac, None if ye is None else ye.sum((0, 2, 3)), r.sum((0, 2, 3)), sabs))
    assert_close(sums[C:], (r * r).sum((0, 2, 3)), F32, "sum y^2",
                 fac=_emu_fac(sfac, None if ye is None else (ye * ye).sum((0, 2, 3)), (r * r).sum((0, 2, 3))))
    if tiled:  # torch's [C,1,3,3] parameter as is: the same taps in the same order
        assert torch.equal(K().dwconv(xd, w4, stride, dil, pro)[0], y)

    # ---- data gradient (stride 1: the forward kernel on reversed taps; stride 2: strip fallback)
    full, out, off = out_slice(H, W)
    g = K().dwconv_dgrad(dyd, w9c.flip(0).contiguous() if stride == 1 else w9c, stride, dil, (H, W),
                         out=out)
    assert g.data_ptr() == out.data_ptr()
    assert_close(to_cpu_nchw(g), dx, dtype, "dgrad")
    border_is_nan(full, off)
    if tiled:  # reversed inside the kernel
        assert torch.equal(K().dwconv_dgrad(dyd, w4, stride, dil, (H, W)), g)

    # ---- separate weight gradient
    dW = K().dwconv_wgrad(xd, dyd, stride, dil, pro)
    if dwe is not None or ye is not None:  # the figures behind the emulated bars (see above)
        rs, rq = r.sum((0, 2, 3)), (r * r).sum((0, 2, 3))
        print("FIG %s mode %d (kernel / emulated, of 2e-5): wgrad %.1f / %.1f, sum %.1f / %.1f, sum^2 %.1f / %.1f" % (
            (N, H, W, C, stride, dil), mode, _nerr(dW.t().reshape(C, 1, 3, 3).cpu(), dwref),
            _nerr(dwe, dwref) if dwe is not None else 0, _nerr(sums[:C], rs, sabs),
            _nerr(ye.sum((0, 2, 3)), rs, sabs) if ye is not None else 0, _nerr(sums[C:], rq),
            _nerr((ye * ye).sum((0, 2, 3)), rq) if ye is not None else 0))
    wfac = _emu_fac(wfac, dwe, dwref)
    assert_close(dW.t().reshape(C, 1, 3, 3).cpu(), dwref, F32, "wgrad", fac=wfac)
    if tiled:
        dW4 = K().dwconv_wgrad(xd, dyd, stride, dil, pro, torch_layout=True)
        assert_close(dW4.cpu(), dwref, F32, "wgrad torch layout", fac=wfac)

    # ---- fused backward
    full, out, off = out_slice(H, W)
    if stride == 2:
        gf, dWf, pb = K().dwconv_bwd_fused_s2(xd, dyd, w4, pro, want_bn=True, out=out)
        gyb = K().LIB.query("seg_dwconv3x3_s2_grid_y", C, N, H, W)
        assert gyb == _s2_bwd_grid(C, N, H, W)[1]
    else:
        gf, dW9, pb = K().dwconv_bwd_fused(xd, dyd, w9c, dil, pro, want_bn=True, out=out)
        dWf = dW9.t().reshape(C, 1, 3, 3)
        gyb = gy[1]
    assert gf.data_ptr() == out.data_ptr() and pb.shape[0] == gyb
    assert_close(to_cpu_nchw(gf), gref, dtype, "fused g")
    border_is_nan(full, off)
    assert_close(dWf.cpu(), dwref, F32, "fused dW", fac=FUSED_DW_FAC)
    sums = K().colsum(pb).cpu()
    gx = gref * x.double()
    assert_close(sums[:C], gref.sum((0, 2, 3)), F32, "fused sum g",
                 scale=gref.abs().sum((0, 2, 3)).max().item(), fac=bfac)
    assert_close(sums[C:], gx.sum((0, 2, 3)), F32, "fused sum gx",
                 scale=gx.abs().sum((0, 2, 3)).max().item(), fac=bfac)
    if tiled:
        g4, dW4, pb4 = K().dwconv_bwd_fused(xd, dyd, w4, dil, pro, want_bn=True, torch_layout=True)
        assert torch.equal(g4, gf) and torch.equal(pb4, pb)
        assert_close(dW4.cpu(), dwref, F32, "fused dW torch layout", fac=FUSED_DW_FAC)

    # ---- the partial rows each launch owns: buffers two rows longer, NaN-filled
    L, p, dt, st = K().LIB, K()._p, K()._DT[dtype], K()._stream()
    ldx, lddy = K().nhwc(xd)[4], K().nhwc(dyd)[4]
    m, sc, sh = pro
    ys, gs = torch.empty((N, Ho, Wo, C), dtype=dtype, device=DEV), torch.empty((N, H, W, C), dtype=dtype, device=DEV)
    pf = torch.full((gy[0] + 2, 2, C), NAN, device=DEV)
    L.call("seg_dwconv3x3", dt, 0, p(xd), ldx, N, H, W, C, p(w9c), 0, stride, dil, m, p(sc), p(sh),
           p(ys), C, Ho, Wo, p(pf), gy[0], st)
    assert _written(pf) == gy[0] and torch.equal(ys, y)
    pg = torch.full((gy[2] + 2, 9 * C), NAN, device=DEV)
    L.call("seg_dwconv3x3_wgrad", dt, p(xd), ldx, N, H, W, C, p(dyd), lddy, Ho, Wo, stride, dil, m,
           p(sc), p(sh), p(pg), gy[2], st)
    assert _written(pg) == gy[2]
    pw = torch.full((gyb + 2, 9 * C), NAN, device=DEV)
    pn = torch.full((gyb + 2, 2 * C), NAN, device=DEV)
    if stride == 2:
        L.call("seg_dwconv3x3_s2_bwd_fused", dt, p(dyd), lddy, p(xd), ldx, N, H, W, C, p(w4), m,
               p(sc), p(sh), p(gs), C, p(pw), p(pn), gyb, st)
    else:
        L.call("seg_dwconv3x3_bwd_fused", dt, p(dyd), lddy, p(xd), ldx, N, H, W, C, p(w9c), 0, dil,
               m, p(sc), p(sh), p(gs), C, p(pw), p(pn), gyb, st)
    assert _written(pw) == gyb and _written(pn) == gyb
    assert torch.equal(gs, gf) and torch.equal(pn[:gyb], pb)


def _id(c):
    return "x".join(map(str, c[0] if isinstance(c[0], tuple) else c))


# ------------------------------------------------------------- LDS-tiled, dilation 2: geometry
# (N, H, W, C) -> what the case is for: the remainder tiling (nb bottom strips, nc right strips,
# tiles) of the forward and of the fused backward, the classic tile count of the weight gradient,
# and per dtype the persistent blocks (grid_y) of forward / fused backward / weight gradient.
# C = 72: a ragged second channel block in both vector widths (9 vectors of 8, 18 of 4).
TILED_CASES = [
    # the benchmark's exit-flow map: bottom and right strips at once
    ((2, 65, 129, 72), dict(fwd=(3, 2, 138), bwd=(3, 2, 138), wg=162)),
    # bottom strip only (H % 8 = 2), the second strip 6 columns wide
    ((1, 18, 70, 72), dict(fwd=(2, 0, 12), bwd=(2, 0, 12), wg=15)),
    # right strip only (W % 16 = 4), the second right tile 8 rows tall, hc = H
    ((2, 40, 20, 72), dict(fwd=(0, 2, 14), bwd=(0, 2, 14), wg=20)),
    # the forward takes a right strip that saves nothing, the fused backward refuses it (< 6 %)
    ((1, 8, 17, 72), dict(fwd=(0, 1, 2), bwd=(0, 0, 2), wg=2)),
    # smaller than one tile, narrower than the halo: no remainder tiling (full_h = full_w = 0)
    ((2, 5, 3, 72), dict(fwd=(0, 0, 2), bwd=(0, 0, 2), wg=2)),
    # both strips on a map of one full tile: the corner they share (rows 8-9 x columns 16-19) is
    # 4 % of the map — counted twice it moves every sum by 40 (fp32) / 7 (bf16) times its bar
    ((2, 10, 20, 72), dict(fwd=(1, 1, 6), bwd=(1, 1, 6), wg=8)),
    # persistent loops with remainder tiles behind them
    ((1, 65, 129, 1024), dict(fwd=(3, 2, 69), bwd=(3, 2, 69), wg=81,
                              gy={F32: [64, 16, 24], BF16: [69, 16, 48]})),
    ((2, 41, 50, 512), dict(fwd=(1, 2, 36), bwd=(1, 2, 36), wg=48, gy={F32: [36, 32, 48], BF16: [36, 32, 48]})),
]


def _assert_tiled_case(shape, want, dtype):
    N, H, W, C = shape
    for kind, key in ((0, "fwd"), (1, "bwd")):
        g, gy = _tiled_grid(dtype, C, N, H, W, kind)
        assert (g["nb"], g["nc"], g["ntiles"]) == want[key], (key, g)
        if "gy" in want:
            assert gy == want["gy"][dtype][kind]
    g, gy = _tiled_grid(dtype, C, N, H, W, 2)
    assert g["nb"] == g["nc"] == 0 and g["ntiles"] == want["wg"]
    if "gy" in want:
        assert gy == want["gy"][dtype][2]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", TILED_CASES, ids=_id)
def test_tiled_dil2_remainder_tiling(case, dtype):
    shape, want = case
    _assert_tiled_case(shape, want, dtype)
    N, H, W, C = shape
    if shape == (1, 18, 70, 72):
        assert W - 64 == 6 and H % 8 == 2
    if shape == (2, 40, 20, 72):
        g = _tiled_geom(N, H, W, True)
        assert g["hc"] == H and H - 32 == 8 and g["wc0"] == 16
    if shape == (1, 65, 129, 1024):  # which launches walk more than one tile per block
        gys = want["gy"][dtype]
        assert (want["fwd"][2] > gys[0]) == (dtype == F32) and want["bwd"][2] > gys[1] and want["wg"] > gys[2]
    if shape == (2, 41, 50, 512):
        assert want["bwd"][2] > want["gy"][dtype][1]
    _check(N, H, W, C, 1, 2, 3 if H % 2 else 1, dtype, sl=(W % 2 == 1), seed=100 + H)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", MODES)
def test_tiled_dil2_prologue_modes(mode, dtype):
    """every dilation-2 launch runs the runtime prologue instance (MODE = -1)"""
    _check(1, 18, 70, 72, 1, 2, mode, dtype, seed=120 + mode)
    _check(2, 65, 129, 72, 1, 2, mode, dtype, sl=True, seed=130 + mode)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tiled_dil1_separate_weight_gradient(dtype):
    """the dilation-1 forward and fused backward moved to the sliding kernels; the separate weight
    gradient of that dilation is still dwconv_wgrad_tiled_kernel<T, 1> (classic tiling)."""
    N, H, W, C = 2, 65, 129, 72
    g, gy = _tiled_grid(dtype, C, N, H, W, 2)
    assert g["ntiles"] == 162 and gy == 162 == _grid_y(dtype, C, N, H, W, 1, 1, 2)
    x, dy = quant(rnd((N, C, H, W), 140), dtype), quant(rnd((N, C, H, W), 141), dtype)
    w = rnd((C, 1, 3, 3), 142, 0.4).double()
    pro, s, t = _pro(3, C, 143)
    _, _, dwref = _ref_autograd(_act_ref(x, 3, s, t).double(), w, dy.double(), 1, 1)
    xd = to_dev_nhwc(x, dtype, pitch=C + 16, off=8)
    dyd = to_dev_nhwc(dy, dtype, pitch=C + 16, off=8)
    wfac = 20
    if dtype == BF16:  # the staged activation's one bf16 rounding: see _check
        dwe = _ref_autograd(quant(_act_ref(x, 3, s, t), BF16).double(), w, dy.double(), 1, 1)[2]
        wfac = _emu_fac(100, dwe, dwref)
    dW = K().dwconv_wgrad(xd, dyd, 1, 1, pro)
    assert_close(dW.t().reshape(C, 1, 3, 3).cpu(), dwref, F32, "wgrad", fac=wfac)
    dW4 = K().dwconv_wgrad(xd, dyd, 1, 1, pro, torch_layout=True)
    assert_close(dW4.cpu(), dwref, F32, "wgrad torch layout", fac=wfac)
    pg = torch.full((gy + 2, 9 * C), NAN, device=DEV)
    K().LIB.call("seg_dwconv3x3_wgrad", K()._DT[dtype], K()._p(xd), C + 16, N, H, W, C, K()._p(dyd),
                 C + 16, H, W, 1, 1, 3, K()._p(pro[1]), K()._p(pro[2]), K()._p(pg), gy, K()._stream())
    assert _written(pg) == gy


# --------------------------------------------------------------------- row chains: geometry
# (N, H, W, C, dil) -> (TW, ntw, chains, grid_y) of row_geom / dw_row_grid_y, the same in both
# dtypes at these sizes.  C = 40: a ragged second channel block (2 live quads of 8; in bf16 one
# live staging vector of 4).
ROW_CASES = [
    # two segments, the last with 80 live pixels; chains of 3 and 2 rows
    ((2, 13, 161, 40, 6), (81, 2, 24, 24)),
    # three segments; the smallest row-chain dilation, next to the tiled dilation 2
    ((1, 9, 321, 40, 3), (107, 3, 9, 9)),
    # the widest single segment: every pixel lane carries MAXP = 5 pixels
    ((2, 26, 160, 72, 24), (160, 1, 48, 48)),
    # rate 36 at output-stride-8 width: three segments, 108 chains
    ((1, 40, 330, 32, 36), (110, 3, 108, 108)),
    # dil >= H and dil >= W: nph = H, only the centre tap is inside the image
    ((1, 5, 7, 40, 12), (7, 1, 5, 5)),
    # 18 chains on 12 blocks: a block walks a second chain (ring re-staged between chains)
    ((1, 37, 24, 2048, 18), (24, 1, 18, 12)),
    # the last dilation of the family
    ((1, 70, 66, 8, 64), (66, 1, 64, 64)),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ROW_CASES, ids=_id)
def test_row_chain_geometry(case, dtype):
    (N, H, W, C, dil), want = case
    TW, ntw = _row_geom(dtype, W, dil)
    assert (TW, ntw) + _row_grid(dtype, C, N, H, W, dil) == want
    if (W, dil) == (161, 6):
        assert W - TW == 80 and sorted({len(range(ph, H, dil)) for ph in range(dil)}) == [2, 3]
    if W == 160:
        assert TW == 160 == 5 * 32
    if dil == 12:
        assert dil >= H and dil >= W and want[2] == N * H
    if C == 2048:
        assert want[2] > want[3]
    _check(N, H, W, C, 1, dil, 3 if H % 2 else 2, dtype, sl=(W, dil) in ((161, 6), (330, 36)),
           seed=200 + dil)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_strip_fallback_begins_at_dilation_65(dtype):
    N, H, W, C = 1, 70, 66, 8
    row, strip = _row_grid(dtype, C, N, H, W, 64)[1], _strip_grid_y(dtype, C, N, H, W)
    assert row == 64 and strip == _cdiv(70 * 17, 32) == 38
    for kind in (0, 1):
        assert _grid_y(dtype, C, N, H, W, 1, 64, kind) == row
        assert _grid_y(dtype, C, N, H, W, 1, 65, kind) == strip
    _check(N, H, W, C, 1, 65, 3, dtype, sl=True, seed=265)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", MODES)
def test_row_chain_prologue_modes(mode, dtype):
    _check(2, 13, 161, 40, 1, 6, mode, dtype, sl=(mode % 2 == 0), seed=220 + mode)


# ------------------------------------------------------------------------ stride 2: geometry
# (N, H, W, C) -> (forward tiles, forward grid_y) per dtype, (backward tiles, backward grid_y)
S2_CASES = [
    ((1, 1, 1, 40), {F32: (1, 1), BF16: (1, 1)}, (1, 1)),      # the smallest map
    ((2, 2, 3, 40), {F32: (2, 2), BF16: (2, 2)}, (2, 2)),
    ((1, 8, 32, 40), {F32: (1, 1), BF16: (1, 1)}, (2, 2)),     # exact tiles
    ((1, 9, 33, 40), {F32: (4, 4), BF16: (4, 4)}, (6, 6)),     # one row / column into the next tile
    ((1, 33, 65, 1024), {F32: (15, 15), BF16: (15, 15)}, (25, 24)),  # backward: 25 tiles on 24 blocks
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", S2_CASES, ids=_id)
def test_stride2_geometry(case, dtype):
    (N, H, W, C), fwd, bwd = case
    assert _s2_fwd_grid(dtype, C, N, (H + 1) // 2, (W + 1) // 2) == fwd[dtype]
    assert _s2_bwd_grid(C, N, H, W) == bwd
    if (H, W) == (8, 32):
        assert H // 2 == 4 and W // 2 == 16 and H % 8 == 0 and W % 16 == 0
    if (H, W) == (9, 33):
        assert (H + 1) // 2 == 4 + 1 and (W + 1) // 2 == 16 + 1
    _check(N, H, W, C, 2, 1, 3 if C == 40 else 7, dtype, sl=(H, W) == (9, 33), seed=300 + H)


def test_stride2_forward_with_more_tiles_than_blocks():
    """(2, 35, 130, 2048) fp32: 50 forward tiles on 32 persistent blocks (64 channel blocks);
    18.6 M elements: the shifted multiply-add reference."""
    N, H, W, C = 2, 35, 130, 2048
    assert _s2_fwd_grid(F32, C, N, 18, 65) == (50, 32) and N * C * H * W > (4 << 20)
    _check(N, H, W, C, 2, 1, 1, F32, seed=335)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", MODES)
def test_stride2_prologue_modes(mode, dtype):
    """bf16 forward: compile-time instances for modes 1 and 3, the runtime one for 0 / 2 / 5 / 7"""
    _check(1, 9, 33, 40, 2, 1, mode, dtype, sl=True, seed=320 + mode)


# -------------------------------------------------------------------------------- mask ties
TIE_GEOMS = [(2, 18, 37, 72, 1, 2), (1, 13, 37, 40, 1, 6), (2, 17, 37, 40, 2, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [1, 3, 5, 7])
@pytest.mark.parametrize("geom", TIE_GEOMS, ids=["dil2", "dil6", "stride2"])
def test_mask_at_exact_relu_and_relu6_boundaries(geom, mode, dtype):
    """Activated values exactly 0 (also from -0 inputs) and exactly 6: the gradient passes
    strictly inside (0, 6), as hardtanh's — in the masked g and in the BatchNorm-backward sums."""
    _check(*geom, mode, dtype, ties=True, seed=400 + mode)


# ------------------------------------------------------------------------ rejected arguments
def _raises_multiples(fn, *a, **k):
    with pytest.raises(RuntimeError, match="multiples"):
        fn(*a, **k)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", [(1, 9, 20, 16, 1, 2), (1, 9, 20, 16, 1, 6), (1, 9, 20, 16, 2, 1)],
                         ids=["dil2", "dil6", "stride2"])
def test_pitch_off_the_vector_width_is_reported_not_launched(geom, dtype):
    N, H, W, C, stride, dil = geom
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    pro = (1, None, None)
    x, dy = rnd((N, C, H, W), 50), rnd((N, C, Ho, Wo), 51)
    xd, dyd = to_dev_nhwc(x, dtype), to_dev_nhwc(dy, dtype)
    xo = to_dev_nhwc(x, dtype, pitch=C + 2)  # rows of C + 2 elements: not a 4-channel vector
    dyo = to_dev_nhwc(dy, dtype, pitch=C + 2)
    w4 = rnd((C, 1, 3, 3), 52).to(DEV)
    w9c = w4.view(C, 9).t().contiguous()
    go = torch.full((N, H, W, C + 2), NAN, dtype=dtype, device=DEV)
    gout = torch.full((N, H, W, C), NAN, dtype=dtype, device=DEV)
    outs = [go, gout]
    if stride == 1:  # (the stride-2 forward is covered by the entry's common check, as dilation 2)
        oo = torch.full((N, Ho, Wo, C + 2), NAN, dtype=dtype, device=DEV)
        out = torch.full((N, Ho, Wo, C), NAN, dtype=dtype, device=DEV)
        outs += [oo, out]
        _raises_multiples(K().dwconv, xo, w9c, 1, dil, pro, out=out)
        _raises_multiples(K().dwconv, xd, w9c, 1, dil, pro, out=oo[..., :C])
        bwd = lambda a, b, **k: K().dwconv_bwd_fused(a, b, w9c, dil, pro, want_bn=True, **k)
    else:
        bwd = lambda a, b, **k: K().dwconv_bwd_fused_s2(a, b, w4, pro, want_bn=True, **k)
    _raises_multiples(bwd, xo, dyd, out=gout)
    _raises_multiples(bwd, xd, dyo, out=gout)
    _raises_multiples(bwd, xd, dyd, out=go[..., :C])
    torch.cuda.synchronize()
    for t in outs:  # nothing was launched
        assert torch.isnan(t.float()).all()
    # ... and the device is fine: the same op on a valid pitch
    _check(N, H, W, C, stride, dil, 1, dtype, sl=True, seed=53)


def test_bf16_row_chain_backward_rejects_half_a_staging_vector():
    """The row-chain kernels stage dy with 16-byte vectors: 8 bf16 channels.  With C = 36 the
    vector at channel 32 would read four channels past C (eight bytes past the tensor on the last
    pixel) at 8-byte alignment, so the entry reports it, as the forward entry and the tiled
    branch do.  The kernels on 4-channel vectors keep taking C = 4 (mod 8): the sliding backward
    (dilation 1) and the stride-2 backward."""
    N, H, W, C = 1, 9, 17, 36
    pro = (1, None, None)
    x, dy = quant(rnd((N, C, H, W), 60), BF16), quant(rnd((N, C, H, W), 61), BF16)
    w = rnd((C, 1, 3, 3), 62, 0.4)
    xd, dyd = to_dev_nhwc(x, BF16), to_dev_nhwc(dy, BF16)
    w9c = w.view(C, 9).t().contiguous().to(DEV)
    gout = torch.full((N, H, W, C), NAN, dtype=BF16, device=DEV)
    for a, b in ((xd, dyd), (to_dev_nhwc(x, BF16, pitch=40), to_dev_nhwc(dy, BF16, pitch=40))):
        _raises_multiples(K().dwconv_bwd_fused, a, b, w9c, 6, pro, want_bn=True, out=gout)
    torch.cuda.synchronize()
    assert torch.isnan(gout.float()).all()  # nothing was launched
    # whole staging vectors: the same launch works
    _check(N, H, W, 40, 1, 6, 1, BF16, seed=63)
    # dilation 1 (sliding kernels) and stride 2 at C = 36
    act = torch.relu(x).double()
    for stride in (1, 2):
        dys = quant(rnd((N, C, (H + stride - 1) // stride, (W + stride - 1) // stride), 64), BF16)
        _, dx, dwref = _ref_autograd(act, w.double(), dys.double(), stride, 1)
        gref = dx * (act > 0)
        dysd = to_dev_nhwc(dys, BF16)
        if stride == 1:
            g, dW, pb = K().dwconv_bwd_fused(xd, dysd, w.to(DEV), 1, pro, want_bn=True, torch_layout=True)
        else:
            g, dW, pb = K().dwconv_bwd_fused_s2(xd, dysd, w.to(DEV), pro, want_bn=True)
        assert_close(to_cpu_nchw(g), gref, BF16, "C=36 g, stride %d" % stride)
        assert_close(dW.cpu(), dwref, F32, "C=36 dW", fac=20)
        sums = K().colsum(pb).cpu()
        gx = gref * x.double()
        assert_close(sums[:C], gref.sum((0, 2, 3)), F32, "C=36 sum g",
                     scale=gref.abs().sum((0, 2, 3)).max().item(), fac=300)
        assert_close(sums[C:], gx.sum((0, 2, 3)), F32, "C=36 sum gx",
                     scale=gx.abs().sum((0, 2, 3)).max().item(), fac=300)
