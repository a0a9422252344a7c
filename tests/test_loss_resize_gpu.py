"""The fused cross-entropy backward (row pass + column pass around an fp32 workspace) and the
block-per-row bilinear resize kernels, at the edges of their launch geometry: several column
segments with a ragged last one, halos at both borders, every magnification tier of the loss, more
than one channel block, downsampling and 1x1 sources.  Reference: float64 torch on the CPU with the
bars of _util.assert_close that the older tests of these operators use (CE dlo at fac=1.0, bilinear
at the default).  Beyond the values: padding channels are exactly zero, nothing outside an output
slice is written, nothing outside an input slice is read, and two calls agree bit for bit (the
kernels have no atomics)."""
import functools

import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
GOUT = 1.7


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def F():
    from segmentron_amd import functional
    return functional


# ------------------------------------------------------------------------------ CE backward
CE_GEOMS = [
    (2, 9, 70, 33, 277, 19),     # exact x4, several column segments, ragged last one
    (1, 8, 8, 8, 8, 2),          # x1
    (1, 10, 37, 38, 141, 21),    # ~3.9x in both directions, halo at both borders
    (1, 5, 40, 33, 313, 30),     # x8, 32-class instance, widest segment footprint
    (1, 3, 19, 33, 289, 19),     # x16
]


@functools.lru_cache(maxsize=None)
def _ce_case(geom, dtype, align):
    """(lo NCHW cpu, target cpu, float64 reference gradient * GOUT) — computed once per case."""
    N, Hi, Wi, H, W, C = geom
    lo = quant(rnd((N, C, Hi, Wi), 1) * 2.0, dtype)
    g = torch.Generator().manual_seed(5)
    target = torch.randint(0, C, (N, H, W), generator=g)
    target[torch.rand(N, H, W, generator=g) < 0.1] = -1
    ref_in = lo.double().requires_grad_()
    ref = TF.cross_entropy(TF.interpolate(ref_in, (H, W), mode="bilinear", align_corners=align),
                           target, ignore_index=-1)
    ref.backward(torch.tensor(GOUT, dtype=torch.float64))
    return lo, target, ref_in.grad


def _ce_pitches(C, dtype):
    vec = K().vec_of(dtype)
    return (C + 2 * vec - 1) // vec * vec, (C + vec - 1) // vec * vec  # logits buffer, dlo


def _ce_bwd(lod, tgt, hw, pitch, align):
    out = K().upsample_ce_fwd(lod, tgt, hw, -1, align)
    gout = torch.tensor([GOUT], device=DEV)
    return K().upsample_ce_bwd(lod, tgt, hw, -1, out, gout, pitch, align)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", CE_GEOMS)
def test_ce_backward_row_and_column_pass(geom, dtype):
    N, Hi, Wi, H, W, C = geom
    lo, target, ref_grad = _ce_case(geom, dtype, True)
    lopitch, pitch = _ce_pitches(C, dtype)
    lod = to_dev_nhwc(lo, dtype, pitch=lopitch, off=0)   # NaN behind the classes
    tgt = target.to(DEV)
    d = _ce_bwd(lod, tgt, (H, W), pitch, True)
    assert tuple(d.shape) == (N, Hi, Wi, pitch) and d.dtype == dtype
    assert_close(to_cpu_nchw(d[..., :C]), ref_grad, dtype, "CE dlo", fac=1.0)
    if pitch > C:
        assert float(d[..., C:].float().abs().max()) == 0.0, "padding channels must be zero"
    d2 = _ce_bwd(lod, tgt, (H, W), pitch, True)
    assert torch.equal(d.view(torch.uint8), d2.view(torch.uint8)), "second call differs"
    # nothing valid: the gradient is zero, not NaN
    none = torch.full_like(tgt, -1)
    dz = _ce_bwd(lod, none, (H, W), pitch, True)
    assert torch.isfinite(dz).all() and float(dz.float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ce_backward_through_logits_view_with_wide_pitch(dtype):
    geom = (2, 17, 33, 65, 129, 19)
    N, Hi, Wi, H, W, C = geom
    lo, target, ref_grad = _ce_case(geom, dtype, True)
    lopitch, _ = _ce_pitches(C, dtype)
    grads = []
    for _ in range(2):
        lod = to_dev_nhwc(lo, dtype, pitch=lopitch, off=0).requires_grad_()
        view = F().LogitsView(lod, (H, W), True)
        loss = TF.cross_entropy(view, target.to(DEV), ignore_index=-1)
        assert view._full is None   # the fused path, nothing materialised
        (loss * GOUT).backward()
        grads.append(lod.grad)
    assert_close(to_cpu_nchw(grads[0]), ref_grad, dtype, "CE dlo (LogitsView)", fac=1.0)
    assert torch.equal(grads[0].view(torch.uint8), grads[1].view(torch.uint8))
    lod = to_dev_nhwc(lo, dtype, pitch=lopitch, off=0).requires_grad_()
    none = torch.full((N, H, W), -1, dtype=torch.long, device=DEV)
    TF.cross_entropy(F().LogitsView(lod, (H, W), True), none, ignore_index=-1).backward()
    assert torch.isfinite(lod.grad).all() and float(lod.grad.float().abs().max()) == 0.0


@pytest.mark.parametrize("align", [True, False], ids=["aligned", "half-pixel"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ce_operator_backward_both_align_corners(dtype, align):
    from segmentron_amd import torch_ops
    geom = (1, 10, 37, 38, 141, 21)
    N, Hi, Wi, H, W, C = geom
    lo, target, ref_grad = _ce_case(geom, dtype, align)
    lopitch, _ = _ce_pitches(C, dtype)
    lod = to_dev_nhwc(lo, dtype, pitch=lopitch, off=0).requires_grad_()
    out = torch_ops.upsample_cross_entropy(lod, target.to(DEV), H, W, -1, align)
    assert tuple(out.shape) == (2,) and out.dtype == torch.float32
    (out[0] * GOUT).backward()
    assert tuple(lod.grad.shape) == (N, Hi, Wi, C)
    assert_close(to_cpu_nchw(lod.grad), ref_grad, dtype, "CE dlo (operator)", fac=1.0)


# ------------------------------------------------------------------------------ bilinear
RESIZE_CASES = [
    (9, 17, 33, 65, True),
    (9, 13, 20, 31, False),
    (12, 10, 7, 5, True),       # downsampling
    (1, 1, 5, 9, True),         # 1x1 source: forward only
    (5, 70, 17, 277, True),     # several column segments, ragged last one
]


@functools.lru_cache(maxsize=None)
def _resize_case(case, C, dtype):
    Hi, Wi, Ho, Wo, ac = case
    N = 2
    x = quant(rnd((N, C, Hi, Wi), 1), dtype)
    s = torch.rand(C, generator=torch.Generator().manual_seed(4)) + 0.5
    t = rnd((C,), 5, 0.3)
    mul = torch.rand(N, C, generator=torch.Generator().manual_seed(6)) * 2.0
    refs = {}
    for mode in (0, 3):
        xa = x.double()
        if mode:
            xa = torch.relu(xa * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1))
        refs[mode] = TF.interpolate(xa, size=(Ho, Wo), mode="bilinear", align_corners=ac)
    g = quant(rnd((N, C, Ho, Wo), 2), dtype)
    xin = x.double().requires_grad_()
    TF.interpolate(xin, size=(Ho, Wo), mode="bilinear", align_corners=ac).backward(g.double())
    return x, s, t, mul, refs, g, xin.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [40, 264])
@pytest.mark.parametrize("case", RESIZE_CASES)
def test_bilinear_forward_prologue_chan_mul_into_a_slice(case, C, dtype):
    Hi, Wi, Ho, Wo, ac = case
    x, s, t, mul, refs, _, _ = _resize_case(case, C, dtype)
    N, off, pitch = x.shape[0], 8, C + 16
    xd = to_dev_nhwc(x, dtype, pitch=pitch, off=off)     # read from a slice as well
    muld = mul.to(DEV)
    for mode in (0, 3):
        pro = (mode, s.to(DEV), t.to(DEV)) if mode else None
        for cm in (None, muld):
            ref = refs[mode] if cm is None else refs[mode] * mul.double().view(N, C, 1, 1)
            what = "bilinear fwd mode %d%s" % (mode, "" if cm is None else " * chan_mul")
            outs = []
            for _ in range(2):
                buf = torch.full((N, Ho, Wo, pitch), float("nan"), dtype=dtype, device=DEV)
                y = K().bilinear(xd, (Ho, Wo), pro, cm, ac, out=buf[..., off:off + C])
                outs.append(y)
                assert torch.isnan(buf[..., :off]).all() and torch.isnan(buf[..., off + C:]).all(), \
                    what + ": wrote outside the slice"
            assert_close(to_cpu_nchw(outs[0]), ref, dtype, what)
            assert torch.equal(outs[0].contiguous().view(torch.uint8),
                               outs[1].contiguous().view(torch.uint8)), what + ": second call differs"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [40, 264])
@pytest.mark.parametrize("case", [c for c in RESIZE_CASES if c[0] > 1])
def test_bilinear_backward_from_a_slice(case, C, dtype):
    Hi, Wi, Ho, Wo, ac = case
    _, _, _, _, _, g, ref = _resize_case(case, C, dtype)
    gd = to_dev_nhwc(g, dtype, pitch=C + 16, off=8)      # NaN on both sides of the gradient
    gx = K().bilinear_bwd(gd, (Hi, Wi), ac)
    assert tuple(gx.shape) == (g.shape[0], Hi, Wi, C)
    assert_close(to_cpu_nchw(gx), ref, dtype, "bilinear bwd")   # (asserts finiteness too)
    gx2 = K().bilinear_bwd(gd, (Hi, Wi), ac)
    assert torch.equal(gx.view(torch.uint8), gx2.view(torch.uint8)), "second call differs"
