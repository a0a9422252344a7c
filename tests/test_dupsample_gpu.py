"""GPU: the DUpsampling kernels (csrc/dupsample.hip) behind functional.DUpLogitsView — the fused
cross-entropy on the low-resolution NHWC tensor against float64 torch on the reference's
rearrangement and against the project's independent row cross-entropy (seg_point_ce_*), the
all-ignored target, determinism, the materialised tensor and its backward, and the fallbacks."""
import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd

pytestmark = pytest.mark.gpu

# (N, h, w, s, C)
GEOMS = [
    (2, 3, 5, 8, 19),   # the model's own row; odd w gives tile tails
    (1, 1, 1, 8, 19),   # one low-resolution pixel
    (2, 4, 3, 2, 19),   # row of 76 elements, not a vector multiple in bf16
    (1, 2, 7, 4, 21),   # s = 4, 21 classes
    (1, 3, 2, 8, 32),   # the class limit
    (3, 2, 9, 8, 2),    # two classes
    (1, 5, 4, 1, 19),   # s = 1, plain row CE
]
DTYPES = [torch.float32, torch.bfloat16]
GRAD_SEED = 1.7


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def F():
    from segmentron_amd import functional
    return functional


def dup_permute(lo, s, C):
    """The reference's rearrangement of an NHWC tensor [N, h, w, s*s*C] -> [N, C, h*s, w*s]."""
    N, h, w, _ = lo.shape
    return lo.view(N, h, w, s, s, C).permute(0, 5, 1, 3, 2, 4).reshape(N, C, h * s, w * s)


def dup_permute_inverse(g, s):
    """Its inverse: [N, C, h*s, w*s] -> NHWC [N, h, w, s*s*C]."""
    N, C, H, W = g.shape
    h, w = H // s, W // s
    return g.view(N, C, h, s, w, s).permute(0, 2, 4, 3, 5, 1).reshape(N, h, w, s * s * C)


_CASES = {}


def case(geom, dtype):
    """Inputs and the float64 reference of one (geometry, dtype), computed once: lo (CPU, rounded
    to dtype), target with 10 % ignored (N = 3: one image ignored entirely), reference loss and
    gradient seeded 1.7."""
    key = (geom, dtype)
    if key not in _CASES:
        N, h, w, s, C = geom
        lo = quant(rnd((N, h, w, s * s * C), 1) * 2.0, dtype)
        g = torch.Generator().manual_seed(5)
        target = torch.randint(0, C, (N, h * s, w * s), generator=g)
        target[torch.rand(N, h * s, w * s, generator=g) < 0.1] = -1
        if N == 3:
            target[1] = -1
        ref_in = lo.double().requires_grad_()
        ref = TF.cross_entropy(dup_permute(ref_in, s, C), target, ignore_index=-1)
        ref.backward(torch.tensor(GRAD_SEED, dtype=torch.float64))
        _CASES[key] = (lo, target, ref.item(), ref_in.grad)
    return _CASES[key]


def on_device(lo, dtype):
    """-> NHWC device view whose row pitch is one vector more than needed, NaN in the pad."""
    vec = K().vec_of(dtype)
    k = lo.shape[-1]
    pitch = (k + 2 * vec - 1) // vec * vec
    buf = torch.full(lo.shape[:3] + (pitch,), float("nan"), dtype=dtype)
    buf[..., :k] = lo.to(dtype)
    return buf.to(DEV)[..., :k]


def one_ulp(a, b, dtype):
    """|a - b| <= one unit in the last place of `dtype` at the larger magnitude."""
    bits = 23 if dtype == torch.float32 else 7
    a, b = a.double(), b.double()
    m = torch.maximum(a.abs(), b.abs())
    _, e = torch.frexp(m)  # m = f * 2^e, f in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(m), e - 1 - bits)
    return bool(((a - b).abs() <= ulp).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_fused_cross_entropy_matches_float64(geom, dtype):
    N, h, w, s, C = geom
    lo, target, ref_loss, ref_grad = case(geom, dtype)
    lod = on_device(lo, dtype).requires_grad_()
    tgt = target.to(DEV)
    view = F().DUpLogitsView(lod, s, C)
    assert tuple(view.shape) == (N, C, h * s, w * s) and view.dim() == 4 and len(view) == N
    assert view.dtype == torch.float32 and view.requires_grad
    loss = TF.cross_entropy(view, tgt, ignore_index=-1)  # __torch_function__ -> fused
    assert loss.dim() == 0 and loss.dtype == torch.float32 and view._full is None
    print("dup CE %s %s: loss %.7f, float64 %.7f" % (geom, dtype, loss.item(), ref_loss))
    assert abs(loss.item() - ref_loss) <= 2e-5 * abs(ref_loss) + 1e-6
    (loss * GRAD_SEED).backward()
    assert view._full is None
    assert_close(lod.grad.cpu(), ref_grad, dtype, "fused DUpsampling CE dlo", fac=1.0)
    # nn.CrossEntropyLoss takes the same path
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1)
    assert crit(view, tgt).item() == loss.item() and view._full is None
    # the pad of a pitched gradient is written as exact zeros
    vec = K().vec_of(dtype)
    k = s * s * C
    pitch = (k + 2 * vec - 1) // vec * vec
    out = K().dup_ce_fwd(lod.detach(), tgt, s, C, -1)
    dlo = K().dup_ce_bwd(lod.detach(), tgt, s, C, -1, out,
                         torch.tensor([GRAD_SEED], device=DEV), pitch)
    assert tuple(dlo.shape) == (N, h, w, pitch)
    assert torch.equal(dlo[..., k:], torch.zeros_like(dlo[..., k:]))
    assert torch.equal(dlo[..., :k], lod.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_agrees_with_the_point_cross_entropy_kernels(geom, dtype):
    """seg_point_ce_fwd/bwd on lo.view(R, C) with the target permuted by torch: an independent
    kernel doing the same float32 arithmetic."""
    N, h, w, s, C = geom
    lo, target, _, _ = case(geom, dtype)
    lod, tgt = on_device(lo, dtype), target.to(DEV)
    g = torch.tensor([GRAD_SEED], device=DEV)
    out = K().dup_ce_fwd(lod, tgt, s, C, -1)
    dlo = K().dup_ce_bwd(lod, tgt, s, C, -1, out, g)[..., :s * s * C]
    rows = lod.contiguous().view(-1, C)
    trow = tgt.view(N, h, s, w, s).permute(0, 1, 3, 2, 4).reshape(-1).contiguous()
    pout = K().point_ce_fwd(rows, trow, -1)
    pd = K().point_ce_bwd(rows, trow, -1, pout, g).view(N, h, w, s * s * C)
    print("dup CE vs point CE %s %s: loss %.7f / %.7f, max |d| %.3e"
          % (geom, dtype, out[0].item(), pout[0].item(),
             (dlo.double() - pd.double()).abs().max().item()))
    assert abs(out[0].item() - pout[0].item()) <= 1e-6 * abs(pout[0].item())
    assert out[1].item() == pout[1].item()
    assert one_ulp(dlo.cpu(), pd.cpu(), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_all_ignored_target_is_nan_with_zero_gradient(dtype):
    N, h, w, s, C = GEOMS[0]
    lo, _, _, _ = case(GEOMS[0], dtype)
    lod = on_device(lo, dtype).requires_grad_()
    tgt = torch.full((N, h * s, w * s), -1, dtype=torch.long, device=DEV)
    out = K().dup_ce_fwd(lod.detach(), tgt, s, C, -1)
    assert torch.isnan(out[0]) and out[1].item() == 0.0
    loss = TF.cross_entropy(F().DUpLogitsView(lod, s, C), tgt, ignore_index=-1)
    assert torch.isnan(loss)
    loss.backward()
    assert torch.isfinite(lod.grad).all() and float(lod.grad.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_two_runs_give_equal_bits(geom, dtype):
    N, h, w, s, C = geom
    lo, target, _, _ = case(geom, dtype)
    lod, tgt = on_device(lo, dtype), target.to(DEV)
    g = torch.tensor([GRAD_SEED], device=DEV)
    runs = []
    for _ in range(2):
        out = K().dup_ce_fwd(lod, tgt, s, C, -1)
        runs.append((out, K().dup_ce_bwd(lod, tgt, s, C, -1, out, g)))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(runs[0][1].view(bits), runs[1][1].view(bits))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_materialize_is_the_permute_and_its_backward_the_inverse(geom, dtype):
    N, h, w, s, C = geom
    lo, _, _, _ = case(geom, dtype)
    lod = on_device(lo, dtype).requires_grad_()
    view = F().DUpLogitsView(lod, s, C)
    full = view.materialize()
    assert view.materialize() is full and full.dtype == torch.float32
    assert tuple(full.shape) == tuple(view.shape) == (N, C, h * s, w * s)
    assert torch.equal(full.detach().cpu(), dup_permute(lo, s, C))
    assert torch.equal(torch.argmax(view, 1), full.argmax(1))
    assert torch.equal(view[0], full[0]) and view.size(1) == C
    gy = rnd(tuple(full.shape), 9)
    full.backward(gy.to(DEV))
    want = dup_permute_inverse(gy, s)
    if dtype == torch.bfloat16:
        want = want.to(torch.bfloat16)
    assert lod.grad.dtype == dtype and torch.equal(lod.grad.cpu(), want)
    # the boundary helper: eager (evaluation) form and lazy form
    with torch.no_grad():
        assert torch.equal(F().dup_logits(lod, s, C, lazy=False), full)
    assert isinstance(F().dup_logits(lod, s, C, lazy=True), F().DUpLogitsView)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_fallbacks_materialise(dtype):
    N, h, w, s, C = GEOMS[3]
    lo, target, _, _ = case(GEOMS[3], dtype)
    lod, tgt = on_device(lo, dtype), target.to(DEV)
    # class weights: not fused, through the materialised tensor
    view = F().DUpLogitsView(lod, s, C)
    wts = torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.5
    l2 = TF.cross_entropy(view, tgt, weight=wts.to(DEV), ignore_index=-1)
    assert view._full is not None
    r2 = TF.cross_entropy(dup_permute(lo.double(), s, C), target, weight=wts.double(),
                          ignore_index=-1)
    assert abs(l2.item() - r2.item()) <= 1e-4 * abs(r2.item())
    # a target of the wrong spatial size raises, as torch does
    view = F().DUpLogitsView(lod, s, C)
    with pytest.raises((RuntimeError, ValueError)):
        TF.cross_entropy(view, tgt[:, :-1], ignore_index=-1)
    # a tensor that is not [N, h, w, s*s*C] is refused at construction
    with pytest.raises(ValueError):
        F().DUpLogitsView(lod, s, C + 1)


def test_segmentation_metric_takes_the_view():
    """utils/score.py: the view materialises and counts as the tensor it stands for."""
    from segmentron_amd.utils.score import SegmentationMetric
    N, h, w, s, C = GEOMS[0]
    lo, target, _, _ = case(GEOMS[0], torch.float32)
    lod, tgt = on_device(lo, torch.float32), target.to(DEV)
    a, b = SegmentationMetric(C, False), SegmentationMetric(C, False)
    a.update(F().DUpLogitsView(lod, s, C), tgt)
    b.update(F().dup_logits(lod, s, C, lazy=False), tgt)
    assert a.get() == b.get() and 0.0 < a.get()[0] < 1.0
