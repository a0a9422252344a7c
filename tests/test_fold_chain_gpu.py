"""The folded-BatchNorm pointwise backward chain (`functional._FoldConvFn.backward`), stage by
stage, at the kernel classes the real layers reach:

    conv_wgrad(raw_partial=True) -> fold_bwd_reduce -> fold_bwd_finalize -> data-gradient GEMM
    with the correction epilogue  dx = dY W'^T - c0 - c1 x

Every stage is compared with a float64 evaluation of the operands THAT STAGE consumed (read back
from the device where an earlier stage produced them), so a failure names the stage.  Bars are the
suite's own (`_util.assert_close`: fp32 2e-5, bf16 6e-3 of the reference's largest magnitude) with
the `fac` the existing fold / weight-gradient tests use for the same quantity.

Geometries (N, H, W, C -> O, stride), each the smallest that reaches its edge; for the bf16
direct-to-LDS weight gradient (1x1, no prologue, M >= 2048, O*C >= 128^2 or M >= 32768) the split
count is asserted, so a change of the split rule that moves a case off its edge fails here:

    A  2,45,47   728->728  M=4230   36 tiles (ragged o / c tiles of 88), 7 splits of 10 slots, the
                                    last one 7 slots, M % 64 = 6; 64 (ds, dt) rows; forward and
                                    corrected data gradient on the direct-to-LDS GEMM (bf16) and
                                    the 256-pixel-tile GEMM (fp32)
    B  1,65,67   200->392  M=4355   8 tiles, 9 splits (one past the reduce's 8-wide load round),
                                    K tail 72, O tail 8, M % 64 = 3
    C  1,113,145 512->256  M=16385  8 tiles, 32 splits of 9 slots over 257 slots: splits 29..31
                                    own no pixel and must still write zero partials
    D  1,190,180 256->48   M=34200  narrow O: 67 splits, one (ds, dt) row, the splits are summed
                                    by `colsum` before the reduce; data gradient on the general GEMM
    E  1,33,63   128->128  M=2079   } either side of M >= 2048 at O*C = 128^2 exactly: one tile,
    E' 1,31,66   128->128  M=2046   } 5 splits, M % 64 = 31 / first-generation kernel
    F  2,11,15   64->128, stride 2  scatter + bn_bwd_apply instead of the epilogue
    G  2,9,11    72->40    M=198    the base case of test_ops_gpu.py

The first-generation and fp32 weight-gradient kernels choose their splits differently: for them
only `partial.shape[0] == seg_conv_gemm_wgrad_splits(...)` is asserted.
"""
import functools

import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
NAN = float("nan")

GEOM = {
    # id: N, H, W, C, O, stride
    "A": (2, 45, 47, 728, 728, 1),
    "B": (1, 65, 67, 200, 392, 1),
    "C": (1, 113, 145, 512, 256, 1),
    "D": (1, 190, 180, 256, 48, 1),
    "E": (1, 33, 63, 128, 128, 1),
    "E'": (1, 31, 66, 128, 128, 1),
    "F": (2, 11, 15, 64, 128, 2),
    "G": (2, 9, 11, 72, 40, 1),
}
GLDS_SPLITS = {"A": 7, "B": 9, "C": 32, "D": 67, "E": 5}  # bf16, direct-to-LDS kernel
COUNT = 4230.0


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t_nhwc, dtype, pitched=False):
    """CPU NHWC float -> device NHWC; pitched: channels 8 .. 8+C of a NaN-filled C+16 buffer."""
    c = t_nhwc.shape[-1]
    return to_dev_nhwc(t_nhwc.permute(0, 3, 1, 2), dtype, pitch=c + 16 if pitched else None,
                       off=8 if pitched else 0)


def _nan_slice(shape, dtype):
    """-> (full NaN buffer [..., C+16], its channel slice 8 .. 8+C)."""
    full = torch.full(tuple(shape[:-1]) + (shape[-1] + 16,), NAN, dtype=dtype, device=DEV)
    return full, full[..., 8:8 + shape[-1]]


def _untouched(full, c):
    return bool(torch.isnan(full[..., :8].float()).all()) and \
        bool(torch.isnan(full[..., 8 + c:].float()).all())


def _splits(gid, dtype, parts):
    """The split count a launch got is the one the library announces (and, on the bf16
    direct-to-LDS kernel, the one this file's geometries were chosen for)."""
    N, H, W, C, O, st = GEOM[gid]
    Ho, Wo = (H - 1) // st + 1, (W - 1) // st + 1
    Km = K()
    q = Km.LIB.query("seg_conv_gemm_wgrad_splits", Km._DT[dtype], N, Ho, Wo, C, O, 1, 1, st, 0, 1, 0)
    assert parts.shape == (q, O * C), (tuple(parts.shape), q)
    if dtype == torch.bfloat16 and gid in GLDS_SPLITS:
        assert q == GLDS_SPLITS[gid], "geometry %s left its edge: %d splits" % (gid, q)
    return q


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    for f in (_int_case, _rand_case, _reduce_case, _finalize_case, _epilogue_case, _chain_case):
        f.cache_clear()


# ------------------------------------------------------------------ 1. weight-gradient partials
@functools.lru_cache(maxsize=None)
def _int_case(gid):
    """x, dy in {-2 .. 2} (exact in bf16): every partial sum is an integer of magnitude
    <= 4 M < 2^24, exact in fp32 in ANY order -> the float64 result must be met bit for bit."""
    N, H, W, C, O, _ = GEOM[gid]
    g = _gen(101)
    x = torch.randint(-2, 3, (N, H, W, C), generator=g).float()
    dy = torch.randint(-2, 3, (N, H, W, O), generator=g).float()
    M = N * H * W
    assert 4 * M < 2 ** 24
    ref = dy.view(M, O).double().t() @ x.view(M, C).double()
    return x, dy, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("gid", ["A", "C", "E", "E'"])
def test_wgrad_split_partials_are_exact_on_small_integers(gid, dtype):
    """A pixel dropped or doubled at a split / slot boundary changes an integer: no tolerance."""
    N, H, W, C, O, _ = GEOM[gid]
    x, dy, ref = _int_case(gid)
    parts = K().conv_wgrad(_dev(x, dtype), _dev(dy, dtype), O, 1, 1, 1, 0, 1, None,
                           raw_partial=True)
    S = _splits(gid, dtype, parts)
    got = parts.sum(0).view(O, C).cpu().double()  # integers: the fp32 sum is exact as well
    bad = int((got != ref).sum())
    assert torch.equal(got, ref), "%d of %d dW elements differ, largest by %g" % (
        bad, ref.numel(), (got - ref).abs().max().item())
    if dtype == torch.bfloat16 and gid in GLDS_SPLITS:
        # pixel range of split s on the direct-to-LDS kernel: [s * chunk, min(M, (s + 1) * chunk))
        M = N * H * W
        slots = (M + 63) // 64
        chunk = (slots + S - 1) // S * 64
        empty = [s for s in range(S) if s * chunk >= M]
        if gid == "C":
            assert empty == [29, 30, 31]
        for s in empty:  # (the partial buffer is torch.empty: a split without pixels must store)
            assert bool((parts[s] == 0).all()), "split %d owns no pixel but is not zero" % s


@functools.lru_cache(maxsize=None)
def _rand_case(gid, dtype):
    N, H, W, C, O, _ = GEOM[gid]
    x = quant(rnd((N, H, W, C), 1), dtype)
    dy = quant(rnd((N, H, W, O), 3), dtype)
    M = N * H * W
    ref = dy.view(M, O).double().t() @ x.view(M, C).double()
    return x, dy, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("gid", ["A", "B", "D", "E"])
def test_wgrad_of_channel_slices_matches_float64_and_the_contiguous_result(gid, dtype):
    """x and dy as channel slices of wider NaN-filled buffers (dy is routinely a slice of a concat
    gradient): same bits as from contiguous operands, and both within the weight-gradient bar."""
    N, H, W, C, O, _ = GEOM[gid]
    x, dy, ref = _rand_case(gid, dtype)
    Km = K()
    dWc = Km.conv_wgrad(_dev(x, dtype), _dev(dy, dtype), O, 1, 1, 1, 0, 1, None)
    xs, dys = _dev(x, dtype, True), _dev(dy, dtype, True)
    dWs = Km.conv_wgrad(xs, dys, O, 1, 1, 1, 0, 1, None)
    _splits(gid, dtype, Km.conv_wgrad(xs, dys, O, 1, 1, 1, 0, 1, None, raw_partial=True))
    assert_close(dWs.view(O, C).cpu(), ref, torch.float32, "dW of slices", fac=20)
    assert_close(dWc.view(O, C).cpu(), ref, torch.float32, "dW", fac=20)
    assert torch.equal(dWs, dWc), "pitched and contiguous operands give different bits"


# ------------------------------------------------------------------ 3. fold_bwd_reduce
def _reduce_ref(W, g, s, t, db):
    """float64: g = sum of the splits; dW = g s + db (x) t; ds = sum_o W g; dt = sum_o W db."""
    W, g, s, t = W.double(), g.double(), s.double(), t.double()
    dbd = torch.zeros(W.shape[0], dtype=torch.float64) if db is None else db.double()
    return g * s[None, :] + dbd[:, None] * t[None, :], (W * g).sum(0), (W * dbd[:, None]).sum(0)


@functools.lru_cache(maxsize=None)
def _reduce_case(S, O, C):
    W = rnd((O, C), 21, 0.2)
    dWp = rnd((S, O, C), 22)
    s = torch.rand(C, generator=_gen(23)) + 0.5
    t = rnd((C,), 24, 0.4)
    db = rnd((O,), 25, 3.0)
    g = dWp.double().sum(0)
    return W, dWp, s, t, db, {True: _reduce_ref(W, g, s, t, db), False: _reduce_ref(W, g, s, t, None)}


def _check_reduce(dW, dsdt, ref, C, with_db, what):
    rdW, rds, rdt = ref
    assert torch.isfinite(dsdt).all(), what + ": a (ds, dt) row was not written"
    assert_close(dW.cpu(), rdW, torch.float32, what + " dW", fac=5)
    rows = dsdt.cpu().double()
    assert_close(rows[:, :C].sum(0), rds, torch.float32, what + " ds", fac=20)
    if with_db:
        assert_close(rows[:, C:].sum(0), rdt, torch.float32, what + " dt", fac=20)
    else:
        assert bool((rows[:, C:] == 0).all()), what + ": dt without db must be zero"


def test_fold_bwd_rows_switches_to_64_row_slices_at_128_outputs():
    q = K().LIB.query
    assert [q("seg_fold_bwd_rows", o) for o in (1, 40, 127, 128, 129, 728)] == [1, 1, 1, 64, 64, 64]


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("oc", [(40, 72), (127, 72), (128, 72), (130, 260), (728, 728), (19, 50)],
                         ids=lambda oc: "%dx%d" % oc)
@pytest.mark.parametrize("S", [1, 7, 8, 9, 16, 17])
def test_fold_bwd_reduce_on_synthetic_split_partials(S, oc, with_db):
    """Both kernels (float4 lanes for C % 4 == 0, scalar for 19 x 50), one row and 64 row slices
    (130 rows: 20 trailing slices own no row and must still write their zero (ds, dt) row into
    the uninitialised buffer; 260 columns: one lane in the second column block), split counts
    around the 8-wide load round.  Once through the wrapper (which sums S > 8 splits of a one-row
    launch with `colsum` first) and once through the C-ABI with the true S into NaN-filled
    outputs."""
    O, C = oc
    W, dWp, s, t, db, refs = _reduce_case(S, O, C)
    ref = refs[with_db]
    Km = K()
    R = Km.LIB.query("seg_fold_bwd_rows", O)
    assert R == (1 if O < 128 else 64)
    Wd, pd, sd, td = W.to(DEV), dWp.to(DEV).view(S, O * C), s.to(DEV), t.to(DEV)
    dbd = db.to(DEV) if with_db else None
    dW, dsdt = Km.fold_bwd_reduce(Wd, pd, sd, td, dbd)
    assert tuple(dW.shape) == (O, C) and tuple(dsdt.shape) == (R, 2 * C)
    _check_reduce(dW, dsdt, ref, C, with_db, "wrapper")
    dW2 = torch.full((O, C), NAN, dtype=torch.float32, device=DEV)
    dsdt2 = torch.full((R, 2 * C), NAN, dtype=torch.float32, device=DEV)
    Km.LIB.call("seg_fold_bwd_reduce", Wd.data_ptr(), pd.data_ptr(), S, sd.data_ptr(),
                td.data_ptr(), Km._p(dbd), dW2.data_ptr(), dsdt2.data_ptr(), O, C, Km._stream())
    _check_reduce(dW2, dsdt2, ref, C, with_db, "C-ABI")


# ------------------------------------------------------------------ 4. fold_bwd_finalize
def _finalize_ref(dsdt, count, mean, invstd, gamma, scale, grad_scale):
    """float64 of the kernel's contract -> dgamma, dbeta, c0, c1 and the magnitude c0 is the
    difference of."""
    C = mean.numel()
    rows = dsdt.double().view(-1, 2 * C)
    ds, dt = rows[:, :C].sum(0), rows[:, C:].sum(0)
    mu, is_ = mean.double(), invstd.double()
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    u = ds - mu * dt
    A = g * u * is_ ** 3 / count
    lead = dt * scale.double() / count
    return is_ * u * grad_scale, dt * grad_scale, lead - A * mu, A, \
        (lead.abs() + (A * mu).abs()).max().item()


def _check_finalize(got, ref, what):
    dgamma, dbeta, c0, c1 = [v.cpu() for v in got]
    rg, rb, r0, r1, c0_scale = ref
    # the kernel accumulates and evaluates in double: only the final fp32 rounding is left
    assert_close(dgamma, rg, torch.float32, what + " dgamma")
    assert_close(dbeta, rb, torch.float32, what + " dbeta")
    assert_close(c1, r1, torch.float32, what + " c1")
    assert_close(c0, r0, torch.float32, what + " c0", scale=c0_scale)


@functools.lru_cache(maxsize=None)
def _finalize_case(R, C):
    dsdt = rnd((R, 2 * C), 31, 2.0)
    mean = rnd((C,), 32, 0.5) + 0.2
    invstd = torch.rand(C, generator=_gen(33)) + 0.5
    gamma = torch.rand(C, generator=_gen(34)) + 0.5
    return dsdt, mean, invstd, gamma, gamma * invstd


@pytest.mark.parametrize("C", [50, 64, 65, 728])
@pytest.mark.parametrize("R", [1, 31, 32, 33, 64, 65])
def test_fold_bwd_finalize_on_synthetic_rows(R, C):
    """Row counts around the 32-row stride of the loop (eight clamped loads at stride 4 per
    round), channel counts around the 64-channel block; host and device-resident count,
    grad_scale 1 and 1/8."""
    dsdt, mean, invstd, gamma, scale = _finalize_case(R, C)
    Km = K()
    d = [v.to(DEV) for v in (dsdt, mean, invstd, gamma, scale)]
    cdev = torch.tensor(COUNT, dtype=torch.float64, device=DEV)
    for count, cname in ((COUNT, "host count"), (cdev, "device count")):
        for gs in (1.0, 0.125):
            got = Km.fold_bwd_finalize(d[0], count, d[1], d[2], d[3], d[4], gs)
            ref = _finalize_ref(dsdt, COUNT, mean, invstd, gamma, scale, gs)
            _check_finalize(got, ref, "%s, grad_scale %g:" % (cname, gs))


def test_fold_bwd_finalize_without_gamma_is_gamma_one():
    R, C = 33, 65
    dsdt, mean, invstd, _, _ = _finalize_case(R, C)
    scale = invstd.clone()
    got = K().fold_bwd_finalize(dsdt.to(DEV), COUNT, mean.to(DEV), invstd.to(DEV), None,
                                scale.to(DEV))
    _check_finalize(got, _finalize_ref(dsdt, COUNT, mean, invstd, None, scale, 1.0), "no gamma:")


# ------------------------------------------------------------------ 5. correction epilogue
@functools.lru_cache(maxsize=None)
def _epilogue_case(gid, dtype):
    """The data gradient of geometry `gid`: dy [M, O] x W'^T [C, O] -> [M, C]; W'^T is the
    tensor fold_weights stored, read back."""
    N, H, W, C, O, _ = GEOM[gid]
    M = N * H * W
    dy = quant(rnd((N, H, W, O), 41), dtype)
    xe = quant(rnd((N, H, W, C), 42), dtype)
    w = rnd((O, C), 43, (2.0 / O) ** 0.5)
    s = torch.rand(C, generator=_gen(44)) + 0.5
    t = rnd((C,), 45, 0.3)
    _, wpt, _ = K().fold_weights(w.to(DEV), s.to(DEV), t.to(DEV), dtype, want_transpose=True,
                                 want_bias=False)
    acc = (dy.view(M, O).double() @ wpt.cpu().double().t()).view(N, H, W, C)
    return dy, xe, wpt, acc


@pytest.mark.parametrize("variant", ["contiguous", "slices", "residual"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("gid", ["A", "C", "D"])
def test_correction_epilogue_by_kernel_class(gid, dtype, variant):
    """y = acc - c0 - c1 x_e against float64 of the stored operands.  A: the eight-wave
    direct-to-LDS kernel in bf16, the 256-pixel-tile kernel in fp32; C: 256 -> 512; D: 48 -> 256
    on the general kernel.  `slices`: x_e and the output are channel slices of NaN-filled
    buffers, nothing outside the output slice may be written; `residual`: c0 = 0, c1 = -1, the
    identity-path add of `_ConvFn.backward`."""
    N, H, W, C, O, _ = GEOM[gid]
    dy, xe, wpt, acc = _epilogue_case(gid, dtype)
    if variant == "residual":
        c0, c1 = torch.zeros(C), -torch.ones(C)
    else:
        c0, c1 = rnd((C,), 46, 0.05), rnd((C,), 47, 0.3)
    ref = acc - c0.double() - c1.double() * xe.double()
    sl = variant == "slices"
    full, out = _nan_slice((N, H, W, C), dtype) if sl else (None, None)
    y, _ = K().conv_gemm(_dev(dy, dtype), wpt, C, 1, 1, 1, 0, 1, out=out,
                         ep=(_dev(xe, dtype, sl), c0.to(DEV), c1.to(DEV)))
    assert_close(y.float().cpu(), ref, dtype, "corrected y")
    if sl:
        assert y.data_ptr() == out.data_ptr()
        assert _untouched(full, C), "the epilogue wrote outside its channel slice"


# ------------------------------------------------------------------ 6. the whole chain
@functools.lru_cache(maxsize=None)
def _chain_case(gid, dtype):
    """float64 autograd of conv2d(batch_norm(x)), stride as the geometry says."""
    N, H, W, C, O, st = GEOM[gid]
    x = quant(rnd((N, C, H, W), 1) * 1.3 + 0.2, dtype)
    wt = rnd((O, C, 1, 1), 2, 0.2)
    gamma, beta = torch.rand(C, generator=_gen(4)) + 0.5, rnd((C,), 3, 0.2)
    xr = x.double().requires_grad_()
    wr = wt.double().requires_grad_()
    gr, br = gamma.double().requires_grad_(), beta.double().requires_grad_()
    xn = TF.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-3)
    y = TF.conv2d(xn, wr, None, st)
    dy = quant(rnd(tuple(y.shape), 5), dtype)
    y.backward(dy.double())
    return x, wt, gamma, beta, dy, y.detach(), xr.grad, wr.grad, gr.grad, br.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("gid", ["G", "A", "B", "D", "F"])
def test_folded_chain_stage_by_stage_and_against_autograd(gid, dtype):
    """test_ops_gpu.py::test_fold_linear_bn_into_pointwise_matches_autograd (geometry G) at the
    production kernel classes: each stage against float64 of what it consumed, then forward, dW,
    dgamma, dbeta and dx against autograd with that test's bars.  F (stride 2): dx at the pixels
    the stride skips is the correction alone, -c0 - c1 x."""
    N, H, W, C, O, st = GEOM[gid]
    x, wt, gamma, beta, dy, y, dx_ref, dW_ref, dgamma_ref, dbeta_ref = _chain_case(gid, dtype)
    Km = K()
    M = N * H * W
    Ho, Wo = dy.shape[2:]
    Mo = N * Ho * Wo
    x2d = x.permute(0, 2, 3, 1).reshape(M, C).double()
    xs2d = x[:, :, ::st, ::st].permute(0, 2, 3, 1).reshape(Mo, C).double()  # the pixels the conv reads
    dy2d = dy.permute(0, 2, 3, 1).reshape(Mo, O).double()
    sums = torch.cat([x.double().sum((0, 2, 3)), (x.double() ** 2).sum((0, 2, 3))]).to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    mean, invstd, scale, shift = Km.bn_finalize(sums, M, gd, bd, 1e-3, 0.1, None, None)
    w2d = wt.view(O, C).to(DEV)
    wp, wpt, bp = Km.fold_weights(w2d, scale, shift, dtype, want_transpose=True)
    xd, dyd = to_dev_nhwc(x, dtype), to_dev_nhwc(dy, dtype)

    # forward
    yd, _ = Km.conv_gemm(xd, wp, O, 1, 1, st, 0, 1, None, bp)
    stage = xs2d @ wp.cpu().double().t() + bp.cpu().double()[None, :]
    assert_close(yd.float().cpu().view(Mo, O), stage, dtype, "stage fwd")
    assert_close(to_cpu_nchw(yd), y, dtype, "folded fwd", fac=2)

    # weight-gradient split partials
    parts = Km.conv_wgrad(xd, dyd, O, 1, 1, st, 0, 1, None, raw_partial=True)
    S = _splits(gid, dtype, parts)
    g64 = parts.cpu().double().sum(0).view(O, C)
    assert_close(g64, dy2d.t() @ xs2d, torch.float32, "stage wgrad", fac=20)

    # reduce: from the partials as they are, from their sum and from a re-weighted three-way split
    db = dy.double().sum((0, 2, 3)).float()  # general case: the constant W@shift carries gradient
    dbd = db.to(DEV)
    dW, dsdt = Km.fold_bwd_reduce(w2d, parts, scale, shift, dbd)
    assert dsdt.shape[0] == (1 if O < 128 else 64)
    rref = _reduce_ref(wt.view(O, C), g64, scale.cpu(), shift.cpu(), db)
    _check_reduce(dW, dsdt, rref, C, True, "stage reduce (%d splits)" % S)
    tot = parts.sum(0)
    fake = torch.stack([tot * 0.25, tot * 0.5, tot * 0.25])
    for pp in (tot.view(O, C), fake):
        dW2, dsdt2 = Km.fold_bwd_reduce(w2d, pp.contiguous(), scale, shift, dbd)
        assert_close(dW2.cpu(), dW.cpu().double(), torch.float32, "fold dW from splits", fac=5)
        assert_close(dsdt2.sum(0).cpu(), dsdt.sum(0).cpu().double(), torch.float32,
                     "fold dsdt from splits", fac=20)

    # finalize
    fin = Km.fold_bwd_finalize(dsdt, M, mean, invstd, gd, scale)
    dgamma, dbeta, c0, c1 = fin
    _check_finalize(fin, _finalize_ref(dsdt.cpu(), float(M), mean.cpu(), invstd.cpu(), gamma,
                                       scale.cpu(), 1.0), "stage finalize")

    # data gradient with the correction
    acc = dy2d @ wpt.cpu().double().t()
    corr = c0.cpu().double()[None, :] + c1.cpu().double()[None, :] * x2d
    if st == 1:
        dx, _ = Km.conv_gemm(dyd, wpt, C, 1, 1, 1, 0, 1, ep=(xd, c0, c1))
        assert_close(dx.float().cpu().view(M, C), acc - corr, dtype, "stage dx")
    else:
        g, _ = Km.conv_gemm(dyd, wpt, C, 1, 1, 1, 0, 1, scatter=(H, W, st))
        ones = torch.ones(C, device=DEV)
        dx = Km.bn_bwd_apply(g, xd, (Km.PRO_AFFINE, ones, ones), c0, c1, out=g)
        full = torch.zeros(N, H, W, C, dtype=torch.float64)
        full[:, ::st, ::st] = acc.view(N, Ho, Wo, C)
        # (the scattered GEMM result is stored in `dtype` before the correction pass rounds
        # again: two roundings, twice the one-rounding bar)
        assert_close(dx.float().cpu().view(M, C), full.view(M, C) - corr, dtype, "stage dx",
                     fac=2)
        skipped = torch.ones(H, W, dtype=torch.bool)
        skipped[::st, ::st] = False
        assert_close(dx.float().cpu()[:, skipped], -corr.view(N, H, W, C)[:, skipped], dtype,
                     "dx at the pixels the stride skips")

    # the whole chain against autograd
    assert_close(dW.view(O, C, 1, 1).cpu(), dW_ref, torch.float32, "folded dW", fac=50)
    assert_close(dgamma.cpu(), dgamma_ref, torch.float32, "folded dgamma", fac=50)
    assert_close(dbeta.cpu(), dbeta_ref, torch.float32, "folded dbeta", fac=50)
    assert_close(to_cpu_nchw(dx), dx_ref, dtype, "folded dx", fac=3)
