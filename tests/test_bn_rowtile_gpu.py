"""GPU parity of the row-tile BatchNorm element-wise kernels (csrc/bn.hip: bn_apply,
bn_bwd_reduce, bn_bwd_apply, sum_n) on every launch geometry of `ew_geom`, and of the
partial-row finalizers (bn_finalize_p, bn_bwd_finalize_p) on their own.

Geometry: the three regimes of `ew_geom` (column blocks for up to 32 channel vectors per row,
whole-row blocks up to 512 vectors with idle lanes in the last wave, column blocks again above
512) are asserted through the host query `hip_ops.ew_geom`, and every row count is sized from the
rows per block the library reports: one row, one unrolled tile of EW_UN = 4 rows per thread
(- 1, exact, + 1: the clamped look-ahead loads) and one count past the grid cap, where the blocks
walk the tensor a second, ragged time.  Rows are laid out as three images whose size is no
multiple of the rows per block wherever the count allows it (the past-the-cap count is rounded up
to the next such multiple of three: at most five rows more than gridDim.y * tile + tile + 1), so
one unrolled batch of a thread takes its `chan_mul` row from two images.

Reference: plain torch float64 on the CPU on the values after rounding to the dtype; bars are
`_util.assert_close` (2e-5 fp32 / 6e-3 bf16 of the output scale).  ReLU / ReLU6 masks cannot hang
on rounding: every activated value is kept 1e-3 away from 0 and 6 on the CPU (asserted, nothing
is excluded from a comparison), and exact boundaries (0, -0, 6 through an exact affine) are
planted on known rows, the last one included.

Everything that needs no device (`_case`, `_finalize_case`, `cpu_selfcheck`) is plain CPU code."""
import pytest
import torch

from _util import DEV, assert_close, quant, rnd, tol

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
NAN = float("nan")
EW_UN = 4        # rows per thread and iteration of the row-tile kernels
MARGIN = 1e-3    # distance every un-planted activated value keeps from the mask boundaries
MODES = [0, 1, 3, 7]

# C -> (lanes per row, rows per block, threads, gx) in fp32 and in bf16
GEOM = {
    8: ((8, 32, 256, 1), (8, 32, 256, 1)),            # 2 / 1 live lanes of 8
    136: ((34, 15, 512, 1), (8, 32, 256, 3)),         # whole row, 2 idle | columns, ragged gx
    264: ((66, 7, 512, 1), (33, 15, 512, 1)),         # whole row, 50 | 17 idle
    512: ((128, 2, 256, 1), (64, 4, 256, 1)),         # whole row, no idle lane
    728: ((182, 2, 384, 1), (91, 4, 384, 1)),         # whole row, 20 idle
    2048: ((512, 1, 512, 1), (256, 1, 256, 1)),       # CV = 512: the upper edge | whole row
    2056: ((8, 32, 256, 65), (257, 1, 320, 1)),       # CV = 514: columns | whole row, 63 idle
    4104: ((8, 32, 256, 129), (8, 32, 256, 65)),      # columns, CV > 512 in both
}
SWEEP_C = (264, 728, 2056)  # the full row sweep; the other C: tile + 1 and past the cap
REGIMES = {"columns gx=1", "columns ragged gx>1", "whole row idle", "whole row full", "CV=512",
           "CV>512"}


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def _vec(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def _regimes(C, dtype, geo):
    """Names of the launch regimes a case is in, from what the library reports."""
    cv = C // _vec(dtype)
    out = set()
    if geo["lanes"] == cv and geo["lanes"] > 32:
        assert geo["gx"] == 1
        out.add("whole row idle" if geo["threads"] > geo["lanes"] * geo["rows"] else "whole row full")
    else:
        assert geo["lanes"] * geo["rows"] == geo["threads"]
        if geo["gx"] == 1:
            out.add("columns gx=1")
        elif cv % geo["lanes"]:
            out.add("columns ragged gx>1")
    if cv == 512:
        out.add("CV=512")
    if cv > 512:
        out.add("CV>512")
    return out


def _layout(M, rpb):
    """(N, H, W) with N * H * W = M: three images whose size is no multiple of the rows per block
    (of the tile when a block has one row), else one image."""
    hw = M // 3
    if M % 3 == 0 and hw % (rpb * EW_UN) and (rpb == 1 or hw % rpb):
        return 3, 1, hw
    return 1, 1, M


def _rows_list(C, dtype):
    """Row counts of a (C, dtype) case, from the library's rows per block and grid cap."""
    rpb = K().ew_geom(dtype, C, 1)["rows"]
    tile = rpb * EW_UN
    cap = K().ew_geom(dtype, C, 1 << 30)["gy"]
    m = cap * tile + tile + 1
    while _layout(m, rpb)[0] != 3:
        m += 1
    assert m <= cap * tile + tile + 6
    return ([1, tile - 1, tile, tile + 1, m] if C in SWEEP_C else [tile + 1, m]), tile


def _second_pass(C, dtype, M, key):
    """True when the blocks of the launch walk the rows more than once (asserted per kernel)."""
    geo = K().ew_geom(dtype, C, M)
    return geo[key] * geo["rows"] * EW_UN < M


# ------------------------------------------------------------------------------ CPU side
def _clear_margins(x, s, t, dtype):
    """Replace every element whose raw or affine value is within MARGIN of a mask boundary (0, and
    6 for ReLU6) by another value the dtype holds, until none is left."""
    s64, t64 = s.double(), t.double()
    for _ in range(64):
        y = x.double() * s64 + t64
        bad = (x.abs() < MARGIN) | (y.abs() < MARGIN) | ((y - 6).abs() < MARGIN)
        if not bad.any():
            return x
        x = torch.where(bad, quant(x + 0.25, dtype), x)
    raise AssertionError("mask margins not cleared")


def _min_margin(x, s, t, planted):
    y = x.double() * s.double() + t.double()
    d = torch.minimum(torch.minimum(x.double().abs(), y.abs()), (y - 6).abs())
    d[planted] = float("inf")
    return d.min().item()


def _case(C, dtype, M, seed=0):
    """All CPU data of one (C, dtype, M) case, rows x channels, already rounded to the dtype."""
    rpb = K().ew_geom(dtype, C, M)["rows"]
    N, H, W = lay = _layout(M, rpb)
    gen = torch.Generator().manual_seed(1000 * C + M + seed)
    s = torch.rand(C, generator=gen) + 0.5
    t = rnd((C,), C + 1, 0.3)
    s[:8], t[:8] = 1.0, 0.0  # the first channel vector: fma(x, 1, 0) is exact
    # x * 3: some activated values lie above 6 (ReLU6's upper branch)
    x = _clear_margins(quant(rnd((M, C), C + M + 2, 3.0), dtype), s, t, dtype)
    planted = torch.zeros(M, C, dtype=torch.bool)
    prow = sorted({0, M // 2, M - 1})
    for p in prow:  # exact boundaries: y = 0, -0 and 6 on the first, a middle and the last row
        x[p, 0], x[p, 1], x[p, 2] = 0.0, -0.0, 6.0
        planted[p, :3] = True
    mm = _min_margin(x, s, t, planted)
    assert mm >= MARGIN, "smallest mask margin of the reference %.3e" % mm
    assert torch.equal(x, quant(x, dtype))
    c = dict(C=C, dtype=dtype, M=M, lay=lay, s=s, t=t, x=x, prow=prow,
             img=torch.arange(M) // (H * W),
             g=quant(rnd((M, C), C + M + 3), dtype), r=quant(rnd((M, C), C + M + 4), dtype),
             sr=torch.rand(C, generator=gen) + 0.5, tr=rnd((C,), C + 5, 0.3),
             cm=(torch.rand(N, C, generator=gen) > 0.3).float() / 0.7,
             em=quant((torch.rand(M, C, generator=gen) > 0.3).float() / 0.7, dtype),
             c0=rnd((C,), C + 6, 0.05), c1=rnd((C,), C + 7, 0.3))
    return c


def _act(x, mode, s, t):
    x = x.double()
    if mode & 2:
        x = x * s.double() + t.double()
    if mode & 1:
        x = torch.relu(x)
    if mode & 4:
        x = x.clamp(max=6.0)
    return x


def _masked_grad(c, mode, mul):
    """g' = g * chan_mul * elem_mul * d act / d y  (0 at y = 0; 0 at y = 6 for ReLU6, 1 for ReLU)"""
    gp = c["g"].double()
    if mul:
        gp = gp * c["cm"].double()[c["img"]] * c["em"].double()
    if mode & 1:
        y = c["x"].double() * c["s"].double() + c["t"].double() if mode & 2 else c["x"].double()
        on = (y > 0) & (y < 6) if mode & 4 else y > 0
        gp = gp * on
    return gp


def _pro(c, mode):
    return (mode, c["s"].to(DEV), c["t"].to(DEV)) if mode & 2 else (mode, None, None)


def _dev(rows, c, pitch=None, off=0):
    """CPU rows [M, C] -> device NHWC view of the case's layout (optionally a channel slice of a
    NaN-filled buffer of `pitch` channels)."""
    M, C = rows.shape
    N, H, W = c["lay"]
    t = rows.to(c["dtype"])
    if pitch is None:
        return t.view(N, H, W, C).to(DEV, copy=True)
    buf = torch.full((M, pitch), NAN, dtype=c["dtype"])
    buf[:, off:off + C] = t
    return buf.view(N, H, W, pitch).to(DEV)[..., off:off + C]


def _nan_slice(c, pitch, off):
    N, H, W = c["lay"]
    buf = torch.full((N, H, W, pitch), NAN, dtype=c["dtype"], device=DEV)
    return buf, buf[..., off:off + c["C"]]


def _host(t):
    return t.detach().float().cpu().reshape(-1, t.shape[-1])


def _flanks_nan(buf, off, C):
    return bool(torch.isnan(buf[..., :off]).all()) and bool(torch.isnan(buf[..., off + C:]).all())


# ------------------------------------------------------------------------------ geometry
def test_geometry_table_and_regimes():
    """Every row of the geometry table through the query, both dtypes; the cases cover every
    regime; every (C, dtype) has a row count past the grid cap for each kernel."""
    seen = set()
    for C, per in GEOM.items():
        for dtype, want in zip(DTYPES, per):
            geo = K().ew_geom(dtype, C, 1000)
            assert (geo["lanes"], geo["rows"], geo["threads"], geo["gx"]) == want, (C, dtype, geo)
            assert geo["gx"] * geo["lanes"] >= C // _vec(dtype)
            seen |= _regimes(C, dtype, geo)
            rows, tile = _rows_list(C, dtype)
            assert tile == want[1] * EW_UN
            assert _second_pass(C, dtype, rows[-1], "gy") and _second_pass(C, dtype, rows[-1], "gy_reduce")
            assert _layout(rows[-1], want[1])[0] == 3
    assert seen >= REGIMES, REGIMES - seen
    for dtype, live in zip(DTYPES, (2, 1)):  # C = 8: 2 (fp32) / 1 (bf16) live lanes of 8
        geo = K().ew_geom(dtype, 8, 1)
        assert (min(8 // _vec(dtype), geo["lanes"]), geo["lanes"], geo["gx"]) == (live, 8, 1)
    with pytest.raises(ValueError):
        K().ew_geom(torch.float32, 6, 10)


# ------------------------------------------------------------------------------ bn_apply
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", list(GEOM))
def test_bn_apply(C, dtype):
    """Prologue modes 0 1 3 7; residual (mode 2, wider pitch) + chan_mul + elem_mul (+ post_relu)
    into a NaN-flanked channel slice; the plain call in place, exact at the planted boundaries."""
    vec = _vec(dtype)
    rows, _ = _rows_list(C, dtype)
    assert _second_pass(C, dtype, rows[-1], "gy")
    for M in rows:
        c = _case(C, dtype, M)
        what = "bn_apply C=%d M=%d " % (C, M)
        xd, rd = _dev(c["x"], c, C + 2 * vec, vec), _dev(c["r"], c, C + 3 * vec, 2 * vec)
        emd, cmd = _dev(c["em"], c, C + vec, 0), c["cm"].to(DEV)
        pr = (2, c["sr"].to(DEV), c["tr"].to(DEV))
        for mode in MODES:
            post = mode in (0, 3)
            ref = (_act(c["x"], mode, c["s"], c["t"]) * c["cm"].double()[c["img"]] * c["em"].double()
                   + _act(c["r"], 2, c["sr"], c["tr"]))
            ref = torch.relu(ref) if post else ref
            buf, out = _nan_slice(c, C + 2 * vec, vec)
            y = K().bn_apply(xd, _pro(c, mode), rd, pr, cmd, post, out, elem_mul=emd)
            assert_close(_host(y), ref, dtype, what + "mode %d fused" % mode)
            assert _flanks_nan(buf, vec, C), what + "mode %d wrote outside its slice" % mode
            # plain, in place
            xi = _dev(c["x"], c)
            y = K().bn_apply(xi, _pro(c, mode), out=xi)
            assert y.data_ptr() == xi.data_ptr()
            got = _host(y)
            assert_close(got, _act(c["x"], mode, c["s"], c["t"]), dtype, what + "mode %d in place" % mode)
            for p in c["prow"]:  # act(0) = act(-0) = 0 and act(6) = 6, exactly
                assert got[p, 0] == 0 and got[p, 1] == 0 and got[p, 2] == 6, (what, mode, p, got[p, :3])


# ------------------------------------------------------------------------------ bn_bwd_reduce
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", list(GEOM))
def test_bn_bwd_reduce_partial(C, dtype):
    """(sum g', sum g' x) partial rows of channel slices (g and x of different pitch, NaN around
    them), with chan_mul and elem_mul.

    Bar: the float64 column sums of the partial rows against the float64 sums, on the scale
    sum |term| of each channel, at the plain fp32 bar (2e-5; the conv statistics tests allow 5 x
    that).  A thread adds at most ceil(M / (grid_y * rows_per_block)) terms in fp32 (9 at the row
    counts used here: grid_y is >= M / (8 * rows_per_block) up to its cap, and the past-the-cap
    count is just over twice the cap) and the LDS pass adds rows_per_block <= 32 more: fewer than
    64 fp32 additions, an error below 64 * 2^-24 = 4e-6 of sum |term|.  Nothing is rounded to bf16
    on this path, so bf16 gets the fp32 bar too.

    One dropped or doubled row of 65 000 moves a column sum by 1.5e-5 of that scale, under any such
    bar: every row count is therefore also reduced on small integers (g, x in -3 .. 3, ReLU mask on
    x), where every fp32 sum is exact, and compared bit for bit."""
    vec = _vec(dtype)
    rows, _ = _rows_list(C, dtype)
    assert _second_pass(C, dtype, rows[-1], "gy_reduce")
    for M in rows:
        c = _case(C, dtype, M)
        geo = K().ew_geom(dtype, C, M)
        assert -(-M // (geo["gy_reduce"] * geo["rows"])) + geo["rows"] < 64
        gd, xd = _dev(c["g"], c, C + vec, 0), _dev(c["x"], c, C + 3 * vec, 2 * vec)
        emd, cmd = _dev(c["em"], c, C + 2 * vec, vec), c["cm"].to(DEV)
        for mode in MODES:
            what = "bn_bwd_reduce C=%d M=%d mode %d " % (C, M, mode)
            part = K().bn_bwd_reduce_partial(gd, xd, _pro(c, mode), cmd, emd)
            assert tuple(part.shape) == (geo["gy_reduce"], 2 * C), (what, part.shape)
            got = part.double().sum(0).cpu().view(2, C)
            gp = _masked_grad(c, mode, True)
            gx = gp * c["x"].double()
            for i, term in enumerate((gp, gx)):
                sc = term.abs().sum(0).clamp_min(1e-30)
                assert_close(got[i] / sc, term.sum(0) / sc, torch.float32, what + ("sum g'", "sum g'x")[i],
                             scale=1.0)
        # integers: |sum| <= 9 M < 2^24, exact in any order
        gen = torch.Generator().manual_seed(C + M)
        gi = torch.randint(-3, 4, (M, C), generator=gen).float()
        xi = torch.randint(-3, 4, (M, C), generator=gen).float()
        gpi = gi * (xi > 0)
        part = K().bn_bwd_reduce_partial(_dev(gi, c, C + vec, 0), _dev(xi, c), (1, None, None))
        got = part.double().sum(0).cpu().view(2, C)
        assert torch.equal(got[0], gpi.double().sum(0)) and torch.equal(got[1], (gpi * xi).double().sum(0)), \
            "bn_bwd_reduce C=%d M=%d: integer sums differ" % (C, M)


# ------------------------------------------------------------------------------ bn_bwd_apply
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", list(GEOM))
def test_bn_bwd_apply(C, dtype):
    """dx = scale g' - c0 - c1 x with synthetic c0 / c1 (the kernel apart from the finalize,
    nothing cancels) into a NaN-flanked slice; c0 = c1 = None (evaluation-mode backward, and the
    plain mask for the modes without the affine bit) in place, exact at the planted boundaries."""
    vec = _vec(dtype)
    rows, _ = _rows_list(C, dtype)
    assert _second_pass(C, dtype, rows[-1], "gy")
    for M in rows:
        c = _case(C, dtype, M)
        gd, xd = _dev(c["g"], c, C + vec, 0), _dev(c["x"], c, C + 3 * vec, 2 * vec)
        emd, cmd = _dev(c["em"], c, C + 2 * vec, vec), c["cm"].to(DEV)
        c0d, c1d = c["c0"].to(DEV), c["c1"].to(DEV)
        for mode in MODES:
            what = "bn_bwd_apply C=%d M=%d mode %d " % (C, M, mode)
            gp = _masked_grad(c, mode, True)
            ref = gp * c["s"].double() - c["c0"].double() - c["c1"].double() * c["x"].double() if mode & 2 else gp
            buf, out = _nan_slice(c, C + 2 * vec, vec)
            dx = K().bn_bwd_apply(gd, xd, _pro(c, mode), c0d if mode & 2 else None,
                                  c1d if mode & 2 else None, cmd, out, emd)
            assert_close(_host(dx), ref, dtype, what + "train")
            assert _flanks_nan(buf, vec, C), what + "wrote outside its slice"
            # no c0 / c1, in place
            gi = _dev(c["g"], c)
            dx = K().bn_bwd_apply(gi, xd, _pro(c, mode), out=gi)
            assert dx.data_ptr() == gi.data_ptr()
            gp = _masked_grad(c, mode, False)
            got = _host(dx)
            assert_close(got, gp * c["s"].double() if mode & 2 else gp, dtype, what + "eval, in place")
            for p in c["prow"]:  # scale = 1 on these channels: dx = g' exactly
                g6 = c["g"][p, 2] if mode in (0, 1, 3) else 0.0  # d relu / dy = 1 at 6, d relu6 / dy = 0
                g0 = c["g"][p, :2] if mode == 0 else torch.zeros(2)
                assert torch.equal(got[p, :2], g0.float()) and got[p, 2] == g6, (what, p, got[p, :3])


# ------------------------------------------------------------------------------ sum_n
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("C", SWEEP_C)
def test_sum_n(C, n, dtype):
    """n operands of mixed pitch past the grid cap: bit-exact against the fp32 in-order sum
    rounded once."""
    vec = _vec(dtype)
    rows, _ = _rows_list(C, dtype)
    M = rows[-1]
    assert _second_pass(C, dtype, M, "gy")
    c = dict(dtype=dtype, lay=_layout(M, K().ew_geom(dtype, C, M)["rows"]))
    xs = [quant(rnd((M, C), 10 * C + i), dtype) for i in range(n)]
    devs = [_dev(t, c, C + (1 + i % 3) * vec if i % 2 else None, (i % 3) * vec if i % 2 else 0)
            for i, t in enumerate(xs)]
    got = K().sum_n(devs)
    acc = xs[0].float().clone()
    for t in xs[1:]:
        acc = acc + t.float()
    assert torch.equal(_host(got), quant(acc, dtype))


# ------------------------------------------------------------------------------ finalizers
R_LIST = [1, 31, 32, 33, 255, 256, 257, 1024, 1025, 5000]
EPS, MOM = 1e-3, 0.1


def _finalize_case(R, C, seed=0):
    """Synthetic partial rows [R, 2, C] from real data — the rows of a float64 tensor in R groups,
    per-group (sum x, sum x^2) and (sum g, sum g x) cast to fp32 — and the float64 reference of both
    finalizers on the float64 sums of those same fp32 rows."""
    rows = R + max(3, R // 3)
    gen = torch.Generator().manual_seed(7919 * R + C + seed)
    f64 = dict(generator=gen, dtype=torch.float64)
    x = torch.randn(rows, C, **f64) * (0.5 + 2 * torch.rand(C, **f64)) + torch.randn(C, **f64)
    g = torch.randn(rows, C, **f64)
    grp = torch.arange(rows) * R // rows  # every group gets a row

    def partial(a, b):
        z = torch.zeros(2, R, C, dtype=torch.float64)
        z[0].index_add_(0, grp, a)
        z[1].index_add_(0, grp, b)
        return z.permute(1, 0, 2).contiguous().float()
    c = dict(R=R, C=C, count=float(rows), pf=partial(x, x * x), pb=partial(g, g * x))
    c["gamma"], c["beta"] = torch.rand(C, generator=gen) + 0.5, rnd((C,), C + 1, 0.2)
    c["rm"], c["rv"] = rnd((C,), C + 2, 0.1), torch.rand(C, generator=gen) + 0.5
    c["moff"] = rnd((C,), C + 3, 0.5)
    n = c["count"]
    sx, sxx = c["pf"].double().sum(0)
    mean = sx / n
    var = (sxx / n - mean * mean).clamp_min(0)
    invstd = 1 / torch.sqrt(var + EPS)
    unb = var * n / (n - 1)
    for tag, gm, bt, off in (("", c["gamma"].double(), c["beta"].double(), c["moff"].double()),
                             ("_plain", torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), 0.0)):
        c["fwd" + tag] = dict(mean=mean, invstd=invstd, scale=gm * invstd, shift=bt - mean * gm * invstd,
                              running_mean=(1 - MOM) * c["rm"].double() + MOM * (mean + off),
                              running_var=(1 - MOM) * c["rv"].double() + MOM * unb)
    # the backward finalizer reads the fp32 statistics the forward stored
    c["mean32"], c["invstd32"] = mean.float(), invstd.float()
    mu, ist = c["mean32"].double(), c["invstd32"].double()
    sg, sgx = c["pb"].double().sum(0)
    dg = (sgx - mu * sg) * ist
    for tag, gm in (("", c["gamma"].double()), ("_plain", torch.ones(C, dtype=torch.float64))):
        c1 = gm * ist * (dg / n) * ist
        c["bwd" + tag] = dict(dgamma=dg, dbeta=sg, c0=gm * ist * (sg / n) - c1 * mu, c1=c1)
    return c


def _cast_fac(ref64):
    """`fac` the float64 -> fp32 cast of the reference itself needs on its own scale: 4 x its gap
    over the fp32 bar, at least 1.  Observed gaps: at most 6e-8 (half an fp32 ulp of the largest
    value), so the factor stays 1 — shift and c0 included — and every output is held to 2e-5."""
    gap = (ref64.float().double() - ref64).abs().max().item() / max(ref64.abs().max().item(), 1e-300)
    return max(1.0, 4 * gap / tol(torch.float32)), gap


def _check_outputs(got, ref, what):
    for k, r in ref.items():
        assert_close(got[k].cpu(), r, torch.float32, what + k, fac=_cast_fac(r)[0])


@pytest.mark.parametrize("C", [7, 72, 728])
def test_bn_finalize_p(C):
    """mean, invstd, scale, shift and the running statistics (mean_offset, unbiased variance) from
    1 .. 5000 partial rows: one pass of the eight-rows-in-flight loop, its clamped tail, several
    passes, and the two-level path above 1024 rows; gamma = beta = None."""
    for R in R_LIST:
        c = _finalize_case(R, C)
        pd = c["pf"].to(DEV)
        for tag in ("", "_plain"):
            rm, rv = c["rm"].to(DEV, copy=True), c["rv"].to(DEV, copy=True)  # updated in place
            gm, bt, off = (c["gamma"].to(DEV), c["beta"].to(DEV), c["moff"].to(DEV)) if not tag else (None,) * 3
            out = K().bn_finalize_p(pd, c["count"], gm, bt, EPS, MOM, rm, rv, off)
            got = dict(zip(("mean", "invstd", "scale", "shift"), out), running_mean=rm, running_var=rv)
            _check_outputs(got, c["fwd" + tag], "bn_finalize_p%s R=%d C=%d " % (tag, R, C))
        out = K().bn_finalize_p(pd, c["count"], None, None, EPS, MOM, None, None)  # no running stats
        assert_close(out[3].cpu(), c["fwd_plain"]["shift"], torch.float32, "shift, no running stats")


@pytest.mark.parametrize("C", [7, 72, 728])
def test_bn_bwd_finalize_p(C):
    """dgamma, dbeta, c0, c1 from 1 .. 5000 partial rows, with gamma and with gamma = None."""
    for R in R_LIST:
        c = _finalize_case(R, C)
        pd, md, sd = c["pb"].to(DEV), c["mean32"].to(DEV), c["invstd32"].to(DEV)
        for tag in ("", "_plain"):
            out = K().bn_bwd_finalize_p(pd, c["count"], md, sd, None if tag else c["gamma"].to(DEV))
            _check_outputs(dict(zip(("dgamma", "dbeta", "c0", "c1"), out)), c["bwd" + tag],
                           "bn_bwd_finalize_p%s R=%d C=%d " % (tag, R, C))


# ------------------------------------------------------------------------------ no device needed
def cpu_selfcheck():
    """Everything above that needs no device: the geometry table through the query, the mask
    margins of every case's reference data, the finalizer references and their cast factors."""
    test_geometry_table_and_regimes()
    n, worst = 0, 0.0
    for C in GEOM:
        for dtype in DTYPES:
            for M in _rows_list(C, dtype)[0]:
                c = _case(C, dtype, M)  # asserts the margins
                assert c["lay"][0] * c["lay"][1] * c["lay"][2] == M
                n += 1
    for C in (7, 72, 728):
        for R in R_LIST:
            c = _finalize_case(R, C)
            for k in ("fwd", "fwd_plain", "bwd", "bwd_plain"):
                for r in c[k].values():
                    fac, gap = _cast_fac(r)
                    assert torch.isfinite(r).all() and fac == 1.0
                    worst = max(worst, gap)
    return n, worst
