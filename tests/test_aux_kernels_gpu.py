"""GPU parity of the small kernels around the convolutions, past the sizes at which their loops
run a second time or their launch geometry changes: max-pool and adaptive average pool
(csrc/pool.hip), the HRNet fuse (csrc/resize.hip: nearest_add / nearest_sum_bwd), the row softmax
(csrc/attention.hip) with DANet's position / channel attention on top of it, and GroupNorm
(csrc/groupnorm.hip).

References are torch CPU ops in float64 on the same seeded inputs, rounded to the compute dtype
first; bars are `_util.assert_close` (2e-5 fp32 / 6e-3 bf16 of the output scale) times the `fac`
the one-shape test of the same op in test_ops_gpu.py uses.  What each case reaches:

  max-pool      even / odd / one-row maps, k/stride/pad other than 3/2/1, all-negative inputs (the
                padding is -inf, not 0), tie-heavy inputs (first maximum wins, like ATen), a pitched
                input, and 363 x 363 x 16 = 2,108,304 output vectors: past the 8192 x 256 threads
                of the capped grid, so the grid-stride loop takes a second trip (backward: 4+)
  adaptive pool two pixel chunks (partial rows + the fp32 column sum), 32-vector channel blocks
                with several blockIdx.x, ragged channel blocks, one pixel per bin, disjoint bins,
                a pitched input, a backward past the grid cap
  HRNet fuse    2,166,784 vectors (second trip, forward and block-sum backward), 3 / 5 / 10
                channel vectors per pixel, x / r / out as slices of NaN-filled wider buffers,
                shift 0
  row softmax   L = 1 .. 2401 (up to ten trips of the 256-thread row loops), every dtype pair,
                both signs, a pitched input, rows that overflow expf without the max pass
  DANet         P = 323 / L = 264 (rows longer than one trip) and 65 x 65 x 384 (the wide and
                direct-to-LDS GEMM classes, K = 4232 not a multiple of 32)
  GroupNorm     3, 5 and 10 channels per group (groups straddle the 4- / 8-channel vectors), a
                group mean of 8 sigma, pitched x and dz"""
import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
NAN = float("nan")
GRID_CAP = 8192 * 256  # threads of the capped grid of the grid-stride kernels


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def F():
    from segmentron_amd import functional
    return functional


def _vec(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def _act_ref(x, mode, scale, shift):
    if mode & 2:
        x = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if mode & 1:
        x = torch.relu(x)
    return x


def _pro(mode, c, seed, negative_shift=False):
    """-> (device prologue triple, scale, shift): scale in [0.5, 1.5), shift ~ 0.3 * randn."""
    if not (mode & 2):
        return (mode, None, None), None, None
    s = torch.rand(c, generator=torch.Generator().manual_seed(seed)) + 0.5
    t = rnd((c,), seed + 1, 0.3)
    if negative_shift:
        t = -t.abs()
    return (mode, s.to(DEV), t.to(DEV)), s, t


# ------------------------------------------------------------------------------ max-pool
def _maxpool_case(x, dtype, k, stride, pad, mode, what, pitch=False, seed=4, negative_shift=False):
    """forward values and the backward through the returned indices against
    TF.max_pool2d(act(x)) and its autograd in float64; -> (gx, reference gradient)"""
    N, C, H, W = x.shape
    pro, s, t = _pro(mode, C, seed, negative_shift)
    xa = _act_ref(x.double(), mode, None if s is None else s.double(),
                  None if t is None else t.double())
    # The kernel activates in fp32 (one fused multiply-add) and compares fp32 values: two
    # activations that differ only below fp32 are a tie on the device and the first one wins, so
    # the reference pools the fp32-rounded activations too (8.4 M windows of the grid-stride case
    # hold such a pair among their largest two about once).  Identity without an affine prologue.
    xa = xa.float().double().requires_grad_()
    ref = TF.max_pool2d(xa, k, stride, pad)
    kw = dict(pitch=C + 16, off=8) if pitch else {}
    y, idx = K().maxpool(to_dev_nhwc(x, dtype, **kw), k, stride, pad, pro)
    assert tuple(y.shape) == (N,) + tuple(ref.shape[2:]) + (C,), what
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, what + " fwd")
    g = quant(rnd(tuple(ref.shape), 2), dtype)
    ref.backward(g.double())
    gx = to_cpu_nchw(K().maxpool_bwd(to_dev_nhwc(g, dtype, **kw), idx, (H, W), k, stride, pad))
    # ties pick the first maximum in (kh, kw) scan order, like ATen: the gradients agree up to the
    # rounding of the sums of overlapping windows
    assert_close(gx, xa.grad, dtype, what + " bwd")
    return gx, xa.grad


MAXPOOL_HW = [(17, 21), (18, 22), (16, 9), (1, 7), (2, 2)]
MAXPOOL_KSP = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (5, 2, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ksp", MAXPOOL_KSP, ids=lambda v: "k%ds%dp%d" % v)
def test_maxpool_geometry_sweep(ksp, dtype):
    """Odd, even, one-row and 2 x 2 maps under every (k, stride, pad); C = 40 is 10 fp32 / 5 bf16
    channel vectors per pixel."""
    k, stride, pad = ksp
    ran = 0
    for H, W in MAXPOOL_HW:
        if (H + 2 * pad - k) // stride + 1 < 1 or (W + 2 * pad - k) // stride + 1 < 1:
            continue  # empty output
        x = quant(rnd((2, 40, H, W), 1 + H), dtype)
        _maxpool_case(x, dtype, k, stride, pad, 0, "maxpool %dx%d %s" % (H, W, ksp))
        ran += 1
    assert ran >= 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("ksp", [(3, 2, 1), (5, 2, 2)], ids=lambda v: "k%ds%dp%d" % v)
def test_maxpool_pads_with_minus_infinity(ksp, mode, dtype):
    """Every activated value is negative (x = -|x| - 1, scale > 0, shift <= 0): a kernel that
    padded with 0 returns 0 in every border window, and no border input would get a gradient."""
    k, stride, pad = ksp
    H, W = 17, 22
    x = quant(-rnd((2, 40, H, W), 3).abs() - 1, dtype)
    gx, gref = _maxpool_case(x, dtype, k, stride, pad, mode, "maxpool -inf", seed=6,
                             negative_shift=True)
    border = torch.zeros((H, W), dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    hit = (gref != 0) & border
    assert hit.sum() > 100, "the reference sends no gradient to the border"
    assert (gx[hit] != 0).all(), "border inputs that win a window got no gradient"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("data", ["relu_zeros", "four_values"])
def test_maxpool_ties_pick_the_first_maximum_like_aten(data, dtype):
    """Tie-heavy inputs: a mode-3 prologue on data with ~50 % negatives (many all-zero windows), and
    an input of four distinct values; the backward must send each window's gradient where ATen
    does."""
    N, C, H, W = 2, 40, 18, 22
    if data == "relu_zeros":
        x, mode = quant(rnd((N, C, H, W), 5), dtype), 3
    else:
        pick = torch.randint(0, 4, (N, C, H, W), generator=torch.Generator().manual_seed(9))
        x, mode = torch.tensor([-1.0, -0.5, 0.5, 1.0])[pick], 0
        assert torch.equal(quant(x, torch.bfloat16), x)
    for ksp in ((3, 2, 1), (3, 1, 1)):
        _maxpool_case(x, dtype, *ksp, mode, "maxpool ties %s %s" % (data, ksp))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_maxpool_pitched_input_and_gradient(dtype):
    """x and dy as channel slices of NaN-filled wider buffers (row pitch C + 16)."""
    x = quant(rnd((2, 40, 18, 21), 7), dtype)
    _maxpool_case(x, dtype, 3, 2, 1, 3, "maxpool pitched", pitch=True)


def test_maxpool_grid_stride_second_trip():
    """fp32 [1, 64, 725, 726], 3/2/1: 363 x 363 x 16 = 2,108,304 output vectors > 2,097,152
    threads, so the forward walks the tensor twice (ragged second trip); the backward's
    725 x 726 x 16 = 8.4 M vectors take four trips and a ragged fifth."""
    N, C, H, W = 1, 64, 725, 726
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert GRID_CAP < N * Ho * Wo * (C // 4) < 2 * GRID_CAP and N * H * W * (C // 4) > 4 * GRID_CAP
    _maxpool_case(rnd((N, C, H, W), 11), torch.float32, 3, 2, 1, 3, "maxpool grid-stride")


# ------------------------------------------------------------------------------ adaptive avg pool
def _avgpool_case(N, C, H, W, o, dtype, pitch=False):
    x = quant(rnd((N, C, H, W), 1), dtype).double().requires_grad_()
    ref = TF.adaptive_avg_pool2d(x, o)
    kw = dict(pitch=C + 16, off=8) if pitch else {}
    xd = to_dev_nhwc(x.detach().float(), dtype, **kw)
    sums = K().adaptive_avgpool_sums(xd, o)
    areas = K().adaptive_bin_areas(H, W, o, sums.device)
    got = (sums / areas.view(1, o, o, 1)).cpu().permute(0, 3, 1, 2)
    what = "adaptive pool %s o=%d" % ((N, C, H, W), o)
    assert_close(got, ref.detach(), torch.float32, what + " fwd", fac=5)
    g = quant(rnd(tuple(ref.shape), 2), dtype)
    ref.backward(g.double())
    gx = K().adaptive_avgpool_bwd(to_dev_nhwc(g, dtype, **kw), (H, W))
    assert_close(to_cpu_nchw(gx), x.grad, dtype, what + " bwd")


AVGPOOL_CASES = [
    (2, 2048, 47, 45, 1),   # 2 chunks; 32-vector channel blocks, 8 (bf16) / 16 (fp32) of them
    (1, 256, 95, 93, 2),    # 2 chunks, overlapping bins
    (2, 40, 13, 17, 3),     # CV = 10 / 5: ragged channel block
    (1, 48, 6, 6, 6),       # one pixel per bin
    (1, 48, 7, 6, 6),       # one pixel per bin along W, overlapping two-row bins along H
    (2, 48, 12, 18, 6),     # bins that do not overlap
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", AVGPOOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_adaptive_avgpool_chunks_channel_blocks_and_bins(case, dtype):
    N, C, H, W, o = case
    from segmentron_amd._lib import LIB
    chunks = LIB.query("seg_adaptive_avgpool_chunks", H, W, o)
    if case in AVGPOOL_CASES[:2]:
        assert chunks > 1, "the case no longer reaches the multi-chunk partial rows"
    _avgpool_case(N, C, H, W, o, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_adaptive_avgpool_pitched_input(dtype):
    _avgpool_case(2, 40, 13, 17, 3, dtype, pitch=True)
    _avgpool_case(1, 64, 95, 93, 2, dtype, pitch=True)  # ... with two chunks


def test_adaptive_avgpool_backward_grid_stride_second_trip():
    """fp32 [1, 64, 368, 368], o = 2: 2,166,784 gradient vectors, past the capped grid."""
    N, C, H, W, o = 1, 64, 368, 368, 2
    assert N * H * W * (C // 4) > GRID_CAP
    g = rnd((N, C, o, o), 2)
    x = torch.zeros((N, C, H, W), dtype=torch.float64, requires_grad=True)
    TF.adaptive_avg_pool2d(x, o).backward(g.double())
    gx = K().adaptive_avgpool_bwd(to_dev_nhwc(g, torch.float32), (H, W))
    assert_close(to_cpu_nchw(gx), x.grad, torch.float32, "adaptive pool bwd past the grid cap")


# ------------------------------------------------------------------------------ HRNet fuse
def _fuse_case(N, C, H, W, shift, post_relu, mode_x, mode_r, dtype, sliced=False):
    """y = relu?(act_x(x) + nearest_up_{2^shift}(act_r(r))) and the block-sum backward of the
    upsampled operand; `sliced`: x, r, out and the gradient are channel slices of NaN-filled
    buffers, and nothing outside `out` may be written.  -> (y, masked gradient) on the device"""
    Hr, Wr = H >> shift, W >> shift
    x = quant(rnd((N, C, H, W), 1), dtype)
    r = quant(rnd((N, C, Hr, Wr), 2), dtype)
    pro_x, sx, tx = _pro(mode_x, C, 7)
    pro_r, sr, tr = _pro(mode_r, C, 5)
    xa = x.double().requires_grad_()
    ra = r.double().requires_grad_()
    d = lambda v: None if v is None else v.double()
    up = TF.interpolate(_act_ref(ra, mode_r, d(sr), d(tr)), scale_factor=2 ** shift, mode="nearest")
    pre = _act_ref(xa, mode_x, d(sx), d(tx)) + up
    ref = torch.relu(pre) if post_relu else pre
    what = "nearest_add %s shift %d" % ((N, C, H, W), shift)
    kw = dict(pitch=C + 16, off=8) if sliced else {}
    xd, rd = to_dev_nhwc(x, dtype, **kw), to_dev_nhwc(r, dtype, **kw)
    if sliced:
        buf = torch.full((N, H, W, C + 16), NAN, dtype=dtype, device=DEV)
        y = K().nearest_add(xd, pro_x, rd, pro_r, shift, post_relu, out=buf[..., 8:8 + C])
        assert y.data_ptr() == buf[..., 8:8 + C].data_ptr()
        assert torch.isnan(buf[..., :8].float()).all() and torch.isnan(buf[..., 8 + C:].float()).all(), \
            what + ": wrote outside the out= slice"
    else:
        y = K().nearest_add(xd, pro_x, rd, pro_r, shift, post_relu)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, what + " fwd")
    g = quant(rnd(tuple(ref.shape), 3), dtype)
    if post_relu:
        # backward reference with the ReLU decisions of the HIP forward: a sum within fp32 rounding
        # of zero may land on either side (millions of elements hold a few), and one flipped unit
        # moves a block sum by its whole gradient.  Decisions may differ ONLY there.
        mask = to_cpu_nchw(y) > 0
        flips = mask != (pre.detach() > 0)
        assert (pre.detach().abs()[flips] < 1e-6).all(), what + ": ReLU decisions differ off a tie"
        (pre * mask.double()).backward(g.double())
    else:
        ref.backward(g.double())
    gd = to_dev_nhwc(g, dtype, **kw)
    if post_relu:
        gd = K().bn_bwd_apply(gd, y, (1, None, None))
        if sliced:  # (the masked gradient comes back dense: slice it again)
            gd = to_dev_nhwc(to_cpu_nchw(gd), dtype, **kw)
    gr = K().nearest_sum_bwd(gd, shift)
    # d/d(act_r(r)); the BN affine backward itself is test_bn_backward_matches_autograd's
    want = ra.grad if sr is None else ra.grad / sr.double().view(1, -1, 1, 1)
    assert_close(to_cpu_nchw(gr), want, dtype, what + " nearest_sum_bwd", fac=4)
    return y, gd


def test_hrnet_fuse_grid_stride_second_trip():
    """fp32 [1, 64, 368, 368], shift 3, ReLU on x, affine on r, ReLU behind the sum: 2,166,784
    vectors, so nearest_add takes a second trip; nearest_sum_bwd with shift 0 (the identity block
    sum) on the same gradient takes a second trip too."""
    N, C, H, W = 1, 64, 368, 368
    assert N * H * W * (C // 4) > GRID_CAP
    _, gd = _fuse_case(N, C, H, W, 3, True, 1, 2, torch.float32)
    same = K().nearest_sum_bwd(gd, 0)
    assert torch.equal(same, gd)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [24, 40])
def test_hrnet_fuse_odd_vector_counts_and_slices(C, shift, dtype):
    """C = 24: 3 bf16 vectors per pixel (6 fp32), C = 40: 5 (10); plain and as slices of NaN-filled
    buffers; shift 0 is the identity upsample."""
    _fuse_case(2, C, 24, 40, shift, shift % 2 == 1, 1, 2, dtype)
    _fuse_case(2, C, 24, 40, shift, shift % 2 == 0, 3, 0, dtype, sliced=True)


# ------------------------------------------------------------------------------ row softmax
SOFTMAX_L = [1, 63, 256, 257, 600, 2401]


def _softmax_rows(R, L, dt_in, seed, scale=1.0):
    """-> (CPU values [R, L] rounded to dt_in, device [R, Lp] view of a NaN-filled [R, Lp + 16]
    buffer whose padding columns L .. Lp - 1 are NaN as well: nothing but the L columns is read)"""
    Lp = (L + 7) // 8 * 8
    v = quant(rnd((R, L), seed, scale), dt_in)
    buf = torch.full((R, Lp + 16), NAN, dtype=dt_in)
    buf[:, 8:8 + L] = v.to(dt_in)
    return v, buf.to(DEV)[:, 8:8 + Lp]


@pytest.mark.parametrize("dt_out", DTYPES, ids=["to_fp32", "to_bf16"])
@pytest.mark.parametrize("dt_in", DTYPES, ids=["from_fp32", "from_bf16"])
def test_row_softmax_forward_and_backward_past_one_trip(dt_in, dt_out):
    """K.row_softmax / K.row_softmax_bwd against torch.softmax and the analytic backward
    de = sign * a * (g - sum_j a_j g_j), both in float64 (the backward on the `a` the kernel
    stored).  The only error is fp32 arithmetic and the rounding of the output to dt_out: the plain
    bars.  Padding columns L .. Lp - 1 must come out exactly 0."""
    Km = K()
    for L in SOFTMAX_L:
        Lp = (L + 7) // 8 * 8
        for R in (1, 5):
            for sign in (1.0, -1.0):
                what = "row_softmax L=%d R=%d sign=%+d" % (L, R, sign)
                v, e = _softmax_rows(R, L, dt_in, 3 * L + R, 2.0)
                assert e.stride(0) == Lp + 16
                a = Km.row_softmax(e, L, dt_out, sign)
                assert tuple(a.shape) == (R, Lp) and a.dtype == dt_out
                ref = torch.softmax(sign * v.double(), dim=-1)
                assert_close(a[:, :L].cpu(), ref, dt_out, what)
                assert (a[:, L:].float() == 0).all(), what + ": padding columns"
                gv, g = _softmax_rows(R, L, dt_in, 5 * L + R)
                de = Km.row_softmax_bwd(a, g, L, dt_out, sign)
                ac = a[:, :L].cpu().double()
                want = sign * ac * (gv.double() - (ac * gv.double()).sum(-1, keepdim=True))
                assert_close(de[:, :L].cpu(), want, dt_out, what + " bwd")
                assert (de[:, L:].float() == 0).all(), what + " bwd: padding columns"


def test_row_softmax_subtracts_the_row_maximum():
    """fp32 rows drawn at scale 150: max |e| is far above 88, where expf overflows — a kernel
    without the max-subtraction pass returns inf / NaN."""
    for L, sign in ((257, 1.0), (600, -1.0)):
        v, e = _softmax_rows(5, L, torch.float32, 17, 150.0)
        assert (sign * v).max(-1).values.min() > 200
        a = K().row_softmax(e, L, torch.float32, sign)
        assert_close(a[:, :L].cpu(), torch.softmax(sign * v.double(), dim=-1), torch.float32,
                     "row_softmax at scale 150")


# ------------------------------------------------------------------------------ DANet
def _ste_round(t, dtype):
    """Value of t rounded to `dtype`, gradient of t: where the bf16 pipeline STORES an
    intermediate (identity for fp32)."""
    if dtype == torch.float32:
        return t
    return t + (t.detach().to(dtype).double() - t.detach())


def _pam_reference(q, k, v, x, gamma, dtype):
    """gamma * (V softmax(Q^T K)^T) + x in float64; for bf16 the energies and the attention matrix
    are rounded where the pipeline stores them (straight-through in the backward)."""
    N, C, H, W = x.shape
    pq = q.view(N, -1, H * W).permute(0, 2, 1)
    energy = _ste_round(torch.bmm(pq, k.view(N, -1, H * W)), dtype)
    att = _ste_round(torch.softmax(energy, dim=-1), dtype)
    return gamma * torch.bmm(v.view(N, -1, H * W), att.permute(0, 2, 1)).view(N, C, H, W) + x


def _cam_reference(x, gamma, dtype):
    """gamma * (softmax(max(E) - E) X) + x, E = X X^T; the pipeline keeps the Gram matrix in fp32
    (weight-gradient GEMM partials) and stores the attention matrix in the compute dtype."""
    N, C, H, W = x.shape
    pq = x.view(N, C, -1)
    energy = torch.bmm(pq, pq.permute(0, 2, 1))
    att = torch.softmax(energy.max(-1, keepdim=True)[0].expand_as(energy) - energy, dim=-1)
    att = _ste_round(att, dtype)
    return gamma * torch.bmm(att, pq).view(N, C, H, W) + x


# geometry, scale of q and k, factor on x for CAM (keeps the Gram matrix of H*W pixels in the
# range the one-shape test has)
DANET_CASES = {
    # P = 323 > 256 (PAM rows), L = 264 > 256 (CAM rows): the row loops take a second trip
    "17x19": dict(N=1, H=17, W=19, D=16, C=264, qk=0.8, cam=0.2),
    # P = 4225 >= 4096 pixels with O >= 384: the wide / direct-to-LDS 1x1 kernels, K = Pp = 4232
    # no multiple of 32; the large-map weight-gradient classes; q, k at 0.5: energies of sigma 2
    "65x65": dict(N=1, H=65, W=65, D=64, C=384, qk=0.5, cam=0.05),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(DANET_CASES))
def test_danet_attention_at_real_kernel_classes(case, dtype):
    """functional.position_attention / channel_attention as in
    test_danet_position_and_channel_attention_fwd_bwd, at sizes where the softmax rows are longer
    than one trip and the GEMMs leave the generic kernel.  Reference: float64, for bf16 rounded at
    the two points where the pipeline stores the energies / attention matrix in bf16.

    fac: the one-shape test's 3 (fp32) / 6 (bf16), 5 x that for dgamma.  They are kept: the CPU
    measurement of the bf16-emulated reference against the unrounded float64 one, in units of
    the bf16 bar 6e-3 (a `fac` has to be twice that), stays below them —
        17x19: PAM fwd 0.98, dq 1.54, dk 1.58, dv 1.04, dgamma 0.23; CAM fwd / dx 0.01, dgamma 0.05
        65x65: PAM fwd 0.81, dq 2.32, dk 1.75, dv 2.00, dgamma 0.31; CAM fwd / dx 0.01, dgamma 6.38
    (largest: 2 x 2.32 = 4.6 < 6, and 2 x 6.38 = 12.8 < 30 for CAM's dgamma, one scalar out of a
    cancelling sum over 1.6 M products).  Energies measure sigma 2.6 / 2.0 (PAM) and Gram diagonals
    of 6.4 / 5.2 (CAM; the one-shape test has 7.8)."""
    Fm = F()
    c = DANET_CASES[case]
    N, H, W, D, C = c["N"], c["H"], c["W"], c["D"], c["C"]
    fac = 3 if dtype == torch.float32 else 6
    x = quant(rnd((N, C, H, W), 1, 0.7), dtype)
    q = quant(rnd((N, D, H, W), 2, c["qk"]), dtype)
    k = quant(rnd((N, D, H, W), 3, c["qk"]), dtype)
    v = quant(rnd((N, C, H, W), 4), dtype)
    gamma = torch.tensor([0.7])
    g = quant(rnd((N, C, H, W), 5), dtype)
    # ---- PAM
    leaves = [t.double().requires_grad_() for t in (q, k, v, x, gamma)]
    ref = _pam_reference(*leaves, dtype)
    ref.backward(g.double())
    dev = [to_dev_nhwc(t, dtype).requires_grad_() for t in (q, k, v, x)]
    gd = gamma.to(DEV).requires_grad_()
    y = Fm.position_attention(*dev, gd)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "PAM fwd", fac=fac)
    y.backward(to_dev_nhwc(g, dtype))
    for name, d, r in zip("qkvx", dev, leaves):
        assert_close(to_cpu_nchw(d.grad), r.grad, dtype, "PAM d" + name, fac=fac)
    assert_close(gd.grad.cpu(), leaves[4].grad, dtype, "PAM dgamma", fac=fac * 5)
    # ---- CAM
    xc = quant(x * c["cam"], dtype)
    xr = xc.double().requires_grad_()
    gr = gamma.double().requires_grad_()
    ref = _cam_reference(xr, gr, dtype)
    ref.backward(g.double())
    xd = to_dev_nhwc(xc, dtype).requires_grad_()
    gd = gamma.to(DEV).requires_grad_()
    y = Fm.channel_attention(xd, gd)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "CAM fwd", fac=fac)
    y.backward(to_dev_nhwc(g, dtype))
    assert_close(to_cpu_nchw(xd.grad), xr.grad, dtype, "CAM dx", fac=fac)
    assert_close(gd.grad.cpu(), gr.grad, dtype, "CAM dgamma", fac=fac * 5)


# ------------------------------------------------------------------------------ GroupNorm
def _group_norm_case(geom, dtype, mean=0.4, std=1.5, pitch=False):
    N, H, W, C = geom
    gn = torch.nn.GroupNorm(min(32, C), C).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.5)
        gn.bias.copy_(rnd((C,), 4, 0.3))
    x = quant(rnd((N, C, H, W), 1) * std + mean, dtype)
    dz = quant(rnd((N, C, H, W), 2), dtype)
    xr = x.double().requires_grad_()
    wr = gn.weight.detach().cpu().double().requires_grad_()
    br = gn.bias.detach().cpu().double().requires_grad_()
    ref = TF.group_norm(xr, gn.num_groups, wr, br, gn.eps)
    ref.backward(dz.double())
    kw = dict(pitch=C + 16, off=8) if pitch else {}
    xd = to_dev_nhwc(x, dtype, **kw).requires_grad_()
    z = F().group_norm(xd, gn).t
    z.backward(to_dev_nhwc(dz, dtype, **kw))
    what = "gn %s " % (geom,)
    assert_close(to_cpu_nchw(z.detach()), ref.detach(), dtype, what + "z", fac=2)
    assert_close(to_cpu_nchw(xd.grad), xr.grad, dtype, what + "dx", fac=4)
    xh = ((x.double() - x.double().mean()) / x.double().std()).abs()
    scale = (dz.double().abs() * xh).sum((0, 2, 3)).max().item()
    assert_close(gn.weight.grad.cpu(), wr.grad, torch.float32, what + "dgamma", scale=scale, fac=20)
    assert_close(gn.bias.grad.cpu(), br.grad, torch.float32, what + "dbeta",
                 scale=dz.double().abs().sum((0, 2, 3)).max().item(), fac=20)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", [(2, 9, 11, 96), (2, 9, 11, 160), (1, 33, 35, 320)],
                         ids=lambda g_: "x".join(map(str, g_)))
def test_group_norm_groups_that_straddle_a_vector(geom, dtype):
    """32 groups of 3, 5 and 10 channels: group boundaries fall inside the 4- (fp32) and 8-channel
    (bf16) vectors the moments and affine kernels move."""
    _group_norm_case(geom, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_group_norm_with_a_mean_of_eight_sigma(dtype):
    """x = randn + 8: the forward takes var = E[x^2] - mean^2 = 65 - 64 from fp32 partial sums
    finished in float64.  A CPU emulation of the kernel's summation order puts the relative error
    of rstd at 4e-7 or less (fp32 partials of ~14 terms each, float64 above them), 65 times the
    rounding of a sum that does not cancel.  Bars as in the zero-mean test: they hold the
    cancellation to 4e-5 of the output scale (z) and 8e-5 (dx)."""
    _group_norm_case((2, 17, 23, 64), dtype, mean=8.0, std=1.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_group_norm_pitched_input_and_gradient(dtype):
    """x and dz as channel slices (pitch C + 16, offset 8) of NaN-filled buffers."""
    _group_norm_case((2, 9, 11, 160), dtype, pitch=True)
