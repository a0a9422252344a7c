"""GPU parity, per op: every C-ABI kernel vs torch CPU float32/float64 functional ops on the same
seeded inputs (the reference delegates exactly these ops to torch — SURVEY.md §8c).
fp32 path: 2e-5 of the output scale (fp32 accumulation-order noise; the model-level bar is 1e-3).
bf16 path: inputs are rounded to bf16 first, so the only error is the final bf16 rounding of the
output (2^-8) plus accumulation order: 6e-3 of the output scale."""
import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def F():
    from segmentron_amd import functional
    return functional


def _act_ref(x, mode, scale, shift):
    if mode & 2:
        x = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if mode & 1:
        x = torch.relu(x)
    if mode & 4:  # ReLU6
        x = x.clamp(max=6.0)
    return x


def _pro(mode, c, seed):
    if not (mode & 2):
        return (mode, None, None), None, None
    s = torch.rand(c, generator=torch.Generator().manual_seed(seed)) + 0.5
    t = rnd((c,), seed + 1, 0.3)
    return (mode, s.to(DEV), t.to(DEV)), s, t


# ------------------------------------------------------------------------------ conv GEMM fwd
CONV_CASES = [
    # N, H, W, C, O, k, stride, pad, dil, mode, bias, slice
    (2, 9, 13, 72, 40, 1, 1, 0, 1, 3, False, False),
    (2, 17, 17, 728, 728, 1, 1, 0, 1, 2, False, False),   # the dominant xception shape
    (1, 12, 20, 256, 19, 1, 1, 0, 1, 3, True, True),      # classifier: ragged O, bias, pitch
    (2, 11, 15, 64, 128, 1, 2, 0, 1, 1, False, False),    # strided shortcut
    (2, 13, 11, 32, 64, 3, 1, 1, 1, 3, False, False),     # xception conv2
    (2, 13, 11, 8, 32, 3, 2, 1, 1, 0, False, False),      # stem on channel-padded input
    (1, 10, 14, 16, 24, 3, 1, 2, 2, 2, False, True),      # dilated dense
    (2, 1, 1, 2048, 256, 1, 1, 0, 1, 0, False, False),    # ASPP image-pooling (M = batch)
    # ... a handful of pixels in float32 on the lanes-split-K kernel (r05): PSP pyramid bins
    # (ragged pixel chunk, ragged channel group + slice output), K not a multiple of 256
    (2, 6, 6, 2048, 512, 1, 1, 0, 1, 0, False, False),
    (2, 3, 3, 512, 2047, 1, 1, 0, 1, 0, False, True),
    (1, 1, 3, 264, 6, 1, 1, 0, 1, 0, False, False),
    (2, 7, 9, 4096, 512, 3, 1, 1, 1, 0, False, False),    # PSP head: K = 36864
    (2, 37, 45, 8, 64, 7, 2, 3, 1, 0, False, False),      # ResNet stem 7x7 s2 p3 (resnet.py:116)
    (1, 29, 31, 8, 64, 7, 2, 3, 1, 2, False, True),       # the same on bf16 padding, prologue
    # 256x128-tile kernel (O >= 384, M >= 4096): ragged M / O / K tails, prologue, slice output
    (2, 45, 47, 728, 728, 1, 1, 0, 1, 0, False, False),
    (1, 65, 67, 200, 392, 1, 1, 0, 1, 3, False, True),
    (2, 33, 63, 264, 1000, 1, 1, 0, 1, 2, True, False),
    # HRNet's 240 -> 240 last layer geometry (>= 65536 pixels, O just below the wide kernels)
    (1, 257, 259, 64, 240, 1, 1, 0, 1, 0, False, False),
    # 256x64-tile general path (KxK, O <= 64, M >= 16384): ragged M, prologue + statistics,
    # the conv2 data-gradient shape (64 -> 32), a strided stem, a slice output with ragged O
    (1, 131, 129, 32, 64, 3, 1, 1, 1, 3, False, False),
    (1, 130, 127, 64, 32, 3, 1, 1, 1, 0, False, False),
    (1, 261, 259, 8, 32, 3, 2, 1, 1, 0, False, False),
    (1, 129, 131, 16, 24, 3, 1, 2, 2, 2, False, True),
    # direct halo-tile 3x3 kernel (bf16, stride 1, C/O in {16, 32, 64}, >= 65536 pixels): ragged
    # tile rows / columns, BatchNorm+ReLU prologue with zero padding, statistics, two images,
    # channel-slice input and output
    (1, 260, 257, 32, 64, 3, 1, 1, 1, 3, False, False),
    (1, 259, 261, 64, 32, 3, 1, 1, 1, 0, False, False),
    (2, 131, 259, 32, 32, 3, 1, 1, 1, 2, False, True),
    (2, 129, 257, 64, 32, 3, 1, 1, 1, 3, False, False),
    # ... C = O = 16 (r05: HRNet's full-resolution basic blocks; half of the kernel's 32-channel
    # group is zero weights): prologue + statistics on ragged tiles, plain on a slice in / out
    (2, 131, 259, 16, 16, 3, 1, 1, 1, 3, False, False),
    (1, 259, 261, 16, 16, 3, 1, 1, 1, 0, False, True),
    # stride-1 KxK on the direct-to-LDS pipeline (bf16, no prologue, C % 32 == 0, O >= 256,
    # >= 4096 pixels): ResNet layer3 / layer4 dilated 3x3, ragged O tile + slice in/out, a
    # padding that shrinks the map (the data-gradient geometry of a padded conv)
    (2, 65, 67, 256, 256, 3, 1, 2, 2, 0, False, False),
    (1, 40, 110, 512, 512, 3, 1, 4, 4, 0, False, False),
    (1, 70, 72, 320, 264, 3, 1, 1, 1, 0, False, True),
    (1, 70, 72, 256, 256, 3, 1, 0, 1, 0, False, False),
    # r06, the four-wave direct-to-LDS kernel (224-row tiles: 1x1 launches of at most two rounds
    # in which 192 rows would need one more round than 224): ragged last row tile, ragged column
    # tile, K not a multiple of 32, slice in / out
    (1, 130, 200, 200, 392, 1, 1, 0, 1, 0, False, True),
    (2, 100, 128, 264, 504, 1, 1, 0, 1, 0, False, False),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_gemm_fwd(case, dtype):
    N, H, W, C, O, k, stride, pad, dil, mode, bias, sl = case
    x = quant(rnd((N, C, H, W), 1), dtype)
    w = quant(rnd((O, C, k, k), 2, (2.0 / (C * k * k)) ** 0.5), dtype)
    b = rnd((O,), 3, 0.5) if bias else None
    pro, s, t = _pro(mode, C, 4)
    xa = _act_ref(x, mode, s, t)
    if dtype == torch.bfloat16:
        xa = quant(xa, dtype)  # the kernel stages the activated operand in bf16
    ref = TF.conv2d(xa.double(), w.double(), None if b is None else b.double(), stride, pad, dil)
    xd = to_dev_nhwc(x, dtype, pitch=C + 16 if sl else None, off=8 if sl else 0)
    wp = F().pack_conv_weight(w.to(DEV), C, dtype)
    Ho, Wo = ref.shape[2:]
    out = None
    if sl:
        vec = 8 if dtype == torch.bfloat16 else 4
        pitch = (O + 2 * vec - 1) // vec * vec + vec
        out = torch.full((N, Ho, Wo, pitch), float("nan"), dtype=dtype, device=DEV)[..., vec:vec + O]
    y, partial = K().conv_gemm(xd, wp, O, k, k, stride, pad, dil, pro,
                               None if b is None else b.to(DEV), out, want_stats=not bias)
    got = to_cpu_nchw(y)
    assert_close(got, ref, dtype, "conv y")
    if partial is not None:
        nb = ref - (0 if b is None else b.view(1, -1, 1, 1).double())
        M = N * ref.shape[2] * ref.shape[3]
        direct = k == 3 and stride == 1 and pad == 1 and dil == 1 and M >= 65536 and \
            (C, O) in ((32, 32), (32, 64), (64, 32), (16, 16))
        glds_kxk = k > 1 and stride == 1 and C % 32 == 0 and O >= 256 and M >= 4096 \
            and mode == 0 and not bias
        wide = k == 1 and stride == 1 and pad == 0 and ((O >= 384 and M >= 4096)
                                                        or (O >= 256 and M >= 65536))
        if dtype == torch.bfloat16 and (direct or glds_kxk or wide):
            # the 256x128, direct-to-LDS and direct-3x3 kernels take the statistics of the values AS STORED
            # (bf16-rounded):
            # that is the tensor the consumer's normalisation is applied to
            nb = quant(nb.float(), dtype).double()
        sums = K().colsum(partial.view(partial.shape[0], -1)).cpu()
        assert_close(sums[:O], nb.sum((0, 2, 3)), torch.float32, "conv sum",
                     scale=nb.abs().sum((0, 2, 3)).max().item(), fac=5)
        assert_close(sums[O:], (nb * nb).sum((0, 2, 3)), torch.float32, "conv sumsq", fac=5)
    if sl:  # nothing outside the slice was touched
        full = y.as_strided((N, Ho, Wo, pitch), y.stride(), y.storage_offset() - vec)
        assert torch.isnan(full[..., :vec].float()).all() and torch.isnan(full[..., vec + O:].float()).all()


@pytest.mark.parametrize("want_stats", [False, True], ids=["correction", "correction+stats"])
@pytest.mark.parametrize("geom", [(1, 130, 200, 200, 392), (2, 45, 47, 328, 728)])
def test_conv_gemm_epilogue_correction_on_the_direct_to_lds_kernels(geom, want_stats):
    """y = acc - c0[o] - c1[o] * x[p][o] (the data gradient through a folded BatchNorm) on the
    bf16 1x1 launches the direct-to-LDS kernels serve.  First geometry: the one whose forward
    takes 224-row tiles on the four-wave kernel (r06) — correction only stays on eight waves
    with its own tile height, correction + statistics must follow the statistics rows the
    caller sized (four waves); second: 192-row tiles on eight waves.  Statistics are those of
    the values as stored."""
    N, H, W, C, O = geom
    dtype = torch.bfloat16
    x = quant(rnd((N, C, H, W), 1), dtype)
    w = quant(rnd((O, C, 1, 1), 2, (2.0 / C) ** 0.5), dtype)
    xe = quant(rnd((N, O, H, W), 3), dtype)
    c0, c1 = rnd((O,), 4, 0.05), rnd((O,), 5, 0.3)
    ref = TF.conv2d(x.double(), w.double()) - c0.view(1, -1, 1, 1).double() \
        - c1.view(1, -1, 1, 1).double() * xe.double()
    xd, xed = to_dev_nhwc(x, dtype), to_dev_nhwc(xe, dtype)
    wp = F().pack_conv_weight(w.to(DEV), C, dtype)
    y, partial = K().conv_gemm(xd, wp, O, 1, 1, 1, 0, 1, None, None, None, want_stats=want_stats,
                               ep=(xed, c0.to(DEV), c1.to(DEV)))
    got = to_cpu_nchw(y)
    assert_close(got, ref, dtype, "corrected y")
    assert (partial is not None) == want_stats
    if want_stats:
        st = got.double()  # the values as stored
        sums = K().colsum(partial.view(partial.shape[0], -1)).cpu()
        assert_close(sums[:O], st.sum((0, 2, 3)), torch.float32, "sum",
                     scale=st.abs().sum((0, 2, 3)).max().item(), fac=5)
        assert_close(sums[O:], (st * st).sum((0, 2, 3)), torch.float32, "sumsq", fac=5)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conv_gemm_scatter_is_strided_dgrad(dtype):
    """data gradient of a stride-2 1x1 conv = GEMM with transposed weights + strided scatter"""
    N, H, W, C, O = 2, 11, 15, 64, 128
    x = rnd((N, C, H, W), 1).requires_grad_()
    w = quant(rnd((O, C, 1, 1), 2, 0.1), dtype)
    y = TF.conv2d(x, w, None, 2)
    dy = quant(rnd(tuple(y.shape), 3), dtype)
    y.backward(dy)
    wt = F().pack_conv_weight_dgrad(w.to(DEV), O, dtype)
    g, _ = K().conv_gemm(to_dev_nhwc(dy, dtype), wt, C, 1, 1, 1, 0, 1, scatter=(H, W, 2))
    assert_close(to_cpu_nchw(g), x.grad, dtype, "strided dgrad")


# ------------------------------------------------------------------------------ conv wgrad
WGRAD_CASES = [
    (2, 17, 17, 728, 728, 1, 1, 0, 1, 3),
    (2, 40, 40, 64, 128, 1, 1, 0, 1, 2),     # several pixel splits
    (2, 11, 15, 64, 128, 1, 2, 0, 1, 1),
    (2, 13, 11, 32, 64, 3, 1, 1, 1, 3),
    (2, 13, 11, 8, 32, 3, 2, 1, 1, 0),
    (1, 12, 20, 256, 19, 1, 1, 0, 1, 3),     # ragged dy channels
    (2, 7, 9, 4096, 512, 3, 1, 1, 1, 0),     # PSP head: K = 36864, one pixel split
    (1, 131, 129, 32, 64, 3, 1, 1, 1, 3),    # xception conv2 geometry across image-row wraps
    (2, 67, 70, 8, 32, 3, 2, 1, 1, 2),       # strided stem, two images, prologue
    # direct halo-tile weight gradient (bf16, 3x3 stride 1, C = 32, >= 65536 pixels)
    (1, 260, 257, 32, 64, 3, 1, 1, 1, 3),
    (2, 131, 259, 32, 32, 3, 1, 1, 1, 0),
    (2, 129, 263, 32, 64, 3, 1, 1, 1, 1),
    # stride-1 KxK on the direct-to-LDS transpose-read kernel (bf16, no prologue, C % 128 == 0,
    # output rows >= 64 pixels): dilated ResNet 3x3s, image-row wraps inside a slot, several
    # splits; the last one (output rows of 62 pixels) stays on the first-generation kernel
    (2, 40, 70, 256, 256, 3, 1, 2, 2, 0),
    (1, 33, 129, 128, 384, 3, 1, 1, 1, 0),
    (1, 70, 66, 256, 136, 3, 1, 4, 4, 0),
    (2, 36, 64, 256, 128, 3, 1, 0, 1, 0),
    # narrow output on a large map (decoder c1_block 256 -> 48: M >= 32768 -> direct-to-LDS kernel
    # with a mostly empty 128-wide tile, 128 pixel splits) and a ragged O
    (1, 190, 180, 256, 48, 1, 1, 0, 1, 0),
    (1, 182, 181, 64, 24, 1, 1, 0, 1, 0),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", WGRAD_CASES)
def test_conv_gemm_wgrad(case, dtype):
    N, H, W, C, O, k, stride, pad, dil, mode = case
    x = quant(rnd((N, C, H, W), 1), dtype)
    pro, s, t = _pro(mode, C, 4)
    xa = _act_ref(x, mode, s, t)
    if dtype == torch.bfloat16:
        xa = quant(xa, dtype)
    w = torch.zeros((O, C, k, k), dtype=torch.float64, requires_grad=True)
    y = TF.conv2d(xa.double(), w, None, stride, pad, dil)
    dy = quant(rnd(tuple(y.shape), 3), dtype)
    y.backward(dy.double())
    vec = 8 if dtype == torch.bfloat16 else 4
    pitch = (O + vec - 1) // vec * vec
    dyd = to_dev_nhwc(dy, dtype, pitch=pitch if pitch != O else None)
    dW = K().conv_wgrad(to_dev_nhwc(x, dtype), dyd, O, k, k, stride, pad, dil, pro)
    got = dW.view(O, k, k, C).permute(0, 3, 1, 2).cpu()
    # bf16: an fp32 fma-vs-mul+add difference in the prologue can flip a bf16 rounding of a
    # single staged element (2^-8 of that element) -> allow 4e-4 of the dW scale
    assert_close(got, w.grad, torch.float32, "dW", fac=20)


# ------------------------------------------------------------------------------ PSP head
def test_psp_head_geometry_on_the_direct_to_lds_kxk_kernels():
    """pspnet.py:49 `_PSPHead.block[0]`: 3x3, 4096 -> 512 at the OS8 map of a 513 x 553 crop
    (65 x 70 = 4550 pixels >= 4096): forward and data gradient on `conv_gemm_glds<KXK>` (K = 36864,
    288 slots per tap sweep; dgrad = 512 -> 4096 with O = 4096), weight gradient on
    `conv_wgrad_glds<KXK>` (C % 128 == 0, output rows of 70 >= 64 pixels) — the kernels
    profiles/r02_infer.json's C4 numbers were measured on.  bf16 (the kernels' only dtype); the
    CPU reference runs in fp32 (oneDNN; an fp64 conv of 171 GFLOP would take minutes)."""
    dtype = torch.bfloat16
    N, H, W, C, O = 1, 65, 70, 4096, 512
    x = quant(rnd((N, C, H, W), 1), dtype)
    w = quant(rnd((O, C, 3, 3), 2, (2.0 / (C * 9)) ** 0.5), dtype)
    ref = TF.conv2d(x, w, None, 1, 1, 1)
    xd = to_dev_nhwc(x, dtype)
    wp = F().pack_conv_weight(w.to(DEV), C, dtype)
    y, partial = K().conv_gemm(xd, wp, O, 3, 3, 1, 1, 1, None, None, None, want_stats=True)
    e1 = assert_close(to_cpu_nchw(y), ref, dtype, "psp head fwd")
    nb = quant(ref, dtype).double()
    sums = K().colsum(partial.view(partial.shape[0], -1)).cpu()
    assert_close(sums[:O], nb.sum((0, 2, 3)), torch.float32, "psp head sum",
                 scale=nb.abs().sum((0, 2, 3)).max().item(), fac=5)
    assert_close(sums[O:], (nb * nb).sum((0, 2, 3)), torch.float32, "psp head sumsq", fac=5)
    # data gradient: dy [N, 512, H, W] -> dx [N, 4096, H, W] through the flipped / transposed pack
    dy = quant(rnd((N, O, H, W), 3), dtype)
    gref = TF.conv_transpose2d(dy, w, None, 1, 1)
    wt = F().pack_conv_weight_dgrad(w.to(DEV), O, dtype)
    dyd = to_dev_nhwc(dy, dtype)
    g, _ = K().conv_gemm(dyd, wt, C, 3, 3, 1, 1, 1)
    e2 = assert_close(to_cpu_nchw(g), gref, dtype, "psp head dgrad")
    # weight gradient
    wr = w.clone().requires_grad_()
    TF.conv2d(x, wr, None, 1, 1, 1).backward(dy)
    dW = K().conv_wgrad(xd, dyd, O, 3, 3, 1, 1, 1, None)
    got = dW.view(O, 3, 3, C).permute(0, 3, 1, 2).cpu()
    e3 = assert_close(got, wr.grad, torch.float32, "psp head dW", fac=20)
    print("PARITY psp-head 3x3 4096->512 @65x70 bf16: fwd %.2e dgrad %.2e wgrad %.2e "
          "(max-normalised)" % (e1, e2, e3))


# ------------------------------------------------------------------------------ depthwise
DW_CASES = [
    # N, H, W, C, stride, dil, mode
    (2, 17, 17, 728, 1, 1, 3),
    (2, 17, 19, 728, 1, 1, 1),
    (2, 21, 25, 128, 2, 1, 3),
    (1, 23, 29, 1024, 1, 2, 2),
    (2, 33, 37, 64, 1, 6, 3),
    (1, 16, 40, 304, 1, 1, 0),
    (1, 20, 24, 2048, 1, 12, 0),
    (1, 40, 44, 256, 1, 18, 2),     # ASPP rate 18 (OS16, module.py:39-41)
    (2, 50, 52, 128, 1, 24, 3),     # ASPP rates 24 / 36 (OS8)
    (1, 75, 80, 64, 1, 36, 0),
    # stride 2 (fused one-pass backward, csrc/dwconv_s2.hip): odd / even sizes, ragged tiles,
    # ReLU6 prologue (MobileNetV2), several tiles per persistent block
    (1, 40, 37, 64, 2, 1, 1),
    (2, 16, 32, 256, 2, 1, 2),
    (1, 33, 47, 96, 2, 1, 7),
    (2, 129, 131, 32, 2, 1, 3),
    (1, 19, 22, 40, 2, 1, 0),       # no prologue, ragged channel vectors
    # r06, register-sliding kernels (csrc/dwconv_slide.hip, stride 1 / dilation 1): a map of >= 30 MB
    # (neighbour columns by lane exchange + half-active buffer loads; odd width, 58 channel quads =
    # 3.6 channel blocks, four strips), a map narrower than one column block, a map lower than one
    # strip with the ReLU6 prologue
    (2, 130, 259, 232, 1, 1, 3),
    (1, 45, 5, 24, 1, 1, 1),
    (1, 7, 130, 136, 1, 1, 7),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", DW_CASES)
def test_dwconv_fwd_dgrad_wgrad(case, dtype):
    N, H, W, C, stride, dil, mode = case
    x = quant(rnd((N, C, H, W), 1), dtype)
    w = rnd((C, 1, 3, 3), 2, 0.4)
    pro, s, t = _pro(mode, C, 4)
    xa = _act_ref(x, mode, s, t).double().requires_grad_()
    wd = w.double().requires_grad_()
    ref = TF.conv2d(xa, wd, None, stride, dil, dil, groups=C)
    w9c = w.view(C, 9).t().contiguous().to(DEV)
    y, partial = K().dwconv(to_dev_nhwc(x, dtype), w9c, stride, dil, pro, want_stats=True)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "dw y")
    sums = K().colsum(partial.view(partial.shape[0], -1)).cpu()
    r = ref.detach()
    # bf16, tiled kernels (stride 1 dil <= 2, stride 2 dil 1): the activated operand is rounded to bf16 once (it
    # is parked in LDS in the storage dtype), so the sums carry that rounding (2^-9 per term)
    sfac = 5 if dtype == torch.float32 else 60
    assert_close(sums[:C], r.sum((0, 2, 3)), torch.float32, "dw sum",
                 scale=r.abs().sum((0, 2, 3)).max().item(), fac=sfac)
    assert_close(sums[C:], (r * r).sum((0, 2, 3)), torch.float32, "dw sumsq", fac=sfac)
    dy = quant(rnd(tuple(ref.shape), 3), dtype)
    ref.backward(dy.double())
    dyd = to_dev_nhwc(dy, dtype)
    g = K().dwconv_dgrad(dyd, w9c.flip(0).contiguous() if stride == 1 else w9c, stride, dil, (H, W))
    assert_close(to_cpu_nchw(g), xa.grad, dtype, "dw dgrad")
    dW = K().dwconv_wgrad(to_dev_nhwc(x, dtype), dyd, stride, dil, pro)
    # (bf16 tiled kernels see the activation rounded to bf16, the fp64 reference does not)
    assert_close(dW.t().reshape(C, 1, 3, 3).cpu(), wd.grad, torch.float32, "dw wgrad",
                 fac=20 if dtype == torch.float32 else 100)
    if K().dw_tiled(stride, dil):
        # the LDS-tiled kernels also take torch's [C,1,3,3] parameter as is (taps reversed in
        # the kernel for the data gradient) and emit dW in that layout: bit-identical results
        w4 = w.to(DEV)
        y4, _ = K().dwconv(to_dev_nhwc(x, dtype), w4, stride, dil, pro)
        assert torch.equal(y4, y)
        assert torch.equal(K().dwconv_dgrad(dyd, w4, stride, dil, (H, W)), g)
        dW4 = K().dwconv_wgrad(to_dev_nhwc(x, dtype), dyd, stride, dil, pro, torch_layout=True)
        assert_close(dW4.cpu(), dW.t().reshape(C, 1, 3, 3).cpu().double(), torch.float32, "dw wgrad layout", fac=2)
    if stride == 2 and dil == 1:  # fused one-pass backward of the strided layers
        gf, dW4, pb = K().dwconv_bwd_fused_s2(to_dev_nhwc(x, dtype), dyd, w.to(DEV), pro, want_bn=True)
        act = xa.detach()
        mask = ((act > 0) & ((act < 6) if (mode & 4) else torch.ones_like(act, dtype=torch.bool))).double() \
            if (mode & 1) else torch.ones_like(act)
        gref = xa.grad * mask
        assert_close(to_cpu_nchw(gf), gref, dtype, "fused s2 dw dgrad")
        assert_close(dW4.cpu(), wd.grad, torch.float32, "fused s2 dw wgrad",
                     fac=20 if dtype == torch.float32 else 100)
        sums = K().colsum(pb).cpu()
        assert_close(sums[:C], gref.sum((0, 2, 3)), torch.float32, "fused s2 sum g",
                     scale=gref.abs().sum((0, 2, 3)).max().item(), fac=300 if dtype == torch.bfloat16 else 5)
        assert_close(sums[C:], (gref * x.double()).sum((0, 2, 3)), torch.float32, "fused s2 sum gx",
                     scale=(gref * x.double()).abs().sum((0, 2, 3)).max().item(),
                     fac=300 if dtype == torch.bfloat16 else 5)
    if stride == 1:  # fused one-pass backward: masked dgrad + wgrad + BN-backward sums
        gf, dWf, pb = K().dwconv_bwd_fused(to_dev_nhwc(x, dtype), dyd, w9c, dil, pro, want_bn=True)
        if K().dw_tiled(stride, dil):  # same kernel fed with the [C,1,3,3] parameter
            g4, dW4, pb4 = K().dwconv_bwd_fused(to_dev_nhwc(x, dtype), dyd, w.to(DEV), dil, pro,
                                                want_bn=True, torch_layout=True)
            assert torch.equal(g4, gf) and torch.equal(pb4, pb)
            assert_close(dW4.cpu(), dWf.t().reshape(C, 1, 3, 3).cpu().double(), torch.float32,
                         "fused dw wgrad layout", fac=2)
        mask = (xa.detach() > 0).double() if (mode & 1) else torch.ones_like(xa.detach())
        gref = xa.grad * mask
        assert_close(to_cpu_nchw(gf), gref, dtype, "fused dw dgrad")
        assert_close(dWf.t().reshape(C, 1, 3, 3).cpu(), wd.grad, torch.float32, "fused dw wgrad", fac=20)
        sums = K().colsum(pb).cpu()
        assert_close(sums[:C], gref.sum((0, 2, 3)), torch.float32, "fused sum g",
                     scale=gref.abs().sum((0, 2, 3)).max().item(), fac=300 if dtype == torch.bfloat16 else 5)
        assert_close(sums[C:], (gref * x.double()).sum((0, 2, 3)), torch.float32, "fused sum gx",
                     scale=(gref * x.double()).abs().sum((0, 2, 3)).max().item(),
                     fac=300 if dtype == torch.bfloat16 else 5)


# ------------------------------------------------------------------------------ batch norm
@pytest.mark.parametrize("rows", [3, 130, 5000])
def test_colsum(rows):
    p = rnd((rows, 77), 1)
    out = K().colsum(p.to(DEV)).cpu()
    assert_close(out, p.double().sum(0), torch.float32, "colsum f64", scale=p.abs().sum(0).max().item())
    out32 = K().colsum(p.to(DEV), f64=False).cpu()
    assert out32.dtype == torch.float32
    assert_close(out32, p.double().sum(0), torch.float32, "colsum f32", scale=p.abs().sum(0).max().item())


def test_bn_finalize_matches_torch_batch_norm():
    N, C, H, W = 2, 96, 9, 11
    x = rnd((N, C, H, W), 1) * 2 + 0.7
    gamma, beta = torch.rand(C) + 0.5, rnd((C,), 3, 0.2)
    rm, rv = rnd((C,), 4, 0.1), torch.rand(C) + 0.5
    rm_ref, rv_ref = rm.clone(), rv.clone()
    y_ref = TF.batch_norm(x, rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-3)
    sums = torch.cat([x.double().sum((0, 2, 3)), (x.double() ** 2).sum((0, 2, 3))]).to(DEV)
    rmd, rvd = rm.to(DEV), rv.to(DEV)
    mean, invstd, scale, shift = K().bn_finalize(sums, N * H * W, gamma.to(DEV), beta.to(DEV), 1e-3,
                                                 0.1, rmd, rvd)
    y = x * scale.cpu().view(1, -1, 1, 1) + shift.cpu().view(1, -1, 1, 1)
    assert_close(y, y_ref, torch.float32, "bn y")
    assert_close(rmd.cpu(), rm_ref, torch.float32, "running_mean")
    assert_close(rvd.cpu(), rv_ref, torch.float32, "running_var")
    es, et = K().bn_eval_affine(gamma.to(DEV), beta.to(DEV), rmd, rvd, 1e-3)
    ye = TF.batch_norm(x, rm_ref, rv_ref, gamma, beta, False, 0.1, 1e-3)
    assert_close(x * es.cpu().view(1, -1, 1, 1) + et.cpu().view(1, -1, 1, 1), ye, torch.float32, "bn eval")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 1, 1), (2, 3, 3), (2, 6, 6), (2, 17, 29)])
def test_bn_finalize_small_two_pass_statistics_with_a_large_mean(shape, dtype):
    """seg_bn_finalize_small (r04): BatchNorm over few samples whose spread is tiny against
    their mean — the 2-sample BatchNorm of the ASPP image-pooling branch (module.py:52-64), PSP's
    pyramid bins (module.py:89-97) — vs torch.batch_norm in float64 on the values as stored.  The
    single-pass E[x^2] - mean^2 form on fp32 partial sums is off by up to 100 % here."""
    N, H, W = shape
    C = 72
    base = rnd((1, C, 1, 1), 5) * 3 + 20.0                       # |mean| ~ 20
    x = quant(base + rnd((N, C, H, W), 6) * 0.02, dtype)         # spread 0.02 (bf16: its ulp grid)
    gamma, beta = torch.rand(C) + 0.5, rnd((C,), 3, 0.2)
    rm, rv = rnd((C,), 4, 0.1), torch.rand(C) + 0.5
    rm_ref, rv_ref = rm.double(), rv.double()
    y_ref = TF.batch_norm(x.double(), rm_ref, rv_ref, gamma.double(), beta.double(), True, 0.1, 1e-5)
    buf = to_dev_nhwc(x, dtype, pitch=C + 8)                     # a channel slice: pitch != C
    rmd, rvd, off = rm.to(DEV), rv.to(DEV), rnd((C,), 8, 0.3)
    mean, invstd, scale, shift = K().bn_finalize_small(buf, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1,
                                                       rmd, rvd, off.to(DEV))
    xd = x.double()
    y = xd * scale.cpu().double().view(1, -1, 1, 1) + shift.cpu().double().view(1, -1, 1, 1)
    # y = x*scale + shift cancels 20/0.02 = 3 digits of the fp32 scale / shift: 1e-3 of the output
    err = ((y - y_ref).abs().max() / y_ref.abs().max()).item()
    assert err < 2e-3, err
    var_ref = xd.var((0, 2, 3), unbiased=False)
    got_var = invstd.cpu().double().pow(-2) - 1e-5
    assert ((got_var - var_ref).abs() <= 1e-4 * var_ref + 1e-9).all()
    assert_close(mean.cpu(), xd.mean((0, 2, 3)), torch.float32, "mean")
    assert_close(rmd.cpu(), rm_ref + 0.1 * off.double(), torch.float32, "running_mean (+ offset)")
    assert_close(rvd.cpu(), rv_ref, torch.float32, "running_var", fac=5)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(2, 1, 1), (2, 6, 6), (4, 9, 13)])
def test_bn_backward_small_float64_in_one_launch(shape, relu):
    """seg_bn_bwd_small (r05): BatchNorm backward over few samples — with two samples per channel
    dx is what is left when three terms cancel (xhat = +-1 up to eps); fp32 `scale*g - c0 - c1*x`
    keeps 6e-8 of the TERMS (ASPP image pooling: 94 % of the C3 model's fp32 gradient error).
    Against torch autograd in float64 on the same fp32 values; channel mask + ReLU mask; a
    channel-slice pitch; in place."""
    N, H, W = shape
    C = 72
    dtype = torch.float32
    base = rnd((1, C, 1, 1), 5) * 3 + 20.0
    x = quant(base + rnd((N, C, H, W), 6) * 0.02, dtype)
    g = quant(rnd((N, C, H, W), 7), dtype)
    gen = torch.Generator().manual_seed(11)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, rnd((C,), 3, 0.2)
    mul = (torch.rand(N, C, generator=gen) > 0.3).float() / 0.7
    xd = x.double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = TF.batch_norm(xd, None, None, gd, bd, True, 0.1, 1e-5)
    if relu:
        y = torch.relu(y)
    (y * mul.double().view(N, C, 1, 1)).backward(g.double())
    xbuf = to_dev_nhwc(x, dtype, pitch=C + 8)
    mean, invstd, scale, shift = K().bn_finalize_small(xbuf, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1,
                                                       None, None)
    gbuf = to_dev_nhwc(g, dtype)
    pro = (3 if relu else 2, scale, shift)
    dx, dgamma, dbeta = K().bn_bwd_small(gbuf, xbuf, pro, float(N * H * W), mean, invstd,
                                         gamma.to(DEV), chan_mul=mul.to(DEV), out=gbuf)
    assert dx.data_ptr() == gbuf.data_ptr()
    ref = xd.grad
    err = ((to_cpu_nchw(dx).double() - ref).abs().max() / ref.abs().max()).item()
    # (the forward's fp32 mean / invstd / scale / shift bound this: 1e-7 * |x| / spread = 1e-4)
    assert err < 5e-3, err
    assert_close(dgamma.cpu(), gd.grad, torch.float32, "dgamma", fac=50)
    assert_close(dbeta.cpu(), bd.grad, torch.float32, "dbeta")
    # the three-launch fp32 path on the same operands loses the result where the terms cancel
    part = K().bn_bwd_reduce_partial(to_dev_nhwc(g, dtype), xbuf, pro, mul.to(DEV))
    _, _, c0, c1 = K().bn_bwd_finalize_p(part, float(N * H * W), mean, invstd, gamma.to(DEV))
    dx32 = K().bn_bwd_apply(to_dev_nhwc(g, dtype), xbuf, pro, c0, c1, mul.to(DEV))
    err32 = ((to_cpu_nchw(dx32).double() - ref).abs().max() / ref.abs().max()).item()
    print("bn backward, %d samples per channel, |mean| / spread = 1e3: float64 launch %.2e, "
          "fp32 reduce + finalize + apply %.2e of max |dx|" % (N * H * W, err, err32))


def test_eval_affine_of_many_batchnorms_in_one_launch_and_cache_invalidation():
    """functional.eval_affine (r05): the evaluation-mode (scale, shift) of every planned BatchNorm
    by ONE seg_bn_eval_affine_multi launch, bit-identical to the per-module kernel, cached on the
    tensors' versions — and dropped when a TRAINING forward rewrites the running statistics through
    the finalize kernels' raw pointers (which torch's version counters do not see)."""
    import torch.nn as nn
    Fm = F()
    gen = torch.Generator().manual_seed(3)
    bns = []
    for C in (24, 728, 2048, 72, 256) * 11:  # 55 modules: two launches of <= 48 jobs
        bn = nn.BatchNorm2d(C, eps=1e-3).to(DEV).eval()
        with torch.no_grad():
            bn.weight.copy_(torch.rand(C, generator=gen) + 0.5)
            bn.bias.copy_(torch.randn(C, generator=gen) * 0.2)
            bn.running_mean.copy_(torch.randn(C, generator=gen) * 0.3)
            bn.running_var.copy_(torch.rand(C, generator=gen) + 0.5)
        bns.append(bn)
    Fm.clear_weight_cache()
    for bn in bns:       # plan them (each request computes what is planned so far)
        Fm.eval_affine(bn)
    Fm.clear_weight_cache()
    misses = Fm._MISSES[0]
    Fm.eval_affine(bns[0])
    after_first = Fm._MISSES[0]
    got = [Fm.eval_affine(bn) for bn in bns]
    # ONE request packed all of them (>=: evaluation-mode BatchNorms of earlier tests that are
    # still alive in this process are planned too and ride along)
    assert Fm._MISSES[0] == after_first and after_first - misses >= len(bns)
    for bn, (sc, sh) in zip(bns, got):
        es, et = K().bn_eval_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        assert torch.equal(sc, es) and torch.equal(sh, et)
    again = Fm.eval_affine(bns[7])
    assert again[0].data_ptr() == got[7][0].data_ptr()           # cached
    # a training-mode BatchNorm evaluation anywhere invalidates the cached affines
    tbn = nn.BatchNorm2d(72).to(DEV).train()
    x = to_dev_nhwc(quant(rnd((2, 72, 5, 7), 1), torch.float32), torch.float32)
    part = K().bn_bwd_reduce_partial(x, x, (0, None, None))  # (sum x, sum x^2) rows
    Fm.finish_bn(tbn, part.view(part.shape[0], 2, 72), 2 * 5 * 7, y=x)
    with torch.no_grad():
        bns[7].running_mean.data.add_(1.0)  # (.data: no version bump, like the kernels' writes)
    fresh = Fm.eval_affine(bns[7])
    es, et = K().bn_eval_affine(bns[7].weight, bns[7].bias, bns[7].running_mean,
                                bns[7].running_var, bns[7].eps)
    assert torch.equal(fresh[1], et) and not torch.equal(fresh[1], got[7][1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_apply_residual_and_channel_mask(dtype):
    N, C, H, W = 2, 72, 7, 9
    x, r = quant(rnd((N, C, H, W), 1), dtype), quant(rnd((N, C, H, W), 2), dtype)
    px, sx, tx = _pro(3, C, 5)
    pr, sr, tr = _pro(2, C, 7)
    mul = (torch.rand(N, C) > 0.3).float() / 0.7
    ref = _act_ref(x, 3, sx, tx) * mul.view(N, C, 1, 1) + _act_ref(r, 2, sr, tr)
    out = torch.full((N, H, W, C + 16), float("nan"), dtype=dtype, device=DEV)[..., 8:8 + C]
    y = K().bn_apply(to_dev_nhwc(x, dtype), px, to_dev_nhwc(r, dtype, pitch=C + 8), pr,
                     mul.to(DEV), False, out)
    assert_close(to_cpu_nchw(y), ref, dtype, "bn_apply")
    y2 = K().bn_apply(to_dev_nhwc(x, dtype), px, to_dev_nhwc(r, dtype), pr, None, True)
    assert_close(to_cpu_nchw(y2), torch.relu(_act_ref(x, 3, sx, tx) + _act_ref(r, 2, sr, tr)), dtype,
                 "bn_apply post_relu")


BN_BWD_SHAPE = (2, 104, 9, 11)
# 728 channels (whole-row blocks of the row-tile kernels: 182 x 2 lanes in fp32, 91 x 4 in bf16, 20
# idle lanes): at 198 rows functional.bn_input_backward still takes the one-launch float64 route
# (seg_bn_bwd_small: at most 1024 rows); 2 x 23 x 23 = 1058 rows is the smallest map that goes
# reduce -> finalize -> apply.  The test asserts which route ran.
BN_BWD_SMALL_728, BN_BWD_ROW = (2, 728, 9, 11), (2, 728, 23, 23)
# Seed of x.  For the 728-channel shapes gamma comes from a fixed generator (not, as for the first
# shape, from the global one that conftest.py seeds from the test's name), so the data the guard
# below sees depends on (shape, dtype) alone and _bn_backward_reference can be called outside
# pytest.  With up to 770 000 values the smallest |BN(x)| of the reference is usually below 1e-5
# (seed 1: 3e-7 .. 5e-6, a ReLU mask that fp32 rounding can flip); these seeds keep it above
# (2.3e-5, 2.4e-5, 1.3e-5, 1.7e-5), which the reference half asserts.
BN_BWD_SEED = {(BN_BWD_SMALL_728, torch.float32): 1, (BN_BWD_SMALL_728, torch.bfloat16): 5,
               (BN_BWD_ROW, torch.float32): 368, (BN_BWD_ROW, torch.bfloat16): 4151}


def _bn_backward_reference(dtype, relu, shape=BN_BWD_SHAPE):
    """CPU half of test_bn_backward_matches_autograd (no device needed): the data, torch
    autograd's float64 gradients, and the guard that no ReLU mask hangs on rounding."""
    N, C, H, W = shape
    first = shape == BN_BWD_SHAPE  # (keeps the data and the checks it always had)
    x = quant(rnd((N, C, H, W), 1 if first else BN_BWD_SEED[shape, dtype]) * 1.5 + 0.3, dtype)
    gamma = torch.rand(C) if first else torch.rand(C, generator=torch.Generator().manual_seed(7))
    gamma, beta = (gamma + 0.5).requires_grad_(), rnd((C,), 3, 0.2).requires_grad_()
    xr = x.double().requires_grad_()
    y = TF.batch_norm(xr, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)
    if not first:
        margin = y.detach().abs().min().item()
        assert margin > 1e-5, "smallest |BN(x)| of the reference %.3e" % margin
    if relu:
        y = torch.relu(y)
    mul = (torch.rand(N, C) > 0.3).double() / 0.7
    g = quant(rnd((N, C, H, W), 5), dtype)
    (y * mul.view(N, C, 1, 1)).backward(g.double())
    return x, gamma, beta, xr, mul, g


# The ids keep the first shape's test names, and with them the seed conftest.py derives from a
# test's name for torch's global generator (its gamma and every channel mask are drawn from it).
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("relu,shape", [pytest.param(False, BN_BWD_SHAPE, id="False"),
                                        pytest.param(True, BN_BWD_SHAPE, id="True"),
                                        pytest.param(False, BN_BWD_SMALL_728, id="False-728"),
                                        pytest.param(True, BN_BWD_SMALL_728, id="True-728"),
                                        pytest.param(False, BN_BWD_ROW, id="False-728-rowtile"),
                                        pytest.param(True, BN_BWD_ROW, id="True-728-rowtile")])
def test_bn_backward_matches_autograd(dtype, relu, shape, monkeypatch):
    """relu(BN_train(x)) * mask consumed with gradient g: dx, dgamma, dbeta vs torch autograd"""
    N, C, H, W = shape
    x, gamma, beta, xr, mul, g = _bn_backward_reference(dtype, relu, shape)
    sums = torch.cat([x.double().sum((0, 2, 3)), (x.double() ** 2).sum((0, 2, 3))]).to(DEV)
    gd, bd = gamma.detach().to(DEV), beta.detach().to(DEV)
    mean, invstd, scale, shift = K().bn_finalize(sums, N * H * W, gd, bd, 1e-5, 0.1, None, None)
    Fm = F()
    route = []
    for name in ("bn_bwd_small", "bn_bwd_reduce_partial", "bn_bwd_finalize_p", "bn_bwd_apply"):
        def spy(*a, _f=getattr(Fm.K, name), _n=name, **kw):
            route.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(Fm.K, name, spy)
    bn = Fm.BNState(gd, bd, mean, invstd, scale, shift, float(N * H * W), True)
    dx, dgamma, dbeta = Fm.bn_input_backward(to_dev_nhwc(g, dtype), to_dev_nhwc(x, dtype), bn, relu,
                                             mul.float().to(DEV))
    assert route == (["bn_bwd_reduce_partial", "bn_bwd_finalize_p", "bn_bwd_apply"]
                     if N * H * W > K().SMALL_BN_ROWS else ["bn_bwd_small"]), route
    assert (shape == BN_BWD_ROW) == (len(route) == 3)
    assert_close(to_cpu_nchw(dx), xr.grad, dtype, "bn dx", fac=3)
    assert_close(dgamma.cpu(), gamma.grad, torch.float32, "dgamma", fac=20)
    assert_close(dbeta.cpu(), beta.grad, torch.float32, "dbeta", fac=20)


# ------------------------------------------------------------------------------ resize
RESIZE_CASES = [(5, 9, 17, 33, True), (17, 33, 65, 129, True), (9, 13, 20, 31, False),
                (1, 1, 5, 9, True), (12, 10, 7, 5, True),
                (2, 4, 16, 32, False), (4, 8, 16, 32, False), (8, 16, 16, 32, False),  # HRNet head
                (3, 5, 40, 77, False), (12, 10, 7, 5, False),
                # PSP pyramid bins -> feature map: >= 64 outputs per source pixel (block-cooperative
                # backward kernel)
                (2, 3, 40, 70, True), (6, 6, 65, 129, True), (3, 3, 49, 65, False),
                (2, 2, 33, 65, True)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", RESIZE_CASES)
def test_bilinear_fwd_bwd(case, dtype):
    Hi, Wi, Ho, Wo, ac = case
    N, C = 2, 40
    x = quant(rnd((N, C, Hi, Wi), 1), dtype)
    pro, s, t = _pro(3, C, 4)
    xa = _act_ref(x, 3, s, t).double().requires_grad_()
    ref = TF.interpolate(xa, size=(Ho, Wo), mode="bilinear", align_corners=ac)
    y = K().bilinear(to_dev_nhwc(x, dtype), (Ho, Wo), pro, None, ac)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "bilinear fwd")
    g = quant(rnd(tuple(ref.shape), 2), dtype)
    ref.backward(g.double())
    gx = K().bilinear_bwd(to_dev_nhwc(g, dtype, pitch=C + 8), (Hi, Wi), ac)
    # (a 1x1 source sums Ho*Wo gradients into one bf16 value: the bar scales with the sum)
    assert_close(to_cpu_nchw(gx), xa.grad, dtype, "bilinear bwd")
    if Hi == 1:
        # 1x1 source (ASPP image pooling, PSP bin 1): the product path is the autograd function,
        # whose backward is a per-image column sum + the pending BN/ReLU backward
        xr = x.double().requires_grad_()
        sr, tr = s.double().requires_grad_(), t.double().requires_grad_()
        r2 = TF.interpolate(torch.relu(xr * sr.view(1, -1, 1, 1) + tr.view(1, -1, 1, 1)),
                            size=(Ho, Wo), mode="bilinear", align_corners=ac)
        r2.backward(g.double())
        xd = to_dev_nhwc(x, dtype).requires_grad_()
        gam, bet = s.to(DEV).requires_grad_(), t.to(DEV).requires_grad_()
        bn = F().BNState(gam, bet, torch.zeros(C, device=DEV), torch.ones(C, device=DEV),
                         pro[1], pro[2], N * Hi * Wi, False)
        yf = F().bilinear(F().Act(xd, bn, True), (Ho, Wo), align_corners=ac)
        assert_close(to_cpu_nchw(yf), ref.detach(), dtype, "bilinear fwd (autograd path)")
        yf.backward(to_dev_nhwc(g, dtype))
        assert_close(to_cpu_nchw(xd.grad), xr.grad, dtype, "bilinear 1x1-source bwd dx", fac=3)
        # eval-mode BN (mean 0, invstd 1): dgamma = sum g' * x, dbeta = sum g'
        assert_close(gam.grad.cpu(), sr.grad, torch.float32, "bilinear 1x1-source dgamma", fac=300 if dtype == torch.bfloat16 else 20)
        assert_close(bet.grad.cpu(), tr.grad, torch.float32, "bilinear 1x1-source dbeta", fac=300 if dtype == torch.bfloat16 else 20)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", [(9, 17, 33, 65, True), (16, 32, 64, 128, False),
                                  (5, 7, 61, 83, False),
                                  (9, 17, 35, 68, True)])  # Wo % 4 == 0: 16-byte plane stores
def test_logits_upsample_to_nchw_fwd_bwd(geom, dtype):
    Hi, Wi, Ho, Wo, ac = geom
    N, C = 2, 19
    x = quant(rnd((N, C, Hi, Wi), 1), dtype).double().requires_grad_()
    ref = TF.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=ac)
    xd = to_dev_nhwc(x.detach().float(), dtype, pitch=32)
    y = K().upsample_to_nchw(xd, C, (Ho, Wo), ac)
    assert y.dtype == torch.float32 and tuple(y.shape) == (N, C, Ho, Wo)
    assert_close(y.cpu(), ref.detach(), torch.float32, "logits up", fac=3)
    g = rnd(tuple(ref.shape), 2)
    ref.backward(g.double())
    vec = 8 if dtype == torch.bfloat16 else 4
    pitch = (C + vec - 1) // vec * vec
    gx = K().upsample_to_nchw_bwd(g.to(DEV), (Hi, Wi), dtype, pitch, ac)
    assert_close(to_cpu_nchw(gx[..., :C]), x.grad, dtype, "logits up bwd")
    assert (gx[..., C:].float() == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_image_to_nhwc_pad(dtype):
    x = rnd((2, 3, 9, 11), 1)
    y = K().nchw_to_nhwc_pad(x.to(DEV), dtype)
    vec = 8 if dtype == torch.bfloat16 else 4
    assert tuple(y.shape) == (2, 9, 11, vec)
    assert_close(to_cpu_nchw(y)[:, :3], quant(x, dtype), dtype, "image")
    assert (y[..., 3:].float() == 0).all()


def test_errors_are_reported_not_fatal():
    x = torch.zeros((1, 4, 4, 6), device=DEV)  # C=6 is not a multiple of the 16-byte vector
    w = torch.zeros((8, 6), device=DEV)
    with pytest.raises(RuntimeError, match="multiples"):
        K().conv_gemm(x, w, 8, 1, 1, 1, 0, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K().bn_apply(torch.zeros(1, 2, 2, 8))
    # sizes beyond what the float-reciprocal index division of the grid-stride kernels divides
    # exactly (csrc/common.h: fast_div; 2400 x 2400 = 5.76 M pixels x 4 vectors) are refused
    # before any launch: the tensors are dummies
    from segmentron_amd._lib import LIB
    d, big = torch.zeros(64, device=DEV).data_ptr(), 2400
    for name, args in (
            ("seg_maxpool_fwd", (0, d, 16, 1, 2 * big, 2 * big, 16, 3, 2, 1, 0, 0, 0, d, 16, big, big, d, 0)),
            ("seg_maxpool_bwd", (0, d, 16, 1, big, big, 16, 3, 2, 1, d, 16, big // 2, big // 2, d, 0)),
            ("seg_adaptive_avgpool_bwd", (0, d, 16, 1, big, big, 16, 2, d, 16, 0)),
            ("seg_adaptive_avgpool_partial", (0, d, 16, 1, 4097, 4096, 16, 1, d, 4, 0)),
            ("seg_nearest_add", (0, d, 16, 0, 0, 0, d, 16, 0, 0, 0, 1, 0, d, 16, 1, big, big, 16, 0)),
            ("seg_nearest_sum_bwd", (0, d, 16, 1, big, big, 16, 0, d, 16, 0))):
        with pytest.raises(RuntimeError, match="float-reciprocal index|divides exactly"):
            LIB.call(name, *args)
    torch.cuda.synchronize()  # (nothing was launched, nothing faulted)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_criss_cross_attention_argument_errors_are_reported_not_fatal(dtype):
    """csrc/cca.hip refuses, with the library's error and before any launch: more than 512
    attended entries (the eight trips of the dot kernels), a channel count or a row pitch that is
    not a multiple of the 16-byte vector.  Every tensor is real and of the stated shape."""
    vec = 8 if dtype == torch.bfloat16 else 4
    z = lambda *s: torch.zeros(s, dtype=dtype, device=DEV)
    # H + W - 1 = 513, in each of the three entry points
    q, att = z(1, 2, 512, vec), torch.zeros((1, 2, 512, 513), device=DEV)
    with pytest.raises(RuntimeError, match="cca_attention: H \\+ W - 1 = 513 exceeds 512"):
        K().cca_attention(q, q)
    with pytest.raises(RuntimeError, match="cca_attention_bwd: H \\+ W - 1 = 513 exceeds 512"):
        K().cca_attention_bwd(q, q, att)
    with pytest.raises(RuntimeError, match="cca_map: H \\+ W - 1 = 513 exceeds 512"):
        K().cca_map(att, q)
    # (512 entries are served: tests/test_attention_gpu.py)
    # C not a multiple of the channel vector
    odd, att = z(1, 4, 5, vec + vec // 2), torch.zeros((1, 4, 5, 8), device=DEV)
    for call in (lambda: K().cca_attention(odd, odd), lambda: K().cca_attention_bwd(odd, odd, att),
                 lambda: K().cca_map(att, odd)):
        with pytest.raises(RuntimeError, match="must be multiples of %d" % vec):
            call()
    # a pitch that is not a vector multiple: input, second input, residual
    ok = z(1, 4, 5, vec)
    pitched = z(1, 4, 5, vec + vec // 2)[..., :vec]
    for call in (lambda: K().cca_attention(pitched, ok), lambda: K().cca_attention(ok, pitched),
                 lambda: K().cca_attention_bwd(ok, pitched, att), lambda: K().cca_map(att, pitched)):
        with pytest.raises(RuntimeError, match="must be multiples of %d" % vec):
            call()
    with pytest.raises(RuntimeError, match="bad residual pitch"):
        K().cca_map(att, ok, res=pitched)
    torch.cuda.synchronize()  # (nothing was launched, nothing faulted)


# ------------------------------------------------------------------------------ BN fold
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("O,C", [(136, 200), (728, 728), (40, 72), (19, 50), (256, 2048)])
def test_fold_weights_pack_transpose_and_bias(dtype, O, C):
    """W' = W diag(s) row-major and transposed, b' = W t — the tiled kernel (C % 4 == 0 and
    O % 8 == 0, ragged 64x64 tiles) and the wave-per-row fallback (19 x 50)."""
    w = rnd((O, C), 11, 0.3)
    s, t = torch.rand(C) + 0.5, rnd((C,), 12, 0.4)
    Km = K()
    wp, wpt, bp = Km.fold_weights(w.to(DEV), s.to(DEV), t.to(DEV), dtype, want_transpose=True)
    ref = (w.double() * s.double()[None, :])
    tol = 2 ** -23 if dtype == torch.float32 else 2 ** -8
    got, gott = wp.cpu().double(), wpt.cpu().double()
    assert got.shape == (O, C) and gott.shape == (C, O)
    assert ((got - ref).abs() <= tol * ref.abs() + 1e-7).all()
    assert torch.equal(gott, got.t())
    bref = w.double() @ t.double()
    assert (bp.cpu().double() - bref).abs().max() <= 1e-5 * (w.abs().double() @ t.abs().double()).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fold_linear_bn_into_pointwise_matches_autograd(dtype):
    """relu_first SeparableConv2d tail: dw_raw -> BN_train(bn_depth) -> 1x1 conv -> (BN_train
    follows, so the constant W@shift is dropped).  Forward, dW, dgamma, dbeta and dx_raw through
    the folded path vs torch autograd of conv(batch_norm(x))."""
    N, C, O, H, W = 2, 72, 40, 9, 11
    x = quant(rnd((N, C, H, W), 1) * 1.3 + 0.2, dtype)
    wt = rnd((O, C, 1, 1), 2, 0.2)
    gamma, beta = (torch.rand(C) + 0.5), rnd((C,), 3, 0.2)
    xr = x.double().requires_grad_()
    wr = wt.double().requires_grad_()
    gr, br = gamma.double().requires_grad_(), beta.double().requires_grad_()
    xn = TF.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-3)
    y = TF.conv2d(xn, wr)
    dy = quant(rnd(tuple(y.shape), 5), dtype)
    y.backward(dy.double())
    Fm, Km = F(), K()
    sums = torch.cat([x.double().sum((0, 2, 3)), (x.double() ** 2).sum((0, 2, 3))]).to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    mean, invstd, scale, shift = Km.bn_finalize(sums, N * H * W, gd, bd, 1e-3, 0.1, None, None)
    w2d = wt.view(O, C).to(DEV)
    wp, wpt, bp = Km.fold_weights(w2d, scale, shift, dtype, want_transpose=True)
    xd = to_dev_nhwc(x, dtype)
    yd, _ = Km.conv_gemm(xd, wp, O, 1, 1, 1, 0, 1, None, bp)
    assert_close(to_cpu_nchw(yd), y.detach(), dtype, "folded fwd", fac=2)
    dyd = to_dev_nhwc(dy, dtype)
    dwp = Km.conv_wgrad(xd, dyd, O, 1, 1, 1, 0, 1, None)
    db = dy.sum((0, 2, 3)).to(DEV)  # general case: the constant term W@shift carries gradient
    dW, dsdt = Km.fold_bwd_reduce(w2d, dwp, scale, shift, db)
    dgamma, dbeta, c0, c1 = Km.fold_bwd_finalize(dsdt, N * H * W, mean, invstd, gd, scale)
    # the same from the weight-gradient GEMM's split partials [S, O*C] (summed inside)
    parts = Km.conv_wgrad(xd, dyd, O, 1, 1, 1, 0, 1, None, raw_partial=True)
    fake = torch.stack([parts.sum(0) * 0.25, parts.sum(0) * 0.5, parts.sum(0) * 0.25])
    for pp in (parts, fake):
        dW2, dsdt2 = Km.fold_bwd_reduce(w2d, pp.contiguous(), scale, shift, db)
        assert_close(dW2.cpu(), dW.cpu().double(), torch.float32, "fold dW from splits", fac=5)
        assert_close(dsdt2.sum(0).cpu(), dsdt.sum(0).cpu().double(), torch.float32,
                     "fold dsdt from splits", fac=20)
    dx, _ = Km.conv_gemm(dyd, wpt, C, 1, 1, 1, 0, 1, ep=(xd, c0, c1))
    assert_close(dW.view(O, C, 1, 1).cpu(), wr.grad, torch.float32, "folded dW", fac=50)
    assert_close(dgamma.cpu(), gr.grad, torch.float32, "folded dgamma", fac=50)
    assert_close(dbeta.cpu(), br.grad, torch.float32, "folded dbeta", fac=50)
    assert_close(to_cpu_nchw(dx), xr.grad, dtype, "folded dx", fac=3)


# ------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", [(2, 17, 23, 64), (3, 6, 6, 512), (2, 1, 1, 2048),
                                  (1, 65, 129, 256), (2, 33, 35, 24)])
def test_group_norm_fwd_bwd_matches_torch(geom, dtype):
    """nn.GroupNorm(min(32, C), C) — the reference's 'GN' norm layer (modules/batch_norm.py:
    105-108) — forward, dx, dgamma, dbeta against torch in float64: 2 .. 64 channels per group,
    one channel per group (C = 24), a 1 x 1 map (statistics over the group's channels only), the
    PSP pyramid bins; also written into a channel slice of a wider buffer."""
    N, H, W, C = geom
    gn = torch.nn.GroupNorm(min(32, C), C).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.5)
        gn.bias.copy_(rnd((C,), 4, 0.3))
    x = quant(rnd((N, C, H, W), 1) * 1.5 + 0.4, dtype)
    dz = quant(rnd((N, C, H, W), 2), dtype)
    xr = x.double().requires_grad_()
    wr, br = gn.weight.detach().cpu().double().requires_grad_(), gn.bias.detach().cpu().double().requires_grad_()
    ref = TF.group_norm(xr, gn.num_groups, wr, br, gn.eps)
    ref.backward(dz.double())
    xd = to_dev_nhwc(x, dtype).requires_grad_()
    z = F().group_norm(xd, gn).t
    z.backward(to_dev_nhwc(dz, dtype))
    assert_close(to_cpu_nchw(z.detach()), ref.detach(), dtype, "gn z", fac=2)
    assert_close(to_cpu_nchw(xd.grad), xr.grad, dtype, "gn dx", fac=4)
    scale = (dz.double().abs() * ((x.double() - x.double().mean()) / x.double().std()).abs()).sum((0, 2, 3)).max().item()
    assert_close(gn.weight.grad.cpu(), wr.grad, torch.float32, "gn dgamma", scale=scale, fac=20)
    assert_close(gn.bias.grad.cpu(), br.grad, torch.float32, "gn dbeta",
                 scale=dz.double().abs().sum((0, 2, 3)).max().item(), fac=20)
    # into a channel slice of a concat buffer (functional.conv_bn(out=...))
    vec = 8 if dtype == torch.bfloat16 else 4
    buf = torch.full((N, H, W, C + 2 * vec), float("nan"), dtype=dtype, device=DEV)
    with torch.no_grad():
        z2 = F().group_norm(xd.detach(), gn, out=buf[..., vec:vec + C]).t
    assert z2.data_ptr() == buf[..., vec:vec + C].data_ptr()
    assert torch.equal(z2, z.detach()) and torch.isnan(buf[..., :vec].float()).all() \
        and torch.isnan(buf[..., vec + C:].float()).all()


# ------------------------------------------------------------------------------ pooling / misc
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_maxpool_fwd_bwd(dtype):
    N, C, H, W = 2, 40, 17, 21
    x = quant(rnd((N, C, H, W), 1), dtype)
    pro, s, t = _pro(3, C, 4)
    xa = _act_ref(x, 3, s, t).double().requires_grad_()
    ref = TF.max_pool2d(xa, 3, 2, 1)
    y, idx = K().maxpool(to_dev_nhwc(x, dtype), 3, 2, 1, pro)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "maxpool fwd")
    g = quant(rnd(tuple(ref.shape), 2), dtype)
    ref.backward(g.double())
    gx = K().maxpool_bwd(to_dev_nhwc(g, dtype), idx, (H, W), 3, 2, 1)
    # ties (ReLU zeros) may pick a different-but-equal winner than ATen only if the scan order
    # differed; it does not: compare exactly up to rounding
    assert_close(to_cpu_nchw(gx), xa.grad, dtype, "maxpool bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("o", [1, 2, 3, 6])
def test_adaptive_avgpool_fwd_bwd(o, dtype):
    N, C, H, W = 2, 48, 13, 17  # not divisible by 2/3/6 -> overlapping bins
    x = quant(rnd((N, C, H, W), 1), dtype).double().requires_grad_()
    ref = TF.adaptive_avg_pool2d(x, o)
    xd = to_dev_nhwc(x.detach().float(), dtype)
    sums = K().adaptive_avgpool_sums(xd, o)
    areas = K().adaptive_bin_areas(H, W, o, sums.device)
    got = (sums / areas.view(1, o, o, 1)).cpu().permute(0, 3, 1, 2)
    assert_close(got, ref.detach(), torch.float32, "adaptive pool fwd", fac=5)
    g = quant(rnd(tuple(ref.shape), 2), dtype)
    ref.backward(g.double())
    gx = K().adaptive_avgpool_bwd(to_dev_nhwc(g, dtype), (H, W))
    assert_close(to_cpu_nchw(gx), x.grad, dtype, "adaptive pool bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [(2, 15, 19, 32, 64, 3, 2, 1, 1), (1, 14, 18, 16, 32, 3, 2, 2, 2),
                                  (2, 12, 12, 64, 32, 3, 1, 1, 1)])
def test_strided_dense_conv_dgrad_via_transposed_gather(case, dtype):
    N, H, W, C, O, k, stride, pad, dil = case
    x = rnd((N, C, H, W), 1).double().requires_grad_()
    w = quant(rnd((O, C, k, k), 2, 0.1), dtype)
    y = TF.conv2d(x, w.double(), None, stride, pad, dil)
    dy = quant(rnd(tuple(y.shape), 3), dtype)
    y.backward(dy.double())
    wt = F().pack_conv_weight_tconv(w.to(DEV), O, dtype)
    g, _ = K().conv_gemm(to_dev_nhwc(dy, dtype), wt, C, k, k, stride, pad, dil, tconv_out_hw=(H, W))
    assert_close(to_cpu_nchw(g), x.grad, dtype, "tconv dgrad")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_elementwise_dropout_mask_forward_backward(dtype):
    N, C, H, W = 2, 40, 7, 9
    x = quant(rnd((N, C, H, W), 1), dtype)
    gamma, beta = torch.rand(C) + 0.5, rnd((C,), 3, 0.2)
    mask = quant((torch.rand(N, C, H, W) > 0.3).float() / 0.7, dtype)
    xr = x.double().requires_grad_()
    y = torch.relu(TF.batch_norm(xr, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)) * mask.double()
    g = quant(rnd((N, C, H, W), 5), dtype)
    y.backward(g.double())
    sums = torch.cat([x.double().sum((0, 2, 3)), (x.double() ** 2).sum((0, 2, 3))]).to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    mean, invstd, scale, shift = K().bn_finalize(sums, N * H * W, gd, bd, 1e-5, 0.1, None, None)
    md = to_dev_nhwc(mask, dtype)
    got = K().bn_apply(to_dev_nhwc(x, dtype), (3, scale, shift), elem_mul=md)
    assert_close(to_cpu_nchw(got), y.detach(), dtype, "dropout fwd")
    bn = F().BNState(gd, bd, mean, invstd, scale, shift, float(N * H * W), True)
    dx, _, _ = F().bn_input_backward(to_dev_nhwc(g, dtype), to_dev_nhwc(x, dtype), bn, True, elem_mul=md)
    assert_close(to_cpu_nchw(dx), xr.grad, dtype, "dropout bwd", fac=3)


# ------------------------------------------------------------------------------ HRNet fuse
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("post_relu", [False, True])
def test_nearest_upsample_add_fwd_bwd(shift, post_relu, dtype):
    """y = relu?(act(x) + nn.Upsample(2^shift, 'nearest')(bn(r)))  (hrnet.py:186,215-229)."""
    N, C, Hr, Wr = 2, 32, 3, 5
    H, W = Hr << shift, Wr << shift
    x = quant(rnd((N, C, H, W), 1), dtype)
    r = quant(rnd((N, C, Hr, Wr), 2), dtype)
    pro_r, s, t = _pro(2, C, 5)
    xa = x.double().requires_grad_()
    ra = r.double().requires_grad_()
    up = TF.interpolate(_act_ref(ra, 2, s.double(), t.double()), scale_factor=2 ** shift, mode="nearest")
    ref = torch.relu(xa) + up
    if post_relu:
        ref = torch.relu(ref)
    xd, rd = to_dev_nhwc(x, dtype), to_dev_nhwc(r, dtype)
    y = K().nearest_add(xd, (1, None, None), rd, pro_r, shift, post_relu)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "nearest_add fwd")
    g = quant(rnd(tuple(ref.shape), 3), dtype)
    ref.backward(g.double())
    gd = to_dev_nhwc(g, dtype)
    if post_relu:
        gd = K().bn_bwd_apply(gd, y, (1, None, None))
    gr = K().nearest_sum_bwd(gd, shift)
    # d/d(bn(r)) — the BN affine backward itself is covered by test_bn_backward_matches_autograd
    want = ra.grad / s.double().view(1, -1, 1, 1)
    assert_close(to_cpu_nchw(gr), want, dtype, "nearest_sum_bwd", fac=4)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conv_bias_before_training_batchnorm_is_dropped_exactly(dtype):
    """conv(+bias) -> training BN (hrnet_seg.py:22-29): the stored tensor omits the bias, the BN
    output, the running_mean (which sees the bias) and all gradients match autograd."""
    import torch.nn as nn
    N, C, O, H, W = 2, 48, 40, 9, 11
    conv = nn.Conv2d(C, O, 1, bias=True)
    bn = nn.BatchNorm2d(O, momentum=0.01)
    with torch.no_grad():
        conv.weight.copy_(quant(rnd((O, C, 1, 1), 1, 0.2), dtype))
        conv.bias.copy_(rnd((O,), 2, 1.0))
        bn.weight.copy_(torch.rand(O, generator=torch.Generator().manual_seed(3)) + 0.5)
        bn.bias.copy_(rnd((O,), 4, 0.3))
    x = quant(rnd((N, C, H, W), 5), dtype)
    import copy
    conv_r, bn_r = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
    xr = x.double().requires_grad_()
    ref = torch.relu(bn_r(conv_r(xr)))
    g = quant(rnd(tuple(ref.shape), 6), dtype)
    ref.backward(g.double())
    conv, bn = conv.to(DEV), bn.to(DEV)
    xd = to_dev_nhwc(x, dtype).requires_grad_()
    a = F().conv_bn(F().Act(xd), conv, bn)
    a.relu = True
    y = F().materialize(a)
    assert_close(to_cpu_nchw(y.detach()), ref.detach(), dtype, "conv+bias+bn fwd", fac=4)
    y.backward(to_dev_nhwc(g, dtype))
    assert_close(bn.running_mean.cpu(), bn_r.running_mean, torch.float32, "running_mean", fac=50)
    assert_close(bn.running_var.cpu(), bn_r.running_var, torch.float32, "running_var", fac=50)
    assert_close(to_cpu_nchw(xd.grad), xr.grad, dtype, "dx", fac=12)
    assert_close(conv.weight.grad.cpu(), conv_r.weight.grad, dtype, "dW", fac=8)
    assert_close(bn.weight.grad.cpu(), bn_r.weight.grad, dtype, "dgamma", fac=8)
    assert conv.bias.grad is not None and float(conv.bias.grad.abs().max()) == 0.0
    assert float(conv_r.bias.grad.abs().max()) < 1e-9


# ------------------------------------------------------------------------------ fused loss tail
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", [(2, 17, 33, 65, 129, 19), (1, 33, 65, 129, 257, 21),
                                  (2, 9, 13, 33, 49, 30), (1, 8, 8, 8, 8, 2),
                                  # r05: 4.1x .. 8.1x (output-stride-8 heads): 3x3 / 2x2 tiles,
                                  # exact x8, ragged (tiles cut by the border), mixed h / w factors
                                  (2, 9, 17, 65, 129, 19), (1, 10, 14, 70, 100, 19),
                                  (1, 7, 11, 49, 81, 30), (1, 6, 21, 41, 84, 24)])
def test_fused_upsample_cross_entropy_matches_torch(geom, dtype):
    """seg_upsample_ce_fwd/bwd vs F.cross_entropy(F.interpolate(lo, size, 'bilinear',
    align_corners=True), target, ignore_index=-1) in float64 (solver/loss.py:16-46 +
    deeplabv3_plus.py:44): loss and the gradient w.r.t. the low-resolution logits."""
    N, Hi, Wi, H, W, C = geom
    lo = quant(rnd((N, C, Hi, Wi), 1) * 2.0, dtype)
    g = torch.Generator().manual_seed(5)
    target = torch.randint(0, C, (N, H, W), generator=g)
    target[torch.rand(N, H, W, generator=g) < 0.1] = -1
    ref_in = lo.double().requires_grad_()
    ref = TF.cross_entropy(TF.interpolate(ref_in, (H, W), mode="bilinear", align_corners=True),
                           target, ignore_index=-1)
    ref.backward(torch.tensor(1.7, dtype=torch.float64))
    vec = K().vec_of(dtype)
    pitch = (C + 2 * vec - 1) // vec * vec
    lod = to_dev_nhwc(lo, dtype, pitch=pitch, off=0).requires_grad_()
    view = F().LogitsView(lod, (H, W), True)
    loss = TF.cross_entropy(view, target.to(DEV), ignore_index=-1)   # __torch_function__ -> fused
    assert loss.dim() == 0 and loss.dtype == torch.float32 and view._full is None
    assert abs(loss.item() - ref.item()) <= 2e-5 * abs(ref.item()) + 1e-6
    (loss * 1.7).backward()
    got = to_cpu_nchw(lod.grad)
    assert_close(got, ref_in.grad, dtype, "fused CE dlo", fac=1.0)
    # every other consumer sees the materialised tensor
    full = view.materialize()
    refu = TF.interpolate(lo.double(), (H, W), mode="bilinear", align_corners=True)
    assert tuple(view.shape) == tuple(full.shape) == (N, C, H, W)
    assert_close(full.detach().cpu(), refu, torch.float32, "materialised logits", fac=5)
    assert torch.equal(torch.argmax(view, 1), full.argmax(1))
    # unsupported variants fall back to the materialised path (class weights here)
    wts = torch.rand(C) + 0.5
    l2 = TF.cross_entropy(view, target.to(DEV), weight=wts.to(DEV), ignore_index=-1)
    r2 = TF.cross_entropy(refu, target, weight=wts.double(), ignore_index=-1)
    assert abs(l2.item() - r2.item()) <= 1e-4 * abs(r2.item())


def test_fused_cross_entropy_all_ignored_is_nan_like_torch():
    lo = to_dev_nhwc(rnd((1, 19, 5, 7), 1), torch.float32, pitch=24, off=0).requires_grad_()
    view = F().LogitsView(lo, (17, 25), True)
    t = torch.full((1, 17, 25), -1, dtype=torch.long, device=DEV)
    loss = TF.cross_entropy(view, t, ignore_index=-1)
    assert torch.isnan(loss)
    loss.backward()
    assert torch.isfinite(lo.grad).all() and float(lo.grad.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_frozen_batchnorm_is_a_constant_affine_in_train_mode(dtype):
    """get_norm('FrozenBN') (segmentron/modules/batch_norm.py:10-104) behind a conv, module in
    TRAIN mode: y = relu(conv(x) * scale + shift) with the buffers' constant scale / shift, no
    statistics, no running-stat update; gradients flow to the conv weight and the input."""
    import torch.nn as nn
    from segmentron_amd.modules.batch_norm import FrozenBatchNorm2d
    Fm = F()
    N, C, O, H, W = 2, 16, 24, 9, 11
    x = quant(rnd((N, C, H, W), 1), dtype)
    conv = nn.Conv2d(C, O, 3, padding=1, bias=False)
    conv.weight.data = quant(rnd((O, C, 3, 3), 2, 0.2), dtype)
    bn = FrozenBatchNorm2d(O, eps=1e-3).train()
    bn.weight.copy_(torch.rand(O) + 0.5)
    bn.bias.copy_(rnd((O,), 3, 0.3))
    bn.running_mean.copy_(rnd((O,), 4, 0.2))
    bn.running_var.copy_(torch.rand(O) + 0.5)
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    xr = x.double().requires_grad_()
    wr = conv.weight.detach().double().requires_grad_()
    scale = bn.weight.double() * (bn.running_var.double() + bn.eps).rsqrt()
    z = TF.conv2d(xr, wr, None, 1, 1) * scale.view(1, -1, 1, 1) \
        + (bn.bias.double() - bn.running_mean.double() * scale).view(1, -1, 1, 1)
    ref = torch.relu(z)
    g = quant(rnd(tuple(ref.shape), 5), dtype)
    conv, bn = conv.to(DEV), bn.to(DEV)
    xd = to_dev_nhwc(x, dtype).requires_grad_()
    a = Fm.conv_bn(Fm.Act(xd), conv, bn)
    a.relu = True
    y = Fm.materialize(a)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "frozen bn fwd", fac=2)
    # backward reference with the ReLU decisions of the HIP forward: a pre-activation within
    # bf16 rounding of zero may land on either side (the conv output is stored in bf16 before the
    # affine), and ONE flipped unit moves a 3x3 patch of dx by its full weight — this test drew
    # its BatchNorm parameters from the unseeded global generator until r05 and failed on such a
    # tie once (7.6e-2) after passing for two rounds
    mask = (to_cpu_nchw(y) > 0).double()
    flips = int((mask != (z.detach() > 0).double()).sum())
    assert flips <= 0.002 * mask.numel(), flips
    (z * mask).backward(g.double())
    y.backward(to_dev_nhwc(g, dtype))
    assert_close(to_cpu_nchw(xd.grad), xr.grad, dtype, "frozen bn dx", fac=4)
    assert_close(conv.weight.grad.cpu(), wr.grad, dtype, "frozen bn dW", fac=4)
    for k, v in bn.state_dict().items():
        assert torch.equal(v.cpu(), before[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [(7, 9), (8, 8)])
def test_danet_position_and_channel_attention_fwd_bwd(hw, dtype):
    """functional.position_attention / channel_attention (DANet PAM / CAM,
    segmentron/modules/module.py:100-162) vs the reference formulas in float64: torch.bmm ->
    softmax -> torch.bmm, gamma * out + x; forward and every gradient.  H*W = 63 exercises the
    masked padding columns of the attention matrix."""
    Fm = F()
    N, C, D = 2, 32, 8
    H, W = hw
    fac = 3 if dtype == torch.float32 else 6
    x = quant(rnd((N, C, H, W), 1, 0.7), dtype)
    q, k = quant(rnd((N, D, H, W), 2, 0.8), dtype), quant(rnd((N, D, H, W), 3, 0.8), dtype)
    v = quant(rnd((N, C, H, W), 4), dtype)
    gamma = torch.tensor([0.7])
    g = quant(rnd((N, C, H, W), 5), dtype)
    # ---- PAM
    leaves = [t.double().requires_grad_() for t in (q, k, v, x, gamma)]
    qr, kr, vr, xr, gr = leaves
    pq = qr.view(N, -1, H * W).permute(0, 2, 1)
    att = torch.softmax(torch.bmm(pq, kr.view(N, -1, H * W)), dim=-1)
    ref = gr * torch.bmm(vr.view(N, -1, H * W), att.permute(0, 2, 1)).view(N, C, H, W) + xr
    ref.backward(g.double())
    dev = [to_dev_nhwc(t, dtype).requires_grad_() for t in (q, k, v, x)]
    gd = gamma.to(DEV).requires_grad_()
    y = Fm.position_attention(*dev, gd)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "PAM fwd", fac=fac)
    y.backward(to_dev_nhwc(g, dtype))
    for name, d, r in zip("qkvx", dev, leaves):
        assert_close(to_cpu_nchw(d.grad), r.grad, dtype, "PAM d" + name, fac=fac)
    # (d gamma = <dout, raw>: ONE scalar out of a cancelling sum over N*H*W*C bf16 products)
    assert_close(gd.grad.cpu(), gr.grad, dtype, "PAM dgamma", fac=fac * 5)
    # ---- CAM
    xr = (x * 0.5).double().requires_grad_()
    gr = gamma.double().requires_grad_()
    pq = xr.view(N, C, -1)
    energy = torch.bmm(pq, pq.permute(0, 2, 1))
    att = torch.softmax(energy.max(-1, keepdim=True)[0].expand_as(energy) - energy, dim=-1)
    ref = gr * torch.bmm(att, pq).view(N, C, H, W) + xr
    ref.backward(g.double())
    xd = to_dev_nhwc(quant(x * 0.5, dtype), dtype).requires_grad_()
    gd = gamma.to(DEV).requires_grad_()
    y = Fm.channel_attention(xd, gd)
    assert_close(to_cpu_nchw(y), ref.detach(), dtype, "CAM fwd", fac=fac)
    y.backward(to_dev_nhwc(g, dtype))
    assert_close(to_cpu_nchw(xd.grad), xr.grad, dtype, "CAM dx", fac=fac)
    assert_close(gd.grad.cpu(), gr.grad, dtype, "CAM dgamma", fac=fac * 5)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [2, 3, 5, 8, 11])
def test_sum_n_and_fork_gradient(n, dtype):
    """seg_sum_n / functional.fork: the gradients of an activation's n consumers meet in one
    n-ary sum (fp32 accumulation in list order, one rounding) — what torch autograd does with
    n-1 element-wise adds (module.py:52-70, xception.py:36-40)."""
    Fm = F()
    N, C, H, W = 2, 40, 7, 9
    xs = [quant(rnd((N, C, H, W), 10 + i), dtype) for i in range(n)]
    devs = [to_dev_nhwc(t, dtype, pitch=C + 8 if i % 2 else None) for i, t in enumerate(xs)]
    got = K().sum_n(devs)
    acc = xs[0].float().clone()
    chunks = [xs[:8], xs[8:]] if n > 8 else [xs]
    ref = None
    for ch in chunks:  # groups of 8, each rounded once (the wrapper's grouping)
        terms = ([ref] if ref is not None else []) + ch
        acc = terms[0].float().clone()
        for t in terms[1:]:
            acc = acc + t.float()
        ref = quant(acc, dtype)
    assert torch.equal(to_cpu_nchw(got), ref)
    # autograd: n consumers with different weights
    t = to_dev_nhwc(xs[0], dtype).requires_grad_()
    parts = Fm.fork(t, n)
    ws = [0.25 * (i + 1) for i in range(n)]
    sum((p * w).sum() for p, w in zip(parts, ws)).backward()
    want = torch.full((N, C, H, W), sum(ws))
    assert_close(to_cpu_nchw(t.grad), want, dtype, "fork gradient")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_multi_matches_torch_casts_and_transposes(dtype):
    """seg_pack_multi / functional.packed_pointwise: the GEMM operands of the non-folded 1x1
    convolutions, re-made once per optimizer step in one multi-tensor launch — bit-identical to
    torch's `.to(dtype)` / transposing copy; the cache follows the parameter version."""
    Fm = F()
    shapes = [(19, 256), (256, 304), (48, 256), (1536, 2048), (130, 70)] + [(64, 64)] * 40
    srcs = [rnd(s, 30 + i).to(DEV) for i, s in enumerate(shapes)]
    jobs = [(t, bool(i % 2)) for i, t in enumerate(srcs)] + [(srcs[3], True), (srcs[4], True)]
    outs = K().pack_multi(jobs, dtype)
    for (t, tr), o in zip(jobs, outs):
        want = (t.t() if tr else t).to(dtype).contiguous()
        assert torch.equal(o, want), (tuple(t.shape), tr)
    # cache: same object until the parameter changes, then ALL planned packs are re-made
    w1 = torch.nn.Parameter(rnd((32, 16, 1, 1), 1).to(DEV))
    w2 = torch.nn.Parameter(rnd((24, 32, 1, 1), 2).to(DEV))
    a, b = Fm.packed_pointwise(w1, False, dtype), Fm.packed_pointwise(w2, True, dtype)
    assert Fm.packed_pointwise(w1, False, dtype) is a and tuple(b.shape) == (32, 24)
    with torch.no_grad():
        w1.mul_(2.0)
        w2.add_(1.0)
    a2 = Fm.packed_pointwise(w1, False, dtype)
    assert a2 is not a and torch.equal(a2, w1.detach().view(32, 16).to(dtype))
    b2 = Fm._WCACHE[(id(w2), ("pw", True, dtype))][3]  # re-made by the same launch
    assert torch.equal(b2, w2.detach().view(24, 32).t().to(dtype).contiguous())
    assert Fm.packed_pointwise(w2, True, dtype) is b2



@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 65, 129, 728), (1, 33, 50, 72), (2, 130, 259, 232)])
def test_dwconv_bwd_fused_adds_the_forked_gradient_in_its_store(shape, dtype):
    """seg_dwconv3x3_bwd_fused_add (the RES instance of the sliding backward, r06; xception.py:36-42:
    a block input feeds the residual sum and the first separable conv): g = relu_mask(x) * dgrad + res
    with ONE rounding — against the same launch without `res` plus a float64 add; weight-gradient
    partials identical to the launch without `res`."""
    N, H, W, C = shape
    g0 = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(N, H, W, C, device=DEV, generator=g0).to(dtype)
    dy = torch.randn(N, H, W, C, device=DEV, generator=g0).to(dtype)
    res = torch.randn(N, H, W, C, device=DEV, generator=g0).to(dtype)
    w = torch.randn(C, 1, 3, 3, device=DEV, generator=g0) * 0.3
    pro = (1, None, None)
    g_plain, pw0, _ = K().dwconv_bwd_fused(x, dy, w, 1, pro, want_bn=False, torch_layout=True, raw_dw=True)
    g_res, pw1, _ = K().dwconv_bwd_fused(x, dy, w, 1, pro, want_bn=False, torch_layout=True, raw_dw=True,
                                         res=res)
    assert torch.equal(pw0, pw1)
    ref = g_plain.double() + res.double()
    # g_plain is already rounded to the storage dtype: one more rounding of the sum
    tol = (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -22) * ref.abs().max().item()
    assert (g_res.double() - ref).abs().max().item() <= tol
