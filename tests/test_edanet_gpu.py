"""GPU: EDANet on the HIP path against the reference's fixtures (tests/golden/edanet_*.npz,
tools/gen_golden_edanet.py) and the float64 restatement (tests/_edanet_oracle.py): evaluation, a
second size divisible by 8 but not by 16, one training step at 4 x 128 x 192 (16 x 24 maps at 1/8:
at dilation 16 every side tap along H is outside), the small fixture on the few-sample BatchNorm
path, bf16, the fused loss tier, HIP-graph replay == eager launches bit for bit — tests/_zoo.py's
checks — and what only this model has: the dense stage buffers, forward and backward, and
Dropout2d on the 40 new channels of a block."""
import pytest
import torch

import _zoo as Z
from _edanet_spec import EDANET as SPEC, fresh_cfg  # noqa: F401  (autouse)
from _util import DEV, quant, rnd

pytestmark = pytest.mark.gpu

O = SPEC.O


def test_eval_fp32_matches_reference_fixture():
    Z.check_eval_fixture(SPEC)


def test_eval_second_size_matches_oracle():
    """72 x 104: 9 x 13 maps at 1/8, odd in both axes."""
    Z.check_eval_second_size(SPEC)


def test_train_fp32_matches_reference_and_fp64_oracle():
    Z.check_train_fp32(SPEC)


def test_small_train_fp32_matches_reference_fixture():
    """2 x 64 x 96: the BatchNorms at 1/8 resolution see 192 rows, the few-sample path."""
    from segmentron_amd import hip_ops
    B, H, W = SPEC.eval_shape
    assert B * (H // 8) * (W // 8) <= hip_ops.SMALL_BN_ROWS
    Z.check_small_train(SPEC, Z.build(SPEC, torch.float32, True)[0])


def test_train_bf16_is_finite_and_as_close_as_autocast():
    Z.check_train_bf16(SPEC)


def test_reference_criterion_takes_the_fused_tier():
    Z.check_fused_tier(SPEC)


def test_graph_mode_equals_eager_bit_for_bit():
    Z.check_graph_equals_eager(SPEC)


# ---------------------------------------------------------------------------- the dense stages
def _traced_step(dtype):
    """One training step at the small fixture's size with hooks on every block: -> per stage the
    blocks' outputs and the gradients that arrived at them, plus the stage input's."""
    from segmentron_amd.models.edanet import EDABlock
    model, _ = Z.build(SPEC, dtype, True)
    outs, grads = {}, {}

    def fwd_hook(idx):
        def hook(mod, args, out):
            outs[idx] = (args[0], out)
            if out.requires_grad:
                out.register_hook(lambda g: grads.__setitem__(idx, g))
            if idx in (2, 8) and args[0].requires_grad:
                args[0].register_hook(lambda g: grads.__setitem__(idx - 1, g))
        return hook
    for i, layer in enumerate(model.layers):
        if isinstance(layer, EDABlock):
            layer.register_forward_hook(fwd_hook(i))
    B, H, W = SPEC.eval_shape
    from oracle import synth
    x = synth.synth_images(B, H, W, seed=0).cuda()
    y = synth.synth_targets(B, H, W, seed=0).cuda()
    loss = Z.mix_loss(SPEC, model(x), y)
    loss.backward()
    torch.cuda.synchronize()
    return outs, grads


STAGES = [(range(2, 7), 60, 264), (range(8, 16), 130, 456)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_block_outputs_alias_one_buffer_per_stage(dtype):
    """Block j of a stage reads the channel suffix behind offset off_j and returns the suffix
    behind off_j - 40 of the SAME buffer: cat([new, input], 1) without a copy."""
    outs, _ = _traced_step(dtype)
    esz = torch.empty((), dtype=dtype).element_size()
    for blocks, cin, width in STAGES:
        n = len(blocks)
        final = outs[blocks[-1]][1]
        base = final.data_ptr()
        assert final.shape[-1] == width and final.stride(2) == width
        pad = width - (cin + 40 * n)
        assert not final[..., width - pad:].any()  # the pad channels are zero
        for j, i in enumerate(blocks):
            xin, out = outs[i]
            off = 40 * (n - j)
            assert xin.shape[-1] == width - off and out.shape[-1] == width - off + 40
            assert xin.data_ptr() == base + off * esz
            assert out.data_ptr() == base + (off - 40) * esz
            assert xin.stride(2) == width and out.stride(2) == width


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_stage_gradients_arrive_as_one_buffer(dtype):
    """The gradient of every block output — and of the stage's input — is a channel suffix of the
    ONE tensor the stage's consumer wrote: the 1x1 convolutions added into it in place."""
    _, grads = _traced_step(dtype)
    esz = torch.empty((), dtype=dtype).element_size()
    for blocks, cin, width in STAGES:
        n = len(blocks)
        g_final = grads[blocks[-1]]
        base = g_final.data_ptr()
        assert g_final.shape[-1] == width and g_final.is_contiguous()
        for j, i in enumerate(blocks[:-1]):
            off = 40 * (n - 1 - j)
            g = grads[i]
            assert g.data_ptr() == base + off * esz and g.shape[-1] == width - off
            assert g.stride(2) == width
        g_in = grads[blocks[0] - 1]  # the stage's input segment (with its pad)
        assert g_in.data_ptr() == base + 40 * n * esz and g_in.shape[-1] == width - 40 * n
        assert torch.isfinite(g_final).all()


def test_dense_cat_falls_back_to_slice_views_without_the_hand_off():
    """No DenseGrad (or a 1x1 convolution that takes no part): the gradients are the two slice
    views of the incoming tensor, as from a plain concat alias."""
    from segmentron_amd import functional as F
    buf = torch.zeros((1, 3, 5, 16), device=DEV)
    new = buf[..., 4:8].detach().requires_grad_(True)
    prev = buf[..., 8:].detach().requires_grad_(True)
    out = F.dense_cat(new, prev, buf, 4)
    assert out.data_ptr() == buf[..., 4:].data_ptr() and out.shape[-1] == 12
    g = torch.randn((1, 3, 5, 12), device=DEV)
    out.backward(g)
    assert torch.equal(new.grad, g[..., :4]) and torch.equal(prev.grad, g[..., 4:])
    with pytest.raises(ValueError, match="dense_cat"):
        F.dense_cat(buf[..., 0:4], prev, buf, 4)


# ------------------------------------------------------------------------------------ Dropout2d
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_dropout2d_zeroes_or_doubles_whole_planes_of_the_new_channels(dtype):
    """One stage-2 block on [2, 8, 12, 130] with p = 0.5: each (image, channel) plane of the 40 new
    channels is all zero or exactly 2 x the p = 0 plane; the 130 old channels are untouched."""
    import segmentron_amd
    from segmentron_amd.models.edanet import EDABlock
    segmentron_amd.set_compute_dtype(dtype)
    torch.manual_seed(0)
    blk = EDABlock(130, 2).to(DEV).train()
    N, H, W, cin = 2, 8, 12, 130
    width = 136 + 40  # round_up8(130) + 40: the input segment with its zero pad behind it
    src = quant(rnd((N, H, W, cin), 7), dtype).to(dtype).to(DEV)

    def run(p):
        blk.dropout.p = p
        buf = torch.full((N, H, W, width), float("nan"), dtype=dtype, device=DEV)
        buf[..., 40:40 + cin] = src
        buf[..., 40 + cin:] = 0
        with torch.no_grad():
            out = blk(buf[..., 40:], buf, 40)
        assert out.data_ptr() == buf.data_ptr() and out.shape[-1] == width
        return buf
    ref = run(0.0)
    assert torch.isfinite(ref).all() and (ref[..., :40] >= 0).all() and ref[..., :40].any()
    torch.manual_seed(1)
    got = run(0.5)
    assert torch.equal(got[..., 40:], ref[..., 40:])
    zero = doubled = 0
    for n in range(N):
        for c in range(40):
            plane, base = got[n, :, :, c].float(), ref[n, :, :, c].float()
            if not plane.any():
                zero += 1
            else:
                assert torch.equal(plane, 2.0 * base), (n, c)
                doubled += 1
    assert zero >= 10 and doubled >= 10  # 80 fair coins
    # p = 0 in training mode takes no mask at all
    assert torch.equal(run(0.0), ref)


# ------------------------------------------------------------------ the down-sampler's placement
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C,width,lo,total", [(15, 16, 45, 64), (3, 8, 12, 16)])
def test_place_writes_a_misaligned_slice_and_brings_its_gradient_back(C, width, lo, total, dtype):
    """cat([conv 45, pool 15]) / cat([conv 12, pool 3]): the pooled channels start at a channel
    offset that is no whole 16-byte vector.  Forward: only [lo, lo + C) of the buffer changes, to
    the source's first C channels, bit for bit.  Backward: the gradient's slice in the source's
    width, exact zeros in its pad channels.  More than one block and a ragged tail (2 x 37 x 29)."""
    from segmentron_amd import functional as F
    N, H, W = 2, 37, 29
    src = quant(rnd((N, H, W, width), 3), dtype).to(dtype).to(DEV).requires_grad_(True)
    buf = torch.full((N, H, W, total), 777.0, dtype=dtype, device=DEV)
    out = F.place(src, C, buf[..., lo:lo + C])
    assert out.data_ptr() == buf[..., lo:].data_ptr()
    assert torch.equal(buf[..., lo:lo + C], src.detach()[..., :C])
    keep = torch.ones(total, dtype=torch.bool, device=DEV)
    keep[lo:lo + C] = False
    assert (buf[..., keep] == 777.0).all()
    g = quant(rnd((N, H, W, total), 4), dtype).to(dtype).to(DEV)
    out.backward(g[..., lo:lo + C])
    assert torch.equal(src.grad[..., :C], g[..., lo:lo + C])
    assert not src.grad[..., C:].any()
