"""GPU: one non-down and one down ContextGuidedBlock (segmentron_amd/models/cgnet.py) in training
mode against the float64 restatement (tests/_cgnet_oracle.py block): output, input gradient and
every parameter gradient.  float32 at 1e-4 relative L2 (the bar of
test_hrnet_module_and_head_gradients_tight); bf16: the output within tol(bf16) of the float64
result computed from bf16-rounded inputs, every gradient tensor within 1.3 x the distance of torch's
own CPU bfloat16 autocast run of the same block from float64 (why: above test_context_guided_block_bf16).

The non-down block (64 -> 64, dilation 2, reduction 8) normalises 2 x 32 x 40 = 2560 rows: the
partial-sum BatchNorm path; the down block (35 -> 64, its input the 35-channel concat in a buffer
of 40) normalises 640: the few-sample path."""
import pytest
import torch

import _cgnet_oracle as O
from _util import assert_close
from oracle import synth, torch_ref

pytestmark = pytest.mark.gpu

N, H, W = 2, 32, 40
# PReLU has a kink at 0: an input within float32 rounding distance of it (|z| ~ 1e-7 after sums of
# O(1) terms) falls on either side depending on the summation order, and that ONE element then
# moves whole gradient tensors by 1e-4 .. 1e-3 relative — in torch's own float32 run exactly as on
# the device (seed 7: one of 81920 inputs of the down block's second PReLU at 3.8e-8; torch
# float32 against float64 then reads 3.3e-4 on the input gradient, the device the same).  The
# inputs are drawn from a seed whose nearest PReLU input stays MIN_MARGIN away in float64, which
# every run asserts before it compares anything.
SEED, MIN_MARGIN = 13, 1e-5


def _block(down, dtype):
    import segmentron_amd
    from segmentron_amd.models.cgnet import ContextGuidedBlock
    segmentron_amd.set_compute_dtype(dtype)
    if down:
        mod = ContextGuidedBlock(35, 64, dilation=2, reduction=8, down=True, residual=False)
    else:
        mod = ContextGuidedBlock(64, 64, dilation=2, reduction=8)
    sd = O.state([(k, tuple(v.shape)) for k, v in mod.state_dict().items()])
    mod.load_state_dict(sd)
    return mod.cuda().train(), sd


def _run(down, dtype):
    """-> [(name, HIP result, float64 result)] : output, input gradient, parameter gradients; in
    bf16 a fourth entry, the gradient of torch's CPU bfloat16 autocast run (None for the output)."""
    import segmentron_amd
    mod, sd = _block(down, dtype)
    cin = 35 if down else 64
    gen = torch.Generator().manual_seed(SEED)
    x = torch.randn(N, cin, H, W, generator=gen)
    Ho, Wo = (H // 2, W // 2) if down else (H, W)
    gy = torch.randn(N, 64, Ho, Wo, generator=gen)
    if dtype == torch.bfloat16:  # the oracle sees what the device stores: bf16-rounded inputs
        x, gy = x.bfloat16().float(), gy.bfloat16().float()
        sd = {k: (v.bfloat16().float() if v.dim() == 4 else v) for k, v in sd.items()}
        mod.load_state_dict(sd)
    try:
        osd = torch_ref.clone_state({("m." + k): (v.double() if v.is_floating_point() else v)
                                     for k, v in sd.items()}, requires_grad=True)
        net = torch_ref.OracleNet(osd, training=True)
        xo = x.double().requires_grad_()
        margins = []
        yo = O.block(net, xo, "m", 2, down, not down, margins)
        # the fixture's own precondition (see SEED): no PReLU input at a tie of the kink
        assert len(margins) == 2 and min(margins) > MIN_MARGIN, margins
        (yo * gy.double()).sum().backward()
        cp = (cin + 7) // 8 * 8
        xh = torch.zeros((N, H, W, cp), dtype=dtype, device="cuda")
        xh[..., :cin] = x.permute(0, 2, 3, 1).to(dtype).cuda()
        xh.requires_grad_()
        yh = mod(xh)
        assert yh.dtype == dtype and tuple(yh.shape) == (N, Ho, Wo, 64)
        (yh.float() * gy.permute(0, 2, 3, 1).contiguous().cuda()).sum().backward()
        gx = xh.grad.float().cpu()
        assert (gx[..., cin:] == 0).all()  # the pad channels of the concat carry no gradient
        out = [("output", yh.detach().float().cpu().permute(0, 3, 1, 2), yo.detach()),
               ("input gradient", gx[..., :cin].permute(0, 3, 1, 2), xo.grad)]
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            out.append((k, p.grad.float().cpu(), osd["m." + k].grad))
        # the running statistics moved as torch's do
        for k, v in mod.state_dict().items():
            if "running_" in k:
                assert_close(v.cpu(), osd["m." + k], dtype, k, fac=2.0)
        if dtype == torch.bfloat16:  # the yardstick: the same step under CPU bfloat16 autocast
            s32 = torch_ref.clone_state({("m." + k): v for k, v in sd.items()}, requires_grad=True)
            xa = x.clone().requires_grad_()
            with torch.autocast("cpu", dtype=torch.bfloat16):
                ya = O.block(torch_ref.OracleNet(s32, training=True), xa, "m", 2, down, not down)
                (ya.float() * gy).sum().backward()
            auto = [None, xa.grad] + [s32["m." + k].grad for k, _ in mod.named_parameters()]
            out = [(n, g, r, a) for (n, g, r), a in zip(out, auto)]
        return out
    finally:
        segmentron_amd.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("down", [False, True], ids=["block", "down"])
def test_context_guided_block_fp32_tight(down):
    rels = {}
    for name, got, ref in _run(down, torch.float32):
        rels[name] = ((got.double() - ref).norm() / ref.norm()).item()
        print("   %-28s rel L2 %.3e" % (name, rels[name]))
    bad = {k: v for k, v in rels.items() if not v < 1e-4}
    assert not bad, bad


# bf16.  The output is a continuous function of every stored tensor: element-wise within tol(bf16)
# of the float64 result computed from bf16-rounded inputs.  A gradient is not: the ~1e-3 of the
# PReLU inputs that lie within a bf16 rounding of the kink take the other slope in ANY bf16 run
# (the inputs are O(1), their density at 0 is about 0.05 per unit, a bf16 rounding is 4e-3: no
# draw of 160 000 inputs keeps them all away), each of them changes the gradient there by
# (1 - alpha) * g, and the BatchNorm affine gradients behind the depthwise pair are remainders of
# cancelling sums (the gradient that leaves a BatchNorm has zero mean per channel).  So the
# distance of a bf16 gradient tensor from float64 is 0.2 - 4.5 % relative L2 on these blocks, in
# torch's own bf16 arithmetic as on the device.  The yardstick is therefore what bf16 costs torch
# itself, tensor by tensor: the same step under CPU bfloat16 autocast, computed here, and for EVERY
# gradient tensor the bar is the project's 1.3 x of that tensor's own autocast distance.
BF16_RATIO = 1.3


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("down", [False, True], ids=["block", "down"])
def test_context_guided_block_bf16(down):
    res = _run(down, torch.bfloat16)
    name, got, ref, _ = res[0]
    assert name == "output"
    print("   %-28s max-normalised error %.3e"
          % (name, ((got.double() - ref).abs().max() / ref.abs().max()).item()))
    assert_close(got, ref, torch.bfloat16, name)
    bad = {}
    for name, got, ref, auto in res[1:]:
        assert torch.isfinite(got).all(), name
        eh, ea = _rel_l2(got, ref), _rel_l2(auto, ref)
        print("   %-28s relative L2 %.3e, CPU autocast %.3e, ratio %.2f (bar %.1f)"
              % (name, eh, ea, eh / ea, BF16_RATIO))
        if not eh <= BF16_RATIO * ea:
            bad[name] = (eh, ea)
    assert not bad, bad
