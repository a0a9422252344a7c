"""GPU: ESPNetV2 on the HIP path against the reference's fixtures (tests/golden/espnetv2_*.npz,
tools/gen_golden_espnetv2.py) and the float64 restatement (tests/_espnetv2_oracle.py): evaluation,
one training step at 4 x 128 x 192 (the 1/8-resolution BatchNorms see 1536 rows, the 1/16 ones 384:
the few-sample path), the small fixture, bf16, SOLVER.AUX, the fused loss tier behind the
reference's criterion, and HIP-graph replay == eager launches bit for bit.  The never-used
level5* / fc parameters keep `grad is None` and their initial values throughout (SPEC.unused).
The checks themselves are tests/_zoo.py's."""
import pytest
import torch

import _zoo as Z
from _zoo import ESPNETV2 as SPEC, fresh_cfg  # noqa: F401  (autouse)
from oracle import synth

pytestmark = pytest.mark.gpu
O = SPEC.O


def test_eval_fp32_matches_reference_fixture():
    Z.check_eval_fixture(SPEC)


def test_eval_second_size_matches_oracle_and_other_sizes_raise():
    """48 x 80: a 3 x 5 map at 1/16, so the pyramid pooling reaches 1 x 1 after two pools.  Sizes
    that are no multiple of 16 raise in the reference (its x2 resizes meet the encoder's maps in a
    concat); here they raise before any launch."""
    model, sd = Z.build(SPEC, torch.float32, False)
    x = synth.synth_images(1, O.H2, O.W2, seed=0)
    with torch.no_grad():
        out = model(x.cuda())[0].cpu()
        for hw in ((65, 97), (64, 100), (56, 96)):
            with pytest.raises(ValueError, match="multiples of 16"):
                model(synth.synth_images(1, hw[0], hw[1], seed=0).cuda())
    ref = O.evaluate(sd, x)[0]
    assert Z.rel(out, ref) < 1e-3


def test_train_fp32_matches_reference_and_fp64_oracle():
    Z.check_train_fp32(SPEC)


def test_small_train_fp32_matches_reference_fixture():
    """2 x 64 x 96: the BatchNorms from 1/8 resolution down see at most 192 rows, the few-sample
    path (the pyramid pooling reaches 1 x 1 maps)."""
    from segmentron_amd import hip_ops
    assert O.B * (O.H // 8) * (O.W // 8) <= hip_ops.SMALL_BN_ROWS
    Z.check_small_train(SPEC, Z.build(SPEC, torch.float32, True)[0])


def test_train_bf16_is_finite_and_as_close_as_autocast():
    Z.check_train_bf16(SPEC)


def test_aux_output_matches_fp64_oracle():
    """SOLVER.AUX True: the second output is project_l3's map before its BatchNorm, resized to the
    input size; no extra parameters.  2 x 64 x 96 against the float64 restatement: both outputs,
    the loss with aux_weight 0.4, the gradients."""
    model, sd = Z.build(SPEC, torch.float32, True, overrides=["SOLVER.AUX", "True"])
    assert model.aux is True
    assert [k for k, _ in model.state_dict().items()] == [k for k, _ in Z.fixture_keys(SPEC)[1]]
    x = synth.synth_images(O.B, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B, O.H, O.W, seed=0)
    outs = model(x.cuda())
    assert len(outs) == 2
    loss = Z.MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=0.4).cuda()(outs, y.cuda())["loss"]
    loss.backward()
    l64, o64, g64, _ = O.train(sd, x, y, torch.float64, aux=True, aux_weight=0.4)
    for i in range(2):
        full = outs[i].materialize() if hasattr(outs[i], "materialize") else outs[i]
        assert tuple(full.shape) == (O.B, 19, O.H, O.W)
        assert Z.rel(full.detach().cpu(), o64[i]) < 1e-3, i
    print("espnetv2 aux: loss %.6f (float64 %.6f)" % (loss.item(), l64))
    assert abs(loss.item() - l64) < 1e-3 * l64
    Z.check_grads_where_used(SPEC, model)
    params = dict(model.named_parameters())
    num = sum((params[k].grad.cpu().double() - g).pow(2).sum().item() for k, g in g64.items())
    den = sum(g.pow(2).sum().item() for g in g64.values())
    print("espnetv2 aux gradients vs fp64 oracle: global rel err %.3e" % (num / den) ** 0.5)
    assert (num / den) ** 0.5 < 1e-3


def test_reference_criterion_takes_the_fused_tier():
    """The final resize is x2 from 1/2 resolution: (H - 1) / (H / 2 - 1) <= 8.1 at every size, so
    a training forward hands the criterion a pending view and the loss runs fused on the
    1/2-resolution logits — 2 x 512 x 528 here."""
    Z.check_fused_tier(SPEC)


def test_graph_mode_equals_eager_bit_for_bit():
    Z.check_graph_equals_eager(SPEC)
