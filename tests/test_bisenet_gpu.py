"""GPU: BiSeNet on the HIP path against the reference's fixtures (tests/golden/bisenet_*.npz,
tools/gen_golden_bisenet.py) and the float64 restatement (tests/_bisenet_oracle.py): evaluation,
one training step at batch 4 (the attention BatchNorms normalise N values per channel), the
OUTPUT_STRIDE 32 leg where the inter-stage resize is real, bf16, HIP-graph replay == eager
launches bit for bit, and the fused loss tier behind the reference's criterion.  The checks
themselves are tests/_zoo.py's."""
import numpy as np
import pytest
import torch

import _zoo as Z
from _zoo import BISENET as SPEC, fresh_cfg  # noqa: F401  (autouse)
from oracle import synth

pytestmark = pytest.mark.gpu
O = SPEC.O


def test_eval_fp32_matches_reference_fixture():
    Z.check_eval_fixture(SPEC)


def test_train_fp32_matches_reference_and_fp64_oracle():
    Z.check_train_fp32(SPEC)


def test_train_fp32_output_stride_32_matches_reference_fixture():
    keys = [(k, s) for k, s in Z.fixture_keys(SPEC)[1] if not k.startswith("auxlayer")]
    model, _ = Z.build(SPEC, torch.float32, True, keys=keys, overrides=[
        "SOLVER.AUX", "False", "SOLVER.AUX_WEIGHT", str(O.AUX_WEIGHT), "MODEL.OUTPUT_STRIDE", "32"])
    x = synth.synth_images(O.B_TRAIN, O.H32, O.W32, seed=0)
    y = synth.synth_targets(O.B_TRAIN, O.H32, O.W32, seed=0)
    outs = model(x.cuda())
    assert len(outs) == 1
    loss = Z.mix_loss(SPEC, outs, y.cuda())
    loss.backward()
    t = np.load(SPEC.file("os32_train.npz"))
    rel = Z.rel(outs[0].detach().cpu()[..., ::2, ::2], torch.from_numpy(t["logits0"]))
    print("bisenet OS 32 train fp32: loss %.6f (fixture %.6f), logits max-rel %.2e"
          % (loss.item(), float(t["loss"]), rel))
    assert abs(loss.item() - float(t["loss"])) < 1e-3 * float(t["loss"]) and rel < 1e-3
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


def test_train_bf16_is_finite_and_as_close_as_autocast():
    Z.check_train_bf16(SPEC)


def test_reference_criterion_takes_the_fused_tier_on_all_three_heads():
    Z.check_fused_on_every_head(SPEC, "LogitsView")


def test_graph_mode_equals_eager_bit_for_bit():
    Z.check_graph_equals_eager(SPEC)
