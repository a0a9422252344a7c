"""GPU: DUNet on the HIP path against the reference's fixtures (tests/golden/dunet_*.npz,
tools/gen_golden_dunet.py) and the float64 restatement (tests/_dunet_oracle.py): evaluation, one
training step, bf16, the fused DUpsampling loss behind the reference's criterion, and HIP-graph
replay == eager launches bit for bit.  The checks themselves are tests/_zoo.py's."""
import numpy as np
import pytest
import torch

import _zoo as Z
from _zoo import DUNET as SPEC, fresh_cfg  # noqa: F401  (autouse)
from oracle import synth

pytestmark = pytest.mark.gpu
O = SPEC.O


def test_eval_fp32_matches_reference_fixture():
    # (the reference returns the aux output in evaluation mode too)
    Z.check_eval_fixture(SPEC)


def test_eval_fp32_output_stride_16_matches_reference_fixture():
    """FeatureFused shrinks c2 to c4's size here (align_corners=True); the output is 8 x c4, half
    the input's size, as in the reference."""
    model, _ = Z.build(SPEC, torch.float32, False, overrides=[
        "SOLVER.AUX", "True", "SOLVER.AUX_WEIGHT", str(O.AUX_WEIGHT), "MODEL.OUTPUT_STRIDE", "16"])
    g = np.load(SPEC.file("os16_eval.npz"))
    with torch.no_grad():
        outs = model(synth.synth_images(O.B, O.H, O.W, seed=0).cuda())
    assert len(outs) == 2
    rels = [Z.rel(outs[i].cpu(), torch.from_numpy(g["logits%d" % i])) for i in range(2)]
    print("dunet OS 16 eval fp32 max-rel %s" % ["%.2e" % r for r in rels])
    assert all(tuple(o.shape) == (O.B, 19, O.H // 2, O.W // 2) for o in outs)
    assert max(rels) < 1e-3


def test_train_fp32_matches_reference_and_fp64_oracle():
    Z.check_train_fp32(SPEC)


def test_train_bf16_is_finite_and_as_close_as_autocast():
    Z.check_train_bf16(SPEC)


def test_reference_criterion_takes_the_fused_path_on_both_heads():
    Z.check_fused_on_every_head(SPEC, "DUpLogitsView")


def test_graph_mode_equals_eager_bit_for_bit():
    Z.check_graph_equals_eager(SPEC)
