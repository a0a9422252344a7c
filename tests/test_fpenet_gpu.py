"""GPU: FPENet on the HIP path against the reference's fixtures (tests/golden/fpenet_*.npz,
tools/gen_golden_fpenet.py) and the float64 restatement (tests/_fpenet_oracle.py): evaluation at
2 x 64 x 96 (8 x 12 maps at 1/8: at dilation 8 every side tap along H is outside) with the output
geometry of 65 x 97, that second size against the restatement, one training step at 4 x 128 x 192
(the plain BatchNorm path at 1/4 resolution, the few-sample one at 1/8), the small fixture, bf16,
the fused loss tier at head stride 2, HIP-graph replay == eager launches bit for bit —
tests/_zoo.py's checks."""
import pytest
import torch

import _zoo as Z
from _fpenet_spec import FPENET as SPEC, fresh_cfg  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

O = SPEC.O


def test_eval_fp32_matches_reference_fixture():
    Z.check_eval_fixture(SPEC)


def test_eval_second_size_matches_oracle():
    """65 x 97: 33 x 49, 17 x 25 and 9 x 13 maps, odd in both axes at every level; 66 x 98 out."""
    Z.check_eval_second_size(SPEC)


def test_train_fp32_matches_reference_and_fp64_oracle():
    from segmentron_amd import hip_ops
    B, H, W = SPEC.train_shape
    assert B * (H // 4) * (W // 4) > hip_ops.SMALL_BN_ROWS >= 1024
    Z.check_train_fp32(SPEC)


def test_small_train_fp32_matches_reference_fixture():
    """2 x 64 x 96: the BatchNorms at 1/4 and 1/8 resolution see 768 and 192 rows, the few-sample
    path."""
    from segmentron_amd import hip_ops
    B, H, W = SPEC.eval_shape
    assert B * (H // 4) * (W // 4) <= hip_ops.SMALL_BN_ROWS
    Z.check_small_train(SPEC, Z.build(SPEC, torch.float32, True)[0])


def test_train_bf16_is_finite_and_as_close_as_autocast():
    Z.check_train_bf16(SPEC)


def test_reference_criterion_takes_the_fused_tier():
    Z.check_fused_tier(SPEC)


def test_graph_mode_equals_eager_bit_for_bit():
    Z.check_graph_equals_eager(SPEC)
