"""GPU: UNet on the HIP path against the reference's fixtures (tests/golden/unet_*.npz,
tools/gen_golden_unet.py) and the float64 restatement (tests/_unet_oracle.py): evaluation at
2 x 64 x 96 (maps down to 4 x 6) with the output geometry of 70 x 97, that second size against the
restatement (the decoder pads one row at two levels and one column at the top one), one training
step at 4 x 64 x 96 (the plain BatchNorm path at levels 0-2, the few-sample one at levels 3-4), the
small fixture, bf16, the fused loss tier at head stride 1, HIP-graph replay == eager launches bit
for bit — tests/_zoo.py's checks."""
import pytest
import torch

import _zoo as Z
from _unet_spec import UNET as SPEC, fresh_cfg  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

O = SPEC.O


def _rows(B, H, W):
    """Rows per BatchNorm at the five levels."""
    return [B * (H >> l) * (W >> l) for l in range(5)]


def test_eval_fp32_matches_reference_fixture():
    Z.check_eval_fixture(SPEC)


def test_eval_second_size_matches_oracle():
    """70 x 97: 35 x 48, 17 x 24, 8 x 12 and 4 x 6 maps below; the resized 34 x 48 and 16 x 24 maps
    are padded by one row, the resized 70 x 96 one by one column."""
    Z.check_eval_second_size(SPEC)


def test_train_fp32_matches_reference_and_fp64_oracle():
    from segmentron_amd import hip_ops
    rows = _rows(*SPEC.train_shape)
    assert rows == [24576, 6144, 1536, 384, 96] and hip_ops.SMALL_BN_ROWS == 1024
    assert all(r > hip_ops.SMALL_BN_ROWS for r in rows[:3])      # the plain path
    assert all(r <= hip_ops.SMALL_BN_ROWS for r in rows[3:])     # the few-sample path
    Z.check_train_fp32(SPEC)


def test_small_train_fp32_matches_reference_fixture():
    """2 x 64 x 96: levels 2-4 see 768, 192 and 48 rows, the few-sample path."""
    from segmentron_amd import hip_ops
    rows = _rows(*SPEC.eval_shape)
    assert all(r <= hip_ops.SMALL_BN_ROWS for r in rows[2:]) and rows[1] > hip_ops.SMALL_BN_ROWS
    Z.check_small_train(SPEC, Z.build(SPEC, torch.float32, True)[0])


def test_train_bf16_is_finite_and_as_close_as_autocast():
    Z.check_train_bf16(SPEC)


def test_reference_criterion_takes_the_fused_tier():
    """Head stride 1: the final resize is the identity and the fused loss runs at factor 1."""
    Z.check_fused_tier(SPEC)


def test_graph_mode_equals_eager_bit_for_bit():
    Z.check_graph_equals_eager(SPEC)
