"""GPU: CGNet on the HIP path against the reference's fixtures (tests/golden/cgnet_*.npz,
tools/gen_golden_cgnet.py) and the float64 restatement (tests/_cgnet_oracle.py): evaluation, one
training step at 4 x 128 x 192 (the stage-2 / stage-3 BatchNorms see 6144 / 1536 rows), the small
fixture on the few-sample BatchNorm path with the block-count options, bf16, the fused loss tier
behind the reference's criterion, and HIP-graph replay == eager launches bit for bit.  The checks
themselves are tests/_zoo.py's."""
import pytest
import torch

import _zoo as Z
from _zoo import CGNET as SPEC, fresh_cfg  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu


def test_eval_fp32_matches_reference_fixture():
    Z.check_eval_fixture(SPEC)


def test_eval_odd_size_matches_oracle():
    """65 x 97: every stride-2 stage and the 3/2/1 pools give ceil(H / 2), the slices agree."""
    Z.check_eval_second_size(SPEC)


def test_train_fp32_matches_reference_and_fp64_oracle():
    Z.check_train_fp32(SPEC)


def test_small_train_fp32_matches_reference_fixture():
    """2 x 64 x 96, STAGE2_BLOCK_NUM 2 / STAGE3_BLOCK_NUM 2: the few-sample BatchNorm path."""
    model, _ = Z.build(SPEC, torch.float32, True, overrides=SPEC.small_overrides,
                       keys=SPEC.small_keys())
    assert len(model.stage2) == 1 and len(model.stage3) == 1
    Z.check_small_train(SPEC, model)


def test_train_bf16_is_finite_and_as_close_as_autocast():
    Z.check_train_bf16(SPEC)


def test_reference_criterion_takes_the_fused_tier():
    """CGNet's head sits at stride 8: (H - 1) / (H / 8 - 1) <= 8.1, the fused loss's tier, holds
    from H = 568 on (the config trains at 768) — 576 x 584 here; the small fixtures above are
    below it and take the materialised logits."""
    Z.check_fused_tier(SPEC)


def test_graph_mode_equals_eager_bit_for_bit():
    Z.check_graph_equals_eager(SPEC)
