"""CPU: UNet (segmentron/models/unet.py) served by the registry — the reference's config and
state_dict schema (tests/golden/unet_state_keys.json, tools/gen_golden_unet.py), the drop-in
overlay, the decoder list, the refusals (BN_TYPE, inputs below 16, a CPU tensor), the host-side
geometry query of the skip + max-pool backward, and the test-side restatement
(tests/_unet_oracle.py) against the reference's own runs."""
import numpy as np
import pytest
import torch

import _zoo as Z
from _unet_spec import UNET as SPEC

O = SPEC.O


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = Z.cfg_for(SPEC)
        assert cfg.MODEL.MODEL_NAME == "UNet"
        assert cfg.TRAIN.CROP_SIZE == 512 and cfg.TRAIN.BATCH_SIZE == 2
    finally:
        reset_cfg()


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = Z.fixture_keys(SPEC)
    assert len(keys) == SPEC.n_keys and ref["n_params"] == SPEC.n_params
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.unet"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert model.encoder is None
        model.load_state_dict(O.state(keys), strict=True)
        # the reference's module tree, the convolution biases included
        from segmentron_amd.models.unet import DoubleConv, Down, OutConv, Up
        blocks = dict(model.named_modules())
        assert isinstance(blocks["inc"], DoubleConv) and isinstance(blocks["head.outc"], OutConv)
        assert all(isinstance(blocks["down%d" % i], Down) for i in range(1, 5))
        assert all(isinstance(blocks["head.up%d" % i], Up) for i in range(1, 5))
        for p in O.LEVELS + tuple("head.up%d.conv" % i for i in range(1, 5)):
            for j in (0, 3):
                conv = blocks["%s.double_conv.%d" % (p, j)]
                assert conv.bias is not None and conv.kernel_size == (3, 3)
                assert conv.out_channels % 64 == 0
        assert blocks["head.outc.conv"].bias is not None
    finally:
        reset_cfg()


def test_decoder_list_is_the_references():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    try:
        Z.cfg_for(SPEC)
        assert segmentron_amd.get_segmentation_model().decoder == ["head"]
        Z.cfg_for(SPEC, "SOLVER.AUX", "True")
        assert segmentron_amd.get_segmentation_model().decoder == ["head", "auxlayer"]
    finally:
        reset_cfg()


def test_resolves_through_the_overlay():
    Z.check_resolves_through_the_overlay(SPEC)


def test_other_norm_layers_are_refused():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC, "MODEL.BN_TYPE", "GN")
    try:
        with pytest.raises(NotImplementedError, match="BN_TYPE"):
            segmentron_amd.get_segmentation_model()
    finally:
        reset_cfg()


@pytest.mark.parametrize("hw", [(15, 64), (64, 15), (8, 8)], ids=lambda v: "%dx%d" % v)
def test_inputs_below_16_are_refused(hw):
    """Four 2x2 pools: the deepest one would see less than a 2 x 2 map.  Raised before any launch."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        with pytest.raises(NotImplementedError, match="smaller than 16"):
            model(torch.zeros(1, 3, *hw))
    finally:
        reset_cfg()


def test_cpu_tensor_raises_before_any_launch():
    """16 x 16 is served (the fixture records the reference's output shape at 70 x 97); a CPU
    tensor is refused by the first op."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    assert tuple(np.load(SPEC.file("eval.npz"))["shape_odd"]) == (1, 19, O.H_ODD, O.W_ODD)
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        with pytest.raises(RuntimeError, match="HIP device tensors"):
            model(torch.zeros(1, 3, 16, 16))
    finally:
        reset_cfg()


def test_skip_pool_refuses_what_it_does_not_serve():
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    with pytest.raises(ValueError, match="2x2 window"):
        F.skip_pool(F.Act(torch.zeros(1, 1, 4, 8)), torch.zeros(1, 1, 4, 8))
    with pytest.raises(ValueError, match="out is"):
        F.skip_pool(F.Act(torch.zeros(1, 4, 4, 8)), torch.zeros(1, 4, 4, 16))
    with pytest.raises(ValueError, match="skip_pool_rows"):
        K.skip_pool_rows(torch.float32, 1, 1, 4, 8)
    with pytest.raises(ValueError, match="skip_pool_rows"):
        K.skip_pool_rows(torch.bfloat16, 1, 4, 4, 12)


def test_skip_pool_rows_geometry():
    """One row per block of 256 / lanes windows (lanes = the channel vectors of a row rounded up to
    a power of two, 32 at the most), 1024 rows at the most."""
    from segmentron_amd import hip_ops as K
    assert K.skip_pool_rows(torch.float32, 1, 2, 2, 4) == 1
    assert K.skip_pool_rows(torch.float32, 1, 3, 3, 8) == 1          # 4 windows, 128 per block
    assert K.skip_pool_rows(torch.bfloat16, 2, 64, 96, 64) == 96     # 3072 windows, 32 per block
    assert K.skip_pool_rows(torch.bfloat16, 2, 512, 512, 64) == 1024
    assert K.skip_pool_rows(torch.float32, 1, 33, 65, 136) == 71     # 561 windows, 8 per block


def test_oracle_reproduces_reference_eval_fixture():
    _, g = Z.check_oracle_eval_fixture(SPEC)
    x = Z.synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0)
    assert tuple(O.evaluate(O.state(Z.fixture_keys(SPEC)[1]), x)[0].shape) == tuple(g["shape_odd"])


def test_oracle_reproduces_reference_train_fixture():
    names, t = Z.check_oracle_train_fixture(SPEC)
    assert len(names) == SPEC.n_grads


def test_oracle_reproduces_reference_small_train_fixture():
    Z.check_oracle_small_train_fixture(SPEC)
