"""CPU: ContextNet (segmentron/models/contextnet.py) served by the registry — the reference's config
and state_dict schema with and without the aux head (tests/golden/contextnet_state_keys.json,
tools/gen_golden_contextnet.py), the drop-in overlay, the missing `decoder` attribute, the refusals
(BN_TYPE, a CPU tensor), the host-side geometry query and argument checks of the resize + depthwise
node, and the test-side restatement (tests/_contextnet_oracle.py) against the reference's own
runs."""
import numpy as np
import pytest
import torch

import _zoo as Z
from _contextnet_spec import CONTEXTNET as SPEC, N_KEYS_AUX, N_PARAMS_AUX

O = SPEC.O


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = Z.cfg_for(SPEC)
        assert cfg.MODEL.MODEL_NAME == "ContextNet"
    finally:
        reset_cfg()


def test_resolves_through_the_overlay():
    Z.check_resolves_through_the_overlay(SPEC)


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = Z.fixture_keys(SPEC)
    assert len(keys) == SPEC.n_keys and ref["n_params"] == SPEC.n_params
    assert ref["n_keys_aux"] == N_KEYS_AUX and ref["n_params_aux"] == N_PARAMS_AUX
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.contextnet"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert model.encoder is None and not hasattr(model, "decoder")
        model.load_state_dict(O.state(keys), strict=True)
        from segmentron_amd.models import contextnet as M
        blocks = dict(model.named_modules())
        assert isinstance(blocks["classifier"], M.Classifer)
        # the quirks: unpadded stride-2 stems, a real depthwise 3x3 in the fusion, biased 1x1s in
        # front of a BatchNorm, the per-element dropout
        for p in ("spatial_detail.conv.conv.0", "context_feature_extractor.conv_.conv.0"):
            assert blocks[p].padding == (0, 0) and blocks[p].stride == (2, 2)
        dw = blocks["feature_fusion.dwconv.conv.0"]
        assert dw.kernel_size == (3, 3) and dw.groups == 128 and dw.bias is None
        assert blocks["feature_fusion.conv_lower_res.0"].bias is not None
        assert blocks["feature_fusion.conv_higher_res.0"].bias is not None
        assert type(blocks["classifier.conv.0"]) is torch.nn.Dropout
        n_blocks = [len(blocks["context_feature_extractor.bottleneck%d" % i]) for i in range(1, 7)]
        assert n_blocks == [1, 1, 3, 3, 2, 2]
    finally:
        reset_cfg()


def test_aux_head_schema_counts():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC, "SOLVER.AUX", "True")
    try:
        model = segmentron_amd.get_segmentation_model()
        assert len(model.state_dict()) == N_KEYS_AUX
        assert sum(p.numel() for p in model.parameters()) == N_PARAMS_AUX
        assert type(model.auxlayer[3]) is torch.nn.Dropout and not hasattr(model, "decoder")
    finally:
        reset_cfg()


def test_other_norm_layers_are_refused():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    Z.cfg_for(SPEC, "MODEL.BN_TYPE", "GN")
    try:
        with pytest.raises(NotImplementedError, match="BN_TYPE"):
            segmentron_amd.get_segmentation_model()
    finally:
        reset_cfg()


def test_cpu_tensor_raises_before_any_launch():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    assert tuple(np.load(SPEC.file("eval.npz"))["shape_odd"]) == (1, 19, O.H_ODD, O.W_ODD)
    Z.cfg_for(SPEC)
    try:
        model = segmentron_amd.get_segmentation_model()
        with pytest.raises(RuntimeError, match="HIP device tensors"):
            model(torch.zeros(1, 3, 32, 32))
    finally:
        reset_cfg()


def test_up_dw_rows_geometry():
    """One row per (image, row strip, column block): lanes = the channel quads of a pixel rounded up
    to a power of two, 16 at the most; 256 / lanes column lanes of which two are halo; strips of at
    least 4 rows, about 1024 blocks.  The two kinds share the geometry."""
    from segmentron_amd import hip_ops as K
    f32, bf16 = torch.float32, torch.bfloat16
    assert K.up_dw_rows(f32, 2, 4, 4, 8) == 2                # 126 columns per block, one strip
    assert K.up_dw_rows(f32, 1, 1, 7, 8) == 1
    assert K.up_dw_rows(bf16, 1, 14, 20, 128) == 2 * 4       # 14 columns per block, 4 strips
    assert K.up_dw_rows(bf16, 4, 96, 96, 128) == 4 * 7 * 16  # 19 strips asked: 6 rows each, 16
    assert K.up_dw_rows(f32, 2, 37, 67, 136) == 2 * 5 * 10
    for args in ((bf16, 4, 96, 96, 128), (f32, 2, 9, 12, 24)):
        assert K.up_dw_rows(*args, kind=0) == K.up_dw_rows(*args, kind=1)


def test_up_dw_refuses_what_it_does_not_serve():
    """Raised on the host, before any launch and without a device."""
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    with pytest.raises(ValueError, match="up_dw_rows"):
        K.up_dw_rows(torch.bfloat16, 1, 4, 4, 12)            # no multiple of 8
    with pytest.raises(ValueError, match="up_dw_rows"):
        K.up_dw_rows(torch.float32, 1, 0, 4, 8)
    with pytest.raises(ValueError, match="up_dw_rows"):
        K.up_dw_rows(torch.float32, 1, 4, 4, 8, kind=2)
    with pytest.raises(ValueError, match="dtype"):
        K.up_dw_rows(torch.float16, 1, 4, 4, 8)
    w = torch.zeros(9, 8)
    with pytest.raises(ValueError, match="dtype"):
        K.up_dw(torch.zeros(1, 2, 2, 8, dtype=torch.float16), (4, 4), w)
    with pytest.raises(ValueError, match="multiple of 4"):
        K.up_dw(torch.zeros(1, 2, 2, 6), (4, 4), torch.zeros(9, 6))
    with pytest.raises(ValueError, match="not contiguous"):
        K.up_dw(torch.zeros(1, 2, 8, 2).transpose(2, 3), (4, 4), w)
    with pytest.raises(ValueError, match="4-d"):
        K.up_dw(torch.zeros(2, 2, 8), (4, 4), w)
    with pytest.raises(ValueError, match="4-d"):
        K.up_dw_bwd(torch.zeros(4, 4, 8), torch.zeros(1, 2, 2, 8), w)
    conv = torch.nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False)
    bn = torch.nn.BatchNorm2d(8)
    for bad in (torch.nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=True),
                torch.nn.Conv2d(8, 8, 3, padding=2, dilation=2, groups=8, bias=False),
                torch.nn.Conv2d(8, 8, 3, stride=2, padding=1, groups=8, bias=False),
                torch.nn.Conv2d(8, 8, 3, padding=1, bias=False),
                torch.nn.Conv2d(16, 16, 3, padding=1, groups=16, bias=False)):
        with pytest.raises(NotImplementedError, match="up_dwconv_bn"):
            F.up_dwconv_bn(F.Act(torch.zeros(1, 2, 2, 8)), (4, 4), bad, bn)
    with pytest.raises(ValueError, match="resized to"):
        F.up_dwconv_bn(F.Act(torch.zeros(1, 2, 2, 8)), (0, 4), conv, bn)
    with pytest.raises(NotImplementedError, match="GroupNorm"):
        F.up_dwconv_bn(F.Act(torch.zeros(1, 2, 2, 8)), (4, 4), conv, torch.nn.GroupNorm(2, 8))


def test_up_dw_routing_switch():
    """SEG_CTX_UP_DW forces a side (read when the package is imported); without it the node runs
    only in the classes the bench measured it faster in."""
    from test_dropin import _run
    for env, want in (("0", "False False"), ("1", "True True")):
        out = _run("""
            import torch
            from segmentron_amd import functional as F
            print('ROUTED', F.up_dw_routed(torch.bfloat16, 128, 36864),
                  F.up_dw_routed(torch.float32, 24, 192))
        """, env_extra={"SEG_CTX_UP_DW": env})
        assert "ROUTED " + want in out


def test_oracle_reproduces_reference_eval_fixture():
    _, g = Z.check_oracle_eval_fixture(SPEC)
    sd = O.state(Z.fixture_keys(SPEC)[1])
    x = Z.synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0)
    assert tuple(O.evaluate(sd, x)[0].shape) == tuple(g["shape_odd"])
    one = O.evaluate(sd, Z.synth.synth_images(1, O.H_ONE, O.W_ONE, seed=0))[0]
    assert tuple(one.shape) == (1, 19, O.H_ONE, O.W_ONE) and torch.isfinite(one).all()


def test_oracle_reproduces_reference_train_fixture():
    names, t = Z.check_oracle_train_fixture(SPEC)
    assert len(names) == SPEC.n_grads
    # the two fusion biases sit in front of a training-mode BatchNorm: zero in exact arithmetic
    whole = sum(float(t["gnorm::" + k]) ** 2 for k in names) ** 0.5
    for k in ("feature_fusion.conv_lower_res.0.bias", "feature_fusion.conv_higher_res.0.bias"):
        assert float(t["gnorm::" + k]) < 1e-6 * whole


def test_oracle_reproduces_reference_small_train_fixture():
    Z.check_oracle_small_train_fixture(SPEC)
