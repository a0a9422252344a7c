"""CPU: ESPNetV2 on EESPNet (segmentron/models/espnetv2.py) served by the registry — the
reference's state_dict schema and `exclusive` list (tests/golden/espnetv2_state_keys.json,
tools/gen_golden_espnetv2.py), the drop-in overlay, conv_bn's refusal of grouped 3x3, and the
test-side restatement (tests/_espnetv2_oracle.py) against the reference's own runs."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _espnetv2_oracle as O
from conftest import GOLDEN
from oracle import synth
from test_dropin import _run

YAML = os.path.join(GOLDEN, "cityscapes_espnetv2.yaml")


def espnetv2_cfg(*overrides):
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(YAML)
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False"] + list(overrides))
    cfg.PHASE = "test"
    cfg.check_and_freeze()
    return cfg


def fixture_keys():
    ref = json.load(open(os.path.join(GOLDEN, "espnetv2_state_keys.json")))
    return ref, [(k, tuple(s)) for k, s in ref["keys"]]


def test_yaml_loads_through_cfg():
    from segmentron_amd.config import reset_cfg
    try:
        cfg = espnetv2_cfg()
        assert cfg.MODEL.MODEL_NAME == "ESPNetV2" and cfg.MODEL.BACKBONE == "eespnet"
        assert tuple(cfg.TRAIN.CROP_SIZE) == (512, 1024) and cfg.TRAIN.BATCH_SIZE == 4
        assert cfg.SOLVER.AUX is False
    finally:
        reset_cfg()


def test_state_dict_schema_equals_reference():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = fixture_keys()
    assert len(keys) == 640 and ref["n_params"] == 2163324
    assert ref["exclusive"] == ["proj_L4_C", "pspMod", "project_l3", "act_l3", "project_l2",
                                "project_l1"]
    espnetv2_cfg()
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.espnetv2"
        assert type(model.encoder).__module__ == "segmentron_amd.models.backbones.eespnet"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert sum(1 for _ in model.parameters()) == 397
        assert model.exclusive == ref["exclusive"] and not hasattr(model, "decoder")
        assert model.aux is False
        model.load_state_dict(O.state(keys), strict=True)
        # the geometry the restatement assumes: four branches, these dilations, groups = 4
        from segmentron_amd.modules import EESP
        units = {n: m for n, m in model.named_modules() if isinstance(m, EESP)}
        reached = {n: m for n, m in units.items() if not O.unused(n + ".")}
        assert len(reached) == 14 and len(units) == 14 + 1 + 7
        for name, m in reached.items():
            assert [c.dilation[0] for c in m.spp_dw] == O.dilations(O._r_lim(name)), name
            assert all(c.padding == c.dilation for c in m.spp_dw)
            assert m.proj_1x1.conv.groups == m.conv_1x1_exp.conv.groups == O.K
        assert O.dilations(9) == [1, 2, 3, 4] and O.dilations(7) == [1, 1, 2, 3]
        assert tuple(model.pspMod[0].proj_1x1.conv.weight.shape) == (32, 64, 1, 1)
        assert tuple(model.encoder.level2_0.eesp.proj_1x1.conv.weight.shape) == (8, 8, 1, 1)
    finally:
        reset_cfg()


def test_resolves_through_the_overlay():
    out = _run("""
        import sys
        sys.path = [p for p in sys.path if 'reference' not in p]
        sys.argv = ['x']
        import segmentron, segmentron_amd
        from segmentron.config import cfg
        from segmentron.models.model_zoo import get_segmentation_model, MODEL_REGISTRY
        assert 'ESPNetV2' in MODEL_REGISTRY.get_list()
        cfg.update_from_file(%r)
        cfg.update_from_list(['TRAIN.BACKBONE_PRETRAINED', 'False'])
        cfg.PHASE = 'test'
        cfg.check_and_freeze()
        model = get_segmentation_model()
        assert type(model).__module__ == 'segmentron_amd.models.espnetv2', type(model).__module__
        print('ESPNETV2_OK')
    """ % YAML, env_extra={"SEGMENTRON_REFERENCE_ROOT": ""})
    assert "ESPNETV2_OK" in out


@pytest.mark.parametrize("kw", [dict(kernel_size=3, padding=1, groups=4),
                                dict(kernel_size=1, stride=2, groups=4),
                                dict(kernel_size=1, padding=1, groups=4),
                                dict(kernel_size=1, groups=4, bias=True)])
def test_conv_bn_refuses_other_grouped_geometry(kw):
    """Grouped convolutions are served as 1x1 / stride 1 / unpadded / bias-free only (the
    block-diagonal packing).  (Raised before any tensor is touched: runs on the CPU.)"""
    from segmentron_amd import functional as F
    kw.setdefault("bias", False)
    conv = nn.Conv2d(32, 32, **kw)
    with pytest.raises(NotImplementedError, match="groups=4"):
        F.conv_bn(F.Act(torch.zeros(1, 8, 8, 32)), conv)


def test_block_diagonal_packing_round_trips():
    """The dense weight of a grouped 1x1 computes the grouped convolution, and the diagonal blocks
    of a dense gradient come back in the parameter's layout."""
    from segmentron_amd import functional as F
    g = torch.Generator().manual_seed(0)
    for C, O_ in ((32, 8), (256, 32), (128, 128)):
        w = torch.randn((O_, C // 4, 1, 1), generator=g, dtype=torch.float64)
        x = torch.randn((2, C, 5, 7), generator=g, dtype=torch.float64)
        dense = F.block_diag_weight(w, 4)
        assert tuple(dense.shape) == (O_, C, 1, 1)
        assert torch.allclose(torch.nn.functional.conv2d(x, dense),
                              torch.nn.functional.conv2d(x, w, groups=4), rtol=0, atol=1e-12)
        assert int((dense != 0).sum()) == w.numel()
        assert torch.equal(F.block_diag_grad(dense.reshape(O_, C), 4), w)


def test_pyramid_contract_and_routing():
    from segmentron_amd import functional as F
    assert F.eesp_pyramid_in_contract(32, (1, 2, 3, 4), 1)
    assert F.eesp_pyramid_in_contract(64, (1, 1, 2, 3), 2)
    for n, dils, s in ((12, (1, 2, 3, 4), 1), (8, (1, 2, 3, 5), 1), (8, (1, 3, 2, 4), 1),
                       (8, (1, 2, 3), 1), (8, (1, 2, 3, 4), 3), (0, (1, 2, 3, 4), 1)):
        assert not F.eesp_pyramid_in_contract(n, dils, s)
        assert not F.eesp_pyramid_routed(torch.bfloat16, n, dils, s)


def test_oracle_reproduces_reference_eval_fixture():
    _, keys = fixture_keys()
    sd = O.state(keys)
    g = np.load(os.path.join(GOLDEN, "espnetv2_eval.npz"))
    outs = O.evaluate(sd, synth.synth_images(O.B, O.H, O.W, seed=0))
    assert len(outs) == int(g["n_outputs"]) == 1
    assert torch.allclose(outs[0][..., ::2, ::2], torch.from_numpy(g["logits0"]), rtol=1e-4,
                          atol=1e-4)
    second = O.evaluate(sd, synth.synth_images(1, O.H2, O.W2, seed=0))
    assert tuple(second[0].shape) == (1, 19, O.H2, O.W2)
    assert torch.allclose(second[0][..., ::2, ::2], torch.from_numpy(g["logits0_second"]),
                          rtol=1e-4, atol=1e-4)


def _check_train(t, logits_ref, loss, outs, grads, after):
    assert abs(loss - float(t["loss"])) < 1e-5
    assert torch.allclose(outs[0][..., ::2, ::2], logits_ref, rtol=1e-4, atol=1e-4)
    names = [k[len("gnorm::"):] for k in t.files if k.startswith("gnorm::")]
    assert set(names) == set(grads)
    for k in names:
        n = float(t["gnorm::" + k])
        assert abs(float(grads[k].double().norm()) - n) <= 1e-3 * max(n, 1e-6) + 1e-9, k
    stats = [k[len("stat::"):] for k in t.files if k.startswith("stat::")]
    assert stats
    for k in stats:
        ref = torch.from_numpy(t["stat::" + k])
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(ref) == (0 if O.unused(k) else 1), k
        else:
            assert (after[k] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-6, k
    return names


def train_fixture_logits():
    return torch.cat([torch.from_numpy(np.load(os.path.join(GOLDEN, f))["logits0"])
                      for f in ("espnetv2_train_logits_a.npz", "espnetv2_train_logits_b.npz")])


def test_oracle_reproduces_reference_train_fixture():
    ref, keys = fixture_keys()
    sd = O.state(keys)
    x = synth.synth_images(O.TB, O.TH, O.TW, seed=O.TRAIN_SEED)
    y = synth.synth_targets(O.TB, O.TH, O.TW, seed=O.TRAIN_SEED)
    t = np.load(os.path.join(GOLDEN, "espnetv2_train.npz"))
    assert int(t["seed"]) == O.TRAIN_SEED
    names = _check_train(t, train_fixture_logits(), *O.train(sd, x, y))
    # the parameters with a gradient are the reference's: level5*, fc (and the module_act a
    # DownSampler's EESP unit returns before) have none
    assert not any(k.startswith(O.UNUSED) for k in names)
    assert not any(O.unused(k) for k in names)
    assert len(names) == 256
    # what the reference's own arithmetic costs on this fixture: the yardsticks of the GPU bars
    assert 0 < float(t["cpu::grad_global"]) <= 1e-4
    assert 0 < float(t["cpu::bf16_loss_rel"]) < 1e-2 and 0.99 < float(t["cpu::bf16_grad_cos"]) < 1


def test_oracle_reproduces_reference_small_train_fixture():
    _, keys = fixture_keys()
    sd = O.state(keys)
    x = synth.synth_images(O.B, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B, O.H, O.W, seed=0)
    t = np.load(os.path.join(GOLDEN, "espnetv2_small_train.npz"))
    _check_train(t, torch.from_numpy(t["logits0"]), *O.train(sd, x, y))


def test_parameters_with_a_gradient_are_the_references():
    """The model's own parameter names split the way the reference's gradients do."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    t = np.load(os.path.join(GOLDEN, "espnetv2_train.npz"))
    with_grad = {k[len("gnorm::"):] for k in t.files if k.startswith("gnorm::")}
    espnetv2_cfg()
    try:
        model = segmentron_amd.get_segmentation_model()
        names = {k for k, _ in model.named_parameters()}
        assert with_grad <= names
        assert {k for k in names if not O.unused(k)} == with_grad
        assert any(k.startswith("encoder.level5.") for k in names - with_grad)
        assert "encoder.fc.weight" in names - with_grad
    finally:
        reset_cfg()
