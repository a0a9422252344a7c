"""CPU: BiSeNet (segmentron/models/bisenet.py) served by the registry — the reference's
state_dict schema (tests/golden/bisenet_state_keys.json, tools/gen_golden_bisenet.py) with and
without the aux heads, the drop-in overlay, and the test-side restatement
(tests/_bisenet_oracle.py) against the reference's own runs."""
import json
import os

import numpy as np
import pytest
import torch

import _bisenet_oracle as O
from conftest import GOLDEN
from oracle import synth
from test_dropin import _run

YAML = os.path.join(GOLDEN, "cityscapes_bisenet.yaml")


def bisenet_cfg(*overrides):
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(YAML)
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False"] + list(overrides))
    cfg.PHASE = "test"
    cfg.check_and_freeze()
    return cfg


def fixture_keys():
    ref = json.load(open(os.path.join(GOLDEN, "bisenet_state_keys.json")))
    return ref, [(k, tuple(s)) for k, s in ref["keys"]]


@pytest.mark.parametrize("aux", [True, False])
def test_state_dict_schema_equals_reference(aux):
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = fixture_keys()
    assert len(keys) == 230 and ref["n_params"] == 13910113
    bisenet_cfg("SOLVER.AUX", str(aux))
    try:
        model = segmentron_amd.get_segmentation_model()
        if not aux:  # the fixture is the AUX True model: without the two aux heads
            keys = [(k, s) for k, s in keys if not k.startswith("auxlayer")]
            n_aux = sum(int(np.prod(s)) for k, s in fixture_keys()[1]
                        if k.startswith("auxlayer") and "running_" not in k
                        and not k.endswith("num_batches_tracked"))
            ref["n_params"] -= n_aux
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
        assert model.decoder == ["spatial_path", "context_path", "ffm", "head"] + \
            (["auxlayer1", "auxlayer2"] if aux else [])
        # built WITHOUT norm_layer in the reference: plain BatchNorm2d, per-element Dropout
        assert type(model.ffm.conv1x1.bn) is torch.nn.BatchNorm2d
        assert type(model.head.block[1]) is torch.nn.Dropout
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
        assert 'BiSeNet' in MODEL_REGISTRY.get_list()
        cfg.update_from_file(%r)
        cfg.update_from_list(['TRAIN.BACKBONE_PRETRAINED', 'False'])
        cfg.PHASE = 'test'
        cfg.check_and_freeze()
        model = get_segmentation_model()
        assert type(model).__module__ == 'segmentron_amd.models.bisenet', type(model).__module__
        print('BISENET_OK')
    """ % YAML, env_extra={"SEGMENTRON_REFERENCE_ROOT": ""})
    assert "BISENET_OK" in out


def test_oracle_reproduces_reference_eval_fixture():
    _, keys = fixture_keys()
    sd = O.state(keys)
    outs = O.evaluate(sd, synth.synth_images(O.B_EVAL, O.H, O.W, seed=0))
    g = np.load(os.path.join(GOLDEN, "bisenet_eval.npz"))
    assert torch.allclose(outs[0], torch.from_numpy(g["logits0"]), rtol=1e-4, atol=1e-4)


def test_oracle_reproduces_reference_train_fixture():
    _, keys = fixture_keys()
    sd = O.state(keys)
    x = synth.synth_images(O.B_TRAIN, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B_TRAIN, O.H, O.W, seed=0)
    loss, outs, grads, after = O.train(sd, x, y)
    t = np.load(os.path.join(GOLDEN, "bisenet_train.npz"))
    assert abs(loss - float(t["loss"])) < 1e-5
    for i, step in enumerate((2, 4, 4)):
        assert torch.allclose(outs[i][..., ::step, ::step], torch.from_numpy(t["logits%d" % i]),
                              rtol=1e-4, atol=1e-4)
    names = [k[len("gnorm::"):] for k in t.files if k.startswith("gnorm::")]
    assert len(names) > 60 and set(names) == set(grads)
    for k in names:
        n = float(t["gnorm::" + k])
        assert abs(float(grads[k].double().norm()) - n) <= 1e-3 * max(n, 1e-6) + 1e-9, k
    stats = [k[len("stat::"):] for k in t.files if k.startswith("stat::")]
    assert stats
    for k in stats:
        ref = torch.from_numpy(t["stat::" + k])
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(ref), k
        else:
            assert (after[k] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-6, k


def test_oracle_reproduces_reference_os32_fixture():
    _, keys = fixture_keys()
    sd = O.state([(k, s) for k, s in keys if not k.startswith("auxlayer")])
    x = synth.synth_images(O.B_TRAIN, O.H32, O.W32, seed=0)
    y = synth.synth_targets(O.B_TRAIN, O.H32, O.W32, seed=0)
    loss, outs, _, _ = O.train(sd, x, y, output_stride=32, aux=False)
    t = np.load(os.path.join(GOLDEN, "bisenet_os32_train.npz"))
    assert abs(loss - float(t["loss"])) < 1e-5
    assert torch.allclose(outs[0][..., ::2, ::2], torch.from_numpy(t["logits0"]), rtol=1e-4,
                          atol=1e-4)
