"""CPU: BiSeNet (segmentron/models/bisenet.py) served by the registry — the reference's
state_dict schema (tests/golden/bisenet_state_keys.json, tools/gen_golden_bisenet.py) with and
without the aux heads, the drop-in overlay, and the test-side restatement
(tests/_bisenet_oracle.py) against the reference's own runs."""
import numpy as np
import pytest
import torch

import _zoo as Z
from _zoo import BISENET as SPEC
from oracle import synth

O = SPEC.O


@pytest.mark.parametrize("aux", [True, False])
def test_state_dict_schema_equals_reference(aux):
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = Z.fixture_keys(SPEC)
    assert len(keys) == SPEC.n_keys and ref["n_params"] == SPEC.n_params  # 230 / 13910113
    Z.cfg_for(SPEC, "SOLVER.AUX", str(aux))
    try:
        model = segmentron_amd.get_segmentation_model()
        if not aux:  # the fixture is the AUX True model: without the two aux heads
            keys = [(k, s) for k, s in keys if not k.startswith("auxlayer")]
            n_aux = sum(int(np.prod(s)) for k, s in Z.fixture_keys(SPEC)[1]
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
    Z.check_resolves_through_the_overlay(SPEC)


def test_oracle_reproduces_reference_eval_fixture():
    Z.check_oracle_eval_fixture(SPEC)


def test_oracle_reproduces_reference_train_fixture():
    Z.check_oracle_train_fixture(SPEC)  # (the three logits at every 2nd / 4th / 4th pixel)


def test_oracle_reproduces_reference_os32_fixture():
    _, keys = Z.fixture_keys(SPEC)
    sd = O.state([(k, s) for k, s in keys if not k.startswith("auxlayer")])
    x = synth.synth_images(O.B_TRAIN, O.H32, O.W32, seed=0)
    y = synth.synth_targets(O.B_TRAIN, O.H32, O.W32, seed=0)
    loss, outs, _, _ = O.train(sd, x, y, output_stride=32, aux=False)
    t = np.load(SPEC.file("os32_train.npz"))
    assert abs(loss - float(t["loss"])) < 1e-5
    assert torch.allclose(outs[0][..., ::2, ::2], torch.from_numpy(t["logits0"]), rtol=1e-4,
                          atol=1e-4)
