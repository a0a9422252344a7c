"""CPU: DUNet (segmentron/models/dunet.py) served by the registry — the reference's state_dict
schema and decoder list (tests/golden/dunet_state_keys.json, tools/gen_golden_dunet.py) with and
without the aux head, the drop-in overlay, and the test-side restatement (tests/_dunet_oracle.py)
against the reference's own runs."""
import numpy as np
import pytest
import torch

import _zoo as Z
from _zoo import DUNET as SPEC
from oracle import synth

O = SPEC.O
AUX_PREFIXES = ("auxlayer.", "aux_dupsample.")


@pytest.mark.parametrize("aux", [True, False])
def test_state_dict_schema_equals_reference(aux):
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    ref, keys = Z.fixture_keys(SPEC)
    assert len(keys) == SPEC.n_keys and ref["n_params"] == SPEC.n_params  # 354 / 34209768
    assert ref["decoder"] == ["dupsample", "head", "auxlayer", "aux_dupsample"]
    Z.cfg_for(SPEC, "SOLVER.AUX", str(aux))
    try:
        model = segmentron_amd.get_segmentation_model()
        assert type(model).__module__ == "segmentron_amd.models.dunet"
        n_params, decoder = ref["n_params"], list(ref["decoder"])
        if not aux:  # the fixture is the AUX True model: without the aux head and its DUpsampling
            n_params -= sum(int(np.prod(s)) for k, s in keys
                            if k.startswith(AUX_PREFIXES) and "running_" not in k
                            and not k.endswith("num_batches_tracked"))
            keys = [(k, s) for k, s in keys if not k.startswith(AUX_PREFIXES)]
            decoder = [d for d in decoder if not d.startswith("aux")]
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
        assert sum(p.numel() for p in model.parameters()) == n_params
        assert model.decoder == decoder
        assert tuple(model.dupsample.conv_w.weight.shape) == (8 * 8 * 19, 256, 1, 1)
        assert model.dupsample.conv_w.bias is None
    finally:
        reset_cfg()


def test_resolves_through_the_overlay():
    Z.check_resolves_through_the_overlay(SPEC)


def test_oracle_dupsample_is_the_reference_rearrangement():
    """The one-permute form against the module's three permute / contiguous / view rounds
    (dunet.py:100-117), restated on a small tensor."""
    s, k, n, h, w = 4, 3, 2, 3, 5
    x = torch.arange(n * s * s * k * h * w, dtype=torch.float32).view(n, s * s * k, h, w)
    c = s * s * k
    r = x.permute(0, 3, 2, 1).contiguous().view(n, w, h * s, c // s)
    r = r.permute(0, 2, 1, 3).contiguous().view(n, h * s, w * s, c // (s * s)).permute(0, 3, 1, 2)
    assert torch.equal(O.dupsample(x, s), r)


def test_oracle_reproduces_reference_eval_fixture():
    sd, g = Z.check_oracle_eval_fixture(SPEC)
    odd = O.evaluate(sd, synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
    assert tuple(odd[0].shape) == tuple(g["shape_odd"]) == (1, 19, 72, 104)


def test_oracle_reproduces_reference_train_fixture():
    Z.check_oracle_train_fixture(SPEC)  # (both logits at every 2nd pixel)


def test_oracle_reproduces_reference_output_stride_16_fixture():
    """FeatureFused's resize of c2 is real at OUTPUT_STRIDE 16; the output is 8 x c4."""
    _, keys = Z.fixture_keys(SPEC)
    outs = O.evaluate(O.state(keys), synth.synth_images(O.B, O.H, O.W, seed=0), output_stride=16)
    g = np.load(SPEC.file("os16_eval.npz"))
    assert tuple(g["logits0"].shape) == (O.B, 19, O.H // 2, O.W // 2)
    for i in range(2):
        assert torch.allclose(outs[i], torch.from_numpy(g["logits%d" % i]), rtol=1e-4, atol=1e-4)


def test_dupsample_cross_entropy_operator_has_a_fake_implementation():
    """torch.ops.segmentron_hip.dupsample_cross_entropy: schema and shape / dtype inference through
    FakeTensorMode — no device is touched."""
    import segmentron_amd  # noqa: F401  registers the operators
    from torch._subclasses.fake_tensor import FakeTensorMode
    ns = torch.ops.segmentron_hip
    assert "nclass" in str(ns.dupsample_cross_entropy.default._schema)
    with FakeTensorMode():
        lo = torch.empty(4, 96, 96, 1216, dtype=torch.bfloat16, device="cuda")
        tgt = torch.empty(4, 768, 768, dtype=torch.int64, device="cuda")
        out = ns.dupsample_cross_entropy(lo, tgt, 8, 19, -1)
        assert tuple(out.shape) == (2,) and out.dtype == torch.float32
        d = ns.dupsample_cross_entropy_backward(lo, tgt, out, out[:1], 8, 19, -1)
        assert tuple(d.shape) == tuple(lo.shape) and d.dtype == torch.bfloat16
