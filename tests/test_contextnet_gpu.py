"""GPU: ContextNet on the HIP path against the reference's fixtures (tests/golden/contextnet_*.npz,
tools/gen_golden_contextnet.py) and the float64 restatement (tests/_contextnet_oracle.py):
evaluation at 2 x 64 x 96 (hi 8 x 12, lo 2 x 3) with the output geometry of 70 x 97, that second
size and 32 x 32 (a 1 x 1 low map: the fusion's resize has scale 0) against the restatement, one
training step at 4 x 112 x 160 (the plain BatchNorm path on the 1/8 maps, the few-sample one from
bottleneck3 on, the fusion's ratios 3/13 and 4/19) with the fusion node forced off and on, the
small fixture, bf16, the fused loss tier at head stride 8, HIP-graph replay == eager launches bit
for bit — tests/_zoo.py's checks."""
import pytest
import torch

import _zoo as Z
from _contextnet_spec import CONTEXTNET as SPEC, fresh_cfg  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

O = SPEC.O


def _maps(B, H, W):
    """-> (hi, x_low, conv_, lo) sizes of a B x H x W input, as the reference produces them."""
    def s2(v, pad):
        return (v + 2 * pad - 3) // 2 + 1
    hi = tuple(s2(s2(s2(v, 0), 1), 1) for v in (H, W))
    xl = (H // 4, W // 4)
    c_ = tuple(s2(v, 0) for v in xl)
    lo = tuple(s2(s2(v, 1), 1) for v in c_)
    return hi, xl, c_, lo


def test_map_sizes_are_the_references():
    assert _maps(1, 64, 96) == ((8, 12), (16, 24), (7, 11), (2, 3))
    assert _maps(1, 70, 97) == ((9, 12), (17, 24), (8, 11), (2, 3))
    assert _maps(1, 32, 32)[0] == (4, 4) and _maps(1, 32, 32)[3] == (1, 1)
    assert _maps(1, 768, 768) == ((96, 96), (192, 192), (95, 95), (24, 24))


def test_eval_fp32_matches_reference_fixture():
    Z.check_eval_fixture(SPEC)


def test_eval_second_size_matches_oracle():
    Z.check_eval_second_size(SPEC)


@pytest.mark.parametrize("side", ["0", "1"], ids=["two_launch", "node"])
def test_eval_with_a_one_pixel_low_map_matches_oracle(side, monkeypatch):
    """32 x 32: the deep branch ends in a 1 x 1 map, every pixel of the upsampled 4 x 4 map copies
    it (scale 0 on both axes)."""
    from segmentron_amd import functional as F
    monkeypatch.setattr(F, "_CTX_UP_DW", side)
    model, sd = Z.build(SPEC, torch.float32, False)
    x = Z.synth.synth_images(1, O.H_ONE, O.W_ONE, seed=0)
    with torch.no_grad():
        out = model(x.cuda())[0].cpu()
    assert Z.rel(out, O.evaluate(sd, x)[0]) < 1e-3


@pytest.mark.parametrize("side", [None, "0", "1"], ids=["routed", "two_launch", "node"])
def test_train_fp32_matches_reference_and_fp64_oracle(side, monkeypatch):
    """The training step as it is routed, with SEG_CTX_UP_DW = 0 and with SEG_CTX_UP_DW = 1."""
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops
    B, H, W = SPEC.train_shape
    hi, xl, c_, lo = _maps(B, H, W)
    assert hi == (14, 20) and lo == (4, 5) and hip_ops.SMALL_BN_ROWS == 1024
    assert B * hi[0] * hi[1] == 1120 > hip_ops.SMALL_BN_ROWS            # the 1/8 maps: plain
    assert B * 7 * 10 == 280 and B * lo[0] * lo[1] == 80                # bottleneck3 onwards: few
    assert (hi[0] - 1) % (lo[0] - 1) != 0 and (hi[1] - 1) % (lo[1] - 1) != 0  # 13 / 3 and 19 / 4
    monkeypatch.setattr(F, "_CTX_UP_DW", side)
    ran = []

    def spy(*a, _f=hip_ops.up_dw, **k):
        ran.append(1)
        return _f(*a, **k)
    monkeypatch.setattr(hip_ops, "up_dw", spy)
    Z.check_train_fp32(SPEC)
    if side is not None:
        assert len(ran) == int(side)


def test_small_train_fp32_matches_reference_fixture():
    """2 x 64 x 96: every BatchNorm sees at most 2 * 31 * 47 rows; the 1/8 maps 192, the few-sample
    path."""
    Z.check_small_train(SPEC, Z.build(SPEC, torch.float32, True)[0])


@pytest.mark.parametrize("side", ["0", "1"], ids=["two_launch", "node"])
def test_one_pixel_low_map_trains(side, monkeypatch):
    """4 x 32 x 32 in training mode: the 1 x 1 low map's gradient is the per-image column sum.
    Inputs of seed 2, the first whose float64 run keeps every ReLU input RELU_MARGIN away from the
    kink at this size (seeds 0 and 1: 4.8e-7 and 7.3e-7)."""
    from segmentron_amd import functional as F
    monkeypatch.setattr(F, "_CTX_UP_DW", side)
    model, sd = Z.build(SPEC, torch.float32, True)
    x = Z.synth.synth_images(4, O.H_ONE, O.W_ONE, seed=2)
    y = Z.synth.synth_targets(4, O.H_ONE, O.W_ONE, seed=2)
    assert O.min_relu_margin(sd, x) >= O.RELU_MARGIN
    loss = Z.mix_loss(SPEC, model(x.cuda()), y.cuda())
    loss.backward()
    l64, _, g64, _ = O.train(sd, x, y, torch.float64)
    _, _, g32, _ = O.train(sd, x, y, torch.float32)
    assert abs(loss.item() - l64) < 1e-3 * l64
    Z.check_gradients(dict(model.named_parameters()), g64, g32, SPEC.unused, SPEC.name,
                      SPEC.key_width)


def test_aux_head_trains_through_the_lazy_view():
    from segmentron_amd import functional as F
    model, _ = Z.build(SPEC, torch.float32, True, overrides=("SOLVER.AUX", "True"),
                       keys=_aux_keys())
    B, H, W = O.FB, O.FH, O.FW
    x = Z.synth.synth_images(B, H, W, seed=3).cuda()
    y = Z.synth.synth_targets(B, H, W, seed=3).cuda()
    outs = model(x)
    assert len(outs) == 2 and all(isinstance(o, F.LogitsView) for o in outs)
    loss = Z.MixSoftmaxCrossEntropyLoss(aux=True).cuda()(outs, y)["loss"]
    loss.backward()
    assert all(o._full is None for o in outs)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def _aux_keys():
    """The schema with SOLVER.AUX True: the fixture's keys and the aux head's."""
    keys = Z.fixture_keys(SPEC)[1]
    return keys + [("auxlayer.0.weight", (32, 128, 3, 3)), ("auxlayer.1.weight", (32,)),
                   ("auxlayer.1.bias", (32,)), ("auxlayer.1.running_mean", (32,)),
                   ("auxlayer.1.running_var", (32,)), ("auxlayer.1.num_batches_tracked", ()),
                   ("auxlayer.4.weight", (19, 32, 1, 1)), ("auxlayer.4.bias", (19,))]


def test_train_bf16_is_finite_and_as_close_as_autocast():
    Z.check_train_bf16(SPEC)


def test_reference_criterion_takes_the_fused_tier():
    """Head stride 8: 576 x 584 -> 72 x 73 logits, within the fused loss's 8.1 tier."""
    Z.check_fused_tier(SPEC)


def test_graph_mode_equals_eager_bit_for_bit():
    Z.check_graph_equals_eager(SPEC)
