"""GPU: DUNet on the HIP path against the reference's fixtures (tests/golden/dunet_*.npz,
tools/gen_golden_dunet.py) and the float64 restatement (tests/_dunet_oracle.py): evaluation, one
training step, bf16, the fused DUpsampling loss behind the reference's criterion, and HIP-graph
replay == eager launches bit for bit."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _dunet_oracle as O
from conftest import GOLDEN
from oracle import synth

pytestmark = pytest.mark.gpu

YAML = os.path.join(GOLDEN, "cityscapes_dunet.yaml")


def _keys():
    keys = json.load(open(os.path.join(GOLDEN, "dunet_state_keys.json")))["keys"]
    return [(k, tuple(s)) for k, s in keys]


def _build(dtype, train, phase="test", output_stride=8):
    import segmentron_amd
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(YAML)
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False", "SOLVER.AUX", "True",
                          "SOLVER.AUX_WEIGHT", str(O.AUX_WEIGHT), "MODEL.OUTPUT_STRIDE",
                          str(output_stride)])
    cfg.PHASE = phase
    cfg.check_and_freeze()
    segmentron_amd.set_compute_dtype(dtype)
    model = segmentron_amd.get_segmentation_model()
    sd = O.state(_keys())
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train(train)
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    return model, sd


@pytest.fixture(autouse=True)
def _fresh_cfg():
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    yield
    segmentron_amd.set_compute_dtype(torch.float32)
    reset_cfg()


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def _mix_loss(outs, y):
    loss = torch.nn.functional.cross_entropy(outs[0], y, ignore_index=-1)
    for o in outs[1:]:
        loss = loss + O.AUX_WEIGHT * torch.nn.functional.cross_entropy(o, y, ignore_index=-1)
    return loss


def test_eval_fp32_matches_reference_fixture():
    model, _ = _build(torch.float32, False)
    g = np.load(os.path.join(GOLDEN, "dunet_eval.npz"))
    with torch.no_grad():
        outs = model(synth.synth_images(O.B, O.H, O.W, seed=0).cuda())
        odd = model(synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0).cuda())
    # (the reference returns the aux output in evaluation mode too)
    assert len(outs) == int(g["n_outputs"]) and all(isinstance(o, torch.Tensor) for o in outs)
    assert all(o.dtype == torch.float32 and tuple(o.shape) == (O.B, 19, O.H, O.W) for o in outs)
    assert tuple(odd[0].shape) == tuple(g["shape_odd"])
    ref = torch.from_numpy(g["logits0"])
    logits = outs[0].cpu()[..., ::2, ::2]
    rel = _rel(logits, ref)
    bad = logits.argmax(1) != ref.argmax(1)
    top2 = ref.topk(2, dim=1).values
    gap = (top2[:, 0] - top2[:, 1])[bad]
    print("dunet eval fp32 max-rel %.3e; argmax mismatches %d of %d (largest reference top-2 gap "
          "among them %.2e)" % (rel, int(bad.sum()), bad.numel(),
                                gap.max().item() if gap.numel() else 0.0))
    assert rel < 1e-3
    # masks identical except at genuine ties of the reference itself (top-2 gap below the 1e-3 bar)
    assert gap.numel() == 0 or gap.max().item() < 1e-3 * ref.abs().max().item()


def test_eval_fp32_output_stride_16_matches_reference_fixture():
    """FeatureFused shrinks c2 to c4's size here (align_corners=True); the output is 8 x c4, half
    the input's size, as in the reference."""
    model, _ = _build(torch.float32, False, output_stride=16)
    g = np.load(os.path.join(GOLDEN, "dunet_os16_eval.npz"))
    with torch.no_grad():
        outs = model(synth.synth_images(O.B, O.H, O.W, seed=0).cuda())
    assert len(outs) == 2
    rels = [_rel(outs[i].cpu(), torch.from_numpy(g["logits%d" % i])) for i in range(2)]
    print("dunet OS 16 eval fp32 max-rel %s" % ["%.2e" % r for r in rels])
    assert all(tuple(o.shape) == (O.B, 19, O.H // 2, O.W // 2) for o in outs)
    assert max(rels) < 1e-3


# the float64 / float32 CPU runs of the oracle on the training fixture, computed once
_ORACLE = {}


def _oracle_runs():
    if not _ORACLE:
        sd = O.state(_keys())
        x = synth.synth_images(O.B, O.H, O.W, seed=0)
        y = synth.synth_targets(O.B, O.H, O.W, seed=0)
        _ORACLE["f64"] = O.train(sd, x, y, torch.float64)
        _ORACLE["f32"] = O.train(sd, x, y, torch.float32)
        _ORACLE["xy"] = (x, y)
    return _ORACLE


def test_train_fp32_matches_reference_and_fp64_oracle():
    from segmentron_amd import functional as HF
    model, sd = _build(torch.float32, True)
    runs = _oracle_runs()
    x, y = runs["xy"]
    outs = model(x.cuda())
    assert len(outs) == 2 and all(isinstance(o, HF.DUpLogitsView) for o in outs)
    loss = _mix_loss(outs, y.cuda())
    assert all(o._full is None for o in outs)
    loss.backward()
    t = np.load(os.path.join(GOLDEN, "dunet_train.npz"))
    ref_loss = float(t["loss"])
    rels = [_rel(outs[i].materialize().detach().cpu()[..., ::2, ::2],
                 torch.from_numpy(t["logits%d" % i])) for i in range(2)]
    print("dunet train fp32: loss %.6f (fixture %.6f), logits max-rel %s"
          % (loss.item(), ref_loss, ["%.2e" % r for r in rels]))
    assert abs(loss.item() - ref_loss) < 1e-3 * ref_loss
    assert max(rels) < 1e-3
    # running statistics after the step against the reference's, every counter against the oracle's
    msd = model.state_dict()
    _, _, g64, ostate = runs["f64"]
    _, _, g32, _ = runs["f32"]
    n_stat = 0
    for k in t.files:
        if k.startswith("stat::") and not k.endswith("num_batches_tracked"):
            ref = torch.from_numpy(t[k])
            err = (msd[k[6:]].cpu() - ref).abs().max().item()
            assert err <= 1e-3 * ref.abs().max().item() + 1e-6, (k, err)
            n_stat += 1
    assert n_stat == sum(1 for k in msd if "running_" in k) > 0
    counters = [k for k in msd if k.endswith("num_batches_tracked")]
    assert counters and any(int(ostate[k]) == 1 for k in counters)
    bad = [(k, int(msd[k]), int(ostate[k])) for k in counters if int(msd[k]) != int(ostate[k])]
    assert not bad, bad[:5]
    assert not HF._PENDING_COUNTERS and HF._COUNTER_SCOPE[0] == 0
    # gradients: the acceptance formula of tests/test_bisenet_gpu.py
    params = dict(model.named_parameters())
    nh = nc = den = 0.0
    allw = []
    for k, t64 in g64.items():
        assert params[k].grad is not None, k
        gh = params[k].grad.detach().cpu().double()
        assert torch.isfinite(gh).all(), k
        eh, ec, n64 = (gh - t64).norm().item(), (g32[k].double() - t64).norm().item(), \
            t64.norm().item()
        nh, nc, den = nh + eh ** 2, nc + ec ** 2, den + n64 ** 2
        bound = 4 * ec + 1e-3 * n64
        allw.append((eh / max(bound, 1e-30), k, eh, ec, n64))
    for w in sorted(allw, reverse=True)[:8]:
        print("   %-55s ratio %.2f err_hip %.3e err_cpu32 %.3e |g64| %.3e"
              % (w[1], w[0], w[2], w[3], w[4]))
    print("dunet gradients vs fp64 oracle: global rel err HIP %.3e, CPU-fp32 %.3e"
          % ((nh / den) ** 0.5, (nc / den) ** 0.5))
    assert (nh / den) ** 0.5 <= 3 * (nc / den) ** 0.5 + 1e-4
    over = [w for w in allw if w[0] > 1.0]
    assert len(over) <= 0.10 * len(allw), (len(over), len(allw), over[:5])
    for _, k, eh, ec, n64 in over:
        assert eh <= 4 * ec + 3e-2 * n64, (k, eh, ec, n64)
    unused = [k for k, p in params.items() if p.grad is None]
    assert all(k.startswith("encoder.fc.") for k in unused), unused


# The reference's arithmetic under CPU bf16 autocast on this fixture (tests/_dunet_oracle.py
# train(autocast=True) against its float64 run, measured by tools/gen_golden_dunet.py and recorded
# in profiles/dunet.md and as `cpu::` entries of the fixture): loss 9.0115e-5 relative, gradient
# cosine 0.999783.  The bars are 1.3 x those distances, the ratio of the project's other bf16 bars.
BF16_LOSS_BAR = 1.3 * 9.0115e-5
BF16_COSINE_BAR = 1.0 - 1.3 * (1.0 - 0.999783)


def test_train_bf16_is_finite_and_as_close_as_autocast():
    model, _ = _build(torch.bfloat16, True)
    runs = _oracle_runs()
    x, y = runs["xy"]
    outs = model(x.cuda())
    loss = _mix_loss(outs, y.cuda())
    loss.backward()
    assert torch.isfinite(loss)
    params = dict(model.named_parameters())
    assert all(torch.isfinite(p.grad).all() for p in params.values() if p.grad is not None)
    l64, _, g64, _ = runs["f64"]
    dot = sum((params[k].grad.cpu().double() * g).sum().item() for k, g in g64.items())
    nh = sum(params[k].grad.cpu().double().pow(2).sum().item() for k in g64) ** 0.5
    n64 = sum(g.pow(2).sum().item() for g in g64.values()) ** 0.5
    lrel, cos = abs(loss.item() - l64) / l64, dot / (nh * n64)
    print("dunet bf16 vs fp64 oracle: loss rel %.3e (bar %.3e), gradient cosine %.6f (bar %.6f)"
          % (lrel, BF16_LOSS_BAR, cos, BF16_COSINE_BAR))
    assert lrel <= BF16_LOSS_BAR
    assert cos >= BF16_COSINE_BAR


class MixSoftmaxCrossEntropyLoss(nn.CrossEntropyLoss):
    """Shape of segmentron/solver/loss.py:16-46 (aux outputs weighted by aux_weight)."""

    def __init__(self, aux=True, aux_weight=0.4, ignore_index=-1):
        super().__init__(ignore_index=ignore_index)
        self.aux, self.aux_weight = aux, aux_weight

    def forward(self, *inputs, **kwargs):
        preds, target = tuple(inputs)
        loss = super().forward(preds[0], target)
        for p in preds[1:]:
            loss = loss + self.aux_weight * super().forward(p, target)
        return dict(loss=loss)


def test_reference_criterion_takes_the_fused_path_on_both_heads():
    from segmentron_amd import functional as F
    model, _ = _build(torch.float32, True)
    x, y = _oracle_runs()["xy"]
    outs = model(x.cuda())
    assert len(outs) == 2 and all(isinstance(o, F.DUpLogitsView) for o in outs)
    crit = MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=O.AUX_WEIGHT).cuda()
    loss = crit(outs, y.cuda())["loss"]
    loss.backward()
    assert all(o._full is None for o in outs)  # nothing was materialised at full resolution
    assert abs(loss.item() - _oracle_runs()["f64"][0]) < 1e-3 * loss.item()


def _run_loop(graph, iters=5):
    """The reference's loop statements (tools/train.py:135-146) on DUNet, bf16, AUX True."""
    from segmentron_amd.config import cfg, reset_cfg
    from segmentron_amd.solver.lr_scheduler import get_scheduler
    from segmentron_amd.solver.optimizer import get_optimizer
    prev = os.environ.get("SEGMENTRON_HIP_GRAPH")
    os.environ["SEGMENTRON_HIP_GRAPH"] = "1" if graph else "0"
    try:
        model, _ = _build(torch.bfloat16, True, phase="train")
        assert (getattr(model, "_transparent_graph", None) is not None) == graph
        criterion = MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=cfg.SOLVER.AUX_WEIGHT,
                                               ignore_index=cfg.DATASET.IGNORE_INDEX).to("cuda")
        optimizer = get_optimizer(model)
        lr_scheduler = get_scheduler(optimizer, max_iters=iters, iters_per_epoch=iters)
        losses_seen = []
        for it in range(iters):
            images = synth.synth_images(O.B, O.H, O.W, seed=100 + it).to("cuda")
            targets = synth.synth_targets(O.B, O.H, O.W, seed=100 + it).to("cuda")
            # ---- tools/train.py:135-146, verbatim
            outputs = model(images)
            loss_dict = criterion(outputs, targets)
            losses = sum(loss for loss in loss_dict.values())
            optimizer.zero_grad()
            losses.backward()
            optimizer.step()
            lr_scheduler.step()
            # ----
            losses_seen.append(losses.item())
        torch.cuda.synchronize()
        tg = getattr(model, "_transparent_graph", None)
        if graph:
            assert tg.disabled is None, tg.disabled
            assert len(tg.segments) == 1, "the loop did not reach the captured path"
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return losses_seen, state
    finally:
        if prev is None:
            os.environ.pop("SEGMENTRON_HIP_GRAPH", None)
        else:
            os.environ["SEGMENTRON_HIP_GRAPH"] = prev
        reset_cfg()


def test_graph_mode_equals_eager_bit_for_bit():
    le, se = _run_loop(False)
    lg, sg = _run_loop(True)
    print("dunet loop losses eager %s\n                  graph %s"
          % (["%.5f" % v for v in le], ["%.5f" % v for v in lg]))
    assert all(np.isfinite(le))
    assert le == lg
    bad = [k for k in se if not torch.equal(se[k], sg[k])]
    assert not bad, bad[:5]
