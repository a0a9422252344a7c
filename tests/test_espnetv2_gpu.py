"""GPU: ESPNetV2 on the HIP path against the reference's fixtures (tests/golden/espnetv2_*.npz,
tools/gen_golden_espnetv2.py) and the float64 restatement (tests/_espnetv2_oracle.py): evaluation,
one training step at 4 x 128 x 192 (the 1/8-resolution BatchNorms see 1536 rows, the 1/16 ones 384:
the few-sample path), the small fixture, bf16, SOLVER.AUX, the fused loss tier behind the
reference's criterion, and HIP-graph replay == eager launches bit for bit.  The never-used
level5* / fc parameters keep `grad is None` and their initial values throughout."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _espnetv2_oracle as O
from conftest import GOLDEN
from oracle import synth
from test_espnetv2 import YAML, fixture_keys, train_fixture_logits

pytestmark = pytest.mark.gpu


def _build(dtype, train, phase="test", overrides=()):
    import segmentron_amd
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(YAML)
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False"] + list(overrides))
    cfg.PHASE = phase
    cfg.check_and_freeze()
    segmentron_amd.set_compute_dtype(dtype)
    model = segmentron_amd.get_segmentation_model()
    sd = O.state(fixture_keys()[1])
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train(train)
    for m in model.modules():
        if isinstance(m, (nn.Dropout, nn.Dropout2d)):
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


def _loss(outs, y):
    return torch.nn.functional.cross_entropy(outs[0], y, ignore_index=-1)


def _no_grad_where_unused(model):
    """level5*, fc and a DownSampler EESP's module_act never run: no gradient, not a zero one
    (weight decay would move them); everything else has a finite gradient."""
    for k, p in model.named_parameters():
        if O.unused(k):
            assert p.grad is None, k
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_eval_fp32_matches_reference_fixture():
    model, _ = _build(torch.float32, False)
    g = np.load(os.path.join(GOLDEN, "espnetv2_eval.npz"))
    with torch.no_grad():
        outs = model(synth.synth_images(O.B, O.H, O.W, seed=0).cuda())
    assert len(outs) == 1 and isinstance(outs[0], torch.Tensor)
    ref = torch.from_numpy(g["logits0"])
    logits = outs[0].cpu()[..., ::2, ::2]
    rel = _rel(logits, ref)
    bad = logits.argmax(1) != ref.argmax(1)
    top2 = ref.topk(2, dim=1).values
    gap = (top2[:, 0] - top2[:, 1])[bad]
    print("espnetv2 eval fp32 max-rel %.3e; argmax mismatches %d of %d (largest reference top-2 "
          "gap among them %.2e)" % (rel, int(bad.sum()), bad.numel(),
                                    gap.max().item() if gap.numel() else 0.0))
    assert rel < 1e-3
    # masks identical except at genuine ties of the reference itself (top-2 gap below the 1e-3 bar)
    assert gap.numel() == 0 or gap.max().item() < 1e-3 * ref.abs().max().item()


def test_eval_second_size_matches_oracle_and_other_sizes_raise():
    """48 x 80: a 3 x 5 map at 1/16, so the pyramid pooling reaches 1 x 1 after two pools.  Sizes
    that are no multiple of 16 raise in the reference (its x2 resizes meet the encoder's maps in a
    concat); here they raise before any launch."""
    model, sd = _build(torch.float32, False)
    x = synth.synth_images(1, O.H2, O.W2, seed=0)
    with torch.no_grad():
        out = model(x.cuda())[0].cpu()
        for hw in ((65, 97), (64, 100), (56, 96)):
            with pytest.raises(ValueError, match="multiples of 16"):
                model(synth.synth_images(1, hw[0], hw[1], seed=0).cuda())
    ref = O.evaluate(sd, x)[0]
    assert _rel(out, ref) < 1e-3


# the float64 / float32 CPU runs of the oracle on the training fixture, computed once
_ORACLE = {}


def _oracle_runs():
    if not _ORACLE:
        sd = O.state(fixture_keys()[1])
        x = synth.synth_images(O.TB, O.TH, O.TW, seed=O.TRAIN_SEED)
        y = synth.synth_targets(O.TB, O.TH, O.TW, seed=O.TRAIN_SEED)
        _ORACLE["f64"] = O.train(sd, x, y, torch.float64)
        _ORACLE["f32"] = O.train(sd, x, y, torch.float32)
        _ORACLE["xy"] = (x, y)
    return _ORACLE


def test_train_fp32_matches_reference_and_fp64_oracle():
    model, sd = _build(torch.float32, True)
    runs = _oracle_runs()
    x, y = runs["xy"]
    outs = model(x.cuda())
    loss = _loss(outs, y.cuda())
    loss.backward()
    t = np.load(os.path.join(GOLDEN, "espnetv2_train.npz"))
    ref_loss = float(t["loss"])
    rel = _rel(outs[0].detach().cpu()[..., ::2, ::2], train_fixture_logits())
    print("espnetv2 train fp32: loss %.6f (fixture %.6f), logits max-rel %.2e"
          % (loss.item(), ref_loss, rel))
    assert abs(loss.item() - ref_loss) < 1e-3 * ref_loss
    assert rel < 1e-3
    # running statistics after the step against the reference's, every counter too
    msd = model.state_dict()
    _, _, g64, _ = runs["f64"]
    _, _, g32, _ = runs["f32"]
    n_stat = 0
    for k in t.files:
        if not k.startswith("stat::"):
            continue
        ref = torch.from_numpy(t[k])
        if k.endswith("num_batches_tracked"):
            assert int(msd[k[6:]]) == int(ref) == (0 if O.unused(k[6:]) else 1), k
        else:
            err = (msd[k[6:]].cpu() - ref).abs().max().item()
            assert err <= 1e-3 * ref.abs().max().item() + 1e-6, (k, err)
            n_stat += 1
    assert n_stat == sum(1 for k in msd if "running_" in k) > 0
    _no_grad_where_unused(model)
    from segmentron_amd import functional as HF
    assert not HF._PENDING_COUNTERS and HF._COUNTER_SCOPE[0] == 0
    # gradients: the project's acceptance rule
    params = dict(model.named_parameters())
    assert {k for k in params if not O.unused(k)} == set(g64), "the used parameters differ"
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
        print("   %-45s ratio %.2f err_hip %.3e err_cpu32 %.3e |g64| %.3e"
              % (w[1], w[0], w[2], w[3], w[4]))
    print("espnetv2 gradients vs fp64 oracle: global rel err HIP %.3e, CPU-fp32 %.3e"
          % ((nh / den) ** 0.5, (nc / den) ** 0.5))
    assert (nh / den) ** 0.5 <= 3 * (nc / den) ** 0.5 + 1e-4
    over = [w for w in allw if w[0] > 1.0]
    assert len(over) <= 0.10 * len(allw), (len(over), len(allw), over[:5])
    for _, k, eh, ec, n64 in over:
        assert eh <= 4 * ec + 3e-2 * n64, (k, eh, ec, n64)


def test_small_train_fp32_matches_reference_fixture():
    """2 x 64 x 96: the BatchNorms from 1/8 resolution down see at most 192 rows, the few-sample
    path (the pyramid pooling reaches 1 x 1 maps)."""
    from segmentron_amd import hip_ops
    model, _ = _build(torch.float32, True)
    assert O.B * (O.H // 8) * (O.W // 8) <= hip_ops.SMALL_BN_ROWS
    x = synth.synth_images(O.B, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B, O.H, O.W, seed=0)
    outs = model(x.cuda())
    loss = _loss(outs, y.cuda())
    loss.backward()
    t = np.load(os.path.join(GOLDEN, "espnetv2_small_train.npz"))
    rel = _rel(outs[0].detach().cpu()[..., ::2, ::2], torch.from_numpy(t["logits0"]))
    print("espnetv2 small train fp32: loss %.6f (fixture %.6f), logits max-rel %.2e"
          % (loss.item(), float(t["loss"]), rel))
    assert abs(loss.item() - float(t["loss"])) < 1e-3 * float(t["loss"]) and rel < 1e-3
    _no_grad_where_unused(model)


# The reference itself under CPU bf16 autocast on this fixture (tests/_espnetv2_oracle.py
# train(autocast=True) against its float64 run; `cpu::` entries of
# tests/golden/espnetv2_train.npz): loss 8.0473e-04 relative, gradient cosine 0.99999495.  The bars
# are 1.3 x those distances, the ratio of the C3 / C4 / BiSeNet / LEDNet bf16 bars.
def _bf16_bars():
    t = np.load(os.path.join(GOLDEN, "espnetv2_train.npz"))
    lrel, cos = float(t["cpu::bf16_loss_rel"]), float(t["cpu::bf16_grad_cos"])
    assert abs(lrel - 8.0473e-04) < 1e-8 and abs(cos - 0.99999495) < 1e-8
    return 1.3 * lrel, 1.0 - 1.3 * (1.0 - cos)


def test_train_bf16_is_finite_and_as_close_as_autocast():
    loss_bar, cos_bar = _bf16_bars()
    model, _ = _build(torch.bfloat16, True)
    runs = _oracle_runs()
    x, y = runs["xy"]
    outs = model(x.cuda())
    loss = _loss(outs, y.cuda())
    loss.backward()
    assert torch.isfinite(loss)
    params = dict(model.named_parameters())
    _no_grad_where_unused(model)
    l64, _, g64, _ = runs["f64"]
    dot = sum((params[k].grad.cpu().double() * g).sum().item() for k, g in g64.items())
    nh = sum(params[k].grad.cpu().double().pow(2).sum().item() for k in g64) ** 0.5
    n64 = sum(g.pow(2).sum().item() for g in g64.values()) ** 0.5
    lrel, cos = abs(loss.item() - l64) / l64, dot / (nh * n64)
    print("espnetv2 bf16 vs fp64 oracle: loss rel %.3e (bar %.3e), gradient cosine %.6f (bar %.6f)"
          % (lrel, loss_bar, cos, cos_bar))
    assert lrel <= loss_bar
    assert cos >= cos_bar


class MixSoftmaxCrossEntropyLoss(nn.CrossEntropyLoss):
    """Shape of segmentron/solver/loss.py:16-46 (aux outputs weighted by aux_weight)."""

    def __init__(self, aux=False, aux_weight=0.4, ignore_index=-1):
        super().__init__(ignore_index=ignore_index)
        self.aux, self.aux_weight = aux, aux_weight

    def forward(self, *inputs, **kwargs):
        preds, target = tuple(inputs)
        loss = super().forward(preds[0], target)
        for p in preds[1:]:
            loss = loss + self.aux_weight * super().forward(p, target)
        return dict(loss=loss)


def test_aux_output_matches_fp64_oracle():
    """SOLVER.AUX True: the second output is project_l3's map before its BatchNorm, resized to the
    input size; no extra parameters.  2 x 64 x 96 against the float64 restatement: both outputs,
    the loss with aux_weight 0.4, the gradients."""
    model, sd = _build(torch.float32, True, overrides=["SOLVER.AUX", "True"])
    assert model.aux is True
    assert [k for k, _ in model.state_dict().items()] == [k for k, _ in fixture_keys()[1]]
    x = synth.synth_images(O.B, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B, O.H, O.W, seed=0)
    outs = model(x.cuda())
    assert len(outs) == 2
    loss = MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=0.4).cuda()(outs, y.cuda())["loss"]
    loss.backward()
    l64, o64, g64, _ = O.train(sd, x, y, torch.float64, aux=True, aux_weight=0.4)
    for i in range(2):
        full = outs[i].materialize() if hasattr(outs[i], "materialize") else outs[i]
        assert tuple(full.shape) == (O.B, 19, O.H, O.W)
        assert _rel(full.detach().cpu(), o64[i]) < 1e-3, i
    print("espnetv2 aux: loss %.6f (float64 %.6f)" % (loss.item(), l64))
    assert abs(loss.item() - l64) < 1e-3 * l64
    _no_grad_where_unused(model)
    params = dict(model.named_parameters())
    num = sum((params[k].grad.cpu().double() - g).pow(2).sum().item() for k, g in g64.items())
    den = sum(g.pow(2).sum().item() for g in g64.values())
    print("espnetv2 aux gradients vs fp64 oracle: global rel err %.3e" % (num / den) ** 0.5)
    assert (num / den) ** 0.5 < 1e-3


def test_reference_criterion_takes_the_fused_tier():
    """The final resize is x2 from 1/2 resolution: (H - 1) / (H / 2 - 1) <= 8.1 at every size, so
    a training forward hands the criterion a pending view and the loss runs fused on the
    1/2-resolution logits — 2 x 512 x 528 here."""
    from segmentron_amd import functional as F
    model, _ = _build(torch.float32, True)
    Hf, Wf = 512, 528
    x = synth.synth_images(2, Hf, Wf, seed=3).cuda()
    y = synth.synth_targets(2, Hf, Wf, seed=3).cuda()
    outs = model(x)
    assert len(outs) == 1 and isinstance(outs[0], F.LogitsView)
    assert tuple(outs[0].lo.shape[1:3]) == (Hf // 2, Wf // 2)
    loss = MixSoftmaxCrossEntropyLoss().cuda()(outs, y)["loss"]
    loss.backward()
    assert outs[0]._full is None  # nothing was materialised at full resolution
    _no_grad_where_unused(model)
    with torch.no_grad():
        full = torch.nn.functional.cross_entropy(outs[0].materialize(), y, ignore_index=-1)
    assert abs(loss.item() - full.item()) < 1e-5 * full.item()


def _run_loop(graph, iters=5):
    """The reference's loop statements (tools/train.py:135-146) on ESPNetV2, bf16."""
    from segmentron_amd.config import cfg, reset_cfg
    from segmentron_amd.solver.lr_scheduler import get_scheduler
    from segmentron_amd.solver.optimizer import get_optimizer
    prev = os.environ.get("SEGMENTRON_HIP_GRAPH")
    os.environ["SEGMENTRON_HIP_GRAPH"] = "1" if graph else "0"
    try:
        model, sd0 = _build(torch.bfloat16, True, phase="train")
        assert (getattr(model, "_transparent_graph", None) is not None) == graph
        criterion = MixSoftmaxCrossEntropyLoss(ignore_index=cfg.DATASET.IGNORE_INDEX).to("cuda")
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
        # the never-used modules: no gradient, so neither momentum nor weight decay moved them
        for k, p in model.named_parameters():
            if O.unused(k):
                assert p.grad is None, k
        moved = [k for k in state if O.unused(k) and not torch.equal(state[k].cpu(), sd0[k])]
        assert not moved, moved[:5]
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
    print("espnetv2 loop losses eager %s\n                    graph %s"
          % (["%.5f" % v for v in le], ["%.5f" % v for v in lg]))
    assert all(np.isfinite(le))
    assert le == lg
    bad = [k for k in se if not torch.equal(se[k], sg[k])]
    assert not bad, bad[:5]
