"""What the per-model tests (tests/test_<m>.py, tests/test_<m>_gpu.py) share: one `Spec` per model
and, once each, the fixture readers, the model builder, the reference's criterion and train loop,
and the checks — the evaluation fixture with its tie rule, the running statistics, the gradient
acceptance rule against the float64 oracle, the bf16 bars, eager == graph.  A test body is a call
into this module with its model's spec; what only one model checks stays in that model's file."""
import json
import os
from dataclasses import dataclass
from types import ModuleType
from typing import Callable, Optional

import numpy as np
import pytest
import torch
import torch.nn as nn

import _bisenet_oracle
import _cgnet_oracle
import _dunet_oracle
import _espnetv2_oracle
import _lednet_oracle
from conftest import GOLDEN
from oracle import synth


@dataclass
class Spec:
    name: str                      # prefix of the fixture files and of the printed lines
    O: ModuleType                  # the float64 restatement, tests/_<name>_oracle.py
    model: str                     # name in the model registry
    eval_shape: tuple              # B, H, W of <name>_eval.npz
    train_shape: tuple             # B, H, W of <name>_train.npz
    loop_shape: tuple              # B, H, W of the eager == graph loop
    n_keys: int                    # pinned by the CPU tests
    n_params: int
    bf16: tuple                    # the reference under CPU bf16 autocast: (loss rel, cosine)
    key_width: int                 # column width of the worst-ratio table
    graph_indent: int              # indent of the loop's second printed line
    n_grads: Optional[int] = None  # gradients the train fixture holds (None: not pinned)
    min_grads: int = 0
    second_shape: Optional[tuple] = None   # H, W of the one-image second evaluation size
    train_seed: int = 0
    eval_step: int = 2             # the eval fixture holds every eval_step-th pixel
    logit_steps: tuple = (2,)      # the train fixture holds every n-th pixel of output i
    split_logits: bool = True      # the train logits lie in <name>_train_logits_a / _b.npz
    overrides: tuple = ()          # cfg overrides of every build
    aux_weight: float = 0.4
    n_eval_outputs: int = 1
    small_overrides: tuple = ()    # the small fixture's model (CGNet)
    small_keys: Optional[Callable] = None
    unused: Callable = lambda key: False   # parameters no forward reaches
    counters_are_one: bool = True  # every num_batches_tracked of a reached module is 1 after a step
    bf16_tol: Optional[tuple] = None  # |fixture's cpu:: entry - literal| bounds (None: no entries)
    train_view: Optional[str] = None  # functional class of the training outputs, never materialised
    head_stride: int = 8           # the fused-loss tier test: logits at 1 / head_stride ...
    fused_shape: Optional[tuple] = None  # ... of this B, H, W

    @property
    def yaml(self):
        return os.path.join(GOLDEN, "cityscapes_%s.yaml" % self.name)

    def file(self, what):
        return os.path.join(GOLDEN, "%s_%s" % (self.name, what))


def cfg_for(spec, *overrides, phase="test"):
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(spec.yaml)
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False"] + list(overrides))
    cfg.PHASE = phase
    cfg.check_and_freeze()
    return cfg


def fixture_keys(spec):
    with open(spec.file("state_keys.json")) as f:
        ref = json.load(f)
    return ref, [(k, tuple(s)) for k, s in ref["keys"]]


def train_fixture_logits(spec):
    """-> the train fixture's logits, one tensor per output."""
    if spec.split_logits:
        return [torch.cat([torch.from_numpy(np.load(spec.file(f))["logits0"])
                           for f in ("train_logits_a.npz", "train_logits_b.npz")])]
    t = np.load(spec.file("train.npz"))
    return [torch.from_numpy(t["logits%d" % i]) for i in range(len(spec.logit_steps))]


def build(spec, dtype, train, phase="test", overrides=None, keys=None):
    """-> (the HIP model on the device with the synthesised state and dropout 0, that state)."""
    import segmentron_amd
    cfg_for(spec, *(spec.overrides if overrides is None else overrides), phase=phase)
    segmentron_amd.set_compute_dtype(dtype)
    model = segmentron_amd.get_segmentation_model()
    sd = spec.O.state(fixture_keys(spec)[1] if keys is None else keys)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train(train)
    for m in model.modules():
        if isinstance(m, (nn.Dropout, nn.Dropout2d)):
            m.p = 0.0
    return model, sd


@pytest.fixture(autouse=True)
def fresh_cfg():
    """(imported by every test_<m>_gpu.py) the next test starts from float32 and an empty cfg."""
    import segmentron_amd
    from segmentron_amd.config import reset_cfg
    yield
    segmentron_amd.set_compute_dtype(torch.float32)
    reset_cfg()


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


def mix_loss(spec, outs, y):
    loss = torch.nn.functional.cross_entropy(outs[0], y, ignore_index=-1)
    for o in outs[1:]:
        loss = loss + spec.aux_weight * torch.nn.functional.cross_entropy(o, y, ignore_index=-1)
    return loss


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


def train_inputs(spec):
    return (synth.synth_images(*spec.train_shape, seed=spec.train_seed),
            synth.synth_targets(*spec.train_shape, seed=spec.train_seed))


_ORACLE = {}


def oracle_runs(spec):
    """The float64 / float32 CPU runs of the oracle on the training fixture, computed once."""
    if spec.name not in _ORACLE:
        sd = spec.O.state(fixture_keys(spec)[1])
        x, y = train_inputs(spec)
        _ORACLE[spec.name] = {"f64": spec.O.train(sd, x, y, torch.float64),
                              "f32": spec.O.train(sd, x, y, torch.float32), "xy": (x, y)}
    return _ORACLE[spec.name]


# ---------------------------------------------------------------------------------------- checks

def check_grads_where_used(spec, model):
    """A parameter that no forward reaches has no gradient, not a zero one (weight decay would
    move it); every other one has a finite gradient."""
    for k, p in model.named_parameters():
        if spec.unused(k):
            assert p.grad is None, k
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k


def check_eval_fixture(spec):
    model, _ = build(spec, torch.float32, False)
    g = np.load(spec.file("eval.npz"))
    B, H, W = spec.eval_shape
    with torch.no_grad():
        outs = model(synth.synth_images(B, H, W, seed=0).cuda())
        if "shape_odd" in g.files:
            odd = model(synth.synth_images(1, *spec.second_shape, seed=0).cuda())
            assert tuple(odd[0].shape) == tuple(g["shape_odd"]) and torch.isfinite(odd[0]).all()
    assert len(outs) == spec.n_eval_outputs and all(isinstance(o, torch.Tensor) for o in outs)
    assert "n_outputs" not in g.files or len(outs) == int(g["n_outputs"])
    assert all(o.dtype == torch.float32 and tuple(o.shape) == (B, 19, H, W) for o in outs)
    ref = torch.from_numpy(g["logits0"])
    logits = outs[0].cpu()[..., ::spec.eval_step, ::spec.eval_step]
    r = rel(logits, ref)
    bad = logits.argmax(1) != ref.argmax(1)
    top2 = ref.topk(2, dim=1).values
    gap = (top2[:, 0] - top2[:, 1])[bad]
    print("%s eval fp32 max-rel %.3e; argmax mismatches %d of %d (largest reference top-2 gap "
          "among them %.2e)" % (spec.name, r, int(bad.sum()), bad.numel(),
                                gap.max().item() if gap.numel() else 0.0))
    assert r < 1e-3
    # masks identical except at genuine ties of the reference itself (top-2 gap below the 1e-3 bar)
    assert gap.numel() == 0 or gap.max().item() < 1e-3 * ref.abs().max().item()


def check_eval_second_size(spec):
    model, sd = build(spec, torch.float32, False)
    x = synth.synth_images(1, *spec.second_shape, seed=0)
    with torch.no_grad():
        out = model(x.cuda())[0].cpu()
    assert rel(out, spec.O.evaluate(sd, x)[0]) < 1e-3


def check_running_stats(spec, model, t, ostate):
    """The running statistics after the step against the reference's (`stat::` of the train
    fixture `t`), every counter against the fixture's and the oracle's."""
    msd = model.state_dict()
    n_stat = 0
    for k in t.files:
        if not k.startswith("stat::"):
            continue
        ref = torch.from_numpy(t[k])
        if k.endswith("num_batches_tracked"):
            assert int(msd[k[6:]]) == int(ref) == int(ostate[k[6:]]), k
            if spec.counters_are_one:
                assert int(ref) == (0 if spec.unused(k[6:]) else 1), k
        else:
            err = (msd[k[6:]].cpu() - ref).abs().max().item()
            assert err <= 1e-3 * ref.abs().max().item() + 1e-6, (k, err)
            n_stat += 1
    assert n_stat == sum(1 for k in msd if "running_" in k) > 0
    counters = [k for k in msd if k.endswith("num_batches_tracked")]
    assert counters and any(int(ostate[k]) == 1 for k in counters)
    bad = [(k, int(msd[k]), int(ostate[k])) for k in counters if int(msd[k]) != int(ostate[k])]
    assert not bad, bad[:5]
    from segmentron_amd import functional as HF
    assert not HF._PENDING_COUNTERS and HF._COUNTER_SCOPE[0] == 0


def check_gradients(params, g64, g32, unused=None, name="", key_width=45):
    """The project's acceptance rule for a model's gradients `params[k].grad` against the float64
    oracle's `g64`, with the float32 CPU run `g32` of the same arithmetic as the yardstick: global
    error <= 3 x CPU-fp32 + 1e-4; per tensor `bound` below, with at most 10 % of the tensors beyond
    it and none beyond the same sum with 3e-2 in place of 1e-3.  The parameters with a gradient
    are the oracle's; with `unused(key)`, those it names have none.
    -> the table (ratio to the bound, key, err_hip, err_cpu32, |g64|), worst first."""
    used = {k for k in params if not (unused and unused(k))}
    assert used == set(g64), ("the used parameters differ", sorted(used ^ set(g64))[:5])
    for k in set(params) - used:
        assert params[k].grad is None, k
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
    allw.sort(reverse=True)
    for w in allw[:8]:
        print("   %-*s ratio %.2f err_hip %.3e err_cpu32 %.3e |g64| %.3e"
              % (key_width, w[1], w[0], w[2], w[3], w[4]))
    print("%s gradients vs fp64 oracle: global rel err HIP %.3e, CPU-fp32 %.3e"
          % (name, (nh / den) ** 0.5, (nc / den) ** 0.5))
    assert (nh / den) ** 0.5 <= 3 * (nc / den) ** 0.5 + 1e-4
    over = [w for w in allw if w[0] > 1.0]
    assert len(over) <= 0.10 * len(allw), (len(over), len(allw), over[:5])
    for _, k, eh, ec, n64 in over:
        assert eh <= 4 * ec + 3e-2 * n64, (k, eh, ec, n64)
    return allw


def check_train_fp32(spec):
    """One training step against the reference's fixture and the float64 oracle."""
    from segmentron_amd import functional as HF
    model, _ = build(spec, torch.float32, True)
    runs = oracle_runs(spec)
    x, y = runs["xy"]
    outs = model(x.cuda())
    assert len(outs) == len(spec.logit_steps)
    if spec.train_view:
        assert all(isinstance(o, getattr(HF, spec.train_view)) for o in outs)
    loss = mix_loss(spec, outs, y.cuda())
    if spec.train_view:
        assert all(o._full is None for o in outs)
    loss.backward()
    t = np.load(spec.file("train.npz"))
    ref_loss = float(t["loss"])
    full = [o.materialize() if spec.train_view else o for o in outs]
    rels = [rel(o.detach().cpu()[..., ::s, ::s], ref)
            for o, s, ref in zip(full, spec.logit_steps, train_fixture_logits(spec))]
    print("%s train fp32: loss %.6f (fixture %.6f), logits max-rel %s"
          % (spec.name, loss.item(), ref_loss,
             "%.2e" % rels[0] if len(rels) == 1 else ["%.2e" % r for r in rels]))
    assert abs(loss.item() - ref_loss) < 1e-3 * ref_loss
    assert max(rels) < 1e-3
    _, _, g64, ostate = runs["f64"]
    _, _, g32, _ = runs["f32"]
    check_running_stats(spec, model, t, ostate)
    check_gradients(dict(model.named_parameters()), g64, g32, spec.unused, spec.name,
                    spec.key_width)


def check_small_train(spec, model):
    """The step of <name>_small_train.npz on `model`: the few-sample BatchNorm path."""
    B, H, W = spec.eval_shape
    x = synth.synth_images(B, H, W, seed=0)
    y = synth.synth_targets(B, H, W, seed=0)
    outs = model(x.cuda())
    loss = mix_loss(spec, outs, y.cuda())
    loss.backward()
    t = np.load(spec.file("small_train.npz"))
    r = rel(outs[0].detach().cpu()[..., ::2, ::2], torch.from_numpy(t["logits0"]))
    print("%s small train fp32: loss %.6f (fixture %.6f), logits max-rel %.2e"
          % (spec.name, loss.item(), float(t["loss"]), r))
    assert abs(loss.item() - float(t["loss"])) < 1e-3 * float(t["loss"]) and r < 1e-3
    check_grads_where_used(spec, model)


def bf16_bars(spec):
    """-> (loss bar, cosine bar): 1.3 x the distances of the reference itself under CPU bf16
    autocast from its float64 run on the training fixture — `spec.bf16`, and where the fixture
    records them (`cpu::`), its entries, which must be those literals."""
    lrel, cos = spec.bf16
    if spec.bf16_tol:
        t = np.load(spec.file("train.npz"))
        flrel, fcos = float(t["cpu::bf16_loss_rel"]), float(t["cpu::bf16_grad_cos"])
        assert abs(flrel - lrel) < spec.bf16_tol[0] and abs(fcos - cos) < spec.bf16_tol[1]
        lrel, cos = flrel, fcos
    return 1.3 * lrel, 1.0 - 1.3 * (1.0 - cos)


def check_train_bf16(spec):
    loss_bar, cos_bar = bf16_bars(spec)
    model, _ = build(spec, torch.bfloat16, True)
    runs = oracle_runs(spec)
    x, y = runs["xy"]
    outs = model(x.cuda())
    loss = mix_loss(spec, outs, y.cuda())
    loss.backward()
    assert torch.isfinite(loss)
    params = dict(model.named_parameters())
    check_grads_where_used(spec, model)
    l64, _, g64, _ = runs["f64"]
    dot = sum((params[k].grad.cpu().double() * g).sum().item() for k, g in g64.items())
    nh = sum(params[k].grad.cpu().double().pow(2).sum().item() for k in g64) ** 0.5
    n64 = sum(g.pow(2).sum().item() for g in g64.values()) ** 0.5
    lrel, cos = abs(loss.item() - l64) / l64, dot / (nh * n64)
    print("%s bf16 vs fp64 oracle: loss rel %.3e (bar %.3e), gradient cosine %.6f (bar %.6f)"
          % (spec.name, lrel, loss_bar, cos, cos_bar))
    assert lrel <= loss_bar
    assert cos >= cos_bar


def check_fused_tier(spec):
    """At `spec.fused_shape` the head's final resize is within the fused loss's tier: a training
    forward hands the reference's criterion a pending view and nothing is materialised."""
    from segmentron_amd import functional as F
    model, _ = build(spec, torch.float32, True)
    B, Hf, Wf = spec.fused_shape
    x = synth.synth_images(B, Hf, Wf, seed=3).cuda()
    y = synth.synth_targets(B, Hf, Wf, seed=3).cuda()
    outs = model(x)
    assert len(outs) == 1 and isinstance(outs[0], F.LogitsView)
    assert tuple(outs[0].lo.shape[1:3]) == (Hf // spec.head_stride, Wf // spec.head_stride)
    loss = MixSoftmaxCrossEntropyLoss().cuda()(outs, y)["loss"]
    loss.backward()
    assert outs[0]._full is None  # nothing was materialised at full resolution
    check_grads_where_used(spec, model)
    with torch.no_grad():
        full = torch.nn.functional.cross_entropy(outs[0].materialize(), y, ignore_index=-1)
    assert abs(loss.item() - full.item()) < 1e-5 * full.item()


def check_fused_on_every_head(spec, view):
    """The training fixture through the reference's criterion: every output is a pending `view`
    and stays one."""
    from segmentron_amd import functional as F
    model, _ = build(spec, torch.float32, True)
    runs = oracle_runs(spec)
    x, y = runs["xy"]
    outs = model(x.cuda())
    assert len(outs) == len(spec.logit_steps)
    assert all(isinstance(o, getattr(F, view)) for o in outs)
    crit = MixSoftmaxCrossEntropyLoss(aux=True, aux_weight=spec.aux_weight).cuda()
    loss = crit(outs, y.cuda())["loss"]
    loss.backward()
    assert all(o._full is None for o in outs)  # nothing was materialised at full resolution
    assert abs(loss.item() - runs["f64"][0]) < 1e-3 * loss.item()


def run_loop(spec, graph, iters=5):
    """The reference's loop statements (tools/train.py:135-146) on the model, bf16."""
    from segmentron_amd.config import cfg, reset_cfg
    from segmentron_amd.solver.lr_scheduler import get_scheduler
    from segmentron_amd.solver.optimizer import get_optimizer
    prev = os.environ.get("SEGMENTRON_HIP_GRAPH")
    os.environ["SEGMENTRON_HIP_GRAPH"] = "1" if graph else "0"
    try:
        model, sd0 = build(spec, torch.bfloat16, True, phase="train")
        assert (getattr(model, "_transparent_graph", None) is not None) == graph
        criterion = MixSoftmaxCrossEntropyLoss(aux=cfg.SOLVER.AUX, aux_weight=cfg.SOLVER.AUX_WEIGHT,
                                               ignore_index=cfg.DATASET.IGNORE_INDEX).to("cuda")
        optimizer = get_optimizer(model)
        lr_scheduler = get_scheduler(optimizer, max_iters=iters, iters_per_epoch=iters)
        losses_seen = []
        for it in range(iters):
            images = synth.synth_images(*spec.loop_shape, seed=100 + it).to("cuda")
            targets = synth.synth_targets(*spec.loop_shape, seed=100 + it).to("cuda")
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
            if spec.unused(k):
                assert p.grad is None, k
        moved = [k for k in state if spec.unused(k) and not torch.equal(state[k].cpu(), sd0[k])]
        assert not moved, moved[:5]
        return losses_seen, state
    finally:
        if prev is None:
            os.environ.pop("SEGMENTRON_HIP_GRAPH", None)
        else:
            os.environ["SEGMENTRON_HIP_GRAPH"] = prev
        reset_cfg()


def check_graph_equals_eager(spec):
    le, se = run_loop(spec, False)
    lg, sg = run_loop(spec, True)
    print("%s loop losses eager %s\n%sgraph %s"
          % (spec.name, ["%.5f" % v for v in le], " " * spec.graph_indent,
             ["%.5f" % v for v in lg]))
    assert all(np.isfinite(le))
    assert le == lg
    bad = [k for k in se if not torch.equal(se[k], sg[k])]
    assert not bad, bad[:5]


# ------------------------------------------------------------------- the CPU files' shared checks

def check_resolves_through_the_overlay(spec, extra=""):
    from test_dropin import _run
    out = _run("""
        import sys
        sys.path = [p for p in sys.path if 'reference' not in p]
        sys.argv = ['x']
        import segmentron, segmentron_amd
        from segmentron.config import cfg
        from segmentron.models.model_zoo import get_segmentation_model, MODEL_REGISTRY
        assert %r in MODEL_REGISTRY.get_list()
        cfg.update_from_file(%r)
        cfg.update_from_list(['TRAIN.BACKBONE_PRETRAINED', 'False'])
        cfg.PHASE = 'test'
        cfg.check_and_freeze()
        model = get_segmentation_model()
        assert type(model).__module__ == 'segmentron_amd.models.%s', type(model).__module__
        %s
        print('%s_OK')
    """ % (spec.model, spec.yaml, spec.name, extra, spec.name.upper()),
               env_extra={"SEGMENTRON_REFERENCE_ROOT": ""})
    assert spec.name.upper() + "_OK" in out


def check_oracle_eval_fixture(spec, **evaluate_kw):
    """The restatement against <name>_eval.npz.  -> (state, fixture) for what a model adds."""
    sd = spec.O.state(fixture_keys(spec)[1])
    outs = spec.O.evaluate(sd, synth.synth_images(*spec.eval_shape, seed=0), **evaluate_kw)
    g = np.load(spec.file("eval.npz"))
    assert len(outs) == spec.n_eval_outputs
    assert "n_outputs" not in g.files or len(outs) == int(g["n_outputs"])
    assert torch.allclose(outs[0][..., ::spec.eval_step, ::spec.eval_step],
                          torch.from_numpy(g["logits0"]), rtol=1e-4, atol=1e-4)
    return sd, g


def _check_train(spec, t, logits_ref, loss, outs, grads, after):
    assert abs(loss - float(t["loss"])) < 1e-5
    assert len(outs) == len(logits_ref)
    for o, s, ref in zip(outs, spec.logit_steps, logits_ref):
        assert torch.allclose(o[..., ::s, ::s], ref, rtol=1e-4, atol=1e-4)
    names = [k[len("gnorm::"):] for k in t.files if k.startswith("gnorm::")]
    assert len(names) > spec.min_grads and set(names) == set(grads)
    for k in names:
        n = float(t["gnorm::" + k])
        assert abs(float(grads[k].double().norm()) - n) <= 1e-3 * max(n, 1e-6) + 1e-9, k
    stats = [k[len("stat::"):] for k in t.files if k.startswith("stat::")]
    assert stats
    for k in stats:
        ref = torch.from_numpy(t["stat::" + k])
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(ref), k
            if spec.counters_are_one:
                assert int(ref) == (0 if spec.unused(k) else 1), k
        else:
            assert (after[k] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-6, k
    return names


def check_oracle_train_fixture(spec):
    """The restatement against <name>_train.npz.  -> (gradient names, fixture)."""
    sd = spec.O.state(fixture_keys(spec)[1])
    t = np.load(spec.file("train.npz"))
    assert "seed" not in t.files or int(t["seed"]) == spec.train_seed
    names = _check_train(spec, t, train_fixture_logits(spec),
                         *spec.O.train(sd, *train_inputs(spec)))
    assert spec.n_grads is None or len(names) == spec.n_grads
    assert not any(spec.unused(k) for k in names)
    if spec.bf16_tol:
        # what the reference's own arithmetic costs on this fixture: the yardsticks of the GPU bars
        assert 0 < float(t["cpu::grad_global"]) <= 1e-4
        assert 0 < float(t["cpu::bf16_loss_rel"]) < 1e-2
        assert 0.99 < float(t["cpu::bf16_grad_cos"]) < 1
    return names, t


def check_oracle_small_train_fixture(spec):
    keys = spec.small_keys() if spec.small_keys else fixture_keys(spec)[1]
    x = synth.synth_images(*spec.eval_shape, seed=0)
    y = synth.synth_targets(*spec.eval_shape, seed=0)
    t = np.load(spec.file("small_train.npz"))
    _check_train(spec, t, [torch.from_numpy(t["logits0"])], *spec.O.train(spec.O.state(keys), x, y))


# ------------------------------------------------------------------------------------ the models

def _cgnet_small_keys():
    """The schema of the STAGE2_BLOCK_NUM 2 / STAGE3_BLOCK_NUM 2 model: the full one without the
    blocks stage2.1 and stage3.1 .. stage3.19."""
    return [(k, s) for k, s in fixture_keys(CGNET)[1]
            if not (k.startswith(("stage2.", "stage3.")) and int(k.split(".")[1]) >= 1)]


def _resnet_fc(key):
    return key.startswith("encoder.fc.")


def _shapes(O):
    """The fixtures' shapes as the three newer oracles name them."""
    return dict(O=O, eval_shape=(O.B, O.H, O.W), loop_shape=(O.B, O.H, O.W),
                train_shape=(O.TB, O.TH, O.TW), train_seed=getattr(O, "TRAIN_SEED", 0))


_BI, _DU = _bisenet_oracle, _dunet_oracle

# The bf16 yardsticks: the reference itself under CPU bf16 autocast on the training fixture
# (tests/_<name>_oracle.py train(autocast=True) against its float64 run; measured by
# tools/gen_golden_<name>.py, recorded in profiles/<name>.md and, from DUNet on, as `cpu::` entries
# of <name>_train.npz).  The bars are 1.3 x those distances, the ratio of the C3 / C4 bf16 bars.
BISENET = Spec(
    O=_BI, name="bisenet", model="BiSeNet", n_keys=230, n_params=13910113, min_grads=60,
    eval_shape=(_BI.B_EVAL, _BI.H, _BI.W), train_shape=(_BI.B_TRAIN, _BI.H, _BI.W),
    loop_shape=(_BI.B_TRAIN, _BI.H, _BI.W), eval_step=1, logit_steps=(2, 4, 4),
    split_logits=False, n_eval_outputs=3,
    overrides=("SOLVER.AUX", "True", "SOLVER.AUX_WEIGHT", str(_BI.AUX_WEIGHT),
               "MODEL.OUTPUT_STRIDE", "16"),
    aux_weight=_BI.AUX_WEIGHT, unused=_resnet_fc, counters_are_one=False,
    bf16=(1.424e-4, 0.999352), key_width=55, graph_indent=20)
DUNET = Spec(
    O=_DU, name="dunet", model="DUNet", n_keys=354, n_params=34209768, min_grads=150,
    eval_shape=(_DU.B, _DU.H, _DU.W), train_shape=(_DU.B, _DU.H, _DU.W),
    loop_shape=(_DU.B, _DU.H, _DU.W), second_shape=(_DU.H_ODD, _DU.W_ODD),
    logit_steps=(2, 2), split_logits=False, n_eval_outputs=2,
    overrides=("SOLVER.AUX", "True", "SOLVER.AUX_WEIGHT", str(_DU.AUX_WEIGHT),
               "MODEL.OUTPUT_STRIDE", "8"),
    aux_weight=_DU.AUX_WEIGHT, unused=_resnet_fc, counters_are_one=False,
    train_view="DUpLogitsView", bf16=(9.0115e-5, 0.999783), key_width=55, graph_indent=18)
CGNET = Spec(
    **_shapes(_cgnet_oracle), second_shape=(_cgnet_oracle.H_ODD, _cgnet_oracle.W_ODD),
    name="cgnet", model="CGNet", n_keys=499, n_params=496325, n_grads=337,
    small_overrides=tuple(_cgnet_oracle.SMALL_OVERRIDES), small_keys=_cgnet_small_keys,
    bf16=(3.7127e-4, 0.999993), bf16_tol=(1e-7, 1e-6), fused_shape=(1, 576, 584),
    key_width=45, graph_indent=18)
# (two images in the tier test: the head's level5 is a plain nn.BatchNorm2d over N pooled rows,
# which raises for N = 1 in training mode here as it does in the reference)
LEDNET = Spec(
    **_shapes(_lednet_oracle), second_shape=(_lednet_oracle.H_ODD, _lednet_oracle.W_ODD),
    name="lednet", model="LEDNet", n_keys=418, n_params=2325022, n_grads=238,
    bf16=(1.8384e-03, 0.997960), bf16_tol=(1e-7, 1e-6), fused_shape=(2, 576, 584),
    key_width=45, graph_indent=18)
ESPNETV2 = Spec(
    **_shapes(_espnetv2_oracle), second_shape=(_espnetv2_oracle.H2, _espnetv2_oracle.W2),
    name="espnetv2", model="ESPNetV2", n_keys=640, n_params=2163324, n_grads=256,
    unused=_espnetv2_oracle.unused, bf16=(8.0473e-04, 0.99999495), bf16_tol=(1e-8, 1e-8),
    head_stride=2, fused_shape=(2, 512, 528), key_width=45, graph_indent=20)
