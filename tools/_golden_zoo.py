"""What the per-model fixture generators (tools/gen_golden_<m>.py) share: the reference model with
the synthesised state, one training step through the reference's own criterion, the float32
against float64 conditioning check with the gradient acceptance rule on the reference's own run,
the input-seed scan, the bf16-autocast yardstick, and the writers.  They read the REFERENCE
(read-only, through oracle.ref_import)."""
import argparse
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parse_args(doc, leg=None):
    """--out DIR (default tests/golden) and, for a generator with a second process, its --<leg>."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"), metavar="DIR",
                    help="write the fixtures here (default: tests/golden)")
    if leg:
        ap.add_argument("--" + leg, action="store_true", help="(second process) this leg only")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    return args


def reference_model(O, yaml, overrides=()):
    """-> (the reference's model with O's synthesised state and dropout 0, keys / shapes, state)."""
    from oracle import ref_import
    model, _ = ref_import.build_reference_model(yaml, list(overrides))
    keys = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    sd = O.state([(k, tuple(s)) for k, s in keys])
    model.load_state_dict(sd)
    _no_dropout(model)
    return model, keys, sd


def _no_dropout(model):
    import torch.nn as nn
    for m in model.modules():
        if isinstance(m, (nn.Dropout, nn.Dropout2d)):
            m.p = 0.0


def write_schema(out, name, yaml, model, keys, **extra):
    """<name>_state_keys.json and the reference's config."""
    from oracle import ref_import
    n_params = sum(p.numel() for p in model.parameters())
    with open(os.path.join(out, name + "_state_keys.json"), "w") as f:
        json.dump(dict({"config": yaml, "keys": keys, "n_params": n_params}, **extra), f)
    shutil.copyfile(os.path.join(ref_import.REFERENCE_ROOT, yaml),
                    os.path.join(out, os.path.basename(yaml)))
    print("%d keys, %d parameters" % (len(keys), n_params))


def train_step(model, x, y, aux=False):
    from segmentron.solver.loss import MixSoftmaxCrossEntropyLoss
    model.train()
    model.zero_grad()
    outs = model(x)
    loss = MixSoftmaxCrossEntropyLoss(aux=aux, aux_weight=0.4, ignore_index=-1)(outs, y)["loss"]
    loss.backward()
    return loss, outs


def grads_of(model):
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def stats_of(model):
    return {"stat::" + k: v.numpy() for k, v in model.state_dict().items()
            if "running_" in k or k.endswith("num_batches_tracked")}


def _train_fixture(model, sd, b, h, w, check, seed=0, unused=None, negligible=None):
    """-> arrays of one training step of the reference (float32, checked against its float64
    run) on synth images / targets of b x 3 x h x w.  `unused(key)`: the parameters that must have
    no gradient.  `negligible`: a gradient whose float64 norm is below this share of the whole is
    zero in exact arithmetic and has no relative error (the global error covers it); with it the
    tensors beyond 1e-3 are listed."""
    import numpy as np
    from oracle import synth
    x = synth.synth_images(b, h, w, seed=seed)
    y = synth.synth_targets(b, h, w, seed=seed)
    model.double()
    model.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    loss64, outs64 = train_step(model, x.double(), y)
    g64 = grads_of(model)
    model.float()
    model.load_state_dict(sd)
    loss, outs = train_step(model, x, y)
    g32 = grads_of(model)
    used = set(k for k, _ in model.named_parameters() if not (unused and unused(k)))
    assert set(g32) == used, ("the parameters with a gradient are not the used ones",
                              sorted(used ^ set(g32)))
    err = {k: (g32[k].double() - g64[k]).norm().item() for k in g64}
    nrm = {k: g64[k].norm().item() for k in g64}
    num = sum(e * e for e in err.values()) ** 0.5
    den = sum(n * n for n in nrm.values()) ** 0.5
    worst = max(err[k] / max(nrm[k], 1e-30) for k in g64)
    lerr = (outs[0].double() - outs64[0]).abs().max().item() / outs64[0].abs().max().item()
    print("%d x %d x %d float32 vs float64: loss %.2e, logits %.2e, gradient global %.2e, worst "
          "tensor %.2e" % (b, h, w, abs(loss.item() - loss64.item()) / loss64.item(), lerr,
                           num / den, worst))
    if check:
        # the acceptance rule of tests/_zoo.py check_gradients on the reference's own float32 run
        # with the margin that rule grants the device (err_cpu32 := 0)
        over = [k for k in g64 if err[k] > 1e-3 * nrm[k]
                and (negligible is None or nrm[k] > negligible * den)]
        print("tensors beyond 1e-3 relative in the reference's float32 run: %d of %d"
              % (len(over), len(g64)))
        if negligible is not None:
            for k in over:
                print("  %s: error %.3e, norm %.3e (global norm %.3e)" % (k, err[k], nrm[k], den))
        assert num / den <= 1e-4, "fixture is not well conditioned: re-condition the state"
        assert len(over) <= 0.1 * len(g64) and all(err[k] <= 3e-2 * nrm[k] for k in over), \
            "fixture is not well conditioned: re-condition the state"
    arrs = {"loss": np.float64(loss.item()), "cpu::grad_global": np.float64(num / den),
            "logits0": outs[0].detach().numpy()[..., ::2, ::2]}
    for k, g in g32.items():
        arrs["gnorm::" + k] = np.float64(g.double().norm().item())
        arrs["gerr32::" + k] = np.float64(err[k])
    arrs.update(stats_of(model))
    print("training step: loss %.6f" % loss.item())
    return arrs, x, y


def scan_seed(O, sd, margin_of, margin, what):
    """-> the first synth seed of the training fixture's inputs whose float64 run has no `what`
    input that float32 cannot resolve: O.TRAIN_SEED, or the oracle's constant is stale."""
    from oracle import synth
    seed = 0
    while True:
        m = margin_of(sd, synth.synth_images(O.TB, O.TH, O.TW, seed=seed))
        print("seed %d: smallest relative %s margin of the float64 run %.2e" % (seed, what, m))
        if m >= margin:
            break
        seed += 1
    assert seed == O.TRAIN_SEED, (seed, O.TRAIN_SEED)
    return seed


def bf16_yardstick(O, sd, x, y):
    """-> the `cpu::` entries behind the bf16 bars: loss distance and gradient cosine of the
    float64-checked restatement under CPU bfloat16 autocast against its float64 run."""
    import numpy as np
    import torch
    l64, _, og64, _ = O.train(sd, x, y, dtype=torch.float64)
    lbf, _, ogbf, _ = O.train(sd, x, y, autocast=True)
    dot = sum((ogbf[k].double() * og64[k]).sum().item() for k in og64)
    na = sum(ogbf[k].double().pow(2).sum().item() for k in og64) ** 0.5
    nb = sum(og64[k].pow(2).sum().item() for k in og64) ** 0.5
    bf_loss, bf_cos = abs(lbf - l64) / abs(l64), dot / (na * nb)
    print("CPU bf16 autocast vs float64: loss %.4e relative, gradient cosine %.6f"
          % (bf_loss, bf_cos))
    return {"cpu::bf16_loss_rel": np.float64(bf_loss), "cpu::bf16_grad_cos": np.float64(bf_cos)}


def save_train(out, name, arrs):
    """<name>_train.npz and its logits, images 0-1 in _a and 2-3 in _b (1 MiB per file)."""
    import numpy as np
    logits = arrs.pop("logits0")
    half = logits.shape[0] // 2
    np.savez_compressed(os.path.join(out, name + "_train.npz"), **arrs)
    np.savez_compressed(os.path.join(out, name + "_train_logits_a.npz"), logits0=logits[:half])
    np.savez_compressed(os.path.join(out, name + "_train_logits_b.npz"), logits0=logits[half:])


def assert_sizes(out, files):
    for f in files:
        size = os.path.getsize(os.path.join(out, f))
        print("%s: %d bytes" % (f, size))
        assert size < (1 << 20), f
