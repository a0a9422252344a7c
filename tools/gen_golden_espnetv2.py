"""Fixtures of the ESPNetV2 tests (tests/test_espnetv2.py, tests/test_espnetv2_gpu.py), generated
from the REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_espnetv2_oracle.py (oracle.synth seed 0, conditioned; PReLU slopes in [0.05, 0.45];
dropout 0):

  tests/golden/cityscapes_espnetv2.yaml     the reference's config (settings only)
  tests/golden/espnetv2_state_keys.json     state_dict keys / shapes / parameter count / exclusive
  tests/golden/espnetv2_eval.npz            evaluation logits (every 2nd pixel) at 2 x 3 x 64 x 96
                                            and at 1 x 3 x 48 x 80
  tests/golden/espnetv2_train.npz           one training forward / backward at 4 x 3 x 128 x 192
  tests/golden/espnetv2_train_logits_a.npz  (the 1/8-resolution BatchNorms see 1536 rows, the 1/16
  tests/golden/espnetv2_train_logits_b.npz  ones 384): loss, logits (every 2nd pixel; images 0-1 in
                                            _a, 2-3 in _b: 1 MiB per committed file), per-parameter
                                            gradient norms (the never-used level5* / fc have none),
                                            the running statistics after the step (`stat::`), and
                                            what the reference's own arithmetic costs on this input
                                            (`cpu::`): float32 against float64 per tensor, and loss
                                            distance / gradient cosine of the float64-checked
                                            restatement under CPU bfloat16 autocast
  tests/golden/espnetv2_small_train.npz     the same step at 2 x 3 x 64 x 96: the few-sample
                                            BatchNorm path

The training fixture's images and targets are the first synth seed whose float64 run keeps every
PReLU input at least 16 * 2^-24 away from the kink, relative to the magnitudes added to form it, so
that the PReLU masks, hence the gradients, are decidable in float32 at all
(tests/_espnetv2_oracle.py TRAIN_SEED; the scan is repeated here and asserted).

Before anything is written the float32 run is compared with the reference in float64: the float32
run must itself satisfy the gradient acceptance rule of tests/test_espnetv2_gpu.py with the margin
that rule grants the device (err_cpu32 := 0): global error <= 1e-4, at most 10 % of the tensors
beyond 1e-3 relative and none beyond 3e-2.

    python tools/gen_golden_espnetv2.py
"""
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = "configs/cityscapes_espnetv2.yaml"


def _no_dropout(model):
    import torch.nn as nn
    for m in model.modules():
        if isinstance(m, (nn.Dropout, nn.Dropout2d)):
            m.p = 0.0


def _train_step(model, x, y):
    from segmentron.solver.loss import MixSoftmaxCrossEntropyLoss
    model.train()
    model.zero_grad()
    outs = model(x)
    loss = MixSoftmaxCrossEntropyLoss(aux=False, ignore_index=-1)(outs, y)["loss"]
    loss.backward()
    return loss, outs


def _train_fixture(model, sd, b, h, w, check, seed=0):
    """-> arrays of one training step of the reference (float32, checked against its float64
    run) on synth images / targets of b x 3 x h x w."""
    import numpy as np
    import torch
    from oracle import synth
    x = synth.synth_images(b, h, w, seed=seed)
    y = synth.synth_targets(b, h, w, seed=seed)
    model.double()
    model.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    loss64, outs64 = _train_step(model, x.double(), y)
    g64 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.float()
    model.load_state_dict(sd)
    loss, outs = _train_step(model, x, y)
    g32 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    import _espnetv2_oracle as O
    used = set(k for k, _ in model.named_parameters() if not O.unused(k))
    assert set(g32) == used, ("the parameters with a gradient are not all but O.UNUSED",
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
        # the acceptance rule of tests/test_espnetv2_gpu.py on the reference's own float32 run
        # (a gradient whose float64 norm is below 1e-12 of the whole is zero in exact arithmetic —
        # here the conv_1x1_exp.bn.bias of level4.2-6, whose PReLU inputs all lie on one side —
        # and has no relative error; the global error covers it)
        over = [k for k in g64 if err[k] > 1e-3 * nrm[k] and nrm[k] > 1e-12 * den]
        print("tensors beyond 1e-3 relative in the reference's float32 run: %d of %d"
              % (len(over), len(g64)))
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
    for k, v in model.state_dict().items():
        if "running_" in k or k.endswith("num_batches_tracked"):
            arrs["stat::" + k] = v.numpy()
    print("training step: loss %.6f" % loss.item())
    return arrs, x, y


def main():
    import numpy as np
    import torch
    import _espnetv2_oracle as O
    from oracle import ref_import, synth
    model, _ = ref_import.build_reference_model(YAML, [])
    keys = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    sd = O.state([(k, tuple(s)) for k, s in keys])
    model.load_state_dict(sd)
    _no_dropout(model)
    n_params = sum(p.numel() for p in model.parameters())
    with open(os.path.join(GOLDEN, "espnetv2_state_keys.json"), "w") as f:
        json.dump({"config": YAML, "keys": keys, "n_params": n_params,
                   "exclusive": list(model.exclusive)}, f)
    shutil.copyfile(os.path.join(ref_import.REFERENCE_ROOT, YAML),
                    os.path.join(GOLDEN, os.path.basename(YAML)))
    print("%d keys, %d parameters" % (len(keys), n_params))
    # evaluation, running statistics as synthesised
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        ev2 = model(synth.synth_images(1, O.H2, O.W2, seed=0))
    np.savez_compressed(os.path.join(GOLDEN, "espnetv2_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2],
                        logits0_second=ev2[0].numpy()[..., ::2, ::2],
                        n_outputs=np.int64(len(ev)))
    print("eval: %d outputs, %s; second shape -> %s" % (len(ev), tuple(ev[0].shape),
                                                         tuple(ev2[0].shape)))
    # the training fixture's inputs: the first seed whose float64 run has no PReLU input that
    # float32 cannot resolve (see tests/_espnetv2_oracle.py TRAIN_SEED)
    seed = 0
    while True:
        m = O.min_prelu_margin(sd, synth.synth_images(O.TB, O.TH, O.TW, seed=seed))
        print("seed %d: smallest relative PReLU margin of the float64 run %.2e" % (seed, m))
        if m >= O.PRELU_MARGIN:
            break
        seed += 1
    assert seed == O.TRAIN_SEED, (seed, O.TRAIN_SEED)
    arrs, x, y = _train_fixture(model, sd, O.TB, O.TH, O.TW, check=True, seed=seed)
    arrs["seed"] = np.int64(seed)
    # the float64-checked restatement under CPU bfloat16 autocast: the bf16 bars
    l64, _, og64, _ = O.train(sd, x, y, dtype=torch.float64)
    lbf, _, ogbf, _ = O.train(sd, x, y, autocast=True)
    dot = sum((ogbf[k].double() * og64[k]).sum().item() for k in og64)
    na = sum(ogbf[k].double().pow(2).sum().item() for k in og64) ** 0.5
    nb = sum(og64[k].pow(2).sum().item() for k in og64) ** 0.5
    bf_loss, bf_cos = abs(lbf - l64) / abs(l64), dot / (na * nb)
    print("CPU bf16 autocast vs float64: loss %.4e relative, gradient cosine %.6f"
          % (bf_loss, bf_cos))
    arrs["cpu::bf16_loss_rel"] = np.float64(bf_loss)
    arrs["cpu::bf16_grad_cos"] = np.float64(bf_cos)
    logits = arrs.pop("logits0")
    half = logits.shape[0] // 2
    np.savez_compressed(os.path.join(GOLDEN, "espnetv2_train.npz"), **arrs)
    np.savez_compressed(os.path.join(GOLDEN, "espnetv2_train_logits_a.npz"), logits0=logits[:half])
    np.savez_compressed(os.path.join(GOLDEN, "espnetv2_train_logits_b.npz"), logits0=logits[half:])
    model.load_state_dict(sd)  # (the step above moved the running statistics)
    arrs, _, _ = _train_fixture(model, sd, O.B, O.H, O.W, check=False)
    np.savez_compressed(os.path.join(GOLDEN, "espnetv2_small_train.npz"), **arrs)
    for f in ("espnetv2_state_keys.json", "espnetv2_eval.npz", "espnetv2_train.npz",
              "espnetv2_train_logits_a.npz", "espnetv2_train_logits_b.npz", "espnetv2_small_train.npz"):
        size = os.path.getsize(os.path.join(GOLDEN, f))
        print("%s: %d bytes" % (f, size))
        assert size < (1 << 20), f


if __name__ == "__main__":
    main()
