"""Fixtures of the BiSeNet tests (tests/test_bisenet.py, tests/test_bisenet_gpu.py), generated from
the REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_bisenet_oracle.py (oracle.synth seed 0, conditioned):

  tests/golden/bisenet_state_keys.json    state_dict keys / shapes / parameter count of the
                                          reference's BiSeNet (resnet18, OS 16, SOLVER.AUX True)
  tests/golden/cityscapes_bisenet.yaml    the reference's config (settings only)
  tests/golden/bisenet_eval.npz           evaluation logits (main head) at 2 x 3 x 65 x 97
  tests/golden/bisenet_train.npz          one training forward / backward at 4 x 3 x 65 x 97 with
                                          MixSoftmaxCrossEntropyLoss (aux weight 0.4), dropout 0:
                                          loss, the three logits (every 2nd / 4th / 4th pixel),
                                          per-parameter
                                          gradient norms,
                                          the running statistics after the step (`stat::`)
  tests/golden/bisenet_os32_train.npz     the same at OUTPUT_STRIDE 32, AUX False, 4 x 3 x 64 x 96:
                                          loss and main logits (the inter-stage resize is real)

The training batch is 4: the attention BatchNorms normalise N values per channel, and with N = 2
the output is the sign of a difference.  Before anything is written the float32 run is compared
with the reference in float64: global gradient error <= 1e-4, worst tensor <= 5e-4.

    python tools/gen_golden_bisenet.py          (the OS 32 leg runs in a second process: the
                                                 reference's cfg is a frozen per-process singleton)
"""
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = "configs/cityscapes_bisenet.yaml"


def _no_dropout(model):
    import torch.nn as nn
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0


def _train_step(model, x, y, aux):
    from segmentron.solver.loss import MixSoftmaxCrossEntropyLoss
    model.train()
    model.zero_grad()
    outs = model(x)
    loss = MixSoftmaxCrossEntropyLoss(aux=aux, aux_weight=0.4, ignore_index=-1)(outs, y)["loss"]
    loss.backward()
    return loss, outs


def main(os32=False):
    import numpy as np
    import torch
    import _bisenet_oracle as O
    from oracle import ref_import, synth
    over = ["MODEL.OUTPUT_STRIDE", "32", "SOLVER.AUX", "False"] if os32 else ["SOLVER.AUX", "True"]
    model, _ = ref_import.build_reference_model(YAML, over)
    keys = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    sd = O.state([(k, tuple(s)) for k, s in keys])
    model.load_state_dict(sd)
    _no_dropout(model)
    if os32:
        x = synth.synth_images(O.B_TRAIN, O.H32, O.W32, seed=0)
        y = synth.synth_targets(O.B_TRAIN, O.H32, O.W32, seed=0)
        loss, outs = _train_step(model, x, y, aux=False)
        np.savez_compressed(os.path.join(GOLDEN, "bisenet_os32_train.npz"),
                            loss=np.float64(loss.item()),
                            logits0=outs[0].detach().numpy()[..., ::2, ::2])
        print("OS 32: loss %.6f" % loss.item())
        return
    n_params = sum(p.numel() for p in model.parameters())
    with open(os.path.join(GOLDEN, "bisenet_state_keys.json"), "w") as f:
        json.dump({"config": YAML, "keys": keys, "n_params": n_params}, f)
    shutil.copyfile(os.path.join(ref_import.REFERENCE_ROOT, YAML),
                    os.path.join(GOLDEN, os.path.basename(YAML)))
    print("%d keys, %d parameters" % (len(keys), n_params))
    # evaluation, running statistics as synthesised
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B_EVAL, O.H, O.W, seed=0))
    np.savez_compressed(os.path.join(GOLDEN, "bisenet_eval.npz"), logits0=ev[0].numpy())
    # one training step: float64 first (the yardstick of the float32 run), then float32
    x = synth.synth_images(O.B_TRAIN, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B_TRAIN, O.H, O.W, seed=0)
    model.double()
    loss64, outs64 = _train_step(model, x.double(), y, aux=True)
    g64 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.float()
    model.load_state_dict(sd)
    loss, outs = _train_step(model, x, y, aux=True)
    g32 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    num = sum((g32[k].double() - g64[k]).pow(2).sum().item() for k in g64) ** 0.5
    den = sum(g64[k].pow(2).sum().item() for k in g64) ** 0.5
    worst = max((g32[k].double() - g64[k]).norm().item() / max(g64[k].norm().item(), 1e-30)
                for k in g64)
    lerr = max((a.double() - b).abs().max().item() / b.abs().max().item()
               for a, b in zip(outs, outs64))
    print("float32 vs float64: loss %.2e, logits %.2e, gradient global %.2e, worst tensor %.2e"
          % (abs(loss.item() - loss64.item()) / loss64.item(), lerr, num / den, worst))
    assert num / den <= 1e-4 and worst <= 5e-4, "fixture is not well conditioned"
    arrs = {"loss": np.float64(loss.item())}
    for i, o in enumerate(outs):
        step = 2 if i == 0 else 4  # (1 MiB per committed file)
        arrs["logits%d" % i] = o.detach().numpy()[..., ::step, ::step]
    for k, g in g32.items():
        arrs["gnorm::" + k] = np.float64(g.double().norm().item())
    for k, v in model.state_dict().items():
        if "running_" in k or k.endswith("num_batches_tracked"):
            arrs["stat::" + k] = v.numpy()
    np.savez_compressed(os.path.join(GOLDEN, "bisenet_train.npz"), **arrs)
    print("training step: loss %.6f" % loss.item())
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--os32"])


if __name__ == "__main__":
    main(os32="--os32" in sys.argv[1:])
