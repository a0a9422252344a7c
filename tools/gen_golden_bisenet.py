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

    python tools/gen_golden_bisenet.py [--out DIR]   (the OS 32 leg runs in a second process: the
                                                      reference's cfg is a frozen per-process
                                                      singleton)
"""
import os
import subprocess
import sys

import _golden_zoo as G

YAML = "configs/cityscapes_bisenet.yaml"


def main():
    import numpy as np
    import torch
    import _bisenet_oracle as O
    from oracle import synth
    args = G.parse_args(__doc__, leg="os32")
    out = args.out
    over = ["MODEL.OUTPUT_STRIDE", "32", "SOLVER.AUX", "False"] if args.os32 \
        else ["SOLVER.AUX", "True"]
    model, keys, sd = G.reference_model(O, YAML, over)
    if args.os32:
        x = synth.synth_images(O.B_TRAIN, O.H32, O.W32, seed=0)
        y = synth.synth_targets(O.B_TRAIN, O.H32, O.W32, seed=0)
        loss, outs = G.train_step(model, x, y, aux=False)
        np.savez_compressed(os.path.join(out, "bisenet_os32_train.npz"),
                            loss=np.float64(loss.item()),
                            logits0=outs[0].detach().numpy()[..., ::2, ::2])
        print("OS 32: loss %.6f" % loss.item())
        return
    G.write_schema(out, "bisenet", YAML, model, keys)
    # evaluation, running statistics as synthesised
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B_EVAL, O.H, O.W, seed=0))
    np.savez_compressed(os.path.join(out, "bisenet_eval.npz"), logits0=ev[0].numpy())
    # one training step: float64 first (the yardstick of the float32 run), then float32
    x = synth.synth_images(O.B_TRAIN, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B_TRAIN, O.H, O.W, seed=0)
    model.double()
    loss64, outs64 = G.train_step(model, x.double(), y, aux=True)
    g64 = G.grads_of(model)
    model.float()
    model.load_state_dict(sd)
    loss, outs = G.train_step(model, x, y, aux=True)
    g32 = G.grads_of(model)
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
    arrs.update(G.stats_of(model))
    np.savez_compressed(os.path.join(out, "bisenet_train.npz"), **arrs)
    print("training step: loss %.6f" % loss.item())
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--os32", "--out", out])


if __name__ == "__main__":
    main()
