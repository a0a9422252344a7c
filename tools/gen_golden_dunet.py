"""Fixtures of the DUNet tests (tests/test_dunet.py, tests/test_dunet_gpu.py), generated from the
REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_dunet_oracle.py (oracle.synth seed 0, conditioned):

  tests/golden/dunet_state_keys.json    state_dict keys / shapes / parameter count / decoder list
                                        of the reference's DUNet (resnet50, OS 8, SOLVER.AUX True)
  tests/golden/cityscapes_dunet.yaml    the reference's config (settings only)
  tests/golden/dunet_eval.npz           evaluation logits (main head, every 2nd pixel) at
                                        2 x 3 x 64 x 96 and the output SHAPE for 1 x 3 x 65 x 97
  tests/golden/dunet_train.npz          one training forward / backward at 2 x 3 x 64 x 96 with
                                        MixSoftmaxCrossEntropyLoss (aux weight 0.4), dropout 0:
                                        loss, both logits (every 2nd pixel), per-parameter gradient
                                        norms, the running statistics after the step (`stat::`),
                                        and what the reference's own arithmetic costs on this
                                        input (`cpu::`): float32 against float64 per tensor, and
                                        loss / gradient cosine of the float64-checked restatement
                                        under CPU bfloat16 autocast

  tests/golden/dunet_os16_eval.npz      evaluation logits of both heads at OUTPUT_STRIDE 16,
                                        2 x 3 x 64 x 96: FeatureFused's resize of c2 is real (it
                                        SHRINKS c2 to c4's size) and the output is 8 x c4 = half the
                                        input's size

Before anything is written the float32 run is compared with the reference in float64: global
gradient error <= 1e-4, worst tensor <= 5e-4, and the float32 run must itself satisfy the
per-tensor acceptance rule of tests/_zoo.py (check_gradients) with the margin that rule grants the
device.

    python tools/gen_golden_dunet.py [--out DIR]     (the OS 16 leg runs in a second process: the
                                                      reference's cfg is a frozen per-process
                                                      singleton)
"""
import os
import subprocess
import sys

import _golden_zoo as G

YAML = "configs/cityscapes_dunet.yaml"


def main():
    import numpy as np
    import torch
    import _dunet_oracle as O
    from oracle import synth
    args = G.parse_args(__doc__, leg="os16")
    out = args.out
    over = ["SOLVER.AUX", "True"] + (["MODEL.OUTPUT_STRIDE", "16"] if args.os16 else [])
    model, keys, sd = G.reference_model(O, YAML, over)
    if args.os16:
        model.eval()
        with torch.no_grad():
            ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        np.savez_compressed(os.path.join(out, "dunet_os16_eval.npz"),
                            logits0=ev[0].numpy(), logits1=ev[1].numpy())
        print("OS 16 eval: %s" % (tuple(ev[0].shape),))
        return
    G.write_schema(out, "dunet", YAML, model, keys, decoder=list(model.decoder))
    # evaluation, running statistics as synthesised
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        odd = model(synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
    np.savez_compressed(os.path.join(out, "dunet_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2],
                        shape_odd=np.array(odd[0].shape, dtype=np.int64),
                        n_outputs=np.int64(len(ev)))
    print("eval: %d outputs, %s; odd input -> %s" % (len(ev), tuple(ev[0].shape),
                                                      tuple(odd[0].shape)))
    # one training step: float64 first (the yardstick of the float32 run), then float32
    x = synth.synth_images(O.B, O.H, O.W, seed=0)
    y = synth.synth_targets(O.B, O.H, O.W, seed=0)
    print("targets: %.1f %% ignored" % (100.0 * (y == -1).float().mean().item()))
    model.double()
    loss64, outs64 = G.train_step(model, x.double(), y, aux=True)
    g64 = G.grads_of(model)
    model.float()
    model.load_state_dict(sd)
    loss, outs = G.train_step(model, x, y, aux=True)
    g32 = G.grads_of(model)
    err = {k: (g32[k].double() - g64[k]).norm().item() for k in g64}
    nrm = {k: g64[k].norm().item() for k in g64}
    num = sum(e * e for e in err.values()) ** 0.5
    den = sum(n * n for n in nrm.values()) ** 0.5
    # (a gradient that is zero in exact arithmetic has no relative error: encoder.bn1.bias, whose
    # shift passes the ReLU and the max pool of this conditioned state unclipped and is removed by
    # the BatchNorms behind layer1's 1x1 convolutions, is measured against the global norm)
    dead = [k for k in g64 if nrm[k] <= 1e-9 * den]
    print("gradients that vanish in float64: %s" % dead)
    assert len(dead) <= 1 and all(err[k] <= 1e-6 * den for k in dead)
    worst = max(err[k] / nrm[k] for k in g64 if k not in dead)
    lerr = max((a.double() - b).abs().max().item() / b.abs().max().item()
               for a, b in zip(outs, outs64))
    print("float32 vs float64: loss %.2e, logits %.2e, gradient global %.2e, worst tensor %.2e"
          % (abs(loss.item() - loss64.item()) / loss64.item(), lerr, num / den, worst))
    assert num / den <= 1e-4 and worst <= 5e-4, "fixture is not well conditioned"
    # the acceptance rule of tests/_zoo.py check_gradients, applied to the reference's own float32
    # run with err_cpu32 := 0 (the strictest reading): at most 10 % of the tensors beyond 1e-3
    over = [k for k in g64 if err[k] > 1e-3 * nrm[k]]
    print("tensors beyond 1e-3 relative in the reference's float32 run: %d of %d"
          % (len(over), len(g64)))
    assert len(over) <= 0.1 * len(g64), "choose another seed"
    arrs = {"loss": np.float64(loss.item()), "cpu::grad_global": np.float64(num / den)}
    arrs.update(G.bf16_yardstick(O, sd, x, y))
    for i, o in enumerate(outs):
        arrs["logits%d" % i] = o.detach().numpy()[..., ::2, ::2]  # (1 MiB per committed file)
    for k, g in g32.items():
        arrs["gnorm::" + k] = np.float64(g.double().norm().item())
        arrs["gerr32::" + k] = np.float64(err[k])
    arrs.update(G.stats_of(model))
    np.savez_compressed(os.path.join(out, "dunet_train.npz"), **arrs)
    print("training step: loss %.6f" % loss.item())
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--os16", "--out", out])
    G.assert_sizes(out, ("dunet_state_keys.json", "dunet_eval.npz", "dunet_train.npz",
                         "dunet_os16_eval.npz"))


if __name__ == "__main__":
    main()
