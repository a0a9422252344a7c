"""Fixtures of the LEDNet tests (tests/test_lednet.py, tests/test_lednet_gpu.py), generated from
the REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_lednet_oracle.py (oracle.synth seed 0, conditioned; the model has no dropout):

  tests/golden/cityscapes_lednet.yaml     the reference's config (settings only)
  tests/golden/lednet_state_keys.json     state_dict keys / shapes / parameter count / decoder list
  tests/golden/lednet_eval.npz            evaluation logits (every 2nd pixel) at 2 x 3 x 64 x 96 and
                                          the output SHAPE for 1 x 3 x 65 x 97
  tests/golden/lednet_train.npz           one training forward / backward at 4 x 3 x 128 x 192 (the
  tests/golden/lednet_train_logits_a.npz  1/8-resolution BatchNorms see 1536 rows): loss, logits
  tests/golden/lednet_train_logits_b.npz  (every 2nd pixel; images 0-1 in _a, 2-3 in _b: 1 MiB per
                                          committed file), per-parameter gradient norms, the running
                                          statistics after the step (`stat::`), and what the
                                          reference's own arithmetic costs on this input (`cpu::`):
                                          float32 against float64 per tensor, and loss distance /
                                          gradient cosine of the float64-checked restatement under
                                          CPU bfloat16 autocast
  tests/golden/lednet_small_train.npz     the same step at 2 x 3 x 64 x 96: the few-sample
                                          BatchNorm path (192 rows at 1/8 resolution)

The training fixture's images and targets are synth seed 12: the first seed whose float64 run
keeps every BatchNorm + ReLU input at least 16 * 2^-24 (relative) away from the kink, so that the
ReLU masks, hence the gradients, are decidable in float32 at all (tests/_lednet_oracle.py
TRAIN_SEED; the scan is repeated here and asserted).

Before anything is written the float32 run is compared with the reference in float64: the float32
run must itself satisfy the gradient acceptance rule of tests/_zoo.py (check_gradients) with the
margin that rule grants the device (err_cpu32 := 0): global error <= 1e-4, at most 10 % of the
tensors beyond 1e-3 relative and none beyond 3e-2.

    python tools/gen_golden_lednet.py [--out DIR]
"""
import os

import _golden_zoo as G

YAML = "configs/cityscapes_lednet.yaml"


def main():
    import numpy as np
    import torch
    import _lednet_oracle as O
    from oracle import synth
    out = G.parse_args(__doc__).out
    model, keys, sd = G.reference_model(O, YAML)
    G.write_schema(out, "lednet", YAML, model, keys, decoder=list(model.decoder))
    # evaluation, running statistics as synthesised
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        odd = model(synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
    np.savez_compressed(os.path.join(out, "lednet_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2],
                        shape_odd=np.array(odd[0].shape, dtype=np.int64),
                        n_outputs=np.int64(len(ev)))
    print("eval: %d outputs, %s; odd input -> %s" % (len(ev), tuple(ev[0].shape),
                                                      tuple(odd[0].shape)))
    # the training fixture's inputs: the first seed whose float64 run has no ReLU input that
    # float32 cannot resolve (see tests/_lednet_oracle.py TRAIN_SEED)
    seed = G.scan_seed(O, sd, O.min_relu_margin, O.RELU_MARGIN, "ReLU")
    arrs, x, y = G._train_fixture(model, sd, O.TB, O.TH, O.TW, check=True, seed=seed)
    arrs["seed"] = np.int64(seed)
    arrs.update(G.bf16_yardstick(O, sd, x, y))
    G.save_train(out, "lednet", arrs)
    model.load_state_dict(sd)  # (the step above moved the running statistics)
    arrs, _, _ = G._train_fixture(model, sd, O.B, O.H, O.W, check=False)
    np.savez_compressed(os.path.join(out, "lednet_small_train.npz"), **arrs)
    G.assert_sizes(out, ("lednet_state_keys.json", "lednet_eval.npz", "lednet_train.npz",
                         "lednet_train_logits_a.npz", "lednet_train_logits_b.npz",
                         "lednet_small_train.npz"))


if __name__ == "__main__":
    main()
