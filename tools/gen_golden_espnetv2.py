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
run must itself satisfy the gradient acceptance rule of tests/_zoo.py (check_gradients) with the
margin that rule grants the device (err_cpu32 := 0): global error <= 1e-4, at most 10 % of the
tensors beyond 1e-3 relative and none beyond 3e-2.

    python tools/gen_golden_espnetv2.py [--out DIR]
"""
import os

import _golden_zoo as G

YAML = "configs/cityscapes_espnetv2.yaml"


def main():
    import numpy as np
    import torch
    import _espnetv2_oracle as O
    from oracle import synth
    out = G.parse_args(__doc__).out
    model, keys, sd = G.reference_model(O, YAML)
    G.write_schema(out, "espnetv2", YAML, model, keys, exclusive=list(model.exclusive))
    # evaluation, running statistics as synthesised
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        ev2 = model(synth.synth_images(1, O.H2, O.W2, seed=0))
    np.savez_compressed(os.path.join(out, "espnetv2_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2],
                        logits0_second=ev2[0].numpy()[..., ::2, ::2],
                        n_outputs=np.int64(len(ev)))
    print("eval: %d outputs, %s; second shape -> %s" % (len(ev), tuple(ev[0].shape),
                                                         tuple(ev2[0].shape)))
    # the training fixture's inputs: the first seed whose float64 run has no PReLU input that
    # float32 cannot resolve (see tests/_espnetv2_oracle.py TRAIN_SEED)
    seed = G.scan_seed(O, sd, O.min_prelu_margin, O.PRELU_MARGIN, "PReLU")
    # (negligible: the conv_1x1_exp.bn.bias of level4.2-6, whose PReLU inputs all lie on one side)
    arrs, x, y = G._train_fixture(model, sd, O.TB, O.TH, O.TW, check=True, seed=seed,
                                  unused=O.unused, negligible=1e-12)
    arrs["seed"] = np.int64(seed)
    arrs.update(G.bf16_yardstick(O, sd, x, y))
    G.save_train(out, "espnetv2", arrs)
    model.load_state_dict(sd)  # (the step above moved the running statistics)
    arrs, _, _ = G._train_fixture(model, sd, O.B, O.H, O.W, check=False, unused=O.unused)
    np.savez_compressed(os.path.join(out, "espnetv2_small_train.npz"), **arrs)
    G.assert_sizes(out, ("espnetv2_state_keys.json", "espnetv2_eval.npz", "espnetv2_train.npz",
                         "espnetv2_train_logits_a.npz", "espnetv2_train_logits_b.npz",
                         "espnetv2_small_train.npz"))


if __name__ == "__main__":
    main()
