"""Fixtures of the EDANet tests (tests/test_edanet.py, tests/test_edanet_gpu.py), generated from
the REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_edanet_oracle.py (oracle.synth seed 0, conditioned; Dropout2d at p = 0):

  tests/golden/cityscapes_edanet.yaml     configs/cityscapes_edanet.yaml of THIS repository (the
                                          reference ships no EDANet config; settings only)
  tests/golden/edanet_state_keys.json     state_dict keys / shapes / parameter count
  tests/golden/edanet_eval.npz            evaluation logits (every 2nd pixel) at 2 x 3 x 64 x 96
  tests/golden/edanet_train.npz           one training forward / backward at 4 x 3 x 128 x 192 (16 x
  tests/golden/edanet_train_logits_a.npz  24 maps at 1/8: at dilation 16 every side tap along H is
  tests/golden/edanet_train_logits_b.npz  outside): loss, logits (every 2nd pixel; images 0-1 in
                                          _a, 2-3 in _b), per-parameter gradient norms, the running
                                          statistics after the step (`stat::`) and the `cpu::`
                                          yardsticks (float32 against float64, and the restatement
                                          under CPU bfloat16 autocast against its float64 run)
  tests/golden/edanet_small_train.npz     the same step at 2 x 3 x 64 x 96: the few-sample
                                          BatchNorm path (96 rows at 1/8 resolution)

The reference raises for inputs not divisible by 8 (the stride-2 convolution rounds up, the 2 x 2
pool down, and their torch.cat fails), so there is no odd-size entry; the second evaluation size of
the GPU test, 1 x 72 x 104, is checked against the restatement.  The training inputs' seed is the
first whose float64 run keeps every ReLU input decidable in float32 (tests/_edanet_oracle.py
TRAIN_SEED; the scan is repeated here and asserted).

    python tools/gen_golden_edanet.py [--out DIR]
"""
import json
import os
import shutil

import _golden_zoo as G

YAML = "configs/cityscapes_edanet.yaml"


def main():
    import numpy as np
    import torch
    import _edanet_oracle as O
    from oracle import synth
    out = G.parse_args(__doc__).out
    # (an absolute path: the reference has no such file, the settings are this repository's)
    model, keys, sd = G.reference_model(O, os.path.join(G.ROOT, YAML))
    n_params = sum(p.numel() for p in model.parameters())
    with open(os.path.join(out, "edanet_state_keys.json"), "w") as f:
        json.dump({"config": YAML, "keys": keys, "n_params": n_params}, f)
    shutil.copyfile(os.path.join(G.ROOT, YAML), os.path.join(out, os.path.basename(YAML)))
    print("%d keys, %d parameters" % (len(keys), n_params))
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        try:
            model(synth.synth_images(1, 65, 97, seed=0))
            raise AssertionError("the reference accepted a size not divisible by 8")
        except RuntimeError as e:
            print("65 x 97 raises in the reference: %s" % str(e).splitlines()[0])
    np.savez_compressed(os.path.join(out, "edanet_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2], n_outputs=np.int64(len(ev)))
    print("eval: %d outputs, %s" % (len(ev), tuple(ev[0].shape)))
    seed = G.scan_seed(O, sd, O.min_relu_margin, O.RELU_MARGIN, "ReLU")
    # (negligible: the 42 convolution biases in front of a BatchNorm — every 1x1, every second
    # line convolution, the three down-samplers' — whose gradient is zero in exact arithmetic)
    arrs, x, y = G._train_fixture(model, sd, O.TB, O.TH, O.TW, check=True, seed=seed,
                                  negligible=1e-12)
    print("gradients in the train fixture: %d" % sum(k.startswith("gnorm::") for k in arrs))
    arrs["seed"] = np.int64(seed)
    arrs.update(G.bf16_yardstick(O, sd, x, y))
    G.save_train(out, "edanet", arrs)
    model.load_state_dict(sd)  # (the step above moved the running statistics)
    arrs, _, _ = G._train_fixture(model, sd, O.B, O.H, O.W, check=False)
    np.savez_compressed(os.path.join(out, "edanet_small_train.npz"), **arrs)
    G.assert_sizes(out, ("edanet_state_keys.json", "edanet_eval.npz", "edanet_train.npz",
                         "edanet_train_logits_a.npz", "edanet_train_logits_b.npz",
                         "edanet_small_train.npz"))


if __name__ == "__main__":
    main()
