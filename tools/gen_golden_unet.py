"""Fixtures of the UNet tests (tests/test_unet.py, tests/test_unet_gpu.py), generated from the
REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_unet_oracle.py (oracle.synth seed 0, conditioned):

  tests/golden/cityscapes_unet.yaml     the reference's config (settings only)
  tests/golden/unet_state_keys.json     state_dict keys / shapes / parameter count
  tests/golden/unet_eval.npz            evaluation logits (every 2nd pixel) at 2 x 3 x 64 x 96 (maps
                                        down to 4 x 6) and the output shape at 1 x 3 x 70 x 97 (the
                                        decoder pads one row at the 35- and 17-row levels and one
                                        column at the top level)
  tests/golden/unet_train.npz           one training forward / backward at 4 x 3 x 64 x 96 (24576 /
  tests/golden/unet_train_logits_a.npz  6144 / 1536 rows per BatchNorm at levels 0-2, the plain path;
  tests/golden/unet_train_logits_b.npz  384 / 96 at levels 3-4, the few-sample path): loss, logits
                                        (every 2nd pixel; images 0-1 in _a, 2-3 in _b), per-parameter
                                        gradient norms, the running statistics after the step
                                        (`stat::`) and the `cpu::` yardsticks (float32 against
                                        float64, and the restatement under CPU bfloat16 autocast
                                        against its float64 run)
  tests/golden/unet_small_train.npz     the same step at 2 x 3 x 64 x 96: levels 2-4 on the
                                        few-sample path

The training inputs' seed is the first whose float64 run keeps every ReLU input and every 2x2
max-pool window with a positive winner decidable in float32 (tests/_unet_oracle.py TRAIN_SEED; the
scan is repeated here and asserted).

    python tools/gen_golden_unet.py [--out DIR]
"""
import os

import _golden_zoo as G

YAML = "configs/cityscapes_unet.yaml"


def main():
    import numpy as np
    import torch
    import _unet_oracle as O
    from oracle import synth
    out = G.parse_args(__doc__).out
    model, keys, sd = G.reference_model(O, YAML)
    G.write_schema(out, "unet", YAML, model, keys)
    print("decoder: %s" % (model.decoder,))
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        odd = model(synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
    np.savez_compressed(os.path.join(out, "unet_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2], n_outputs=np.int64(len(ev)),
                        shape_odd=np.array(odd[0].shape))
    print("eval: %d outputs, %s; %d x %d -> %s" % (len(ev), tuple(ev[0].shape), O.H_ODD, O.W_ODD,
                                                   tuple(odd[0].shape)))
    seed = G.scan_seed(O, sd, O.min_relu_margin, O.RELU_MARGIN, "ReLU / max-pool")
    # (negligible: the biases of the convolutions in front of a training-mode BatchNorm, which
    # removes any constant: their gradient is zero in exact arithmetic)
    arrs, x, y = G._train_fixture(model, sd, O.TB, O.TH, O.TW, check=True, seed=seed,
                                  negligible=1e-12)
    print("gradients in the train fixture: %d" % sum(k.startswith("gnorm::") for k in arrs))
    arrs["seed"] = np.int64(seed)
    arrs.update(G.bf16_yardstick(O, sd, x, y))
    G.save_train(out, "unet", arrs)
    model.load_state_dict(sd)  # (the step above moved the running statistics)
    arrs, _, _ = G._train_fixture(model, sd, O.B, O.H, O.W, check=False)
    np.savez_compressed(os.path.join(out, "unet_small_train.npz"), **arrs)
    G.assert_sizes(out, ("unet_state_keys.json", "unet_eval.npz", "unet_train.npz",
                         "unet_train_logits_a.npz", "unet_train_logits_b.npz",
                         "unet_small_train.npz"))


if __name__ == "__main__":
    main()
