"""Fixtures of the FPENet tests (tests/test_fpenet.py, tests/test_fpenet_gpu.py), generated from the
REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_fpenet_oracle.py (oracle.synth seed 0, conditioned):

  tests/golden/cityscapes_fpenet.yaml     the reference's config (settings only)
  tests/golden/fpenet_state_keys.json     state_dict keys / shapes / parameter count
  tests/golden/fpenet_eval.npz            evaluation logits (every 2nd pixel) at 2 x 3 x 64 x 96 (8 x
                                          12 maps at 1/8: at dilation 8 every side tap along H is
                                          outside) and the output shape at 1 x 3 x 65 x 97
  tests/golden/fpenet_train.npz           one training forward / backward at 4 x 3 x 128 x 192 (6144
  tests/golden/fpenet_train_logits_a.npz  rows per BatchNorm at 1/4, the plain path; 1536 at 1/8, the
  tests/golden/fpenet_train_logits_b.npz  few-sample path): loss, logits (every 2nd pixel; images
                                          0-1 in _a, 2-3 in _b), per-parameter gradient norms, the
                                          running statistics after the step (`stat::`) and the
                                          `cpu::` yardsticks (float32 against float64, and the
                                          restatement under CPU bfloat16 autocast against its
                                          float64 run)
  tests/golden/fpenet_small_train.npz     the same step at 2 x 3 x 64 x 96: every BatchNorm behind
                                          the stem on the few-sample path

The training inputs' seed is the first whose float64 run keeps every ReLU input — the BatchNorm +
ReLU pairs, the block tails and the ReLU in the MEU's channel-attention path — decidable in
float32 (tests/_fpenet_oracle.py TRAIN_SEED; the scan is repeated here and asserted).

    python tools/gen_golden_fpenet.py [--out DIR]
"""
import os

import _golden_zoo as G

YAML = "configs/cityscapes_fpenet.yaml"


def main():
    import numpy as np
    import torch
    import _fpenet_oracle as O
    from oracle import synth
    out = G.parse_args(__doc__).out
    model, keys, sd = G.reference_model(O, YAML)
    G.write_schema(out, "fpenet", YAML, model, keys)
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        odd = model(synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
    np.savez_compressed(os.path.join(out, "fpenet_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2], n_outputs=np.int64(len(ev)),
                        shape_odd=np.array(odd[0].shape))
    print("eval: %d outputs, %s; %d x %d -> %s" % (len(ev), tuple(ev[0].shape), O.H_ODD, O.W_ODD,
                                                   tuple(odd[0].shape)))
    for p, _, _ in O.BLOCKS:
        print("%s: %d channels per quarter" % (p, sd[p + ".conv2.0.weight"].shape[0]))
    seed = G.scan_seed(O, sd, O.min_relu_margin, O.RELU_MARGIN, "ReLU")
    # (negligible: the bn3 biases of layer3.2 .. layer3.8 — 7e-19 of the global norm in float64.
    # With this state the tails of those blocks are active everywhere, so the bias is a constant
    # added to every later block input, which the next training-mode BatchNorm behind each 1x1
    # convolution removes: its gradient is zero in exact arithmetic)
    arrs, x, y = G._train_fixture(model, sd, O.TB, O.TH, O.TW, check=True, seed=seed,
                                  negligible=1e-12)
    print("gradients in the train fixture: %d" % sum(k.startswith("gnorm::") for k in arrs))
    arrs["seed"] = np.int64(seed)
    arrs.update(G.bf16_yardstick(O, sd, x, y))
    G.save_train(out, "fpenet", arrs)
    model.load_state_dict(sd)  # (the step above moved the running statistics)
    arrs, _, _ = G._train_fixture(model, sd, O.B, O.H, O.W, check=False)
    np.savez_compressed(os.path.join(out, "fpenet_small_train.npz"), **arrs)
    G.assert_sizes(out, ("fpenet_state_keys.json", "fpenet_eval.npz", "fpenet_train.npz",
                         "fpenet_train_logits_a.npz", "fpenet_train_logits_b.npz",
                         "fpenet_small_train.npz"))


if __name__ == "__main__":
    main()
