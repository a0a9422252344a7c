"""Fixtures of the ContextNet tests (tests/test_contextnet.py, tests/test_contextnet_gpu.py),
generated from the REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_contextnet_oracle.py (oracle.synth seed 0, conditioned):

  tests/golden/cityscapes_contextnet.yaml     the reference's config (settings only)
  tests/golden/contextnet_state_keys.json     state_dict keys / shapes / parameter count, and the
                                              counts with SOLVER.AUX True
  tests/golden/contextnet_eval.npz            evaluation logits (every 2nd pixel) at 2 x 3 x 64 x 96
                                              (hi 8 x 12, lo 2 x 3) and the output shape at
                                              1 x 3 x 70 x 97 (hi 9 x 12, x_low 17 x 24)
  tests/golden/contextnet_train.npz           one training forward / backward at 4 x 3 x 112 x 160:
  tests/golden/contextnet_train_logits_a.npz  the 1/8 maps hold 1120 rows per BatchNorm (the plain
  tests/golden/contextnet_train_logits_b.npz  path), bottleneck3 onwards 280 / 80 (the few-sample
                                              path), the fusion resizes 4 x 5 to 14 x 20: loss,
                                              logits (every 2nd pixel; images 0-1 in _a, 2-3 in
                                              _b), per-parameter gradient norms, the running
                                              statistics after the step (`stat::`) and the `cpu::`
                                              yardsticks (float32 against float64, and the
                                              restatement under CPU bfloat16 autocast against its
                                              float64 run)
  tests/golden/contextnet_small_train.npz     the same step at 2 x 3 x 64 x 96: every BatchNorm on
                                              the few-sample path

The training inputs' seed is the first whose float64 run keeps every ReLU input decidable in
float32 (tests/_contextnet_oracle.py TRAIN_SEED; the scan is repeated here and asserted).

    python tools/gen_golden_contextnet.py [--out DIR]
"""
import os
import subprocess
import sys

import _golden_zoo as G

YAML = "configs/cityscapes_contextnet.yaml"


def main():
    import numpy as np
    import torch
    import _contextnet_oracle as O
    from oracle import ref_import, synth
    args = G.parse_args(__doc__, leg="aux")
    out = args.out
    if args.aux:  # (second process: the reference's cfg is frozen once a model has been built)
        aux_model, _ = ref_import.build_reference_model(YAML, ["SOLVER.AUX", "True"])
        print("AUX %d %d" % (len(aux_model.state_dict()),
                             sum(p.numel() for p in aux_model.parameters())))
        return
    leg = subprocess.run([sys.executable, os.path.abspath(__file__), "--aux", "--out", out],
                         check=True, capture_output=True, text=True).stdout
    n_keys_aux, n_params_aux = [int(v) for v in
                                [l for l in leg.splitlines() if l.startswith("AUX ")][-1].split()[1:]]
    print("with SOLVER.AUX True: %d keys, %d parameters" % (n_keys_aux, n_params_aux))
    model, keys, sd = G.reference_model(O, YAML)
    G.write_schema(out, "contextnet", YAML, model, keys, n_keys_aux=n_keys_aux,
                   n_params_aux=n_params_aux)
    print("decoder attribute: %s" % hasattr(model, "decoder"))
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        odd = model(synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
        one = model(synth.synth_images(1, O.H_ONE, O.W_ONE, seed=0))
    np.savez_compressed(os.path.join(out, "contextnet_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2], n_outputs=np.int64(len(ev)),
                        shape_odd=np.array(odd[0].shape))
    print("eval: %d outputs, %s; %d x %d -> %s; %d x %d -> %s"
          % (len(ev), tuple(ev[0].shape), O.H_ODD, O.W_ODD, tuple(odd[0].shape), O.H_ONE, O.W_ONE,
             tuple(one[0].shape)))
    seed = G.scan_seed(O, sd, O.min_relu_margin, O.RELU_MARGIN, "ReLU")
    # (negligible: the biases of the fusion's two 1x1 convolutions in front of a training-mode
    # BatchNorm, which removes any constant: their gradient is zero in exact arithmetic)
    arrs, x, y = G._train_fixture(model, sd, O.TB, O.TH, O.TW, check=True, seed=seed,
                                  negligible=1e-12)
    print("gradients in the train fixture: %d" % sum(k.startswith("gnorm::") for k in arrs))
    arrs["seed"] = np.int64(seed)
    arrs.update(G.bf16_yardstick(O, sd, x, y))
    G.save_train(out, "contextnet", arrs)
    model.load_state_dict(sd)  # (the step above moved the running statistics)
    arrs, _, _ = G._train_fixture(model, sd, O.B, O.H, O.W, check=False)
    np.savez_compressed(os.path.join(out, "contextnet_small_train.npz"), **arrs)
    G.assert_sizes(out, ("contextnet_state_keys.json", "contextnet_eval.npz",
                         "contextnet_train.npz", "contextnet_train_logits_a.npz",
                         "contextnet_train_logits_b.npz", "contextnet_small_train.npz"))


if __name__ == "__main__":
    main()
