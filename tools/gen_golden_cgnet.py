"""Fixtures of the CGNet tests (tests/test_cgnet.py, tests/test_cgnet_gpu.py), generated from the
REFERENCE (read-only, through oracle.ref_import) with the synthesised weights of
tests/_cgnet_oracle.py (oracle.synth seed 0, conditioned; PReLU slopes in [0.05, 0.45]):

  tests/golden/cityscapes_cgnet.yaml     the reference's config (settings only)
  tests/golden/cgnet_state_keys.json     state_dict keys / shapes / parameter count / decoder list
  tests/golden/cgnet_eval.npz            evaluation logits (every 2nd pixel) at 2 x 3 x 64 x 96 and
                                         the output SHAPE for 1 x 3 x 65 x 97
  tests/golden/cgnet_train.npz           one training forward / backward at 4 x 3 x 128 x 192,
  tests/golden/cgnet_train_logits_a.npz  dropout 0 (the stage-2 / stage-3 BatchNorms see 6144 / 1536
  tests/golden/cgnet_train_logits_b.npz  rows): loss, logits (every 2nd pixel; images 0-1 in _a,
                                         2-3 in _b: 1 MiB per committed file),
                                         per-parameter gradient norms, the running statistics after
                                         the step (`stat::`), and what the reference's own
                                         arithmetic costs on this input (`cpu::`): float32 against
                                         float64 per tensor, and loss distance / gradient cosine of
                                         the float64-checked restatement under CPU bfloat16 autocast
  tests/golden/cgnet_small_train.npz     the same step at 2 x 3 x 64 x 96 with
                                         MODEL.CGNET.STAGE2_BLOCK_NUM 2 STAGE3_BLOCK_NUM 2: the
                                         few-sample BatchNorm path (768 / 192 rows)

Before anything is written the float32 run is compared with the reference in float64: the float32
run must itself satisfy the gradient acceptance rule of tests/_zoo.py (check_gradients) with the
margin that rule grants the device (err_cpu32 := 0): global error <= 1e-4, at most 10 % of the
tensors beyond 1e-3 relative and none beyond 3e-2.

    python tools/gen_golden_cgnet.py [--out DIR]   (the small leg runs in a second process: the
                                                    reference's cfg is a frozen per-process
                                                    singleton)
"""
import os
import subprocess
import sys

import _golden_zoo as G

YAML = "configs/cityscapes_cgnet.yaml"


def main():
    import numpy as np
    import torch
    import _cgnet_oracle as O
    from oracle import synth
    args = G.parse_args(__doc__, leg="small")
    out = args.out
    model, keys, sd = G.reference_model(O, YAML, O.SMALL_OVERRIDES if args.small else [])
    if args.small:
        assert (len(model.stage2), len(model.stage3)) == (1, 1)
        arrs, _, _ = G._train_fixture(model, sd, O.B, O.H, O.W, check=False)
        np.savez_compressed(os.path.join(out, "cgnet_small_train.npz"), **arrs)
        return
    G.write_schema(out, "cgnet", YAML, model, keys, decoder=list(model.decoder))
    # evaluation, running statistics as synthesised
    model.eval()
    with torch.no_grad():
        ev = model(synth.synth_images(O.B, O.H, O.W, seed=0))
        odd = model(synth.synth_images(1, O.H_ODD, O.W_ODD, seed=0))
    np.savez_compressed(os.path.join(out, "cgnet_eval.npz"),
                        logits0=ev[0].numpy()[..., ::2, ::2],
                        shape_odd=np.array(odd[0].shape, dtype=np.int64),
                        n_outputs=np.int64(len(ev)))
    print("eval: %d outputs, %s; odd input -> %s" % (len(ev), tuple(ev[0].shape),
                                                      tuple(odd[0].shape)))
    arrs, x, y = G._train_fixture(model, sd, O.TB, O.TH, O.TW, check=True)
    arrs.update(G.bf16_yardstick(O, sd, x, y))
    G.save_train(out, "cgnet", arrs)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--small", "--out", out])
    G.assert_sizes(out, ("cgnet_state_keys.json", "cgnet_eval.npz", "cgnet_train.npz",
                         "cgnet_train_logits_a.npz", "cgnet_train_logits_b.npz",
                         "cgnet_small_train.npz"))


if __name__ == "__main__":
    main()
