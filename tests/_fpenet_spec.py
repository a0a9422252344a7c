"""The `Spec` of the FPENet tests (tests/test_fpenet.py, tests/test_fpenet_gpu.py): tests/_zoo.py's
checks with FPENet's fixtures (tools/gen_golden_fpenet.py) and restatement
(tests/_fpenet_oracle.py).  The pinned numbers are what the generator printed from the reference."""
import _fpenet_oracle as O
from _zoo import Spec, fresh_cfg  # noqa: F401  (autouse, re-exported to the GPU file)

# bf16: the restatement under CPU bfloat16 autocast against its float64 run on the training
# fixture (the `cpu::` entries of fpenet_train.npz, which must be these literals); the bars are
# 1.3 x these distances (_zoo.bf16_bars).
FPENET = Spec(
    O=O, name="fpenet", model="FPENet", n_keys=516, n_params=115125, n_grads=261,
    eval_shape=(O.B, O.H, O.W), loop_shape=(O.B, O.H, O.W), train_shape=(O.TB, O.TH, O.TW),
    train_seed=O.TRAIN_SEED, second_shape=(O.H_ODD, O.W_ODD),
    bf16=(1.09671e-04, 0.99997527), bf16_tol=(1e-8, 1e-8), head_stride=2,
    fused_shape=(2, 512, 528), key_width=45, graph_indent=18)
