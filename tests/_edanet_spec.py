"""The `Spec` of the EDANet tests (tests/test_edanet.py, tests/test_edanet_gpu.py): tests/_zoo.py's
checks with EDANet's fixtures (tools/gen_golden_edanet.py) and restatement
(tests/_edanet_oracle.py).  The pinned numbers are what the generator printed from the reference."""
import _edanet_oracle as O
from _zoo import Spec, fresh_cfg  # noqa: F401  (autouse, re-exported to the GPU file)

# bf16: the restatement under CPU bfloat16 autocast against its float64 run on the training
# fixture (the `cpu::` entries of edanet_train.npz, which must be these literals); the bars are
# 1.3 x these distances (_zoo.bf16_bars).
EDANET = Spec(
    O=O, name="edanet", model="EDANet", n_keys=348, n_params=689485, n_grads=222,
    eval_shape=(O.B, O.H, O.W), loop_shape=(O.B, O.H, O.W), train_shape=(O.TB, O.TH, O.TW),
    train_seed=O.TRAIN_SEED, second_shape=(O.H2, O.W2),
    bf16=(1.19012e-04, 0.99998852), bf16_tol=(1e-8, 1e-8), fused_shape=(2, 576, 584),
    key_width=45, graph_indent=18)
