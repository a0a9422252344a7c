"""The `Spec` of the ContextNet tests (tests/test_contextnet.py, tests/test_contextnet_gpu.py):
tests/_zoo.py's checks with ContextNet's fixtures (tools/gen_golden_contextnet.py) and restatement
(tests/_contextnet_oracle.py).  The pinned numbers are what the generator printed from the
reference."""
import _contextnet_oracle as O
from _zoo import Spec, fresh_cfg  # noqa: F401  (autouse, re-exported to the GPU file)

N_KEYS_AUX, N_PARAMS_AUX = 318, 914118  # with SOLVER.AUX True

# bf16: the restatement under CPU bfloat16 autocast against its float64 run on the training
# fixture (the `cpu::` entries of contextnet_train.npz, which must be these literals); the bars are
# 1.3 x these distances (_zoo.bf16_bars).
CONTEXTNET = Spec(
    O=O, name="contextnet", model="ContextNet", n_keys=310, n_params=876563, n_grads=157,
    eval_shape=(O.B, O.H, O.W), loop_shape=(O.B, O.H, O.W), train_shape=(O.TB, O.TH, O.TW),
    train_seed=O.TRAIN_SEED, second_shape=(O.H_ODD, O.W_ODD),
    bf16=(6.735001e-04, 0.99999002), bf16_tol=(1e-8, 1e-8), head_stride=8,
    fused_shape=(O.FB, O.FH, O.FW), key_width=60, graph_indent=22)
