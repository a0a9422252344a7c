"""The `Spec` of the UNet tests (tests/test_unet.py, tests/test_unet_gpu.py): tests/_zoo.py's
checks with UNet's fixtures (tools/gen_golden_unet.py) and restatement (tests/_unet_oracle.py).
The pinned numbers are what the generator printed from the reference."""
import _unet_oracle as O
from _zoo import Spec, fresh_cfg  # noqa: F401  (autouse, re-exported to the GPU file)

# bf16: the restatement under CPU bfloat16 autocast against its float64 run on the training
# fixture (the `cpu::` entries of unet_train.npz, which must be these literals); the bars are
# 1.3 x these distances (_zoo.bf16_bars).
UNET = Spec(
    O=O, name="unet", model="UNet", n_keys=128, n_params=13396499, n_grads=74,
    eval_shape=(O.B, O.H, O.W), loop_shape=(O.B, O.H, O.W), train_shape=(O.TB, O.TH, O.TW),
    train_seed=O.TRAIN_SEED, second_shape=(O.H_ODD, O.W_ODD),
    bf16=(1.06138e-04, 0.99991268), bf16_tol=(1e-8, 1e-8), head_stride=1,
    fused_shape=(O.FB, O.FH, O.FW), key_width=50, graph_indent=16)
