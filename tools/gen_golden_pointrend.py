"""Fixtures of the PointRend tests (tests/test_pointrend.py), generated from the REFERENCE
(read-only, through oracle.ref_import):

  tests/golden/pointrend_state_keys.json          state_dict keys / shapes of the reference's
                                                  PointRend on DeepLabV3_Plus / xception65
  tests/golden/cityscapes_pointrend_deeplabv3_plus.yaml   the reference's config (settings only)
  tests/golden/pointrend_ref_run.npz              one reference run at 2 x 3 x 97 x 129 with the
                                                  synthesised weights of tests/_pointrend_oracle.py:
                                                  evaluation output (every 2nd pixel), then one
                                                  training forward with its torch.rand draws
                                                  recorded, the points and PointRendLoss

    python tools/gen_golden_pointrend.py
"""
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = "configs/cityscapes_pointrend_deeplabv3_plus.yaml"


def main():
    from oracle import ref_import
    model, _ = ref_import.build_reference_model(YAML)
    keys = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    out = {"config": YAML, "keys": keys, "n_params": sum(p.numel() for p in model.parameters()),
           "encoder_is_none": model.encoder is None}
    with open(os.path.join(GOLDEN, "pointrend_state_keys.json"), "w") as f:
        json.dump(out, f)
    shutil.copyfile(os.path.join(ref_import.REFERENCE_ROOT, YAML),
                    os.path.join(GOLDEN, os.path.basename(YAML)))
    print("%d keys, %d parameters" % (len(keys), out["n_params"]))
    reference_run(model)


def reference_run(model):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _pointrend_oracle as O
    from oracle import synth
    from segmentron.solver.loss import PointRendLoss
    sd = O.state([(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    model.load_state_dict(sd)
    model.backbone.head.aspp.dropout.p = 0.0
    x = synth.synth_images(O.B, O.H, O.W, seed=1)
    y = synth.synth_targets(O.B, O.H, O.W, seed=1)
    model.eval()
    with torch.no_grad():
        fine = model(x)[0]
    model.train()
    rec, rand = [], torch.rand

    def recording_rand(*a, **k):
        t = rand(*a, **k)
        rec.append(t.clone())
        return t
    torch.manual_seed(0)
    torch.rand = recording_rand
    try:
        out = model(x)
    finally:
        torch.rand = rand
    loss = PointRendLoss()(out, y)["loss"]
    assert len(rec) == 2
    np.savez_compressed(os.path.join(GOLDEN, "pointrend_ref_run.npz"),
                        fine_sub2=fine[..., ::2, ::2].numpy(), over=rec[0].numpy(),
                        cover=rec[1].numpy(), points=out["points"].detach().numpy(),
                        loss=np.float64(loss.item()))
    print("reference run: loss %.6f, %d points" % (loss.item(), out["points"].shape[1]))


if __name__ == "__main__":
    main()
