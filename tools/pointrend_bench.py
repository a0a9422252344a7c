"""PointRend cost on one GPU: warmed, device-synchronised eager timings, one JSON line.

  train  ms/step (forward + loss + backward) at 769 x 769, B = 2, for PointRend (PointRendLoss
         of segmentron/solver/loss.py:364-387) and for DeepLabV3_Plus with ENABLE_DECODER False
         on the same backbone (cross-entropy of its x16-resized logits): the difference is the
         point head and the point loss
  eval   ms per image at 1025 x 2049, B = 1, for both models

    python tools/pointrend_bench.py [--steps 10] [--warmup 3] [--dtypes bf16,fp32]
                                    [--models PointRend,DeepLabV3_Plus] [--no-eval]

Weights are synthesised (oracle.synth); timings do not depend on them.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/pointrend_bench.py --steps 3 --warmup 1` for the
per-kernel times (profiles/r08_pointrend_*).
"""
import argparse
import json
import os
import sys

from _bench_zoo import timed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(name, dtype):
    import torch
    import segmentron_amd
    from oracle import synth
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_list(["DATASET.NAME", "cityscape", "MODEL.MODEL_NAME", name,
                          "MODEL.BACKBONE", "xception65", "MODEL.DEEPLABV3_PLUS.ENABLE_DECODER",
                          "False", "TRAIN.BACKBONE_PRETRAINED", "False"])
    cfg.PHASE = "train"
    cfg.check_and_freeze()
    segmentron_amd.set_compute_dtype(dtype)
    model = segmentron_amd.get_segmentation_model()
    model.load_state_dict(synth.synth_like(model.state_dict(), seed=0, conditioned=True))
    reset_cfg()
    return model.cuda()


def loss_of(name, out, y):
    import torch.nn.functional as TF
    if name != "PointRend":
        return TF.cross_entropy(out[0], y, ignore_index=-1)
    from segmentron_amd.models.pointrend import point_sample
    pred = TF.interpolate(out["coarse"], y.shape[-2:], mode="bilinear", align_corners=True)
    gt = point_sample(y.float().unsqueeze(1), out["points"], mode="nearest",
                      align_corners=False).squeeze_(1).long()
    return TF.cross_entropy(pred, y, ignore_index=-1) + \
        TF.cross_entropy(out["rend"], gt, ignore_index=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--models", default="PointRend,DeepLabV3_Plus")
    ap.add_argument("--no-eval", action="store_true")
    args = ap.parse_args()
    import torch
    from oracle import synth
    dts = {"bf16": torch.bfloat16, "fp32": torch.float32}
    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "train_769x769_b2_ms_per_step": {}, "eval_1025x2049_ms_per_image": {}}
    x = synth.synth_images(2, 769, 769, seed=0).cuda()
    y = synth.synth_targets(2, 769, 769, seed=0).cuda()
    xe = synth.synth_images(1, 1025, 2049, seed=0).cuda()
    for dn in args.dtypes.split(","):
        for name in args.models.split(","):
            model = build(name, dts[dn])
            model.train()

            def step():
                model.zero_grad(set_to_none=True)
                loss_of(name, model(x), y).backward()
            res["train_769x769_b2_ms_per_step"]["%s/%s" % (name, dn)] = round(
                timed(step, args.steps, args.warmup), 3)
            if not args.no_eval:
                model.eval()

                def infer():
                    with torch.no_grad():
                        model(xe)
                res["eval_1025x2049_ms_per_image"]["%s/%s" % (name, dn)] = round(
                    timed(infer, args.steps, args.warmup), 3)
            del model
            torch.cuda.empty_cache()
    for key in ("train_769x769_b2_ms_per_step", "eval_1025x2049_ms_per_image"):
        r = res[key]
        for dn in args.dtypes.split(","):
            a, b = r.get("PointRend/" + dn), r.get("DeepLabV3_Plus/" + dn)
            if a and b:
                r["PointRend_over_DeepLabV3_Plus/" + dn] = round(a / b, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
