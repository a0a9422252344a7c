"""DUNet (resnet50, OS 8, SOLVER.AUX True) cost on one GPU — one JSON line.

  op     the fused DUpsampling cross-entropy (csrc/dupsample.hip), forward + backward, at
         lo = [4, 96, 96, 1216] (the config's 4 x 768 x 768 crop) against the two paths that exist
         without it:
           point  seg_point_ce_fwd/bwd on lo.view(R, C), the target permuted by torch (included)
           aten   the permuted NCHW float32 view + F.cross_entropy, forward and backward
         Every variant is captured `--iters` times into ONE HIP graph and the replay is timed,
         `--repeats` times: median and spread (max - min) in microseconds per call, and the
         achieved bytes per second of the fused kernels against their traffic counts.
  train  ms/step and img/s of the reference's loop statements (model, MixSoftmaxCrossEntropyLoss,
         zero_grad, backward, SGD step) at 4 x 3 x 768 x 768 with SEGMENTRON_HIP_GRAPH=1

Every leg runs in a child process of its own under a time limit; the first leg that fails ends the
run.

    python tools/dunet_bench.py [--legs op,train] [--dtypes bf16,fp32] [--out FILE]

Weights and inputs are synthesised (oracle.synth); timings do not depend on them."""
import argparse
import sys

import _bench_zoo as Z

OP_SHAPE = (4, 96, 96, 8, 19)  # N, h, w, s, C
TRAIN_SHAPE = (4, 768, 768)
TRAIN = {"yaml": "cityscapes_dunet.yaml", "shape": TRAIN_SHAPE, "aux_weight": 0.4,
         "overrides": ("SOLVER.AUX", "True", "SOLVER.AUX_WEIGHT", "0.4")}


def op_leg(dtype, iters, repeats):
    import torch
    import torch.nn.functional as TF
    from segmentron_amd import hip_ops as K
    N, h, w, s, C = OP_SHAPE
    k = s * s * C
    g = torch.Generator(device="cuda").manual_seed(0)
    lo = (torch.randn(N, h, w, k, device="cuda", generator=g) * 2.0).to(dtype)
    tgt = torch.randint(0, C, (N, h * s, w * s), device="cuda", generator=g)
    tgt[torch.rand(N, h * s, w * s, device="cuda", generator=g) < 0.05] = -1
    one = torch.ones(1, device="cuda")
    lo_req = lo.clone().requires_grad_()

    def fused_fwd():
        return K.dup_ce_fwd(lo, tgt, s, C, -1)
    out = fused_fwd()

    def fused_bwd():
        return K.dup_ce_bwd(lo, tgt, s, C, -1, out, one)

    def point_perm():
        return tgt.view(N, h, s, w, s).permute(0, 1, 3, 2, 4).reshape(-1)
    rows = lo.view(-1, C)
    trow = point_perm()
    pout = K.point_ce_fwd(rows, trow, -1)

    def point_fwd():
        return K.point_ce_fwd(rows, point_perm(), -1)

    def point_bwd():
        return K.point_ce_bwd(rows, trow, -1, pout, one)

    def aten_view(t):
        return t.view(N, h, w, s, s, C).permute(0, 5, 1, 3, 2, 4).reshape(N, C, h * s, w * s)

    def aten_fwd():
        with torch.no_grad():
            return TF.cross_entropy(aten_view(lo).float(), tgt, ignore_index=-1)

    def aten_fwd_bwd():
        loss = TF.cross_entropy(aten_view(lo_req).float(), tgt, ignore_index=-1)
        return torch.autograd.grad(loss, lo_req)[0]

    assert abs(out[0].item() - pout[0].item()) <= 1e-6 * abs(pout[0].item())
    assert abs(out[0].item() - aten_fwd().item()) <= 1e-4 * abs(out[0].item())
    variants = {"fused_fwd": fused_fwd, "fused_bwd": fused_bwd, "point_fwd": point_fwd,
                "point_bwd": point_bwd, "aten_fwd": aten_fwd, "aten_fwd_bwd": aten_fwd_bwd}
    res = Z.measure(variants, iters, repeats)
    eb = lo.element_size()
    traffic = {"fused_fwd": lo.numel() * eb + tgt.numel() * 8,
               "fused_bwd": 2 * lo.numel() * eb + tgt.numel() * 8}
    for name, nbytes in traffic.items():
        res[name]["bytes"] = nbytes
        res[name]["TB_per_s"] = round(nbytes / (res[name]["median_us"] * 1e-6) / 1e12, 3)
    return res


def child(args):
    import torch
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.dtype]
    if args.leg == "op":
        val = op_leg(dtype, args.iters, args.repeats)
    else:
        val = Z.train_leg(TRAIN, dtype, args.steps, args.warmup, graph=True)
    Z.emit_result(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20, help="calls per captured graph (op leg)")
    ap.add_argument("--repeats", type=int, default=9, help="timed replays per variant (op leg)")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--legs", default="op,train")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) run this one leg in this process")
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    header = {"op_shape": OP_SHAPE, "train_shape": TRAIN_SHAPE, "steps": args.steps,
              "warmup": args.warmup, "iters": args.iters, "repeats": args.repeats}
    legs = [("%s/%s" % (leg, dn), ["--leg", leg, "--dtype", dn])
            for leg in args.legs.split(",") for dn in args.dtypes.split(",")
            if dn == "bf16" or leg != "train"]
    return Z.run_legs(__file__, legs, args, header, passed=("steps", "warmup", "iters", "repeats"))


if __name__ == "__main__":
    sys.exit(main())
