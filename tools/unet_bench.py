"""UNet cost on one GPU — one JSON line.

  skip_pool   the encoder skip + max-pool pass (csrc/unet.hip) at the workload's levels, a
              2 x 512 x 512 batch in bf16 — [2,512,512,64], [2,256,256,128], [2,128,128,256],
              [2,64,64,512] — the skip and its gradient as the leading C channels of a 2C-channel
              concat buffer, affine + ReLU pending:
                hip_fwd       seg_skip_pool_fwd
                hip_bwd       seg_skip_pool_bwd, seg_bn_bwd_finalize_p on its rows and
                              seg_bn_bwd_apply in its affine-only mode
                composed_fwd  the existing route: seg_bn_apply into the slice and seg_maxpool_fwd with
                              the prologue (y read twice, an index byte per pooled element)
                composed_bwd  seg_maxpool_bwd, the 2-ary sum with the skip's gradient, then the
                              masked BatchNorm backward (reduce, finalize, apply)
              Every variant cycles through enough operand sets that a call finds none of its
              operands in the last-level cache (at least 512 MiB between two uses of a set), as a
              layer's operands are inside a train step.
  train       ms/step and img/s of the reference's loop statements (model, cross-entropy,
              zero_grad, backward, SGD step) at 2 x 3 x 512 x 512 (the config's batch and crop), bf16:
              eager launches and SEGMENTRON_HIP_GRAPH=1, each with the fused node routed as committed
              and with it forced off (SEG_UNET_SKIP_POOL=0), and the torch restatement
              (tests/_unet_oracle.py) on torch's own kernels under bf16 autocast (forward + loss +
              backward only)

Every op variant is captured `--iters` times into ONE HIP graph and the replay is timed,
`--repeats` times, the variants interleaved: median and spread (max - min) in microseconds per
call.  Every leg runs in a child process of its own under a time limit; the first leg that fails
ends the run.

    python tools/unet_bench.py [--legs skip_pool,train_eager,train_graph,train_eager_off,
                                       train_graph_off,train_aten] [--out FILE]

Weights and inputs are synthesised; timings do not depend on them."""
import argparse
import json
import os
import sys

import _bench_zoo as Z

# N, H, W, C
LEVELS = [(2, 512, 512, 64), (2, 256, 256, 128), (2, 128, 128, 256), (2, 64, 64, 512)]
TRAIN_SHAPE = (2, 512, 512)
TRAIN = {"yaml": "cityscapes_unet.yaml", "shape": TRAIN_SHAPE, "aux_weight": 0.4}
COLD_BYTES = 512 << 20


def _operands(N, H, W, C, dt, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rand(shape):
        return torch.randn(shape, device="cuda", generator=g).to(dt)
    t = {"y": rand((N, H, W, C)), "cat": rand((N, H, W, 2 * C)), "gcat": rand((N, H, W, 2 * C)),
         "gp": rand((N, H // 2, W // 2, C)), "g": torch.empty((N, H, W, C), dtype=dt, device="cuda")}
    t["skip"], t["gs"] = t["cat"][..., :C], t["gcat"][..., :C]
    for k in ("s", "mean", "invstd", "gamma"):
        t[k] = torch.rand(C, device="cuda", generator=g) + 0.5
    t["t"] = torch.rand(C, device="cuda", generator=g) - 0.5
    return t


def skip_pool_leg(iters, repeats):
    import torch
    from segmentron_amd import hip_ops as K
    dt = torch.bfloat16
    AR = K.PRO_AFFINE_RELU
    out = {}
    for N, H, W, C in LEVELS:
        per_set = 2 * N * H * W * C * 6  # y, cat, gcat, g (and the pooled pair) in bf16
        nsets = max(2, -(-COLD_BYTES // per_set))
        count = float(N * H * W)

        def make(i):
            t = _operands(N, H, W, C, dt, i)
            _, t["idx"] = K.maxpool(t["y"], 2, 2, 0, (AR, t["s"], t["t"]))
            return t

        def hip_fwd(t):
            K.skip_pool_fwd(t["y"], (AR, t["s"], t["t"]), out=t["skip"])

        def hip_bwd(t):
            g, pb = K.skip_pool_bwd(t["gs"], t["gp"], t["y"], (AR, t["s"], t["t"]), out=t["g"])
            _, _, c0, c1 = K.bn_bwd_finalize_p(pb.view(pb.shape[0], -1), count, t["mean"],
                                               t["invstd"], t["gamma"])
            K.bn_bwd_apply(g, t["y"], (K.PRO_AFFINE, t["s"], t["t"]), c0, c1, out=g)

        def composed_fwd(t):
            K.bn_apply(t["y"], (AR, t["s"], t["t"]), out=t["skip"])
            K.maxpool(t["y"], 2, 2, 0, (AR, t["s"], t["t"]))

        def composed_bwd(t):
            pro = (AR, t["s"], t["t"])
            ga = K.maxpool_bwd(t["gp"], t["idx"], (H, W), 2, 2, 0)
            g = K.sum_n([t["gs"], ga], out=t["g"])
            pb = K.bn_bwd_reduce_partial(g, t["y"], pro)
            _, _, c0, c1 = K.bn_bwd_finalize_p(pb, count, t["mean"], t["invstd"], t["gamma"])
            K.bn_bwd_apply(g, t["y"], pro, c0, c1, out=g)
        sets = [make(i) for i in range(nsets)]
        variants = {name: Z.rotating(lambda i: sets[i], fn, nsets)
                    for name, fn in (("hip_fwd", hip_fwd), ("composed_fwd", composed_fwd),
                                     ("hip_bwd", hip_bwd), ("composed_bwd", composed_bwd))}
        key = "%dx%dx%dx%d" % (N, H, W, C)
        out[key] = Z.measure(variants, max(iters, nsets), repeats)
        out[key]["operand_sets"] = nsets
        sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
        del sets, variants
        torch.cuda.empty_cache()
    return out


def child(args):
    import torch
    if args.leg == "skip_pool":
        val = skip_pool_leg(args.iters, args.repeats)
    elif args.leg == "train_aten":
        from _unet_spec import UNET
        val = Z.train_aten_leg(UNET, TRAIN_SHAPE, args.steps, args.warmup)
    else:
        if args.leg.endswith("_off"):  # (read when segmentron_amd.functional is imported)
            os.environ["SEG_UNET_SKIP_POOL"] = "0"
        val = Z.train_leg(TRAIN, torch.bfloat16, args.steps, args.warmup,
                          graph=args.leg.startswith("train_graph"))
    Z.emit_result(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20, help="calls per captured graph (op legs)")
    ap.add_argument("--repeats", type=int, default=9, help="timed replays per variant (op legs)")
    ap.add_argument("--legs", default="skip_pool,train_eager,train_graph,train_eager_off,"
                                      "train_graph_off,train_aten")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    header = {"levels": LEVELS, "train_shape": TRAIN_SHAPE, "dtype": "bf16", "steps": args.steps,
              "warmup": args.warmup, "iters": args.iters, "repeats": args.repeats}
    legs = [(leg, ["--leg", leg]) for leg in args.legs.split(",")]
    return Z.run_legs(__file__, legs, args, header, passed=("steps", "warmup", "iters", "repeats"))


if __name__ == "__main__":
    sys.exit(main())
