"""ContextNet cost on one GPU — one JSON line.

  up_dw       the feature fusion's resize + depthwise 3x3 (csrc/contextnet.hip) in bf16 at the
              training shape, [4,24,24,128] -> 96 x 96 (4 x 768 x 768 images), and at the evaluation
              shape, [1,32,64,128] -> 128 x 256 (1024 x 2048), the low map's BatchNorm affine pending,
              the statistics rows taken:
                node_fwd      seg_up_dw_fwd
                node_bwd      seg_up_dw_bwd, seg_dwconv3x3_wgrad_finalize on its rows and
                              seg_bilinear_bwd of the transient d_up
                composed_fwd  the existing route: seg_bilinear_fwd into a stored upsampled map and
                              seg_dwconv3x3 on it
                composed_bwd  the fused depthwise backward on the stored upsampled map and
                              seg_bilinear_bwd of its data gradient
              Every variant cycles through enough operand sets that a call finds none of its
              operands in the last-level cache (at least 512 MiB between two uses of a set), as a
              layer's operands are inside a train step.
  train       ms/step and img/s of the reference's loop statements (model, cross-entropy,
              zero_grad, backward, SGD step) at 4 x 3 x 768 x 768, bf16: eager launches and
              SEGMENTRON_HIP_GRAPH=1 with the node routed as committed, the graph with the node forced
              off (SEG_CTX_UP_DW=0) and on (SEG_CTX_UP_DW=1), and the torch restatement
              (tests/_contextnet_oracle.py) on torch's own kernels under bf16 autocast (forward +
              loss + backward only)

Every op variant is captured `--iters` times into ONE HIP graph and the replay is timed,
`--repeats` times, the variants interleaved: median and spread (max - min) in microseconds per
call.  Every leg runs in a child process of its own under a time limit; the first leg that fails
ends the run.

    python tools/contextnet_bench.py [--legs up_dw,train_eager,train_graph,train_graph_off,
                                             train_graph_on,train_aten] [--out FILE]

Weights and inputs are synthesised; timings do not depend on them."""
import argparse
import json
import os
import sys

import _bench_zoo as Z

# N, h, w, H, W, C
SHAPES = [(4, 24, 24, 96, 96, 128), (1, 32, 64, 128, 256, 128)]
TRAIN_SHAPE = (4, 768, 768)
TRAIN = {"yaml": "cityscapes_contextnet.yaml", "shape": TRAIN_SHAPE, "aux_weight": 0.4}
COLD_BYTES = 512 << 20


def _operands(N, h, w, H, W, C, dt, seed):
    import torch
    from segmentron_amd import functional as F
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rand(shape):
        return torch.randn(shape, device="cuda", generator=g).to(dt)
    t = {"lo": rand((N, h, w, C)), "dy": rand((N, H, W, C)),
         "weight": torch.randn((C, 1, 3, 3), device="cuda", generator=g)}
    for k in ("U", "y", "g"):
        t[k] = torch.empty((N, H, W, C), dtype=dt, device="cuda")
    t["w9c"] = F.pack_dw_weight(t["weight"])
    t["s"] = torch.rand(C, device="cuda", generator=g) + 0.5
    t["t"] = torch.rand(C, device="cuda", generator=g) - 0.5
    return t


def up_dw_leg(iters, repeats):
    import torch
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    dt = torch.bfloat16
    out = {}
    for N, h, w, H, W, C in SHAPES:
        per_set = 2 * N * H * W * C * 4  # U, y, dy, g in bf16 (the low map is 1/16 of one)
        nsets = max(2, -(-COLD_BYTES // per_set))

        def make(i):
            t = _operands(N, h, w, H, W, C, dt, i)
            K.bilinear(t["lo"], (H, W), (K.PRO_AFFINE, t["s"], t["t"]), out=t["U"])
            return t

        def node_fwd(t):
            K.up_dw(t["lo"], (H, W), t["w9c"], (K.PRO_AFFINE, t["s"], t["t"]), out=t["y"],
                    want_stats=True)

        def composed_fwd(t):
            K.bilinear(t["lo"], (H, W), (K.PRO_AFFINE, t["s"], t["t"]), out=t["U"])
            K.dwconv(t["U"], t["weight"], 1, 1, None, out=t["y"], want_stats=True)

        def node_bwd(t):
            d_up, pw = K.up_dw_bwd(t["dy"], t["lo"], t["w9c"], (K.PRO_AFFINE, t["s"], t["t"]),
                                   out=t["g"])
            K.dw_wgrad_finalize(pw.view(pw.shape[0], 9 * C), C)
            K.bilinear_bwd(d_up, (h, w), True)

        def composed_bwd(t):
            g, _, _ = F.dw_backward_fused(t["U"], t["dy"], t["weight"], 1, 1, out=t["g"])
            K.bilinear_bwd(g, (h, w), True)
        sets = [make(i) for i in range(nsets)]
        variants = {name: Z.rotating(lambda i: sets[i], fn, nsets)
                    for name, fn in (("node_fwd", node_fwd), ("composed_fwd", composed_fwd),
                                     ("node_bwd", node_bwd), ("composed_bwd", composed_bwd))}
        key = "%dx%dx%dx%d_to_%dx%d" % (N, h, w, C, H, W)
        out[key] = Z.measure(variants, max(iters, nsets), repeats)
        out[key]["operand_sets"] = nsets
        sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
        del sets, variants
        torch.cuda.empty_cache()
    return out


def child(args):
    import torch
    if args.leg == "up_dw":
        val = up_dw_leg(args.iters, args.repeats)
    elif args.leg == "train_aten":
        from _contextnet_spec import CONTEXTNET
        val = Z.train_aten_leg(CONTEXTNET, TRAIN_SHAPE, args.steps, args.warmup)
    else:
        for tail, side in (("_off", "0"), ("_on", "1")):
            if args.leg.endswith(tail):  # (read when segmentron_amd.functional is imported)
                os.environ["SEG_CTX_UP_DW"] = side
        val = Z.train_leg(TRAIN, torch.bfloat16, args.steps, args.warmup,
                          graph=args.leg.startswith("train_graph"))
    Z.emit_result(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20, help="calls per captured graph (op legs)")
    ap.add_argument("--repeats", type=int, default=9, help="timed replays per variant (op legs)")
    ap.add_argument("--legs", default="up_dw,train_eager,train_graph,train_graph_off,"
                                      "train_graph_on,train_aten")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    header = {"shapes": SHAPES, "train_shape": TRAIN_SHAPE, "dtype": "bf16", "steps": args.steps,
              "warmup": args.warmup, "iters": args.iters, "repeats": args.repeats}
    legs = [(leg, ["--leg", leg]) for leg in args.legs.split(",")]
    return Z.run_legs(__file__, legs, args, header, passed=("steps", "warmup", "iters", "repeats"))


if __name__ == "__main__":
    sys.exit(main())
