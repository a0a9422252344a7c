"""ESPNetV2 cost on one GPU — one JSON line.

  pyramid   functional.eesp_pyramid (forward, statistics and finish_bn included) at the EESP
            shapes of the config's 4 x 512 x 1024 crop, bf16 and fp32, on both routes, each
            selected through functional.eesp_pyramid_routed: the joint kernel
            (csrc/espnetv2.hip) and the per-branch route (four depthwise launches, three adds, one
            moments pass).  Achieved bytes/s against the 5 n-channel passes the joint kernel needs
            (read n once, write 4n once).  `bwd`: the backward both routes share (suffix sums,
            four depthwise backward launches, one 4-ary sum).
  ops       seg_bn_add_prelu_fwd / _bwd, seg_avgpool3x3s2_fwd / _bwd and the grouped 1x1
            convolution through the block-diagonal packing (forward, data and weight gradient),
            each against ATen on dense channels-last tensors of the same size.
  train     ms/step and img/s of the reference's loop statements (model, cross-entropy,
            zero_grad, backward, SGD step) at 4 x 3 x 512 x 1024, bf16: eager launches,
            SEGMENTRON_HIP_GRAPH=1, the same with every pyramid forced onto the per-branch route,
            and the torch restatement (tests/_espnetv2_oracle.py) on torch's own kernels under
            bf16 autocast (forward + loss + backward only).

Every op variant is captured `--iters` times into ONE HIP graph and the replay is timed,
`--repeats` times, the variants interleaved: median and spread (max - min) in microseconds per
call.  Consecutive calls of one graph rotate through ROTATE sets of operands, so that a call does
not find its own input and output in L2 from the call before (in the train step they come from
the producer, not from a previous run of the same kernel).  ATen runs on torch's own kernels (no
vendor convolution library: its first call would search for minutes).  Every leg runs in a child
process of its own under a time limit; the first leg that fails ends the run.

    python tools/espnetv2_bench.py [--legs pyramid,ops,train_eager,train_graph,
                                           train_graph_per_branch,train_aten] [--out FILE]

Weights and inputs are synthesised; timings do not depend on them."""
import argparse
import json
import sys

import _bench_zoo as Z

# N, H, W, n, stride, dilations: the EESP units of a 4 x 512 x 1024 crop
PYR_SHAPES = [(4, 64, 128, 32, 1, (1, 2, 3, 4)), (4, 32, 64, 64, 1, (1, 1, 2, 3)),
              (4, 256, 512, 8, 2, (1, 2, 3, 4)), (4, 128, 256, 16, 2, (1, 2, 3, 4)),
              (4, 64, 128, 32, 2, (1, 2, 3, 4))]
ADD_SHAPE = (4, 64, 128, 128)
POOL_SHAPE = (4, 128, 256, 64)
GROUPED_SHAPES = [(4, 64, 128, 128, 128), (4, 32, 64, 256, 64)]  # N, H, W, C, O (groups 4)
TRAIN_SHAPE = (4, 512, 1024)
ROTATE = 8


def _state(keys):
    import _espnetv2_oracle as O
    return O.state(keys)


TRAIN = {"yaml": "cityscapes_espnetv2.yaml", "shape": TRAIN_SHAPE, "aux_weight": 0.4,
         "state": _state}


def _rotating(make, call):
    return Z.rotating(make, call, ROTATE)


def pyramid_leg(iters, repeats):
    import torch
    import torch.nn as nn
    from segmentron_amd import functional as F
    real_routed = F.eesp_pyramid_routed
    out = {}
    for dtype, dname in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for N, H, W, n, s, dils in PYR_SHAPES:
            g = torch.Generator(device="cuda").manual_seed(0)
            convs = [nn.Conv2d(n, n, 3, s, d, d, groups=n, bias=False).cuda() for d in dils]
            bn = nn.BatchNorm2d(4 * n).cuda().train()
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1

            def make(i):
                return (torch.randn(N, H, W, n, device="cuda", generator=g).to(dtype),
                        torch.randn(N, Ho, Wo, 4 * n, device="cuda", generator=g).to(dtype))

            def fwd(joint):
                def call(ops):
                    F.eesp_pyramid_routed = (lambda *a: joint)
                    try:
                        with torch.no_grad():
                            return F.eesp_pyramid(ops[0], convs, bn)
                    finally:
                        F.eesp_pyramid_routed = real_routed
                return call

            def bwd(ops):
                x, gy = ops
                spec = F.EESPPyrSpec(dils, s, False, True)
                S = F.K.eesp_suffix_sum(gy)
                gs = [F.dw_backward(x, S[..., j * n:(j + 1) * n], c.weight, s, d)[0]
                      for j, (c, d) in enumerate(zip(convs, dils))]
                return F.K.sum_n(gs), spec
            variants = {"joint_fwd": _rotating(make, fwd(True)),
                        "per_branch_fwd": _rotating(make, fwd(False)),
                        "bwd": _rotating(make, bwd)}
            r = Z.measure(variants, iters, repeats)
            esz = 2 if dtype == torch.bfloat16 else 4
            nbytes = (N * H * W * n + N * Ho * Wo * 4 * n) * esz  # read n once, write 4n once
            for k in ("joint_fwd", "per_branch_fwd"):
                r[k]["GB_per_s"] = round(nbytes / (r[k]["median_us"] * 1e-6) / 1e9, 1)
            r["routed_joint"] = bool(real_routed(dtype, n, dils, s))
            key = "%s/%dx%dx%dx%d/s%d/d%s" % (dname, N, H, W, n, s, "".join(map(str, dils)))
            out[key] = r
            sys.stderr.write("%s %s\n" % (key, json.dumps(r)))
    return out


def ops_leg(iters, repeats):
    import torch
    import torch.nn as nn
    import torch.nn.functional as TF
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    torch.backends.cudnn.enabled = False
    dt = torch.bfloat16
    out = {}
    g = torch.Generator(device="cuda").manual_seed(0)

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=g).to(dt)
    # ---- BatchNorm + add + PReLU
    N, H, W, C = ADD_SHAPE
    sa, ta, sb, tb = (0.5 + torch.rand(C, device="cuda", generator=g) for _ in range(4))
    al = 0.05 + 0.4 * torch.rand(C, device="cuda", generator=g)
    v = [x.to(dt).view(1, C, 1, 1) for x in (sa, ta, sb, tb, al)]

    def aten_add(ops):
        a, b = ops[0].permute(0, 3, 1, 2), ops[1].permute(0, 3, 1, 2)
        return TF.prelu(a * v[0] + v[1] + b * v[2] + v[3], v[4].view(C))

    def aten_add_bwd(ops):
        a = ops[0].permute(0, 3, 1, 2).requires_grad_()
        b = ops[1].permute(0, 3, 1, 2).requires_grad_()
        alpha = v[4].view(C).clone().requires_grad_()
        y = TF.prelu(a * v[0] + v[1] + b * v[2] + v[3], alpha)
        return torch.autograd.grad(y, [a, b, alpha], ops[2].permute(0, 3, 1, 2))
    mk = lambda i: (rn(N, H, W, C), rn(N, H, W, C), rn(N, H, W, C))
    r = Z.measure({
        "hip_fwd": _rotating(mk, lambda o: K.bn_add_prelu(o[0], o[1], al, (sa, ta), (sb, tb))),
        "hip_bwd": _rotating(mk, lambda o: K.bn_add_prelu_bwd(o[2], o[0], o[1], al, (sa, ta),
                                                              (sb, tb))),
        "aten_fwd": _rotating(mk, aten_add),
        "aten_fwdbwd": _rotating(mk, aten_add_bwd)}, iters, repeats)
    elems = N * H * W * C * 2
    r["hip_fwd"]["GB_per_s"] = round(3 * elems / (r["hip_fwd"]["median_us"] * 1e-6) / 1e9, 1)
    r["hip_bwd"]["GB_per_s"] = round(4 * elems / (r["hip_bwd"]["median_us"] * 1e-6) / 1e9, 1)
    out["bn_add_prelu/%dx%dx%dx%d" % ADD_SHAPE] = r
    # ---- average pool
    N, H, W, C = POOL_SHAPE
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    mk = lambda i: (rn(N, H, W, C), rn(N, Ho, Wo, C))

    def aten_pool_bwd(ops):
        x = ops[0].permute(0, 3, 1, 2).requires_grad_()
        return torch.autograd.grad(TF.avg_pool2d(x, 3, 2, 1), x, ops[1].permute(0, 3, 1, 2))
    r = Z.measure({
        "hip_fwd": _rotating(mk, lambda o: K.avgpool3x3s2(o[0])),
        "hip_bwd": _rotating(mk, lambda o: K.avgpool3x3s2_bwd(o[1], (H, W))),
        "aten_fwd": _rotating(mk, lambda o: TF.avg_pool2d(o[0].permute(0, 3, 1, 2), 3, 2, 1)),
        "aten_fwdbwd": _rotating(mk, aten_pool_bwd)}, iters, repeats)
    nb = (N * H * W * C + N * Ho * Wo * C) * 2
    for k in ("hip_fwd", "hip_bwd"):
        r[k]["GB_per_s"] = round(nb / (r[k]["median_us"] * 1e-6) / 1e9, 1)
    out["avgpool3x3s2/%dx%dx%dx%d" % POOL_SHAPE] = r
    # ---- grouped 1x1 through the block-diagonal packing
    for N, H, W, C, O in GROUPED_SHAPES:
        conv = nn.Conv2d(C, O, 1, groups=4, bias=False).cuda()
        w = conv.weight.detach()
        wp = F.pack_conv_weight(F.block_diag_weight(w, 4), C, dt)
        wt = F.pack_conv_weight_dgrad(F.block_diag_weight(w, 4), O, dt)
        wa = w.to(dt).contiguous(memory_format=torch.channels_last)
        mk = lambda i: (rn(N, H, W, C), rn(N, H, W, O))

        def aten_bwd(mask):
            return lambda o: torch.ops.aten.convolution_backward(
                o[1].permute(0, 3, 1, 2), o[0].permute(0, 3, 1, 2), wa, None, (1, 1), (0, 0),
                (1, 1), False, (0, 0), 4, mask)
        r = Z.measure({
            "hip_fwd": _rotating(mk, lambda o: K.conv_gemm(o[0], wp, O, 1, 1, 1, 0, 1)),
            "hip_dgrad": _rotating(mk, lambda o: K.conv_gemm(o[1], wt, C, 1, 1, 1, 0, 1)),
            "hip_wgrad": _rotating(mk, lambda o: F.block_diag_grad(
                K.conv_wgrad(o[0], o[1], O, 1, 1, 1, 0, 1, None).view(O, C), 4)),
            "aten_fwd": _rotating(mk, lambda o: TF.conv2d(o[0].permute(0, 3, 1, 2), wa, None, 1, 0,
                                                          1, 4)),
            "aten_dgrad": _rotating(mk, aten_bwd((True, False, False))),
            "aten_wgrad": _rotating(mk, aten_bwd((False, True, False)))}, iters, repeats)
        out["grouped1x1/%dx%dx%dx%d->%d" % (N, H, W, C, O)] = r
    return out


def _per_branch():
    """Every pyramid onto the per-branch route."""
    from segmentron_amd import functional as F
    F.eesp_pyramid_routed = lambda *a: False


def child(args):
    import torch
    if args.leg == "pyramid":
        val = pyramid_leg(args.iters, args.repeats)
    elif args.leg == "ops":
        val = ops_leg(args.iters, args.repeats)
    elif args.leg == "train_aten":
        from _zoo import ESPNETV2
        val = Z.train_aten_leg(ESPNETV2, TRAIN_SHAPE, args.steps, args.warmup)
    else:
        hook = _per_branch if args.leg == "train_graph_per_branch" else None
        val = Z.train_leg(TRAIN, torch.bfloat16, args.steps, args.warmup,
                          graph=args.leg != "train_eager", before_build=hook)
    Z.emit_result(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--iters", type=int, default=24, help="calls per captured graph (op legs)")
    ap.add_argument("--repeats", type=int, default=9, help="timed replays per variant (op legs)")
    ap.add_argument("--legs", default="pyramid,ops,train_eager,train_graph,"
                                      "train_graph_per_branch,train_aten")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    header = {"pyramid_shapes": PYR_SHAPES, "add_shape": ADD_SHAPE, "pool_shape": POOL_SHAPE,
              "grouped_shapes": GROUPED_SHAPES, "train_shape": TRAIN_SHAPE, "rotate": ROTATE,
              "steps": args.steps, "warmup": args.warmup, "iters": args.iters,
              "repeats": args.repeats}
    legs = [(leg, ["--leg", leg]) for leg in args.legs.split(",")]
    return Z.run_legs(__file__, legs, args, header, passed=("steps", "warmup", "iters", "repeats"))


if __name__ == "__main__":
    sys.exit(main())
