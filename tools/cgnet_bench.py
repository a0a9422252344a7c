"""CGNet cost on one GPU — one JSON line.

  joint  the joint local / surround depthwise launch (csrc/cgnet.hip), forward, at the two
         workload shapes of the config's 4 x 768 x 768 crop — [4,192,192,32] dilation 2 and
         [4,96,96,64] dilation 4 — against what the library could already do for the same result,
         two seg_dwconv3x3 launches into the two channel slices (statistics included): this
         comparison decides functional.cg_joint_routed.  And the backward both routes share: two
         fused depthwise backward launches (data gradient + weight-gradient rows each) with the
         2-ary sum of the data gradients (bwd_pair_sum) or with the surround gradient added in the
         local launch's store path (bwd_pair_res, what runs).  (A direct joint backward kernel
         lost against both and was not kept: profiles/cgnet.md.)
  prelu  bn_prelu(pool=True) and its backward (seg_prelu_bwd + the BatchNorm backward) at
         [4,96,96,128] against ATen on the same device (channels-last affine + prelu + mean, and
         autograd through them)
  train  ms/step and img/s of the reference's loop statements (model, cross-entropy, zero_grad,
         backward, SGD step) at 4 x 3 x 768 x 768, bf16: eager launches, and SEGMENTRON_HIP_GRAPH=1

Every op variant is captured `--iters` times into ONE HIP graph and the replay is timed,
`--repeats` times, the variants interleaved: median and spread (max - min) in microseconds per
call.  Every leg runs in a child process of its own under a time limit; the first leg that fails
ends the run.

    python tools/cgnet_bench.py [--legs joint,train_eager,train_graph,prelu] [--dtypes bf16,fp32]
                                [--out FILE]

Weights and inputs are synthesised; timings do not depend on them."""
import argparse
import sys

import _bench_zoo as Z

JOINT_SHAPES = [(4, 192, 192, 32, 2), (4, 96, 96, 64, 4)]  # N, H, W, C, dilation
PRELU_SHAPE = (4, 96, 96, 128)
TRAIN_SHAPE = (4, 768, 768)
TRAIN = {"yaml": "cityscapes_cgnet.yaml", "shape": TRAIN_SHAPE, "aux_weight": 0.4}


def joint_leg(dtype, iters, repeats):
    import torch
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    out = {}
    for N, H, W, C, d in JOINT_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(N, H, W, C, device="cuda", generator=g).to(dtype)
        gy = torch.randn(N, H, W, 2 * C, device="cuda", generator=g).to(dtype)
        wl = torch.randn(C, 1, 3, 3, device="cuda", generator=g) * 0.3
        ws = torch.randn(C, 1, 3, 3, device="cuda", generator=g) * 0.3
        ws_taps = F._dw_taps(ws, 1, d)  # (packed once per step, not per call)
        buf = torch.empty(N, H, W, 2 * C, device="cuda", dtype=dtype)

        def joint_fwd():
            return K.cg_joint(x, wl, ws, d)

        def comp_fwd():
            _, p1 = K.dwconv(x, wl, 1, 1, None, buf[..., :C], True)
            _, p2 = K.dwconv(x, ws_taps, 1, d, None, buf[..., C:], True)
            return buf, p1, p2

        def bwd_pair_sum():
            g1, dw1, _ = F.dw_backward_fused(x, gy[..., :C], wl, 1, 1)
            g2, dw2, _ = F.dw_backward_fused(x, gy[..., C:], ws, 1, d)
            return K.sum_n([g1, g2]), dw1, dw2

        def bwd_pair_res():  # what functional._CGJointFn.backward runs
            g2, dw2, _ = F.dw_backward_fused(x, gy[..., C:], ws, 1, d)
            g1, dw1, _ = F.dw_backward_fused(x, gy[..., :C], wl, 1, 1, res=g2)
            return g1, dw1, dw2

        # the two paths compute the same thing
        yj, pj = joint_fwd()
        yc, p1, p2 = comp_fwd()
        tol = 2e-5 if dtype == torch.float32 else 8e-3
        assert (yj.float() - yc.float()).abs().max().item() <= tol * yc.float().abs().max().item()
        sj = pj.double().sum(0)
        sc = torch.cat([p1.double().sum(0), p2.double().sum(0)], 1)
        assert (sj - sc).abs().max().item() <= 1e-4 * sc.abs().max().item()
        c1, c2 = bwd_pair_sum(), bwd_pair_res()
        assert (c2[0].float() - c1[0].float()).abs().max().item() \
            <= 2 * tol * c1[0].float().abs().max().item()
        assert torch.equal(c1[1], c2[1]) and torch.equal(c1[2], c2[2])
        res = Z.measure({"joint_fwd": joint_fwd, "composed_fwd": comp_fwd,
                        "bwd_pair_sum": bwd_pair_sum, "bwd_pair_res": bwd_pair_res}, iters, repeats)
        eb = x.element_size()
        res["joint_fwd"]["bytes"] = 3 * x.numel() * eb          # read x, write 2C
        res["joint_fwd"]["TB_per_s"] = round(res["joint_fwd"]["bytes"]
                                             / (res["joint_fwd"]["median_us"] * 1e-6) / 1e12, 3)
        out["%dx%dx%dx%d_d%d" % (N, H, W, C, d)] = res
    return out


def prelu_leg(dtype, iters, repeats):
    import torch
    import torch.nn as nn
    import torch.nn.functional as TF
    from segmentron_amd import functional as F
    N, H, W, C = PRELU_SHAPE
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(N, H, W, C, device="cuda", generator=g).to(dtype).requires_grad_()
    gy = torch.randn(N, H, W, C, device="cuda", generator=g).to(dtype)
    gp = torch.randn(N, 1, 1, C, device="cuda", generator=g)
    bn = nn.BatchNorm2d(C).cuda().train()
    prelu = nn.PReLU(C).cuda()
    with torch.no_grad():
        prelu.weight.uniform_(0.05, 0.45)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)

    def hip_fwd():
        with torch.no_grad():
            return F.bn_prelu(F.bn_of_concat(x.detach(), bn), prelu, pool=True)

    def hip_fwd_bwd():
        y, p = F.bn_prelu(F.bn_of_concat(x, bn), prelu, pool=True)
        return torch.autograd.grad([y, p], [x, bn.weight, bn.bias, prelu.weight], [gy, gp])

    # ATen: the same math on a channels-last view (what the reference's modules run), on torch's
    # own kernels (no vendor library: its first call would search / compile for minutes)
    torch.backends.cudnn.enabled = False
    xa = x.detach().permute(0, 3, 1, 2).requires_grad_()
    gya, gpa = gy.permute(0, 3, 1, 2), gp.view(N, C)

    def aten(xin):
        z = TF.batch_norm(xin, None, None, bn.weight, bn.bias, True)  # (native kernel, fp32 stats)
        y = TF.prelu(z, prelu.weight.to(dtype))
        return y, y.float().mean((2, 3))

    def aten_fwd():
        with torch.no_grad():
            return aten(xa.detach())

    def aten_fwd_bwd():
        y, p = aten(xa)
        return torch.autograd.grad([y, p], [xa, bn.weight, bn.bias, prelu.weight], [gya, gpa])

    yh, ph = hip_fwd()
    ya, pa = aten_fwd()
    tol = 2e-5 if dtype == torch.float32 else 1.6e-2
    assert (yh.float() - ya.permute(0, 2, 3, 1).float()).abs().max().item() \
        <= tol * ya.float().abs().max().item()
    assert (ph.view(N, C) - pa).abs().max().item() <= tol * pa.abs().max().item()
    return Z.measure({"hip_fwd": hip_fwd, "hip_fwd_bwd": hip_fwd_bwd, "aten_fwd": aten_fwd,
                     "aten_fwd_bwd": aten_fwd_bwd}, iters, repeats)


def child(args):
    import torch
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.dtype]
    if args.leg == "joint":
        val = joint_leg(dtype, args.iters, args.repeats)
    elif args.leg == "prelu":
        val = prelu_leg(dtype, args.iters, args.repeats)
    else:
        val = Z.train_leg(TRAIN, dtype, args.steps, args.warmup, graph=args.leg == "train_graph")
    Z.emit_result(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20, help="calls per captured graph (op legs)")
    ap.add_argument("--repeats", type=int, default=9, help="timed replays per variant (op legs)")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--legs", default="joint,train_eager,train_graph,prelu")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) run this one leg in this process")
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    header = {"joint_shapes": JOINT_SHAPES, "prelu_shape": PRELU_SHAPE, "train_shape": TRAIN_SHAPE,
              "steps": args.steps, "warmup": args.warmup, "iters": args.iters,
              "repeats": args.repeats}
    legs = [("%s/%s" % (leg, dn), ["--leg", leg, "--dtype", dn])
            for leg in args.legs.split(",") for dn in args.dtypes.split(",")
            if dn == "bf16" or not leg.startswith("train")]
    return Z.run_legs(__file__, legs, args, header, passed=("steps", "warmup", "iters", "repeats"))


if __name__ == "__main__":
    sys.exit(main())
