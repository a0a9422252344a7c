"""LEDNet cost on one GPU — one JSON line.

  line      the 3-tap line convolution (csrc/conv_line.hip) at LEDNet's own shapes for the
            config's 4 x 768 x 768 crop — one channel half of [4,384,384,32], [4,192,192,64] and
            [4,96,96,128] (the last at dilation 1, 2, 5, 9, 17), both axes: forward, data gradient
            (the same kernel with the residual addend) and weight gradient (seg_colsum included),
            against ATen's conv2d / convolution_backward on dense channels-last tensors of the same
            size on the same device.  Achieved bytes/s next to each time: the tensors a launch
            must read and write once (x and y; dy, add and dx; x and dy).
  tail      seg_ssnbt_tail_fwd / _bwd at the three block shapes against the torch composition
            (affine, relu, cat, add, relu, channel shuffle, and autograd through them)
  launches  the device kernels of one SSnbt block, forward and backward, in launch order
  train     ms/step and img/s of the reference's loop statements (model, cross-entropy,
            zero_grad, backward, SGD step) at 4 x 3 x 768 x 768, bf16: eager launches,
            SEGMENTRON_HIP_GRAPH=1, and the torch restatement (tests/_lednet_oracle.py) on torch's
            own kernels under bf16 autocast (forward + loss + backward only)

Every op variant is captured `--iters` times into ONE HIP graph and the replay is timed,
`--repeats` times, the variants interleaved: median and spread (max - min) in microseconds per
call.  ATen runs on torch's own kernels (no vendor convolution library: its first call would
search for minutes).  Every leg runs in a child process of its own under a time limit; the first
leg that fails ends the run.

    python tools/lednet_bench.py [--legs line,tail,launches,train_eager,train_graph,train_aten]
                                 [--out FILE]

Weights and inputs are synthesised; timings do not depend on them."""
import argparse
import json
import os
import sys

import _bench_zoo as Z

# N, H, W, C (one branch: half of the block's channels), dilations
LINE_SHAPES = [(4, 384, 384, 16, (1,)), (4, 192, 192, 32, (1,)), (4, 96, 96, 64, (1, 2, 5, 9, 17))]
TAIL_SHAPES = [(4, 384, 384, 32), (4, 192, 192, 64), (4, 96, 96, 128)]
TRAIN_SHAPE = (4, 768, 768)
TRAIN = {"yaml": "cityscapes_lednet.yaml", "shape": TRAIN_SHAPE, "aux_weight": 0.4}


def _with_rates(res, nbytes):
    for name, r in res.items():
        r["GB_per_s"] = round(nbytes[name.split("_", 1)[1]] / (r["median_us"] * 1e-6) / 1e9, 1)
    return res


def line_leg(iters, repeats):
    import torch
    import torch.nn.functional as TF
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    torch.backends.cudnn.enabled = False
    dt = torch.bfloat16
    out = {}
    for N, H, W, C, dils in LINE_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        xb = torch.randn(N, H, W, 2 * C, device="cuda", generator=g).to(dt)
        gb = torch.randn(N, H, W, 2 * C, device="cuda", generator=g).to(dt)
        ab = torch.randn(N, H, W, 2 * C, device="cuda", generator=g).to(dt)
        ob = torch.empty(N, H, W, 2 * C, device="cuda", dtype=dt)
        x, dy, add, o = xb[..., :C], gb[..., C:], ab[..., :C], ob[..., :C]
        xa = xb[..., :C].contiguous().permute(0, 3, 1, 2)  # dense channels-last NCHW views
        dya = gb[..., C:].contiguous().permute(0, 3, 1, 2)
        adda = ab[..., :C].contiguous().permute(0, 3, 1, 2)
        elems = N * H * W * C * 2
        nbytes = {"fwd": 2 * elems, "dgrad": 3 * elems, "wgrad": 2 * elems}
        for axis in (K.AXIS_H, K.AXIS_W):
            for d in dils:
                shape = (C, C, 3, 1) if axis == K.AXIS_H else (C, C, 1, 3)
                pad, dil = ((d, 0), (d, 1)) if axis == K.AXIS_H else ((0, d), (1, d))
                w = torch.randn(shape, device="cuda", generator=g) * (3 * C) ** -0.5
                wp = F.pack_conv_weight(w, C, dt)
                wt = F.pack_conv_weight_dgrad(w, C, dt)
                wa = w.to(dt).contiguous(memory_format=torch.channels_last)

                def bwd(mask):
                    return torch.ops.aten.convolution_backward(
                        dya, xa, wa, None, (1, 1), pad, dil, False, (0, 0), 1, mask)
                variants = {
                    "hip_fwd": lambda: K.conv_line(x, wp, axis, d, out=o),
                    "hip_dgrad": lambda: K.conv_line(dy, wt, axis, d, out=o, add=add),
                    "hip_wgrad": lambda: K.conv_line_wgrad(x, dy, axis, d),
                    "aten_fwd": lambda: TF.conv2d(xa, wa, None, 1, pad, dil),
                    "aten_dgrad": lambda: bwd((True, False, False))[0] + adda,
                    "aten_wgrad": lambda: bwd((False, True, False))[1],
                }
                key = "%dx%dx%dx%d/%s/d%d" % (N, H, W, C, "HW"[axis], d)
                out[key] = _with_rates(Z.measure(variants, iters, repeats), nbytes)
                sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
    return out


def _shuffle(x):
    n, c, h, w = x.shape
    return x.view(n, 2, c // 2, h, w).transpose(1, 2).contiguous().view(n, c, h, w)


def tail_leg(iters, repeats):
    import torch
    from segmentron_amd import hip_ops as K
    dt = torch.bfloat16
    out = {}
    for N, H, W, C in TAIL_SHAPES:
        h = C // 2
        g = torch.Generator(device="cuda").manual_seed(0)
        yb = torch.randn(N, H, W, C, device="cuda", generator=g).to(dt)
        x = torch.randn(N, H, W, C, device="cuda", generator=g).to(dt)
        go = torch.randn(N, H, W, C, device="cuda", generator=g).to(dt)
        s = [0.5 + torch.rand(h, device="cuda", generator=g) for _ in range(2)]
        t = [torch.randn(h, device="cuda", generator=g) * 0.3 for _ in range(2)]
        res = K.ssnbt_tail_fwd(yb[..., :h], s[0], t[0], yb[..., h:], s[1], t[1], x)
        ya = yb.permute(0, 3, 1, 2).requires_grad_()
        xa = x.permute(0, 3, 1, 2).requires_grad_()
        goa = go.permute(0, 3, 1, 2)
        sc = torch.cat(s).to(dt).view(1, C, 1, 1)
        sh = torch.cat(t).to(dt).view(1, C, 1, 1)

        def aten(yin, xin):
            return _shuffle(torch.relu(torch.relu(yin * sc + sh) + xin))

        def aten_fwd():
            with torch.no_grad():
                return aten(ya.detach(), xa.detach())

        def aten_fwd_bwd():
            return torch.autograd.grad(aten(ya, xa), [ya, xa], goa)
        elems = N * H * W * C * 2
        variants = {
            "hip_fwd": lambda: K.ssnbt_tail_fwd(yb[..., :h], s[0], t[0], yb[..., h:], s[1], t[1], x),
            "hip_bwd": lambda: K.ssnbt_tail_bwd(go, res),
            "aten_fwd": aten_fwd,
            "aten_fwdbwd": aten_fwd_bwd,
        }
        r = Z.measure(variants, iters, repeats)
        r["hip_fwd"]["GB_per_s"] = round(3 * elems / (r["hip_fwd"]["median_us"] * 1e-6) / 1e9, 1)
        r["hip_bwd"]["GB_per_s"] = round(3 * elems / (r["hip_bwd"]["median_us"] * 1e-6) / 1e9, 1)
        out["%dx%dx%dx%d" % (N, H, W, C)] = r
    return out


def launches_leg():
    """Device kernels of one SSnbt block (128 channels at [4,96,96], dilation 5), forward and
    backward, in launch order."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    os.environ["SEGMENTRON_HIP_GRAPH"] = "0"
    model, _ = Z.build_model(TRAIN["yaml"], torch.bfloat16)
    block = model.encoder[10]
    x = torch.randn(4, 96, 96, 128, device="cuda").to(torch.bfloat16).relu_().requires_grad_()
    go = torch.randn(4, 96, 96, 128, device="cuda").to(torch.bfloat16)
    from segmentron_amd import functional as F
    names = {}
    leaves = [x] + list(block.parameters())

    def fwd():  # (inside a model forward the BatchNorm counters are one deferred launch)
        with F.bn_counter_scope():
            return block(x)
    torch.autograd.grad(fwd(), leaves, go)
    torch.cuda.synchronize()
    for phase in ("forward", "backward"):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            if phase == "forward":
                out = fwd()
            else:
                torch.autograd.grad(out, leaves, go)
            torch.cuda.synchronize()
        evs = sorted((e for e in prof.events() if e.device_type.name == "CUDA"),
                     key=lambda e: e.time_range.start)
        names[phase] = [e.name.split("(")[0][:80] for e in evs]
    return names


def child(args):
    import torch
    if args.leg == "line":
        val = line_leg(args.iters, args.repeats)
    elif args.leg == "tail":
        val = tail_leg(args.iters, args.repeats)
    elif args.leg == "launches":
        val = launches_leg()
    elif args.leg == "train_aten":
        from _zoo import LEDNET
        val = Z.train_aten_leg(LEDNET, TRAIN_SHAPE, args.steps, args.warmup)
    else:
        val = Z.train_leg(TRAIN, torch.bfloat16, args.steps, args.warmup,
                          graph=args.leg == "train_graph")
    Z.emit_result(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20, help="calls per captured graph (op legs)")
    ap.add_argument("--repeats", type=int, default=9, help="timed replays per variant (op legs)")
    ap.add_argument("--legs", default="line,tail,launches,train_eager,train_graph,train_aten")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    header = {"line_shapes": LINE_SHAPES, "tail_shapes": TAIL_SHAPES, "train_shape": TRAIN_SHAPE,
              "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "iters": args.iters,
              "repeats": args.repeats}
    legs = [(leg, ["--leg", leg]) for leg in args.legs.split(",")]
    return Z.run_legs(__file__, legs, args, header, passed=("steps", "warmup", "iters", "repeats"))


if __name__ == "__main__":
    sys.exit(main())
