"""EDANet cost on one GPU — one JSON line.

  line      the 40-channel 3-tap line convolution (csrc/conv_line.hip) at EDANet's own shapes for
            a 4 x 512 x 1024 batch — [4,128,256,40] (stage 1) and [4,64,128,40] (stage 2), both
            axes, dilation 1, 2 and 16, operands and results as 40-channel slices of the stage
            buffers' pitch (264 / 456): forward with bias and statistics, data gradient with the
            statistics row that carries the producer's bias gradient, and weight gradient
            (seg_colsum included), against ATen's conv2d / convolution_backward on dense
            channels-last tensors of the same size on the same device.  Achieved bytes/s next to
            each time: the tensors a launch must read and write once.
  pair      the fused (3,1) -> (1,3) pair (csrc/conv_line_pair.hip: both biases, statistics, `mid`
            written) against the two single launches it replaces, in the same graph-replay
            harness: [4,128,256,40] and [4,64,128,40], dilation 1, 2 and 16, both axis orders
  launches  the device kernels of stage 1 (DownsamplerBlock 2 and the five dense blocks, 60 -> 260
            channels), forward and backward, in launch order (torch.profiler, as
            tools/step_trace.py): no cat, no slice backward, no zero-fill of a full-size tensor
            and no element-wise add may appear among them
  train     ms/step and img/s of the reference's loop statements (model, cross-entropy,
            zero_grad, backward, SGD step) at 4 x 3 x 512 x 1024, bf16: eager launches,
            SEGMENTRON_HIP_GRAPH=1 (each also with SEG_LINE_PAIR=0 and =1: every pair as two
            launches / as one wherever the kernel can run), and the torch restatement (tests/_edanet_oracle.py) on torch's
            own kernels under bf16 autocast (forward + loss + backward only)

Every op variant is captured `--iters` times into ONE HIP graph and the replay is timed,
`--repeats` times, the variants interleaved: median and spread (max - min) in microseconds per
call.  ATen runs on torch's own kernels (no vendor convolution library: its first call would
search for minutes).  Every leg runs in a child process of its own under a time limit; the first
leg that fails ends the run.

    python tools/edanet_bench.py [--legs line,pair,launches,train_eager,train_graph,
                                         train_eager_pair0,train_eager_pair1,train_graph_pair0,
                                         train_graph_pair1,train_aten]
                                 [--out FILE]

Weights and inputs are synthesised; timings do not depend on them."""
import argparse
import json
import os
import sys

import _bench_zoo as Z

C = 40
# N, H, W, pitch of the stage buffer, dilations
LINE_SHAPES = [(4, 128, 256, 264, (1, 2)), (4, 64, 128, 456, (2, 16))]
TRAIN_SHAPE = (4, 512, 1024)
TRAIN = {"yaml": "cityscapes_edanet.yaml", "shape": TRAIN_SHAPE, "aux_weight": 0.4}


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
    for N, H, W, pitch, dils in LINE_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        xb = torch.randn(N, H, W, pitch, device="cuda", generator=g).to(dt)
        gb = torch.randn(N, H, W, pitch, device="cuda", generator=g).to(dt)
        ob = torch.empty(N, H, W, pitch, device="cuda", dtype=dt)
        x, dy, o = xb[..., 40:80], gb[..., 80:120], ob[..., 120:160]
        xa = x.contiguous().permute(0, 3, 1, 2)  # dense channels-last NCHW views
        dya = dy.contiguous().permute(0, 3, 1, 2)
        bias = torch.randn(C, device="cuda", generator=g)
        elems = N * H * W * C * 2
        nbytes = {"fwd": 2 * elems, "dgrad": 2 * elems, "wgrad": 2 * elems}
        for axis in (K.AXIS_H, K.AXIS_W):
            for d in dils:
                shape = (C, C, 3, 1) if axis == K.AXIS_H else (C, C, 1, 3)
                pad, dil = ((d, 0), (d, 1)) if axis == K.AXIS_H else ((0, d), (1, d))
                w = torch.randn(shape, device="cuda", generator=g) * (3 * C) ** -0.5
                wp = F.pack_conv_weight(w, C, dt)
                wt = F.pack_conv_weight_dgrad(w, C, dt)
                wa = w.to(dt).contiguous(memory_format=torch.channels_last)
                ba = bias.to(dt)

                def bwd(mask):
                    return torch.ops.aten.convolution_backward(
                        dya, xa, wa, None, (1, 1), pad, dil, False, (0, 0), 1, mask)
                variants = {
                    "hip_fwd": lambda: K.conv_line_bias(x, wp, bias, axis, d, out=o,
                                                        want_stats=True),
                    "hip_dgrad": lambda: K.conv_line_bias(dy, wt, None, axis, d, out=o,
                                                          want_stats=True),
                    "hip_wgrad": lambda: K.conv_line_wgrad(x, dy, axis, d),
                    "aten_fwd": lambda: TF.conv2d(xa, wa, ba, 1, pad, dil),
                    "aten_dgrad": lambda: bwd((True, False, False))[0],
                    "aten_wgrad": lambda: bwd((False, True, False))[1],
                }
                key = "%dx%dx%dx%d/%s/d%d" % (N, H, W, C, "HW"[axis], d)
                out[key] = _with_rates(Z.measure(variants, iters, repeats), nbytes)
                sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
    return out


def pair_leg(iters, repeats):
    import torch
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    dt = torch.bfloat16
    out = {}
    for N, H, W, pitch, _ in LINE_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        xb = torch.randn(N, H, W, pitch, device="cuda", generator=g).to(dt)
        ob = torch.empty(N, H, W, pitch, device="cuda", dtype=dt)
        x, o = xb[..., 40:80], ob[..., 120:160]
        ba = torch.randn(C, device="cuda", generator=g)
        bb = torch.randn(C, device="cuda", generator=g)
        wh = torch.randn((C, C, 3, 1), device="cuda", generator=g) * (3 * C) ** -0.5
        ww = torch.randn((C, C, 1, 3), device="cuda", generator=g) * (3 * C) ** -0.5
        ph, pw = F.pack_conv_weight(wh, C, dt), F.pack_conv_weight(ww, C, dt)
        for order in (0, 1):
            pa, pb = (ph, pw) if order == 0 else (pw, ph)
            ax_a, ax_b = (K.AXIS_H, K.AXIS_W) if order == 0 else (K.AXIS_W, K.AXIS_H)
            for d in (1, 2, 16):
                def two():
                    mid, _ = K.conv_line_bias(x, pa, ba, ax_a, d)
                    return K.conv_line_bias(mid, pb, bb, ax_b, d, out=o, want_stats=True)
                variants = {
                    "pair": lambda: K.conv_line_pair(x, pa, ba, pb, bb, order, d, out=o,
                                                     want_mid=True, want_stats=True),
                    "pair_nomid": lambda: K.conv_line_pair(x, pa, ba, pb, bb, order, d, out=o,
                                                           want_mid=False, want_stats=True),
                    "two_launches": two,
                }
                key = "%dx%dx%dx%d/%s/d%d" % (N, H, W, C, ("HW", "WH")[order], d)
                out[key] = Z.measure(variants, iters, repeats)
                sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
    return out


def launches_leg():
    """Device kernels of stage 1 at [4, 256, 512, 16] -> [4, 128, 256, 264], forward and backward,
    in launch order."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    from segmentron_amd import functional as F
    os.environ["SEGMENTRON_HIP_GRAPH"] = "0"
    model, _ = Z.build_model(TRAIN["yaml"], torch.bfloat16)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    x = torch.randn(4, 256, 512, 16, device="cuda").to(torch.bfloat16).relu_()
    x[..., 15] = 0
    x.requires_grad_()
    go = torch.randn(4, 128, 256, 264, device="cuda").to(torch.bfloat16)
    go[..., 260:] = 0
    leaves = [x] + [p for layer in model.layers[1:7] for p in layer.parameters()]
    names = {}

    def fwd():  # (inside a model forward the BatchNorm counters are one deferred launch)
        with F.bn_counter_scope():
            return model._stage(model.layers[2:7], model.layers[1], x)
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
    elif args.leg == "pair":
        val = pair_leg(args.iters, args.repeats)
    elif args.leg == "launches":
        val = launches_leg()
    elif args.leg == "train_aten":
        from _edanet_spec import EDANET
        val = Z.train_aten_leg(EDANET, TRAIN_SHAPE, args.steps, args.warmup)
    else:
        if args.leg.endswith(("_pair0", "_pair1")):
            os.environ["SEG_LINE_PAIR"] = args.leg[-1]
        val = Z.train_leg(TRAIN, torch.bfloat16, args.steps, args.warmup,
                          graph=args.leg.startswith("train_graph"))
    Z.emit_result(val)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20, help="calls per captured graph (op legs)")
    ap.add_argument("--repeats", type=int, default=9, help="timed replays per variant (op legs)")
    ap.add_argument("--legs", default="line,pair,launches,train_eager,train_graph,train_eager_pair0,"
                                      "train_eager_pair1,train_graph_pair0,train_graph_pair1,"
                                      "train_aten")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    header = {"line_shapes": LINE_SHAPES, "train_shape": TRAIN_SHAPE, "dtype": "bf16",
              "steps": args.steps, "warmup": args.warmup, "iters": args.iters,
              "repeats": args.repeats}
    legs = [(leg, ["--leg", leg]) for leg in args.legs.split(",")]
    return Z.run_legs(__file__, legs, args, header, passed=("steps", "warmup", "iters", "repeats"))


if __name__ == "__main__":
    sys.exit(main())
