"""FPENet cost on one GPU — one JSON line.

  stage       one stage of the FPE pyramid (csrc/fpenet.hip) at the workload's shapes, a
              4 x 768 x 768 batch in bf16 — [4,384,384] x 4 (layer1.0), [4,192,192] x 16 and x 8
              (layer2), [4,96,96] x 32 and x 16 (layer3) — operands and results as n-channel slices
              of 4n-channel buffers: dilation 1 without `b` (stage 0), dilations 2, 4, 8 with it.
                hip_fwd       seg_fpe_stage_fwd with the side output and the statistics rows
                hip_bwd       seg_fpe_stage_bwd and the two BatchNorm-backward applies on its
                              gradients (seg_fpe_bn_bwd_apply)
                composed_fwd  the parent's kernels, where their contract admits the shape (bf16: n a
                              multiple of 8): seg_bn_apply with a residual (the sum), seg_bn_apply
                              (the concat slice), seg_dwconv3x3 with statistics; stage 0: the
                              depthwise launch with its prologue alone
                composed_bwd  the depthwise backward of the materialised sum, then per operand the
                              masked reduce and the masked BatchNorm-backward apply (and the 2-ary
                              sum with `res` for b)
  stage_aten  the same stages on torch's own kernels (dense channels-last bf16 tensors): forward,
              and forward + backward through autograd
  meu         seg_meu_fwd, seg_meu_bwd_low and seg_meu_bwd_high at 96 -> 192 x 64 and
              192 -> 384 x 32 (each backward with the BatchNorm-backward apply that follows it)
  meu_aten    the MEU tail on torch's own kernels: forward, and forward + backward
  train       ms/step and img/s of the reference's loop statements (model, cross-entropy,
              zero_grad, backward, SGD step) at 4 x 3 x 768 x 768, bf16: eager launches,
              SEGMENTRON_HIP_GRAPH=1, and the torch restatement (tests/_fpenet_oracle.py) on torch's
              own kernels under bf16 autocast (forward + loss + backward only)

Every op variant is captured `--iters` times into ONE HIP graph and the replay is timed,
`--repeats` times, the variants interleaved: median and spread (max - min) in microseconds per
call.  ATen runs on torch's own kernels (no vendor convolution library: its first call would
search for minutes).  Every leg runs in a child process of its own under a time limit; the first
leg that fails ends the run.

    python tools/fpenet_bench.py [--legs stage,stage_aten,meu,meu_aten,train_eager,train_graph,
                                         train_aten] [--out FILE]

Weights and inputs are synthesised; timings do not depend on them."""
import argparse
import json
import sys

import _bench_zoo as Z

# N, H, W, n
STAGE_SHAPES = [(4, 384, 384, 4), (4, 192, 192, 16), (4, 192, 192, 8), (4, 96, 96, 32),
                (4, 96, 96, 16)]
# N, (h2, w2), (h, w), C
MEU_SHAPES = [(4, (96, 96), (192, 192), 64), (4, (192, 192), (384, 384), 32)]
DILS = (1, 2, 4, 8)
TRAIN_SHAPE = (4, 768, 768)
TRAIN = {"yaml": "cityscapes_fpenet.yaml", "shape": TRAIN_SHAPE, "aux_weight": 0.4}


def _rand(shape, g, dt):
    import torch
    return torch.randn(shape, device="cuda", generator=g).to(dt)


def _vecs(n, g, k):
    import torch
    return [torch.rand(n, device="cuda", generator=g) + 0.5 for _ in range(k)]


def _stage_operands(N, H, W, n, dt):
    """Slice s = 1 of 4n-channel buffers, as the pyramid node lays them out."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    bufs = {k: _rand((N, H, W, 4 * n), g, dt) for k in ("u", "yraw", "dy", "res", "out", "ga", "gb")}
    t = {"a": bufs["u"][..., n:2 * n], "b": bufs["yraw"][..., :n], "y": bufs["yraw"][..., n:2 * n],
         "o": bufs["out"][..., :n], "dy": bufs["dy"][..., n:2 * n], "res": bufs["res"][..., :n],
         "ga": bufs["ga"][..., n:2 * n], "gb": bufs["gb"][..., :n]}
    t["sa"], t["ta"], t["sb"], t["tb"], t["c0"], t["c1"] = _vecs(n, g, 6)
    t["ta"], t["tb"] = t["ta"] - 1.0, t["tb"] - 1.0
    t["w"] = torch.randn((n, 1, 3, 3), device="cuda", generator=g) * 0.3
    return t


def stage_leg(iters, repeats):
    import torch
    from segmentron_amd import functional as F
    from segmentron_amd import hip_ops as K
    dt = torch.bfloat16
    AR = K.PRO_AFFINE_RELU
    out = {}
    for N, H, W, n in STAGE_SHAPES:
        t = _stage_operands(N, H, W, n, dt)
        a, b, w = t["a"], t["b"], t["w"]
        pro_a, pro_b = (AR, t["sa"], t["ta"]), (AR, t["sb"], t["tb"])
        wparam = torch.nn.Parameter(w)
        rows = K.fpe_stage_rows(dt, N, H, W, n)
        pa = torch.empty((rows, 2, 4 * n), dtype=torch.float32, device="cuda")
        s_in = torch.empty((N, H, W, n), dtype=dt, device="cuda")
        for d in DILS:
            has_b = d > 1
            kw = dict(b=b, sb=t["sb"], tb=t["tb"]) if has_b else {}

            def hip_fwd():
                K.fpe_stage_fwd(a, t["sa"], t["ta"], w, d, out=t["y"],
                                **(dict(kw, b_act=t["o"]) if has_b else {}))

            def hip_bwd():
                K.fpe_stage_bwd(t["dy"], a, t["sa"], t["ta"], w, d, ga=t["ga"], pa=pa, pa_col=n,
                                **(dict(kw, res=t["res"], gb=t["gb"]) if has_b else {}))
                K.fpe_bn_bwd_apply(t["ga"], a, t["sa"], t["c0"], t["c1"], out=t["ga"])
                if has_b:
                    K.fpe_bn_bwd_apply(t["gb"], b, t["sb"], t["c0"], t["c1"], out=t["gb"])
            variants = {"hip_fwd": hip_fwd, "hip_bwd": hip_bwd}
            if n % K.vec_of(dt) == 0:
                taps = F._dw_taps(wparam, 1, d)

                def composed_fwd():
                    if not has_b:
                        return K.dwconv(a, taps, 1, d, pro_a, t["y"], True)
                    K.bn_apply(a, pro_a, b, pro_b, out=s_in)
                    K.bn_apply(b, pro_b, out=t["o"])
                    return K.dwconv(s_in, taps, 1, d, None, t["y"], True)

                def composed_bwd():
                    if not has_b:  # (stride 1: the one-pass half, as _DwFn.backward runs it)
                        g = F.dw_backward(a, t["dy"], wparam, 1, d, pro_a, want_bn=True)[0]
                        return K.bn_bwd_apply(g, a, (K.PRO_AFFINE, t["sa"], t["ta"]), t["c0"],
                                              t["c1"], out=t["ga"])
                    g = F.dw_backward(s_in, t["dy"], wparam, 1, d)[0]
                    K.bn_bwd_reduce_partial(g, a, pro_a)
                    K.bn_bwd_apply(g, a, pro_a, t["c0"], t["c1"], out=t["ga"])
                    if has_b:
                        gs = K.sum_n([g, t["res"]])
                        K.bn_bwd_reduce_partial(gs, b, pro_b)
                        K.bn_bwd_apply(gs, b, pro_b, t["c0"], t["c1"], out=t["gb"])
                variants.update(composed_fwd=composed_fwd, composed_bwd=composed_bwd)
            key = "%dx%dx%dx%d/d%d" % (N, H, W, n, d)
            out[key] = Z.measure(variants, iters, repeats)
            sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
    return out


def stage_aten_leg(iters, repeats):
    import torch
    import torch.nn.functional as TF
    torch.backends.cudnn.enabled = False
    dt = torch.bfloat16
    out = {}
    for N, H, W, n in STAGE_SHAPES:
        t = _stage_operands(N, H, W, n, dt)

        def cl(x):  # dense channels-last NCHW view
            return x.contiguous().permute(0, 3, 1, 2)
        a, b, dy, res = (cl(t[k]).requires_grad_(k in "ab") for k in ("a", "b", "dy", "res"))
        sa, ta, sb, tb = (t[k].to(dt).view(1, n, 1, 1) for k in ("sa", "ta", "sb", "tb"))
        w = t["w"].to(dt).requires_grad_()
        for d in DILS:
            has_b = d > 1

            def fwd():
                x = TF.relu(a * sa + ta)
                rb = None
                if has_b:
                    rb = TF.relu(b * sb + tb)
                    x = x + rb
                return TF.conv2d(x, w, None, 1, d, d, n), rb

            def fwd_only():
                with torch.no_grad():
                    fwd()

            def fwd_bwd():
                y, rb = fwd()
                if has_b:
                    torch.autograd.grad([y, rb], [a, b, w], [dy, res])
                else:
                    torch.autograd.grad([y], [a, w], [dy])
            key = "%dx%dx%dx%d/d%d" % (N, H, W, n, d)
            out[key] = Z.measure({"aten_fwd": fwd_only, "aten_fwd_bwd": fwd_bwd}, iters, repeats)
            sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
    return out


def _meu_operands(N, hw2, hw, C, dt):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    (h2, w2), (h, w) = hw2, hw
    t = {"L": _rand((N, h, w, C), g, dt), "H": _rand((N, h2, w2, C), g, dt),
         "g": _rand((N, h, w, C), g, dt),
         "a": torch.rand((N, C), device="cuda", generator=g),
         "dpool": torch.randn((N, C), device="cuda", generator=g),
         "wsa": torch.full((1,), 1.3, device="cuda")}
    t["sl"], t["tl"], t["sh"], t["th"], t["c0"], t["c1"] = _vecs(C, g, 6)
    return t


def meu_leg(iters, repeats):
    import torch
    from segmentron_amd import hip_ops as K
    dt = torch.bfloat16
    out = {}
    for N, hw2, hw, C in MEU_SHAPES:
        t = _meu_operands(N, hw2, hw, C, dt)
        aff_l, aff_h = (t["sl"], t["tl"]), (t["sh"], t["th"])
        o = torch.empty_like(t["L"])
        dl = torch.empty_like(t["L"])
        dh = torch.empty_like(t["H"])
        _, sa = K.meu_fwd(t["L"], aff_l, t["H"], aff_h, t["a"], t["wsa"], out=o)

        def bwd_low():
            K.meu_bwd_low(t["g"], t["L"], aff_l, t["H"], aff_h, t["a"], t["wsa"], sa, out=dl)
            K.bn_bwd_apply(dl, t["L"], (K.PRO_AFFINE, t["sl"], t["tl"]), t["c0"], t["c1"], out=dl)

        def bwd_high():
            K.meu_bwd_high(t["g"], sa, t["H"], t["dpool"], out=dh)
            K.bn_bwd_apply(dh, t["H"], (K.PRO_AFFINE, t["sh"], t["th"]), t["c0"], t["c1"], out=dh)
        variants = {
            "hip_fwd": lambda: K.meu_fwd(t["L"], aff_l, t["H"], aff_h, t["a"], t["wsa"], out=o),
            "hip_bwd_low": bwd_low, "hip_bwd_high": bwd_high}
        key = "%dx%dx%d->%dx%dx%d" % ((N,) + hw2 + hw + (C,))
        out[key] = Z.measure(variants, iters, repeats)
        sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
    return out


def meu_aten_leg(iters, repeats):
    import torch
    import torch.nn.functional as TF
    dt = torch.bfloat16
    out = {}
    for N, hw2, hw, C in MEU_SHAPES:
        t = _meu_operands(N, hw2, hw, C, dt)
        L = t["L"].permute(0, 3, 1, 2).requires_grad_()
        Hr = t["H"].permute(0, 3, 1, 2).requires_grad_()
        g = t["g"].permute(0, 3, 1, 2)
        a = t["a"].to(dt).view(N, C, 1, 1).requires_grad_()
        wsa = t["wsa"].to(dt).requires_grad_()
        sl, tl, sh, th = (t[k].to(dt).view(1, C, 1, 1) for k in ("sl", "tl", "sh", "th"))
        dpool = t["dpool"].to(dt).view(N, C, 1, 1)

        def fwd():
            low, high = L * sl + tl, Hr * sh + th
            sa = torch.sigmoid(wsa * low.mean(1, keepdim=True))
            up = TF.interpolate(high, size=hw, mode="bilinear", align_corners=True)
            return a * low + sa * up, high.mean((2, 3), keepdim=True)

        def fwd_only():
            with torch.no_grad():
                fwd()

        def fwd_bwd():
            torch.autograd.grad(list(fwd()), [L, Hr, a, wsa], [g, dpool])
        key = "%dx%dx%d->%dx%dx%d" % ((N,) + hw2 + hw + (C,))
        out[key] = Z.measure({"aten_fwd": fwd_only, "aten_fwd_bwd": fwd_bwd}, iters, repeats)
        sys.stderr.write("%s %s\n" % (key, json.dumps(out[key])))
    return out


def child(args):
    import torch
    legs = {"stage": stage_leg, "stage_aten": stage_aten_leg, "meu": meu_leg,
            "meu_aten": meu_aten_leg}
    if args.leg in legs:
        val = legs[args.leg](args.iters, args.repeats)
    elif args.leg == "train_aten":
        from _fpenet_spec import FPENET
        val = Z.train_aten_leg(FPENET, TRAIN_SHAPE, args.steps, args.warmup)
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
    ap.add_argument("--legs", default="stage,stage_aten,meu,meu_aten,train_eager,train_graph,"
                                      "train_aten")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    header = {"stage_shapes": STAGE_SHAPES, "meu_shapes": MEU_SHAPES, "train_shape": TRAIN_SHAPE,
              "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "iters": args.iters,
              "repeats": args.repeats}
    legs = [(leg, ["--leg", leg]) for leg in args.legs.split(",")]
    return Z.run_legs(__file__, legs, args, header, passed=("steps", "warmup", "iters", "repeats"))


if __name__ == "__main__":
    sys.exit(main())
