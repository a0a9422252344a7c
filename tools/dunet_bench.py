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
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OP_SHAPE = (4, 96, 96, 8, 19)  # N, h, w, s, C
TRAIN_SHAPE = (4, 768, 768)
LEG_TIMEOUT = 420  # seconds per child


def graph_time(fn, iters):
    """`iters` calls captured into one HIP graph; microseconds per call of one timed replay."""
    import torch
    from segmentron_amd.graph import capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        with capture(graph, stream=side):
            for _ in range(iters):
                fn()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters
    return once


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
    timers = {name: graph_time(fn, iters) for name, fn in variants.items()}
    samples = {name: [] for name in variants}
    for _ in range(repeats):  # interleaved: drift hits every variant alike
        for name, once in timers.items():
            samples[name].append(once())
    res = {}
    for name, v in samples.items():
        v = sorted(v)
        res[name] = {"median_us": round(v[len(v) // 2], 2), "spread_us": round(v[-1] - v[0], 2)}
    eb = lo.element_size()
    traffic = {"fused_fwd": lo.numel() * eb + tgt.numel() * 8,
               "fused_bwd": 2 * lo.numel() * eb + tgt.numel() * 8}
    for name, nbytes in traffic.items():
        res[name]["bytes"] = nbytes
        res[name]["TB_per_s"] = round(nbytes / (res[name]["median_us"] * 1e-6) / 1e12, 3)
    return res


def train_leg(dtype, steps, warmup):
    import torch
    import torch.nn as nn
    import _dunet_oracle as O
    import segmentron_amd
    from oracle import synth
    from segmentron_amd.config import cfg, reset_cfg
    from segmentron_amd.solver.optimizer import get_optimizer
    os.environ["SEGMENTRON_HIP_GRAPH"] = "1"
    reset_cfg()
    cfg.update_from_file(os.path.join(ROOT, "tests", "golden", "cityscapes_dunet.yaml"))
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False", "SOLVER.AUX", "True",
                          "SOLVER.AUX_WEIGHT", str(O.AUX_WEIGHT)])
    cfg.PHASE = "train"
    cfg.check_and_freeze()
    segmentron_amd.set_compute_dtype(dtype)
    model = segmentron_amd.get_segmentation_model()
    model.load_state_dict(synth.synth_like(model.state_dict(), seed=0, conditioned=True))
    model = model.cuda().train()
    crit = nn.CrossEntropyLoss(ignore_index=-1)
    optimizer = get_optimizer(model)
    B, H, W = TRAIN_SHAPE
    x = synth.synth_images(B, H, W, seed=0).cuda()
    y = synth.synth_targets(B, H, W, seed=0).cuda()

    def step():
        outputs = model(x)
        loss = crit(outputs[0], y) + O.AUX_WEIGHT * crit(outputs[1], y)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    tg = model._transparent_graph
    assert tg.disabled is None and len(tg.segments) == 1, tg.disabled
    assert torch.isfinite(loss)
    reset_cfg()
    return {"ms_per_step": round(ms, 3), "img_per_s": round(B * 1e3 / ms, 2)}


def child(args):
    import torch
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.dtype]
    if args.leg == "op":
        val = op_leg(dtype, args.iters, args.repeats)
    else:
        val = train_leg(dtype, args.steps, args.warmup)
    print("RESULT " + json.dumps({"leg": args.leg, "dtype": args.dtype, "value": val,
                                  "device": torch.cuda.get_device_name(0)}))


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
    res = {"op_shape": OP_SHAPE, "train_shape": TRAIN_SHAPE, "steps": args.steps,
           "warmup": args.warmup, "iters": args.iters, "repeats": args.repeats, "results": {}}
    for leg in args.legs.split(","):
        for dn in args.dtypes.split(","):
            if leg == "train" and dn != "bf16":
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--dtype", dn,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--iters",
                   str(args.iters), "--repeats", str(args.repeats)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT)
            except subprocess.TimeoutExpired:
                sys.stderr.write("leg %s/%s ran past %d s: stopping\n" % (leg, dn, LEG_TIMEOUT))
                return 124
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:  # nothing more is started on the GPU
                sys.stderr.write("leg %s/%s failed (%d): stopping\n%s\n"
                                 % (leg, dn, p.returncode, p.stderr[-3000:]))
                return p.returncode or 1
            r = json.loads(line[0][len("RESULT "):])
            res["device"] = r["device"]
            res["results"]["%s/%s" % (leg, dn)] = r["value"]
            sys.stderr.write("%s/%s: %s\n" % (leg, dn, json.dumps(r["value"])))
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
