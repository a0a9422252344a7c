"""What the per-model benches (tools/<m>_bench.py) share: the timers, the model builder, the train
legs, and the parent / child pair that runs every leg in a process of its own."""
import itertools
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LEG_TIMEOUT = 420  # seconds per child


def timed(fn, steps, warmup):
    """Milliseconds per call of `fn`: warmed, eager, device-synchronised."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


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


def measure(variants, iters, repeats):
    """-> {name: median and spread (max - min) in microseconds per call} of `repeats` replays."""
    timers = {name: graph_time(fn, iters) for name, fn in variants.items()}
    samples = {name: [] for name in variants}
    for _ in range(repeats):  # interleaved: drift hits every variant alike
        for name, once in timers.items():
            samples[name].append(once())
    res = {}
    for name, v in samples.items():
        v = sorted(v)
        res[name] = {"median_us": round(v[len(v) // 2], 2), "spread_us": round(v[-1] - v[0], 2)}
    return res


def rotating(make, call, n):
    """A variant that cycles through `n` operand sets built by `make(i)`."""
    it = itertools.cycle([make(i) for i in range(n)])
    return lambda: call(next(it))


def build_model(yaml, dtype, phase="train", state=None, overrides=()):
    """-> (the HIP model on the device in training mode, its state): `yaml` of tests/golden, the
    state `state(keys and shapes)`, or synthesised like the model's own when None."""
    import segmentron_amd
    from oracle import synth
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(os.path.join(ROOT, "tests", "golden", yaml))
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False"] + list(overrides))
    cfg.PHASE = phase
    cfg.check_and_freeze()
    segmentron_amd.set_compute_dtype(dtype)
    model = segmentron_amd.get_segmentation_model()
    if state is None:
        sd = synth.synth_like(model.state_dict(), seed=0, conditioned=True)
    else:
        sd = state([(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    model.load_state_dict(sd)
    return model.cuda().train(), sd


def _rate(ms, batch):
    return {"ms_per_step": round(ms, 3), "img_per_s": round(batch * 1e3 / ms, 2)}


def train_leg(spec, dtype, steps, warmup, graph, before_build=None):
    """ms/step and img/s of the reference's loop statements (model, cross-entropy of every output,
    zero_grad, backward, SGD step) at `spec["shape"]`, eager or under the transparent graph."""
    import torch
    import torch.nn as nn
    from oracle import synth
    from segmentron_amd.config import reset_cfg
    from segmentron_amd.solver.optimizer import get_optimizer
    os.environ["SEGMENTRON_HIP_GRAPH"] = "1" if graph else "0"
    if before_build:
        before_build()
    model, _ = build_model(spec["yaml"], dtype, state=spec.get("state"),
                           overrides=spec.get("overrides", ()))
    crit = nn.CrossEntropyLoss(ignore_index=-1)
    optimizer = get_optimizer(model)
    B, H, W = spec["shape"]
    x = synth.synth_images(B, H, W, seed=0).cuda()
    y = synth.synth_targets(B, H, W, seed=0).cuda()
    last = []

    def step():
        outputs = model(x)
        loss = crit(outputs[0], y)
        for o in outputs[1:]:
            loss = loss + spec["aux_weight"] * crit(o, y)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        last[:] = [loss]
    ms = timed(step, steps, warmup)
    if graph:
        tg = model._transparent_graph
        assert tg.disabled is None and len(tg.segments) == 1, tg.disabled
    assert torch.isfinite(last[0])
    reset_cfg()
    return _rate(ms, B)


def train_aten_leg(zoo_spec, shape, steps, warmup):
    """The torch restatement of tests/_zoo.py's `zoo_spec` on torch's own device kernels, float32
    parameters under bf16 autocast: forward + cross-entropy + backward (no optimizer step)."""
    import torch
    from _zoo import fixture_keys
    from oracle import synth
    torch.backends.cudnn.enabled = False
    O = zoo_spec.O
    sd = {k: v.cuda() for k, v in O.state(fixture_keys(zoo_spec)[1]).items()}
    B, H, W = shape
    x = synth.synth_images(B, H, W, seed=0).cuda()
    y = synth.synth_targets(B, H, W, seed=0).cuda()
    return _rate(timed(lambda: O.train(sd, x, y, autocast=True), steps, warmup), B)


def emit_result(value):
    """(child) the one line the parent reads."""
    import torch
    print("RESULT " + json.dumps({"value": value, "device": torch.cuda.get_device_name(0)}))


def run_legs(script, legs, args, header, results="results", passed=("steps", "warmup")):
    """(parent) One child process of `script` per leg, each under LEG_TIMEOUT; the first leg that
    fails or runs past it ends the run with its exit status and nothing more is started.
    `legs`: (key in the output, the child's extra arguments); `passed`: the counts handed on.
    Prints `header` with the children's values under `results` as one JSON line."""
    res = dict(header)
    res[results] = {}
    for key, extra in legs:
        cmd = [sys.executable, os.path.abspath(script)] + list(extra)
        for name in passed:
            cmd += ["--" + name, str(getattr(args, name))]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.stderr.write("leg %s ran past %d s: stopping\n" % (key, LEG_TIMEOUT))
            return 124
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:  # nothing more is started on the GPU
            sys.stderr.write("leg %s failed (%d): stopping\n%s\n" % (key, p.returncode,
                                                                     p.stderr[-3000:]))
            return p.returncode or 1
        r = json.loads(line[0][len("RESULT "):])
        res["device"] = r["device"]
        res[results][key] = r["value"]
        sys.stderr.write("%s: %s\n" % (key, json.dumps(r["value"])))
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0
