"""The gradient hand-off of forked activations (functional.GradFork) and the kernels behind it,
against float64 torch autograd on the CPU:

  * the sliding depthwise backward with a second gradient added like the 2-ary sum it replaces
    (seg_dwconv3x3_bwd_fused_sum): the fused backward followed by sum_n, bit for bit;
  * bn_bwd_apply with a second gradient (seg_bn_bwd_apply_add) on every launch geometry of
    `ew_geom`: bit for bit the separate apply passes followed by sum_n;
  * XceptionBlock with a conv skip (input with a pending BatchNorm + ReLU, and plain) and with a
    low-level feature that feeds a BN-folding 1x1 conv: the SAME gradients, bit for bit, as the
    `fork` / sum_n path, within the bar of the float64 reference, no sum_n launch left;
  * nothing parked is lost or left over when a consumer does not take part in backward;
  * a captured DeepLabv3+/xception65 train loop equals the eager one bit for bit.

The hand-off removes passes, not roundings, so the bar against the `fork` path is equality; the
float64 bar is tests/_util.assert_close (2e-5 of the max in fp32) times the composite's factor."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def F():
    from segmentron_amd import functional
    return functional


# ----------------------------------------------- depthwise: residual with the 2-ary sum's arithmetic
# maps of >= 30 MiB take the lane-exchange kernels (tests/test_dwconv_slide_gpu.py ABOVE); below:
# width no multiple of 16, channels no multiple of 64, several strips (45 rows) / one strip
ABOVE = {torch.float32: (2, 100, 601, 72), torch.bfloat16: (2, 151, 771, 72)}
SUM_SHAPES = [(2, 45, 19, 72), (1, 9, 5, 8), "above"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [1, 3], ids=["relu", "affine_relu"])
@pytest.mark.parametrize("shape", SUM_SHAPES, ids=lambda s: s if s == "above" else "x".join(map(str, s)))
def test_dw_bwd_sum_is_the_fused_backward_plus_sum_n_bit_for_bit(shape, mode, dtype):
    """seg_dwconv3x3_bwd_fused_sum: the stored gradient is sum_n([g of the launch without res, res])
    bit for bit; weight-gradient and BatchNorm-backward partials do not involve res.  Operands are
    channel slices of wider buffers (NaN around them)."""
    N, H, W, C = ABOVE[dtype] if shape == "above" else shape
    if shape == "above":
        assert N * H * W * C * (2 if dtype == torch.bfloat16 else 4) >= (30 << 20)
    k = K()
    cshape = (N, C, H, W)
    x = to_dev_nhwc(quant(rnd(cshape, 1), dtype), dtype, pitch=C + 16, off=8)
    dy = to_dev_nhwc(quant(rnd(cshape, 2), dtype), dtype, pitch=C + 16, off=8)
    res = to_dev_nhwc(quant(rnd(cshape, 3), dtype), dtype, pitch=C + 8, off=0)
    w = (rnd((C, 1, 3, 3), 4) * 0.4).to(DEV)
    pro = (mode, None, None)
    if mode & 2:
        gen = torch.Generator().manual_seed(5)
        pro = (mode, (torch.rand(C, generator=gen) + 0.5).to(DEV), rnd((C,), 6, 0.3).to(DEV))
    kw = dict(want_bn=True, torch_layout=True, raw_dw=True)
    g0, pw0, pb0 = k.dwconv_bwd_fused(x, dy, w, 1, pro, **kw)
    g, pw, pb = k.dwconv_bwd_fused(x, dy, w, 1, pro, res=res, res_sum=True, **kw)
    assert torch.equal(g, k.sum_n([g0, res]))
    assert torch.equal(pw, pw0) and torch.equal(pb, pb0)
    assert 0.3 < (g0 == 0).float().mean().item() < 0.7  # (the ReLU mask is in it)
    if dtype == torch.float32:  # no storage rounding: the one-rounding entry gives the same values
        ga, _, _ = k.dwconv_bwd_fused(x, dy, w, 1, pro, res=res, **kw)
        assert torch.equal(g, ga)


def test_the_sum_entry_needs_the_sliding_family():
    k = K()
    assert k.dwconv_bwd_fused_sum_ok(torch.float32, 64, 1)
    assert k.dwconv_bwd_fused_sum_ok(torch.bfloat16, 72, 1)
    assert not k.dwconv_bwd_fused_sum_ok(torch.bfloat16, 12, 1)  # C % 8
    assert not k.dwconv_bwd_fused_sum_ok(torch.float32, 6, 1)    # tiled family
    assert not k.dwconv_bwd_fused_sum_ok(torch.float32, 64, 2)


# ----------------------------------------------------------------------- bn_bwd_apply + addend
# channel vectors per row (fp32 / bf16): 72 -> 18 / 9 column blocks; 728 -> 182 / 91 whole rows;
# 2056 -> 514 wide rows (column blocks again) / 257 whole rows; 4104 -> 1026 / 513 wide rows
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [2, 3], ids=["affine", "affine_relu"])
@pytest.mark.parametrize("C", [72, 728, 2056, 4104])
def test_bn_bwd_apply_with_addend_equals_apply_then_add(C, mode, dtype):
    k = K()
    N, H, W = 1, 7, 43  # 301 rows: a ragged last batch of rows in every geometry
    vec = k.vec_of(dtype)
    cv = C // vec
    lpr = k.LIB.query("seg_ew_geom_query", k._DT[dtype], C, N * H * W, 0)
    assert (lpr == cv) == (32 < cv <= 512)  # whole rows exactly there
    shape = (N, C, H, W)
    g = to_dev_nhwc(quant(rnd(shape, 1), dtype), dtype, pitch=C + 2 * vec, off=vec)
    x = to_dev_nhwc(quant(rnd(shape, 2), dtype), dtype, pitch=C + vec, off=0)
    add = to_dev_nhwc(quant(rnd(shape, 3), dtype), dtype, pitch=C + 3 * vec, off=2 * vec)
    gen = torch.Generator().manual_seed(4)
    sc = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    sh = rnd((C,), 5, 0.3).to(DEV)
    c0, c1 = rnd((C,), 6, 0.2).to(DEV), rnd((C,), 7, 0.2).to(DEV)
    for coef in ((c0, c1), (None, None)):  # training / evaluation-mode BatchNorm backward
        plain = k.bn_bwd_apply(g, x, (mode, sc, sh), *coef)
        full = torch.full((N, H, W, C + 2 * vec), float("nan"), dtype=dtype, device=DEV)
        out = k.bn_bwd_apply(g, x, (mode, sc, sh), *coef, out=full[..., vec:vec + C], add=add)
        assert out.data_ptr() == full[..., vec:].data_ptr()
        assert torch.isnan(full[..., :vec].float()).all() and torch.isnan(full[..., vec + C:].float()).all()
        assert torch.equal(out, k.sum_n([plain, add]))  # the two passes it replaces
        # `add` as a gradient w.r.t. another consumer's ACTIVATED input: that consumer's own
        # BatchNorm backward (its mask, its coefficients) applied on the way
        for amode, acoef in ((3, (c1, c0)), (3, (None, None)), (2, (c1, c0))):
            theirs = k.bn_bwd_apply(add, x, (amode, sc, sh), *acoef)
            out = k.bn_bwd_apply(g, x, (mode, sc, sh), *coef, add=add, add_pro=(amode,) + acoef)
            assert torch.equal(out, k.sum_n([plain, theirs])), (amode, acoef[0] is None)
    # in place on g (how _DwFn.backward calls it)
    gc = g.clone()
    out = k.bn_bwd_apply(gc, x, (mode, sc, sh), c0, c1, out=gc, add=add)
    ref = k.bn_bwd_apply(g, x, (mode, sc, sh), c0, c1, add=add)
    assert torch.equal(out, ref)


# -------------------------------------------------------------------------- XceptionBlock forks
CIN, CMID, CLOW = 16, 24, 8


class _Net(nn.Module):
    """[1x1 conv -> BN -> ReLU pending] -> XceptionBlock(conv skip) [-> low-level feature -> a
    BN-folding 1x1 conv -> BN -> ReLU]: the first entry-flow block / the block whose low-level
    feature feeds the decoder, at 16 -> 24 channels."""

    def __init__(self, stride, pending, low_feat):
        super().__init__()
        from segmentron_amd.models.backbones.xception import XceptionBlock
        self.pending, self.low_feat, self.stride = pending, low_feat, stride
        self.conv0 = nn.Conv2d(CIN, CIN, 1, bias=False)
        self.bn0 = nn.BatchNorm2d(CIN)
        self.block = XceptionBlock([CIN, CMID, CMID, CMID], stride=stride, low_feat=low_feat)
        self.low_conv = nn.Conv2d(CMID, CLOW, 1, bias=False)
        self.low_bn = nn.BatchNorm2d(CLOW)

    def forward(self, x, use_low=True, use_out=True):
        f = F()
        a = f.Act(x)
        if self.pending:
            a = f.conv_bn(a, self.conv0, self.bn0)
            a.relu = True
        out = self.block(a)
        low = None
        if self.low_feat:
            out, low = out
            low = f.conv_bn(low, self.low_conv, self.low_bn)
            low.relu = True
            low = f.materialize(low)
        return (out.t if use_out else None), (low if use_low else None)

    def oracle(self, sd, x, use_low=True, use_out=True):
        from oracle import torch_ref
        o = torch_ref.OracleNet(sd, training=True)
        h = x
        if self.pending:
            h = torch.relu(o.bn(o.conv(h, "conv0"), "bn0"))
        out = o.xception_block(h, "block", self.stride, 1, "conv", True, self.low_feat)
        low = None
        if self.low_feat:
            out, low = out
            low = torch.relu(o.bn(o.conv(low, "low_conv"), "low_bn"))
        return (out if use_out else None), (low if use_low else None)


def _init(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * (0.4 if p.shape[1] == 1 else 0.25))
            elif name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)


def _loss(outs, ws):
    return sum((o.double() * w).sum() for o, w in zip(outs, ws) if o is not None)


def _run_hip(net, x, ws, monkeypatch, forked, x_grad=True, **use):
    """One forward + backward of `net` on the device -> ({name: grad}, dx, sum_n launches, the
    GradForks armed).  forked: today's path — every fork's gradients meet in `fork`'s sum."""
    f, k = F(), K()
    forks, calls = [], [0]
    real_skip, real_low, real_sum = f.conv_skip_fork, f.low_feat_fork, k.sum_n

    def note(fn):
        def wrapped(*a):
            fk = None if forked else fn(*a)
            if fk is not None:
                forks.append(fk)
            return fk
        return wrapped

    def sum_n(ts):
        calls[0] += 1
        return real_sum(ts)
    monkeypatch.setattr(f, "conv_skip_fork", note(real_skip))
    monkeypatch.setattr(f, "low_feat_fork", note(real_low))
    monkeypatch.setattr(k, "sum_n", sum_n)
    net.zero_grad()
    xd = to_dev_nhwc(x, torch.float32).requires_grad_(x_grad)
    outs = net(xd, **use)
    # (the weights in the outputs' own dense NHWC layout: the gradient the model would get)
    _loss(outs, [None if w is None else w.permute(0, 2, 3, 1).contiguous() for w in ws]).backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    grads = {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()
             if p.grad is not None}
    dx = None if xd.grad is None else to_cpu_nchw(xd.grad)
    return grads, dx, calls[0], forks


def _run_oracle(net, x, ws, x_grad=True, **use):
    from oracle import torch_ref
    sd = torch_ref.clone_state({k_: v.detach().cpu().double() if v.is_floating_point()
                                else v.detach().cpu().clone()
                                for k_, v in net.state_dict().items()}, requires_grad=True)
    xr = x.double().requires_grad_(x_grad)
    outs = net.oracle(sd, xr, **use)
    _loss(outs, [None if w is None else w.cpu() for w in ws]).backward()
    return {k_: v.grad for k_, v in sd.items() if v.grad is not None}, xr.grad


def _weights(net, x, seed):
    """fixed random weights of the linear loss, one per output (shape from a dry oracle run)"""
    with torch.no_grad():
        from oracle import torch_ref
        sd = torch_ref.clone_state({k_: v.detach().cpu().double() if v.is_floating_point()
                                    else v.detach().cpu().clone()
                                    for k_, v in net.state_dict().items()})
        outs = net.oracle(sd, x.double())
    return [None if o is None else rnd(tuple(o.shape), seed + i).double().to(DEV)
            for i, o in enumerate(outs)]


# A block is a chain of a dozen kernels with fp32 BatchNorm statistics in between: the fp32 bar of
# the same composite in tests/test_composites_gpu.py (5e-4 of the max) = 25 x assert_close's 2e-5
BLOCK_FAC = 25


def _compare(got, dx, ref, dxr, what):
    assert set(got) == set(ref), (what, set(ref) ^ set(got))
    # bn_depth.bias has NO gradient analytically: the 1x1 conv + training-mode BatchNorm behind it
    # cancel a per-channel constant (float64 reference ~1e-16) — it is measured against the
    # largest BatchNorm-parameter gradient of the block instead of against itself
    bn_scale = max(v.abs().max().item() for v in ref.values() if v.dim() == 1)
    for name in sorted(ref):
        scale = bn_scale if name.endswith("bn_depth.bias") else None
        err = assert_close(got[name], ref[name].float(), torch.float32, "%s %s" % (what, name),
                           scale=scale, fac=BLOCK_FAC)
        print("%-18s %-40s %.2e" % (what, name, err))
    if dxr is not None:
        print("%-18s %-40s %.2e" % (what, "dx", assert_close(dx, dxr.float(), torch.float32,
                                                             what + " dx", fac=BLOCK_FAC)))


BLOCK_CASES = [
    # stride, input with pending BN + ReLU, low-level feature
    (2, True, False),
    (1, True, False),
    (2, False, False),
    (1, False, False),
    (2, False, True),
    (1, True, True),
]


@pytest.mark.parametrize("case", BLOCK_CASES,
                         ids=lambda c: "s%d_%s%s" % (c[0], "pending" if c[1] else "plain",
                                                     "_low" if c[2] else ""))
def test_conv_skip_block_hands_its_gradients_over(case, monkeypatch):
    """17 x 21 maps, 16 -> 24 channels, fp32; 4 images: 1428 samples per channel, above the
    few-sample BatchNorm backward (1024) that keeps the `fork` path."""
    import segmentron_amd
    stride, pending, low_feat = case
    segmentron_amd.set_compute_dtype(torch.float32)
    net = _Net(stride, pending, low_feat)
    _init(net, 7)
    net = net.to(DEV).train()
    x = rnd((4, CIN, 17, 21), 11) * 1.2 + 0.1
    ws = _weights(net, x, 20)
    ref, dxr = _run_oracle(net, x, ws)
    new, dxn, n_new, forks = _run_hip(net, x, ws, monkeypatch, forked=False)
    old, dxo, n_old, _ = _run_hip(net, x, ws, monkeypatch, forked=True)
    kinds = sorted(fk.kind for fk in forks)
    G = F().GradFork
    assert kinds == sorted([G.PRE if pending else G.SUM] + ([G.RAW] if low_feat else []))
    assert n_new == 0 and n_old == 1 + int(low_feat)  # every 2-ary sum is gone
    assert all(fk.g is None and fk.closed for fk in forks)  # parked, taken, nothing left
    _compare(new, dxn, ref, dxr, "hand-off")
    _compare(old, dxo, ref, dxr, "fork")
    # the hand-off removes passes, not roundings: the very same numbers
    assert torch.equal(dxn, dxo)
    assert not [n for n in old if not torch.equal(new[n], old[n])]


def test_few_sample_batchnorm_keeps_the_fork_path(monkeypatch):
    """2 images of 17 x 21: 714 samples per channel — the pending BatchNorm's backward is the
    one-launch float64 kernel, which takes no parked gradient."""
    import segmentron_amd
    segmentron_amd.set_compute_dtype(torch.float32)
    net = _Net(2, True, True)
    _init(net, 8)
    net = net.to(DEV).train()
    x = rnd((2, CIN, 17, 21), 12) * 1.2 + 0.1
    ws = _weights(net, x, 30)
    ref, dxr = _run_oracle(net, x, ws)
    new, dxn, n_new, forks = _run_hip(net, x, ws, monkeypatch, forked=False)
    assert not forks and n_new == 2
    _compare(new, dxn, ref, dxr, "few-sample")


@pytest.mark.parametrize("which", ["input_needs_no_grad", "low_unused", "low_conv_frozen"])
def test_no_gradient_is_lost_or_left_parked_without_a_second_consumer(which, monkeypatch):
    import segmentron_amd
    segmentron_amd.set_compute_dtype(torch.float32)
    net = _Net(2, False, True)
    _init(net, 9)
    net = net.to(DEV).train()
    x = rnd((4, CIN, 17, 21), 13) * 1.2 + 0.1
    ws = _weights(net, x, 40)
    use, x_grad = {}, True
    if which == "input_needs_no_grad":
        # the taking depthwise conv needs no input gradient: conv_skip_fork arms nothing then (a
        # fork is armed only where the forked tensor requires grad, so an armed fork's taker
        # always computes dx) — asserted below; the low-level feature's fork is still armed
        x_grad = False
    elif which == "low_unused":  # the parking consumer of the low-level feature never runs
        use = dict(use_low=False)
    else:  # the parking conv only needs its input gradient
        net.low_conv.weight.requires_grad_(False)
    ref, dxr = _run_oracle(net, x, ws, x_grad=x_grad, **use)
    if which == "low_conv_frozen":
        ref.pop("low_conv.weight", None)
    new, dxn, _, forks = _run_hip(net, x, ws, monkeypatch, forked=False, x_grad=x_grad, **use)
    old, dxo, _, _ = _run_hip(net, x, ws, monkeypatch, forked=True, x_grad=x_grad, **use)
    assert all(fk.g is None for fk in forks)
    G = F().GradFork
    assert sorted(fk.kind for fk in forks) == ([G.RAW] if not x_grad else [G.RAW, G.SUM])
    assert (dxn is None) == (not x_grad)
    _compare(new, dxn, ref, dxr, which)
    assert (dxn is None and dxo is None) or torch.equal(dxn, dxo)
    assert not [n for n in old if not torch.equal(new[n], old[n])]


# --------------------------------------------------------------------------------- graph replay
def test_captured_deeplab_xception_step_equals_eager_bit_for_bit():
    """DeepLabv3+/xception65 at 65 x 129, bf16, the reference's loop statements: 2 eager calls,
    the capturing one, 2 replays — GradForks are host objects of one forward; the captured
    backward replays the hand-off's launches."""
    from test_train_loop_gpu import _run_loop
    le, se, _ = _run_loop(False, 5, (65, 129))
    lg, sg, _ = _run_loop(True, 5, (65, 129))
    assert le == lg
    bad = [k_ for k_ in se if not torch.equal(se[k_], sg[k_])]
    assert not bad, bad[:5]


def test_deeplab_xception_backward_keeps_only_the_aspp_sum(monkeypatch):
    """One eager train step of the whole model: the 2-ary sums of the four conv-skip blocks and
    of the low-level feature are gone, the ASPP's 5-ary sum stays."""
    import segmentron_amd
    from conftest import C3_OVERRIDES
    from oracle import synth
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    try:
        cfg.update_from_list(C3_OVERRIDES)
        cfg.PHASE = "train"
        cfg.check_and_freeze()
        segmentron_amd.set_compute_dtype(torch.bfloat16)
        model = segmentron_amd.get_segmentation_model()
        model.load_state_dict(synth.synth_like(model.state_dict(), seed=0, conditioned=True))
        model = model.to(DEV).train()
        for m in model.modules():  # (the two steps below must see the same masks)
            if isinstance(m, (nn.Dropout, nn.Dropout2d)):
                m.p = 0.0
        k = K()
        seen, real = [], k.sum_n

        def sum_n(ts):
            seen.append(len(ts))
            return real(ts)
        monkeypatch.setattr(k, "sum_n", sum_n)
        # 129 x 257: 2 x 65 x 129 samples per channel at the first block, 2 x 33 x 65 at the
        # low-level feature — every pending BatchNorm above the few-sample path
        x = synth.synth_images(2, 129, 257, seed=3).to(DEV)
        y = synth.synth_targets(2, 129, 257, seed=3).to(DEV)

        def step():
            model.zero_grad()
            out = model(x)
            loss = TF.cross_entropy(out[0], y, ignore_index=-1)
            loss.backward()
            torch.cuda.synchronize()
            return loss.item(), {n: p.grad.clone() for n, p in model.named_parameters()}
        loss_new, g_new = step()
        assert seen == [5], seen
        # ... and every gradient of the bf16 step is bit for bit what the `fork` path computes
        f = F()
        monkeypatch.setattr(f, "conv_skip_fork", lambda *a: None)
        monkeypatch.setattr(f, "low_feat_fork", lambda *a: None)
        del seen[:]
        loss_old, g_old = step()
        assert sorted(seen) == [2, 2, 2, 2, 2, 5], seen
        assert loss_new == loss_old
        assert not [n for n in g_old if not torch.equal(g_new[n], g_old[n])]
    finally:
        reset_cfg()
