"""GPU: the channel-attention kernels (csrc/chan_gate.hip: seg_apply_pool_fwd, seg_chan_gate_fwd /
_bwd / _bwd_finalize, seg_bcast_add), functional.channel_gate / global_avg_pool_all on top of them,
and one BasicBlockV1b stage (resnet18 / resnet34: never run on the device before BiSeNet).  The
reference is torch float64 on the CPU; bars are _util.assert_close / tol(dtype) for the kernels
and the 1e-4 relative L2 of test_hrnet_module_and_head_gradients_tight for the composites.

Shapes — the smallest at which these kernels can go wrong: N in {1, 3, 5}; H x W in {1x1, 7x9,
33x65, 48x48} (one row, fewer rows than a block, a count that is no multiple of the block's rows,
several chunks per image); C in {8, 128, 136}, the last a slice at channel 8 of a NaN-filled
256-pitch buffer (a read outside the slice poisons the result)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

from _util import assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc
from oracle import synth, torch_ref

pytestmark = pytest.mark.gpu

NS, HWS, CS = (1, 3, 5), ((1, 1), (7, 9), (33, 65), (48, 48)), (8, 128, 136)
DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32


def _K():
    from segmentron_amd import hip_ops
    return hip_ops


def _dev(x_nchw, dtype, C):
    """device NHWC; C = 136: a channel slice of a wider NaN-filled buffer"""
    if C == 136:
        return to_dev_nhwc(x_nchw, dtype, pitch=256, off=8)
    return to_dev_nhwc(x_nchw, dtype)


def _shapes():
    for N in NS:
        for H, W in HWS:
            yield N, H, W


def _nc(t):
    """[N, C] device float32 -> CPU float64 [N, C, 1, 1]"""
    return t.detach().cpu().double()[:, :, None, None]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", CS)
def test_apply_pool_all_modes(dtype, C):
    K = _K()
    scale = (rnd((C,), 1) * 0.5 + 1.0)
    shift = rnd((C,), 2) * 0.3
    for N, H, W in _shapes():
        x = quant(rnd((N, C, H, W), 3 + N + H), dtype)
        xd = _dev(x, dtype, C)
        for mode in (K.PRO_NONE, K.PRO_RELU, K.PRO_AFFINE, K.PRO_AFFINE_RELU):
            pro = (mode, scale.cuda(), shift.cuda()) if mode & K.PRO_AFFINE else (mode, None, None)
            f = x.double()
            if mode & K.PRO_AFFINE:
                f = f * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
            if mode & K.PRO_RELU:
                f = f.clamp_min(0)
            what = "apply_pool N%d %dx%d C%d mode %d" % (N, H, W, C, mode)
            y, sums = K.apply_pool(xd, pro, want_y=True)
            assert_close(to_cpu_nchw(y), f, dtype, what + " y")
            ref = f.mean((2, 3), keepdim=True)
            # (the sums are of the float32 activated values in every element type)
            assert_close(_nc(sums) / (H * W), ref, F32, what + " mean",
                         scale=max(f.abs().max().item(), 1e-12))
            y0, sums0 = K.apply_pool(xd, pro, want_y=False)
            assert y0 is None and torch.equal(sums0, sums), what  # pool-only: the same bits
            _, again = K.apply_pool(xd, pro, want_y=True)
            assert torch.equal(again, sums), what + ": not deterministic"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_apply_pool_images_do_not_leak_into_each_other(dtype):
    K = _K()
    for C in CS:
        for H, W in HWS:
            x = quant(rnd((3, C, H, W), 17), dtype)
            _, base = K.apply_pool(_dev(x, dtype, C), None, want_y=False)
            x2 = x.clone()
            x2[1] = 1e30
            _, huge = K.apply_pool(_dev(x2, dtype, C), None, want_y=False)
            assert torch.equal(huge[0], base[0]) and torch.equal(huge[2], base[2]), (C, H, W)
            assert (huge[1] > 1e29).all()


def _gate_a(N, C, seed):
    """pre-sigmoid values as the branch leaves them: behind a ReLU (exact zeros), plus 0, +-30"""
    a = rnd((N, C), seed).clamp_min(0)
    a[0, 0], a[0, 1], a[0, 2] = 0.0, 30.0, -30.0
    a[-1, 3] = torch.tensor(-0.7).clamp_min(0)  # (at C = 8 the draw above may clip nothing)
    assert (a == 0).sum() >= 2
    return a


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", CS)
def test_chan_gate_forward(dtype, C):
    K = _K()
    for N, H, W in _shapes():
        x = quant(rnd((N, C, H, W), 5 + N + W), dtype)
        r = quant(rnd((N, C, H, W), 6 + N + W), dtype)
        radd = rnd((N, C), 7 + N)
        a = _gate_a(N, C, 8 + N)
        xd, rd = _dev(x, dtype, C), _dev(r, dtype, C)
        for identity in (False, True):
            for has_r in (False, True):
                for has_b in (False, True):
                    ref = x.double() * (float(identity) + torch.sigmoid(a.double()))[:, :, None, None]
                    if has_r:
                        ref = ref + r.double()
                    if has_b:
                        ref = ref + radd.double()[:, :, None, None]
                    y = K.chan_gate(xd, a.cuda(), identity, rd if has_r else None,
                                    radd.cuda() if has_b else None)
                    assert_close(to_cpu_nchw(y), ref, dtype, "chan_gate N%d %dx%d C%d id%d r%d b%d"
                                 % (N, H, W, C, identity, has_r, has_b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", CS)
def test_chan_gate_backward_matches_autograd(dtype, C):
    K = _K()
    for N, H, W in _shapes():
        for identity in (False, True):
            x = quant(rnd((N, C, H, W), 9 + N + H), dtype)
            dy = quant(rnd((N, C, H, W), 10 + N + H), dtype)
            a = _gate_a(N, C, 11 + N)
            xo = x.double().requires_grad_()
            ao = a.double().requires_grad_()
            bo = torch.zeros(N, C, dtype=torch.float64, requires_grad=True)
            yo = xo * (float(identity) + torch.sigmoid(ao))[:, :, None, None] + bo[:, :, None, None]
            (yo * dy.double()).sum().backward()
            what = "chan_gate_bwd N%d %dx%d C%d id%d" % (N, H, W, C, identity)
            xd, dyd = _dev(x, dtype, C), _dev(dy, dtype, C)
            dx, da, db = K.chan_gate_bwd(dyd, xd, a.cuda(), identity)
            assert_close(to_cpu_nchw(dx), xo.grad, dtype, what + " dx")
            # (fp32 sums of products of exactly representable factors in both element types;
            # normalised by the sum's own scale, |dy||x| ~ sqrt(HW))
            s = max((dy.double() * x.double()).abs().sum((2, 3)).max().item() * 0.25, 1e-12)
            assert_close(da.cpu(), ao.grad, F32, what + " da", scale=s)
            assert_close(db.cpu(), bo.grad, F32, what + " dradd",
                         scale=max(dy.double().abs().sum((2, 3)).max().item(), 1e-12))
            dx2, da2, db2 = K.chan_gate_bwd(dyd, xd, a.cuda(), identity)
            assert torch.equal(da, da2) and torch.equal(db, db2) and torch.equal(dx, dx2), what
            _, da3, db3 = K.chan_gate_bwd(dyd, xd, a.cuda(), identity, want_dx=False)
            assert torch.equal(da, da3) and torch.equal(db, db3), what


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", CS)
def test_bcast_add(dtype, C):
    K = _K()
    for N, H, W in _shapes():
        g = quant(rnd((N, C, H, W), 12 + N + W), dtype)
        v = rnd((N, C), 13 + N)
        sc = 1.0 / (H * W)
        ref = g.double() + v.double()[:, :, None, None] * sc
        gd = _dev(g, dtype, C)
        fresh = K.bcast_add(gd, v.cuda(), sc, inplace=False)
        assert fresh.data_ptr() != gd.data_ptr()
        out = K.bcast_add(gd, v.cuda(), sc)
        assert torch.equal(fresh, out)
        assert out.data_ptr() == gd.data_ptr()  # in place
        assert_close(to_cpu_nchw(out), ref, dtype, "bcast_add N%d %dx%d C%d" % (N, H, W, C))
        alone = K.bcast_add(None, v.cuda(), sc, like=gd)
        assert tuple(alone.shape) == (N, H, W, C) and alone.dtype == dtype
        assert_close(to_cpu_nchw(alone), (ref - g.double()), dtype, "bcast alone")


def test_bad_arguments_are_errors():
    K = _K()
    x = torch.zeros(2, 3, 3, 8, device="cuda")
    with pytest.raises(RuntimeError):
        K.chan_gate(x, torch.zeros(2, 4, device="cuda"))
    with pytest.raises(RuntimeError):
        K.apply_pool(torch.zeros(2, 3, 3, 6, device="cuda"))  # C no multiple of the vector
    with pytest.raises(RuntimeError):
        K.apply_pool(torch.zeros(2, 3, 3, 8))  # no CPU fallback


# ------------------------------------------------------------------------------ the operator
class _Gate(nn.Module):
    def __init__(self, C, mids, with_context):
        from segmentron_amd.modules import _ConvBNReLU
        super().__init__()
        self.pre = _ConvBNReLU(C, C, 1)
        chans = [C] + list(mids) + [C]
        self.att = nn.Sequential(*[_ConvBNReLU(a, b, 1) for a, b in zip(chans[:-1], chans[1:])])
        if with_context:
            self.ctx = _ConvBNReLU(C, C, 1)


def _rel(a, b):
    return ((a.double() - b).norm() / b.norm()).item()


@pytest.mark.parametrize("case", ["arm", "ffm"])
def test_channel_gate_end_to_end_against_fp64_autograd(case):
    """functional.channel_gate behind a conv + BatchNorm + ReLU: output, input gradient, the
    producer's and the branch's weights and BatchNorm affine gradients against float64 autograd of
    the torch composition, relative L2 1e-4.  arm: [4,12,12,128], one-layer branch, x * s plus a
    plain residual and a broadcast residual (the pooled global context); ffm: [4,9,13,256],
    branch 256 -> 64 -> 256, x + x * s."""
    import segmentron_amd
    from segmentron_amd import functional as F
    segmentron_amd.set_compute_dtype(torch.float32)
    N, H, W, C, mids, arm = (4, 12, 12, 128, (), True) if case == "arm" else \
        (4, 9, 13, 256, (64,), False)
    mod = _Gate(C, mids, arm)
    # (conditioned: BatchNorm beta = +2 gamma, few ReLUs sit at ties)
    names = {"m." + k: v for k, v in mod.state_dict().items()}
    sd = synth.synth_like(names, seed=4, conditioned=True)
    mod.load_state_dict({k[2:]: v for k, v in sd.items()})
    mod = mod.cuda().train()
    x = rnd((N, C, H, W), 21)
    res = rnd((N, C, H, W), 22)
    gw = rnd((N, C, H, W), 23)
    # float64 oracle
    osd = torch_ref.clone_state({k: (v.double() if v.is_floating_point() else v)
                                 for k, v in sd.items()}, requires_grad=True)
    net = torch_ref.OracleNet(osd, training=True)
    xo, ro = x.double().requires_grad_(), res.double().requires_grad_()
    fo = net.conv_bn_relu(xo, "m.pre")
    ao = TF.adaptive_avg_pool2d(fo, 1)
    for i in range(len(mids) + 1):
        ao = net.conv_bn_relu(ao, "m.att.%d" % i)
    so = torch.sigmoid(ao)
    if arm:
        yo = fo * so + ro + net.conv_bn_relu(TF.adaptive_avg_pool2d(xo, 1), "m.ctx")
    else:
        yo = fo + fo * so
    (yo * gw.double()).sum().backward()
    # HIP
    xh = to_dev_nhwc(x, F32).requires_grad_()
    rh = to_dev_nhwc(res, F32).requires_grad_()

    def branch(p):
        assert p.t.dtype == torch.float32 and tuple(p.t.shape) == (N, 1, 1, C)
        for m in mod.att:
            p = m(p)
        return p
    if arm:
        ctx = mod.ctx(F.Act(F.global_avg_pool_all(F.Act(xh))))
        yh = F.channel_gate(mod.pre(F.Act(xh)), branch, identity=False, residual=rh,
                            bcast_residual=ctx)
    else:
        yh = F.channel_gate(mod.pre(F.Act(xh)), branch, identity=True)
    assert _rel(to_cpu_nchw(yh), yo.detach()) < 1e-5
    (yh * to_dev_nhwc(gw, F32)).sum().backward()
    errs = {"x": _rel(to_cpu_nchw(xh.grad), xo.grad)}
    if arm:
        errs["residual"] = _rel(to_cpu_nchw(rh.grad), ro.grad)
    for k, p in mod.named_parameters():
        errs[k] = _rel(p.grad.cpu(), osd["m." + k].grad)
    print(case, {k: "%.2e" % v for k, v in errs.items()})
    assert len(errs) >= 7 and max(errs.values()) < 1e-4, errs
    # the BatchNorms behind the pool saw N samples: counters and running statistics moved
    assert int(mod.att[0].bn.num_batches_tracked) == 1
    ref = osd["m.att.0.bn.running_var"]
    assert (mod.att[0].bn.running_var.cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_channel_gate_on_a_plain_input():
    """Nothing pending on the input: no copy is written, the gate reads the tensor itself, and
    its gradient is the gate's plus the pool's."""
    import segmentron_amd
    from segmentron_amd import functional as F
    segmentron_amd.set_compute_dtype(torch.float32)
    N, H, W, C = 3, 7, 9, 136
    mod = _Gate(C, (), False)
    sd = synth.synth_like({"m." + k: v for k, v in mod.state_dict().items()}, seed=8,
                          conditioned=True)
    mod.load_state_dict({k[2:]: v for k, v in sd.items()})
    mod = mod.cuda().train()
    x, gw = rnd((N, C, H, W), 51), rnd((N, C, H, W), 52)
    osd = torch_ref.clone_state({k: (v.double() if v.is_floating_point() else v)
                                 for k, v in sd.items()}, requires_grad=True)
    net = torch_ref.OracleNet(osd, training=True)
    xo = x.double().requires_grad_()
    so = torch.sigmoid(net.conv_bn_relu(TF.adaptive_avg_pool2d(xo, 1), "m.att.0"))
    yo = xo + xo * so
    (yo * gw.double()).sum().backward()
    xh = to_dev_nhwc(x, F32, pitch=256, off=8).requires_grad_()
    yh = F.channel_gate(F.Act(xh), mod.att[0], identity=True)
    assert _rel(to_cpu_nchw(yh), yo.detach()) < 1e-5
    (yh * to_dev_nhwc(gw, F32)).sum().backward()
    assert _rel(to_cpu_nchw(xh.grad), xo.grad) < 1e-4
    assert _rel(mod.att[0].conv.weight.grad.cpu(), osd["m.att.0.conv.weight"].grad) < 1e-4


def test_channel_gate_bf16_pools_in_float32():
    import segmentron_amd
    from segmentron_amd import functional as F
    segmentron_amd.set_compute_dtype(torch.bfloat16)
    try:
        x = quant(rnd((3, 128, 7, 9), 31), torch.bfloat16)
        xh = to_dev_nhwc(x, torch.bfloat16)
        p = F.global_avg_pool_all(F.Act(xh, None, True))
        assert p.dtype == torch.float32 and tuple(p.shape) == (3, 1, 1, 128)
        ref = x.double().clamp_min(0).mean((2, 3), keepdim=True)
        assert_close(p.cpu().permute(0, 3, 1, 2), ref, F32, "bf16 pool in float32")
        assert F.global_avg_pool_all(F.Act(xh), keep_fp32=False).dtype == torch.bfloat16
    finally:
        segmentron_amd.set_compute_dtype(torch.float32)


def test_basic_block_stage_against_fp64():
    """BasicBlockV1b as ResNetV1._make_layer(128, 2 blocks, stride 2, dilation 2) builds it:
    64 -> 128 stride 2 with a downsample, conv2 dilated by previous_dilation = 2, then a dilated
    block — against torch_ref._res_layer in float64, relative L2 1e-4."""
    import segmentron_amd
    from segmentron_amd import functional as F
    from segmentron_amd.models.backbones.resnet import BasicBlockV1b
    segmentron_amd.set_compute_dtype(torch.float32)
    ds = nn.Sequential(nn.Conv2d(64, 128, 1, 2, bias=False), nn.BatchNorm2d(128))
    layer = nn.Sequential(BasicBlockV1b(64, 128, 2, dilation=1, downsample=ds, previous_dilation=2),
                          BasicBlockV1b(128, 128, dilation=2, previous_dilation=2))
    sd = synth.synth_like({"m.layer1." + k: v for k, v in layer.state_dict().items()}, seed=6,
                          conditioned=True)
    layer.load_state_dict({k[len("m.layer1."):]: v for k, v in sd.items()})
    layer = layer.cuda().train()
    N, H, W = 2, 17, 23
    x, gw = rnd((N, 64, H, W), 41), rnd((N, 128, 9, 12), 42)
    osd = torch_ref.clone_state({k: (v.double() if v.is_floating_point() else v)
                                 for k, v in sd.items()}, requires_grad=True)
    net = torch_ref.OracleNet(osd, training=True)
    xo = x.double().requires_grad_()
    yo = torch_ref._res_layer(net, xo, "m.layer1", 2, 2)
    assert tuple(yo.shape) == tuple(gw.shape)
    (yo * gw.double()).sum().backward()
    xh = to_dev_nhwc(x, F32).requires_grad_()
    a = F.Act(xh)
    for blk in layer:
        a = blk(a)
    yh = F.materialize(a)
    assert _rel(to_cpu_nchw(yh), yo.detach()) < 1e-5
    (yh * to_dev_nhwc(gw, F32)).sum().backward()
    errs = {"x": _rel(to_cpu_nchw(xh.grad), xo.grad)}
    for k, p in layer.named_parameters():
        errs[k] = _rel(p.grad.cpu(), osd["m.layer1." + k].grad)
    print({k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) < 1e-4, errs
