"""GPU: the PointRend point-head kernels (csrc/pointrend.hip) against torch on the CPU, and one
fp32 train step / evaluation of PointRend against a CPU restatement (OracleNet's xception65, ASPP
and separable convs composed into the decoder-less head, plus the point head of
segmentron/models/pointrend.py restated with F.grid_sample, conv1d and a stable sort)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import _pointrend_oracle as O
from conftest import GOLDEN
from oracle import synth

pytestmark = pytest.mark.gpu


def _K():
    from segmentron_amd import hip_ops
    return hip_ops


_grid = O.grid


def _edge_points(N, P, H, W, gen):
    p = torch.rand(N, P, 2, generator=gen)
    p[:, 0] = 0.0
    p[:, 1] = 1.0 - 2.0 ** -24
    p[:, 2, 0], p[:, 2, 1] = 0.0, 1.0 - 2.0 ** -24
    for j in range(3, 9):  # exact pixel centres
        p[:, j, 0] = (j + 0.5) / W
        p[:, j, 1] = (j % H + 0.5) / H
    return p


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 256, 7])
def test_point_sample_matches_grid_sample(C, dtype):
    K = _K()
    gen = torch.Generator().manual_seed(C)
    N, H, W, P = 2, 13, 17, 300
    ld = C + 2 * K.vec_of(dtype)
    buf = torch.randn(N, H, W, ld, generator=gen).to(dtype).cuda()
    x = buf[..., :C]
    p = _edge_points(N, P, H, W, gen)
    rows = torch.full((N * P, C + 8), 7.0, device="cuda")
    K.point_sample(K.map_nhwc(x), p.cuda(), rows, 5)
    ref = _grid(x.cpu().double().permute(0, 3, 1, 2), p.double())
    got = rows[:, 5:5 + C].view(N, P, C).permute(0, 2, 1).cpu().double()
    assert (got - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()
    assert (rows[:, :5] == 7.0).all() and (rows[:, 5 + C:] == 7.0).all()
    # the same map as NCHW float32, written in the compute dtype
    rows2 = torch.zeros((N * P, C), dtype=dtype, device="cuda")
    K.point_sample(K.map_nchw(x.float().permute(0, 3, 1, 2).contiguous()), p.cuda(), rows2)
    got2 = rows2.float().view(N, P, C).permute(0, 2, 1).cpu().double()
    tol = 1e-2 if dtype == torch.bfloat16 else 2e-6
    assert (got2 - ref).abs().max().item() <= tol * ref.abs().max().item()


def test_point_sample_nearest_labels_half_way_and_outside():
    from segmentron_amd.models.pointrend import point_sample
    gen = torch.Generator().manual_seed(3)
    N, H, W = 2, 16, 32
    gt = torch.randint(-1, 19, (N, H, W), generator=gen)
    # half-way coordinates (ix = k - 0.5: nearbyint rounds to even), random, and outside [0, 1)
    px = torch.cat([torch.arange(0, W + 1) / W, torch.rand(40, generator=gen),
                    torch.tensor([-0.2, 1.3])])
    py = torch.cat([torch.arange(0, W + 1) % (H + 1) / H, torch.rand(40, generator=gen),
                    torch.tensor([0.5, 0.5])])
    p = torch.stack([px, py], -1).unsqueeze(0).repeat(N, 1, 1).contiguous()
    got = point_sample(gt.cuda().float().unsqueeze(1), p.cuda(), mode="nearest",
                       align_corners=False).squeeze_(1).long().cpu()
    ref = _grid(gt.float().unsqueeze(1), p, mode="nearest").squeeze(1).long()
    assert torch.equal(got, ref)
    assert (got[:, -2:] == 0).all()  # zeros padding: label 0, not ignore


@pytest.mark.parametrize("C,dtype", [(19, torch.float32), (256, torch.float32),
                                     (256, torch.bfloat16)])
def test_point_sample_backward_matches_and_is_deterministic(C, dtype):
    K = _K()
    gen = torch.Generator().manual_seed(7 + C)
    N, H, W, P = 2, 9, 11, 2000
    p = torch.rand(N, P, 2, generator=gen)
    p[:, : P // 2] = 0.4 + 0.05 * p[:, : P // 2]  # clustered: many points share tap cells
    p[:, -9:] = _edge_points(N, 9, H, W, gen)
    col, ld = 3, C + 3 + K.vec_of(dtype)
    g = torch.randn(N * P, ld, generator=gen).to(dtype)
    dx = K.point_sample_bwd(g.cuda(), col, C, p.cuda(), (H, W), dtype, C + 5)
    dx2 = K.point_sample_bwd(g.cuda(), col, C, p.cuda(), (H, W), dtype, C + 5)
    assert torch.equal(dx, dx2), "backward is not bitwise reproducible"
    x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    _grid(x, p.double()).backward(g[:, col:col + C].double().view(N, P, C).permute(0, 2, 1))
    ref = x.grad.permute(0, 2, 3, 1)
    tol = 1e-2 if dtype == torch.bfloat16 else 2e-6
    assert (dx.cpu().double() - ref).abs().max().item() <= tol * ref.abs().max().item()


def test_uncertainty_grid_and_at_points():
    K = _K()
    gen = torch.Generator().manual_seed(11)
    N, H, W, C, P = 2, 10, 14, 19, 500
    x = torch.randn(N, H, W, 24, generator=gen)[..., :C]
    x[:, 2, :, 1] = x[:, 2, :, 0] = 5.0  # exact top-2 ties
    xc = x.contiguous().cuda()
    buf = torch.zeros(N, H, W, 24, device="cuda")
    buf[..., :C] = xc
    m = K.map_nhwc(buf[..., :C])
    srt = x.permute(0, 3, 1, 2).double().sort(1, descending=True)[0]
    ref = -(srt[:, 0] - srt[:, 1]).reshape(N, -1)
    assert (K.point_uncertainty(m).cpu().double() - ref).abs().max().item() <= 1e-6
    p = _edge_points(N, P, H, W, gen)
    og = _grid(srt[:, :2], p.double())
    ref_p = -(og[:, 0] - og[:, 1])
    got = K.point_uncertainty(m, p.cuda()).cpu().double()
    assert (got - ref_p).abs().max().item() <= 2e-6 * srt.abs().max().item()


def _ref_topk(keys, k):
    order = torch.sort(-keys, dim=1, stable=True)[1]
    return order[:, :k].sort(1)[0]


def test_topk_large_and_with_ties():
    K = _K()
    gen = torch.Generator().manual_seed(5)
    keys = torch.randn(1, 1025 * 2049, generator=gen)
    idx = K.point_topk(keys.cuda(), 8096).cpu()
    assert torch.equal(idx, _ref_topk(keys, 8096))
    ties = torch.randint(0, 5, (2, 49152), generator=gen).float()
    ties[1, ::3] = -0.0  # -0 and +0 are equal keys
    idx = K.point_topk(ties.cuda(), 12288).cpu()
    assert torch.equal(idx, _ref_topk(ties, 12288))
    small = torch.randn(2, 37, generator=gen)
    assert torch.equal(K.point_topk(small.cuda(), 37).cpu(), _ref_topk(small, 37))


def test_coords_and_scatter():
    K = _K()
    gen = torch.Generator().manual_seed(9)
    N, H, W, C, L = 2, 65, 129, 19, 300
    idx = torch.stack([torch.randperm(H * W, generator=gen)[:500].sort()[0] for _ in range(N)])
    pts = K.point_coords_grid(idx.cuda(), (H, W)).cpu()
    W_step, H_step = 1 / W, 1 / H
    ref = torch.zeros(N, 500, 2)
    ref[:, :, 0] = W_step / 2.0 + (idx % W).to(torch.float) * W_step
    ref[:, :, 1] = H_step / 2.0 + (idx // W).to(torch.float) * H_step
    assert torch.equal(pts, ref)
    over = torch.rand(N, L, 2, generator=gen)
    sel = torch.stack([torch.randperm(L, generator=gen)[:75].sort()[0] for _ in range(N)])
    cover = torch.rand(N, 25, 2, generator=gen)
    got = K.point_coords_train(over.cuda(), sel.cuda(), cover.cuda()).cpu()
    shift = L * torch.arange(N)
    imp = over.view(-1, 2)[(sel + shift[:, None]).view(-1), :].view(N, 75, 2)
    assert torch.equal(got, torch.cat([imp, cover], 1))
    out = torch.randn(N, C, H, W, generator=gen)
    rend = torch.randn(N * 500, 24, generator=gen)
    o = out.clone().cuda()
    K.point_scatter(rend.cuda()[:, :C], idx.cuda(), K.map_nchw(o))
    ref = out.reshape(N, C, -1).scatter_(2, idx.unsqueeze(1).expand(-1, C, -1),
                                        rend[:, :C].view(N, 500, C).permute(0, 2, 1))
    assert torch.equal(o.cpu(), ref.view(N, C, H, W))


def test_resize_matches_interpolate():
    K = _K()
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, 7, 9, 20, generator=gen)[..., :19]
    xg = torch.zeros(2, 7, 9, 20, device="cuda")
    xg[..., :19] = x.cuda()
    m = K.map_nhwc(xg[..., :19])
    ref = TF.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2, mode="bilinear",
                         align_corners=False)
    assert (K.point_resize(m, (14, 18)).cpu().double() - ref).abs().max().item() <= 1e-5
    ref = TF.interpolate(x.permute(0, 3, 1, 2).double(), (97, 129), mode="bilinear",
                         align_corners=False)
    assert (K.point_resize(m, (97, 129)).cpu().double() - ref).abs().max().item() <= 1e-5


def test_point_cross_entropy_forward_backward_and_all_ignored():
    K = _K()
    gen = torch.Generator().manual_seed(4)
    R, C = 2 * 2304, 19
    rows = 3 * torch.randn(R, 24, generator=gen)
    t = torch.randint(-1, C, (R,), generator=gen)
    out = K.point_ce_fwd(rows.cuda()[:, :C], t.cuda(), -1)
    r64 = rows[:, :C].double().requires_grad_(True)
    ref = TF.cross_entropy(r64, t, ignore_index=-1)
    ref.backward()
    assert abs(out[0].item() - ref.item()) <= 1e-6 * ref.item()
    g = K.point_ce_bwd(rows.cuda()[:, :C], t.cuda(), -1, out, torch.ones(1, device="cuda"))
    assert (g.cpu().double() - r64.grad).abs().max().item() <= 1e-6 * r64.grad.abs().max().item()
    # targets outside [0, C) that are not ignore_index are ignored as well (torch raises there)
    t_bad = t.clone()
    t_bad[::7] = C + 6
    got = K.point_ce_fwd(rows.cuda()[:, :C], t_bad.cuda(), -1)[0].item()
    want = TF.cross_entropy(rows[:, :C].double(), t_bad.masked_fill(t_bad >= C, -1),
                            ignore_index=-1).item()
    assert abs(got - want) <= 1e-6 * want
    none = torch.full((R,), -1, dtype=torch.long)
    assert torch.isnan(K.point_ce_fwd(rows.cuda()[:, :C], none.cuda(), -1)[0]).item()
    assert torch.isnan(TF.cross_entropy(rows[:, :C], none, ignore_index=-1)).item()


# ------------------------------------------------------------------------------- x16 fused loss
@pytest.mark.parametrize("hw_lo,hw,dtype", [((7, 9), (97, 129), torch.float32),
                                            ((33, 65), (513, 1025), torch.float32),
                                            ((13, 9), (190, 128), torch.float32),
                                            ((7, 9), (97, 129), torch.bfloat16)])
def test_upsample_ce_x16_forward_backward(hw_lo, hw, dtype):
    """seg_upsample_ce_* at 8.1 < 1/scale <= 16.1 (exact x16 and ragged 15.75 / 15.875), routed
    from PointRendLoss's F.interpolate of `coarse`, against torch on the CPU in float64."""
    from segmentron_amd import hip_ops as K
    from segmentron_amd.models.pointrend import CoarseLogits, CoarseUpsampled
    gen = torch.Generator().manual_seed(hw[0])
    N, C = 2, 19
    vec = K.vec_of(dtype)
    buf = (2 * torch.randn(N, hw_lo[0], hw_lo[1], (C + vec - 1) // vec * vec,
                           generator=gen)).to(dtype)
    t = torch.randint(-1, C, (N,) + hw, generator=gen)
    lo = buf.cuda()[..., :C].requires_grad_(True)
    pred = TF.interpolate(CoarseLogits(lo, hw_lo), hw, mode="bilinear", align_corners=True)
    assert isinstance(pred, CoarseUpsampled)
    loss = TF.cross_entropy(pred, t.cuda(), ignore_index=-1)
    assert pred._full is None  # fused: the [N, C, H, W] logits were never materialised
    loss.backward()
    x = buf[..., :C].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = TF.cross_entropy(TF.interpolate(x, hw, mode="bilinear", align_corners=True), t,
                           ignore_index=-1)
    ref.backward()
    tol = 1e-2 if dtype == torch.bfloat16 else 1e-5
    assert abs(loss.item() - ref.item()) <= tol * ref.item()
    g = lo.grad.float().cpu().double().permute(0, 3, 1, 2)
    gr = x.grad
    assert (g - gr).abs().max().item() <= 5 * tol * gr.abs().max().item()


# ------------------------------------------------------------------------------- the model
def _model(dtype):
    import segmentron_amd
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_list(["DATASET.NAME", "cityscape", "MODEL.MODEL_NAME", "PointRend",
                          "MODEL.BACKBONE", "xception65", "MODEL.DEEPLABV3_PLUS.ENABLE_DECODER",
                          "False", "TRAIN.BACKBONE_PRETRAINED", "False"])
    cfg.PHASE = "test"
    cfg.check_and_freeze()
    segmentron_amd.set_compute_dtype(dtype)
    model = segmentron_amd.get_segmentation_model()
    sd = O.state([(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    model.load_state_dict(sd)
    model = model.cuda().train()
    model.backbone.head.aspp.dropout.p = 0.0
    reset_cfg()
    return model, sd


def _train_step(model, x, y, over, cover):
    """PointRend forward at the recorded draws + PointRendLoss (solver/loss.py:371-387,
    verbatim) + backward."""
    from segmentron_amd.models.pointrend import point_sample
    with model.head.recorded_draws(over.cuda(), cover.cuda()):
        out = model(x.cuda())
    yc = y.cuda()
    pred = TF.interpolate(out["coarse"], yc.shape[-2:], mode="bilinear", align_corners=True)
    seg_loss = TF.cross_entropy(pred, yc, ignore_index=-1)
    gt_points = point_sample(yc.float().unsqueeze(1), out["points"], mode="nearest",
                             align_corners=False).squeeze_(1).long()
    points_loss = TF.cross_entropy(out["rend"], gt_points, ignore_index=-1)
    loss = seg_loss + points_loss
    loss.backward()
    return out, loss


def test_pointrend_train_step_fp32_matches_oracle():
    model, sd = _model(torch.float32)
    x = synth.synth_images(O.B, O.H, O.W, seed=1)
    y = synth.synth_targets(O.B, O.H, O.W, seed=1)
    over, cover = O.draws()  # the reference run's recorded draws (tests/golden/pointrend_ref_run.npz)
    P, n_imp = over.shape[1] // 3, int(0.75 * (over.shape[1] // 3))
    out, loss = _train_step(model, x, y, over, cover)
    assert set(out) == {"res2", "coarse", "rend", "points"}
    assert tuple(out["rend"].shape) == (O.B, 19, P) and tuple(out["points"].shape) == (O.B, P, 2)
    assert model.head._draws is None
    pts = out["points"].detach().cpu()
    assert torch.equal(pts[:, n_imp:], cover)
    # importance points = the oracle's top-n_imp of the over-generated points, up to oracle
    # near-ties at the n_imp-th value
    rloss, _, _, g32, coarse, _ = O.train(sd, x, y, torch.float32, pts=pts)
    unc = O.uncertainty_at(coarse.double(), over.double())
    for b in range(O.B):
        kth = unc[b].sort(descending=True)[0][n_imp - 1].item()
        want = set(torch.sort(-unc[b], stable=True)[1][:n_imp].tolist())
        lookup = {tuple(v): j for j, v in enumerate(over[b].tolist())}
        got = {lookup[tuple(v)] for v in pts[b, :n_imp].tolist()}
        delta = 1e-4 * unc[b].abs().max().item()
        assert all(abs(unc[b, j].item() - kth) <= delta for j in got ^ want), (b, got ^ want)
    g = np.load(os.path.join(GOLDEN, "pointrend_ref_run.npz"))
    print("PointRend train fp32: loss hip %.6f oracle %.6f reference %.6f"
          % (loss.item(), rloss, float(g["loss"])))
    assert abs(loss.item() - rloss) <= 1e-4 * rloss
    _, _, _, g64, _, _ = O.train(sd, x, y, torch.float64, pts=pts)
    params = dict(model.named_parameters())
    nh = nc = den = 0.0
    allw = []
    for k, t64 in g64.items():
        gh = params[k].grad
        assert gh is not None and torch.isfinite(gh).all(), k
        eh = (gh.cpu().double() - t64).norm().item()
        ec = (g32[k].double() - t64).norm().item()
        n64 = t64.norm().item()
        nh, nc, den = nh + eh ** 2, nc + ec ** 2, den + n64 ** 2
        # per tensor: as accurate as the CPU fp32 path (the tests/test_more_models.py yardstick)
        bound = 4 * ec + 1e-3 * n64 if n64 > 10 * ec else 20 * ec + 1e-12
        allw.append((eh / max(bound, 1e-30), k, eh, ec, n64))
    for w in sorted(allw, reverse=True)[:5]:
        print("   %-45s ratio %.2f err_hip %.3e err_cpu32 %.3e |g64| %.3e" % (w[1], w[0], w[2], w[3], w[4]))
    print("gradients vs fp64 oracle: global rel err HIP %.3e, CPU-fp32 %.3e"
          % ((nh / den) ** 0.5, (nc / den) ** 0.5))
    assert (nh / den) ** 0.5 <= 3 * (nc / den) ** 0.5 + 1e-4
    over_bound = [w for w in allw if w[0] > 1.0]
    assert len(over_bound) <= 0.10 * len(allw), (len(over_bound), len(allw))
    for _, k, eh, ec, n64 in over_bound:
        assert eh <= 4 * ec + 3e-2 * n64, (k, eh, ec, n64)
    for k in params:  # the MLP (incl. the small last bias) against the tight bound, always
        if k.startswith("head.mlp."):
            assert [w for w in allw if w[1] == k][0][0] <= 1.0, k


def _clear_pixel_check(fine, ref, tag):
    top2 = ref.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    err = (fine - ref).abs().amax(1)
    scale = ref.abs().max().item()
    clear = gap > 1e-3 * scale  # pixels whose selection cannot flip on rounding noise
    print("%s: max err %.3e on %d of %d clear pixels, argmax differs at %d"
          % (tag, err[clear].max().item(), int(clear.sum()), clear.numel(),
             int((fine.argmax(1) != ref.argmax(1)).sum())))
    assert (fine.argmax(1) != ref.argmax(1))[clear].sum().item() == 0
    assert (err[clear] <= 1e-3 * scale).float().mean().item() >= 0.999


def test_pointrend_eval_fp32_matches_oracle():
    model, sd = _model(torch.float32)
    model.eval()
    x = synth.synth_images(O.B, O.H, O.W, seed=1)
    with torch.no_grad():
        outs = model(x.cuda())
    assert isinstance(outs, tuple) and len(outs) == 1
    fine = outs[0].cpu()
    steps = []
    ref = O.evaluate(sd, x, steps)
    assert steps == [(14, 18), (28, 36), (56, 72), (O.H, O.W)]
    assert fine.shape == ref.shape == (O.B, 19, O.H, O.W) and fine.dtype == torch.float32
    _clear_pixel_check(fine, ref, "PointRend eval fp32 97x129")


def test_pointrend_eval_1025x2049():
    """The production shape, B = 1: four subdivision steps (130x258 .. 520x1032, then the input
    size), a 2.1 M-key top-k and a 160 MB float32 map.  The oracle's point head runs on the
    model's own encoder / head outputs (the backbone has its own full-size tests)."""
    from segmentron_amd import functional as F
    model, sd = _model(torch.float32)
    model.eval()
    x = synth.synth_images(1, 1025, 2049, seed=3)
    with torch.no_grad():
        fine = model(x.cuda())[0].cpu()
        c1, _, _, c4 = model.backbone.encoder(x.cuda())
        coarse = model.backbone.head(c4, c1)
        c1 = F.materialize(c1)
    c1 = c1.permute(0, 3, 1, 2).float().cpu()
    coarse = coarse.permute(0, 3, 1, 2).float().cpu()
    steps = []
    ref = O.eval_head({k: v for k, v in sd.items()}, c1, coarse, (1025, 2049), steps)
    assert steps == [(130, 258), (260, 516), (520, 1032), (1025, 2049)]
    assert fine.shape == ref.shape == (1, 19, 1025, 2049)
    _clear_pixel_check(fine, ref, "PointRend eval fp32 1025x2049")


def test_pointrend_bf16_train_step_within_the_bf16_bar():
    """bf16 step at the same recorded draws: finite, and its loss within the 2e-2 relative bar
    of the C3 bf16 train test (tests/test_model_gpu.py) of the fp32 step's."""
    import segmentron_amd
    x = synth.synth_images(O.B, O.H, O.W, seed=1)
    y = synth.synth_targets(O.B, O.H, O.W, seed=1)
    over, cover = O.draws()
    model32, _ = _model(torch.float32)
    _, l32 = _train_step(model32, x, y, over, cover)
    del model32
    try:
        model, _ = _model(torch.bfloat16)
        _, loss = _train_step(model, x, y, over, cover)
        print("PointRend train bf16: loss %.5f vs fp32 %.5f" % (loss.item(), l32.item()))
        assert torch.isfinite(loss).item()
        assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
        assert abs(loss.item() - l32.item()) <= 2e-2 * l32.item()
    finally:
        segmentron_amd.set_compute_dtype(torch.float32)
