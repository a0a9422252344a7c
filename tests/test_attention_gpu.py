"""The attention heads at the kernel classes their real maps reach.

1. Short-K products on the direct-to-LDS 1x1 kernels (gemm_glds.h / gemm_glds4.h): the ring of
   four 32-k slots with FEWER slots of K than the ring is deep (K = 8 .. 96; every other case of
   the suite has K >= 200), on each of the three tile-row classes, the class pinned through
   seg_conv_gemm_stat_rows before any value is compared.
2. DANet position / channel attention (functional._PAMFn / _CAMFn) at a 65 x 65 map with C = 512,
   D = 64 — where the GEMMs leave the 128x128 tile kernel — and at two 47 x 45 images.
3. Criss-cross attention (csrc/cca.hip) kernel by kernel at the trip boundaries of its 64-lane
   loops, the 512-entry limit, empty row / column parts, ragged channel trips, pitched inputs.

Every reference is float64 on the CPU, computed once per case and shared by both dtypes: the
inputs are rounded to bf16 first, which float32 holds exactly."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as TF

from _util import DEV, assert_close, quant, rnd, to_cpu_nchw, to_dev_nhwc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import torch_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
BF = torch.bfloat16


def K():
    from segmentron_amd import hip_ops
    return hip_ops


def F():
    from segmentron_amd import functional
    return functional


def _unit_roundoff(dtype):
    """largest relative error of one round-to-nearest: 2^-p for p significant bits"""
    return 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -8


def _err(got, ref, scale=None):
    s = ref.abs().max().item() if scale is None else scale
    return (got.double() - ref.double()).abs().max().item() / max(s, 1e-12)


# ------------------------------------------------------------- 1. short K, direct-to-LDS kernels
# (H, W, O, tile rows): glds_pick_rows by hand, confirmed by the query in every case —
#   4225 x 4232: 17 column tiles; 256 rows 289 tiles, 224 rows 323, 192 rows 391: two rounds each,
#                the shortest tile wins                                   -> 192 rows, eight waves
#   26000 x 392: 204 / 234 / 272 tiles: 224 rows still fit one round      -> 224 rows, four waves
#   30000 x 392: 236 / 268 / 314 tiles: only 256 rows fit one round       -> 256 rows, eight waves
# (at 256 rows the row count alone cannot tell the direct-to-LDS kernel from conv_gemm_px256;
# every argument conv_gemm_glds_usable looks at — bf16, no prologue / bias, K, O and both pitches
# multiples of 8 — is as it wants it)
GLDS_GEOMS = {"192rows": (65, 65, 4232, 192), "224rows": (130, 200, 392, 224),
              "256rows": (150, 200, 392, 256)}
# in ring slots of 32: one quarter-filled, one full, one + a partial, two, three (the ring holds 4)
SHORT_K = [8, 32, 40, 64, 96]


def _stat_rows(dtype, M, C, O):
    Km = K()
    return Km.LIB.query("seg_conv_gemm_stat_rows", Km._DT[dtype], 1, 1, M, C, O, 1, 1, 1, 0, 1, 0,
                        0, 0)


def _check_stats(partial, vals, O):
    """the bars of test_conv_gemm_fwd: column sums of the partial rows vs float64 sums of `vals`"""
    sums = K().colsum(partial.view(partial.shape[0], -1)).cpu()
    assert_close(sums[:O], vals.sum((0, 2, 3)), torch.float32, "sum",
                 scale=vals.abs().sum((0, 2, 3)).max().item(), fac=5)
    assert_close(sums[O:], (vals * vals).sum((0, 2, 3)), torch.float32, "sumsq", fac=5)


def _short_k_case(dtype, H, W, C, O, bm, sl):
    M = H * W
    rows = _stat_rows(dtype, M, C, O)
    assert rows == (M + bm - 1) // bm, "%d x %d x %d left the %d-row class: %d statistics rows" % (
        M, O, C, bm, rows)
    x = quant(rnd((1, C, H, W), 1), dtype)
    w = quant(rnd((O, C, 1, 1), 2, (2.0 / C) ** 0.5), dtype)
    ref = TF.conv2d(x.double(), w.double())
    xd = to_dev_nhwc(x, dtype, pitch=C + 16 if sl else None, off=8 if sl else 0)
    wp = F().pack_conv_weight(w.to(DEV), C, dtype)
    out, vec = None, 8 if dtype == BF else 4
    if sl:
        pitch = O + 2 * vec
        out = torch.full((1, H, W, pitch), float("nan"), dtype=dtype, device=DEV)[..., vec:vec + O]
    y, partial = K().conv_gemm(xd, wp, O, 1, 1, 1, 0, 1, None, None, out, want_stats=True)
    assert partial.shape[0] == rows
    got = to_cpu_nchw(y)
    assert_close(got, ref, dtype, "y")
    # bf16: statistics of the values AS STORED (test_conv_gemm_fwd, the wide kernels)
    _check_stats(partial, quant(ref.float(), dtype).double() if dtype == BF else ref, O)
    if sl:  # nothing outside the slice was touched
        full = y.as_strided((1, H, W, pitch), y.stride(), y.storage_offset() - vec)
        assert torch.isnan(full[..., :vec].float()).all() and torch.isnan(full[..., vec + O:].float()).all()


@pytest.mark.parametrize("k", SHORT_K)
@pytest.mark.parametrize("geom", list(GLDS_GEOMS))
def test_short_k_on_the_direct_to_lds_kernels(geom, k):
    """1x1 conv_gemm with 1 .. 3 ring slots of K (bf16) vs TF.conv2d in float64: y, the statistics
    rows of the values as stored; K = 40 reads and writes channel slices of NaN-filled buffers."""
    H, W, O, bm = GLDS_GEOMS[geom]
    _short_k_case(BF, H, W, k, O, bm, sl=(k == 40))


def test_short_k_on_conv_gemm_px256_fp32():
    """The attention energy product (K = 64, O = 4232 at 4225 pixels) in float32: 256-pixel tiles
    of conv_gemm_px256 (17 statistics rows; the 128x128 tile kernel would write 34)."""
    _short_k_case(torch.float32, 65, 65, 64, 4232, 256, sl=False)


@pytest.mark.parametrize("want_stats", [False, True], ids=["correction", "correction+stats"])
@pytest.mark.parametrize("geom,k", [("224rows", 40), ("192rows", 8)])
def test_short_k_epilogue_correction_on_the_direct_to_lds_kernels(geom, k, want_stats):
    """y = acc - c0[o] - c1[o] * x[p][o] at short K (bf16).  With statistics the launch follows the
    statistics rows (pinned); correction alone never takes 224 rows (launch_glds_rows): 26000 x 392
    then runs 256-row tiles, 4225 x 4232 stays on 192 — both on eight waves, and no row count is
    handed out that could be pinned."""
    H, W, O, bm = GLDS_GEOMS[geom]
    M, dtype = H * W, BF
    rows = _stat_rows(dtype, M, k, O)
    assert rows == (M + bm - 1) // bm, (rows, bm)
    x = quant(rnd((1, k, H, W), 1), dtype)
    w = quant(rnd((O, k, 1, 1), 2, (2.0 / k) ** 0.5), dtype)
    xe = quant(rnd((1, O, H, W), 3), dtype)
    c0, c1 = rnd((O,), 4, 0.05), rnd((O,), 5, 0.3)
    ref = TF.conv2d(x.double(), w.double()) - c0.view(1, -1, 1, 1).double() \
        - c1.view(1, -1, 1, 1).double() * xe.double()
    wp = F().pack_conv_weight(w.to(DEV), k, dtype)
    y, partial = K().conv_gemm(to_dev_nhwc(x, dtype), wp, O, 1, 1, 1, 0, 1, None, None, None,
                               want_stats=want_stats,
                               ep=(to_dev_nhwc(xe, dtype), c0.to(DEV), c1.to(DEV)))
    got = to_cpu_nchw(y)
    assert_close(got, ref, dtype, "corrected y")
    assert (partial is not None) == want_stats
    if want_stats:
        assert partial.shape[0] == rows
        _check_stats(partial, got.double(), O)  # the values as stored


# ------------------------------------------------------------- 2. DANet attention at a real map
# name: (N, H, W, C, D).  65 x 65: the smallest odd map with >= 4096 pixels; P = 4225 pads to 4232
# (bf16) / 4228 (fp32) columns, so the masked columns are live.  2 x 47 x 45: P = 2115 keeps the
# forward on the 128x128 tile kernel while gemm_tn (>= 2048 pixels) is on conv_wgrad_glds.
DANET = {"65x65": (1, 65, 65, 512, 64), "2x47x45": (2, 47, 45, 512, 64)}
GAMMA = 0.7


@functools.lru_cache(maxsize=None)
def _danet_ref(name):
    """inputs (bf16-exact) and the float64 reference of PAM and CAM: forward, every gradient, the
    un-scaled attention output `raw` (for the d gamma bound)."""
    N, H, W, C, D = DANET[name]
    P = H * W
    img = torch.ones(N, 1, 1, 1)
    if N > 1:  # the second image is not a copy of the first in any statistic
        img[1] = 1.5
    x = quant(rnd((N, C, H, W), 1, 0.7) * img, BF)
    q = quant(rnd((N, D, H, W), 2, 0.3) * img, BF)
    k = quant(rnd((N, D, H, W), 3, 0.3), BF)
    v = quant(rnd((N, C, H, W), 4) / img, BF)
    g = quant(rnd((N, C, H, W), 5), BF)
    xc = quant(rnd((N, C, H, W), 6, 0.05) * img, BF)
    gamma = torch.tensor([GAMMA])
    out = {"in": (q, k, v, x, g, xc, gamma)}
    # ---- PAM: torch.bmm -> softmax -> torch.bmm, gamma * out + x (module.py:100-130)
    qr, kr, vr, xr, gr = [t.double().requires_grad_() for t in (q, k, v, x, gamma)]
    att = torch.softmax(torch.bmm(qr.view(N, -1, P).permute(0, 2, 1), kr.view(N, -1, P)), dim=-1)
    raw = torch.bmm(vr.view(N, -1, P), att.permute(0, 2, 1)).view(N, C, H, W)
    ref = gr * raw + xr
    ref.backward(g.double())
    out["pam"] = dict(fwd=ref.detach(), raw=raw.detach(), dq=qr.grad, dk=kr.grad, dv=vr.grad,
                      dx=xr.grad, dgamma=gr.grad.item(),
                      rowmax=att.detach().max(-1)[0].mean().item(), att=att.detach()[0])
    # ---- CAM: softmax(max - X^T X) (module.py:133-162)
    xr, gr = xc.double().requires_grad_(), gamma.double().requires_grad_()
    pq = xr.view(N, C, -1)
    energy = torch.bmm(pq, pq.permute(0, 2, 1))
    att = torch.softmax(energy.max(-1, keepdim=True)[0].expand_as(energy) - energy, dim=-1)
    raw = torch.bmm(att, pq).view(N, C, H, W)
    ref = gr * raw + xr
    ref.backward(g.double())
    out["cam"] = dict(fwd=ref.detach(), raw=raw.detach(), dx=xr.grad, dgamma=gr.grad.item(),
                      rowmax=att.detach().max(-1)[0].mean().item())
    return out


def _dgamma_bound(g, raw, dtype):
    """d gamma = <dout, raw> is ONE scalar out of a cancelling sum: bounded against the
    root-sum-square of its terms as in test_cca.py (bf16 stores raw rounded, 2^-9 relative and
    independent per element: 4 sigma of that walk; fp32: 1e-4 of the same scale)."""
    sigma = (g.double() * raw).pow(2).sum().sqrt().item()
    return sigma, (1e-4 if dtype == torch.float32 else 4 * 2.0 ** -9) * sigma


def _part_close(got, ref, residual, dtype, what, fac):
    """The attention's share of a sum that a residual dominates (out = gamma * raw + x, dx = dout +
    ...): got - residual vs ref - residual at the bar of `assert_close`, on the scale of that share
    alone, plus the ONE rounding of the stored total, which the subtraction cannot take out: half
    an ulp, at most the unit roundoff 2^-24 (fp32) / 2^-8 (bf16: 8 significant bits — half an
    ulp is 2^-8 of a value just above a power of two, 2^-9 only just below one) of its largest
    element."""
    part = (ref - residual).double()
    ulp = _unit_roundoff(dtype) * ref.abs().max().item()
    bar = (2e-5 if dtype == torch.float32 else 6e-3) * fac * part.abs().max().item() + ulp
    err = ((got.double() - residual.double()) - part).abs().max().item()
    assert err <= bar, "%s: attention share off by %.3e > %.3e" % (what, err, bar)
    return err / part.abs().max().item()


@pytest.mark.parametrize("name,dtype", [("65x65", torch.float32), ("65x65", BF), ("2x47x45", BF)],
                         ids=["65x65-fp32", "65x65-bf16", "2x47x45-bf16"])
def test_danet_attention_at_a_real_map(name, dtype):
    """functional.position_attention / channel_attention vs the float64 formulas, forward and every
    gradient, at the bars of test_danet_position_and_channel_attention_fwd_bwd (fac 3 / 6);
    d gamma against the root-sum-square of its terms; the attention's own share of the forward
    and of dx apart from the residual that dominates them.  Prints the parity line DESIGN.md
    quotes."""
    Fm = F()
    ref = _danet_ref(name)
    q, k, v, x, g, xc, gamma = ref["in"]
    fac = 3 if dtype == torch.float32 else 6
    # the reference attentions are far from one-hot: every path of the gradient carries weight
    assert ref["pam"]["rowmax"] <= 0.5 and ref["cam"]["rowmax"] <= 0.5, (
        ref["pam"]["rowmax"], ref["cam"]["rowmax"])
    line = []
    # ---- PAM
    r = ref["pam"]
    dev = [to_dev_nhwc(t, dtype).requires_grad_() for t in (q, k, v, x)]
    gd = gamma.to(DEV).requires_grad_()
    y = Fm.position_attention(*dev, gd)
    y.backward(to_dev_nhwc(g, dtype))
    grads = {n: to_cpu_nchw(d.grad) for n, d in zip("qkvx", dev)}
    sigma, bound = _dgamma_bound(g, r["raw"], dtype)
    line.append("PAM fwd %.2e (attention share %.2e)" % (
        _err(to_cpu_nchw(y), r["fwd"]), _err(to_cpu_nchw(y) - x, r["fwd"] - x)))
    line += ["d%s %.2e" % (n, _err(grads[n], r["d" + n])) for n in "qkvx"]
    line.append("dgamma %.2e sigma (bound %.2e)" % (abs(gd.grad.item() - r["dgamma"]) / sigma,
                                                    bound / sigma))
    print("danet %s %s: %s" % (name, IDS[DTYPES.index(dtype)], ", ".join(line)))
    assert_close(to_cpu_nchw(y), r["fwd"], dtype, "PAM fwd", fac=fac)
    _part_close(to_cpu_nchw(y), r["fwd"], x, dtype, "PAM fwd", fac)
    for n in "qkvx":
        assert_close(grads[n], r["d" + n], dtype, "PAM d" + n, fac=fac)
    assert abs(gd.grad.item() - r["dgamma"]) <= bound, (gd.grad.item(), r["dgamma"], bound)
    # ---- CAM
    r = ref["cam"]
    xd = to_dev_nhwc(xc, dtype).requires_grad_()
    gd = gamma.to(DEV).requires_grad_()
    y = Fm.channel_attention(xd, gd)
    y.backward(to_dev_nhwc(g, dtype))
    dx = to_cpu_nchw(xd.grad)
    sigma, bound = _dgamma_bound(g, r["raw"], dtype)
    print("danet %s %s: CAM fwd %.2e (attention share %.2e), dx %.2e (attention share %.2e), "
          "dgamma %.2e sigma (bound %.2e)" % (
              name, IDS[DTYPES.index(dtype)], _err(to_cpu_nchw(y), r["fwd"]),
              _err(to_cpu_nchw(y) - xc, r["fwd"] - xc), _err(dx, r["dx"]),
              _err(dx - g, r["dx"] - g), abs(gd.grad.item() - r["dgamma"]) / sigma, bound / sigma))
    assert_close(to_cpu_nchw(y), r["fwd"], dtype, "CAM fwd", fac=fac)
    _part_close(to_cpu_nchw(y), r["fwd"], xc, dtype, "CAM fwd", fac)
    assert_close(dx, r["dx"], dtype, "CAM dx", fac=fac)
    _part_close(dx, r["dx"], g, dtype, "CAM dx", fac)
    assert abs(gd.grad.item() - r["dgamma"]) <= bound, (gd.grad.item(), r["dgamma"], bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_danet_real_map_gemms_take_the_wide_kernel_classes(dtype):
    """Where the GEMMs of the 65 x 65 case go (the table in DESIGN.md, "attention heads"), by the
    library's own queries: bf16 products with >= 384 outputs on the direct-to-LDS kernel at 192
    rows, fp32 ones on 256-pixel tiles of conv_gemm_px256; dq (64 outputs) stays on the 128x128
    tile kernel; bf16 gemm_tn on conv_wgrad_glds (its split count differs from the
    first-generation kernel's), fp32 gemm_tn on the first-generation kernel."""
    Km = K()
    N, H, W, C, D = DANET["65x65"]
    P = H * W
    Pp = (P + Km.vec_of(dtype) - 1) // Km.vec_of(dtype) * Km.vec_of(dtype)
    bf = dtype == BF
    wide = (P + 191) // 192 if bf else (P + 255) // 256
    nt = {"e = q k^T": (D, Pp, wide), "raw = a v^T": (Pp, C, wide), "dA = dO v^T": (C, Pp, wide),
          "dq = dE k": (Pp, D, (P + 127) // 128), "CAM raw = x a^T": (C, C, wide)}
    for what, (Kd, O, rows) in nt.items():
        assert _stat_rows(dtype, P, Kd, O) == rows, what
    # gemm_tn(a [P, M], b [P, K]): a weight gradient with O = M, C = K over P pixels
    tn = {"dv = a^T dO": (Pp, C, 2 if bf else 3), "dk = dE^T q": (Pp, D, 8 if bf else 15),
          "Gram = x^T x": (C, C, 9 if bf else 17)}
    for what, (O, Cc, splits) in tn.items():
        got = Km.LIB.query("seg_conv_gemm_wgrad_splits", Km._DT[dtype], 1, 1, P, Cc, O, 1, 1, 1,
                           0, 1, 0)
        assert got == splits, (what, got)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_rows_at_4225_pixels_are_probabilities_with_zero_padding(dtype):
    """gemm_nt + row_softmax as _PAMFn.forward runs them at P = 4225: every row sums to 1 (1e-3 in
    bf16, 1e-5 in fp32), the padding columns P .. Pp are exact zeros, the rows match float64."""
    Km = K()
    ref = _danet_ref("65x65")
    q, k = ref["in"][:2]
    P, vec = 65 * 65, Km.vec_of(dtype)
    Pp = (P + vec - 1) // vec * vec
    qd = to_dev_nhwc(q, dtype)[0].reshape(P, -1)
    kp = torch.zeros((Pp, qd.shape[1]), dtype=dtype, device=DEV)
    kp[:P] = to_dev_nhwc(k, dtype)[0].reshape(P, -1)
    a = Km.row_softmax(Km.gemm_nt(qd.contiguous(), kp), P, dtype)
    assert tuple(a.shape) == (P, Pp) and Pp > P
    assert (a[:, P:].float() == 0).all()
    s = a[:, :P].double().sum(1)
    assert (s - 1).abs().max().item() <= (1e-5 if dtype == torch.float32 else 1e-3)
    assert_close(a[:, :P].float().cpu(), ref["pam"]["att"], dtype, "attention rows", fac=3)


# ------------------------------------------------------------- 3. criss-cross attention
# name: (N, H, W, C, C').  The dot kernels give lane l the entries l + 64 i, i < 8, of the
# L = H + W - 1 attended ones; the map kernels give it 8 (bf16) / 4 (fp32) channels per trip of 64
# lanes; one wave per pixel, four per block.
CCA_SHAPES = {
    "L64": (2, 33, 32, 64, 8),          # one trip exactly full
    "L65-row": (1, 1, 65, 64, 8),       # no column part
    "L65-col": (1, 65, 1, 64, 8),       # no row partner but the pixel itself
    "L128": (1, 3, 126, 64, 8),         # two full trips; 378 pixels: a ragged last block
    "L129": (2, 64, 66, 520, 72),       # C = 520: ragged 2nd (bf16) / 3rd (fp32) channel trip
    "L512": (1, 3, 510, 520, 64),       # the limit: all eight trips
}
CCA_IDS = list(CCA_SHAPES)


def _lhw(t):      # oracle [N, L, H, W] -> kernel layout [N, H, W, L]
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _cca_in(name):
    """bf16-exact inputs; q . k has unit standard deviation whatever C' is"""
    N, H, W, C, Cq = CCA_SHAPES[name]
    q = quant(rnd((N, Cq, H, W), 11, Cq ** -0.25), BF)
    k = quant(rnd((N, Cq, H, W), 12, Cq ** -0.25), BF)
    v, x, dout = [quant(rnd((N, C, H, W), s), BF) for s in (13, 14, 15)]
    return q, k, v, x, dout


@functools.lru_cache(maxsize=None)
def _cca_att(name):
    """float64 softmax(cca_weight) [N, L, H, W] and the float32 copy the kernels are handed"""
    q, k = _cca_in(name)[:2]
    att = torch.softmax(R.cca_weight(q.double(), k.double()), 1)
    return att, _lhw(att).float()


@functools.lru_cache(maxsize=None)
def _cca_map_ref(name, transposed):
    """cca_map(att32, v) in float64; transposed: its adjoint, through autograd of the oracle
    (<map(w, b), c> == <b, map^T(w, c)>: map^T(w, c) = d <map(w, b), c> / d b)"""
    v = _cca_in(name)[2].double()
    w = _cca_att(name)[1].double().permute(0, 3, 1, 2)  # the fp32 weights, exactly
    if not transposed:
        return R.cca_map(w, v)
    b = torch.zeros_like(v).requires_grad_()
    R.cca_map(w, b).backward(v)
    return b.grad


@functools.lru_cache(maxsize=None)
def _cca_bwd_ref(name, scale):
    """d energy of <dout, scale * cca_map(softmax(energy), v)> by autograd of the oracle"""
    q, k, v, _, dout = _cca_in(name)
    e = R.cca_weight(q.double(), k.double()).requires_grad_()
    (scale * R.cca_map(torch.softmax(e, 1), v.double())).backward(dout.double())
    return _lhw(e.grad)


def _nhwc_cpu(t_nhwc):
    return t_nhwc.detach().float().cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CCA_IDS)
def test_cca_attention_matches_softmax_of_the_oracle_energies(name, dtype):
    """The output is float32 in both dtypes and the inputs are exact in both: the float32 bar."""
    q, k = _cca_in(name)[:2]
    N, H, W = CCA_SHAPES[name][:3]
    qd, kd = to_dev_nhwc(q, dtype), to_dev_nhwc(k, dtype)
    att = K().cca_attention(qd, kd)
    assert tuple(att.shape) == (N, H, W, H + W - 1) and att.dtype == torch.float32
    assert torch.equal(att, K().cca_attention(qd, kd))
    got = _nhwc_cpu(att)
    assert (got.double().sum(-1) - 1).abs().max().item() < 1e-5 and got.min().item() >= 0
    assert_close(got, _lhw(_cca_att(name)[0]), torch.float32, "attention")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("transposed", [False, True], ids=["map", "mapT"])
@pytest.mark.parametrize("name", CCA_IDS)
def test_cca_map_and_its_epilogue(name, transposed, dtype):
    """out = gamma * sum + res with every combination the callers use; `raw` is the un-scaled sum
    (bit-equal to the plain launch), and without gamma and res out == raw bit for bit."""
    Km = K()
    v, x = _cca_in(name)[2:4]
    wt = _cca_att(name)[1].to(DEV)
    ref = _cca_map_ref(name, transposed)
    b, res = to_dev_nhwc(v, dtype), to_dev_nhwc(x, dtype)
    gamma = torch.tensor([GAMMA], device=DEV)
    plain = Km.cca_map(wt, b, transposed)
    assert_close(to_cpu_nchw(plain), ref, dtype, "plain")
    out, raw = Km.cca_map(wt, b, transposed, want_raw=True)
    assert torch.equal(out, raw) and torch.equal(out, plain)
    assert_close(to_cpu_nchw(Km.cca_map(wt, b, transposed, gamma=gamma)), GAMMA * ref, dtype, "gamma")
    assert_close(to_cpu_nchw(Km.cca_map(wt, b, transposed, res=res)), ref + x.double(), dtype, "res")
    out, raw = Km.cca_map(wt, b, transposed, gamma=gamma, res=res, want_raw=True)
    assert torch.equal(raw, plain)
    assert_close(to_cpu_nchw(out), GAMMA * ref + x.double(), dtype, "gamma + res")
    # the attention's share apart from the residual, which is several times larger at L >= 128
    err = ((to_cpu_nchw(out).double() - x.double()) - GAMMA * ref).abs().max().item()
    half_ulp = _unit_roundoff(dtype)  # the one rounding of the stored total (see _part_close)
    assert err <= (2e-5 if dtype == torch.float32 else 6e-3) * GAMMA * ref.abs().max().item() \
        + half_ulp * (GAMMA * ref + x.double()).abs().max().item(), err
    again, raw2 = Km.cca_map(wt, b, transposed, gamma=gamma, res=res, want_raw=True)
    assert torch.equal(again, out) and torch.equal(raw2, raw)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("scale", [None, GAMMA], ids=["noscale", "scale"])
@pytest.mark.parametrize("name", CCA_IDS)
def test_cca_attention_bwd_matches_autograd_of_the_oracle(name, scale, dtype):
    """dE = att * (dA - sum att dA), dA = scale * dout . v[partner]; float32 out, exact inputs."""
    Km = K()
    v, _, dout = _cca_in(name)[2:]
    att = _cca_att(name)[1].to(DEV)
    dd, vd = to_dev_nhwc(dout, dtype), to_dev_nhwc(v, dtype)
    sc = None if scale is None else torch.tensor([scale], device=DEV)
    de = Km.cca_attention_bwd(dd, vd, att, sc)
    assert torch.equal(de, Km.cca_attention_bwd(dd, vd, att, sc))
    assert_close(_nhwc_cpu(de), _cca_bwd_ref(name, 1.0 if scale is None else scale),
                 torch.float32, "dE")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cca_kernels_read_nothing_behind_a_channel_slice(dtype):
    """Every input as a channel slice of a wider NaN-filled buffer (L = 129, C = 520): the same
    arithmetic on the same values, so the results equal the dense launches bit for bit."""
    Km = K()
    name = "L129"
    q, k, v, x, dout = _cca_in(name)
    C, Cq = CCA_SHAPES[name][3:]
    wt = _cca_att(name)[1].to(DEV)
    gamma = torch.tensor([GAMMA], device=DEV)
    dense = lambda t: to_dev_nhwc(t, dtype)
    sl = lambda t, c: to_dev_nhwc(t, dtype, pitch=c + 24, off=8)
    assert Km.nhwc(sl(q, Cq))[4] == Cq + 24
    assert torch.equal(Km.cca_attention(sl(q, Cq), sl(k, Cq)), Km.cca_attention(dense(q), dense(k)))
    for tr in (False, True):
        a = Km.cca_map(wt, sl(v, C), tr, gamma=gamma, res=sl(x, C), want_raw=True)
        b = Km.cca_map(wt, dense(v), tr, gamma=gamma, res=dense(x), want_raw=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.isfinite(a[0].float()).all()
    assert torch.equal(Km.cca_attention_bwd(sl(dout, C), sl(v, C), wt, gamma),
                       Km.cca_attention_bwd(dense(dout), dense(v), wt, gamma))


@functools.lru_cache(maxsize=None)
def _cca_e2e_ref(name):
    q, k, v, x, dout = _cca_in(name)
    leaves = [t.double().requires_grad_() for t in (q, k, v, x, torch.tensor([GAMMA]))]
    raw = R.cca_map(torch.softmax(R.cca_weight(leaves[0], leaves[1]), 1), leaves[2])
    ref = leaves[4] * raw + leaves[3]
    ref.backward(dout.double())
    return ref.detach(), raw.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["L129", "L512"])
def test_criss_cross_attention_end_to_end_at_the_loop_limits(name, dtype):
    """functional.criss_cross_attention, forward and the five gradients, at the bars of
    test_criss_cross_attention_fwd_bwd_matches_oracle (2e-5 / 1.2e-2 of each tensor's scale; d gamma
    against the root-sum-square of its terms)."""
    q, k, v, x, dout = _cca_in(name)
    ref, raw, grads = _cca_e2e_ref(name)
    dev = [to_dev_nhwc(t, dtype).requires_grad_() for t in (q, k, v, x)]
    dg = torch.tensor([GAMMA], device=DEV).requires_grad_()
    out = F().criss_cross_attention(*dev, dg)
    out.backward(to_dev_nhwc(dout, dtype))
    tol = 2e-5 if dtype == torch.float32 else 1.2e-2
    for what, got, want in [("out", out, ref)] + [("d" + n, d.grad, r)
                                                  for n, d, r in zip("qkvx", dev, grads)]:
        err = _err(to_cpu_nchw(got), want)
        assert err <= tol, "%s: max-normalised error %.3e > %.3e" % (what, err, tol)
    sigma, bound = _dgamma_bound(dout, raw, dtype)
    assert abs(dg.grad.item() - grads[4].item()) <= bound + 1e-6, (dg.grad.item(), grads[4].item(),
                                                                  bound)
