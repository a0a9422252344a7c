"""GPU: the fused pair of line convolutions (csrc/conv_line_pair.hip, C = 40):
    mid = lineA(act(x)) + biasA,  y = lineB(mid) + biasB (+ add)
for both axis orders, both dtypes, lines of 5, 37 and 40 pixels and dilation 1, 2 and 16 (which
includes d >= L), with and without the biases, the prologue, the addend and a null `mid`.

  1. y and mid are BIT-IDENTICAL to the two single launches (hip_ops.conv_line_bias twice).
  2. y against a float64 conv2d whose `mid` is rounded to the dtype.  With the single launch's
     bound b(n, S, r) = n * 2^-23 * S (+ 2^-8 |r| in bf16), of tests/test_conv_line_gpu.py:
         |y - y64| <= b_B + lineB(|w_B|) applied to (b_A + [bf16] 2^-9 |mid64|)
     (b_A bounds the device's mid against mid64, 2^-9 |mid64| the oracle's own rounding of it).
  3. statistics of y and the per-channel sums of mid against the stored values, n = pixels.
  4. a line beyond the LDS budget is refused by the host query and line_pair_bn then gives the
     two-launch result.
  5. every launch repeated gives the same bits."""
import pytest
import torch
import torch.nn as nn

import test_conv_line_gpu as L
from _util import DEV, quant, rnd, to_cpu_nchw, to_dev_nhwc

pytestmark = pytest.mark.gpu

DTYPES, IDS, H_, W_ = L.DTYPES, L.IDS, L.H_, L.W_
C, N = 40, 2
LINES = [5, 37, 40]
DILS = [1, 2, 16]
VARIANTS = {"plain": (), "biases": ("ba", "bb"), "bias_a": ("ba",), "pro": ("pro", "ba"),
            "add": ("add", "bb"), "nomid": ("nomid", "ba", "bb"),
            "all": ("pro", "ba", "bb", "add")}


def _shape(order, line):
    """order 0: lines along W (A = H); 1: lines along H (A = W).  The other extent is 6."""
    return (6, line) if order == 0 else (line, 6)


def _case(order, line, d, dtype, opts, seed):
    K, F = L._K(), L._F()
    H, W = _shape(order, line)
    ax_a, ax_b = (H_, W_) if order == 0 else (W_, H_)
    pro_kind = "affine_relu" if "pro" in opts else "none"
    x, wa, s, t = L._inputs((N, H, W, C, ax_a, d), dtype, seed, pro_kind)
    wb = L._weight(C, ax_b, dtype, seed + 11)
    ba = rnd((C,), seed + 12, 0.5) if "ba" in opts else None
    bb = rnd((C,), seed + 13, 0.5) if "bb" in opts else None
    add = quant(rnd((N, C, H, W), seed + 14), dtype) if "add" in opts else None
    pa, pb = F.pack_conv_weight(wa.to(DEV), C, dtype), F.pack_conv_weight(wb.to(DEV), C, dtype)
    xd = to_dev_nhwc(x, dtype, pitch=C + 16, off=8)
    addd = None if add is None else to_dev_nhwc(add, dtype, pitch=C + 8, off=8)
    bad, bbd = (None if b is None else b.to(DEV) for b in (ba, bb))
    pro = L._pro_arg(K, pro_kind, s, t)
    assert K.conv_line_pair_ok(dtype, C, line, d)
    want_mid = "nomid" not in opts

    def run():
        obuf = torch.full((N, H, W, 264), L.SENTINEL, dtype=dtype, device=DEV)
        r = K.conv_line_pair(xd, pa, bad, pb, bbd, order, d, pro, out=obuf[..., 80:120], add=addd,
                             want_mid=want_mid, want_stats=True, want_mid_sums=True)
        keep = torch.ones(264, dtype=torch.bool, device=DEV)
        keep[80:120] = False
        assert (obuf[..., keep] == L.SENTINEL).all()
        return r
    y, mid, stat, msum = run()
    # 1. the two single launches
    mid1, _ = K.conv_line_bias(xd, pa, bad, ax_a, d, pro)
    y1, _ = K.conv_line_bias(mid1, pb, bbd, ax_b, d, add=addd)
    assert torch.equal(y, y1)
    assert (mid is None) == (not want_mid)
    if want_mid:
        assert torch.equal(mid, mid1)
    # 2. float64, mid rounded to the dtype
    xa = L._activated(x, pro_kind, s, t, dtype)
    mid64 = L._conv64(xa, wa.double(), ax_a, d)
    s_a = L._conv64(xa.abs(), wa.double().abs(), ax_a, d)
    n_a = 3 * C
    if ba is not None:
        mid64, s_a, n_a = mid64 + ba.double().view(1, -1, 1, 1), \
            s_a + ba.double().abs().view(1, -1, 1, 1), n_a + 1
    b_a = L._bound(n_a, s_a, mid64, dtype)
    if dtype == torch.bfloat16:
        b_a = b_a + 2.0 ** -9 * mid64.abs()
    mq = quant(mid64.float(), dtype).double()
    y64 = L._conv64(mq, wb.double(), ax_b, d)
    s_b = L._conv64(mq.abs(), wb.double().abs(), ax_b, d)
    n_b = 3 * C
    for extra in (None if bb is None else bb.double().view(1, -1, 1, 1),
                  None if add is None else add.double()):
        if extra is not None:
            y64, s_b, n_b = y64 + extra, s_b + extra.abs(), n_b + 1
    bound = L._bound(n_b, s_b, y64, dtype) + L._conv64(b_a, wb.double().abs(), ax_b, d)
    got = to_cpu_nchw(y).double()
    assert torch.isfinite(got).all()
    over = ((got - y64).abs() - bound).max().item()
    assert over <= 0.0, "y: %.3e beyond the bound" % over
    # 3. statistics of y and sums of mid, of the values as stored
    P = N * H * W
    rows = K.LIB.query("seg_conv_line_pair_rows", N, H, W, order)
    assert rows == N * (H if order == 0 else W)
    assert tuple(stat.shape) == (rows, 2, C) and tuple(msum.shape) == (rows, C)
    sums = K.colsum(stat.view(rows, 2 * C), f64=False).double().cpu().view(2, C)
    a1, a2 = got.abs().sum((0, 2, 3)), (got * got).sum((0, 2, 3))
    assert ((sums[0] - got.sum((0, 2, 3))).abs() <= P * 2.0 ** -23 * a1).all()
    assert ((sums[1] - a2).abs() <= P * 2.0 ** -23 * a2).all()
    ms = to_cpu_nchw(mid1).double()
    got_ms = K.colsum(msum, f64=False).double().cpu()
    assert ((got_ms - ms.sum((0, 2, 3))).abs() <= P * 2.0 ** -23 * ms.abs().sum((0, 2, 3))).all()
    # 5. the same bits again
    y2, mid2, stat2, msum2 = run()
    assert torch.equal(y2, y) and torch.equal(stat2, stat) and torch.equal(msum2, msum)
    if want_mid:
        assert torch.equal(mid2, mid)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("line", LINES)
@pytest.mark.parametrize("order", [0, 1], ids=["HW", "WH"])
def test_pair_equals_two_launches_and_the_oracle(order, line, variant, dtype):
    for d in DILS:
        _case(order, line, d, dtype, VARIANTS[variant], seed=3 + d)


def _budget_line(dtype):
    """The first line length the host query refuses."""
    K = L._K()
    line = 1
    while K.conv_line_pair_ok(dtype, C, line, 1):
        line += 1
    return line


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_host_query_refuses_lines_beyond_the_lds_budget(dtype):
    K = L._K()
    line = _budget_line(dtype)
    esz = 2 if dtype == torch.bfloat16 else 4
    fixed = 4 * 3 * C * 4 + 2 * C * (3 * C * esz + (32 if esz == 2 else 16))
    assert line == (64 * 1024 - fixed) // (C * esz + 16) + 1  # 437 / 137
    assert K.conv_line_pair_ok(dtype, C, line - 1, 16) and not K.conv_line_pair_ok(dtype, C, line, 16)
    assert not K.conv_line_pair_ok(dtype, 32, 8, 1) and not K.conv_line_pair_ok(dtype, C, 8, 0)
    x = torch.zeros((1, 2, line, C), dtype=dtype, device=DEV)
    w = torch.zeros((C, 3 * C), dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError):
        K.conv_line_pair(x, w, None, w, None, 0, 1)
    K.conv_line_pair(x, w, None, w, None, 1, 1)  # (its lines, along H, have 2 pixels)


def _modules(d, order, seed):
    torch.manual_seed(seed)
    ch = nn.Conv2d(C, C, (3, 1), padding=(d, 0), dilation=d).to(DEV)
    cw = nn.Conv2d(C, C, (1, 3), padding=(0, d), dilation=d).to(DEV)
    return (ch, cw) if order == 0 else (cw, ch)


def _step(monkeypatch, mode, dtype, order, H, W, d):
    """line_pair_bn forward + backward under SEG_LINE_PAIR=mode -> (y, gradients)."""
    F = L._F()
    monkeypatch.setenv("SEG_LINE_PAIR", mode)
    ca, cb = _modules(d, order, 5)
    x = to_dev_nhwc(quant(rnd((N, C, H, W), 31), dtype), dtype).requires_grad_(True)
    act = F.Act(x, None, True)  # a pending ReLU in the prologue
    y = F.line_pair_bn(act, ca, cb, None).t
    y.backward(to_dev_nhwc(quant(rnd((N, C, H, W), 32), dtype), dtype))
    return y.detach(), [x.grad, ca.weight.grad, cb.weight.grad, ca.bias.grad, cb.bias.grad]


def _first_bias_bound(dtype, order, H, W, d):
    """Two sums of the same stored d mid in two fixed orders differ by at most twice the bound of
    one such sum: 2 * P * 2^-23 * sum |d mid| per channel."""
    K, F = L._K(), L._F()
    _, cb = _modules(d, order, 5)
    dy = to_dev_nhwc(quant(rnd((N, C, H, W), 32), dtype), dtype)
    tb = F.pack_conv_weight_dgrad(cb.weight.detach(), C, dtype)
    dmid, _ = K.conv_line_bias(dy, tb, None, W_ if order == 0 else H_, d)
    return 2 * N * H * W * 2.0 ** -23 * dmid.double().abs().sum((0, 1, 2))


def _same_step(g0, g1, bound):
    for i in (0, 1, 2, 4):  # dx, both weight gradients, the second bias gradient: the same bits
        assert torch.equal(g0[i], g1[i]), i
    assert ((g0[3].double() - g1[3].double()).abs() <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("order", [0, 1], ids=["HW", "WH"])
def test_line_pair_bn_routes_by_the_switch_and_keeps_the_bits(order, dtype, monkeypatch):
    """SEG_LINE_PAIR=1 against =0 on 2 x 9 x 11, dilation 2, forward and backward (whose data
    gradient is the pair kernel with the axes swapped): y, dx and both weight gradients are the
    same bits; the first bias gradient is summed in another fixed order (per line, not per 128
    pixels)."""
    F = L._F()
    H, W, d = 9, 11, 2
    y0, g0 = _step(monkeypatch, "0", dtype, order, H, W, d)
    assert not F.line_pair_routed(dtype, C, W, d)
    y1, g1 = _step(monkeypatch, "1", dtype, order, H, W, d)
    assert F.line_pair_routed(dtype, C, W, d) and F.line_pair_routed(dtype, C, H, d)
    assert torch.equal(y0, y1)
    _same_step(g0, g1, _first_bias_bound(dtype, order, H, W, d))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_line_pair_bn_falls_back_beyond_the_budget(dtype, monkeypatch):
    """Lines (along W) one pixel beyond the budget: under SEG_LINE_PAIR=1 the forward pass is the
    two launches (the backward pair runs along H, 3 pixels, and is routed)."""
    F = L._F()
    line = _budget_line(dtype)
    y0, g0 = _step(monkeypatch, "0", dtype, 0, 3, line, 1)
    y1, g1 = _step(monkeypatch, "1", dtype, 0, 3, line, 1)
    assert not F.line_pair_routed(dtype, C, line, 1) and F.line_pair_routed(dtype, C, 3, 1)
    assert torch.equal(y0, y1)
    _same_step(g0, g1, _first_bias_bound(dtype, 0, 3, line, 1))


def test_default_routing_is_the_measured_classes_and_keeps_the_bits(monkeypatch):
    """SEG_LINE_PAIR unset: only bf16, order (H, W), no `mid` to keep (no backward pass follows)
    on 256-pixel lines or at dilation 16 — profiles/edanet.md.  An evaluation-mode pair on such
    lines then takes the kernel and gives the two-launch bits."""
    F = L._F()
    monkeypatch.delenv("SEG_LINE_PAIR", raising=False)
    bf, f32 = torch.bfloat16, torch.float32
    assert F.line_pair_routed(bf, C, 256, 1, 0, False) and F.line_pair_routed(bf, C, 128, 16, 0, False)
    assert not F.line_pair_routed(bf, C, 128, 2, 0, False)
    assert not F.line_pair_routed(bf, C, 256, 1, 0, True)
    assert not F.line_pair_routed(bf, C, 256, 1, 1, False)
    assert not F.line_pair_routed(f32, C, 128, 16, 0, False)
    assert not F.line_pair_routed(bf, C, 437, 16, 0, False)  # beyond the budget
    ca, cb = _modules(1, 0, 5)
    x = to_dev_nhwc(quant(rnd((1, C, 3, 256), 31), bf), bf)
    with torch.no_grad():
        y = F.line_pair_bn(F.Act(x, None, True), ca, cb, None).t
        monkeypatch.setenv("SEG_LINE_PAIR", "0")
        y0 = F.line_pair_bn(F.Act(x, None, True), ca, cb, None).t
    assert torch.equal(y, y0)
