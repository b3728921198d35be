"""The EfficientNet kernels (csrc/efficientnet.hip) against float64: dle_dwconv2d_act_fwd, dle_se_gate_act, dle_silu_avgpool_fwd.
GPU only.

Reference: torch float64 on the CPU, written with shifted slices of a zero-padded copy (tests/_effnet_ref.py: no conv2d, nothing of
this library).  T_r x T_q output pixels and C_chunk channels per workgroup are read from include/dle_mi355x.h; the shapes sit on
both sides of each.

Exact cases (in_act = out_act = 0): inputs and weights k / 4 with |k| <= 4 (tests/_exact_grid.py), scale in +-{0.5, 1, 2}, shift a
multiple of 1/16.  A 25-term sum of such products is exact in fp32 in any order (check_exact on the terms of the output with the
largest sum of magnitudes; that sum is asserted below 2^20 for every output), v = scale * acc + shift is a multiple of 1/32 below 64
and exact too, so y is the float64 value rounded once and pool (sums of at most T_r T_q multiples of 1/32 below 64) is exact: bit
for bit, in bf16 and fp16, with and without pool, and y identical with and without pool.

Random cases: the same shapes, all four (in_act, out_act), under the DERIVED per-element bar of tests/_effnet_ref.py (its self-test:
tests/test_efficientnet_host.py).  The largest use of the bar and the share of near-tie inputs are printed; the share must stay
below 1 % (a margin of 8 u on either side of a boundary against a spacing of 2^-10 .. 2^-11 (fp16) or 2^-7 .. 2^-8 (bf16) of the
value: about 2^-10 and 2^-13 of well-scaled inputs; values that underflow towards the subnormals add to it).  Measured with the
float64 reference alone, before the assertions were written: at most 0.13 % (bf16) and 0.06 % (fp16) over the depthwise cases,
0.30 % and 0.08 % over the pooling cases, 260 and 56 of the 65,280 / 63,488 finite inputs of the sweep.
"""
import functools

import pytest
import torch

from deeplearningexamples_amd import functional as F
from tests import _effnet_ref as R
from tests._exact_grid import Out, assert_same, bits, check_exact, gen, grid, ulp16

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
DEV = "cuda"
TR, TQ, CCH = R.tile_constants()
U = R.U


def _cases():
    c = []
    for k in (3, 5):
        for s in (1, 2):
            c.append(("one_pixel_k%d_s%d" % (k, s), 2, 8, k, s, 1, 1))
    c += [("smaller_than_kernel_2x2", 2, 144, 5, 2, 2, 2), ("smaller_than_kernel_3x2", 2, 144, 5, 2, 3, 2)]
    c += [("odd_even_s2_%dx%d" % hw, 2, 96, 3, 2) + hw for hw in ((9, 9), (10, 10), (9, 10))]
    c.append(("k5_s2_odd", 2, 24, 5, 2, 7, 5))
    c += [("row_tile_edges_h%d" % h, 2, 8, 3, 1, h, 5) for h in (TR - 1, TR, TR + 1, 2 * TR + 1)]
    c += [("col_tile_edges_w%d" % w, 2, 8, 3, 1, 5, w) for w in (TQ - 1, TQ, TQ + 1, 2 * TQ + 1)]
    c += [("chunk_edges_c%d" % ch, 2, ch, 5, 1, 6, 6) for ch in (CCH - 8, CCH, CCH + 8)]
    c.append(("widest", 1, 2688, 3, 1, 4, 4))
    c.append(("b0_last", 2, 1152, 5, 1, 7, 7))
    c.append(("many_workgroups", 3, 32, 3, 2, 67, 67))
    # with T_r x T_q x C_chunk tiles the case above is 45 workgroups; this one is 4 x 9 x 5 x 2 = 360, more than the 256 CUs
    c.append(("more_workgroups_than_cus", 4, 128, 3, 1, 72, 80))
    return c


CASES = {c[0]: c[1:] for c in _cases()}
NAMES = list(CASES)
DT = pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])


def _run(x, w, scale, shift, stride, in_act, out_act, pool):
    """Outputs in over-long NaN buffers: -> (y, pool or None), on the CPU."""
    n, h, wd, c = x.shape
    k = w.shape[0]
    p, q = R.out_hw(h, wd, k, stride)
    yo = Out((n, p, q, c), x.dtype, DEV)
    args = (x.to(DEV), w.to(DEV), scale.to(DEV), shift.to(DEV), stride)
    if not pool:
        y = F.dwconv2d_act_fwd(*args, in_act=in_act, out_act=out_act, out=yo.t)
        assert y is yo.t
        return yo.check("dwconv2d_act_fwd").cpu(), None
    g = F.dwconv2d_pool_bands(h, wd, c, k, stride)
    po = Out((n, g, c), torch.float32, DEV)
    y, pl = F.dwconv2d_act_fwd(*args, in_act=in_act, out_act=out_act, pool=po.t, out=yo.t)
    assert y is yo.t and pl is po.t
    return yo.check("dwconv2d_act_fwd").cpu(), po.check("dwconv2d_act_fwd (pool)").cpu()


@functools.lru_cache(maxsize=None)
def exact_case(name, dtype):
    n, c, k, s, h, w = CASES[name]
    x = grid((n, h, w, c), 11, dtype, "cpu")
    wt = grid((k, k, c), 12, dtype, "cpu")
    g = gen("cpu", 13)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g)] * (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float()
    shift = torch.randint(-32, 33, (c,), generator=g).float() / 16
    ref = R.dwconv_ref(x, wt, scale, shift, s, 0, 0)
    assert float(ref["absacc"].max()) < 2.0 ** 20
    idx = torch.nonzero(ref["absacc"].sum(3) == ref["absacc"].sum(3).max())[0].tolist()
    check_exact(R.window_terms(ref["a"], wt.double(), k, s, *idx))
    v = ref["v64"]
    assert torch.equal(v * 32, torch.round(v * 32)) and float(v.abs().max()) < 64
    want = v.float().to(dtype)                                       # (v is exact in fp32: one rounding)
    pool, _, _ = R.pool_ref(want, TR, TQ)
    return x, wt, scale, shift, s, want, pool.float()


@DT
@pytest.mark.parametrize("name", NAMES)
def test_dwconv_exact_grid_bits(name, dtype):
    x, w, scale, shift, s, want, want_pool = exact_case(name, dtype)
    y0, _ = _run(x, w, scale, shift, s, 0, 0, pool=False)
    y1, pool = _run(x, w, scale, shift, s, 0, 0, pool=True)
    assert_same(bits(y0), bits(want), "%s: y" % name)
    assert_same(bits(y1), bits(y0), "%s: y with pool against y without" % name)
    assert tuple(pool.shape) == tuple(want_pool.shape)
    assert_same(bits(pool), bits(want_pool), "%s: pool" % name)


@functools.lru_cache(maxsize=None)
def random_case(name, dtype, in_act, out_act):
    n, c, k, s, h, w = CASES[name]
    g = gen("cpu", 21)
    x = (torch.randn((n, h, w, c), generator=g) * 2).to(dtype)
    wt = (torch.randn((k, k, c), generator=g) * 0.5).to(dtype)
    scale = (torch.rand(c, generator=g) + 0.5) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float()
    shift = torch.randn(c, generator=g)
    return x, wt, scale, shift, s, R.dwconv_ref(x, wt, scale, shift, s, in_act, out_act)


@DT
@pytest.mark.parametrize("in_act,out_act", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("name", NAMES)
def test_dwconv_random_inputs_derived_bar(name, dtype, in_act, out_act):
    x, w, scale, shift, s, ref = random_case(name, dtype, in_act, out_act)
    y, pool = _run(x, w, scale, shift, s, in_act, out_act, pool=True)
    assert bool(torch.isfinite(y).all())
    err = (y.double() - ref["y64"]).abs()
    use = float((err / ref["bar"]).max())
    print("%s %s in_act %d out_act %d: largest use of the bar %.3f, near-tie inputs %.4f %%" % (name, dtype, in_act, out_act, use,
                                                                                               100 * ref["ties"]))
    assert ref["ties"] < 0.01
    assert bool((err <= ref["bar"]).all()), "largest use of the bar %.3f" % use
    # pool: the fp32 sum of the RETURNED y per tile, any fixed order
    want, mag, pixels = R.pool_ref(y, TR, TQ)
    assert tuple(pool.shape) == tuple(want.shape)
    perr = (pool.double() - want).abs()
    pbar = pixels * U * mag
    print("    pool: largest use of the bar %.3f" % float((perr / pbar.clamp_min(1e-300)).max()))
    assert bool((perr <= pbar).all())


@DT
def test_input_silu_over_every_finite_value(dtype):
    """in_act alone: centre-tap weight 1, scale 1, shift 0, so y = round16(silu(x)) element for element, swept over all finite
    16-bit values at C = 8.  Equal to the float64 SiLU rounded once wherever that is not a near-tie, within one spacing otherwise;
    no NaN for large |x| and silu(large negative) = -0 or 0."""
    pat = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    x = pat.view(dtype)
    x = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).view(1, 64, 128, 8)
    w = torch.zeros((3, 3, 8), dtype=dtype)
    w[1, 1] = 1
    y, _ = _run(x, w, torch.ones(8), torch.zeros(8), 1, 1, 0, pool=False)
    assert bool(torch.isfinite(y).all())
    s64 = R.silu64(x.double())
    want, near = R.r16(s64, dtype), R.near_tie(s64, dtype)
    print("%s: %d finite inputs, %d near-ties" % (dtype, x.numel(), int(near.sum())))
    assert float(near.double().mean()) < 0.01
    assert_same(torch.where(near, want, y.double()), want, "silu of the inputs that are not near-ties")
    assert bool(((y.double() - want).abs() <= ulp16(want, dtype))[near].all())
    big = x.double() < -200
    assert int(big.sum()) > 0 and bool((y.double()[big] == 0).all())


def test_an_inf_pixel_stays_inside_its_windows():
    n, c, k, s, h, w = 2, 16, 5, 2, 11, 19
    x = grid((n, h, w, c), 31, BF, "cpu")
    wt = grid((k, k, c), 32, BF, "cpu")
    wt = torch.where(wt == 0, torch.ones_like(wt), wt)               # (0 x inf would be NaN in every window, which is "reached" too)
    scale, shift = torch.ones(c), torch.zeros(c)
    base, _ = _run(x, wt, scale, shift, s, 0, 0, pool=False)
    x2 = x.clone()
    x2[1, 6, 9, 5] = float("inf")
    y, _ = _run(x2, wt, scale, shift, s, 0, 0, pool=False)
    p, q = R.out_hw(h, w, k, s)
    hit = torch.zeros((n, p, q, c), dtype=torch.bool)
    for pp in range(p):
        for qq in range(q):
            if abs(pp * s - 6) <= k // 2 and abs(qq * s - 9) <= k // 2:
                hit[1, pp, qq, 5] = True
    assert int(hit.sum()) == 3 * 2                                   # rows 2..4 (|2 p - 6| <= 2), columns 4..5 (|2 q - 9| <= 2)
    assert bool((~torch.isfinite(y))[hit].all()) and bool(torch.isfinite(y)[~hit].all())
    assert_same(bits(torch.where(hit, base, y)), bits(base), "outputs outside the inf's windows")


def test_dwconv_argument_checks_raise_without_a_launch(monkeypatch):
    from deeplearningexamples_amd import _cabi as C
    launched = []
    real = C.call
    monkeypatch.setattr(C, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    z = lambda *shape, dtype=BF: torch.zeros(shape, dtype=dtype, device=DEV)
    x, w, sc, sh = z(1, 4, 4, 16), z(3, 3, 16), z(16, dtype=torch.float32), z(16, dtype=torch.float32)
    g = F.dwconv2d_pool_bands(4, 4, 16, 3, 1)
    for args, kw, msg in (((z(1, 4, 4, 12), z(3, 3, 12), sc[:12], sh[:12]), {}, "C must be a multiple of 8"),
                          ((x, z(7, 7, 16), sc, sh), {}, "k 3 or 5"),
                          ((x, w, sc, sh), {"stride": 3}, "stride 1 or 2"),
                          ((z(16 * 16 + 4)[4:].view(1, 4, 4, 16), w, sc, sh), {}, "x must be 16-byte aligned"),
                          ((x, w, sc, sh), {"pool": z(1, g + 1, 16, dtype=torch.float32)}, r"pool must be a contiguous, 16-byte aligned fp32 \[N,G,C\]")):
        with pytest.raises(ValueError, match=msg):
            F.dwconv2d_act_fwd(*args, **kw)
    assert launched == []
    # the C entry point checks on its own: a short pool buffer and a bad kernel size are argument errors, nothing is launched
    lib = C.lib()
    y, pool = torch.empty_like(x), z(1, g, 16, dtype=torch.float32)
    a = (C.ptr(x), C.ptr(w), C.ptr(y), C.ptr(sc), C.ptr(sh), C.ptr(pool))
    assert lib.dle_dwconv2d_act_fwd(*a, pool.numel() * 4 - 4, 1, 4, 4, 16, 3, 1, 0, 0, C.BF16, C.stream()) == -1
    assert b"N * G * C" in lib.dle_last_error()
    assert lib.dle_dwconv2d_act_fwd(*a, pool.numel() * 4, 1, 4, 4, 16, 7, 1, 0, 0, C.BF16, C.stream()) == -1
    assert lib.dle_dwconv2d_act_fwd(*a, pool.numel() * 4, 1, 4, 4, 16, 3, 1, 0, 0, C.F32, C.stream()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the gate
@pytest.mark.parametrize("act", ["silu", "relu"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c,s,g", [(8, 1, 1), (96, 4, 3), (1152, 48, 2), (1152, 288, 1), (2688, 672, 4)])
def test_se_gate_act_against_float64(c, s, g, n, act):
    gn = gen("cpu", 41)
    hw = 49
    pool = torch.randn((n, g, c), generator=gn) * hw / g
    w1, b1 = torch.randn((s, c), generator=gn) * c ** -0.5, torch.randn(s, generator=gn) * 0.3
    w2, b2 = torch.randn((c, s), generator=gn) * s ** -0.5, torch.randn(c, generator=gn) * 0.3
    want, bar = R.gate_ref(pool, 1.0 / hw, w1, b1, w2, b2, act)
    o = Out((n, c), torch.float32, DEV)
    got = F.se_gate_act(pool.to(DEV), 1.0 / hw, w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), act=act, out=o.t)
    assert got is o.t
    err = (o.check("se_gate_act").cpu().double() - want).abs()
    print("C %d S %d G %d N %d %s: largest use of the bar %.3f (bar up to %.2e)" % (c, s, g, n, act, float((err / bar).max()), float(bar.max())))
    assert bool((err <= bar).all())


@pytest.mark.parametrize("c,s", [(8, 1), (96, 4), (1152, 48)])
def test_se_gate_act_agrees_with_se_gate(c, s):
    """act = ReLU, G = 1, S <= 64: the same gate as dle_se_gate on a tensor whose per-channel sums are exact (a grid of k / 4), within
    the two kernels' derived bars (their sums run in different orders: bit equality is not promised)."""
    n, hw = 3, 49
    t = grid((n, hw, c), 51, BF, DEV)
    pool = t.float().sum(1, keepdim=True)                             # exact: at most 49 multiples of 1/4 below 1
    assert torch.equal(pool.cpu().double(), t.cpu().double().sum(1, keepdim=True))
    gn = gen("cpu", 52)
    w1, b1 = torch.randn((s, c), generator=gn) * c ** -0.5, torch.randn(s, generator=gn) * 0.3
    w2, b2 = torch.randn((c, s), generator=gn) * s ** -0.5, torch.randn(c, generator=gn) * 0.3
    dw = [v.to(DEV) for v in (w1, b1, w2, b2)]
    a = F.se_gate_act(pool, 1.0 / hw, *dw, act="relu").cpu().double()
    b = F.se_gate(t, *dw).cpu().double()
    want, bar = R.gate_ref(pool.cpu(), 1.0 / hw, w1, b1, w2, b2, "relu")
    assert bool(((a - want).abs() <= bar).all()) and bool(((b - want).abs() <= bar).all())
    assert bool(((a - b).abs() <= 2 * bar).all())


# ------------------------------------------------------------------------------------------------------- SiLU + average pooling
@DT
@pytest.mark.parametrize("c", [8, 1280, 1792])
@pytest.mark.parametrize("hw", [1, 49, 144])
def test_silu_avgpool_exact_and_derived_bar(hw, c, dtype):
    n = 2
    g = gen("cpu", 61)
    # exact: per (image, channel) one value v in {0, 32, 48, 64, 96} at every pixel: silu(v) == v in 16 bits (v e^-v < 1e-12), the
    # sum hw v is exact and (1 / hw) * (hw v) is v to 2^-23, far inside v's rounding interval
    v = torch.tensor([0.0, 32.0, 48.0, 64.0, 96.0])[torch.randint(0, 5, (n, 1, c), generator=g)]
    x = v.expand(n, hw, c).contiguous().to(dtype)
    o = Out((n, c), dtype, DEV)
    assert F.silu_avgpool_fwd(x.to(DEV), out=o.t) is o.t
    assert_same(bits(o.check("silu_avgpool_fwd").cpu()), bits(v[:, 0].to(dtype)), "constant planes")
    # random
    x = (torch.randn((n, hw, c), generator=g) * 3).to(dtype)
    want, bar, ties = R.silu_avgpool_ref(x)
    got = F.silu_avgpool_fwd(x.view(n, 1, hw, c).to(DEV)).cpu().double()
    err = (got - want).abs()
    print("HW %d C %d %s: largest use of the bar %.3f, near-tie inputs %.4f %%" % (hw, c, dtype, float((err / bar).max()), 100 * ties))
    assert ties < 0.01
    assert bool((err <= bar).all())
